"""The flat-parameter optimiser path on the host, no GPU needed: the return codes of sahs_adam_step for every rejected argument (before any
GPU call), models.flatten_parameters_() on CPU tensors for the three architectures (state_dict untouched, every parameter and gradient a
view at its canonical byte offset, the autograd link of the flat buffer), and training.FlatAdam speaking torch.optim.Adam's state format."""
import copy

import numpy as np
import pytest
import torch

from conftest import pkg

A = 1 << 20          # fabricated device addresses, never dereferenced: every case below returns before a launch
B, C, D = A + (1 << 16), A + (2 << 16), A + (3 << 16)
GOOD = dict(params=A, grad=B, exp_avg=C, exp_avg_sq=D, n=1024, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0, stream=None)
ORDER = "params grad exp_avg exp_avg_sq n lr beta1 beta2 eps step grad_scale stream".split()
INF, NAN = float("inf"), float("nan")

REJECTED = [dict(params=None), dict(grad=None), dict(exp_avg=None), dict(exp_avg_sq=None),
            dict(n=-1), dict(step=0), dict(step=-3),
            dict(lr=0.0), dict(lr=-1e-3), dict(lr=INF), dict(lr=NAN),
            dict(eps=0.0), dict(eps=-1e-8), dict(eps=INF), dict(eps=NAN),
            dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=NAN), dict(beta2=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=NAN),
            dict(exp_avg=A), dict(exp_avg_sq=A), dict(exp_avg_sq=C),              # the same buffer twice
            dict(exp_avg=A + 4 * 1023), dict(params=D + 4 * 1023),                # overlapping by one element
            dict(params=A + 2)]                                                   # not a float address


def _adam(L, **kw):
    v = dict(GOOD, **kw)
    return L.sahs_adam_step(*[v[k] for k in ORDER])


@pytest.mark.parametrize("case", REJECTED, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_adam_step_rejects(case):
    L = pkg("_lib").lib()
    assert _adam(L, **case) == 1
    assert b"sahs_adam_step" in L.sahs_last_error()


def test_adam_step_of_nothing_succeeds():
    L = pkg("_lib").lib()
    assert _adam(L, n=0) == 0
    assert _adam(L, n=0, params=None, grad=None, exp_avg=None, exp_avg_sq=None) == 0      # (the ABI's convention for an empty call)


# ---- flatten_parameters_ ----
ARCHS = ("audio", "nerface", "nerface_static")


def _model(arch):
    sahs = pkg()
    if arch == "audio":
        return sahs.AudioFaceModel(sahs.default_config())
    return sahs.NeRFaceModel(sahs.default_config("expression" if arch == "nerface" else "expression_static"))


def _assert_views(model):
    W = pkg("weights")
    flat, grad = model.flat_params(), model._flat_grad
    assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == sum(int(np.prod(s)) for _, s in W.canonical_spec(model.arch))
    named = dict(model.named_parameters())
    off = 0
    for k, shape in W.canonical_spec(model.arch):
        p = named[k]
        assert tuple(p.shape) == tuple(shape) and p.is_contiguous(), k
        assert p.data_ptr() == flat.data_ptr() + 4 * off, k
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.data_ptr() == grad.data_ptr() + 4 * off, k
        off += p.numel()
    assert off == flat.numel() == grad.numel()


@pytest.mark.parametrize("arch", ARCHS)
def test_flatten_parameters(arch):
    torch.manual_seed(1)
    model = _model(arch)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.flatten_parameters_() is model
    after = model.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert after[k].shape == before[k].shape and after[k].dtype == before[k].dtype
        assert np.array_equal(after[k].numpy().view(np.uint32), before[k].numpy().view(np.uint32)), k
    _assert_views(model)
    assert model.flat_params() is model.flat_params()                              # the buffer itself: nothing is concatenated
    assert torch.equal(model.flat_params(), torch.cat([v.reshape(-1) for v in before.values()]))
    # the autograd link: a gradient w.r.t. the flat buffer lands in the flat gradient buffer, hence in every .grad view
    r = torch.randn(model.flat_params().numel())
    (model.flat_params(differentiable=True) * r).sum().backward()
    assert torch.equal(model._flat_grad, r)
    off = 0
    for p in model.parameters():
        assert torch.equal(p.grad.reshape(-1), r[off:off + p.numel()])
        off += p.numel()
    (model.flat_params(differentiable=True) * r).sum().backward()                  # ... and accumulates
    assert torch.equal(model._flat_grad, r + r)
    # a parameter used directly (train_step's spatial-embedding regulariser) accumulates into its view
    model.spatial_embeddings.sum().backward()
    n0 = model.spatial_embeddings.numel()
    assert torch.equal(model._flat_grad[:n0], r[:n0] + r[:n0] + 1.0) and torch.equal(model._flat_grad[n0:], (r + r)[n0:])
    Tr = pkg("training")
    for zero in (lambda: model.zero_grad(set_to_none=True), lambda: Tr.FlatAdam(model, lr=1e-3).zero_grad(set_to_none=True),
                 lambda: Tr.FlatAdam(model, lr=1e-3).zero_grad(set_to_none=False)):
        model._flat_grad.fill_(3.0)
        zero()
        assert not bool(model._flat_grad.any())
        _assert_views(model)
    # gradients asked for per parameter are not silently missing
    with pytest.raises(RuntimeError):
        torch.autograd.grad((model.flat_params(differentiable=True) * r).sum(), list(model.parameters()))


@pytest.mark.parametrize("arch", ARCHS)
def test_flattened_model_writes_through(arch):
    W = pkg("weights")
    model = _model(arch).flatten_parameters_()
    fw = W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)
    assert model.load_flat(fw) is model
    _assert_views(model)
    assert np.array_equal(model.flat_params().numpy(), fw)
    sd = {k: torch.from_numpy(v) for k, v in W.hash_state_dict(1, 2.0, 30.0, model=arch).items()}
    model.load_state_dict(sd)
    _assert_views(model)
    assert np.array_equal(model.flat_params().numpy(), W.flatten_state_dict(W.hash_state_dict(1, 2.0, 30.0, model=arch), model=arch))
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    with torch.no_grad():
        list(model.parameters())[-1].add_(1.0)
    assert float(model.flat_params()[-1]) == float(sd[list(sd)[-1]].reshape(-1)[-1] + 1.0)
    with pytest.raises(RuntimeError):
        model.load_state_dict(sd, assign=True)          # rebinding the parameters is reported, not trained on


def test_flatten_requires_trainable_parameters_and_keeps_its_layout():
    model = _model("nerface_static")
    model.nerf_mlps["fine"].fc_rgb.bias.requires_grad_(False)
    with pytest.raises(RuntimeError):
        model.flatten_parameters_()
    model.nerf_mlps["fine"].fc_rgb.bias.requires_grad_(True)
    model.flatten_parameters_()
    with pytest.raises(RuntimeError):
        model.double()                                 # leaves nothing half-converted
    _assert_views(model)
    with pytest.raises(RuntimeError):
        model.to(torch.bfloat16)
    _assert_views(model)
    want = model.flat_params().clone()
    model.to("cpu").float()                            # conversions that keep fp32 keep the flat layout
    _assert_views(model)
    assert torch.equal(model.flat_params(), want)
    twin = copy.deepcopy(model)
    _assert_views(twin)
    assert torch.equal(twin.flat_params(), want) and twin.flat_params().data_ptr() != model.flat_params().data_ptr()
    sd = model.state_dict()
    model.unflatten_parameters_()
    assert model._flat is None and all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    ptrs = sorted(p.data_ptr() for p in model.parameters())
    assert len(set(ptrs)) == len(ptrs)
    with pytest.raises(ValueError):
        pkg("training").FlatAdam(model, lr=1e-3)       # needs a flattened model


# ---- FlatAdam's state ----
@pytest.mark.parametrize("arch", ARCHS)
def test_flat_adam_state_dict_is_torch_adams(arch):
    Tr = pkg("training")
    model = _model(arch).flatten_parameters_()
    opt = Tr.FlatAdam(model, lr=5e-4)
    ref = torch.optim.Adam([torch.zeros(3, requires_grad=True)], lr=5e-4).state_dict()
    sd = opt.state_dict()
    assert set(sd) == set(ref) == {"state", "param_groups"}
    assert len(sd["param_groups"]) == 1 and set(sd["param_groups"][0]) == set(ref["param_groups"][0])
    assert sd["param_groups"][0]["params"] == list(range(len(list(model.parameters()))))
    assert {k: v for k, v in sd["param_groups"][0].items() if k != "params"} == {k: v for k, v in ref["param_groups"][0].items() if k != "params"}
    assert sd["state"] == {}                                                        # empty before the first step, as torch's
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 5e-4
    # the state of a stepped torch.optim.Adam loads and reads back equal
    other = _model(arch)
    adam = torch.optim.Adam(other.parameters(), lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        for p in other.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        adam.step()
    want = adam.state_dict()
    opt.load_state_dict(copy.deepcopy(want))
    got = opt.state_dict()
    assert got["param_groups"] == want["param_groups"]
    assert list(got["state"]) == list(want["state"])
    for i, st in want["state"].items():
        assert set(got["state"][i]) == set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(got["state"][i]["step"]) == float(st["step"]) == 3.0 and got["state"][i]["step"].dtype == st["step"].dtype
        assert torch.equal(got["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(got["state"][i]["exp_avg_sq"], st["exp_avg_sq"])
    assert opt.param_groups[0]["lr"] == 3e-4 and tuple(opt.param_groups[0]["betas"]) == (0.8, 0.99) and opt.param_groups[0]["eps"] == 1e-7
    # ... and goes back into torch's class
    back = torch.optim.Adam(_model(arch).parameters(), lr=1.0)
    back.load_state_dict(got)
    assert torch.equal(back.state_dict()["state"][5]["exp_avg_sq"], want["state"][5]["exp_avg_sq"])
    # an empty state resets
    opt.load_state_dict(torch.optim.Adam(_model(arch).parameters(), lr=1e-3).state_dict())
    assert opt.state_dict()["state"] == {} and not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())
    # what the kernel does not do is refused
    for bad in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(NotImplementedError):
            opt.load_state_dict(torch.optim.Adam(_model(arch).parameters(), lr=1e-3, **bad).state_dict())
    two = torch.optim.Adam([dict(params=[torch.zeros(1, requires_grad=True)]), dict(params=[torch.zeros(1, requires_grad=True)])], lr=1e-3)
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(two.state_dict())
    opt.param_groups.append(dict(opt.param_groups[0]))
    with pytest.raises(NotImplementedError):
        opt.step()


def test_ops_adam_step_needs_gpu_tensors():
    ops, E = pkg("ops"), pkg("_lib").SahsError
    t = [torch.zeros(8) for _ in range(4)]
    with pytest.raises(E):
        ops.adam_step(*t, lr=1e-3)
