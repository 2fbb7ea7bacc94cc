"""The fused spectral norm on the GPU (csrc/spectral_norm.hip behind ``ops.spectral_normalize`` and ``spade.fuse_spectral_norm_``).

Op level, on the cases of tests/spectral_norm_reference.py, training on and off, fp32 and bf16 output.  The yardstick is float64 of the same
formula on the same fp32 inputs (CPU); E = max error over the largest reference magnitude.
  fp32 output, u, v, sigma, dW:  E_fused <= max(4 E_torch32, 2^-21), E_torch32 from torch's own SpectralNorm.compute_weight and its
    autograd in fp32 on the same GPU; 1 x 1, where dW is analytically 0: |dW| <= 2^-21 |G / sigma|.
  bf16 output (under autocast): every element within one bf16 ulp of bfloat16(ref64), at most max(1, 0.1 %) of a case's elements
    different from it at all; dW from a bf16 grad_out: the fp32 rule, the reference fed the bf16 values.
Generators, on the fixture of tests/golden/spade_train.npz: the bounds are stated at each test.
Every test prints its figures before it asserts.

Measured on an MI355X: fp32 out / sigma / dW at 256 x 2304, training: E_fused 4.8e-8 / 9.3e-9 / 8.0e-8, E_torch32 1.2e-7 / 8.5e-8 / 1.2e-7;
1 x 1: dW exactly 0; bf16 output: 0 .. 6 of up to 589,824 elements differ from bfloat16(ref64), none by more than one ulp; fused generators,
fp32: loss within 0 and 1.2e-7 of the fixture's, G_fused 4.5e-6 / 4.1e-6 (G_unfused 4.6e-6 / 4.4e-6); under autocast: |loss - loss_c|
4.2e-5 / 3.1e-5 against |loss_c - fixture| 1.3e-4 / 5.0e-4, G_fused 0.242 / 0.258, G_c 0.262 / 0.257; ten steps: worst weight_u E_fused
1.09e-2 where E_unfused is 1.23e-2; eval: E_fused 1.5e-6 / 3.1e-6, E_unfused 1.7e-6 / 2.2e-6.
"""
import contextlib
import copy

import pytest
import torch
from torch.nn.utils.spectral_norm import SpectralNorm

import spade_reference as R
import spectral_norm_reference as N
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
AUTOCAST = lambda: torch.autocast("cuda", dtype=BF16)
ALL = sorted(N.CASES)


def _place(t, off=0):
    """t on the GPU, contiguous, starting ``off`` elements past a 16-byte boundary."""
    if not off:
        return t.to(DEV)
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off * t.element_size()
    return v


def _jobs(names):
    return [N.case(n) + (N.CASES[n][2],) for n in names]


def _fused(jobs, training, bf16, needs=None, backward=True):
    """jobs: [(W, u, v, G, offset)] on the CPU -> per job dict(out, u, v, sigma, dW): the op's results for fresh copies of the inputs;
    u, v the buffers after the call; sigma from the saved area, whose u and v must be the ones the call left or read."""
    ops = pkg("ops")
    needs = needs or [True] * len(jobs)
    Ws = [_place(W, off).requires_grad_(need) for (W, _, _, _, off), need in zip(jobs, needs)]
    us, vs = [j[1].to(DEV) for j in jobs], [j[2].to(DEV) for j in jobs]
    keep = [(u.data_ptr(), v.data_ptr(), u.clone(), v.clone()) for u, v in zip(us, vs)]
    with AUTOCAST() if bf16 else contextlib.nullcontext():
        outs = ops.spectral_normalize(Ws, us, vs, training)
    fn = outs[0].grad_fn
    assert len(outs) == len(jobs) and len({o.grad_fn for o in outs}) == 1
    assert all(o.dtype == (BF16 if bf16 else torch.float32) and o.shape == W.shape and o.is_contiguous() for o, W in zip(outs, Ws))
    saved = dict(zip(fn.saved_names, fn.saved_tensors))
    if backward:
        torch.autograd.backward(outs, [_place(j[3].to(o.dtype), j[4]) for j, o in zip(jobs, outs)])
    res = []
    for k, (W, u, v, (pu, pv, u0, v0)) in enumerate(zip(Ws, us, vs, keep)):
        h, area = W.shape[0], saved["saved%d" % k]
        assert (u.data_ptr(), v.data_ptr()) == (pu, pv) and area.numel() == W.numel() // h + h + 1
        assert torch.equal(area[:h], u) and torch.equal(area[h:-1], v)
        if not training:
            assert torch.equal(u, u0) and torch.equal(v, v0)
        res.append(dict(out=outs[k].detach(), u=u, v=v, sigma=area[-1], dW=W.grad))
    return res


def _torch32(job, training, grad_bf16=False):
    W, u, v, G, _ = job
    G = G.bfloat16().float() if grad_bf16 else G
    return dict(zip(("out", "u", "v", "sigma", "dW"), N.torch_spectral_norm(W.to(DEV), u.to(DEV), v.to(DEV), training, G.to(DEV))))


def _ref64(job, training, grad_bf16=False):
    W, u, v, G, _ = job
    out, u1, v1, sigma = N.compute_weight64(W, u, v, training)
    return dict(out=out, u=u1, v=v1, sigma=sigma, dW=N.backward64(W, u1, v1, sigma, G.bfloat16() if grad_bf16 else G))


def _fp32_rule(tag, got, t32, ref, names):
    bad = []
    for what in names:
        if what == "dW" and ref["dW"].numel() == 1:      # analytically 0: an absolute bound on the scale of its two terms
            e, bound = float(got["dW"].abs().max()), N.FLOOR * float((N.case("1x1")[3].double() / ref["sigma"]).abs().max())
            print("%s dW: |dW| %.3e, bound %.3e" % (tag, e, bound))
        else:
            e, e32 = N.rel_max(got[what], ref[what]), N.rel_max(t32[what], ref[what])
            bound = max(4.0 * e32, N.FLOOR)
            print("%s %s: E_fused %.3e, E_torch32 %.3e" % (tag, what, e, e32))
        if not e <= bound:
            bad.append((what, e, bound))
    return bad


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("name", ALL)
def test_op_fp32(name, training):
    (job,) = _jobs([name])
    (got,) = _fused([job], training, False)
    bad = _fp32_rule("%s training %d" % (name, training), got, _torch32(job, training), _ref64(job, training), ("out", "u", "v", "sigma", "dW"))
    assert not bad, bad


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("name", ALL)
def test_op_bf16(name, training):
    (job,) = _jobs([name])
    (got,) = _fused([job], training, True)
    ref = _ref64(job, training, grad_bf16=True)
    ok, text = N.bf16_rule(got["out"], ref["out"])
    print("%s training %d out: %s" % (name, training, text))
    bad = _fp32_rule("%s training %d (bf16 grad_out)" % (name, training), got, _torch32(job, training, grad_bf16=True), ref, ("u", "v", "sigma", "dW"))
    assert ok and not bad, (text, bad)
    assert got["dW"].dtype == torch.float32


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("training", (True, False))
def test_mixed_table_is_the_single_jobs(training, bf16):
    """All cases as ONE call: a job's result does not depend on the table around it -- the same bits as its own call, which
    test_op_fp32 / test_op_bf16 hold to the yardstick."""
    jobs = _jobs(ALL)
    for name, job, got in zip(ALL, jobs, _fused(jobs, training, bf16)):
        (alone,) = _fused([job], training, bf16)
        assert all(torch.equal(got[k], alone[k]) for k in got), name


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("training", (True, False))
def test_33_jobs_take_two_calls(training, bf16):
    jobs = [j + (0,) for j in N.small_cases(33)]
    assert len(jobs) > pkg("ops").SPECTRAL_NORM_MAX_JOBS
    bad = []
    for k, (job, got) in enumerate(zip(jobs, _fused(jobs, training, bf16))):
        ref = _ref64(job, training, grad_bf16=bf16)
        if bf16:
            ok, text = N.bf16_rule(got["out"], ref["out"])
            bad += [] if ok else [(k, text)]
        with contextlib.redirect_stdout(None):
            bad += [(k,) + b for b in _fp32_rule("", got, _torch32(job, training, grad_bf16=bf16), ref, ("u", "v", "sigma", "dW") + (() if bf16 else ("out",)))]
    assert not bad, bad


def test_a_second_forward_does_not_disturb_the_first_backward():
    ops = pkg("ops")
    W0, u0, v0, G, _ = _jobs(["65x577"])[0]
    grads = []
    for again in (False, True, False):
        W, u, v = W0.to(DEV).requires_grad_(True), u0.to(DEV), v0.to(DEV)
        (out,) = ops.spectral_normalize([W], [u], [v], True)
        if again:
            held = u.clone()
            (second,) = ops.spectral_normalize([W], [u], [v], True)
            assert not torch.equal(u, held) and not torch.equal(second, out)      # the buffers moved on
        out.backward(G.to(DEV))
        grads.append((out.detach().clone(), W.grad))
    for out, dW in grads[1:]:      # the intervening forward changes nothing; two identical runs give the same bits
        assert torch.equal(out, grads[0][0]) and torch.equal(dW, grads[0][1])


def test_only_the_weights_that_ask_get_a_gradient():
    names = ["3x5", "64x576", "65x577"]
    full = _fused(_jobs(names), True, False)
    some = _fused(_jobs(names), True, False, needs=[True, False, True])
    assert some[1]["dW"] is None and all(torch.equal(a["out"], b["out"]) for a, b in zip(some, full))
    assert torch.equal(some[0]["dW"], full[0]["dW"]) and torch.equal(some[2]["dW"], full[2]["dW"])


def test_grad_mode_and_dtypes():
    ops, lib = pkg("ops"), pkg("_lib")
    W, u, v, G = (t.to(DEV) for t in N.case("3x5"))
    (tracked,) = ops.spectral_normalize([W.clone().requires_grad_(True)], [u.clone()], [v.clone()], True)
    (plain,) = ops.spectral_normalize([W], [u.clone()], [v.clone()], True)
    with torch.no_grad():
        (held,) = ops.spectral_normalize([W.clone().requires_grad_(True)], [u.clone()], [v.clone()], True)
    assert tracked.grad_fn is not None and plain.grad_fn is None and held.grad_fn is None
    assert torch.equal(tracked.detach(), plain) and torch.equal(held, plain)
    conv = W.reshape(3, 5, 1, 1)      # a weight keeps its own shape
    assert ops.spectral_normalize([conv], [u.clone()], [v.clone()], False)[0].shape == conv.shape
    with AUTOCAST():
        assert ops.spectral_normalize([W], [u.clone()], [v.clone()], False)[0].dtype == BF16
    with torch.autocast("cuda", dtype=torch.float16):
        assert ops.spectral_normalize([W], [u.clone()], [v.clone()], False)[0].dtype == torch.float32
    for bad in (torch.float64, BF16):
        with pytest.raises(lib.SahsError, match=r"weights\[0\] must be torch\.float32"):
            ops.spectral_normalize([W.to(bad)], [u], [v], True)
        with pytest.raises(lib.SahsError, match=r"us\[0\] must be torch\.float32"):
            ops.spectral_normalize([W], [u.to(bad)], [v], True)
    with pytest.raises(lib.SahsError, match=r"vs\[0\] must be a contiguous vector of 5"):
        ops.spectral_normalize([W], [u], [torch.zeros(10, device=DEV)[::2]], True)
    with pytest.raises(lib.SahsError, match="grad_out"):
        tracked.grad_fn.apply(G.bfloat16())


# ---- the generators ----
@contextlib.contextmanager
def _power_iteration_outside_autocast():
    """Variant (c): torch's hooks with SpectralNorm.compute_weight run outside autocast (its matrix-vector products in fp32)."""
    torch_own = SpectralNorm.compute_weight

    def guarded(self, module, do_power_iteration):
        with torch.autocast("cuda", enabled=False):
            return torch_own(self, module, do_power_iteration)

    SpectralNorm.compute_weight = guarded
    try:
        yield
    finally:
        SpectralNorm.compute_weight = torch_own


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_fused_generator_reproduces_the_fixture(name):
    """Train mode, fp32: loss and every buffer's abs-sum (the 36 weight_u / weight_v included) within 1e-6 of the fixture's -- the bounds
    test_train_mode_forward_reproduces_the_reference puts on the torch path; gradients: G_fused <= 2 G_unfused, global relative L2
    against the float64 CPU step, G_unfused from the unfused module on the same GPU."""
    S, g, c = pkg("spade"), load_golden("spade_train"), R.cpu_step(name)
    G = R.seeded(name).to(DEV)
    twin = copy.deepcopy(G)
    S.fuse_spectral_norm_(G)
    inputs = R.step_inputs(name, DEV)
    _, loss, fused = R.loss_and_grads(G, *inputs)
    _, loss_unfused, unfused = R.loss_and_grads(twin, *inputs)
    fixture = float(g[name + ":loss"])
    have, want = R.buffer_abs_sums(G), g[name + ":buffer_abs_sums"]
    drop = lambda d: {k: v for k, v in d.items() if v is not None}
    g_fused, g_unfused = R.global_rel_l2(drop(fused), c["grads64"]), R.global_rel_l2(drop(unfused), c["grads64"])
    print("%s: loss %.9g (fixture %.9g: %.2e of it; unfused %.9g)  buffers: worst %.2e  G_fused %.3e  G_unfused %.3e"
          % (name, loss, fixture, abs(loss - fixture) / fixture, loss_unfused, (abs(have - want) / abs(want).clip(1e-300)).max(), g_fused, g_unfused))
    assert [k for k, _ in G.named_buffers()] == [str(k) for k in g[name + ":buffer_names"]]
    assert abs(loss - fixture) <= 1e-6 * fixture
    assert (abs(have - want) <= 1e-6 * abs(want)).all()
    assert g_fused <= 2.0 * g_unfused, (g_fused, g_unfused)
    assert sorted(k for k, v in fused.items() if v is None) == c["unreached"]


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_fused_refine_step_under_autocast(name):
    """refine_step(..., autocast_dtype=bfloat16) on a fused G against variant (c) on the same GPU:
    |loss - loss_c| <= 2 |loss_c - fixture loss|, G_fused <= 2 G_c."""
    S, g, c = pkg("spade"), load_golden("spade_train"), R.cpu_step(name)
    G = R.seeded(name).to(DEV)
    twin = copy.deepcopy(G)
    S.fuse_spectral_norm_(G)
    inputs = R.step_inputs(name, DEV)
    step = lambda net: float(S.refine_step(net, torch.optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.999)), *inputs, autocast_dtype=BF16))
    loss = step(G)
    with _power_iteration_outside_autocast():
        loss_c = step(twin)
    fixture = float(g[name + ":loss"])
    grads = lambda net: {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    g_fused, g_c = R.global_rel_l2(grads(G), c["grads64"]), R.global_rel_l2(grads(twin), c["grads64"])
    print("%s: loss %.9g, (c) %.9g, fixture %.9g  |loss - loss_c| %.3e, |loss_c - fixture| %.3e  G_fused %.3e  G_c %.3e"
          % (name, loss, loss_c, fixture, abs(loss - loss_c), abs(loss_c - fixture), g_fused, g_c))
    assert abs(loss - loss_c) <= 2.0 * abs(loss_c - fixture)
    assert g_fused <= 2.0 * g_c, (g_fused, g_c)
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in G.parameters())
    assert sorted(k for k, p in G.named_parameters() if p.grad is None) == c["unreached"]


def test_ten_steps_keep_the_power_iteration_on_course():
    """Ten fp32 refine_steps of Generator on a fused and on an unfused copy, same seed, against the same ten steps in float64 (the
    swapped tree on the CPU): for every weight_u, E_fused <= max(4 E_unfused, 2^-21) after the ten iterations."""
    S, name = pkg("spade"), "generator"
    G = R.seeded(name)
    runs = {"ref": copy.deepcopy(G).double(), "unfused": copy.deepcopy(G).to(DEV), "fused": S.fuse_spectral_norm_(copy.deepcopy(G).to(DEV))}
    for tag, net in runs.items():
        inputs = R.step_inputs(name, "cpu", torch.float64) if tag == "ref" else R.step_inputs(name, DEV)
        opt = torch.optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.999))
        with R.swapped() if tag == "ref" else contextlib.nullcontext():
            for _ in range(10):
                S.refine_step(net, opt, *inputs)
    us = {tag: {k: v for k, v in net.named_buffers() if k.endswith("weight_u")} for tag, net in runs.items()}
    assert len(us["ref"]) == 18      # (named_buffers names each module's buffer once, though 12 modules go under two names)
    worst, bad = (0.0, 0.0), []
    for k, ref in us["ref"].items():
        ef, eu = N.rel_max(us["fused"][k], ref), N.rel_max(us["unfused"][k], ref)
        worst = max(worst, (ef, eu))
        if not ef <= max(4.0 * eu, N.FLOOR):
            bad.append((k, ef, eu))
    print("ten steps: worst E_fused %.3e (E_unfused there %.3e)" % worst)
    assert not bad, bad


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_eval_output(name):
    """eval() under no_grad: the fused output against float64 of the same tree, E_fused <= max(4 E_unfused, 2^-21) of scale."""
    S = pkg("spade")
    G = R.seeded(name).eval()
    inputs = [t for t in R.step_inputs(name, "cpu", torch.float64) if t is not None]
    inputs = inputs[:2] + inputs[3:]      # (the target is not an input of the forward)
    with torch.no_grad():
        with R.swapped():
            ref = copy.deepcopy(G).double()(*inputs)
        on_gpu = copy.deepcopy(G).to(DEV)
        unfused = on_gpu(*(t.float().to(DEV) for t in inputs))
        fused = S.fuse_spectral_norm_(on_gpu)(*(t.float().to(DEV) for t in inputs))
    ef, eu = N.rel_max(fused, ref), N.rel_max(unfused, ref)
    print("%s eval: E_fused %.3e, E_unfused %.3e" % (name, ef, eu))
    assert ef <= max(4.0 * eu, N.FLOOR), (ef, eu)
    assert all(not k.endswith(("weight_u", "weight_v")) or torch.equal(b, dict(G.named_buffers())[k].to(DEV)) for k, b in on_gpu.named_buffers())
