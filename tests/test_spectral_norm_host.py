"""The fused spectral norm, the parts a CPU can check: the float64 restatements of tests/spectral_norm_reference.py against torch's own
SpectralNorm and its autograd in float64; the hook surgery of ``spade.fuse_spectral_norm_`` / ``unfuse_spectral_norm_`` on CPU modules
(no forward needed); the refusals of the two C entry points, which are answered before any launch; and that the cap the GPU test puts on
bf16 outputs is one torch's own fp32 result meets on the same inputs."""
import copy
import ctypes

import pytest
import torch
from torch.nn.utils import spectral_norm
from torch.nn.utils.spectral_norm import SpectralNorm

import spectral_norm_reference as N
from conftest import pkg


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("name", sorted(N.CASES))
def test_float64_restatement_is_torch_in_float64(name, training):
    W, u, v, G = (t.double() for t in N.case(name))
    out, u1, v1, sigma, dW = N.torch_spectral_norm(W, u, v, training, G)
    ref = N.compute_weight64(W, u, v, training)
    for what, got, want in zip(("out", "u", "v", "sigma"), (out, u1, v1, sigma), ref):
        assert N.rel_max(got, want) <= 1e-12, (what, N.rel_max(got, want))
    if not training:
        assert torch.equal(u1, u) and torch.equal(v1, v)
    want = N.backward64(W, ref[1], ref[2], ref[3], G)
    scale = float((G / ref[3]).abs().max())      # (1 x 1: dW is analytically 0 -- the scale is that of its two terms)
    assert float((dW - want).abs().max()) <= 1e-12 * scale, float((dW - want).abs().max()) / scale


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("name", sorted(N.CASES))
def test_bf16_cap_is_met_by_torch_fp32(name, training):
    """What autocast's cast of torch's fp32 result gives, against bfloat16(float64 result): the GPU test's rule for the fused bf16 output."""
    W, u, v, _ = N.case(name)
    out32 = N.torch_spectral_norm(W, u, v, training)[0]
    ok, text = N.bf16_rule(out32.bfloat16(), N.compute_weight64(W, u, v, training)[0])
    print("%s training %d: %s" % (name, training, text))
    assert ok, text


def test_bf16_of_float64_rounds_once():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -0.05, 3.0e-3], dtype=torch.float64)
    got = N.bf16_of_float64(x)
    assert got.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]      # ties to even; the last is past the tie only in float64
    assert float(x[3].float().bfloat16()) == 1.0                                 # (torch's cast rounds to float32 first: the tie again)
    assert torch.equal(got[4:], x[4:].bfloat16().double())


# ---- hook surgery ----
def _sn_hooks(module):
    return [(m, k) for m in module.modules() for k, h in m._forward_pre_hooks.items() if isinstance(h, SpectralNorm)]


def _fused(module):
    S = pkg("spade")
    return [h for h in module._forward_pre_hooks.values() if isinstance(h, S._FusedSpectralNorm)]


@pytest.mark.parametrize("name", ("Generator", "Generator_audio"))
def test_fuse_and_unfuse_leave_the_state_alone(name):
    S = pkg("spade")
    torch.manual_seed(3)
    G = getattr(S, name)()
    sd = {k: v.clone() for k, v in G.state_dict().items()}
    params, hooks = [id(p) for p in G.parameters()], _sn_hooks(G)
    assert len(hooks) == 18 and any(k.endswith("conv1_sn.weight_u") for k in sd)

    def same_state():
        now = G.state_dict()
        return list(now) == list(sd) and all(torch.equal(now[k], sd[k]) for k in sd) and [id(p) for p in G.parameters()] == params

    assert S.unfuse_spectral_norm_(G) is G and _sn_hooks(G) == hooks and not _fused(G)      # unfusing an unfused module: nothing
    assert S.fuse_spectral_norm_(G) is G and same_state()
    (hook,) = _fused(G)
    assert not _sn_hooks(G) and len(hook.entries) == 18 and len({id(m) for m, _, _ in hook.entries}) == 18
    assert all(isinstance(m, torch.nn.Conv2d) for m, _, _ in hook.entries)
    assert S.fuse_spectral_norm_(G) is G and _fused(G) == [hook] and len(hook.entries) == 18            # fusing twice: nothing
    twin = copy.deepcopy(G)
    (thook,) = _fused(twin)
    mine, theirs = {id(m) for m in twin.modules()}, {id(m) for m in G.modules()}
    ids = {id(m) for m, _, _ in thook.entries}
    assert len(ids) == 18 and ids <= mine and not ids & theirs
    G.load_state_dict(sd)
    assert same_state()
    assert S.unfuse_spectral_norm_(G) is G and sorted(map(id, (m for m, _ in _sn_hooks(G)))) == sorted(map(id, (m for m, _ in hooks)))
    assert not _fused(G) and same_state()
    assert all(isinstance(m._forward_pre_hooks[k], SpectralNorm) for m, k in hooks)
    S.fuse_spectral_norm_(G)
    assert len(_fused(G)) == 1 and not _sn_hooks(G) and same_state()


@pytest.mark.parametrize("bad, word", (("iterations", "n_power_iterations=2"), ("transposed", "dim=1")))
def test_fuse_refuses_what_the_op_does_not_do(bad, word):
    S = pkg("spade")
    odd = spectral_norm(torch.nn.Conv2d(3, 4, 3), n_power_iterations=2) if bad == "iterations" else spectral_norm(torch.nn.ConvTranspose2d(3, 4, 3))
    net = torch.nn.Sequential(spectral_norm(torch.nn.Conv2d(3, 3, 3)), odd)
    before = _sn_hooks(net)
    assert len(before) == 2
    with pytest.raises(ValueError, match=word):
        S.fuse_spectral_norm_(net)
    assert _sn_hooks(net) == before and not _fused(net)


# ---- the C entry points refuse before any launch ----
def _table(n, value=1 << 20):
    return (ctypes.c_void_p * n)(*([value] * n))


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def test_entries_refuse_before_any_launch():
    """Every call here is answered by argument validation (fabricated addresses, never dereferenced) -- with or without a GPU."""
    L = pkg("_lib").lib()

    def forward(jobs=2, W=True, u=True, v=True, out=True, saved=True, h=(3, 4), w=(5, 6), bf16=0, power_iteration=1, eps=1e-12, hole=None):
        n = max(jobs, 1)
        tables = {k: (_table(n) if given else None) for k, given in (("W", W), ("u", u), ("v", v), ("out", out), ("saved", saved))}
        if hole:
            tables[hole][n - 1] = None
        return L.sahs_spectral_norm_forward(jobs, tables["W"], tables["u"], tables["v"], tables["out"], tables["saved"],
                                            None if h is None else _ints(h), None if w is None else _ints(w), bf16, power_iteration, eps, None)

    def backward(jobs=2, W=True, saved=True, grad_out=True, dW=True, h=(3, 4), w=(5, 6), bf16=0, hole=None):
        n = max(jobs, 1)
        tables = {k: (_table(n) if given else None) for k, given in (("W", W), ("saved", saved), ("grad_out", grad_out), ("dW", dW))}
        if hole:
            tables[hole][n - 1] = None
        return L.sahs_spectral_norm_backward(jobs, tables["W"], tables["saved"], tables["grad_out"], tables["dW"],
                                             None if h is None else _ints(h), None if w is None else _ints(w), bf16, None)

    def refused(code, *words):
        msg = L.sahs_last_error()
        assert code == 1 and all(word in msg for word in words), (code, msg)

    many = dict(h=(1,) * 33, w=(1,) * 33)
    for call, name in ((forward, b"sahs_spectral_norm_forward"), (backward, b"sahs_spectral_norm_backward")):
        refused(call(jobs=0), name, b"jobs = 0")
        refused(call(jobs=-1), name, b"jobs = -1")
        refused(call(jobs=33, **many), name, b"jobs = 33", b"32")
        refused(call(h=None), name, b"null pointer", b"h or w")
        refused(call(w=None), name, b"null pointer", b"h or w")
        refused(call(h=(3, 0)), name, b"job 1 is 0 x 6")
        refused(call(w=(0, 6)), name, b"job 0 is 3 x 0")
        refused(call(h=(3, -4)), name, b"job 1")
        refused(call(h=(65536, 4), w=(32768, 6)), name, b"job 0 is 65536 x 32768", b"2^31")
        assert call(jobs=1, h=(65536,), w=(32767,), W=False) == 1 and b"2^31" not in L.sahs_last_error()      # just below: the next check answers
    for table in ("W", "u", "v", "out", "saved"):
        refused(forward(**{table: False}), b"null pointer for the table " + table.encode())
        refused(forward(hole=table), b"null pointer " + table.encode() + b"[1]")
    for table in ("W", "saved", "grad_out", "dW"):
        refused(backward(**{table: False}), b"null pointer for the table " + table.encode())
        refused(backward(hole=table), b"null pointer " + table.encode() + b"[1]")
    for eps in (0.0, -1e-12, float("nan")):
        refused(forward(eps=eps), b"eps")
    for it in (2, -1):
        refused(forward(power_iteration=it), b"power_iteration = %d" % it)


def test_spectral_normalize_has_no_cpu_path():
    ops, lib = pkg("ops"), pkg("_lib")
    W, u, v, _ = N.case("3x5")
    with pytest.raises(lib.SahsError, match="GPU tensor"):
        ops.spectral_normalize([W], [u], [v], True)
    with pytest.raises(lib.SahsError, match="one length"):
        ops.spectral_normalize([W], [u, u], [v], True)
    assert ops.spectral_normalize([], [], [], True) == []
