"""The bf16 form of the fused SPADE modulation on the GPU (csrc/spade_ops.hip: the <unsigned short, 8> and <unsigned short, 1> instances
of instance_stats_kernel, spade_modulate_kernel, spade_backward_sums_kernel and spade_backward_apply_kernel, the loop bodies the fp32
instances run): at op level against a float64 yardstick on the same bf16 values, the
dtype dispatch of ``ops.spade_modulate``, SPADELayer / SPADEBlock and one ``refine_step`` of each generator under
``torch.autocast("cuda", dtype=torch.bfloat16)``, and ``G.bfloat16()`` inference.

Op level: the rule of tests/spade_bf16_reference.py -- (a) every element within one bf16 ulp of bfloat16(ref), (b) at most
ceil(1e-3 n) elements differ from it at all, (c) E <= 2^-8 + 4 max(E32, 2^-21), E32 from the fp32 kernels on the same values in the
same test.

Modules and generators: "swapped" is the same tree with ``ops.spade_modulate`` replaced by the written-out torch formula
(spade_reference.swapped) under the SAME autocast on the same GPU; the yardstick is float64 on the CPU.  Required: E_fused <= 2 E_swapped
(modules: E = the largest |g - g64| over x and every parameter, over the module's largest float64 gradient, the scale
test_gpu_spade_backward.py::test_module_gradients uses) and G_fused <= 2 G_swapped (generators: global relative L2).  The fused op rounds
once where the formula rounds after each op that autocast leaves in bf16, so the ratio is expected near or below 1; the factor 2 covers
activation-kink flips in either direction at bf16 resolution on fixtures too small to average them out.

Measured on an MI355X (each test prints its figures before it asserts; DESIGN.md section 9 has them too): see MEASURED below.
"""
import copy
import itertools
import math
import time

import pytest
import torch

import spade_bf16_reference as B
import spade_reference as R
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
GRADS = ("dx", "dgamma", "dbeta")
AUTOCAST = lambda: torch.autocast("cuda", dtype=BF16)

# refine_step under autocast, from the SWAPPED tree's first measured run on an MI355X (the reference of these bounds, not the code under
# test): |loss_swapped - fixture loss| (the loss bound is twice that) and G_swapped (its cap is three times that).
SWAPPED_LOSS_DEVIATION = {"generator": 2.742e-05, "generator_audio": 3.973e-04}      # loss bounds: 5.484e-05 and 7.946e-04
SWAPPED_G = {"generator": 2.457e-01, "generator_audio": 2.609e-01}                   # caps: 7.371e-01 and 7.827e-01
MEASURED = """
op level, 8 shapes x 3 slopes x (out, dx, dgamma, dbeta): never more than one ulp from bfloat16(ref); elements that differ from it at all:
  at most 7 of 81920 (many_planes dx, slope 0; cap 82), 1 of 34816 (partial_trip), 1 of 945 (ragged dx, slope 0.2; cap 1), none in the
  other cases; E at most 3.37e-3 (one_vector dx) against the bound 3.91e-3, E32 of the fp32 kernels on the same values 0 .. 2.0e-7;
SPADELayer: E_fused 2.751e-2, E_swapped 2.738e-2 (both at mlp_shared.0.weight); SPADEBlock: 9.055e-2 and 9.055e-2 (conv2.weight_orig):
  under autocast the error is that of the bf16 convolutions, which both trees share;
refine_step: Generator loss 0.266985744 (fixture 0.267020047; swapped 0.267047465), G_fused 2.448e-1, G_swapped 2.457e-1;
  Generator_audio loss 0.260223806 (fixture 0.259922206; swapped 0.260319471), G_fused 2.576e-1, G_swapped 2.609e-1 -- a quarter of the
  gradient's norm on these 32 x 32 frames is bf16 convolution error and kink flips, the same in both trees; cold wall time of the fused
  step, MIOpen's first bf16 convolutions included: 4.7 s and 2.9 s;
G.bfloat16().eval(): PSNR against the fp32 output, Generator 21.88 dB fused and 21.64 dB swapped, Generator_audio 22.32 dB and 20.34 dB.
"""


def _gpu(case, t):
    """t on the GPU; a bf16 tensor of the unaligned cases as a view OFFSET[case] elements into a flat buffer (contiguous, not 16-byte
    aligned).  The fp32 run of the same values is only the source of E32 and stays aligned."""
    off = B.OFFSET.get(case, 0) if t.dtype == BF16 else 0
    if not off:
        return t.to(DEV)
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off * t.element_size()
    return v


def _run(case, slope, needs=(True, True, True), grad_out=None, dtype=BF16):
    """The op on the case's values in ``dtype`` (bf16: the new kernels; float32: the fp32 kernels on the same values widened)
    -> (out, [dx, dgamma, dbeta])."""
    ops = pkg("ops")
    x, gamma, beta, g = (t.to(dtype) for t in B.op_case_bf16(case, slope))
    leaves = [_gpu(case, t).requires_grad_(n) for t, n in zip((x, gamma, beta), needs)]
    out = ops.spade_modulate(*leaves, eps=B.EPS, slope=slope)
    assert out.grad_fn is not None and out.dtype == dtype
    out.backward(_gpu(case, g) if grad_out is None else grad_out(out))
    assert all(t.grad is None or t.grad.dtype == dtype for t in leaves)
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("slope", B.SLOPES)
@pytest.mark.parametrize("case", sorted(B.OP_CASES))
def test_op_accuracy(case, slope):
    ref = B.reference(case, slope)
    out, grads = _run(case, slope)
    out32, grads32 = _run(case, slope, dtype=torch.float32)
    verdicts = []
    for name, got, f32, r in zip(B.NAMES, [out] + grads, [out32] + grads32, ref):
        ok, text = B.rule(got, r, R.rel_max(f32, r))
        print("%s slope %g %s: %s" % (case, slope, name, text))
        verdicts.append((name, ok, text))
    assert all(ok for _, ok, _ in verdicts), [v for v in verdicts if not v[1]]


@pytest.mark.parametrize("case", ("ragged", "partial_trip"))      # the scalar and the 16-byte path
def test_every_subset_of_wanted_gradients(case):
    out, full = _run(case, 0.2)
    for needs in itertools.product((False, True), repeat=3):
        if not any(needs):
            continue
        again, grads = _run(case, 0.2, needs)
        assert torch.equal(again, out)
        for n, need, got, ref in zip(GRADS, needs, grads, full):
            assert (got is None) if not need else torch.equal(got, ref), (needs, n)
    _, second = _run(case, 0.2)
    assert all(torch.equal(a, b) for a, b in zip(full, second))      # no atomics: the same bits


@pytest.mark.parametrize("slope", (0.2, 1.0))
def test_stride0_gradient(slope):
    """out.sum().backward() hands the backward a stride-0 expansion of a bf16 one."""
    ops = pkg("ops")
    _, ones = _run("partial_trip", slope, grad_out=torch.ones_like)
    leaves = [t.to(DEV).requires_grad_(True) for t in B.op_case_bf16("partial_trip", slope)[:3]]
    ops.spade_modulate(*leaves, eps=B.EPS, slope=slope).sum().backward()
    assert all(t.grad.dtype == BF16 and torch.equal(t.grad, a) for t, a in zip(leaves, ones))


def test_dispatch_on_dtype():
    ops, lib = pkg("ops"), pkg("_lib")
    x, gamma, beta, g = (t.to(DEV) for t in B.op_case_bf16("ragged", 0.2))
    plain = ops.spade_modulate(x, gamma, beta, slope=0.2)
    assert plain.dtype == BF16 and plain.grad_fn is None
    assert B.rule(plain, B.reference("ragged", 0.2)[0], 0.0)[0]
    # a mixture is the fp32 op on the widened tensors, bit for bit -- forward and gradients (autograd narrows a bf16 leaf's gradient)
    want = ops.spade_modulate(x.float(), gamma.float(), beta.float(), slope=0.2)
    for mix in itertools.product((False, True), repeat=3):
        if all(mix) or not any(mix):
            continue
        got = ops.spade_modulate(*(t if keep else t.float() for t, keep in zip((x, gamma, beta), mix)), slope=0.2)
        assert got.dtype == torch.float32 and torch.equal(got, want), mix
    wide = [t.float().requires_grad_(True) for t in (x, gamma, beta)]
    ops.spade_modulate(*wide, slope=0.2).backward(g.float())
    leaves = [x.clone().requires_grad_(True), gamma.float().requires_grad_(True), beta.clone().requires_grad_(True)]
    out = ops.spade_modulate(*leaves, slope=0.2)
    assert out.dtype == torch.float32
    out.backward(g.float())
    for t, w in zip(leaves, wide):
        assert t.grad.dtype == t.dtype and torch.equal(t.grad, w.grad.to(t.dtype))
    for bad in (torch.float16, torch.float64):
        with pytest.raises(lib.SahsError, match=r"torch\.float32 or torch\.bfloat16"):
            ops.spade_modulate(x.to(bad), gamma.to(bad), beta.to(bad))
        with pytest.raises(lib.SahsError, match=r"torch\.float32 or torch\.bfloat16"):
            ops.spade_modulate(x, gamma.to(bad), beta)
    # the backward wants grad_out in the dtype of the saved x
    held = ops.spade_modulate(x.clone().requires_grad_(True), gamma, beta, slope=0.2)
    with pytest.raises(lib.SahsError, match="grad_out"):
        held.grad_fn.apply(g.float())


def test_plane_limit_is_named():
    """65536 planes: both bf16 entry points refuse with a message that names the limit, before any launch."""
    ops, lib = pkg("ops"), pkg("_lib")
    z = torch.zeros(1, 65536, 1, 1, dtype=BF16, device=DEV)
    with pytest.raises(lib.SahsError, match="65535"):
        ops.spade_modulate(z, z, z)
    L, P = lib.lib(), ops._p
    stats = torch.zeros(int(L.sahs_spade_modulate_workspace_words(65536)), device=DEV)
    d = torch.empty_like(z)
    assert L.sahs_spade_modulate_backward_bf16(65536, 1, P(z), P(z), P(z), P(stats), P(z), 1e-5, 0.2, P(d), None, None, P(stats), None) == 1
    assert b"65535" in L.sahs_last_error()
    ok = torch.zeros(1, 65535, 1, 1, dtype=BF16, device=DEV)
    assert float(ops.spade_modulate(ok, ok, ok).abs().max()) == 0.0


# ---- SPADELayer / SPADEBlock under autocast ----
def _module(name):
    S, g = pkg("spade"), load_golden("spade")
    cfg = [int(v) for v in g[name + ":cfg"]]
    m = S.SPADELayer(cfg[0], cfg[1]) if name == "layer" else S.SPADEBlock(cfg[0], cfg[1], cfg[2])
    pre = name + ":sd:"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g if k.startswith(pre)})
    # x is rounded to bf16 once and every run reads those values: as in the network, where a convolution hands x over in bf16
    return m.eval(), torch.from_numpy(g[name + ":x"]).bfloat16(), torch.from_numpy(g[name + ":fid"])


def _module_grads(m, x, fid, w, device, dtype=None):
    """dtype None: fp32 parameters under autocast with x as a bf16 leaf; else everything in ``dtype``, no autocast."""
    m = copy.deepcopy(m).to(device=device, dtype=dtype or torch.float32)
    x = x.to(device=device, dtype=dtype or BF16).requires_grad_(True)
    fid, w = fid.to(device=device, dtype=dtype or torch.float32), w.to(device=device, dtype=dtype or torch.float32)
    if dtype is None:
        with AUTOCAST():
            y = m(x, fid)
        y = y.float()
    else:
        y = m(x, fid)
    (y * w).sum().backward()
    return dict([("x", x.grad)] + [(k, p.grad) for k, p in m.named_parameters()])


@pytest.mark.parametrize("name", ("layer", "block"))
def test_module_gradients_under_autocast(name):
    m, x, fid = _module(name)
    with torch.no_grad(), R.swapped():
        shape = m(x.float(), fid).shape
    w = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    with R.swapped():
        want = _module_grads(m, x, fid, w, "cpu", torch.float64)
        swapped = _module_grads(m, x, fid, w, DEV)
    fused = _module_grads(m, x, fid, w, DEV)
    assert all(v is not None for v in want.values()) and sorted(fused) == sorted(want)
    scale = max(float(v.abs().max()) for v in want.values())
    e = {}
    for tag, d in (("fused", fused), ("swapped", swapped)):
        per = {k: float((d[k].double().cpu() - ref).abs().max()) / scale for k, ref in want.items()}
        e[tag] = max(per.values())
        print("%s %s: E %.3e (worst tensor %s)" % (name, tag, e[tag], max(per, key=per.get)))
    assert e["fused"] <= 2.0 * e["swapped"], e


# ---- refine_step under autocast ----
@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_refine_step_under_autocast(name):
    """One refine_step(..., autocast_dtype=torch.bfloat16) of the generator in train() mode with torch.optim.Adam, on the fixture's inputs."""
    S, g, c = pkg("spade"), load_golden("spade_train"), R.cpu_step(name)
    fixture = float(g[name + ":loss"])
    t0 = time.perf_counter()
    G = R.seeded(name).to(DEV)
    twin = copy.deepcopy(G)
    before = {k: p.detach().clone() for k, p in G.named_parameters()}
    inputs = R.step_inputs(name, DEV)
    opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    loss = float(S.refine_step(G, opt, *inputs, autocast_dtype=BF16))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    fused = {k: p.grad for k, p in G.named_parameters()}
    i_src, i_raw, target, driving = inputs
    with R.swapped(), AUTOCAST():
        y = twin(i_src, i_raw) if driving is None else twin(i_src, i_raw, driving)
        loss_swapped = torch.nn.functional.mse_loss(y.clamp(0, 1), target)
    loss_swapped.backward()
    swapped = {k: p.grad for k, p in twin.named_parameters()}
    g_fused, g_swapped = R.global_rel_l2(fused, c["grads64"]), R.global_rel_l2(swapped, c["grads64"])
    print("%s: loss %.9g (fixture %.9g, swapped %.9g: deviation %.3e)  G_fused %.3e  G_swapped %.3e  wall of the fused step %.1f s"
          % (name, loss, fixture, float(loss_swapped), abs(float(loss_swapped) - fixture), g_fused, g_swapped, wall))
    assert abs(loss - fixture) <= 2.0 * SWAPPED_LOSS_DEVIATION[name], (loss, fixture)
    assert g_swapped <= 3.0 * SWAPPED_G[name], g_swapped
    assert g_fused <= 2.0 * g_swapped, (g_fused, g_swapped)
    assert sorted(k for k, v in fused.items() if v is None) == c["unreached"]
    after = dict(G.named_parameters())
    for k, ref in c["grads64"].items():
        if float(ref.abs().max()) > 0.0:
            assert not torch.equal(after[k].detach(), before[k]), k
    assert all(p.dtype == torch.float32 and (p.grad is None or p.grad.dtype == torch.float32) for p in G.parameters())
    state = [v for s in opt.state.values() for k, v in s.items() if k in ("exp_avg", "exp_avg_sq")]
    assert state and all(v.dtype == torch.float32 for v in state)


# ---- G.bfloat16().eval() ----
def _psnr(a, b):
    return 10.0 * math.log10(1.0 / max(float((a.double() - b.double()).pow(2).mean()), 1e-300))


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_bfloat16_module_inference(name):
    """G.bfloat16().eval() on the inputs of tests/golden/spade.npz against the fp32 fused output, PSNR over the clamped image: the fused
    tree must be no further from it than the swapped tree under the same cast."""
    S, g = pkg("spade"), load_golden("spade")
    torch.manual_seed(int(g[name + ":seed"]))
    G = getattr(S, R.GENERATORS[name])().eval().to(DEV)
    inputs = [torch.from_numpy(g[name + ":" + k]).to(DEV) for k in ("i_src", "i_raw", "window") if name + ":" + k in g]
    Gb = copy.deepcopy(G).bfloat16()
    with torch.no_grad():
        y32 = G(*inputs).clamp(0, 1)
        fused = Gb(*(t.bfloat16() for t in inputs))
        with R.swapped():
            swapped = Gb(*(t.bfloat16() for t in inputs))
    assert fused.dtype == BF16 and fused.shape == y32.shape
    p_fused, p_swapped = _psnr(fused.float().clamp(0, 1), y32), _psnr(swapped.float().clamp(0, 1), y32)
    print("%s: PSNR against the fp32 output, fused %.2f dB, swapped %.2f dB" % (name, p_fused, p_swapped))
    assert p_fused >= p_swapped, (p_fused, p_swapped)
