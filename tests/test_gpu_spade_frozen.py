"""Stage-II inference on the GPU: ``ops.spade_modulate_frozen`` (csrc/spade_ops.hip: spade_modulate_frozen_kernel and
spade_modulate_frozen_up_kernel behind the statistics passes of the per-frame op), ``spade.freeze_identity`` and ``spade.refine_frames``.

Op level: the frozen kernels share the statistics kernel and the per-element device function with ``ops.spade_modulate`` and the build
forbids contraction, so the results are held to BIT equality with that op: for up=False on the same operands (a shared map against the
per-frame op called row by row with it); for up=True phase by phase -- out[:, :, di::2, dj::2] is the per-frame op on the source x with
that phase of gamma and beta (same statistics: every source value occurs four times in the upsampled plane).

Generators: conftest.yardstick with the project's own factors -- rms <= 2x, max <= 3x the unfrozen GPU path's error against float64, plus
``ulps``.  For dtype=bfloat16 ref32 is G under bf16 autocast on the GPU and ulps = 2^16 k with k = 1: bf16 keeps 8 significant bits
where fp32 keeps 24, so one bf16 ulp is 2^16 fp32 ulps, and both outputs are rounded to bf16 ONCE at the last convolution -- two
equally good runs may land one bf16 ulp of the largest magnitude apart, and no more is granted.
"""
import pytest
import torch

import spade_frozen_reference as FR
import spade_reference as R
from conftest import pkg, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BF16_ULPS = 2.0 ** 16 * 1


def _gpu(t, offset=0):
    """t on the GPU, contiguous, starting ``offset`` elements past a 256-byte aligned address."""
    v = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)[offset:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == offset * t.element_size()
    return v


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("case", sorted(R.OP_CASES))
def test_op_bits_of_the_per_frame_op(case, slope, dtype):
    ops = pkg("ops")
    off = 1 if case == "unaligned" else 0
    x, gamma, beta = (_gpu(t.to(DTYPES[dtype]), off) for t in R.op_case(case, slope)[:3])
    want = ops.spade_modulate(x, gamma, beta, eps=R.EPS, slope=slope)
    got = ops.spade_modulate_frozen(x, gamma, beta, eps=R.EPS, slope=slope)
    assert got.dtype == want.dtype == DTYPES[dtype] and torch.equal(got, want), "Bg = B"
    shared = torch.cat([ops.spade_modulate(x[b:b + 1], gamma[:1], beta[:1], eps=R.EPS, slope=slope) for b in range(x.shape[0])])
    got = ops.spade_modulate_frozen(x, gamma[:1], beta[:1], eps=R.EPS, slope=slope)
    assert torch.equal(got, shared), "Bg = 1"
    assert torch.equal(got, ops.spade_modulate_frozen(x, gamma[:1], beta[:1], eps=R.EPS, slope=slope)), "twice: equal bits"
    if x.shape[0] > 1:
        assert not torch.equal(got, want)      # (the shared map is another operand: the two halves of this test are two tests)


# name -> (source shape, element offset of x, element offset of gamma / beta)
UP_CASES = {"scalar": ((3, 5, 3, 5), 0, 0),               # W = 10: no group of 4 divides the output row
            "tiny": ((1, 2, 1, 2), 0, 0),                 # hw = 2: fewer elements than statistics chunks
            "vector": ((2, 3, 48, 96), 0, 0),             # 16-byte path; 288 source groups per chunk, a partial second trip
            "unaligned": ((2, 4, 4, 4), 1, 1),            # every tensor one element into its buffer: element by element
            "half_aligned": ((1, 2, 4, 8), None, 0)}      # x 8 bytes past alignment: 16-byte modulate path over scalar statistics


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("case", sorted(UP_CASES))
def test_op_up_phases_are_the_per_frame_op(case, slope, dtype):
    ops = pkg("ops")
    shape, xoff, moff = UP_CASES[case]
    dt = DTYPES[dtype]
    if xoff is None:
        xoff = 8 // torch.empty(0, dtype=dt).element_size()
    gen = torch.Generator().manual_seed(2000 + sorted(UP_CASES).index(case))
    B, C, h, w = shape
    x = _gpu((torch.randn(shape, generator=gen) * 3 + 1).to(dt), xoff)
    gamma, beta = (_gpu(torch.randn(B, C, 2 * h, 2 * w, generator=gen).to(dt), moff) for _ in range(2))
    for maps in ((gamma, beta), (gamma[:1], beta[:1])):
        got = ops.spade_modulate_frozen(x, maps[0], maps[1], eps=R.EPS, slope=slope, up=True)
        assert tuple(got.shape) == (B, C, 2 * h, 2 * w) and got.dtype == dt
        for di in range(2):
            for dj in range(2):
                g, b = (m[:, :, di::2, dj::2].contiguous() for m in maps)
                if g.shape[0] == B:
                    want = ops.spade_modulate(x, g, b, eps=R.EPS, slope=slope)
                else:
                    want = torch.cat([ops.spade_modulate(x[k:k + 1], g, b, eps=R.EPS, slope=slope) for k in range(B)])
                assert torch.equal(got[:, :, di::2, dj::2], want), (case, "Bg = %d" % g.shape[0], di, dj)
        assert torch.equal(got, ops.spade_modulate_frozen(x, maps[0], maps[1], eps=R.EPS, slope=slope, up=True))
    # and the phases are laid out as F.interpolate lays them out: against the written-out formula in float64 on the same values, to the
    # output's rounding (bf16: half an ulp, 2^-9 of the element <= 2^-9 of the largest, doubled) or 1e-5 (fp32: ~100 ulps)
    ref = FR.torch_modulate_frozen(x.double().cpu(), gamma.double().cpu(), beta.double().cpu(), slope=slope, up=True)
    E = R.rel_max(ops.spade_modulate_frozen(x, gamma, beta, eps=R.EPS, slope=slope, up=True), ref)
    print("%s %s slope %g: E = %.3e" % (case, dtype, slope, E))
    assert E <= (2.0 ** -8 if dt == torch.bfloat16 else 1e-5)


def test_op_more_planes_than_a_grid_dimension():
    """B * C = 70000 planes of one element: the channel is on the grid, the batch a loop.  A plane of one element normalises to exactly
    0, so the output is lrelu(beta) bit for bit."""
    ops = pkg("ops")
    gen = torch.Generator().manual_seed(5)
    x, gamma, beta = (torch.randn(14000, 5, 1, 1, generator=gen).to(DEV) for _ in range(3))
    got = ops.spade_modulate_frozen(x, gamma, beta, slope=0.2)
    assert torch.equal(got, torch.nn.functional.leaky_relu(beta, 0.2))
    got = ops.spade_modulate_frozen(x, gamma[:1], beta[:1], slope=0.2)
    assert torch.equal(got, torch.nn.functional.leaky_relu(beta[:1], 0.2).expand_as(x))


def test_op_refusals():
    ops, lib = pkg("ops"), pkg("_lib")
    x, m = torch.randn(3, 2, 4, 4, device=DEV), torch.randn(3, 2, 4, 4, device=DEV)
    with pytest.raises(lib.SahsError, match=r"\(2, 2, 4, 4\)"):      # Bg = 2 with B = 3; the message names the shapes
        ops.spade_modulate_frozen(x, m[:2], m[:2])
    with pytest.raises(lib.SahsError, match="invalid argument"):      # ... and the C entry refuses it on its own
        lib.check(lib.lib().sahs_spade_modulate_frozen(3, 2, 4, 4, 2, 0, ops._p(x), ops._p(m), ops._p(m), 1e-5, 1.0, ops._p(torch.empty_like(x)),
                                                       ops._p(torch.empty(96, device=DEV)), ops._stream()), "sahs_spade_modulate_frozen")
    with pytest.raises(lib.SahsError, match="channels <= 65535"):
        lib.check(lib.lib().sahs_spade_modulate_frozen(1, 65536, 1, 1, 1, 0, ops._p(x), ops._p(m), ops._p(m), 1e-5, 1.0, ops._p(x),
                                                       ops._p(x), ops._stream()), "sahs_spade_modulate_frozen")
    with pytest.raises(lib.SahsError, match=r"\(3, 2, 4, 4\)"):      # up=True wants (8, 8) maps
        ops.spade_modulate_frozen(x, m, m, up=True)
    with pytest.raises(lib.SahsError, match="no backward"):
        ops.spade_modulate_frozen(x.clone().requires_grad_(True), m, m)
    with torch.no_grad():
        ops.spade_modulate_frozen(x.clone().requires_grad_(True), m, m)
    with pytest.raises(lib.SahsError):
        ops.spade_modulate_frozen(x.double(), m.double(), m.double())
    mixed = ops.spade_modulate_frozen(x.bfloat16(), m, m)      # a mixture is widened to float32
    assert mixed.dtype == torch.float32 and torch.equal(mixed, ops.spade_modulate_frozen(x.bfloat16().float(), m, m))


@pytest.fixture(scope="module")
def gpu_runs():
    """name, dtype -> (G on the GPU, ref32 (3, 3, H, W) float32 on the CPU): the unfrozen path row by row, computed once."""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            G = FR.generator(name).to(DEV)
            i_src, i_raw, windows = (None if t is None else t.to(DEV) for t in FR.inputs(name))
            if dtype == "bf16":
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    ref32 = FR.run(G, i_src, i_raw, windows)
                assert ref32.dtype == torch.bfloat16
            else:
                ref32 = FR.run(G, i_src, i_raw, windows)
            cache[name, dtype] = G, ref32.float().cpu()
        return cache[name, dtype]

    return get


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(FR.SIZES))
def test_frozen_generator(gpu_runs, name, dtype, batch, fold):
    S = pkg("spade")
    G, ref32 = gpu_runs(name, dtype)
    i_src, i_raw, windows = (None if t is None else t.to(DEV) for t in FR.inputs(name))
    frozen = S.freeze_identity(G, i_src, dtype=DTYPES[dtype], fold_upsample=fold)
    got = frozen(i_raw[:batch]) if windows is None else frozen(i_raw[:batch], windows[:batch])
    assert got.dtype == torch.float32 and tuple(got.shape) == (batch, 3) + FR.SIZES[name]
    rec = yardstick(got, ref32[:batch].numpy(), FR.reference64(name)[:batch].numpy(), "frozen %s %s B=%d fold=%s" % (name, dtype, batch, fold),
                    ulps=BF16_ULPS if dtype == "bf16" else 32.0)
    print("max %.3e (unfrozen %.3e)  rms %.3e (unfrozen %.3e)  scale %.3e" % rec[1:])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_frozen_generator_after_fuse_spectral_norm(gpu_runs, dtype):
    """The snapshot takes its spectral-normalised weights from fuse_spectral_norm_'s single hook (ops.spectral_normalize) as well."""
    import copy
    S = pkg("spade")
    name = "generator"
    G, ref32 = gpu_runs(name, dtype)
    i_src, i_raw, _ = (None if t is None else t.to(DEV) for t in FR.inputs(name))
    got = S.freeze_identity(S.fuse_spectral_norm_(copy.deepcopy(G)), i_src, dtype=DTYPES[dtype])(i_raw)
    yardstick(got, ref32.numpy(), FR.reference64(name).numpy(), "frozen %s %s after fuse_spectral_norm_" % (name, dtype),
              ulps=BF16_ULPS if dtype == "bf16" else 32.0)


@pytest.mark.parametrize("name", sorted(FR.SIZES))
def test_refine_frames_bytes(name):
    S = pkg("spade")
    G = FR.generator(name, image_range=True).to(DEV)
    i_src, _, windows = (None if t is None else t.to(DEV) for t in FR.inputs(name))
    frames = [f.to(DEV) for f in FR.frames_u8(name)]
    got = S.refine_frames(S.freeze_identity(G, i_src), frames, driving=windows, batch=2, log=None)
    assert all(g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == FR.SIZES[name] + (3,) for g in got)
    want, scaled = FR.frames_bytes64(name)
    worst, equal = FR.bytes_agreement(got, want)
    with FR.swapped():      # the cap is one the unfrozen float32 path keeps on these inputs (CPU)
        y32 = FR.run(FR.generator(name, image_range=True), FR.inputs(name)[0], FR.frames_input(FR.frames_u8(name)), FR.inputs(name)[2])
    worst32, equal32 = FR.bytes_agreement(FR.to_bytes(y32), want)
    print("%s: worst %d level, %.4f %% equal (unfrozen fp32 on the CPU: %d, %.4f %%); %.1f %% of the values inside (0, 255)"
          % (name, worst, 100 * equal, worst32, 100 * equal32, 100 * float(((scaled > 0) & (scaled < 255)).double().mean())))
    assert worst32 <= 1 and equal32 >= FR.BYTES_EQUAL_CAP
    assert worst <= 1 and equal >= FR.BYTES_EQUAL_CAP
