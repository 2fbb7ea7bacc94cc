"""Host checks of tests/field_reference.py, the shared half of the field kernels' tile tests (tests/test_gpu_field_tiles.py): the size
planner against a direct walk of the persistent loop, slicing and re-assembly of plane buffers against direct indexing, the sign-bit
decoder, the float64 eager field against the golden float64 run, the comparators' sensitivity, and the restated plane tables against the
library's own sizes."""
import os

import numpy as np
import pytest
import torch

import field_reference as FR
from conftest import load_golden, pkg

CUS = (64, 104, 256, 304)
PRECISIONS = ("fp32", "bf16", "bf16x3")


def _walk(P, cus, tile):
    """tiles per workgroup, as the kernels' loop `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)` hands them out"""
    ntiles = -(-P // tile)
    grid = min(ntiles, cus)
    return [len(range(g, ntiles, grid)) for g in range(grid)], ntiles


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("cus", CUS)
def test_planner(cus, precision):
    tile, wave = FR.TILE[precision], FR.WAVE[precision]
    for size in FR.SIZES:
        pl = FR.plan(cus, precision, size)
        P, N, S = pl["P"], pl["N"], pl["S"]
        per_wg, ntiles = _walk(P, cus, tile)
        assert N * S == P and pl["tiles"] == ntiles and len(per_wg) == cus
        assert max(per_wg) == pl["most"] and min(per_wg) == pl["least"]
        assert [g for g, n in enumerate(per_wg) if n == pl["most"]] == list(range(pl["busiest"]))      # the low workgroups get the extra tile
        assert S == 1 or (2 <= S <= 192 and not any(P % s == 0 for s in range(S + 1, 193)))
        assert S > 1 or not any(P % s == 0 for s in range(2, 193))
        if size == "one_past":
            assert (ntiles, pl["most"], pl["least"], pl["busiest"], pl["last_tile_samples"]) == (cus + 1, 2, 1, 1, 1)
        elif size == "two_rounds":
            assert (ntiles, pl["most"], pl["least"], pl["last_tile_samples"], pl["partial_wave"]) == (2 * cus, 2, 2, tile, None)
        else:
            rem = pl["last_tile_samples"]
            assert (ntiles, pl["most"], pl["least"], pl["busiest"]) == (2 * cus + 2, 3, 2, 2)
            assert 0 < rem < tile and rem % wave != 0 and pl["partial_wave"] == rem // wave >= 1      # a partly filled wave, not the first
            assert P == 2 * cus * tile + tile + rem
        sl = FR.ray_slices(N, S, cus, tile)
        assert sl[0][0] == 0 and sl[-1][1] == N and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < (n1 - n0) * S <= cus * tile // 2 for n0, n1 in sl)
        assert all(_walk((n1 - n0) * S, cus, tile)[0].count(1) == len(_walk((n1 - n0) * S, cus, tile)[0]) for n0, n1 in sl)      # one tile each
        if S % tile != 0 and len(sl) > 2:
            assert any((n0 * S) % tile != 0 for n0, _ in sl[1:]), "no slice boundary falls inside a tile"


def test_ragged_remainder():
    assert [FR.ragged_remainder(FR.TILE[p], FR.WAVE[p]) for p in PRECISIONS] == [77, 77, 77]
    assert 77 // 16 == 4 and 77 // 64 == 1 and 77 // 32 == 2      # the fifth / second / third wave holds the 13 left over
    assert FR.ragged_remainder(256, 128) == 129                    # (77 would sit in the first wave of so wide a one)


def test_factor():
    assert FR.factor(32769) == (331, 99) and FR.factor(65536) == (512, 128) and FR.factor(65537) == (65537, 1) and FR.factor(65741) == (389, 169)


def test_slice_and_reassemble_planes():
    """a synthetic save of 3 planes, cut into ray slices saved separately, against direct indexing of the whole"""
    rng = np.random.default_rng(0)
    N, S, widths = 11, 7, (16, 64, 4)
    P = N * S
    vals = [rng.standard_normal((P, w)).astype(np.float32) for w in widths]
    whole = torch.from_numpy(np.concatenate([v.reshape(-1) for v in vals]))
    parts = []
    for n0, n1 in ((0, 4), (4, 5), (5, 11)):
        parts.append(torch.from_numpy(np.concatenate([v[n0 * S:n1 * S].reshape(-1) for v in vals])))
    again = FR.reassemble_planes(parts, widths)
    assert FR.same_bits(again, whole)
    col = 0
    for v, w in zip(vals, widths):
        assert np.array_equal(FR.plane(whole, P, col, w).numpy(), v)
        col += w
    # a plane table column is a float offset of column * P: the second plane of the whole starts at 16 * P
    assert float(whole[16 * P + 5 * 64 + 3]) == float(vals[1][5, 3])


@pytest.mark.parametrize("width", [64, 128, 256])
def test_sign_bit_decoder(width):
    rng = np.random.default_rng(width)
    P = 37
    acts = rng.standard_normal((P, width)).astype(np.float32)
    acts[3, 5] = 0.0
    words = FR.encode_sign_bits(acts > 0)
    assert words.shape == (P, FR.sign_words(width))
    # spot checks of the layout itself: feature 16 t + 4 q + r -> word q * NW + t // 8, bit 4 (t % 8) + r
    nw = max(1, width // 128)
    for f in (0, 5, 17, width - 1):
        t, q, r = f // 16, (f % 16) // 4, f % 4
        for p in (0, P - 1):
            assert ((int(words[p, q * nw + t // 8]) >> (4 * (t % 8) + r)) & 1) == int(acts[p, f] > 0)
    # in a buffer of several planes, at word column 8
    buf = np.concatenate([np.full(8 * P, 0x5A5A5A5A, np.int32), words.reshape(-1), np.full(4 * P, -1, np.int32)])
    got = FR.decode_sign_bits(torch.from_numpy(buf), P, 8, width)
    assert np.array_equal(got.numpy(), acts > 0)


@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_tables_against_layout_header(arch):
    """the restated tables agree with themselves and with the numbers of csrc/sahs_layout.hpp that the tests elsewhere use"""
    rows, stride = FR.act_table(arch)
    assert [r[1] for r in rows] == list(np.cumsum([0] + [r[2] for r in rows[:-1]])) and all(r[1] % 16 == 0 for r in rows)
    assert stride == {"audio": 4752, "nerface": 3792, "nerface_static": 3696}[arch]
    assert FR.act_words(arch, 0) == FR.act_words(arch, 1) + FR.act_words(arch, 2) - 16
    tab, (whole, bd, br) = FR.bits_table(arch)
    assert (bd, br) == {"audio": (48, 96), "nerface": (48, 64), "nerface_static": (0, 64)}[arch] and whole == bd + br
    assert {r[5] for r in rows if r[5]} == set(tab)


@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_tables_against_library(arch):
    lib_path = pkg("_lib").LIB_PATH
    if not os.path.exists(lib_path):
        pytest.skip("the HIP library is not built (%s)" % lib_path)
    ops = pkg("ops")
    assert int(ops._fn("act_words_per_sample", arch)[0]()) == FR.act_words(arch, FR.FIELD_ALL)
    _, (whole, bd, br) = FR.bits_table(arch)
    for part, words in ((0, whole), (1, bd), (2, br)):
        assert int(ops._fn("act_words_part", arch)[0](part)) == FR.act_words(arch, part), (arch, part)
        assert int(ops._fn("bits_words_part", arch)[0](part)) == words, (arch, part)


def _golden_eager(dtype):
    W = pkg("weights")
    from oracle import torch_eager as TE
    g = load_golden("field")
    sd_np = FR.state_dict_np(W, "audio")
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in sd_np.items()}
    f = TE.EagerField(sd)
    with torch.no_grad():
        drv = f.audionet(torch.from_numpy(g["audio"]).to(dtype))
        p36 = f.pose_encoding(torch.from_numpy(g["pose"]).to(dtype))[0]
    x6 = torch.from_numpy(g["x"])
    return g, {lv: FR.eager_field(sd_np, "audio", lv, x6, drv, p36, dtype, chunk=100) for lv in (0, 1)}


def test_eager_float64_against_golden():
    """the float64 wrapper (conditioning precomputed, evaluated in chunks, dx / w / grid tapped) against the reference model's own float64
    run on the golden points (tests/golden/field.npz, hdr weights).  The two are not the same float64 program: the golden run's pose goes
    through the reference's pose_to_euler_trans, which rounds to fp32 on the way, so its conditioning vectors differ from the restatement's
    by up to an fp32 ulp (6e-8 relative) and the outputs by a small multiple of that.  The bound is the floor below which the yardstick
    itself does not tell two results apart: 32 fp32 ulps of the tensor's largest magnitude (conftest.yardstick, eps)."""
    g, out = _golden_eager(torch.float64)
    for name, got in (("hdr_raw_coarse_f64", out[0]["raw"]), ("hdr_raw_fine_f64", out[1]["raw"]), ("hdr_dx_f64", out[0]["dx"]),
                      ("hdr_w_f64", out[0]["w"]), ("hdr_grid_coarse_f64", out[0]["grid"])):
        ref = np.asarray(g[name], np.float64)
        err = float(np.abs(got.numpy() - ref).max()) / float(np.abs(ref).max())
        print("%s: %.2e of scale" % (name, err))
        assert got.dtype == torch.float64 and err <= 32.0 * 2.0 ** -24, (name, err)


def test_comparators_are_sensitive():
    g, out32 = _golden_eager(torch.float32)
    _, out64 = _golden_eager(torch.float64)
    raw32, raw64 = out32[1]["raw"], out64[1]["raw"]
    P = raw32.shape[0]
    # bitwise: one ulp in one sample
    other = raw32.clone()
    assert FR.same_bits(raw32, other)
    other.view(torch.int32)[P - 1, 15] += 1
    assert not FR.same_bits(raw32, other) and FR.first_difference(raw32, other) == (1, (P - 1) * 16 + 15, P - 1)
    nan = torch.full((4, 8), float("nan"))
    assert FR.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())      # why sentinels compare through an int32 view
    with pytest.raises(AssertionError):
        FR.assert_same_bits(raw32, other, "one ulp")
    # the edge-set yardstick on eager fp32 data: passes as it is, fails with either row fault
    tile, cus = 64, 2
    rows = FR.edge_rows(P, cus, tile)
    assert set(rows) == set(range(0, 64)) | set(range(128, 256))      # tiles 0 and 2 (round starts), 2 and 3 (the last two), the last 16
    from conftest import YARDSTICK_LOG
    before = len(YARDSTICK_LOG)
    sig32, sig64 = raw32[:, 15], raw64[:, 15]
    assert not FR.would_fail(sig32, sig32, sig64, rows)
    assert FR.would_fail(FR.swap_last_two(sig32), sig32, sig64, rows)
    assert FR.would_fail(FR.stale_row(sig32, tile), sig32, sig64, rows)
    assert FR.would_fail(FR.swap_last_two(raw32)[:, :15], raw32[:, :15], raw64[:, :15], rows)
    assert not FR.would_fail(FR.stale_row(sig32, 155), sig32, sig64, rows), "row P - 156 is outside the edge set: the fault is not this check's to see"
    assert len(YARDSTICK_LOG) == before


def test_edge_rows():
    rows = FR.edge_rows(2 * 256 * 128 + 128 + 77, 256, 128)
    assert len(rows) == 3 * 128 + 77 and rows[0] == 0 and rows[-1] == 2 * 256 * 128 + 128 + 76
    assert set(range(256 * 128, 257 * 128)) <= set(rows) and 128 not in rows
    assert list(FR.edge_rows(5, 256, 128)) == [0, 1, 2, 3, 4]
