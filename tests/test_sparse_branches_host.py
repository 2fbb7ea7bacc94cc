"""CPU-side checks of the sparse branches' host contract (include/sahs_nerf.h: sahs_model_render_rays_rows_sparse,
sahs_model_render_sparse_workspace_bytes, sahs_model_render_sparse_fused_workspace_bytes; ops.sparse_branches): sizes, refusals that happen
before any kernel runs, the selector.  Without a device the library counts 256 compute units, so the ring need is a fixed number here."""
import pytest

from conftest import pkg

A = 1 << 20      # a fabricated, 16-byte aligned device address: never dereferenced (every call here is refused before a launch)


def test_workspace_bytes():
    L = pkg("_lib").lib()
    # 256 bytes of head + per record a 16-byte header and 16 k-blocks x 16 floats of feat; slots in whole 128-record tiles
    for m in (0, 1, 2):
        assert [L.sahs_model_render_sparse_workspace_bytes(m, n) for n in (0, 1, 128, 129, 1 << 20)] == \
            [256, 256 + 128 * 1040, 256 + 128 * 1040, 256 + 256 * 1040, 256 + (1 << 20) * 1040]
    assert L.sahs_model_render_sparse_workspace_bytes(3, 128) == 0 and L.sahs_model_render_sparse_workspace_bytes(0, -1) == 0


def _call(L, model=0, precision=0, ws=A, ws_bytes=256 + 128 * 1040, rows=A, row_ld=36, nf=64, N=1):
    return L.sahs_model_render_rays_rows_sparse(model, A, A, precision, N, A, 8, 64, nf, 0, 0, None, None, None, None, None, A, A, A, A, rows, row_ld,
                                                None, None, None, ws, ws_bytes, None)


def test_refusals_before_any_launch():
    L = pkg("_lib").lib()
    assert _call(L, model=3) == 3
    assert _call(L, rows=None) == 1 and _call(L, row_ld=35) == 1
    assert _call(L, ws=None) == 1 and _call(L, ws=A + 4) == 1
    assert _call(L, nf=193) == 1
    assert _call(L, ws_bytes=256 + 128 * 1040 - 1) == 5      # one ray of 64 + 64 samples: one tile, 128 slots
    assert b"sahs_model_render_sparse_fused_workspace_bytes" in L.sahs_last_error() and b"holds 0 record slots" in L.sahs_last_error()
    assert _call(L, ws_bytes=0) == 5
    # any other precision is the dense entry point's business: its own refusal (bf16 of the NeRFaceModel needs the xw workspace)
    assert _call(L, model=1, precision=1) == L.sahs_model_render_rays_rows(1, A, A, 1, 1, A, 8, 64, 64, 0, 0, None, None, None, None, None, A, A, A, A, A,
                                                                            36, None, None, None, None) != 0


def test_rings_of_both_passes_must_fit():
    """300 rays of 64 + 64 samples; without a device the library counts 256 compute units, so the fine pass is 300 tiles on 256 workgroups:
    44 rings of 256 slots and 212 of 128"""
    L = pkg("_lib").lib()
    need = L.sahs_model_render_sparse_fused_workspace_bytes(0, 300 * 128)
    assert need == 256 + 38400 * 1040 and 38400 == 256 * 128 + 44 * 128
    for short in (need - 128 * 1040, L.sahs_model_render_sparse_fused_workspace_bytes(0, 300 * 64)):      # one tile short; the coarse pass's only
        assert short < need
        assert _call(L, N=300, ws_bytes=short) == 5
        msg = L.sahs_last_error()
        assert b"sahs_model_render_sparse_fused_workspace_bytes" in msg and b"need 38400" in msg and b"holds %d record slots" % ((short - 256) // 1040) in msg


def test_ring_need_never_shrinks_as_the_pass_grows():
    """what lets one workspace, sized for the fine pass, serve the coarse pass too (ops.render_rays_rows)"""
    L = pkg("_lib").lib()
    counts = sorted(set(list(range(0, 3 * 256 * 128 + 1024, 64)) + [(1 << k) + d for k in range(7, 31) for d in (-1, 0, 1) if (1 << k) + d <= 1 << 30]))
    need = [L.sahs_model_render_sparse_fused_workspace_bytes(0, n) for n in counts]
    assert all(a <= b for a, b in zip(need, need[1:])) and need[0] == 256 and need[-1] == 256 + 256 * 512 * 1040


def test_pass_of_more_than_2_30_samples():
    L = pkg("_lib").lib()
    N = ((1 << 30) + 128) // 128
    assert N * (64 + 64) == (1 << 30) + 128
    assert _call(L, N=N, ws_bytes=1 << 40) == 5
    msg = L.sahs_last_error()
    assert b"more than 2^30" in msg and b"sample index as an int" in msg and b"sahs_model_render_sparse_fused_workspace_bytes" in msg
    assert _call(L, N=N - 1, nf=0, ws_bytes=256 + 256 * 512 * 1040 - 128 * 1040) == 5 and b"need 131072" in L.sahs_last_error()      # (2^29 samples: the plain refusal)


def test_selector_is_validated():
    ops, lib = pkg("ops"), pkg("_lib")
    assert ops.sparse_branches() is True
    try:
        assert ops.sparse_branches(False) is False and ops.sparse_branches() is False
        assert ops.sparse_branches(True) is True
        for bad in ("yes", 2, 1.0, []):
            with pytest.raises(lib.SahsError):
                ops.sparse_branches(bad)
        with pytest.raises(TypeError):      # the record workspace is no longer an option: a render sizes it for its pass
            ops.sparse_branches(workspace_bytes=1)
        assert ops.sparse_branches() is True and not hasattr(ops, "sparse_workspace_bytes")
    finally:
        ops.sparse_branches(True)
