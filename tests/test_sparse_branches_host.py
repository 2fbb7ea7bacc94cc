"""CPU-side checks of the sparse branches' host contract (include/sahs_nerf.h: sahs_model_render_rays_rows_sparse,
sahs_model_render_sparse_workspace_bytes; ops.sparse_branches): sizes, refusals that happen before any kernel runs, the selector."""
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


def _call(L, model=0, precision=0, ws=A, ws_bytes=256 + 128 * 1040, rows=A, row_ld=36, nf=64):
    return L.sahs_model_render_rays_rows_sparse(model, A, A, precision, 1, A, 8, 64, nf, 0, 0, None, None, None, None, None, A, A, A, A, rows, row_ld,
                                                None, None, None, ws, ws_bytes, None)


def test_refusals_before_any_launch():
    L = pkg("_lib").lib()
    assert _call(L, model=3) == 3
    assert _call(L, rows=None) == 1 and _call(L, row_ld=35) == 1
    assert _call(L, ws=None) == 1 and _call(L, ws=A + 4) == 1
    assert _call(L, nf=193) == 1
    assert _call(L, ws_bytes=256 + 128 * 1040 - 1) == 5
    assert b"less than one tile" in L.sahs_last_error()
    assert _call(L, ws_bytes=0) == 5
    # any other precision is the dense entry point's business: its own refusal (bf16 of the NeRFaceModel needs the xw workspace)
    assert _call(L, model=1, precision=1) == L.sahs_model_render_rays_rows(1, A, A, 1, 1, A, 8, 64, 64, 0, 0, None, None, None, None, None, A, A, A, A, A,
                                                                            36, None, None, None, None) != 0


def test_selector_is_validated():
    ops, lib = pkg("ops"), pkg("_lib")
    assert ops.sparse_branches() is True
    was = ops.sparse_workspace_bytes()
    try:
        assert ops.sparse_branches(False) is False and ops.sparse_branches() is False
        assert ops.sparse_branches(True, workspace_bytes=1 << 20) is True and ops.sparse_workspace_bytes() == 1 << 20
        for bad in ("yes", 2, 1.0, []):
            with pytest.raises(lib.SahsError):
                ops.sparse_branches(bad)
        for bad in (0, -1, 1.5, True, "8G"):
            with pytest.raises(lib.SahsError):
                ops.sparse_branches(workspace_bytes=bad)
        assert ops.sparse_branches() is True and ops.sparse_workspace_bytes() == 1 << 20
    finally:
        ops.sparse_branches(True, workspace_bytes=was)
