"""sahs_frame_products' argument validation (include/sahs_nerf.h), which needs no GPU: every refusal comes before any HIP call and
names what it refuses."""
import ctypes

import pytest

from conftest import pkg

T = 32      # SAHS_FRAME_PRODUCTS_TILE


def call(L, C=15, rgb=64, strides=(0, 120, 15), disp=64, w_bg=64, intr=(30.0, 30.0, 0.5, 0.5), B=1, H=8, W=8, image=64, seg=None, nu8=None,
         nf32=None, disparity=None, work=None, work_bytes=0):
    """Pointers are made-up addresses: a refused call never reads them."""
    s = (ctypes.c_long * 3)(*strides) if strides is not None else None
    i = (ctypes.c_float * 4)(*intr) if intr is not None else None
    return L.sahs_frame_products(rgb, C, s, disp, w_bg, i, B, H, W, 1, 0, image, seg, nu8, nf32, disparity, work, work_bytes, None)


def test_workspace_query():
    L = pkg("_lib").lib()
    assert L.sahs_frame_products_workspace_bytes(1, 1, 1) == 16
    assert L.sahs_frame_products_workspace_bytes(3, T + 1, 2 * T) == 3 * 2 * 2 * 16
    for bad in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 32769, 8), (1 << 40, 64, 64)):
        assert L.sahs_frame_products_workspace_bytes(*bad) == 0, bad


@pytest.mark.parametrize("kw,text", [
    (dict(C=12), "C = 12 channels, must be 3"), (dict(H=0), "needs 1 <= H, W <= 32768"), (dict(W=40000), "needs 1 <= H, W <= 32768"),
    (dict(B=-1), "B = -1 frames"), (dict(C=3, seg=64), "seg asked for with C = 3"), (dict(nu8=64, intr=None), "normals asked for without intrinsics"),
    (dict(nf32=64, disp=None), "normals asked for without disp"), (dict(disparity=64, disp=None), "disparity asked for without disp"),
    (dict(rgb=None), "null rgb"), (dict(strides=None), "null stride_rgb"), (dict(strides=(0, -120, 15)), "stride 1 is negative"),
    (dict(intr=(0.0, 30.0, 0.5, 0.5), nu8=64), "fx = 0"), (dict(rgb=66), "aligned to their 4-byte elements"),
    (dict(disparity=64), "null pointer for workspace"), (dict(disparity=64, work=72), "workspace must be 16-byte aligned"),
    (dict(disparity=64, work=64, work_bytes=15), "workspace of 15 bytes, needs 16")])
def test_refusals_name_what_they_refuse(kw, text):
    L = pkg("_lib").lib()
    code, msg = call(L, **kw), L.sahs_last_error().decode()
    assert code == 1 and msg.startswith("sahs_frame_products:") and text in msg, (kw, code, msg)


def test_nothing_to_do_succeeds_without_a_launch():
    L = pkg("_lib").lib()
    assert call(L, B=0, rgb=None, strides=None, image=None) == 0      # B = 0
    assert call(L, image=None) == 0      # no plane asked for
    assert call(L, image=None, H=1, W=1, nu8=64, nf32=64) == 0      # only an empty normal plane
