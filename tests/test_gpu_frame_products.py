"""ops.frame_products on the GPU (include/sahs_nerf.h: sahs_frame_products): image, mask and disparity bytes exactly as evaluation.py's torch
functions give them on the CPU (in the NaN cases, which torch leaves undefined: as tests/frame_products_reference.py states them); the
normal map against the float64 statement, allowed 4 e where e is the error of the torch functions' own fp32 arithmetic on the same
input (the factor 4: a different but legitimate order of the same fp32 operations), and its bytes the truncations of that interval.
The shapes put one pixel below, at and above the kernel's 32-pixel tile edge in each axis, include an empty and a 1 x 1 normal plane,
and odd-sized byte planes in a batch (frame 1 starts off a dword boundary).  On the CPU e came out at 1e-5 .. 5e-4 for these shapes
(it grows with H: 5e-3 at 512 x 512, which is why the shapes stay small); each test prints the e it measured and the op's own deviation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import frame_products_reference as R
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(H, W, 1) for H, W in R.SHAPES] + [(3, 3, 2), (33, 31, 2)]
FLAGS = [(True, False), (True, True), (False, False), (False, True)]      # (clean, central_difference)
AMBIGUOUS_CAP = 0.02      # share of non-white entries whose interval holds two bytes: a cap, not a measurement


def torch_normal_map(depthmap, focal, weights=None, clean=True, central_difference=False):
    """evaluation.normal_map operation for operation in torch fp32 on the CPU, for rectangular (H, W) maps too: the column index enters
    x with cx * W, the row index y with cy * H (test_square_torch_statement_is_evaluation_normal_map: the same bits on square maps)."""
    H, W = depthmap.shape
    cx, cy, fx, fy = focal[2] * W, focal[3] * H, focal[0], focal[1]
    ii, jj = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy")
    pts = torch.stack([((ii - cx) * depthmap) / fx, -((jj - cy) * depthmap) / fy, depthmap], dim=-1)
    d = 2 if central_difference else 1
    dx = pts[d:, :, :] - pts[:-d, :, :]
    dy = pts[:, d:, :] - pts[:, :-d, :]
    n = torch.cross(dy[:-d, :, :], dx[:, :-d, :], dim=2)
    n = n / torch.sqrt(torch.sum(n * n, 2, keepdim=True))
    n = n * 0.5 + 0.5
    if clean and weights is not None:
        m = weights[..., None].expand(-1, -1, 3)[:-d, :-d]
        n = torch.where(m > 0.22, torch.ones_like(n), n)
        n = (1 - m) * n + m * torch.ones_like(n)
    return n * 255


@functools.lru_cache(maxsize=None)
def inputs(H, W, B):
    """Frame b of a case has seed 10 b + 3: (rgb (B, H, W, 15), disp, w_bg (B, H, W), focal) in numpy."""
    seeds = [10 * b + 3 for b in range(B)]
    return (np.stack([R.make_rgb(H, W, s) for s in seeds]), np.stack([R.make_disp(H, W, s) for s in seeds]),
            np.stack([R.make_w_bg(H, W, s) for s in seeds]), R.focal_for(H, W))


@functools.lru_cache(maxsize=None)
def references(H, W, B):
    """Computed once per case and left unchanged: the torch functions' bytes on the CPU, and per (clean, central) the float64 normals,
    the white mask and e."""
    E = pkg("evaluation")
    rgb, disp, w_bg, focal = inputs(H, W, B)
    ref = dict(image=np.stack([E.cast_to_image(torch.from_numpy(f[..., :3])) for f in rgb]),
               seg=np.stack([E.cast_to_image(E.label2color(torch.from_numpy(f[..., 3:]))) for f in rgb]),
               disparity=np.stack([E.cast_to_disparity_image(torch.from_numpy(f)) for f in disp]) if H * W > 1 else None)
    for clean, central in FLAGS:
        d = 2 if central else 1
        r64 = np.stack([R.normals(disp[b], focal, w_bg[b], clean, central) for b in range(B)])
        white = np.stack([R.white_mask(w_bg[b], central) for b in range(B)]) if clean and H > d and W > d else np.zeros(r64.shape[:3], bool)
        if H > d and W > d:
            t32 = np.stack([torch_normal_map(torch.from_numpy(disp[b]), focal, torch.from_numpy(w_bg[b]), clean, central).numpy() for b in range(B)])
            e = float(np.abs(t32 - r64)[~white].max()) if (~white).any() else 0.0
        else:
            e = 0.0
        ref[clean, central] = (r64, white, e)
    return ref


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_normals(what, f32, u8, r64, white, e):
    """f32, u8: the op's planes (numpy); r64, white, e: references().  Returns (e, the op's own deviation)."""
    assert f32.shape == r64.shape and u8.shape == r64.shape and f32.dtype == np.float32 and u8.dtype == np.uint8
    if r64.size == 0:
        return e, 0.0
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(f32), nan) and np.all(u8[nan] == 0), what      # the NaN rule
    assert np.all(f32[white] == 255.0) and np.all(u8[white] == 255), what      # white pixels: exactly 255
    rest = ~white[..., None] & ~nan
    dev = float(np.abs(f32.astype(np.float64) - r64)[rest].max()) if rest.any() else 0.0
    print("%s: e = %.3e, op deviation = %.3e" % (what, e, dev))
    assert dev <= 4 * e, (what, dev, e)
    lo, hi = R.byte_bounds(r64, 4 * e)
    assert np.all((u8 >= lo) & (u8 <= hi)), (what, int(((u8 < lo) | (u8 > hi)).sum()))
    if rest.any():
        share = float((hi > lo)[rest].mean())
        assert share <= AMBIGUOUS_CAP, (what, share)      # over the cap by the reference alone: change the input, not the cap
    return e, dev


def test_square_torch_statement_is_evaluation_normal_map():
    E = pkg("evaluation")
    for H in (3, 24, 32):
        _, disp, w_bg, focal = inputs(H, H, 1)
        for clean, central in FLAGS:
            a = torch_normal_map(torch.from_numpy(disp[0]), focal, torch.from_numpy(w_bg[0]), clean, central)
            b = E.normal_map(torch.from_numpy(disp[0]), focal, torch.from_numpy(w_bg[0]), clean, central)
            assert torch.equal(a, b)


@pytest.mark.parametrize("H,W,B", CASES)
def test_frame_products(H, W, B):
    ops = pkg("ops")
    rgb, disp, w_bg, focal = inputs(H, W, B)
    ref = references(H, W, B)
    squeeze = (lambda a: a[0]) if B == 1 else (lambda a: a)      # B = 1 runs without the batch dimension
    render = gpu(squeeze(rgb))      # the contiguous (H W, 15) render layout
    layouts = dict(render=render, view3=render[..., :3], c3=render[..., :3].contiguous())
    t_disp, t_wbg = gpu(squeeze(disp)), gpu(squeeze(w_bg))
    lead = () if B == 1 else (B,)
    for name, t in layouts.items():
        for clean, central in FLAGS:
            what = "%dx%d B=%d %s clean=%d central=%d" % (H, W, B, name, clean, central)
            out = ops.frame_products(t, t_disp, t_wbg, focal, clean=clean, central_difference=central, float_normals=True)
            assert set(out) == {"image", "disparity", "normals", "normals_f32"} | ({"seg"} if name == "render" else set()), what
            got = {k: v.cpu().numpy().reshape((B,) + tuple(v.shape[len(lead):])) for k, v in out.items()}
            assert all(v.shape[:len(lead)] == lead and v.is_contiguous() for v in out.values())
            assert np.array_equal(got["image"], ref["image"]), what
            if name == "render":
                assert np.array_equal(got["seg"], ref["seg"]), what
            if ref["disparity"] is not None:
                assert np.array_equal(got["disparity"], ref["disparity"]), what
            else:
                assert got["disparity"].max() == 0      # one pixel: a constant map
            r64, white, e = ref[clean, central]
            check_normals(what, got["normals_f32"], got["normals"], r64, white, e)
            if B > 1 and name == "render":      # a batch gives the bits of its single calls, in every plane
                for b in range(B):
                    one = ops.frame_products(t[b], t_disp[b], t_wbg[b], focal, clean=clean, central_difference=central, float_normals=True)
                    for k in out:
                        assert torch.equal(out[k][b].view(torch.uint8), one[k].view(torch.uint8)), (what, b, k)
    only = ops.frame_products(layouts["c3"])      # no disp: the image alone
    assert set(only) == {"image"} and np.array_equal(only["image"].cpu().numpy().reshape(ref["image"].shape), ref["image"])
    no_focal = ops.frame_products(layouts["render"], t_disp)
    assert set(no_focal) == {"image", "seg", "disparity"}


def test_reference_vectors():
    """The 24 x 24 case of the reference's own vectors (tests/golden/post.npz), at the tolerance the host test holds evaluation.py to."""
    ops = pkg("ops")
    g = load_golden("post")
    rgb = gpu(np.concatenate([np.zeros((24, 24, 3), np.float32), g["seg"]], -1))
    disp, w_bg = gpu(g["disp"]), gpu(g["w_bg"])
    for key, kw in (("normals_clean", dict(w_bg=w_bg, clean=True)), ("normals_raw", dict(w_bg=None, clean=False)),
                    ("normals_central", dict(w_bg=w_bg, clean=True, central_difference=True))):
        out = ops.frame_products(rgb, disp, focal=g["focal"], float_normals=True, **kw)
        n = out["normals_f32"].cpu().numpy()
        assert n.shape == g[key].shape and np.abs(n - g[key]).max() <= 2e-3, (key, np.abs(n - g[key]).max())
        assert np.array_equal(out["seg"].cpu().numpy(), R.image(g["seg_color"]))
        assert np.array_equal(out["disparity"].cpu().numpy(), g["disp_img"])


@pytest.mark.parametrize("H,W", R.SHAPES[1:])
def test_disparity_edges(H, W):
    """Values on the byte boundaries of the map's own range (a reciprocal in place of the division shows there), a constant map, and the
    maximum and the minimum each in the last row and column of the last tile."""
    ops, E = pkg("ops"), pkg("evaluation")
    rgb = gpu(np.zeros((H, W, 3), np.float32))
    maps = [R.make_disp_on_byte_edges(H, W, 5)]
    for sign in (1.0, -1.0):
        m = R.make_disp(H, W, 6)
        m[H - 1, W - 1] = 1.5 + sign * 2.0
        maps.append(m)
    for m in maps:
        got = ops.frame_products(rgb, gpu(m))["disparity"].cpu().numpy()
        assert np.array_equal(got, E.cast_to_disparity_image(torch.from_numpy(m)))
    assert ops.frame_products(rgb, gpu(np.full((H, W), 0.75, np.float32)))["disparity"].max().item() == 0


@pytest.mark.parametrize("H,W", [(3, 3), (33, 31), (70, 33)])
def test_nan_rule(H, W):
    """What torch leaves undefined, against the statement: a NaN that reaches a byte is 0; a NaN score is the arg-max; one NaN in frame
    0's disparity zeroes that frame's plane and leaves frame 1's as its single call gives it."""
    ops = pkg("ops")
    rgb = np.stack([R.make_rgb(H, W, 7, nan=True), R.make_rgb(H, W, 8, nan=True)])
    disp = np.stack([R.make_disp(H, W, 7), R.make_disp(H, W, 8)])
    disp[0, H - 1, W // 2] = np.nan
    w_bg, focal = np.stack([R.make_w_bg(H, W, 7), R.make_w_bg(H, W, 8)]), R.focal_for(H, W)
    w_bg[0, H - 2, W // 2] = 0.1      # the pixel whose normal reads the NaN is not whitened: the NaN reaches its bytes
    out = {k: v.cpu().numpy() for k, v in ops.frame_products(gpu(rgb), gpu(disp), gpu(w_bg), focal, float_normals=True).items()}
    assert np.array_equal(out["image"], R.image(rgb)) and out["image"].reshape(2, -1, 3)[0, H * W // 2, 1] == 0
    assert np.array_equal(out["seg"], R.seg(rgb[..., 3:]))
    assert out["disparity"][0].max() == 0 and np.array_equal(out["disparity"][1], R.disparity(disp[1])) and out["disparity"][1].max() == 255
    single = ops.frame_products(gpu(rgb[1]), gpu(disp[1]), gpu(w_bg[1]), focal, float_normals=True)
    for k in out:
        assert np.array_equal(out[k][1].view(np.uint8), single[k].cpu().numpy().view(np.uint8)), k
    r64 = R.normals(disp[0], focal, w_bg[0])
    nan = np.isnan(r64)
    assert nan.any() and np.array_equal(np.isnan(out["normals_f32"][0]), nan) and np.all(out["normals"][0][nan] == 0)


def test_argument_errors():
    ops, _lib = pkg("ops"), pkg("_lib")
    f = torch.zeros(8, 8, 15, device=DEV)
    d = torch.ones(8, 8, device=DEV)
    with pytest.raises(_lib.SahsError, match="C = 12 channels, must be 3"):
        ops.frame_products(f[..., :12].contiguous())
    with pytest.raises(_lib.SahsError, match="normals asked for without intrinsics"):
        ops.frame_products(f, d, float_normals=True)
    with pytest.raises(_lib.SahsError, match="normals asked for without disp"):
        ops.frame_products(f, focal=R.focal_for(8, 8), float_normals=True)
    with pytest.raises(_lib.SahsError, match="must be a GPU tensor"):
        ops.frame_products(f.cpu())
    with pytest.raises(_lib.SahsError, match="must be a GPU tensor"):
        ops.frame_products(f, d.cpu())
    with pytest.raises(_lib.SahsError, match="needs rgb's frames and pixels"):
        ops.frame_products(f, d[:4])
    # seg with C = 3 cannot be asked for through ops.frame_products (the key follows C): the C side's refusal, called directly
    L = _lib.lib()
    c3, seg = f[..., :3].contiguous(), torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    code = L.sahs_frame_products(ops._p(c3), 3, (ctypes.c_long * 3)(*c3[None].stride()[:3]), None, None, None, 1, 8, 8, 1, 0, None, ops._p(seg),
                                 None, None, None, None, 0, None)
    assert code == 1 and "seg asked for with C = 3" in L.sahs_last_error().decode()
    assert L.sahs_frame_products(None, 3, None, None, None, None, 0, 8, 8, 1, 0, None, None, None, None, None, None, 0, None) == 0      # B = 0
    assert L.sahs_frame_products_workspace_bytes(3, 33, 65) == 3 * 2 * 3 * 16 and L.sahs_frame_products_workspace_bytes(1, 0, 8) == 0


@pytest.mark.parametrize("B", [1, 3])
def test_two_launches_whatever_the_batch(B):
    from torch.profiler import ProfilerActivity, profile
    ops = pkg("ops")
    rgb, disp, w_bg = (torch.rand(B, 40, 40, 15, device=DEV), torch.rand(B, 40, 40, device=DEV) + 0.5, torch.rand(B, 40, 40, device=DEV) * 0.3)
    call = lambda: ops.frame_products(rgb, disp, w_bg, R.focal_for(40, 40), float_normals=True)      # noqa: E731
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "frame_products" in e.name]
    assert len(names) == 2 and "tile_kernel" in names[0] and "disparity_kernel" in names[1], names
