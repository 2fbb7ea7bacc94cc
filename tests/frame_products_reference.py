"""The statement of the frame products (ops.frame_products; include/sahs_nerf.h: sahs_frame_products) in numpy, and the inputs and the
byte rule their tests share.  It imports nothing from the package.

* image and disparity are DEFINED in fp32 -- one product, resp. one subtraction, one division and one product, each correctly
  rounded -- so their statement is those numpy float32 operations and a byte either matches or does not.
* seg is numpy's argmax (the first maximum wins, a NaN counts as the maximum) through the colour table.
* normals are stated in float64 from the fp32 inputs, for rectangular maps too: the column index enters x with cx * W, the row index
  enters y with cy * H.  Where the background weight exceeds 0.22 the value is exactly 1 (255 after the scale): (1 - m) * 1 + m.
* NaN rule: a NaN that reaches a byte conversion is 0.  numpy's min and max propagate NaN as torch's do, so a frame whose disparity holds
  a NaN, or is constant (0 / 0), has an all-zero disparity plane.
``fault`` plants one single fault ("swap": cross-product operands swapped; "no_white": the 0.22 rule dropped; "reciprocal": the division
replaced by a product with the reciprocal) so that a test can show its bound catches it."""
import numpy as np

SEG_COLOURS = np.array([(0, 0, 0), (0, 0, 204), (0, 153, 76), (0, 204, 204), (255, 51, 51), (255, 255, 0), (0, 51, 102), (0, 204, 102),
                        (0, 255, 255), (204, 0, 0), (51, 153, 255), (0, 204, 0)], np.uint8)
SHAPES = [(1, 1), (2, 2), (3, 3), (24, 24), (31, 33), (32, 32), (33, 31), (65, 64), (70, 33)]      # around the 32-pixel tile edge in each axis
WHITE = np.float32(0.22)


def to_u8(v):
    """Truncation to a byte of values already clamped to [0, 255]; NaN -> 0."""
    v = np.asarray(v)
    out = np.zeros(v.shape, np.uint8)
    ok = ~np.isnan(v)
    out[ok] = v[ok].astype(np.int64).astype(np.uint8)
    return out


def image(rgb):
    """(.., >= 3) float32 -> (.., 3) uint8: clamp(x, 0, 1) * 255 in fp32, truncated."""
    x = np.asarray(rgb, np.float32)[..., :3]
    return to_u8(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255))      # (np.clip propagates NaN)


def seg(scores):
    """(.., 12) float32 class scores -> (.., 3) uint8 colours."""
    return SEG_COLOURS[np.argmax(np.asarray(scores), axis=-1)]


def disparity(t, fault=None):
    """(H, W) float32, ONE frame -> (H, W) uint8."""
    t = np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        mn, mx = t.min(), t.max()      # NaN if any
        v = (t - mn) * (np.float32(1) / (mx - mn)) if fault == "reciprocal" else (t - mn) / (mx - mn)
        assert v.dtype == np.float32
        return to_u8(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255))


def normals(disp, focal, w_bg=None, clean=True, central_difference=False, fault=None):
    """(H, W) float32, ONE frame -> (H - d, W - d, 3) float64, in [0, 255] where finite (not clamped); an empty plane for H <= d or W <= d."""
    t = np.asarray(disp, np.float64)
    H, W = t.shape
    d = 2 if central_difference else 1
    if H <= d or W <= d:
        return np.zeros((max(H - d, 0), max(W - d, 0), 3))
    fx, fy, cx, cy = (float(v) for v in np.asarray(focal))
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    pts = np.stack([((col - cx * W) * t) / fx, -((row - cy * H) * t) / fy, t], -1)
    drow = (pts[d:] - pts[:-d])[:, :-d]      # evaluation.normal_map's dx
    dcol = (pts[:, d:] - pts[:, :-d])[:-d]      # its dy
    with np.errstate(all="ignore"):
        n = np.cross(drow, dcol) if fault == "swap" else np.cross(dcol, drow)
        n = n / np.sqrt(np.sum(n * n, -1, keepdims=True))
        n = n * 0.5 + 0.5
        if clean and w_bg is not None:
            w = np.asarray(w_bg, np.float32)[:-d, :-d, None]
            m = w.astype(np.float64)
            n = (1.0 - m) * n + m
            if fault != "no_white":
                n = np.where(white_mask(w_bg, central_difference)[..., None], 1.0, n)      # (1 - m) * 1 + m, exactly
        return n * 255.0


def white_mask(w_bg, central_difference=False):
    """(H - d, W - d) bool: the pixels the 0.22 rule whitens."""
    d = 2 if central_difference else 1
    return np.asarray(w_bg, np.float32)[:-d, :-d] > WHITE


def byte_bounds(r64, tol):
    """The bytes that truncations of [r64 - tol, r64 + tol] can give: (lowest, highest), NaN -> (0, 0)."""
    r64 = np.asarray(r64, np.float64)
    return to_u8(np.clip(r64 - tol, 0.0, 255.0)), to_u8(np.clip(r64 + tol, 0.0, 255.0))


# ---- the inputs the tests share ----
def focal_for(H, W):
    return np.array([1200.0 * W / 512, 1150.0 * H / 512, 0.48, 0.52], np.float32)


def special_values():
    """Image values at which the cast can go wrong: outside [0, 1], the ends, -0.0, and k / 255 with its two fp32 neighbours."""
    vals = [-0.5, 1.5, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))]
    for k in (1, 2, 3, 51, 127, 128, 204, 254):
        x = np.float32(k) / np.float32(255)
        vals += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))]
    return np.array(vals, np.float32)


def make_rgb(H, W, seed, nan=False):
    """(H, W, 15) float32 [rgb3 | seg12]: colours in (-0.2, 1.2) with special_values() planted from the LAST pixel backwards (as many
    as fit); scores with an exact two-way tie (pixel 0: the first must win), a row of equal scores (pixel 1) and, with ``nan``, a
    NaN score (pixel 2, or 0), a NaN before a larger score, and a NaN colour."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.uniform(-0.2, 1.2, (H * W, 3)), rng.standard_normal((H * W, 12))], 1).astype(np.float32)
    sp = special_values()
    k = min(len(sp), H * W * 3)
    flat = a[:, :3].copy().reshape(-1)
    flat[::-1][:k] = sp[:k]
    a[:, :3] = flat.reshape(-1, 3)
    a[0, 3:] = [0.1, 2.0, -1.0, 2.0, 0.5, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    if H * W > 1:
        a[1, 3:] = 0.25
    if nan:
        p = 2 if H * W > 2 else 0
        a[p, 3:] = [0.0, 1.0, np.nan, 5.0, np.nan, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0]
        a[H * W // 2, 1] = np.nan
    return a.reshape(H, W, 15)


def make_disp(H, W, seed):
    return (1.0 / np.random.default_rng(seed + 1000).uniform(0.5, 1.0, (H, W))).astype(np.float32)


def make_disp_on_byte_edges(H, W, seed):
    """A map whose values sit on the byte boundaries of its own range, min + (max - min) k / 255: there the quotient's last bit decides
    the byte, and a product with the reciprocal gives other bytes than the division does (the host test shows it)."""
    rng = np.random.default_rng(seed + 3000)
    mn, mx = np.float32(rng.uniform(0.9, 1.1)), np.float32(rng.uniform(1.8, 2.2))
    k = rng.integers(0, 256, (H, W)).astype(np.float32)
    t = (mn + (mx - mn) * (k / np.float32(255))).astype(np.float32)
    t.flat[0], t.flat[-1] = mn, mx
    return t


def make_w_bg(H, W, seed):
    """U(0, 0.3): about 27 % of the pixels take the white branch, the rest exercise the blend."""
    return np.random.default_rng(seed + 2000).uniform(0.0, 0.3, (H, W)).astype(np.float32)
