"""Shared references for the fused spectral norm (tests/test_spectral_norm_host.py, tests/test_gpu_spectral_norm.py):

* ``compute_weight64`` / ``backward64``: float64 restatements of torch's ``SpectralNorm.compute_weight`` (dim 0, one power iteration or
  none) and of the backward the kernel implements, dW = G / sigma - (sum(G o W) / sigma^2) u v^T;
* ``torch_spectral_norm``: torch's OWN ``SpectralNorm.compute_weight`` and its autograd backward on a holder module, in whatever dtype
  and on whatever device the inputs have -- the source of E_torch32 and, in float64, what the restatements are checked against;
* the op-level cases (seeded W = 0.05 randn, unit u and v, G = randn), the same tensors for every caller;
* the bf16 rule: ``bf16_of_float64`` rounds float64 to bfloat16 ONCE (torch's own cast goes through float32), ``bf16_rule`` counts the
  elements that differ from it and measures the largest difference in bf16 ulps.
"""
import functools

import numpy as np
import torch
from torch.nn.utils.spectral_norm import SpectralNorm

EPS = 1e-12
FLOOR = 2.0 ** -21      # the project's floor beside 4 x torch's own fp32 error (tests/test_gpu_spade_backward.py)
# name -> (h, w, offset in floats of W / out / grad from a 16-byte boundary on the GPU).  1 x 1: dW is analytically 0; 1 x 7 and 5 x 1:
# one row, one column; 3 x 5: fewer rows than waves; 64 x 576 and 256 x 2304: the smallest and the largest matrix of Generator (16-byte
# path, w % 8 == 0); 65 x 577 and 130 x 1153: odd sizes past one and several 256-column tiles (element-by-element path); the last: the
# 16-byte shape pushed off alignment.
CASES = {"1x1": (1, 1, 0), "1x7": (1, 7, 0), "5x1": (5, 1, 0), "3x5": (3, 5, 0), "64x576": (64, 576, 0), "65x577": (65, 577, 0),
         "130x1153": (130, 1153, 0), "256x2304": (256, 2304, 0), "64x576_unaligned": (64, 576, 1)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> float32 CPU tensors W (h, w), u (h), v (w), G (h, w)."""
    h, w, _ = CASES[name]
    gen = torch.Generator().manual_seed(4000 + sorted(CASES).index(name))
    W = 0.05 * torch.randn(h, w, generator=gen)
    u, v = (torch.nn.functional.normalize(torch.randn(n, generator=gen), dim=0) for n in (h, w))
    return W, u, v, torch.randn(h, w, generator=gen)


def small_cases(n):
    """n small jobs of mixed shapes (the split of a list into calls of 32) -> [(W, u, v, G)]."""
    gen = torch.Generator().manual_seed(77)
    out = []
    for k in range(n):
        h, w = 2 + k % 5, 3 + k % 7
        out.append((0.05 * torch.randn(h, w, generator=gen), torch.nn.functional.normalize(torch.randn(h, generator=gen), dim=0),
                    torch.nn.functional.normalize(torch.randn(w, generator=gen), dim=0), torch.randn(h, w, generator=gen)))
    return out


def compute_weight64(W, u, v, training, eps=EPS):
    """-> (out, u, v, sigma) in float64 on the CPU; u, v: after the power iteration when ``training``, as given otherwise."""
    W, u, v = (t.detach().double().cpu() for t in (W, u, v))
    if training:
        t = W.t() @ u
        v = t / max(float(t.norm()), eps)
        s = W @ v
        u = s / max(float(s.norm()), eps)
    sigma = torch.dot(u, W @ v)
    return W / sigma, u, v, sigma


def backward64(W, u, v, sigma, G):
    """dW for the u, v, sigma that formed the output (compute_weight64's), float64."""
    W, u, v, G = (t.detach().double().cpu() for t in (W, u, v, G))
    sigma = float(sigma)
    return G / sigma - float((G * W).sum()) / sigma ** 2 * torch.outer(u, v)


def torch_spectral_norm(W, u, v, training, G=None, eps=EPS):
    """torch's SpectralNorm.compute_weight on a holder of clones of W, u, v (their dtype, their device)
    -> (out, u, v, sigma, dW or None): u, v as the call left them, sigma = u . (W v) recomputed with torch's ops as the call forms it,
    dW from autograd when G is given."""
    holder = torch.nn.Module()
    holder.weight_orig = torch.nn.Parameter(W.detach().clone())
    holder.register_buffer("weight_u", u.detach().clone())
    holder.register_buffer("weight_v", v.detach().clone())
    out = SpectralNorm("weight", 1, 0, eps).compute_weight(holder, do_power_iteration=bool(training))
    dW = None
    if G is not None:
        out.backward(G.to(out.dtype))
        dW = holder.weight_orig.grad
    with torch.no_grad():
        sigma = torch.dot(holder.weight_u, torch.mv(holder.weight_orig, holder.weight_v))
    return out.detach(), holder.weight_u, holder.weight_v, sigma, dW


def rel_max(got, ref):
    """E = max |got - ref| / max |ref|  (ref in float64)."""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def bf16_of_float64(x):
    """float64 tensor -> the nearest bfloat16 values (ties to even), as float64: ONE rounding, on the bits (normal numbers only)."""
    bits = x.detach().double().cpu().contiguous().numpy().view(np.int64)
    drop = 52 - 7
    bits = (bits + ((bits >> drop) & 1) + (1 << (drop - 1)) - 1) & ~((1 << drop) - 1)
    return torch.from_numpy(bits.view(np.float64).copy())


def bf16_cap(n):
    """How many of a case's n elements may differ from bfloat16(float64 result): max(1, 0.1 %)."""
    return max(1, int(0.001 * n))


def bf16_rule(got, ref64):
    """got: bfloat16 values (any float dtype holding them).  -> (ok, text): every element within one bf16 ulp of bfloat16(ref64), at most
    bf16_cap(n) elements different from it at all."""
    want, got = bf16_of_float64(ref64), got.detach().double().cpu()
    assert bool(torch.isfinite(want).all()) and want.shape == got.shape
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want.abs())[1] - 8)      # |want| = m 2^e, m in [0.5, 1): 8 significant bits
    diff = (got - want).abs()
    n_diff, worst = int((diff > 0).sum()), float((diff / ulp).max())
    text = "%d of %d elements differ from bfloat16(ref64) (cap %d), the largest difference %.2f ulp" % (n_diff, want.numel(), bf16_cap(want.numel()), worst)
    return (worst <= 1.0 and n_diff <= bf16_cap(want.numel())), text
