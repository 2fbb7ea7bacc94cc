"""Shared references for the differentiable SPADE modulation (tests/test_spade_train_host.py, tests/test_gpu_spade_backward.py):

* ``torch_modulate``: the reference's arithmetic -- InstanceNorm, 1 + gamma, multiply, add beta, LeakyReLU -- as six differentiable torch
  ops, with the mean and the biased variance written out (``F.instance_norm`` refuses one element per plane) and the mean as a true
  division (a plane of equal values then normalises to exactly 0 in any precision);
* ``analytic_backward``: the backward the fused kernel implements, in float64;
* ``swapped``: ``ops.spade_modulate`` replaced by ``torch_modulate`` (spade.py reaches the op through the module attribute), which makes
  the drop-in tree run on the CPU and in float64;
* the op-level cases and the generator yardsticks, computed once per session.
"""
import contextlib
import copy
import functools

import numpy as np
import torch

from conftest import load_golden, pkg

EPS = 1e-5
SLOPES = (0.2, 1.0, 0.0)
# name -> shape.  The smallest shapes at which each path of the kernels can go wrong:
OP_CASES = {"ragged": (3, 5, 7, 9),            # scalar path; plane [1, 2] is constant with beta 0: variance 0 and y == 0 exactly
            "one_element": (1, 1, 1, 1),
            "one_vector": (1, 2, 2, 2),        # hw = 4: one 16-byte vector, seven empty chunks
            "partial_trip": (2, 3, 96, 96),    # a chunk of 288 vectors: the second 256-thread trip is partial
            "many_planes": (64, 160, 2, 2),    # 10240 planes: the apply pass's workgroup cap is 1 and it strides
            "unaligned": (2, 4, 8, 8)}         # hw % 4 == 0 but the tensors start one float into their buffers: scalar path


def torch_modulate(x, gamma, beta, eps=EPS, slope=1.0):
    hw = x.shape[2] * x.shape[3]
    mean = x.sum((2, 3), keepdim=True) / hw
    d = x - mean
    var = (d * d).sum((2, 3), keepdim=True) / hw
    return torch.nn.functional.leaky_relu(d / torch.sqrt(var + eps) * (1 + gamma) + beta, slope)


def analytic_backward(x, gamma, beta, g, eps=EPS, slope=1.0):
    """-> dx, dgamma, dbeta in float64; the mask from the output, as the kernel takes it."""
    x, gamma, beta, g = (t.detach().double().cpu() for t in (x, gamma, beta, g))
    hw = x.shape[2] * x.shape[3]
    mean = x.sum((2, 3), keepdim=True) / hw
    r = 1.0 / torch.sqrt(((x - mean) ** 2).sum((2, 3), keepdim=True) / hw + eps)
    xh = (x - mean) * r
    y = xh * (1 + gamma) + beta
    out = torch.where(y > 0, y, slope * y)
    dy = g * torch.where(out > 0, torch.ones_like(g), torch.full_like(g, slope))
    dxh = dy * (1 + gamma)
    dx = r * (dxh - dxh.mean((2, 3), keepdim=True) - xh * (dxh * xh).mean((2, 3), keepdim=True))
    return dx, dy * xh, dy


def autograd_backward(x, gamma, beta, g, eps=EPS, slope=1.0, dtype=torch.float64, device="cpu"):
    """Autograd of torch_modulate in ``dtype`` on ``device`` -> dx, dgamma, dbeta."""
    leaves = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in (x, gamma, beta)]
    torch_modulate(*leaves, eps=eps, slope=slope).backward(g.detach().to(device=device, dtype=dtype))
    return tuple(t.grad for t in leaves)


@functools.lru_cache(maxsize=None)
def op_case(name, slope):
    """float32 CPU tensors x, gamma, beta, g of OP_CASES[name], the same for every caller.  beta is nudged so that |y| >= 0.05 wherever y
    is not exactly 0: no comparison between two precisions then hinges on which side of the kink a value fell."""
    shape = OP_CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(OP_CASES).index(name))
    x = torch.randn(shape, generator=gen) * 3 + 1
    gamma, beta, g = (torch.randn(shape, generator=gen) for _ in range(3))
    if name == "ragged":
        x[1, 2], beta[1, 2] = 0.25, 0.0
    for _ in range(2):      # (the second round moves nothing unless float32 rounding of beta undid the first)
        y = torch_modulate(x.double(), gamma.double(), beta.double(), slope=1.0)
        near = (y != 0) & (y.abs() < 0.05)
        beta = torch.where(near, (beta.double() + torch.sign(y) * 0.05).float(), beta)
    y = torch_modulate(x.double(), gamma.double(), beta.double(), slope=1.0)
    assert bool(((y == 0) | (y.abs() >= 0.049)).all())
    if name == "ragged":
        assert bool((y[1, 2] == 0).all())
    return x, gamma, beta, g


def rel_max(got, ref):
    """E = max |got - ref| / max |ref|  (ref in float64)."""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def global_rel_l2(grads, ref):
    """sqrt(sum |g - g64|^2) / sqrt(sum |g64|^2) over every parameter that has a yardstick gradient."""
    num = sum(float((grads[k].detach().double().cpu() - ref[k]).pow(2).sum()) for k in ref)
    return (num / sum(float(ref[k].pow(2).sum()) for k in ref)) ** 0.5


@contextlib.contextmanager
def swapped():
    ops = pkg("ops")
    fused = ops.spade_modulate
    ops.spade_modulate = torch_modulate
    try:
        yield
    finally:
        ops.spade_modulate = fused


# ---- the generators' training step on the inputs of tests/golden/spade_train.npz ----
GENERATORS = {"generator": "Generator", "generator_audio": "Generator_audio"}


def seeded(name):
    """The drop-in generator under the fixture's seed, in train() mode; the checksum pins the initialisation to the reference's."""
    g = load_golden("spade_train")
    torch.manual_seed(int(g[name + ":seed"]))
    G = getattr(pkg("spade"), GENERATORS[name])().train()
    sd = G.state_dict()
    assert sum(v.numel() for v in sd.values()) == int(g[name + ":param_count"])
    total = sum(float(v.double().abs().sum()) for v in sd.values())
    assert abs(total - float(g[name + ":param_abs_sum"])) <= 1e-9 * total, "seeded initialisation differs from the fixture's (another torch build?)"
    return G


def step_inputs(name, device="cpu", dtype=torch.float32):
    """-> (I_src, I_raw, target, driving or None) of the fixture."""
    g = load_golden("spade_train")
    T = lambda k: torch.from_numpy(g[name + ":" + k]).to(device=device, dtype=dtype)
    return T("i_src"), T("i_raw"), T("target"), (T("window") if name + ":window" in g else None)


def loss_and_grads(G, i_src, i_raw, target, driving):
    """The step's forward and backward without an optimiser -> (pre-clamp output, loss, {parameter name: gradient or None})."""
    G.zero_grad()
    y = G(i_src, i_raw) if driving is None else G(i_src, i_raw, driving)
    loss = torch.nn.functional.mse_loss(y.clamp(0, 1), target)
    loss.backward()
    return y.detach(), float(loss.detach()), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in G.named_parameters()}


@functools.lru_cache(maxsize=None)
def cpu_step(name):
    """The swapped tree on the CPU in float32 and in float64 (the yardstick), each from the seeded initialisation.
    -> dict(G32 = the float32 module after its forward, y32, loss32, grads32, loss64, grads64); gradients that are None are left out."""
    G32 = seeded(name)
    G64 = copy.deepcopy(G32).double()
    with swapped():
        y32, loss32, grads32 = loss_and_grads(G32, *step_inputs(name))
        _, loss64, grads64 = loss_and_grads(G64, *step_inputs(name, dtype=torch.float64))
    unreached = sorted(k for k, v in grads64.items() if v is None)
    return dict(G32=G32, y32=y32, loss32=loss32, loss64=loss64, unreached=unreached,
                grads32={k: v for k, v in grads32.items() if v is not None}, grads64={k: v for k, v in grads64.items() if v is not None})


def buffer_abs_sums(G):
    return np.array([float(v.double().abs().sum()) for _, v in G.named_buffers()], np.float64)
