"""Stage-II refiner training, the parts a CPU can check: the backward formula the fused kernel implements against float64 autograd of
the six-op formula; the drop-in generators in train() mode (BatchNorm on batch statistics, spectral norm's power iteration) against the
reference's own train-mode forward (tests/golden/spade_train.npz), with ``ops.spade_modulate`` swapped for the torch formula; and the
condition that makes the fixture's inputs a usable yardstick: float32 and float64 gradients of that tree agree."""
import numpy as np
import pytest
import torch

import spade_reference as R
from conftest import load_golden, pkg


@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("case", sorted(R.OP_CASES))
def test_analytic_backward_is_float64_autograd_of_the_formula(case, slope):
    x, gamma, beta, g = R.op_case(case, slope)
    want = R.autograd_backward(x, gamma, beta, g, slope=slope)
    for name, got, ref in zip(("dx", "dgamma", "dbeta"), R.analytic_backward(x, gamma, beta, g, slope=slope), want):
        assert R.rel_max(got, ref) <= 1e-12, (name, R.rel_max(got, ref))


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_train_mode_forward_reproduces_the_reference(name):
    """Fails while SPADELayer.forward refuses tensors that need a gradient."""
    g, c = load_golden("spade_train"), R.cpu_step(name)
    assert abs(c["loss32"] - float(g[name + ":loss"])) <= 1e-6 * float(g[name + ":loss"])
    ref = g[name + ":y"]
    assert float((c["y32"] - torch.from_numpy(ref)).abs().max()) <= 2e-4 * float(np.abs(ref).max())      # (test_spade.py's bound for the eval-mode forward)
    assert [k for k, _ in c["G32"].named_buffers()] == [str(k) for k in g[name + ":buffer_names"]]
    have, want = R.buffer_abs_sums(c["G32"]), g[name + ":buffer_abs_sums"]
    assert np.all(np.abs(have - want) <= 1e-6 * np.abs(want)), np.abs(have / want - 1).max()


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_float32_gradients_agree_with_float64(name):
    """Global relative L2 over all parameters (measured: 6.0e-6 Generator, 4.2e-6 Generator_audio; 1.4e-3 at 64 x 64, where activation
    kinks flip between the precisions -- the reason the fixture stays at 32 x 32 and 32 x 48)."""
    c = R.cpu_step(name)
    assert sorted(c["grads32"]) == sorted(c["grads64"])
    err = R.global_rel_l2(c["grads32"], c["grads64"])
    print("%s: float32 vs float64 gradients, global relative L2 %.3e" % (name, err))
    assert err <= 2e-5, err
    assert abs(c["loss32"] - c["loss64"]) <= 1e-6 * c["loss64"]


@pytest.mark.parametrize("name", sorted(R.GENERATORS))
def test_parameters_the_forward_never_reaches(name):
    """The ``residual`` Sequential of the two downsampling ResBlock2d's; for Generator_audio also the identity encoder's deepest block
    (its map is replaced by the audio code) and AudioNet's unused encoder_fc1."""
    prefixes = ["idencoder.layer3.residual.", "idencoder.layer4.residual."]
    if name == "generator_audio":
        prefixes = ["idencoder.layer3.residual.", "idencoder.layer4.", "AudioNet.encoder_fc1."]
    G = R.cpu_step(name)["G32"]
    want = sorted(k for k, _ in G.named_parameters() if k.startswith(tuple(prefixes)))
    assert want and R.cpu_step(name)["unreached"] == want


def test_backward_entry_refuses_before_any_launch():
    """Every call here is answered by argument validation (fabricated addresses, never dereferenced) -- with or without a GPU."""
    L = pkg("_lib").lib()
    A = 1 << 20
    call = lambda planes=6, hw=16, out=A, slope=0.2, dx=A, dgamma=A, dbeta=A, work=A, eps=1e-5: L.sahs_spade_modulate_backward(
        planes, hw, A, A, out, A, A, eps, slope, dx, dgamma, dbeta, work, None)
    assert [L.sahs_spade_modulate_backward_workspace_words(p) for p in (-1, 0, 1, 7)] == [0, 0, 16, 112]
    assert L.sahs_spade_modulate_backward_workspace_words(7) == L.sahs_spade_modulate_workspace_words(7)
    assert call(planes=0) == 0 and call(hw=0) == 0                      # nothing to do: success without a launch
    assert call(planes=65536) == 1 and b"65535" in L.sahs_last_error()      # gridDim.y: the message names the limit
    assert L.sahs_spade_modulate(65536, 16, A, A, A, 1e-5, 0.2, A, A, None) == 1 and b"65535" in L.sahs_last_error()      # the forward's too
    assert call(planes=-1) == 1 and call(hw=-1) == 1 and call(eps=0.0) == 1
    assert call(out=None) == 1                                          # the mask is read from out unless slope == 1
    assert call(slope=-0.1) == 1 and call(slope=float("nan")) == 1
    assert call(dx=None, dgamma=None, dbeta=None) == 1
    assert call(work=None) == 1                                         # dx needs the workspace


def test_refine_learning_rate_is_the_reference_schedule():
    """train_get_texture_photo.py:147-155."""
    S, CfgNode = pkg("spade"), pkg("cfgnode").CfgNode
    cfg = CfgNode({"texture_refine": {"lr_G": 2e-4, "epochs": 3, "epochs_decay": 4}})
    assert [S.refine_learning_rate(cfg, e) for e in range(3)] == [2e-4] * 3
    for e in range(3, 7):
        assert S.refine_learning_rate(cfg, e) == 2e-4 / 4 * (7 - e)
    assert S.refine_learning_rate(cfg, 3) == 2e-4 and S.refine_learning_rate(cfg, 6) == 2e-4 / 4


def test_refine_step_is_the_reference_step():
    """zero_grad, forward, clamp, MSE, backward, optimiser step -- on a stand-in module: the step itself holds no SPADE-specific code."""
    S = pkg("spade")

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 3, 1)

        def forward(self, i_src, i_raw, driving=None):
            return self.conv(i_raw) + i_src.mean() + (0 if driving is None else driving.sum())

    torch.manual_seed(0)
    a, b = Tiny(), Tiny()
    b.load_state_dict(a.state_dict())
    i_src, i_raw, target, drv = torch.rand(1, 3, 4, 4), torch.rand(1, 3, 4, 4) * 3 - 1, torch.rand(1, 3, 4, 4), torch.rand(2, 2) * 0.1
    for driving in (None, drv):
        oa, ob = torch.optim.Adam(a.parameters(), lr=1e-2), torch.optim.Adam(b.parameters(), lr=1e-2)
        a.conv.weight.grad = torch.ones_like(a.conv.weight)      # a stale gradient: the step clears it
        loss = S.refine_step(a, oa, i_src, i_raw, target, driving)
        want = torch.nn.MSELoss()(b(i_src, i_raw, driving).clamp(0, 1), target)
        want.backward()
        ob.step()
        assert not loss.requires_grad and float(loss) == float(want)
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        b.zero_grad()
