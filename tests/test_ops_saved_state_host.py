"""ops.py hands state from an autograd forward to its backward BY NAME (ops._save_named / ops._load_named).  Host-only: the module imports
without the HIP library, a stand-in ctx takes the place of autograd's, and RenderRaysFn's forward and backward run over stub launchers
that only make tensors of the right shapes and note which backward launches were asked for."""
import pytest
import torch

from conftest import pkg


class Ctx:
    """What ops.py uses of an autograd ctx."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


@pytest.mark.parametrize("present", [(), ("a",), ("b", "d"), ("a", "b", "c", "d")])
def test_names_round_trip_with_absent_tensors(present):
    ops = pkg("ops")
    tensors = {n: (torch.full((2,), float(i)) if n in present else None) for i, n in enumerate("abcd")}
    ctx = Ctx()
    ops._save_named(ctx, **tensors)
    s = ops._load_named(ctx)
    for n, t in tensors.items():
        assert getattr(s, n) is t      # the very tensor, or None: no sentinel, no neighbour


def test_a_name_that_was_not_saved_is_an_attribute_error():
    ops = pkg("ops")
    ctx = Ctx()
    ops._save_named(ctx, raw=torch.zeros(1), bits=None)
    s = ops._load_named(ctx)
    assert s.bits is None
    with pytest.raises(AttributeError):
        s.act


BASE = {"flat", "audio", "rays", "frame", "packed", "bg", "noise_c", "noise_f", "z_c", "z_f", "map_c", "map_f", "loss_target", "loss_mask", "loss_stats"}
SAVED = {"shared": BASE | {"raw0", "act0", "bits0", "raw1", "act_d", "bits_d", "act_r", "bits_r", "src"},
         "whole": BASE | {"raw0", "act0", "bits0", "raw1", "act1", "bits1"},
         "recompute": BASE}


def _stub_launchers(ops, monkeypatch, calls):
    Z = torch.zeros
    outs = lambda N, S: (Z(N, 15), Z(N), Z(N), Z(N, S), Z(N))

    def split_save(pk, frame, level, mode, rays, xw, z=None, src=None, xw_col0=0, arch="audio", bits=None, precision=0, whole=None):
        N, S = rays.shape[0], (src if mode == ops.FIELD_RADIANCE else z).shape[1]
        return None if mode == ops.FIELD_DEFORM else Z(N, S, 16), whole[0] if whole is not None else Z(N * S, 2)

    def render_rays(packed, frame, rays, nc, nf, workspace=None, **kw):
        N = rays.shape[0]
        workspace.update(z_c=Z(N, nc), z_f=Z(N, nc + nf))
        fine = (Z(N, 15), Z(N), Z(N)) if nf > 0 else (None, None, None)
        return (Z(N, 15), Z(N), Z(N)) + fine + (Z(N), Z(N))

    def backward_split(flat, frame, level, part, act, grad_flat, grad_cond, d_raw=None, xw_grad_in=None, arch="audio", full_act=False, bits=None):
        calls.append(("split", level, part, xw_grad_in is not None))
        return Z(act.shape[0], 8) if part == ops.FIELD_RADIANCE else None

    stubs = dict(fold_conditioning=lambda flat, audio, pose, arch="audio": Z(4),
                 stratified_depths=lambda rays, nc, lindisp, t_rand: Z(rays.shape[0], nc),
                 alloc_sign_bits=lambda samples, mode, arch, dev: Z(samples, 1, dtype=torch.int32),
                 _fn=lambda name, arch="audio": ((lambda *a: 2), name),
                 field_forward_split_save=split_save,
                 field_forward_save=lambda pk, frame, level, rays, z, arch="audio", bits=None, precision=0: (Z(*z.shape, 16), Z(z.numel(), 2)),
                 composite_forward=lambda raw, z, rays, noise=None, bg=None, white_background=False: outs(*z.shape),
                 resample_merge=lambda z, w, nf, u=None: (Z(z.shape[0], z.shape[1] + nf), Z(z.shape[0], nf), Z(z.shape[0], z.shape[1] + nf, dtype=torch.int32)),
                 resample=lambda z, w, nf, u=None: Z(z.shape[0], z.shape[1] + nf),
                 render_rays=render_rays,
                 stage1_loss_forward=lambda mc, mf, tgt, msk, cw: Z(64),
                 composite_backward=lambda raw, z, *a, **kw: Z(*z.shape, 16),
                 field_backward_split=backward_split,
                 field_backward=lambda flat, frame, level, *a: calls.append(("whole", level)),
                 route_xw_grad=lambda src, g_f, nc: (Z(src.shape[0] * nc, 8), Z(src.shape[0] * (src.shape[1] - nc), 8)),
                 _driving_grad=lambda arch, flat, driving, grad_flat, grad_cond: torch.zeros_like(driving))
    for name, stub in stubs.items():
        monkeypatch.setattr(ops, name, stub)


@pytest.mark.parametrize("with_loss", [False, True])
@pytest.mark.parametrize("strategy", ["shared", "whole", "recompute"])
def test_each_strategy_saves_the_names_its_backward_asks_for(strategy, with_loss, monkeypatch):
    """The forward of each strategy saves exactly the names listed above, and the backward -- whichever levels have an upstream gradient --
    finds every name it asks for (a missing one would be an AttributeError) and issues the walks of that pattern: the shared strategy's
    coarse level still runs on a fine-only gradient (the seam gradient of the fine pass), the fine level is skipped on a coarse-only one."""
    ops = pkg("ops")
    calls = []
    _stub_launchers(ops, monkeypatch, calls)
    monkeypatch.setenv("SAHS_BWD_ONE_STREAM", "1")      # (the two-stream order needs a device's streams)
    monkeypatch.setattr(ops.RenderRaysFn, "SHARE_DEFORMATION", strategy == "shared")
    monkeypatch.setattr(ops.RenderRaysFn, "BLOCK_RAYS", 2 if strategy == "recompute" else 4096)
    N, nc, nf = 5, 4, 3
    Z = torch.zeros
    loss = (Z(N, 3), Z(N, 12), Z(12)) if with_loss else (None, None, None)
    R, D = ops.FIELD_RADIANCE, ops.FIELD_DEFORM
    fine = [("split", 1, R, False), ("split", 1, D, True)]
    expected = {"shared": {"both": fine + [("split", 0, 3, True)], "fine": fine + [("split", 0, 3, True)], "coarse": [("split", 0, 3, False)]},
                "whole": {"both": [("whole", 1), ("whole", 0)], "fine": [("whole", 1)], "coarse": [("whole", 0)]},      # (no sign bits: per-layer)
                "recompute": {"both": [("whole", 1), ("whole", 0)] * 3, "fine": [("whole", 1)] * 3, "coarse": [("whole", 0)] * 3}}[strategy]
    for pattern in ("both", "fine", "coarse"):
        ctx = Ctx()
        outs = ops.RenderRaysFn.forward(ctx, Z(10), Z(16, 29), Z(3, 4), Z(N, 8), Z(N, 15), Z(N, nc), Z(N, nc), Z(N, nf), Z(N, nc + nf), Z(12), nc, nf,
                                        False, False, "audio", *loss)
        assert ctx.strategy == strategy and len(outs) == (10 if with_loss else 8)
        assert set(ctx.saved_names) == SAVED[strategy]
        assert len(ctx.saved_names) == len(ctx.saved_tensors) == len(SAVED[strategy])
        s = ops._load_named(ctx)
        assert (s.loss_stats is not None) == with_loss and (s.map_f is not None) == with_loss
        grads = [torch.ones_like(o) for o in outs[:8]]
        if pattern == "fine":
            grads[0:3] = [None] * 3
        elif pattern == "coarse":
            grads[3:8] = [None] * 5
        del calls[:]
        res = ops.RenderRaysFn.backward(ctx, *grads)      # (no gradient for the loss output: the levels are chosen by the plain gradients)
        assert len(res) == 19 and res[0].shape == (10,) and res[1].shape == (16, 29) and all(r is None for r in res[2:])
        assert calls == expected[pattern], (pattern, calls)
    if with_loss:      # a gradient for the loss output reaches both levels, whatever else has one
        del calls[:]
        ops.RenderRaysFn.backward(ctx, *([None] * 8), torch.ones(()), None)
        assert calls == expected["both"]
