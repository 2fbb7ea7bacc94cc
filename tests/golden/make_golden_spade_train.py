#!/usr/bin/env python3
"""Golden vectors for one TRAIN-MODE step of the Stage-II generators (reference nerf/_init_spade.py ``Generator`` :315-325 and
``Generator_audio`` :359-372, imported unmodified as in make_golden_spade.py; the step is train_get_texture_photo.py:168-177 /
train_get_texture_photo_audio.py:180-190: ``G.train()``, ``G(...)``, ``.clamp(0, 1)``, ``nn.MSELoss``).

What the reference pins here is the train-mode FORWARD: BatchNorm on batch statistics with its running-statistics update, spectral norm
with its power iteration (u, v move), the pre-clamp output and the loss.  It pins NO gradient: under a current torch the unmodified
reference's own backward raises (``out += identity`` on a ReLU output, _init_spade.py:36, modifies a tensor that ReLU's backward
needs), so ``loss.backward()`` is never called here and the gradient tests take their yardstick from float64 autograd of the drop-in
tree instead (tests/spade_reference.py).

Per case: the inputs, the reference's pre-clamp output ``y`` and ``loss``, the absolute sum of every buffer after that forward (in
``named_buffers()`` order, with the names), and the seed, parameter count and parameter checksum as spade.npz has them.  Data only.
The sizes stay at 32 x 32 and 32 x 48: there float32 gradients of the tree are within 6e-6 (relative L2) of its float64 gradients; at
64 x 64 activation-kink flips between the two precisions raise that to 1e-3, which would blunt every comparison made against it.

usage:  python tests/golden/make_golden_spade_train.py            (writes tests/golden/spade_train.npz)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_spade import import_spade      # noqa: E402

#        name,              class,             model seed, input seed, (H, W),  audio window
CASES = (("generator", "Generator", 7, 11, (32, 32), False),
         ("generator_audio", "Generator_audio", 9, 13, (32, 48), True))


def main():
    S = import_spade()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    mine = importlib.import_module("sahs-deformable-nerf_amd.spade")
    out = {}
    for name, cls, seed, input_seed, (H, W), audio in CASES:
        torch.manual_seed(seed)
        G = getattr(S, cls)()
        torch.manual_seed(seed)
        Gm = getattr(mine, cls)()
        sd, sdm = G.state_dict(), Gm.state_dict()
        assert list(sd.keys()) == list(sdm.keys()), name + ": state_dict layout differs from the reference's"
        assert all(torch.equal(sd[k], sdm[k]) for k in sd), name + ": seeded initialisation differs from the reference's"
        out[name + ":seed"] = np.array(seed, np.int64)
        out[name + ":param_count"] = np.array(sum(v.numel() for v in sd.values()), np.int64)
        out[name + ":param_abs_sum"] = np.array(sum(float(v.double().abs().sum()) for v in sd.values()), np.float64)
        gen = torch.Generator().manual_seed(input_seed)
        i_src, i_raw, target = (torch.rand(1, 3, H, W, generator=gen) for _ in range(3))
        args = (i_src, i_raw)
        if audio:
            window = torch.randn(16, 29, generator=gen)
            args += (window,)
            out[name + ":window"] = window.numpy()
        G.train()
        with torch.no_grad():      # (the forward is all the reference can do: see the docstring)
            y = G(*args)
            loss = torch.nn.MSELoss()(y.clamp(0, 1), target)
        out[name + ":input_seed"] = np.array(input_seed, np.int64)
        out[name + ":i_src"], out[name + ":i_raw"], out[name + ":target"] = i_src.numpy(), i_raw.numpy(), target.numpy()
        out[name + ":y"], out[name + ":loss"] = y.numpy(), np.array(float(loss), np.float64)
        buffers = list(G.named_buffers())
        out[name + ":buffer_names"] = np.array([k for k, _ in buffers])
        out[name + ":buffer_abs_sums"] = np.array([float(v.double().abs().sum()) for _, v in buffers], np.float64)
        print(name, tuple(i_src.shape), "->", tuple(y.shape), "loss %.17g" % float(loss), "buffers:", len(buffers))
    path = os.path.join(HERE, "spade_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
