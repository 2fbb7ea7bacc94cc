"""Stage-II inference on the host: ``spade.freeze_identity`` / ``FrozenRefiner`` / ``spade.refine_frames`` with the fused ops swapped for
torch statements (tests/spade_frozen_reference.py), everything in float64.  The frozen form and the generator then differ only by the
order of float64 sums -- the statistics of an upsampled plane are taken from its source, batched convolutions -- which is ~1e-15; a
wrong map for a block, a missed layer, a stale or un-normalised weight moves the output by 1e-2 or more.  The bound is 1e-9 of the
output's largest magnitude."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import spade_frozen_reference as FR
from conftest import REPO, pkg

TOL = 1e-9
NAMES = sorted(FR.SIZES)


def _close(got, ref, what):
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print("%s: max |got - ref| = %.3e, scale %.3e" % (what, err, scale))
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert err <= TOL * scale, "%s: %.3e > %g * %.3e" % (what, err, TOL, scale)


def _frozen64(name, fuse=False, image_range=False, **kw):
    S = pkg("spade")
    G = FR.generator(name, image_range).double()
    if fuse:
        S.fuse_spectral_norm_(G)
    return G, S.freeze_identity(G, FR.inputs(name)[0].double(), dtype=torch.float64, **kw)


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_frozen_equals_generator(name, fuse, fold):
    _, i_raw, windows = (None if t is None else t.double() for t in FR.inputs(name))
    ref = FR.reference64(name)
    assert float(ref.abs().max()) > 1e-2
    with FR.swapped():
        _, frozen = _frozen64(name, fuse=fuse, fold_upsample=fold)
        batched = frozen(i_raw) if windows is None else frozen(i_raw, windows)
        single = torch.cat([frozen(i_raw[b:b + 1]) if windows is None else frozen(i_raw[b:b + 1], windows[b]) for b in range(3)])
    _close(batched, ref, "%s B=3" % name)
    _close(single, ref, "%s B=1" % name)
    _close(batched, single, "%s batched rows against single calls" % name)
    assert float((ref[0] - ref[1]).abs().max()) > 1e-3      # the rows are different frames
    if windows is not None:      # one (16, 29) window for the whole batch
        with FR.swapped():
            G, frozen = _frozen64(name, fuse=fuse, fold_upsample=fold)
            _close(frozen(i_raw, windows[1]), FR.run(G, FR.inputs(name)[0].double(), i_raw, windows[1:2].expand(3, 16, 29)), "one window")


def test_layers_missed_would_show():
    """The margin the 1e-9 bound has: the cached maps of one layer zeroed move the output by far more."""
    name = "generator"
    i_raw = FR.inputs(name)[1].double()
    with FR.swapped():
        _, frozen = _frozen64(name)
        good = frozen(i_raw)
        for t in frozen.blocks[3]["spade2"][1]:
            t.zero_()
        bad = frozen(i_raw)
    assert float((good - bad).abs().max()) > 1e-2 * float(good.abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_refusals_and_snapshot(name):
    S = pkg("spade")
    i_src, i_raw, windows = (None if t is None else t.double() for t in FR.inputs(name))
    args = lambda x: (x,) if windows is None else (x, windows[:x.shape[0]])
    with FR.swapped():
        G, frozen = _frozen64(name)
        before = frozen(*args(i_raw))
        with pytest.raises(ValueError, match="eval"):
            S.freeze_identity(copy.deepcopy(G).train(), i_src, dtype=torch.float64)
        h, w = FR.SIZES[name]
        with pytest.raises(ValueError) as e:
            frozen(*args(torch.zeros(3, 3, h, w + 2, dtype=torch.float64)))
        assert str((3, 3, h, w + 2)) in str(e.value) and "%d, %d" % (h, w) in str(e.value)      # names both sizes
        with pytest.raises(ValueError):
            frozen(i_raw, None) if windows is not None else frozen(i_raw, torch.zeros(3, 16, 29, dtype=torch.float64))
        with torch.no_grad():      # the snapshot is a copy: G changes, the frozen output does not
            for p in G.parameters():
                p.mul_(1.5).add_(0.1)
            for b in G.buffers():
                if b.is_floating_point():
                    b.add_(0.1)
        assert torch.equal(frozen(*args(i_raw)), before)
    assert frozen.cached_bytes > frozen.cached_map_bytes > 0
    if name == "generator":      # gamma and beta of the 18 layers in float64, from the layer shapes at 32 x 32
        assert frozen.cached_map_bytes == 2 * _map_elements(16) * 8


def _map_elements(res):
    """Elements of gamma over the 18 SPADE layers for a stem output of res x res: spade1 modulates the block's input channels at the
    input resolution, spade2 (output channels) and spade_s (input channels) at the block's output resolution."""
    total = 0
    for cin, cout, _, how in pkg("spade").RefineNetwork.PLAN:
        after = {"down": res // 2, "up": res * 2, None: res}[how]
        total += cin * res * res + cout * after * after + cin * after * after
        res = after
    return total


def test_map_elements_at_512():
    """The figure the documents quote: 107,741,184 elements of gamma (and as many of beta) for Generator at 512 x 512."""
    assert _map_elements(256) == 107_741_184


@pytest.mark.parametrize("name", NAMES)
def test_byte_cap_holds_for_unfrozen_fp32(name):
    """The cap the GPU test holds refine_frames to (within one level of the float64 bytes everywhere, equal in 99 % of positions) is
    one the UNFROZEN float32 generator keeps on the same seeded inputs -- it is a cap on float32 arithmetic, not a measurement."""
    i_src, _, windows = FR.inputs(name)
    with FR.swapped():
        y32 = FR.run(FR.generator(name, image_range=True), i_src, FR.frames_input(FR.frames_u8(name)), windows)
    worst, equal = FR.bytes_agreement(FR.to_bytes(y32), FR.frames_bytes64(name)[0])
    inside = float(((FR.frames_bytes64(name)[1] > 0) & (FR.frames_bytes64(name)[1] < 255)).double().mean())
    print("%s: unfrozen fp32 bytes: worst %d level, %.4f %% equal; %.1f %% of the values lie inside (0, 255)" % (name, worst, 100 * equal, 100 * inside))
    assert inside > 0.25      # the seed leaves enough unclamped values for the comparison to mean something
    assert worst <= 1 and equal >= FR.BYTES_EQUAL_CAP


@pytest.mark.parametrize("name", NAMES)
def test_refine_frames_bytes(name, tmp_path):
    from PIL import Image
    S = pkg("spade")
    frames = FR.frames_u8(name)
    i_src, _, windows = (None if t is None else t.double() for t in FR.inputs(name))
    x = FR.frames_input(frames, torch.float64)      # the reference's input: / 255 in float32
    with FR.swapped():
        G, frozen = _frozen64(name, image_range=True)
        y = FR.run(G, i_src, x, windows)
        log = []
        got = S.refine_frames(frozen, (f.numpy() for f in frames), driving=None if windows is None else list(windows), batch=2,
                              savedir=str(tmp_path / "out"), log=log.append)      # a generator of arrays, a ragged last batch
        floats = [f.double() / 255 * 0.999 + 0.0004 for f in frames]
        via_cast = S.refine_frames(frozen, floats, driving=windows, batch=8, log=None)
        cast = [torch.from_numpy(pkg("evaluation").cast_to_image(f)) for f in floats]
        fed_cast = S.refine_frames(frozen, cast, driving=windows, batch=8, log=None)
        raw = S.refine_frames(frozen, floats, driving=windows, batch=8, quantise=False, log=None)
        y_raw = FR.run(G, i_src, torch.stack(floats).float().permute(0, 3, 1, 2).double(), windows)
    assert len(got) == 3 and len(log) == 1
    want, scaled = FR.to_bytes(y), (y.clamp(0, 1) * 255).permute(0, 2, 3, 1)
    for i, img in enumerate(got):
        assert img.dtype == torch.uint8 and tuple(img.shape) == FR.SIZES[name] + (3,)
        diff = (img.int() - want[i].int()).abs()
        near = (scaled[i] - scaled[i].round()).abs() <= 1e-6      # a byte may differ, by one level, only where x255 lies at an integer
        assert int(diff.max()) <= 1 and bool((near | (diff == 0)).all())
        back = np.asarray(Image.open(os.path.join(str(tmp_path / "out"), "f_%04d.png" % i)))
        assert np.array_equal(back, img.numpy())
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["f_0000.png", "f_0001.png", "f_0002.png"]
    assert all(torch.equal(a, b) for a, b in zip(via_cast, fed_cast))      # quantise=True on floats = feeding their cast_to_image bytes
    want_raw, scaled_raw = FR.to_bytes(y_raw), (y_raw.clamp(0, 1) * 255).permute(0, 2, 3, 1)
    for i, img in enumerate(raw):      # quantise=False: the float frames as they are (float32)
        diff = (img.int() - want_raw[i].int()).abs()
        assert bool((((scaled_raw[i] - scaled_raw[i].round()).abs() <= 1e-6) | (diff == 0)).all()) and int(diff.max()) <= 1
    assert any(not torch.equal(a, b) for a, b in zip(raw, via_cast))


def test_lib_table_declares_the_frozen_entries():
    """_lib's table lists the new symbols with the header's argument counts (the header's text is the contract)."""
    text = open(os.path.join(REPO, "include", "sahs_nerf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs = pkg("_lib").SIGNATURES
    for name in ("sahs_spade_modulate_frozen_workspace_words", "sahs_spade_modulate_frozen", "sahs_spade_modulate_frozen_bf16"):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/sahs_nerf.h" % name
        assert name in sigs and len(sigs[name][1]) == len(m.group(1).split(",")), name
    ops = pkg("ops")
    with pytest.raises(pkg("_lib").SahsError):      # no CPU fallback
        ops.spade_modulate_frozen(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2))
