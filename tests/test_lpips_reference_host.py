"""The float64 LPIPS reference of tests/lpips_reference.py against itself, on the CPU: the two-pass head equals an independent loop over
pixels, the one-pass expansion the kernel evaluates agrees with it to 1e-15, the closed-form properties of the definition hold, and
the feature maps have the sizes the definition gives.  Nothing here touches the product: these tests say that the yardstick of
tests/test_gpu_lpips.py is the definition."""
import functools

import numpy as np
import pytest
import torch

import lpips_reference as R


def hashed_weights(seed=0):
    """He-scaled float64 convolution weights and non-negative channel weights, independent of the product's LPIPS.from_seed."""
    g = torch.Generator().manual_seed(seed)
    convs, lins = [], []
    for cout, cin, k, _, _, _ in R.CONVS:
        fan_in = cin * k * k
        convs.append((torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5,
                      (torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1) / fan_in ** 0.5))
        lins.append((torch.rand(cout, generator=g, dtype=torch.float64) * 2.0 / cout).numpy())
    return convs, lins


@functools.lru_cache(maxsize=None)
def maps_of(name, H=31, W=31, normalize=False):
    convs, lins = hashed_weights()
    a, b = dict((n, (x, y)) for n, x, y in R.content(H, W, np.uint8))[name]
    x = torch.from_numpy(np.concatenate([R.scaling(a[None], normalize), R.scaling(b[None], normalize)]))
    with torch.no_grad():
        return [m.numpy() for m in R.feature_maps(x, convs)], lins


def test_two_pass_head_equals_the_pixel_loop():
    maps, lins = maps_of("noisy")
    for f, w in zip(maps, lins):
        two, loop = R.head_two_pass(f[0], f[1], w), R.head_pixel_loop(f[0], f[1], w)
        assert two > 0.0 and abs(two - loop) <= 1e-15, (f.shape, two, loop)


@pytest.mark.parametrize("name", ["textured", "noisy", "pixel", "identical", "constant"])
def test_one_pass_expansion_agrees(name):
    worst = 0.0
    for normalize in (False, True):
        maps, lins = maps_of(name, 45, 71, normalize)
        for f, w in zip(maps, lins):
            d = abs(R.head_one_pass(f[0], f[1], w) - R.head_two_pass(f[0], f[1], w))
            worst = max(worst, d)
            assert d <= 1e-15, (name, normalize, f.shape, d)
    print("%s: one-pass vs two-pass float64 head, worst difference %.2e" % (name, worst))
    # and on synthetic features with all-zero pixels at the sizes of the GPU head tests
    for h, w in ((1, 1), (1, 3), (7, 7), (15, 16), (16, 17), (31, 31)):
        f, lw = R.synthetic_features(1, 64, h, w, 7)
        assert abs(R.head_one_pass(f[0], f[1], lw) - R.head_two_pass(f[0], f[1], lw)) <= 1e-15 * max(1.0, 64 * lw.max())


def test_identity_and_symmetry():
    maps, lins = maps_of("noisy")
    for f, w in zip(maps, lins):
        assert R.head_two_pass(f[0], f[0], w) == 0.0 and R.head_one_pass(f[0], f[0], w) == 0.0
        assert R.head_two_pass(f[0], f[1], w) == R.head_two_pass(f[1], f[0], w)
    rows = R.head_rows(*maps_of("identical"))
    assert np.all(rows == 0.0)
    # all-zero pixels: finite, and they count in the mean
    f, lw = R.synthetic_features(1, 64, 7, 7, 3, zero_fraction=0.5)
    assert np.isfinite(R.head_two_pass(f[0], f[1], lw)) and np.isfinite(R.head_one_pass(f[0], f[1], lw))
    assert R.head_two_pass(np.zeros((4, 2, 2)), np.zeros((4, 2, 2)), np.ones(4)) == 0.0


def test_scaling_laws():
    maps, lins = maps_of("textured")
    for f, w in zip(maps, lins):
        d = R.head_two_pass(f[0], f[1], w)
        assert abs(R.head_two_pass(f[0], f[1], 3.0 * w) - 3.0 * d) <= 1e-15 * 3.0 * d * 4      # w_l -> k w_l scales d_l by k
        # a positive constant on a layer's features leaves d_l unchanged (but for the 1e-10 in the norm: features are O(1))
        assert abs(R.head_two_pass(8.0 * f[0], 8.0 * f[1], w) - d) <= 1e-9 * d


def test_small_images_are_refused_and_map_sizes():
    convs, _ = hashed_weights()
    for H, W in ((30, 64), (64, 30)):
        with pytest.raises(ValueError, match="needs 31 <= H, W"):
            R.feature_maps(torch.zeros(1, 3, H, W, dtype=torch.float64), convs)
    for (H, W), sizes in R.MAP_SIZES.items():
        maps = R.feature_maps(torch.zeros(2, 3, H, W, dtype=torch.float64), convs)
        assert [tuple(m.shape[2:]) for m in maps] == sizes and [m.shape[1] for m in maps] == [c[0] for c in R.CONVS]
    assert R.MAP_SIZES[(31, 31)] == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]


def test_inputs_are_what_they_say():
    for dtype in (np.uint8, np.float32):
        items = {n: (a, b) for n, a, b in R.content(45, 71, dtype)}
        full = 255.0 if dtype == np.uint8 else 1.0
        a, b = items["pixel"]
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64)) / full
        assert (diff > 0).sum() == 1 and abs(diff.max() - 1 / 255) < 1e-7
        a, b = items["noisy"]
        assert 0 < np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / full <= 20.5 / 255
        a, b = items["identical"]
        assert np.array_equal(a, b) and a is not b
        a, b = items["constant"]
        assert not a[:, :40].any() and not b[:, :40].any() and a[:, 50:].any()
        assert all(x.dtype == dtype and x.shape == (45, 71, 3) for pair in items.values() for x in pair)
    # the reference ranks them: identical < one pixel < noisy < another image
    convs, lins = hashed_weights()
    score = {}
    for name, a, b in R.content(45, 71, np.uint8):
        x = torch.from_numpy(np.concatenate([R.scaling(a[None], False), R.scaling(b[None], False)]))
        with torch.no_grad():
            score[name] = R.head_rows([m.numpy() for m in R.feature_maps(x, convs)], lins)[0, 0]
    assert 0.0 == score["identical"] < score["pixel"] < score["noisy"] < score["textured"], score
