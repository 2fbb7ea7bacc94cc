"""CPU-side checks of the fused backward walk's host contract for the NeRFaceModels (include/sahs_nerf.h: sahs_model_bits_words_part,
sahs_model_field_backward_fused_workspace_words): sign-word counts and workspace sizes per model and part, no GPU needed."""
import pytest

from conftest import pkg

AUDIO, NERFACE, STATIC = 0, 1, 2


def _sbits(warp_h, hyp_h, trunk_layers, deform):
    """sahs_layout.hpp, namespace sbits: words(width) = 4 * ceil(width / 16 / 8) per (leaky-)ReLU layer; six warp-field layers (128 wide)
    and six hyper-sheet layers (64 wide) in the deformation part, the trunk (256 wide) and four colour + four seg layers (128 wide) in the
    radiance part -> (deformation, radiance) words per sample"""
    words = lambda w: 4 * ((w // 16 + 7) // 8)
    bd = (6 * words(warp_h) + 6 * words(hyp_h)) if deform else 0
    br = trunk_layers * words(256) + 4 * words(128) + 4 * words(128)
    return bd, br


def test_sign_words_per_sample():
    L = pkg("_lib").lib()
    # NeRFaceModel (4-layer trunk, warp + hyper sheet): 6*4 + 6*4 = 48, 4*8 + 16 + 16 = 64, together 112
    assert _sbits(128, 64, 4, True) == (48, 64)
    assert [L.sahs_model_bits_words_part(NERFACE, p) for p in (1, 2, 0, 3)] == [48, 64, 112, 112]
    # without deformation nets: the whole network is the radiance part, 64 words
    assert _sbits(128, 64, 4, False) == (0, 64)
    assert L.sahs_model_bits_words_part(STATIC, 0) == 64 and L.sahs_model_bits_words_part(STATIC, 3) == 64
    assert L.sahs_model_bits_words_part(STATIC, 1) == 0
    # the AudioFaceModel's (8-layer trunk) are unchanged: 48 / 96 / 144
    assert _sbits(128, 64, 8, True) == (48, 96)
    assert [L.sahs_model_bits_words_part(AUDIO, p) for p in (1, 2, 0)] == [48, 96, 144]
    assert L.sahs_model_bits_words_part(3, 0) == 0 and L.sahs_model_bits_words_part(NERFACE, 4) == 0


# floats of workspace per sample of the fused walk (include/sahs_nerf.h), from the act:: table of sahs_layout.hpp: part 2 = the radiance
# dZ planes (act::STRIDE - act::XW) + d grid features 32 + two encodings' gradient rows 2 * 16 * (KB_XYZ + KB_AMB) + seam 8; part 1 = the
# deformation dZ planes (act::XW) + 8; part 3 = both + the seam rows 8
PER_SAMPLE = {(AUDIO, 1): 1256, (AUDIO, 2): 3736, (AUDIO, 3): 5000,
              (NERFACE, 1): 1288, (NERFACE, 2): 2808, (NERFACE, 3): 4104,
              (STATIC, 3): 2616}


@pytest.mark.parametrize("model,part", sorted(PER_SAMPLE))
def test_fused_workspace_words(model, part):
    L = pkg("_lib").lib()
    w = lambda P: L.sahs_model_field_backward_fused_workspace_words(model, part, P)
    assert w(1) > 0 and w(131072) > 0
    assert (w(2048 + 4096) - w(2048)) == 4096 * PER_SAMPLE[(model, part)]       # linear in P at the documented rate
    assert w(0) > 0                                                               # (the constant part: grid copies, weight stream, scratch)


@pytest.mark.parametrize("part", [1, 2])
def test_static_model_has_part_3_only(part):
    L = pkg("_lib").lib()
    assert L.sahs_model_field_backward_fused_workspace_words(STATIC, part, 4096) == -1
    assert L.sahs_model_field_backward_fused_workspace_words(STATIC, 3, 4096) > 0


def test_fused_workspace_rejects_bad_arguments():
    L = pkg("_lib").lib()
    for model, part, P in ((3, 3, 16), (-1, 3, 16), (NERFACE, 0, 16), (NERFACE, 4, 16), (NERFACE, 3, -1)):
        assert L.sahs_model_field_backward_fused_workspace_words(model, part, P) == -1, (model, part, P)


def test_alloc_sign_bits_for_the_nerface_models():
    """ops.alloc_sign_bits returns a buffer (not None) for both NeRFaceModels, so their training forward writes the planes the fused
    walk reads; checked on the CPU here only for its shape logic (no kernel runs)."""
    ops = pkg("ops")
    for arch, mode, words in (("nerface", ops.FIELD_ALL, 112), ("nerface", ops.FIELD_DEFORM, 48), ("nerface", ops.FIELD_RADIANCE, 64),
                              ("nerface_static", ops.FIELD_ALL, 64)):
        b = ops.alloc_sign_bits(10, mode, arch, "cpu")
        assert b is not None and tuple(b.shape) == (10, words), (arch, mode)
