"""CPU-side checks of precision SAHS_BF16X3 for the NeRFaceModels (include/sahs_nerf.h: sahs_model_packed_words,
sahs_model_executed_macs_part, the Python model and the split-chain predicate), no GPU needed."""
import ctypes

import pytest

from conftest import pkg

AUDIO, NERFACE, STATIC = 0, 1, 2
F32, BF16, RESERVED, BF16X3 = 0, 1, 2, 3


@pytest.mark.parametrize("model", [NERFACE, STATIC])
def test_packed_words(model):
    L = pkg("_lib").lib()
    assert L.sahs_model_packed_words(model, BF16X3) > 0
    assert L.sahs_model_packed_words(model, RESERVED) == -1      # the A/B precision id stays out of the shipped library
    assert L.sahs_model_packed_words(model, 4) == -1


def test_packed_layouts():
    """with deformation nets: the AudioFaceModel's [hi/lo streams | fp32 pack] (the fp32 pack serves SAHS_X3_DEFORM=f32); without them:
    the hi/lo streams alone.  A hi/lo stream is the bf16 stream twice over, behind the same fp32 feature grid."""
    L = pkg("_lib").lib()
    grid = 32 * 32 ** 3
    for model in (AUDIO, NERFACE):
        x3 = L.sahs_model_packed_words(model, BF16X3)
        f32 = L.sahs_model_packed_words(model, F32)
        assert x3 > f32 and (x3 - f32) % 4 == 0
    static_bf16 = L.sahs_model_packed_words(STATIC, BF16)
    static_x3 = L.sahs_model_packed_words(STATIC, BF16X3)
    # bf16: [grid | 2 levels x STREAM_HW halfwords = STREAM_HW words | chunk table]; x3: [grid | 2 levels x 2 STREAM_HW halfwords]
    assert static_x3 > static_bf16 and (static_x3 - grid) % 1024 == 0
    assert L.sahs_model_packed_words(STATIC, BF16X3) < L.sahs_model_packed_words(NERFACE, BF16X3)


@pytest.mark.parametrize("arch", ["nerface", "nerface_static"])
@pytest.mark.parametrize("part", [0, 1, 2])
def test_executed_macs_three_times_bf16(arch, part):
    ops = pkg("ops")
    x3 = ops.executed_macs_per_sample(arch, ops.SAHS_BF16X3, part)
    if arch == "nerface":      # the model's SAHS_BF16 is mixed (split-operand deformation nets): the plain-bf16 tiles of its layer program
        f = pkg("_lib").lib().sahs_layout_executed_macs_nf
        f.restype, f.argtypes = ctypes.c_long, [ctypes.c_int, ctypes.c_int]
        bf16 = f(BF16, part)
        assert ops.executed_macs_per_sample(arch, ops.SAHS_BF16, 2) == f(BF16, 2) and ops.executed_macs_per_sample(arch, ops.SAHS_BF16, 1) == 3 * f(BF16, 1)
    else:
        bf16 = ops.executed_macs_per_sample(arch, ops.SAHS_BF16, part)
    assert x3 == 3 * bf16
    if arch == "nerface_static" and part == 1:
        assert x3 == 0                                                            # no deformation nets
    else:
        assert x3 > 0


def test_executed_macs_parts_add_up():
    ops = pkg("ops")
    for arch in ("nerface", "nerface_static"):
        m = [ops.executed_macs_per_sample(arch, ops.SAHS_BF16X3, p) for p in (0, 1, 2)]
        assert m[0] == m[1] + m[2], (arch, m)


@pytest.mark.parametrize("name", ["expression", "expression_static"])
def test_model_accepts_bf16x3(name):
    sahs, ops = pkg(), pkg("ops")
    m = sahs.NeRFaceModel(sahs.default_config(name), precision="bf16x3")
    assert m.precision == ops.SAHS_BF16X3
    assert m.arch == ("nerface" if name == "expression" else "nerface_static")


def test_split_chain_predicate():
    ops = pkg("ops")
    assert ops.is_mixed("nerface", ops.SAHS_BF16X3)
    assert not ops.is_mixed("nerface_static", ops.SAHS_BF16X3)      # one whole-network launch
    assert ops.is_mixed("audio", ops.SAHS_BF16X3) and ops.is_mixed("nerface", ops.SAHS_BF16)
    assert not ops.is_mixed("nerface", ops.SAHS_F32) and not ops.is_mixed("nerface_static", ops.SAHS_BF16)


def test_new_symbols_are_exported():
    L = pkg("_lib")
    for name in ("sahs_model_field_forward_save_bits_x3", "sahs_model_field_forward_split_save_bits_x3"):
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    # every forward launcher the dispatch table (csrc/capi.hip: kModels) holds, for every model build: each build defines all of them
    for sfx in ("", "_nf", "_ns"):
        for family in ("sahs_field_f32_launch", "sahs_field_f32_sparse_launch", "sahs_field_f32_sparse_ws_bytes", "sahs_field_f32_sparse_ring_slots",
                       "sahs_field_bf16w_launch", "sahs_field_bf16x3_launch"):
            assert hasattr(L.lib(), family + sfx), family + sfx
