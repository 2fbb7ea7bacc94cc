"""The fp32 field forward at its two chunk caps: the instance that saves activations against the one that does not, bit for bit.

field_forward_f32_kernel<SAVE, MODE> streams its weights into two LDS buffers whose size is the instance's chunk cap (csrc/field_f32.hip:
field_chunk_cap): 32 KB where activations are saved (the training forward), 64 KB where they are not (the inference forward).  A chunking
is a schedule -- which tiles of a layer share a barrier, how many DMA pieces a chunk has, where in LDS the biases and the stash sit --
and not arithmetic: the k-order of every accumulation chain is the same under both.  So the two instances of a mode, given the same
samples, must write the same raw rows and the same x', w, bit for bit, and any slip of the schedule (a chunk read before its last piece
landed, a buffer parity lost across a wrap, a piece count off by one) shows as a difference between them.

Through the Python entry points of the two forwards, per architecture, level and mode:
  FIELD_ALL       ops.field_forward_split        vs ops.field_forward_split_save        raw, and x', w in xw
  FIELD_DEFORM    the same two                                                           x', w in xw
  FIELD_RADIANCE  the same two, reading one xw through a permuting src                   raw
  the NeRFaceModel without deformation nets has the whole network only: ops.field_forward vs ops.field_forward_save, raw.
At three sample counts (CUs = the device's compute units, one persistent workgroup each, 128-sample tiles):
  one           P = 1
  wrap_to_one   P = 128 CUs + 1        one workgroup wraps the stream into a second tile that holds one sample
  three_ragged  P = 3 x 128 CUs + 129  every workgroup runs at least three tiles and the last tile is ragged: both buffer parities and
                                       every chunk size (the 4-8 KB chunks of the one-tile layers included) recur behind a wrap
The compared values must be finite and not all equal; xw buffers are compared whole, NaN prefill included (a launch writes five floats
of its own slots and nothing else).

Run first on the commit before the caps were split, where both instances use 32 KB chunks: 9 passed (2.4 s on a 256-CU MI355X); then on
the 64 KB / 32 KB pair, also with the fragment reads of the 64 KB instances pinned 3, 4 and 5 deep: 9 passed each time.
"""
import pytest
import torch

import field_reference as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

TILE = FR.TILE["fp32"]
SIZES = {"one": lambda cus: 1, "wrap_to_one": lambda cus: TILE * cus + 1, "three_ragged": lambda cus: 3 * TILE * cus + TILE + 1}
XW_PAD, XW_COL0 = 5, 3      # xw rows hold S + 5 slots; the launches own columns 3 .. 3 + S - 1
_MODELS = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def model(arch):
    if arch not in _MODELS:
        ops, W = pkg("ops"), pkg("weights")
        flat = torch.from_numpy(W.flatten_state_dict(FR.state_dict_np(W, arch), model=arch)).to(dev())
        frame = ops.fold_conditioning(flat, FR.driving_input(arch, dev()), FR.pose_of(arch, dev()), arch=arch)
        _MODELS[arch] = dict(frame=frame, packed=ops.pack_weights(flat, ops.SAHS_F32, arch=arch))
    return _MODELS[arch]


def nan(*shape):
    return torch.full(shape, float("nan"), device=dev())


def meaningful(t, what):
    """the compared values are finite and not all equal"""
    assert bool(torch.isfinite(t).all()), what + ": not finite"
    assert float(t.min()) != float(t.max()), what + ": all values equal"


def same(a, b, what):
    FR.assert_same_bits(a, b, what + ": 64 KB chunks (no save) vs 32 KB chunks (saving)")


def split_pair(arch, level, mode, rays, z, xw_in=None, src=None):
    """one mode through the inference forward and through the training forward -> (raw, xw) of each (raw None for FIELD_DEFORM; xw the
    buffer the launch wrote, None for FIELD_RADIANCE, which reads xw_in)"""
    ops, m = pkg("ops"), model(arch)
    N, S = rays.shape[0], (src if mode == ops.FIELD_RADIANCE else z).shape[1]
    out = []
    for saving in (False, True):
        xw = xw_in if mode == ops.FIELD_RADIANCE else nan(N, S + XW_PAD, 8)
        kw = dict(z=z, src=src, xw_col0=0 if mode == ops.FIELD_RADIANCE else XW_COL0, arch=arch)
        if saving:
            raw, _ = ops.field_forward_split_save(m["packed"], m["frame"], level, mode, rays, xw, bits=ops.alloc_sign_bits(N * S, mode, arch, dev()), **kw)
        else:
            raw = ops.field_forward_split(m["packed"], m["frame"], level, mode, rays, xw, **kw)
        out.append((raw, None if mode == ops.FIELD_RADIANCE else xw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_saving_and_plain_forward_agree(arch, size):
    ops = pkg("ops")
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    P = SIZES[size](cus)
    N, S = FR.factor(P)
    rays, z, _ = FR.build_scene(arch, N, S, dev())
    print("%s %s: P=%d (N=%d x S=%d), %d tiles of %d on %d CUs" % (arch, size, P, N, S, -(-P // TILE), TILE, cus))
    for level in (0, 1):
        what = "%s %s level %d" % (arch, size, level)
        if not FR.ARCH_DIMS[arch]["deform"]:      # whole network only
            m = model(arch)
            plain = ops.field_forward(m["packed"], m["frame"], level, rays, z, arch=arch)
            saved, _ = ops.field_forward_save(m["packed"], m["frame"], level, rays, z, arch, bits=ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, dev()))
            torch.cuda.synchronize()
            meaningful(plain, what + " raw")
            same(plain.reshape(P, 16), saved.reshape(P, 16), what + " raw")
            continue
        own = slice(XW_COL0, XW_COL0 + S)
        (raw_a, xw_a), (raw_b, xw_b) = split_pair(arch, level, ops.FIELD_ALL, rays, z)
        meaningful(raw_a, what + " FIELD_ALL raw")
        meaningful(xw_a[:, own, :5], what + " FIELD_ALL x', w")
        same(raw_a.reshape(P, 16), raw_b.reshape(P, 16), what + " FIELD_ALL raw")
        same(xw_a, xw_b, what + " FIELD_ALL xw")
        (_, xd_a), (_, xd_b) = split_pair(arch, level, ops.FIELD_DEFORM, rays, z)
        meaningful(xd_a[:, own, :5], what + " FIELD_DEFORM x', w")
        same(xd_a, xd_b, what + " FIELD_DEFORM xw")
        src = (FR.ray_permutation(N, S, dev()) + XW_COL0).contiguous()
        (rr_a, _), (rr_b, _) = split_pair(arch, level, ops.FIELD_RADIANCE, rays, None, xw_in=xw_a, src=src)
        meaningful(rr_a, what + " FIELD_RADIANCE raw")
        same(rr_a.reshape(P, 16), rr_b.reshape(P, 16), what + " FIELD_RADIANCE raw")
