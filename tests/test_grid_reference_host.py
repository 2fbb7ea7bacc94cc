"""The instruments of tests/test_gpu_grid_edges.py, on the host: the position sets are what they claim to be, the float32 run of the
reference passes the comparisons the HIP kernels are held to, and the mutants of tests/grid_reference.py -- border padding,
align_corners=False, a sample's contribution missing from the grid gradient, the face samples' coordinate gradient taken in the
neighbouring cell -- fail them, tensor by tensor, at the bounds the GPU file uses.  A (set, tensor) pair no mutant fails on is a failure
of this file: the inputs have to change, not the bound."""
import pytest
import torch

import backward_reference as BR
import grid_reference as GR
from conftest import YARDSTICK_LOG, pkg

ARCHS = ("audio", "nerface", "nerface_static")
LEVEL = {"audio": 0, "nerface": 1, "nerface_static": 1}
CPU = torch.device("cpu")
# the loosest bound any fp32-arithmetic walk of the architecture is held to in tests/test_gpu_grid_edges.py
BOUND = {a: max(b for (arch, fwd, walk, prec), b in BR.FIELD_BOUNDS.items() if arch == a and fwd == "f32" and prec == "fp32") for a in ARCHS}

# the mutants that must fail, by construction of the sets: half_pixel moves every sample with a corner inside; border differs from zeros
# wherever a corner with a nonzero weight is outside (not in `faces`: the outside corner of a sample exactly on a face weighs 0);
# drop_one wherever sample 0 reaches the grid; inward wherever a +1 face is (at -1 the cell is the same one)
MUST_FAIL = {
    ("faces", "features"): {"half_pixel"}, ("faces", "grid"): {"half_pixel", "drop_one"}, ("faces", "coord"): {"half_pixel", "inward"},
    ("half_out", "features"): {"half_pixel", "border"}, ("half_out", "grid"): {"half_pixel", "border", "drop_one"}, ("half_out", "coord"): {"half_pixel", "border"},
    ("just_out", "features"): {"border"}, ("just_out", "grid"): {"border"}, ("just_out", "coord"): {"border"},
    ("far_out", "features"): {"border"},
    ("runs", "features"): {"half_pixel"}, ("runs", "grid"): {"half_pixel", "drop_one"}, ("runs", "coord"): {"half_pixel"},
    ("pile", "features"): {"half_pixel"}, ("pile", "grid"): {"half_pixel", "drop_one"}, ("pile", "coord"): {"half_pixel"},
}


def rejected(check):
    """whether `check` raises AssertionError; leaves no line in the session's yardstick log"""
    before = len(YARDSTICK_LOG)
    try:
        check()
        return False
    except AssertionError:
        return True
    finally:
        del YARDSTICK_LOG[before:]


def test_position_sets():
    sets = GR.position_sets()
    assert tuple(sets) == GR.SETS
    for ps in sets.values():
        GR.check_positions(ps)
        rays, z, x6 = GR.launch_inputs(ps, CPU)
        x = rays[:, 0:3].double() + rays[:, 3:6].double() * z.double()      # what reaches the kernel is the set's x, bit for bit
        assert torch.equal(x, torch.from_numpy(ps["x"])) and torch.equal(x6[:, :3].double(), x)
        assert torch.equal(torch.addcmul(rays[:, 0:3], rays[:, 3:6], z).double(), x)     # (the fused multiply-add's float32 result)
    sizes = {k: v["P"] for k, v in sets.items()}
    print("position sets:", sizes)
    assert sizes["pile"] == 512 and sizes["runs"] % 16 == 1 and all(p < 100 for k, p in sizes.items() if k != "pile")      # tens of samples each


def test_significant_bits():
    assert list(GR.significant_bits([0.0, 1.0, 0.75, 255.0 / 64, 257.0 / 64, 2.0 ** 20, 0.875 * 2.0 ** 128])) == [0, 1, 2, 8, 9, 1, 3]


def test_a_rounding_operand_is_refused():
    ps = dict(GR.position_sets()["faces"])
    ps["o"] = ps["o"] + 2.0 ** -12
    ps["x"] = ps["o"] + ps["d"] * ps["z"][:, None]
    with pytest.raises(AssertionError):
        GR.check_positions(ps)
    ps = dict(GR.position_sets()["runs"])
    ps["x"] = ps["x"].copy()
    ps["x"][3, 1] = 2.0 * 7 / 31 - 1.0 + 2.0 ** -16       # 2^-11 of a cell behind a lattice plane
    ps["o"] = ps["x"] - ps["d"] * ps["z"][:, None]
    with pytest.raises(AssertionError):
        GR.check_positions(ps)


@pytest.mark.parametrize("name", GR.SETS)
@pytest.mark.parametrize("arch", ARCHS)
def test_features_reference_and_mutants(arch, name):
    sd_np = GR.edge_state_dict(pkg("weights"), arch)
    x = GR.launch_inputs(GR.position_sets()[name], CPU)[2][:, :3]
    r64, r32 = GR.features(sd_np, arch, x, torch.float64), GR.features(sd_np, arch, x, torch.float32)
    what = "host %s %s features" % (arch, name)
    GR.feature_check(r32, r32, r64, name, what)
    if name in GR.ZERO_SETS:
        assert float(r32.abs().max()) == 0.0
    else:
        assert float(r64.abs().min(1).values.max()) > 0.0
    failed = {m for m in ("border", "half_pixel") if rejected(lambda: GR.feature_check(GR.features(sd_np, arch, x, torch.float64, m).float(), r32, r64, name, what))}
    print("%s: mutants rejected: %s" % (what, sorted(failed)))
    assert failed >= MUST_FAIL[(name, "features")], "%s: not rejected: %s" % (what, sorted(MUST_FAIL[(name, "features")] - failed))


@pytest.mark.parametrize("name", GR.BACKWARD_SETS)
@pytest.mark.parametrize("arch", ARCHS)
def test_backward_reference_and_mutants(arch, name):
    c = GR.make_case(pkg("weights"), arch, name, LEVEL[arch], CPU, GR.host_frame(arch))
    masks = GR.reference_masks(c)
    ref = BR._eager(c, masks, 0, c["P"])
    got32 = BR._eager(c, masks, 0, c["P"], dtype=torch.float32)
    bound = BOUND[arch]
    what = "host %s %s backward" % (arch, name)
    fails, errs = GR.backward_check(got32, ref, bound, arch, ref32=got32)
    print("%s: float32 reference, worst %s (bound %.1e)" % (what, ", ".join("%s %.2e" % kv for kv in sorted(errs.items(), key=lambda kv: -kv[1])[:3]), bound))
    assert not any(fails.values()), "%s: the float32 reference fails its own comparison: %s" % (what, fails)
    if "warp_field_mlp.fc_final.weight" in ref:      # x' = x: the warp head's own gradient carries d loss / d x'
        assert float(ref["warp_field_mlp.fc_final.bias"].abs().max()) > 0.0
    groups = ("grid", "coord") if arch != "nerface_static" else ("grid",)      # (no deformation nets: nothing receives d x')
    table = {g: set() for g in groups}
    for m, grads in GR.mutants(c, masks, ref).items():
        mf, me = GR.backward_check(grads, ref, bound, arch, ref32=got32)
        for g in groups:
            if mf[g]:
                table[g].add(m)
        print("%s: mutant %-10s worst %s" % (what, m, ", ".join("%s %.2e" % kv for kv in sorted(me.items(), key=lambda kv: -kv[1])[:3])))
    print("%s: mutants rejected: %s" % (what, {g: sorted(v) for g, v in table.items()}))
    for g in groups:
        assert table[g], "%s: no mutant fails on the %s tensors: change the inputs" % (what, g)
        assert table[g] >= MUST_FAIL[(name, g)], "%s, %s: not rejected: %s" % (what, g, sorted(MUST_FAIL[(name, g)] - table[g]))
