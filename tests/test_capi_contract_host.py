"""The C ABI's answers pinned as literals, no GPU needed: every size query over a grid of arguments, and the return code of the
forward, saving, backward and render entry points for inputs that are rejected (or short-circuit) before any kernel runs.

The values were recorded from the library as it stood before its dispatch moved into one table per model
(csrc/capi.hip: kModels); a change to any of them is a change of the ABI's behaviour, not a refactor.  The sparse render entry's
(SPARSE_CASES) were recorded at commit 0c084c6, before the field forward launchers took one argument block."""
import pytest
import torch

from conftest import pkg

MODELS = (-1, 0, 1, 2, 3)
PRECISIONS = (-1, 0, 1, 2, 3, 4)
PARTS = (-1, 0, 1, 2, 3, 4)
SIZES = (0, 1, 4096)


def _queries(L):
    """(a): every size query of the ABI over the grid, in a fixed order"""
    out = {
        "param_count": [L.sahs_param_count()] + [L.sahs_model_param_count(m) for m in MODELS],
        "frame_words": [L.sahs_frame_words()] + [L.sahs_model_frame_words(m) for m in MODELS],
        "act_words_per_sample": [L.sahs_act_words_per_sample()] + [L.sahs_model_act_words_per_sample(m) for m in MODELS],
        "packed_words": [[L.sahs_packed_words(p) for p in PRECISIONS]] + [[L.sahs_model_packed_words(m, p) for p in PRECISIONS] for m in MODELS],
        "macs_per_sample": [[L.sahs_model_executed_macs_per_sample(m, p) for p in PRECISIONS] for m in MODELS],
        "macs_part": [[[L.sahs_model_executed_macs_part(m, p, q) for q in PARTS] for p in PRECISIONS] for m in MODELS],
        "act_words_part": [[L.sahs_model_act_words_part(m, q) for q in PARTS] for m in MODELS],
        "bits_words_part": [[L.sahs_model_bits_words_part(m, q) for q in PARTS] for m in MODELS],
        "bwd_ws_words": [[L.sahs_field_backward_workspace_words(P) for P in SIZES]] +
                        [[L.sahs_model_field_backward_workspace_words(m, P) for P in SIZES] for m in MODELS],
        "fused_ws_words": [[[L.sahs_model_field_backward_fused_workspace_words(m, q, P) for P in SIZES] for q in PARTS] for m in MODELS],
    }
    return out


EXPECTED_QUERIES = {'act_words_part': [[-1, -1, -1, -1, -1, -1], [-1, 4752, 1264, 3504, 4752, -1], [-1, 3792, 1296, 2512, 3792, -1], [-1, 3696, 1264, 2448, 3696, -1],
                                       [-1, -1, -1, -1, -1, -1]],
                    'act_words_per_sample': [4752, -1, 4752, 3792, 3696, -1],
                    'bits_words_part': [[0, 0, 0, 0, 0, 0], [0, 144, 48, 96, 144, 0], [0, 112, 48, 64, 112, 0], [0, 64, 0, 64, 64, 0], [0, 0, 0, 0, 0, 0]],
                    'bwd_ws_words': [[4218944, 4219860, 7970880], [-1, -1, -1], [4218944, 4219860, 7970880], [4218944, 4219892, 8101952], [4218944, 4219828, 7839808],
                                     [-1, -1, -1]],
                    'frame_words': [9184, -1, 9184, 7136, 4768, -1],
                    'fused_ws_words': [[[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]],
                                       [[-1, -1, -1], [-1, -1, -1], [122880, 124136, 5267456], [2908224, 2911960, 18210880], [3031104, 3036104, 23511104], [-1, -1, -1]],
                                       [[-1, -1, -1], [-1, -1, -1], [122880, 124168, 5398528], [2646080, 2648888, 14147648], [2768960, 2773064, 19578944], [-1, -1, -1]],
                                       [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [2580544, 2583160, 13295680], [-1, -1, -1]],
                                       [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]],
                    'macs_part': [[[-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1],
                                   [-1, -1, -1, -1, -1, -1]],
                                  [[-1, -1, -1, -1, -1, -1], [-1, 883712, 130048, 753664, -1, -1], [-1, 894976, 133120, 761856, -1, -1],
                                   [-1, 894976, 133120, 761856, -1, -1], [-1, 2684928, 399360, 2285568, -1, -1], [-1, -1, -1, -1, -1, -1]],
                                  [[-1, -1, -1, -1, -1, -1], [-1, 650240, 142336, 507904, -1, -1], [-1, 952320, 436224, 516096, -1, -1],
                                   [-1, 661504, 145408, 516096, -1, -1], [-1, 1984512, 436224, 1548288, -1, -1], [-1, -1, -1, -1, -1, -1]],
                                  [[-1, -1, -1, -1, -1, -1], [-1, 475136, 0, 475136, -1, -1], [-1, 483328, 0, 483328, -1, -1], [-1, 483328, 0, 483328, -1, -1],
                                   [-1, 1449984, 0, 1449984, -1, -1], [-1, -1, -1, -1, -1, -1]],
                                  [[-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1],
                                   [-1, -1, -1, -1, -1, -1]]],
                    'macs_per_sample': [[-1, -1, -1, -1, -1, -1], [-1, 883712, 894976, 894976, 2684928, -1], [-1, 650240, 952320, 661504, 1984512, -1],
                                        [-1, 475136, 483328, 483328, 1449984, -1], [-1, -1, -1, -1, -1, -1]],
                    'packed_words': [[-1, 2816120, 1943600, -1, 5654648, -1], [-1, -1, -1, -1, -1, -1], [-1, 2816120, 1943600, -1, 5654648, -1],
                                     [-1, 2349144, 6430848, -1, 4720728, -1], [-1, 1998912, 1531928, -1, 2015232, -1], [-1, -1, -1, -1, -1, -1]],
                    'param_count': [2775633, -1, 2775633, 2311140, 2066976, -1]}


def test_size_queries():
    assert _queries(pkg("_lib").lib()) == EXPECTED_QUERIES


# ---- (b) return codes ----
A = 1 << 20          # a fabricated, 16-byte aligned device address: never dereferenced (these cases skip when a GPU is present)
M = A + 4            # ... and a misaligned one
BIG = 4000001        # samples: one over the cap of the entry points that have one

ARGS = {
    "sahs_field_forward": "packed frame level N S rays ray_stride z raw dbg precision stream",
    "sahs_model_field_forward": "model packed frame level N S rays ray_stride z raw dbg precision stream",
    "sahs_model_field_forward_split": "model packed frame precision level mode N S rays ray_stride z raw xw xw_row xw_col0 src stream",
    "sahs_field_forward_save": "packed frame level N S rays ray_stride z raw act stream",
    "sahs_model_field_forward_save": "model packed frame level N S rays ray_stride z raw act stream",
    "sahs_model_field_forward_save_bits": "model packed frame level N S rays ray_stride z raw act bits stream",
    "sahs_model_field_forward_save_bits_x3": "model packed frame level N S rays ray_stride z raw act bits stream",
    "sahs_model_field_forward_split_save": "model packed frame level mode N S rays ray_stride z raw xw xw_row xw_col0 src act stream",
    "sahs_model_field_forward_split_save_bits": "model packed frame level mode N S rays ray_stride z raw xw xw_row xw_col0 src act bits stream",
    "sahs_model_field_forward_split_save_bits_x3": "model packed frame level mode N S rays ray_stride z raw xw xw_row xw_col0 src act bits stream",
    "sahs_field_backward": "flat frame level P act d_raw grad_flat grad_cond ws stream",
    "sahs_model_field_backward": "model flat frame level P act d_raw grad_flat grad_cond ws stream",
    "sahs_model_field_backward_split": "model flat frame level part P act d_raw xwg_in xwg_out grad_flat grad_cond ws stream",
    "sahs_model_field_backward_fused": "model flat frame level part P act bits d_raw xwg_in xwg_out grad_flat grad_cond ws stream",
    "sahs_pack_weights": "flat packed precision stream",
    "sahs_model_pack_weights": "model flat packed precision stream",
    "sahs_render_rays": "packed frame precision N rays ray_stride Sc nf lindisp white bg t_rand noise_c u noise_f z_c z_f raw weights "
                        "rgb_c disp_c acc_c rgb_f disp_f acc_f w_bg depth_f stream",
    "sahs_model_render_rays": "model packed frame precision N rays ray_stride Sc nf lindisp white bg t_rand noise_c u noise_f z_c z_f raw "
                              "weights rgb_c disp_c acc_c rgb_f disp_f acc_f w_bg depth_f stream",
    "sahs_model_render_rays_rows": "model packed frame precision N rays ray_stride Sc nf lindisp white bg t_rand noise_c u noise_f z_c z_f raw "
                                   "weights rows row_ld xw src z_new stream",
    "sahs_model_render_rays_rows_sparse": "model packed frame precision N rays ray_stride Sc nf lindisp white bg t_rand noise_c u noise_f z_c z_f "
                                          "raw weights rows row_ld xw src z_new ws ws_bytes stream",
}
SPARSE = "sahs_model_render_rays_rows_sparse"      # (its cases are a list of their own, SPARSE_CASES: the first list's literal stays as recorded)
# every argument not named in a case: a valid shape (one ray of one sample, level 0, mode 0, part 3, fp32) and, for pointers, null
DEFAULTS = dict(model=0, level=0, N=1, S=1, P=1, ray_stride=8, precision=0, mode=0, part=3, xw_row=1, xw_col0=0, Sc=1, nf=0, lindisp=0,
                white=0, row_ld=16)
ALL_PTRS = dict(packed=A, frame=A, rays=A, z=A, raw=A, act=A, bits=A, xw=A, src=A, flat=A, d_raw=A, xwg_in=A, xwg_out=A, grad_flat=A,
                grad_cond=A, ws=A, z_c=A, z_f=A, weights=A, rgb_c=A, disp_c=A, acc_c=A, rgb_f=A, disp_f=A, acc_f=A, w_bg=A, depth_f=A,
                rows=A, z_new=A)


def _call(L, name, kw):
    vals = dict(DEFAULTS, **kw)
    if name == SPARSE:      # ws_bytes: what the ABI's query asks for the render's larger pass, `ws_records` records more (negative: fewer)
        m = vals["model"]
        record = (L.sahs_model_render_sparse_workspace_bytes(m, 128) - L.sahs_model_render_sparse_workspace_bytes(m, 0)) // 128
        vals["ws_bytes"] = max(0, L.sahs_model_render_sparse_fused_workspace_bytes(m, vals["N"] * (vals["Sc"] + vals["nf"])) + record * vals.get("ws_records", 0))
    return getattr(L, name)(*[vals.get(a, None) for a in ARGS[name].split()])


def _cases():
    """(function, arguments) of every return-code case, in a fixed order; `ptrs`: every pointer fabricated and aligned (then
    overridden per case)"""
    MODEL_FNS = [n for n in ARGS if n.startswith("sahs_model_") and n != SPARSE]
    SAVES = ["sahs_model_field_forward_save", "sahs_model_field_forward_save_bits", "sahs_model_field_forward_save_bits_x3"]
    SPLIT_SAVES = ["sahs_model_field_forward_split_save", "sahs_model_field_forward_split_save_bits", "sahs_model_field_forward_split_save_bits_x3"]
    FWDS = ["sahs_model_field_forward", "sahs_model_field_forward_split"] + SAVES + SPLIT_SAVES
    BWDS = ["sahs_model_field_backward", "sahs_model_field_backward_split", "sahs_model_field_backward_fused"]
    cases = []
    def c(name, **kw): cases.append((name, kw))
    def cp(name, **kw): cases.append((name, dict(ptrs=True, **kw)))
    # unknown model: before anything else
    for n in MODEL_FNS:
        for m in (-1, 3):
            c(n, model=m)
    # the model without deformation nets on a split / deformation call
    for n in ["sahs_model_field_forward_split"] + SPLIT_SAVES:
        for mode in (0, 1, 2):
            c(n, model=2, mode=mode)
            cp(n, model=2, mode=mode)
        c(n, model=2, N=0)
    for n in ["sahs_model_field_backward_split", "sahs_model_field_backward_fused"]:
        for part in (0, 1, 2):
            c(n, model=2, part=part)
            cp(n, model=2, part=part)
    for m in (0, 1):
        c("sahs_model_field_forward_save_bits_x3", model=m)
        c("sahs_model_field_forward_save_bits_x3", model=m, N=0)
    # N = 0 / P = 0
    for m in (0, 1, 2):
        for n in FWDS + ["sahs_model_render_rays", "sahs_model_render_rays_rows"]:
            c(n, model=m, N=0)
            cp(n, model=m, N=0, mode=1 if n.endswith("_x3") and "split" in n else 0)
        for n in BWDS:
            cp(n, model=m, P=0)
            c(n, model=m, P=0)
    for n in ["sahs_field_forward", "sahs_field_forward_save", "sahs_render_rays"]:
        c(n, N=0); cp(n, N=0)
    cp("sahs_field_backward", P=0); c("sahs_field_backward", P=0)
    # null pointers with a valid shape
    for m in (0, 1, 2):
        for n in FWDS + BWDS + ["sahs_model_pack_weights", "sahs_model_render_rays", "sahs_model_render_rays_rows"]:
            c(n, model=m)
    for n in ["sahs_field_forward", "sahs_field_forward_save", "sahs_field_backward", "sahs_pack_weights", "sahs_render_rays"]:
        c(n)
    # precision not built (or an unknown id)
    for p in (-1, 1, 2, 3, 4):
        cp("sahs_field_forward", precision=p)
        cp("sahs_pack_weights", precision=p)
        for m in (0, 1, 2):
            cp("sahs_model_field_forward", model=m, precision=p)
            cp("sahs_model_pack_weights", model=m, precision=p)
            for mode in (0, 1, 2):
                cp("sahs_model_field_forward_split", model=m, precision=p, mode=mode, xw_row=2)
    # bad level / mode / part / shape
    for n in ["sahs_field_forward", "sahs_field_forward_save"] + ["sahs_model_field_forward"] + SAVES + SPLIT_SAVES + ["sahs_model_field_forward_split"]:
        for kw in (dict(level=2), dict(level=-1), dict(S=0), dict(N=-1), dict(ray_stride=7)):
            cp(n, model=1, mode=1, **kw) if n.startswith("sahs_model") else cp(n, **kw)
    for n in SPLIT_SAVES + ["sahs_model_field_forward_split"]:
        for m in (0, 1):
            for mode in (-1, 0, 3):
                cp(n, model=m, mode=mode)
            cp(n, model=m, mode=1, xw_col0=-1)
            cp(n, model=m, mode=1, xw_row=0)
            cp(n, model=m, mode=2, src=0)
            cp(n, model=m, mode=1, z=0)
            cp(n, model=m, mode=2, raw=0)
        cp("sahs_model_field_forward_split", model=1, precision=1, mode=0, xw_col0=1, xw_row=4)
        cp("sahs_model_field_forward_split", model=0, precision=3, mode=2, src=0)
        cp("sahs_model_field_forward_split", model=1, precision=1, mode=2, src=0)
    for n in ["sahs_field_backward"] + BWDS:
        for kw in (dict(level=2), dict(level=-1), dict(P=-1), dict(part=0), dict(part=4), dict(part=-1), dict(part=1, xwg_in=0), dict(part=2, xwg_out=0),
                   dict(part=2, d_raw=0), dict(part=1, d_raw=0)):
            for m in (0, 1, 2):
                cp(n, model=m, **kw)
    # misaligned buffers
    for key in ("packed", "frame", "raw", "dbg", "act", "bits", "xw", "z", "rays"):
        cp("sahs_field_forward", **{key: M}); cp("sahs_field_forward_save", **{key: M})
        for m in (0, 1, 2):
            for n in ["sahs_model_field_forward"] + SAVES:
                cp(n, model=m, **{key: M})
            for n in SPLIT_SAVES + ["sahs_model_field_forward_split"]:
                cp(n, model=m, mode=1 if n.endswith("_x3") else 0, **{key: M})
    for key in ("act", "bits", "ws", "d_raw", "xwg_in", "xwg_out", "flat"):
        for n in ["sahs_field_backward"] + BWDS:
            cp(n, model=1, **{key: M})
    cp("sahs_pack_weights", packed=M)
    for m in (0, 1, 2):
        for p in (0, 1, 3):
            cp("sahs_model_pack_weights", model=m, precision=p, packed=M)
    # more than 4e6 samples
    for m in (0, 1, 2):
        for n in SAVES + SPLIT_SAVES:
            for mode in (0, 1, 2):
                cp(n, model=m, N=BIG, mode=mode)
        for n in BWDS:
            cp(n, model=m, P=BIG)
            cp(n, model=m, P=BIG, part=1)
    cp("sahs_field_forward_save", N=BIG); cp("sahs_field_backward", P=BIG)
    # render entry points
    for m in (0, 1, 2):
        for p in (0, 1, 3):
            cp("sahs_model_render_rays_rows", model=m, precision=p, xw=0, nf=1)
            cp("sahs_model_render_rays_rows", model=m, precision=p, nf=0)
            cp("sahs_model_render_rays_rows", model=m, precision=p, row_ld=15)
            cp("sahs_model_render_rays_rows", model=m, precision=p, rows=0)
            cp("sahs_model_render_rays_rows", model=m, precision=p, nf=1, Sc=256)
            cp("sahs_model_render_rays_rows", model=m, precision=p, nf=1, packed=0)
            cp("sahs_model_render_rays", model=m, precision=p, nf=1, z_f=0)
            cp("sahs_model_render_rays", model=m, precision=p, w_bg=0)
    cp("sahs_render_rays", nf=1, z_f=0); cp("sahs_render_rays", depth_f=0)

    return _unique(cases)


def _unique(cases):
    out, seen = [], set()
    for name, kw in cases:
        key = (name, tuple(sorted(kw.items())))
        if key not in seen:
            seen.add(key)
            out.append((name, kw))
    return out


def _sparse_cases():
    """the sparse render entry: the checks it shares with sahs_model_render_rays_rows, then those of its record workspace"""
    cases = []
    def c(**kw): cases.append((SPARSE, dict(dict(row_ld=36), **kw)))      # (36: a full row, SAHS_ROW_COLUMNS)
    def cp(**kw): c(ptrs=True, **kw)
    for m in (-1, 3):      # unknown model: before anything else
        c(model=m); cp(model=m); c(model=m, N=0); cp(model=m, precision=1)
    for m in (0, 1, 2):
        c(model=m, N=0); cp(model=m, N=0); cp(model=m, N=0, nf=1, Sc=256)
        c(model=m); c(model=m, nf=1)      # null pointers with a valid shape
        cp(model=m); cp(model=m, nf=1); cp(model=m, nf=1, N=300, Sc=64, ws_records=1)      # a workspace that fits: the first launch
        for key in ("rows", "packed", "frame", "rays", "z_c", "raw", "weights", "z_f", "ws", "xw", "src", "z_new", "bg"):
            cp(model=m, nf=1, **{key: 0})
        cp(model=m, z_f=0)
        for key in ("packed", "frame", "raw", "xw", "ws", "rays", "z_c", "rows"):
            cp(model=m, nf=1, **{key: M})
        for kw in (dict(row_ld=35), dict(N=-1), dict(Sc=0), dict(nf=-1), dict(ray_stride=7), dict(nf=1, Sc=256), dict(nf=0, Sc=256), dict(nf=0, Sc=257)):
            cp(model=m, **kw)
        for p in (-1, 1, 2, 3, 4):      # no sparse branches in the other precisions: sahs_model_render_rays_rows answers
            cp(model=m, precision=p, nf=1); cp(model=m, precision=p, nf=1, xw=0); cp(model=m, precision=p, nf=1, Sc=256); cp(model=m, precision=p, rows=0)
            c(model=m, precision=p, N=0)
        # a workspace one record short of its rings, coarse pass alone and both passes; none at all; a pass over 2^30 samples
        cp(model=m, ws_records=-1); cp(model=m, nf=1, N=300, Sc=64, ws_records=-1); cp(model=m, ws_records=-10 ** 6)
        cp(model=m, N=(1 << 22) + 1, Sc=256); cp(model=m, N=(1 << 23), Sc=128, nf=1); cp(model=m, N=(1 << 22), Sc=256)
    return _unique(cases)


CASES = _cases()
SPARSE_CASES = _sparse_cases()
# one character per case: the code returned, or L = validation passed and a launch was attempted (no GPU here: a HIP error, 100 + e)
EXPECTED_CODES = (
    "3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 3 4 4 4 4 4 4 0 4 4 4 4 4 4 0 4 4 4 4 4 4 4 4 4 4 4 4 4 4 1 L 1 4 1 4 4 4 4 4 4 4 4 4 "
    "4 4 0 0 0 0 1 0 1 0 4 0 0 0 0 0 0 0 0 0 0 0 1 0 1 0 1 0 0 0 0 1 0 1 0 4 0 0 0 0 0 0 0 0 0 0 0 1 0 1 0 1 0 0 0 1 0 1 0 1 0 0 4 4 0 0 0 0 0 1 "
    "0 1 0 1 0 0 1 0 0 0 0 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 4 1 1 1 4 4 4 1 1 1 1 1 1 1 1 1 1 1 2 2 2 2 4 4 4 2 2 4 4 4 2 "
    "2 4 4 4 L L L L L L L 2 L L L L L L 4 4 4 2 2 2 2 4 4 4 2 2 4 4 4 2 2 4 4 4 2 L 2 L L L L 2 L L L L L L 4 4 4 2 2 2 2 4 4 4 2 2 4 4 4 2 2 4 "
    "4 4 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 4 4 4 4 4 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L 1 1 1 1 1 1 1 L 1 1 1 1 1 1 1 L "
    "L 1 L 1 1 1 1 1 1 1 L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L 1 1 1 1 1 1 1 L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L L L L L L L L L L L L "
    "L L L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L L L L L L L L L L L L L L L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 L L 4 1 1 "
    "1 1 1 1 1 1 1 1 1 1 1 4 1 1 4 1 1 4 1 1 4 1 1 4 L L 4 1 1 1 1 1 4 1 1 1 1 1 1 1 4 1 1 1 1 1 1 1 1 4 4 4 4 1 1 1 1 1 4 1 1 1 1 1 1 1 4 1 1 1 "
    "1 1 1 1 1 4 4 4 4 1 1 1 1 1 4 1 1 1 1 1 1 1 4 1 1 1 1 1 1 1 1 4 4 4 4 1 L 1 L L 4 L L L L 1 L L 4 L L L L 1 L L L 4 4 4 4 L 1 L 1 1 4 1 1 1 "
    "L L 1 1 4 1 1 1 L L 1 1 1 4 4 4 4 L L L L 1 4 L 1 1 L L L 1 4 L 1 1 L L L 1 1 4 4 4 4 L L L L L 4 1 1 1 1 L L L 4 1 1 1 1 L L L L 4 4 4 4 L "
    "L L L L 4 L L L L L L L 4 L L L L L L L L 4 4 4 4 L L L L L 4 L L L L L L L 4 L L L L L L L L 4 4 4 4 L L L 1 L L L 1 L L L 1 L L L 1 L L L "
    "1 L L L 1 L L L L 1 1 1 1 1 1 1 1 1 1 L L L 1 1 1 4 4 4 L L L 1 1 1 1 1 1 1 1 1 1 1 1 L L L 1 1 1 4 4 4 L L L 1 1 1 1 1 1 1 1 1 1 1 1 L L L "
    "1 1 1 1 1 1 4 4 4 4 4 4 4 4 4 1 1 1 1 1 4 L 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 "
    "1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 1 ")


EXPECTED_SPARSE_CODES = (
    "3 3 3 3 3 3 3 3 0 0 0 1 1 L L L 1 1 1 1 1 1 1 1 1 L L L L L 1 1 1 1 1 L L L 1 1 1 1 1 1 L 1 L L L 1 0 L L 1 1 0 L L L 1 0 L 1 1 1 0 L L L 1 "
    "0 5 5 5 5 5 L 0 0 0 1 1 L L L 1 1 1 1 1 1 1 1 1 L L L L L 1 1 1 1 1 L L L 1 1 1 1 1 1 L 1 L L L 1 0 L 1 1 1 0 L L L 1 0 L 1 1 1 0 L L L 1 0 "
    "5 5 5 5 5 L 0 0 0 1 1 L L L 1 1 1 1 1 1 1 1 1 L L L L L 1 1 1 1 1 L L L 1 1 1 1 1 1 L 1 L L L 1 0 L L L 1 0 L L L 1 0 L L L 1 0 L L L 1 0 5 "
    "5 5 5 5 L ")


def _codes(L, fabricated, cases):
    out = []
    for name, kw in cases:
        kw = dict(kw)
        if kw.pop("ptrs", False) != fabricated:
            continue
        if fabricated:
            kw = dict(ALL_PTRS, **kw)
        r = _call(L, name, kw)
        out.append((name, kw, "L" if r >= 100 else str(r) if 0 <= r <= 9 else "?%d" % r))
    return out


def _check(fabricated, cases=CASES, expected=EXPECTED_CODES):
    assert len(cases) == len(expected.split())
    want = [w for (_, kw), w in zip(cases, expected.split()) if bool(kw.get("ptrs")) == fabricated]
    got = _codes(pkg("_lib").lib(), fabricated, cases)
    assert len(got) == len(want)
    bad = ["%s(%s): %s, expected %s" % (n, kw, g, w) for (n, kw, g), w in zip(got, want) if g != w]
    assert not bad, "\n".join(bad[:20])


def test_return_codes_null_pointers():
    """cases that fail (or return) before the pointers are looked at"""
    _check(False)


def test_return_codes_fabricated_pointers():
    if torch.cuda.is_available():
        pytest.skip("fabricated device pointers are only passed where no GPU can run a kernel")
    _check(True)


def test_sparse_render_return_codes_null_pointers():
    _check(False, SPARSE_CASES, EXPECTED_SPARSE_CODES)


def test_sparse_render_return_codes_fabricated_pointers():
    if torch.cuda.is_available():
        pytest.skip("fabricated device pointers are only passed where no GPU can run a kernel")
    _check(True, SPARSE_CASES, EXPECTED_SPARSE_CODES)
