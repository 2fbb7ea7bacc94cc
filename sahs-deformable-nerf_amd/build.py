"""Build the C-ABI HIP library (libsahs_nerf.so) in-tree for gfx950.

hipcc cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box with the
working tree.  ``python -m`` style use: ``python sahs-deformable-nerf_amd/build.py [--force]``.

One table (UNITS) says what is compiled and how; build() is five steps over it: plan() the compiler runs, run them in a bounded pool,
hold every kernel to its scratch allowance, check the hand-scheduled kernels' ISA, link.
"""
import collections
import os
import re
import subprocess
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsahs_nerf.so")
CHECKER = os.path.join(HERE, "..", "tools", "check_lds_inflight.py")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-Wall", "-Wno-unused-function"]

# One translation unit of the library: its source in csrc/, the models it is built for, its own flags (fp: floating-point semantics,
# tune: code generation; a command is FLAGS, fp, -DSAHS_MODEL, tune, the caller's defines -- the order the objects have always been
# built with) and, per model, the name patterns of its hand-scheduled kernels.
Unit = collections.namedtuple("Unit", "src models fp tune hand", defaults=((), (), {}))
ONCE = (0,)
# built again for the NeRFaceModel architectures (csrc/sahs_model.hpp: -DSAHS_MODEL=1 / 2, symbols suffixed _nf / _ns)
EVERY_MODEL = (0, 1, 2)
# field kernels: no sNaN-quieting v_max before every fmaxf (activations); NaNs still propagate through the MFMAs
FIELD = ("-fno-honor-nans", "-mno-amdgpu-ieee")
# No SLP vectorisation: left on, the compiler packs the operand splits' subtractions into v_pk_add_f32, which is an anti-lever beside
# MFMAs on this chip (MI355X_MICROARCH.md); without it the training step is 1.1 % faster (same-box A/B: 17.95 -> 17.75 ms).  The
# forward kernels measure neutral (+-0.5 %) and keep the default.
NO_SLP = ("-fno-slp-vectorize",)
# MFMA accumulators must live in ARCH VGPRs (one wave per SIMD, 512 registers).  Left to its heuristics the compiler puts them in AGPRs,
# and every accumulator value the activation code touches then costs a v_accvgpr_read -- which, unlike plain VALU work, does NOT hide
# under the wave's own MFMAs (tools/micro/mfma_valu_overlap.hip: 2 reads per MFMA = 55 cycles per MFMA instead of 36).
ARCH_ACC = ("-mllvm", "-amdgpu-mfma-vgpr-form=1")
# `hand`: kernels with hand-issued `asm volatile ds_read_b128` + counted waits (csrc/bf16_pipe.hpp).  Every build compiles their unit
# to ISA as well and runs tools/check_lds_inflight.py on it: an object in which anything touches a read's destination before the wait
# that retires it is never linked.
W, RAD, DEF = "field_forward_bf16w_kernel", "field_radiance_bf16x3_kernel", "field_deform_bf16x3_kernel"
CRAD, CDEF = "field_backward_chain_rad_kernel", "field_backward_chain_def_kernel"
# Longest compile first (the first three take 25-60 s a run, field_f32.hip 15-30 s, the next 11 s, the rest 2-6 s): the pool starts
# the units in this order, so that it does not end on a long straggler.  HAND_SCHEDULED, and with it the in-flight report, follows it too.
UNITS = [
    # the bf16 radiance nets (NeRFaceModel with deformation nets: those stay fp32; without: the whole net)
    Unit("field_bf16w.hip", EVERY_MODEL, FIELD, ARCH_ACC, {0: (W,), 1: (W,), 2: (W,)}),
    # the split-operand kernels (SAHS_BF16X3; with deformation nets also the mixed precision's)
    Unit("field_bf16x3.hip", EVERY_MODEL, FIELD, ARCH_ACC, {0: (RAD, DEF), 1: (DEF, RAD), 2: (RAD,)}),
    Unit("field_bwd_chain.hip", EVERY_MODEL, FIELD, ARCH_ACC, {0: (CRAD, CDEF), 1: (CRAD, CDEF), 2: (CRAD,)}),
    Unit("field_f32.hip", EVERY_MODEL, FIELD),
    # with field_bwd_gemm.hip, which it includes (ONE translation unit: apart, every kernel of both gets another prologue); reads no
    # layout constant and is built once (every model's field_bwd.hip calls its launchers)
    Unit("field_bwd_tn_jobs.hip", ONCE, FIELD, NO_SLP),
    Unit("field_bwd_chain_f32.hip", EVERY_MODEL, FIELD),
    # (its kernels were built with the GEMMs when those lived here)
    Unit("field_bwd.hip", EVERY_MODEL, FIELD, NO_SLP),
    Unit("train_bwd.hip", ONCE),
    Unit("render_ops.hip", ONCE),
    Unit("pack.hip", EVERY_MODEL),
    Unit("capi.hip", ONCE),
    Unit("spade_ops.hip", ONCE),
    Unit("spectral_norm.hip", ONCE),
    Unit("image_metrics.hip", ONCE),
    Unit("image_loss.hip", ONCE),
    Unit("lpips.hip", ONCE),
    Unit("frame_products.hip", ONCE),
    Unit("optim.hip", ONCE),
]
HAND_SCHEDULED = [(u.src, m, pat) for u in UNITS for m in u.models for pat in u.hand.get(m, ())]

# Scratch: zero unless named.  Kernels whose correctness or speed rests on an exact count of the wave's memory instructions (a counted
# s_waitcnt vmcnt behind LDS-DMA, a counted lgkmcnt behind hand-issued LDS reads) must not get scratch: a spill reload is a VMEM
# instruction the count does not know about, and a spilled in-flight destination would be stored before its data has landed.  The build
# reads the compiler's own resource remarks (build/<library>.resource_usage.txt) and FAILS if any kernel uses more scratch than its row
# here allows -- full mangled name -> bytes/lane -- and no row means none.  For the rest zero is a performance guard:
#   * the headline fp32 forward (no activation saving): a reload's wait also drains its in-flight weight prefetch;
#   * the image-metric, image-loss and LPIPS kernels: their channel loop must stay a loop (unrolled, four channels' float64
#     accumulators spill);
#   * the spectral-norm kernels: 1024-thread workgroups, 128 registers;
#   * the frame-product kernels: a pixel per thread, its 15 values stay in LDS, not in an indexed array;
#   * the streaming kernels (SPADE, Adam): nothing to spill.
ALLOWED_SCRATCH = {
    # the activation-saving fp32 forwards: with the tile stores unconditional (f32_pipe.hpp: kStores) they keep two plane pointers in
    # scratch, reloaded twice per 128-sample tile -- extra vector-memory operations can only make a counted wait stricter, never weaker
    "_ZN4sahs24field_forward_f32_kernelILb1ELi0EEEvPKfS2_iliS2_iS2_PfS3_S3_S3_iiPKiPjNS_10SparseArgsE": 96,      # (uses 80)
    "_ZN4sahs24field_forward_f32_kernelILb1ELi2EEEvPKfS2_iliS2_iS2_PfS3_S3_S3_iiPKiPjNS_10SparseArgsE": 96,      # (uses 32)
    "_ZN7sahs_nf24field_forward_f32_kernelILb1ELi0EEEvPKfS2_iliS2_iS2_PfS3_S3_S3_iiPKiPjNS_10SparseArgsE": 96,
    "_ZN7sahs_nf24field_forward_f32_kernelILb1ELi2EEEvPKfS2_iliS2_iS2_PfS3_S3_S3_iiPKiPjNS_10SparseArgsE": 48,
    # A debt, pinned so that it cannot grow: this kernel runs twice per default training step behind an LDS-DMA
    # ring -- the construction the paragraph above says must not spill -- and spills 112 bytes/lane.
    "_ZN4sahs22gemm_tn_jobs256_kernelENS_7TnBatchEillPKf": 112,
}


def jobs_limit():
    """Compilers that run at a time: MAX_JOBS when set, else one per CPU; never above 16."""
    return max(1, min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)))


def unit_command(src, model, defines, form, out, hipcc=None):
    """The hipcc command for one unit (src: a name in UNITS, or a path that ends in one) and model: form "obj" makes the object `out`
    and prints the resource remarks, "isa" the device side's assembly from the same flags.  build() and the ISA tools get it here."""
    unit = next((u for u in UNITS if u.src == os.path.basename(src)), None)
    if unit is None or model not in unit.models:
        raise ValueError("%s (SAHS_MODEL=%d) is not a unit of the library (build.py: UNITS)" % (src, model))
    mode = {"obj": ["-Rpass-analysis=kernel-resource-usage", "-c"], "isa": ["--cuda-device-only", "-S"]}[form]
    return [hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + list(unit.fp) + (["-DSAHS_MODEL=%d" % model] if model else []) + \
        list(unit.tune) + ["-D" + d for d in defines] + mode + [os.path.join(CSRC, unit.src), "-o", out]


def plan(lib=LIB, defines=(), check_inflight=True, hipcc=None):
    """Every compiler run of one build, in starting order -> [(src, model, form, output path, command)].  A diagnostic library
    (lib is not LIB) prefixes its objects with its own name; one ISA run per (unit, model) that has hand-scheduled kernels."""
    bdir, tag = os.path.join(HERE, "build"), os.path.basename(lib)
    runs = []
    for u in UNITS:
        for m in u.models:
            obj = os.path.join(bdir, ("" if lib == LIB else tag + ".") + u.src.replace(".hip", ".m%d.o" % m if m else ".o"))
            runs.append((u.src, m, "obj", obj, unit_command(u.src, m, defines, "obj", obj, hipcc)))
            if check_inflight and u.hand.get(m):
                isa = os.path.join(bdir, "%s.%s.m%d.s" % (tag, u.src.replace(".hip", ""), m))
                runs.append((u.src, m, "isa", isa, unit_command(u.src, m, defines, "isa", isa, hipcc)))
    return runs


def run_pool(items, jobs, run):
    """run(item) for every item, started in order, at most `jobs` at a time -> the results, in the order of items.  After the first
    exception nothing further is started; it is raised once the runs under way have ended."""
    results, failed, todo, lock = {}, [], iter(enumerate(items)), threading.Lock()

    def worker():
        while True:
            with lock:
                nxt = None if failed else next(todo, None)
            if nxt is None:
                return
            try:
                results[nxt[0]] = run(nxt[1])
            except Exception as e:
                failed.append(e)
    threads = [threading.Thread(target=worker) for _ in range(max(1, jobs))]
    for t in threads:
        t.start()
    try:
        for t in threads:
            t.join()
    except BaseException as e:      # an interrupt: start nothing further either
        failed.append(e)
    if failed:
        raise failed[0]
    return [results[i] for i in range(len(results))]


def _compile(run, verbose=False):
    """One entry of plan() -> the compiler's stderr (an object run's holds the resource remarks)."""
    src, model, form, _, cmd = run
    if verbose and form == "obj":
        print(" ".join(cmd), flush=True)
    p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    diag = [l for l in p.stderr.splitlines() if "[-Rpass-analysis=kernel-resource-usage]" not in l and not l.lstrip().startswith(("|", "^")) and
            not (l[:1] == " " and l.strip()[:1].isdigit() and "|" in l)]
    if diag and (p.returncode != 0 or (verbose and form == "obj")):
        print("\n".join(diag), file=sys.stderr)
    if p.returncode != 0:
        raise RuntimeError("hipcc%s failed on %s (SAHS_MODEL=%d)" % (" -S" if form == "isa" else "", src, model))
    return p.stderr


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "sahs_nerf.h"), os.path.abspath(__file__), CHECKER]
    return any(os.path.getmtime(d) > t for d in deps)


def _resource_usage(remarks):
    """Parse clang's -Rpass-analysis=kernel-resource-usage remarks -> {mangled kernel name: dict}."""
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
            "LDS Size [bytes/block]": "lds"}
    for line in remarks.splitlines():
        if "remark:" not in line:
            continue
        body = line.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = dict(sgpr=0, vgpr=0, agpr=0, scratch=0, occ=0, lds=0)
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            if k.strip() in keys:
                out[cur][keys[k.strip()]] = int(v)
    return out


def scratch_violations(usage, defines=()):
    """One line per kernel of a resource table that uses more scratch than ALLOWED_SCRATCH grants it (none, unless named in full).
    Ablation builds (defines) are diagnostics and may spill."""
    return [] if defines else ["%s: %d bytes/lane of scratch (allowed: %d)" % (k, v["scratch"], ALLOWED_SCRATCH.get(k, 0))
                               for k, v in sorted(usage.items()) if v["scratch"] > ALLOWED_SCRATCH.get(k, 0)]


def _inflight_report(isa_text, usage):
    """tools/check_lds_inflight.py over the ISA of every hand-scheduled kernel (isa_text: {(src, model): assembly}) -> one report
    line per row of HAND_SCHEDULED; raises on a violation."""
    sys.path.insert(0, os.path.dirname(CHECKER))
    import check_lds_inflight as chk
    report = []
    for src, model, pat in HAND_SCHEDULED:
        text = isa_text[src, model]
        total, viol, dist = chk.check(text, pat)
        # the ISA checked must be the ISA linked: same register allocation as the object's kernels (unified file: accumulation
        # registers start at the arch-VGPR count rounded up to 4)
        for n in re.findall(r"^(\S*%s\S*):" % re.escape(pat), text, re.M):
            want, meta = usage.get(n), re.search(r"\.amdhsa_kernel %s\b.*?\.end_amdhsa_kernel" % re.escape(n), text, re.S)
            nxt = re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta.group(0)) if meta else None
            if want is not None and nxt is not None:
                expect = want["vgpr"] if not want["agpr"] else (want["vgpr"] + 3) // 4 * 4 + want["agpr"]
                if int(nxt.group(1)) != expect:
                    raise RuntimeError("in-flight check: the ISA of %s is not the object's (next_free_vgpr %s, object vgpr %d agpr %d)"
                                       % (n, nxt.group(1), want["vgpr"], want["agpr"]))
        report.append("%s (SAHS_MODEL=%d) %s: %d hand-issued ds_read_b128, %d violations, longest in-flight window %d instructions"
                      % (src, model, pat, total, len(viol), max(dist) if dist else 0))
        if viol or total == 0:
            raise RuntimeError("hand-issued LDS reads touched in flight (tools/check_lds_inflight.py) in %s SAHS_MODEL=%d:\n  %s"
                               % (src, model, "\n  ".join("%s | %s" % (r, w) for _, r, w in viol[:8]) or "no reads found"))
    return report


def build(force=False, verbose=False, defines=(), out=None, check_inflight=True):
    """defines/out: diagnostic variants (tools/ablate.py, tools/stamp_*.py) -- extra -D flags, separate output .so.  Every timing-only
    ablation or stamp in the sources sits behind SAHS_DIAG, which the shipped library (out=None) refuses."""
    if out is None and defines:
        raise RuntimeError("libsahs_nerf.so is built without extra defines (SAHS_DIAG variants go to their own file: out=...)")
    lib = LIB if out is None else out
    if out is None and not (force or _stale()):
        return lib
    report_base = os.path.join(HERE, "build", os.path.basename(lib))      # one resource table, one in-flight report per output library
    os.makedirs(os.path.dirname(report_base), exist_ok=True)
    # 1. plan, 2. compile
    runs = plan(lib, defines, check_inflight)
    stderr = run_pool(runs, jobs_limit(), lambda r: _compile(r, verbose))
    # 3. scratch
    usage = _resource_usage("\n".join(err for run, err in zip(runs, stderr) if run[2] == "obj"))
    with open(report_base + ".resource_usage.txt", "w") as f:
        for k in sorted(usage):
            f.write("%-110s vgpr %3d agpr %3d sgpr %3d scratch %4d lds %6d occupancy %d\n" % (
                k, usage[k]["vgpr"], usage[k]["agpr"], usage[k]["sgpr"], usage[k]["scratch"], usage[k]["lds"], usage[k]["occ"]))
    bad = scratch_violations(usage, defines)
    if bad:
        raise RuntimeError("kernels must not use scratch (build.py: ALLOWED_SCRATCH):\n  " + "\n  ".join(bad))
    # 4. the in-flight check, on the same translation units' device side as ISA text (same flags => same code; the register counts of
    # the two compilations are compared)
    if check_inflight:
        report = _inflight_report({(r[0], r[1]): open(r[3]).read() for r in runs if r[2] == "isa"}, usage)
        with open(report_base + ".lds_inflight.txt", "w") as f:
            f.write("\n".join(report) + "\n")
        if verbose:
            print("\n".join(report))
    # 5. link.  -z defs: a launcher that some table names but no object defines fails here, not at dlopen
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", "-o", lib] + [r[3] for r in runs if r[2] == "obj"])
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
