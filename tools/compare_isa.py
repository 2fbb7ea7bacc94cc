"""Compare the kernels of two gfx950 assembly files, names aside: is the device code of B the device code of A?

    hipcc <the build's flags for that unit> --cuda-device-only -S csrc/x.hip -o x.s
    (build.py: unit_command(..., "isa", "x.s"); `tools/check_isa.py x.hip <kernel> [model]` prints the command it runs)
    python tools/compare_isa.py A.s B.s [kernel name pattern]

Made for moving kernels between translation units and files (field_bwd.hip -> field_bwd_gemm.hip -> field_bwd_tn_jobs.hip, which
includes the former: one unit).  Byte equality is the wrong bar for that: a
kernel that calls an out-of-line function (the job kernels' 64-bit division) gets the workgroup-id registers its ABI needs inferred from
the whole translation unit, so scalar registers are renumbered and a prologue may gain or lose a v_mov_b32.  What is compared instead,
per kernel present in both files (namespaces sahs / sahs_nf / sahs_ns / anonymous are folded into one):

  * kernels with a barrier, an LDS-DMA load or an MFMA -- the ordered sequence of non-scalar opcodes together with every s_waitcnt,
    s_barrier, s_nop, s_setprio and s_sleep WITH its operands must be identical over the whole function and the count of the other
    scalar instructions equal ("same").  Failing that, the same sequence from the first barrier / LDS-DMA / MFMA to the end must be
    identical and the whole-function opcode histogram may differ in v_mov_b32 and s_nop only, by at most 2 ("same hot part");
  * the others (streaming helpers) -- the opcode histogram may differ in v_mov_b32 only, by at most 2.

Exit status 1 if any kernel fails, or if no kernel was compared.
"""
import collections
import re
import sys

KEEP = ("s_waitcnt", "s_barrier", "s_setprio", "s_sleep", "s_nop")
HOT = ("s_barrier", "global_load_lds", "v_mfma")


def kernels(path):
    t = open(path).read()
    t = re.sub(r"_ZN(?:4sahs|7sahs_nf|7sahs_ns|12_GLOBAL__N_1)(?=\d)", "_ZN", t)
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", t, re.M))
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", t, re.S | re.M):
        if m.group(1) not in names:
            continue
        seq, salu = [], 0
        for l in m.group(2).splitlines():
            l = l.split(";")[0].strip()
            if not l or l.startswith(".") or l.endswith(":"):
                continue
            op = l.split()[0]
            if op.startswith("s_") and op not in KEEP:
                salu += 1
            else:
                seq.append(" ".join(l.split()) if op.startswith("s_") else op)
        out[m.group(1)] = (seq, salu)
    return out


def hot_part(seq):
    i = next((i for i, x in enumerate(seq) if x.startswith(HOT)), None)
    return None if i is None else seq[i:]


def compare(a, b):
    """-> (verdict, ok, detail) for one kernel's (sequence, scalar count) pair."""
    (va, sa), (vb, sb) = a, b
    op = lambda x: re.sub(r"_(e32|e64)$", "", x.split()[0])      # (an encoding suffix is not another opcode)
    ha, hb = collections.Counter(op(x) for x in va), collections.Counter(op(x) for x in vb)
    diff = {o: (ha[o], hb[o]) for o in set(ha) | set(hb) if ha[o] != hb[o]}
    small = lambda allowed: all(o in allowed and abs(x - y) <= 2 for o, (x, y) in diff.items())
    ta, tb = hot_part(va), hot_part(vb)
    if ta is None and tb is None:
        return ("helper: histogram " + ("equal" if not diff else "differs"), small(("v_mov_b32",)), diff)
    if va == vb and sa == sb:
        return ("same", True, {})
    if ta == tb and small(("v_mov_b32", "s_nop")):
        return ("same hot part (%d instr)" % len(ta), True, diff)
    first = next((i for i, (x, y) in enumerate(zip(va, vb)) if x != y), min(len(va), len(vb)))
    return ("DIFFERS at %d" % first, False, diff)


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    pat = re.compile(argv[3]) if len(argv) > 3 else None
    bad = n = 0
    print("%-72s %13s %11s  %s" % ("kernel", "non-scalar A/B", "scalar A/B", "verdict"))
    for k in sorted(a):
        if k not in b or (pat and not pat.search(k)):
            continue
        verdict, ok, detail = compare(a[k], b[k])
        n += 1
        bad += not ok
        print("%-72s %6d/%6d %5d/%5d  %s%s%s" % (k[:72], len(a[k][0]), len(b[k][0]), a[k][1], b[k][1], "" if ok else "FAIL: ", verdict,
                                                   "  %s" % detail if detail else ""))
    only = sorted(k for k in set(a) ^ set(b) if not pat or pat.search(k))
    if only:
        print("in one file only: " + ", ".join(only))
    print("%d kernels compared, %d fail" % (n, bad))
    return 1 if bad or n == 0 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
