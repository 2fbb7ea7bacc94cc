#!/usr/bin/env python3
"""How far ahead of its first use is every weight-fragment read of a kernel issued?  Read off the ISA.

The fp32 layer pipeline (csrc/f32_pipe.hpp: dense_ep) issues the `ds_read_b128` of the fragment a few steps on behind the 4 MFMAs of the
current step, so that an LDS round trip runs under 8-12 MFMAs.  The compiler is free to sink a read down to its first use, and under
register pressure it does: the step then opens with `s_waitcnt lgkmcnt(0)` on a read issued one instruction earlier, and only the SIMD's
other wave can cover the round trip.  This listing is what showed it (LAB_NOTES.md, "fp32 field forward: 64 KB chunks"): at 64 KB chunks
1,411 of the fine pass's 2,208 reads sat directly in front of their MFMA.

    python tools/scan_frag_reads.py kernels.s [kernel-name-substring]
    (kernels.s: hipcc <the build's flags for that unit> --cuda-device-only -S csrc/x.hip -o kernels.s -- build.py: unit_command;
    `tools/check_isa.py x.hip <kernel> [model]` prints the command it runs)

Per kernel: instructions, MFMAs, `ds_read_b128`, and the histogram {MFMAs issued between a read and the first MFMA that takes its
destination as the A operand: reads}; "other" = reads first used by something else (activations, records).
"""
import collections
import re
import sys


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def distances(lines, window=600):
    dist = collections.Counter()
    for i, l in enumerate(lines):
        if not l.startswith("ds_read_b128"):
            continue
        dst, n = regs(l.split()[1].rstrip(",")), 0
        for j in range(i + 1, min(i + window, len(lines))):
            t = lines[j].replace(",", " ").split()
            if t[0].startswith("v_mfma"):
                if regs(t[2]) & dst:
                    dist[n] += 1
                    break
                n += 1
            elif any(regs(x) & dst for x in t[1:]):
                dist["other"] += 1
                break
    return dist


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    txt, pat = open(argv[1]).read(), argv[2] if len(argv) > 2 else ""
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M))
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        if m.group(1) not in names or pat not in m.group(1):
            continue
        lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
        lines = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
        d = distances(lines)
        if not d:
            continue
        ops = collections.Counter(l.split()[0] for l in lines)
        print("%s\n  %d instructions, %d MFMAs, %d ds_read_b128, %d s_barrier, %d s_waitcnt" % (
            m.group(1), len(lines), sum(v for k, v in ops.items() if k.startswith("v_mfma")), ops["ds_read_b128"], ops["s_barrier"], ops["s_waitcnt"]))
        print("  MFMAs between read and use: " + ", ".join("%s: %d" % (k, d[k]) for k in sorted(d, key=lambda k: (isinstance(k, str), k))))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
