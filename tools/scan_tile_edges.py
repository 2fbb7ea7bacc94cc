#!/usr/bin/env python3
"""What stands at the two edges of every output tile of a kernel: its bias read and its activation?  Read off the ISA.

The fp32 layer pipeline (csrc/f32_pipe.hpp: dense_ep) starts a 16 x 16 output tile from its bias -- a `ds_read_b128` whose destination
is the C operand of the tile's first MFMA -- and ends it with the activation of the accumulator, VALU instructions that read the result
of the tile's last MFMA.  A wave issues in order: a bias read directly in front of its MFMA makes the wave sit out an LDS round trip
(`s_waitcnt lgkmcnt(0)`, which also drains every fragment read issued before it), an activation directly behind its MFMA makes it sit
out the MFMA's latency.  Beside tools/scan_frag_reads.py (the A operands) this lists the other two:

    python tools/scan_tile_edges.py kernels.s [kernel-name-substring]
    (kernels.s: hipcc <the build's flags for that unit> --cuda-device-only -S csrc/x.hip -o kernels.s -- build.py: unit_command;
    `tools/check_isa.py x.hip <kernel> [model]` prints the command it runs)

Per kernel, two histograms:
  tile starts   {MFMAs issued between a `ds_read_b128` and the first MFMA that takes its destination as srcC: reads}
                (reads first used as an A or B operand or by a non-MFMA instruction are not tile starts and are not counted)
  tile ends     {MFMAs issued between an MFMA and the first non-MFMA instruction that reads its result: such instructions' producers}
                (an MFMA whose result is next read by another MFMA -- the accumulation chain -- or overwritten is not a tile end)
Both look ahead in program order and stop at a branch or a label, like the scheduler: distances are within a basic block.
"""
import collections
import re
import sys

WINDOW = 800


def regs(tok):
    m = re.match(r"[va]\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"[va](\d+)$", tok)
    return {int(m.group(1))} if m else set()


def is_mfma(op):
    return op.startswith("v_mfma")


def block_end(line):
    return line.endswith(":") or line.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))


def tile_starts(lines):
    """{MFMAs between a bias read and the MFMA that starts from it: count}"""
    dist = collections.Counter()
    for i, l in enumerate(lines):
        if not l.startswith("ds_read_b128"):
            continue
        dst, n = regs(l.split()[1].rstrip(",")), 0
        for j in range(i + 1, min(i + WINDOW, len(lines))):
            if block_end(lines[j]):
                break
            t = lines[j].replace(",", " ").split()
            if is_mfma(t[0]):      # v_mfma vdst, srcA, srcB, srcC
                if regs(t[2]) & dst or regs(t[3]) & dst:
                    break          # a weight fragment (or an operand): scan_frag_reads.py's
                if len(t) > 4 and regs(t[4]) & dst:
                    dist[n] += 1
                    break
                n += 1
            elif any(regs(x) & dst for x in t[1:]):
                break              # read or overwritten by something else
    return dist


def tile_ends(lines):
    """{MFMAs between an MFMA and the first non-MFMA reader of its result: count}"""
    dist = collections.Counter()
    for i, l in enumerate(lines):
        t = l.replace(",", " ").split()
        if not is_mfma(t[0]):
            continue
        dst, n = regs(t[1]), 0
        for j in range(i + 1, min(i + WINDOW, len(lines))):
            if block_end(lines[j]):
                break
            u = lines[j].replace(",", " ").split()
            if is_mfma(u[0]):
                if regs(u[1]) & dst or any(regs(x) & dst for x in u[2:5]):
                    break          # the chain goes on (or the registers are taken over)
                n += 1
            elif any(regs(x) & dst for x in u[(1 if "store" in u[0] or "write" in u[0] else 2):]):      # (a store has no destination operand)
                dist[n] += 1
                break
            elif len(u) > 1 and regs(u[1]) & dst:
                break              # overwritten unread
    return dist


def kernel_bodies(txt, pat=""):
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M))
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        if m.group(1) not in names or pat not in m.group(1):
            continue
        lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
        yield m.group(1), [l for l in lines if l and not l.startswith(".")]


def fmt(d):
    return ", ".join("%d: %d" % (k, d[k]) for k in sorted(d)) or "none"


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    txt, pat = open(argv[1]).read(), argv[2] if len(argv) > 2 else ""
    for name, lines in kernel_bodies(txt, pat):
        ops = collections.Counter(l.split()[0] for l in lines)
        mfmas = sum(v for k, v in ops.items() if is_mfma(k))
        if not mfmas:
            continue
        waits0 = sum(1 for l in lines if l.startswith("s_waitcnt") and "lgkmcnt(0)" in l)
        print("%s\n  %d MFMAs, %d ds_read_b128, %d s_waitcnt (%d with lgkmcnt(0))" % (name, mfmas, ops["ds_read_b128"], ops["s_waitcnt"], waits0))
        print("  tile starts, MFMAs between bias read and first MFMA: " + fmt(tile_starts(lines)))
        print("  tile ends, MFMAs between last MFMA and first reader:  " + fmt(tile_ends(lines)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
