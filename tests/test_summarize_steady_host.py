"""``tools/summarize_profiles.py --steady``: per-kernel statistics of the steady part of a kernel trace -- only the dispatches behind the
skip-th marker dispatch count, so a library's first-call algorithm search (which, for the Stage-II training step, is a hundred times the
step itself) stays out of the summary.  A synthetic trace with known sums; no GPU, no profiler."""
import csv
import os
import subprocess
import sys

from conftest import REPO

TOOL = os.path.join(REPO, "tools", "summarize_profiles.py")


def _trace(path):
    """Three 'steps', each a slow search kernel only in step 0, two conv dispatches and one marker; timestamps out of file order."""
    rows, t = [], 1000
    for step in range(3):
        if step == 0:
            rows.append(("naive_search_kernel", t, t + 90000))
            t += 90010
        for dur in (100 + step, 300 + step):
            rows.append(("conv_kernel", t, t + dur))
            t += dur + 5
        rows.append(("void other::elementwise<float>(float*, long)", t, t + 7))
        t += 12
        rows.append(("void sahs::adam_step_kernel(float*, float const*)", t, t + 3))
        t += 8
    rows.append(("late_kernel", t, t + 11))      # behind the last marker: counted with the steady part
    rows = rows[::2] + rows[1::2]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for name, a, b in rows:
            w.writerow(["KERNEL_DISPATCH", name, a, b])


def test_steady_summary_counts_only_dispatches_behind_the_marker(tmp_path):
    """Fails without the option (the tool then takes its first argument for a round tag)."""
    src, dst = str(tmp_path / "trace.csv"), str(tmp_path / "out.csv")
    _trace(src)
    run = subprocess.run([sys.executable, TOOL, "--steady", src, "adam_step_kernel", "1", dst, "a header"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(dst).read().splitlines()
    assert lines[0] == "# a header" and lines[1].startswith("# steady part: the 2 steps after marker 1 of 3 (adam_step_kernel)")
    rows = {r["Name"]: r for r in csv.DictReader(lines[2:])}
    assert sorted(rows) == ["conv_kernel", "late_kernel", "void other::elementwise<float>(float*, long)"]      # no search, no marker
    conv = rows["conv_kernel"]
    assert (int(conv["Calls"]), int(conv["TotalDurationNs"]), int(conv["MinNs"]), int(conv["MaxNs"])) == (4, 101 + 301 + 102 + 302, 101, 302)
    total = 806 + 14 + 11
    assert abs(float(conv["Percentage"]) - 100.0 * 806 / total) < 0.01
    assert list(rows)[0] == "conv_kernel"                                                                      # sorted by total time
    assert "%.3f ms of kernel time per steady step" % (total / 2 / 1e6) in run.stdout
    # skipping two markers leaves one step
    run = subprocess.run([sys.executable, TOOL, "--steady", src, "adam_step_kernel", "2", dst, "h"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = {r["Name"]: r for r in csv.DictReader(open(dst).read().splitlines()[2:])}
    assert (int(rows["conv_kernel"]["Calls"]), int(rows["conv_kernel"]["TotalDurationNs"])) == (2, 102 + 302)
