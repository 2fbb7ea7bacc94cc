"""The build's plan, scratch guard, job count and pool (sahs-deformable-nerf_amd/build.py), without a compiler or a GPU."""
import os
import threading

import pytest

from conftest import GOLDEN, REPO, pkg

HIPCC = "/opt/rocm/bin/hipcc"
JOBS256 = "_ZN4sahs22gemm_tn_jobs256_kernelENS_7TnBatchEillPKf"


def render(cmd):
    return " ".join(cmd).replace(REPO + os.sep, "@REPO@/")


def test_the_plan_is_the_recorded_one():
    """tests/golden/build_commands.txt: the 32 object commands that the build printed before it had a unit table, repository path
    replaced.  Same commands => same objects."""
    b = pkg("build")
    runs = b.plan(hipcc=HIPCC)
    objs, isas = [r for r in runs if r[2] == "obj"], [r for r in runs if r[2] == "isa"]
    assert len(objs) + len(isas) == len(runs)
    recorded = open(os.path.join(GOLDEN, "build_commands.txt")).read().splitlines()
    assert len(recorded) == 32 and len(objs) == 32
    assert {render(r[4]) for r in objs} == set(recorded)
    assert len({(r[0], r[1]) for r in objs}) == 32, "a (source, model) built twice"
    assert len({r[3] for r in objs}) == 32, "two units share an object file"
    assert all(r[4][-1] == r[3] and r[4][-2] == "-o" for r in runs)
    # one ISA run per (source, model) with hand-scheduled kernels, each to a file of its own, from its object's command
    assert len(isas) == 9 and len({r[3] for r in isas}) == 9 and len({(r[0], r[1]) for r in isas}) == 9
    obj_cmd = {(r[0], r[1]): r[4] for r in objs}
    for src, model, _, path, cmd in isas:
        want = list(obj_cmd[src, model][:-1]) + [path]
        i = want.index("-Rpass-analysis=kernel-resource-usage")
        assert want[i + 1] == "-c"
        want[i:i + 2] = ["--cuda-device-only", "-S"]
        assert cmd == want
    assert len(b.HAND_SCHEDULED) == 13 and len(set(b.HAND_SCHEDULED)) == 13
    for src, model, pat in b.HAND_SCHEDULED:
        assert len([r for r in isas if (r[0], r[1]) == (src, model)]) == 1, (src, model, pat)
    assert {(s, m) for s, m, _ in b.HAND_SCHEDULED} == {(r[0], r[1]) for r in isas}
    # without the in-flight check there is no ISA run; a diagnostic library gets objects of its own
    assert [r for r in b.plan(hipcc=HIPCC, check_inflight=False)] == objs
    other = b.plan(lib=os.path.join(REPO, "variants", "libsahs_x.so"), defines=["SAHS_DIAG"], hipcc=HIPCC)
    assert not {r[3] for r in other} & {r[3] for r in runs} and all("-DSAHS_DIAG" in r[4] for r in other)


def test_unit_command_knows_only_the_units():
    b = pkg("build")
    cmd = b.unit_command("csrc/field_bwd_chain_f32.hip", 1, ["X=2"], "isa", "k.s", hipcc=HIPCC)
    assert "-DSAHS_MODEL=1" in cmd and "-DX=2" in cmd and cmd[-3:] == [os.path.join(b.CSRC, "field_bwd_chain_f32.hip"), "-o", "k.s"]
    with pytest.raises(ValueError):
        b.unit_command("field_bwd_gemm.hip", 0, [], "isa", "k.s")      # included by field_bwd_tn_jobs.hip, never a unit
    with pytest.raises(ValueError):
        b.unit_command("capi.hip", 1, [], "obj", "k.o")      # built once


def usage(**scratch):
    return {k: dict(sgpr=0, vgpr=0, agpr=0, scratch=v, occ=0, lds=0) for k, v in scratch.items()}


def test_scratch_is_zero_unless_named_in_full():
    b = pkg("build")
    assert len(b.ALLOWED_SCRATCH) == 5 and b.ALLOWED_SCRATCH[JOBS256] == 112
    assert b.scratch_violations(usage(_Z9unlistedv=0)) == []
    bad = b.scratch_violations(usage(_Z9unlistedv=16, _Z5otherv=0))
    assert len(bad) == 1 and bad[0].startswith("_Z9unlistedv: 16 bytes/lane")
    for name, cap in b.ALLOWED_SCRATCH.items():
        assert b.scratch_violations(usage(**{name: cap})) == []
        assert len(b.scratch_violations(usage(**{name: cap + 1}))) == 1
        # a name that merely contains a listed one is a kernel of its own
        assert len(b.scratch_violations(usage(**{name + "S0_": 16, "_ZN2ns" + name[3:]: 16}))) == 2
    # the spill the substring table let through: pinned, so it cannot grow
    assert len(b.scratch_violations(usage(**{JOBS256: 113}))) == 1
    # diagnostic builds may spill
    assert b.scratch_violations(usage(_Z9unlistedv=16, **{JOBS256: 4096}), defines=["SAHS_DIAG"]) == []


def test_job_count(monkeypatch):
    b = pkg("build")
    monkeypatch.setenv("MAX_JOBS", "64")
    assert b.jobs_limit() == 16
    monkeypatch.setenv("MAX_JOBS", "4")
    assert b.jobs_limit() == 4
    monkeypatch.delenv("MAX_JOBS")
    assert b.jobs_limit() == min(16, os.cpu_count())
    monkeypatch.setattr(os, "cpu_count", lambda: 192)
    assert b.jobs_limit() == 16




class Runner:
    """An injected runner that records how many runs overlap, and holds them so that they do (no sleeps).  Without a failure a run
    waits until `jobs` of them have been under way at once or the last item has started.  With fail_at, the runs before it pass; the
    failing one waits until every other worker holds a later item, then raises; the held ones return once the failing run's thread has
    ended, that is once the pool knows of the failure."""

    def __init__(self, total, jobs, fail_at=None):
        self.total, self.jobs, self.fail_at = total, min(jobs, total), fail_at
        self.cv, self.now, self.peak, self.started, self.failing = threading.Condition(), 0, 0, [], None

    def __call__(self, item):
        with self.cv:
            self.started.append(item)
            self.now += 1
            self.peak = max(self.peak, self.now)
            self.cv.notify_all()
            if self.fail_at is None:
                assert self.cv.wait_for(lambda: self.peak >= self.jobs or len(self.started) == self.total, timeout=5.0)
            elif item == self.fail_at:
                self.failing = threading.current_thread()
                assert self.cv.wait_for(lambda: len(self.started) == self.fail_at + self.jobs, timeout=5.0)
            elif item > self.fail_at:
                assert self.cv.wait_for(lambda: self.failing is not None, timeout=5.0)
        try:
            if item == self.fail_at:
                raise RuntimeError("item %d" % item)
            if self.fail_at is not None and item > self.fail_at:
                self.failing.join(5.0)
                assert not self.failing.is_alive()
            return item * item
        finally:
            with self.cv:
                self.now -= 1


@pytest.mark.parametrize("total,jobs", [(41, 8), (41, 16), (3, 8), (5, 1)])
def test_pool_never_exceeds_its_jobs(total, jobs):
    b = pkg("build")
    run = Runner(total, jobs)
    assert b.run_pool(range(total), jobs, run) == [i * i for i in range(total)]      # results in the order of the items
    assert run.peak == min(jobs, total) and sorted(run.started) == list(range(total))
    assert sorted(run.started[:run.peak]) == list(range(run.peak)), "items start in order"


@pytest.mark.parametrize("jobs", [1, 4])
def test_pool_starts_nothing_after_a_failure(jobs):
    b = pkg("build")
    run = Runner(41, jobs, fail_at=9)
    with pytest.raises(RuntimeError, match="item 9"):
        b.run_pool(range(41), jobs, run)
    # the items before the failing one, itself, and those the other workers already held when it failed: nothing of the other 28
    assert sorted(run.started) == list(range(9 + jobs)) and run.peak == jobs
