"""A solve's launch plan and the row-step ladder (csrc/solve_plan.inc: solve_plan, ksm_of, with_ksm) — no GPU.
tests/solve_plan_main.cpp includes that file alone; it is built here with the host compiler under AddressSanitizer and
UBSan and run as a plain executable.  The expected step lists below were derived by hand from the three nested launch
functions the plan replaced (the host's launch_solve and launch, and the wave launcher's choice of build, form and
grid), not from the plan's code."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_CLANG = "/opt/rocm/llvm/bin/clang++"
SLOTS, SLOTS_RESTO, TEAM_CAP = 1024, 512, 128   # (the restoration-capable builds hold fewer waves)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or (ROCM_CLANG if os.path.exists(ROCM_CLANG) else shutil.which("clang++"))
    assert cxx, "no host C++ compiler (g++ or ROCm's clang++)"
    out = str(tmp_path_factory.mktemp("solve_plan") / "solve_plan_main")
    # the sanitizers' runtimes linked into the program (clang's default), so that it runs whatever else a process loads
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *static, "-o", out, os.path.join(HERE, "solve_plan_main.cpp")])
    return out


def facts(program, resto=0, B=64, it=0, tr=0, pair=0, allow=0, ordered=0, records=1):
    return (program, resto, B, SLOTS, SLOTS_RESTO, it, tr, pair, allow, ordered, records)


@pytest.fixture(scope="module")
def plans(exe):
    def run(*cases):
        """cases: facts(...) each -> per case the list of steps; a step is its kind and what that kind carries"""
        args = [str(v) for c in cases for v in c]
        txt = subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=60).stdout
        out = []
        for line in txt.splitlines():
            w = line.split()
            if w[0] == "case":
                out.append([])
            elif w[0] == "WAVE":
                out[-1].append(wave(int(w[1]), w[3], resto=int(w[2]), team=int(w[4]), it=int(w[5]), tr=int(w[6])))
            elif w[0] == "HANDOFF":
                out[-1].append((w[0], int(w[2]), w[3]))
            elif w[0] in ("SENS", "SENS_OBS"):
                out[-1].append((w[0], int(w[2])))
            else:
                out[-1].append(w[0])
        assert len(out) == len(cases)
        return out
    return run


def wave(phase, form, resto=0, team=0, it=0, tr=0):
    return ("WAVE", phase, "resto" if resto else "lean", form, team, it, tr)


HANDOFF = ("HANDOFF", 1, "QUEUE")   # always the fp64 restoration-capable build's work queue
ZH, ZL = "ZERO_HEADER", "ZERO_LIST"


def test_dd(plans):
    # (no queue, no split, no restoration phase: one launch whatever the cuts and cfg.restoration say)
    assert plans(facts("DD"), facts("DD", resto=1, it=14, tr=40, pair=1, allow=1)) == [["DD"]] * 2


def test_lane(plans):
    assert plans(facts("LANE"), facts("LANE", it=14, tr=40), facts("LANE", B=SLOTS + 1)) == [["LANE"]] * 3
    assert plans(facts("LANE", resto=1), facts("LANE", resto=1, it=16, tr=40, B=5000)) == [[ZL, "LANE", HANDOFF]] * 2


def test_sens(plans):
    for prog in ("SENS", "SENS_OBS"):
        assert plans(facts(prog), facts(prog, resto=1), facts(prog, resto=1, it=20, tr=40, B=5000)) == [
            [(prog, 0)], [(prog, 1)], [(prog, 1)]]


def test_fp64_one_phase(plans):
    one, queue = [wave(0, "ONE_WAVE")], [wave(0, "QUEUE")]
    # no cut; B = 1 with cuts; a launch order; no record buffer
    assert plans(facts("WAVE_F64"), facts("WAVE_F64", B=1, it=14, tr=40), facts("WAVE_F64", it=14, ordered=1),
                 facts("WAVE_F64", it=14, tr=40, records=0)) == [one] * 4
    # more instances than slots: the work queue, cuts or not, ordered or not
    assert plans(facts("WAVE_F64", B=SLOTS + 1), facts("WAVE_F64", B=SLOTS + 1, it=14, tr=40),
                 facts("WAVE_F64", B=SLOTS + 1, it=14, ordered=1)) == [queue] * 3
    assert plans(facts("WAVE_F64", B=SLOTS)) == [one]


def test_fp64_one_phase_restoration_build(plans):
    """Without a split the restoration-capable build runs, and its own residency decides between one wave per instance
    and the work queue."""
    assert plans(facts("WAVE_F64", resto=1), facts("WAVE_F64", resto=1, B=SLOTS_RESTO),
                 facts("WAVE_F64", resto=1, B=SLOTS_RESTO + 1), facts("WAVE_F64", resto=1, B=SLOTS, it=16, ordered=1)) == [
        [wave(0, "ONE_WAVE", resto=1)], [wave(0, "ONE_WAVE", resto=1)], [wave(0, "QUEUE", resto=1)],
        [wave(0, "QUEUE", resto=1)]]


def test_fp64_iteration_cut(plans):
    split = [ZH, wave(1, "ONE_WAVE", it=14), wave(2, "ONE_WAVE")]
    assert plans(facts("WAVE_F64", B=2, it=14), facts("WAVE_F64", B=SLOTS, it=14),
                 facts("WAVE_F64", B=SLOTS, it=14, allow=1)) == [split] * 3
    assert plans(facts("WAVE_F64", B=SLOTS + 1, it=14)) == [[wave(0, "QUEUE")]]
    # cfg.restoration = IPOPT: phase 1 on the lean build, phase 2 on the restoration-capable one; the lean build's slots
    # decide the split; the pair where the handle has it and the caller takes it
    r4 = [ZH, wave(1, "ONE_WAVE", it=13), wave(2, "ONE_WAVE", resto=1)]
    rp = [ZH, wave(1, "ONE_WAVE", it=13), wave(2, "PAIR", resto=1)]
    assert plans(facts("WAVE_F64", resto=1, it=13), facts("WAVE_F64", resto=1, it=13, B=SLOTS, pair=1),
                 facts("WAVE_F64", resto=1, it=13, allow=1), facts("WAVE_F64", resto=1, it=13, pair=1, allow=1),
                 facts("WAVE_F64", resto=1, it=13, B=SLOTS, pair=1, allow=1)) == [r4, r4, r4, rp, rp]


def test_fp64_trial_cut(plans):
    def team(t, it, resto=0):
        return [ZH, wave(1, "TEAM", team=t, it=it, tr=40), wave(2, "TEAM", resto=resto, team=t)]
    assert plans(facts("WAVE_F64", it=20, tr=40), facts("WAVE_F64", B=TEAM_CAP + 1, it=20, tr=40),
                 facts("WAVE_F64", B=2, tr=40), facts("WAVE_F64", resto=1, it=20, tr=40, pair=1, allow=1)) == [
        team(64, 20), team(TEAM_CAP, 20), team(2, 0), team(64, 20, resto=1)]


def test_fp32(plans):
    one, split = wave(0, "ONE_WAVE"), [wave(1, "ONE_WAVE", it=16), wave(2, "ONE_WAVE")]
    # cfg.restoration = IPOPT: the hand-off after the last launch of the solve; the trial cut is not read
    assert plans(facts("WAVE_F32", resto=1), facts("WAVE_F32", resto=1, tr=40),
                 facts("WAVE_F32", resto=1, it=16, records=0)) == [[ZL, one, HANDOFF]] * 3
    assert plans(facts("WAVE_F32", resto=1, B=SLOTS + 1, it=16)) == [[ZL, wave(0, "QUEUE"), HANDOFF]]
    assert plans(facts("WAVE_F32", resto=1, it=16, tr=40, pair=1, allow=1), facts("WAVE_F32", resto=1, B=SLOTS, it=16)) == [
        [ZH, ZL, *split, HANDOFF]] * 2
    assert plans(facts("WAVE_F32"), facts("WAVE_F32", tr=40), facts("WAVE_F32", it=16, tr=40),
                 facts("WAVE_F32", B=SLOTS + 1, it=16)) == [[one], [one], [ZH, *split], [wave(0, "QUEUE")]]


def test_ladder(exe):
    """ksm_of's contract: the smallest compiled size K with rows <= 4 K, and past the largest the sentinel alipmpc_create
    refuses; with_ksm hands out the same K as a compile-time value (the largest one past the ladder, where no handle
    exists)."""
    table = [4, 8, 10, 12, 16, 24, 32, 48]
    txt = subprocess.run([exe, "ladder"], check=True, capture_output=True, text=True, timeout=60).stdout
    rows = [tuple(int(v) for v in line.split()) for line in txt.splitlines()]
    assert [r[0] for r in rows] == list(range(1, 201))
    for r, k_of, k_with in rows:
        if r <= 192:
            want = min(k for k in table if r <= 4 * k)
            assert (k_of, k_with) == (want, want), r
        else:
            assert (k_of, k_with) == (1 << 20, 48), r
