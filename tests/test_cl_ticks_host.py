"""The closed loop's tick plan (csrc/cl_ticks.inc: cl_tick_plan) — no GPU.  tests/cl_ticks_main.cpp includes that file
alone; it is built here with the host compiler under AddressSanitizer and UBSan and run as a plain executable.  The
expected segments below were derived by hand from the loop the plan replaced."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or (ROCM_CLANG if os.path.exists(ROCM_CLANG) else shutil.which("clang++"))
    assert cxx, "no host C++ compiler (g++ or ROCm's clang++)"
    exe = str(tmp_path_factory.mktemp("cl_ticks") / "cl_ticks_main")
    # the sanitizers' runtimes linked into the program (clang's default), so that it runs whatever else a process loads
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *static, "-o", exe, os.path.join(HERE, "cl_ticks_main.cpp")])

    def run(cases):
        """cases: (S, f, scheduled, mask, mode, fuse) each -> a list of segments (kind, t0, nt, s, i, live, anchor) each"""
        args = [str(int(v)) for c in cases for v in c]
        txt = subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=60).stdout
        out = []
        for line in txt.splitlines():
            w = line.split()
            if w[0] == "case":
                out.append([])
            else:
                out[-1].append((w[0], int(w[1]), int(w[2]), int(w[3]), int(w[4]), bool(int(w[5])), bool(int(w[6]))))
        assert len(out) == len(cases)
        return out
    return run


def seg(kind, t0, nt, f, live=False, anchor=False):
    return (kind, t0, nt, t0 // f, t0 % f, live, anchor)


def run_(a, b, f, live=False):
    return seg("RUN", a, b - a, f, live)


def test_mode_0_fused(plans):
    f = 6
    assert plans([(2, f, 1, 1 << 2, 0, 1)])[0] == [
        run_(0, 2, f), seg("SOLVE", 2, 1, f), run_(3, 8, f), seg("SOLVE", 8, 1, f), run_(9, 12, f)]


def test_mode_1_fused(plans):
    f = 6
    assert plans([(2, f, 1, 1 << 2, 1, 1)])[0] == [
        run_(0, 2, f), seg("SOLVE", 2, 1, f, anchor=True), run_(3, 6, f, live=True), run_(6, 8, f),
        seg("SOLVE", 8, 1, f, anchor=True), run_(9, 12, f, live=True)]


def test_mode_3(plans):
    f = 6
    want = [run_(0, 2, f), seg("SOLVE", 2, 1, f, anchor=True),
            seg("GUARDED", 3, 1, f, live=True, anchor=True), seg("GUARDED", 4, 1, f, live=True, anchor=True),
            seg("GUARDED", 5, 1, f, live=True, anchor=False), run_(6, 8, f), seg("SOLVE", 8, 1, f, anchor=True),
            seg("GUARDED", 9, 1, f, live=True, anchor=True), seg("GUARDED", 10, 1, f, live=True, anchor=True),
            seg("GUARDED", 11, 1, f, live=True, anchor=False)]
    fused, per_tick = plans([(2, f, 1, 1 << 2, 3, 1), (2, f, 1, 1 << 2, 3, 0)])
    assert fused == want
    # without fusing the two runs before the solves are a tick each; the rest is taken tick by tick anyway
    assert per_tick == [run_(0, 1, f), run_(1, 2, f), *want[1:5], run_(6, 7, f), run_(7, 8, f), *want[6:]]


def test_mode_1_per_tick(plans):
    f = 6
    live = {3, 4, 5, 9, 10, 11}
    assert plans([(2, f, 1, 1 << 2, 1, 0)])[0] == [
        seg("SOLVE", t, 1, f, anchor=True) if t % f == 2 else run_(t, t + 1, f, live=t in live) for t in range(12)]


def test_unscheduled(plans):
    # (the mask and the mode are not read, fused or not)
    want = [seg("SOLVE", t, 1, 3) for t in range(6)]
    assert plans([(2, 3, 0, 0, 0, 1), (2, 3, 0, 0b010, 1, 1), (2, 3, 0, 0, 3, 0)]) == [want] * 3


def test_all_ones_mask(plans):
    want = [seg("SOLVE", t, 1, 3) for t in range(6)]
    assert plans([(2, 3, 1, 0b111, 1, 1), (2, 3, 1, 0b111, 3, 1)]) == [want] * 2


def test_mask_0(plans):
    S, f = 3, 5
    assert plans([(S, f, 1, 0, m, 1) for m in (0, 1, 3)]) == [[run_(0, S * f, f)]] * 3


def test_solve_without_anchor_in_a_live_step(plans):
    """f = 4, mask {0, 3}: tick 3 solves with nothing after it to anchor for, in a step tick 0 made live: live stays
    set on that segment (the driver's anchor kernel clears the episodes' bits), and the next step starts afresh."""
    f = 4
    step = lambda t: [seg("SOLVE", t, 1, f, anchor=True), run_(t + 1, t + 3, f, live=True),   # noqa: E731
                      seg("SOLVE", t + 3, 1, f, live=True, anchor=False)]
    assert plans([(2, f, 1, 0b1001, 1, 1)])[0] == step(0) + step(4)


def test_every_mask_of_f_5(plans):
    """Every mask of f_cyc = 5 in the three modes, fused and not, from the header's description of the plan: the
    segments tile [0, S f) once and in order; SOLVE and GUARDED are one tick; a SOLVE sits on every tick of the mask and
    nowhere else; GUARDED appears in mode 3 alone and nothing is live or anchored in mode 0; no run holds a solve tick,
    a live run stays inside its step, and without fusing every run is one tick."""
    S, f = 3, 5
    cases = [(S, f, 1, mask, mode, fuse) for mask, mode, fuse in itertools.product(range(1 << f), (0, 1, 3), (1, 0))]
    for (_, _, _, mask, mode, fuse), plan in zip(cases, plans(cases)):
        t, solved = 0, []
        for kind, t0, nt, s, i, live, anchor in plan:
            assert t0 == t and nt >= 1 and (s, i) == divmod(t0, f), (mask, mode, fuse, plan)
            ticks = range(t0, t0 + nt)
            if kind == "RUN":
                assert not anchor and all(not (mask >> (u % f)) & 1 for u in ticks), (mask, mode, fuse, plan)
                assert fuse or nt == 1
                assert not live or (t0 + nt - 1) // f == s
            else:
                assert nt == 1, (mask, mode, fuse, plan)
                later = any(not (mask >> j) & 1 for j in range(i + 1, f))
                assert anchor == (later and mode != 0), (mask, mode, fuse, plan)
            if kind == "SOLVE":
                solved.append(t0)
            if kind == "GUARDED":
                assert mode == 3 and live
            if mode == 0:
                assert not live and not anchor
            if mode == 3:
                assert not (kind == "RUN" and live)
            t = t0 + nt
        assert t == S * f
        assert solved == [u for u in range(S * f) if (mask >> (u % f)) & 1]
