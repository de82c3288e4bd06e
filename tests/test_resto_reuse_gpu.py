"""The restoration phase works on its caller's row registers and hands back what it computed (csrc/resto_wave.inc):
nothing is decoded or evaluated twice around a call, and no output bit moves.

1. Frozen bits.  tests/golden/resto_reuse_bits.npz holds status, iters and the raw 64-bit patterns of u, foot and
   x_pred of the B = 64 batches of test_resto_gpu._forms_batch (rows 1 and 3: 32 recovered instances spread over the
   oracle's restoration counts, 32 that never restore), through the default split launch and through the one-phase
   launch, as the build BEFORE the reuse computed them.  The file is the project's own output and is regenerated
   (python tests/test_resto_reuse_gpu.py --regenerate, on the GPU) only by a change that alters the restoration's
   arithmetic on purpose.
2. Every exit of the phase at a small shape: B = 64 of row 1 under iteration caps, against the C oracle with
   test_resto_gpu.test_iteration_cap_inside_restoration's comparison.  The caps are held, without a GPU, to contain
   every exit (test_caps_contain_every_exit).
3. Two row groups per lane (N = 5, 5 + 5 obstacle slots) through the work queue, against the C oracle.
4. B = 1 (one phase) and B = 2 (the smallest split launch) on recovered instances of 1., equal to their rows of the
   B = 64 run bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_resto_gpu as T  # noqa: E402

gpu = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resto_reuse_bits.npz")
FROZEN_ROWS = (1, 3)
FORMS = ("split", "one")            # the default launch of B = 64 (split, paired phase 2) / ALIPMPC_SPLIT_IT=0
# 8, 12, 20, 30 stop instances inside their restorations and hold both kinds of return through the original-problem
# check; the oracle's infeasible returns on this batch come after more than 30 iterations, so the uncapped solve
# (MAX_ITER) is the fifth case
EXIT_CAPS = (8, 12, 20, 30, T.MAX_ITER)
SPLIT_ENV = ("ALIPMPC_SPLIT_IT", "ALIPMPC_SPLIT_PAIR", "ALIPMPC_SPLIT_TR")

_FORMS = {}
_RUNS = {}


def _forms_batch(coracle, row):
    if row not in _FORMS:
        _FORMS[row] = T._forms_batch(coracle, row)
    return _FORMS[row]


def _set_form(setenv, delenv, form):
    for v in SPLIT_ENV:
        delenv(v)
    if form == "one":
        setenv("ALIPMPC_SPLIT_IT", "0")


def _form_run(gpu_lib, coracle, setenv, delenv, row, form):
    """The row's B = 64 batch through one launch form (the environment is read when the handle is made), once per
    session."""
    if (row, form) not in _RUNS:
        bt = _forms_batch(coracle, row)[0]
        _set_form(setenv, delenv, form)
        s = T._solver(gpu_lib, row)
        assert s.solve_launches(64)[0] == (2 if form == "split" else 1)
        _RUNS[row, form] = T._run(s, bt)
    return _RUNS[row, form]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _mp(monkeypatch):
    return monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------------------------------------------- 1. frozen bits
@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("row", FROZEN_ROWS)
def test_frozen_bits(gpu_lib, coracle, monkeypatch, row, form):
    """status, iters and every bit of u, foot, x_pred equal what the build before the reuse computed."""
    want = np.load(GOLDEN)
    out = _form_run(gpu_lib, coracle, *_mp(monkeypatch), row, form)
    T._always(out, 64, T.ROWS[row][1], T.MAX_ITER)
    is_rec = _forms_batch(coracle, row)[2]
    assert (is_rec & np.isin(out["status"], (0, 1))).sum() >= 16    # the batch recovers on the GPU
    for k in T.KEYS:
        got, ref = _bits(out[k]), want[f"row{row}_{form}_{k}"]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (k, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(got, ref), (row, form, k, np.flatnonzero((got != ref).reshape(64, -1).any(axis=1)))


# ---------------------------------------------------------------------------------------------------- 2. every exit
def _exit_counts(coracle, cap):
    """What the restoration calls of the oracle's run of row 1, B = 64, under the cap end in: the numpy oracle's
    calls (np_oracle._resto, spied as tests/test_oracle.py does), counted on the instances whose status and iteration
    count the C oracle — the reference of the GPU comparison — reproduces.  'first' / 'later': left through the
    original-problem check after one / after more restoration iterations."""
    import np_oracle as O
    bt, ref = T._case(coracle, 1, B=64, max_iter=cap)
    cfg = O.default_cfg(0, 3, nc_max=5, ne_max=0, max_iter=cap)
    cnt = dict(maxiter=0, infeasible=0, first=0, later=0, instances=0)
    calls = []
    orig = O._resto

    def spy(*a):
        r = orig(*a)
        calls.append((r[0], a[13], r[5]))     # (code, it on entry, it on return)
        return r
    O._resto = spy
    try:
        for i in np.flatnonzero(ref["restorations"] > 0):
            del calls[:]
            pr = O.Problem(cfg, bt["x0"][i], bt["goal"][i], bt["leg"][i], bt["cir"][i][:bt["nc"][i]], np.zeros((0, 5)))
            _, st, it = O.solve_footholds(pr, bt["u0"][i])
            if st != ref["status"][i] or it != ref["iters"][i] or len(calls) != ref["restorations"][i]:
                continue
            cnt["instances"] += 1
            for code, it0, it1 in calls:
                if code == "ok":
                    cnt["first" if it1 - it0 == 1 else "later"] += it1 > it0
                elif code in ("maxiter", "infeasible"):
                    cnt[code] += 1
    finally:
        O._resto = orig
    return cnt


def test_caps_contain_every_exit(coracle):
    """Without a GPU: under one or another cap of EXIT_CAPS the oracle's run holds an instance stopped inside a
    restoration, one the restoration returns as infeasible, one that leaves through the original-problem check on
    its first eligible iteration and one that leaves on a later one; the caps below MAX_ITER alone hold the stops
    inside the phase and both kinds of return."""
    tot = {}
    low = {}
    for cap in EXIT_CAPS:
        c = _exit_counts(coracle, cap)
        print(cap, c)
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
            if cap < T.MAX_ITER:
                low[k] = low.get(k, 0) + v
    assert min(tot["maxiter"], tot["infeasible"], tot["first"], tot["later"]) > 0, tot
    assert min(low["maxiter"], low["first"], low["later"]) > 0, low


@gpu
@pytest.mark.parametrize("max_iter", EXIT_CAPS)
def test_every_exit_under_caps(gpu_lib, coracle, max_iter):
    """Row 1 at B = 64 under the cap, against the C oracle: test_iteration_cap_inside_restoration's comparison.  The
    stratum is the instances the oracle has restored by the cap; each share (status, foothold, iteration count)
    reaches the oracle's share against its own solve from a warm start one ulp away, minus MARGIN, and every instance
    the oracle stops at the cap has the oracle's count."""
    N = T.ROWS[1][1]
    bt, ref, nud = T._case(coracle, 1, B=64, nudged=True, max_iter=max_iter)
    S = ref["restorations"] > 0
    assert S.sum() > 0
    out = T._run(T._solver(gpu_lib, 1, max_iter=max_iter), bt)
    got, own = T._shares(out, ref, S), T._shares(nud, ref, S)
    at_cap = (ref["iters"] == max_iter) & (ref["status"] != 0) & (ref["status"] != 1)
    cap_equal = int((out["iters"][at_cap] == ref["iters"][at_cap]).sum())
    print(f"cap {max_iter}: gpu {got}\n        self {own}  at cap {int(at_cap.sum())} equal {cap_equal}")
    T._always(out, 64, N, max_iter)
    T._check_bars(max_iter, got, own, ("status", "foot", "iters"))
    assert (at_cap.sum() > 0 or max_iter == T.MAX_ITER) and cap_equal == at_cap.sum(), (cap_equal, at_cap.sum())


# ---------------------------------------------------------------------------------------------------- 3. two row groups
@gpu
def test_two_row_groups_work_queue(gpu_lib, coracle):
    """Row 3 (N = 5, 5 circle and 5 ellipse slots: two row groups per lane, the build whose register pressure decides
    which parts of the reuse apply), B = 32 tiled beyond the resident slots so that the work queue runs it.  Every copy
    equals the first bit for bit, and the first equals the same 32 instances through the resident launch.  Against
    the C oracle, bars as test_recovered_restorations_vs_oracle's (the oracle's share against its solve from a warm
    start one ulp away, minus MARGIN): the recovered stratum R on status and foothold, the infeasible stratum I on
    status (the oracle does not reproduce its own status-2 iterates on this row, test_resto_gpu.I_STATUS_ROWS).  The
    iteration-count share is asserted where test_resto_gpu asserts a small stratum, at MIN_ASSERTED instances: the
    count of a restoring instance follows its path (one ulp moves it on 4 of the oracle's own 21 in R here), and below
    that size one instance weighs more than the margin; it is printed."""
    N = T.ROWS[3][1]
    bt, ref, nud = T._case(coracle, 3, B=32, nudged=True)
    st = T._strata(ref)
    assert st["R"].sum() >= 16 and st["I"].sum() >= 4, (st["R"].sum(), st["I"].sum())
    s = T._solver(gpu_lib, 3)
    B = s.solve_slots() + 32
    assert s.solve_launches(B)[0] == 1 and s.solve_launches(32)[0] == 2
    idx = np.arange(B) % 32
    big = T._run(s, T._take(bt, idx))
    T._always(big, B, N, T.MAX_ITER)
    out = {k: big[k][:32] for k in T.KEYS}
    res = T._run(s, bt)
    for k in T.KEYS:
        assert np.array_equal(big[k], out[k][idx]), k
        assert np.array_equal(out[k], res[k]), (k, np.flatnonzero(~T._same_rows(out, res)))
    got = {k: T._shares(out, ref, sel) for k, sel in st.items()}
    own = {k: T._shares(nud, ref, sel) for k, sel in st.items()}
    print(f"gpu {got}\nself {own}")
    for tag, keys in (("R", ("status", "foot")), ("I", ("status",))):
        T._check_bars(tag, got[tag], own[tag], keys + (("iters",) if got[tag]["n"] >= T.MIN_ASSERTED else ()))


# ---------------------------------------------------------------------------------------------------- 4. B = 1, B = 2
@gpu
@pytest.mark.parametrize("row", FROZEN_ROWS)
def test_smallest_batches(gpu_lib, coracle, monkeypatch, row):
    """Recovered instances of the B = 64 batch alone (B = 1: one phase) and with their calm neighbour (B = 2: the
    smallest split launch), default launch settings: the rows of the B = 64 run, bit for bit."""
    setenv, delenv = _mp(monkeypatch)
    ref = _form_run(gpu_lib, coracle, setenv, delenv, row, "split")
    bt, _, is_rec = _forms_batch(coracle, row)
    _set_form(setenv, delenv, "split")
    s = T._solver(gpu_lib, row)
    assert s.solve_launches(1)[0] == 1 and s.solve_launches(2)[0] == 2
    for b in np.flatnonzero(is_rec)[::4]:
        for idx in (np.array([b]), np.array([b, b + 1])):
            o = T._run(s, T._take(bt, idx))
            for k in T.KEYS:
                assert np.array_equal(_bits(o[k]), _bits(ref[k][idx])), (b, len(idx), k)


# ---------------------------------------------------------------------------------------------------- regeneration
if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_resto_reuse_gpu.py --regenerate   (on the GPU; see the module docstring)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "mujoco-lip-mpc-simulation_amd"), os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    import alipmpc
    import oracle
    oracle.build()
    arrays = {}
    for row_ in FROZEN_ROWS:
        for form_ in FORMS:
            o_ = _form_run(alipmpc, oracle, os.environ.__setitem__, lambda v: os.environ.pop(v, None), row_, form_)
            for k_ in T.KEYS:
                arrays[f"row{row_}_{form_}_{k_}"] = _bits(o_[k_])
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes; library build", alipmpc.build_id())
