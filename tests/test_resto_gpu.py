"""IPOPT's feasibility restoration phase where it RECOVERS — a failed line search enters the phase, the original filter
accepts a restoration iterate, the regular iteration resumes and the solve converges — on every route an instance can
take through libalipmpc.so: the fp64 wave program in one phase, as a split launch (4-wave and paired phase 2), through
the work queue and at B = 1, and the hand-off of the fp32 wave program and of the lane programs.

scenes.make_batch scenes restore on 3-13 % of a batch and recover on almost none.  The batches here keep the scene
and move the warm start by a unit normal perturbation: most instances then restore (up to 18 times each) and most of
those recover, while the C oracle still reproduces itself from a warm start one ulp away (ROWS: the strata the oracle
measures; test_oracle_strata_hold_recovered_instances asserts them without a GPU).  Instances are split by the ORACLE
into R (restored, status 0 / 1), I (restored, status 2) and the rest, and every bar on a stratum is the oracle's own
agreement with its nudged self on that stratum, computed here, minus MARGIN — never a figure the GPU produced.

Measured GPU figures are written under $ALIPMPC_TEST_ARTIFACTS (resto_parity/*.json; profiles/resto_parity/parity.json
is their collection from one MI355X run)."""
import json
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

KEYS = ("u", "foot", "x_pred", "status", "iters")
MAX_ITER = 100
# GPU vs oracle may differ by what one ulp does to the oracle, plus a little for Gauss-Jordan vs Cholesky: the margin
# test_gpu.py::test_closed_loop_matches_oracle sets against the oracle loop's self drift
MARGIN = 0.03
# (variant, N, circles, ellipses, B, seed) — numbered as the table of DESIGN.md §2 item 4
ROWS = {1: (0, 3, 5, 0, 512, 201), 2: (1, 3, 5, 0, 512, 202), 3: (0, 5, 5, 5, 256, 203), 4: (0, 6, 3, 0, 256, 204),
        5: (0, 1, 2, 0, 512, 205), 6: (0, 3, 12, 8, 256, 206), 7: (0, 2, 0, 0, 256, 207), 8: (0, 3, 3, 2, 512, 208)}
I_ROWS = (1, 5, 6, 8)        # the oracle reproduces its own status-2 iterates there: all three shares asserted on I
I_STATUS_ROWS = (3, 4)       # it does not (footholds 0.77 / 0.20 against itself): the status share alone
MIN_R, MIN_I, MIN_CAP = 100, 25, 40
CAPS = (8, 10, 14, 20, 30)
CUTS = (2, 5, 8, 11, 16, 24)
FP32_TOLS = dict(tol=1e-4, acceptable_tol=1e-3)
# a stratum is asserted where one instance weighs less than the margin (1 / 34 < 0.03); smaller ones are recorded
MIN_ASSERTED = 34


# ---------------------------------------------------------------------------------------------------- inputs, oracle
def _batch(row, B=None, perturb=True):
    from alipmpc import scenes
    _, N, n_cir, n_elp, B0, seed = ROWS[row]
    bt = scenes.make_batch(B or B0, seed, n_cir, n_elp, N)
    if perturb:
        bt["u0"] = bt["u0"] + 1.0 * np.random.default_rng(seed + 1000).standard_normal(bt["u0"].shape)
    return bt


def _take(bt, idx):
    return {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in bt.items()}


def _oracle(coracle, row, bt, u0=None, **kw):
    variant, N, n_cir, n_elp = ROWS[row][:4]
    cfg = coracle.default_cfg(variant, N, nc_max=n_cir, ne_max=n_elp, **{"max_iter": MAX_ITER, **kw})
    return coracle.solve_batch(cfg, bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt["elp"], bt["ne"],
                               bt["u0"] if u0 is None else u0, nthreads=8)


_CASES = {}


def _case(coracle, row, B=None, nudged=False, **kw):
    """(batch, oracle solve[, the same oracle solve from np.nextafter(u0, inf)]) of a row, computed once per session."""
    key = (row, B, tuple(sorted(kw.items())))
    c = _CASES.setdefault(key, {})
    if "ref" not in c:
        c["bt"] = _batch(row, B)
        c["ref"] = _oracle(coracle, row, c["bt"], **kw)
    if nudged and "nud" not in c:
        c["nud"] = _oracle(coracle, row, c["bt"], u0=np.nextafter(c["bt"]["u0"], np.inf), **kw)
    return (c["bt"], c["ref"], c["nud"]) if nudged else (c["bt"], c["ref"])


def _strata(ref):
    rs = ref["restorations"] > 0
    R = rs & ((ref["status"] == 0) | (ref["status"] == 1))
    I = rs & (ref["status"] == 2)
    return {"R": R, "I": I, "rest": ~(R | I), "all": np.ones(len(rs), bool)}


# ---------------------------------------------------------------------------------------------------- measures
def _close(out, ref):
    """test_gpu.py::_compare's measure per instance: foothold and predicted states within 1e-4 relative."""
    B = len(ref["status"])
    ok = np.all(np.abs(out["foot"] - ref["foot"]) <= 1e-4 * np.maximum(1.0, np.abs(ref["foot"])), axis=1)
    dx = np.abs(out["x_pred"] - ref["x_pred"]).reshape(B, -1)
    return ok & np.all(dx <= 1e-4 * np.maximum(1.0, np.abs(ref["x_pred"]).reshape(B, -1)), axis=1)


def _foot_rel(out, ref):
    return np.max(np.abs(out["foot"] - ref["foot"]) / np.maximum(1.0, np.abs(ref["foot"])), axis=1)


def _shares(out, ref, sel):
    n = int(sel.sum())
    if n == 0:
        return {"n": 0}
    return {"n": n, "status": float((out["status"] == ref["status"])[sel].mean()),
            "foot": float(_close(out, ref)[sel].mean()), "iters": float((out["iters"] == ref["iters"])[sel].mean()),
            "foot_rel_median": float(np.median(_foot_rel(out, ref)[sel]))}


def _check_bars(tag, got, own, keys):
    """Every share of `got` (GPU vs oracle) reaches the oracle's share against its nudged self minus MARGIN."""
    for k in keys:
        assert got[k] >= own[k] - MARGIN, (tag, k, "gpu", got, "oracle self", own)


def _always(out, B, N, max_iter):
    assert np.isfinite(out["u"]).all() and np.isfinite(out["foot"]).all()
    assert (out["iters"] <= max_iter).all() and (out["iters"] >= 0).all(), out["iters"].max()
    assert np.array_equal(out["u"].reshape(B, N, 5), out["x_pred"])   # bit for bit


def _same_rows(a, b):
    """Per instance: the five outputs equal bit for bit."""
    B = len(a["status"])
    eq = np.ones(B, bool)
    for k in KEYS:
        eq &= (a[k].reshape(B, -1) == b[k].reshape(B, -1)).all(axis=1)
    return eq


def _record(name, obj):
    """A small JSON record of a case's measured numbers under $ALIPMPC_TEST_ARTIFACTS/resto_parity (if set)."""
    d = os.environ.get("ALIPMPC_TEST_ARTIFACTS")
    if d:
        d = os.path.join(d, "resto_parity")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as fh:
            json.dump(obj, fh, indent=1)


# ---------------------------------------------------------------------------------------------------- GPU side
def _solver(gpu_lib, row, **kw):
    variant, N, n_cir, n_elp = ROWS[row][:4]
    return gpu_lib.Solver(gpu_lib.default_cfg(variant, N, nc_max=n_cir, ne_max=n_elp, **{"max_iter": MAX_ITER, **kw}))


def _run(s, bt):
    return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt["elp"], bt["ne"], u0=bt["u0"])


def _form(gpu_lib, monkeypatch, row, cut, pair, **kw):
    """A handle of the row's shape with the split launch cut at `cut` iterations (0: one phase) and the paired
    (True) or 4-wave (False) phase 2; the environment is read when the handle is made."""
    monkeypatch.setenv("ALIPMPC_SPLIT_IT", str(cut))
    monkeypatch.setenv("ALIPMPC_SPLIT_PAIR", "1" if pair else "0")
    monkeypatch.setenv("ALIPMPC_SPLIT_TR", "0")
    return _solver(gpu_lib, row, **kw)


# ---------------------------------------------------------------------------------------------------- CPU: the strata
@pytest.mark.parametrize("row", sorted(ROWS))
def test_oracle_strata_hold_recovered_instances(coracle, row):
    """The conditions the GPU tests stand on, checked on the oracle alone: every row holds at least MIN_R recovered
    instances, rows I_ROWS at least MIN_I that end infeasible after restoring; rows 1 and 8 keep their strata at the
    fp32 handles' tolerances; row 1 at B = 256 has at least MIN_CAP instances that have restored by every cap of
    CAPS."""
    _, ref = _case(coracle, row)
    st = _strata(ref)
    assert st["R"].sum() >= MIN_R, st["R"].sum()
    if row in I_ROWS:
        assert st["I"].sum() >= MIN_I, st["I"].sum()
    if row in (1, 8):
        st32 = _strata(_case(coracle, row, **FP32_TOLS)[1])
        assert st32["R"].sum() >= MIN_R and st32["I"].sum() >= MIN_I, (st32["R"].sum(), st32["I"].sum())
    if row == 1:
        for cap in CAPS:
            restored = _case(coracle, 1, B=256, max_iter=cap)[1]["restorations"] > 0
            assert restored.sum() >= MIN_CAP, (cap, restored.sum())


# ---------------------------------------------------------------------------------------------------- 1. parity
@gpu
@pytest.mark.parametrize("row", sorted(ROWS))
def test_recovered_restorations_vs_oracle(gpu_lib, coracle, row):
    """fp64 wave program against the C oracle, stratified by the oracle: per stratum the shares of instances with the
    oracle's status, with its foothold and predicted states (1e-4 relative) and with its iteration count — the
    restoration's iterations are part of the count, so it is the visible trace of how long the phase ran.  Each bar
    is the oracle's share on that stratum against its own solve from np.nextafter(u0, inf), minus MARGIN.  R: all
    three shares on every row, and the median relative foothold error at most 1000 x the oracle's self median
    (floored at 1e-12).  I: all three on I_ROWS, the status share on I_STATUS_ROWS.  The rest of the batch: all three
    where it holds MIN_ASSERTED instances (rows 3, 4 and 6 leave 14, 18 and 24: recorded).  The whole batch's shares
    are recorded too; they are not asserted, since on rows 3 and 4 they move with the I iterates the oracle does not
    reproduce."""
    variant, N, n_cir, n_elp, B, _ = ROWS[row]
    bt, ref, nud = _case(coracle, row, nudged=True)
    st = _strata(ref)
    assert st["R"].sum() >= MIN_R and (row not in I_ROWS or st["I"].sum() >= MIN_I)
    out = _run(_solver(gpu_lib, row), bt)
    got = {k: _shares(out, ref, sel) for k, sel in st.items()}
    own = {k: _shares(nud, ref, sel) for k, sel in st.items()}
    med_bar = max(1000.0 * own["R"]["foot_rel_median"], 1e-12)
    _record(f"parity_row{row}", {"row": row, "variant": variant, "N": N, "n_cir": n_cir, "n_elp": n_elp, "B": B,
                                 "max_restorations": int(ref["restorations"].max()), "gpu_vs_oracle": got,
                                 "oracle_vs_nudged_self": own, "R_foot_rel_median_bar": med_bar})
    print(f"row {row}: gpu {got}\n        self {own}")
    _always(out, B, N, MAX_ITER)
    three = ("status", "foot", "iters")
    _check_bars((row, "R"), got["R"], own["R"], three)
    if row in I_ROWS:
        _check_bars((row, "I"), got["I"], own["I"], three)
    elif row in I_STATUS_ROWS:
        _check_bars((row, "I"), got["I"], own["I"], ("status",))
    if got["rest"]["n"] >= MIN_ASSERTED:
        _check_bars((row, "rest"), got["rest"], own["rest"], three)
    assert got["R"]["foot_rel_median"] <= med_bar, (got["R"]["foot_rel_median"], own["R"]["foot_rel_median"])


# ---------------------------------------------------------------------------------------------------- 2. the cap
@gpu
@pytest.mark.parametrize("max_iter", CAPS)
def test_iteration_cap_inside_restoration(gpu_lib, coracle, max_iter):
    """Row 1 at B = 256 stopped by max_iter inside its restoration sequences: the iterate in the middle of a sequence,
    the counting of restoration iterations against the cap and the stop rule at the cap (an instance the cap stops
    inside the phase ends with status 2, one it stops in a regular iteration with -1).  Stratum: the instances the
    oracle has restored by the cap; bars as test_recovered_restorations_vs_oracle.  An instance the oracle stops at the
    cap has nothing left to diverge in its count: the GPU's iters equal the oracle's on every one of them."""
    N = ROWS[1][1]
    bt, ref, nud = _case(coracle, 1, B=256, nudged=True, max_iter=max_iter)
    S = ref["restorations"] > 0
    assert S.sum() >= MIN_CAP, S.sum()
    out = _run(_solver(gpu_lib, 1, max_iter=max_iter), bt)
    got, own = _shares(out, ref, S), _shares(nud, ref, S)
    at_cap = (ref["iters"] == max_iter) & (ref["status"] != 0) & (ref["status"] != 1)
    cap_equal = int((out["iters"][at_cap] == ref["iters"][at_cap]).sum())
    _record(f"cap_{max_iter}", {"max_iter": max_iter, "B": 256, "gpu_vs_oracle": got, "oracle_vs_nudged_self": own,
                                "oracle_stops_at_cap": int(at_cap.sum()), "gpu_iters_equal_there": cap_equal,
                                "oracle_status_in_stratum": {str(k): int(v) for k, v in
                                                             zip(*np.unique(ref["status"][S], return_counts=True))}})
    print(f"cap {max_iter}: gpu {got}\n        self {own}  at cap {int(at_cap.sum())} equal {cap_equal}")
    _always(out, 256, N, max_iter)
    _check_bars(max_iter, got, own, ("status", "foot", "iters"))
    assert at_cap.sum() >= MIN_CAP and cap_equal == at_cap.sum(), (cap_equal, at_cap.sum())


# ---------------------------------------------------------------------------------------------------- 3. launch forms
def _forms_batch(coracle, row):
    """B = 64: 32 recovered instances (spread over the oracle's restoration counts, 1 to the row's largest) at the even
    positions, 32 that never restore at the odd ones.  Where the perturbed batch holds fewer than 32 that never restore
    (row 3: 10), the others are instances of the same scenes from make_batch's own warm start, which the oracle solves
    without restoring."""
    bt, ref = _case(coracle, row)
    R = np.flatnonzero(_strata(ref)["R"])
    R = R[np.argsort(ref["restorations"][R], kind="stable")]
    rec = R[np.linspace(0, len(R) - 1, 32).astype(int)]
    calm = np.flatnonzero(ref["restorations"] == 0)[:32]
    parts = [_take(bt, rec), _take(bt, calm)]
    if len(calm) < 32:
        plain = _batch(row, perturb=False)
        more = np.flatnonzero(_oracle(coracle, row, plain)["restorations"] == 0)[:32 - len(calm)]
        parts.append(_take(plain, more))
    cat = {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in parts[0]}
    assert len(cat["x0"]) == 64
    order = np.empty(64, int)
    order[0::2], order[1::2] = np.arange(32), np.arange(32, 64)
    b64 = _take(cat, order)
    o64 = _oracle(coracle, row, b64)
    is_rec = np.arange(64) % 2 == 0
    assert (_strata(o64)["R"] == is_rec).all() and (o64["restorations"][~is_rec] == 0).all()
    return b64, o64, is_rec


@gpu
@pytest.mark.parametrize("row", [1, 3])
def test_launch_forms_with_recovered_restorations(gpu_lib, coracle, monkeypatch, row):
    """test_wave_helpers_gpu.py::_three_forms' contract — u, foot, x_pred, status, iters bit for bit — on a batch whose
    restoring instances RECOVER (rows 1 and 3: one and two row groups per lane): one phase, the split launch cut at
    every iteration of CUTS with the 4-wave and the paired phase 2, the work queue (the 64 instances tiled beyond the
    resident slots, every copy compared) and 8 recovered instances at B = 1.

    Where the cuts land.  The oracle's recovered instances take 24+ iterations (row 3: 32+), so none can finish
    below a cut: every one crosses every cut, which is asserted.  What differs per cut is the record it leaves: a
    failed line search before the cut cuts the instance there with its restoration pending, otherwise the cut's own
    record is written ahead of the first restoration.  The oracle stopped at the cut tells the two apart
    (restorations > 0 by then); asserted: the smallest cut is ahead of the first restoration of some recovered
    instances, the largest behind it for some, and at least one cut separates the recovered instances into both
    kinds."""
    variant, N = ROWS[row][:2]
    bt, o64, is_rec = _forms_batch(coracle, row)
    s1 = _form(gpu_lib, monkeypatch, row, 0, True)
    ref = _run(s1, bt)
    assert s1.solve_launches(64)[0] == 1
    _always(ref, 64, N, MAX_ITER)
    # (a condition, not a parity bar — that is test_recovered_restorations_vs_oracle's: the batch holds recovered
    # instances on the GPU too, at least half of the oracle's 32)
    rec_gpu = is_rec & np.isin(ref["status"], (0, 1))
    assert rec_gpu.sum() >= 16, (ref["status"], ref["iters"])
    kinds = {}
    for cut in CUTS:
        by_cut = _oracle(coracle, row, bt, max_iter=cut)["restorations"][is_rec] > 0
        kinds[cut] = (int(by_cut.sum()), int((~by_cut).sum()))   # (restoration pending at the cut, cut ahead of it)
        for pair in (False, True):
            s = _form(gpu_lib, monkeypatch, row, cut, pair)
            assert s.solve_launches(64)[0] == 2
            o = _run(s, bt)
            for k in KEYS:
                assert np.array_equal(o[k], ref[k]), (cut, pair, k, np.flatnonzero(~_same_rows(o, ref)))
    assert (ref["iters"][rec_gpu] > CUTS[-1]).all(), ref["iters"][rec_gpu]   # every recovered instance crosses every cut
    assert kinds[CUTS[0]][1] > 0 and kinds[CUTS[-1]][0] > 0 and any(a > 0 and b > 0 for a, b in kinds.values()), kinds
    # the work queue
    B = s1.solve_slots() + 64
    idx = np.arange(B) % 64
    assert s1.solve_launches(B)[0] == 1
    big = _run(s1, _take(bt, idx))
    for k in KEYS:
        assert np.array_equal(big[k], ref[k][idx]), (k, np.flatnonzero(~_same_rows(big, {q: ref[q][idx] for q in KEYS})))
    # B = 1, default launch settings
    for v in ("ALIPMPC_SPLIT_IT", "ALIPMPC_SPLIT_PAIR", "ALIPMPC_SPLIT_TR"):
        monkeypatch.delenv(v, raising=False)
    sd = _solver(gpu_lib, row)
    for b in np.flatnonzero(is_rec)[::4]:
        o = _run(sd, _take(bt, np.array([b])))
        for k in KEYS:
            assert np.array_equal(o[k][0], ref[k][b]), (b, k)
    _record(f"forms_row{row}", {"row": row, "recovered_on_gpu": int(rec_gpu.sum()),
                                "recovered_iters_min_max": [int(ref["iters"][rec_gpu].min()),
                                                            int(ref["iters"][rec_gpu].max())],
                                "oracle_restorations_max": int(o64["restorations"].max()),
                                "status_equal_oracle": float((ref["status"] == o64["status"]).mean()),
                                "recovered_pending_or_ahead_at_cut": {str(c): v for c, v in kinds.items()},
                                "work_queue_B": int(B)})


# ---------------------------------------------------------------------------------------------------- 4. the hand-off
HANDLES = {"wave_fp32": (1, dict(precision=1, program=0, **FP32_TOLS), FP32_TOLS),
           "lane_fp32": (1, dict(precision=1, program=1, **FP32_TOLS), FP32_TOLS),
           "lane_fp64": (1, dict(program=1), {}),
           "lane_form_fp64": (8, dict(program=1), {})}


@gpu
@pytest.mark.parametrize("name", sorted(HANDLES))
def test_handoff_equals_fp64_wave_program(gpu_lib, coracle, name):
    """include/alipmpc.h: an instance whose line search fails in the fp32 wave program or in a lane program is solved
    from its start by the fp64 wave program's work queue, and an instance's result does not depend on its batch or
    launch form.  So every handed-off instance's five outputs equal, bit for bit, those of an fp64 wave handle with the
    same tol, acceptable_tol and max_iter: at least lane_handoffs() instances do (which ones were handed off the ABI
    does not say), and at least 100 are handed off.  A second solve gives the same bits and the same count (the list
    starts empty at every solve), and so do solves through device pointers on a stream of the caller's.  On the
    oracle's R stratum, at the handle's tolerances, the status and foothold shares reach the same-tolerance oracle's
    self shares minus MARGIN.  (The list across graph capture and growth, and with many solves in flight:
    tests/test_streams_gpu.py.)"""
    import torch
    row, kw, tols = HANDLES[name]
    variant, N, n_cir, n_elp, B, _ = ROWS[row]
    bt, ref, nud = _case(coracle, row, nudged=True, **tols)
    R = _strata(ref)["R"]
    assert R.sum() >= MIN_R
    s = _solver(gpu_lib, row, **kw)
    want = "lane_kernel" if kw["program"] else f"solve_kernel<{N},"
    assert s.solve_program().startswith(want) and ("float" in s.solve_program()) == bool(kw.get("precision"))
    o1 = _run(s, bt)
    h1 = s.lane_handoffs()
    w64 = _run(_solver(gpu_lib, row, **tols), bt)
    eq = _same_rows(o1, w64)
    got, own = _shares(o1, ref, R), _shares(nud, ref, R)
    rec = {"handle": name, "row": row, "B": B, "lane_handoffs": h1, "rows_equal_fp64_wave_handle": int(eq.sum()),
           "oracle_restores": int((ref["restorations"] > 0).sum()), "gpu_vs_oracle_R": got,
           "oracle_vs_nudged_self_R": own}
    _record(f"handoff_{name}", rec)
    print(rec)
    _always(o1, B, N, MAX_ITER)
    assert h1 >= 100, h1
    assert eq.sum() >= h1, (int(eq.sum()), h1)
    o2 = _run(s, bt)
    assert _same_rows(o2, o1).all() and s.lane_handoffs() == h1
    # device pointers, a stream of the caller's
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
    inp["leg"] = inp["leg"].to(torch.int8)
    inp["nc"] = inp["nc"].to(torch.int32)
    if "ne" in inp:
        inp["ne"] = inp["ne"].to(torch.int32)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    for _ in range(2):
        out = {"u": torch.full((B, 5 * N), float("nan"), dtype=torch.float64, device=dev),
               "foot": torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev),
               "x_pred": torch.full((B, N, 5), float("nan"), dtype=torch.float64, device=dev),
               "status": torch.full((B,), -99, dtype=torch.int32, device=dev),
               "iters": torch.full((B,), -99, dtype=torch.int32, device=dev)}
        torch.cuda.synchronize()
        s.solve_device(inp, out, stream=st)
        assert s.lane_handoffs(st) == h1       # (synchronises the stream)
        od = {k: v.cpu().numpy() for k, v in out.items()}
        assert _same_rows(od, o1).all(), np.flatnonzero(~_same_rows(od, o1))
    _check_bars(name, got, own, ("status", "foot"))
