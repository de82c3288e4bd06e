"""The lane program's obstacle-form build (csrc/lane_solve.inc, lane_kernel<3,5,true,Form<R>>): modi, N = 3, circles
and ellipses in nc_max + ne_max <= 5 quadratic-form slots, through the C ABI against the C oracle (oracle/), which
takes elp / ne.  Batches and oracle solves are computed once per session and shared (never modified)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle_solve(coracle, cfg_kw, bt, nthreads=8):
    cfg = coracle.default_cfg(**cfg_kw)
    return coracle.solve_batch(cfg, bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt.get("elp"),
                               bt.get("ne"), bt["u0"], nthreads=nthreads)


def _compare(out, ref, min_conv=0.8, min_agree=0.97, min_status=0.97):
    """Parity on the foothold p_list[0] and the predicted states where both solves converged (the NLP is
    nonconvex: rounding-level differences can steer a few instances into another basin)."""
    both = (out["status"] == 0) & (ref["status"] == 0)
    assert both.mean() >= min_conv, both.mean()
    scale = np.maximum(1.0, np.abs(ref["foot"]))
    ok = np.all(np.abs(out["foot"] - ref["foot"]) <= 1e-4 * scale, axis=1)
    okx = np.all(np.abs(out["x_pred"] - ref["x_pred"]).reshape(len(ok), -1) <= 1e-4 * np.maximum(1.0, np.abs(ref["x_pred"]).reshape(len(ok), -1)), axis=1)
    agree = (ok & okx)[both].mean()
    assert agree >= min_agree, agree
    same_status = (out["status"] == ref["status"]).mean()
    assert same_status >= min_status, same_status
    return agree


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The seeded batches of this file (read-only; (batch, nc_max, ne_max))."""
    from alipmpc import scenes
    if name == "vec":
        return scenes.make_batch_vec(512, seed=7301, n_cir=3, n_elp=2, N=3), 3, 2
    if name == "mix":
        return scenes.make_batch(1024, seed=7303, n_cir=3, n_elp=2), 3, 2
    if name == "ragged":   # nc = 2 < nc_max = 3: an unused circle slot ahead of the ellipse slots
        return scenes.make_batch(1024, seed=7304, n_cir=2, n_elp=2, nc_max=3, ne_max=2), 3, 2
    if name == "elp_only":   # the mix batch with every circle switched off
        bt, ncm, nem = _batch("mix")
        bt = dict(bt)
        bt["nc"] = np.zeros_like(bt["nc"])
        return bt, ncm, nem
    raise KeyError(name)


_REF = {}


def _ref(coracle, name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        bt, ncm, nem = _batch(name)
        _REF[key] = _oracle_solve(coracle, dict(variant=0, N=3, nc_max=ncm, ne_max=nem, **kw), bt)
    return _REF[key]


def _lane(gpu_lib, nc_max, ne_max, prec=0, variant=0, **kw):
    if prec:
        kw["precision"] = gpu_lib.PREC_FP32
    return gpu_lib.Solver(gpu_lib.default_cfg(variant, 3, nc_max=nc_max, ne_max=ne_max, program=gpu_lib.PROGRAM_LANE,
                                              **kw))


def _solve(s, bt):
    return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt.get("elp"), bt.get("ne"), u0=bt["u0"])


def _elp_in_range(bt, r2=16.0):
    """Share of the instances with at least one ellipse inside select_obs's range (np_oracle.select_obs)."""
    d = bt["x0"][:, None, :2] - bt["elp"][:, :, :2]
    rm = np.maximum(bt["elp"][:, :, 2], bt["elp"][:, :, 3])
    inr = (d[..., 0] ** 2 + d[..., 1] ** 2 - rm ** 2 <= r2) & (np.arange(bt["elp"].shape[1])[None, :] < bt["ne"][:, None])
    return float(inr.any(axis=1).mean())


@pytest.mark.parametrize("prec", [0, 1])
def test_lane_elp_create_rule(gpu_lib, prec):
    """ne_max >= 1 on the lane program: modi, N = 3, nc_max + ne_max <= 5 take the form build; more slots and sig_step
    are refused.  The program string names the build and differs from the circle build's."""
    cir5 = _lane(gpu_lib, 5, 0, prec).solve_program()
    progs = set()
    for ncm, nem in ((3, 2), (0, 5), (4, 1), (2, 1)):
        s = _lane(gpu_lib, ncm, nem, prec)
        p = s.solve_program()
        assert p.startswith("lane_kernel<3,") and p != cir5, p
        assert "Form<" in p and ("float" in p) == bool(prec), p
        assert s.solve_slots() > 0
        progs.add(p)
    assert len(progs) == 1, progs   # one build serves every supported (nc_max, ne_max)
    for ncm, nem, variant in ((3, 3, 0), (5, 1, 0), (3, 2, 1)):
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            _lane(gpu_lib, ncm, nem, prec, variant=variant)


@pytest.mark.parametrize("name,select_obs", [("vec", 1), ("vec", 0), ("ragged", 1)])
@pytest.mark.parametrize("max_iter", [1, 3])
def test_lane_elp_first_iterates(gpu_lib, coracle, name, select_obs, max_iter):
    """The form rows' value, coefficients and Hessian blocks, pinned by the first interior-point iterates against the
    C oracle with test_first_iterates_pin_solve_callbacks's bars (a wrong coefficient or a swapped a / b shows at
    iteration 1)."""
    bt, ncm, nem = _batch(name)
    assert _elp_in_range(bt) >= 0.5, _elp_in_range(bt)   # else the batch pins nothing
    o = _solve(_lane(gpu_lib, ncm, nem, max_iter=max_iter, select_obs=select_obs), bt)
    ref = _ref(coracle, name, max_iter=max_iter, select_obs=select_obs)
    B = len(bt["x0"])
    assert np.array_equal(o["iters"] <= max_iter, np.ones(B, bool))
    scale = np.maximum(1.0, np.abs(ref["u"]))
    err = (np.abs(o["u"] - ref["u"]) / scale).max(axis=1)
    print("first iterates", name, select_obs, max_iter, np.mean(err <= 1e-8), np.median(err),
          (o["status"] == ref["status"]).mean())
    assert np.mean(err <= 1e-8) >= 0.99, (np.mean(err <= 1e-8), np.median(err))
    assert np.median(err) <= 1e-11, np.median(err)
    assert (o["status"] == ref["status"]).mean() >= 0.99


def _common(o):
    assert np.array_equal(o["u"].reshape(-1, 3, 5), o["x_pred"])
    for k in ("u", "foot", "x_pred"):
        assert np.isfinite(o[k]).all(), k


@pytest.mark.parametrize("name", ["mix", "ragged", "elp_only"])
def test_lane_elp_fp64_vs_oracle(gpu_lib, coracle, name):
    """Full fp64 solves against the oracle with test_lane_program_vs_oracle's fp64 bars (the oracle alone converges
    on 0.90-0.92 of these batches); on the mix batch the oracle reports 94 status-2 instances, so the hand-off to the
    fp64 wave program's restoration-capable queue must have run."""
    bt, ncm, nem = _batch(name)
    s = _lane(gpu_lib, ncm, nem)
    o = _solve(s, bt)
    hand = s.lane_handoffs()
    ref = _ref(coracle, name)
    both = (o["status"] == 0) & (ref["status"] == 0)
    print("fp64", name, "both", both.mean(), "status eq", (o["status"] == ref["status"]).mean(), "handoffs", hand)
    _common(o)
    _compare(o, ref, min_conv=0.8, min_agree=0.99, min_status=0.99)
    if name == "mix":
        assert hand > 0


def test_lane_elp_fp32_vs_oracle(gpu_lib, coracle):
    """The fp32 form build on the mix batch with test_lane_program_vs_oracle's fp32 bars: both converged >= 0.75,
    footholds within 1e-3 on >= 98 % of those, status-2 verdicts equal on >= 97 %."""
    bt, ncm, nem = _batch("mix")
    s = _lane(gpu_lib, ncm, nem, prec=1)
    o = _solve(s, bt)
    hand = s.lane_handoffs()
    ref = _ref(coracle, "mix")
    both = (o["status"] == 0) & (ref["status"] == 0)
    err = np.abs(o["foot"] - ref["foot"]).max(axis=1)
    print("fp32 mix both", both.mean(), "foot", np.mean(err[both] <= 1e-3), "status2",
          ((o["status"] == 2) == (ref["status"] == 2)).mean(), "handoffs", hand)
    _common(o)
    assert both.mean() >= 0.75, both.mean()
    assert np.mean(err[both] <= 1e-3) >= 0.98, np.mean(err[both] <= 1e-3)
    assert ((o["status"] == 2) == (ref["status"] == 2)).mean() >= 0.97
    assert hand > 0


@pytest.mark.parametrize("prec", [0, 1])
def test_lane_elp_batch_independence(gpu_lib, prec):
    """An instance's result does not depend on the batch, across refills and form kinds: lanes meet mix, circle-only,
    ellipse-only and empty instances in turn (a slot that held an ellipse holds a circle or nothing next).  One batch
    above the resident lane slots equals the same instances in chunks of half the slots and as short prefixes, bit for
    bit; NaN / -99 filled device outputs are all written and a second launch reproduces the first.  The scenes are the
    counter stream of scenes.make_batch_counter(seed=7310, n_cir=3, n_elp=2), taken from the device generator, which
    tests/test_scenes_gpu.py holds to that stream (the host loop takes ~20 s at this size)."""
    import torch
    s = _lane(gpu_lib, 3, 2, prec)
    slots = s.solve_slots()
    assert slots >= 16384 and slots % 32 == 0, slots
    B = slots + slots // 2 + 37
    bt = s.scenes(B, seed=7310, n_cir=3, n_elp=2)
    idx = np.arange(B)
    bt["ne"] = np.where(idx % 2 == 1, 0, bt["ne"]).astype(np.int32)
    bt["nc"] = np.where(idx % 3 == 0, 0, bt["nc"]).astype(np.int32)
    kinds = {(bool(c), bool(e)) for c, e in zip(bt["nc"][:64], bt["ne"][:64])}
    assert len(kinds) == 4, kinds
    big = _solve(s, bt)
    for k in ("u", "foot", "x_pred"):
        assert np.isfinite(big[k]).all(), k
    ch = slots // 2
    parts = [_solve(s, {k: v[i:i + ch] for k, v in bt.items()}) for i in range(0, B, ch)]
    for k in big:
        assert np.array_equal(big[k], np.concatenate([p[k] for p in parts])), k
    for nb in (1, 33, 65):
        o = _solve(s, {k: v[:nb] for k, v in bt.items()})
        for k in big:
            assert np.array_equal(o[k], big[k][:nb]), (k, nb)
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items()}
    inp["leg"] = inp["leg"].to(torch.int8)
    inp["nc"] = inp["nc"].to(torch.int32)
    inp["ne"] = inp["ne"].to(torch.int32)
    for _ in range(2):
        out = {"u": torch.full((B, 15), float("nan"), dtype=torch.float64, device=dev),
               "foot": torch.full((B, 3), float("nan"), dtype=torch.float64, device=dev),
               "x_pred": torch.full((B, 3, 5), float("nan"), dtype=torch.float64, device=dev),
               "status": torch.full((B,), -99, dtype=torch.int32, device=dev),
               "iters": torch.full((B,), -99, dtype=torch.int32, device=dev)}
        s.solve_device(inp, out)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in got:
            assert np.array_equal(got[k], big[k]), k


def test_lane_elp_rollout_vs_oracle(gpu_lib, coracle):
    """Closed-loop rollouts of the form build (retired instances skipped through the lane work queue's active mask)
    against the oracle's closed loop, with test_lane_program_rollout_vs_oracle's bars."""
    from alipmpc import scenes
    N, B, S = 3, 256, 4
    bt = scenes.make_batch(B, seed=7320, n_cir=3, n_elp=2)
    s = _lane(gpu_lib, 3, 2)
    o = s.rollout(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt["elp"], bt["ne"], u0=bt["u0"], steps=S)
    ref = coracle.rollout_batch(coracle.default_cfg(0, N, nc_max=3, ne_max=2), bt["x0"], bt["goal"], bt["leg"],
                                bt["cir"], bt["nc"], bt["elp"], bt["ne"], bt["u0"], None, steps=S, nthreads=8)
    same_status = (o["status"] == ref["status"]).all(1)
    fo, fr = np.nan_to_num(o["foot"], nan=1e9), np.nan_to_num(ref["foot"], nan=1e9)
    same_path = (np.abs(fo - fr) <= 1e-4 * np.maximum(1.0, np.abs(fr))).all((1, 2))
    print("rollout", (same_status & same_path).mean(), (o["steps_to_goal"] == ref["steps_to_goal"]).mean())
    assert (same_status & same_path).mean() >= 0.85
    assert (o["steps_to_goal"] == ref["steps_to_goal"]).mean() >= 0.9
    for b in np.nonzero(o["steps_to_goal"] > 0)[0]:
        assert (o["status"][b, o["steps_to_goal"][b]:] == gpu_lib.ROLLOUT_DONE).all()


def test_lane_elp_form_symmetry(gpu_lib):
    """Independent of the oracle: the ellipses (a, b, phi) and (b, a, phi + pi / 2) are the same sets and the same
    qa, qb, qc, k up to rounding, so the solves agree (statuses equal, u within 1e-8 where status is 0)."""
    from alipmpc import scenes
    bt = scenes.make_batch(64, seed=7330, n_cir=3, n_elp=2)
    sw = dict(bt)
    sw["elp"] = bt["elp"][:, :, [0, 1, 3, 2, 4]].copy()
    sw["elp"][:, :, 4] += np.pi / 2
    s = _lane(gpu_lib, 3, 2, select_obs=0)
    a, b = _solve(s, bt), _solve(s, sw)
    assert np.array_equal(a["status"], b["status"])
    conv = a["status"] == 0
    assert conv.any()
    err = np.abs(a["u"] - b["u"])[conv].max()
    print("symmetry max |du|", err, "converged", conv.sum())
    assert err <= 1e-8, err
