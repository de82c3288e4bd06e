"""alipmpc_closed_loop_dataset_batch on the device: the imitation-learning rows (X, y_mpc, y_act, row_status,
row_start) against the same call's loop outputs, against the existing call, across shards / pointer modes / episode
groups, on the other programs and shapes, and at the capacity and argument edges.

Base case (B = 48, S = 4, f_cyc = 8, modi, 5 circles, scenes.make_batch(48, seed=900), the first 12 starts moved to
goal - (0.6, 0.5), foot0 from a solve at x0).  The C oracle's loop on exactly these episodes: kick 0 — 4 episodes stop
before S, 1504 rows of 1536; kick 0.05 — 5 stop, 1488 rows; sig_step (offset (1.0, 0.8), seed 901) — 14 stop."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B0, S0, F0 = 48, 4, 8
TOL, TOL_CHAIN = 1e-12, 1e-9    # the project's bars for heading inputs and controller commands
# fp32's bar for the v_des chain: 4 x the maximal residual of the same identity (velocity of the flow of x0 about foot
# over T against x_pred[:, 0, 2:4]) on the converged instances of the existing fp32 lane Solver.solve over 4096
# make_batch_vec scenes — recorded in profiles/r9/dataset/fp32_identity.json by tools/ds_fp32_identity.py and read
# from there (_fp32_chain_tol)
FP32_IDENTITY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r9", "dataset",
                             "fp32_identity.json")
ROW_KEYS = ("X", "y_mpc", "y_act", "row_status", "row_start")
LOOP_KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")


def _episodes(gpu_lib, variant=0, seed=900, B=B0, near=12, program=0, prec=0, nc_max=5, ne_max=0):
    from alipmpc import scenes
    if ne_max:   # a mix field of 2 circles + 1 ellipse in 3 + 2 slots: the slots past the counts hold junk on purpose
        bt = scenes.make_batch(B, seed=seed, n_cir=2, n_elp=1, nc_max=nc_max, ne_max=ne_max)
        bt["cir"][:, 2:] = 7.0
        bt["elp"][:, 1:] = 7.0
    else:
        bt = scenes.make_batch(B, seed=seed, n_cir=nc_max)
    x0 = bt["x0"].copy()
    x0[:near, 0:2] = bt["goal"][:near] - (np.array([1.0, 0.8]) if variant == 1 else np.array([0.6, 0.5]))
    leg = bt["leg"].astype(np.int8)
    kw = dict(nc_max=nc_max, ne_max=ne_max, program=program)
    if prec:
        kw["precision"] = gpu_lib.PREC_FP32
    cfg = gpu_lib.default_cfg(variant, 3, **kw)
    foot0 = gpu_lib.Solver(cfg).solve(x0, bt["goal"], leg, bt["cir"], bt["nc"], bt["elp"], bt["ne"],
                                      u0=np.tile(x0, (1, 3)))["foot"][:, 0:2].copy()
    return dict(cfg=cfg, x0=x0, foot0=foot0, goal=bt["goal"], leg=leg, cir=bt["cir"], nc=bt["nc"], elp=bt["elp"],
                ne=bt["ne"])


def _run(gpu_lib, e, S=S0, F=F0, sl=slice(None), **kw):
    a = [e[k][sl] for k in ("x0", "foot0", "goal", "leg", "cir", "nc")]
    el = {} if e["elp"] is None else dict(elp=e["elp"][sl], ne=e["ne"][sl])
    return gpu_lib.Solver(e["cfg"]).closed_loop_dataset(*a, steps=S, f_cyc=F, **el, **kw)


_cache = {}


def _base(gpu_lib, kick):
    """The base case and its dataset run, computed once per kick and left unchanged."""
    if kick not in _cache:
        e = _episodes(gpu_lib)
        _cache[kick] = (e, _run(gpu_lib, e, kick=kick, seed=7))
    return _cache[kick]


def _check_consistency(gpu_lib, e, o, S, F, safe_dis=0.4, tol_chain=TOL_CHAIN):
    """Case 1: the rows against the same call's loop outputs (exact unless stated) and check_rows."""
    from alipmpc import dataset
    cfg = e["cfg"]
    B = len(e["x0"])
    n3, n5 = 3 * cfg.nc_max, 5 * cfg.ne_max
    c0 = n3 + n5
    X, ym, ya, rs = o["X"], o["y_mpc"], o["y_act"], o["row_start"]
    assert X.shape[1] == c0 + 11 and rs.shape == (B + 1,) and rs.dtype == np.int64 and rs[0] == 0
    ran = o["status"] != gpu_lib.ROLLOUT_DONE
    assert (ran.all(-1) == ran.any(-1)).all()
    nst = ran[:, :, 0].sum(1)
    stg = o["steps_to_goal"]
    assert ((stg > 0) & (stg < S)).sum() >= 2, "compaction is not exercised"
    assert (nst == np.where(stg < 0, S, stg)).all()
    assert np.array_equal(np.diff(rs), F * nst)
    R = int(rs[B])
    assert len(X) == len(ym) == len(ya) == len(o["row_status"]) == R < B * S * F
    assert np.array_equal(o["row_status"], o["status"][ran])
    T = cfg.dt
    cir = e["cir"].copy()
    cir[:, :, 2] -= safe_dis
    cir[np.arange(cfg.nc_max)[None, :] >= e["nc"][:, None]] = 0.0
    if cfg.ne_max:
        elp = e["elp"].copy()
        elp[:, :, 2:4] -= safe_dis
        elp[np.arange(cfg.ne_max)[None, :] >= e["ne"][:, None]] = 0.0
    for b in range(B):
        for s in range(nst[b]):
            r = rs[b] + s * F
            blk = slice(r, r + F)
            assert np.array_equal(X[r, c0:c0 + 5], o["x"][b, s])
            stf = e["foot0"][b] if s == 0 else o["foot"][b, s - 1, 0:2]
            assert np.array_equal(X[blk, c0 + 5:c0 + 7], np.tile(stf, (F, 1)))
            assert np.array_equal(X[blk, c0 + 7:c0 + 9], np.tile(e["goal"][b], (F, 1)))
            assert np.array_equal(X[blk, c0 + 9], np.full(F, float(e["leg"][b]) * (-1) ** s))
            assert np.array_equal(X[blk, c0 + 10], T - np.arange(F) * (T / F))
            assert np.array_equal(X[blk, :n3], np.tile(cir[b].ravel(), (F, 1)))
            if cfg.ne_max:
                assert np.array_equal(X[blk, n3:c0], np.tile(elp[b].ravel(), (F, 1)))
            assert np.array_equal(ym[r + F - 1, 0:2], o["foot"][b, s, 0:2])
            assert np.abs(ym[blk, 3] - (o["hd"][b, s].sum() - e["x0"][b, 4])).max() <= TOL
            td = np.concatenate([o["foot"][b, s, 0:2], [0.0, o["x"][b, s + 1, 4]], o["x"][b, s + 1, 0:4]])
            assert np.array_equal(ya[blk], np.tile(td, (F, 1)))
            # the planned foothold and x_nex recovered from the controller command: rotated back through the row's
            # heading, plus the stance foot
            a = o["action"][b, s]
            c, sn = np.cos(X[blk, c0 + 4]), np.sin(X[blk, c0 + 4])
            for j, k in ((0, 0), (4, 4)):
                rec = np.stack([stf[0] + c * a[:, j] - sn * a[:, j + 1], stf[1] + sn * a[:, j] + c * a[:, j + 1]], 1)
                assert np.abs(ym[blk, k:k + 2] - rec).max() <= TOL_CHAIN
    res = dataset.check_rows(X, ym, ya, rs, F, cfg.nc_max, cfg.ne_max, cfg, tol=TOL, tol_chain=tol_chain, tol_stance=0.0)
    print("check_rows", res)
    return res


@pytest.mark.parametrize("kick", [0.0, 0.05])
def test_rows_consistent_with_loop_outputs(gpu_lib, kick):
    e, o = _base(gpu_lib, kick)
    print("rows", int(o["row_start"][-1]), "stopped early", int(((o["steps_to_goal"] > 0) & (o["steps_to_goal"] < S0)).sum()))
    _check_consistency(gpu_lib, e, o, S0, F0)


@pytest.mark.parametrize("kick", [0.0, 0.05])
def test_loop_outputs_equal_existing_call(gpu_lib, kick):
    e, o = _base(gpu_lib, kick)
    ref = gpu_lib.Solver(e["cfg"]).closed_loop(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], steps=S0,
                                               f_cyc=F0, kick=kick, seed=7)
    assert set(ref) == set(LOOP_KEYS)
    for k in LOOP_KEYS:
        assert np.array_equal(o[k], ref[k], equal_nan=True), k


def _assert_loop_equal(a, b, tag):
    """The loop outputs of two runs; hd only over the steps that ran (the loop leaves hd_traj unwritten after an
    episode's stop, as the existing call does)."""
    for k in LOOP_KEYS:
        x, y = a[k], b[k]
        if k == "hd":
            m = (a["status"][:, :, 0] != -10)[:, :, None]
            x, y = np.where(m, x, 0.0), np.where(m, y, 0.0)
        assert np.array_equal(x, y, equal_nan=True), (tag, k)


def _rows_of(o, lo, hi):
    r0, r1 = int(o["row_start"][lo]), int(o["row_start"][hi])
    return {k: o[k][r0:r1] for k in ROW_KEYS[:4]}, o["row_start"][lo:hi + 1] - r0


def test_shards_give_the_rows_of_the_whole(gpu_lib):
    e, whole = _base(gpu_lib, 0.05)
    for lo, hi in ((0, 24), (24, 48)):
        part = _run(gpu_lib, e, sl=slice(lo, hi), kick=0.05, seed=7, first=lo)
        want, want_rs = _rows_of(whole, lo, hi)
        assert np.array_equal(part["row_start"], want_rs)
        for k in want:
            assert np.array_equal(part[k], want[k]), (lo, k)
        _assert_loop_equal(part, {k: whole[k][lo:hi] for k in LOOP_KEYS}, lo)
    # the second shard with the wrong first index takes other kicks: first is what makes the shard the whole's
    other = _run(gpu_lib, e, sl=slice(24, 48), kick=0.05, seed=7, first=0)
    assert not np.array_equal(other["x"], whole["x"][24:48])


def _device_call(gpu_lib, e, S, F, keys=ROW_KEYS + LOOP_KEYS, max_rows=None, rows_alloc=None, sentinel=None, **kw):
    """The device-pointer call on torch tensors; returns numpy copies of the outputs asked for."""
    import torch
    cfg = e["cfg"]
    B = len(e["x0"])
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(e[k])).to(dev)
           for k in ("x0", "foot0", "goal", "leg", "cir", "nc", "elp", "ne") if e[k] is not None}
    n = B * S * F if rows_alloc is None else rows_alloc
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    fill = 0.0 if sentinel is None else sentinel
    shapes = dict(X=((n, 3 * cfg.nc_max + 5 * cfg.ne_max + 11), f64), y_mpc=((n, 8), f64), y_act=((n, 8), f64),
                  row_status=((n,), i32), row_start=((B + 1,), dict(dtype=torch.int64, device=dev)),
                  foot=((B, S, 3), f64), x=((B, S + 1, 5), f64), hd=((B, S, 2), f64), status=((B, S, F), i32),
                  iters=((B, S, F), i32), steps_to_goal=((B,), i32), action=((B, S, F, 8), f64))
    out = {k: torch.full(shapes[k][0], int(fill) if shapes[k][1]["dtype"] != torch.float64 else fill, **shapes[k][1])
           for k in keys}
    gpu_lib.Solver(cfg).closed_loop_dataset_device(inp, out, S, F, max_rows=n if max_rows is None else max_rows, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_device_pointers_equal_host_pointers(gpu_lib):
    e, host = _base(gpu_lib, 0.05)
    d = _device_call(gpu_lib, e, S0, F0, kick=0.05, seed=7)
    R = int(host["row_start"][-1])
    assert np.array_equal(d["row_start"], host["row_start"])
    for k in ROW_KEYS[:4]:
        assert np.array_equal(d[k][:R], host[k]), k
    _assert_loop_equal(d, host, "device")


def test_episode_groups_do_not_change_rows(gpu_lib, monkeypatch):
    e = _episodes(gpu_lib, seed=902, B=768, near=192)
    outs = {}
    for grp in ("1", "3"):
        monkeypatch.setenv("ALIPMPC_CL_GROUPS", grp)
        outs[grp] = _run(gpu_lib, e, S=1, F=F0, kick=0.05, seed=7)
    assert int(outs["1"]["row_start"][-1]) == 768 * F0
    for k in ROW_KEYS + LOOP_KEYS:
        assert np.array_equal(outs["1"][k], outs["3"][k], equal_nan=True), k


def _fp32_chain_tol():
    with open(FP32_IDENTITY) as fh:
        rec = json.load(fh)
    return 4.0 * rec["lane_fp32"]["max_residual_converged"]


@pytest.mark.parametrize("name", ["sig_step", "lane_fp64", "lane_fp32", "mix_3c_2e", "six_circles_f5"])
def test_programs_and_shapes(gpu_lib, name):
    """six_circles_f5: the reference's 29 columns with an odd f_cyc, so that episodes' blocks of X start at odd
    element offsets (8- but not 16-byte aligned) and have odd lengths — the compaction's peeled first and last
    element; every other case has whole 16-byte blocks."""
    kw = dict(sig_step=dict(variant=1, seed=901), lane_fp64=dict(program=1), lane_fp32=dict(program=1, prec=1),
              mix_3c_2e=dict(nc_max=3, ne_max=2, seed=903), six_circles_f5=dict(nc_max=6))[name]
    S, F = (3, 5) if name == "six_circles_f5" else (S0, F0)   # (3 x 5 rows: an odd count for whoever does not stop)
    e = _episodes(gpu_lib, **kw)
    assert e["cfg"].program == kw.get("program", 0) and e["cfg"].variant == kw.get("variant", 0)
    o = _run(gpu_lib, e, S=S, F=F, kick=0.05, seed=7)
    tol_chain = TOL_CHAIN
    if name == "lane_fp32":
        tol_chain = _fp32_chain_tol()
        assert 1e-9 < tol_chain < 1e-2
    res = _check_consistency(gpu_lib, e, o, S, F, tol_chain=tol_chain)
    if name == "six_circles_f5":
        assert o["X"].shape[1] == 29 and (np.diff(o["row_start"]) % 2 == 1).any()
    if name == "mix_3c_2e":   # the layout: 3 circle slots (2 used), 2 ellipse slots (1 used), 11 -> 30 columns
        assert o["X"].shape[1] == 30 and (o["X"][:, 6:9] == 0).all() and (o["X"][:, 14:19] == 0).all()
        assert (o["X"][:, 0:6] != 0).any() and (o["X"][:, 9:14] != 0).any()
    assert res["v_des"] <= tol_chain


def test_safe_dis_zero_keeps_inflated_radii(gpu_lib):
    e, o = _base(gpu_lib, 0.0)
    z = _run(gpu_lib, e, kick=0.0, seed=7, safe_dis=0.0)
    assert np.array_equal(z["X"][:, 15:], o["X"][:, 15:]) and np.array_equal(z["y_mpc"], o["y_mpc"])
    b = np.repeat(np.arange(B0), np.diff(o["row_start"]))
    assert np.array_equal(z["X"][:, :15], e["cir"][b].reshape(-1, 15))


def test_capacity(gpu_lib):
    e, full = _base(gpu_lib, 0.05)
    R = int(full["row_start"][-1])
    cap = R // 2
    assert 0 < cap < R
    d = _device_call(gpu_lib, e, S0, F0, keys=ROW_KEYS, max_rows=cap, rows_alloc=R, sentinel=-77.0, kick=0.05, seed=7)
    assert np.array_equal(d["row_start"], full["row_start"])
    for k in ROW_KEYS[:4]:
        assert np.array_equal(d[k][:cap], full[k][:cap]), k
        assert (d[k][cap:] == -77).all(), k
    h = _run(gpu_lib, e, kick=0.05, seed=7, max_rows=cap)
    assert np.array_equal(h["row_start"], full["row_start"])
    for k in ROW_KEYS[:4]:
        assert len(h[k]) == cap and np.array_equal(h[k], full[k][:cap]), k
    z = _run(gpu_lib, e, kick=0.05, seed=7, max_rows=0)
    assert np.array_equal(z["row_start"], full["row_start"]) and len(z["X"]) == 0


def test_row_start_alone(gpu_lib):
    from alipmpc._lib import _ptr
    e, full = _base(gpu_lib, 0.05)
    d = _device_call(gpu_lib, e, S0, F0, keys=("row_start",), max_rows=0, kick=0.05, seed=7)
    assert np.array_equal(d["row_start"], full["row_start"])
    s = gpu_lib.Solver(e["cfg"])
    rs = np.full(B0 + 1, -1, np.int64)
    rc = s._L.alipmpc_closed_loop_dataset_batch(
        s._h, B0, S0, F0, 0.05, 7, _ptr(e["x0"]), _ptr(e["foot0"]), _ptr(e["goal"]), _ptr(e["leg"]), _ptr(e["cir"]),
        _ptr(e["nc"]), None, None, None, None, None, None, None, None, None, 0, 0.4, 0, None, None, None, None,
        _ptr(rs), None)
    assert rc == 0 and np.array_equal(rs, full["row_start"])


def test_empty_batch_and_bad_arguments(gpu_lib):
    e, _ = _base(gpu_lib, 0.0)
    o = _run(gpu_lib, e, sl=slice(0, 0))
    assert np.array_equal(o["row_start"], [0]) and o["X"].shape == (0, 26) and o["y_mpc"].shape == (0, 8)
    o = _run(gpu_lib, e, S=0)
    assert np.array_equal(o["row_start"], np.zeros(B0 + 1, np.int64)) and len(o["X"]) == 0
    for bad in (dict(first=-1), dict(first=2 ** 32 - B0 + 1), dict(max_rows=-1), dict(safe_dis=-0.1),
                dict(safe_dis=float("nan")), dict(safe_dis=float("inf"))):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _run(gpu_lib, e, **bad)
    _run(gpu_lib, e, sl=slice(0, 4), S=1, first=2 ** 32 - 4)   # the last episodes of the index space
    dd = gpu_lib.default_cfg(gpu_lib.VARIANT_DD, 3, nc_max=5, ne_max=0)
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        gpu_lib.Solver(dd).closed_loop_dataset(np.zeros((4, 3)), np.zeros((4, 2)), e["goal"][:4], e["leg"][:4],
                                               e["cir"][:4], e["nc"][:4], steps=1, f_cyc=F0)
