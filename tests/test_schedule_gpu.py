"""alipmpc_closed_loop_schedule_batch on the device: solves on scheduled ticks, the nominal ALIP foothold between
(Solver.closed_loop_schedule), against the existing loop, the numpy restatement (alipmpc/schedule.py) and the C oracle."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")
DONE, NOMINAL = -10, -20
B0 = 70          # more than one wave, no multiple of 64
_cache = {}


def _case(gpu_lib, variant=0, program=0, prec=0, ncm=5, B=B0):
    """Solver, cfg and episodes of a case, made once: sixteen episodes start within 0.3 m of the goal, so some stop."""
    key = (variant, program, prec, ncm, B)
    if key not in _cache:
        from alipmpc import scenes
        kw = dict(nc_max=ncm, ne_max=0, program=program)
        if prec:
            kw["precision"] = gpu_lib.PREC_FP32
        cfg = gpu_lib.default_cfg(variant, 3, **kw)
        s = gpu_lib.Solver(cfg)
        bt = scenes.make_batch(B, seed=1620 + variant + 3 * program + 7 * ncm, n_cir=max(ncm, 1))
        x0 = bt["x0"].copy()
        x0[:16, 0:2] = bt["goal"][:16] - np.array([0.2, 0.15])
        leg = bt["leg"].astype(np.int8)
        cir = bt["cir"] if ncm else np.zeros((B, 0, 3))
        nc = bt["nc"] if ncm else np.zeros(B, np.int32)
        foot0 = s.solve(x0, bt["goal"], leg, cir, nc, u0=np.tile(x0, (1, 3)))["foot"][:, 0:2].copy()
        _cache[key] = (s, cfg, dict(x0=x0, foot0=foot0, goal=bt["goal"], leg=leg, cir=cir, nc=nc))
    return _cache[key]


def _sched(s, e, **kw):
    return s.closed_loop_schedule(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], **kw)


def _same(a, b, keys, tag=""):
    """Bit for bit, NaN positions included.  (hd of a step an episode never entered is never written, by the existing
    loop either: those rows keep what the buffer held, so they are compared on the steps entered.)"""
    ran = a["status"][:, :, 0] != DONE
    for k in keys:
        if k == "hd":
            assert np.array_equal(a[k][ran], b[k][ran]), (tag, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _close(a, b, tol, tag):
    assert np.array_equal(np.isnan(a), np.isnan(b)), tag
    err = np.nanmax(np.abs(a - b)) if np.isfinite(a).any() else 0.0
    print(tag, err)
    assert err <= tol, (tag, err)


@pytest.mark.parametrize("variant,program,prec,ncm", [(0, 0, 0, 5), (1, 0, 0, 0), (0, 1, 1, 5)])
def test_all_ones_mask_is_the_existing_loop(gpu_lib, variant, program, prec, ncm):
    """Every tick solving: every output equals Solver.closed_loop's bit for bit, NaN positions included; the recorded
    plan of a step's last tick feeds Solver.trace."""
    s, cfg, e = _case(gpu_lib, variant, program, prec, ncm)
    S, F = 2, 6
    ref = s.closed_loop(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], steps=S, f_cyc=F, kick=0.02, seed=5)
    o = _sched(s, e, steps=S, f_cyc=F, mpc_ticks=(1 << F) - 1, kick=0.02, seed=5, want_plans=True)
    _same(o, ref, KEYS)
    ran = o["status"] != DONE
    assert ran.any() and np.isfinite(o["plan"][ran]).all() and np.isnan(o["plan"][~ran]).all()
    assert (o["status"] != NOMINAL).all()
    for st in range(S):
        on = ran[:, st, F - 1]
        tr = s.trace(o["x"][on, st], o["plan"][on, st, F - 1])
        assert tr.shape[0] == on.sum() and np.isfinite(tr).all()


@pytest.mark.parametrize("kick", [0.0, 0.02])
def test_mask_zero_matches_the_host_loop(gpu_lib, kick):
    """No solve: every float output within 1e-9 of schedule.run (at most 40 ticks x ~50 roundings x 2^-53 x magnitude
    20 x e^(beta T) ~ 3.5 is about 2e-11), statuses and iterations exact; on the ideal plant the touchdown velocity is
    alip_des_vel(0.6, leg_ind) from the third touchdown on (the law is deadbeat)."""
    from alipmpc import schedule
    s, cfg, e = _case(gpu_lib)
    S, F = 4, 20
    o = _sched(s, e, steps=S, f_cyc=F, mpc_ticks=0, kick=kick, seed=5, want_plans=True)
    ref = schedule.run(cfg, e, 0, steps=S, f_cyc=F, kick=kick, seed=5)
    assert (o["status"] == NOMINAL).all() and (o["iters"] == 0).all() and (o["steps_to_goal"] == -1).all()
    _same(o, ref, ("status", "iters", "steps_to_goal"))
    assert np.isnan(o["plan"]).all()
    for k in ("foot", "x", "hd", "action"):
        _close(o[k], ref[k], 1e-9, k)
    if kick == 0.0:
        kc = schedule.constants(cfg)
        for st in range(2, S + 1):
            err = np.abs(o["x"][:, st, 2:4] - schedule.des_vel(kc, e["leg"].astype(float) * (-1) ** st)).max()
            print("deadbeat", st, err)
            assert err <= 1e-9, (st, err)


def _reference_schedule(gpu_lib, variant):
    key = ("ref", variant)
    if key not in _cache:
        from alipmpc import schedule
        s, cfg, e = _case(gpu_lib, variant)
        o = _sched(s, e, steps=3, f_cyc=20, mpc_ticks=(15,), kick=0.02, seed=5, want_plans=True)
        rp = schedule.replay(cfg, e, [15], o["x"], o["plan"], o["status"], kick=0.02, seed=5)
        _cache[key] = (o, rp)
    return _cache[key]


@pytest.mark.parametrize("variant", [0, 1])
def test_reference_schedule_replays(gpu_lib, variant):
    """f_cyc = 20 with one solve at tick 15 (main_sim_mpc_alip.py): every step recomputed on the host from the device's
    own touchdown state, plans and statuses reproduces foot, hd, x and action within 1e-9; nominal ticks carry
    TICK_NOMINAL, 0 iterations and NaN plan rows, stopped episodes ROLLOUT_DONE / NaN."""
    o, rp = _reference_schedule(gpu_lib, variant)
    B, S, F = o["status"].shape
    st = o["status"]
    ran = st[:, :, 0] != DONE                       # the steps an episode entered
    assert ran[:, 0].all()
    nom = np.delete(np.arange(F), 15)
    assert (st[ran][:, nom] == NOMINAL).all() and (st[ran][:, 15] != NOMINAL).all() and (st[ran][:, 15] != DONE).all()
    assert (st[~ran] == DONE).all() and (o["iters"][~ran] == 0).all() and (o["iters"][ran][:, nom] == 0).all()
    assert (o["iters"][ran][:, 15] > 0).all()
    assert np.isnan(o["plan"][ran][:, nom]).all() and np.isfinite(o["plan"][ran][:, 15]).all()
    assert np.isnan(o["plan"][~ran]).all() and np.isnan(o["action"][~ran]).all() and np.isnan(o["foot"][~ran]).all()
    stopped = o["steps_to_goal"] > 0
    print("stopped", int(stopped.sum()), "of", B)
    assert stopped.any() and (~stopped).any()
    for b in np.nonzero(stopped)[0]:
        assert ran[b, :o["steps_to_goal"][b]].all() and not ran[b, o["steps_to_goal"][b]:].any()
    assert (o["steps_to_goal"][~stopped] == -1).all() and ran[~stopped].all()
    _close(o["foot"], rp["foot"], 1e-9, "foot")
    _close(o["action"], rp["action"], 1e-9, "action")
    _close(o["x"], rp["x"], 1e-9, "x")
    _close(o["hd"][ran], rp["hd"][ran], 1e-9, "hd")


@pytest.mark.parametrize("variant", [0, 1])
def test_solves_at_the_replayed_inputs(gpu_lib, coracle, variant):
    """The inputs schedule.replay derives for every solved tick of the reference schedule, solved again on the same
    handle, give the recorded plan (same status, u within 1e-6) on a share of the ticks no smaller than the C oracle's
    own under a relative 1e-12 perturbation of those inputs, minus 0.02; against the oracle's solves of those inputs the
    project's same-inputs bars hold."""
    o, rp = _reference_schedule(gpu_lib, variant)
    s, cfg, e = _case(gpu_lib, variant)
    sv = rp["solves"]
    b = sv["b"]
    K = len(b)
    assert K >= 150
    plan = o["plan"][b, sv["s"], sv["i"]]
    st_dev = o["status"][b, sv["s"], sv["i"]]
    r = s.solve(sv["x_nex"], e["goal"][b], sv["leg"], e["cir"][b], e["nc"][b], u0=sv["u0"])
    ok = (r["status"] == st_dev) & (np.abs(r["u"] - plan).max(-1) <= 1e-6)
    co = coracle.default_cfg(variant, 3, nc_max=cfg.nc_max, ne_max=0)
    cir = e["cir"][b] if cfg.nc_max else np.zeros((K, 0, 3))
    ro = coracle.solve_batch(co, sv["x_nex"], e["goal"][b], sv["leg"], cir, e["nc"][b], None, None, sv["u0"],
                             nthreads=8)
    rng = np.random.default_rng(5)
    px = sv["x_nex"] * (1.0 + 1e-12 * rng.uniform(-1, 1, sv["x_nex"].shape))
    pu = sv["u0"] * (1.0 + 1e-12 * rng.uniform(-1, 1, sv["u0"].shape))
    rq = coracle.solve_batch(co, px, e["goal"][b], sv["leg"], cir, e["nc"][b], None, None, pu, nthreads=8)
    oracle_share = ((ro["status"] == rq["status"]) & (np.abs(ro["u"] - rq["u"]).max(-1) <= 1e-6)).mean()
    print("solved ticks", K, "device share", ok.mean(), "oracle share under 1e-12", oracle_share)
    assert ok.mean() >= oracle_share - 0.02, (ok.mean(), oracle_share)
    same_st = r["status"] == ro["status"]
    conv = (r["status"] == 0) & (ro["status"] == 0)
    same_path = conv & (r["iters"] == ro["iters"])
    ferr = np.abs(r["foot"] - ro["foot"]).max(-1)
    print("status agree", same_st.mean(), "1e-6 same path", (ferr[same_path] <= 1e-6).mean(), "1e-3 converged",
          (ferr[conv] <= 1e-3).mean())
    assert same_st.mean() >= 0.99, same_st.mean()
    assert (ferr[same_path] <= 1e-6).mean() >= 0.995, (ferr[same_path] <= 1e-6).mean()
    assert (ferr[conv] <= 1e-3).mean() >= 0.99, (ferr[conv] <= 1e-3).mean()


@pytest.mark.parametrize("mask,F", [(1 << 15, 20), (0b00101, 5), (1 << 3, 4), (1, 4)])
def test_fused_runs_change_no_bit(gpu_lib, monkeypatch, mask, F):
    """A maximal run of nominal ticks in one launch against one launch per tick (ALIPMPC_CL_FUSE=0)."""
    s, cfg, e = _case(gpu_lib)
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("ALIPMPC_CL_FUSE", fuse)
        outs[fuse] = _sched(s, e, steps=3, f_cyc=F, mpc_ticks=mask, kick=0.02, seed=5, want_plans=True)
    monkeypatch.delenv("ALIPMPC_CL_FUSE")
    _same(outs["0"], outs["1"], KEYS + ("plan",), (mask, F))
    dflt = _sched(s, e, steps=3, f_cyc=F, mpc_ticks=mask, kick=0.02, seed=5, want_plans=True)
    _same(dflt, outs["1"], KEYS + ("plan",), "default")
    nom = [i for i in range(F) if not mask >> i & 1]
    assert (outs["1"]["status"][:, 0][:, nom] == NOMINAL).all()


def test_episode_groups_change_no_bit(gpu_lib, monkeypatch):
    """B = 600 in one and in two episode groups (ALIPMPC_CL_GROUPS), runs of nominal ticks before and after the solve."""
    s, cfg, e = _case(gpu_lib, B=600)
    outs = {}
    for g in ("1", "2"):
        monkeypatch.setenv("ALIPMPC_CL_GROUPS", g)
        outs[g] = _sched(s, e, steps=1, f_cyc=4, mpc_ticks=(1,), kick=0.02, seed=5, want_plans=True)
    _same(outs["1"], outs["2"], KEYS + ("plan",))
    assert (outs["1"]["status"][:, 0, [0, 2, 3]] == NOMINAL).all()


def test_pointer_modes(gpu_lib):
    """Device pointers on a torch stream give the host-pointer bits; plan_traj = NULL changes no other output."""
    import torch
    s, cfg, e = _case(gpu_lib)
    S, F = 3, 20
    host = _sched(s, e, steps=S, f_cyc=F, mpc_ticks=(15,), kick=0.02, seed=5, want_plans=True)
    noplan = _sched(s, e, steps=S, f_cyc=F, mpc_ticks=(15,), kick=0.02, seed=5)
    assert noplan["plan"] is None
    _same(noplan, host, KEYS, "no plan")
    dev = torch.device("cuda")
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in e.items()}
    inp["nc"] = inp["nc"].to(torch.int32)
    B = B0
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = dict(foot=torch.zeros((B, S, 3), dtype=torch.float64, device=dev),
                   x=torch.zeros((B, S + 1, 5), dtype=torch.float64, device=dev),
                   hd=torch.zeros((B, S, 2), dtype=torch.float64, device=dev),
                   status=torch.zeros((B, S, F), dtype=torch.int32, device=dev),
                   iters=torch.zeros((B, S, F), dtype=torch.int32, device=dev),
                   steps_to_goal=torch.zeros(B, dtype=torch.int32, device=dev),
                   action=torch.zeros((B, S, F, 8), dtype=torch.float64, device=dev),
                   plan=torch.zeros((B, S, F, 15), dtype=torch.float64, device=dev))
        s.closed_loop_schedule_device(inp, out, S, f_cyc=F, mpc_ticks=(15,), kick=0.02, seed=5, stream=st)
    st.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _same(got, host, KEYS + ("plan",), "device pointers")


def test_refusals(gpu_lib):
    """f_cyc above 64 and a mask bit at or above f_cyc: EINVAL; a DD handle: EUNSUPPORTED; B = 0 or S = 0: success with
    nothing written."""
    s, cfg, e = _case(gpu_lib)
    L = gpu_lib.load()
    EINVAL, EUNSUPPORTED = -1, -4
    B = 4
    sent = 12345.0

    def call(handle, Bn, S, F, mask):
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        bufs = dict(foot=np.full((B, 2, 3), sent), x=np.full((B, 3, 5), sent), hd=np.full((B, 2, 2), sent),
                    status=np.full((B, 2, 64), 777, np.int32), iters=np.full((B, 2, 64), 777, np.int32),
                    stg=np.full(B, 777, np.int32), action=np.full((B, 2, 64, 8), sent),
                    plan=np.full((B, 2, 64, 15), sent))
        x0 = np.ascontiguousarray(e["x0"][:B])
        f0 = np.ascontiguousarray(e["foot0"][:B])
        goal = np.ascontiguousarray(e["goal"][:B])
        leg = np.ascontiguousarray(e["leg"][:B])
        cir = np.ascontiguousarray(e["cir"][:B])
        nc = np.ascontiguousarray(e["nc"][:B], np.int32)
        rc = L.alipmpc_closed_loop_schedule_batch(handle, Bn, S, F, mask, 0.0, 0, P(x0), P(f0), P(goal), P(leg), P(cir),
                                                  P(nc), None, None, P(bufs["foot"]), P(bufs["x"]), P(bufs["hd"]),
                                                  P(bufs["status"]), P(bufs["iters"]), P(bufs["stg"]),
                                                  P(bufs["action"]), P(bufs["plan"]), None)
        clean = all((v == (777 if v.dtype == np.int32 else sent)).all() for v in bufs.values())
        return rc, clean

    assert call(s._h, B, 2, 65, 0) == (EINVAL, True)
    assert call(s._h, B, 2, 0, 0) == (EINVAL, True)
    assert call(s._h, B, 2, 20, 1 << 20) == (EINVAL, True)
    assert call(s._h, B, 2, 63, 1 << 63) == (EINVAL, True)
    assert call(s._h, 0, 2, 20, 1 << 15) == (0, True)
    assert call(s._h, B, 0, 20, 1 << 15) == (0, True)
    dd = gpu_lib.Solver(gpu_lib.default_cfg(gpu_lib.VARIANT_DD, 3, nc_max=5, ne_max=0))
    assert call(dd._h, B, 2, 20, 1 << 15) == (EUNSUPPORTED, True)
    with pytest.raises(RuntimeError, match="EINVAL"):
        _sched(s, e, steps=1, f_cyc=4, mpc_ticks=(4,))
    # and a valid call at the upper end of f_cyc still runs: the last tick's bit is bit 63
    o = s.closed_loop_schedule(e["x0"][:B], e["foot0"][:B], e["goal"][:B], e["leg"][:B], e["cir"][:B], e["nc"][:B],
                               steps=1, f_cyc=64, mpc_ticks=(63,))
    assert (o["status"][:, 0, :63] == NOMINAL).all() and (o["status"][:, 0, 63] != NOMINAL).all()
