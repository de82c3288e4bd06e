"""First-order ticks of the scheduled closed loop on the device (cfg.cl_between = 1, include/alipmpc.h): between the
solves of a step the last solve's plan follows the plant through the solve's own sensitivities.  A mode-0 and a mode-1
handle of otherwise the same cfg, on test_schedule_gpu.py's episodes (B = 70, N = 3, 5 circles, 16 episodes near the
goal; with the C oracle as the solver the scene seed gives, at tick 3 of step 0 under mask {3} / f_cyc 8 / kick 0.02,
61 status-0, 7 status-2 and 2 status -1 instances, and at tick 0 under mask {0} / kick 0.05 a status-0 share of
0.84)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action", "plan")
DONE, NOMINAL, FIRST_ORDER = -10, -20, -21
B0 = 70
SEED = 1655
_cache = {}


def _solver(gpu_lib, mode, **kw):
    key = ("solver", mode, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0, cl_between=mode, **kw))
    return _cache[key]


def _episodes(gpu_lib, B=B0):
    if ("ep", B) not in _cache:
        from alipmpc import scenes
        bt = scenes.make_batch(B, seed=SEED, n_cir=5)
        x0 = bt["x0"].copy()
        x0[:16, 0:2] = bt["goal"][:16] - np.array([0.2, 0.15])
        leg = bt["leg"].astype(np.int8)
        foot0 = _solver(gpu_lib, 0).solve(x0, bt["goal"], leg, bt["cir"], bt["nc"],
                                          u0=np.tile(x0, (1, 3)))["foot"][:, 0:2].copy()
        _cache[("ep", B)] = dict(x0=x0, foot0=foot0, goal=bt["goal"], leg=leg, cir=bt["cir"], nc=bt["nc"])
    return _cache[("ep", B)]


def _sched(s, e, **kw):
    return s.closed_loop_schedule(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], want_plans=True, **kw)


def _same(a, b, keys=KEYS, tag=""):
    """Bit for bit, NaN positions included (hd on the steps entered: the loop never writes the others)."""
    ran = a["status"][:, :, 0] != DONE
    for k in keys:
        if k == "hd":
            assert np.array_equal(a[k][ran], b[k][ran]), (tag, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _close(a, b, tol, tag):
    assert np.array_equal(np.isnan(a), np.isnan(b)), tag
    err = np.nanmax(np.abs(a - b)) if np.isfinite(a).any() else 0.0
    print(tag, err, "bar", tol)
    assert err <= tol, (tag, err, tol)


def _replayed(gpu_lib, mask, S, F, kick):
    """A mode-1 loop, its replay with Solver.solve_sens on the same handle as `sens`, and what solve_sens returned at
    every replayed solve tick (rows in the order of the replay's anchors)."""
    key = ("replay", tuple(mask), S, F, kick)
    if key not in _cache:
        from alipmpc import schedule
        s1, e = _solver(gpu_lib, 1), _episodes(gpu_lib)
        o = _sched(s1, e, steps=S, f_cyc=F, mpc_ticks=mask, kick=kick, seed=5)
        calls = []

        def sens(xn, od, u0, idx):
            r = s1.solve_sens(xn, e["goal"][idx], od, e["cir"][idx], e["nc"][idx], u0=u0)
            calls.append(r)
            return r["du"], r["sens_ok"]
        rp = schedule.replay(s1.cfg, e, mask, o["x"], o["plan"], o["status"], kick=kick, seed=5, sens=sens,
                             foot_traj=o["foot"], hd_traj=o["hd"])
        again = {k: np.concatenate([c[k] for c in calls]) for k in ("u", "status", "sens_ok")}
        an = rp["anchors"]
        M = float(np.abs(an["du"][an["sens_ok"]][:, :, 0:5]).max())
        print("anchors", len(an["b"]), "valid", int(an["sens_ok"].sum()), "first-order ticks", len(rp["fo"]["b"]),
              "M = max|du[:, :, 0:5]| over the valid anchors", M)
        _cache[key] = (o, rp, again, M)
    return _cache[key]


def test_nothing_changes_where_nothing_should(gpu_lib):
    """All-ones mask and mask 0: the mode-1 handle gives the mode-0 handle's bits on every output.  Mask {2}: up to and
    including the solve — the in-loop sensitivity launch with its active mask, queue and groups — the rows are mode
    0's."""
    s0, s1, e = _solver(gpu_lib, 0), _solver(gpu_lib, 1), _episodes(gpu_lib)
    for mask in ((1 << 6) - 1, 0):
        kw = dict(steps=2, f_cyc=6, mpc_ticks=mask, kick=0.02, seed=5)
        _same(_sched(s1, e, **kw), _sched(s0, e, **kw), tag=mask)
    kw = dict(steps=1, f_cyc=6, mpc_ticks=(2,), kick=0.02, seed=5)
    a, b = _sched(s1, e, **kw), _sched(s0, e, **kw)
    for k in ("status", "iters", "plan", "action"):
        assert np.array_equal(a[k][:, :, 0:3], b[k][:, :, 0:3], equal_nan=True), k
    assert (a["status"][:, 0, 3:6] == FIRST_ORDER).any() and (b["status"][:, 0, 3:6] == NOMINAL).all()


def test_first_order_ticks_follow_the_anchors(gpu_lib):
    """Mask {3}, 3 steps of 8 ticks, kick 0.02, replayed with Solver.solve_sens on the same handle: a tick after the
    solve is first-order (-21) exactly where its anchor's sens_ok is 1 and nominal (-20) where it is 0, ticks 0-2 are
    nominal, both kinds of anchor occur, and an anchor solve that ended with status 2 or -1 is never valid."""
    o, rp, again, M = _replayed(gpu_lib, (3,), 3, 8, 0.02)
    an, fo, st = rp["anchors"], rp["fo"], o["status"]
    assert np.array_equal(again["sens_ok"] != 0, an["sens_ok"])
    ran = st[:, :, 0] != DONE
    assert ran[:, 0].all() and len(an["b"]) == ran.sum()
    assert (st[ran][:, 0:3] == NOMINAL).all() and (st[~ran] == DONE).all()
    ok = np.zeros(ran.shape, bool)
    ok[an["b"], an["s"]] = an["sens_ok"]
    assert (ok & ran).any() and (~ok & ran).any(), "anchors of both kinds"
    assert (st[ok & ran][:, 4:8] == FIRST_ORDER).all() and (st[~ok & ran][:, 4:8] == NOMINAL).all()
    assert (o["iters"][ran][:, 4:8] == 0).all() and (o["iters"][ran][:, 3] > 0).all()
    bad_status = ~np.isin(st[an["b"], an["s"], 3], (0, 1))
    assert bad_status.any() and not an["sens_ok"][bad_status].any()
    assert np.isfinite(o["plan"][st == FIRST_ORDER]).all() and np.isnan(o["plan"][st == NOMINAL]).all()
    assert len(fo["b"]) == (st == FIRST_ORDER).sum() and (fo["anchor_i"] == 3).all()


def test_solve_sens_at_the_replayed_inputs_gives_the_recorded_plans(gpu_lib):
    """The same run: solve_sens's u at the replayed solve inputs equals the recorded plan rows bit for bit, and its
    status the recorded status.  That needs the device's own bits as inputs: schedule.replay gets foot_traj and hd_traj
    too and rounds the plant moves and the projection as the device kernels do (schedule.flow_device); with numpy's
    roundings no row was bit-equal (median |u - plan| 4.2e-14, max 2.1e-5: the interior point amplifies the last bit)."""
    o, rp, again, M = _replayed(gpu_lib, (3,), 3, 8, 0.02)
    an = rp["anchors"]
    plan, st = o["plan"][an["b"], an["s"], 3], o["status"][an["b"], an["s"], 3]
    du = np.abs(again["u"] - plan).max(-1)
    print("solve ticks", len(du), "bit-equal plans", int((du == 0).sum()), "by step",
          [int((du[an["s"] == s] == 0).sum()) for s in range(3)], "of", [int((an["s"] == s).sum()) for s in range(3)],
          "max |u - plan|", du.max(), "median", np.median(du), "status differs on", int((again["status"] != st).sum()))
    assert np.array_equal(again["status"], st)
    assert np.array_equal(again["u"], plan)


def test_replay_within_the_rounding_budget(gpu_lib):
    """The same run: the recomputed first-order plans, foot, x, action and hd are within 1e-9 max(1, M) of the device's
    (the replay bar of the nominal loop, 1e-9, plus about 6 roundings of size |du| |d| <= M |d| per update).  Measured
    with the bit-exact solve inputs, M = 51.3: plans 2.8e-14, foot 1.9e-14, x 1.1e-14, action 1.6e-14, hd 0."""
    o, rp, again, M = _replayed(gpu_lib, (3,), 3, 8, 0.02)
    fo, ran = rp["fo"], o["status"][:, :, 0] != DONE
    tol = 1e-9 * max(1.0, M)
    e = np.abs(o["plan"][fo["b"], fo["s"], fo["i"]] - rp["plan"][fo["b"], fo["s"], fo["i"]]).max(-1)
    print("first-order plan rows", len(e), "median error", np.median(e), "p90", np.quantile(e, 0.9), "max", e.max(),
          "share within the bar", (e <= tol).mean(), "bar", tol)
    for k in ("foot", "x", "action"):
        print(k, "max error", np.nanmax(np.abs(o[k] - rp[k])))
    print("hd max error", np.abs(o["hd"][ran] - rp["hd"][ran]).max())
    _close(o["plan"][fo["b"], fo["s"], fo["i"]], rp["plan"][fo["b"], fo["s"], fo["i"]], tol, "first-order plans")
    _close(o["foot"], rp["foot"], tol, "foot")
    _close(o["x"], rp["x"], tol, "x")
    _close(o["action"], rp["action"], tol, "action")
    _close(o["hd"][ran], rp["hd"][ran], tol, "hd")


def test_kick_zero_keeps_the_anchor_plan(gpu_lib):
    """On the ideal plant x_nex does not move between the ticks of a step beyond rounding (some 100 roundings of
    2^-53 x magnitude 20 x e^(beta T) ~ 3.5, about 1e-12: bar 1e-11), so every first-order plan row is its anchor's
    within 1e-10 max(1, M)."""
    o, rp, again, M = _replayed(gpu_lib, (3,), 2, 8, 0.0)
    fo, sv = rp["fo"], rp["solves"]
    assert len(fo["b"]) >= 100
    xa = np.full(o["x"].shape[:2] + (5,), np.nan)
    xa[sv["b"], sv["s"]] = sv["x_nex"]
    dx = np.abs(fo["x_nex"] - xa[fo["b"], fo["s"]]).max()
    print("x_nex moves by", dx)
    assert dx <= 1e-11
    _close(o["plan"][fo["b"], fo["s"], fo["i"]], o["plan"][fo["b"], fo["s"], 3], 1e-10 * max(1.0, M), "plan vs anchor")


def test_first_order_beats_no_update(gpu_lib):
    """One solve at tick 0 of one 8-tick step, kick 0.05: at every first-order tick the plan is compared with a re-solve
    on the device at the replayed x_nex, warm-started from the anchor plan (max_iter 100).  Over the ticks where anchor
    and re-solve both end with status 0 — at least half of the first-order ticks — the median error of u_fo is below
    that of the unchanged anchor plan."""
    o, rp, again, M = _replayed(gpu_lib, (0,), 1, 8, 0.05)
    e, fo = _episodes(gpu_lib), rp["fo"]
    b, i = fo["b"], fo["i"]
    assert len(b) >= 200 and (fo["s"] == 0).all()
    ua, u_fo = o["plan"][b, 0, 0], o["plan"][b, 0, i]
    re = _solver(gpu_lib, 0, max_iter=100).solve(fo["x_nex"], e["goal"][b], (-e["leg"][b]).astype(np.int8), e["cir"][b],
                                                 e["nc"][b], u0=ua)
    keep = (o["status"][b, 0, 0] == 0) & (re["status"] == 0)
    print("first-order ticks", len(b), "kept", int(keep.sum()), "anchor status-0 share at tick 0",
          (o["status"][:, 0, 0] == 0).mean())
    assert keep.sum() >= 0.5 * len(b)
    e1 = np.abs(u_fo - re["u"]).max(-1)[keep]
    e0 = np.abs(ua - re["u"]).max(-1)[keep]
    print("median e1", np.median(e1), "median e0", np.median(e0), "ratio", np.median(e1) / np.median(e0))
    assert np.median(e1) < np.median(e0)


@pytest.mark.parametrize("mask,F", [(1 << 3, 8), (0b00101, 5), (1, 4)])
def test_fused_runs_change_no_bit(gpu_lib, monkeypatch, mask, F):
    """A maximal run of non-solve ticks in one launch against one launch per tick (ALIPMPC_CL_FUSE=0)."""
    s1, e = _solver(gpu_lib, 1), _episodes(gpu_lib)
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("ALIPMPC_CL_FUSE", fuse)
        outs[fuse] = _sched(s1, e, steps=3, f_cyc=F, mpc_ticks=mask, kick=0.02, seed=5)
    _same(outs["0"], outs["1"], tag=(mask, F))
    assert (outs["1"]["status"] == FIRST_ORDER).any()


def test_episode_groups_change_no_bit(gpu_lib, monkeypatch):
    """B = 600 in one and in two episode groups (ALIPMPC_CL_GROUPS): nominal ticks before the solve, first-order
    after."""
    s1, e = _solver(gpu_lib, 1), _episodes(gpu_lib, 600)
    outs = {}
    for g in ("1", "2"):
        monkeypatch.setenv("ALIPMPC_CL_GROUPS", g)
        outs[g] = _sched(s1, e, steps=2, f_cyc=4, mpc_ticks=(1,), kick=0.02, seed=5)
    _same(outs["1"], outs["2"])
    st = outs["1"]["status"]
    assert (st[:, 0, 0] == NOMINAL).all() and (st[:, 0, 2:4] == FIRST_ORDER).any()
    assert (st[300:, 0, 2:4] == FIRST_ORDER).any() and (st[:300, 0, 2:4] == FIRST_ORDER).any()


def test_pointer_modes(gpu_lib):
    """Device pointers on a torch stream give the host-pointer bits."""
    import torch
    s1, e = _solver(gpu_lib, 1), _episodes(gpu_lib)
    S, F = 3, 8
    host = _sched(s1, e, steps=S, f_cyc=F, mpc_ticks=(3,), kick=0.02, seed=5)
    dev = torch.device("cuda")
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in e.items()}
    inp["nc"] = inp["nc"].to(torch.int32)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        out = dict(foot=z((B0, S, 3)), x=z((B0, S + 1, 5)), hd=z((B0, S, 2)), status=z((B0, S, F), torch.int32),
                   iters=z((B0, S, F), torch.int32), steps_to_goal=z(B0, torch.int32), action=z((B0, S, F, 8)),
                   plan=z((B0, S, F, 15)))
        s1.closed_loop_schedule_device(inp, out, S, f_cyc=F, mpc_ticks=(3,), kick=0.02, seed=5, stream=st)
    st.synchronize()
    _same({k: v.cpu().numpy() for k, v in out.items()}, host, tag="device pointers")
    assert (host["status"] == FIRST_ORDER).any()


def test_refusals_and_the_other_entry_points(gpu_lib):
    """cl_between = 1 outside solve_sens's domain: EUNSUPPORTED at create; another value: EINVAL.  Every other entry
    point of a mode-1 handle is the mode-0 handle's."""
    L = gpu_lib
    for variant, N, kw in ((0, 3, dict(precision=L.PREC_FP32)), (0, 3, dict(program=L.PROGRAM_LANE)),
                           (L.VARIANT_DD, 3, {}), (0, 6, dict(nc_max=3))):
        kw = dict(dict(nc_max=5, ne_max=0), **kw)
        L.Solver(L.default_cfg(variant, N, **kw)).close()                    # the cfg itself is fine
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            L.Solver(L.default_cfg(variant, N, cl_between=1, **kw))
    for bad in (2, -1):
        with pytest.raises(RuntimeError, match="EINVAL"):
            L.Solver(L.default_cfg(0, 3, nc_max=5, ne_max=0, cl_between=bad))
    s0, s1, e = _solver(gpu_lib, 0), _solver(gpu_lib, 1), _episodes(gpu_lib)
    sc = (e["x0"], e["goal"], e["leg"], e["cir"], e["nc"])
    u0 = np.tile(e["x0"], (1, 3))
    for name, a, b in (("solve", s1.solve(*sc, u0=u0), s0.solve(*sc, u0=u0)),
                       ("solve_sens", s1.solve_sens(*sc, u0=u0), s0.solve_sens(*sc, u0=u0))):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
    cl = [s.closed_loop(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], steps=2, f_cyc=4, kick=0.02,
                        seed=5) for s in (s1, s0)]
    _same(cl[0], cl[1], KEYS[:-1], "closed_loop")
