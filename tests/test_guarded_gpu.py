"""Guarded first-order ticks of the scheduled closed loop on the device (cfg.cl_between = 3, include/alipmpc.h): a
first-order tick is accepted only if its plan passes the constraint rows at the tick's own x_nex (cl_guard_kernel, the
audit's violation pass); an episode whose plan fails re-solves on that tick and takes a new anchor.

test_first_order_gpu.py's episodes, restated: B = 70, N = 3, 5 circles, scene seed 1655, 16 episodes moved near the
goal, kick seed 5.  Two further shapes at B = 32: modi N = 5 with 3 circles and 2 ellipses, sig_step N = 3 with 4
circles.  The development override ALIPMPC_CL_GUARD_TOL (read per call) sets the guard's bar: inf never fires, -1
always.  The referee of every decision is Solver.audit — alipmpc_audit_batch, a kernel of its own — on the recorded
plan rows at the x_nex that schedule.replay recomputes.

Measured (profiles/guarded/guarded_tests.txt): the kick _decision chooses is 0.02 for modi N = 3 (16.6 % of run A's
guarded ticks above the bar) and modi N = 5 with ellipses (11.6 %), 0.05 for sig_step (5.9 % at 0.02, 11.7 % at 0.05);
refused plans >= 1.0016e-4, accepted ones <= 9.895e-5, none inside the band; 50 of 50 first triggered solves and 264
of 264 scheduled ones reproduce."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action", "plan")
DONE, NOMINAL, FIRST_ORDER = -10, -20, -21
BAR = 1e-4          # ALIPMPC_CL_GUARD_VIOL
BAND = 1e-6         # referee values within BAR (1 +- BAND) are left out (at most 2 per case)
SEED = 1655
CASES = {"modi3": dict(variant=0, N=3, n_cir=5, n_elp=0, B=70, seed=SEED),
         "modi5_elp": dict(variant=0, N=5, n_cir=3, n_elp=2, B=32, seed=SEED + 1),
         "sig3": dict(variant=1, N=3, n_cir=4, n_elp=0, B=32, seed=SEED + 2)}
_cache = {}


def _solver(L, case, mode, **kw):
    key = ("solver", case, mode, tuple(sorted(kw.items())))
    if key not in _cache:
        c = CASES[case]
        _cache[key] = L.Solver(L.default_cfg(c["variant"], c["N"], nc_max=c["n_cir"], ne_max=c["n_elp"], cl_between=mode,
                                             **kw))
    return _cache[key]


def _episodes(L, case, B=None):
    c = CASES[case]
    B = B or c["B"]
    if ("ep", case, B) not in _cache:
        from alipmpc import scenes
        bt = scenes.make_batch(B, seed=c["seed"], n_cir=c["n_cir"], n_elp=c["n_elp"], N=c["N"])
        x0 = bt["x0"].copy()
        x0[:16, 0:2] = bt["goal"][:16] - np.array([0.2, 0.15])
        leg = bt["leg"].astype(np.int8)
        e = dict(x0=x0, goal=bt["goal"], leg=leg, cir=bt["cir"], nc=bt["nc"],
                 elp=bt["elp"] if c["n_elp"] else None, ne=bt["ne"] if c["n_elp"] else None)
        e["foot0"] = _solver(L, case, 0).solve(*_scene(e), u0=np.tile(x0, (1, c["N"])))["foot"][:, 0:2].copy()
        _cache[("ep", case, B)] = e
    return _cache[("ep", case, B)]


def _scene(e, b=None, x0=None, leg=None):
    """(x0, goal, leg, cir, nc, elp, ne) of the episodes b (all: None), x0 / leg replaced where given."""
    cut = (lambda v: v) if b is None else (lambda v: None if v is None else v[b])
    return (cut(e["x0"]) if x0 is None else x0, cut(e["goal"]), cut(e["leg"]) if leg is None else leg, cut(e["cir"]),
            cut(e["nc"]), cut(e["elp"]), cut(e["ne"]))


def _sched(s, e, **kw):
    return s.closed_loop_schedule(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], e["elp"], e["ne"],
                                  want_plans=True, **kw)


def _tol(monkeypatch, tol):
    if tol is None:
        monkeypatch.delenv("ALIPMPC_CL_GUARD_TOL", raising=False)
    else:
        monkeypatch.setenv("ALIPMPC_CL_GUARD_TOL", tol)


def _loop(L, monkeypatch, case, mode, tol, mask, S, F, kick):
    key = ("loop", case, mode, tol, tuple(mask), S, F, kick)
    if key not in _cache:
        _tol(monkeypatch, tol)
        _cache[key] = _sched(_solver(L, case, mode), _episodes(L, case), steps=S, f_cyc=F, mpc_ticks=mask, kick=kick,
                             seed=5)
        _tol(monkeypatch, None)
    return _cache[key]


def _same(a, b, keys=KEYS, tag=""):
    """Bit for bit, NaN positions included (hd on the steps entered: the loop never writes the others)."""
    ran = a["status"][:, :, 0] != DONE
    for k in keys:
        if k == "hd":
            assert np.array_equal(a[k][ran], b[k][ran]), (tag, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _od(e, b, s):
    """od_ev = -leg_ind of episode b in step s (the stance switches at every touchdown)."""
    return (-e["leg"][b] * np.where(np.asarray(s) % 2, -1, 1)).astype(np.int8)


def _replayed(L, monkeypatch, case, tol, mask, S, F, kick):
    """A mode-3 loop under the tolerance `tol` and its bit-exact replay with Solver.solve_sens of the same handle."""
    key = ("replay", case, tol, tuple(mask), S, F, kick)
    if key not in _cache:
        from alipmpc import schedule
        s3, e = _solver(L, case, 3), _episodes(L, case)
        o = _loop(L, monkeypatch, case, 3, tol, mask, S, F, kick)

        def sens(xn, od, u0, idx):
            r = s3.solve_sens(*_scene(e, idx, xn, od), u0=u0)
            return r["du"], r["sens_ok"]
        rp = schedule.replay(s3.cfg, e, mask, o["x"], o["plan"], o["status"], kick=kick, seed=5, sens=sens,
                             foot_traj=o["foot"], hd_traj=o["hd"], guarded=True)
        _cache[key] = (o, rp)
    return _cache[key]


def _referee(L, case, x_nex, b, s, rows):
    """alipmpc_audit_batch's viol of the plan rows at x_nex for the episodes b in the steps s."""
    if len(b) == 0:
        return np.zeros(0)
    e = _episodes(L, case)
    return _solver(L, case, 3).audit(*_scene(e, b, x_nex, _od(e, b, s)), u=rows)["metrics"][:, 0]


MASKS = ((0,), (3,))
S3, F3 = 2, 8


def _decision(L, monkeypatch, case):
    """Run A (tolerance inf) of masks {0} and {3} at the smallest kick of 0.02, 0.05, 0.1 for which the referee puts
    between 10 % and 90 % of A's guarded ticks above the bar; None if no kick does."""
    key = ("decision", case)
    if key not in _cache:
        _cache[key] = None
        for kick in (0.02, 0.05, 0.1):
            v = []
            for mask in MASKS:
                o, rp = _replayed(L, monkeypatch, case, "inf", mask, S3, F3, kick)
                fo = rp["fo"]
                assert len(fo["b"]) == (o["status"] == FIRST_ORDER).sum() > 0
                v.append(_referee(L, case, fo["x_nex"], fo["b"], fo["s"], o["plan"][fo["b"], fo["s"], fo["i"]]))
            share = [float((x > BAR).mean()) for x in v]
            both = float((np.concatenate(v) > BAR).mean())
            print(case, "kick", kick, "guarded ticks", [len(x) for x in v], "share above the bar per mask", share,
                  "both", both)
            if 0.1 <= both <= 0.9:
                _cache[key] = (kick, both, v)
                break
    assert _cache[key] is not None, "no kick of 0.02, 0.05, 0.1 puts 10-90 % of the guarded ticks above the bar"
    return _cache[key]


def _triggered(status, mask, F):
    """(B, S, F) bool: a solve status on a tick whose mask bit is clear."""
    t = ~np.isin(status, (DONE, NOMINAL, FIRST_ORDER))
    t[:, :, [i for i in range(F) if (sum(1 << j for j in mask) >> i) & 1]] = False
    return t


@pytest.mark.parametrize("case", list(CASES))
def test_a_guard_that_never_fires_is_mode_1(gpu_lib, monkeypatch, case):
    """ALIPMPC_CL_GUARD_TOL=inf, mask {3}, 3 steps of 8 ticks, kick 0.02: the mode-3 handle gives the mode-1 handle's bits
    on every output — through the per-tick launches, the guard and the (empty) re-solve launches.  All-ones and mask 0
    are mode 0.  Kick 0 under the default tolerance is mode 1 too: x_nex moves by <= 1e-11 between the ticks of a step,
    so u_fo is the anchor plan, whose own violation is at the solve's 1e-8 scale."""
    a = _loop(gpu_lib, monkeypatch, case, 3, "inf", (3,), 3, 8, 0.02)
    b = _loop(gpu_lib, monkeypatch, case, 1, None, (3,), 3, 8, 0.02)
    _same(a, b, tag="inf")
    assert (a["status"] == FIRST_ORDER).sum() >= 30
    for mask in ((1 << 6) - 1, 0):
        kw = dict(steps=2, f_cyc=6, mpc_ticks=mask, kick=0.02, seed=5)
        e = _episodes(gpu_lib, case)
        _same(_sched(_solver(gpu_lib, case, 3), e, **kw), _sched(_solver(gpu_lib, case, 0), e, **kw), tag=mask)
    a = _loop(gpu_lib, monkeypatch, case, 3, None, (3,), 2, 8, 0.0)
    b = _loop(gpu_lib, monkeypatch, case, 1, None, (3,), 2, 8, 0.0)
    _same(a, b, tag="kick 0")
    assert (a["status"] == FIRST_ORDER).sum() >= 30


def test_a_guard_that_always_fires_is_a_solve_at_every_tick(gpu_lib, monkeypatch):
    """ALIPMPC_CL_GUARD_TOL=-1, mask {0}, one step of 6 ticks, kick 0.02.  Per episode, the ticks up to and including the
    first solve that left no valid anchor are the bits of the mode-0 loop that solves at every tick; the ticks after it
    are nominal; no tick is first-order.  (A re-solve is the sensitivity build's launch on the fired episodes alone: the
    solve's own bits.)"""
    case, F = "modi3", 6
    a = _loop(gpu_lib, monkeypatch, case, 3, "-1", (0,), 1, F, 0.02)
    ev = _loop(gpu_lib, monkeypatch, case, 0, None, tuple(range(F)), 1, F, 0.02)
    st = a["status"][:, 0]
    assert not (a["status"] == FIRST_ORDER).any() and (st != DONE).all()
    nom = st == NOMINAL
    n = np.where(nom.any(1), nom.argmax(1), F)          # ticks solved, per episode
    print("episodes by ticks solved", np.bincount(n, minlength=F + 1))
    assert (n >= 1).all() and (n == F).sum() >= 10 and (n < F).any()
    lead = np.arange(F)[None, :] < n[:, None]
    assert (nom | lead).all() and not (nom & lead).any()          # solved ticks, then nominal ticks, nothing else
    for k in ("status", "iters", "plan", "action"):
        assert np.array_equal(a[k][:, 0][lead], ev[k][:, 0][lead], equal_nan=True), k
    assert (a["iters"][:, 0][lead] > 0).all() and (a["iters"][:, 0][nom] == 0).all() and np.isnan(a["plan"][:, 0][nom]).all()
    full = n == F
    for k in ("foot", "x", "hd", "steps_to_goal"):
        assert np.array_equal(a[k][full], ev[k][full], equal_nan=True), k


@pytest.mark.parametrize("case", list(CASES))
def test_the_decision(gpu_lib, monkeypatch, case):
    """Default tolerance, masks {0} and {3}, 2 steps of 8 ticks, at the kick _decision chooses.  Run A never fires (inf),
    run B is the guarded loop.  Per episode, B is A bit for bit up to B's first triggered tick; at that tick the referee
    finds A's row — the plan B's guard refused — above the bar, and at every first-order tick of B it finds B's row at
    or below it: A has rows above the bar, B has none, B has both first-order and triggered ticks, and a first-order tick
    is never followed by a nominal one (an anchored episode's tick is first-order or a re-solve).
    (A's row is B's candidate while the two loops agree, i.e. at an episode's first triggered tick of the run.)"""
    L = gpu_lib
    kick, share, viol_a = _decision(L, monkeypatch, case)
    print(case, "kick chosen", kick, "share of A's guarded ticks above the bar", share)
    left_out = 0
    for mask, va in zip(MASKS, viol_a):
        oa, rpa = _replayed(L, monkeypatch, case, "inf", mask, S3, F3, kick)
        ob, rpb = _replayed(L, monkeypatch, case, None, mask, S3, F3, kick)
        sa, sb = oa["status"], ob["status"]
        trig = _triggered(sb, mask, F3)
        assert not _triggered(sa, mask, F3).any() and (va > BAR).any()
        assert trig.any() and (sb == FIRST_ORDER).any()
        # -21 is never followed by -20 inside a step; triggered ticks carry a solve's iterations and a plan row
        assert not ((sb[:, :, :-1] == FIRST_ORDER) & (sb[:, :, 1:] == NOMINAL)).any()
        assert (ob["iters"][trig] > 0).all() and np.isfinite(ob["plan"][trig]).all()
        tg = rpb["triggered"]
        assert len(tg["b"]) == trig.sum() and trig[tg["b"], tg["s"], tg["i"]].all()
        # B = A up to the first triggered tick of every episode
        tflat = trig.reshape(len(trig), -1)
        first = np.where(tflat.any(1), tflat.argmax(1), S3 * F3)
        lead = np.arange(S3 * F3)[None, :] < first[:, None]
        for k in ("status", "iters", "plan", "action"):
            x, y = (v[k].reshape(len(trig), S3 * F3, -1) for v in (oa, ob))
            assert np.array_equal(x[lead], y[lead], equal_nan=True), (mask, k)
        whole = first >= F3          # step 0 ran untriggered: its touchdown is A's
        assert np.array_equal(oa["foot"][whole, 0], ob["foot"][whole, 0], equal_nan=True)
        assert np.array_equal(oa["x"][whole, 0:2], ob["x"][whole, 0:2])
        # the refused plans: A's row at B's replayed x_nex
        b1 = np.nonzero(first < S3 * F3)[0]
        s1, i1 = first[b1] // F3, first[b1] % F3
        at = {(b, s, i): j for j, (b, s, i) in enumerate(zip(tg["b"], tg["s"], tg["i"]))}
        xn = tg["x_nex"][[at[k] for k in zip(b1, s1, i1)]]
        v1 = _referee(L, case, xn, b1, s1, oa["plan"][b1, s1, i1])
        band = np.abs(v1 - BAR) <= BAR * BAND
        print(mask, "first triggered ticks", len(b1), "of", int(trig.sum()), "triggered; referee min", v1.min(),
              "in the band", v1[band])
        assert (v1[~band] > BAR).all() and np.isfinite(v1).all()
        # the accepted plans: B's own rows
        fo = rpb["fo"]
        assert len(fo["b"]) == (sb == FIRST_ORDER).sum()
        v2 = _referee(L, case, fo["x_nex"], fo["b"], fo["s"], ob["plan"][fo["b"], fo["s"], fo["i"]])
        band2 = np.abs(v2 - BAR) <= BAR * BAND
        print(mask, "first-order ticks of B", len(v2), "referee max", v2.max(), "in the band", v2[band2],
              "A's ticks", len(va), "above the bar", int((va > BAR).sum()))
        assert (v2[~band2] <= BAR).all()
        left_out += int(band.sum() + band2.sum())
    assert left_out <= 2, left_out


def test_triggered_solves_and_their_anchors(gpu_lib, monkeypatch):
    """The same runs (modi N = 3).  At B's first triggered tick of every episode and step, Solver.solve on the same
    handle from the replayed x_nex and the device's previous plan row as warm start returns the recorded status and the
    recorded plan within 1e-6, on a share of the ticks no smaller than the same check gives on A's scheduled solve ticks
    minus 0.02 (test_schedule_gpu.py's margin).  The first-order rows that follow a triggered solve are within
    1e-9 max(1, M) of the replay's, which takes the new anchors from solve_sens (M over the valid anchors)."""
    L, case = gpu_lib, "modi3"
    kick = _decision(L, monkeypatch, case)[0]
    s3, e = _solver(L, case, 3), _episodes(L, case)
    ok_a, ok_b, err, nfo = [], [], [], 0
    for mask in MASKS:
        oa, rpa = _replayed(L, monkeypatch, case, "inf", mask, S3, F3, kick)
        ob, rpb = _replayed(L, monkeypatch, case, None, mask, S3, F3, kick)
        sv = rpa["solves"]
        r = s3.solve(*_scene(e, sv["b"], sv["x_nex"], sv["leg"]), u0=sv["u0"])
        ok_a.append((r["status"] == oa["status"][sv["b"], sv["s"], sv["i"]]) &
                    (np.abs(r["u"] - oa["plan"][sv["b"], sv["s"], sv["i"]]).max(-1) <= 1e-6))
        tg = rpb["triggered"]
        key = tg["b"] * S3 + tg["s"]
        firsts = np.array([np.nonzero(key == k)[0][tg["i"][key == k].argmin()] for k in np.unique(key)])
        b, s, i = tg["b"][firsts], tg["s"][firsts], tg["i"][firsts]
        r = s3.solve(*_scene(e, b, tg["x_nex"][firsts], _od(e, b, s)), u0=tg["u0"][firsts])
        ok_b.append((r["status"] == ob["status"][b, s, i]) & (np.abs(r["u"] - ob["plan"][b, s, i]).max(-1) <= 1e-6))
        an, fo = rpb["anchors"], rpb["fo"]
        M = float(np.abs(an["du"][an["sens_ok"]][:, :, 0:5]).max())
        after = ~np.isin(fo["anchor_i"], mask)          # first-order ticks about a re-solve's anchor
        nfo += int(after.sum())
        d = np.abs(ob["plan"][fo["b"], fo["s"], fo["i"]] - rpb["plan"][fo["b"], fo["s"], fo["i"]]).max(-1)
        print(mask, "anchors", len(an["b"]), "valid", int(an["sens_ok"].sum()), "M", M, "first-order rows after a "
              "triggered solve", int(after.sum()), "max error", d[after].max() if after.any() else 0.0,
              "all first-order rows", d.max())
        err.append(d[after] / (1e-9 * max(1.0, M)))
    ok_a, ok_b, err = np.concatenate(ok_a), np.concatenate(ok_b), np.concatenate(err)
    print("scheduled solve ticks of A", len(ok_a), "share", ok_a.mean(), "first triggered ticks of B", len(ok_b), "share",
          ok_b.mean())
    assert len(ok_b) >= 20 and ok_b.mean() >= ok_a.mean() - 0.02, (ok_b.mean(), ok_a.mean())
    assert nfo >= 10 and (err <= 1.0).all(), (nfo, err.max())


def test_launch_forms_change_no_bit(gpu_lib, monkeypatch):
    """The guarded loop at the default tolerance: one launch per nominal tick (ALIPMPC_CL_FUSE=0) and device pointers on
    a caller's stream give the host-pointer bits; B = 600 in two episode groups gives one group's bits."""
    import torch
    L, case = gpu_lib, "modi3"
    kick = _decision(L, monkeypatch, case)[0]
    s3, e = _solver(L, case, 3), _episodes(L, case)
    S, F, mask = S3, F3, (3,)
    host = _loop(L, monkeypatch, case, 3, None, mask, S, F, kick)
    assert _triggered(host["status"], mask, F).any() and (host["status"] == FIRST_ORDER).any()
    monkeypatch.setenv("ALIPMPC_CL_FUSE", "0")
    _same(_sched(s3, e, steps=S, f_cyc=F, mpc_ticks=mask, kick=kick, seed=5), host, tag="fuse 0")
    monkeypatch.delenv("ALIPMPC_CL_FUSE")
    dev = torch.device("cuda")
    B = len(e["x0"])
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in e.items() if v is not None}
    inp["nc"] = inp["nc"].to(torch.int32)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        out = dict(foot=z((B, S, 3)), x=z((B, S + 1, 5)), hd=z((B, S, 2)), status=z((B, S, F), torch.int32),
                   iters=z((B, S, F), torch.int32), steps_to_goal=z(B, torch.int32), action=z((B, S, F, 8)),
                   plan=z((B, S, F, 15)))
        s3.closed_loop_schedule_device(inp, out, S, f_cyc=F, mpc_ticks=mask, kick=kick, seed=5, stream=st)
    st.synchronize()
    _same({k: v.cpu().numpy() for k, v in out.items()}, host, tag="device pointers")
    e6 = _episodes(L, case, 600)
    outs = {}
    for g in ("1", "2"):
        monkeypatch.setenv("ALIPMPC_CL_GROUPS", g)
        outs[g] = _sched(s3, e6, steps=2, f_cyc=4, mpc_ticks=(1,), kick=kick, seed=5)
    _same(outs["1"], outs["2"], tag="groups")
    t = _triggered(outs["1"]["status"], (1,), 4)
    assert t[:300].any() and t[300:].any() and (outs["1"]["status"][:, 0, 2:4] == FIRST_ORDER).any()


def test_refusals_and_the_other_entry_points(gpu_lib):
    """cl_between = 3 outside solve_sens's domain: EUNSUPPORTED at create; 2, 4 and -1: EINVAL.  solve, solve_sens,
    closed_loop and audit of a mode-3 handle are the mode-0 handle's bits."""
    L, case = gpu_lib, "modi3"
    for variant, N, kw in ((0, 3, dict(precision=L.PREC_FP32)), (0, 3, dict(program=L.PROGRAM_LANE)),
                           (L.VARIANT_DD, 3, {}), (0, 6, dict(nc_max=3))):
        kw = dict(dict(nc_max=5, ne_max=0), **kw)
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            L.Solver(L.default_cfg(variant, N, cl_between=3, **kw))
    for bad in (2, 4, -1):
        with pytest.raises(RuntimeError, match="EINVAL"):
            L.Solver(L.default_cfg(0, 3, nc_max=5, ne_max=0, cl_between=bad))
    s0, s3, e = _solver(L, case, 0), _solver(L, case, 3), _episodes(L, case)
    sc = _scene(e)
    u0 = np.tile(e["x0"], (1, 3))
    sol = s0.solve(*sc, u0=u0)
    for name, a, b in (("solve", s3.solve(*sc, u0=u0), sol),
                       ("solve_sens", s3.solve_sens(*sc, u0=u0), s0.solve_sens(*sc, u0=u0)),
                       ("audit", s3.audit(*sc, u=sol["u"], status=sol["status"], edges=(0.0, 0.1)),
                        s0.audit(*sc, u=sol["u"], status=sol["status"], edges=(0.0, 0.1)))):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
    cl = [s.closed_loop(e["x0"], e["foot0"], e["goal"], e["leg"], e["cir"], e["nc"], steps=2, f_cyc=4, kick=0.02,
                        seed=5) for s in (s3, s0)]
    _same(cl[0], cl[1], KEYS[:-1], "closed_loop")
