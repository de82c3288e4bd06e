"""Guarded first-order ticks of the scheduled closed loop on the host (alipmpc/schedule.py: run with between = 3) — no
GPU.  test_first_order_host.py's affine stand-in solver, u = U0 + D (x_nex - c), restated here: its first-order updates
are exact, so a loop whose guard never fires is the first-order loop and one whose guard always fires is the loop that
solves at every tick."""
import ctypes
import types

import numpy as np
import pytest

NOMINAL, FIRST_ORDER = -20, -21
B, S, F, KICK = 6, 3, 6, 0.05
BAD = [1, 4]


def _standin(bad=()):
    """cfg, episodes and the affine solver; the episodes in `bad` report sens_ok = 0."""
    from alipmpc import schedule
    cfg = types.SimpleNamespace(N=3, variant=0, dt=0.4, g=9.81, H=1.0, cl_between=0)
    k = schedule.constants(cfg)
    rng = np.random.default_rng(2110)
    x0 = np.concatenate([rng.uniform(-0.5, 0.5, (B, 2)), rng.uniform(0.1, 0.4, (B, 1)), rng.uniform(-0.1, 0.1, (B, 1)),
                         rng.uniform(-0.2, 0.2, (B, 1))], axis=1)
    inp = dict(x0=x0, foot0=x0[:, 0:2] + rng.uniform(-0.1, 0.1, (B, 2)), goal=np.full((B, 2), 50.0),
               leg=np.where(np.arange(B) % 2, 1, -1).astype(np.int8))
    c = rng.uniform(-0.3, 0.3, 5)
    D = np.concatenate([np.linalg.matrix_power(k["A"], j + 1) for j in range(3)], axis=0) * 0.2 \
        + 0.01 * rng.uniform(-1, 1, (15, 5))
    U0 = np.tile(np.array([0.3, 0.0, 0.5, 0.0, 0.0]), 3) + 0.05 * rng.uniform(-1, 1, 15)
    bad = np.asarray(bad, int)

    def solve(xn, od, u0, idx):
        u = U0 + (xn - c) @ D.T
        foot, xp = schedule.plan_outputs(k, xn, u)
        du = np.zeros((len(idx), 15, 7))
        du[:, :, 0:5] = D
        return dict(u=u, foot=foot, x_pred=xp, status=np.zeros(len(idx), np.int32), iters=np.ones(len(idx), np.int32),
                    du=du, sens_ok=(~np.isin(idx, bad)).astype(np.int32))
    return schedule, cfg, inp, solve


def _run(schedule, cfg, inp, solve, mask, between, **kw):
    return schedule.run(cfg, inp, mask, solve=solve, steps=S, f_cyc=F, kick=KICK, seed=3, between=between, **kw)


def _const(value):
    calls = []

    def viol(xn, od, u, idx):
        assert xn.shape == (len(idx), 5) and od.shape == (len(idx),) and u.shape == (len(idx), 15)
        calls.append(len(idx))
        return np.full(len(idx), value)
    return viol, calls


def test_a_guard_that_never_fires_is_the_first_order_loop():
    """viol = 0 everywhere: every output of between = 3 is between = 1's, bit for bit; the guard was asked at every
    first-order tick."""
    schedule, cfg, inp, solve = _standin(BAD)
    viol, calls = _const(0.0)
    g = _run(schedule, cfg, inp, solve, [2], 3, viol=viol)
    fo = _run(schedule, cfg, inp, solve, [2], 1)
    assert set(g) == set(fo)
    for key in fo:
        assert np.array_equal(g[key], fo[key], equal_nan=True), key
    assert (g["status"] == FIRST_ORDER).sum() == sum(calls) > 0
    # a tolerance of inf never fires on a finite violation either
    viol, _ = _const(0.5)
    g = _run(schedule, cfg, inp, solve, [2], 3, viol=viol, guard_tol=np.inf)
    assert all(np.array_equal(g[key], fo[key], equal_nan=True) for key in fo)


@pytest.mark.parametrize("value,tol", [(np.inf, 1e-4), (0.0, -1.0), (np.nan, np.inf), (2e-4, 1e-4)])
def test_a_guard_that_always_fires_is_a_solve_at_every_tick(value, tol):
    """Mask {0}, the guard firing at every guarded tick (viol = inf; any viol under a negative tolerance; a NaN under any
    tolerance; a value above the bar): the episodes whose anchors are valid equal the all-ones mask in mode 0 within
    1e-12 max(1, |value|) — with this solver a re-solve's plan is the plan a scheduled solve would have had — and no tick
    is first-order.  The episodes without valid sensitivities are mode 0 under the same mask, bit for bit."""
    schedule, cfg, inp, solve = _standin(BAD)
    viol, calls = _const(value)
    g = _run(schedule, cfg, inp, solve, [0], 3, viol=viol, guard_tol=tol)
    ev = _run(schedule, cfg, inp, solve, schedule.all_ones(F), 0)
    nom = _run(schedule, cfg, inp, solve, [0], 0)
    good = np.setdiff1d(np.arange(B), BAD)
    assert (g["status"] != FIRST_ORDER).all() and sum(calls) == len(good) * S * (F - 1)
    assert (g["status"][good] == 0).all() and (g["iters"][good] == 1).all()
    assert np.abs(g["x"][good, -1, 0:2] - inp["x0"][good, 0:2]).max() > 0.2      # the loop walks
    for key in ("foot", "x", "hd", "action", "target", "plan"):
        a, b = g[key][good], ev[key][good]
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        m = np.isfinite(a)
        err = (np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))).max()
        print(key, err)
        assert err <= 1e-12, (key, err)
    for key in g:
        assert np.array_equal(g[key][BAD], nom[key][BAD], equal_nan=True), key
    assert (g["status"][BAD][:, :, 1:] == NOMINAL).all()


def test_the_guard_decides_per_episode_and_tick():
    """A guard that fires for episode 2 alone, at tick 4 alone (mask {2}): that tick carries a solve's status and
    iterations, ticks 3 and 5 stay first-order (tick 5 about the new anchor), every other episode is the first-order
    loop bit for bit, and with the affine solver episode 2 stays within 1e-12 of it too."""
    schedule, cfg, inp, solve = _standin()
    seen = []

    def viol(xn, od, u, idx):
        seen.append(np.array(idx))
        return np.where(idx == 2, 1.0, 0.0) * (len(seen) % 3 == 2)   # calls come at ticks 3, 4, 5 of each step

    g = _run(schedule, cfg, inp, solve, [2], 3, viol=viol)
    fo = _run(schedule, cfg, inp, solve, [2], 1)
    assert len(seen) == 3 * S
    others = np.setdiff1d(np.arange(B), [2])
    for key in fo:
        assert np.array_equal(g[key][others], fo[key][others], equal_nan=True), key
    assert (g["status"][2, :, 4] == 0).all() and (g["iters"][2, :, 4] == 1).all()
    assert (g["status"][2][:, [3, 5]] == FIRST_ORDER).all() and (g["status"][2, :, 0:2] == NOMINAL).all()
    # after the re-solve the guard is asked about episode 2 again (it has a new anchor)
    assert all(2 in c for c in seen)
    for key in ("foot", "x", "action", "target", "plan"):
        a, b = g[key][2], fo[key][2]
        m = np.isfinite(a)
        assert np.array_equal(m, np.isfinite(b)) and (np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))).max() <= 1e-12


def test_nothing_to_guard_is_mode_0():
    """Mask 0 and the all-ones mask never have an anchor: mode 0's outputs, and the guard is never asked."""
    schedule, cfg, inp, solve = _standin()
    for mask in (0, schedule.all_ones(F)):
        viol, calls = _const(np.inf)
        a, b = _run(schedule, cfg, inp, solve, mask, 3, viol=viol), _run(schedule, cfg, inp, solve, mask, 0)
        assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in a) and not calls, mask
    with pytest.raises(ValueError):
        _run(schedule, cfg, inp, solve, [2], 3)          # no viol callable
    with pytest.raises(ValueError):
        _run(schedule, cfg, inp, solve, [2], 2)          # value 2 stays refused


def test_constants_and_cfg_layout():
    """The new mode is a value of the existing field: 3 in the header, in _lib and in schedule; the cfg keeps its 200
    bytes and round-trips the value; the bar is the header's 1e-4."""
    import os
    import re
    from alipmpc import _lib, schedule
    assert _lib.CL_BETWEEN_GUARDED == schedule.BETWEEN_GUARDED == 3
    assert (_lib.CL_BETWEEN_NOMINAL, _lib.CL_BETWEEN_FIRST_ORDER) == (0, 1)
    assert ctypes.sizeof(_lib.Cfg) == 200 and _lib.Cfg.cl_between.offset == 196
    cfg = _lib.default_cfg(_lib.VARIANT_MODI, 3, cl_between=3)
    assert cfg.cl_between == 3 and _lib.default_cfg(_lib.VARIANT_MODI, 3).cl_between == 0
    assert schedule._between(cfg, None) == 3 and schedule._between(cfg, 1) == 1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "alipmpc.h")).read()
    assert re.search(r"#define ALIPMPC_CL_BETWEEN_GUARDED 3\b", hdr)
    bar = float(re.search(r"#define ALIPMPC_CL_GUARD_VIOL (\S+)", hdr).group(1))
    assert bar == _lib.CL_GUARD_VIOL == schedule.GUARD_VIOL == 1e-4
    assert "ALIPMPC_CL_GUARD_TOL" in hdr
