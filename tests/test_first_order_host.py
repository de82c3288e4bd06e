"""First-order ticks of the scheduled closed loop on the host (alipmpc/schedule.py: run with between = 1) — no GPU.
An affine stand-in solver, u = U0 + D (x_nex - c), has exact first-order updates: a loop that solves once per step and
updates the plan between equals the loop that solves at every later tick."""
import ctypes
import types

import numpy as np

NOMINAL, FIRST_ORDER = -20, -21
B, S, F, KICK = 6, 3, 6, 0.05


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
    # a plan near the ALIP flow of x_nex (u_k = x_{k+1}), so that the loop walks: D moves every planned state with x_nex
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


def _run(schedule, cfg, inp, solve, mask, between):
    return schedule.run(cfg, inp, mask, solve=solve, steps=S, f_cyc=F, kick=KICK, seed=3, between=between)


def test_affine_solver_first_order_is_a_solve_at_every_tick():
    """Mask {2} with first-order ticks equals mask {2, 3, 4, 5} without, within 1e-12 max(1, |value|); statuses -20
    before the solve of every step and -21 after it."""
    schedule, cfg, inp, solve = _standin()
    fo = _run(schedule, cfg, inp, solve, [2], 1)
    ev = _run(schedule, cfg, inp, solve, [2, 3, 4, 5], 0)
    assert (fo["status"][:, :, 0:2] == NOMINAL).all() and (fo["status"][:, :, 2] == 0).all()
    assert (fo["status"][:, :, 3:6] == FIRST_ORDER).all() and (fo["iters"][:, :, 3:6] == 0).all()
    assert (ev["status"][:, :, 2:6] == 0).all()
    assert np.abs(fo["x"][:, -1, 0:2] - inp["x0"][:, 0:2]).max() > 0.2      # the loop walks
    for key in ("foot", "x", "hd", "action", "target", "plan"):
        a, b = fo[key], ev[key]
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        m = np.isfinite(a)
        err = (np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))).max()
        print(key, err)
        assert err <= 1e-12, (key, err)
    # the default mode is the cfg's
    cfg.cl_between = 1
    dflt = schedule.run(cfg, inp, [2], solve=solve, steps=S, f_cyc=F, kick=KICK, seed=3)
    assert all(np.array_equal(dflt[key], fo[key], equal_nan=True) for key in fo)
    # and the updates are not the unchanged plan: with the kick, the plan rows of a step differ
    assert np.abs(fo["plan"][:, :, 5] - fo["plan"][:, :, 2]).max() > 1e-3


def test_without_an_anchor_the_tick_is_nominal():
    """Episodes whose solver reports sens_ok = 0, and every tick before a step's first solve, are the mode-0 loop bit
    for bit; the other episodes get first-order ticks."""
    bad = [1, 4]
    schedule, cfg, inp, solve = _standin(bad)
    fo = _run(schedule, cfg, inp, solve, [2], 1)
    nom = _run(schedule, cfg, inp, solve, [2], 0)
    good = np.setdiff1d(np.arange(B), bad)
    assert (nom["status"][:, :, [0, 1, 3, 4, 5]] == NOMINAL).all()
    assert (fo["status"][bad][:, :, 3:6] == NOMINAL).all() and (fo["status"][good][:, :, 3:6] == FIRST_ORDER).all()
    for key in fo:
        assert np.array_equal(fo[key][bad], nom[key][bad], equal_nan=True), key
    # step 0 up to and including its solve: nothing has been updated yet, in any episode
    for key in ("status", "iters", "action", "target", "plan"):
        assert np.array_equal(fo[key][:, 0, 0:3], nom[key][:, 0, 0:3], equal_nan=True), key
    assert (fo["status"][:, :, 0:2] == NOMINAL).all()
    assert np.abs(fo["foot"][good, 0] - nom["foot"][good, 0]).max() > 1e-6    # (they touch down on the updated plan)
    # mask 0 and the all-ones mask never have an anchor to use
    for mask in (0, schedule.all_ones(F)):
        a, b = _run(schedule, cfg, inp, solve, mask, 1), _run(schedule, cfg, inp, solve, mask, 0)
        assert all(np.array_equal(a[key], b[key], equal_nan=True) for key in a), mask


def test_cfg_layout_is_the_parents():
    """cl_between takes the place of reserved_: sizeof(alipmpc_cfg) stays 200 (8 int32, 19 doubles, 4 int32 — the
    parent's value, in ctypes and by the header's layout), and the default is the nominal mode."""
    from alipmpc import _lib
    assert ctypes.sizeof(_lib.Cfg) == 200
    assert _lib.Cfg.cl_between.offset == 196 and _lib.Cfg.cl_between.size == 4
    assert [k for k, _ in _lib.Cfg._fields_][-4:] == ["program", "goal_singular", "restoration", "cl_between"]
    from alipmpc import schedule
    assert schedule.TICK_FIRST_ORDER == _lib.TICK_FIRST_ORDER == -21
    assert (_lib.CL_BETWEEN_NOMINAL, _lib.CL_BETWEEN_FIRST_ORDER) == (0, 1)
    assert _lib.default_cfg(_lib.VARIANT_MODI, 3).cl_between == 0


def test_device_roundings_of_the_flow():
    """schedule._fma is a * b + c rounded once, and flow_device — the flow with the fma's of the device kernels, for
    replay's bit-exact solve inputs — is flow within a few roundings, in both of its forms."""
    from alipmpc import schedule
    assert schedule._fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0)[()] == 2.0 ** -29 + 2.0 ** -60   # (plain: 2^-29)
    assert schedule._fma(3.0, 5.0, 7.0)[()] == 22.0
    rng = np.random.default_rng(7)
    a, b, c = rng.normal(size=(3, 200))
    f = schedule._fma(a, b, c)
    assert (f != a * b + c).any() and np.abs(f - (a * b + c)).max() <= 4 * np.finfo(float).eps * 4
    x, (fx, fy, hp) = rng.normal(size=(9, 5)), rng.normal(size=(3, 9))
    ch, shb, bsh = schedule.flow_consts(3.13, 0.17)
    ref = schedule.flow(x, fx, fy, hp, ch, shb, bsh, 0.425)
    for project in (True, False):
        got = schedule.flow_device(x, fx, fy, hp, ch, shb, bsh, 0.425, project)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-14
