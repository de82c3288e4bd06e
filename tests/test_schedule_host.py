"""The scheduled closed loop on the host (alipmpc/schedule.py: run) with the C oracle as the solver — no GPU."""
import numpy as np
import pytest

TICK_NOMINAL = -20


def _episodes(coracle, variant, B, seed):
    from alipmpc import scenes
    bt = scenes.make_batch(B, seed=seed, n_cir=5)
    x0 = bt["x0"].copy()
    x0[:8, 0:2] = bt["goal"][:8] - np.array([0.3, 0.2])      # some episodes next to the goal, so that some stop
    leg = bt["leg"].astype(np.int8)
    co = coracle.default_cfg(variant, 3, nc_max=5, ne_max=0)
    foot0 = coracle.solve_batch(co, x0, bt["goal"], leg, bt["cir"], bt["nc"], None, None,
                                np.tile(x0, (1, 3)))["foot"][:, 0:2]
    inp = dict(x0=x0, foot0=foot0, goal=bt["goal"], leg=leg, cir=bt["cir"], nc=bt["nc"])

    def solve(xn, od, u0, idx):
        return coracle.solve_batch(co, xn, bt["goal"][idx], od, bt["cir"][idx], bt["nc"][idx], None, None, u0,
                                   nthreads=8)
    return co, inp, solve


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kick", [0.0, 0.02])
def test_all_ones_mask_is_the_control_rate_loop(coracle, variant, kick):
    """Every tick solving, schedule.run is oracle.closed_loop_batch: statuses, iterations and steps_to_goal equal, every
    float output within 1e-12 (the same formulas in numpy on both sides)."""
    from alipmpc import schedule
    B, S, F = 24, 2, 6
    co, inp, solve = _episodes(coracle, variant, B, 1520 + variant)
    o = schedule.run(co, inp, schedule.all_ones(F), solve=solve, steps=S, f_cyc=F, kick=kick, seed=7)
    ref = coracle.closed_loop_batch(co, inp["x0"], inp["foot0"], inp["goal"], inp["leg"], inp["cir"], inp["nc"],
                                    steps=S, f_cyc=F, kick=kick, seed=7)
    for k in ("status", "iters", "steps_to_goal"):
        assert np.array_equal(o[k], ref[k]), k
    assert (ref["status"] != -10).any()
    for k in ("foot", "x", "hd", "action"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(ref[k])), k
        err = np.nanmax(np.abs(o[k] - ref[k]))
        print(k, err)
        assert err <= 1e-12, (k, err)
    # the recorded plans are the solves' u: row 0 is the touchdown state the foothold and x_nex give
    assert np.isfinite(o["plan"][o["status"] != -10]).all() and np.isnan(o["plan"][o["status"] == -10]).all()


def test_mask_zero_is_the_deadbeat_nominal_gait(coracle):
    """No solve at all: every tick is nominal, nobody reaches a goal, and from the third touchdown on the touchdown
    velocity is alip_des_vel(0.6, leg_ind) of the step it starts — the one-step law is deadbeat."""
    from alipmpc import schedule
    B, S, F = 24, 6, 20
    co, inp, _ = _episodes(coracle, 0, B, 1530)
    o = schedule.run(co, inp, 0, steps=S, f_cyc=F, kick=0.0)
    assert (o["status"] == TICK_NOMINAL).all() and (o["iters"] == 0).all()
    assert (o["steps_to_goal"] == -1).all()
    assert np.isnan(o["plan"]).all() and np.isfinite(o["action"]).all() and np.isfinite(o["foot"]).all()
    k = schedule.constants(co)
    for s in range(2, S + 1):
        want = schedule.des_vel(k, inp["leg"].astype(float) * (-1) ** s)
        err = np.abs(o["x"][:, s, 2:4] - want).max()
        print(s, err)
        assert err <= 1e-12, (s, err)
    # the first two touchdowns are not there yet: the property is not vacuous
    assert np.abs(o["x"][:, 1, 2:4] - schedule.des_vel(k, -inp["leg"].astype(float))).max() > 1e-3


@pytest.mark.parametrize("variant", [0, 1])
def test_nominal_ticks_after_a_solve_keep_its_foothold(coracle, variant):
    """The reference's schedule (tick 15 of 20), ideal plant: on the nominal ticks after the solve, within that step,
    the foothold target is the plan's p_list[0][0:2] (v_des is row 0 of the plan's states, x_1 = A x_nex + B p_0, and
    the projections of later ticks compose to the solve's x_nex)."""
    from alipmpc import schedule
    B, S, F = 24, 3, 20
    co, inp, solve = _episodes(coracle, variant, B, 1540 + variant)
    o = schedule.run(co, inp, [15], solve=solve, steps=S, f_cyc=F, kick=0.0)
    ran = o["status"][:, :, 15] != -10
    assert ran[:, 0].all() and (o["status"][:, :, 15] != TICK_NOMINAL).all()
    nom = np.delete(np.arange(F), 15)
    assert (o["status"][ran][:, nom] == TICK_NOMINAL).all()
    assert np.isnan(o["plan"][:, :, nom]).all() and np.isfinite(o["plan"][ran][:, 15]).all()
    solved = o["target"][ran][:, 15]
    for i in range(16, F):
        err = np.abs(o["target"][ran][:, i] - solved).max()
        print(i, err)
        assert err <= 1e-9, (i, err)
    assert np.abs(o["foot"][ran][:, 0:2] - solved).max() <= 1e-9


def test_mask_of():
    from alipmpc import schedule
    assert schedule.mask_of([15]) == 1 << 15 and schedule.mask_of((0, 2), 5) == 0b101 and schedule.mask_of(6, 3) == 6
    assert schedule.all_ones(64) == (1 << 64) - 1 == schedule.mask_of(range(64), 64)
    for ticks, f in (([5], 5), (1 << 4, 4), ([0], 65), ([0], 0), ([64], None), (-1, None)):
        with pytest.raises(ValueError):
            schedule.mask_of(ticks, f)
