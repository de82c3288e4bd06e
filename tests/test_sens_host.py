"""alipmpc.sensitivity on the CPU: the column layout, the detour's chain rule against central differences of the numpy
detour formula, and the first-order update's shapes."""
import numpy as np
import pytest

from alipmpc import sensitivity as sv


def test_column_layout():
    assert sv.NCOLS == 7 and len(sv.COLUMNS) == 7
    assert (sv.COL_X0.start, sv.COL_X0.stop) == (0, 5) and (sv.COL_GOAL.start, sv.COL_GOAL.stop) == (5, 7)
    assert sv.COLUMNS[:5] == ("x0_px", "x0_py", "x0_vx", "x0_vy", "x0_theta") and sv.COLUMNS[5:] == ("goal_x", "goal_y")


def test_detour_goal_matches_oracle_formula():
    import np_oracle
    rng = np.random.default_rng(5)
    cfg = np_oracle.default_cfg()
    fired = 0
    for _ in range(200):
        x0 = rng.uniform(-1, 1, 2)
        goal = x0 + rng.uniform(3, 6) * np.array([1.0, rng.uniform(-0.3, 0.3)])
        cir = np.array([[x0[0] + rng.uniform(0.8, 2.0), x0[1] + rng.uniform(-0.4, 0.4), rng.uniform(0.4, 0.9)]])
        g, side = sv.detour_goal(x0, goal, cir)
        fired += side != 0
        assert sv.detour_side(x0, goal, g) == side
        assert np.array_equal(g, np_oracle.detour_goal(cfg, x0, goal, cir))
    assert fired >= 20


@pytest.mark.parametrize("side", [1, -1])
def test_detour_jacobian_against_central_differences(side):
    """d g_eff / d goal and d g_eff / d x0_pos of a fired detour, the side held fixed as the kernel holds it"""
    x0 = np.array([0.3, -0.2])
    goal = np.array([5.0, 0.4])
    th = np.arctan2(goal[1] - x0[1], goal[0] - x0[0])
    # a circle just off the line to the goal, on the side that turns the detour to `side`
    al = th - side * 0.05
    cir = np.array([[x0[0] + 1.5 * np.cos(al), x0[1] + 1.5 * np.sin(al), 0.7]])
    g, s0 = sv.detour_goal(x0, goal, cir)
    assert s0 == side
    dg, dx = sv.detour_jacobian(side)
    h = 1e-6
    for j in range(2):
        e = np.zeros(2)
        e[j] = h
        gp, sp = sv.detour_goal(x0, goal + e, cir)
        gm, sm = sv.detour_goal(x0, goal - e, cir)
        assert sp == side and sm == side
        assert np.allclose((gp - gm) / (2 * h), dg[:, j], atol=1e-8)
        gp, sp = sv.detour_goal(x0 + e, goal, cir)
        gm, sm = sv.detour_goal(x0 - e, goal, cir)
        assert sp == side and sm == side
        assert np.allclose((gp - gm) / (2 * h), dx[:, j], atol=1e-8)
    assert np.allclose(dg + dx, np.eye(2))
    i2, z2 = sv.detour_jacobian(0)
    assert np.array_equal(i2, np.eye(2)) and np.array_equal(z2, np.zeros((2, 2)))


def test_fold_detour_is_the_chain_rule():
    rng = np.random.default_rng(2)
    d = rng.normal(size=(4, 9, 7))
    assert np.array_equal(sv.fold_detour(d, 0), d)
    for side in (1, -1):
        rot, om = sv.detour_jacobian(side)
        t = sv.fold_detour(d, side)
        assert np.allclose(t[..., 5:7], d[..., 5:7] @ rot)
        assert np.allclose(t[..., 0:2], d[..., 0:2] + d[..., 5:7] @ om)
        assert np.array_equal(t[..., 2:5], d[..., 2:5])


def test_first_order_shapes():
    rng = np.random.default_rng(3)
    B, n = 6, 15
    u, du = rng.normal(size=(B, n)), rng.normal(size=(B, n, 7))
    dx0, dg = rng.normal(size=(B, 5)), rng.normal(size=(B, 2))
    out = sv.first_order(u, du, dx0, dg)
    assert out.shape == (B, n)
    ref = u + np.einsum("bij,bj->bi", du[:, :, :5], dx0) + np.einsum("bij,bj->bi", du[:, :, 5:], dg)
    assert np.allclose(out, ref)
    assert np.array_equal(sv.first_order(u, du), u)
    assert np.allclose(sv.first_order(u, du, dx0=dx0[0]), u + du[:, :, :5] @ dx0[0])   # one dx0 for the batch
    foot, dfoot = rng.normal(size=(B, 3)), rng.normal(size=(B, 3, 7))
    assert sv.first_order(foot, dfoot, dgoal=dg).shape == (B, 3)
    du[2] = np.nan                                                                       # sens_ok = 0 rows stay NaN
    o = sv.first_order(u, du, dx0, dg)
    assert np.isnan(o[2]).all() and np.isfinite(np.delete(o, 2, axis=0)).all()
    with pytest.raises(ValueError):
        sv.first_order(u, du[:, :, :6], dx0)
