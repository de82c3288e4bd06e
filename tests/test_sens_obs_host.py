"""Obstacle sensitivities (alipmpc_solve_sens_obs_batch), the host side: the column layout, first_order's obstacle terms,
the blocked test scenes, and the referee itself — the C oracle's central differences over x0, goal and every obstacle
parameter (sens_obs_ref.py), which must find the obstacle columns (the random fields leave them at zero) and must
satisfy the translation identity that the device's derivatives are later held to.
"""
import numpy as np
import pytest

import sens_obs_ref as R


def test_obs_columns_and_indices():
    from alipmpc import sensitivity as S
    assert S.obs_columns(2, 1) == ("cir0_cx", "cir0_cy", "cir0_r", "cir1_cx", "cir1_cy", "cir1_r",
                                   "elp0_cx", "elp0_cy", "elp0_a", "elp0_b", "elp0_phi")
    assert S.obs_columns(0, 0) == () and len(S.obs_columns(5, 5)) == 40
    assert S.obs_columns(3, 2)[-1] == "elp1_phi"
    for nc_max, ne_max in ((5, 0), (3, 2), (0, 2)):
        names = S.obs_columns(nc_max, ne_max)
        assert len(names) == 3 * nc_max + 5 * ne_max and len(set(names)) == len(names)
        for j in range(nc_max):
            assert names[S.obs_col("cir", j, nc_max)] == f"cir{j}_cx"
            assert names[S.obs_col("cir", j, nc_max) + 2] == f"cir{j}_r"
        for j in range(ne_max):
            assert names[S.obs_col("elp", j, nc_max)] == f"elp{j}_cx"
            assert names[S.obs_col("elp", j, nc_max) + 4] == f"elp{j}_phi"
    with pytest.raises(ValueError):
        S.obs_col("cir", 3, 3)
    with pytest.raises(ValueError):
        S.obs_col("box", 0, 3)


def test_first_order_with_obstacle_deltas():
    from alipmpc import sensitivity as S
    rng = np.random.default_rng(3)
    B, n, nc_max, ne_max = 6, 15, 3, 2
    P = 3 * nc_max + 5 * ne_max
    u, du, du_obs = rng.normal(size=(B, n)), rng.normal(size=(B, n, 7)), rng.normal(size=(B, n, P))
    dx0, dg = 1e-2 * rng.normal(size=(B, 5)), 1e-2 * rng.normal(size=(2,))
    dcir, delp = 1e-2 * rng.normal(size=(B, nc_max, 3)), 1e-2 * rng.normal(size=(ne_max, 5))
    old = S.first_order(u, du, dx0, dg)
    assert np.array_equal(old, S.first_order(u, du, dx0=dx0, dgoal=dg, du_obs=du_obs))   # no deltas: the old result
    assert np.array_equal(S.first_order(u, du), u)
    delta = np.concatenate([dcir.reshape(B, -1), np.broadcast_to(delp.reshape(-1), (B, 5 * ne_max))], axis=1)
    want = u + np.einsum("bij,bj->bi", du_obs, delta)
    got = S.first_order(u, du, du_obs=du_obs, dcir=dcir, delp=delp)
    assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want))
    # one group at a time, by its columns
    c0 = S.obs_col("elp", 0, nc_max)
    got_c = S.first_order(u, du, du_obs=du_obs, dcir=dcir)
    want_c = u + np.einsum("bij,bj->bi", du_obs[..., :c0], delta[:, :c0])
    assert np.max(np.abs(got_c - want_c)) <= 1e-15 * np.max(np.abs(want_c))
    got_e = S.first_order(u, du, du_obs=du_obs, delp=delp)
    want_e = u + np.einsum("bij,bj->bi", du_obs[..., c0:], delta[:, c0:])
    assert np.max(np.abs(got_e - want_e)) <= 1e-15 * np.max(np.abs(want_e))
    all_ = S.first_order(u, du, dx0, dg, du_obs, dcir, delp)
    assert np.max(np.abs(all_ - (old + want - u))) <= 1e-15 * np.max(np.abs(all_))
    # NaN rows stay NaN; deltas without du_obs, or of another layout, are refused
    bad = du_obs.copy()
    bad[2] = np.nan
    out = S.first_order(u, du, du_obs=bad, dcir=dcir)
    assert np.isnan(out[2]).all() and np.isfinite(np.delete(out, 2, axis=0)).all()
    with pytest.raises(ValueError):
        S.first_order(u, du, dcir=dcir)
    with pytest.raises(ValueError):
        S.first_order(u, du, du_obs=du_obs, dcir=dcir[:, :2], delp=delp)


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_block_path_geometry(name):
    from alipmpc import scenes
    variant, N, nci, nel, seed, B, gap, lat = R.SHAPES[name]
    base = scenes.make_batch(B, seed=seed, n_cir=nci, n_elp=nel, N=N)
    keep = {k: None if v is None else v.copy() for k, v in base.items()}
    a, b = scenes.block_path(base, seed, gap=gap, lat=lat), scenes.block_path(base, seed, gap=gap, lat=lat)
    for k in base:   # a copy: the batch given is untouched, and the result is deterministic
        assert (base[k] is None and a[k] is None) or np.array_equal(base[k], keep[k]), k
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k
    other = scenes.block_path(base, seed + 1, gap=gap, lat=lat)
    assert not np.array_equal(other["cir"], a["cir"])
    rng = np.random.default_rng(1000 + seed)
    g = rng.uniform(gap[0], gap[1], B)
    t = rng.uniform(-lat, lat, B)
    moved_c = np.any(a["cir"] != base["cir"], axis=2)
    moved_e = np.any(a["elp"] != base["elp"], axis=2) if nel else np.zeros((B, 0), bool)
    assert np.all(moved_c.sum(axis=1) + moved_e.sum(axis=1) == 1)   # one obstacle per instance, its centre only
    assert np.array_equal(a["cir"][:, :, 2], base["cir"][:, :, 2])
    if nel:
        assert np.array_equal(a["elp"][:, :, 2:], base["elp"][:, :, 2:])
    for k in ("x0", "goal", "leg", "nc", "u0"):
        assert np.array_equal(a[k], base[k]), k
    slots = set()
    for i in range(B):
        pos = base["x0"][i, :2]
        d = base["goal"][i] - pos
        d /= np.linalg.norm(d)
        n = np.array([-d[1], d[0]])
        if nel and i % 2 == 1:
            j = (i // 2) % nel
            assert moved_e[i, j]
            o, Rad = a["elp"][i, j], max(base["elp"][i, j, 2:4])
            slots.add(("elp", j))
        else:
            j = i % nci
            assert moved_c[i, j]
            o, Rad = a["cir"][i, j], base["cir"][i, j, 2]
            slots.add(("cir", j))
        rel = o[:2] - pos
        assert abs(rel @ d - (Rad + g[i])) <= 1e-12 and abs(rel @ n - t[i] * Rad) <= 1e-12
        assert gap[0] - 1e-12 <= rel @ d - Rad <= gap[1] + 1e-12 and abs(rel @ n) <= lat * Rad + 1e-12   # in the way
    assert len(slots) == nci + nel   # every slot takes its turn


# least (kept, active, ellipse-active) counts of the oracle's reference, detour on and off
COUNTS = {"modi_n3_c5": (55, 55, None), "sig_step_n3_c4": (120, 90, None), "modi_n3_c3e2": (55, 55, 30),
          "modi_n5_c3e2": (40, 40, 14)}


@pytest.mark.parametrize("detour", [1, 0])
@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.slow) if R.SHAPES[n][1] > 3 else n
                                  for n in R.SHAPES])
def test_referee_finds_the_obstacle_columns(coracle, name, detour):
    """On the blocked scenes the oracle's finite differences have obstacle columns of order 1 on most instances, and
    they satisfy the translation identity — which fails by 0.3 and more without the obstacle columns."""
    ref = R.oracle_fd(coracle, name, detour, 1e-10)
    kept, active, elp_active = R.subsets(name, ref)
    amp = np.abs(ref["du"][:, :, 7:]).reshape(len(kept), -1).max(axis=1)
    res = R.translation_residual(name, ref["dfoot"][:, :, :7], ref["du"][:, :, :7], ref["dfoot"][:, :, 7:],
                                 ref["du"][:, :, 7:])[active]
    res0 = R.translation_residual(name, ref["dfoot"][:, :, :7], ref["du"][:, :, :7], None, None)[active]
    print(f"{name} detour {detour}: kept {kept.sum()} active {active.sum()} ellipse-active {elp_active.sum()}  "
          f"median max|du_obs| on active {np.median(amp[active]):.3g}  translation residual median {np.median(res):.3e} "
          f"(without the obstacle columns {np.median(res0):.3g})")
    k, a, e = COUNTS[name]
    assert kept.sum() >= k and active.sum() >= a
    assert e is None or elp_active.sum() >= e
    assert np.median(res) <= 1e-7
    assert np.median(res0) >= 0.1
