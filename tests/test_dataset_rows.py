"""alipmpc.dataset on the host: check_rows is first validated on the reference's own recorded rows (the first 160
of sup_learn/X_data.csv, y_mpc_data.csv, y_act_data.csv: tests/golden/g6_sup_learn_rows.npz, tools/gen_goldens.py),
then shown not to be vacuous; and the writers round-trip."""
import numpy as np
import pytest

from alipmpc import dataset

CFG = dict(dt=0.4, g=9.81, H=1.0)   # the reference's step time and pendulum (alipmpc_default_cfg)
# What the recorded rows show on this checker: x_nex 4.4e-16 (0.0 row by row through planner.next_state), y_act
# 0.0, rest_t 5.6e-17, v_des0 0.0, the v_des chain 4.3e-13 (it goes through IPOPT's own x_pred).
TOL, TOL_CHAIN = 1e-12, 1e-9


@pytest.fixture(scope="module")
def rows(golden):
    z = golden("g6_sup_learn_rows")
    return dict(X=z["X"], y_mpc=z["y_mpc"], y_act=z["y_act"], f=int(z["f_cyc"]))


def _check(r, X=None, y_mpc=None, y_act=None, row_start=None):
    X = r["X"] if X is None else X
    return dataset.check_rows(X, r["y_mpc"] if y_mpc is None else y_mpc, r["y_act"] if y_act is None else y_act,
                              [0, len(X)] if row_start is None else row_start, r["f"], 6, 0, CFG, tol=TOL,
                              tol_chain=TOL_CHAIN)


def test_recorded_rows_pass(rows):
    assert rows["X"].shape == (160, 29) and rows["y_mpc"].shape == (160, 8) and rows["y_act"].shape == (160, 8)
    assert rows["f"] == 8
    res = _check(rows)
    print(res)
    assert set(res) == {"rest_t", "step", "stance", "leg", "x_nex", "y_act", "v_des", "v_des0"}
    assert all(res[k] <= TOL for k in ("rest_t", "step", "leg", "x_nex", "y_act", "v_des0")) and res["v_des"] <= TOL_CHAIN
    # the recorded stance foot is the simulated robot's measured one: it moves within a step, so that invariant is
    # reported but only enforced on request (rows written by the library: exactly constant, test_dataset_gpu.py)
    assert 1e-3 < res["stance"] < 2e-2
    with pytest.raises(dataset.RowCheckError, match="stance"):
        dataset.check_rows(rows["X"], rows["y_mpc"], rows["y_act"], [0, 160], 8, 6, 0, CFG, tol_stance=0.0)


def test_x_nex_is_next_state(rows):
    """The vectorised x_nex of check_rows is planner.next_state row by row (the recorded x_nex: 0.0 away)."""
    from alipmpc import planner
    X, y = rows["X"], rows["y_mpc"]
    beta = np.sqrt(CFG["g"] / CFG["H"])
    for r in range(0, 160, 7):
        s0 = r // 8 * 8
        hd_pr = y[r, 3] - (X[s0, 22] - X[0, 22])
        xn, _ = planner.next_state(beta, CFG["dt"], X[r, 18:20], X[r, 20:22], X[r, 22], [*X[r, 23:25], hd_pr], X[r, 28])
        assert np.abs(xn[0:2] - y[r, 4:6]).max() <= TOL


def test_two_episodes_and_empty(rows):
    """row_start splits the rows into episodes: the chain invariants stop at the boundary (an episode's first row
    must then carry alip_des_vel: the second episode here does not)."""
    with pytest.raises(dataset.RowCheckError, match="v_des0"):
        _check(rows, row_start=[0, 80, 160])
    z = np.zeros((0, 8))
    res = dataset.check_rows(np.zeros((0, 29)), z, z, [0, 0, 0], 8, 6, 0, CFG)
    assert max(res.values()) == 0.0


@pytest.mark.parametrize("what", ["y_act_shift", "leg_flip", "v_des", "x_nex", "short_step", "y_act_value", "rest_t"])
def test_checker_not_vacuous(rows, what):
    X, y_mpc, y_act = rows["X"].copy(), rows["y_mpc"].copy(), rows["y_act"].copy()
    rs = None
    if what == "y_act_shift":
        y_act = np.roll(y_act, 1, axis=0)
    elif what == "leg_flip":
        X[43, 27] = -X[43, 27]
    elif what == "v_des":
        y_mpc[43, 6] += 1e-6            # row 43 = tick 3 of step 5: inside the chain
    elif what == "x_nex":
        y_mpc[43, 4] += 1e-9
    elif what == "short_step":
        X, y_mpc, y_act = X[:159], y_mpc[:159], y_act[:159]
    elif what == "y_act_value":
        y_act[40:48, 5] += 1e-9         # constant within the step, but no longer the next step's first state
    elif what == "rest_t":
        X[43, 28] += 1e-9
    with pytest.raises(dataset.RowCheckError):
        _check(rows, X, y_mpc, y_act, rs)


def test_csv_npz_round_trip(rows, tmp_path):
    paths = dataset.write_csv(str(tmp_path / "csv"), rows["X"], rows["y_mpc"], rows["y_act"])
    assert [p.rsplit("/", 1)[1] for p in paths] == ["X_data.csv", "y_mpc_data.csv", "y_act_data.csv"]
    X, y_mpc, y_act = dataset.read_csv(str(tmp_path / "csv"))
    assert np.array_equal(X, rows["X"]) and np.array_equal(y_mpc, rows["y_mpc"]) and np.array_equal(y_act, rows["y_act"])
    p = dataset.write_npz(str(tmp_path / "shards" / "rows_0_1.npz"), rows["X"], rows["y_mpc"], rows["y_act"],
                          row_status=np.zeros(160, np.int32), row_start=[0, 160], seed=3, first=0, f_cyc=8)
    z = dataset.read_npz(p)
    assert np.array_equal(z["X"], rows["X"]) and np.array_equal(z["y_mpc"], rows["y_mpc"])
    assert np.array_equal(z["y_act"], rows["y_act"]) and z["row_start"].dtype == np.int64 and int(z["seed"]) == 3
    assert z["row_status"].dtype == np.int32 and int(z["f_cyc"]) == 8
    _check(rows, z["X"], z["y_mpc"], z["y_act"], z["row_start"])
