"""Imitation-learning rows (X, y_mpc, y_act) of the closed loop: a host checker and the writers.

The rows are what the reference's logger appends per MPC call (data_procs/logger_iml.py:377-401 X and y_mpc,
gen_act_res :416-428 y_act) and ships as sup_learn/X_data.csv, y_mpc_data.csv, y_act_data.csv;
Solver.closed_loop_dataset / alipmpc_closed_loop_dataset_batch (include/alipmpc.h) write them on the device.
check_rows restates the identities the logger's arithmetic implies between the columns, so it holds for the
reference's recorded rows (tests/golden/g6_sup_learn_rows.npz) and for rows produced here alike.  Host only:
nothing in this module touches the library.
"""
import math
import os

import numpy as np

from . import planner

CSV_NAMES = ("X_data.csv", "y_mpc_data.csv", "y_act_data.csv")   # the reference's sup_learn/ file names
VX_MAX = 0.6        # main_sim_mpc.py:54: vel_des = alip_des_vel(0.6, leg_ind)
STEP_GAP = 0.3      # MPC_LIP_modi.py:181-186


class RowCheckError(ValueError):
    """check_rows: an invariant of the rows is violated (or their layout is not whole steps)."""


def x_cols(nc_max, ne_max):
    return 3 * nc_max + 5 * ne_max + 11


def _get(cfg, k):
    return float(cfg[k] if isinstance(cfg, dict) else getattr(cfg, k))


def check_rows(X, y_mpc, y_act, row_start, f_cyc, nc_max, ne_max, cfg, tol=1e-12, tol_chain=1e-9, tol_stance=None):
    """Check the invariants of dataset rows; returns {invariant: maximal residual}, raises RowCheckError on a violation.

    X (R, 3 nc_max + 5 ne_max + 11), y_mpc (R, 8), y_act (R, 8); row_start (B + 1,) CSR offsets of the episodes;
    cfg: anything with dt, g, H (a Cfg or a dict).  tol bounds every invariant but the v_des chain (tol_chain), which
    goes through the solver's own prediction.  With T = cfg.dt, i the position in the step, s the step:
      rest_t     X[:, -1] == T - i (T / f_cyc)
      step       leg_ind, y_mpc[:, 3] and y_act are constant within a step; y_mpc[:, 2] == y_act[:, 2] == 0
      stance     the stance foot is constant within a step.  Always reported, enforced only with tol_stance: it holds
                 for an ALIP plant (rows written here: exactly), not for the reference's recorded rows, whose stance
                 foot is the simulated robot's measured one and moves up to 1.06e-2 within a step
      leg        leg_ind is +-1 and alternates between the steps of an episode
      x_nex      y_mpc[:, 4:6] == get_next_states(pos, vel, hd, [stance foot, hd_pr], rest_t)[0:2] with the matrices of
                 planner.next_state, hd_pr = y_mpc[:, 3] - (heading of the step's first row - of the episode's first)
      y_act      y_act of step s == stance foot, heading, position, velocity of the first X row of step s + 1
      v_des      v_des of row r + 1 (not the first of a step) == velocity of the ALIP flow of x_nex(r) about
                 y_mpc[r, 0:2] over a full step T (main_sim_mpc.py:88: vel_des <- mpc_state_tar[0][2:4])
      v_des0     v_des of the episode's first row == alip_des_vel(0.6, leg_ind)
    """
    X, y_mpc, y_act = (np.asarray(a, np.float64) for a in (X, y_mpc, y_act))
    rs = np.asarray(row_start, np.int64)
    f = int(f_cyc)
    o = 3 * nc_max + 5 * ne_max
    if X.ndim != 2 or X.shape[1] != o + 11 or y_mpc.shape != (len(X), 8) or y_act.shape != (len(X), 8):
        raise RowCheckError(f"shapes X {X.shape}, y_mpc {y_mpc.shape}, y_act {y_act.shape} for {o + 11} columns")
    cnt = np.diff(rs)
    if rs.ndim != 1 or len(rs) < 1 or rs[0] != 0 or rs[-1] != len(X) or (cnt < 0).any():
        raise RowCheckError(f"row_start does not cover the {len(X)} rows")
    if (cnt % f).any():
        b = int(np.nonzero(cnt % f)[0][0])
        raise RowCheckError(f"episode {b} has {int(cnt[b])} rows: not whole steps of {f}")
    R = len(X)
    res = dict(rest_t=0.0, step=0.0, stance=0.0, leg=0.0, x_nex=0.0, y_act=0.0, v_des=0.0, v_des0=0.0)
    if R == 0:
        return res
    T, g, H = _get(cfg, "dt"), _get(cfg, "g"), _get(cfg, "H")
    beta = math.sqrt(g / H)
    pos, vel, hd, stf = X[:, o:o + 2], X[:, o + 2:o + 4], X[:, o + 4], X[:, o + 5:o + 7]
    leg, rest = X[:, o + 9], X[:, o + 10]
    ep = np.repeat(np.arange(len(cnt)), cnt)            # episode of each row
    i = (np.arange(R) - rs[ep]) % f                     # position in the step
    nst = R // f                                        # all steps, episode-major
    first = np.arange(nst) * f                          # first row of each step
    ep_s = ep[first]
    rest_pos = T - i * (T / f)
    res["rest_t"] = float(np.abs(rest - rest_pos).max())

    def within(a):   # maximal deviation from the step's first row
        a = a.reshape(nst, f, -1)
        return float(np.abs(a - a[:, :1]).max())
    res["step"] = max(within(leg), within(y_mpc[:, 3]), within(y_act),
                      float(np.abs(y_mpc[:, 2]).max()), float(np.abs(y_act[:, 2]).max()))
    res["stance"] = within(stf)
    nxt = np.nonzero(ep_s[1:] == ep_s[:-1])[0]          # steps with a successor in their episode
    res["leg"] = float(np.abs(np.abs(leg) - 1.0).max())
    if len(nxt):
        res["leg"] = max(res["leg"], float(np.abs(leg[first[nxt]] + leg[first[nxt + 1]]).max()))
        a, b = first[nxt], first[nxt + 1]
        res["y_act"] = float(max(np.abs(y_act[a, 0:2] - stf[b]).max(), np.abs(y_act[a, 3] - hd[b]).max(),
                                 np.abs(y_act[a, 4:6] - pos[b]).max(), np.abs(y_act[a, 6:8] - vel[b]).max()))
    # x_nex of every row, tick by tick with planner.next_state's matrices
    hd_pr = y_mpc[:, 3] - (hd[np.repeat(first, f)] - hd[rs[ep]])
    xk = np.concatenate([pos, vel, hd[:, None]], 1)
    p = np.concatenate([stf, hd_pr[:, None]], 1)
    xn = np.empty((R, 5))
    for k in range(f):
        A, Bm = planner._alip_matrices(beta, T - k * (T / f), T)
        m = i == k
        xn[m] = xk[m] @ A.T + p[m] @ Bm.T
    res["x_nex"] = float(np.abs(y_mpc[:, 4:6] - xn[:, 0:2]).max())
    # v_des chain: the flow of x_nex(r) about the planned foothold over T
    A, Bm = planner._alip_matrices(beta, T, T)
    vnext = (xn @ A.T)[:, 2:4] + y_mpc[:, 0:2] @ Bm[2:4, 0:2].T
    r = np.nonzero(i[1:] != 0)[0]                       # rows r whose successor is in the same step
    if len(r):
        res["v_des"] = float(np.abs(y_mpc[r + 1, 6:8] - vnext[r]).max())
    e0 = rs[:-1][cnt > 0]
    sigma = beta / math.tanh(T * beta / 2)
    v0 = np.stack([np.full(len(e0), sigma * VX_MAX * T / 2),
                   0.5 * (-0.5 * leg[e0] * STEP_GAP) * (beta * math.sinh(beta * T)) / (math.cosh(beta * T) + 1)], 1)
    res["v_des0"] = float(np.abs(y_mpc[e0, 6:8] - v0).max())
    bars = {k: (tol_chain if k == "v_des" else tol) for k in res}
    bars["stance"] = math.inf if tol_stance is None else tol_stance
    bad = {k: v for k, v in res.items() if not v <= bars[k]}   # (a NaN residual is a violation)
    if bad:
        raise RowCheckError("dataset rows violate " + ", ".join(f"{k}: {v:.3g} > {bars[k]:.3g}" for k, v in bad.items()))
    return res


def write_csv(dir, X, y_mpc, y_act):
    """Write the reference's three files (sup_learn/: X_data.csv, y_mpc_data.csv, y_act_data.csv; comma-separated,
    no header, 17 significant digits so the doubles read back exactly).  Returns the paths."""
    os.makedirs(dir, exist_ok=True)
    paths = []
    for name, a in zip(CSV_NAMES, (X, y_mpc, y_act)):
        p = os.path.join(dir, name)
        np.savetxt(p, np.asarray(a, np.float64), delimiter=",", fmt="%.17g")
        paths.append(p)
    return paths


def read_csv(dir):
    """(X, y_mpc, y_act) from a directory of the reference's three files."""
    return tuple(np.loadtxt(os.path.join(dir, n), delimiter=",", ndmin=2) for n in CSV_NAMES)


def write_npz(path, X, y_mpc, y_act, row_status=None, row_start=None, **meta):
    """Write one shard: the row arrays, row_start, and scalar metadata (seed, first, f_cyc, ...)."""
    d = dict(X=np.asarray(X, np.float64), y_mpc=np.asarray(y_mpc, np.float64), y_act=np.asarray(y_act, np.float64))
    if row_status is not None:
        d["row_status"] = np.asarray(row_status, np.int32)
    if row_start is not None:
        d["row_start"] = np.asarray(row_start, np.int64)
    d.update({k: np.asarray(v) for k, v in meta.items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **d)
    return path


def read_npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
