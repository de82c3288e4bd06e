"""Plan sensitivities (alipmpc_solve_sens_batch, Solver.solve_sens; alipmpc_solve_sens_obs_batch,
Solver.solve_sens_obs for the obstacle columns): the column layouts, the detour's chain rule in numpy, and the first-order
update of a plan.

The kernel returns dfoot (B, 3, 7) and du (B, 5N, 7): derivatives of the first foothold and of the canonical plan
u_k = x_{k+1} with respect to theta = (x0[0..4], goal[0..1]), taken at the accepted iterate with the barrier parameter
and the prologue's piecewise-constant decisions (obstacle selection, leg parity, whether the detour fires and to which
side) held fixed.  Where the detour fired, the objective's goal is g_eff = x0_pos + Rot(+-pi/12) (g - x0_pos); the
kernel folds d g_eff / d g = Rot and d g_eff / d x0_pos = I - Rot into the columns, so the outputs are total derivatives
with respect to the caller's x0 and goal.  detour_goal / detour_jacobian restate that map here.
"""
import math

import numpy as np

# columns of dfoot / du
COL_X0 = slice(0, 5)      # the five components of x0: px, py, vx, vy, theta
COL_GOAL = slice(5, 7)    # the goal: gx, gy
NCOLS = 7
COLUMNS = ("x0_px", "x0_py", "x0_vx", "x0_vy", "x0_theta", "goal_x", "goal_y")
DETOUR_ANGLE = math.pi / 12


def detour_goal(x0_pos, goal, circles, detour=True):
    """The goal the objective sees (MPC_LIP_modi.py:247-271): (g_eff (2,), side) with side 0 where the detour does not
    fire and +1 / -1 for a turn of +pi/12 / -pi/12.  circles: the selected circles (k, 3) in their order; the first one
    that triggers decides."""
    x0_pos = np.asarray(x0_pos, float)
    g = np.asarray(goal, float).copy()
    if not detour:
        return g, 0
    for c in np.asarray(circles, float).reshape(-1, 3):
        cen = (x0_pos[0] - c[0]) ** 2 + (x0_pos[1] - c[1]) ** 2
        gd = (x0_pos[0] - g[0]) ** 2 + (x0_pos[1] - g[1]) ** 2
        if cen < gd and cen < 9 * c[2] ** 2:
            th = math.atan2(g[1] - x0_pos[1], g[0] - x0_pos[0])
            al = math.atan2(c[1] - x0_pos[1], c[0] - x0_pos[0])
            d = th - al
            if d < 0 and abs(d) > math.pi:
                d += 2 * math.pi
            elif d > 0 and abs(d) > math.pi:
                d -= 2 * math.pi
            if abs(d) < DETOUR_ANGLE:
                side = -1 if d < 0 else 1
                na = th + side * DETOUR_ANGLE
                rr = math.sqrt(gd)
                return np.array([x0_pos[0] + rr * math.cos(na), x0_pos[1] + rr * math.sin(na)]), side
    return g, 0


def detour_side(x0_pos, goal, goal_eff):
    """The side of a fired detour from its result (0: g_eff == goal): the sign of the turn from g - x0 to g_eff - x0, as
    the kernel recovers it."""
    x0_pos, goal, goal_eff = (np.asarray(a, float) for a in (x0_pos, goal, goal_eff))
    if np.array_equal(goal, goal_eff):
        return 0
    a, b = goal - x0_pos, goal_eff - x0_pos
    return 1 if a[0] * b[1] - a[1] * b[0] > 0 else -1


def detour_jacobian(side):
    """(d g_eff / d goal, d g_eff / d x0_pos), both (2, 2), with the decision `side` held fixed: g_eff = x0_pos +
    Rot(side pi/12) (goal - x0_pos) is linear, so they are Rot and I - Rot (I and 0 where the detour did not fire)."""
    if side == 0:
        return np.eye(2), np.zeros((2, 2))
    c, s = math.cos(DETOUR_ANGLE), math.sin(side * DETOUR_ANGLE)
    rot = np.array([[c, -s], [s, c]])
    return rot, np.eye(2) - rot


def fold_detour(d_partial, side):
    """Total derivatives (.., 7) from partial ones whose goal columns are with respect to g_eff and whose x0 columns hold
    g_eff fixed — the chain rule the kernel applies."""
    d = np.array(d_partial, float)
    rot, one_minus = detour_jacobian(side)
    dg = d[..., COL_GOAL].copy()
    d[..., 0:2] += dg @ one_minus
    d[..., COL_GOAL] = dg @ rot
    return d


def obs_columns(nc_max, ne_max):
    """Names of the obstacle columns of dfoot_obs / du_obs (alipmpc_solve_sens_obs_batch, Solver.solve_sens_obs), by the
    caller's input slots: "cir0_cx", "cir0_cy", "cir0_r", ..., then "elp0_cx", "elp0_cy", "elp0_a", "elp0_b",
    "elp0_phi", ... — 3 nc_max + 5 ne_max of them."""
    return tuple(f"cir{j}_{p}" for j in range(nc_max) for p in ("cx", "cy", "r")) + \
        tuple(f"elp{j}_{p}" for j in range(ne_max) for p in ("cx", "cy", "a", "b", "phi"))


def obs_col(kind, slot, nc_max):
    """First column of input slot `slot` of kind "cir" (3 columns: cx, cy, r) or "elp" (5: cx, cy, a, b, phi)."""
    if kind == "cir":
        if not 0 <= slot < nc_max:
            raise ValueError(f"circle slot {slot} outside 0 .. {nc_max - 1}")
        return 3 * slot
    if kind == "elp":
        if slot < 0:
            raise ValueError(f"ellipse slot {slot}")
        return 3 * nc_max + 5 * slot
    raise ValueError(f"kind {kind!r}: 'cir' or 'elp'")


def first_order(u, du, dx0=None, dgoal=None, du_obs=None, dcir=None, delp=None):
    """First-order update of a plan: u + du[..., 0:5] dx0 + du[..., 5:7] dgoal + du_obs [dcir, delp].  u (B, n) with du
    (B, n, 7) (a solve's u and du, or foot (B, 3) and dfoot (B, 3, 7)); dx0 (B, 5) or (5,), dgoal (B, 2) or (2,); either
    may be None (zero).  du_obs (B, n, 3 nc_max + 5 ne_max) (solve_sens_obs' du_obs or dfoot_obs) with dcir (B, nc_max, 3)
    or (nc_max, 3), the change of the circles (cx, cy, r), and delp (B, ne_max, 5) or (ne_max, 5), that of the ellipses
    (cx, cy, a, b, phi); either may be None (zero), and nc_max is read from dcir (0 without it: no circle slots).
    Rows whose derivative is NaN (sens_ok = 0) come back NaN."""
    u = np.asarray(u, float)
    du = np.asarray(du, float)
    if du.shape != u.shape + (NCOLS,):
        raise ValueError(f"du has shape {du.shape}, {u.shape + (NCOLS,)} expected")
    out = u.copy()
    if dx0 is not None:
        out = out + np.einsum("...ij,...j->...i", du[..., COL_X0], np.broadcast_to(np.asarray(dx0, float),
                                                                                  u.shape[:-1] + (5,)))
    if dgoal is not None:
        out = out + np.einsum("...ij,...j->...i", du[..., COL_GOAL], np.broadcast_to(np.asarray(dgoal, float),
                                                                                    u.shape[:-1] + (2,)))
    if dcir is not None or delp is not None:
        if du_obs is None:
            raise ValueError("dcir / delp need du_obs")
        du_obs = np.asarray(du_obs, float)
        if du_obs.shape[:-1] != u.shape:
            raise ValueError(f"du_obs has shape {du_obs.shape}, {u.shape + ('P',)} expected")
        ncol = du_obs.shape[-1]
        if dcir is not None:
            dcir = np.asarray(dcir, float)
            nc3 = 3 * dcir.shape[-2]
            if dcir.shape[-1] != 3 or nc3 > ncol:
                raise ValueError(f"dcir has shape {dcir.shape} for {ncol} obstacle columns")
            flat = np.broadcast_to(dcir.reshape(dcir.shape[:-2] + (nc3,)), u.shape[:-1] + (nc3,))
            out = out + np.einsum("...ij,...j->...i", du_obs[..., :nc3], flat)
        if delp is not None:
            delp = np.asarray(delp, float)
            ne5 = 5 * delp.shape[-2]
            if delp.shape[-1] != 5 or ne5 > ncol or (dcir is not None and nc3 + ne5 != ncol):
                raise ValueError(f"delp has shape {delp.shape} for {ncol} obstacle columns")
            flat = np.broadcast_to(delp.reshape(delp.shape[:-2] + (ne5,)), u.shape[:-1] + (ne5,))
            out = out + np.einsum("...ij,...j->...i", du_obs[..., ncol - ne5:], flat)
    return out
