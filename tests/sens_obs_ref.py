"""The referee of the obstacle sensitivities (alipmpc_solve_sens_obs_batch): central differences of the C oracle's
solves over all 7 + P parameters (x0, goal, every obstacle slot), on scenes with an obstacle in the way
(scenes.block_path).  Shared by test_sens_obs_host.py (the referee alone) and test_sens_obs_gpu.py (the device against
it); computed once per (shape, detour, tol) and read-only afterwards.
"""
import numpy as np

H = 1e-5
ACTIVE = 0.05   # an instance is active where the reference's max |du_obs| reaches this
# name: variant, N, circles, ellipses, seed, B, gap, lat
SHAPES = {
    "modi_n3_c5": (0, 3, 5, 0, 11, 128, (0.6, 1.4), 0.5),
    "sig_step_n3_c4": (1, 3, 4, 0, 12, 128, (0.6, 1.4), 0.5),
    "modi_n3_c3e2": (0, 3, 3, 2, 13, 128, (0.6, 1.4), 0.5),
    "modi_n5_c3e2": (0, 5, 3, 2, 14, 96, (1.0, 2.5), 0.8),
}
_FD = {}


def batch(name):
    from alipmpc import scenes
    variant, N, nci, nel, seed, B, gap, lat = SHAPES[name]
    return scenes.block_path(scenes.make_batch(B, seed=seed, n_cir=nci, n_elp=nel, N=N), seed, gap=gap, lat=lat)


def ncols(name):
    return 3 * SHAPES[name][2] + 5 * SHAPES[name][3]


def _osolve(coracle, cfg, bt, x0, goal, cir, elp, u0):
    o = coracle.solve_batch(cfg, x0, goal, bt["leg"], cir, bt["nc"], elp, bt.get("ne"), u0, nthreads=8)
    return o["foot"], o["x_pred"].reshape(len(x0), -1), o["status"]   # the plan as the GPU returns it: u_k = x_{k+1}


def oracle_fd(coracle, name, detour, tol):
    """dict(u (B,5N) the base plan, dfoot (B,3,7+P), du (B,5N,7+P): columns 0-6 as solve_sens, then the obstacle
    columns; ok (B,): every one of the 1 + 2 (7 + P) solves ended with status 0) — central differences, h = 1e-5, every
    perturbed solve warm-started from the base plan."""
    key = (name, detour, tol)
    if key in _FD:
        return _FD[key]
    variant, N, nci, nel, seed, B, _, _ = SHAPES[name]
    bt = batch(name)
    P = ncols(name)
    cfg = coracle.default_cfg(variant, N, nc_max=nci, ne_max=nel, tol=tol, max_iter=300, detour=detour)
    _, ub, st = _osolve(coracle, cfg, bt, bt["x0"], bt["goal"], bt["cir"], bt.get("elp"), bt["u0"])
    ok = st == 0
    dfoot, du = np.zeros((B, 3, 7 + P)), np.zeros((B, 5 * N, 7 + P))
    for c in range(7 + P):
        res = []
        for sgn in (1.0, -1.0):
            x0, goal, cir = bt["x0"].copy(), bt["goal"].copy(), bt["cir"].copy()
            elp = None if bt.get("elp") is None else bt["elp"].copy()
            if c < 5:
                x0[:, c] += sgn * H
            elif c < 7:
                goal[:, c - 5] += sgn * H
            elif c < 7 + 3 * nci:
                cir[:, (c - 7) // 3, (c - 7) % 3] += sgn * H
            else:
                e = c - 7 - 3 * nci
                elp[:, e // 5, e % 5] += sgn * H
            f, u, st = _osolve(coracle, cfg, bt, x0, goal, cir, elp, ub)
            ok &= st == 0
            res.append((f, u))
        dfoot[:, :, c] = (res[0][0] - res[1][0]) / (2 * H)
        du[:, :, c] = (res[0][1] - res[1][1]) / (2 * H)
    out = dict(u=ub, dfoot=dfoot, du=du, ok=ok)
    for v in out.values():
        v.setflags(write=False)
    _FD[key] = out
    return out


def subsets(name, ref):
    """(kept, active, ellipse-active) masks of a reference"""
    nci = SHAPES[name][2]
    B = len(ref["ok"])
    amp = np.abs(ref["du"][:, :, 7:]).reshape(B, -1).max(axis=1)
    amp_e = np.abs(ref["du"][:, :, 7 + 3 * nci:]).reshape(B, -1).max(axis=1, initial=0.0)
    kept = np.array(ref["ok"])
    return kept, kept & (amp >= ACTIVE), kept & (amp_e >= ACTIVE)


def centre_cols(name, ax):
    """the obstacle columns (offsets into the P obstacle columns) of every slot's centre coordinate `ax`"""
    _, _, nci, nel = SHAPES[name][:4]
    return [3 * j + ax for j in range(nci)] + [3 * nci + 5 * j + ax for j in range(nel)]


def translation_residual(name, dfoot, du, dfoot_obs, du_obs):
    """Per instance: how far the derivatives are from the translation identity.  Moving x0's position, the goal and
    every obstacle centre by one vector moves the plan's positions by it: along axis ax, du[:, :, ax] + du[:, :, 5 + ax]
    + sum over slots of du_obs[:, :, centre column ax] is 1 on the plan's position rows of that axis and 0 elsewhere,
    and the same sum of dfoot is (1, 0, 0) or (0, 1, 0).  dfoot_obs / du_obs None: without the obstacle columns.
    A non-finite derivative counts as infinitely far."""
    B, n = du.shape[:2]
    res = np.zeros(B)
    for ax in (0, 1):
        tu = du[:, :, ax] + du[:, :, 5 + ax]
        tf = dfoot[:, :, ax] + dfoot[:, :, 5 + ax]
        if du_obs is not None:
            cc = centre_cols(name, ax)
            tu = tu + du_obs[:, :, cc].sum(axis=2)
            tf = tf + dfoot_obs[:, :, cc].sum(axis=2)
        eu = (np.arange(n) % 5 == ax).astype(float)
        ef = (np.arange(3) == ax).astype(float)
        r = np.maximum(np.abs(tu - eu).max(axis=1), np.abs(tf - ef).max(axis=1))
        res = np.maximum(res, np.where(np.isfinite(r), r, np.inf))
    return res
