"""Plan audit (alipmpc_audit_batch, include/alipmpc.h): names for the layout, a numpy restatement of the
geometric columns, and the summary.

  COLS, WHERE, SUMMARY_FIELDS   names of the metrics columns, the where columns and the first summary words
  radial_clearance(p, obs)      signed distance to an obstacle's boundary along the ray from its centre
  audit_host(cfg, inputs, u)    columns 1-4 and where[1:3] with numpy, on planner.plan_traces (the pos_det traces,
                                pinned to the reference by the g4_aux golden); column 0 (viol) is the eval hook's
                                business and stays NaN here
  summarise(metrics, status, edges, viol_tol)   the summary words from a metrics array
  describe(summary, n_edges)    the summary as a dict for JSON
"""
import numpy as np

from . import planner

COLS = ("viol", "clear", "clear_knot", "goal_1", "goal_N")
WHERE = ("viol_row", "clear_row", "clear_obs")
SUMMARY_FIELDS = ("instances", "nonfinite", "viol_ok", "clear_ok", "both_ok", "between_knots")
STATUS_CLASSES = ("0", "1", "-1", "2", "other")   # cross-table classes, in order
HEAD, CROSS = len(SUMMARY_FIELDS), 4 * len(STATUS_CLASSES)


def summary_len(n_edges):
    return HEAD + (int(n_edges) + 1) + CROSS


def radial_clearance(p, obs):
    """Radial clearance of points p (..., 2) to obstacles obs (..., 5) = [cx, cy, a, b, phi] (broadcast against each
    other; a circle is a = b = r, phi = 0; the semi-axis a lies along phi): with d = p - c and
    Q = ((dx cos + dy sin) / a)^2 + ((-dx sin + dy cos) / b)^2 it is |d| (1 - 1 / sqrt(Q)), and -min(a, b) at d = 0."""
    p, obs = np.asarray(p, float), np.asarray(obs, float)
    dx, dy = p[..., 0] - obs[..., 0], p[..., 1] - obs[..., 1]
    a, b, c, s = obs[..., 2], obs[..., 3], np.cos(obs[..., 4]), np.sin(obs[..., 4])
    dn = np.hypot(dx, dy)
    Q = ((dx * c + dy * s) / a) ** 2 + ((-dx * s + dy * c) / b) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dn * (1.0 - 1.0 / np.sqrt(Q))
    return np.where(dn > 0, out, -np.minimum(a, b) + 0.0 * dn)


def obstacle_list(nc_max, cir, nc, elp=None, ne=None):
    """One instance's valid obstacles as (n, 5) rows [cx, cy, a, b, phi] and their slots (circle j: j, ellipse j:
    nc_max + j), in slot order."""
    nc = int(min(max(nc, 0), nc_max))
    rows = [[c[0], c[1], c[2], c[2], 0.0] for c in np.asarray(cir, float).reshape(-1, 3)[:nc]]
    slots = list(range(nc))
    if elp is not None and ne is not None:
        e = np.asarray(elp, float).reshape(-1, 5)
        n = int(min(max(ne, 0), len(e)))
        rows += [list(r) for r in e[:n]]
        slots += [nc_max + j for j in range(n)]
    return np.asarray(rows, float).reshape(-1, 5), np.asarray(slots, np.int32)


def audit_host(cfg, inputs, u):
    """numpy restatement of metrics columns 1-4 and where columns 1-2 for inputs = dict(x0, goal, cir, nc[, elp, ne])
    and plans u (B, 5N).  Returns dict(metrics (B, 5) with column 0 NaN, where (B, 3) with column 0 = -1, trace
    (B, N * rows, 2)).  Ties: the first minimum in row-major (row, slot) order."""
    x0 = np.asarray(inputs["x0"], float).reshape(-1, 5)
    B, N = len(x0), int(cfg.N)
    u = np.asarray(u, float).reshape(B, 5 * N)
    goal = np.broadcast_to(np.asarray(inputs["goal"], float), (B, 2))
    k = planner.alip_constants(cfg.dt, cfg.g, cfg.H)
    finite = np.isfinite(x0).all(1) & np.isfinite(goal).all(1) & np.isfinite(u).all(1)
    safe_x0, safe_u = np.where(finite[:, None], x0, 0.0), np.where(finite[:, None], u, 0.0)
    tr = planner.plan_traces(k["beta"], cfg.dt, k["A"], k["W"], k["M_A"], k["M_B"], safe_x0, safe_u)
    rows = tr.shape[2]
    tr = tr.reshape(B, N * rows, 2)
    knots = [j * rows for j in range(N)] + [N * rows - 1]
    metrics = np.full((B, 5), np.nan)
    where = np.full((B, 3), -1, np.int32)
    elp, ne = inputs.get("elp"), inputs.get("ne")
    for b in range(B):
        if not finite[b]:
            continue
        obs, slots = obstacle_list(cfg.nc_max, inputs["cir"][b] if cfg.nc_max else np.zeros((0, 3)), inputs["nc"][b],
                                   None if elp is None else elp[b], None if ne is None else ne[b])
        if len(obs):
            cl = radial_clearance(tr[b][:, None, :], obs[None, :, :])
            i = int(np.argmin(cl))                       # first minimum, row-major
            metrics[b, 1], where[b, 1], where[b, 2] = cl.flat[i], i // len(obs), slots[i % len(obs)]
            metrics[b, 2] = cl[knots].min()
        else:
            metrics[b, 1] = metrics[b, 2] = np.inf
        metrics[b, 3] = np.hypot(*(tr[b, knots[1]] - goal[b]))
        metrics[b, 4] = np.hypot(*(tr[b, knots[N]] - goal[b]))
    return dict(metrics=metrics, where=where, trace=tr)


def status_class(status):
    """Cross-table class of solve statuses: 0, 1, -1, 2, other -> 0..4."""
    s = np.asarray(status)
    return np.select([s == 0, s == 1, s == -1, s == 2], [0, 1, 2, 3], 4)


def summarise(metrics, status=None, edges=(), viol_tol=1e-4):
    """The summary words (int64, summary_len(len(edges))) of a metrics array (B, 5); status (B,) or None (the 20
    cross-table words then stay 0)."""
    m = np.asarray(metrics, float).reshape(-1, 5)
    edges = np.asarray(edges, float).reshape(-1)
    out = np.zeros(summary_len(len(edges)), np.int64)
    bad = np.isnan(m).any(1)
    ok = ~bad
    viol, clear, knot = m[ok, 0], m[ok, 1], m[ok, 2]
    vok, cok = viol <= viol_tol, clear >= 0
    out[0:6] = [len(m), bad.sum(), vok.sum(), cok.sum(), (vok & cok).sum(), ((clear < 0) & (knot >= 0)).sum()]
    bins = np.searchsorted(edges, clear, side="right")   # edges[i - 1] <= clear < edges[i]
    out[HEAD:HEAD + len(edges) + 1] = np.bincount(bins, minlength=len(edges) + 1)
    if status is not None:
        idx = status_class(np.asarray(status).reshape(-1)[ok]) * 4 + 2 * cok + vok
        out[HEAD + len(edges) + 1:] = np.bincount(idx, minlength=CROSS)
    return out


def describe(summary, n_edges, edges=None):
    """The summary as a dict (JSON-ready): the named counts, the histogram, the cross table by status class."""
    s = [int(v) for v in np.asarray(summary).reshape(-1)]
    if len(s) != summary_len(n_edges):
        raise ValueError(f"summary has {len(s)} words, expected {summary_len(n_edges)}")
    d = dict(zip(SUMMARY_FIELDS, s[:HEAD]))
    d["clear_hist"] = s[HEAD:HEAD + n_edges + 1]
    if edges is not None:
        d["clear_edges"] = [float(e) for e in edges]
    cross = s[HEAD + n_edges + 1:]
    d["by_status"] = {c: {"clear_neg_viol_bad": cross[4 * i], "clear_neg_viol_ok": cross[4 * i + 1],
                          "clear_ok_viol_bad": cross[4 * i + 2], "clear_ok_viol_ok": cross[4 * i + 3]}
                      for i, c in enumerate(STATUS_CLASSES)}
    return d
