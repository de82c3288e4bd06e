"""CPU: the plan audit's host side (alipmpc/audit.py) — the radial clearance against hand values, audit_host against a
brute force written here (a loop over planner.plan_traces rows x obstacles), and summarise against brute-force counts."""
import math

import numpy as np
import pytest

from alipmpc import audit, planner


class Cfg:
    """the fields audit_host reads (an alipmpc_cfg without the library)"""
    def __init__(self, N, nc_max, ne_max):
        self.N, self.nc_max, self.ne_max = N, nc_max, ne_max
        self.dt, self.g, self.H = 0.4, 9.81, 1.0


def test_radial_clearance_hand_values():
    rc = audit.radial_clearance
    # circle: hypot - r
    assert rc([3.0, 4.0], [0, 0, 2.0, 2.0, 0.0]) == pytest.approx(3.0, abs=1e-15)
    assert rc([1.5, -1.0], [0.5, -1.0, 2.5, 2.5, 0.0]) == pytest.approx(-1.5, abs=1e-15)
    # ellipse on each axis: |d| - a and |d| - b
    e = [1.0, 2.0, 0.8, 0.5, 0.0]
    assert rc([1.0 + 2.0, 2.0], e) == pytest.approx(2.0 - 0.8, abs=1e-15)
    assert rc([1.0, 2.0 - 1.5], e) == pytest.approx(1.5 - 0.5, abs=1e-15)
    # on the boundary: 0
    assert rc([1.8, 2.0], e) == pytest.approx(0.0, abs=1e-15)
    assert rc([1.0, 2.5], e) == pytest.approx(0.0, abs=1e-15)
    th = 0.7
    assert rc([1.0 + 0.8 * math.cos(th), 2.0 + 0.8 * math.sin(th)], [1.0, 2.0, 0.8, 0.5, th]) == pytest.approx(0.0, abs=1e-15)
    # phi = pi / 2 swaps the axes: a now lies along y
    q = [1.0, 2.0, 0.8, 0.5, math.pi / 2]
    assert rc([1.0, 2.0 + 2.0], q) == pytest.approx(2.0 - 0.8, abs=1e-15)
    assert rc([1.0 - 1.5, 2.0], q) == pytest.approx(1.5 - 0.5, abs=1e-15)
    # the centre: -min(a, b)
    assert rc([1.0, 2.0], e) == -0.5
    assert rc([0.0, 0.0], [0, 0, 2.0, 2.0, 0.0]) == -2.0
    # broadcast: points x obstacles
    out = rc(np.array([[3.0, 4.0], [0.0, 0.0]])[:, None, :], np.array([[0, 0, 2.0, 2.0, 0.0], e])[None])
    assert out.shape == (2, 2) and out[1, 0] == -2.0 and out[0, 0] == pytest.approx(3.0)


def _case(N, nc_max, ne_max, B, seed):
    r = np.random.default_rng(seed)
    x0 = np.column_stack([r.uniform(0, 8, B), r.uniform(0, 8, B), r.uniform(0.3, 0.7, B), r.uniform(-0.3, 0.3, B),
                          r.uniform(-1, 1, B)])
    u = np.tile(x0, (1, N)) + 0.3 * r.standard_normal((B, 5 * N))
    cir = np.zeros((B, nc_max, 3))
    cir[..., 0:2] = x0[:, None, 0:2] + r.uniform(-2, 2, (B, nc_max, 2))
    cir[..., 2] = r.uniform(0.5, 1.2, (B, nc_max))
    elp = np.zeros((B, ne_max, 5))
    elp[..., 0:2] = x0[:, None, 0:2] + r.uniform(-2, 2, (B, ne_max, 2))
    elp[..., 2] = r.uniform(0.6, 1.2, (B, ne_max))
    elp[..., 3] = elp[..., 2] * r.uniform(0.5, 1.0, (B, ne_max))
    elp[..., 4] = r.uniform(0, math.pi, (B, ne_max))
    nc = r.integers(0, nc_max + 1, B).astype(np.int32)
    ne = r.integers(0, ne_max + 1, B).astype(np.int32)
    nc[0] = 0
    ne[0] = 0                                     # an instance without obstacles
    goal = np.tile([10.0, 10.0], (B, 1))
    inp = dict(x0=x0, goal=goal, cir=cir, nc=nc)
    if ne_max:
        inp.update(elp=elp, ne=ne)
    return inp, u


@pytest.mark.parametrize("N,nc_max,ne_max", [(1, 1, 0), (3, 5, 0), (5, 5, 5), (3, 3, 4)])
def test_audit_host_matches_brute_force(N, nc_max, ne_max):
    B = 12
    cfg = Cfg(N, nc_max, ne_max)
    inp, u = _case(N, nc_max, ne_max, B, 100 + N)
    got = audit.audit_host(cfg, inp, u)
    k = planner.alip_constants()
    tr = planner.plan_traces(k["beta"], 0.4, k["A"], k["W"], k["M_A"], k["M_B"], inp["x0"], u)
    rows = tr.shape[2]
    assert rows == 42
    for b in range(B):
        obs = [(j, inp["cir"][b, j, 0], inp["cir"][b, j, 1], inp["cir"][b, j, 2], inp["cir"][b, j, 2], 0.0)
               for j in range(inp["nc"][b])]
        if ne_max:
            obs += [(nc_max + j, *inp["elp"][b, j]) for j in range(inp["ne"][b])]
        best, best_at, knot = math.inf, (-1, -1), math.inf
        for kk in range(N):
            for r in range(rows):
                px, py = tr[b, kk, r]
                for slot, cx, cy, a, bb, phi in obs:
                    dx, dy = px - cx, py - cy
                    dn = math.hypot(dx, dy)
                    if dn == 0:
                        c = -min(a, bb)
                    else:
                        qu = (dx * math.cos(phi) + dy * math.sin(phi)) / a
                        qv = (-dx * math.sin(phi) + dy * math.cos(phi)) / bb
                        c = dn * (1 - 1 / math.sqrt(qu * qu + qv * qv))
                    if c < best:                       # strict: the first (row, slot) of equal minima stays
                        best, best_at = c, (kk * rows + r, slot)
                    if r == 0 or (kk == N - 1 and r == rows - 1):
                        knot = min(knot, c)
        m, w = got["metrics"][b], got["where"][b]
        assert np.isnan(m[0]) and w[0] == -1
        if not obs:
            assert m[1] == math.inf and m[2] == math.inf and w[1] == -1 and w[2] == -1
        else:
            assert abs(m[1] - best) <= 1e-13 and abs(m[2] - knot) <= 1e-13
            assert (w[1], w[2]) == best_at
            assert w[1] % rows != 1                    # rows 0 and 1 of a step are one point: row 0 wins the tie
        k1 = tr[b, 1, 0] if N > 1 else tr[b, 0, rows - 1]
        kN = tr[b, N - 1, rows - 1]
        assert m[3] == pytest.approx(math.hypot(*(k1 - inp["goal"][b])), abs=1e-13)
        assert m[4] == pytest.approx(math.hypot(*(kN - inp["goal"][b])), abs=1e-13)


def test_audit_host_tie_rule_and_non_finite():
    """Row 0 and row 1 of a step are bit-equal, so a minimum at a knot is a tie: the smaller row wins; two identical
    obstacles tie on the slot: the smaller slot wins.  Non-finite instances are NaN / -1."""
    cfg = Cfg(3, 3, 0)
    inp, u = _case(3, 3, 0, 4, 7)
    inp["nc"][:] = 3
    x0 = inp["x0"]
    # an obstacle right behind the start, twice: x_0 is the closest trace point, slots 1 and 2 are the same circle
    inp["cir"][:, 0] = [50.0, 50.0, 0.5]
    inp["cir"][:, 1, 0:2] = x0[:, 0:2] - 0.2 * np.column_stack([np.cos(x0[:, 4]), np.sin(x0[:, 4])])
    inp["cir"][:, 1, 2] = 0.5
    inp["cir"][:, 2] = inp["cir"][:, 1]
    u = np.tile(x0 + np.column_stack([0.3 * np.cos(x0[:, 4]), 0.3 * np.sin(x0[:, 4]), 0 * x0[:, 0:3]]), (1, 3))
    tr = audit.audit_host(cfg, inp, u)["trace"]
    assert np.array_equal(tr[:, 0], tr[:, 1])
    u[2, 4] = np.nan
    got = audit.audit_host(cfg, inp, u)
    for b in (0, 1, 3):
        assert tuple(got["where"][b, 1:]) == (0, 1), got["where"][b]
    assert np.isnan(got["metrics"][2]).all() and (got["where"][2] == -1).all()


def test_summarise_counts_additivity_and_edges():
    r = np.random.default_rng(5)
    B = 400
    m = np.column_stack([np.where(r.random(B) < 0.5, 0.0, r.uniform(0, 1e-3, B)), r.normal(0.1, 0.3, B),
                         r.normal(0.2, 0.3, B), r.uniform(0, 5, B), r.uniform(0, 5, B)])
    m[:, 2] = np.maximum(m[:, 2], m[:, 1])
    m[5] = np.nan
    m[9] = np.nan
    m[11, 1] = m[11, 2] = np.inf
    edges = np.array([-0.2, 0.0, 0.125, 0.5])
    m[20, 1] = 0.125                                # equal to an edge: the upper bin
    m[21, 1] = 0.0
    status = r.choice([0, 1, -1, 2, -3, -13], B).astype(np.int32)
    tol = 1e-4
    s = audit.summarise(m, status, edges, tol)
    assert s.dtype == np.int64 and len(s) == 6 + 5 + 20 == audit.summary_len(4)
    want = np.zeros_like(s)
    for b in range(B):
        want[0] += 1
        if np.isnan(m[b]).any():
            want[1] += 1
            continue
        vok, cok = m[b, 0] <= tol, m[b, 1] >= 0
        want[2] += vok
        want[3] += cok
        want[4] += vok and cok
        want[5] += m[b, 1] < 0 <= m[b, 2]
        want[6 + sum(e <= m[b, 1] for e in edges)] += 1
        cls = {0: 0, 1: 1, -1: 2, 2: 3}.get(int(status[b]), 4)
        want[6 + 5 + cls * 4 + 2 * cok + vok] += 1
    assert np.array_equal(s, want)
    assert s[1] == 2 and s[6:11].sum() == B - 2 and s[11:].sum() == B - 2
    # additive over a split of the batch
    parts = sum(audit.summarise(m[a:b], status[a:b], edges, tol) for a, b in ((0, 1), (1, 64), (64, B)))
    assert np.array_equal(parts, s)
    # a value equal to an edge lands in the upper bin, +inf in the last
    one = audit.summarise(m[20:21], None, edges, tol)
    assert one[6 + 3] == 1 and one[6:11].sum() == 1
    assert audit.summarise(m[21:22], None, edges, tol)[6 + 2] == 1
    assert audit.summarise(m[11:12], None, edges, tol)[6 + 4] == 1
    assert not audit.summarise(m, None, edges, tol)[11:].any()          # no status: the cross table stays 0
    d = audit.describe(s, 4, edges)
    assert d["instances"] == B and d["nonfinite"] == 2 and d["clear_hist"] == [int(v) for v in s[6:11]]
    assert sum(sum(v.values()) for v in d["by_status"].values()) == B - 2
    with pytest.raises(ValueError):
        audit.describe(s, 3)


def test_audit_module_layout_names_and_no_oracle_import():
    src = open(audit.__file__).read()
    assert "import oracle" not in src and "from oracle" not in src
    assert audit.COLS == ("viol", "clear", "clear_knot", "goal_1", "goal_N")
    assert audit.WHERE == ("viol_row", "clear_row", "clear_obs") and len(audit.SUMMARY_FIELDS) == 6
