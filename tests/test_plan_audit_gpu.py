"""GPU: alipmpc_audit_batch (csrc/audit.inc) — the geometric columns against the numpy restatement (alipmpc.audit) and
against clearances recomputed from the handle's own alipmpc_trace_batch output, viol against the eval hook, the
summary as exact integers, batch / pointer-mode / handle independence, non-finite rows, and the error returns.

Shapes (the smallest with ragged 16-lane groups, lanes owning several rows, and the slot / horizon limits):
  B = 257 modi N = 3 nc = 5;  B = 67 modi N = 5 nc = 5 ne = 5;  B = 33 sig_step N = 3 nc = 6;  B = 5 N = 1 nc = 1;
  the limits as two handles, B = 19 each: N = 3 with 12 + 12 slots (ALIPMPC_MAX_OBS) and N = 6 with 3 + 3 slots
  (ALIPMPC_MAX_N) — one handle with N = 6 and 24 slots has 6 * 29 rows, above the 128 rows alipmpc_create accepts.
Plans: the first half of each batch are the handle's own solve outputs, the second half tile(x0) + 0.3 m seeded noise;
every other noisy instance has its first circle moved onto the start, so both clearance signs occur.

Bars.  Columns 1-4: 1e-11 — the trace agrees to 1e-12 (test_trace_batch_matches_plan_traces), the radial clearance is
Lipschitz in the position with constant <= the axis ratio <= 2 (the generator's ellipses), which leaves a x5 margin.
viol: 1e-12 max(1, |c|) of the violating row, the eval kernel's own bar against the reference goldens.

The file name sorts after test_dataset_gpu.py on purpose: test_loop_outputs_equal_existing_call there compares hd_traj
whole, including the entries the closed loop leaves unwritten after an episode's stop, so it passes only while no
earlier GPU test of the process has left anything in device memory."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {
    "modi_n3": dict(B=257, variant=0, N=3, nc=5, ne=0, seed=11),
    "modi_n5_mix": dict(B=67, variant=0, N=5, nc=5, ne=5, seed=12),
    "sig_n3": dict(B=33, variant=1, N=3, nc=6, ne=0, seed=13),
    "slots_24": dict(B=19, variant=0, N=3, nc=12, ne=12, seed=14),
    "horizon_6": dict(B=19, variant=0, N=6, nc=3, ne=3, seed=15),
    "n1": dict(B=5, variant=0, N=1, nc=1, ne=0, seed=16),
}
TOL = 1e-11
STATUS_FILL = np.array([0, 1, -1, 2, -3], np.int32)


def build_inputs(case):
    """Seeded inputs of a case: ragged nc / ne (instance 0 without obstacles) and, for every other instance of the
    noisy half, the first circle moved onto the start."""
    from alipmpc import scenes
    B, N, nc_max, ne_max = case["B"], case["N"], case["nc"], case["ne"]
    bt = scenes.make_batch(B, seed=case["seed"], n_cir=nc_max, n_elp=ne_max, N=N)
    r = np.random.default_rng(1000 + case["seed"])
    nc = bt["nc"].astype(np.int32).copy()
    ne = None if bt["ne"] is None else bt["ne"].astype(np.int32).copy()
    rag = np.arange(B) % 5 == 2
    nc[rag] = r.integers(0, nc_max + 1, rag.sum())
    if ne is not None:
        ne[rag] = r.integers(0, ne_max + 1, rag.sum())
        ne[0] = 0
    nc[0] = 0
    cir = bt["cir"].copy()
    half = B // 2
    planted = np.arange(B)[(np.arange(B) >= half) & ((np.arange(B) - half) % 2 == 0)]
    cir[planted, 0, 0:2] = bt["x0"][planted, 0:2] + [0.1, 0.0]
    nc[planted] = np.maximum(nc[planted], 1)
    noise = 0.3 * r.standard_normal((B, 5 * N))
    return dict(x0=bt["x0"], goal=bt["goal"], leg=bt["leg"].astype(np.int8), cir=cir, nc=nc, elp=bt["elp"], ne=ne,
                u0=bt["u0"]), noise, half


def plans_of(inp, noise, half, solved_u, solved_status):
    N = noise.shape[1] // 5
    u = np.array(solved_u, float)
    u[half:] = np.tile(inp["x0"][half:], (1, N)) + noise[half:]
    status = np.array(solved_status, np.int32)
    status[half:] = STATUS_FILL[np.arange(len(u) - half) % len(STATUS_FILL)]
    return u, status


def check_signs(ref_clear):
    """the condition on the inputs: both clearance signs occur in at least a tenth of the instances"""
    B = len(ref_clear)
    assert (ref_clear < 0).sum() >= 0.1 * B, ((ref_clear < 0).sum(), B)
    assert (ref_clear > 0).sum() >= 0.1 * B, ((ref_clear > 0).sum(), B)


def _args(inp):
    return inp["x0"], inp["goal"], inp["leg"], inp["cir"], inp["nc"], inp["elp"], inp["ne"]


_built = {}


@pytest.fixture(params=list(CASES))
def case(request, gpu_lib):
    """One shape, built once per session: inputs, plans, the device audit, the host restatement, the eval hook."""
    name = request.param
    if name not in _built:
        from alipmpc import audit
        c = CASES[name]
        cfg = gpu_lib.default_cfg(c["variant"], c["N"], nc_max=c["nc"], ne_max=c["ne"])
        s = gpu_lib.Solver(cfg)
        inp, noise, half = build_inputs(c)
        o = s.solve(*_args(inp), u0=inp["u0"])
        u, status = plans_of(inp, noise, half, o["u"], o["status"])
        ref = audit.audit_host(cfg, inp, u)
        check_signs(ref["metrics"][:, 1])
        out = s.audit(*_args(inp), u=u, status=status)
        _built[name] = dict(name=name, cfg=cfg, s=s, inp=inp, u=u, status=status, ref=ref, out=out)
    return _built[name]


def _same(a, b):
    """|a - b| with equal infinities counting as 0"""
    with np.errstate(invalid="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b))


def test_geometry_matches_host_and_own_trace(case, gpu_lib):
    from alipmpc import audit
    s, cfg, inp, u, out, ref = (case[k] for k in ("s", "cfg", "inp", "u", "out", "ref"))
    B, N = len(u), cfg.N
    m, w = out["metrics"], out["where"]
    err = _same(m[:, 1:5], ref["metrics"][:, 1:5])
    print(f"{case['name']}: max |device - audit_host| per column {err.max(0)}")
    assert err.max() <= TOL
    # the handle's own trace
    tr = s.trace(inp["x0"], u)
    rows = tr.shape[2]
    assert rows == gpu_lib.trace_len(cfg)
    tr = tr.reshape(B, N * rows, 2)
    knots = [k * rows for k in range(N)] + [N * rows - 1]
    none = (inp["nc"] == 0) & (True if inp["ne"] is None else inp["ne"] == 0)
    assert none.any()
    for b in range(B):
        obs, slots = audit.obstacle_list(cfg.nc_max, inp["cir"][b], inp["nc"][b],
                                         None if inp["elp"] is None else inp["elp"][b],
                                         None if inp["ne"] is None else inp["ne"][b])
        assert np.hypot(*(tr[b, knots[1]] - inp["goal"][b])) == pytest.approx(m[b, 3], abs=TOL)
        assert np.hypot(*(tr[b, knots[N]] - inp["goal"][b])) == pytest.approx(m[b, 4], abs=TOL)
        if none[b]:
            assert m[b, 1] == np.inf and m[b, 2] == np.inf and w[b, 1] == -1 and w[b, 2] == -1
            continue
        assert np.isfinite(m[b, 1]) and w[b, 2] >= 0
        cl = audit.radial_clearance(tr[b][:, None, :], obs[None])
        assert abs(cl.min() - m[b, 1]) <= TOL and abs(cl[knots].min() - m[b, 2]) <= TOL
        # where: the host clearance at the device's (row, obs) is the host minimum (no near-tie exclusions)
        j = int(np.nonzero(slots == w[b, 2])[0][0])
        assert 0 <= w[b, 1] < N * rows
        assert abs(cl[w[b, 1], j] - cl.min()) <= TOL
        href = audit.radial_clearance(ref["trace"][b][:, None, :], obs[None])
        assert abs(href[w[b, 1], j] - ref["metrics"][b, 1]) <= TOL
        assert w[b, 1] % rows != 1      # rows 0 and 1 of a step are bit-equal: the tie goes to row 0
    assert (m[:, 2] >= m[:, 1]).all()


def test_viol_matches_eval(case):
    s, inp, u, out = (case[k] for k in ("s", "inp", "u", "out"))
    ev = s.eval(*_args(inp), u=u, want_J=False)
    act = ev["row_active"] != 0
    with np.errstate(invalid="ignore"):
        v = np.where(act, np.maximum(np.maximum(ev["cl"] - ev["c"], ev["c"] - ev["cu"]), 0.0), 0.0)
    want, row = v.max(1), v.argmax(1)
    viol, vrow = out["metrics"][:, 0], out["where"][:, 0]
    assert np.array_equal(viol == 0, want == 0)
    assert np.array_equal(vrow == -1, want == 0)
    assert (want > 0).any()
    hit = want > 0
    idx = np.nonzero(hit)[0]
    scale = np.maximum(1.0, np.abs(ev["c"][idx, row[idx]]))
    print(f"{case['name']}: viol bit-equal on {(viol[hit] == want[hit]).sum()} of {hit.sum()} violating instances, "
          f"rows equal on {(vrow[hit] == row[hit]).sum()}, max |d| {np.abs(viol[hit] - want[hit]).max():.3e}")
    assert (np.abs(viol[hit] - want[hit]) <= 1e-12 * scale).all()
    assert (vrow[hit] >= 0).all() and act[idx, vrow[idx]].all()
    assert (np.abs(v[idx, vrow[idx]] - want[hit]) <= 1e-12 * scale).all()


def test_summary_exact_accumulating_and_edges_on_values(case, gpu_lib):
    import torch
    from alipmpc import audit
    s, inp, u, status, out = (case[k] for k in ("s", "inp", "u", "status", "out"))
    B = len(u)
    clear = out["metrics"][:, 1]
    fin = np.unique(clear[np.isfinite(clear)])
    picked = fin[[0, len(fin) // 2, len(fin) - 1]] if len(fin) >= 3 else fin
    edges = np.unique(np.concatenate([picked, [-0.25, 0.0, 1.0]]))     # some clear values are bit-equal to an edge
    tol = 1e-4
    n = gpu_lib.audit_summary_len(len(edges))
    assert n == 6 + len(edges) + 1 + 20
    got = s.audit(*_args(inp), u=u, status=status, edges=edges, viol_tol=tol)
    assert np.array_equal(got["metrics"], out["metrics"], equal_nan=True) and np.array_equal(got["where"], out["where"])
    want = audit.summarise(got["metrics"], status, edges, tol)
    assert got["summary"].dtype == np.int64 and np.array_equal(got["summary"], want)
    assert want[0] == B and want[1] == 0 and want[6:6 + len(edges) + 1].sum() == B and want[-20:].sum() == B
    for e in picked:                                                    # equal to an edge: the upper bin
        i = int(np.nonzero(edges == e)[0][0])
        assert audit.summarise(got["metrics"][clear == e], None, edges, tol)[6 + i + 1] == (clear == e).sum()
    # a pre-filled buffer is added to; status = NULL leaves the cross table at its sentinel (host and device pointers)
    pre = np.arange(n, dtype=np.int64) * 7 + 1000
    nost = audit.summarise(got["metrics"], None, edges, tol)
    host = s.audit(*_args(inp), u=u, edges=edges, viol_tol=tol, summary=pre.copy())
    assert np.array_equal(host["summary"], pre + nost) and np.array_equal(host["summary"][-20:], pre[-20:])
    dev = torch.device("cuda", 0)
    dinp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items() if v is not None}
    dinp["u"] = torch.from_numpy(u).to(dev)
    dsum = torch.from_numpy(pre.copy()).to(dev)
    s.audit_device(dinp, dict(summary=dsum), edges=edges, viol_tol=tol)
    dinp["status"] = torch.from_numpy(status).to(dev)
    s.audit_device(dinp, dict(summary=dsum), edges=edges, viol_tol=tol)
    torch.cuda.synchronize()
    assert np.array_equal(dsum.cpu().numpy(), pre + nost + want)


@pytest.fixture(scope="module")
def batch300(gpu_lib):
    c = dict(B=300, variant=0, N=3, nc=5, ne=0, seed=21)
    cfg = gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0)
    s = gpu_lib.Solver(cfg)
    inp, noise, half = build_inputs(c)
    o = s.solve(*_args(inp), u0=inp["u0"])
    u, status = plans_of(inp, noise, half, o["u"], o["status"])
    edges = np.array([-0.5, -0.1, 0.0, 0.05, 0.2, 0.6])
    return dict(cfg=cfg, s=s, inp=inp, u=u, status=status, edges=edges,
                whole=s.audit(*_args(inp), u=u, status=status, edges=edges))


def _cut(inp, lo, hi):
    return {k: (None if v is None else v[lo:hi]) for k, v in inp.items()}


def test_batch_independence_chunks_pointer_modes_and_handles(batch300, gpu_lib):
    import torch
    s, inp, u, status, edges, whole = (batch300[k] for k in ("s", "inp", "u", "status", "edges", "whole"))
    B = len(u)
    # chunks of 1 / 63 / 236: the same bits, and the accumulated summary is the whole batch's
    acc = np.zeros_like(whole["summary"])
    lo = 0
    for n in (1, 63, 236):
        part = s.audit(*_args(_cut(inp, lo, lo + n)), u=u[lo:lo + n], status=status[lo:lo + n], edges=edges, summary=acc)
        assert np.array_equal(part["metrics"], whole["metrics"][lo:lo + n], equal_nan=True)
        assert np.array_equal(part["where"], whole["where"][lo:lo + n])
        acc = part["summary"]
        lo += n
    assert lo == B and np.array_equal(acc, whole["summary"])
    # device pointers
    dev = torch.device("cuda", 0)
    dinp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items() if v is not None}
    dinp["u"], dinp["status"] = torch.from_numpy(u).to(dev), torch.from_numpy(status).to(dev)
    dout = dict(metrics=torch.full((B, 5), -7.0, dtype=torch.float64, device=dev),
                where=torch.full((B, 3), -7, dtype=torch.int32, device=dev),
                summary=torch.zeros(len(whole["summary"]), dtype=torch.int64, device=dev))
    s.audit_device(dinp, dout, edges=edges)
    torch.cuda.synchronize()
    assert np.array_equal(dout["metrics"].cpu().numpy(), whole["metrics"], equal_nan=True)
    assert np.array_equal(dout["where"].cpu().numpy(), whole["where"])
    assert np.array_equal(dout["summary"].cpu().numpy(), whole["summary"])
    # a lane / fp32 handle of the same shape audits with the same bits (the audit arithmetic is always fp64)
    lane = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0, precision=gpu_lib.PREC_FP32,
                                              program=gpu_lib.PROGRAM_LANE))
    assert lane.solve_program().startswith("lane_kernel")
    other = lane.audit(*_args(inp), u=u, status=status, edges=edges)
    for k in ("metrics", "where", "summary"):
        assert np.array_equal(other[k], whole[k], equal_nan=True), k
    own = lane.solve(*_args(inp), u0=inp["u0"])
    mine = lane.audit(*_args(inp), u=own["u"], status=own["status"])
    assert mine["summary"][0] == B and mine["summary"][1] == 0


def test_non_finite_rows(batch300):
    s, inp, u, status, edges, whole = (batch300[k] for k in ("s", "inp", "u", "status", "edges", "whole"))
    B = len(u)
    bad = [0, B // 2 + 1, B - 1]
    x0, goal, ub = inp["x0"].copy(), inp["goal"].copy(), u.copy()
    x0[bad[0], 3] = np.nan
    ub[bad[1], 7] = np.inf
    goal[bad[2], 1] = -np.inf
    got = s.audit(x0, goal, inp["leg"], inp["cir"], inp["nc"], inp["elp"], inp["ne"], u=ub, status=status, edges=edges)
    ok = np.ones(B, bool)
    ok[bad] = False
    assert np.isnan(got["metrics"][bad]).all() and (got["where"][bad] == -1).all()
    assert np.array_equal(got["metrics"][ok], whole["metrics"][ok]) and np.array_equal(got["where"][ok], whole["where"][ok])
    assert got["summary"][0] == B and got["summary"][1] == 3
    from alipmpc import audit
    assert np.array_equal(got["summary"], audit.summarise(got["metrics"], status, edges, 1e-4))
    assert got["summary"][6:6 + len(edges) + 1].sum() == B - 3 and got["summary"][-20:].sum() == B - 3


def test_errors(batch300, gpu_lib):
    s, inp, u = batch300["s"], batch300["inp"], batch300["u"]
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        dd = gpu_lib.Solver(gpu_lib.default_cfg(gpu_lib.VARIANT_DD, 3, nc_max=5, ne_max=0))
        dd.audit(inp["x0"][:4, :3], inp["goal"][:4], None, inp["cir"][:4], inp["nc"][:4], u=np.zeros((4, 6)))
    a = _args(_cut(inp, 0, 8))
    for kw in (dict(edges=np.linspace(0, 1, 63)), dict(edges=[0.0, 0.0]), dict(edges=[0.2, 0.1]),
               dict(edges=[0.0, np.nan]), dict(edges=[np.inf]), dict(viol_tol=-1e-9), dict(viol_tol=np.nan),
               dict(viol_tol=np.inf), dict(u=None)):
        kw.setdefault("u", u[:8])
        with pytest.raises(RuntimeError, match="EINVAL"):
            s.audit(*a, **kw)
    with pytest.raises(ValueError):
        gpu_lib.audit_summary_len(63)
    assert gpu_lib.audit_summary_len(0) == 27 and gpu_lib.audit_summary_len(62) == 89
    # through the C ABI: B < 0 and all three outputs NULL
    from alipmpc._lib import _ptr
    L, P = s._L, [_ptr(np.ascontiguousarray(v)) for v in a[:5]]
    m = np.zeros((8, 5))
    uu = np.ascontiguousarray(u[:8])

    def raw(B, metrics):
        return L.alipmpc_audit_batch(s._h, B, *P, None, None, _ptr(uu), None, metrics, None, 1e-4, None, 0, None, None)

    assert raw(-1, _ptr(m)) == -1 and raw(8, None) == -1
    assert raw(0, _ptr(m)) == 0 and raw(8, _ptr(m)) == 0
    assert np.array_equal(m, batch300["whole"]["metrics"][:8], equal_nan=True)
