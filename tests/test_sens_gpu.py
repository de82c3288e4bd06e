"""Plan sensitivities (alipmpc_solve_sens_batch) on the device.

1 / 2: the analytic dfoot / du against central differences of the C oracle's solves (tol 1e-10, max_iter 300, h = 1e-5,
every perturbed solve warm-started from the oracle's base u), with and without the detour.  The referee is the oracle's
own sensitivity to its termination tolerance: S_ref is the share of kept instances whose finite differences at tol 1e-8
stay within 1e-3 max(1, max |D|) of those at tol 1e-10, m_ref the median of that error; the GPU, which stops at tol 1e-8
and carries no finite-difference noise, must reach S_ref - 0.02 (two or three instances of a kept batch) and a median of
at most max(10 m_ref, 1e-7) (the factor 10 is the spread of m_ref across the shapes).
3: the solve inside solve_sens is the handle's solve, bit for bit.  4: invalid instances.  5: refusals.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 1e-5
# name: variant, N, circles, ellipses, seed, B, least share of the batch the filter must keep
SHAPES = {
    "modi_n3_c5": (0, 3, 5, 0, 11, 128, 0.70),
    "sig_step_n3_c4": (1, 3, 4, 0, 12, 128, 0.70),
    "modi_n3_c3e2": (0, 3, 3, 2, 13, 128, 0.70),
    "modi_n5_c3e2": (0, 5, 3, 2, 14, 64, 0.40),
}
_FD = {}      # (shape, detour) -> the oracle's reference, computed once
_GPU = {}     # (shape, detour) -> the GPU's solve_sens


def _batch(name):
    from alipmpc import scenes
    variant, N, nci, nel, seed, B, _ = SHAPES[name]
    return scenes.make_batch(B, seed=seed, n_cir=nci, n_elp=nel, N=N)


def _artifact(name, obj):
    d = os.environ.get("ALIPMPC_TEST_ARTIFACTS")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as fh:
            json.dump(obj, fh, indent=1)


def _osolve(coracle, cfg, bt, x0, goal, u0):
    o = coracle.solve_batch(cfg, x0, goal, bt["leg"], bt["cir"], bt["nc"], bt.get("elp"), bt.get("ne"), u0, nthreads=8)
    # the plan as the GPU returns it: the canonical u_k = x_{k+1}
    return o["foot"], o["x_pred"].reshape(len(x0), -1), o["status"]


def _oracle_fd(coracle, name, detour, tol):
    """(base u, dfoot (B,3,7), du (B,5N,7), every one of the 15 solves ended with status 0) by central differences"""
    variant, N, nci, nel, seed, B, _ = SHAPES[name]
    bt = _batch(name)
    cfg = coracle.default_cfg(variant, N, nc_max=nci, ne_max=nel, tol=tol, max_iter=300, detour=detour)
    _, ub, st = _osolve(coracle, cfg, bt, bt["x0"], bt["goal"], bt["u0"])
    ok = st == 0
    dfoot, du = np.zeros((B, 3, 7)), np.zeros((B, 5 * N, 7))
    for c in range(7):
        res = []
        for sgn in (1.0, -1.0):
            x0, goal = bt["x0"].copy(), bt["goal"].copy()
            if c < 5:
                x0[:, c] += sgn * H
            else:
                goal[:, c - 5] += sgn * H
            f, u, st = _osolve(coracle, cfg, bt, x0, goal, ub)
            ok &= st == 0
            res.append((f, u))
        dfoot[:, :, c] = (res[0][0] - res[1][0]) / (2 * H)
        du[:, :, c] = (res[0][1] - res[1][1]) / (2 * H)
    return ub, dfoot, du, ok


def _reference(coracle, name, detour):
    key = (name, detour)
    if key not in _FD:
        ub, df10, du10, ok = _oracle_fd(coracle, name, detour, 1e-10)
        _, df8, du8, _ = _oracle_fd(coracle, name, detour, 1e-8)
        _FD[key] = dict(u=ub, dfoot=df10, du=du10, ok=ok, dfoot8=df8, du8=du8)
        for v in _FD[key].values():
            v.setflags(write=False)
    return _FD[key]


def _gpu(gpu_lib, name, detour):
    key = (name, detour)
    if key not in _GPU:
        variant, N, nci, nel, seed, B, _ = SHAPES[name]
        bt = _batch(name)
        s = gpu_lib.Solver(gpu_lib.default_cfg(variant, N, nc_max=nci, ne_max=nel, max_iter=100, detour=detour))
        _GPU[key] = s.solve_sens(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt.get("elp"), bt.get("ne"),
                                 u0=bt["u0"])
    return _GPU[key]


def _err(D, Dref):
    """per instance: max |D - Dref| / max(1, max |Dref|); a non-finite D counts as infinitely far"""
    B = len(D)
    e = np.abs(D - Dref).reshape(B, -1).max(axis=1) / np.maximum(1.0, np.abs(Dref).reshape(B, -1).max(axis=1))
    return np.where(np.isfinite(e), e, np.inf)


def _bars(tag, o, ref, keep, record):
    """the GPU's dfoot and du against the tol-1e-10 finite differences on the instances `keep`"""
    for q in ("dfoot", "du"):
        e_ref = _err(ref[q + "8"], ref[q])[keep]
        e_gpu = _err(o[q], ref[q])[keep]
        S_ref, m_ref = float(np.mean(e_ref <= 1e-3)), float(np.median(e_ref))
        S, m = float(np.mean(e_gpu <= 1e-3)), float(np.median(e_gpu))
        record[f"{tag}/{q}"] = dict(kept=int(keep.sum()), S_ref=S_ref, m_ref=m_ref, share=S, median=m)
        print(f"{tag} {q}: kept {int(keep.sum())}  S_ref {S_ref:.4f} m_ref {m_ref:.3e}  GPU share {S:.4f} median {m:.3e}")
    for q in ("dfoot", "du"):
        r = record[f"{tag}/{q}"]
        assert r["share"] >= r["S_ref"] - 0.02, (tag, q, r)
        assert r["median"] <= max(10 * r["m_ref"], 1e-7), (tag, q, r)


def _kept(o, ref):
    same = np.abs(o["u"] - ref["u"]).max(axis=1) <= 1e-6
    return ref["ok"] & (o["status"] == 0) & same


@pytest.mark.parametrize("name", list(SHAPES))
def test_sens_matches_oracle_finite_differences(gpu_lib, coracle, name):
    ref = _reference(coracle, name, 1)
    o = _gpu(gpu_lib, name, 1)
    keep = _kept(o, ref)
    record = {}
    print(f"{name}: kept {keep.mean():.3f} of {len(keep)} (oracle alone {ref['ok'].mean():.3f})")
    assert keep.mean() >= SHAPES[name][6], keep.mean()
    assert np.all(o["sens_ok"][keep] == 1)
    _bars(name, o, ref, keep, record)
    _artifact(f"sens_parity_{name}.json", record)


def test_sens_detour_chain(gpu_lib, coracle):
    """The modi 5-circle case with the detour off on both sides (no chain rule at all), and, with it on, the kept
    instances whose detour fired on their own: their goal columns carry Rot, their position columns I - Rot."""
    name = "modi_n3_c5"
    record = {}
    ref0, o0 = _reference(coracle, name, 0), _gpu(gpu_lib, name, 0)
    keep0 = _kept(o0, ref0)
    assert keep0.mean() >= SHAPES[name][6], keep0.mean()
    _bars(name + "/detour_off", o0, ref0, keep0, record)
    ref1, o1 = _reference(coracle, name, 1), _gpu(gpu_lib, name, 1)
    bt = _batch(name)
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0))
    ge = s.eval(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u=bt["u0"], want_J=False)["goal_eff"]
    fired = np.any(ge != bt["goal"], axis=1)
    sub = _kept(o1, ref1) & fired
    print(f"detour fired on {int(fired.sum())} instances, {int(sub.sum())} of them kept")
    assert sub.sum() >= 1
    _bars(name + "/detour_fired", o1, ref1, sub, record)
    _artifact("sens_parity_detour.json", record)


SOLVE_KEYS = ("u", "foot", "x_pred", "status", "iters")


def _same_solve(a, b):
    for k in SOLVE_KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_sens_solve_is_the_solve(gpu_lib):
    """u, foot, x_pred, status and iters of solve_sens equal solve on the same handle bit for bit: B = 1, B = 5 (not a
    multiple of a workgroup's 4 instances), B = 300 whole and in chunks of 64 plus the remainder, and device pointers
    with NaN-prefilled outputs (every element written)."""
    import torch
    from alipmpc import scenes
    Bt = 300
    bt = scenes.make_batch(Bt, seed=31, n_cir=5)
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, nc_max=5, ne_max=0))
    args = lambda a, b: (bt["x0"][a:b], bt["goal"][a:b], bt["leg"][a:b], bt["cir"][a:b], bt["nc"][a:b])
    whole = s.solve(*args(0, Bt), u0=bt["u0"])
    assert len(np.unique(whole["status"])) >= 2   # (not only converged instances)
    for B in (1, 5, Bt):
        o = s.solve_sens(*args(0, B), u0=bt["u0"][:B])
        _same_solve(o, s.solve(*args(0, B), u0=bt["u0"][:B]))
        _same_solve(o, {k: whole[k][:B] for k in SOLVE_KEYS})
    sens = s.solve_sens(*args(0, Bt), u0=bt["u0"])
    for a in range(0, Bt, 64):
        b = min(a + 64, Bt)
        o = s.solve_sens(*args(a, b), u0=bt["u0"][a:b])
        _same_solve(o, {k: whole[k][a:b] for k in SOLVE_KEYS})
        for k in ("dfoot", "du", "sens_ok"):
            assert np.array_equal(o[k], sens[k][a:b], equal_nan=True), k
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=dev)
    out = dict(u=nan(Bt, 15), foot=nan(Bt, 3), x_pred=nan(Bt, 3, 5), dfoot=nan(Bt, 3, 7), du=nan(Bt, 15, 7),
               status=torch.full((Bt,), -77, dtype=torch.int32, device=dev),
               iters=torch.full((Bt,), -77, dtype=torch.int32, device=dev),
               sens_ok=torch.full((Bt,), -77, dtype=torch.int32, device=dev))
    s.solve_sens_device(inp, out)
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in out.items()}
    _same_solve(d, whole)
    assert np.all(np.isin(d["sens_ok"], (0, 1)))
    for k in ("dfoot", "du", "sens_ok"):
        assert np.array_equal(d[k], sens[k], equal_nan=True), k
    assert np.isfinite(d["dfoot"][d["sens_ok"] == 1]).all() and np.isfinite(d["du"][d["sens_ok"] == 1]).all()
    # du may be left out
    o = s.solve_sens(*args(0, 5), u0=bt["u0"][:5], want_du=False)
    assert o["du"] is None and np.array_equal(o["dfoot"], sens["dfoot"][:5], equal_nan=True)


def test_sens_invalid_instances(gpu_lib):
    """Infeasible scenes (a CoM velocity no leg of 0.3 m can bring into the body-velocity bounds: status 2) and solves
    that stop at the iteration cap get sens_ok = 0 and NaN in every derivative, exactly those; every other instance is
    finite with sens_ok = 1.  B = 0 returns OK and touches nothing."""
    from alipmpc import scenes
    B = 64
    bt = scenes.make_batch(B, seed=33, n_cir=5)
    x0, u0 = bt["x0"].copy(), bt["u0"].copy()
    x0[::4, 2:4] = [3.0, 3.0]
    u0[::4] = np.tile(x0[::4], (1, 3))
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, nc_max=5, ne_max=0))
    o = s.solve_sens(x0, bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=u0)
    assert np.all(o["status"][::4] == 2)
    bad = ~np.isin(o["status"], (0, 1))
    assert bad.sum() >= B // 4 and (~bad).sum() >= B // 4
    assert np.array_equal(o["sens_ok"], (~bad).astype(np.int32))
    assert np.isnan(o["dfoot"][bad]).all() and np.isnan(o["du"][bad]).all()
    assert np.isfinite(o["dfoot"][~bad]).all() and np.isfinite(o["du"][~bad]).all()
    from alipmpc._lib import _ptr
    sent = np.full((2, 3, 7), 5.0)
    rc = s._L.alipmpc_solve_sens_batch(s._h, 0, *([None] * 9), None, None, None, None, None, _ptr(sent), None, None, None)
    assert rc == 0 and np.all(sent == 5.0)


def test_sens_refusals(gpu_lib):
    """fp32, lane-program, DD and N = 6 handles refuse the new entry point with EUNSUPPORTED and still solve."""
    from alipmpc import scenes
    bt = scenes.make_batch(8, seed=35, n_cir=5)
    a = (bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"])
    for kw in (dict(precision=gpu_lib.PREC_FP32), dict(program=gpu_lib.PROGRAM_LANE)):
        s = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0, **kw))
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            s.solve_sens(*a, u0=bt["u0"])
        assert np.isfinite(s.solve(*a, u0=bt["u0"])["u"]).all()
    b6 = scenes.make_batch(8, seed=36, n_cir=3, N=6)
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, 6, nc_max=3, ne_max=0))
    a6 = (b6["x0"], b6["goal"], b6["leg"], b6["cir"], b6["nc"])
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        s.solve_sens(*a6, u0=b6["u0"])
    assert np.isfinite(s.solve(*a6, u0=b6["u0"])["u"]).all()
    s = gpu_lib.Solver(gpu_lib.default_cfg(2, 3, nc_max=5, ne_max=0))
    xd = np.stack([bt["x0"][:, 0], bt["x0"][:, 1], bt["x0"][:, 4]], 1)
    lu = np.tile([0.6, 0.0], (8, 1))
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        s.solve_sens(xd, bt["goal"], None, bt["cir"], bt["nc"], u0=np.tile(lu, (1, 3)))
    assert np.isfinite(s.solve(xd, bt["goal"], None, bt["cir"], bt["nc"], u0=np.tile(lu, (1, 3)), last_u=lu)["u"]).all()
