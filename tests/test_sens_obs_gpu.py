"""Obstacle sensitivities (alipmpc_solve_sens_obs_batch) on the device.

1: dfoot_obs / du_obs against central differences of the C oracle's solves (sens_obs_ref.py: tol 1e-10, h = 1e-5) on
scenes with an obstacle in the way (scenes.block_path), detour on and off, on the active instances (the reference's
max |du_obs| >= 0.05) where the GPU (max_iter 100, default tol) also ends with status 0 and its plan agrees with the
oracle's to 1e-6.  The bars are test_sens_gpu.py's rule on the obstacle columns: the share of instances within 1e-3
max(1, max |D|) reaches S_ref - 0.02 and the median error stays below max(10 m_ref, 1e-7), S_ref and m_ref being the
oracle's own finite differences at tol 1e-8 against those at tol 1e-10 on the same instances and columns.
2: the translation identity (sens_obs_ref.translation_residual) on the same instances: the GPU's median residual is at
most the reference's, and its share of instances with a residual <= 1e-6 at least the reference's - 0.02.  It needs no
oracle tolerance and pins sign and scale of the new columns against du's.
3: bits (the solve is solve's, dfoot / du / sens_ok are solve_sens', the obstacle columns do not depend on B, chunking
or the pointer mode).  4: exact zeros and NaN.  5: refusals.
"""
import json
import os

import numpy as np
import pytest

import sens_obs_ref as R

pytestmark = pytest.mark.gpu

# least instances left after the GPU's filter (all, ellipse-active)
LEAST = {"modi_n3_c5": (35, None), "sig_step_n3_c4": (60, None), "modi_n3_c3e2": (35, 18), "modi_n5_c3e2": (25, 8)}
_GPU = {}
_RECORD = {}


def _artifact(name, obj):
    d = os.environ.get("ALIPMPC_TEST_ARTIFACTS")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as fh:
            json.dump(obj, fh, indent=1)


def _scene(bt, a=None, b=None):
    return tuple(None if bt.get(k) is None else bt[k][a:b] for k in ("x0", "goal", "leg", "cir", "nc", "elp", "ne"))


def _gpu(gpu_lib, name, detour):
    key = (name, detour)
    if key not in _GPU:
        variant, N, nci, nel = R.SHAPES[name][:4]
        bt = R.batch(name)
        s = gpu_lib.Solver(gpu_lib.default_cfg(variant, N, nc_max=nci, ne_max=nel, max_iter=100, detour=detour))
        _GPU[key] = s.solve_sens_obs(*_scene(bt), u0=bt["u0"])
    return _GPU[key]


def _err(D, Dref):
    """per instance: max |D - Dref| / max(1, max |Dref|); a non-finite D counts as infinitely far (test_sens_gpu.py's)"""
    B = len(D)
    e = np.abs(D - Dref).reshape(B, -1).max(axis=1) / np.maximum(1.0, np.abs(Dref).reshape(B, -1).max(axis=1))
    return np.where(np.isfinite(e), e, np.inf)


def _bars(tag, o, ref, ref8, keep, cols, record):
    """the GPU's obstacle columns `cols` against the tol-1e-10 finite differences on the instances `keep`"""
    for q in ("dfoot", "du"):
        D10, D8 = ref[q][:, :, 7:][:, :, cols], ref8[q][:, :, 7:][:, :, cols]
        e_ref = _err(D8, D10)[keep]
        e_gpu = _err(o[q + "_obs"][:, :, cols], D10)[keep]
        S_ref, m_ref = float(np.mean(e_ref <= 1e-3)), float(np.median(e_ref))
        S, m = float(np.mean(e_gpu <= 1e-3)), float(np.median(e_gpu))
        record[f"{tag}/{q}_obs"] = dict(kept=int(keep.sum()), S_ref=S_ref, m_ref=m_ref, share=S, median=m)
        print(f"{tag} {q}_obs: kept {int(keep.sum())}  S_ref {S_ref:.4f} m_ref {m_ref:.3e}  GPU share {S:.4f} "
              f"median {m:.3e}")
    for q in ("dfoot", "du"):
        r = record[f"{tag}/{q}_obs"]
        assert r["share"] >= r["S_ref"] - 0.02, (tag, q, r)
        assert r["median"] <= max(10 * r["m_ref"], 1e-7), (tag, q, r)


def _instances(gpu_lib, coracle, name, detour):
    """(reference at tol 1e-10, at tol 1e-8, the GPU's outputs, the active instances the GPU's filter keeps, the
    ellipse-active ones among them)"""
    ref, ref8 = R.oracle_fd(coracle, name, detour, 1e-10), R.oracle_fd(coracle, name, detour, 1e-8)
    o = _gpu(gpu_lib, name, detour)
    _, active, elp_active = R.subsets(name, ref)
    same = (o["status"] == 0) & (np.abs(o["u"] - ref["u"]).max(axis=1) <= 1e-6)
    return ref, ref8, o, active & same, elp_active & same


PARAMS = [(n, d) for n in R.SHAPES for d in (1, 0)]


@pytest.mark.parametrize("name, detour", PARAMS)
def test_sens_obs_matches_oracle_finite_differences(gpu_lib, coracle, name, detour):
    ref, ref8, o, keep, keep_e = _instances(gpu_lib, coracle, name, detour)
    tag = f"{name}/detour_{'on' if detour else 'off'}"
    nci, nel = R.SHAPES[name][2:4]
    least, least_e = LEAST[name]
    print(f"{tag}: {int(keep.sum())} active instances kept ({int(keep_e.sum())} ellipse-active)")
    assert keep.sum() >= least, keep.sum()
    assert np.all(o["sens_ok"][keep] == 1)
    record = {}
    _bars(tag, o, ref, ref8, keep, np.arange(3 * nci + 5 * nel), record)
    if least_e is not None:
        assert keep_e.sum() >= least_e, keep_e.sum()
        _bars(tag + "/ellipse", o, ref, ref8, keep_e, np.arange(3 * nci, 3 * nci + 5 * nel), record)
    _RECORD.update(record)
    _artifact("sens_obs_parity.json", _RECORD)


@pytest.mark.parametrize("name, detour", PARAMS)
def test_sens_obs_translation_identity(gpu_lib, coracle, name, detour):
    ref, _, o, keep, _ = _instances(gpu_lib, coracle, name, detour)
    assert keep.sum() >= LEAST[name][0], keep.sum()
    r_ref = R.translation_residual(name, ref["dfoot"][:, :, :7], ref["du"][:, :, :7], ref["dfoot"][:, :, 7:],
                                   ref["du"][:, :, 7:])[keep]
    r_gpu = R.translation_residual(name, o["dfoot"], o["du"], o["dfoot_obs"], o["du_obs"])[keep]
    r_without = R.translation_residual(name, o["dfoot"], o["du"], None, None)[keep]
    print(f"{name} detour {detour}: translation residual median GPU {np.median(r_gpu):.3e} reference "
          f"{np.median(r_ref):.3e} (GPU without the obstacle columns {np.median(r_without):.3g}); share <= 1e-6: GPU "
          f"{np.mean(r_gpu <= 1e-6):.4f} reference {np.mean(r_ref <= 1e-6):.4f}")
    assert np.median(r_gpu) <= np.median(r_ref)
    assert np.mean(r_gpu <= 1e-6) >= np.mean(r_ref <= 1e-6) - 0.02


SOLVE_KEYS = ("u", "foot", "x_pred", "status", "iters")
SENS_KEYS = ("dfoot", "du", "sens_ok")
OBS_KEYS = ("dfoot_obs", "du_obs")


def _same(a, b, keys, sl=slice(None)):
    for k in keys:
        assert np.array_equal(a[k], b[k][sl], equal_nan=True), k


@pytest.mark.parametrize("name", ["modi_n3_c5", "modi_n3_c3e2"])
def test_sens_obs_bits(gpu_lib, name):
    """B = 1, 5 and 300, whole and in chunks of 64 plus the remainder, host and device pointers (NaN-prefilled outputs:
    every element is written)."""
    import torch
    from alipmpc import scenes
    variant, N, nci, nel, seed = R.SHAPES[name][:5]
    Bt, P = 300, 3 * nci + 5 * nel
    bt = scenes.block_path(scenes.make_batch(Bt, seed=seed + 20, n_cir=nci, n_elp=nel, N=N), seed + 20)
    s = gpu_lib.Solver(gpu_lib.default_cfg(variant, N, nc_max=nci, ne_max=nel))
    assert s.sens_obs_cols == P
    whole = s.solve(*_scene(bt), u0=bt["u0"])
    sens = s.solve_sens(*_scene(bt), u0=bt["u0"])
    obs = s.solve_sens_obs(*_scene(bt), u0=bt["u0"])
    assert len(np.unique(whole["status"])) >= 2   # (not only converged instances)
    _same(obs, whole, SOLVE_KEYS)
    _same(obs, sens, SENS_KEYS)
    assert obs["dfoot_obs"].shape == (Bt, 3, P) and obs["du_obs"].shape == (Bt, 5 * N, P)
    ok = obs["sens_ok"] == 1
    assert np.isfinite(obs["dfoot_obs"][ok]).all() and np.isfinite(obs["du_obs"][ok]).all()
    assert np.abs(obs["du_obs"][ok]).max() > 0.05
    for B in (1, 5):
        o = s.solve_sens_obs(*_scene(bt, 0, B), u0=bt["u0"][:B])
        _same(o, s.solve(*_scene(bt, 0, B), u0=bt["u0"][:B]), SOLVE_KEYS)
        _same(o, s.solve_sens(*_scene(bt, 0, B), u0=bt["u0"][:B]), SENS_KEYS)
        _same(o, obs, SOLVE_KEYS + SENS_KEYS + OBS_KEYS, slice(0, B))
    for a in range(0, Bt, 64):
        b = min(a + 64, Bt)
        _same(s.solve_sens_obs(*_scene(bt, a, b), u0=bt["u0"][a:b]), obs, SOLVE_KEYS + SENS_KEYS + OBS_KEYS, slice(a, b))
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda: torch.full((Bt,), -77, dtype=torch.int32, device=dev)               # noqa: E731
    out = dict(u=nan(Bt, 5 * N), foot=nan(Bt, 3), x_pred=nan(Bt, N, 5), dfoot=nan(Bt, 3, 7), du=nan(Bt, 5 * N, 7),
               status=i32(), iters=i32(), sens_ok=i32(), dfoot_obs=nan(Bt, 3, P), du_obs=nan(Bt, 5 * N, P))
    s.solve_sens_obs_device(inp, out)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in out.items()}, obs, SOLVE_KEYS + SENS_KEYS + OBS_KEYS)
    # the state columns and du_obs may be left out, in either mode
    o = s.solve_sens_obs(*_scene(bt, 0, 5), u0=bt["u0"][:5], want_du=False, want_state=False)
    assert o["du_obs"] is None and o["dfoot"] is None and o["du"] is None and o["sens_ok"] is None
    _same(o, obs, SOLVE_KEYS + ("dfoot_obs",), slice(0, 5))
    out2 = dict(u=nan(Bt, 5 * N), dfoot_obs=nan(Bt, 3, P))
    s.solve_sens_obs_device(inp, out2)
    torch.cuda.synchronize()
    _same({k: v.cpu().numpy() for k, v in out2.items()}, obs, ("u", "dfoot_obs"))


@pytest.mark.parametrize("variant", [0, 1])
def test_sens_obs_zero_and_nan_columns(gpu_lib, variant):
    """Ragged nc / ne and, for modi, obstacles clearly outside the detection range (h > detect_r2 + 1e-6): the columns
    of a slot at or above the count, or one select_obs dropped, are exactly 0.0 in both outputs; an invalid instance
    (some forced with max_iter = 3) is NaN throughout."""
    from alipmpc import scenes
    B, N, nci, nel = 300, 3, 3, 2
    bt = scenes.block_path(scenes.make_batch(B, seed=41, n_cir=nci, n_elp=nel, N=N), 41)
    nc, ne = (np.arange(B) % (nci + 1)).astype(np.int32), ((np.arange(B) // 4) % (nel + 1)).astype(np.int32)
    # garbage beyond the counts: it must not be read
    for b in range(B):
        bt["cir"][b, nc[b]:] = [1e3, -1e3, 7.0]
        bt["elp"][b, ne[b]:] = [1e3, -1e3, 7.0, 3.0, 0.5]
    cfg = gpu_lib.default_cfg(variant, N, nc_max=nci, ne_max=nel)
    pos = bt["x0"][:, None, 0:2]
    hc = ((pos - bt["cir"][:, :, 0:2]) ** 2).sum(axis=2) - bt["cir"][:, :, 2] ** 2
    he = ((pos - bt["elp"][:, :, 0:2]) ** 2).sum(axis=2) - np.maximum(bt["elp"][:, :, 2], bt["elp"][:, :, 3]) ** 2
    in_c, in_e = np.arange(nci)[None] < nc[:, None], np.arange(nel)[None] < ne[:, None]
    if variant == 0:   # select_obs: keep h <= detect_r2; leave out the obstacles within 1e-6 of the threshold
        r2 = cfg.detect_r2
        assert not np.any(in_c & (np.abs(hc - r2) <= 1e-6)) and not np.any(in_e & (np.abs(he - r2) <= 1e-6))
        far_c, far_e = in_c & (hc > r2 + 1e-6), in_e & (he > r2 + 1e-6)
        assert far_c.sum() >= 20 and far_e.sum() >= 5
        # a dropped slot in front of a kept one: the slot map matters
        assert np.any(far_c[:, :-1] & (in_c & ~far_c)[:, 1:])
    else:
        far_c, far_e = np.zeros_like(in_c), np.zeros_like(in_e)
    zero = np.concatenate([np.repeat(~in_c | far_c, 3, axis=1), np.repeat(~in_e | far_e, 5, axis=1)], axis=1)   # (B, P)
    for max_iter in (100, 3):
        cfg = gpu_lib.default_cfg(variant, N, nc_max=nci, ne_max=nel, max_iter=max_iter)
        s = gpu_lib.Solver(cfg)
        o = s.solve_sens_obs(bt["x0"], bt["goal"], bt["leg"], bt["cir"], nc, bt["elp"], ne, u0=bt["u0"])
        ok = o["sens_ok"] == 1
        assert np.array_equal(ok, np.isin(o["status"], (0, 1)) & np.isfinite(o["dfoot"]).all(axis=(1, 2)))
        if max_iter == 3:
            assert (~ok).sum() >= B // 4
        else:
            assert ok.sum() >= B // 2
            live = np.abs(o["du_obs"][ok]).max(axis=1)[~zero[ok]]
            assert np.mean(live > 0) >= 0.9   # the other columns are not zero
        for k in OBS_KEYS + ("dfoot", "du"):
            assert np.isnan(o[k][~ok]).all(), k
            assert np.isfinite(o[k][ok]).all(), k
        for k in OBS_KEYS:
            z = np.broadcast_to(zero[:, None, :], o[k].shape)
            assert np.all(o[k][ok][z[ok]] == 0.0) and not np.any(np.signbit(o[k][ok][z[ok]])), k


def test_sens_obs_refusals(gpu_lib):
    """fp32, lane-program, DD and N = 6 handles refuse the entry point with EUNSUPPORTED and still solve; a handle
    without obstacle slots and a call without dfoot_obs get EINVAL."""
    from alipmpc import scenes
    from alipmpc._lib import _ptr
    bt = scenes.make_batch(8, seed=35, n_cir=5)
    a = (bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"])
    for kw in (dict(precision=gpu_lib.PREC_FP32), dict(program=gpu_lib.PROGRAM_LANE)):
        s = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0, **kw))
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            s.solve_sens_obs(*a, u0=bt["u0"])
        assert np.isfinite(s.solve(*a, u0=bt["u0"])["u"]).all()
    b6 = scenes.make_batch(8, seed=36, n_cir=3, N=6)
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, 6, nc_max=3, ne_max=0))
    a6 = (b6["x0"], b6["goal"], b6["leg"], b6["cir"], b6["nc"])
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        s.solve_sens_obs(*a6, u0=b6["u0"])
    assert np.isfinite(s.solve(*a6, u0=b6["u0"])["u"]).all()
    s = gpu_lib.Solver(gpu_lib.default_cfg(2, 3, nc_max=5, ne_max=0))
    xd = np.stack([bt["x0"][:, 0], bt["x0"][:, 1], bt["x0"][:, 4]], 1)
    lu = np.tile([0.6, 0.0], (8, 1))
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        s.solve_sens_obs(xd, bt["goal"], None, bt["cir"], bt["nc"], u0=np.tile(lu, (1, 3)))
    assert np.isfinite(s.solve(xd, bt["goal"], None, bt["cir"], bt["nc"], u0=np.tile(lu, (1, 3)), last_u=lu)["u"]).all()
    # P = 0
    s = gpu_lib.Solver(gpu_lib.default_cfg(1, 3, nc_max=0, ne_max=0))
    assert s.sens_obs_cols == 0
    z = (bt["x0"], bt["goal"], bt["leg"], np.zeros((8, 0, 3)), np.zeros(8, np.int32))
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.solve_sens_obs(*z, u0=bt["u0"])
    assert np.isfinite(s.solve(*z, u0=bt["u0"])["u"]).all()
    # dfoot_obs = NULL
    s = gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0))
    x0, goal, leg, cir, nc, u0 = (np.ascontiguousarray(v) for v in (bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"],
                                                                    bt["u0"]))
    u, df = np.zeros((8, 15)), np.full((8, 3, 7), 5.0)
    rc = s._L.alipmpc_solve_sens_obs_batch(s._h, 8, _ptr(x0), _ptr(goal), _ptr(leg), _ptr(cir), _ptr(nc), None, None,
                                           _ptr(u0), None, _ptr(u), None, None, None, None, _ptr(df), None, None, None,
                                           None, None)
    assert rc == -1   # ALIPMPC_EINVAL
    assert np.all(df == 5.0) and np.all(u == 0.0)   # nothing ran
    assert np.isfinite(s.solve(*a, u0=bt["u0"])["u"]).all()
