"""The wave helpers of the solve kernels' interior-point loop against the forms they replaced, bit for bit.

alipmpc_dbg_wave_helpers (a test hook of the library, not part of the ABI) runs one wave that evaluates, side by side:
wreduce2 (two values in one butterfly) and two wreduce calls for sum / max / min, the max-min pair, rbcast<P> (row
broadcast) and readlane for every P, llog and the error scalings packed into lanes and one call per argument, and
gj_regs<9> with row broadcasts and with readlane broadcasts.  The new forms reorder no floating-point operation, so
every result must carry the same bits; where both are NaN only that is required (a NaN's payload may differ).

The solve-level tests run the smallest shapes that exercise every path of the kernels that use these helpers: the
one-phase launch, the 4-wave split and the paired split must agree bit for bit, at N = 3 with scenes that enter the
restoration phase and at N = 5 with ellipses (two row groups per lane, register Cholesky)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE = 64
KEYS = ("status", "iters", "u", "foot", "x_pred")


def _input_sets():
    """(S, 2, 64) lane values a, b: normal, wide exponent range, specials, NaN lanes."""
    rng = np.random.default_rng(20260)
    sets = []
    for _ in range(3):                                   # random normal
        sets.append(rng.standard_normal((2, WAVE)))
    for _ in range(3):                                   # wide exponent range, both signs
        sets.append(rng.standard_normal((2, WAVE)) * 10.0 ** rng.uniform(-300, 300, (2, WAVE)))
    for _ in range(2):                                   # positive, wide range (finite logs, positive scalings)
        sets.append(np.abs(rng.standard_normal((2, WAVE))) * 10.0 ** rng.uniform(-200, 200, (2, WAVE)) + 1e-300)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1.1e-308, 1.0, -1.0])
    for k in range(3):                                   # signed zeros, infinities, denormals in every lane position
        sets.append(rng.choice(special, (2, WAVE)))
        sets[-1][:, :len(special)] = np.roll(special, k)
    zeros = np.where(rng.random((2, WAVE)) < 0.5, 0.0, -0.0)   # only signed zeros: max / min must order them alike
    sets.append(zeros)
    sets.append(np.stack([np.full(WAVE, np.inf), np.full(WAVE, -np.inf)]))   # empty max / min pair
    for k in (1, 7):                                     # lanes holding NaN
        v = rng.standard_normal((2, WAVE))
        v[0, rng.choice(WAVE, k, replace=False)] = np.nan
        v[1, rng.choice(WAVE, k, replace=False)] = np.nan
        sets.append(v)
    nan_low = rng.standard_normal((2, WAVE))             # NaN in the lanes the packed functions read
    nan_low[:, :3] = np.nan
    sets.append(nan_low)
    sets.append(np.full((2, WAVE), np.nan))
    return np.ascontiguousarray(np.stack(sets))


def _systems():
    """(M, 9, 10) rows [K | rhs]: SPD systems of growing condition number, then one indefinite one."""
    rng = np.random.default_rng(20261)
    out = []
    for cond in (1.0, 1e4, 1e10):
        q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
        k = (q * np.geomspace(1.0, cond, 9)) @ q.T
        k = 0.5 * (k + k.T)
        out.append(np.concatenate([k, rng.standard_normal((9, 1))], axis=1))
    a = rng.standard_normal((9, 9))
    k = a @ a.T + 9.0 * np.eye(9)
    k[4, 4] = -1.0                                       # a non-positive pivot on the way
    out.append(np.concatenate([k, rng.standard_normal((9, 1))], axis=1))
    return np.ascontiguousarray(np.stack(out))


@pytest.fixture(scope="module")
def helpers(gpu_lib):
    """One launch of the hook for every helper test."""
    L = ctypes.CDLL(gpu_lib.lib_path())
    f = L.alipmpc_dbg_wave_helpers
    P = ctypes.c_void_p
    f.argtypes = [P, ctypes.c_int, P, ctypes.c_int, P, P]
    f.restype = ctypes.c_int
    sets, syst = _input_sets(), _systems()
    per = 32 + 2 * 16 * WAVE
    out = np.full((len(sets), per), 12345.0)
    gj = np.full((len(syst), 2, 10), 12345.0)
    rc = f(sets.ctypes.data_as(P), len(sets), syst.ctypes.data_as(P), len(syst), out.ctypes.data_as(P),
           gj.ctypes.data_as(P))
    assert rc == per, rc
    return sets, syst, out, gj


def _same_bits(new, old, what):
    new, old = np.asarray(new, np.float64), np.asarray(old, np.float64)
    both_nan = np.isnan(new) & np.isnan(old)
    eq = (new.view(np.uint64) == old.view(np.uint64)) | both_nan
    assert eq.all(), (what, np.argwhere(~eq)[:8].tolist(), new[~eq][:4], old[~eq][:4])


def test_paired_reductions(helpers):
    sets, _, out, _ = helpers
    names = ("sum a", "sum b", "max a", "max b", "min a", "min b")
    for i, nm in enumerate(names):
        _same_bits(out[:, 6 + i], out[:, i], ("wreduce2", nm))
    _same_bits(out[:, 14], out[:, 12], "wmaxmin_pair max")
    _same_bits(out[:, 15], out[:, 13], "wmaxmin_pair min")
    # the old forms themselves do what their names say (numpy's fmax / fmin skip NaN as the device's do)
    with np.errstate(invalid="ignore"):
        fin = ~np.isnan(sets).any(axis=(1, 2))
        assert np.array_equal(out[fin, 2], sets[fin, 0].max(axis=1))
        assert np.array_equal(out[fin, 5], sets[fin, 1].min(axis=1))


def test_row_broadcast(helpers):
    sets, _, out, _ = helpers
    old = out[:, 32:32 + 16 * WAVE].reshape(-1, 16, WAVE)
    new = out[:, 32 + 16 * WAVE:].reshape(-1, 16, WAVE)
    _same_bits(new, old, "rbcast")
    lane = np.arange(WAVE)
    for p in range(16):                                  # and the old form is the row's lane p
        _same_bits(old[:, p, :], sets[:, 0, (lane & 48) + p], ("readlane", p))


def test_packed_scalar_functions(helpers):
    sets, _, out, _ = helpers
    _same_bits(out[:, 19:22], out[:, 16:19], "llog3")
    _same_bits(out[:, 24:26], out[:, 22:24], "err_scales")
    pos = (sets[:, 0, :3] > 0).all(axis=1) & np.isfinite(sets[:, 0, :3]).all(axis=1)
    assert pos.sum() >= 2
    np.testing.assert_allclose(out[pos, 16:19], np.log(sets[pos, 0, :3]), rtol=1e-14, atol=1e-15)


def test_gauss_jordan_row_broadcast(helpers):
    _, syst, _, gj = helpers
    _same_bits(gj[:, 1, :], gj[:, 0, :], "gj_regs")
    assert gj[:3, 0, 9].tolist() == [1.0, 1.0, 1.0] and gj[3, 0, 9] == 0.0   # the pivot verdicts
    for m in range(2):                                   # the well-conditioned systems are solved
        x = np.linalg.solve(syst[m, :, :9], syst[m, :, 9])
        np.testing.assert_allclose(gj[m, 0, :9], x, rtol=1e-9, atol=1e-12)


def _solve(gpu_lib, monkeypatch, cfg, bt, cut, pair):
    monkeypatch.setenv("ALIPMPC_SPLIT_IT", str(cut))
    monkeypatch.setenv("ALIPMPC_SPLIT_PAIR", "1" if pair else "0")
    monkeypatch.setenv("ALIPMPC_SPLIT_TR", "0")
    s = gpu_lib.Solver(cfg)
    return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], elp=bt.get("elp"), ne=bt.get("ne"),
                   u0=bt["u0"])


def _three_forms(gpu_lib, monkeypatch, cfg, bt, cuts):
    ref = _solve(gpu_lib, monkeypatch, cfg, bt, 0, True)          # one phase
    for cut in cuts:
        for pair in (False, True):                                # 4-wave phase 2, paired phase 2
            o = _solve(gpu_lib, monkeypatch, cfg, bt, cut, pair)
            for k in KEYS:
                assert np.array_equal(o[k], ref[k]), (cut, pair, k)
    return ref


def test_solve_forms_agree_n3_with_restorations(gpu_lib, monkeypatch):
    """B = 64, N = 3, 5 circle slots: every other instance an infeasible obstacle field (restoration phase)."""
    from alipmpc import scenes
    cfg = gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0)
    big = scenes.make_batch(512, seed=77, n_cir=5)
    st = _solve(gpu_lib, monkeypatch, cfg, big, 0, True)["status"]
    bad, good = np.flatnonzero(st == 2), np.flatnonzero(st == 0)
    B = 64
    assert len(bad) >= B // 2 and len(good) >= B // 2
    idx = np.where(np.arange(B) % 2 == 0, bad[np.arange(B) // 2 % len(bad)], good[np.arange(B) // 2])
    bt = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in big.items()}
    ref = _three_forms(gpu_lib, monkeypatch, cfg, bt, (5, 11))
    assert (ref["status"] == 2).sum() == B // 2 and (ref["status"] == 0).sum() == B // 2


def test_solve_forms_agree_n5_with_ellipses(gpu_lib, monkeypatch):
    """B = 64, N = 5, 5 circles + 5 ellipses: two row groups per lane, register Cholesky."""
    from alipmpc import scenes
    cfg = gpu_lib.default_cfg(0, 5, nc_max=5, ne_max=5)
    bt = scenes.make_batch(64, seed=5, n_cir=5, n_elp=5, N=5)
    ref = _three_forms(gpu_lib, monkeypatch, cfg, bt, (6,))
    assert (ref["status"] == 0).any() and (ref["iters"] > 6).any()   # (some instances cross the cut)
