"""The KKT solvers of the solve kernels on their own: gj_regs (readlane and row-broadcast forms), gj_lds and chol_rows.

alipmpc_dbg_kkt_solves (a test hook of the library, not part of the ABI) runs one wave per system on rows [K | rhs]:
gj_regs<n, R, false / true> and gj_lds<n, n + 1, R> for n = 3, 6, 9, 12, 15, chol_rows<18, R> (the N = 6 shape), R =
double and float.

Systems: K = Q diag(geomspace(1, cond)) Q^T, symmetrised, cond = 1, 1e4, 1e8, 1e12 (fp32: 1, 1e2, 1e4), four seeds
each; in fp64 one system scaled by 1e-150 and one by 1e+150; one with a pivot of +1e-300 (fp32: +1e-30, the like
among fp32's normal numbers), which must pass; and the verdict cases, which must fail: a zero pivot at step 0, a
negative pivot at the last step, a matrix that is SPD except for one eigenvalue of -1e-12 ||K||, a NaN entry.  (The
eigenvalue case in fp32: the cast of K to fp32 alone moves every eigenvalue by up to 6e-8 ||K||, so -1e-12 ||K|| has
no sign there; fp32 takes -1e-3 ||K||, well above n eps cond of that matrix.)  The system the solver sees is the one
cast to R; every error is measured against that one.

Checks.  The normwise backward error ||K x - b|| / (||K|| ||x|| + ||b||) (infinity norms, residual in the reference
precision: mpmath at 200 bits, numpy.longdouble without it) of every form is at most 4 x that of a plain numpy
restatement of the same elimination in the same type — same pivot order, 1 / d where the kernel has rcp_nr(d), a
separate multiply and subtract where the kernel has an fma — with a floor of n eps: every pivot's reciprocal and every
contracted fma may differ from numpy by one rounding, which moves the error by a small factor but not its order.  x
is compared with the reference solution through the condition number: a backward error eta bounds the forward error
by 2 cond eta / (1 - cond eta).  chol_rows: ||L L^T - K|| / ||K|| the same way, and idg[j] L[j][j] = 1 within 2 ulp.
gj_regs<false> = gj_regs<true> bit for bit; gj_lds and gj_regs normalise the pivot row at different times, so they
agree within the bound their backward errors give.  The verdict equals the restatement's on every system.
"""
import ctypes

import numpy as np
import pytest

try:
    import mpmath
    HAVE_MP = True
except ImportError:                                      # the longdouble reference (no skip)
    mpmath = None
    HAVE_MP = False

pytestmark = pytest.mark.gpu

GJ_N = (3, 6, 9, 12, 15)
CHOL_N = 18
PREC = 200


# ------------------------------------------------------------------------------------------------ systems
def _spd(rng, n, cond):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    k = (q * np.geomspace(1.0, cond, n)) @ q.T
    return 0.5 * (k + k.T)


def systems(n, fp32):
    """(sys (M, n, n + 1) as the solver sees them, names, must: the verdict each case has to get, None = the
    restatement's)."""
    rng = np.random.default_rng(52000 + 10 * n + fp32)
    rhs = lambda: rng.standard_normal((n, 1))
    out, names, must = [], [], []

    def add(k, b, name, verdict=None):
        out.append(np.concatenate([k, b], axis=1))
        names.append(name)
        must.append(verdict)
    for cond in ((1.0, 1e2, 1e4) if fp32 else (1.0, 1e4, 1e8, 1e12)):
        for seed in range(4):
            add(_spd(rng, n, cond), rhs(), f"cond {cond:g} #{seed}", 1)
    if not fp32:
        add(_spd(rng, n, 1e4) * 1e-150, rhs(), "scaled 1e-150", 1)
        add(_spd(rng, n, 1e4) * 1e+150, rhs(), "scaled 1e+150", 1)
    tiny = 1e-30 if fp32 else 1e-300
    k = np.diag(np.concatenate([[tiny], np.geomspace(1.0, 10.0, n - 1)]))
    b = rhs()
    b[0] *= tiny
    add(k, b, f"pivot +{tiny:g}", 1)
    # the verdict cases
    k = _spd(rng, n, 10.0)
    k[0, 0] = 0.0
    add(k, rhs(), "zero pivot at step 0", 0)
    lo = np.tril(rng.uniform(-0.5, 0.5, (n, n)), -1) + np.eye(n)
    d = np.ones(n)
    d[-1] = -1.0
    k = (lo * d) @ lo.T
    add(0.5 * (k + k.T), rhs(), "negative pivot at the last step", 0)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.geomspace(1.0, 100.0, n)
    ev[0] = (-1e-3 if fp32 else -1e-12) * 100.0
    k = (q * ev) @ q.T
    add(0.5 * (k + k.T), rhs(), "one eigenvalue of -%g ||K||" % (1e-3 if fp32 else 1e-12), 0)
    k = _spd(rng, n, 10.0)
    k[n // 2, 0] = k[0, n // 2] = np.nan
    add(k, rhs(), "NaN entry", 0)
    s = np.ascontiguousarray(np.stack(out))
    if fp32:
        s = s.astype(np.float32).astype(np.float64)
    s.setflags(write=False)
    return s, names, must


# ------------------------------------------------------------------------------------------------ restatements
def gj_regs_np(s, R):
    """gj_regs in numpy, type R: the pivot row stays, columns j > p of every other row are updated, the diagonal
    divides the right-hand side at the end."""
    a = s.astype(R)
    n = a.shape[0]
    with np.errstate(all="ignore"):
        for p in range(n):
            d = a[p, p]
            if not d > 0:
                return None
            m = a[:, p] * (R(1) / d)
            m[p] = 0
            a[:, p + 1:] = a[:, p + 1:] - (m[:, None] * a[p, p + 1:][None, :]).astype(R)
        return (a[:, n] * (R(1) / np.diag(a))).astype(np.float64)


def gj_lds_np(s, R):
    """gj_lds in numpy, type R: the pivot row is scaled by 1 / d, then every other row -= a_ip row p."""
    a = s.astype(R)
    n = a.shape[0]
    with np.errstate(all="ignore"):
        for p in range(n):
            d = a[p, p]
            if not d > 0:
                return None
            f = a[p, p + 1:] * (R(1) / d)
            mip = a[:, p].copy()
            a[:, p + 1:] = a[:, p + 1:] - (mip[:, None] * f[None, :]).astype(R)
            a[p, p + 1:] = f
        return a[:, n].astype(np.float64)


def chol_rows_np(k, R):
    """chol_rows in numpy, type R: right-looking, 1 / sqrt(d) where the kernel has rsqrt_nr(d).  (L, idg) or None."""
    a = k.astype(R)
    n = a.shape[0]
    idg = np.ones(n, R)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = a[j, j]
            if not d > 0:
                return None
            inv = R(1) / np.sqrt(d)
            idg[j] = inv
            lij = a[:, j] * inv
            a[:, j] = lij
            a[j, j] = d * inv
            a[:, j + 1:] = a[:, j + 1:] - (lij[:, None] * lij[None, j + 1:]).astype(R)
    return np.tril(a).astype(np.float64), idg.astype(np.float64)


# ------------------------------------------------------------------------------------------------ reference
def _norm_inf(m):
    return float(np.abs(m).sum(axis=1).max()) if m.ndim == 2 else float(np.abs(m).max())


def ref_solve(k, b):
    """x of K x = b in the reference precision, rounded to fp64."""
    if HAVE_MP:
        with mpmath.workprec(PREC):
            # rows scaled by powers of two (exact): lu_solve's singularity test is absolute
            a, r = mpmath.matrix(k.tolist()), mpmath.matrix(b.tolist())
            for i in range(len(b)):
                e = -int(np.frexp(np.abs(k[i]).max())[1])
                for j in range(len(b)):
                    a[i, j] = mpmath.ldexp(a[i, j], e)
                r[i] = mpmath.ldexp(r[i], e)
            return np.array([float(v) for v in mpmath.lu_solve(a, r)])
    L = np.longdouble                                    # Gaussian elimination with partial pivoting + refinement
    n = len(b)
    a = np.concatenate([k.astype(L), np.eye(n, dtype=L)], axis=1)
    for p in range(n):
        i = p + int(np.argmax(np.abs(a[p:, p])))
        a[[p, i]] = a[[i, p]]
        a[p] = a[p] / a[p, p]
        for r in range(n):
            if r != p:
                a[r] = a[r] - a[r, p] * a[p]
    inv, x = a[:, n:], np.zeros(n, L)
    for _ in range(4):
        x = x + inv @ (b.astype(L) - k.astype(L) @ x)
    return x.astype(np.float64)


def backward_error(k, b, x):
    """||K x - b|| / (||K|| ||x|| + ||b||), infinity norms, the residual in the reference precision."""
    if not np.isfinite(x).all():
        return np.inf
    if HAVE_MP:
        with mpmath.workprec(PREC):
            r = mpmath.matrix(k.tolist()) * mpmath.matrix(x.tolist()) - mpmath.matrix(b.tolist())
            rn = float(max(abs(v) for v in r))
    else:
        L = np.longdouble
        rn = float(np.abs(k.astype(L) @ x.astype(L) - b.astype(L)).max())
    # (the norms through longdouble: at a scale of 1e+-150 their product leaves fp64's range)
    den = np.longdouble(_norm_inf(k)) * np.longdouble(_norm_inf(x)) + np.longdouble(_norm_inf(b))
    return float(np.longdouble(rn) / den)


def factor_error(k, lo):
    """||L L^T - K|| / ||K||, the product in the reference precision."""
    if not np.isfinite(lo).all():
        return np.inf
    if HAVE_MP:
        with mpmath.workprec(PREC):
            m = mpmath.matrix(lo.tolist())
            e = m * m.T - mpmath.matrix(k.tolist())
            rn = max(sum(abs(e[i, j]) for j in range(e.cols)) for i in range(e.rows))
            return float(rn / mpmath.mpf(_norm_inf(k)))
    L = np.longdouble
    return float(np.abs(lo.astype(L) @ lo.astype(L).T - k.astype(L)).sum(axis=1).max() / L(_norm_inf(k)))


# ------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope="module")
def kkt(gpu_lib):
    L = ctypes.CDLL(gpu_lib.lib_path())
    f = L.alipmpc_dbg_kkt_solves
    P = ctypes.c_void_p
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_int, P, P]
    f.restype = ctypes.c_int

    def run(form, n, fp32, s):
        s = np.ascontiguousarray(s, np.float64)
        assert s.shape[1:] == (n, n + 1)
        x = np.full((len(s), n, n + 1) if form == 3 else (len(s), n), 12345.0)
        ok = np.full(len(s), -7, np.int32)
        rc = f(form, n, int(fp32), s.ctypes.data_as(P), len(s), x.ctypes.data_as(P), ok.ctypes.data_as(P))
        assert rc == 0, (form, n, fp32, rc)
        assert np.isin(ok, (0, 1)).all()
        return x, ok
    return run


def test_hook_refuses_shapes_it_does_not_hold(kkt, gpu_lib):
    L = ctypes.CDLL(gpu_lib.lib_path())
    f = L.alipmpc_dbg_kkt_solves
    z = np.zeros(18 * 19)
    p = z.ctypes.data_as(ctypes.c_void_p)
    ok = np.zeros(1, np.int32)
    for form, n in ((0, 4), (1, 18), (2, 16), (3, 15), (4, 9), (-1, 9)):
        assert f(form, n, 0, p, 1, p, ok.ctypes.data_as(ctypes.c_void_p)) == -1, (form, n)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", GJ_N)
def test_gauss_jordan(kkt, n, fp32):
    """Backward error of gj_regs / gj_lds <= max(4 x the numpy restatement's, n eps) on every system that passes, the
    verdicts, the two broadcast forms bit for bit.  MI355X (profiles/fastmath/kkt.txt): the largest backward error is
    0.151 of the bar (n = 3, fp64, both forms), 0.103 for n = 15 (gj_lds, fp64), 0.044 in fp32; every figure sits under
    the n eps floor.  Against the restatement the device is at most 7.7 x (gj_regs, n = 9, cond 1e8 #3: 9.8e-17
    against 1.3e-17, a twentieth of the floor), gj_lds 4.3 x, fp32 3.6 x / 3.4 x."""
    R, eps = (np.float32, 2.0 ** -23) if fp32 else (np.float64, 2.0 ** -52)
    s, names, must = systems(n, fp32)
    dev = {form: kkt(form, n, fp32, s) for form in (0, 1, 2)}
    # gj_regs<false> = gj_regs<true>, bit for bit, on every system (x of a refused system included: the same code
    # stopped at the same step)
    x0, x1 = dev[0][0], dev[1][0]
    eq = (x0.view(np.uint64) == x1.view(np.uint64)) | (np.isnan(x0) & np.isnan(x1))
    assert eq.all() and np.array_equal(dev[0][1], dev[1][1]), np.argwhere(~eq)[:8].tolist()
    worst = {0: 0.0, 2: 0.0}
    for m, name in enumerate(names):
        k, b = s[m, :, :n], s[m, :, n]
        restate = {0: gj_regs_np(s[m], R), 2: gj_lds_np(s[m], R)}
        xs = {}
        for form in (0, 2):
            x, ok = dev[form]
            want = restate[form] is not None
            if must[m] is not None:
                assert int(want) == must[m], ("restatement", name, form)
            assert ok[m] == int(want), (name, "form", form, "device", int(ok[m]), "restatement", int(want))
            if not want:
                continue
            be_np, be = backward_error(k, b, restate[form]), backward_error(k, b, x[m])
            bar = max(4.0 * be_np, n * eps)
            worst[form] = max(worst[form], be / bar)
            print(f"KKT {'gj_lds' if form else 'gj_regs'} n={n} {'fp32' if fp32 else 'fp64'} [{name}]: backward error "
                  f"{be:.3e}, restatement {be_np:.3e}, bar {bar:.3e}")
            assert be <= bar, (name, form, be, be_np, bar)
            xs[form] = (x[m], bar)
        if 0 in xs:
            # forward: against the reference solution, and the two forms against each other, through cond(K)
            xr = ref_solve(k, b)
            if name.startswith("pivot"):
                # diagonal, with entries 1e300 apart: the normwise bound says nothing; x_i = b_i / d_i to 2 roundings
                for form, (x, _) in xs.items():
                    assert (np.abs(x - xr) <= 2.0 * np.spacing(np.abs(xr).astype(R)).astype(np.float64)).all(), form
                continue
            cond = _norm_inf(k) * _norm_inf(np.linalg.inv(k))
            scale = _norm_inf(xr)
            for form, (x, bar) in xs.items():
                assert cond * bar < 0.5, (name, cond, bar)
                fwd = 2.0 * cond * bar / (1.0 - cond * bar)
                assert _norm_inf(x - xr) <= fwd * scale, (name, form, _norm_inf(x - xr) / scale, fwd)
            fwd = sum(2.0 * cond * bar / (1.0 - cond * bar) for _, bar in xs.values())
            assert _norm_inf(xs[0][0] - xs[2][0]) <= fwd * scale, name
    print(f"KKT n={n} {'fp32' if fp32 else 'fp64'}: largest backward error / bar: gj_regs {worst[0]:.3f}, "
          f"gj_lds {worst[2]:.3f} over {len(names)} systems")


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_chol_rows(kkt, fp32):
    """||L L^T - K|| / ||K|| <= max(4 x the numpy restatement's, n eps), idg[j] L[j][j] = 1 within 2 ulp, the
    verdicts.  MI355X (profiles/fastmath/kkt.txt): the largest factor error is 0.090 of the bar in fp64 and 0.037 in
    fp32, at most 2.0 x / 1.5 x the restatement's; |idg L_jj - 1| reaches 1.792 ulp in both types (the restatement,
    with a correctly rounded 1 / sqrt, reaches 1.53)."""
    n = CHOL_N
    R, eps = (np.float32, 2.0 ** -23) if fp32 else (np.float64, 2.0 ** -52)
    s, names, must = systems(n, fp32)
    out, ok = kkt(3, n, fp32, s)
    worst, worst_dg = 0.0, 0.0
    for m, name in enumerate(names):
        k = s[m, :, :n]
        restate = chol_rows_np(k, R)
        want = restate is not None
        if must[m] is not None:
            assert int(want) == must[m], ("restatement", name)
        assert ok[m] == int(want), (name, "device", int(ok[m]), "restatement", int(want))
        if not want:
            continue
        lo, idg = out[m, :, :n], out[m, :, n]
        assert (np.triu(lo, 1) == 0).all()
        fe_np, fe = factor_error(k, restate[0]), factor_error(k, lo)
        bar = max(4.0 * fe_np, n * eps)
        one = np.abs(idg.astype(np.longdouble) * np.diag(lo).astype(np.longdouble) - 1).astype(np.float64) / eps
        worst, worst_dg = max(worst, fe / bar), max(worst_dg, float(one.max()))
        print(f"KKT chol_rows n={n} {'fp32' if fp32 else 'fp64'} [{name}]: factor error {fe:.3e}, restatement "
              f"{fe_np:.3e}, bar {bar:.3e}; max |idg L_jj - 1| {one.max():.3f} ulp")
        assert fe <= bar, (name, fe, fe_np, bar)
        assert (one <= 2.0).all(), (name, one.max())
    print(f"KKT chol_rows n={n} {'fp32' if fp32 else 'fp64'}: largest factor error / bar {worst:.3f}, largest "
          f"|idg L_jj - 1| {worst_dg:.3f} ulp over {len(names)} systems")
