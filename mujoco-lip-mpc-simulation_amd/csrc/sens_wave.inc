// Plan sensitivities of the wave program's fp64 solve (alipmpc_solve_sens_batch; DESIGN.md §3.7).  Device code,
// included by alipmpc.hip after resto_wave.inc; only the sensitivity builds of solve_one (SN = 1, sens_kernel; SN = 2,
// sens_obs_kernel, which adds the obstacle columns of alipmpc_solve_sens_obs_batch, DESIGN.md §3.10) call it, so no
// other instantiation holds a line of it.
//
// At the accepted iterate of an instance that ended with status 0 or 1 the barrier KKT conditions of the slack
// formulation, differentiated with mu and the prologue's decisions (obstacle selection, leg parity, the detour and its
// side) held fixed, read
//     (W + J^T Sigma J) dp = -(L_p,theta + J^T Sigma c_theta) dtheta .
// In generator space (V = E x0 + G p, J = C G, c_x0 = C E, W = G^T S G) the left side is the iteration's own
// K = G^T (S + C^T Sigma C) G at delta = 0 and the x0 columns of the right side are R = G^T (S + C^T Sigma C) E: the same
// product with E as the second operand.  The constraints do not see the goal and the objective sees it only through
// g - pos_k, so the goal columns are G^T times minus the position columns of the objective's own part of S (hobj).
// Where the detour fired the objective's goal is g_eff = x0_pos + Rot(+-pi/12)(g - x0_pos): d g_eff / d g = Rot and
// d g_eff / d x0_pos = I - Rot are folded into the columns, so the outputs are total derivatives.
// [K | R] is eliminated on register rows (gj_regs with 7 right-hand sides: lane i holds row i, the same pivot order
// and the same "every pivot > 0" test; no regularisation: a pivot <= 0 makes the instance's sensitivity invalid; the
// rows' part of K and R and the elimination in double-double, for the reason given at dd2 below) and
// dp / dtheta = -K^-1 R gives dfoot (rows of p_0) and du = d(x_1 .. x_N) / dtheta = E + G dp (the canonical u_k = x_{k+1}).
// Columns: 0-4 the components of x0, 5-6 the goal.  An invalid instance gets NaN in every derivative and sens_ok = 0.

constexpr int SENS_COLS = 7;

// the sensitivity outputs travel in KP's eval-output slots, which a solve launch leaves unused (a member of their own
// would change sizeof(KP), the LDS layout and with it the code of every existing kernel)
__device__ __forceinline__ double* sens_dfoot(const KP& P) { return P.grad_out; }                              // B x 3 x 7
__device__ __forceinline__ double* sens_du(const KP& P) { return P.J_out; }                                    // B x 5N x 7
__device__ __forceinline__ int32_t* sens_okp(const KP& P) { return reinterpret_cast<int32_t*>(P.active_out); }  // B

// Why double-double.  At the accepted iterate mu is ~1e-9, so an active row has Sigma = z / d ~ 1e9 .. 1e10 and K =
// H + sum Sigma_r j_r j_r^T holds entries of that size next to a Hessian of order 1 .. 100.  An iteration's step
// tolerates the 1e-16 |K| ~ 1e-7 that fp64 assembly and elimination leave on H (Newton corrects itself); a derivative
// does not: measured against the oracle's finite differences the fp64 epilogue missed by a median 7e-7 (N = 3) to 3e-4
// (du at N = 5), twenty times and more what the oracle's own tolerance costs.  The remedy keeps the system and changes
// the arithmetic: each row enters as b_r = sqrt(Sigma_r) j_r rounded ONCE (a 1e-16 change of a constraint's own
// gradient, which the solution does not amplify), the products b_ri b_rj are exact (fma), and their sums and the
// elimination run in double-double.  The Hessian part G^T S G keeps fp64 and the MFMA: its entries are of order H.
struct dd2 {
    double h, l;
};
__device__ __forceinline__ dd2 dd_fast(double s, double e)   // |s| >= |e|
{
#pragma clang fp contract(off)
    const double h = s + e;
    return dd2{h, e - (h - s)};
}
__device__ __forceinline__ dd2 dd_add(dd2 x, dd2 y)
{
#pragma clang fp contract(off)
    const double s = x.h + y.h, bb = s - x.h;
    double e = (x.h - (s - bb)) + (y.h - bb);
    e = e + (x.l + y.l);
    return dd_fast(s, e);
}
__device__ __forceinline__ dd2 dd_prod(double a, double b)   // exact
{
#pragma clang fp contract(off)
    const double p = a * b;
    return dd2{p, __builtin_fma(a, b, -p)};
}
__device__ __forceinline__ dd2 dd_mul(dd2 x, dd2 y)
{
#pragma clang fp contract(off)
    const double p = x.h * y.h;
    double e = __builtin_fma(x.h, y.h, -p);
    e = e + (x.h * y.l + x.l * y.h);
    return dd_fast(p, e);
}
__device__ __forceinline__ dd2 dd_neg(dd2 x) { return dd2{-x.h, -x.l}; }
__device__ __forceinline__ dd2 dd_div(dd2 x, dd2 y)
{
#pragma clang fp contract(off)
    const double q1 = x.h / y.h;
    dd2 r = dd_add(x, dd_neg(dd_mul(y, dd2{q1, 0.0})));
    const double q2 = r.h / y.h;
    r = dd_add(r, dd_neg(dd_mul(y, dd2{q2, 0.0})));
    const double q3 = r.h / y.h;
    return dd_add(dd_fast(q1, q2), dd2{q3, 0.0});
}

// gj_steps / gj_regs with NR right-hand sides in double-double: (ah, al)[0..n-1] row i of K, [n..n+NR-1] row i of the
// right-hand sides; the same pivot order, the same "every pivot > 0" test (on the leading part)
template <int p, int n, int NR>
__device__ __forceinline__ bool gj_steps_m(double (&ah)[n + NR], double (&al)[n + NR], int lane)
{
    if constexpr (p < n) {
        const dd2 d{bcast(ah[p], p), bcast(al[p], p)};
        if (!(d.h > 0.0)) return false;   // wave-uniform
        dd2 m = dd_div(dd2{ah[p], al[p]}, d);
        if (lane == p) m = dd2{0.0, 0.0};
#pragma unroll
        for (int j = p + 1; j < n + NR; ++j) {
            const dd2 x{bcast(ah[j], p), bcast(al[j], p)};
            const dd2 t = dd_add(dd2{ah[j], al[j]}, dd_neg(dd_mul(m, x)));
            ah[j] = t.h;
            al[j] = t.l;
        }
        return gj_steps_m<p + 1, n, NR>(ah, al, lane);
    } else {
        return true;
    }
}
// on success a lane i < n holds x_i of right-hand side c in ah[n + c] (fp64)
template <int n, int NR>
__device__ __forceinline__ bool gj_regs_m(double (&ah)[n + NR], double (&al)[n + NR], int lane)
{
    static_assert(n <= 16, "the rows sit in one 16-lane row");
    if (!gj_steps_m<0, n, NR>(ah, al, lane)) return false;
    dd2 dg{ah[0], al[0]};
#pragma unroll
    for (int i = 1; i < n; ++i) dg = lane == i ? dd2{ah[i], al[i]} : dg;
    if (lane >= n) dg = dd2{1.0, 0.0};
#pragma unroll
    for (int c = 0; c < NR; ++c) ah[n + c] = dd_div(dd2{ah[n + c], al[n + c]}, dg).h;
    return true;
}

// acc[jj] += b * (b of lane jj of this 16-lane row), jj = 0 .. n - 1, exact products, double-double sums
template <int jj, int n>
__device__ __forceinline__ void sens_acc_row(double b, double (&h)[n], double (&l)[n])
{
    if constexpr (jj < n) {
        const dd2 t = dd_add(dd2{h[jj], l[jj]}, dd_prod(b, rbcast<jj>(b)));
        h[jj] = t.h;
        l[jj] = t.l;
        sens_acc_row<jj + 1, n>(b, h, l);
    }
}
template <int c, int NC>
__device__ __forceinline__ void sens_acc_rhs(double b, double be, double (&h)[NC], double (&l)[NC])
{
    if constexpr (c < NC) {
        const dd2 t = dd_add(dd2{h[c], l[c]}, dd_prod(b, rbcast<c>(be)));
        h[c] = t.h;
        l[c] = t.l;
        sens_acc_rhs<c + 1, NC>(b, be, h, l);
    }
}
// sum over the 4 lane groups (lanes c, c + 16, c + 32, c + 48) of a double-double
__device__ __forceinline__ dd2 dd_gsum(dd2 v)
{
    double ah, bh, al, bl;
    swap16(v.h, ah, bh);
    swap16(v.l, al, bl);
    v = dd_add(dd2{ah, al}, dd2{bh, bl});
    swap32(v.h, ah, bh);
    swap32(v.l, al, bl);
    return dd_add(dd2{ah, al}, dd2{bh, bl});
}

// ---- the obstacle columns (alipmpc_solve_sens_obs_batch, sens_obs_kernel; DESIGN.md §3.10)
// The same system with further right-hand sides.  A parameter theta of the obstacle in selected slot j enters only the
// N D-CBF rows (k, j), c = h(x_{k+1}) + (gamma - 1) h(x_k) with h = qa dx^2 + qb dx dy + qc dy^2 - ek on
// (dx, dy) = pos - (ox, oy), so its column of the right-hand side is
//     G^T sum_k [ -y_r d2c_r/dV dtheta + (dc_r/dV) Sigma_r (dc_r/dtheta) ] ,   r = row (k, j),
// the first term from the y and the form entries hess_blocks puts into S for these rows (so K T + R t = 0 for a common
// translation, up to rounding), the second as the state columns above: b_r = sqrt(Sigma_r) j_r times sqrt(Sigma_r)
// dc_r/dtheta, exact products, double-double sums and elimination.  The centre enters through dx, dy of both states; a
// shape parameter through (qa', qb', qc', ek'), its derivatives of the form: a circle's r has (0, 0, 0, 2 r), an
// ellipse's a, b, phi follow from qa = (b cos)^2 + (a sin)^2, qb = 2 cos sin (b^2 - a^2), qc = (b sin)^2 + (a cos)^2,
// ek = (a b)^2.  No E term: x0 does not move.
// Columns are indexed by the caller's input slot (circle j: 3 j + cx, cy, r; ellipse j: 3 nc_max + 5 j + cx, cy, a, b,
// phi); the prologue's keep masks (w.cst[K_SMAP]) give the selected slot.  A slot select_obs dropped, or one at or
// above the instance's count, gets exact zeros.  One elimination per selected slot (5 right-hand sides, a circle uses 3), K
// rebuilt from the kept double-double row parts and w.K, so the pivots are the first elimination's.
constexpr int SENS_OBS_NR = 5;
__device__ __forceinline__ double* sens_dfoot_obs(const KP& P) { return P.c_out; }   // B x 3 x PC
__device__ __forceinline__ double* sens_du_obs(const KP& P) { return P.cl_out; }     // B x 5N x PC (nullable)

// every obstacle column of instance b = v
template <int N>
__device__ __forceinline__ void sens_obs_fill(const KP& P, long long b, int lane, double v)
{
    const int PC = 3 * rfl(P.nc_max) + 5 * rfl(P.ne_max);
    for (int i = lane; i < 3 * PC; i += WAVE) sens_dfoot_obs(P)[(size_t)b * 3 * PC + i] = v;
    if (sens_du_obs(P))
        for (int i = lane; i < 5 * N * PC; i += WAVE) sens_du_obs(P)[(size_t)b * 5 * N * PC + i] = v;
}

template <int N>
__device__ __forceinline__ void sens_obs_columns(const KP& P, const WSS<N, double>& w, const double* G, long long b,
                                                 int lane, const double (&kh)[Dim<N>::n], const double (&kl)[Dim<N>::n],
                                                 int rps)
{
    using R = double;
    using D = Dim<N>;
    constexpr int n = D::n, NCP = D::NCP, KLD = D::KLD, NR = SENS_OBS_NR;
    const int nc_max = rfl(P.nc_max), ne_max = rfl(P.ne_max), PC = 3 * nc_max + 5 * ne_max;
    const long long kmb = __double_as_longlong(w.cst[K_SMAP]);
    const uint32_t mc = (uint32_t)rfl((int)(kmb & 0xffffffffll)), me = (uint32_t)rfl((int)(kmb >> 32));
    const int col = lane & 15;
    const R gm1 = w.cst[K_GM1];
    R* const dfo = sens_dfoot_obs(P) + (size_t)b * 3 * PC;
    R* const duo = sens_du_obs(P) ? sens_du_obs(P) + (size_t)b * 5 * N * PC : nullptr;
    for (int s = 0; s < nc_max + ne_max; ++s) {   // the caller's input slots: circles, then ellipses
        const bool elp = s >= nc_max;
        const int si = elp ? s - nc_max : s;
        const uint32_t m = elp ? me : mc;
        const int cb = elp ? 3 * nc_max + 5 * si : 3 * si, ncol = elp ? 5 : 3;
        if (!((m >> si) & 1u)) {   // (wave-uniform) not selected: zero columns
            for (int i = lane; i < 3 * ncol; i += WAVE) dfo[(i / ncol) * PC + cb + i % ncol] = R(0.0);
            if (duo)
                for (int i = lane; i < 5 * N * ncol; i += WAVE) duo[(size_t)(i / ncol) * PC + cb + i % ncol] = R(0.0);
            continue;
        }
        const int pos = __builtin_popcount(m & ((1u << si) - 1u));
        const int j6 = elp ? nc_max + pos : pos;   // the slot's row of obs6 and its place among a step's obstacle rows
        // (qa', qb', qc', ek') of the shape parameters (columns 2 ..)
        R dq[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) dq[p][i] = R(0.0);
        if (!elp) {
            dq[0][3] = 2 * w.obs[3 * pos + 2];
        } else {
            const R* e = w.obs + 3 * nc_max + 5 * pos;
            const R ea = e[2], eb = e[3];
            R sn, cs;
            sincos(e[4], &sn, &cs);
            const R qb = w.obs6[6 * j6 + 3];
            dq[0][0] = 2 * ea * sn * sn; dq[0][1] = -4 * ea * cs * sn;
            dq[0][2] = 2 * ea * cs * cs; dq[0][3] = 2 * ea * eb * eb;
            dq[1][0] = 2 * eb * cs * cs; dq[1][1] = 4 * eb * cs * sn;
            dq[1][2] = 2 * eb * sn * sn; dq[1][3] = 2 * ea * ea * eb;
            dq[2][0] = -qb; dq[2][1] = 2 * (cs * cs - sn * sn) * (eb * eb - ea * ea); dq[2][2] = qb;
        }
        const R ox = w.obs6[6 * j6], oy = w.obs6[6 * j6 + 1];
        const R qa = w.obs6[6 * j6 + 2], qb = w.obs6[6 * j6 + 3], qc = w.obs6[6 * j6 + 4];
        R f1[NR], rh[NR], rl[NR];   // the y term (fp64: of order y q) and the Sigma term (double-double) of row `col`
#pragma unroll
        for (int c = 0; c < NR; ++c) f1[c] = rh[c] = rl[c] = R(0.0);
        for (int k = 0; k < N; ++k) {
            const int r = k * rps + 2 + j6;
            const uint32_t pk = w.rgen[r];
            R c0, c1, c2, c3;
            ld4(w.rcoef + 4 * r, c0, c1, c2, c3);
            const int t0 = gen_i(pk, 0), t1 = gen_i(pk, 1), t2 = gen_i(pk, 2), t3 = gen_i(pk, 3);
            const R g0 = G[t0 * NCP + col], g1 = G[t1 * NCP + col], g2 = G[t2 * NCP + col], g3 = G[t3 * NCP + col];
            const R sq = sqrt(w.rsig[r]), y = w.ry[r];
            const R bj = sq * (c0 * g0 + c1 * g1 + c2 * g2 + c3 * g3);
            const R x1 = w.V[t0] - ox, y1 = w.V[t1] - oy, x0 = w.V[t2] - ox, y0 = w.V[t3] - oy;
            R ct[NR];
            ct[0] = -(c0 + c2);
            ct[1] = -(c1 + c3);
            f1[0] += y * (2 * qa * g0 + qb * g1 + gm1 * (2 * qa * g2 + qb * g3));
            f1[1] += y * (qb * g0 + 2 * qc * g1 + gm1 * (qb * g2 + 2 * qc * g3));
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const R A = dq[p][0], Bq = dq[p][1], Cq = dq[p][2], Ek = dq[p][3];
                ct[2 + p] = (A * x1 * x1 + Bq * x1 * y1 + Cq * y1 * y1 - Ek) +
                            gm1 * (A * x0 * x0 + Bq * x0 * y0 + Cq * y0 * y0 - Ek);
                f1[2 + p] -= y * ((2 * A * x1 + Bq * y1) * g0 + (2 * Cq * y1 + Bq * x1) * g1 +
                                  gm1 * ((2 * A * x0 + Bq * y0) * g2 + (2 * Cq * y0 + Bq * x0) * g3));
            }
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const dd2 t = dd_add(dd2{rh[c], rl[c]}, dd_prod(bj, sq * ct[c]));
                rh[c] = t.h;
                rl[c] = t.l;
            }
        }
        R a[n + NR], al[n + NR];
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const dd2 t = dd_add(dd2{kh[j], kl[j]}, dd2{w.K[col * KLD + j], R(0.0)});
            a[j] = t.h;
            al[j] = t.l;
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const dd2 t = dd_add(dd2{rh[c], rl[c]}, dd2{f1[c], R(0.0)});
            a[n + c] = t.h;
            al[n + c] = t.l;
        }
        const bool ok = gj_regs_m<n, NR>(a, al, lane);   // (the first elimination's pivots: it cannot fail here)
        const R qn = __longlong_as_double(0x7ff8000000000000ll);
        wave_sync();   // (the last pass' reads of dp precede these writes)
        if (lane < n) {
#pragma unroll
            for (int c = 0; c < NR; ++c) w.S[lane * 8 + c] = ok ? -a[n + c] : qn;
        }
        wave_sync();
        for (int i = lane; i < 3 * ncol; i += WAVE)
            dfo[(i / ncol) * PC + cb + i % ncol] = w.S[(i / ncol) * 8 + i % ncol];
        if (duo) {
            for (int i = lane; i < 5 * N * ncol; i += WAVE) {
                const int l = i / ncol, c = i % ncol;
                const int t = gx(l / 5 + 1, l % 5);
                R v = R(0.0);
                for (int j = 0; j < n; ++j) v = fma(G[t * NCP + j], w.S[j * 8 + c], v);
                duo[(size_t)l * PC + cb + c] = v;
            }
        }
    }
    wave_sync();
}

// OB (the obstacle-sensitivity build, sens_obs_kernel): dfoot may be absent, and the obstacle columns get NaN as well
template <int N, bool OB = false>
__device__ __forceinline__ void sens_invalid(const KP& P, long long b, int lane)
{
    const double qn = __longlong_as_double(0x7ff8000000000000ll);
    if (lane < 3 * SENS_COLS && (!OB || sens_dfoot(P))) sens_dfoot(P)[(size_t)b * 3 * SENS_COLS + lane] = qn;
    if (sens_du(P))
        for (int i = lane; i < 5 * N * SENS_COLS; i += WAVE) sens_du(P)[(size_t)b * 5 * N * SENS_COLS + i] = qn;
    if (sens_okp(P) && lane == 0) sens_okp(P)[b] = 0;
    if constexpr (OB) sens_obs_fill<N>(P, b, lane, qn);
}

// the row state is solve_one's at its end: generator values rv, transcendentals ra0 / ra1, bound multipliers zl / zu and
// inverse slack distances idl / idu of the accepted iterate; w.V holds the iterate, w.cst the (scaled) weights and the
// effective goal
template <int N, int KSM, int RPL, bool OB = false>
__device__ __forceinline__ void sens_epilogue(const KP& P, const WSS<N, double>& w, const double* G, long long b, int lane,
                                              bool valid, const int (&rtype)[RPL], const int (&rk)[RPL],
                                              const int (&roi)[RPL], const double (&rv)[RPL][4], const double (&ra0)[RPL],
                                              const double (&ra1)[RPL], const double (&zl)[RPL], const double (&zu)[RPL],
                                              const double (&idl)[RPL], const double (&idu)[RPL], int mo4, int rps, int nobs,
                                              int modi)
{
    using R = double;
    using D = Dim<N>;
    constexpr int n = D::n, NCP = D::NCP, NG = D::NG, KLD = D::KLD, NR = SENS_COLS;
    static_assert(D::NT == 1 && n <= ALIP_GJ_MAX_N && n <= 16, "the gj_regs domain: n <= 15");
    static_assert(16 * 8 <= 64 * (N + 1), "R and dp (16 x 8) fit the Hessian-block buffer");
    if (!valid) {
        sens_invalid<N, OB>(P, b, lane);
        return;
    }
    const int g4 = lane >> 4, col = lane & 15;
    const RowK<R> C = load_rowk(w.cst);
    // ---- row layout: coefficients, y and Sigma at the accepted iterate, as a direction phase computes them
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = lane + WAVE * q;
        R o[6], cf[4], hx[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = w.obs6[6 * roi[q] + i];
        row_coef(rtype[q], rk[q], rv[q], ra0[q], ra1[q], o, C, cf, hx);
        if (r < mo4) {
            st4(w.rcoef + 4 * r, cf[0], cf[1], cf[2], cf[3]);
            w.ry[r] = rtype[q] == R_OBJ ? -R(1.0) : zl[q] - zu[q];
            w.rsig[r] = zl[q] * idl[q] + zu[q] * idu[q];
        }
        if (rtype[q] == R_VBX) {
            w.CT[rk[q] + 1] = ra1[q];
            w.ST[rk[q] + 1] = ra0[q];
        }
        if (rtype[q] == R_OBJ) {
#pragma unroll
            for (int i = 0; i < 6; ++i) w.hobj[6 * rk[q] + i] = hx[i];
        }
    }
    wave_sync();
    if constexpr (16 * (N + 1) <= WAVE)
        hess_blocks_lanes<N, R>(w, lane, rps, nobs, modi);
    else
        hess_blocks<N, R>(w, lane, rps, nobs, modi);
    wave_sync();
    // ---- the rows' part J^T Sigma [J | C E] in double-double (above): lane (g4, col) sums rows r = 4 s + g4 into row
    // `col` of K and of the 5 state columns (the constraints do not see the goal), then the 4 groups are added
    R kh[n], kl[n], rh[5], rl[5];
#pragma unroll
    for (int j = 0; j < n; ++j) kh[j] = kl[j] = R(0.0);
#pragma unroll
    for (int c = 0; c < 5; ++c) rh[c] = rl[c] = R(0.0);
    const int ce = col < 5 ? col : 0;
    const R em = col < 5 ? R(1.0) : R(0.0);
#pragma unroll 2
    for (int s = 0; s < KSM; ++s) {
        const int r = 4 * s + g4;
        const uint32_t pk = w.rgen[r];
        R c0, c1, c2, c3;
        ld4(w.rcoef + 4 * r, c0, c1, c2, c3);
        const R sq = sqrt(w.rsig[r]);   // padding / OBJ rows: sigma = 0
        const int t0 = gen_i(pk, 0), t1 = gen_i(pk, 1), t2 = gen_i(pk, 2), t3 = gen_i(pk, 3);
        const R j = c0 * G[t0 * NCP + col] + c1 * G[t1 * NCP + col] + c2 * G[t2 * NCP + col] + c3 * G[t3 * NCP + col];
        const R je = em * (c0 * P.E[t0 * 5 + ce] + c1 * P.E[t1 * 5 + ce] + c2 * P.E[t2 * 5 + ce] + c3 * P.E[t3 * 5 + ce]);
        const R bj = sq * j, be = sq * je;
        sens_acc_row<0, n>(bj, kh, kl);
        sens_acc_rhs<0, 5>(bj, be, rh, rl);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) {
        const dd2 t = dd_gsum(dd2{kh[j], kl[j]});
        kh[j] = t.h;
        kl[j] = t.l;
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const dd2 t = dd_gsum(dd2{rh[c], rl[c]});
        rh[c] = t.h;
        rl[c] = t.l;
    }
    // ---- the Hessian part G^T S G and G^T (S E | -S_obj[:, pos]) by f64 MFMA: the B operand of R's chain is column
    // `col` of the 7 right-hand sides (lanes with col >= 7 feed zeros)
    {
        d4 aK[2], aR[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) aK[h] = aR[h] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 1; s < NG / 4; ++s) {
            const int t = 4 * s + g4;
            const int kb = t >> 3, c = t & 7;
            const R* Srow = w.S + 64 * kb + 8 * c;
            const R gv = G[t * NCP + col];
            R sgv = R(0.0), sev = R(0.0);
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) {
                sgv += Srow[c2] * G[(8 * kb + c2) * NCP + col];
                sev += Srow[c2] * P.E[(8 * kb + c2) * 5 + ce];
            }
            sev *= em;
            if (col >= 5 && col < NR && kb >= 1) {
                // goal column col - 5: minus the objective's own second derivatives on (px, py) of x_kb
                // (hobj = [h00 h01 h11 h04 h14 h44]; generator rows 0, 1, 4 of the block)
                const R* ho = w.hobj + 6 * kb;
                const int gc = col - 5;
                R v = R(0.0);
                v = c == 0 ? (gc == 0 ? ho[0] : ho[1]) : v;
                v = c == 1 ? (gc == 0 ? ho[1] : ho[2]) : v;
                v = c == 4 ? (gc == 0 ? ho[3] : ho[4]) : v;
                sev = -v;
            }
            aK[s & 1] = Mfma<R>::run(gv, sgv, aK[s & 1]);
            aR[s & 1] = Mfma<R>::run(gv, sev, aR[s & 1]);
        }
        wave_sync();   // (every read of S precedes the writes of R into its buffer)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = Mfma<R>::row(g4, i);
            w.K[row * KLD + col] = aK[0][i] + aK[1][i];
            if (col < 8) w.S[row * 8 + col] = aR[0][i] + aR[1][i];
        }
    }
    wave_sync();
    // ---- rows of [K | R] in registers; the detour's chain rule on the goal columns
    // (every 16-lane row holds the rows' part of row `col`; lanes 0 .. n - 1 are the elimination's rows)
    R a[n + NR], al[n + NR];
#pragma unroll
    for (int j = 0; j < n; ++j) {
        const dd2 t = dd_add(dd2{kh[j], kl[j]}, dd2{w.K[col * KLD + j], R(0.0)});
        a[j] = t.h;
        al[j] = t.l;
    }
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        a[n + c] = w.S[col * 8 + c];
        al[n + c] = R(0.0);
    }
    {
        const R x0x = P.x0[5 * b], x0y = P.x0[5 * b + 1], g0 = P.goal[2 * b], g1 = P.goal[2 * b + 1];
        const R gxg = w.cst[K_GXG], gyg = w.cst[K_GYG];
        if (P.detour && (gxg != g0 || gyg != g1)) {   // (wave-uniform) the detour fired: which side, from the turn taken
            const R cross = (g0 - x0x) * (gyg - x0y) - (g1 - x0y) * (gxg - x0x);
            const R cs = R(0.9659258262890683), sn = cross > R(0.0) ? R(0.25881904510252074) : R(-0.25881904510252074);
            const R r5 = a[n + 5], r6 = a[n + 6];
            const R t5 = r5 * cs + r6 * sn, t6 = r6 * cs - r5 * sn;   // [r5 r6] Rot
            a[n + 0] += r5 - t5;                                       // [r5 r6] (I - Rot) on x0's position
            a[n + 1] += r6 - t6;
            a[n + 5] = t5;
            a[n + 6] = t6;
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const dd2 t = dd_add(dd2{rh[c], rl[c]}, dd2{a[n + c], R(0.0)});
        a[n + c] = t.h;
        al[n + c] = t.l;
    }
    wave_sync();
    if (!gj_regs_m<n, NR>(a, al, lane)) {   // a pivot <= 0 at delta = 0: no regularisation, the sensitivity is invalid
        sens_invalid<N, OB>(P, b, lane);
        return;
    }
    // ---- dp / dtheta = -K^-1 R; dfoot = its rows of p_0; du = E + G dp on the rows of x_1 .. x_N
    if (lane < n) {
#pragma unroll
        for (int c = 0; c < NR; ++c) w.S[lane * 8 + c] = -a[n + c];
    }
    if (lane < 3 && (!OB || sens_dfoot(P))) {
#pragma unroll
        for (int c = 0; c < NR; ++c) sens_dfoot(P)[((size_t)b * 3 + lane) * NR + c] = -a[n + c];
    }
    wave_sync();
    if (sens_du(P)) {
        for (int l = lane; l < 5 * N; l += WAVE) {
            const int t = gx(l / 5 + 1, l % 5);
            R v[NR];
#pragma unroll
            for (int c = 0; c < NR; ++c) v[c] = c < 5 ? P.E[t * 5 + c] : R(0.0);
            for (int j = 0; j < n; ++j) {
                const R g = G[t * NCP + j];
#pragma unroll
                for (int c = 0; c < NR; ++c) v[c] = fma(g, w.S[j * 8 + c], v[c]);
            }
#pragma unroll
            for (int c = 0; c < NR; ++c) sens_du(P)[((size_t)b * 5 * N + l) * NR + c] = v[c];
        }
    }
    if (sens_okp(P) && lane == 0) sens_okp(P)[b] = 1;
    wave_sync();
    if constexpr (OB) sens_obs_columns<N>(P, w, G, b, lane, kh, kl, rps);
}
