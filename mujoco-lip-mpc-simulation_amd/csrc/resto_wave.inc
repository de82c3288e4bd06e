// IPOPT's feasibility restoration phase for the wave program (cfg.restoration = ALIPMPC_RESTORATION_IPOPT; included
// by alipmpc.hip ahead of solve_one).  Restated from Wächter & Biegler 2006 §3.3 and IPOPT's MinC_1NrmRestorationPhase
// defaults (version unpinned; the reference's cyipopt ran it whenever a filter line search failed,
// MPC_LIP_modi.py:274-296); the same algorithm as np_oracle._resto / alipmpc_oracle.c oresto, step for step:
//
//   min  rho sum(p + n) + zeta/2 sum_j D_j^2 (x_j - xR_j)^2   s.t.  c(x) - p + n - s = 0,  cl <= s <= cu,  p, n >= 0
//
// x = the footholds (the solve's variables), x_R the iterate where the line search failed, D_j = 1 / max(1, |xR_j|),
// rho = 1000, zeta = sqrt(mu) of the restoration's own barrier parameter (from max(mu, |c - s|_inf)).  p, n start at
// the minimiser of rho (p + n) - mu (ln p + ln n) on p - n = c - s (IPOPT eq. 33), their multipliers at mu / p, mu / n,
// the slack multipliers at min(rho, current), y at 0.  Per restoration iteration (the same wave layout as solve_one:
// lane r = row r, J layout for J^T y and the MFMA products): the restoration's own error and barrier update; the
// condensed Newton system (W_c + zeta D^2 + J^T diag(1 / (1/S_p + 1/S_n + 1/S_s)) J) dx = -g + J^T (y + b / D) with
// W_c the constraint part of the Hessian blocks (objective rows carry y = 0); the steps of y, p, n, s and their
// multipliers row by row; fraction to the boundary; a filter line search of its own on theta = sum |c - p + n - s| and
// phi = rho sum(p + n) + zeta/2 |D (x - xR)|^2 - mu sum ln(p n dl du).  Before each iteration after the first the
// ORIGINAL problem is tested: an iterate whose violation sum |c - s| is <= 0.9 theta_R and that the original filter
// (augmented with the failed point by the caller) accepts ends the phase.
//
// Interface (inlined into the restoration-capable build of solve_one, RS = true, at the top of the iteration after a
// failed line search; the lean build that phase 1 of a split launch runs never contains it): in — the workspace holds
// the iterate (w.V); the caller's row registers, by reference, hold everything else at the failed point: the row
// descriptors and bounds, the rows' generator values, sin / cos and values, the slacks and the slack multipliers
// zl / zu (nothing is decoded or evaluated again here, and nothing but the iterate goes through LDS); the original
// filter entries (two per lane), their count, the regular barrier parameter, theta_R and the iteration count.  Out —
// w.V holds the new iterate, the same registers the rows, slacks and multipliers at it; the return value is
// (it << 4) | code:
//   RS_OK_ORIG     back to the regular phase through the original-problem check (multipliers: the complementarity
//                  Newton step over the restoration's whole slack change, reset to 1 above bound_mult_reset_threshold
//                  = 1000).  The row values are the accepted trial's at the returned iterate, and lsum_o / f_o the
//                  barrier sum and objective the check computed there: the caller evaluates nothing again
//   RS_OK          back to the regular phase from a converged restoration problem whose original violation is below
//                  1e-4 (the caller re-evaluates the rows, as for the codes below)
//   RS_INFEASIBLE  the restoration problem converged (error <= tol) with the original violation above 1e-4: IPOPT's
//                  Infeasible_Problem_Detected (status 2), the restoration iterate returned
//   RS_MAXITER     the iteration cap inside the phase (its current iterate returned)
//   RS_FAILED      the restoration's own factorisation or line search failed (status 2)
enum { RSW_OK = 0, RSW_INFEASIBLE = 1, RSW_MAXITER = 2, RSW_FAILED = 3, RSW_OK_ORIG = 4 };

template <int N, int KSM, class R, int RPL>
__device__ __forceinline__ int resto_wave(int wv, R fth0, R fph0, R fth1, R fph1, int nfo, R mu_o, R theta_R, int it,
                                          int (&rtype)[RPL], int (&rk)[RPL], int (&roi)[RPL], uint32_t (&rg)[RPL],
                                          R (&cl)[RPL], R (&cu)[RPL], R (&rv)[RPL][4], R (&ra0)[RPL], R (&ra1)[RPL],
                                          R (&cr)[RPL], R (&sr)[RPL], R (&zl0)[RPL], R (&zu0)[RPL], R& lsum_o, R& f_o)
{
    static_assert(RPL == (4 * KSM + WAVE - 1) / WAVE, "one row group per 64 rows");
    using D = Dim<N>;
    constexpr int n = D::n;
    constexpr int NT = D::NT;
    constexpr int NCP = D::NCP;
    constexpr int NG = D::NG;
    constexpr int KLD = D::KLD;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const KP& P = *reinterpret_cast<const KP*>(smem);
    const R* G = reinterpret_cast<const R*>(smem + KP_DOUBLES);
    R* wsb = const_cast<R*>(G) + NG * NCP;
    int lane = lane_id();
    RSTAMP_DECL
    const int mr4 = rfl(P.mr4), mo4 = rfl(P.mo4), rps = rfl(P.rps);
    const int nc_max = rfl(P.nc_max), ne_max = rfl(P.ne_max), nobs = nc_max + ne_max;
    const int modi = rfl(P.modi), max_iter = rfl(P.max_iter);
    WSS<N, R> w = carve_s<N, R>(wsb + (size_t)wv * wss_elems<N, R>(nc_max, ne_max, mr4, mo4), nc_max, ne_max, mr4, mo4);
    const R rho = R(1000.0), tol = w.cst[K_TOL];
    const R gth = R(1e-5), gph = R(1e-8), sth = R(1.1), sph = R(2.3), eta = R(1e-8), gal = R(0.05);
    int g4 = lane >> 4, col = lane & 15;
    // lane-derived values re-derived at each section (as solve_one's RELANE): hoisted, the per-lane LDS addresses and
    // row descriptors stay live across the whole kernel and are spilled
#define RS_RELANE()                                                                                               \
    do {                                                                                                          \
        RELAUNDER(lane);                                                                                          \
        g4 = lane >> 4;                                                                                           \
        col = lane & 15;                                                                                          \
        for (int q_ = 0; q_ < RPL; ++q_) {                                                                        \
            RELAUNDER(rtype[q_]);                                                                                 \
            RELAUNDER(rk[q_]);                                                                                    \
            RELAUNDER(roi[q_]);                                                                                   \
            RELAUNDER(rg[q_]);                                                                                    \
            RELAUNDER(cl[q_]);                                                                                    \
            RELAUNDER(cu[q_]);                                                                                    \
        }                                                                                                         \
    } while (0)
#define RCK load_rowk(w.cst)
    // ---- the restoration's start: the rows are the caller's own registers (descriptors, bounds, generator values,
    // sin / cos, row values, slacks and slack multipliers at the failed point: rows without a constraint carry
    // s = zl = zu = 0 and infinite bounds there)
    R rdv[RPL][4];
    R vl[RPL], vu[RPL], pp[RPL], nn[RPL], zp[RPL], zn[RPL], yv[RPL], s0[RPL];
    // active rows and bounds are the instance's constants: sum over the active rows of 2 + (cl finite) + (cu finite) =
    // 2 K_MACT + K_NBL (the caller's counts: small integers, exact)
    const R mal = w.cst[K_MACT], nbl = R(2) * mal + w.cst[K_NBL];
    R mu = mu_o;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        s0[q] = sr[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) rdv[q][i] = R(0);
        if (rtype[q] < R_NONE) mu = fmax(mu, fabs(cr[q] - sr[q]));
    }
    mu = wmax(mu);
    // x_R and the proximity weights D_j^2 (lane j < n: foothold j = 3k + c at V[gp(k, c)])
    const R xR = lane < n ? w.V[gp(lane / 3, lane % 3)] : R(0);
    const R d2 = lane < n ? R(1) / (fmax(R(1), fabs(xR)) * fmax(R(1), fabs(xR))) : R(0);
    R th0 = R(0);
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const bool isc = rtype[q] < R_NONE;
        const R r_ = cr[q] - sr[q];
        const R a = (mu - rho * r_) / (R(2) * rho);
        const R sq = sqrt(a * a + mu * r_ / (R(2) * rho));
        const R nv = a >= R(0) ? a + sq : (mu * r_ / (R(2) * rho)) / (sq - a);
        nn[q] = isc ? nv : R(1);
        pp[q] = isc ? r_ + nv : R(1);
        zp[q] = isc ? mu / pp[q] : R(0);
        zn[q] = isc ? mu / nn[q] : R(0);
        vl[q] = isc && isfinite(cl[q]) ? fmin(rho, zl0[q]) : R(0);
        vu[q] = isc && isfinite(cu[q]) ? fmin(rho, zu0[q]) : R(0);
        yv[q] = R(0);
        if (isc) th0 += fabs(cr[q] - pp[q] + nn[q] - sr[q]);
    }
    th0 = wsum(th0);
    const R theta_max = R(1e4) * fmax(R(1), th0), theta_min = R(1e-4) * fmax(R(1), th0);
    R rft0 = INFINITY, rfp0 = INFINITY, rft1 = INFINITY, rfp1 = INFINITY;   // the restoration's own filter
    int nfr = 0;
    R dw_last = R(0);
    int code = RSW_OK;
    bool first = true;
    const int it_in = it;
    RSTAMP(0);
    for (;;) {
        RS_RELANE();
        R xc = lane < n ? w.V[gp(lane / 3, lane % 3)] : R(0);   // current footholds (lane j)
        if (!first) {
            // ---- progress on the ORIGINAL problem (RestoConvergenceCheck): violation reduced to kappa_resto theta_R
            // and acceptable to the original filter with the original barrier function
            // (the violation decides first: the barrier sum, one log per row, only for an iterate it lets through)
            R tho = R(0);
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                if (rtype[q] < R_NONE) tho += fabs(cr[q] - sr[q]);
            tho = wsum(tho);
            bool acc = tho <= R(0.9) * theta_R;
            if (acc) {
                R lso = R(0);
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const R d1 = sr[q] - cl[q], d2_ = cu[q] - sr[q];
                    lso += llog(isfinite(cl[q]) ? (isfinite(cu[q]) ? d1 * d2_ : d1) : (isfinite(cu[q]) ? d2_ : R(1.0)));
                }
                lso = wsum(lso);
                const R fo = obj_sum<N, RPL>(cr, mr4);
                const R pho = fo - mu_o * lso;
                lsum_o = lso;
                f_o = fo;
                acc = isfinite(pho);
                if (acc) {
                    const bool b0 = lane < nfo && !(tho < fth0 || pho < fph0);
                    const bool b1 = lane + WAVE < nfo && !(tho < fth1 || pho < fph1);
                    acc = __ballot(b0 || b1) == 0ull;
                }
            }
            if (acc) {
                // slack multipliers: the complementarity Newton step over the whole restoration (fraction to the
                // boundary), all reset to 1 when one exceeds bound_mult_reset_threshold
                const R tau = uni(fmax(R(0.99), R(1) - mu_o));
                R dzl[RPL], dzu[RPL], ad = R(1);
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const bool hl = rtype[q] < R_NONE && isfinite(cl[q]), hu = rtype[q] < R_NONE && isfinite(cu[q]);
                    const R e1 = s0[q] - cl[q], e2 = cu[q] - s0[q];
                    dzl[q] = hl ? mu_o / e1 - zl0[q] - zl0[q] / e1 * (sr[q] - s0[q]) : R(0);
                    dzu[q] = hu ? mu_o / e2 - zu0[q] + zu0[q] / e2 * (sr[q] - s0[q]) : R(0);
                    if (hl && dzl[q] < R(0)) ad = fmin(ad, -tau * zl0[q] / dzl[q]);
                    if (hu && dzu[q] < R(0)) ad = fmin(ad, -tau * zu0[q] / dzu[q]);
                }
                ad = wmin(ad);
                R zmax = R(0);
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    zl0[q] += ad * dzl[q];
                    zu0[q] += ad * dzu[q];
                    zmax = fmax(zmax, fmax(zl0[q], zu0[q]));
                }
                zmax = wmax(zmax);
                if (zmax > R(1000)) {
#pragma unroll
                    for (int q = 0; q < RPL; ++q) {
                        zl0[q] = rtype[q] < R_NONE && isfinite(cl[q]) ? R(1) : R(0);
                        zu0[q] = rtype[q] < R_NONE && isfinite(cu[q]) ? R(1) : R(0);
                    }
                }
                code = RSW_OK_ORIG;
                break;
            }
        }
        first = false;
        RSTAMP(1);
        // ---- row layout: generator-form coefficients, y (objective rows: 0), the velocity rows' sin / cos
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = lane + WAVE * q;
            R o[6], cf[4], hx[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = w.obs6[6 * roi[q] + i];
            row_coef(rtype[q], rk[q], rv[q], ra0[q], ra1[q], o, RCK, cf, hx);
            if (r < mo4) {
                const bool isc = rtype[q] < R_NONE;
                st4(w.rcoef + 4 * r, isc ? cf[0] : R(0), isc ? cf[1] : R(0), isc ? cf[2] : R(0), isc ? cf[3] : R(0));
                w.ry[r] = isc ? yv[q] : R(0);
            }
            if (rtype[q] == R_VBX) {
                w.CT[rk[q] + 1] = ra1[q];
                w.ST[rk[q] + 1] = ra0[q];
            }
            if (rtype[q] == R_OBJ) {
#pragma unroll
                for (int i = 0; i < 6; ++i) w.hobj[6 * rk[q] + i] = R(0);
            }
        }
        wave_sync();
        // ---- J layout: gl = J^T y (the J tile kept in registers for the MFMA product, as solve_one's JC: the
        // product below then reads no G from LDS)
        constexpr bool JCR = KSM * NT <= 16;
        R jv[JCR ? KSM : 1][NT];
        R gl[NT];
#pragma unroll
        for (int T = 0; T < NT; ++T) gl[T] = R(0);
#pragma unroll
        for (int s = 0; s < KSM; ++s) {
            const int r = 4 * s + g4;
            const uint32_t pk = w.rgen[r];
            R ca0, ca1, cb0, cb1;
            ld4(w.rcoef + 4 * r, ca0, ca1, cb0, cb1);
            const R y = w.ry[r];
#pragma unroll
            for (int T = 0; T < NT; ++T) {
                const int cc = 16 * T + col;
                const R j = ca0 * G[gen_i(pk, 0) * NCP + cc] + ca1 * G[gen_i(pk, 1) * NCP + cc] +
                            cb0 * G[gen_i(pk, 2) * NCP + cc] + cb1 * G[gen_i(pk, 3) * NCP + cc];
                if constexpr (JCR) jv[JCR ? s : 0][T] = j;
                gl[T] += j * y;
            }
        }
#pragma unroll
        for (int T = 0; T < NT; ++T) gl[T] = gsum(gl[T]);
        R glme = gl[0];
#pragma unroll
        for (int T = 1; T < NT; ++T) glme = (lane >> 4) == T ? gl[T] : glme;   // lane j: (J^T y)_j
        RSTAMP(2);
        // ---- the restoration's error and barrier update
        R zeta = uni(sqrt(mu));
        R gxv = lane < n ? zeta * d2 * (xc - xR) - glme : R(0);
        R dual = fabs(gxv), prim = R(0), nz = R(0), ny = R(0), whi = -INFINITY, wlo = INFINITY;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            if (rtype[q] < R_NONE) {
                const R dl = sr[q] - cl[q], du = cu[q] - sr[q];
                dual = fmax(dual, fmax(fabs(rho + yv[q] - zp[q]), fabs(rho - yv[q] - zn[q])));
                dual = fmax(dual, fabs(yv[q] - vl[q] + vu[q]));
                prim = fmax(prim, fabs(cr[q] - pp[q] + nn[q] - sr[q]));
                ny += fabs(yv[q]);
                nz += fabs(zp[q]) + fabs(zn[q]) + fabs(vl[q]) + fabs(vu[q]);
                whi = fmax(whi, fmax(pp[q] * zp[q], nn[q] * zn[q]));
                wlo = fmin(wlo, fmin(pp[q] * zp[q], nn[q] * zn[q]));
                if (isfinite(cl[q])) {
                    whi = fmax(whi, dl * vl[q]);
                    wlo = fmin(wlo, dl * vl[q]);
                }
                if (isfinite(cu[q])) {
                    whi = fmax(whi, du * vu[q]);
                    wlo = fmin(wlo, du * vu[q]);
                }
            }
        }
        wsum_pair(nz, ny);
        wmax_pair(dual, prim);
        wmaxmin_pair(whi, wlo);
        const R sd = uni(fmax(R(100), (nz + ny) / (R(n) + mal * R(3))) / R(100));
        const R sc = uni(fmax(R(100), nz / fmax(R(1), nbl)) / R(100));
        const R base = fmax(dual / sd, prim);
        const R e0 = uni(fmax(base, fmax(fabs(whi), fabs(wlo)) / sc));
        if (e0 <= tol) {
            R viol = R(0);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = lane + WAVE * q;
                if (r < mr4 && rtype[q] < R_NONE) {
                    if (isfinite(cl[q])) viol = fmax(viol, w.rclo[r] - cr[q]);
                    if (isfinite(cu[q])) viol = fmax(viol, cr[q] - w.rcuo[r]);
                }
            }
            viol = wmax(viol);
            code = viol > R(1e-4) ? RSW_INFEASIBLE : RSW_OK;
            break;
        }
        if (it >= max_iter) {
            code = RSW_MAXITER;
            break;
        }
        const R mu_prev = mu;
        for (int t = 0; t < 8; ++t) {
            const R cm = fmax(fabs(whi - mu), fabs(wlo - mu));
            if (fmax(base, cm / sc) <= R(10) * mu && mu > tol / R(11))
                mu = uni(fmax(tol / R(11), fmin(R(0.2) * mu, mu * sqrt(mu))));
            else
                break;
        }
        if (mu != mu_prev) {
            nfr = 0;
            zeta = uni(sqrt(mu));
            gxv = lane < n ? zeta * d2 * (xc - xR) - glme : R(0);
        }
        const R tau = uni(fmax(R(0.99), R(1) - mu));
        RSTAMP(3);
        // ---- condensed system weights per row: 1 / D, and the rhs weight y + b / D
        // (reciprocals with one Newton step, rcp_nr, as the regular loop; per row kept for the step pass: the inverse
        // weights 1 / S_p, 1 / S_n, 1 / S_s, 1 / D and b, and the reciprocals 1 / p, 1 / n, 1 / dl, 1 / du)
        R iD[RPL], bv[RPL], iSp[RPL], iSn[RPL], iSs[RPL], ipv[RPL], inv[RPL], idl_[RPL], idu_[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = lane + WAVE * q;
            const bool isc = rtype[q] < R_NONE;
            const R dl = sr[q] - cl[q], du = cu[q] - sr[q];
            ipv[q] = rcp_nr(pp[q]);
            inv[q] = rcp_nr(nn[q]);
            idl_[q] = isfinite(cl[q]) ? rcp_nr(dl) : R(0);
            idu_[q] = isfinite(cu[q]) ? rcp_nr(du) : R(0);
            iSp[q] = isc ? pp[q] * rcp_nr(zp[q]) : R(0);
            iSn[q] = isc ? nn[q] * rcp_nr(zn[q]) : R(0);
            iSs[q] = isc ? rcp_nr(vl[q] * idl_[q] + vu[q] * idu_[q]) : R(0);
            const R mdl = mu * idl_[q], mdu = mu * idu_[q];
            const R rc = cr[q] - pp[q] + nn[q] - sr[q];
            iD[q] = isc ? rcp_nr(iSp[q] + iSn[q] + iSs[q]) : R(0);
            bv[q] = isc ? -rc + (-rho - yv[q] + mu * ipv[q]) * iSp[q] - (-rho + yv[q] + mu * inv[q]) * iSn[q] +
                              (-yv[q] + mdl - mdu) * iSs[q]
                        : R(0);
            if (r < mo4) {
                w.rsig[r] = iD[q];
                w.rw[r] = isc ? yv[q] + bv[q] * iD[q] : R(0);
            }
        }
        wave_sync();
        RS_RELANE();
        RSTAMP(4);
        if constexpr (16 * (N + 1) <= WAVE)
            hess_blocks_lanes<N, R>(w, lane, rps, nobs, modi);
        else
            hess_blocks<N, R>(w, lane, rps, nobs, modi);
        wave_sync();
        RS_RELANE();
        RSTAMP(5);
        // ---- K = J^T diag(1/D) J + G^T S G (MFMA), rhs = J^T (y + b / D)
        R rhsc[NT];
        {
            constexpr int NA = NT * (NT + 1) / 2;
            typename Mfma<R>::acc acc[2][NA];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < NA; ++i) acc[h][i] = typename Mfma<R>::acc{R(0), R(0), R(0), R(0)};
            R pw[NT];
#pragma unroll
            for (int T = 0; T < NT; ++T) pw[T] = R(0);
#pragma unroll
            for (int s = 0; s < KSM; ++s) {
                const int r = 4 * s + g4;
                const R sg = w.rsig[r], wr = w.rw[r];
                R j[NT];
                if constexpr (JCR) {
#pragma unroll
                    for (int T = 0; T < NT; ++T) j[T] = jv[JCR ? s : 0][T];
                } else {
                    const uint32_t pk = w.rgen[r];
                    R ca0, ca1, cb0, cb1;
                    ld4(w.rcoef + 4 * r, ca0, ca1, cb0, cb1);
#pragma unroll
                    for (int T = 0; T < NT; ++T) {
                        const int cc = 16 * T + col;
                        j[T] = ca0 * G[gen_i(pk, 0) * NCP + cc] + ca1 * G[gen_i(pk, 1) * NCP + cc] +
                               cb0 * G[gen_i(pk, 2) * NCP + cc] + cb1 * G[gen_i(pk, 3) * NCP + cc];
                    }
                }
#pragma unroll
                for (int T = 0; T < NT; ++T) pw[T] += j[T] * wr;
                auto* a = acc[s & 1];
                a[0] = Mfma<R>::run(j[0], sg * j[0], a[0]);
                if constexpr (NT == 2) {
                    a[1] = Mfma<R>::run(j[0], sg * j[1], a[1]);
                    a[2] = Mfma<R>::run(j[1], sg * j[1], a[2]);
                }
            }
#pragma unroll
            for (int s = 1; s < NG / 4; ++s) {
                const int t = 4 * s + g4;
                const int kb = t >> 3;
                const R* Srow = w.S + 64 * kb + 8 * (t & 7);
                const R* Gb = G + 8 * kb * NCP;
                R gv[NT], sgv[NT];
                // (hess_blocks' zero columns of S skipped, as solve_one: +0 terms, the same sums)
                const unsigned SCOLS = (s & 1) ? 0x7Fu : 0x73u;
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    gv[T] = G[t * NCP + 16 * T + col];
                    R a = R(0);
#pragma unroll
                    for (int c2 = 0; c2 < 8; ++c2)
                        if ((SCOLS >> c2) & 1u) a += Srow[c2] * Gb[c2 * NCP + 16 * T + col];
                    sgv[T] = a;
                }
                auto* a = acc[s & 1];
                a[0] = Mfma<R>::run(gv[0], sgv[0], a[0]);
                if constexpr (NT == 2) {
                    a[1] = Mfma<R>::run(gv[0], sgv[1], a[1]);
                    a[2] = Mfma<R>::run(gv[1], sgv[1], a[2]);
                }
            }
#pragma unroll
            for (int T = 0; T < NT; ++T) rhsc[T] = gsum(pw[T]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = Mfma<R>::row(g4, i);
                w.K[row * KLD + col] = acc[0][0][i] + acc[1][0][i];
                if constexpr (NT == 2) {
                    const R k1 = acc[0][1][i] + acc[1][1][i];
                    w.K[row * KLD + 16 + col] = k1;
                    w.K[(16 + col) * KLD + row] = k1;
                    w.K[(16 + row) * KLD + 16 + col] = acc[0][2][i] + acc[1][2][i];
                }
            }
        }
        wave_sync();
        // the proximity term on the diagonal; rhs = -zeta D^2 (x - xR) + J^T (y + b / D)
        if (lane < n) w.K[lane * KLD + lane] += zeta * d2;
        wave_sync();
        R rhs_l = R(0);
#pragma unroll
        for (int T = 0; T < NT; ++T) rhs_l = (lane < n && (lane >> 4) == T) ? rhsc[T] : rhs_l;
        rhs_l = lane < n ? rhs_l - zeta * d2 * (xc - xR) : R(0);
        RSTAMP(6);
        // ---- register Cholesky with inertia correction, forward / backward sweeps
        R xv;
        if constexpr (n <= ALIP_GJ_MAX_N) {
            // Gauss-Jordan on register rows (gj_regs), as the regular loop
            R a[n + 1];
            auto fill = [&](R dw) {
#pragma unroll
                for (int j = 0; j < n; ++j) a[j] = (lane < n ? w.K[lane * KLD + j] : R(0)) + (lane == j ? dw : R(0));
                a[n] = rhs_l + R(0);
            };
            // (one loop, one inlined elimination: dw = 0 first, then the correction's sequence)
            R dw = R(0);
            bool ok;
            for (;;) {
                fill(dw);
                ok = gj_regs<n, R, gj_rb<RPL>>(a, lane);
                if (ok) break;
                if (dw == R(0)) {
                    dw = dw_last == R(0) ? R(1e-4) : fmax(R(1e-20), dw_last / R(3));
                } else {
                    dw *= dw_last == R(0) ? R(100) : R(8);
                    if (dw > R(sizeof(R) == 8 ? 1e40 : 1e30)) break;
                }
            }
            if (dw != R(0)) dw_last = uni(dw);
            if (!ok) {
                code = RSW_FAILED;
                break;
            }
            xv = lane < n ? a[n] : R(0);
        } else {
            R a[n];
            R myidg = R(1);
            R dw = R(0);
            bool ok;
            for (;;) {
#pragma unroll
                for (int j = 0; j < n; ++j) {
                    const R kv = lane < n ? w.K[lane * KLD + j] : (lane == j ? R(1) : R(0));
                    a[j] = dw == R(0) ? kv : kv + (lane == j ? dw : R(0));   // (the first try adds nothing, not + 0)
                }
                ok = chol_rows<n>(a, myidg, lane);
                if (ok) break;
                if (dw == R(0)) {
                    dw = dw_last == R(0) ? R(1e-4) : fmax(R(1e-20), dw_last / R(3));
                } else {
                    dw *= dw_last == R(0) ? R(100) : R(8);
                    if (dw > R(sizeof(R) == 8 ? 1e40 : 1e30)) break;
                }
            }
            if (dw != R(0)) dw_last = uni(dw);
            if (!ok) {
                code = RSW_FAILED;
                break;
            }
            R acc = R(0), yy = R(0);
#pragma unroll
            for (int k = 0; k < n; ++k) {
                const R yk = bcast((rhs_l - acc) * myidg, k);
                yy = lane == k ? yk : yy;
                acc += lane > k ? a[k] * yk : R(0);
            }
            wave_sync();
            if (lane < n) {
#pragma unroll
                for (int j = 0; j < n; ++j) w.K[lane * KLD + j] = j <= lane ? a[j] : R(0);
            }
            wave_sync();
            acc = R(0);
            xv = R(0);
#pragma unroll
            for (int i = n - 1; i >= 0; --i) {
                const R xi = bcast((yy - acc) * myidg, i);
                xv = lane == i ? xi : xv;
                acc += lane < i ? w.K[i * KLD + (lane & 31)] * xi : R(0);
            }
        }
        RS_RELANE();
        RSTAMP(7);
        // ---- dV = G dx; the rows' steps
        {
            R v = R(0);
            if constexpr (dp_rows<n, NG, R>) {   // (as the regular loop)
                v = gdp_rows<n, NCP>(G, xv, lane < NG ? lane : 0);
            } else {
#pragma unroll
                for (int j = 0; j < n; ++j) v += G[(lane < NG ? lane : 0) * NCP + j] * bcast(xv, j);
            }
            if (lane < NG) w.dV[lane] = v;
        }
        wave_sync();
        R dy[RPL], dpv[RPL], dnv[RPL], ds[RPL], dzp[RPL], dzn[RPL], dvl[RPL], dvu[RPL];
        R ap = R(1), az = R(1), theta = R(0), lin = R(0), gpn = R(0);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = lane + WAVE * q;
#pragma unroll
            for (int i = 0; i < 4; ++i) rdv[q][i] = w.dV[gen_i(rg[q], i)];
            R jd = R(0);
            if (r < mo4) {
                R ca0, ca1, cb0, cb1;
                ld4(w.rcoef + 4 * r, ca0, ca1, cb0, cb1);
                jd = ca0 * rdv[q][0] + ca1 * rdv[q][1] + cb0 * rdv[q][2] + cb1 * rdv[q][3];
            }
            const bool isc = rtype[q] < R_NONE, hl = isc && isfinite(cl[q]), hu = isc && isfinite(cu[q]);
            const R dl = sr[q] - cl[q], du = cu[q] - sr[q];
            // (1 / p, 1 / n, 1 / dl, 1 / du: the weights pass's, their arguments unchanged since)
            const R mdl = mu * idl_[q], mdu = mu * idu_[q];
            dy[q] = isc ? (bv[q] - jd) * iD[q] : R(0);
            dpv[q] = isc ? (-rho - yv[q] + mu * ipv[q] - dy[q]) * iSp[q] : R(0);
            dnv[q] = isc ? (-rho + yv[q] + mu * inv[q] + dy[q]) * iSn[q] : R(0);
            ds[q] = isc ? (-yv[q] + mdl - mdu - dy[q]) * iSs[q] : R(0);
            dzp[q] = isc ? mu * ipv[q] - zp[q] - zp[q] * ipv[q] * dpv[q] : R(0);
            dzn[q] = isc ? mu * inv[q] - zn[q] - zn[q] * inv[q] * dnv[q] : R(0);
            dvl[q] = hl ? mdl - vl[q] - vl[q] * idl_[q] * ds[q] : R(0);
            dvu[q] = hu ? mdu - vu[q] + vu[q] * idu_[q] * ds[q] : R(0);
            if (isc) {
                if (dpv[q] < R(0)) ap = fmin(ap, -tau * pp[q] * rcp_nr(dpv[q]));
                if (dnv[q] < R(0)) ap = fmin(ap, -tau * nn[q] * rcp_nr(dnv[q]));
                if (dzp[q] < R(0)) az = fmin(az, -tau * zp[q] * rcp_nr(dzp[q]));
                if (dzn[q] < R(0)) az = fmin(az, -tau * zn[q] * rcp_nr(dzn[q]));
                theta += fabs(cr[q] - pp[q] + nn[q] - sr[q]);
                gpn += (rho - mu * ipv[q]) * dpv[q] + (rho - mu * inv[q]) * dnv[q] - (mdl - mdu) * ds[q];
                lin += rho * (pp[q] + nn[q]) - mu * llog(pp[q] * nn[q] * (hl ? (hu ? dl * du : dl) : (hu ? du : R(1))));
            }
            const R ids = rcp_nr(ds[q]);
            if (hl && ds[q] < R(0)) ap = fmin(ap, -tau * dl * ids);
            if (hu && ds[q] > R(0)) ap = fmin(ap, tau * du * ids);
            if (hl && dvl[q] < R(0)) az = fmin(az, -tau * vl[q] * rcp_nr(dvl[q]));
            if (hu && dvu[q] < R(0)) az = fmin(az, -tau * vu[q] * rcp_nr(dvu[q]));
        }
        // proximity parts (lane j < n)
        const R ex = lane < n ? xc - xR : R(0);
        lin += R(0.5) * zeta * d2 * ex * ex;
        gpn += zeta * d2 * ex * xv;
        wmin_pair(ap, az);
        wsum_pair(theta, gpn);
        const R gphi = gpn;
        const R phi = wsum(lin);   // rho sum(p + n) + zeta/2 |D (x - xR)|^2 - mu sum ln(p n dl du)
        R amin;
        if (gphi < R(0)) {
            amin = fmin(gth, gph * theta / -gphi);
            if (theta <= theta_min) amin = fmin(amin, exp(sth * llog(theta) - sph * llog(-gphi)));
        } else {
            amin = gth;
        }
        amin *= gal;
        amin = uni(amin > R(0) ? amin : R(8.673617379884035e-19));
        RSTAMP(8);
        // ---- filter line search of the restoration problem
        R al = ap;
        bool accepted = false, ftype = false;
        R ctr[RPL], ta0[RPL], ta1[RPL];
        const R dxl = lane < n ? xv : R(0);
        while (al >= amin) {
            R tht = R(0), lt = R(0);
            bool bad = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                R vt[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) vt[i] = fma(al, rdv[q][i], rv[q][i]);
                R o[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) o[i] = w.obs6[6 * roi[q] + i];
                row_trans(rtype[q], vt, w.cst[K_GXG], w.cst[K_GYG], ta0[q], ta1[q]);
                ctr[q] = row_value(rtype[q], rk[q], vt, ta0[q], ta1[q], o, RCK);
                if (rtype[q] < R_NONE) {
                    const R pt = pp[q] + al * dpv[q], nt = nn[q] + al * dnv[q], st = sr[q] + al * ds[q];
                    tht += fabs(ctr[q] - pt + nt - st);
                    const R d1 = st - cl[q], d2_ = cu[q] - st;
                    if (!(pt > R(0)) || !(nt > R(0))) bad = true;
                    if (isfinite(cl[q]) && !(d1 > R(0))) bad = true;
                    if (isfinite(cu[q]) && !(d2_ > R(0))) bad = true;
                    // rho (p + n) - mu ln(p n dl du): one log per row, one sum with the proximity term
                    lt += rho * (pt + nt) -
                          mu * llog(pt * nt * (isfinite(cl[q]) ? (isfinite(cu[q]) ? d1 * d2_ : d1)
                                                               : (isfinite(cu[q]) ? d2_ : R(1))));
                }
            }
            const R et = ex + al * dxl;
            lt += R(0.5) * zeta * d2 * et * et;
            wsum_pair(tht, lt);
            const R pht = __ballot(bad) != 0ull ? R(INFINITY) : lt;
            bool ok = isfinite(pht) && tht < theta_max;
            if (ok) {
                const bool b0 = lane < nfr && !(tht < rft0 || pht < rfp0);
                const bool b1 = lane + WAVE < nfr && !(tht < rft1 || pht < rfp1);
                ok = __ballot(b0 || b1) == 0ull;
            }
            if (ok) {
                bool switching = false;
                if (gphi < R(0)) {   // (the three logs in one evaluation, llog3)
                    R lal, lgp, lth;
                    llog3(al, -gphi, theta, lal, lgp, lth);
                    switching = lal + sph * lgp > sth * lth;
                }
                if (switching && theta <= theta_min) {
                    if (pht <= phi + eta * al * gphi) {
                        accepted = true;
                        ftype = true;
                    }
                } else if (tht <= (R(1) - gth) * theta || pht <= phi - gph * theta) {
                    accepted = true;
                    ftype = false;
                }
            }
            if (accepted) break;
            al = uni(al * R(0.5));
        }
        RSTAMP(9);
        if (!accepted) {
            code = RSW_FAILED;
            break;
        }
        if (!ftype && nfr < FILTER_CAP) {
            const R fvt = (R(1) - gth) * theta, fvp = phi - gph * theta;
            if ((nfr & (WAVE - 1)) == lane) {
                if (nfr < WAVE) {
                    rft0 = fvt;
                    rfp0 = fvp;
                } else {
                    rft1 = fvt;
                    rfp1 = fvp;
                }
            }
            nfr++;
        }
        // ---- accept: iterate, slacks, p, n, multipliers (kappa_sigma safeguard)
        if (lane < NG) w.V[lane] = fma(al, w.dV[lane], w.V[lane]);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
#pragma unroll
            for (int i = 0; i < 4; ++i) rv[q][i] = fma(al, rdv[q][i], rv[q][i]);
            ra0[q] = ta0[q];
            ra1[q] = ta1[q];
            cr[q] = ctr[q];
            if (rtype[q] < R_NONE) {
                pp[q] += al * dpv[q];
                nn[q] += al * dnv[q];
                sr[q] += al * ds[q];
                yv[q] += al * dy[q];
                zp[q] += az * dzp[q];
                zn[q] += az * dzn[q];
                vl[q] += az * dvl[q];
                vu[q] += az * dvu[q];
                const R ks = R(1e10);
                zp[q] = fmin(fmax(zp[q], mu / (ks * pp[q])), ks * mu / pp[q]);
                zn[q] = fmin(fmax(zn[q], mu / (ks * nn[q])), ks * mu / nn[q]);
                const R d1 = sr[q] - cl[q], d2_ = cu[q] - sr[q];
                vl[q] = isfinite(cl[q]) ? fmin(fmax(vl[q], mu / (ks * d1)), ks * mu / d1) : R(0);
                vu[q] = isfinite(cu[q]) ? fmin(fmax(vu[q], mu / (ks * d2_)), ks * mu / d2_) : R(0);
            }
        }
        wave_sync();
        ++it;
        RSTAMP(10);
    }
    // ---- the iterate is in w.V; rows, slacks and slack multipliers are the caller's registers
    RSTAMP(11);
    RSTAMP_FLUSH(it - it_in);
    return (it << 4) | code;
#undef RS_RELANE
#undef RCK
}
