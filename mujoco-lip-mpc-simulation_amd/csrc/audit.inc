// audit.inc — plan audit on the device (alipmpc_audit_batch, include/alipmpc.h).
// Included by alipmpc.hip in the ALIP_PART == 0 unit.
//
// Per instance, in one launch and without materialising rows or traces: the largest constraint violation of the
// plan u (the rows alipmpc_eval_batch returns), the smallest radial clearance of its dense CoM trace (the rows
// alipmpc_trace_batch returns) to the obstacles as given, the same over the knots only, the goal distances of the
// first and last knot; per launch, integer counts of those (summary, a clearance histogram, status class x
// clearance sign x violation).
//
// Mapping: one instance per 16-lane group (one DPP row), 16 instances per 256-thread workgroup, grid-stride — the
// eval kernel's.
//   viol    the eval kernel's set-up on the same lanes (select_obs compaction by ballots, V = E x0 + G u from the G / E
//           copies in LDS, lsincos of the N headings on lanes 1..N) and its row functions (row_eval, row_bounds), one
//           pass per row family, lane t owning items t, t + 16, ...; the detour goal is not formed (no row reads it).
//   clear   the trace kernel's recurrence x_{k+1} = M_A x_k + M_B u_k, p_k = W (u_k - A x_k) on lanes 0..6 (lane i one
//           component, the sums in trace_kernel's order), the knots in LDS; lane t then owns the flat trace rows
//           t, t + 16, ... and walks the instance's obstacles (LDS: centre, cos / sin phi, 1 / a, 1 / b, min(a, b);
//           every lane of the group reads the same address) — circles by |d| - r, ellipses by the quadratic form.
//           cosh / sinh(beta t_i) come from a per-handle table.
//   minima  per lane (value, packed index) with the smaller index winning among equal values, then a 4-step DPP
//           butterfly over the row with the same rule.
//   counts  ds_add on a per-workgroup LDS copy of the summary, then one global 64-bit integer atomicAdd per non-zero
//           word and workgroup: integers only, so the summary does not depend on the order of execution.
namespace alip {

constexpr int AU_MAX_EDGES = ALIPMPC_AUDIT_MAX_EDGES;
constexpr int AU_HEAD = 6;                               // summary words ahead of the histogram
constexpr int AU_CROSS = 20;                             // status class (5) x clear >= 0 (2) x viol <= tol (2)
constexpr int AU_WORDS = AU_HEAD + AU_MAX_EDGES + 1 + AU_CROSS;
constexpr int AU_OBS = 8;                                // doubles per audited obstacle in LDS
// per-handle table (doubles): M_A, M_B, A (25 each), W (15), then per trace sample i: cosh(beta t_i),
// sinh(beta t_i) / beta, 1 - cosh(beta t_i)
constexpr int AU_TAB_MA = 0, AU_TAB_MB = 25, AU_TAB_A = 50, AU_TAB_W = 75, AU_TAB_S = 90;
__host__ __device__ constexpr int au_tab_doubles(int rows) { return AU_TAB_S + 3 * (rows - 1) + ((rows - 1) & 1); }

struct AuP {
    KP kp;                  // the eval hook's parameters (make_kp(h, B, false)); kp.u0 = the plan
    int N, rows;            // horizon, trace rows per step
    int n_edges, has_status;
    const double* tab;      // per-handle table (au_tab_doubles(rows))
    const int32_t* status;  // nullable
    double* metrics;        // nullable, B x 5
    int32_t* where;         // nullable, B x 3
    unsigned long long* summary;   // nullable
    double viol_tol;
    double edges[AU_MAX_EDGES];
};

constexpr int AUP_DOUBLES = (int)((sizeof(AuP) + 15) / 16 * 2);

// per-group workspace (doubles)
template <int N>
struct AWS {
    double* V;     // NG
    double* CT;    // N+1
    double* ST;    // N+1
    double* uv;    // nu
    double* obs;   // the eval layout's selected obstacles (3 nc_max + 9 ne_max)
    double* ao;    // audited obstacles, circles then ellipses in slot order, AU_OBS each: cx, cy, cos phi, sin phi,
                   // 1/a, 1/b, min(a, b) (a circle: cx, cy and r in the last; the others unused), one of padding
    double* xs;    // 5 (N+1): the trace recurrence's states
    double* ps;    // 2 N: stance feet
};
template <int N>
__host__ __device__ constexpr int aws_doubles(int nc_max, int ne_max)
{
    const int d = Dim<N>::NG + 2 * (N + 1) + Dim<N>::nu + 3 * nc_max + 9 * ne_max + AU_OBS * (nc_max + ne_max) +
                  5 * (N + 1) + 2 * N;
    return d + ((4 - d) % 16 + 16) % 16;   // group stride 4 (mod 16) doubles, as gws_doubles
}
template <int N>
__device__ AWS<N> carve_a(double* p, int nc_max, int ne_max)
{
    AWS<N> w;
    w.V = p; p += Dim<N>::NG;
    w.CT = p; p += N + 1;
    w.ST = p; p += N + 1;
    w.uv = p; p += Dim<N>::nu;
    w.obs = p; p += 3 * nc_max + 9 * ne_max;
    w.ao = p; p += AU_OBS * (nc_max + ne_max);
    w.xs = p; p += 5 * (N + 1);
    w.ps = p;
    return w;
}
template <int N>
__host__ __device__ constexpr size_t audit_smem(int nc_max, int ne_max, int rows)
{
    return sizeof(double) * ((size_t)Dim<N>::NG * Dim<N>::NCPU + Dim<N>::NG * 5 + ((Dim<N>::NG * 5) & 1) +
                             au_tab_doubles(rows) + AUP_DOUBLES +
                             (size_t)GROUPS_PER_BLOCK * aws_doubles<N>(nc_max, ne_max)) +
           sizeof(unsigned) * (AU_WORDS + (AU_WORDS & 1));
}

__device__ __forceinline__ bool au_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN

template <int CTRL>
__device__ __forceinline__ int au_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, DPP_BC);
}
// (value, index) of the row's minimum / maximum in every lane; equal values: the smaller index
template <bool MAX, int CTRL>
__device__ __forceinline__ void au_step(double& v, int& i)
{
    const double ov = dpp<CTRL>(v);
    const int oi = au_dpp<CTRL>(i);
    const bool take = (MAX ? ov > v : ov < v) || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}
template <bool MAX>
__device__ __forceinline__ void au_reduce16(double& v, int& i)
{
    au_step<MAX, 0xB1>(v, i);
    au_step<MAX, 0x4E>(v, i);
    au_step<MAX, 0x141>(v, i);
    au_step<MAX, 0x140>(v, i);
}
__device__ __forceinline__ double au_min16(double v)
{
    v = fmin(v, dpp<0xB1>(v));
    v = fmin(v, dpp<0x4E>(v));
    v = fmin(v, dpp<0x141>(v));
    v = fmin(v, dpp<0x140>(v));
    return v;
}

// one row family (eval_rows' item order and row functions): this lane's largest max(cl - c, c - cu, 0) and its row
template <int N, int TYPE>
__device__ __forceinline__ void audit_rows(const KP& P, const AWS<N>& w, int t, int legv, int nsel, int cnt, int loff,
                                           double& vmax, int& vrow)
{
    const int total = N * cnt;
    for (int i = t; i < total; i += GLANES) {
        const int k = cnt == 1 ? i : i / cnt, slot = i - k * cnt;
        const int r = k * P.rps + loff + slot;
        if ((TYPE == R_CIR || TYPE == R_ELP) && slot >= nsel) continue;   // inactive row
        RowInfo ri;
        ri.type = TYPE;
        ri.k = k;
        ri.slot = slot;
        double cf[4];
        int gn[4];
        const double c = row_eval<N, false>(P, ri, w.V, w.CT, w.ST, w.obs, 0.0, cf, gn);
        double clv, cuv;
        row_bounds(P, ri, legv, clv, cuv);
        const double v = fmax(fmax(clv - c, c - cuv), 0.0);
        const bool take = v > vmax || (v == vmax && v > 0.0 && r < vrow);
        vmax = take ? v : vmax;
        vrow = take ? r : vrow;
    }
}

// The obstacles of instance b: the eval layout's select_obs compaction about (px, py) (eval_group_one's) into w.obs,
// ncs circles and nes ellipses kept; AO: also, unfiltered, the audited list w.ao.
template <int N, bool AO>
__device__ __forceinline__ void audit_select(const KP& P, const AWS<N>& w, long long b, int t, double px, double py,
                                             int ncr, int ner, int& ncs, int& nes)
{
    ncs = 0;
    nes = 0;
    for (int base = 0; base < P.nc_max; base += GLANES) {
        const int j = base + t;
        const bool valid = j < ncr;
        double c0 = 0, c1 = 0, c2 = 0;
        if (valid) {
            const gdouble* c = gptr(P.cir) + ((size_t)b * P.nc_max + j) * 3;
            c0 = c[0]; c1 = c[1]; c2 = c[2];
            if (AO) {
                double* o = w.ao + AU_OBS * j;
                o[0] = c0; o[1] = c1;
                o[6] = c2;
            }
        }
        const double d = (px - c0) * (px - c0) + (py - c1) * (py - c1) - c2 * c2;
        const bool keep = valid && (!P.select_obs || d <= P.detect_r2);
        const unsigned m = gballot(keep);
        const int pos = ncs + __builtin_popcount(m & ((1u << t) - 1u));
        if (keep) {
            w.obs[3 * pos + 0] = c0;
            w.obs[3 * pos + 1] = c1;
            w.obs[3 * pos + 2] = c2;
        }
        ncs += __builtin_popcount(m);
    }
    for (int base = 0; base < P.ne_max; base += GLANES) {
        const int j = base + t;
        const bool valid = j < ner;
        double e[5] = {0, 0, 0, 0, 0};
        double ce = 1.0, se = 0.0;
        if (valid) {
            const gdouble* ep = gptr(P.elp) + ((size_t)b * P.ne_max + j) * 5;
            for (int i = 0; i < 5; ++i) e[i] = ep[i];
            sincos(e[4], &se, &ce);
            if (AO) {
                double* o = w.ao + AU_OBS * (ncr + j);
                o[0] = e[0]; o[1] = e[1]; o[2] = ce; o[3] = se;
                o[4] = 1.0 / e[2];
                o[5] = 1.0 / e[3];
                o[6] = fmin(e[2], e[3]);
            }
        }
        const double rmax = e[2] > e[3] ? e[2] : e[3];
        const double d = (px - e[0]) * (px - e[0]) + (py - e[1]) * (py - e[1]) - rmax * rmax;
        const bool keep = valid && (!P.select_obs || d <= P.detect_r2);
        const unsigned m = gballot(keep);
        const int pos = nes + __builtin_popcount(m & ((1u << t) - 1u));
        if (keep) {
            double* o = w.obs + 3 * P.nc_max + 5 * pos;
            for (int i = 0; i < 5; ++i) o[i] = e[i];
            double* qq = w.obs + 3 * P.nc_max + 5 * P.ne_max;
            qq[pos] = (e[3] * ce) * (e[3] * ce) + (e[2] * se) * (e[2] * se);
            qq[P.ne_max + pos] = 2 * ce * se * (e[3] * e[3] - e[2] * e[2]);
            qq[2 * P.ne_max + pos] = (e[3] * se) * (e[3] * se) + (e[2] * ce) * (e[2] * ce);
            qq[3 * P.ne_max + pos] = (e[3] * e[2]) * (e[3] * e[2]);
        }
        nes += __builtin_popcount(m);
    }
}

// The violation pass, shared by audit_kernel and the scheduled loop's guard (cl_guard_kernel), in two parts (the audit
// runs its trace recurrence between them, as it always did).  audit_V: V = E x + G u into w.V from xb and w.uv (in LDS,
// visible to the group).  audit_viol, after a wave_sync: the headings' sincos, one pass per row family over w.obs (ncs,
// nes selected), the row reduction — the largest max(cl - c, c - cu, 0) and its row, in every lane of the group.
template <int N>
__device__ __forceinline__ void audit_V(const AWS<N>& w, const double* G, const double* E, const double* xb, int t)
{
    using D = Dim<N>;
    constexpr int nu = D::nu, NCP = D::NCPU, NG = D::NG;
    // V = E x0 + G u (eval_group_one's sums)
    for (int g = t; g < NG; g += GLANES) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 5; ++c) v += E[g * 5 + c] * xb[c];
        const double* gr = G + g * NCP;
#pragma unroll
        for (int j = 0; j < nu; ++j) v += gr[j] * w.uv[j];
        w.V[g] = v;
    }
}
template <int N>
__device__ __forceinline__ void audit_viol(const KP& P, const AWS<N>& w, int t, int legv, int ncs, int nes, double& vmax,
                                           int& vrow)
{
    // state pass: lanes 1..N own cos / sin of theta_k
    if (t >= 1 && t <= N) {
        double s_, c_;
        lsincos(w.V[gx(t, 4)], &s_, &c_);
        w.CT[t] = c_;
        w.ST[t] = s_;
    }
    wave_sync();
    // the eval rows
    vmax = 0.0;
    vrow = 0x7fffffff;
    {
        const int nc = P.nc_max, ne = P.ne_max, lo = 2 + nc + ne;
        audit_rows<N, R_VBX>(P, w, t, legv, 0, 1, 0, vmax, vrow);
        audit_rows<N, R_VBY>(P, w, t, legv, 0, 1, 1, vmax, vrow);
        if (nc) audit_rows<N, R_CIR>(P, w, t, legv, ncs, nc, 2, vmax, vrow);
        if (ne) audit_rows<N, R_ELP>(P, w, t, legv, nes, ne, 2 + nc, vmax, vrow);
        audit_rows<N, R_LEG>(P, w, t, legv, 0, 1, lo, vmax, vrow);
        audit_rows<N, R_DTH>(P, w, t, legv, 0, 1, lo + 1, vmax, vrow);
        if (P.rps > lo + 2) audit_rows<N, R_FEN>(P, w, t, legv, 0, 1, lo + 2, vmax, vrow);
    }
    au_reduce16<true>(vmax, vrow);
}

template <int N>
__device__ __forceinline__ void audit_group_one(const AuP& A, const AWS<N>& w, const double* G, const double* E,
                                                const double* tab, unsigned* cnt, long long b, int t)
{
    constexpr int nu = Dim<N>::nu;
    const KP& P = A.kp;
    const gdouble* x0 = gptr(P.x0) + 5 * b;
    const int legv = P.leg[b];
    const int ncr = min(max(P.nc[b], 0), P.nc_max);
    const int ner = P.ne ? min(max(P.ne[b], 0), P.ne_max) : 0;
    const double x0v0 = x0[0], x0v1 = x0[1];
    const double g0 = gptr(P.goal)[2 * b], g1 = gptr(P.goal)[2 * b + 1];
    double xb[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) xb[c] = x0[c];
    bool fin = au_finite(g0) && au_finite(g1);
#pragma unroll
    for (int c = 0; c < 5; ++c) fin = fin && au_finite(xb[c]);
    int ncs, nes;
    audit_select<N, true>(P, w, b, t, x0v0, x0v1, ncr, ner, ncs, nes);
    // the plan
    for (int j = t; j < nu; j += GLANES) {
        const double v = gptr(P.u0)[(size_t)b * nu + j];
        w.uv[j] = v;
        fin = fin && au_finite(v);
    }
    fin = gballot(!fin) == 0u;
    if (t < 5) w.xs[t] = xb[t];
    wave_sync();
    audit_V<N>(w, G, E, xb, t);
    // the trace's recurrence (trace_kernel's sums): lanes 0..4 x_{k+1}[t], lanes 5, 6 p_k[t - 5]
    for (int k = 0; k < N; ++k) {
        const double* x = w.xs + 5 * k;
        const double* uk = w.uv + 5 * k;
        if (t < 5) {
            double v = 0.0;
            for (int c = 0; c < 5; ++c) v += tab[AU_TAB_MA + t * 5 + c] * x[c];
            for (int c = 0; c < 5; ++c) v += tab[AU_TAB_MB + t * 5 + c] * uk[c];
            w.xs[5 * (k + 1) + t] = v;
        } else if (t < 7) {
            double p = 0.0;
            for (int i = 0; i < 5; ++i) {
                double v = 0.0;
                for (int c = 0; c < 5; ++c) v += tab[AU_TAB_A + i * 5 + c] * x[c];
                p += tab[AU_TAB_W + (t - 5) * 5 + i] * (uk[i] - v);
            }
            w.ps[2 * k + (t - 5)] = p;
        }
        wave_sync();
    }
    // ---- viol: the eval rows
    double vmax;
    int vrow;
    audit_viol<N>(P, w, t, legv, ncs, nes, vmax, vrow);
    // ---- clear: trace rows x obstacles
    const int rows = A.rows, nobs = ncr + ner, total = N * rows;
    double cmin = INFINITY, kmin = INFINITY;
    int cidx = 0x7fffffff;
    for (int fr = t; fr < total; fr += GLANES) {
        const int k = fr / rows, r = fr - k * rows;
        const double* x = w.xs + 5 * k;
        double px = x[0], py = x[1];
        if (r > 0) {
            const double* s = tab + AU_TAB_S + 3 * (r - 1);
            const double ch = s[0], shb = s[1], omc = s[2];
            px = ch * x[0] + shb * x[2] + omc * w.ps[2 * k];
            py = ch * x[1] + shb * x[3] + omc * w.ps[2 * k + 1];
        }
        double rmin = INFINITY;
        int ro = 0;
        for (int o = 0; o < ncr; ++o) {   // circles: |d| - r, no quadratic form
            const double* ob = w.ao + AU_OBS * o;
            const double dx = px - ob[0], dy = py - ob[1];
            const double d2 = dx * dx + dy * dy;
            double cl = d2 * rsqrt_nr(d2) - ob[6];
            cl = d2 > 0.0 ? cl : -ob[6];
            const bool take = cl < rmin;   // ascending o: the first of equal values stays
            rmin = take ? cl : rmin;
            ro = take ? o : ro;
        }
        for (int o = ncr; o < nobs; ++o) {
            const double* ob = w.ao + AU_OBS * o;
            const double dx = px - ob[0], dy = py - ob[1];
            const double d2 = dx * dx + dy * dy;
            const double qu = (dx * ob[2] + dy * ob[3]) * ob[4], qv = (dy * ob[2] - dx * ob[3]) * ob[5];
            const double Q = qu * qu + qv * qv;
            const double dn = d2 * rsqrt_nr(d2);
            double cl = dn * (1.0 - rsqrt_nr(Q));
            cl = d2 > 0.0 ? cl : -ob[6];
            const bool take = cl < rmin;   // ascending o: the first of equal values stays
            rmin = take ? cl : rmin;
            ro = take ? o : ro;
        }
        const int slot = ro < ncr ? ro : P.nc_max + (ro - ncr);
        if (rmin < cmin) {   // ascending rows: the first of equal values stays
            cmin = rmin;
            cidx = fr * 32 + slot;
        }
        if (r == 0 || fr == total - 1) kmin = fmin(kmin, rmin);
    }
    au_reduce16<false>(cmin, cidx);
    kmin = au_min16(kmin);
    // goal distances of knots 1 and N (knot k < N: row 0 of step k; knot N: the last row of step N - 1)
    double kNx, kNy;
    {
        const double* x = w.xs + 5 * (N - 1);
        const double* s = tab + AU_TAB_S + 3 * (rows - 2);
        kNx = s[0] * x[0] + s[1] * x[2] + s[2] * w.ps[2 * (N - 1)];
        kNy = s[0] * x[1] + s[1] * x[3] + s[2] * w.ps[2 * (N - 1) + 1];
    }
    const double k1x = N > 1 ? w.xs[5] : kNx, k1y = N > 1 ? w.xs[6] : kNy;
    const double goal1 = sqrt((k1x - g0) * (k1x - g0) + (k1y - g1) * (k1y - g1));
    const double goalN = sqrt((kNx - g0) * (kNx - g0) + (kNy - g1) * (kNy - g1));
    // ---- outputs
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double viol = fin ? vmax : nan, clear = fin ? cmin : nan, knot = fin ? kmin : nan;
    const bool hit = nobs > 0 && cidx != 0x7fffffff;
    if (A.metrics && t < ALIPMPC_AUDIT_COLS) {
        const double m = t == 0 ? viol : t == 1 ? clear : t == 2 ? knot : t == 3 ? (fin ? goal1 : nan) : (fin ? goalN : nan);
        gptr(A.metrics)[(size_t)b * ALIPMPC_AUDIT_COLS + t] = m;
    }
    if (A.where && t < ALIPMPC_AUDIT_WHERE) {
        const int wv = t == 0 ? (vmax > 0.0 ? vrow : -1) : t == 1 ? (hit ? cidx >> 5 : -1) : (hit ? cidx & 31 : -1);
        A.where[(size_t)b * ALIPMPC_AUDIT_WHERE + t] = fin ? wv : -1;
    }
    if (A.summary && t == 0) {
        atomicAdd(&cnt[0], 1u);
        if (!fin) {
            atomicAdd(&cnt[1], 1u);
        } else {
            const bool vok = viol <= A.viol_tol, cok = clear >= 0.0;
            if (vok) atomicAdd(&cnt[2], 1u);
            if (cok) atomicAdd(&cnt[3], 1u);
            if (vok && cok) atomicAdd(&cnt[4], 1u);
            if (clear < 0.0 && knot >= 0.0) atomicAdd(&cnt[5], 1u);
            int bin = 0;
            for (int i = 0; i < A.n_edges; ++i) bin += A.edges[i] <= clear ? 1 : 0;
            atomicAdd(&cnt[AU_HEAD + bin], 1u);
            if (A.has_status) {
                const int s = A.status[b];
                const int cls = s == 0 ? 0 : s == 1 ? 1 : s == -1 ? 2 : s == 2 ? 3 : 4;
                atomicAdd(&cnt[AU_HEAD + A.n_edges + 1 + cls * 4 + 2 * (cok ? 1 : 0) + (vok ? 1 : 0)], 1u);
            }
        }
    }
    wave_sync();
}

template <int N>
__global__ __launch_bounds__(256) void audit_kernel(AuP Av)
{
    using D = Dim<N>;
    constexpr int NCP = D::NCPU, NG = D::NG;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // the parameters live in LDS (as eval_kernel's): keeps the kernarg SGPRs from being pinned across the audit
    AuP* As = reinterpret_cast<AuP*>(smem);
    double* G = smem + AUP_DOUBLES;
    double* E = G + NG * NCP;
    double* tab = E + NG * 5 + ((NG * 5) & 1);
    const int ntab = au_tab_doubles(Av.rows);
    double* wsb = tab + ntab;
    const int wsd = aws_doubles<N>(Av.kp.nc_max, Av.kp.ne_max);
    unsigned* cnt = reinterpret_cast<unsigned*>(wsb + (size_t)GROUPS_PER_BLOCK * wsd);
    if (threadIdx.x == 0) *As = Av;
    for (int i = threadIdx.x; i < NG * NCP; i += blockDim.x) G[i] = Av.kp.G[i];
    for (int i = threadIdx.x; i < NG * 5; i += blockDim.x) E[i] = Av.kp.E[i];
    for (int i = threadIdx.x; i < ntab; i += blockDim.x) tab[i] = Av.tab[i];
    for (int i = threadIdx.x; i < AU_WORDS; i += blockDim.x) cnt[i] = 0u;
    __syncthreads();
    const AuP& A = *As;
    const int gi = threadIdx.x / GLANES, t = threadIdx.x & (GLANES - 1);
    const AWS<N> w = carve_a<N>(wsb + (size_t)gi * wsd, A.kp.nc_max, A.kp.ne_max);
    for (long long b0 = (long long)blockIdx.x * GROUPS_PER_BLOCK; b0 < A.kp.B; b0 += (long long)gridDim.x * GROUPS_PER_BLOCK) {
        const long long b = b0 + gi;
        if (b < A.kp.B) audit_group_one<N>(A, w, G, E, tab, cnt, b, t);
    }
    if (A.summary) {
        __syncthreads();
        const int words = AU_HEAD + A.n_edges + 1 + (A.has_status ? AU_CROSS : 0);
        for (int i = threadIdx.x; i < words; i += blockDim.x)
            if (cnt[i]) atomicAdd(&A.summary[i], (unsigned long long)cnt[i]);
    }
}

template <int N>
static hipError_t launch_audit_t(const AuP& A, hipStream_t st)
{
    const size_t smem = audit_smem<N>(A.kp.nc_max, A.kp.ne_max, A.rows);
    set_smem((const void*)audit_kernel<N>, smem);
    const unsigned need = (unsigned)((A.kp.B + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK);
    const unsigned res = resident_blocks((const void*)audit_kernel<N>, smem);
    const unsigned grid = res > 0 && res < need ? res : (need > 0 ? need : 1u);
    hipLaunchKernelGGL(audit_kernel<N>, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), smem, st, A);
    return hipGetLastError();
}

static hipError_t launch_audit(int N, const AuP& A, hipStream_t st)
{
    switch (N) {
    case 1: return launch_audit_t<1>(A, st);
    case 2: return launch_audit_t<2>(A, st);
    case 3: return launch_audit_t<3>(A, st);
    case 4: return launch_audit_t<4>(A, st);
    case 5: return launch_audit_t<5>(A, st);
    case 6: return launch_audit_t<6>(A, st);
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------
// The guard of the scheduled closed loop's first-order ticks (cfg.cl_between = ALIPMPC_CL_BETWEEN_GUARDED, closed_loop.inc:
// cl_between_run_kernel).  Before a first-order tick commands u_fo = ua + du[:, 0:5] (x_nex - xa), this kernel holds it
// against the eval hook's rows at the tick's own x_nex — alipmpc_audit_batch's column 0 of (x0 = x_nex, u = u_fo,
// leg = -leg_ind), obstacle selection at x_nex included — and sets CL_FLAG_FIRED where !(viol <= tol): that episode
// re-solves on this tick instead (closed_loop_host.inc).  The audit's mapping: one episode per 16-lane row, 16 per workgroup,
// grid-stride, the workspace of a group in LDS (AWS without the clearance pass's parts); episodes that have stopped or
// have no anchor are skipped.  x_nex is formed by every lane of the row (cl_flow, the tick kernels' expression), u_fo by
// the lane that owns the component (cl_first_order_plan's sum).  A plan or state that is not finite has viol = NaN, as
// in the audit, and so fires at any tolerance.
// ------------------------------------------------------------------------------------------------
struct CLG {
    KP kp;                // the eval hook's parameters of the episode group (goal, cir, nc, elp, ne; x0, leg, u0 unread)
    uint8_t* flags;       // CLP::flags
    const double* x;      // B x 5 plant state
    const double* pst;    // B x 2 stance foot
    const double* hdv;    // B x 4 (hd_input_pr at 1)
    const int8_t* leg;    // B leg_ind
    const double* xa;     // the anchors (CLB)
    const double* ua;
    const double* du;
    double ch, shb, bsh, tt;   // the rest flow of this tick index (CLN::rest)
    double tol;
};
constexpr int CLG_DOUBLES = (int)((sizeof(CLG) + 15) / 16 * 2);

template <int N>
__host__ __device__ constexpr int cgws_doubles(int nc_max, int ne_max)
{
    const int d = Dim<N>::NG + 2 * (N + 1) + Dim<N>::nu + 3 * nc_max + 9 * ne_max;
    return d + ((4 - d) % 16 + 16) % 16;   // group stride 4 (mod 16) doubles, as aws_doubles
}
template <int N>
__host__ __device__ constexpr size_t guard_smem(int nc_max, int ne_max)
{
    return sizeof(double) * ((size_t)Dim<N>::NG * Dim<N>::NCPU + Dim<N>::NG * 5 + ((Dim<N>::NG * 5) & 1) + CLG_DOUBLES +
                             (size_t)GROUPS_PER_BLOCK * cgws_doubles<N>(nc_max, ne_max));
}

template <int N>
__global__ __launch_bounds__(256) void cl_guard_kernel(CLG Qv)
{
    using D = Dim<N>;
    constexpr int nu = D::nu, NCP = D::NCPU, NG = D::NG;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    CLG* Qs = reinterpret_cast<CLG*>(smem);   // (the parameters in LDS, as audit_kernel keeps them)
    double* G = smem + CLG_DOUBLES;
    double* E = G + NG * NCP;
    double* wsb = E + NG * 5 + ((NG * 5) & 1);
    if (threadIdx.x == 0) *Qs = Qv;
    for (int i = threadIdx.x; i < NG * NCP; i += blockDim.x) G[i] = Qv.kp.G[i];
    for (int i = threadIdx.x; i < NG * 5; i += blockDim.x) E[i] = Qv.kp.E[i];
    __syncthreads();
    const CLG& Q = *Qs;
    const KP& P = Q.kp;
    const int gi = threadIdx.x / GLANES, t = threadIdx.x & (GLANES - 1);
    AWS<N> w;
    {
        double* p = wsb + (size_t)gi * cgws_doubles<N>(P.nc_max, P.ne_max);
        w.V = p; p += NG;
        w.CT = p; p += N + 1;
        w.ST = p; p += N + 1;
        w.uv = p; p += nu;
        w.obs = p;
        w.ao = w.xs = w.ps = nullptr;   // (the clearance pass's: not carved here)
    }
    for (long long b0 = (long long)blockIdx.x * GROUPS_PER_BLOCK; b0 < P.B; b0 += (long long)gridDim.x * GROUPS_PER_BLOCK) {
        const long long b = b0 + gi;
        if (b >= P.B) continue;
        const uint8_t fl = Q.flags[b];
        if (!(fl & 1) || !(fl & CL_FLAG_ANCHOR)) continue;
        double x[5], xn[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) x[c] = gptr(Q.x)[5 * b + c];
        cl_flow(x, gptr(Q.pst)[2 * b], gptr(Q.pst)[2 * b + 1], gptr(Q.hdv)[4 * b + 1], Q.ch, Q.shb, Q.bsh, Q.tt, xn);
        const int legv = -(int)Q.leg[b];
        const int ncr = min(max(P.nc[b], 0), P.nc_max);
        const int ner = P.ne ? min(max(P.ne[b], 0), P.ne_max) : 0;
        bool fin = au_finite(gptr(P.goal)[2 * b]) && au_finite(gptr(P.goal)[2 * b + 1]);
        double d[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            fin = fin && au_finite(xn[c]);
            d[c] = xn[c] - gptr(Q.xa)[5 * b + c];
        }
        int ncs, nes;
        audit_select<N, false>(P, w, b, t, xn[0], xn[1], ncr, ner, ncs, nes);
        for (int j = t; j < nu; j += GLANES) {
            const gdouble* r = gptr(Q.du) + ((size_t)b * nu + j) * 7;
            double v = 0.0;
            for (int c = 0; c < 5; ++c) v += r[c] * d[c];
            const double uj = gptr(Q.ua)[(size_t)b * nu + j] + v;
            w.uv[j] = uj;
            fin = fin && au_finite(uj);
        }
        fin = gballot(!fin) == 0u;
        wave_sync();
        audit_V<N>(w, G, E, xn, t);
        wave_sync();
        double vmax;
        int vrow;
        audit_viol<N>(P, w, t, legv, ncs, nes, vmax, vrow);
        const bool fire = !(fin && vmax <= Q.tol);
        if (t == 0 && fire) Q.flags[b] = fl | CL_FLAG_FIRED;
        wave_sync();
    }
}

template <int N>
static hipError_t launch_guard_t(const CLG& Q, hipStream_t st)
{
    const size_t smem = guard_smem<N>(Q.kp.nc_max, Q.kp.ne_max);
    set_smem((const void*)cl_guard_kernel<N>, smem);
    const unsigned need = (unsigned)((Q.kp.B + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK);
    const unsigned res = resident_blocks((const void*)cl_guard_kernel<N>, smem);
    const unsigned grid = res > 0 && res < need ? res : (need > 0 ? need : 1u);
    hipLaunchKernelGGL(cl_guard_kernel<N>, dim3(grid), dim3(WAVE * WAVES_PER_BLOCK), smem, st, Q);
    return hipGetLastError();
}

static hipError_t launch_guard(int N, const CLG& Q, hipStream_t st)
{
    switch (N) {
    case 1: return launch_guard_t<1>(Q, st);
    case 2: return launch_guard_t<2>(Q, st);
    case 3: return launch_guard_t<3>(Q, st);
    case 4: return launch_guard_t<4>(Q, st);
    case 5: return launch_guard_t<5>(Q, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace alip
