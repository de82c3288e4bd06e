// lane_solve.inc — the lane solver: ONE NLP instance per LANE (64 instances per wavefront).
// Included by alipmpc.hip inside namespace alip (device part).
//
// Same problem and the same interior-point algorithm as solve_kernel / oracle/alipmpc_oracle.c osolve
// (IPOPT's monotone barrier update, fraction to boundary, Wachter-Biegler filter line search, inertia
// correction, restoration substitute, IPOPT statuses — DESIGN.md §2), restated for a lane:
//   reference                                  here
//   MPCCBF.select_obs  MPC_LIP_modi.py:325-338  lane_init: range filter per circle slot (slots stay in place)
//   solveMPCCBF set-up :205-271                 lane_init: bounds by row kind + leg parity, detour goal
//   LIP_Prob callbacks :430-583, :586-655       row_eval / obj terms, Jacobians in foothold space
//   cyipopt solve      :274-296                 phases A (direction) and T (one line-search trial)
//   gen_control_test rollout :102-112           lane_finish (u_k = x_{k+1}, foot = p_0)
//
// Why: the per-wave kernel spends ~3.9k wave instructions per interior-point iteration on a 9-variable
// problem (reductions, broadcasts, control), i.e. it is issue-bound with 36 of 64 lanes busy at best.
// Here each lane runs the whole iteration on its own instance with every array in registers, unrolled at
// compile time over the (compile-time) row layout, so one wave instruction advances 64 instances.
//
// Layout: the row layout is a template (N, NC circle slots, MODI) — rows per step k:
//   [vbx, vby, circle slot 0..NC-1, leg, dtheta, (modi) vbx + s dth <= hi, vbx - s dth <= hi]
// Unselected circle slots stay in place and are inactive (no bounds, no multipliers): the compacted row
// order of the reference differs only in the order of the sums.
// The form build (FM: lane_kernel<N, NS, true, Form<R>>, modi only) has NS obstacle-form slots in the circle slots'
// place: slot j < cfg.nc_max is circle j, slot cfg.nc_max + j is ellipse j (the padded row order of alipmpc.h), each a
// quadratic form (ox, oy, qa, qb, qc, k) with the D-CBF row of MPC_LIP_modi.py:598-617 (h_elp; kind FRM below).
// Decision: footholds p = [fx_k, fy_k, dth_k]_k (n = 3N) as in solve_kernel (DESIGN.md §2 item 2); the
// x/y/theta channels of the ALIP step map are decoupled, so d x_k / d p_j is two scalars per axis
// (SP/SV below) and a 1 for theta: every Jacobian row is built from <= 4 state-space coefficients.
//
// Divergence: a lane is in one of three phases — 0 (no instance: take one from the work queue), 1 (new
// direction: convergence test, barrier update, KKT assemble/factor/solve, step bounds) or 2 (one filter
// line-search trial).  Every pass of the wave's loop runs phase 0 for the lanes that need it (when enough
// are idle), phase 1 for the lanes in it, then phase 2: a lane whose trial is rejected simply stays in
// phase 2, so line searches of different lengths do not serialise the wave.
//
// Per lane: s, z_l, z_u, dS for every row, p, dp, the obstacle forms — registers; the filter and the copy
// of K kept for inertia-correction retries — LDS (structure of arrays, [entry][lane]).

namespace lane {

template <int I, int E, class F>
__device__ __forceinline__ void sfor(F&& f)
{
    if constexpr (I < E) {
        f(std::integral_constant<int, I>());
        sfor<I + 1, E>(f);
    }
}

// KP::lk slots (host: lane_constants)
enum {
    LK_CH = 0, LK_SHB, LK_BSH, LK_OMC, LK_WCH, LK_WSH,
    LK_SP = 6,    // SP[m] = d px_k / d fx_{k-1-m} = (Abar^m bbar)[0], m < 6
    LK_SV = 12,   // SV[m] = d vx_k / d fx_{k-1-m} = (Abar^m bbar)[1]
    LK_VXL = 18, LK_VXU, LK_VYLP, LK_VYUP, LK_VYLN, LK_VYUN, LK_CIRL, LK_LEGL, LK_LEGU, LK_DTL, LK_DTU,   // relaxed
    LK_OVXL = 29, LK_OVXU, LK_OVYLP, LK_OVYUP, LK_OVYLN, LK_OVYUN, LK_OLEGU, LK_ODT,                      // original
    LK_Q = 37, LK_P, LK_R, LK_GM1, LK_S, LK_TOL, LK_ACC, LK_MU0, LK_DET2,
    LK_SU0 = 46,  // SU0[m] = d px_{k+1+m} / d u_k[px] (the reference's u: per axis (MA^m MB)[0][0]), m < 6
    LK_SU1 = 52,  // SU1[m] = d px_{k+1+m} / d u_k[vx]
    LK_COUNT = 58
};
constexpr int LK_BUF = 64;   // lane-constant buffer (fp64 and fp32 copies)

enum { VBX = 0, VBY, CIR, LEG, DTH, FEN, FENM, FRM };
template <int KD>
constexpr bool is_obs() { return KD == CIR || KD == FRM; }   // an obstacle slot's row: circle or quadratic form
enum { GPX = 0, GPY, GVX, GVY, GTH, GFX, GFY, GFT, GNONE };


// the lane constants, read through a scalar constant-address-space pointer that the kernel launders at every
// phase (asm volatile), so nothing derived from them is hoisted out of the instance loop and kept live in
// VGPRs (or spilled) across the whole solve: they are re-read as s_load into SGPRs where they are used
template <class R>
struct LK {
    const __attribute__((address_space(4))) R* p;
    __device__ __forceinline__ R operator[](int i) const { return p[i]; }
};
template <class R>
__device__ __forceinline__ LK<R> lk_of(const KP& P)
{
    const R* q = sizeof(R) == 8 ? (const R*)(const void*)P.lkd : (const R*)(const void*)P.lkfd;
    asm volatile("" : "+s"(q));
    LK<R> c;
    c.p = (const __attribute__((address_space(4))) R*)q;
    return c;
}


template <int N, int NC, bool MODI>
struct Shape {
    static constexpr int n = 3 * N;
    static constexpr int RPS = 4 + NC + (MODI ? 2 : 0);   // rows per step
    static constexpr int M = N * RPS;
    static constexpr int ZLS = 4 + NC;                     // rows with a lower bound per step (all but f_en)
    static constexpr int ZUS = MODI ? 6 : 4;               // rows with an upper bound per step (all but circles)
    static constexpr int NZL = N * ZLS, NZU = N * ZUS;
};

// the kernel's arithmetic argument: R, or Form<R> for the obstacle-form build of the same arithmetic
template <class R>
struct Form {};
template <class RT>
struct Real { using type = RT; static constexpr bool form = false; };
template <class R>
struct Real<Form<R>> { using type = R; static constexpr bool form = true; };

template <int K_>
using KindT = std::integral_constant<int, K_>;

// an opaque (re)definition of every element: later expressions of them are recomputed, not CSE'd with earlier
// identical ones (that would keep values of many rows alive across the whole phase)
template <class T, int K0>
__device__ __forceinline__ void launder_all(T (&v)[K0])
{
#pragma unroll
    for (int i = 0; i < K0; ++i) asm volatile("" : "+v"(v[i]));
}
template <class T, int K0, int K1>
__device__ __forceinline__ void launder_all(T (&v)[K0][K1])
{
#pragma unroll
    for (int i = 0; i < K0; ++i) launder_all(v[i]);
}

// a[i] for a runtime (wave-uniform) i, from register arrays
template <class T, int K0>
__device__ __forceinline__ T pick(const T (&a)[K0], int i)
{
    T v = a[0];
#pragma unroll
    for (int t = 1; t < K0; ++t) v = i == t ? a[t] : v;
    return v;
}

constexpr int FCAP = 8;   // filter entries per lane (dominated entries are pruned; see the trial phase)

// the barrier function / filter arithmetic (merit_t): the rows' precision.  r5 kept it in fp64 in the fp32 build for a
// while (objective, log-barrier sum, filter entries as hi / lo fp32 pairs): once the objective's goal differences are
// taken in map coordinates (eval_states) that form changed no closed-loop status count against the fp32 one and cost
// 25 % of cfg5 (53.6 vs 66.5 M solves/s; DESIGN.md §2).  -DALIP_LANE_M32=0 builds it for A/B.
#ifndef ALIP_LANE_M32
#define ALIP_LANE_M32 1
#endif
template <class R>
using merit_t = typename std::conditional<(sizeof(R) == 4 && ALIP_LANE_M32), float, double>::type;

// instances per wave: fp32 64 (one per lane), fp64 32 — the per-row state lives in LDS and 32 fp64 lanes
// use the LDS of 64 fp32 lanes
template <class R>
constexpr int lanes_of() { return sizeof(R) == 8 ? 32 : 64; }

// per-wave LDS, [entry][lane] (each access conflict-free).  Entries: s (M rows), dS (M), z_l (rows with a
// lower bound), z_u (rows with an upper bound), circle forms ox / oy / r^2 (NC each), filter theta / phi.
// OE entries per obstacle slot: 3 (circles) or 6 (the form build: ox / oy / k, then qa / qb / qc).
// The lane base is laundered at every pass so loads are not CSE'd across passes into long-lived registers.
template <class R, int N, int NC, bool MODI, int L, int OE = 3>
struct Lds {
    using S = Shape<N, NC, MODI>;
    // (fp32: the filter's barrier-function values are fp64, kept as hi / lo fp32 pairs: FCAP more entries)
    static constexpr int ENT = 2 * S::M + S::NZL + S::NZU + OE * NC + 2 * FCAP + (sizeof(R) == 4 && !ALIP_LANE_M32 ? FCAP : 0);
    // an LDS-address-space pointer: a generic one (which the laundering would leave the compiler with)
    // turns every access into a FLAT instruction on the vector-memory path
    typedef __attribute__((address_space(3))) R lr;
    typedef lr* lptr;
    lptr b;
    __device__ __forceinline__ lr& s(int i) const { return b[i * L]; }
    __device__ __forceinline__ lr& ds(int i) const { return b[(S::M + i) * L]; }
    __device__ __forceinline__ lr& zl(int i) const { return b[(2 * S::M + i) * L]; }
    __device__ __forceinline__ lr& zu(int i) const { return b[(2 * S::M + S::NZL + i) * L]; }
    __device__ __forceinline__ lr& ox(int j) const { return b[(2 * S::M + S::NZL + S::NZU + j) * L]; }
    __device__ __forceinline__ lr& oy(int j) const { return b[(2 * S::M + S::NZL + S::NZU + NC + j) * L]; }
    __device__ __forceinline__ lr& orr(int j) const { return b[(2 * S::M + S::NZL + S::NZU + 2 * NC + j) * L]; }
    // (OE = 6: orr holds the form's k; circles in a form slot have qa = qc = 1, qb = 0, k = r^2)
    __device__ __forceinline__ lr& qa(int j) const { return b[(2 * S::M + S::NZL + S::NZU + 3 * NC + j) * L]; }
    __device__ __forceinline__ lr& qb(int j) const { return b[(2 * S::M + S::NZL + S::NZU + 4 * NC + j) * L]; }
    __device__ __forceinline__ lr& qc(int j) const { return b[(2 * S::M + S::NZL + S::NZU + 5 * NC + j) * L]; }
    __device__ __forceinline__ lr& fth(int e) const { return b[(2 * S::M + S::NZL + S::NZU + OE * NC + e) * L]; }
    __device__ __forceinline__ lr& fph(int e) const { return b[(2 * S::M + S::NZL + S::NZU + OE * NC + FCAP + e) * L]; }
    __device__ __forceinline__ lr& fpl(int e) const { return b[(2 * S::M + S::NZL + S::NZU + OE * NC + 2 * FCAP + e) * L]; }
    // a filter entry's barrier-function value (merit_t: with ALIP_LANE_M32=0 the fp32 build keeps fp64 hi / lo pairs)
    __device__ __forceinline__ merit_t<R> fphi(int e) const
    {
        if constexpr (sizeof(R) == 4 && !ALIP_LANE_M32)
            return (double)fph(e) + (double)fpl(e);
        else
            return fph(e);
    }
    __device__ __forceinline__ void set_fphi(int e, merit_t<R> v) const
    {
        if constexpr (sizeof(R) == 4 && !ALIP_LANE_M32) {
            const float hi = (float)v;
            fph(e) = hi;
            fpl(e) = (float)(v - (double)hi);
        } else {
            fph(e) = v;
        }
    }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(b)); }
};

// per-lane instance data (registers)
template <class R>
struct Inst {
    R x0[5];
    R gx, gy;    // goal after the detour heuristic
    int act;     // bit j: circle (form build: obstacle) slot j selected
    int legp;    // od_ev > 0
};

// a point of the NLP: states, their trig, the objective with its state-space gradient / Hessian parts
template <int N, class R>
struct Pt {
    R X[N + 1][5];
    R cs[N + 1], sn[N + 1];
    double f;         // the objective, summed in fp64 from the fp64 heading errors (the line search takes it as merit_t)
    R ph[N + 1];      // theta_k - atan2(goal - p_k): the objective's heading error (its gradient / Hessian parts are
                      // rebuilt per step in the row pass, obj_parts: kept for every step they held 72 VGPRs there)
};

// gradient [g0 g1 g2] and Hessian parts [h00 h01 h11 h04 h14 h44] of f_k on (px, py, theta) of x_k, in fp64 in both
// precisions (they go into the fp64 KKT system; in fp32 the curvature 1 / |g - p|^4 of a goal-frame position would
// overflow long before the position reaches the goal)
template <class R, class I>
__device__ __forceinline__ void obj_parts(const LK<R>& C, const I& in, int k, double px, double py, R ph_,
                                          double (&g)[3], double (&h)[6], double dfo, double ox, double oy)
{
    using D = double;
    // (dfo: IPOPT's objective scaling of this instance — the objective is linear in its weights)
    const D rw = dfo * (D)C[LK_R];
    const D w = dfo * ((D)C[LK_Q] + (k == 1 ? (D)C[LK_P] : D(0)));
    // (ox, oy: the goal frame's origin — the difference is taken in map coordinates, as the oracle rounds it; see
    // eval_states)
    const D dxg = ((D)in.gx + ox) - (px + ox), dyg = ((D)in.gy + oy) - (py + oy), ph = (D)ph_;
    // (p = goal exactly: the target heading's derivatives are 0 there instead of 0 / 0, DESIGN.md §2 item 7)
    const D rho2 = fma(dxg, dxg, dyg * dyg);
    const D ir2 = rho2 > D(0) ? rcp_nr(rho2) : D(0);
    const D gp0 = -dyg * ir2, gp1 = dxg * ir2;
    const D ir4 = ir2 * ir2;
    const D s00 = D(2) * dxg * dyg * ir4, s01 = (dyg * dyg - dxg * dxg) * ir4, s11 = D(-2) * dxg * dyg * ir4;
    g[0] = D(-2) * w * dxg + D(2) * rw * ph * gp0;
    g[1] = D(-2) * w * dyg + D(2) * rw * ph * gp1;
    g[2] = D(2) * rw * ph;
    h[0] = D(2) * w + D(2) * rw * (gp0 * gp0 - ph * s00);
    h[1] = D(2) * rw * (gp0 * gp1 - ph * s01);
    h[2] = D(2) * w + D(2) * rw * (gp1 * gp1 - ph * s11);
    h[3] = D(2) * rw * gp0;
    h[4] = D(2) * rw * gp1;
    h[5] = D(2) * rw;
}

// the heading error theta - atan2(goal - p): fp32 takes the difference in fp64 (the two angles are O(1) and their
// fp32 difference carries ~2e-7 of rounding, which the objective's gradient multiplies by 2 r / |g - p| near the goal:
// above the fp32 program's tol 1e-4 within ~0.5 m of the goal)
template <class R>
__device__ __forceinline__ R heading_error(R th, double dyg, double dxg)
{
    if constexpr (sizeof(R) == 4)
        return (R)((double)th - latan2_br(dyg, dxg));
    else
        return th - latan2_br(dyg, dxg);
}

template <int N, class R>
__device__ __forceinline__ void rollout(const LK<R>& C, const R (&x0)[5], const R (&p)[3 * N], R (&X)[N + 1][5])
{
    const R ch = C[LK_CH], shb = C[LK_SHB], bsh = C[LK_BSH], omc = C[LK_OMC];
#pragma unroll
    for (int c = 0; c < 5; ++c) X[0][c] = x0[c];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        X[k + 1][0] = fma(ch, X[k][0], fma(shb, X[k][2], omc * p[3 * k]));
        X[k + 1][1] = fma(ch, X[k][1], fma(shb, X[k][3], omc * p[3 * k + 1]));
        X[k + 1][2] = fma(bsh, X[k][0] - p[3 * k], ch * X[k][2]);
        X[k + 1][3] = fma(bsh, X[k][1] - p[3 * k + 1], ch * X[k][3]);
        X[k + 1][4] = X[k][4] + p[3 * k + 2];
    }
}

// the same affine map without x0: the state change of a foothold change dp
template <int N, class R>
__device__ __forceinline__ void lin_rollout(const LK<R>& C, const R (&dp)[3 * N], R (&dX)[N + 1][5])
{
    const R ch = C[LK_CH], shb = C[LK_SHB], bsh = C[LK_BSH], omc = C[LK_OMC];
#pragma unroll
    for (int c = 0; c < 5; ++c) dX[0][c] = R(0);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        dX[k + 1][0] = fma(ch, dX[k][0], fma(shb, dX[k][2], omc * dp[3 * k]));
        dX[k + 1][1] = fma(ch, dX[k][1], fma(shb, dX[k][3], omc * dp[3 * k + 1]));
        dX[k + 1][2] = fma(bsh, dX[k][0] - dp[3 * k], ch * dX[k][2]);
        dX[k + 1][3] = fma(bsh, dX[k][1] - dp[3 * k + 1], ch * dX[k][3]);
        dX[k + 1][4] = dX[k][4] + dp[3 * k + 2];
    }
}

// evaluate the point p: rollout, trig of theta_1..N, objective (MPC_LIP_modi.py:430-465) with its state-space
// gradient / Hessian parts.  One sincos / atan2 code copy: a runtime loop over the states.
// XP: the states x_1..x_N in the iterate's own type (fp32 build: the fp64 iterate, so that the objective's distance
// and heading terms near the goal are taken on exact differences and the exact heading)
template <int N, class R, class I, class XT>
__device__ __forceinline__ void eval_states(const LK<R>& C, const I& in, Pt<N, R>& pt, const XT (&XP)[N + 1][5],
                                            double dfo, double ox = 0.0, double oy = 0.0)
{
    pt.cs[0] = R(1);
    pt.sn[0] = R(0);
    double f = 0.0;
    const R rw = C[LK_R];
#pragma unroll 1
    for (int k = 1; k <= N; ++k) {
        R th = pt.X[1][4];
        XT px = XP[1][0], py = XP[1][1], thx = XP[1][4];
#pragma unroll
        for (int t = 2; t <= N; ++t) {
            th = k == t ? pt.X[t][4] : th;
            px = k == t ? XP[t][0] : px;
            py = k == t ? XP[t][1] : py;
            thx = k == t ? XP[t][4] : thx;
        }
        R sn_, cs_;
        lsincos_sel(th, &sn_, &cs_);
        const R w = C[LK_Q] + (k == 1 ? C[LK_P] : R(0));
        // goal - p in map coordinates (ox, oy: the goal frame's origin; 0 outside it): a goal-frame position converging
        // onto the goal keeps full relative precision down to 1e-300, where 1 / |g - p|^4 of the objective's curvature
        // overflowed (status -3 in the fp32 closed loop); the map-frame difference is exactly 0 there, as in the oracle
        const XT dxd = ((XT)in.gx + (XT)ox) - (px + (XT)ox), dyd = ((XT)in.gy + (XT)oy) - (py + (XT)oy);
        R ph;
        if constexpr (sizeof(R) == 4) {
            const double phd = (double)thx - latan2_br((double)dyd, (double)dxd);
            ph = (R)phd;
            f += (double)w * fma((double)dxd, (double)dxd, (double)dyd * (double)dyd) + (double)rw * phd * phd;
        } else {
            ph = heading_error<R>(th, (double)dyd, (double)dxd);
            f += w * fma(dxd, dxd, dyd * dyd) + rw * ph * ph;
        }
#pragma unroll
        for (int t = 1; t <= N; ++t) {
            const bool me = k == t;
            pt.cs[t] = me ? cs_ : pt.cs[t];
            pt.sn[t] = me ? sn_ : pt.sn[t];
            pt.ph[t] = me ? ph : pt.ph[t];
        }
    }
    pt.f = dfo == 1.0 ? f : dfo * f;   // (IPOPT's objective scaling of the instance)
}
template <int N, class R, class I>
__device__ __forceinline__ void eval_point(const LK<R>& C, const I& in, const R (&p)[3 * N], Pt<N, R>& pt, double dfo)
{
    rollout<N, R>(C, in.x0, p, pt.X);
    eval_states<N, R>(C, in, pt, pt.X, dfo);
}

// the quantities of one step k (runtime) of a point
template <class R>
struct Step {
    R x1[5], x0[5];   // x_{k+1}, x_k
    R c1, s1;         // cos / sin theta_{k+1}
    R fx, fy, ft;     // p_k
};
template <int N, class R>
__device__ __forceinline__ Step<R> step_of(const R (&X)[N + 1][5], const R (&cs)[N + 1], const R (&sn)[N + 1],
                                           const R (&p)[3 * N], int k)
{
    Step<R> st;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        R a = X[0][c], b1 = X[1][c];
#pragma unroll
        for (int t = 1; t < N; ++t) {
            a = k == t ? X[t][c] : a;
            b1 = k == t ? X[t + 1][c] : b1;
        }
        st.x0[c] = a;
        st.x1[c] = b1;
    }
    R c1 = cs[1], s1 = sn[1], fx = p[0], fy = p[1], ft = p[2];
#pragma unroll
    for (int t = 1; t < N; ++t) {
        c1 = k == t ? cs[t + 1] : c1;
        s1 = k == t ? sn[t + 1] : s1;
        fx = k == t ? p[3 * t] : fx;
        fy = k == t ? p[3 * t + 1] : fy;
        ft = k == t ? p[3 * t + 2] : ft;
    }
    st.c1 = c1; st.s1 = s1; st.fx = fx; st.fy = fy; st.ft = ft;
    return st;
}

// row value and its state-space coefficients.  Generators per kind:
//   VEL (vbx, vby, f_en halves): [vx, vy, theta of x_{k+1}, dth_k]   CIR: [px, py of x_{k+1}, px, py of x_k]
//   LEG: [px, py of x_k, fx_k, fy_k]                                   DTH: [dth_k]
template <int KD, class R>
__device__ __forceinline__ R row_eval(const LK<R>& C, const Step<R>& st, R ox, R oy, R rr, R (&cf)[4])
{
    cf[0] = cf[1] = cf[2] = cf[3] = R(0);
    if constexpr (KD == VBX || KD == VBY || KD == FEN || KD == FENM) {
        const R vx = st.x1[2], vy = st.x1[3];
        const R vbx = fma(st.c1, vx, st.s1 * vy), vby = fma(st.c1, vy, -st.s1 * vx);
        if constexpr (KD == VBY) {
            cf[0] = -st.s1; cf[1] = st.c1; cf[2] = -vbx;
            return vby;
        } else {
            cf[0] = st.c1; cf[1] = st.s1; cf[2] = vby;
            if constexpr (KD == VBX) {
                return vbx;
            } else {
                const R sw = KD == FEN ? C[LK_S] : -C[LK_S];
                cf[3] = sw;
                return fma(sw, st.ft, vbx);
            }
        }
    } else if constexpr (KD == CIR) {
        const R gm1 = C[LK_GM1];
        const R x1 = st.x1[0] - ox, y1 = st.x1[1] - oy, x0 = st.x0[0] - ox, y0 = st.x0[1] - oy;
        cf[0] = R(2) * x1; cf[1] = R(2) * y1; cf[2] = R(2) * gm1 * x0; cf[3] = R(2) * gm1 * y0;
        return (fma(x1, x1, y1 * y1) - rr) + gm1 * (fma(x0, x0, y0 * y0) - rr);
    } else if constexpr (KD == LEG) {
        const R ex = st.x0[0] - st.fx, ey = st.x0[1] - st.fy;
        cf[0] = R(2) * ex; cf[1] = R(2) * ey; cf[2] = R(-2) * ex; cf[3] = R(-2) * ey;
        return fma(ex, ex, ey * ey);
    } else {
        cf[0] = R(1);
        return st.ft;
    }
}

// the form build's obstacle row (kind FRM): h(p) = qa dx^2 + qb dx dy + qc dy^2 - k, d = p - (ox, oy), and the D-CBF
// row c = h(x_{k+1}) + (gamma - 1) h(x_k) (MPC_LIP_modi.py:598-617), coefficients on the CIR generators
template <class R>
__device__ __forceinline__ R form_eval(const LK<R>& C, const Step<R>& st, R ox, R oy, R qa, R qb, R qc, R kk, R (&cf)[4])
{
    const R gm1 = C[LK_GM1];
    const R x1 = st.x1[0] - ox, y1 = st.x1[1] - oy, x0 = st.x0[0] - ox, y0 = st.x0[1] - oy;
    cf[0] = fma(R(2) * qa, x1, qb * y1);
    cf[1] = fma(R(2) * qc, y1, qb * x1);
    cf[2] = gm1 * fma(R(2) * qa, x0, qb * y0);
    cf[3] = gm1 * fma(R(2) * qc, y0, qb * x0);
    const R h1 = fma(qa * x1, x1, fma(qb * x1, y1, qc * y1 * y1)) - kk;
    const R h0 = fma(qa * x0, x0, fma(qb * x0, y0, qc * y0 * y0)) - kk;
    return fma(gm1, h0, h1);
}
// a row's value and coefficients with its obstacle slot's entries (slot j) read from LDS where they are used
template <int KD, class R, class LD>
__device__ __forceinline__ R row_value(const LK<R>& C, const Step<R>& st, const LD& ld, int j, R (&cf)[4])
{
    if constexpr (KD == FRM)
        return form_eval<R>(C, st, ld.ox(j), ld.oy(j), ld.qa(j), ld.qb(j), ld.qc(j), ld.orr(j), cf);
    else
        return row_eval<KD, R>(C, st, KD == CIR ? ld.ox(j) : R(0), KD == CIR ? ld.oy(j) : R(0),
                               KD == CIR ? ld.orr(j) : R(0), cf);
}

// relaxed (IPOPT bound_relax_factor 1e-8, as the oracle) or original bounds of a row of kind KD at step k
template <int KD, class R>
__device__ __forceinline__ void row_bounds(const LK<R>& C, int legp, int k, R& cl, R& cu, bool orig = false)
{
    const bool pos = (legp != 0) == ((k & 1) == 0);
    const int o = orig ? LK_OVXL - LK_VXL : 0;
    if constexpr (KD == VBX) {
        cl = C[LK_VXL + o]; cu = C[LK_VXU + o];
    } else if constexpr (KD == VBY) {
        cl = pos ? C[LK_VYLP + o] : C[LK_VYLN + o];
        cu = pos ? C[LK_VYUP + o] : C[LK_VYUN + o];
    } else if constexpr (is_obs<KD>()) {
        cl = orig ? R(0) : C[LK_CIRL]; cu = R(INFINITY);
    } else if constexpr (KD == LEG) {
        cl = orig ? R(0) : C[LK_LEGL]; cu = orig ? C[LK_OLEGU] : C[LK_LEGU];
    } else if constexpr (KD == DTH) {
        cl = orig ? -C[LK_ODT] : C[LK_DTL]; cu = orig ? C[LK_ODT] : C[LK_DTU];
    } else {
        cl = R(-INFINITY); cu = orig ? C[LK_OVXU] : C[LK_VXU];
    }
}
template <int KD>
constexpr bool has_lo() { return KD != FEN && KD != FENM; }
template <int KD>
constexpr bool has_up() { return !is_obs<KD>(); }

// every row of step k: f(KindT<kind>, l (row within the step), j (obstacle slot)); circle / form rows in a loop
template <int NC, bool MODI, bool FM = false, class F>
__device__ __forceinline__ void step_rows(F&& f)
{
    f(KindT<VBX>(), 0, 0);
    f(KindT<VBY>(), 1, 0);
#pragma unroll 1
    for (int j = 0; j < NC; ++j) f(KindT<FM ? FRM : CIR>(), 2 + j, j);
    f(KindT<LEG>(), 2 + NC, 0);
    f(KindT<DTH>(), 3 + NC, 0);
    if constexpr (MODI) {
        f(KindT<FEN>(), 4 + NC, 0);
        f(KindT<FENM>(), 5 + NC, 0);
    }
}

// z_l / z_u index of row l of step k (rows without that bound: unused)
template <int N, int NC, bool MODI>
__device__ __forceinline__ int zl_index(int k, int l) { return k * Shape<N, NC, MODI>::ZLS + l; }
template <int N, int NC, bool MODI>
__device__ __forceinline__ int zu_index(int k, int l)
{
    return k * Shape<N, NC, MODI>::ZUS + (l < 2 ? l : l - NC);
}

// IPOPT's slack push (oracle push_slacks) onto the relaxed bounds
template <class R>
__device__ __forceinline__ R push_slack(R v, R cl, R cu, bool hl, bool hu)
{
    const R pl = hl ? fmin(R(1e-2) * fmax(R(1), fabs(cl)), R(1e-2) * (cu - cl)) : R(0);
    const R pu = hu ? fmin(R(1e-2) * fmax(R(1), fabs(cu)), R(1e-2) * (cu - cl)) : R(0);
    if (hl && hu) return fmin(fmax(v, cl + pl), cu - pu);
    if (hl) return fmax(v, cl + pl);
    if (hu) return fmin(v, cu - pu);
    return v;
}

// foothold-space sensitivities of step k (wave-uniform): columns j = 0..N-1 of each axis
template <int N, class R>
struct Sens {
    R sp1[N], sv1[N], sp0[N], t1[N], e[N];   // d px_{k+1}, d vx_{k+1}, d px_k / d fx_j; d theta_{k+1} / d dth_j; j == k
};
template <int N, class R, class RK>
__device__ __forceinline__ Sens<N, RK> sens_of(const LK<R>& C, int k)
{
    Sens<N, RK> z;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int m1 = k - j < 0 ? 0 : k - j, m0 = k - 1 - j < 0 ? 0 : k - 1 - j;
        z.sp1[j] = j <= k ? (RK)C[LK_SP + m1] : RK(0);
        z.sv1[j] = j <= k ? (RK)C[LK_SV + m1] : RK(0);
        z.sp0[j] = j < k ? (RK)C[LK_SP + m0] : RK(0);
        z.t1[j] = j <= k ? RK(1) : RK(0);
        z.e[j] = j == k ? RK(1) : RK(0);
    }
    return z;
}

// K (lower triangle) += sg jr jr^T over the axes AX (bit 0: x columns 3j, bit 1: y 3j+1, bit 2: theta 3j+2)
template <int n, int AX, class RK>
__device__ __forceinline__ void kupd(RK (&K)[n][n], const RK (&jr)[n], RK sg)
{
#pragma unroll
    for (int a = 0; a < n; ++a) {
        if (!((AX >> (a % 3)) & 1)) continue;
        const RK sj = sg * jr[a];
#pragma unroll
        for (int b = 0; b <= a; ++b)
            if ((AX >> (b % 3)) & 1) K[a][b] = fma(sj, jr[b], K[a][b]);
    }
}
template <int n, class RK>
__device__ __forceinline__ void ksym(RK (&K)[n][n], int a, int b, RK v)
{
    if (a >= b) K[a][b] += v;
    else K[b][a] += v;
}

}  // namespace lane

#ifndef ALIP_F32_FLOOR
#define ALIP_F32_FLOOR 8   // the fp32 stationarity floor: this many units of 2^-24 of sum |J_r y_r|
#endif
// refill the wave's idle lanes once at least this many are idle (or none is busy): 8 of the fp32 build's 64 lanes, 4 of
// the fp64 build's 32 (r5, profiles/r5/ab/r5x_refill_groups.log: fp32 4 / 8 / 16 / 32 = 15.95 / 15.71 / 16.2 / 17.5 ms on
// cfg5; fp64 4 / 8 / 16 = 8.87 / 9.01 / 10.0 ms on cfg4)
#ifndef ALIP_LANE_REFILL
#define ALIP_LANE_REFILL 8
#endif
#ifndef ALIP_LANE_REFILL_F64
#define ALIP_LANE_REFILL_F64 4
#endif

// R: arithmetic of the rows, line search and state (cfg.precision); the KKT system (K, its Cholesky factor,
// the right-hand side and the multiplier sums) is fp64 in both precisions.
//
// A lane's pass: phase 0 (take an instance), phase 1 (one evaluation at p and ONE pass over the rows: the
// pending update of the previous iteration — accepted step, restoration reset or initial point — is
// applied to the slacks and multipliers in the same pass that assembles K, the right-hand side and the
// error terms; then the barrier update, the factorisation and one pass for dS and the step bounds), phase 2
// (one line-search trial: one evaluation and one pass).  A rejected trial keeps the lane in phase 2.
//
// RT: R itself (NC circle slots), or lane::Form<R> — the form build: NC obstacle-form slots (circles and ellipses,
// modi) in their place, a kernel of its own name (lane_kernel<N, NS, true, alip::lane::Form<R>>).  Its entry count per
// lane at N = 3: 2 * 3 * (6 + NS) + 3 * (4 + NS) + 18 + 6 * NS + 16 = 157 at NS = 5; four one-wave workgroups per CU
// need <= 160 entries (160 x 256 B x 4 = the CU's 160 KB), NS = 6 has 172.
template <int N, int NC, bool MODI, class RT>
__global__ __launch_bounds__(64, 1) void lane_kernel(KP P)
{
    using namespace lane;
    using R = typename Real<RT>::type;
    constexpr bool FM = Real<RT>::form;
    static_assert(!FM || MODI, "the form build is modi's (sig_step has no ellipse rows)");
    using RK = double;
    using S = Shape<N, NC, MODI>;
    constexpr int n = S::n, RPS = S::RPS;
    constexpr int L = lanes_of<R>();
    constexpr int NKL = n * (n + 1) / 2;
    constexpr int U_NONE = 0, U_INIT = 1, U_ACC = 2, U_REST = 3;   // pending update kinds
    using LD = Lds<R, N, NC, MODI, L, FM ? 6 : 3>;
    static_assert(!FM || LD::ENT <= 160, "a form build above 160 LDS entries per lane loses the fourth wave of a CU");
    __shared__ R smem_[LD::ENT * L];
    const int lane = threadIdx.x;
    LD ld;
    ld.b = (typename LD::lptr)(smem_ + (lane < L ? lane : 0));   // lanes >= L hold no instance
    uint32_t* const q = P.queue;
    const long long B = P.B;
    const int max_iter = P.max_iter;
    const R gth = R(1e-5), gph = R(1e-8), sth = R(1.1), sph = R(2.3), eta = R(1e-8), gal = R(0.05);

    // ---- per-lane state (registers).  fp32 keeps the states x_1..x_N and moves them with the step
    // (x + a dx, as solve_kernel's V + a dV): re-rolling them out of the footholds through A^k every
    // evaluation amplifies fp32 rounding into objective noise above the line search's decrease tests
    // (measured: 46 % vs 85 % solved at the cap).  fp64 rolls out of the footholds as the oracle does.
    constexpr bool INC = sizeof(R) == 4;
    // fp32 also works in the frame of the instance's (local) goal: the NLP is invariant under a common shift of
    // every position (x_{k+1} = A x_k + B p_k with A's position rows summing to 1 with B's; rows and objective use
    // position differences only), and near the goal — where the heading term's curvature grows as 1 / |g - p|^2 —
    // goal-relative fp32 positions keep their relative precision instead of the 1e-6 m of a map coordinate of
    // 10 m.  The shift is taken and undone in fp64 (org: the goal in map coordinates).
#ifndef ALIP_LANE_GOAL_FRAME
#define ALIP_LANE_GOAL_FRAME 1
#endif
    constexpr bool GF = INC && ALIP_LANE_GOAL_FRAME;
    double orgx = 0.0, orgy = 0.0;
    double dfo = 1.0;   // IPOPT's objective scaling of the lane's instance (set up in phase 0)
    Inst<R> in;
    // fp32: the iterate itself — footholds p and states Xs — is kept in fp64 (RP), the rows and the line search's
    // arithmetic in fp32.  Near the goal the objective's curvature (2 r / |g - p|^2, 10^4 at 10 cm) turns the 3e-8
    // resolution of an fp32 position of ~0.3 m into stationarity noise above tol 1e-4, and an fp32 iterate cannot move
    // by the Newton steps that would remove it (r5: tools/cl_fp32_study.py, the dual infeasibility of the fp32 loop's
    // extra iteration-cap stops, in the first foothold's x / y, grew as 1 / |g - p|)
    using RP = typename std::conditional<INC, double, R>::type;
    RP p[n];
    R dU[n];
    RP Xs[INC ? N + 1 : 1][5];
    R mu = R(0), thmax = R(0), thmin = R(0);
    using MT = merit_t<R>;
    MT fcur = MT(0), lcur = MT(0);   // objective and log-barrier sum at the iterate
    RK dwl = RK(0);   // last regularisation (fp64 in both precisions, as the KKT system it regularises)
    R mact = R(0), nbl = R(0);
    R a = R(0), la = R(0), amin = R(0), theta = R(0), lsw = R(0), az = R(0);
    MT phi = MT(0), gphi = MT(0);   // barrier function and its directional derivative
    int phase = 0, it = 0, nrest = 0, nf = 0, upd = U_NONE;
    long long b = -1;
    bool qdone = false, first = true;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        p[i] = RP(0);
        dU[i] = R(0);
    }
#pragma unroll
    for (int k = 0; k < (INC ? N + 1 : 1); ++k)
#pragma unroll
        for (int c = 0; c < 5; ++c) Xs[k][c] = RP(0);
    in.act = 0;
    in.legp = 0;

    for (;;) {
        // ================= phase 0: take instances from the work queue, load and set them up
        {
            const LK<double> CD = lk_of<double>(P);
            ld.launder();
            const unsigned long long idle = __ballot(phase == 0 && lane < L);
            const int nidle = __builtin_popcountll(idle);
            if (!qdone && (nidle >= (sizeof(R) == 8 ? ALIP_LANE_REFILL_F64 : ALIP_LANE_REFILL) || nidle == L || first)) {
                int want = nidle;
                if (first) {
                    // first fetch: a small batch is spread over every resident wave (latency = one instance)
                    const long long per = (B + (long long)gridDim.x - 1) / (long long)gridDim.x;
                    want = (int)(per < (long long)nidle ? per : (long long)nidle);
                }
                first = false;
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(q, (uint32_t)want);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if ((long long)base + want >= B) qdone = true;
                const int rank = __builtin_popcountll(idle & ((1ull << lane) - 1ull));
                const long long bb = (long long)base + rank;
                if (phase == 0 && lane < L && rank < want && bb < B && (!P.active || P.active[bb])) {
                    b = bb;
                    // (fp64: the discrete selections do not depend on precision)
                    const double* xp = P.x0 + 5 * b;
                    double x0d[5];
#pragma unroll
                    for (int c = 0; c < 5; ++c) x0d[c] = xp[c];
                    double g0 = P.goal[2 * b], g1 = P.goal[2 * b + 1];
                    in.legp = P.leg[b] > 0;
                    const int ncr = P.nc[b];
                    int ner = 0;
                    if constexpr (FM) ner = P.ne ? P.ne[b] : 0;
                    in.act = 0;
                    // select_obs (MPC_LIP_modi.py:325-338) and the detour goal (MPC_LIP_modi.py:247-271): the
                    // first selected circle, in input order, that triggers
                    bool fired = false;
                    double nx = g0, ny = g1;
                    const double gd = fma(x0d[0] - g0, x0d[0] - g0, (x0d[1] - g1) * (x0d[1] - g1));
#pragma unroll 1
                    for (int j = 0; j < NC; ++j) {
                        double ox = 0.0, oy = 0.0, orr = 0.0;
                        bool keep = false;
                        if (j < ncr && j < P.nc_max) {
                            const double* c = P.cir + ((size_t)b * P.nc_max + j) * 3;
                            ox = c[0]; oy = c[1]; orr = c[2];
                            const double cen = fma(x0d[0] - ox, x0d[0] - ox, (x0d[1] - oy) * (x0d[1] - oy));
                            keep = !P.select_obs || cen - orr * orr <= P.detect_r2;
                            if (keep && P.detour && !fired && cen < gd && cen < 9 * orr * orr) {
                                const double th = latan2_br(g1 - x0d[1], g0 - x0d[0]);
                                const double al = latan2_br(oy - x0d[1], ox - x0d[0]);
                                double dd = th - al;
                                if (dd < 0 && fabs(dd) > M_PI)
                                    dd += 2 * M_PI;
                                else if (dd > 0 && fabs(dd) > M_PI)
                                    dd -= 2 * M_PI;
                                if (fabs(dd) < M_PI / 12) {
                                    fired = true;
                                    const double na = dd < 0 ? th - M_PI / 12 : th + M_PI / 12;
                                    const double rg = sqrt(gd);
                                    double sn_, cs_;
                                    lsincos_sel(na, &sn_, &cs_);
                                    nx = fma(rg, cs_, x0d[0]);
                                    ny = fma(rg, sn_, x0d[1]);
                                }
                            }
                        }
                        double fqa = 0.0, fqb = 0.0, fqc = 0.0, fk = 0.0;
                        if constexpr (FM) {
                            // every entry of the slot is written for every instance: a circle is the form qa = qc = 1,
                            // qb = 0, k = r^2; an unused slot is all zeros.  An ellipse [cx, cy, a, b, phi] in slot
                            // nc_max + e: np_oracle.select_obs's range test on max(a, b), the coefficients in fp64
                            // (oracle/np_oracle.py:198-203); it never fires the detour.
                            const bool cs = j < ncr && j < P.nc_max;
                            fqa = fqc = cs ? 1.0 : 0.0;
                            fk = orr * orr;
                            const int e = j - P.nc_max;
                            if (e >= 0 && e < ner && e < P.ne_max) {
                                const double* c = P.elp + ((size_t)b * P.ne_max + e) * 5;
                                ox = c[0]; oy = c[1];
                                const double ea = c[2], eb = c[3];
                                const double rm = ea > eb ? ea : eb;
                                const double cen = fma(x0d[0] - ox, x0d[0] - ox, (x0d[1] - oy) * (x0d[1] - oy));
                                keep = !P.select_obs || cen - rm * rm <= P.detect_r2;
                                double se, ce;
                                lsincos_sel(c[4], &se, &ce);
                                fqa = (eb * ce) * (eb * ce) + (ea * se) * (ea * se);
                                fqb = 2 * ce * se * (eb * eb - ea * ea);
                                fqc = (eb * se) * (eb * se) + (ea * ce) * (ea * ce);
                                fk = (eb * ea) * (eb * ea);
                            }
                        }
                        in.act |= keep ? 1 << j : 0;
                        ld.ox(j) = (R)ox;   // (goal frame: shifted below, once the goal is known)
                        ld.oy(j) = (R)oy;
                        if constexpr (FM) {
                            ld.orr(j) = (R)fk;
                            ld.qa(j) = (R)fqa;
                            ld.qb(j) = (R)fqb;
                            ld.qc(j) = (R)fqc;
                        } else {
                            ld.orr(j) = (R)(orr * orr);
                        }
                    }
                    if constexpr (GF) {
                        orgx = nx;
                        orgy = ny;
#pragma unroll 1
                        for (int j = 0; j < NC; ++j) {
                            if (j < ncr && j < P.nc_max) {
                                const double* c = P.cir + ((size_t)b * P.nc_max + j) * 3;
                                ld.ox(j) = (R)(c[0] - nx);
                                ld.oy(j) = (R)(c[1] - ny);
                            }
                            if constexpr (FM) {
                                const int e = j - P.nc_max;
                                if (e >= 0 && e < ner && e < P.ne_max) {
                                    const double* c = P.elp + ((size_t)b * P.ne_max + e) * 5;
                                    ld.ox(j) = (R)(c[0] - nx);
                                    ld.oy(j) = (R)(c[1] - ny);
                                }
                            }
                        }
                    }
                    // warm start: p0_k = W (u0_k - A x_k), x_{k+1} = A x_k + B p0_k (the rollout of u0)
                    {
                        const double ch = CD[LK_CH], shb = CD[LK_SHB], bsh = CD[LK_BSH], omc = CD[LK_OMC];
                        const double Wc = CD[LK_WCH], Ws = CD[LK_WSH];
                        double x[5];
#pragma unroll
                        for (int c = 0; c < 5; ++c) x[c] = x0d[c];
                        const double* u0 = P.u0 + (size_t)b * 5 * N;
                        // the objective's gradient on (px, py, theta) of x_{k+1} at the starting point, for IPOPT's
                        // scaling (nlp_scaling_method = gradient-based, MPC_LIP_modi.py:274-296 sets no scaling option)
                        double ogx[N], ogy[N], ogt[N];
#pragma unroll
                        for (int k = 0; k < N; ++k) {
                            const double ax0 = ch * x[0] + shb * x[2], ax1 = ch * x[1] + shb * x[3];
                            const double ax2 = bsh * x[0] + ch * x[2], ax3 = bsh * x[1] + ch * x[3];
                            const double fx = Wc * (u0[5 * k] - ax0) + Ws * (u0[5 * k + 2] - ax2);
                            const double fy = Wc * (u0[5 * k + 1] - ax1) + Ws * (u0[5 * k + 3] - ax3);
                            const double ft = u0[5 * k + 4] - x[4];
                            p[3 * k] = (RP)(fx - orgx);
                            p[3 * k + 1] = (RP)(fy - orgy);
                            p[3 * k + 2] = (RP)ft;
                            x[0] = ax0 + omc * fx;
                            x[1] = ax1 + omc * fy;
                            x[2] = ax2 - bsh * fx;
                            x[3] = ax3 - bsh * fy;
                            x[4] = x[4] + ft;
                            {
                                const double wq = CD[LK_Q] + (k == 0 ? CD[LK_P] : 0.0), rw = CD[LK_R];
                                const double dxg = nx - x[0], dyg = ny - x[1];
                                const double rho2 = fma(dxg, dxg, dyg * dyg), ir2 = rho2 > 0.0 ? 1.0 / rho2 : 0.0;
                                const double ph = x[4] - latan2_br(dyg, dxg);
                                ogx[k] = -2.0 * wq * dxg + 2.0 * rw * ph * (-dyg * ir2);
                                ogy[k] = -2.0 * wq * dyg + 2.0 * rw * ph * (dxg * ir2);
                                ogt[k] = 2.0 * rw * ph;
                            }
                            if constexpr (INC) {
                                Xs[k + 1][0] = (RP)(x[0] - orgx);
                                Xs[k + 1][1] = (RP)(x[1] - orgy);
#pragma unroll
                                for (int c = 2; c < 5; ++c) Xs[k + 1][c] = (RP)x[c];
                            }
                        }
                        // the gradient in the reference's u (d x_{k+1+m} / d u_k per axis: SU0 / SU1; theta_{k+1} = u_k[4])
                        // and the scale 100 / max |grad| where that exceeds 100 (nlp_scaling_max_gradient)
                        double gmax = 0.0;
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            double gpx = 0.0, gvx = 0.0, gpy = 0.0, gvy = 0.0;
#pragma unroll
                            for (int k = j; k < N; ++k) {
                                const double s0 = CD[LK_SU0 + (k - j)], s1 = CD[LK_SU1 + (k - j)];
                                gpx = fma(ogx[k], s0, gpx);
                                gvx = fma(ogx[k], s1, gvx);
                                gpy = fma(ogy[k], s0, gpy);
                                gvy = fma(ogy[k], s1, gvy);
                            }
                            gmax = fmax(gmax, fmax(fmax(fabs(gpx), fabs(gvx)), fmax(fmax(fabs(gpy), fabs(gvy)), fabs(ogt[j]))));
                        }
                        dfo = gmax > 100.0 ? fmax(1e-8, 100.0 / gmax) : 1.0;
                        if constexpr (INC) {
                            Xs[0][0] = (RP)(x0d[0] - orgx);
                            Xs[0][1] = (RP)(x0d[1] - orgy);
#pragma unroll
                            for (int c = 2; c < 5; ++c) Xs[0][c] = (RP)x0d[c];
                        }
                    }
                    in.x0[0] = (R)(x0d[0] - orgx);
                    in.x0[1] = (R)(x0d[1] - orgy);
#pragma unroll
                    for (int c = 2; c < 5; ++c) in.x0[c] = (R)x0d[c];
                    in.gx = (R)(nx - orgx);   // (0 in the goal frame)
                    in.gy = (R)(ny - orgy);
                    dwl = RK(0);
                    nf = 0;
                    it = 0;
                    nrest = 0;
                    upd = U_INIT;   // slacks, multipliers, barrier terms at the first evaluation (phase 1)
                    phase = 1;
                }
            }
            const bool busy = __ballot(phase != 0) != 0ull;
            if (!busy && qdone) break;
            if (!busy) continue;
        }

        // ================= phase 1
        if (phase == 1) {
            const LK<R> C = lk_of<R>(P);
            ld.launder();
            Pt<N, R> pt;
            if constexpr (INC) {
#pragma unroll
                for (int k = 0; k <= N; ++k)
#pragma unroll
                    for (int c = 0; c < 5; ++c) pt.X[k][c] = (R)Xs[k][c];
                eval_states<N, R>(C, in, pt, Xs, dfo, orgx, orgy);
            } else {
                eval_point<N, R>(C, in, p, pt, dfo);
            }
            R pr[n];   // the footholds in the rows' arithmetic
#pragma unroll
            for (int i = 0; i < n; ++i) pr[i] = (R)p[i];
            int status = -1;
            bool done = false;
#ifdef ALIP_LANE_DBG
            // (diagnostic build, tools/cl_fp32_study.py: the last convergence test's terms replace x_pred)
            double dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
            RK K[n][n];
            RK gl[n], pw1[n], pw2[n], gf[n];
            // fp32: per column, sum |J_r y_r| — the rounding floor of the stationarity residual (below)
            RK ga[INC ? n : 1];
#pragma unroll
            for (int i = 0; i < n; ++i) {
                gl[i] = pw1[i] = pw2[i] = gf[i] = RK(0);
#pragma unroll
                for (int j = 0; j < n; ++j) K[i][j] = RK(0);
            }
#pragma unroll
            for (int i = 0; i < (INC ? n : 1); ++i) ga[i] = RK(0);
            // error terms; complementarity products w = dl z_l, du z_u: their max / min give the barrier
            // update's max |w - mu| for every candidate mu without another pass (|w - mu| peaks at an extreme w)
            R rcm = R(0), nz = R(0), wmax = R(-INFINITY), wmin = R(INFINITY), violc = R(0), violo = R(0);
            R th0 = R(0), ma = R(0), nb = R(0);
            MT lsum = MT(0);
            const int u = upd;
            const R au = a, azu = az, muu = mu;   // the pending update's step, z step and barrier parameter
#pragma unroll 1
            for (int k = 0; k < N; ++k) {
                const Step<R> st = step_of<N, R>(pt.X, pt.cs, pt.sn, pr, k);
                const Sens<N, RK> z = sens_of<N, double, RK>(lk_of<double>(P), k);   // (fp64 constants in both builds)
                // state-space Hessian parts: x_{k+1} (velocity / circle rows of step k, here; the objective f_{k+1}
                // after the rows) and x_k (the circle rows' gamma - 1 terms)
                R hp[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) hp[t] = R(0);
                R h0x = R(0);
                R hxy = R(0), h0y = R(0), h0xy = R(0);   // (form build: the forms' cross terms and the y part on x_k)
                R prod = R(1);
                step_rows<NC, MODI, FM>([&](auto KD_, int l, int j) {
                    constexpr int KD = decltype(KD_)::value;
                    const int i = k * RPS + l;
                    R cf[4], cl, cu, clo, cuo;
                    const R c = row_value<KD, R>(C, st, ld, j, cf);
                    row_bounds<KD, R>(C, in.legp, k, cl, cu);
                    row_bounds<KD, R>(C, in.legp, k, clo, cuo, true);
                    const bool act = !is_obs<KD>() || ((in.act >> j) & 1);
                    const int zli_ = zl_index<N, NC, MODI>(k, l), zui_ = zu_index<N, NC, MODI>(k, l);
                    R si = ld.s(i);
                    R zli = has_lo<KD>() ? ld.zl(zli_) : R(0);
                    R zui = has_up<KD>() ? ld.zu(zui_) : R(0);
                    // ---- the pending update
                    if (u == U_INIT) {
                        // IPOPT's initial slacks (pushed into the bounds) and z = 1 on every bound
                        si = act ? push_slack(c, cl, cu, has_lo<KD>(), has_up<KD>()) : R(0);
                        zli = has_lo<KD>() && act ? R(1) : R(0);
                        zui = has_up<KD>() && act ? R(1) : R(0);
                        th0 += act ? fabs(c - si) : R(0);
                        ma += act ? R(1) : R(0);
                        nb += act ? R((int)has_lo<KD>() + (int)has_up<KD>()) : R(0);
                    } else if (u != U_NONE) {
                        // accepted step s + a dS, or the restoration reset onto c(p); then the direction's z step
                        // (dZ from the slacks before the update) and the clamp at the new slacks
                        const R dsv = ld.ds(i);
                        const R sn_ = u == U_ACC ? fma(au, dsv, si) : (act ? push_slack(c, cl, cu, has_lo<KD>(), has_up<KD>()) : R(0));
                        if constexpr (has_lo<KD>()) {
                            const R idl = rcp_nr(si - cl), idn = rcp_nr(sn_ - cl);
                            const R zz = fma(azu, muu * idl - zli - zli * idl * dsv, zli);
                            zli = act ? fmin(fmax(zz, muu * R(1e-10) * idn), R(1e10) * muu * idn) : R(0);
                            if (act) violo = fmax(violo, clo - c);
                        }
                        if constexpr (has_up<KD>()) {
                            const R idu = rcp_nr(cu - si), idn = rcp_nr(cu - sn_);
                            const R zz = fma(azu, muu * idu - zui + zui * idu * dsv, zui);
                            zui = act ? fmin(fmax(zz, muu * R(1e-10) * idn), R(1e10) * muu * idn) : R(0);
                            if (act) violo = fmax(violo, c - cuo);
                        }
                        si = sn_;
                    }
                    if (u != U_NONE) {
                        ld.s(i) = si;
                        if constexpr (has_lo<KD>()) ld.zl(zli_) = zli;
                        if constexpr (has_up<KD>()) ld.zu(zui_) = zui;
                    }
                    // barrier terms of the new slacks (initial point / restoration)
                    {
                        R t = R(1);
                        if constexpr (has_lo<KD>()) t = act ? si - cl : R(1);
                        if constexpr (has_up<KD>()) t = act ? t * (cu - si) : t;
                        prod *= t;
                        if constexpr (sizeof(R) == 4) {   // fp32: one log per row (log(dl du), as solve_kernel)
                            lsum += (u == U_INIT || u == U_REST) ? (MT)llog(prod) : MT(0);
                            prod = R(1);
                        }
                    }
                    // ---- assembly
                    const R dl = si - cl, du = cu - si;
                    const R idl = has_lo<KD>() && act ? rcp_nr(dl) : R(0);
                    const R idu = has_up<KD>() && act ? rcp_nr(du) : R(0);
                    const R y = zli - zui;
                    const RK sg = (RK)zli * (RK)idl + (RK)zui * (RK)idu;
                    const R rc = act ? c - si : R(0);
                    rcm = fmax(rcm, fabs(rc));
                    nz += fabs(zli) + fabs(zui);
                    if (has_lo<KD>() && act) {
                        const R w = dl * zli;
                        wmax = fmax(wmax, w);
                        wmin = fmin(wmin, w);
                        violc = fmax(violc, clo - c);
                    }
                    if (has_up<KD>() && act) {
                        const R w = du * zui;
                        wmax = fmax(wmax, w);
                        wmin = fmin(wmin, w);
                        violc = fmax(violc, c - cuo);
                    }
                    const RK wm = (RK)idl - (RK)idu, wr = -sg * (RK)rc;   // rhs weight = mu wm + wr
                    // Jacobian row in foothold space (x, y, theta columns of steps j <= k)
                    RK jr[n];
#pragma unroll
                    for (int t = 0; t < n; ++t) jr[t] = RK(0);
                    constexpr int AX = (is_obs<KD>() || KD == LEG) ? 3 : KD == DTH ? 4 : 7;
#pragma unroll
                    for (int t = 0; t < N; ++t) {
                        if constexpr (is_obs<KD>()) {
                            jr[3 * t] = fma((RK)cf[0], z.sp1[t], (RK)cf[2] * z.sp0[t]);
                            jr[3 * t + 1] = fma((RK)cf[1], z.sp1[t], (RK)cf[3] * z.sp0[t]);
                        } else if constexpr (KD == LEG) {
                            jr[3 * t] = fma((RK)cf[0], z.sp0[t], (RK)cf[2] * z.e[t]);
                            jr[3 * t + 1] = fma((RK)cf[1], z.sp0[t], (RK)cf[3] * z.e[t]);
                        } else if constexpr (KD == DTH) {
                            jr[3 * t + 2] = z.e[t];
                        } else {
                            jr[3 * t] = (RK)cf[0] * z.sv1[t];
                            jr[3 * t + 1] = (RK)cf[1] * z.sv1[t];
                            jr[3 * t + 2] = fma((RK)cf[2], z.t1[t], (RK)cf[3] * z.e[t]);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < n; ++t) {
                        if (!((AX >> (t % 3)) & 1)) continue;
                        gl[t] = fma(jr[t], (RK)y, gl[t]);
                        if constexpr (INC && ALIP_F32_FLOOR > 0) ga[INC ? t : 0] = fma(fabs(jr[t]), fabs((RK)y), ga[INC ? t : 0]);
                        pw1[t] = fma(jr[t], wm, pw1[t]);
                        pw2[t] = fma(jr[t], wr, pw2[t]);
                    }
                    kupd<n, AX, RK>(K, jr, sg);
                    // Hessian of -y c
                    if constexpr (KD == VBY) {
                        hp[5] = fma(y, st.c1, hp[5]);
                        hp[6] = fma(y, st.s1, hp[6]);
                        hp[7] = fma(y, c, hp[7]);   // c = vby
                    } else if constexpr (KD == VBX || KD == FEN || KD == FENM) {
                        hp[5] = fma(y, st.s1, hp[5]);
                        hp[6] = fma(-y, st.c1, hp[6]);
                        hp[7] = fma(y, fma(st.c1, st.x1[2], st.s1 * st.x1[3]), hp[7]);
                    } else if constexpr (KD == CIR) {
                        hp[0] = fma(R(-2), y, hp[0]);
                        hp[2] = fma(R(-2), y, hp[2]);
                        h0x = fma(R(-2) * C[LK_GM1], y, h0x);
                    } else if constexpr (KD == FRM) {
                        // -y [[2 qa, qb], [qb, 2 qc]] on the position block of x_{k+1}, (gamma - 1) times it on x_k
                        const R qa_ = ld.qa(j), qb_ = ld.qb(j), qc_ = ld.qc(j), gy = C[LK_GM1] * y;
                        hp[0] = fma(R(-2) * qa_, y, hp[0]);
                        hp[2] = fma(R(-2) * qc_, y, hp[2]);
                        hxy = fma(-qb_, y, hxy);
                        h0x = fma(R(-2) * qa_, gy, h0x);
                        h0y = fma(R(-2) * qc_, gy, h0y);
                        h0xy = fma(-qb_, gy, h0xy);
                    } else if constexpr (KD == LEG) {
                        // -y d2/dp2 |pos_k - f_k|^2 = -2 y u u^T per axis, u = d(px_k - fx_k)/dp
#pragma unroll
                        for (int ja = 0; ja < N; ++ja) {
                            const RK ua = z.sp0[ja] - z.e[ja];
#pragma unroll
                            for (int jb = 0; jb <= ja; ++jb) {
                                const RK h = RK(-2) * (RK)y * ua * (z.sp0[jb] - z.e[jb]);
                                K[3 * ja][3 * jb] += h;
                                K[3 * ja + 1][3 * jb + 1] += h;
                            }
                        }
                    }
                });
                if constexpr (sizeof(R) == 8) lsum += (u == U_INIT || u == U_REST) ? llog(prod) : 0.0;   // one log per step
                // the objective f_{k+1}: gradient and Hessian parts on x_{k+1} (fp64), rebuilt from the heading error
                RK og[3], hv[8];
                {
                    RP px, py;
                    if constexpr (INC) {
                        px = Xs[1][0];
                        py = Xs[1][1];
                    } else {
                        px = pt.X[1][0];
                        py = pt.X[1][1];
                    }
                    R ph = pt.ph[1];
#pragma unroll
                    for (int t = 2; t <= N; ++t) {
                        if constexpr (INC) {
                            px = k + 1 == t ? Xs[t][0] : px;
                            py = k + 1 == t ? Xs[t][1] : py;
                        } else {
                            px = k + 1 == t ? pt.X[t][0] : px;
                            py = k + 1 == t ? pt.X[t][1] : py;
                        }
                        ph = k + 1 == t ? pt.ph[t] : ph;
                    }
                    RK h[6];
                    obj_parts<R>(C, in, k + 1, px, py, ph, og, h, dfo, orgx, orgy);
                    hv[0] = (RK)hp[0] + h[0]; hv[1] = FM ? h[1] + (RK)hxy : h[1]; hv[2] = (RK)hp[2] + h[2]; hv[3] = h[3]; hv[4] = h[4];
                    hv[5] = (RK)hp[5]; hv[6] = (RK)hp[6]; hv[7] = (RK)hp[7] + h[5];
                }
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    gf[3 * j] = fma(og[0], z.sp1[j], gf[3 * j]);
                    gf[3 * j + 1] = fma(og[1], z.sp1[j], gf[3 * j + 1]);
                    gf[3 * j + 2] = fma(og[2], z.t1[j], gf[3 * j + 2]);
                }
                // state Hessian parts -> foothold space: x_{k+1} (sens sp1 / sv1 / t1), x_k (sp0)
#pragma unroll
                for (int ja = 0; ja < N; ++ja) {
                    const RK pa = z.sp1[ja], va = z.sv1[ja], ta = z.t1[ja], qa = z.sp0[ja];
                    const RK hxt = fma(hv[3], pa, hv[5] * va), hyt = fma(hv[4], pa, hv[6] * va);
#pragma unroll
                    for (int jb = 0; jb < N; ++jb) {
                        const RK pb = z.sp1[jb], tb = z.t1[jb], qb = z.sp0[jb];
                        if (jb <= ja) {
                            K[3 * ja][3 * jb] += fma(hv[0] * pa, pb, (RK)h0x * qa * qb);
                            K[3 * ja + 1][3 * jb + 1] += fma(hv[2] * pa, pb, (RK)(FM ? h0y : h0x) * qa * qb);
                            K[3 * ja + 2][3 * jb + 2] += hv[7] * ta * tb;
                        }
                        if constexpr (FM)
                            ksym<n, RK>(K, 3 * ja + 1, 3 * jb, fma(hv[1] * pa, pb, (RK)h0xy * qa * qb));
                        else
                            ksym<n, RK>(K, 3 * ja + 1, 3 * jb, hv[1] * pa * pb);   // (y_ja, x_jb)
                        ksym<n, RK>(K, 3 * ja, 3 * jb + 2, hxt * tb);          // (x_ja, theta_jb)
                        ksym<n, RK>(K, 3 * ja + 1, 3 * jb + 2, hyt * tb);      // (y_ja, theta_jb)
                    }
                }
            }
            // ---- bookkeeping of the pending update
            if (u == U_INIT) {
                thmax = R(1e4) * fmax(R(1), th0);
                thmin = R(1e-4) * fmax(R(1), th0);
                mact = ma;
                nbl = nb;
                mu = C[LK_MU0];
                fcur = (MT)pt.f;
                lcur = lsum;
            } else if (u == U_REST) {
                fcur = (MT)pt.f;
                lcur = lsum;
                nf = 0;
                nrest++;
                if (nrest >= REST_FAIL && violo > R(1e-4)) {
                    status = 2;   // stands in for IPOPT's failed restoration: Infeasible_Problem_Detected
                    done = true;
                }
            }
            upd = U_NONE;
            if (!done && P.goal_abort) {
                // cfg.goal_singular = ABORT: a planned state exactly on the goal makes the reference's gradient NaN
                // (cal_dtar_ang_du, MPC_LIP_modi.py:650-655): IPOPT's Invalid_Number_Detected, this iterate returned
                bool sing = false;
#pragma unroll
                for (int k = 1; k <= N; ++k) {
                    const RP xk = INC ? (RP)Xs[INC ? k : 0][0] : (RP)pt.X[k][0];
                    const RP yk = INC ? (RP)Xs[INC ? k : 0][1] : (RP)pt.X[k][1];
                    // (in map coordinates, as the oracle and the reference take it: the goal frame's origin added)
                    const RP dxg = ((RP)in.gx + (RP)orgx) - (xk + (RP)orgx), dyg = ((RP)in.gy + (RP)orgy) - (yk + (RP)orgy);
                    sing |= fma(dxg, dxg, dyg * dyg) == RP(0);
                }
                if (sing) {
                    status = -13;
                    done = true;
                }
            }
            if (!done) {
                // ---- convergence test (IPOPT scaled overall error)
                RK ru = RK(0);
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    RK r = fabs(gf[i] - gl[i]);
                    // fp32: the multipliers and row coefficients are fp32 values, so no iterate resolves stationarity
                    // below ~eps32 sum |J_r y_r| per column; the test takes the residual beyond that floor
                    // (ALIP_F32_FLOOR x 2^-24 of it; DESIGN.md §2 item 12).  fp64: the plain residual.
                    if constexpr (INC && ALIP_F32_FLOOR > 0) r = fmax(RK(0), r - RK(ALIP_F32_FLOOR) * RK(5.9604644775390625e-08) * ga[INC ? i : 0]);
                    ru = fmax(ru, r);
                }
                const RK sd = fmax(RK(100), (RK)nz / ((RK)mact + RK(n))) / RK(100);
                const RK sc = fmax(RK(100), (RK)nz / fmax(RK(1), (RK)nbl)) / RK(100);
                const RK base_err = fmax(ru / sd, (RK)rcm);
                const bool anyb = wmax >= wmin;   // some active bound
                const RK e0 = fmax(base_err, anyb ? (RK)wmax / sc : RK(0));
#ifdef ALIP_LANE_DBG
                {
                    int im = 0;
                    RK rm = RK(0);
#pragma unroll
                    for (int i = 0; i < n; ++i) {
                        const RK v = fabs(gf[i] - gl[i]);
                        im = v > rm ? i : im;
                        rm = v > rm ? v : rm;
                    }
                    RK rho = RK(1e30);
#pragma unroll
                    for (int k = 1; k <= N; ++k) {
                        const RK dx = (RK)in.gx - (RK)pt.X[k][0], dy = (RK)in.gy - (RK)pt.X[k][1];
                        rho = fmin(rho, sqrt(dx * dx + dy * dy));
                    }
                    dbg[0] = ru; dbg[1] = sd; dbg[2] = rcm; dbg[3] = anyb ? (RK)wmax : RK(0); dbg[4] = sc;
                    dbg[5] = (RK)mu; dbg[6] = rho; dbg[7] = (RK)im;
                    if constexpr (INC) dbg[6] = pick(ga, im);   // (fp32: the floor magnitude of the worst column)
                }
#endif
                if (e0 <= (RK)C[LK_TOL]) {
                    status = 0;
                    done = true;
                } else if (it >= max_iter) {
                    // iteration cap: acceptable / infeasible verdicts on the reference's exact rows
                    if (e0 <= (RK)C[LK_ACC])
                        status = 1;
                    else if (violc > R(1e-4))
                        status = 2;
                    done = true;
                }
                if (!done) {
                    // ---- barrier update (monotone Fiacco-McCormick): max |w - mu| = max(wmax - mu, mu - wmin)
                    const RK mu_min = (RK)C[LK_TOL] / RK(11);   // (IPOPT's floor, as solve_kernel)
                    RK mud = (RK)mu;
                    const RK mu_prev = mud;
                    for (int t = 0; t < 8; ++t) {
                        const R muv = (R)mud;
                        const RK cm = anyb ? (RK)fmax(wmax - muv, muv - wmin) : RK(0);
                        if (fmax(base_err, cm / sc) <= RK(10) * mud && mud > mu_min)
                            mud = fmax(mu_min, fmin(RK(0.2) * mud, mud * sqrt(mud)));
                        else
                            break;
                    }
                    mu = (R)mud;
                    if (mud != mu_prev) nf = 0;
                    const R tau = fmax(R(0.99), R(1) - mu);
                    RK rhs[n];
#pragma unroll
                    for (int i = 0; i < n; ++i) rhs[i] = fma((RK)mu, pw1[i], pw2[i]) - gf[i];
                    // ---- factor K + dw I (Cholesky, L with inverse diagonal in place) with IPOPT's inertia
                    // correction; a register copy of K for the retries
                    RK K0[NKL];
                    {
                        int e = 0;
#pragma unroll
                        for (int i = 0; i < n; ++i)
#pragma unroll
                            for (int j = 0; j <= i; ++j) K0[e++] = K[i][j];
                    }
                    auto chol = [&]() -> bool {
                        bool ok = true;
#pragma unroll
                        for (int j = 0; j < n; ++j) {
                            RK d = K[j][j];
#pragma unroll
                            for (int t = 0; t < j; ++t) d = fma(-K[j][t], K[j][t], d);
                            ok = ok && d > RK(0);
                            const RK inv = rsqrt_nr(d);
                            K[j][j] = inv;
#pragma unroll
                            for (int i = j + 1; i < n; ++i) {
                                RK v = K[i][j];
#pragma unroll
                                for (int t = 0; t < j; ++t) v = fma(-K[i][t], K[j][t], v);
                                K[i][j] = v * inv;
                            }
                        }
                        return ok;
                    };
                    bool fact_ok = true;
                    if (!chol()) {
                        RK dw = dwl == RK(0) ? RK(1e-4) : fmax(RK(1e-20), dwl / RK(3));
                        for (;;) {
                            int e = 0;
#pragma unroll
                            for (int i = 0; i < n; ++i)
#pragma unroll
                                for (int j = 0; j <= i; ++j) {
                                    K[i][j] = K0[e] + (i == j ? dw : RK(0));
                                    ++e;
                                }
                            if (chol()) break;
                            dw *= dwl == RK(0) ? RK(100) : RK(8);
                            if (dw > RK(1e40)) {   // (the system is fp64 in both precisions: the oracle's cap, DESIGN.md §2)
                                fact_ok = false;
                                break;
                            }
                        }
                        dwl = dw;
                    }
                    if (!fact_ok) {
                        // regularisation exhausted: IPOPT's Error_In_Step_Computation, the iterate is returned
                        status = -3;
                        done = true;
                    } else {
                        // L y = rhs, L^T x = y
                        RK xs[n];
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            RK v = rhs[i];
#pragma unroll
                            for (int t = 0; t < i; ++t) v = fma(-K[i][t], xs[t], v);
                            xs[i] = v * K[i][i];
                        }
#pragma unroll
                        for (int i = n - 1; i >= 0; --i) {
                            RK v = xs[i];
#pragma unroll
                            for (int t = i + 1; t < n; ++t) v = fma(-K[t][i], xs[t], v);
                            xs[i] = v * K[i][i];
                        }
                        RK gdv = RK(0);
#pragma unroll
                        for (int i = 0; i < n; ++i) {
                            dU[i] = (R)xs[i];
                            gdv = fma(gf[i], xs[i], gdv);
                        }
                        // ---- slack step, fraction to boundary, merit terms (rows recomputed at the point)
                        R dX[N + 1][5];
                        lin_rollout<N, R>(C, dU, dX);
                        R ap = R(1), azz = R(1), th = R(0), slv = R(0);
                        ld.launder();
                        launder_all(pt.X);
                        launder_all(pt.cs);
                        launder_all(pt.sn);
                        launder_all(pr);
#pragma unroll 1
                        for (int k = 0; k < N; ++k) {
                            const Step<R> st = step_of<N, R>(pt.X, pt.cs, pt.sn, pr, k);
                            const Step<R> dst = step_of<N, R>(dX, pt.cs, pt.sn, dU, k);
                            step_rows<NC, MODI, FM>([&](auto KD_, int l, int j) {
                                constexpr int KD = decltype(KD_)::value;
                                const int i = k * RPS + l;
                                R cf[4], cl, cu;
                                const R c = row_value<KD, R>(C, st, ld, j, cf);
                                row_bounds<KD, R>(C, in.legp, k, cl, cu);
                                const bool act = !is_obs<KD>() || ((in.act >> j) & 1);
                                R jd;
                                if constexpr (is_obs<KD>())
                                    jd = cf[0] * dst.x1[0] + cf[1] * dst.x1[1] + cf[2] * dst.x0[0] + cf[3] * dst.x0[1];
                                else if constexpr (KD == LEG)
                                    jd = cf[0] * dst.x0[0] + cf[1] * dst.x0[1] + cf[2] * dst.fx + cf[3] * dst.fy;
                                else if constexpr (KD == DTH)
                                    jd = dst.ft;
                                else
                                    jd = cf[0] * dst.x1[2] + cf[1] * dst.x1[3] + cf[2] * dst.x1[4] + cf[3] * dst.ft;
                                const R si = ld.s(i);
                                const R rc = act ? c - si : R(0);
                                const R dsv = act ? jd + rc : R(0);
                                ld.ds(i) = dsv;
                                th += fabs(rc);
                                if constexpr (has_lo<KD>()) {
                                    if (act) {
                                        const R zli = ld.zl(zl_index<N, NC, MODI>(k, l));
                                        const R dl = si - cl, idl = rcp_nr(dl);
                                        const R dzl = mu * idl - zli - zli * idl * dsv;
                                        if (dsv < R(0)) ap = fmin(ap, -tau * dl * rcp_nr(dsv));
                                        if (dzl < R(0)) azz = fmin(azz, -tau * zli * rcp_nr(dzl));
                                        slv += dsv * idl;
                                    }
                                }
                                if constexpr (has_up<KD>()) {
                                    if (act) {
                                        const R zui = ld.zu(zu_index<N, NC, MODI>(k, l));
                                        const R du = cu - si, idu = rcp_nr(du);
                                        const R dzu = mu * idu - zui + zui * idu * dsv;
                                        if (dsv > R(0)) ap = fmin(ap, tau * du * rcp_nr(dsv));
                                        if (dzu < R(0)) azz = fmin(azz, -tau * zui * rcp_nr(dzu));
                                        slv -= dsv * idu;
                                    }
                                }
                            });
                        }
                        theta = th;
                        az = azz;
                        phi = fcur - (MT)mu * lcur;
                        gphi = (MT)gdv - (MT)mu * (MT)slv;
                        // switching condition a (-gphi)^s_phi > theta^s_theta in log space
                        lsw = gphi < MT(0) ? sth * llog(theta) - sph * (R)llog(-gphi) : R(0);
                        R am;
                        if (gphi < MT(0)) {
                            am = (R)fmin((double)gth, (double)gph * (double)theta / -gphi);
                            if (theta <= thmin) am = fmin(am, exp(lsw));
                        } else {
                            am = gth;
                        }
                        am *= gal;
                        amin = am > R(0) ? am : R(8.673617379884035e-19);   // (floor where am is 0: DESIGN.md §2 item 8)
                        a = ap;
                        la = llog(ap);
                        phase = 2;
                    }
                }
            }
            if (done) {
                // outputs: u_k = x_{k+1} (the reference's "desired next state"), foot = p_0, x_pred
#pragma unroll
                for (int k = 0; k < N; ++k)
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        double v = INC ? (double)Xs[INC ? k + 1 : 0][c] : (double)pt.X[k + 1][c];
                        if constexpr (GF) v += c == 0 ? orgx : c == 1 ? orgy : 0.0;
                        P.u_out[(size_t)b * 5 * N + 5 * k + c] = v;
                        if (P.x_pred) P.x_pred[(size_t)b * 5 * N + 5 * k + c] = v;
                    }
#ifdef ALIP_LANE_DBG
                if (P.x_pred)
#pragma unroll
                    for (int c = 0; c < 8; ++c) P.x_pred[(size_t)b * 5 * N + c] = dbg[c];
#endif
                if (P.foot_out)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double v = (double)p[c];
                        if constexpr (GF) v += c == 0 ? orgx : c == 1 ? orgy : 0.0;
                        P.foot_out[3 * b + c] = v;
                    }
                if (P.status) P.status[b] = status;
                if (P.iters) P.iters[b] = it;
                phase = 0;
                b = -1;
            }
        }

        // ================= phase 2: one filter line-search trial; restoration when the step is exhausted
        if (phase == 2) {
            const LK<R> C = lk_of<R>(P);
            ld.launder();
            bool accepted = false, ftype = false;
            RP pt_[n];
            R ptr_[n];   // (the trial footholds in the rows' arithmetic)
#pragma unroll
            for (int i = 0; i < n; ++i) {
                pt_[i] = fma((RP)a, (RP)dU[i], p[i]);
                ptr_[i] = (R)pt_[i];
            }
            MT ft = MT(0), lgt = MT(0);
            R dXs[INC ? N + 1 : 1][5];
            if constexpr (INC) lin_rollout<N, R>(C, dU, dXs);
            if (a >= amin) {
                Pt<N, R> pt;
                if constexpr (INC) {
                    RP XPt[N + 1][5];   // the trial's states in the iterate's type
#pragma unroll
                    for (int k = 0; k <= N; ++k)
#pragma unroll
                        for (int c = 0; c < 5; ++c) XPt[k][c] = fma((RP)a, (RP)dXs[k][c], Xs[k][c]);
#pragma unroll
                    for (int k = 0; k <= N; ++k)
#pragma unroll
                        for (int c = 0; c < 5; ++c) pt.X[k][c] = (R)XPt[k][c];
                    eval_states<N, R>(C, in, pt, XPt, dfo, orgx, orgy);
                } else {
                    eval_point<N, R>(C, in, ptr_, pt, dfo);
                }
                ft = (MT)pt.f;
                R tht = R(0);
                bool bad = false;
#pragma unroll 1
                for (int k = 0; k < N; ++k) {
                    const Step<R> st = step_of<N, R>(pt.X, pt.cs, pt.sn, ptr_, k);
                    R prod = R(1);
                    step_rows<NC, MODI, FM>([&](auto KD_, int l, int j) {
                        constexpr int KD = decltype(KD_)::value;
                        const int i = k * RPS + l;
                        R cf[4], cl, cu;
                        const R c = row_value<KD, R>(C, st, ld, j, cf);
                        row_bounds<KD, R>(C, in.legp, k, cl, cu);
                        const bool act = !is_obs<KD>() || ((in.act >> j) & 1);
                        const R sv = fma(a, ld.ds(i), ld.s(i));
                        tht += act ? fabs(c - sv) : R(0);
                        R t = R(1);
                        if constexpr (has_lo<KD>()) {
                            const R d = sv - cl;
                            bad |= act && !(d > R(0));
                            t = act ? d : R(1);
                        }
                        if constexpr (has_up<KD>()) {
                            const R d = cu - sv;
                            bad |= act && !(d > R(0));
                            t = act ? t * d : t;
                        }
                        prod *= t;
                        if constexpr (sizeof(R) == 4) {
                            lgt += (MT)llog(prod);
                            prod = R(1);
                        }
                    });
                    if constexpr (sizeof(R) == 8) lgt += llog(prod);
                }
                const MT pht = bad ? (MT)INFINITY : ft - (MT)mu * lgt;
                bool ok = isfinite(pht) && tht < thmax;
                if (ok) {
                    for (int e = 0; e < FCAP; ++e) {
                        if (__ballot(ok && e < nf) == 0ull) break;
                        if (e < nf && !(tht < ld.fth(e) || pht < ld.fphi(e))) ok = false;
                    }
                }
                if (ok) {
                    const bool switching = gphi < MT(0) && la > lsw;
                    if (switching && theta <= thmin) {
                        if (pht <= phi + (MT)eta * (MT)a * gphi) {
                            accepted = true;
                            ftype = true;
                        }
                    } else if (tht <= (R(1) - gth) * theta || pht <= phi - (MT)gph * (MT)theta) {
                        accepted = true;
                    }
                }
                if (!accepted) {
                    a = a * R(0.5);
                    la = la - R(M_LN2);
                }
            }
            if (accepted) {
                if (!ftype) {
                    // filter entry; entries it dominates are dropped (they reject nothing the new one does not
                    // reject: the same acceptance test with fewer entries)
                    const R fvt = (R(1) - gth) * theta;
                    const MT fvp = phi - (MT)gph * (MT)theta;
                    int w = 0;
                    for (int e = 0; e < FCAP; ++e) {
                        if (__ballot(e < nf) == 0ull) break;
                        if (e < nf) {
                            const R t0 = ld.fth(e);
                            const MT t1 = ld.fphi(e);
                            if (!(t0 >= fvt && t1 >= fvp)) {
                                ld.fth(w) = t0;
                                ld.set_fphi(w, t1);
                                ++w;
                            }
                        }
                    }
                    if (w == FCAP) {   // full (not seen in practice): drop the oldest entry
                        for (int e = 1; e < FCAP; ++e) {
                            ld.fth(e - 1) = ld.fth(e);
                            ld.set_fphi(e - 1, ld.fphi(e));
                        }
                        --w;
                    }
                    ld.fth(w) = fvt;
                    ld.set_fphi(w, fvp);
                    nf = w + 1;
                }
#pragma unroll
                for (int i = 0; i < n; ++i) p[i] = pt_[i];
                if constexpr (INC) {
#pragma unroll
                    for (int k = 0; k <= N; ++k)
#pragma unroll
                        for (int c = 0; c < 5; ++c) Xs[k][c] = fma((RP)a, (RP)dXs[k][c], Xs[k][c]);
                }
                fcur = ft;
                lcur = lgt;
                upd = U_ACC;   // s += a dS and the z step: applied in the next assembly pass
                it++;
                phase = 1;
            } else if (!(a >= amin) && P.redo) {
                // cfg.restoration = IPOPT: the instance goes to the fp64 wave program, which solves it from its start
                // with IPOPT's restoration phase (launch: the hand-off list); this lane writes no outputs for it
                const uint32_t k = atomicAdd(P.redo, 1u);
                P.redo[1 + k] = (uint32_t)b;
                phase = 0;
                b = -1;
            } else if (!(a >= amin)) {   // (a NaN step length ends here too: no endless trials)
                // restoration substitute at the shortest step: applied in the next assembly pass
                a = fmax(a, amin);
#pragma unroll
                for (int i = 0; i < n; ++i) p[i] = fma((RP)a, (RP)dU[i], p[i]);
                if constexpr (INC) {
#pragma unroll
                    for (int k = 0; k <= N; ++k)
#pragma unroll
                        for (int c = 0; c < 5; ++c) Xs[k][c] = fma((RP)a, (RP)dXs[k][c], Xs[k][c]);
                }
                upd = U_REST;
                it++;
                phase = 1;
            }
        }
    }
    // the last wave out resets the launch's queue counters (one wave per workgroup)
    __threadfence();
    if (lane == 0 && atomicAdd(q + 1, 1u) == gridDim.x - 1) {
        atomicExch(q, 0u);
        atomicExch(q + 1, 0u);
    }
}
