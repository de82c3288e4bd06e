// ================================================================================================
// host side: constants, handle, argument staging, C ABI (included by alipmpc.hip into translation unit ALIP_PART=0)
// ================================================================================================
namespace {

using namespace alip;

struct Handle {
    alipmpc_cfg cfg;
    int device = 0;
    int N = 3, n = 9, NG = 32, NCP = 16, NCPU = 16, rps = 0, m_max = 0, mr4 = 0;
    int rps_s = 0, m_s = 0, mr4_s = 0, mo4 = 0;   // solve-kernel row layout (f_en split, objective rows)
    double* dGp = nullptr;
    double* dEp = nullptr;
    double* dGu = nullptr;
    double* dEu = nullptr;
    double* dau = nullptr;   // plan audit (audit.inc): trace matrices and the per-sample cosh / sinh table
    // lane solver (lane_solve.inc): constants and the compiled circle-slot count it runs with (-1: the
    // per-wave solve_kernel serves this configuration)
    double* dlk = nullptr;
    float* dlkf = nullptr;
    int lane_nct = -1;
    // eval hook: the circle-slot count sweep_kernel runs with (-1: eval_kernel serves this configuration)
    int sweep_nc = -1;
    // work-queue counter pairs of persistent solve launches (a ring: launches in flight on different
    // streams use different pairs; each pair is reset by the last wave of the launch that used it), followed by
    // MAXG pairs owned by the closed loop's episode groups (one per group)
    static constexpr unsigned NQ = 64;
    uint32_t* dq = nullptr;
    mutable std::atomic<unsigned> qi{0};
    // staging for host-pointer calls
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // rollout working set (evolving state, warm starts, per-step solve outputs)
    void* rstage = nullptr;
    size_t rstage_bytes = 0;
    hipStream_t own = nullptr;
    // closed loop: episode groups on streams of their own (ALIPMPC_CL_GROUPS), fork / join events
    static constexpr int MAXG = 8;
    hipStream_t gst[MAXG] = {};
    hipEvent_t gev[MAXG + 1] = {};
    // split launch of the wave program (ALIPMPC_SPLIT_IT): the phase-1 iteration cap (0 = off) and, per stream, the
    // record buffer (launches on one stream run in order, so they may share it; other streams get their own)
    int split_it = 0;
    int split_tr = 0;   // phase-1 trial cut: an instance at this many line-search trials resumes as a team (0 = off)
    int cl_split_it = 0, cl_split_tr = 0;   // the closed loop's per-tick solves (ALIPMPC_CL_SPLIT_IT / _TR)
    // the paired phase 2 of the batch API's split (ALIPMPC_SPLIT_PAIR=0 turns it off): fp64 wave program with
    // cfg.restoration = IPOPT, one row group per lane, 8 workspaces within the LDS; only without team records
    bool split_pair = false;
    // the wave program's resident slots, lean and restoration-capable work-queue build, taken on first use
    // (resident_slots; -1: not yet)
    mutable std::atomic<long long> slots_c[2] = {{-1}, {-1}};
    // Record buffers are sized ONCE for the resident slots (the largest batch that splits) and never reallocated or
    // freed before alipmpc_destroy, so a graph captured on a stream keeps a valid pointer whatever batch sizes run on
    // that stream later.  At most SPLIT_STREAMS of them: a further stream runs the one-phase form.
    static constexpr size_t SPLIT_STREAMS = 8;
    struct SplitBuf {
        void* p = nullptr;
        size_t bytes = 0;
    };
    std::map<hipStream_t, SplitBuf> split;
    std::mutex split_mtx;
    // lane program and fp32 wave program with cfg.restoration = IPOPT: per stream, the list of instances handed to the
    // fp64 wave program (count + indices).  A list too small for a batch is RETIRED, not freed: the stream gets a new
    // one of at least twice the bytes and the old one is kept here until alipmpc_destroy, so a graph captured on the
    // stream keeps a valid pointer whatever batch sizes run on that stream later (redo_list)
    std::map<hipStream_t, SplitBuf> redo;
    struct Retired {
        hipStream_t st;
        SplitBuf buf;
    };
    std::vector<Retired> redo_retired;   // newest last
    // launch timing: a ring of event pairs, so a re-record never targets an event still pending on the
    // stream (that serialises the host with the previous launch)
    static constexpr int NEV = 16;
    hipEvent_t ev[NEV][2] = {};
    int evi = 0, evlast = -1;
    bool timed = false;
    std::string err;
};

int fail(Handle* h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    return code;
}

#define HIPCHK(h, x)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) return fail(h, ALIPMPC_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

void mm(const double* a, const double* b, double* c, int n1, int n2, int n3)
{
    for (int i = 0; i < n1; ++i)
        for (int j = 0; j < n3; ++j) {
            double s = 0;
            for (int k = 0; k < n2; ++k) s += a[i * n2 + k] * b[k * n3 + j];
            c[i * n3 + j] = s;
        }
}

// the ALIP step map of one stance phase T = cfg.dt (row-major): x+ = A x + B p, the foothold p = W (u - A x) of the
// reference's u, and x+ = M_A x + M_B u with M_A = (I - B W) A, M_B = B W; beta = sqrt(g / H), ch / sh = cosh / sinh
// (beta T).  Every table and kernel constant derived from these takes them from here.
struct AlipMats {
    double beta, ch, sh;
    double A[25], B[15], W[15], MA[25], MB[25];
};

AlipMats alip_mats(const alipmpc_cfg& cfg)
{
    AlipMats m;
    const double b = m.beta = std::sqrt(cfg.g / cfg.H), T = cfg.dt;
    const double ch = m.ch = std::cosh(b * T), sh = m.sh = std::sinh(b * T);
    const double A[25] = {ch, 0, sh / b, 0, 0, 0, ch, 0, sh / b, 0, sh * b, 0, ch, 0, 0, 0, sh * b, 0, ch, 0, 0, 0, 0, 0, 1};
    const double Bm[15] = {1 - ch, 0, 0, 0, 1 - ch, 0, -sh * b, 0, 0, 0, -sh * b, 0, 0, 0, 1};
    const double Dd = 5.0 * (ch - 1) * (ch - 1) + (sh * b) * (sh * b);
    const double Ch = -5.0 * (ch - 1) / Dd, Sh = -sh * b / Dd;
    const double W[15] = {Ch, 0, Sh, 0, 0, 0, Ch, 0, Sh, 0, 0, 0, 0, 0, 1};
    double BWA[25];
    std::memcpy(m.A, A, sizeof(A));
    std::memcpy(m.B, Bm, sizeof(Bm));
    std::memcpy(m.W, W, sizeof(W));
    mm(m.B, m.W, m.MB, 5, 3, 5);
    mm(m.MB, m.A, BWA, 5, 5, 5);
    for (int i = 0; i < 25; ++i) m.MA[i] = m.A[i] - BWA[i];
    return m;
}

// alip_des_vel(vx, leg_ind) (MPC_LIP_modi.py:181-186): the forward velocity and the size of the lateral one
void alip_des_vel(const AlipMats& m, double T, double vx, double& vdx, double& vdy0)
{
    vdx = m.beta / std::tanh(T * m.beta / 2) * vx * T / 2;   // beta coth(beta T / 2) vx T / 2
    vdy0 = (m.beta * m.sh) / (m.ch + 1);
}

// generator tables.  Row 8k+c (c<5): state x_k[c]; row 8k+5+c (c<3): foothold p_k[c]; V = E x0 + G z.
//  u-parametrisation (the reference's decision, eval + warm start): x_{k+1} = M_A x_k + M_B u_k,
//    p_k = W(u_k - A x_k)                                           (MPC_LIP_modi.py:64-87, 630-634)
//  foothold parametrisation (the solve): x_{k+1} = A x_k + B p_k   (W B = I, so the two describe the same
//    NLP; u enters it only through W u_k, which leaves a 2N-dim null space in u that p removes)
void build_tables(const alipmpc_cfg& cfg, int NCPP, int NCPU, std::vector<double>& Gp, std::vector<double>& Ep,
                  std::vector<double>& Gu, std::vector<double>& Eu)
{
    const int N = cfg.N, n = 5 * N, NG = 8 * (N + 1);
    const AlipMats am = alip_mats(cfg);
    const double *A = am.A, *Bm = am.B, *W = am.W, *MA = am.MA, *MB = am.MB;
    double WA[15];
    mm(W, A, WA, 3, 5, 5);
    // ---- u tables
    std::vector<double> Phi((N + 1) * 5 * n, 0.0), Pk((N + 1) * 25, 0.0);
    for (int i = 0; i < 5; ++i) Pk[i * 5 + i] = 1.0;
    for (int k = 1; k <= N; ++k) {
        mm(MA, &Phi[(k - 1) * 5 * n], &Phi[k * 5 * n], 5, 5, n);
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) Phi[k * 5 * n + i * n + 5 * (k - 1) + j] += MB[i * 5 + j];
        mm(MA, &Pk[(k - 1) * 25], &Pk[k * 25], 5, 5, 5);
    }
    Gu.assign((size_t)NG * NCPU, 0.0);
    Eu.assign((size_t)NG * 5, 0.0);
    for (int k = 0; k <= N; ++k) {
        for (int c = 0; c < 5; ++c) {
            for (int j = 0; j < n; ++j) Gu[(8 * k + c) * NCPU + j] = Phi[k * 5 * n + c * n + j];
            for (int j = 0; j < 5; ++j) Eu[(8 * k + c) * 5 + j] = Pk[k * 25 + c * 5 + j];
        }
        if (k < N) {
            std::vector<double> WAPhi(3 * n), WAPk(15);
            mm(WA, &Phi[k * 5 * n], WAPhi.data(), 3, 5, n);
            mm(WA, &Pk[k * 25], WAPk.data(), 3, 5, 5);
            for (int c = 0; c < 3; ++c) {
                for (int j = 0; j < n; ++j) Gu[(8 * k + 5 + c) * NCPU + j] = -WAPhi[c * n + j];
                for (int j = 0; j < 5; ++j) Gu[(8 * k + 5 + c) * NCPU + 5 * k + j] += W[c * 5 + j];
                for (int j = 0; j < 5; ++j) Eu[(8 * k + 5 + c) * 5 + j] = -WAPk[c * 5 + j];
            }
        }
    }
    // ---- foothold tables: x_k = A^k x0 + sum_{j<k} A^{k-1-j} B p_j
    std::vector<double> Ak((N + 1) * 25, 0.0);
    for (int i = 0; i < 5; ++i) Ak[i * 5 + i] = 1.0;
    for (int k = 1; k <= N; ++k) mm(A, &Ak[(k - 1) * 25], &Ak[k * 25], 5, 5, 5);
    Gp.assign((size_t)NG * NCPP, 0.0);
    Ep.assign((size_t)NG * 5, 0.0);
    for (int k = 0; k <= N; ++k) {
        for (int c = 0; c < 5; ++c) {
            for (int j = 0; j < 5; ++j) Ep[(8 * k + c) * 5 + j] = Ak[k * 25 + c * 5 + j];
            for (int jj = 0; jj < k; ++jj) {
                double AB[15];
                mm(&Ak[(k - 1 - jj) * 25], Bm, AB, 5, 5, 3);
                for (int c2 = 0; c2 < 3; ++c2) Gp[(8 * k + c) * NCPP + 3 * jj + c2] = AB[c * 3 + c2];
            }
        }
        if (k < N)
            for (int c = 0; c < 3; ++c) Gp[(8 * k + 5 + c) * NCPP + 3 * k + c] = 1.0;
    }
}

// plan audit table (audit.inc, AU_TAB_*): the matrices alipmpc_trace_batch passes to trace_kernel and, per trace sample
// t_i = i * 0.01, cosh(beta t_i), sinh(beta t_i) / beta, 1 - cosh(beta t_i)
void audit_table(const alipmpc_cfg& cfg, std::vector<double>& tab)
{
    const int rows = alipmpc_trace_len(&cfg);
    tab.assign((size_t)au_tab_doubles(rows), 0.0);
    const AlipMats am = alip_mats(cfg);
    const double b = am.beta;
    std::memcpy(&tab[AU_TAB_A], am.A, sizeof(am.A));
    std::memcpy(&tab[AU_TAB_W], am.W, sizeof(am.W));
    std::memcpy(&tab[AU_TAB_MB], am.MB, sizeof(am.MB));
    std::memcpy(&tab[AU_TAB_MA], am.MA, sizeof(am.MA));
    for (int i = 0; i + 1 < rows; ++i) {
        const double t = i * 0.01, c = std::cosh(b * t), s = std::sinh(b * t);
        tab[AU_TAB_S + 3 * i] = c;
        tab[AU_TAB_S + 3 * i + 1] = s / b;
        tab[AU_TAB_S + 3 * i + 2] = 1 - c;
    }
}

// lane-solver constants (lane::LK_* slots): the ALIP step map per axis, W, the foothold sensitivities
// d px_k / d fx_j = (Abar^(k-1-j) bbar)[0] and d vx_k / d fx_j = (...)[1], the relaxed (IPOPT
// bound_relax_factor 1e-8, as the oracle) and original bounds, weights and tolerances
void lane_constants(const alipmpc_cfg& cfg, double* lk)
{
    using namespace alip::lane;
    static_assert(LK_COUNT <= LK_BUF, "lane constants fit their buffer");
    for (int i = 0; i < LK_BUF; ++i) lk[i] = 0.0;
    // per axis (position, velocity): A = [[ch, sh / beta], [sh beta, ch]], B = (1 - ch, -sh beta), W = (W[0], W[2])
    const AlipMats am = alip_mats(cfg);
    const double ch = am.ch, shb = am.A[2], bsh = am.A[10], omc = am.B[0], nbsh = am.B[6];
    lk[LK_CH] = ch;
    lk[LK_SHB] = shb;
    lk[LK_BSH] = bsh;
    lk[LK_OMC] = omc;
    lk[LK_WCH] = am.W[0];
    lk[LK_WSH] = am.W[2];
    double v0 = omc, v1 = nbsh;
    for (int m = 0; m < 6; ++m) {
        lk[LK_SP + m] = v0;
        lk[LK_SV + m] = v1;
        const double w0 = ch * v0 + shb * v1, w1 = bsh * v0 + ch * v1;
        v0 = w0;
        v1 = w1;
    }
    auto rl = [](double x) { return x - 1e-8 * std::fmax(1.0, std::fabs(x)); };
    auto ru = [](double x) { return x + 1e-8 * std::fmax(1.0, std::fabs(x)); };
    lk[LK_VXL] = rl(cfg.bvx_lo);
    lk[LK_VXU] = ru(cfg.bvx_hi);
    lk[LK_VYLP] = rl(cfg.bvy_lo);
    lk[LK_VYUP] = ru(cfg.bvy_hi);
    lk[LK_VYLN] = rl(-cfg.bvy_hi);
    lk[LK_VYUN] = ru(-cfg.bvy_lo);
    lk[LK_CIRL] = rl(0.0);
    lk[LK_LEGL] = rl(0.0);
    lk[LK_LEGU] = ru(cfg.leg2_max);
    lk[LK_DTL] = rl(-cfg.dtheta_max);
    lk[LK_DTU] = ru(cfg.dtheta_max);
    lk[LK_OVXL] = cfg.bvx_lo;
    lk[LK_OVXU] = cfg.bvx_hi;
    lk[LK_OVYLP] = cfg.bvy_lo;
    lk[LK_OVYUP] = cfg.bvy_hi;
    lk[LK_OVYLN] = -cfg.bvy_hi;
    lk[LK_OVYUN] = -cfg.bvy_lo;
    lk[LK_OLEGU] = cfg.leg2_max;
    lk[LK_ODT] = cfg.dtheta_max;
    lk[LK_Q] = cfg.q;
    lk[LK_P] = cfg.p;
    lk[LK_R] = cfg.r;
    lk[LK_GM1] = cfg.gamma - 1.0;
    lk[LK_S] = cfg.s;
    lk[LK_TOL] = cfg.tol;
    lk[LK_ACC] = cfg.acceptable_tol;
    lk[LK_MU0] = cfg.mu_init;
    lk[LK_DET2] = cfg.detect_r2;
    // d px_{k+1+m} / d u_k[px], [vx] of the reference's u (per axis: (MA^m MB)[0][0], [0][1], MA = (I - B W) A, MB = B W),
    // for IPOPT's objective scaling at the starting point (lane_solve.inc)
    {
        const double Ax[2][2] = {{ch, shb}, {bsh, ch}}, Bx[2] = {omc, nbsh};
        const double Wx[2] = {lk[LK_WCH], lk[LK_WSH]};
        double MA[2][2], MB[2][2], Mm[2][2] = {{1, 0}, {0, 1}};   // Mm = MA^m
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                MB[i][j] = Bx[i] * Wx[j];
                MA[i][j] = Ax[i][j] - Bx[i] * (Wx[0] * Ax[0][j] + Wx[1] * Ax[1][j]);
            }
        for (int m = 0; m < 6; ++m) {
            lk[LK_SU0 + m] = Mm[0][0] * MB[0][0] + Mm[0][1] * MB[1][0];
            lk[LK_SU1 + m] = Mm[0][0] * MB[0][1] + Mm[0][1] * MB[1][1];
            double T[2][2];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) T[i][j] = Mm[i][0] * MA[0][j] + Mm[i][1] * MA[1][j];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) Mm[i][j] = T[i][j];
        }
    }
}

// the compiled lane-solver instance serving cfg, or -1 when none does: N = 3 with circles only (<= 6 circle slots),
// modi / sig_step (BASELINE cfg1/2/4/5 shapes); with ellipses (ne_max >= 1) modi's form build, nc_max + ne_max <= 5
// (LANE_FORM5: its 157 LDS entries per lane keep four waves on a CU, a sixth slot would not — lane_solve.inc)
int lane_slots_for(const alipmpc_cfg& c)
{
    if (c.variant == ALIPMPC_VARIANT_DD || c.N != 3) return -1;
    if (c.ne_max != 0)
        return c.variant == ALIPMPC_VARIANT_MODI && c.ne_max >= 1 && c.nc_max + c.ne_max <= 5 ? LANE_FORM5 : -1;
    if (c.nc_max > 6) return -1;
    return c.nc_max == 0 ? 0 : c.nc_max <= 5 ? 5 : 6;
}

size_t smem_bytes(const Handle* h, bool solve, int force_f64 = 0)
{
    const alipmpc_cfg& c = h->cfg;
    if (c.variant == ALIPMPC_VARIANT_DD) {
        const int wsd = with_n(h->N, 0, [&](auto n) { return ddw_doubles<decltype(n)::value>(c.nc_max + c.ne_max, h->mo4); });
        return sizeof(double) * ((size_t)KP_DOUBLES + (size_t)WAVES_PER_BLOCK * wsd);
    }
    const bool f32 = solve && c.precision == ALIPMPC_PREC_FP32 && !force_f64;
    const int wsd = with_n(h->N, 0, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        return solve ? (f32 ? wss_elems<NN, float>(c.nc_max, c.ne_max, h->mr4_s, h->mo4)
                            : wss_elems<NN, double>(c.nc_max, c.ne_max, h->mr4_s, h->mo4))
                     : gws_doubles<NN>(c.nc_max, c.ne_max, h->mr4);
    });
    const int e = solve ? 0 : h->NG * 5 + ((h->NG * 5) & 1);   // (solve_kernel: E from global memory)
    const int ncp = solve ? h->NCP : h->NCPU;
    // KP in fp64 units, then G, E and the per-wave workspaces in the kernel's arithmetic type
    const size_t per_block = solve ? (size_t)WAVES_PER_BLOCK : (size_t)GROUPS_PER_BLOCK;   // workspaces
    return sizeof(double) * (size_t)KP_DOUBLES +
           (f32 ? sizeof(float) : sizeof(double)) * ((size_t)h->NG * ncp + e + per_block * wsd);
}

KP make_kp(const Handle* h, long long B, bool solve)
{
    const alipmpc_cfg& c = h->cfg;
    KP P;
    std::memset(&P, 0, sizeof(P));
    P.nc_max = c.nc_max;
    P.ne_max = c.ne_max;
    P.rps = solve ? h->rps_s : h->rps;
    P.m_max = solve ? h->m_s : h->m_max;
    P.mr4 = solve ? h->mr4_s : h->mr4;
    P.mo4 = h->mo4;
    P.modi = c.variant == ALIPMPC_VARIANT_MODI;
    P.max_iter = c.max_iter;
    P.select_obs = c.select_obs;
    P.detour = c.detour;
    P.goal_abort = c.goal_singular == ALIPMPC_GOAL_SINGULAR_ABORT;
    P.resto_ipopt = c.restoration == ALIPMPC_RESTORATION_IPOPT && c.variant != ALIPMPC_VARIANT_DD;
    P.tol = c.tol;
    P.acc_tol = c.acceptable_tol;
    P.q = c.q;
    P.p = c.p;
    P.r = c.r;
    P.gm1 = c.gamma - 1.0;
    P.s = c.s;
    P.detect_r2 = c.detect_r2;
    P.leg2 = c.leg2_max;
    P.bvx_lo = c.bvx_lo;
    P.bvx_hi = c.bvx_hi;
    P.bvy_lo = c.bvy_lo;
    P.bvy_hi = c.bvy_hi;
    P.dth = c.dtheta_max;
    P.mu_init = c.mu_init;
    P.dt = c.dt;
    P.dd_t = c.dd_t;
    P.G = solve ? h->dGp : h->dGu;
    P.E = solve ? h->dEp : h->dEu;
    P.Gu = h->dGu;
    P.Eu = h->dEu;
    P.B = B;
    P.lkd = h->dlk;
    P.lkfd = h->dlkf;
    if (solve && c.variant != ALIPMPC_VARIANT_DD) P.queue = h->dq + 2 * (h->qi.fetch_add(1u) % Handle::NQ);
    return P;
}

// cfg.restoration = IPOPT, fp32 programs and the lane program: the stream's hand-off list ([0] = count, then the
// instances), allocated outside a capture (a capture needs an uncaptured solve of at least its B on the stream first).
// A list too small for B is retired to Handle::redo_retired, where it stays allocated until alipmpc_destroy: launches
// already queued and graphs already captured go on using it, so growth neither frees nor synchronises.  The new list
// holds max(need, twice the old bytes): the retired lists of a stream sum to less than its live one.
static hipError_t redo_list(const Handle* h, hipStream_t st, long long B, uint32_t** out)
{
    Handle* hm = const_cast<Handle*>(h);
    std::lock_guard<std::mutex> lk(hm->split_mtx);
    Handle::SplitBuf& rb = hm->redo[st];
    const size_t need = sizeof(uint32_t) * (size_t)(B + 1);
    if (rb.bytes < need) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return hipErrorNotSupported;
        Handle::SplitBuf nb;
        nb.bytes = std::max(need, 2 * rb.bytes);
        if (hipError_t e = hipMalloc(&nb.p, nb.bytes)) return e;
        if (rb.p) hm->redo_retired.push_back({st, rb});
        rb = nb;
    }
    *out = (uint32_t*)rb.p;
    return hipSuccess;
}

// the eval hook's launch: DD's kernel, the sweep kernel where the handle has one, or the grid-stride eval kernel
hipError_t launch_eval_hook(const Handle* h, const KP& P, hipStream_t st)
{
    const size_t smem = smem_bytes(h, false);
    if (h->cfg.variant == ALIPMPC_VARIANT_DD)
        return with_n(h->N, hipErrorInvalidValue, [&](auto n) { return launch_dd<decltype(n)::value>(false, P, smem, st); });
    if (h->sweep_nc >= 0) return launch_sweep(h->sweep_nc, h->cfg.variant == ALIPMPC_VARIANT_MODI, P, st);
    return with_n(h->N, hipErrorInvalidValue, [&](auto n) { return launch_eval<decltype(n)::value>(P, smem, st); });
}

// the program a solve of the handle runs (solve_plan.inc)
SpProgram program_of(const Handle* h)
{
    return h->cfg.variant == ALIPMPC_VARIANT_DD ? SP_PROG_DD : h->lane_nct >= 0 ? SP_PROG_LANE
         : h->cfg.precision == ALIPMPC_PREC_FP32 ? SP_PROG_WAVE_F32 : SP_PROG_WAVE_F64;
}

// instances resident at once on the handle's work-queue solve kernel (alipmpc_solve_slots; 0 for DD: no queue); resto:
// on the wave program's restoration-capable build
long long resident_slots(const Handle* h, bool resto = false)
{
    const bool f32 = h->cfg.precision == ALIPMPC_PREC_FP32, modi = h->cfg.variant == ALIPMPC_VARIANT_MODI;
    switch (program_of(h)) {
    case SP_PROG_DD: return 0;
    case SP_PROG_LANE:
        return f32 ? (long long)lane_resident<float>(h->lane_nct, modi) * lane::lanes_of<float>()
                   : (long long)lane_resident<double>(h->lane_nct, modi) * lane::lanes_of<double>();
    default: break;
    }
    long long s = h->slots_c[resto].load(std::memory_order_relaxed);
    if (s < 0) {
        const size_t smem = smem_bytes(h, true);
        s = (long long)WAVES_PER_BLOCK *
            with_n(h->N, 0u, [&](auto n) { return wave_resident<decltype(n)::value>(f32, resto, h->mo4, smem); });
        h->slots_c[resto].store(s, std::memory_order_relaxed);
    }
    return s;
}

// hip_stream argument -> the stream to launch on (NULL = host-pointer mode on the handle's own stream,
// ALIPMPC_STREAM_NULL = device pointers on the null stream)
hipStream_t stream_of(const Handle* h, void* hip_stream)
{
    if (!hip_stream) return h->own;
    if (hip_stream == ALIPMPC_STREAM_NULL) return nullptr;
    return (hipStream_t)hip_stream;
}

bool create_events(Handle* h)
{
    for (auto& pr : h->ev)
        for (hipEvent_t& e : pr)
            if (hipEventCreate(&e) != hipSuccess) return false;
    return true;
}

// a span of launches timed on the handle's event ring (alipmpc_last_kernel_ms reports the last span ended)
struct TimedSpan {
    Handle* h;
    hipStream_t st;
    int ei = 0;
    int begin()
    {
        ei = h->evi;
        h->evi = (ei + 1) % Handle::NEV;
        HIPCHK(h, hipEventRecord(h->ev[ei][0], st));
        return ALIPMPC_OK;
    }
    int end()
    {
        HIPCHK(h, hipEventRecord(h->ev[ei][1], st));
        h->evlast = ei;
        h->timed = true;
        return ALIPMPC_OK;
    }
};

// grow-only device buffer (Handle::stage, Handle::rstage); what: the allocation as a failure names it; *err: hipMalloc's
// error, for a caller with a message of its own
int ensure(Handle* h, void*& buf, size_t& have, size_t bytes, const char* what, hipError_t* err = nullptr)
{
    if (have >= bytes) return ALIPMPC_OK;
    if (buf) hipFree(buf);
    buf = nullptr;
    have = 0;
    const hipError_t e = hipMalloc(&buf, bytes);
    if (err) *err = e;
    if (e != hipSuccess) return fail(h, ALIPMPC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    have = bytes;
    return ALIPMPC_OK;
}

// One call's view of its array arguments.  An entry point registers every array with the member of its kernel-parameter
// struct (or a local pointer) that is to address it on the device, then calls commit(), launches, and calls finish().
//  device-pointer mode (hip_stream given): in / out / inout slots get the caller's pointer at once; nothing is allocated,
//    copied or synchronised for them.
//  host-pointer mode (hip_stream NULL): every non-null slot gets a 256-byte-aligned area of the buffer; commit() sizes the
//    buffer from the registered slots, grows it, assigns the areas and queues the uploads; finish() queues the downloads
//    and synchronises the stream.  A null array registers a null slot; a zero count copies nothing.
//  work slots (a loop's working set) get an area in both modes.
// The slots live in a fixed array on the stack: no host allocation in either mode.
struct Staging {
    Handle* h;
    hipStream_t st;
    bool host;
    void*& buf;
    size_t& have;
    const char* what;
    static constexpr int MAX_SLOTS = 48;   // (the closed loop with dataset rows registers 39)
    struct Slot {
        void* slot;        // the pointer variable to set
        const void* up;    // host source, uploaded by commit()
        void* down;        // host destination, downloaded by finish()
        size_t bytes;
        void* dev;
    } slots[MAX_SLOTS];
    int n = 0;
    bool overflow = false;
    size_t need = 0;                     // bytes of the buffer this call asked for
    hipError_t alloc_err = hipSuccess;   // != hipSuccess: commit() failed growing the buffer

    // loop = false: the staging buffer of the batch calls; true: the working-set buffer of rollout and closed loop
    Staging(Handle* h_, void* hip_stream, bool loop = false)
        : h(h_), st(stream_of(h_, hip_stream)), host(hip_stream == nullptr), buf(loop ? h_->rstage : h_->stage),
          have(loop ? h_->rstage_bytes : h_->stage_bytes),
          what(loop ? "hipMalloc(&h->rstage, need)" : "hipMalloc(&h->stage, bytes)")
    {
    }

    template <class T>
    void add(T& slot, const void* up, void* down, size_t bytes)
    {
        static_assert(std::is_pointer<T>::value, "a slot is a pointer variable");
        slot = nullptr;
        if (n == MAX_SLOTS) {
            overflow = true;
            return;
        }
        slots[n++] = Slot{&slot, up, down, bytes, nullptr};
    }
    // the caller's pointer as the slot's type: elements of the same size (audit's summary: int64_t as unsigned long
    // long), and no const input behind a slot the kernel may write through
    template <class T, class U>
    static T as_slot(U* p)
    {
        static_assert(std::is_pointer<T>::value && sizeof(std::remove_pointer_t<T>) == sizeof(U),
                      "slot and array have elements of one size");
        return reinterpret_cast<T>(p);
    }
    template <class T, class U>
    void in(T& slot, const U* p, size_t count)
    {
        slot = as_slot<T>(p);
        if (host && p) add(slot, p, nullptr, count * sizeof(U));
    }
    template <class T, class U>
    void out(T& slot, U* p, size_t count)
    {
        slot = as_slot<T>(p);
        if (host && p) add(slot, nullptr, p, count * sizeof(U));
    }
    template <class T, class U>
    void inout(T& slot, U* p, size_t count)
    {
        slot = as_slot<T>(p);
        if (host && p) add(slot, p, p, count * sizeof(U));
    }
    // an output the caller downloads itself (get) once it knows how much of it exists
    template <class T, class U>
    void out_area(T& slot, U* p, size_t count)
    {
        slot = as_slot<T>(p);
        if (host && p) add(slot, nullptr, nullptr, count * sizeof(U));
    }
    template <class T>
    void work(T*& slot, size_t count)
    {
        add(slot, nullptr, nullptr, count * sizeof(T));
    }

    int commit()
    {
        if (overflow) return fail(h, ALIPMPC_EINVAL, "staging: more array arguments than slots");
        if (n == 0) return ALIPMPC_OK;
        auto aligned = [](size_t off) { return (off + 255) & ~(size_t)255; };
        size_t off = 0;
        for (int i = 0; i < n; ++i) off = aligned(off) + slots[i].bytes;
        need = off + 256;
        if (int e = ensure(h, buf, have, need, what, &alloc_err)) return e;
        off = 0;
        for (int i = 0; i < n; ++i) {
            Slot& s = slots[i];
            off = aligned(off);
            s.dev = (char*)buf + off;
            std::memcpy(s.slot, &s.dev, sizeof(void*));
            off += s.bytes;
            if (s.up && s.bytes) HIPCHK(h, hipMemcpyAsync(s.dev, s.up, s.bytes, hipMemcpyHostToDevice, st));
        }
        return ALIPMPC_OK;
    }
    // a working-set area's initial contents: from the caller's array, host or device by mode
    int put(void* dev, const void* src, size_t bytes)
    {
        HIPCHK(h, hipMemcpyAsync(dev, src, bytes, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
        return ALIPMPC_OK;
    }
    int get(void* dst, const void* dev, size_t bytes)
    {
        HIPCHK(h, hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, st));
        return ALIPMPC_OK;
    }
    int finish()
    {
        if (!host) return ALIPMPC_OK;
        for (int i = 0; i < n; ++i)
            if (slots[i].down && slots[i].bytes)
                if (int e = get(slots[i].down, slots[i].dev, slots[i].bytes)) return e;
        HIPCHK(h, hipStreamSynchronize(st));
        return ALIPMPC_OK;
    }
};

// the scene arguments shared by solve / eval, rollout, closed loop and audit (x0, leg, u: null where the entry point keeps
// a working copy of its own or has none)
struct SceneIn {
    const double *x0, *goal;
    const int8_t* leg;
    const double* cir;
    const int32_t* nc;
    const double* elp;
    const int32_t* ne;
    const double* u;
};

// leg: every variant but DD; u: where the entry point reads one (need_u); obstacle arrays: where the handle has slots
bool scene_inputs_ok(const alipmpc_cfg& cf, const SceneIn& s, bool need_u)
{
    const bool dd = cf.variant == ALIPMPC_VARIANT_DD;
    return s.x0 && s.goal && (s.leg || dd) && s.nc && (s.u || !need_u) && (cf.nc_max == 0 || s.cir) &&
           (cf.ne_max == 0 || (s.elp && s.ne));
}

// registers the scene with P.  Without ellipse slots (ne_max == 0) the kernels get elp = ne = nullptr in both pointer
// modes: every reader guards on ne_max (prologue, eval_group_one, dd_prologue, lane_solve.inc, audit.inc).
void stage_scene(Staging& S, KP& P, const Handle* h, const SceneIn& s, size_t Bz)
{
    const alipmpc_cfg& cf = h->cfg;
    const bool dd = cf.variant == ALIPMPC_VARIANT_DD;
    S.in(P.x0, s.x0, Bz * (dd ? 3 : 5));
    S.in(P.goal, s.goal, Bz * 2);
    S.in(P.leg, s.leg, Bz);
    S.in(P.cir, s.cir, Bz * 3 * cf.nc_max);
    S.in(P.nc, s.nc, Bz);
    S.in(P.elp, cf.ne_max ? s.elp : nullptr, Bz * 5 * cf.ne_max);
    S.in(P.ne, cf.ne_max ? s.ne : nullptr, Bz);
    S.in(P.u0, s.u, Bz * (size_t)alipmpc_num_vars(&cf));
}

}  // namespace

extern "C" {

int alipmpc_default_cfg(int32_t variant, int32_t N, alipmpc_cfg* c)
{
    if (!c) return ALIPMPC_EINVAL;
    std::memset(c, 0, sizeof(*c));
    c->N = N;
    c->nc_max = 6;
    c->ne_max = 6;
    c->variant = variant;
    // the reference's IPOPT caps: MPC_LIP_modi.py:287 (30), MPC_LIP_sig_step.py:269 (20), MPC_DD_sig_step.py:183 (40)
    c->max_iter = variant == ALIPMPC_VARIANT_SIG_STEP ? 20 : variant == ALIPMPC_VARIANT_DD ? 40 : 30;
    c->precision = ALIPMPC_PREC_FP64;
    c->select_obs = 1;
    c->detour = 1;
    c->tol = 1e-8;
    c->acceptable_tol = 1e-6;
    c->dt = 0.4;
    c->H = 1.0;
    c->g = 9.81;
    c->leg2_max = 0.09;
    c->bvx_lo = 0.4;
    c->bvx_hi = 0.8;
    c->bvy_lo = 0.15;
    c->bvy_hi = 0.35;
    c->dtheta_max = M_PI / 16;
    c->q = 1.0;
    c->p = 0.0;
    c->r = 50.0;
    c->gamma = 0.2;
    c->s = 0.024 * 180 / M_PI;
    c->detect_r2 = 16.0;
    c->dd_t = 2.0;
    c->mu_init = 0.1;
    if (variant == ALIPMPC_VARIANT_SIG_STEP) {   // MPC_LIP_sig_step.py:38,340-353
        c->bvy_hi = 0.30;
        c->p = 2.0;
        c->r = 15.0;
        c->gamma = 0.4;
        c->s = 0.014 * 180 / M_PI;
        c->select_obs = 0;
    } else if (variant == ALIPMPC_VARIANT_DD) {  // MPC_DD_sig_step.py:33-37,323-338
        c->select_obs = 0;
        c->detour = 0;
    } else if (variant != ALIPMPC_VARIANT_MODI) {
        return ALIPMPC_EINVAL;
    }
    return ALIPMPC_OK;
}

int32_t alipmpc_rows_per_step(const alipmpc_cfg* c)
{
    if (!c) return 0;
    if (c->variant == ALIPMPC_VARIANT_DD) return c->nc_max + c->ne_max + 1;
    return 4 + c->nc_max + c->ne_max + (c->variant == ALIPMPC_VARIANT_MODI ? 1 : 0);
}

int32_t alipmpc_num_vars(const alipmpc_cfg* c)
{
    if (!c) return 0;
    return c->variant == ALIPMPC_VARIANT_DD ? 2 * c->N : 5 * c->N;
}

int alipmpc_create(const alipmpc_cfg* cfg, int device, void** handle)
{
    if (!cfg || !handle) return ALIPMPC_EINVAL;
    *handle = nullptr;
    if (cfg->N < 1 || cfg->N > ALIPMPC_MAX_N || cfg->nc_max < 0 || cfg->ne_max < 0 ||
        cfg->nc_max + cfg->ne_max > ALIPMPC_MAX_OBS || cfg->max_iter < 0 || cfg->max_iter > FILTER_CAP - 2)
        return ALIPMPC_EINVAL;
    if (cfg->precision != ALIPMPC_PREC_FP64 && cfg->precision != ALIPMPC_PREC_FP32) return ALIPMPC_EINVAL;
    if (cfg->program != ALIPMPC_PROGRAM_WAVE && cfg->program != ALIPMPC_PROGRAM_LANE) return ALIPMPC_EINVAL;
    // enum fields: callers start from alipmpc_default_cfg (a struct filled by hand must set them to a defined value)
    if (cfg->goal_singular != ALIPMPC_GOAL_SINGULAR_ZERO && cfg->goal_singular != ALIPMPC_GOAL_SINGULAR_ABORT)
        return ALIPMPC_EINVAL;
    if (cfg->restoration != ALIPMPC_RESTORATION_IPOPT && cfg->restoration != ALIPMPC_RESTORATION_SUBSTITUTE)
        return ALIPMPC_EINVAL;
    // fp32 arithmetic is implemented for the LIP solve kernels (modi, sig_step)
    if (cfg->precision == ALIPMPC_PREC_FP32 && cfg->variant == ALIPMPC_VARIANT_DD) return ALIPMPC_EUNSUPPORTED;
    if (cfg->variant != ALIPMPC_VARIANT_MODI && cfg->variant != ALIPMPC_VARIANT_SIG_STEP &&
        cfg->variant != ALIPMPC_VARIANT_DD)
        return ALIPMPC_EINVAL;
    if (cfg->cl_between != ALIPMPC_CL_BETWEEN_NOMINAL && cfg->cl_between != ALIPMPC_CL_BETWEEN_FIRST_ORDER &&
        cfg->cl_between != ALIPMPC_CL_BETWEEN_GUARDED)
        return ALIPMPC_EINVAL;
    // first-order ticks (guarded or not) read the sensitivity build's du: alipmpc_solve_sens_batch's domain
    if (cfg->cl_between != ALIPMPC_CL_BETWEEN_NOMINAL &&
        (cfg->variant == ALIPMPC_VARIANT_DD || cfg->precision == ALIPMPC_PREC_FP32 ||
         cfg->program == ALIPMPC_PROGRAM_LANE || cfg->N > 5))
        return ALIPMPC_EUNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ALIPMPC_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ALIPMPC_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ALIPMPC_ENODEV;
    Handle* h = new Handle();
    h->cfg = *cfg;
    if (cfg->precision == ALIPMPC_PREC_FP32 && cfg->tol == 1e-8 && cfg->acceptable_tol == 1e-6) {
        // the fp64 defaults are below fp32 resolution: use the horizon-aware fp32 defaults (the ctypes
        // layer's FP32_TOL*); N > 3 decision-space gradients grow through A^k and lift the fp32 floor
        h->cfg.tol = cfg->N > 3 ? 3e-4 : 1e-4;
        h->cfg.acceptable_tol = cfg->N > 3 ? 3e-3 : 1e-3;
    }
    h->device = device;
    h->N = cfg->N;
    h->n = 3 * cfg->N;
    h->NG = 8 * (cfg->N + 1);
    h->NCP = 16 * ((h->n + 15) / 16);
    h->NCPU = 16 * ((5 * cfg->N + 15) / 16);
    h->rps = alipmpc_rows_per_step(cfg);
    h->m_max = cfg->N * h->rps;
    h->mr4 = (h->m_max + 3) & ~3;
    if (cfg->variant == ALIPMPC_VARIANT_DD) {
        // DD solve rows per step: cbf slots, v +- s w, v bound, w bound; + N objective rows; whole
        // 64-lane row groups (dd_solve_kernel<N, RPL>)
        h->rps_s = cfg->nc_max + cfg->ne_max + 4;
        h->m_s = cfg->N * h->rps_s;
        h->mr4_s = (h->m_s + 3) & ~3;
        const int rpl = (h->mr4_s + cfg->N + WAVE - 1) / WAVE;
        h->mo4 = rpl <= 3 ? WAVE * rpl : 1 << 20;
    } else {
        h->rps_s = h->rps + (cfg->variant == ALIPMPC_VARIANT_MODI ? 1 : 0);   // f_en -> two smooth rows
        h->m_s = cfg->N * h->rps_s;
        h->mr4_s = (h->m_s + 3) & ~3;
        // + the objective pseudo-rows of the solve kernel, rounded up to the compiled J-layout size (4 KSM)
        h->mo4 = 4 * ksm_of(h->mr4_s + 4 * ((cfg->N + 3) / 4));
    }
    if (h->mr4 > MAX_ROWS || h->mo4 > MAX_ROWS + 64) {
        delete h;
        return ALIPMPC_EINVAL;
    }
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return ALIPMPC_ENODEV;
    }
    std::vector<double> Gp, Ep, Gu, Eu;
    build_tables(*cfg, h->NCP, h->NCPU, Gp, Ep, Gu, Eu);
    auto up = [](double** d, const std::vector<double>& v) {
        return hipMalloc(d, v.size() * sizeof(double)) == hipSuccess &&
               hipMemcpy(*d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&h->dGp, Gp) || !up(&h->dEp, Ep) || !up(&h->dGu, Gu) || !up(&h->dEu, Eu) ||
        hipMalloc(&h->dq, 2 * (Handle::NQ + Handle::MAXG) * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&h->dlk, alip::lane::LK_BUF * sizeof(double)) != hipSuccess ||
        hipMalloc(&h->dlkf, alip::lane::LK_BUF * sizeof(float)) != hipSuccess ||
        hipMemset(h->dq, 0, 2 * (Handle::NQ + Handle::MAXG) * sizeof(uint32_t)) != hipSuccess ||
        hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess ||
        !create_events(h)) {
        alipmpc_destroy(h);
        return ALIPMPC_EHIP;
    }
    if (cfg->variant != ALIPMPC_VARIANT_DD && alipmpc_trace_len(cfg) > 1) {
        std::vector<double> au;
        audit_table(h->cfg, au);
        if (!up(&h->dau, au)) {
            alipmpc_destroy(h);
            return ALIPMPC_EHIP;
        }
    }
    {
        double lk[alip::lane::LK_BUF];
        float lkf[alip::lane::LK_BUF];
        lane_constants(h->cfg, lk);
        for (int i = 0; i < alip::lane::LK_BUF; ++i) lkf[i] = (float)lk[i];
        if (hipMemcpy(h->dlk, lk, sizeof(lk), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->dlkf, lkf, sizeof(lkf), hipMemcpyHostToDevice) != hipSuccess) {
            alipmpc_destroy(h);
            return ALIPMPC_EHIP;
        }
        // the eval hook's sweep kernel: N = 3, circle slots only (ALIPMPC_EVAL_KERNEL=group selects eval_kernel,
        // for A/B and the bit-identity test)
        const char* ek = std::getenv("ALIPMPC_EVAL_KERNEL");
        if (h->cfg.variant != ALIPMPC_VARIANT_DD && h->cfg.N == 3 && h->cfg.ne_max == 0 && h->cfg.nc_max <= 6 &&
            !(ek && std::strcmp(ek, "group") == 0))
            h->sweep_nc = h->cfg.nc_max;
        {   // split launch of one-wave-per-instance batches (ALIPMPC_SPLIT_IT=0 turns it off)
            const char* se = std::getenv("ALIPMPC_SPLIT_IT");
            h->split_it = se ? std::atoi(se)
                             : (cfg->restoration == ALIPMPC_RESTORATION_IPOPT ? SPLIT_IT_DEFAULT_RESTO : SPLIT_IT_DEFAULT);
            if (h->split_it < 0 || h->split_it >= h->cfg.max_iter) h->split_it = 0;
            auto env_int = [](const char* name, int dflt) {
                const char* t = std::getenv(name);
                return t ? std::max(0, std::atoi(t)) : dflt;
            };
            h->split_tr = env_int("ALIPMPC_SPLIT_TR", SPLIT_TR_DEFAULT);
            h->cl_split_it = env_int("ALIPMPC_CL_SPLIT_IT", CL_SPLIT_IT_DEFAULT);
            if (h->cl_split_it >= h->cfg.max_iter) h->cl_split_it = 0;
            h->cl_split_tr = env_int("ALIPMPC_CL_SPLIT_TR", CL_SPLIT_TR_DEFAULT);
        }
        if (h->cfg.program == ALIPMPC_PROGRAM_LANE) {
            h->lane_nct = lane_slots_for(h->cfg);
            if (h->lane_nct < 0) {
                alipmpc_destroy(h);
                return ALIPMPC_EUNSUPPORTED;
            }
        }
    }
    // (fp32 with cfg.restoration = IPOPT hands instances to the fp64 wave program: its workspace must fit as well)
    const bool handoff = cfg->variant != ALIPMPC_VARIANT_DD && cfg->restoration == ALIPMPC_RESTORATION_IPOPT &&
                         (cfg->precision == ALIPMPC_PREC_FP32 || h->lane_nct >= 0);
    if (smem_bytes(h, true) > 160 * 1024 || smem_bytes(h, false) > 160 * 1024 ||
        (handoff && smem_bytes(h, true, 1) > 160 * 1024)) {
        alipmpc_destroy(h);
        return ALIPMPC_EUNSUPPORTED;
    }
    // team records need the team-capable build's TEAM_WAVES workspaces in one workgroup: without room, no trial cut
    if (cfg->variant != ALIPMPC_VARIANT_DD && cfg->precision != ALIPMPC_PREC_FP32 && h->lane_nct < 0) {
        const size_t sm = smem_bytes(h, true);
        const size_t st_ = with_n(h->N, (size_t)0, [&](auto n) { return team_smem<decltype(n)::value, double>(sm); });
        if (st_ > 160 * 1024) h->split_tr = h->cl_split_tr = 0;
        // the paired phase 2 (solve_kernel<..., PR>): where its 8 workspaces fit; it has a cut of its own
        const size_t sp_ = with_n(h->N, (size_t)0, [&](auto n) { return pair_smem<decltype(n)::value>(sm); });
        const char* pe = std::getenv("ALIPMPC_SPLIT_PAIR");
        h->split_pair = !(pe && std::atoi(pe) == 0) && cfg->restoration == ALIPMPC_RESTORATION_IPOPT &&
                        pair_ksm(h->mo4 / 4) && sp_ <= 160 * 1024;
        if (h->split_pair && !std::getenv("ALIPMPC_SPLIT_IT") && SPLIT_IT_DEFAULT_RESTO_PAIR < h->cfg.max_iter)
            h->split_it = SPLIT_IT_DEFAULT_RESTO_PAIR;
    }
    *handle = h;
    return ALIPMPC_OK;
}

// A wave-program solve whose batch fits the resident slots (one wave per instance) runs as a SPLIT launch: phase 1
// solves every instance for up to split_it iterations; an instance still running then writes its loop state to a
// record and stops; phase 2 resumes those instances, one wave each.  The long instances (cfg2: 12 % run to the
// 30-iteration cap, DESIGN.md) otherwise finish at the pace of the busiest SIMDs, which hold two or three of them
// among their four waves; in phase 2 they are few enough for a SIMD each.  Every instance executes the same
// arithmetic either way (the record holds its exact loop state): same bits (test_split_launch_bit_identical).
// the stream's record buffer (Handle::split), sized for `slots` instances; nullptr: run the one-phase form
static void* split_buffer(Handle* h, hipStream_t st, size_t need, hipError_t& err)
{
    err = hipSuccess;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return nullptr;
    const bool capturing = cs != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lk(h->split_mtx);
    auto it = h->split.find(st);
    if (it == h->split.end()) {
        if (capturing) return nullptr;   // no allocation inside a capture: the one-phase form
        // every buffer is kept until alipmpc_destroy (ADVICE r4: an eviction's hipFree synchronised the device and
        // could free a buffer another thread had just been handed); a stream beyond SPLIT_STREAMS runs the one-phase
        // form, which computes the same bits
        // (the closed loop's own group streams do not count: ADVICE r5 — cycling user streams would otherwise leave
        // its episode groups on the one-phase form)
        bool group = false;
        for (int g = 0; g < Handle::MAXG; ++g) group |= st != nullptr && st == h->gst[g];
        size_t users = 0;
        for (auto& kv : h->split) {
            bool gk = false;
            for (int g = 0; g < Handle::MAXG; ++g) gk |= kv.first != nullptr && kv.first == h->gst[g];
            users += gk ? 0 : 1;
        }
        if (!group && users >= Handle::SPLIT_STREAMS) return nullptr;
        Handle::SplitBuf sb;
        if ((err = hipMalloc(&sb.p, need)) != hipSuccess) return nullptr;
        sb.bytes = need;
        it = h->split.emplace(st, sb).first;
    }
    if (it->second.bytes < need) return nullptr;   // (sized for the slots: does not happen)
    return it->second.p;
}

// what solve_plan is told about a solve of the handle's B = P.B instances: the program (a sensitivity solve names its
// own), the cuts, and pair, whether the caller takes the paired phase 2 (the batch API; the closed loop's per-tick
// solves keep the 4-wave form).  The record buffer is the driver's to add.
static SpFacts solve_facts(const Handle* h, SpProgram prog, long long B, bool ordered, int split_it, int split_tr, bool pair)
{
    SpFacts f{};
    f.program = prog;
    f.resto_ipopt = h->cfg.restoration == ALIPMPC_RESTORATION_IPOPT && prog != SP_PROG_DD;
    f.B = B;
    if (prog == SP_PROG_WAVE_F64 || prog == SP_PROG_WAVE_F32) {   // (the programs whose plan reads them)
        f.slots = resident_slots(h);
        if (f.resto_ipopt && prog == SP_PROG_WAVE_F64) f.slots_resto = resident_slots(h, true);
    }
    f.split_it = split_it;
    f.split_tr = split_tr;
    f.split_pair = h->split_pair;
    f.allow_pair = pair;
    f.ordered = ordered;
    return f;
}

// the buffers of one solve: the stream's records and their counters (a split launch) and its hand-off list, which the
// plan's ZERO_LIST step takes
struct SolveBufs {
    void* rec = nullptr;
    uint32_t* cont = nullptr;
    size_t hdr_bytes = 0;
    uint32_t* list = nullptr;
};

// one step of a solve's plan; P: the caller's parameters
static hipError_t issue_step(const Handle* h, const SpStep& s, const KP& P, hipStream_t st, SolveBufs& b)
{
    const bool f32 = h->cfg.precision == ALIPMPC_PREC_FP32, modi = h->cfg.variant == ALIPMPC_VARIANT_MODI;
    switch (s.kind) {
    case SP_ZERO_HEADER: return hipMemsetAsync(b.cont, 0, b.hdr_bytes, st);
    case SP_ZERO_LIST:
        if (hipError_t e = redo_list(h, st, P.B, &b.list)) return e;
        return hipMemsetAsync(b.list, 0, sizeof(uint32_t), st);
    case SP_DD:
        return with_n(h->N, hipErrorInvalidValue,
                      [&](auto n) { return launch_dd<decltype(n)::value>(true, P, smem_bytes(h, true), st); });
    case SP_SENS:
    case SP_SENS_OBS:
        return with_n(h->N, hipErrorInvalidValue, [&](auto n) {
            return launch_sens<decltype(n)::value>(s.kind == SP_SENS_OBS, s.resto, P, smem_bytes(h, true), st);
        });
    case SP_LANE: {   // (with a list: an instance whose line search fails is listed, lane_solve.inc)
        KP K = P;
        K.redo = b.list;
        return f32 ? launch_lane<float>(h->lane_nct, modi, K, st) : launch_lane<double>(h->lane_nct, modi, K, st);
    }
    case SP_WAVE: {   // (phase 1 of a split launch starts the list and phase 2 continues it)
        KP K = P;
        K.redo = b.list;
        K.ckpt_it = s.ckpt_it;
        K.ckpt_tr = s.ckpt_tr;
        K.team = s.team;
        K.resume = s.phase == 2 ? (s.form == SP_PAIR ? 2 : 1) : 0;
        K.ckpt = s.phase ? (double*)b.rec : nullptr;
        K.cont = s.phase ? b.cont : nullptr;
        return with_n(h->N, hipErrorInvalidValue, [&](auto n) {
            return launch_wave<decltype(n)::value>(f32, s.resto, s.form, K, smem_bytes(h, true), st);
        });
    }
    case SP_HANDOFF: {   // slot k of the fp64 work queue solves list[1 + k], k < list[0], on the same stream and queue pair
        KP K = P;
        K.order = reinterpret_cast<const int32_t*>(b.list + 1);
        K.bcount = b.list;
        return with_n(h->N, hipErrorInvalidValue, [&](auto n) {
            return launch_wave<decltype(n)::value>(false, s.resto, s.form, K, smem_bytes(h, true, 1), st);
        });
    }
    }
    return hipErrorInvalidValue;
}

// Every solve of the library: the facts, the buffers, the plan (solve_plan.inc), its steps in order.
static hipError_t launch_solve(Handle* h, const KP& P, hipStream_t st, SpProgram prog, int split_it = 0, int split_tr = 0,
                               bool pair = false)
{
    SpFacts f = solve_facts(h, prog, P.B, P.order != nullptr, split_it, split_tr, pair);
    SolveBufs b;
    if (sp_splits(f)) {
        // records for the slots, not for this B: the buffer of a stream never changes size
        const size_t rec_bytes = ((size_t)f.slots * ckpt_doubles(h->mo4) * sizeof(double) + 255) & ~(size_t)255;
        // (the counters, then instance ids and the two class lists of the single records)
        const size_t need = rec_bytes + ((size_t)cont_hdr(f.slots) + (size_t)CONT_WORDS_PER_SLOT * (size_t)f.slots) * sizeof(uint32_t);
        hipError_t berr = hipSuccess;
        b.rec = split_buffer(h, st, need, berr);
        if (berr != hipSuccess) return berr;
        b.cont = reinterpret_cast<uint32_t*>((char*)b.rec + rec_bytes);
        b.hdr_bytes = (size_t)cont_hdr(f.slots) * sizeof(uint32_t);
    }
    f.records = b.rec != nullptr;
    for (const SpStep& s : solve_plan(f))
        if (hipError_t e = issue_step(h, s, P, st, b)) return e;
    return hipSuccess;
}

static int run_batch(Handle* h, bool solve, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                     const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u0,
                     const double* last_u, double* u_out, double* foot_out, double* x_pred, int32_t* status, int32_t* iters, double* f,
                     double* grad, double* c, double* J, double* cl, double* cu, double* goal_eff, int8_t* row_active,
                     void* hip_stream)
{
    if (!h) return ALIPMPC_EINVAL;
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (B == 0) return ALIPMPC_OK;
    const alipmpc_cfg& cf = h->cfg;
    const bool dd = cf.variant == ALIPMPC_VARIANT_DD;
    const SceneIn scene{x0, goal, leg, cir, nc, elp, ne, u0};
    if (!scene_inputs_ok(cf, scene, true)) return fail(h, ALIPMPC_EINVAL, "missing input pointer");
    if (solve && !u_out) return fail(h, ALIPMPC_EINVAL, "u_out is required");
    if (solve && B >= (int64_t)1 << 31) return fail(h, ALIPMPC_EINVAL, "B >= 2^31 (32-bit work-queue counter)");
    HIPCHK(h, hipSetDevice(h->device));
    // host-facing u: the reference's 5N-vector (LIP) / 2N controls (DD); state dimension 5 / 3
    const int N = h->N, n = dd ? 2 * N : 5 * N, sd = dd ? 3 : 5;
    const size_t Bz = (size_t)B, mm_ = (size_t)h->m_max;
    KP P = make_kp(h, B, solve);
    Staging S(h, hip_stream);
    stage_scene(S, P, h, scene, Bz);
    S.in(P.last_u, last_u, Bz * 2);
    // (a solve's outputs for a solve, an eval's for an eval: the others are null)
    S.out(P.u_out, u_out, Bz * n);
    S.out(P.foot_out, foot_out, Bz * 3);
    S.out(P.x_pred, x_pred, Bz * sd * N);
    S.out(P.status, status, Bz);
    S.out(P.iters, iters, Bz);
    S.out(P.f_out, f, Bz);
    S.out(P.grad_out, grad, Bz * n);
    S.out(P.c_out, c, Bz * mm_);
    S.out(P.J_out, J, Bz * mm_ * n);
    S.out(P.cl_out, cl, Bz * mm_);
    S.out(P.cu_out, cu, Bz * mm_);
    S.out(P.goal_eff_out, goal_eff, Bz * 2);
    S.out(P.active_out, row_active, Bz * mm_);
    if (int e = S.commit()) return e;
    TimedSpan span{h, S.st};
    if (int e = span.begin()) return e;
    HIPCHK(h, solve ? launch_solve(h, P, S.st, program_of(h), h->split_it, h->split_tr, true) : launch_eval_hook(h, P, S.st));
    if (int e = span.end()) return e;
    return S.finish();
}

int alipmpc_solve_batch(void* handle, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                        const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u0,
                        const double* last_u, double* u_out, double* foot_out, double* x_pred, int32_t* status,
                        int32_t* iters, void* hip_stream)
{
    return run_batch((Handle*)handle, true, B, x0, goal, leg, cir, nc, elp, ne, u0, last_u, u_out, foot_out, x_pred, status,
                     iters, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hip_stream);
}

// the calls of alipmpc_solve_sens_batch and alipmpc_solve_sens_obs_batch (obs): a handle in the sensitivity build's domain
// (fp64 wave program, N <= 5); P carries dfoot, du and sens_ok in grad_out, J_out and active_out, and the
// obstacle-sensitivity build's dfoot_obs and du_obs in c_out and cl_out
static int run_sens(Handle* h, bool obs, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                    const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u0,
                    double* u_out, double* foot_out, double* x_pred, int32_t* status, int32_t* iters, double* dfoot,
                    double* du, int32_t* sens_ok, double* dfoot_obs, double* du_obs, void* hip_stream)
{
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "solve_sens: LIP variants only");
    if (cf.precision == ALIPMPC_PREC_FP32) return fail(h, ALIPMPC_EUNSUPPORTED, "solve_sens: fp64 handles only");
    if (h->lane_nct >= 0) return fail(h, ALIPMPC_EUNSUPPORTED, "solve_sens: wave-program handles only");
    if (h->N > 5) return fail(h, ALIPMPC_EUNSUPPORTED, "solve_sens: N <= 5 (the Gauss-Jordan solve's domain, n <= 15)");
    const size_t PC = (size_t)alipmpc_sens_obs_cols(&cf);
    if (obs && PC == 0) return fail(h, ALIPMPC_EINVAL, "solve_sens_obs: the handle has no obstacle slots");
    if (obs && !dfoot_obs) return fail(h, ALIPMPC_EINVAL, "solve_sens_obs: dfoot_obs is required");
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (B == 0) return ALIPMPC_OK;
    const SceneIn scene{x0, goal, leg, cir, nc, elp, ne, u0};
    if (!scene_inputs_ok(cf, scene, true)) return fail(h, ALIPMPC_EINVAL, "missing input pointer");
    if (!u_out || (!obs && !dfoot))
        return fail(h, ALIPMPC_EINVAL, obs ? "u_out is required" : "u_out and dfoot are required");
    if (B >= (int64_t)1 << 31) return fail(h, ALIPMPC_EINVAL, "B >= 2^31 (32-bit work-queue counter)");
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N;
    const size_t Bz = (size_t)B;
    KP P = make_kp(h, B, true);
    Staging S(h, hip_stream);
    stage_scene(S, P, h, scene, Bz);
    S.out(P.u_out, u_out, Bz * 5 * N);
    S.out(P.foot_out, foot_out, Bz * 3);
    S.out(P.x_pred, x_pred, Bz * 5 * N);
    S.out(P.status, status, Bz);
    S.out(P.iters, iters, Bz);
    double *d_dfoot = nullptr, *d_du = nullptr, *d_dfo = nullptr, *d_duo = nullptr;
    int32_t* d_ok = nullptr;
    S.out(d_dfoot, dfoot, Bz * 3 * 7);
    S.out(d_du, du, Bz * 5 * N * 7);
    S.out(d_ok, sens_ok, Bz);
    if (obs) {
        S.out(d_dfo, dfoot_obs, Bz * 3 * PC);
        S.out(d_duo, du_obs, Bz * 5 * N * PC);
    }
    if (int e = S.commit()) return e;
    P.grad_out = d_dfoot;
    P.J_out = d_du;
    P.active_out = reinterpret_cast<int8_t*>(d_ok);
    P.c_out = d_dfo;
    P.cl_out = d_duo;
    TimedSpan span{h, S.st};
    if (int e = span.begin()) return e;
    HIPCHK(h, launch_solve(h, P, S.st, obs ? SP_PROG_SENS_OBS : SP_PROG_SENS));
    if (int e = span.end()) return e;
    return S.finish();
}

// The solve with its sensitivities (DESIGN.md §3.7): one launch of the sensitivity build's work queue.  Its three
// outputs reach the kernel in KP's eval-output slots (sens_wave.inc: sens_dfoot, sens_du, sens_okp), which a solve
// launch leaves unused.
int alipmpc_solve_sens_batch(void* handle, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                             const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u0,
                             const double* last_u, double* u_out, double* foot_out, double* x_pred, int32_t* status,
                             int32_t* iters, double* dfoot, double* du, int32_t* sens_ok, void* hip_stream)
{
    (void)last_u;   // (DD only, and DD has no sensitivity build)
    return run_sens((Handle*)handle, false, B, x0, goal, leg, cir, nc, elp, ne, u0, u_out, foot_out, x_pred, status,
                    iters, dfoot, du, sens_ok, nullptr, nullptr, hip_stream);
}

int32_t alipmpc_sens_obs_cols(const alipmpc_cfg* cfg) { return cfg ? 3 * cfg->nc_max + 5 * cfg->ne_max : 0; }

// The solve with its sensitivities and their obstacle columns (DESIGN.md §3.10): one launch of the
// obstacle-sensitivity build's work queue.  dfoot_obs and du_obs reach the kernel in two further eval-output slots (sens_wave.inc:
// sens_dfoot_obs, sens_du_obs).
int alipmpc_solve_sens_obs_batch(void* handle, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                                 const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                                 const double* u0, const double* last_u, double* u_out, double* foot_out,
                                 double* x_pred, int32_t* status, int32_t* iters, double* dfoot, double* du,
                                 int32_t* sens_ok, double* dfoot_obs, double* du_obs, void* hip_stream)
{
    (void)last_u;
    return run_sens((Handle*)handle, true, B, x0, goal, leg, cir, nc, elp, ne, u0, u_out, foot_out, x_pred, status,
                    iters, dfoot, du, sens_ok, dfoot_obs, du_obs, hip_stream);
}

int alipmpc_eval_batch(void* handle, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                       const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u,
                       const double* last_u, double* f, double* grad, double* c, double* J, double* cl, double* cu,
                       double* goal_eff, int8_t* row_active, void* hip_stream)
{
    return run_batch((Handle*)handle, false, B, x0, goal, leg, cir, nc, elp, ne, u, last_u, nullptr, nullptr, nullptr,
                     nullptr, nullptr, f, grad, c, J, cl, cu, goal_eff, row_active, hip_stream);
}

int alipmpc_rollout_batch(void* handle, int64_t B, int32_t S, const double* x0, const double* goal, const int8_t* leg,
                          const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u0,
                          const double* last_u, double* foot_traj, double* x_traj, int32_t* status_traj,
                          int32_t* iters_traj, int32_t* steps_to_goal, double* u_traj, void* hip_stream)
{
    Handle* h = (Handle*)handle;
    if (!h) return ALIPMPC_EINVAL;
    if (B < 0 || S < 0) return fail(h, ALIPMPC_EINVAL, "B < 0 or S < 0");
    if (B == 0 || S == 0) return ALIPMPC_OK;
    const alipmpc_cfg& cf = h->cfg;
    const bool dd = cf.variant == ALIPMPC_VARIANT_DD;
    if (!scene_inputs_ok(cf, SceneIn{x0, goal, leg, cir, nc, elp, ne, u0}, true))
        return fail(h, ALIPMPC_EINVAL, "missing input pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N, n = dd ? 2 * N : 5 * N, sd = dd ? 3 : 5;
    const size_t Bz = (size_t)B, Sz = (size_t)S;
    KP P = make_kp(h, B, true);
    AdvP A;
    std::memset(&A, 0, sizeof(A));
    Staging Z(h, hip_stream, true);
    const hipStream_t st = Z.st;
    // the working set: the evolving state, warm start and last control, and each step's solve outputs
    struct {
        double *x, *u0, *lu, *u, *foot, *xp;
        int8_t* leg;
        int32_t *st, *it;
        uint8_t* act;
    } l{};
    Z.work(l.x, Bz * sd); Z.work(l.u0, Bz * n); Z.work(l.lu, Bz * 2);
    Z.work(l.u, Bz * n); Z.work(l.foot, Bz * 3); Z.work(l.xp, Bz * N * sd);
    Z.work(l.leg, Bz); Z.work(l.st, Bz); Z.work(l.it, Bz); Z.work(l.act, Bz);
    stage_scene(Z, P, h, SceneIn{nullptr, goal, nullptr, cir, nc, elp, ne, nullptr}, Bz);
    Z.out(A.foot_traj, foot_traj, Bz * Sz * 3);
    Z.out(A.x_traj, x_traj, Bz * (Sz + 1) * sd);
    Z.out(A.status_traj, status_traj, Bz * Sz);
    Z.out(A.iters_traj, iters_traj, Bz * Sz);
    Z.out(A.steps_to_goal, steps_to_goal, Bz);
    Z.out(A.u_traj, u_traj, Bz * Sz * n);
    if (int e = Z.commit()) return e;
    if (int e = Z.put(l.x, x0, Bz * sd * 8)) return e;
    if (int e = Z.put(l.u0, u0, Bz * n * 8)) return e;
    if (leg)
        if (int e = Z.put(l.leg, leg, Bz)) return e;
    if (last_u) {
        if (int e = Z.put(l.lu, last_u, Bz * 2 * 8)) return e;
    } else {
        HIPCHK(h, hipMemsetAsync(l.lu, 0, Bz * 2 * 8, st));
    }
    const unsigned g1 = (unsigned)((B + 255) / 256);
    hipLaunchKernelGGL(rollout_init_kernel, dim3(g1), dim3(256), 0, st, (long long)B, (int)S, sd, (const double*)l.x,
                       A.x_traj, l.act, A.steps_to_goal);
    HIPCHK(h, hipGetLastError());
    P.x0 = l.x; P.leg = dd ? nullptr : l.leg; P.u0 = l.u0; P.last_u = dd ? l.lu : nullptr; P.active = l.act;
    P.u_out = l.u; P.foot_out = l.foot; P.x_pred = l.xp; P.status = l.st; P.iters = l.it;
    A.B = B; A.S = S; A.N = N; A.sd = sd; A.n = n; A.variant = cf.variant; A.goal = P.goal;
    A.x = l.x; A.u0 = l.u0; A.leg = l.leg; A.last_u = l.lu; A.u = l.u; A.foot = l.foot; A.x_pred = l.xp;
    A.status = l.st; A.iters = l.it; A.active = l.act;
    TimedSpan span{h, st};
    if (int e = span.begin()) return e;
    for (int t = 0; t < S; ++t) {
        HIPCHK(h, launch_solve(h, P, st, program_of(h)));
        A.t = t;
        hipLaunchKernelGGL(advance_kernel, dim3(g1), dim3(256), 0, st, A);
        HIPCHK(h, hipGetLastError());
    }
    if (int e = span.end()) return e;
    return Z.finish();
}

#include "closed_loop_host.inc"   // alipmpc_closed_loop_batch, _schedule_batch, _dataset_batch and their driver

int32_t alipmpc_trace_len(const alipmpc_cfg* cfg)
{
    if (!cfg || cfg->variant == ALIPMPC_VARIANT_DD || !(cfg->dt > 0)) return 0;
    // numpy arange length: ceil((stop - start) / step) with stop = dt + 0.01, step = 0.01; + the x_k row
    return 1 + (int32_t)std::ceil((cfg->dt + 0.01) / 0.01);
}

int alipmpc_trace_batch(void* handle, int64_t B, const double* x0, const double* u, double* trace, void* hip_stream)
{
    Handle* h = (Handle*)handle;
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "trace: LIP variants only");
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (B == 0) return ALIPMPC_OK;
    if (!x0 || !u || !trace) return fail(h, ALIPMPC_EINVAL, "missing pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N, rows = alipmpc_trace_len(&cf);
    const size_t Bz = (size_t)B, nout = Bz * N * rows * 2;
    TrP T;
    std::memset(&T, 0, sizeof(T));
    T.B = B; T.N = N; T.rows = rows; T.step = 0.01;
    const AlipMats am = alip_mats(cf);
    T.beta = am.beta;
    std::memcpy(T.A, am.A, sizeof(T.A));
    std::memcpy(T.W, am.W, sizeof(T.W));
    std::memcpy(T.MA, am.MA, sizeof(T.MA));
    std::memcpy(T.MB, am.MB, sizeof(T.MB));
    Staging Z(h, hip_stream);
    Z.in(T.x0, x0, Bz * 5);
    Z.in(T.u, u, Bz * 5 * N);
    Z.out(T.trace, trace, nout);
    if (int e = Z.commit()) return e;
    const long long total = (long long)B * N * rows;
    hipLaunchKernelGGL(trace_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, Z.st, T);
    HIPCHK(h, hipGetLastError());
    return Z.finish();
}

int32_t alipmpc_audit_summary_len(int32_t n_edges)
{
    if (n_edges < 0 || n_edges > ALIPMPC_AUDIT_MAX_EDGES) return ALIPMPC_EINVAL;
    return AU_HEAD + (n_edges + 1) + AU_CROSS;
}

int alipmpc_audit_batch(void* handle, int64_t B, const double* x0, const double* goal, const int8_t* leg,
                        const double* cir, const int32_t* nc, const double* elp, const int32_t* ne, const double* u,
                        const int32_t* status, double* metrics, int32_t* where, double viol_tol, const double* edges,
                        int32_t n_edges, int64_t* summary, void* hip_stream)
{
    Handle* h = (Handle*)handle;
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "audit: LIP variants only");
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (n_edges < 0 || n_edges > ALIPMPC_AUDIT_MAX_EDGES)
        return fail(h, ALIPMPC_EINVAL, "audit: n_edges outside [0, ALIPMPC_AUDIT_MAX_EDGES]");
    if (n_edges > 0 && !edges) return fail(h, ALIPMPC_EINVAL, "audit: edges is NULL");
    for (int i = 0; i < n_edges; ++i)
        if (!std::isfinite(edges[i]) || (i > 0 && !(edges[i] > edges[i - 1])))
            return fail(h, ALIPMPC_EINVAL, "audit: edges must be finite and strictly increasing");
    if (!std::isfinite(viol_tol) || viol_tol < 0) return fail(h, ALIPMPC_EINVAL, "audit: viol_tol must be finite and >= 0");
    if (!u) return fail(h, ALIPMPC_EINVAL, "audit: u is NULL");
    if (!metrics && !where && !summary) return fail(h, ALIPMPC_EINVAL, "audit: no output requested");
    const SceneIn scene{x0, goal, leg, cir, nc, elp, ne, u};
    if (!scene_inputs_ok(cf, scene, true)) return fail(h, ALIPMPC_EINVAL, "missing input pointer");
    if (!h->dau) return fail(h, ALIPMPC_EUNSUPPORTED, "audit: the plan has no dense trace (dt <= 0)");
    if (B == 0) return ALIPMPC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int N = h->N;
    const size_t Bz = (size_t)B, nsum = (size_t)alipmpc_audit_summary_len(n_edges);
    AuP A;
    std::memset(&A, 0, sizeof(A));
    A.kp = make_kp(h, B, false);
    A.N = N;
    A.rows = alipmpc_trace_len(&cf);
    A.n_edges = n_edges;
    A.has_status = status != nullptr;
    A.tab = h->dau;
    A.viol_tol = viol_tol;
    for (int i = 0; i < n_edges; ++i) A.edges[i] = edges[i];
    Staging Z(h, hip_stream);
    stage_scene(Z, A.kp, h, scene, Bz);
    Z.in(A.status, status, Bz);
    Z.out(A.metrics, metrics, Bz * ALIPMPC_AUDIT_COLS);
    Z.out(A.where, where, Bz * ALIPMPC_AUDIT_WHERE);
    Z.inout(A.summary, summary, nsum);   // (added to: a chunked sweep carries it along)
    if (int e = Z.commit()) return e;
    HIPCHK(h, launch_audit(N, A, Z.st));
    return Z.finish();
}

int alipmpc_nominal_gait_batch(void* handle, int64_t B, double vx_max, const double* x, const int8_t* leg,
                               const double* vel_des_in, double* vel_des, double* foot, void* hip_stream)
{
    Handle* h = (Handle*)handle;
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "nominal gait: LIP variants only");
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (B == 0) return ALIPMPC_OK;
    if (!x || !foot || (!leg && !vel_des_in)) return fail(h, ALIPMPC_EINVAL, "missing pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Bz = (size_t)B;
    NgP Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.B = B;
    const AlipMats am = alip_mats(cf);
    alip_des_vel(am, cf.dt, vx_max, Q.vdx, Q.vdy0);
    Q.bsh = am.A[10];          // beta sinh(beta T)
    Q.ch = am.ch;
    Q.ibv = 1.0 / am.B[6];     // 1 / (-beta sinh(beta T))
    Staging Z(h, hip_stream);
    Z.in(Q.x, x, Bz * 5);
    Z.in(Q.vin, vel_des_in, Bz * 2);
    Z.in(Q.leg, leg, Bz);
    Z.out(Q.vout, vel_des, Bz * 2);
    Z.out(Q.foot, foot, Bz * 2);
    if (int e = Z.commit()) return e;
    hipLaunchKernelGGL(nominal_gait_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, Z.st, Q);
    HIPCHK(h, hipGetLastError());
    return Z.finish();
}

int alipmpc_scenes_batch(void* handle, int64_t B, uint64_t seed, int64_t first_index, int32_t n_cir, int32_t n_elp,
                         int64_t fields, int32_t max_candidates, double* x0, double* goal, int8_t* leg, double* cir,
                         int32_t* nc, double* elp, int32_t* ne, double* u0, void* hip_stream)
{
    Handle* h = (Handle*)handle;
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "scenes: LIP variants only");
    if (B < 0) return fail(h, ALIPMPC_EINVAL, "B < 0");
    if (n_cir < 0 || n_cir > cf.nc_max) return fail(h, ALIPMPC_EINVAL, "scenes: n_cir outside [0, nc_max]");
    if (n_elp < 0 || n_elp > cf.ne_max) return fail(h, ALIPMPC_EINVAL, "scenes: n_elp outside [0, ne_max]");
    if (n_cir + n_elp > ALIPMPC_MAX_OBS) return fail(h, ALIPMPC_EINVAL, "scenes: n_cir + n_elp > ALIPMPC_MAX_OBS");
    if (n_elp > 0 && n_cir - n_elp != 0 && n_cir - n_elp != 1)
        return fail(h, ALIPMPC_EINVAL, "scenes: a mix field needs n_cir = ceil(tot / 2), n_elp = floor(tot / 2)");
    if (fields < 0) return fail(h, ALIPMPC_EINVAL, "scenes: fields < 0");
    if (max_candidates < 0 || max_candidates > SC_MAX_CAND)
        return fail(h, ALIPMPC_EINVAL, "scenes: max_candidates outside [0, 2^18]");
    const int64_t id_end = (int64_t)1 << 40;
    if (first_index < 0 || first_index > id_end || B > id_end - first_index)
        return fail(h, ALIPMPC_EINVAL, "scenes: global indices outside [0, 2^40)");
    if (B == 0) return ALIPMPC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t Bz = (size_t)B, nem = (size_t)cf.ne_max;
    ScP S;
    std::memset(&S, 0, sizeof(S));
    S.B = B; S.first = first_index; S.fields = fields; S.seed = seed;
    S.n_cir = n_cir; S.n_elp = n_elp; S.nc_max = cf.nc_max; S.ne_max = cf.ne_max; S.N = h->N;
    S.max_cand = max_candidates ? max_candidates : SC_MAX_CAND;
    if (!nem) elp = nullptr, ne = nullptr;   // no ellipse slots: ignored
    Staging Z(h, hip_stream);
    Z.out(S.x0, x0, Bz * 5);
    Z.out(S.goal, goal, Bz * 2);
    Z.out(S.cir, cir, Bz * 3 * cf.nc_max);
    Z.out(S.elp, elp, Bz * 5 * nem);
    Z.out(S.u0, u0, Bz * 5 * h->N);
    Z.out(S.nc, nc, Bz);
    Z.out(S.ne, ne, Bz);
    Z.out(S.leg, leg, Bz);
    if (int e = Z.commit()) return e;
    // one wavefront per instance; a bounded grid strides over larger batches
    const long long blocks = std::min<long long>((B + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 1ll << 20);
    hipLaunchKernelGGL(scenes_kernel, dim3((unsigned)blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, Z.st, S);
    HIPCHK(h, hipGetLastError());
    return Z.finish();
}

#ifdef ALIP_STAMPS
int alipmpc_dbg_stamps(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(alip::g_stamps), sizeof(unsigned long long) * alip::NSTAMP) != hipSuccess)
        return -1;
    if (reset) {
        unsigned long long z[alip::NSTAMP] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(alip::g_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return alip::NSTAMP;
}
#endif

#ifdef ALIP_WSTAMP
// diagnostic: copy the first `slots` per-instance records (8 values each) of the wave program and reset the base
int alipmpc_dbg_wstamps(unsigned long long* out, long long slots)
{
    if (slots > alip::WSTAMP_CAP) slots = alip::WSTAMP_CAP;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(alip::g_wstamp), sizeof(unsigned long long) * 8 * (size_t)slots) != hipSuccess)
        return -1;
    const long long z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(alip::g_wstamp_base), &z, sizeof(z)) != hipSuccess) return -1;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(alip::g_wstamp)) != hipSuccess ||
        hipMemset(p, 0, sizeof(unsigned long long) * 8 * (size_t)alip::WSTAMP_CAP) != hipSuccess)
        return -1;
    return (int)slots;
}
#endif

// test hook (not part of the ABI): wave_helpers_kernel on host arrays — in (nsets x 128), sys (nsys x 90),
// out (nsets x alip::WH_SET), gj_out (nsys x 20); returns alip::WH_SET, or -1 on a HIP error
int alipmpc_dbg_wave_helpers(const double* in, int nsets, const double* sys, int nsys, double* out, double* gj_out)
{
    if (nsets < 0 || nsys < 0 || nsets > 4096 || nsys > 4096) return -1;
    const size_t zi = sizeof(double) * 2 * alip::WAVE * (size_t)nsets, zs = sizeof(double) * 90 * (size_t)nsys;
    const size_t zo = sizeof(double) * alip::WH_SET * (size_t)nsets, zg = sizeof(double) * 20 * (size_t)nsys;
    double* d = nullptr;
    if (hipMalloc((void**)&d, zi + zs + zo + zg + 8) != hipSuccess) return -1;
    double *di = d, *ds = di + 2 * alip::WAVE * (size_t)nsets, *dout = ds + 90 * (size_t)nsys,
           *dg = dout + alip::WH_SET * (size_t)nsets;
    bool ok = (zi == 0 || hipMemcpy(di, in, zi, hipMemcpyHostToDevice) == hipSuccess) &&
              (zs == 0 || hipMemcpy(ds, sys, zs, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        hipLaunchKernelGGL(alip::wave_helpers_kernel, dim3(1), dim3(alip::WAVE), 0, 0, di, nsets, ds, nsys, dout, dg);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             (zo == 0 || hipMemcpy(out, dout, zo, hipMemcpyDeviceToHost) == hipSuccess) &&
             (zg == 0 || hipMemcpy(gj_out, dg, zg, hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? alip::WH_SET : -1;
}

// test hook (not part of the ABI): fastmath_kernel<op> on host arrays of n elements (b: the second argument of
// rcp_div / latan2, otherwise unused and may be null; out1: the cosine of lsincos, otherwise untouched and may be
// null); returns 0, or -1 on a bad argument or a HIP error
extern "C++" {
template <int OP>
static void dbg_fastmath_launch(int op, const double* a, const double* b, long long n, double* o0, double* o1)
{
    if constexpr (OP < alip::FM_OPS) {
        if (op == OP)
            hipLaunchKernelGGL(alip::fastmath_kernel<OP>, dim3((unsigned)((n + alip::FM_BLOCK - 1) / alip::FM_BLOCK)),
                               dim3(alip::FM_BLOCK), 0, 0, a, b, n, o0, o1);
        else
            dbg_fastmath_launch<OP + 1>(op, a, b, n, o0, o1);
    }
}
}  // extern "C++"
int alipmpc_dbg_fastmath(int op, const double* a, const double* b, int64_t n, double* out0, double* out1)
{
    if (op < 0 || op >= alip::FM_OPS || n < 0 || n > (int64_t(1) << 22) || !a || !out0) return -1;
    const bool two_in = op == 2 || op == 6 || op == 12 || op == 13, two_out = op == 8 || op == 9;
    if ((two_in && !b) || (two_out && !out1)) return -1;
    if (n == 0) return 0;
    const size_t z = sizeof(double) * (size_t)n;
    double* d = nullptr;
    if (hipMalloc((void**)&d, 4 * z) != hipSuccess) return -1;
    double *da = d, *db = d + n, *d0 = d + 2 * n, *d1 = d + 3 * n;
    bool ok = hipMemcpy(da, a, z, hipMemcpyHostToDevice) == hipSuccess &&
              (!two_in || hipMemcpy(db, b, z, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        dbg_fastmath_launch<0>(op, da, db, (long long)n, d0, d1);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out0, d0, z, hipMemcpyDeviceToHost) == hipSuccess &&
             (!two_out || hipMemcpy(out1, d1, z, hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? 0 : -1;
}

// test hook (not part of the ABI): kkt_solves_kernel on host arrays, one wave per system.  form 0 / 1: gj_regs with
// readlane / row broadcasts, 2: gj_lds (n = 3, 6, 9, 12, 15; x is nsys x n), 3: chol_rows (n = 18; x is
// nsys x n x (n + 1), L and the idg column); sys is nsys x n x (n + 1) rows [K | rhs]; ok gets the verdicts.
// Returns 0, or -1 on a shape the hook does not hold or a HIP error
extern "C++" {
template <int FORM, int N, class R>
static void dbg_kkt_launch(const double* s, int nsys, double* x, int* ok)
{
    hipLaunchKernelGGL((alip::kkt_solves_kernel<FORM, N, R>), dim3(nsys), dim3(alip::WAVE), 0, 0, s, x, ok);
}
template <int FORM, class R>
static bool dbg_kkt_pick(int n, const double* s, int nsys, double* x, int* ok)
{
    switch (n) {
    case 3: dbg_kkt_launch<FORM, 3, R>(s, nsys, x, ok); return true;
    case 6: dbg_kkt_launch<FORM, 6, R>(s, nsys, x, ok); return true;
    case 9: dbg_kkt_launch<FORM, 9, R>(s, nsys, x, ok); return true;
    case 12: dbg_kkt_launch<FORM, 12, R>(s, nsys, x, ok); return true;
    case 15: dbg_kkt_launch<FORM, 15, R>(s, nsys, x, ok); return true;
    default: return false;
    }
}
}  // extern "C++"
int alipmpc_dbg_kkt_solves(int form, int n, int fp32, const double* sys, int nsys, double* x, int32_t* ok)
{
    if (form < 0 || form > 3 || nsys < 0 || nsys > 65536 || n < 1 || n > 18 || !sys || !x || !ok) return -1;
    if (form == 3 ? n != 18 : (n % 3 != 0 || n > 15)) return -1;
    if (nsys == 0) return 0;
    const size_t ns = (size_t)nsys * n * (n + 1), nx = form == 3 ? ns : (size_t)nsys * n;
    double* d = nullptr;
    if (hipMalloc((void**)&d, sizeof(double) * (ns + nx) + sizeof(int) * (size_t)nsys) != hipSuccess) return -1;
    double *ds = d, *dx = d + ns;
    int* dok = (int*)(dx + nx);
    bool ok_ = hipMemcpy(ds, sys, sizeof(double) * ns, hipMemcpyHostToDevice) == hipSuccess &&
               hipMemset(dx, 0, sizeof(double) * nx + sizeof(int) * (size_t)nsys) == hipSuccess;
    if (ok_) {
        if (form == 3) {
            if (fp32) dbg_kkt_launch<3, 18, float>(ds, nsys, dx, dok);
            else dbg_kkt_launch<3, 18, double>(ds, nsys, dx, dok);
        } else if (form == 2) {
            ok_ = fp32 ? dbg_kkt_pick<2, float>(n, ds, nsys, dx, dok) : dbg_kkt_pick<2, double>(n, ds, nsys, dx, dok);
        } else if (form == 1) {
            ok_ = fp32 ? dbg_kkt_pick<1, float>(n, ds, nsys, dx, dok) : dbg_kkt_pick<1, double>(n, ds, nsys, dx, dok);
        } else {
            ok_ = fp32 ? dbg_kkt_pick<0, float>(n, ds, nsys, dx, dok) : dbg_kkt_pick<0, double>(n, ds, nsys, dx, dok);
        }
        ok_ = ok_ && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
              hipMemcpy(x, dx, sizeof(double) * nx, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(ok, dok, sizeof(int) * (size_t)nsys, hipMemcpyDeviceToHost) == hipSuccess;
    }
    hipFree(d);
    return ok_ ? 0 : -1;
}

// test hook (not part of the ABI): the hand-off lists the handle owns for a stream (hip_stream as the batch calls read
// it) — the live one first, then the retired ones, newest first; fills up to cap (address, bytes) pairs and returns the
// number of lists, or -1 on a bad argument.  Host bookkeeping only: no device memory is touched, nothing synchronises.
int alipmpc_dbg_handoff_lists(void* handle, void* hip_stream, uint64_t* addr, uint64_t* bytes, int cap)
{
    Handle* h = (Handle*)handle;
    if (!h || cap < 0 || (cap > 0 && (!addr || !bytes))) return -1;
    const hipStream_t st = stream_of(h, hip_stream);
    std::lock_guard<std::mutex> lk(h->split_mtx);
    int n = 0;
    auto put = [&](const Handle::SplitBuf& b) {
        if (n < cap) {
            addr[n] = (uint64_t)(uintptr_t)b.p;
            bytes[n] = (uint64_t)b.bytes;
        }
        ++n;
    };
    auto it = h->redo.find(st);
    if (it != h->redo.end() && it->second.p) put(it->second);
    for (auto r = h->redo_retired.rbegin(); r != h->redo_retired.rend(); ++r)
        if (r->st == st) put(r->buf);
    return n;
}

const char* alipmpc_build_id(void)
{
#ifdef ALIP_BUILD_ID
    return ALIP_BUILD_ID;
#else
    return "unknown";
#endif
}

double alipmpc_last_kernel_ms(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h || !h->timed) return 0.0;
    if (h->evlast < 0) return 0.0;
    hipEvent_t e0 = h->ev[h->evlast][0], e1 = h->ev[h->evlast][1];
    if (hipEventSynchronize(e1) != hipSuccess) return 0.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 0.0;
    return (double)ms;
}

const char* alipmpc_last_error(void* handle)
{
    Handle* h = (Handle*)handle;
    return h ? h->err.c_str() : "null handle";
}

int alipmpc_solve_slots(void* handle, int64_t* slots)
{
    Handle* h = (Handle*)handle;
    if (!h || !slots) return fail(h, ALIPMPC_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    *slots = resident_slots(h);
    return ALIPMPC_OK;
}

int alipmpc_lane_handoffs(void* handle, void* hip_stream, int64_t* count)
{
    Handle* h = (Handle*)handle;
    if (!h || !count) return fail(h, ALIPMPC_EINVAL, "null argument");
    *count = 0;
    hipStream_t st = stream_of(h, hip_stream);
    void* p = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->split_mtx);
        auto it = h->redo.find(st);
        if (it != h->redo.end()) p = it->second.p;
    }
    if (!p) return ALIPMPC_OK;
    uint32_t c = 0;
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(&c, p, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, ALIPMPC_EHIP, "alipmpc_lane_handoffs: reading the hand-off count");
    *count = c;
    return ALIPMPC_OK;
}

int alipmpc_solve_launches(void* handle, int64_t B, int32_t* launches, int32_t* team)
{
    Handle* h = (Handle*)handle;
    if (!h || !launches || !team) return fail(h, ALIPMPC_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    // the plan of a batch solve on a stream with a record buffer (no launch order on the batch API): its launches other
    // than the hand-off's
    SpFacts f = solve_facts(h, program_of(h), B, false, h->split_it, h->split_tr, true);
    f.records = true;
    *launches = 0;
    *team = 1;
    for (const SpStep& s : solve_plan(f)) {
        if (sp_is_launch(s.kind) && s.kind != SP_HANDOFF) ++*launches;
        if (s.kind == SP_WAVE && s.form == SP_TEAM) *team = TEAM_WAVES;
    }
    return ALIPMPC_OK;
}

const char* alipmpc_solve_program(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return "";
    static thread_local char buf[96];
    const alipmpc_cfg& c = h->cfg;
    const char* r = c.precision == ALIPMPC_PREC_FP32 ? "float" : "double";
    if (c.variant == ALIPMPC_VARIANT_DD) {
        const int rpl = h->mo4 / WAVE;
        std::snprintf(buf, sizeof(buf), "dd_solve_kernel<%d,%d>", h->N, rpl);
    } else if (h->lane_nct == LANE_FORM5) {
        std::snprintf(buf, sizeof(buf), "lane_kernel<%d,5,true,Form<%s>>", h->N, r);
    } else if (h->lane_nct >= 0) {
        std::snprintf(buf, sizeof(buf), "lane_kernel<%d,%d,%s,%s>", h->N, h->lane_nct,
                      c.variant == ALIPMPC_VARIANT_MODI ? "true" : "false", r);
    } else {
        std::snprintf(buf, sizeof(buf), "solve_kernel<%d,%d,%s>", h->N, h->mo4 / 4, r);
    }
    return buf;
}

void alipmpc_destroy(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return;
    hipSetDevice(h->device);
    if (h->own) hipStreamSynchronize(h->own);
    for (double* d : {h->dGp, h->dEp, h->dGu, h->dEu, h->dau})
        if (d) (void)hipFree(d);
    if (h->dq) hipFree(h->dq);
    if (h->dlk) hipFree(h->dlk);
    if (h->dlkf) hipFree(h->dlkf);
    if (h->stage) hipFree(h->stage);
    if (h->rstage) hipFree(h->rstage);
    for (auto& kv : h->split)
        if (kv.second.p) hipFree(kv.second.p);
    for (auto& kv : h->redo)
        if (kv.second.p) hipFree(kv.second.p);
    for (auto& r : h->redo_retired)
        if (r.buf.p) hipFree(r.buf.p);
    for (auto& pr : h->ev)
        for (hipEvent_t e : pr)
            if (e) hipEventDestroy(e);
    if (h->own) hipStreamDestroy(h->own);
    for (int g = 0; g < Handle::MAXG; ++g) {
        if (h->gst[g]) hipStreamDestroy(h->gst[g]);
        if (h->gev[g]) hipEventDestroy(h->gev[g]);
    }
    if (h->gev[Handle::MAXG]) hipEventDestroy(h->gev[Handle::MAXG]);
    delete h;
}

}  // extern "C"
