// Host side of the closed loop: alipmpc_closed_loop_batch, alipmpc_closed_loop_schedule_batch and
// alipmpc_closed_loop_dataset_batch, and the driver behind the three.  Included from host_api.inc, inside its
// extern "C" block.  The kernels are closed_loop.inc's (the guard: audit.inc, the rows: dataset.inc); which launches a
// call issues, and in what order, is cl_ticks.inc's plan.
//
// Without ds and sch the launches, grouping and results are those of alipmpc_closed_loop_batch as it always was:
// everything the dataset and the schedule add is registered after the existing areas and sits behind a test of ds / sch.

static_assert(CL_MODE_FIRST_ORDER == ALIPMPC_CL_BETWEEN_FIRST_ORDER && CL_MODE_GUARDED == ALIPMPC_CL_BETWEEN_GUARDED,
              "cl_ticks.inc's modes are cfg.cl_between's values");

// what the three entry points share
struct ClIn {
    int64_t B;
    int32_t S, f_cyc;
    double kick;
    uint64_t seed;
    const double *x0, *foot0, *goal;
    const int8_t* leg;
    const double* cir;
    const int32_t* nc;
    const double* elp;
    const int32_t* ne;
    double *foot_traj, *x_traj, *hd_traj;
    int32_t *status_traj, *iters_traj, *steps_to_goal;
    double* action_traj;
    void* hip_stream;
};

// the dataset end of alipmpc_closed_loop_dataset_batch (nullptr: no rows)
struct DsArgs {
    int64_t first_index;
    double safe_dis;
    int64_t max_rows;
    double *X, *y_mpc, *y_act;
    int32_t* row_status;
    int64_t* row_start;
};

// a schedule of alipmpc_closed_loop_schedule_batch (nullptr: every tick solves, whatever f_cyc is)
struct SchedArgs {
    uint64_t mask;       // bit i: tick i of every step solves
    double* plan_traj;   // B x S x f_cyc x 5N or NULL
};

// first-order mode: each episode's anchor (xa, ua), and du, dfoot and sens_ok of the sensitivity build that left it
struct ClAnchor {
    double *xa, *ua, *du, *dfoot;
    int32_t* ok;
};

// an episode group: a contiguous range of episodes whose ticks run on a stream of their own
struct ClGroup {
    CLP C;
    KP P;
    hipStream_t s;
    unsigned g1;
    double* plan_traj;
    ClAnchor an;
};

// ALIP flow over the rest of a step from tick index i: cosh, sinh / beta, beta sinh, rest_t / T, with
// rest_t = step_t - i * (step_t / f_cyc)   (main_sim_mpc.py:78)
struct ClRest {
    double ch, shb, bsh, tt;
};
static ClRest cl_rest_flow(double beta, double T, int32_t f_cyc, int i)
{
    const double rest = T - i * (T / f_cyc);
    return ClRest{std::cosh(beta * rest), std::sinh(beta * rest) / beta, std::sinh(beta * rest) * beta,
                  rest * (1.0 / T)};
}

// one call's state
struct ClLoop {
    Handle* h;
    const ClIn& in;
    const DsArgs* ds;
    const SchedArgs* sch;
    Staging Z;
    int N, n;
    size_t Bz, Sz, Fz;
    bool ds_rows;    // are rows wanted (or row_start alone)
    size_t ds_cap;   // the rows the host-mode copies of the row arrays hold
    bool fo_mode, guarded, order_ok;
    CLP C;
    KP P;
    DsP D;
    int32_t* ord = nullptr;
    double* d_plan = nullptr;
    long long* d_rs = nullptr;
    ClAnchor an{};
    AlipMats am;
    int G = 1;
    ClGroup grp[Handle::MAXG];
    CLN Qn;   // a scheduled loop's nominal ticks: the arguments every run shares
    CLB Qb;   // first-order mode: cl_between_run_kernel's arguments, a run's CLN and the step map of cl_first_order_plan
    CLG Qg;   // guarded mode: the guard's arguments, the eval hook's parameters on the scene the solves read

    ClLoop(Handle* h_, const ClIn& in_, const DsArgs* ds_, const SchedArgs* sch_)
        : h(h_), in(in_), ds(ds_), sch(sch_), Z(h_, in_.hip_stream, true), N(h_->N), n(5 * h_->N), Bz((size_t)in_.B),
          Sz((size_t)in_.S), Fz((size_t)in_.f_cyc), P(make_kp(h_, in_.B, true)), am(alip_mats(h_->cfg))
    {
        const alipmpc_cfg& cf = h->cfg;
        ds_rows = ds && (ds->X || ds->y_mpc || ds->y_act || ds->row_status);
        ds_cap = ds ? std::min<size_t>((size_t)ds->max_rows, Bz * Sz * Fz) : 0;
        guarded = sch && cf.cl_between == ALIPMPC_CL_BETWEEN_GUARDED;   // (mode 1 with the guard)
        fo_mode = (sch && cf.cl_between == ALIPMPC_CL_BETWEEN_FIRST_ORDER) || guarded;
        // longest-first launch order of each tick (wave program; opt-in, ALIPMPC_CL_ORDER=1): it puts at most one long
        // instance on a SIMD, but a tick's time is set by its single slowest instance, a warm-started one whose line
        // search halves ~20 times per iteration (tools/cl_wstamps.py, profiles/r3/wst): 52.13 vs 52.00 ms per loop
        const char* oe = std::getenv("ALIPMPC_CL_ORDER");
        order_ok = cf.program != ALIPMPC_PROGRAM_LANE && oe && std::strcmp(oe, "1") == 0;
        std::memset(&C, 0, sizeof(C));
        std::memset(&D, 0, sizeof(D));
        std::memset(&Qn, 0, sizeof(Qn));
        std::memset(&Qb, 0, sizeof(Qb));
        std::memset(&Qg, 0, sizeof(Qg));
    }
};

static int cl_x_cols(const alipmpc_cfg& cf) { return 3 * cf.nc_max + 5 * cf.ne_max + 11; }   // columns of X

// The argument checks.  *empty: the call is valid and has no episode or no step (a dataset call's row_start is then
// all zero, and set here).
static int cl_check_args(Handle* h, const ClIn& a, const DsArgs* ds, const SchedArgs* sch, bool* empty)
{
    *empty = false;
    if (!h) return ALIPMPC_EINVAL;
    const alipmpc_cfg& cf = h->cfg;
    if (cf.variant == ALIPMPC_VARIANT_DD) return fail(h, ALIPMPC_EUNSUPPORTED, "closed loop: LIP variants only");
    if (a.B < 0 || a.S < 0 || a.f_cyc < 1 || !(a.kick >= 0))
        return fail(h, ALIPMPC_EINVAL, "B, S < 0, f_cyc < 1 or kick < 0");
    if (sch) {
        if (a.f_cyc > CL_MAX_F) return fail(h, ALIPMPC_EINVAL, "closed loop schedule: f_cyc outside 1..64");
        if (a.f_cyc < 64 && (sch->mask >> a.f_cyc) != 0)
            return fail(h, ALIPMPC_EINVAL, "closed loop schedule: mpc_mask has a tick at or above f_cyc");
    }
    if (ds) {
        if (ds->first_index < 0 || ds->first_index > (int64_t)1 << 32 || ds->first_index + a.B > (int64_t)1 << 32)
            return fail(h, ALIPMPC_EINVAL, "closed loop dataset: first_index < 0 or first_index + B > 2^32");
        if (!(ds->safe_dis >= 0) || !std::isfinite(ds->safe_dis))
            return fail(h, ALIPMPC_EINVAL, "closed loop dataset: safe_dis negative or not finite");
        if (ds->max_rows < 0) return fail(h, ALIPMPC_EINVAL, "closed loop dataset: max_rows < 0");
        if ((long long)a.S * a.f_cyc * cl_x_cols(cf) > 0x7fffffffLL)
            return fail(h, ALIPMPC_EINVAL, "closed loop dataset: S * f_cyc * columns of X > 2^31 - 1");
    }
    if (a.B == 0 || a.S == 0) {
        *empty = true;
        if (ds && ds->row_start) {   // no rows: row_start is all zero
            if (a.hip_stream == nullptr) {
                std::memset(ds->row_start, 0, ((size_t)a.B + 1) * 8);
            } else {
                HIPCHK(h, hipSetDevice(h->device));
                HIPCHK(h, hipMemsetAsync(ds->row_start, 0, ((size_t)a.B + 1) * 8, stream_of(h, a.hip_stream)));
            }
        }
        return ALIPMPC_OK;
    }
    if (!a.foot0 || !scene_inputs_ok(cf, SceneIn{a.x0, a.goal, a.leg, a.cir, a.nc, a.elp, a.ne, nullptr}, false))
        return fail(h, ALIPMPC_EINVAL, "missing input pointer");
    return ALIPMPC_OK;
}

// The workspace: every array of the call registered with the pointer that is to address it, the buffer grown, the
// plant's initial state uploaded.
static int cl_workspace(ClLoop& L)
{
    Handle* h = L.h;
    const ClIn& a = L.in;
    const DsArgs* ds = L.ds;
    Staging& Z = L.Z;
    CLP& C = L.C;
    KP& P = L.P;
    const size_t Bz = L.Bz, Sz = L.Sz, Fz = L.Fz, n = (size_t)L.n;
    // the working set: plant and controller state, each tick's solve inputs and outputs
    Z.work(C.vdes, Bz * 2); Z.work(C.pose0, Bz * 3);
    Z.work(C.x, Bz * 5); Z.work(C.pst, Bz * 2); Z.work(C.hdv, Bz * 4);
    Z.work(C.mhd, Bz * 3); Z.work(C.plan, Bz * n); Z.work(C.xs, Bz * 5);
    Z.work(C.u0, Bz * n); Z.work(P.u_out, Bz * n); Z.work(P.foot_out, Bz * 3);
    Z.work(P.x_pred, Bz * n); Z.work(C.leg, Bz); Z.work(C.sleg, Bz);
    Z.work(C.flags, Bz); Z.work(C.active, Bz); Z.work(P.status, Bz);
    Z.work(P.iters, Bz);
    Z.work(L.ord, Bz);
    stage_scene(Z, P, h, SceneIn{nullptr, a.goal, nullptr, a.cir, a.nc, a.elp, a.ne, nullptr}, Bz);
    Z.out(C.foot_traj, a.foot_traj, Bz * Sz * 3);
    Z.out(C.x_traj, a.x_traj, Bz * (Sz + 1) * 5);
    Z.out(C.hd_traj, a.hd_traj, Bz * Sz * 2);
    // (row_status is compacted from the ticks' statuses: they are kept even when the caller does not ask for them)
    if (a.status_traj || !(L.ds_rows && ds->row_status)) Z.out(C.status_traj, a.status_traj, Bz * Sz * Fz);
    else Z.work(C.status_traj, Bz * Sz * Fz);
    Z.out(C.iters_traj, a.iters_traj, Bz * Sz * Fz);
    Z.out(C.steps_to_goal, a.steps_to_goal, Bz);
    Z.out(C.action_traj, a.action_traj, Bz * Sz * Fz * 8);
    if (L.sch) Z.out(L.d_plan, L.sch->plan_traj, Bz * Sz * Fz * n);
    if (ds) {   // host mode reads row_start back itself (cl_rows_back): the rows are downloaded once their number is known
        if (Z.host || !ds->row_start) Z.work(L.d_rs, Bz + 1);
        else L.d_rs = (long long*)ds->row_start;
        Z.work(C.ds_nst, Bz);
        if (L.ds_rows) {
            Z.work(C.ds_step, Bz * Sz * DS_STEP);
            Z.work(C.ds_tick, Bz * Sz * Fz * DS_TICK);
            Z.out_area(L.D.X, ds->X, L.ds_cap * (size_t)cl_x_cols(h->cfg));
            Z.out_area(L.D.y_mpc, ds->y_mpc, L.ds_cap * 8);
            Z.out_area(L.D.y_act, ds->y_act, L.ds_cap * 8);
            Z.out_area(L.D.row_status, ds->row_status, L.ds_cap);
        }
    }
    // first-order ticks (cfg.cl_between, a scheduled loop only): each episode's anchor, and the other two outputs of
    // the sensitivity build (a host-pointer schedule registers 32 slots, + 5: within Staging::MAX_SLOTS)
    if (L.fo_mode) {
        ClAnchor& an = L.an;
        Z.work(an.xa, Bz * 5); Z.work(an.ua, Bz * n); Z.work(an.du, Bz * n * 7); Z.work(an.dfoot, Bz * 21);
        Z.work(an.ok, Bz);
    }
    if (int e = Z.commit()) {
        if (Z.alloc_err == hipSuccess) return e;
        (void)hipGetLastError();
        return fail(h, ALIPMPC_EHIP, "closed loop: workspace of " + std::to_string(Z.need) + " bytes" +
                    (L.ds_rows ? " (row staging " + std::to_string(Bz * Sz * Fz * DS_TICK * 8) + " bytes)" : "") +
                    ": " + hipGetErrorString(Z.alloc_err));
    }
    if (int e = Z.put(C.x, a.x0, Bz * 5 * 8)) return e;
    if (int e = Z.put(C.pst, a.foot0, Bz * 2 * 8)) return e;
    if (int e = Z.put(C.leg, a.leg, Bz)) return e;
    return ALIPMPC_OK;
}

// The whole batch's kernel arguments (what no tick changes), and the episodes' initial state on the device.
static int cl_init(ClLoop& L)
{
    Handle* h = L.h;
    const ClIn& a = L.in;
    const alipmpc_cfg& cf = h->cfg;
    CLP& C = L.C;
    KP& P = L.P;
    C.B = a.B; C.S = a.S; C.f = a.f_cyc; C.variant = cf.variant; C.N = L.N; C.kick = a.kick;
    C.seed = (unsigned long long)a.seed;
    C.goal = P.goal; C.u = P.u_out; C.foot = P.foot_out; C.x_pred = P.x_pred; C.status = P.status; C.iters = P.iters;
    const double beta = L.am.beta, T = cf.dt, dt = T / a.f_cyc;
    alip_des_vel(L.am, T, 0.6, C.vdx, C.vdy0);
    C.ch_d = std::cosh(beta * dt); C.shb_d = std::sinh(beta * dt) / beta; C.bsh_d = std::sinh(beta * dt) * beta;
    C.td = dt / T;
    hipLaunchKernelGGL(cl_init_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, L.Z.st, C);
    HIPCHK(h, hipGetLastError());
    P.x0 = C.xs; P.leg = C.sleg; P.u0 = C.u0; P.active = C.active;
    return ALIPMPC_OK;
}

// Episode groups (ALIPMPC_CL_GROUPS, >= 256 episodes each): contiguous ranges of episodes whose ticks run on
// streams of their own, so a tick that waits on one slow instance holds back only its group; the other groups'
// launches fill the device meanwhile.  Every episode runs the same kernels on the same values (the kick is seeded
// by the global episode index), so the outputs do not depend on the grouping (GPU test).
static int cl_make_groups(ClLoop& L)
{
    Handle* h = L.h;
    const alipmpc_cfg& cf = h->cfg;
    const long long B = L.in.B, S = L.in.S;
    int G = env_groups();
#ifdef ALIP_WSTAMP
    G = 1;   // (diagnostic records are indexed by the whole batch)
#endif
    if (L.order_ok) G = 1;   // (the opt-in launch order is a permutation of the whole batch)
    G = (int)std::max<long long>(1, std::min<long long>({(long long)G, (long long)Handle::MAXG, B / 256}));
    L.G = G;
    const long long nn = L.n, SF = S * L.in.f_cyc;
    for (int g = 0; g < G; ++g) {
        const long long b0 = B * g / G, Bg = B * (g + 1) / G - b0;
        auto o = [&](auto& p, long long per) {
            if (p) p += b0 * per;
        };
        ClGroup& gr = L.grp[g];
        CLP& c = gr.C;
        c = L.C;
        c.B = Bg;
        c.b0 = (L.ds ? (long long)L.ds->first_index : 0) + b0;
        o(c.goal, 2); o(c.x, 5); o(c.pst, 2); o(c.hdv, 4); o(c.mhd, 3); o(c.plan, nn); o(c.leg, 1); o(c.flags, 1);
        o(c.xs, 5); o(c.u0, nn); o(c.sleg, 1); o(c.u, nn); o(c.foot, 3); o(c.x_pred, nn); o(c.status, 1);
        o(c.iters, 1); o(c.active, 1); o(c.foot_traj, 3 * S); o(c.x_traj, 5 * (S + 1)); o(c.hd_traj, 2 * S);
        o(c.status_traj, SF); o(c.iters_traj, SF); o(c.steps_to_goal, 1); o(c.action_traj, 8 * SF); o(c.vdes, 2);
        o(c.pose0, 3);
        o(c.ds_tick, DS_TICK * SF); o(c.ds_step, DS_STEP * S); o(c.ds_nst, 1);
        KP& q = gr.P;
        q = L.P;
        q.B = Bg;
        o(q.goal, 2); o(q.cir, 3LL * cf.nc_max); o(q.nc, 1); o(q.elp, 5LL * cf.ne_max); o(q.ne, 1); o(q.x0, 5);
        o(q.leg, 1); o(q.u0, nn); o(q.active, 1); o(q.u_out, nn); o(q.foot_out, 3); o(q.x_pred, nn); o(q.status, 1);
        o(q.iters, 1);
        gr.g1 = (unsigned)((Bg + 255) / 256);
        gr.plan_traj = L.d_plan ? L.d_plan + b0 * SF * nn : nullptr;
        gr.an = L.an;
        o(gr.an.xa, 5); o(gr.an.ua, nn); o(gr.an.du, 7 * nn); o(gr.an.dfoot, 21); o(gr.an.ok, 1);
        gr.s = L.Z.st;
        if (G > 1) {
            if (!h->gst[g]) HIPCHK(h, hipStreamCreateWithFlags(&h->gst[g], hipStreamNonBlocking));
            if (!h->gev[g]) HIPCHK(h, hipEventCreateWithFlags(&h->gev[g], hipEventDisableTiming));
            gr.s = h->gst[g];
        }
    }
    if (G > 1 && !h->gev[Handle::MAXG]) HIPCHK(h, hipEventCreateWithFlags(&h->gev[Handle::MAXG], hipEventDisableTiming));
    return ALIPMPC_OK;
}

// What the launches between the solves share: the rest-flow constants of every tick index (a scheduled loop), the step
// map (first-order mode), the guard's bar (ALIPMPC_CL_GUARD_TOL: development, read per call) and parameters.
static void cl_between_args(ClLoop& L)
{
    const alipmpc_cfg& cf = L.h->cfg;
    const AlipMats& am = L.am;
    if (L.sch) {
        L.Qn.bsh = am.A[10]; L.Qn.ch = am.ch; L.Qn.ibv = 1.0 / am.B[6];
        for (int i = 0; i < L.in.f_cyc; ++i) {
            const ClRest r = cl_rest_flow(am.beta, cf.dt, L.in.f_cyc, i);
            L.Qn.rest[i][0] = r.ch; L.Qn.rest[i][1] = r.shb; L.Qn.rest[i][2] = r.bsh; L.Qn.rest[i][3] = r.tt;
        }
    }
    if (L.fo_mode) {
        std::memcpy(L.Qb.A, am.A, sizeof(L.Qb.A));
        std::memcpy(L.Qb.W, am.W, sizeof(L.Qb.W));
        std::memcpy(L.Qb.MA, am.MA, sizeof(L.Qb.MA));
        std::memcpy(L.Qb.MB, am.MB, sizeof(L.Qb.MB));
    }
    if (L.guarded) {
        L.Qg.tol = ALIPMPC_CL_GUARD_VIOL;
        if (const char* ge = std::getenv("ALIPMPC_CL_GUARD_TOL")) {
            char* end = nullptr;
            const double v = std::strtod(ge, &end);
            if (end != ge && *end == '\0' && !std::isnan(v)) L.Qg.tol = v;
        }
        L.Qg.kp = make_kp(L.h, L.in.B, false);
    }
}

// The nominal ticks of a segment on group g, one launch, plus the first-order kernel on the anchored episodes when the
// step is live (cl_nominal_run_kernel then skips those).  guard (a GUARDED segment, with its tick's rest flow): between
// the two, the guard marks the anchored episodes whose u_fo fails the rows, and the first-order kernel skips those.
static int cl_nominal_ticks(ClLoop& L, int g, const ClSeg& seg, const ClRest* guard)
{
    Handle* h = L.h;
    const ClGroup& gr = L.grp[g];
    CLN& Qn = L.Qn;
    Qn.C = gr.C;
    Qn.t0 = seg.t0;
    Qn.nt = seg.nt;
    Qn.skip_anchored = seg.live ? 1 : 0;
    Qn.plan_traj = gr.plan_traj;
    hipLaunchKernelGGL(cl_nominal_run_kernel, dim3(gr.g1), dim3(256), 0, gr.s, Qn);
    HIPCHK(h, hipGetLastError());
    if (guard) {
        CLG& Qg = L.Qg;
        Qg.kp.B = gr.C.B;
        Qg.kp.goal = gr.P.goal; Qg.kp.cir = gr.P.cir; Qg.kp.nc = gr.P.nc; Qg.kp.elp = gr.P.elp; Qg.kp.ne = gr.P.ne;
        Qg.flags = gr.C.flags; Qg.x = gr.C.x; Qg.pst = gr.C.pst; Qg.hdv = gr.C.hdv; Qg.leg = gr.C.leg;
        Qg.xa = gr.an.xa; Qg.ua = gr.an.ua; Qg.du = gr.an.du;
        Qg.ch = guard->ch; Qg.shb = guard->shb; Qg.bsh = guard->bsh; Qg.tt = guard->tt;
        HIPCHK(h, launch_guard(L.N, Qg, gr.s));
    }
    if (seg.live) {
        CLB& Qb = L.Qb;
        Qb.Q = Qn;
        Qb.xa = gr.an.xa; Qb.ua = gr.an.ua; Qb.du = gr.an.du;
        hipLaunchKernelGGL(cl_between_run_kernel, dim3(gr.g1), dim3(256), 0, gr.s, Qb);
        HIPCHK(h, hipGetLastError());
    }
    return ALIPMPC_OK;
}

// The solve tick of a segment on group g, as alipmpc_closed_loop_batch always ran it.  fired_only (a GUARDED segment):
// the launches act on the episodes the guard marked alone, every one is issued whether or not an episode fired, and
// the solve is the sensitivity build's launch whether or not the tick leaves an anchor.
static int cl_solve_tick(ClLoop& L, int g, const ClSeg& seg, const ClRest& r, bool fired_only)
{
    Handle* h = L.h;
    ClGroup& gr = L.grp[g];
    CLP& Cg = gr.C;
    const hipStream_t sg = gr.s;
    const int fo = fired_only ? 1 : 0;
    Cg.s = seg.s;
    Cg.i = seg.i;
    Cg.ch_r = r.ch; Cg.shb_r = r.shb; Cg.bsh_r = r.bsh; Cg.tr = r.tt;
    hipLaunchKernelGGL(cl_project_kernel, dim3(gr.g1), dim3(256), 0, sg, Cg, fo);
    HIPCHK(h, hipGetLastError());
    KP Ps = gr.P;
    // wave program: after the first tick, solve last tick's long instances first (same bits per instance)
    Ps.order = nullptr;
    if (!fired_only && L.order_ok && (seg.s > 0 || seg.i > 0)) {   // (one group: its arrays are the batch's)
        hipLaunchKernelGGL(cl_order_kernel, dim3(1), dim3(CL_ORDER_THREADS), 0, sg, (const int32_t*)L.P.iters,
                           (const uint8_t*)L.C.active, (long long)L.in.B, L.ord);
        HIPCHK(h, hipGetLastError());
        Ps.order = L.ord;
    }
    // each group's own counter pair (after the ring): its launches run in order on its stream, and no
    // other group or call can take the pair while one of them is in flight (ADVICE r4: ring pairs taken
    // per tick let a group running ticks ahead land on a pair another group's launch still used)
    Ps.queue = h->dq + 2 * (Handle::NQ + g);
#ifdef ALIP_WSTAMP
    if (!fired_only) {   // diagnostic record slots of this tick: (s f_cyc + i) B + instance
        const long long base = seg.t0 * L.in.B;
        HIPCHK(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(alip::g_wstamp_base), &base, sizeof(base), 0,
                                         hipMemcpyHostToDevice, sg));
        HIPCHK(h, hipStreamSynchronize(sg));   // &base is a stack value
    }
#endif
    // first-order mode, a later tick of the step does not solve: the sensitivity build's launch (the solve's
    // own bits, DESIGN.md §3.7) on the group's queue pair, du straight into the group's anchors
    if (seg.anchor || fired_only) {
        Ps.order = nullptr;
        Ps.grad_out = gr.an.dfoot;
        Ps.J_out = gr.an.du;
        Ps.active_out = reinterpret_cast<int8_t*>(gr.an.ok);
        HIPCHK(h, launch_solve(h, Ps, sg, SP_PROG_SENS));
    } else {
        HIPCHK(h, launch_solve(h, Ps, sg, program_of(h), h->cl_split_it, h->cl_split_tr));
    }
    hipLaunchKernelGGL(cl_update_kernel, dim3(gr.g1), dim3(256), 0, sg, Cg, fo);
    HIPCHK(h, hipGetLastError());
    if (gr.plan_traj) {
        hipLaunchKernelGGL(cl_plan_kernel, dim3(gr.g1), dim3(256), 0, sg, Cg, gr.plan_traj, fo);
        HIPCHK(h, hipGetLastError());
    }
    if (seg.anchor || seg.live) {   // (a live anchor bit, and the guard's mark, is cleared by a tick without an anchor)
        CLA A;
        std::memset(&A, 0, sizeof(A));
        A.B = Cg.B; A.n = L.n; A.have = seg.anchor ? 1 : 0; A.active = Cg.active; A.flags = Cg.flags;
        A.xs = Cg.xs; A.u = Cg.u; A.ok = gr.an.ok; A.xa = gr.an.xa; A.ua = gr.an.ua;
        hipLaunchKernelGGL(cl_anchor_kernel, dim3(gr.g1), dim3(256), 0, sg, A);
        HIPCHK(h, hipGetLastError());
    }
    return ALIPMPC_OK;
}

// The launches of the tick plan, segment by segment and group by group.  A GUARDED segment (after a solve of its step
// left anchors) is one tick, so that no episode runs two ticks' worth: the episodes without an anchor run the nominal
// tick, the anchored ones the first-order tick unless the guard fires, and the solve tick's launches then act on the
// fired ones alone (cl_anchor_kernel clears the mark).
static int cl_issue(ClLoop& L)
{
    // (ALIPMPC_CL_FUSE=0: a launch per nominal tick, for the A/B comparison)
    const char* fe = L.sch ? std::getenv("ALIPMPC_CL_FUSE") : nullptr;
    const bool fuse = !(fe && std::strcmp(fe, "0") == 0);
    const ClIn& a = L.in;
    const uint64_t mask = L.sch ? L.sch->mask : 0;
    for (const ClSeg& seg : cl_tick_plan(a.S, a.f_cyc, L.sch != nullptr, mask, L.h->cfg.cl_between, fuse)) {
        ClRest r{};
        if (seg.kind != CL_NOMINAL_RUN) r = cl_rest_flow(L.am.beta, L.h->cfg.dt, a.f_cyc, seg.i);
        for (int g = 0; g < L.G; ++g) {
            if (seg.kind != CL_SOLVE)
                if (int e = cl_nominal_ticks(L, g, seg, seg.kind == CL_GUARDED ? &r : nullptr)) return e;
            if (seg.kind != CL_NOMINAL_RUN)
                if (int e = cl_solve_tick(L, g, seg, r, seg.kind == CL_GUARDED)) return e;
        }
    }
    return ALIPMPC_OK;
}

// rows: scan the steps entered into row_start, then one wavefront per episode compacts its rows
static int cl_rows(ClLoop& L)
{
    Handle* h = L.h;
    const ClIn& a = L.in;
    const alipmpc_cfg& cf = h->cfg;
    const hipStream_t st = L.Z.st;
    DsP& D = L.D;
    hipLaunchKernelGGL(ds_scan_kernel, dim3(1), dim3(DS_SCAN_THREADS), 0, st, (const int32_t*)L.C.ds_nst,
                       (long long)a.B, (int)a.f_cyc, L.d_rs);
    HIPCHK(h, hipGetLastError());
    if (L.ds_rows && L.ds->max_rows > 0) {
        D.B = a.B; D.max_rows = L.ds->max_rows; D.S = a.S; D.f = a.f_cyc; D.nc_max = cf.nc_max; D.ne_max = cf.ne_max;
        D.safe = L.ds->safe_dis; D.T = cf.dt; D.Td = cf.dt / a.f_cyc;
        D.tick = L.C.ds_tick; D.step = L.C.ds_step; D.stt = L.C.status_traj;
        D.cir = L.P.cir; D.nc = L.P.nc; D.elp = L.P.elp; D.ne = L.P.ne; D.goal = L.P.goal; D.row_start = L.d_rs;
        constexpr int WPB = 256 / WAVE;
        hipLaunchKernelGGL(ds_compact_kernel, dim3((unsigned)((a.B + WPB - 1) / WPB)), dim3(256), 0, st, D);
        HIPCHK(h, hipGetLastError());
    }
    return ALIPMPC_OK;
}

// host mode: the rows back to the caller, the total first: only the rows that exist (and fit) are copied back
static int cl_rows_back(ClLoop& L)
{
    Handle* h = L.h;
    const DsArgs* ds = L.ds;
    Staging& Z = L.Z;
    const size_t Bz = L.Bz, ncx = (size_t)cl_x_cols(h->cfg);
    std::vector<long long> rs(Bz + 1);
    if (int e = Z.get(rs.data(), L.d_rs, (Bz + 1) * 8)) return e;
    HIPCHK(h, hipStreamSynchronize(Z.st));
    if (ds->row_start) std::memcpy(ds->row_start, rs.data(), (Bz + 1) * 8);
    const size_t nr = std::min<size_t>((size_t)rs[Bz], L.ds_cap);
    if (nr && ds->X)
        if (int e = Z.get(ds->X, L.D.X, nr * ncx * 8)) return e;
    if (nr && ds->y_mpc)
        if (int e = Z.get(ds->y_mpc, L.D.y_mpc, nr * 8 * 8)) return e;
    if (nr && ds->y_act)
        if (int e = Z.get(ds->y_act, L.D.y_act, nr * 8 * 8)) return e;
    if (nr && ds->row_status)
        if (int e = Z.get(ds->row_status, L.D.row_status, nr * 4)) return e;
    return ALIPMPC_OK;
}

// the closed-loop entry points' driver
static int closed_loop_run(Handle* h, const ClIn& in, const DsArgs* ds, const SchedArgs* sch)
{
    bool empty = false;
    if (int e = cl_check_args(h, in, ds, sch, &empty)) return e;
    if (empty) return ALIPMPC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    ClLoop L(h, in, ds, sch);
    if (int e = cl_workspace(L)) return e;
    if (int e = cl_init(L)) return e;
    if (int e = cl_make_groups(L)) return e;
    const hipStream_t st = L.Z.st;
    TimedSpan span{h, st};
    if (int e = span.begin()) return e;
    if (L.G > 1) {   // fork
        HIPCHK(h, hipEventRecord(h->gev[Handle::MAXG], st));
        for (int g = 0; g < L.G; ++g) HIPCHK(h, hipStreamWaitEvent(L.grp[g].s, h->gev[Handle::MAXG], 0));
    }
    cl_between_args(L);
    if (int e = cl_issue(L)) return e;
    if (L.G > 1) {   // join
        for (int g = 0; g < L.G; ++g) {
            HIPCHK(h, hipEventRecord(h->gev[g], L.grp[g].s));
            HIPCHK(h, hipStreamWaitEvent(st, h->gev[g], 0));
        }
    }
    if (ds)
        if (int e = cl_rows(L)) return e;
    if (int e = span.end()) return e;
    if (L.Z.host && ds)
        if (int e = cl_rows_back(L)) return e;
    return L.Z.finish();
}

int alipmpc_closed_loop_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, double kick, uint64_t seed,
                              const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                              const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                              double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                              int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj, void* hip_stream)
{
    const ClIn in{B, S, f_cyc, kick, seed, x0, foot0, goal, leg, cir, nc, elp, ne, foot_traj, x_traj, hd_traj,
                  status_traj, iters_traj, steps_to_goal, action_traj, hip_stream};
    return closed_loop_run((Handle*)handle, in, nullptr, nullptr);
}

int alipmpc_closed_loop_schedule_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, uint64_t mpc_mask,
                                       double kick, uint64_t seed,
                                       const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                                       const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                                       double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                                       int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj,
                                       double* plan_traj, void* hip_stream)
{
    const ClIn in{B, S, f_cyc, kick, seed, x0, foot0, goal, leg, cir, nc, elp, ne, foot_traj, x_traj, hd_traj,
                  status_traj, iters_traj, steps_to_goal, action_traj, hip_stream};
    const SchedArgs sch{mpc_mask, plan_traj};
    return closed_loop_run((Handle*)handle, in, nullptr, &sch);
}

int alipmpc_closed_loop_dataset_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, double kick, uint64_t seed,
                                      const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                                      const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                                      double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                                      int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj,
                                      int64_t first_index, double safe_dis, int64_t max_rows, double* X, double* y_mpc,
                                      double* y_act, int32_t* row_status, int64_t* row_start, void* hip_stream)
{
    const ClIn in{B, S, f_cyc, kick, seed, x0, foot0, goal, leg, cir, nc, elp, ne, foot_traj, x_traj, hd_traj,
                  status_traj, iters_traj, steps_to_goal, action_traj, hip_stream};
    const DsArgs ds{first_index, safe_dis, max_rows, X, y_mpc, y_act, row_status, row_start};
    return closed_loop_run((Handle*)handle, in, &ds, nullptr);
}
