// ------------------------------------------------------------------------------------------------
// closed loop at the reference's control rate (alipmpc_closed_loop_batch): main_sim_mpc.py:41,65-135 driving
// Logger.set_stf_head / gen_nex_foot_input (data_procs/logger_mpc.py:270-371) on an ALIP plant.  Per tick
// i of step s (rest_t = T - i T / f_cyc):
//   cl_project_kernel  tick 0: set_stf_head (tube_func, avg_hd -> hd_input_pr, hd_input_cos);
//                      x_nex = get_next_states(plant, [stance foot, hd_input_pr], rest_t) (MPC_LIP_modi.py:149-178);
//                      warm start: [x_nex] x 3 on the first call, else the previous plan x_mpc_tar (unshifted,
//                      num_step >= 1 in the driver; sig_step: [g2..gN, gN] as solveMPCCBF does it)
//   solve launch       od_ev = -leg_ind
//   cl_update_kernel   nex_turn, mpc_hds_list, mpc_state_tar from the solve; the plant moves dt = T / f_cyc
//                      around the stance foot (+ an optional seeded velocity kick: plant mismatch); after the
//                      last tick: touchdown, stance foot <- p_list[0][0:2] of that solve, leg_ind <- -leg_ind,
//                      and the episode stops if close_2_goal was reported before this tick (the driver's
//                      real_close check precedes the close2goal update, main_sim_mpc.py:124-135)
// ------------------------------------------------------------------------------------------------
struct CLP {
    long long B;
    long long b0;     // global index of episode 0 of this launch (an episode group's offset: the kick's seed index)
    int S, f, s, i, variant, N;
    double ch_r, shb_r, bsh_r, tr;   // ALIP flow over rest_t: cosh, sinh / beta, beta sinh, rest_t / T
    double ch_d, shb_d, bsh_d, td;   // ... over dt = T / f_cyc
    double kick;
    unsigned long long seed;
    const double* goal;
    double* x;        // B x 5 plant state
    double* pst;      // B x 2 stance foot
    double* hdv;      // B x 4: nex_turn, hd_input_pr, hd_input_cos, -
    double* mhd;      // B x 3 mpc_hds_list
    double* plan;     // B x 5N mpc_state_tar
    int8_t* leg;      // B leg_ind
    uint8_t* flags;   // B: bit 0 active, bit 1 has a plan, bit 2 real_close
    double* xs;       // solve inputs
    double* u0;
    int8_t* sleg;
    const double* u;  // solve outputs
    const double* foot;
    const double* x_pred;
    const int32_t* status;
    const int32_t* iters;
    uint8_t* active;  // the solve's active mask
    double* foot_traj;      // B x S x 3
    double* x_traj;         // B x (S+1) x 5
    double* hd_traj;        // B x S x 2
    int32_t* status_traj;   // B x S x f
    int32_t* iters_traj;    // B x S x f
    int32_t* steps_to_goal; // B
    // task-space-controller command per tick (Logger.gen_nex_foot_input / gen_tsc_control), optional
    double* action_traj;    // B x S x f x 8
    double* vdes;           // B x 2 v_des_map (main_sim_mpc.py:54, 88, 112)
    double* pose0;          // B x 3 the initial pose: origin / heading of the Logger's robot-global frame
    double vdx, vdy0;       // alip_des_vel(0.6, leg_ind) = [vdx, -0.25 * 0.3 * leg_ind * vdy0]
    // imitation-learning rows (alipmpc_closed_loop_dataset_batch, dataset.inc), all three NULL otherwise
    double* ds_tick;        // B x S x f x DS_TICK: plant state (5), planned foothold (2), x_nex (2), v_des (2)
    double* ds_step;        // B x S x DS_STEP: stance foot (2), heading input, leg_ind, touchdown state (5)
    int32_t* ds_nst;        // B: steps entered (wanted for row_start alone too)
};
constexpr int DS_TICK = 11, DS_STEP = 9;

// Logger.angle_A_minus_B (logger_mpc.py:169-175)
__host__ __device__ inline double ang_diff(double A, double B)
{
    double r = A - B;
    if (r < 0 && fabs(r) > M_PI)
        r += 2 * M_PI;
    else if (r > 0 && fabs(r) > M_PI)
        r -= 2 * M_PI;
    return r;
}
// Logger.tube_func (logger_mpc.py:283-300)
__host__ __device__ inline double tube_turn(double turning, double init)
{
    double tv = init;
    if (turning > 0)
        tv += (0.15 > turning ? 0.4 : 0.7) * turning;
    else if (turning < 0)
        tv += (-0.15 < turning ? 0.4 : 0.7) * turning;
    return ang_diff(tv, init);
}

// splitmix64 -> uniform [0, 1): the plant's velocity kick of (episode, step, tick, axis)
__host__ __device__ inline double cl_uniform(unsigned long long seed, long long b, int s, int i, int axis)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull *
                                      (((((unsigned long long)b * 1048576ull + (unsigned long long)s) * 1024ull +
                                         (unsigned long long)i) * 2ull + (unsigned long long)axis) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// The per-tick arithmetic of the loop, stated once for the per-tick kernels (cl_project_kernel, cl_update_kernel) and
// the nominal-run kernel (cl_nominal_run_kernel).
// set_stf_head (logger_mpc.py:270-280) with the plant heading cur: hv = nex_turn, hd_input_pr, hd_input_cos
__device__ inline void cl_set_stf_head(double cur, double* hv, const double* mh)
{
    hv[2] = cur;
    hv[0] = tube_turn(hv[0], cur);
    double sum = hv[0];
    const double nc[3] = {cur, mh[0], mh[1]};
    for (int k = 0; k < 3; ++k) sum += ang_diff(mh[k], nc[k]);
    hv[1] = sum / 4.0;
}
// get_next_states(pos, vel, hd, [foot, hp], t) with the flow constants of t: cosh, sinh / beta, beta sinh, t / T
__device__ inline void cl_flow(const double* x, double fx, double fy, double hp, double ch, double shb, double bsh,
                               double tt, double* xn)
{
    xn[0] = ch * x[0] + shb * x[2] + (1.0 - ch) * fx;
    xn[1] = ch * x[1] + shb * x[3] + (1.0 - ch) * fy;
    xn[2] = bsh * x[0] + ch * x[2] - bsh * fx;
    xn[3] = bsh * x[1] + ch * x[3] - bsh * fy;
    xn[4] = x[4] + tt * hp;
}
// the plant's velocity kick of (episode, step, tick)
__device__ inline void cl_kick(double kick, unsigned long long seed, long long b, int s, int i, double* xn)
{
    if (kick > 0) {
        xn[2] += kick * (2.0 * cl_uniform(seed, b, s, i, 0) - 1.0);
        xn[3] += kick * (2.0 * cl_uniform(seed, b, s, i, 1) - 1.0);
    }
}
// gen_nex_foot_input / cal_foot_input (logger_mpc.py:318-360, logger.py:380-410) + gen_tsc_control (:374-384) for the
// next foothold nf: robot-global frame = the map frame moved to the initial pose p0 (pos/vel_map_glo_2_robo_glo,
// :134-150); the foot frame is the stance foot (fx, fy) rotated by the base heading x[4]; xn x_nex of this tick, vd
// v_des_map, hv nex_turn, hd_input_pr, hd_input_cos.  (Pointers: each value is read where the command uses it.)
__device__ inline void cl_command(const double* p0, const double* nf, double fx, double fy, const double* xn,
                                  const double* vd, const double* x, const double* hv, int f, int i, double* a)
{
    double s0, c0;
    sincos(p0[2], &s0, &c0);
    auto rob = [&](double px, double py, double& rx, double& ry) {
        const double dx = px - p0[0], dy = py - p0[1];
        rx = c0 * dx + s0 * dy;
        ry = -s0 * dx + c0 * dy;
    };
    double nsx, nsy, csx, csy, npx, npy;
    rob(nf[0], nf[1], nsx, nsy);   // nex_stf_rob
    rob(fx, fy, csx, csy);         // pos_stf_rob_glo_frame
    rob(xn[0], xn[1], npx, npy);   // nex_pos_rob
    const double vx = vd[0], vy = vd[1];
    const double nvx = c0 * vx + s0 * vy, nvy = -s0 * vx + c0 * vy;   // nex_vel_rob
    double sb, cb;
    sincos(x[4] - p0[2], &sb, &cb);                         // M_T of hd_base_rob_glo_fram
    a[0] = cb * (nsx - csx) + sb * (nsy - csy);
    a[1] = -sb * (nsx - csx) + cb * (nsy - csy);
    a[2] = 0.0;
    a[3] = hv[1] / f * (i + 4.5) + (hv[2] - p0[2]);         // hd_input_pr ramp + hd_input_cos (robot frame)
    a[4] = cb * (npx - csx) + sb * (npy - csy);
    a[5] = -sb * (npx - csx) + cb * (npy - csy);
    a[6] = cb * nvx + sb * nvy;
    a[7] = 0.0;
    (void)nvy;
}
// the lateral part of alip_des_vel(vx, leg_ind) (MPC_LIP_modi.py:181-186), vdy0 = beta sinh(beta T) / (cosh(beta T) + 1)
__device__ inline double des_vel_y(double leg, double vdy0) { return 0.5 * (-0.5 * leg * 0.3) * vdy0; }
// one axis of cal_foot_with_veldes (MPC_LIP_modi.py:188-194): B_vel^-1 (vel_des - (A x)[2:4]), bsh = beta sinh(beta T),
// ch = cosh(beta T), ibv = 1 / (-beta sinh(beta T))
__device__ inline double veldes_foot(double bsh, double ch, double ibv, double pos, double vel, double vd)
{
    const double a = bsh * pos + ch * vel;
    return ibv * (vd - a);
}

// fired_only (the guarded mode's re-solve of a tick, cl_guard_kernel): the episodes with CL_FLAG_FIRED alone are
// projected and solved; cl_update_kernel and cl_plan_kernel then leave the others' state and rows as they are
constexpr uint8_t CL_FLAG_FIRED = 16;   // CLP::flags bit 4: the guard fired on this tick (cleared by cl_anchor_kernel)
__global__ __launch_bounds__(256) void cl_project_kernel(CLP C, int fired_only)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    const uint8_t fl = C.flags[b];
    const bool on = (fl & 1) && (!fired_only || (fl & CL_FLAG_FIRED));
    C.active[b] = on ? 1 : 0;
    if (!on) return;
    double* x = C.x + 5 * b;
    double* hv = C.hdv + 4 * b;
    const double* mh = C.mhd + 3 * b;
    if (C.i == 0) {
        cl_set_stf_head(x[4], hv, mh);
        if (C.hd_traj) {
            C.hd_traj[((size_t)b * C.S + C.s) * 2] = hv[1];
            C.hd_traj[((size_t)b * C.S + C.s) * 2 + 1] = hv[2];
        }
    }
    // get_next_states(pos, vel, hd, [foot, hd_input_pr], rest_t)
    const double fx = C.pst[2 * b], fy = C.pst[2 * b + 1], hp = hv[1];
    double xn[5];
    cl_flow(x, fx, fy, hp, C.ch_r, C.shb_r, C.bsh_r, C.tr, xn);
    for (int c = 0; c < 5; ++c) C.xs[5 * b + c] = xn[c];
    const int n = 5 * C.N;
    double* g = C.u0 + (size_t)b * n;
    const double* pl = C.plan + (size_t)b * n;
    if (!(fl & 2)) {
        for (int k = 0; k < C.N; ++k)
            for (int c = 0; c < 5; ++c) g[5 * k + c] = xn[c];
    } else if (C.variant == ALIPMPC_VARIANT_SIG_STEP) {
        for (int k = 0; k < C.N; ++k) {
            const int src = k + 1 < C.N ? k + 1 : C.N - 1;
            for (int c = 0; c < 5; ++c) g[5 * k + c] = pl[5 * src + c];
        }
    } else {
        for (int i = 0; i < n; ++i) g[i] = pl[i];
    }
    C.sleg[b] = (int8_t)(-C.leg[b]);
}

// launch order of the next tick's solve (wave program): instances by the iteration count of their last solve,
// longest first (a counting sort; ties in any order), so the instances that will take longest start first and
// the launch does not wait on a late-starting long instance (tools/placement.py: cfg2 0.604 -> 0.417 ms with the
// long instances first).  One workgroup; inactive instances go last.
constexpr int CL_ORDER_THREADS = 1024;
__global__ __launch_bounds__(CL_ORDER_THREADS) void cl_order_kernel(const int32_t* iters, const uint8_t* active,
                                                                    long long B, int32_t* order)
{
    constexpr int NK = 64;
    __shared__ unsigned hist[NK];
    const int t = threadIdx.x;
    auto key = [&](long long b) {
        if (active && !active[b]) return NK - 1;
        const int it = iters[b];
        return NK - 2 - (it < 0 ? 0 : (it > NK - 2 ? NK - 2 : it));
    };
    if (t < NK) hist[t] = 0u;
    __syncthreads();
    for (long long b = t; b < B; b += CL_ORDER_THREADS) atomicAdd(&hist[key(b)], 1u);
    __syncthreads();
    if (t == 0) {
        unsigned acc = 0;
        for (int k = 0; k < NK; ++k) {
            const unsigned c = hist[k];
            hist[k] = acc;
            acc += c;
        }
    }
    __syncthreads();
    for (long long b = t; b < B; b += CL_ORDER_THREADS) order[atomicAdd(&hist[key(b)], 1u)] = (int32_t)b;
}

__global__ __launch_bounds__(256) void cl_update_kernel(CLP C, int fired_only)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    uint8_t fl = C.flags[b];
    if (fired_only && !(fl & CL_FLAG_FIRED)) return;
    const size_t ti = ((size_t)b * C.S + C.s) * C.f + C.i;
    if (!(fl & 1)) {
        if (C.status_traj) C.status_traj[ti] = ALIPMPC_ROLLOUT_DONE;
        if (C.iters_traj) C.iters_traj[ti] = 0;
        if (C.action_traj)
            for (int c = 0; c < 8; ++c) C.action_traj[ti * 8 + c] = NAN;
        if (C.i == C.f - 1) {
            if (C.foot_traj)
                for (int c = 0; c < 3; ++c) C.foot_traj[((size_t)b * C.S + C.s) * 3 + c] = NAN;
            if (C.x_traj)
                for (int c = 0; c < 5; ++c) C.x_traj[((size_t)b * (C.S + 1) + C.s + 1) * 5 + c] = C.x[5 * b + c];
        }
        return;
    }
    const int n = 5 * C.N;
    if (C.status_traj) C.status_traj[ti] = C.status[b];
    if (C.iters_traj) C.iters_traj[ti] = C.iters[b];
    const double* ub = C.u + (size_t)b * n;
    const double* xp = C.x_pred + (size_t)b * n;
    for (int i = 0; i < n; ++i) C.plan[(size_t)b * n + i] = ub[i];
    fl |= 2;
    double* hv = C.hdv + 4 * b;
    hv[0] = C.foot[3 * b + 2];   // nex_turn = nex_contr[2]
    for (int k = 0; k < 3 && k < C.N; ++k) C.mhd[3 * b + k] = xp[5 * k + 4];
    // close_2_goal of this solve (modi |pos_1 - goal| <= 0.15, MPC_LIP_modi.py:108-115; sig_step any step
    // <= 0.35, MPC_LIP_sig_step.py:104-111)
    const double gx_ = C.goal[2 * b], gy_ = C.goal[2 * b + 1];
    bool close = false;
    const int kmax = C.variant == ALIPMPC_VARIANT_SIG_STEP ? C.N : 1;
    const double rad = C.variant == ALIPMPC_VARIANT_MODI ? 0.15 : 0.35;
    for (int k = 0; k < kmax; ++k) {
        const double dx = xp[5 * k] - gx_, dy = xp[5 * k + 1] - gy_;
        close = close || sqrt(dx * dx + dy * dy) <= rad;
    }
    double* x = C.x + 5 * b;
    const double fx = C.pst[2 * b], fy = C.pst[2 * b + 1];
    if (C.ds_tick) {
        // what the reference's logger records of this tick (logger_iml.py:377-401): the plant before it moves, the
        // planned foothold, x_nex and v_des_map before this tick's update
        double* d = C.ds_tick + ti * DS_TICK;
        for (int c = 0; c < 5; ++c) d[c] = x[c];
        d[5] = C.foot[3 * b];
        d[6] = C.foot[3 * b + 1];
        d[7] = C.xs[5 * b];
        d[8] = C.xs[5 * b + 1];
        d[9] = C.vdes[2 * b];
        d[10] = C.vdes[2 * b + 1];
        if (C.i == 0) {
            double* e = C.ds_step + ((size_t)b * C.S + C.s) * DS_STEP;
            e[0] = fx;
            e[1] = fy;
            e[2] = hv[1] + (hv[2] - C.pose0[3 * b + 2]);   // hd_input_pr + hd_input_cos (robot frame)
            e[3] = (double)C.leg[b];
        }
    }
    if (C.ds_nst && C.i == 0) C.ds_nst[b] = C.s + 1;
    if (C.action_traj)   // the command of this tick's plan: p_list[0], x_nex and v_des_map before this tick's update
        cl_command(C.pose0 + 3 * b, C.foot + 3 * b, fx, fy, C.xs + 5 * b, C.vdes + 2 * b, x, hv, C.f, C.i,
                   C.action_traj + ti * 8);
    // vel_des <- mpc_state_tar[0][2:4] after every solve, [1][2:4] at touchdown (main_sim_mpc.py:88, 112)
    if (C.vdes) {
        const int kv = (C.i == C.f - 1 && C.N > 1) ? 1 : 0;
        C.vdes[2 * b] = xp[5 * kv + 2];
        C.vdes[2 * b + 1] = xp[5 * kv + 3];
    }
    // the plant moves dt around the stance foot (+ the velocity kick)
    double xn[5];
    cl_flow(x, fx, fy, hv[1], C.ch_d, C.shb_d, C.bsh_d, C.td, xn);
    cl_kick(C.kick, C.seed, C.b0 + b, C.s, C.i, xn);
    for (int c = 0; c < 5; ++c) x[c] = xn[c];
    if (C.i == C.f - 1) {
        // touchdown: the planned foothold becomes the stance foot, stance switch
        C.pst[2 * b] = C.foot[3 * b];
        C.pst[2 * b + 1] = C.foot[3 * b + 1];
        C.leg[b] = (int8_t)(-C.leg[b]);
        if (C.foot_traj)
            for (int c = 0; c < 3; ++c) C.foot_traj[((size_t)b * C.S + C.s) * 3 + c] = C.foot[3 * b + c];
        if (C.x_traj)
            for (int c = 0; c < 5; ++c) C.x_traj[((size_t)b * (C.S + 1) + C.s + 1) * 5 + c] = xn[c];
        if (C.ds_step)
            for (int c = 0; c < 5; ++c) C.ds_step[((size_t)b * C.S + C.s) * DS_STEP + 4 + c] = xn[c];
        if (fl & 4) {
            fl &= (uint8_t)~1u;
            if (C.steps_to_goal) C.steps_to_goal[b] = C.s + 1;
        }
    }
    if (close) fl |= 4;
    C.flags[b] = fl;
}

__global__ __launch_bounds__(256) void cl_init_kernel(CLP C)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    C.flags[b] = 1;
    for (int k = 0; k < 4; ++k) C.hdv[4 * b + k] = 0.0;   // nex_turn = 0 (logger_mpc.py:90)
    // mpc_hds_list = [0, 0, 0] in the Logger's robot frame, whose origin is the initial pose (logger_mpc.py:27):
    // the initial heading in the map frame the plant and the MPC share here
    for (int k = 0; k < 3; ++k) C.mhd[3 * b + k] = C.x[5 * b + 4];
    if (C.steps_to_goal) C.steps_to_goal[b] = -1;
    if (C.ds_nst) C.ds_nst[b] = 0;
    if (C.x_traj)
        for (int c = 0; c < 5; ++c) C.x_traj[(size_t)b * (C.S + 1) * 5 + c] = C.x[5 * b + c];
    if (C.vdes) {   // vel_des = alip_des_vel(0.6, leg_ind) (main_sim_mpc.py:54)
        C.vdes[2 * b] = C.vdx;
        C.vdes[2 * b + 1] = des_vel_y((double)C.leg[b], C.vdy0);
        C.pose0[3 * b] = C.x[5 * b];
        C.pose0[3 * b + 1] = C.x[5 * b + 1];
        C.pose0[3 * b + 2] = C.x[5 * b + 4];
    }
}

// nominal gait (MPC_LIP_modi.py:181-194): vel_des = alip_des_vel(vx_max, leg_ind) unless a target velocity is
// given, foot = cal_foot_with_veldes(x, vel_des) = B_vel^-1 (vel_des - (A x)[2:4]) with B_vel = -beta sinh(beta T) I
struct NgP {
    long long B;
    double vdx, vdy0;     // sigma vx_max T / 2 and -0.25 step_gap beta sinh(beta T) / (cosh(beta T) + 1) per unit leg_ind
    double bsh, ch, ibv;  // beta sinh(beta T), cosh(beta T), 1 / (-beta sinh(beta T))
    const double* x;
    const int8_t* leg;
    const double* vin;
    double* vout;
    double* foot;
};
__global__ __launch_bounds__(256) void nominal_gait_kernel(NgP Q)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Q.B) return;
    const double* x = Q.x + 5 * b;
    double v0, v1;
    if (Q.vin) {
        v0 = Q.vin[2 * b];
        v1 = Q.vin[2 * b + 1];
    } else {
        v0 = Q.vdx;
        v1 = des_vel_y((double)Q.leg[b], Q.vdy0);
    }
    if (Q.vout) {
        Q.vout[2 * b] = v0;
        Q.vout[2 * b + 1] = v1;
    }
    const double f0 = veldes_foot(Q.bsh, Q.ch, Q.ibv, x[0], x[2], v0);
    const double f1 = veldes_foot(Q.bsh, Q.ch, Q.ibv, x[1], x[3], v1);
    Q.foot[2 * b] = f0;
    Q.foot[2 * b + 1] = f1;
}

// ------------------------------------------------------------------------------------------------
// nominal ticks of the scheduled closed loop (alipmpc_closed_loop_schedule_batch): main_sim_mpc_alip.py:96-105,
// 121-124 driving Logger.cal_foot_input (data_procs/logger.py:380-410).  A tick without a solve projects the plant
// (cl_project_kernel's x_nex), takes the foothold f = cal_foot_with_veldes(x_nex, v_des_map) (nominal_gait_kernel's
// expression), packs the command with f in place of p_list[0][0:2] and moves the plant as cl_update_kernel does;
// nex_turn, mpc_hds_list, the plan, v_des_map and the close flag stay as the last solve left them.  A touchdown on
// such a tick: stance foot <- f, leg_ind <- -leg_ind, v_des_map <- plan row 1 [2:4] (row 0 at N = 1; alip_des_vel(0.6,
// leg_ind) before the first solve), then the stop test.
// One episode per thread over a maximal run of consecutive nominal ticks (it may cross step boundaries): the
// episode's state is loaded once, kept in registers over the run and stored once; the outputs of every tick are
// written as the per-tick kernels write them.  The flow constants of each tick index travel by value.
// ------------------------------------------------------------------------------------------------
constexpr uint8_t CL_FLAG_ANCHOR = 8;   // CLP::flags bit 3, first-order mode: the episode has a valid anchor (below)
constexpr int CL_MAX_F = 64;   // f_cyc of a scheduled loop: a bit of the mask and a row of CLN::rest per tick
struct CLN {
    CLP C;                    // the episode group's arguments (its s, i and rest-flow constants are not read)
    long long t0;             // first tick of the run, s * f + i
    int nt;                   // ticks of the run, t0 + nt <= S * f
    int skip_anchored;        // first-order mode: leave the episodes with the anchor bit to cl_between_run_kernel
    double bsh, ch, ibv;      // cal_foot_with_veldes: beta sinh(beta T), cosh(beta T), 1 / (-beta sinh(beta T))
    double* plan_traj;        // B x S x f x 5N or NULL: NaN rows on these ticks
    double rest[CL_MAX_F][4]; // per tick index: cosh, sinh / beta, beta sinh of rest_t, rest_t / T
};

__global__ __launch_bounds__(256) void cl_nominal_run_kernel(CLN Q)
{
    const CLP& C = Q.C;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    uint8_t fl = C.flags[b];
    if (Q.skip_anchored && (fl & CL_FLAG_ANCHOR)) return;   // (first-order mode: cl_between_run_kernel's episodes)
    double x[5], hv[3], mh[3], p0[3];
    for (int c = 0; c < 5; ++c) x[c] = C.x[5 * b + c];
    for (int c = 0; c < 3; ++c) {
        hv[c] = C.hdv[4 * b + c];
        mh[c] = C.mhd[3 * b + c];
        p0[c] = C.pose0[3 * b + c];
    }
    double fx = C.pst[2 * b], fy = C.pst[2 * b + 1], vd[2] = {C.vdes[2 * b], C.vdes[2 * b + 1]};
    int leg = C.leg[b];
    const int n = 5 * C.N;
    int s = (int)(Q.t0 / C.f), i = (int)(Q.t0 - (long long)s * C.f);
    for (int t = 0; t < Q.nt; ++t) {
        const size_t si = (size_t)b * C.S + s, ti = si * C.f + i;
        if (Q.plan_traj)
            for (int c = 0; c < n; ++c) Q.plan_traj[ti * n + c] = NAN;
        if (C.iters_traj) C.iters_traj[ti] = 0;
        if (!(fl & 1)) {   // (the fills of cl_update_kernel)
            if (C.status_traj) C.status_traj[ti] = ALIPMPC_ROLLOUT_DONE;
            if (C.action_traj)
                for (int c = 0; c < 8; ++c) C.action_traj[ti * 8 + c] = NAN;
            if (i == C.f - 1) {
                if (C.foot_traj)
                    for (int c = 0; c < 3; ++c) C.foot_traj[si * 3 + c] = NAN;
                if (C.x_traj)
                    for (int c = 0; c < 5; ++c) C.x_traj[((size_t)b * (C.S + 1) + s + 1) * 5 + c] = x[c];
            }
        } else {
            if (C.status_traj) C.status_traj[ti] = ALIPMPC_TICK_NOMINAL;
            if (i == 0) {
                cl_set_stf_head(x[4], hv, mh);
                if (C.hd_traj) {
                    C.hd_traj[si * 2] = hv[1];
                    C.hd_traj[si * 2 + 1] = hv[2];
                }
            }
            const double* r = Q.rest[i];
            double xn[5];
            cl_flow(x, fx, fy, hv[1], r[0], r[1], r[2], r[3], xn);
            const double nf[2] = {veldes_foot(Q.bsh, Q.ch, Q.ibv, xn[0], xn[2], vd[0]),
                                  veldes_foot(Q.bsh, Q.ch, Q.ibv, xn[1], xn[3], vd[1])};
            if (C.action_traj) cl_command(p0, nf, fx, fy, xn, vd, x, hv, C.f, i, C.action_traj + ti * 8);
            double xa[5];
            cl_flow(x, fx, fy, hv[1], C.ch_d, C.shb_d, C.bsh_d, C.td, xa);
            cl_kick(C.kick, C.seed, C.b0 + b, s, i, xa);
            for (int c = 0; c < 5; ++c) x[c] = xa[c];
            if (i == C.f - 1) {   // touchdown on the nominal foothold
                fx = nf[0];
                fy = nf[1];
                leg = -leg;
                if (C.foot_traj) {
                    C.foot_traj[si * 3] = nf[0];
                    C.foot_traj[si * 3 + 1] = nf[1];
                    C.foot_traj[si * 3 + 2] = hv[0];
                }
                if (fl & 2) {
                    const double* pr = C.plan + (size_t)b * n + (C.N > 1 ? 5 : 0);
                    vd[0] = pr[2];
                    vd[1] = pr[3];
                } else {
                    vd[0] = C.vdx;
                    vd[1] = des_vel_y((double)leg, C.vdy0);
                }
                if (C.x_traj)
                    for (int c = 0; c < 5; ++c) C.x_traj[((size_t)b * (C.S + 1) + s + 1) * 5 + c] = x[c];
                if (fl & 4) {
                    fl &= (uint8_t)~1u;
                    if (C.steps_to_goal) C.steps_to_goal[b] = s + 1;
                }
            }
        }
        if (++i == C.f) {
            i = 0;
            ++s;
        }
    }
    for (int c = 0; c < 5; ++c) C.x[5 * b + c] = x[c];
    for (int c = 0; c < 3; ++c) C.hdv[4 * b + c] = hv[c];
    C.pst[2 * b] = fx;
    C.pst[2 * b + 1] = fy;
    C.vdes[2 * b] = vd[0];
    C.vdes[2 * b + 1] = vd[1];
    C.leg[b] = (int8_t)leg;
    C.flags[b] = fl;
}

// ------------------------------------------------------------------------------------------------
// first-order ticks (cfg.cl_between = ALIPMPC_CL_BETWEEN_FIRST_ORDER): between the solves of a step the last solve's
// plan follows the plant to first order, u_fo = ua + du[:, 0:5] (x_nex - xa), about the anchor (xa, ua, du) that
// solve left (its x_nex, its u and alipmpc_solve_sens_batch's du, DESIGN.md §3.7; the goal columns are not read: the
// goal does not move in the loop).  Bit 3 of CLP::flags says that the episode has a valid anchor: set by
// cl_anchor_kernel after a solve tick whose sensitivities are valid, cleared by a later solve of the step without
// them and at every touchdown.  A non-solve tick with the bit set is a solve tick whose outputs are (u_fo, and the
// foothold and predicted states gen_control_test derives from it: cl_first_order_plan); without it, the nominal tick.
// ------------------------------------------------------------------------------------------------
struct CLB {
    CLN Q;
    const double* xa;   // B x 5: x_nex of the anchor solve
    const double* ua;   // B x 5N: its plan
    const double* du;   // B x 5N x 7: its sensitivities (columns 0..4: x0)
    double A[25], W[15], MA[25], MB[25];   // the step map (AlipMats), row-major
};
static_assert(sizeof(CLB) <= 4096, "kernel arguments of cl_between_run_kernel");

// The plan of a first-order tick and what cl_update_kernel takes from a solve's outputs, row by row (N is a run-time
// value: no array of 5N lives in registers): u_fo into plan (and row, the plan_traj row, if not NULL);
// foot = p_0 = W (u_0 - A x_nex); x_{k+1} = M_A x_k + M_B u_k (trace_kernel's expressions), of which mh takes the
// headings of the first three, nvd the velocity of state kv, and the return value is close_2_goal.
__device__ inline bool cl_first_order_plan(const CLB& F, int N, int variant, int kv, const double* goal,
                                           const double* xn, const double* xa, const double* ua, const double* du,
                                           double* plan, double* row, double* foot, double* mh, double* nvd)
{
    double d[5], xk[5];
    for (int c = 0; c < 5; ++c) {
        d[c] = xn[c] - xa[c];
        xk[c] = xn[c];
    }
    const int kmax = variant == ALIPMPC_VARIANT_SIG_STEP ? N : 1;
    const double rad = variant == ALIPMPC_VARIANT_MODI ? 0.15 : 0.35;
    bool close = false;
    for (int k = 0; k < N; ++k) {
        double uk[5];
        for (int c = 0; c < 5; ++c) {
            const double* r = du + (size_t)(5 * k + c) * 7;
            double v = 0.0;
            for (int j = 0; j < 5; ++j) v += r[j] * d[j];
            uk[c] = ua[5 * k + c] + v;
        }
        if (k == 0) {
            double e[5];
            for (int i = 0; i < 5; ++i) {
                double v = 0.0;
                for (int c = 0; c < 5; ++c) v += F.A[i * 5 + c] * xn[c];
                e[i] = uk[i] - v;
            }
            for (int i = 0; i < 3; ++i) {
                double v = 0.0;
                for (int c = 0; c < 5; ++c) v += F.W[i * 5 + c] * e[c];
                foot[i] = v;
            }
        }
        double y[5];
        for (int i = 0; i < 5; ++i) {
            double v = 0.0;
            for (int c = 0; c < 5; ++c) v += F.MA[i * 5 + c] * xk[c];
            for (int c = 0; c < 5; ++c) v += F.MB[i * 5 + c] * uk[c];
            y[i] = v;
        }
        for (int c = 0; c < 5; ++c) {
            xk[c] = y[c];
            plan[5 * k + c] = uk[c];
            if (row) row[5 * k + c] = uk[c];
        }
        if (k == 0) mh[0] = xk[4];
        else if (k == 1) mh[1] = xk[4];
        else if (k == 2) mh[2] = xk[4];
        if (k == kv) {
            nvd[0] = xk[2];
            nvd[1] = xk[3];
        }
        if (k < kmax) {
            const double dx = xk[0] - goal[0], dy = xk[1] - goal[1];
            close = close || sqrt(dx * dx + dy * dy) <= rad;
        }
    }
    return close;
}

// anchor of a mode-1 solve tick (after cl_update_kernel).  have: the tick ran the sensitivity build (a later tick of
// the step does not solve), which wrote du itself: xa, ua <- this tick's x_nex and u, the anchor bit <- sens_ok.
// Otherwise the bit is cleared (no tick reads it before the touchdown clears it anyway).
struct CLA {
    long long B;
    int n, have;
    const uint8_t* active;   // the solve's active mask (cl_project_kernel)
    uint8_t* flags;
    const double *xs, *u;
    const int32_t* ok;
    double *xa, *ua;
};
__global__ __launch_bounds__(256) void cl_anchor_kernel(CLA Q)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Q.B || !Q.active[b]) return;
    uint8_t fl = Q.flags[b] & (uint8_t)~(CL_FLAG_ANCHOR | CL_FLAG_FIRED);   // (the guarded mode's re-solve ends here)
    if (Q.have && Q.ok[b] != 0) {
        for (int c = 0; c < 5; ++c) Q.xa[5 * b + c] = Q.xs[5 * b + c];
        for (int c = 0; c < Q.n; ++c) Q.ua[(size_t)b * Q.n + c] = Q.u[(size_t)b * Q.n + c];
        fl |= CL_FLAG_ANCHOR;
    }
    Q.flags[b] = fl;
}

// The first-order ticks of a run of non-solve ticks inside one step, for the episodes whose anchor bit is set (the
// others run cl_nominal_run_kernel, which skips these: a nominal tick is computed by one kernel, mode 0's, so that it
// has mode 0's bits).  The bit changes only at a solve tick or a touchdown, i.e. at the ends of such a run, so every
// tick here is first-order: x_nex as the nominal tick has it, cl_first_order_plan, then cl_update_kernel's sequence
// with the state in registers, as cl_nominal_run_kernel keeps it.  (Tick 0 of a step never comes here: the bit is
// set by a solve of the step.)  The anchor rows are read where a tick uses them: 840 B per episode and tick at N = 3,
// from the caches after the first.
__global__ __launch_bounds__(256) void cl_between_run_kernel(CLB F)
{
    const CLN& Q = F.Q;
    const CLP& C = Q.C;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    uint8_t fl = C.flags[b];
    // (guarded mode: an episode whose guard fired on this tick re-solves instead)
    if (!(fl & 1) || !(fl & CL_FLAG_ANCHOR) || (fl & CL_FLAG_FIRED)) return;
    double x[5], hv[3], mh[3], p0[3];
    for (int c = 0; c < 5; ++c) x[c] = C.x[5 * b + c];
    for (int c = 0; c < 3; ++c) {
        hv[c] = C.hdv[4 * b + c];
        mh[c] = C.mhd[3 * b + c];
        p0[c] = C.pose0[3 * b + c];
    }
    double fx = C.pst[2 * b], fy = C.pst[2 * b + 1], vd[2] = {C.vdes[2 * b], C.vdes[2 * b + 1]};
    int leg = C.leg[b];
    const int n = 5 * C.N;
    const int s = (int)(Q.t0 / C.f);
    int i = (int)(Q.t0 - (long long)s * C.f);
    const size_t si = (size_t)b * C.S + s;
    for (int t = 0; t < Q.nt; ++t, ++i) {   // (host: the run stays inside step s)
        const size_t ti = si * C.f + i;
        if (C.status_traj) C.status_traj[ti] = ALIPMPC_TICK_FIRST_ORDER;
        if (C.iters_traj) C.iters_traj[ti] = 0;
        const double* r = Q.rest[i];
        double xn[5], ft[3], nvd[2] = {0.0, 0.0};
        cl_flow(x, fx, fy, hv[1], r[0], r[1], r[2], r[3], xn);
        const bool close = cl_first_order_plan(F, C.N, C.variant, (i == C.f - 1 && C.N > 1) ? 1 : 0, C.goal + 2 * b, xn,
                                               F.xa + 5 * b, F.ua + (size_t)b * n, F.du + (size_t)b * n * 7,
                                               C.plan + (size_t)b * n, Q.plan_traj ? Q.plan_traj + ti * n : nullptr,
                                               ft, mh, nvd);
        hv[0] = ft[2];   // nex_turn
        // the command of this tick's plan: p_0, x_nex and v_des_map before this tick's update
        if (C.action_traj) cl_command(p0, ft, fx, fy, xn, vd, x, hv, C.f, i, C.action_traj + ti * 8);
        vd[0] = nvd[0];
        vd[1] = nvd[1];
        double xa[5];
        cl_flow(x, fx, fy, hv[1], C.ch_d, C.shb_d, C.bsh_d, C.td, xa);
        cl_kick(C.kick, C.seed, C.b0 + b, s, i, xa);
        for (int c = 0; c < 5; ++c) x[c] = xa[c];
        if (i == C.f - 1) {   // touchdown on p_0; the linearisation does not carry over
            fx = ft[0];
            fy = ft[1];
            leg = -leg;
            if (C.foot_traj)
                for (int c = 0; c < 3; ++c) C.foot_traj[si * 3 + c] = ft[c];
            if (C.x_traj)
                for (int c = 0; c < 5; ++c) C.x_traj[((size_t)b * (C.S + 1) + s + 1) * 5 + c] = x[c];
            if (fl & 4) {
                fl &= (uint8_t)~1u;
                if (C.steps_to_goal) C.steps_to_goal[b] = s + 1;
            }
            fl &= (uint8_t)~CL_FLAG_ANCHOR;
        }
        if (close) fl |= 4;
    }
    for (int c = 0; c < 5; ++c) C.x[5 * b + c] = x[c];
    for (int c = 0; c < 3; ++c) {
        C.hdv[4 * b + c] = hv[c];
        C.mhd[3 * b + c] = mh[c];
    }
    C.pst[2 * b] = fx;
    C.pst[2 * b + 1] = fy;
    C.vdes[2 * b] = vd[0];
    C.vdes[2 * b + 1] = vd[1];
    C.leg[b] = (int8_t)leg;
    C.flags[b] = fl;
}

// plan_traj row of a solved tick (after cl_update_kernel): the solve's u, NaN for an episode the tick did not solve
// (fired_only: the rows of the episodes it did not solve are the tick kernels')
__global__ __launch_bounds__(256) void cl_plan_kernel(CLP C, double* plan_traj, int fired_only)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= C.B) return;
    const int n = 5 * C.N;
    const size_t ti = ((size_t)b * C.S + C.s) * C.f + C.i;
    const bool on = C.active[b] != 0;
    if (fired_only && !on) return;
    for (int c = 0; c < n; ++c) plan_traj[ti * n + c] = on ? C.u[(size_t)b * n + c] : NAN;
}
