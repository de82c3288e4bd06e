/*
 * alipmpc.h — C ABI of the MI355X batched ALIP-MPC-CBF footstep planner (libalipmpc.so).
 *
 * Drop-in boundary for the reference's per-step NLP solve.  The reference has no C ABI: its planner API
 * is the Python class MPCCBF (MPC_LIP_modi.py:13-391) whose solveMPCCBF (MPC_LIP_modi.py:197-301)
 * hands an NLP plugin object LIP_Prob (MPC_LIP_modi.py:394-655: objective / gradient / constraints /
 * jacobian) to cyipopt.Problem + nlp.solve(u0) (MPC_LIP_modi.py:274-296).  Each entry point below
 * replaces one of those interfaces for a whole batch of independent instances:
 *
 *   alipmpc_solve_batch  <- MPCCBF.select_obs + MPCCBF.solveMPCCBF + cyipopt.Problem.solve, and the
 *                           rollout of MPCCBF.gen_control_test   (MPC_LIP_modi.py:90-112,197-301,325-338;
 *                           MPC_LIP_sig_step.py:89-111,184-278; MPC_DD_sig_step.py:70-97,123-193)
 *   alipmpc_eval_batch   <- LIP_Prob.objective/gradient/constraints/jacobian + the cl/cu/goal set-up
 *                           of solveMPCCBF                     (MPC_LIP_modi.py:205-271,430-583;
 *                           MPC_LIP_sig_step.py:195-254,372-496; MPC_DD_sig_step.py:127-141,351-477)
 *   alipmpc_default_cfg  <- the hard-coded constants of MPCCBF.__init__ / LIP_Prob.__init__
 *                           (MPC_LIP_modi.py:17-45,397-411; MPC_LIP_sig_step.py:17-44,340-353;
 *                           MPC_DD_sig_step.py:15-40,323-338)
 *
 * Conventions
 *   - The caller owns every buffer.  hip_stream == NULL: all pointers are HOST pointers; the library
 *     stages them through its own device workspace and synchronises before returning.
 *     hip_stream != NULL: all pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) and the call
 *     is asynchronous on that stream (no host synchronisation; graph-capturable).  The device allocations are two
 *     per-stream buffers, the split launch's record buffer and the hand-off list (below), both made outside a capture
 *     only and kept until alipmpc_destroy.  The record buffer (alipmpc_solve_launches): one per stream, made by the
 *     stream's first split solve, sized for the resident slots (per slot one loop-state record and three index words: the record's
 *     instance and the two class lists of the paired phase 2) and kept until alipmpc_destroy — a capture on a stream that has
 *     none yet records the one-phase form.  A captured graph uses its capture stream's buffer: replay it on that
 *     stream (or ordered with the solves there).  At most 8 streams per handle hold one (kept until destroy, never
 *     evicted); solves on a further stream run the one-phase form (same bits).  The hand-off list (lane program, and fp32
 *     wave program with cfg.restoration = ALIPMPC_RESTORATION_IPOPT: alipmpc_lane_handoffs): one per stream, B + 1 words,
 *     allocated by the stream's first uncaptured lane or fp32 solve.  It grows only outside a capture — a larger batch
 *     gets a new list of at least twice the bytes, without synchronising — and the old lists are kept until
 *     alipmpc_destroy, so queued launches and captured graphs that hold one stay valid.  A capture therefore needs an
 *     earlier uncaptured solve of at least its B on that stream; without one the captured call fails with ALIPMPC_EHIP.
 *     ALIPMPC_STREAM_NULL selects device pointers on the null (default) stream, whose handle value is 0.
 *   - Every LIP solve launch takes one of the handle's 64 work-queue counter pairs (a ring; each pair is
 *     reset by the last wave of the launch that used it).  A solve captured into a hipGraph bakes in one
 *     pair: do not replay such a graph concurrently with itself, and keep fewer than 64 solve launches of
 *     one handle in flight at once (across all streams), or two launches share counters and instances
 *     are skipped or solved twice.  alipmpc_closed_loop_batch's ticks do not take ring pairs: each of its
 *     episode groups owns one pair of its own (its launches run in order on the group's stream).
 *   - Row-major, instance-major arrays ("B x k" = k contiguous values per instance).
 *   - Return 0 on success, a negative ALIPMPC_E* code on error; alipmpc_last_error(h) gives the text.
 *   - There is no CPU execution path: a handle needs a visible gfx950 device.
 *   - One handle per host thread / stream; distinct handles are independent.
 *
 * Problem layout (variant 0 = "modi" MPC_LIP_modi.py, 1 = "sig_step" MPC_LIP_sig_step.py, 2 = "dd"
 * MPC_DD_sig_step.py):
 *   LIP (0,1): state x = [px, py, vx, vy, theta] (sdim = 5), decision u = [u_1..u_N], u_i in R^5
 *              (n = 5N), foothold p_i = W(u_i - A x_i) = [foot x, foot y, turn].
 *   DD  (2):   state x = [px, py, theta] (sdim = 3), decision u = [v_1, w_1, ..., v_N, w_N] (n = 2N).
 *   Constraint rows are laid out in a FIXED padded order, rows_per_step rows per step k = 0..N-1:
 *     LIP: [vbx, vby, circle slot 0..nc_max-1, ellipse slot 0..ne_max-1, leg, dtheta, (f_en if modi)]
 *     DD : [circle slot 0..nc_max-1, ellipse slot 0..ne_max-1, f_en]
 *   select_obs (modi) compacts the kept obstacles, in input order, into the first slots; unused slots
 *   are inactive (row_active = 0, cl = -inf, cu = +inf, value/Jacobian rows = 0).  Dropping the
 *   inactive rows gives exactly the reference's row order.
 *   The lane program (cfg.program = ALIPMPC_PROGRAM_LANE) keeps the solve's own rows in this slot order without
 *   compacting them (an unselected obstacle's slot stays in place, inactive).  Its shapes, all N = 3:
 *     circles only (ne_max = 0), nc_max <= 6, modi / sig_step: circle slots [cx, cy, r^2];
 *     circles and ellipses (ne_max >= 1), nc_max + ne_max <= 5, modi: 5 quadratic-form slots — slot j < nc_max is
 *     circle j, slot nc_max + j is ellipse j, each (ox, oy, qa, qb, qc, k) with h(p) = qa dx^2 + qb dx dy + qc dy^2 - k
 *     (an ellipse [cx, cy, a, b, phi]: qa = (b cos)^2 + (a sin)^2, qb = 2 cos sin (b^2 - a^2), qc = (b sin)^2 +
 *     (a cos)^2, k = (a b)^2; a circle: qa = qc = 1, qb = 0, k = r^2).  A sixth slot would cost the kernel its fourth
 *     wave per compute unit, so nc_max = 6 stays circles only.
 */
#ifndef ALIPMPC_H
#define ALIPMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIPMPC_VARIANT_MODI 0
#define ALIPMPC_VARIANT_SIG_STEP 1
#define ALIPMPC_VARIANT_DD 2

#define ALIPMPC_PREC_FP64 0
#define ALIPMPC_PREC_FP32 1

/* IPOPT-compatible status codes written to status[] (cyipopt info['status']) */
#define ALIPMPC_SOLVE_SUCCEEDED 0
#define ALIPMPC_SOLVED_TO_ACCEPTABLE_LEVEL 1
#define ALIPMPC_INFEASIBLE_PROBLEM_DETECTED 2
#define ALIPMPC_MAXIMUM_ITERATIONS_EXCEEDED (-1)
#define ALIPMPC_ERROR_IN_STEP_COMPUTATION (-3)   /* KKT regularisation exhausted; last iterate returned */
#define ALIPMPC_INVALID_NUMBER_DETECTED (-13)    /* cfg.goal_singular = ABORT only: see alipmpc_cfg */
/* rollout only: the instance had already reached its goal, no solve was run at this step */
#define ALIPMPC_ROLLOUT_DONE (-10)

/* error codes */
#define ALIPMPC_OK 0
#define ALIPMPC_EINVAL (-1)
#define ALIPMPC_ENODEV (-2)
#define ALIPMPC_EHIP (-3)
#define ALIPMPC_EUNSUPPORTED (-4)

/* cfg.program */
#define ALIPMPC_PROGRAM_WAVE 0
#define ALIPMPC_PROGRAM_LANE 1

/* hip_stream value meaning "device pointers, asynchronous on the null (default) stream" */
#define ALIPMPC_STREAM_NULL ((void*)(intptr_t)-1)

#define ALIPMPC_MAX_N 6      /* horizon limit of the kernels (n = 5N <= 32 -> two 16-column MFMA tiles) */
#define ALIPMPC_MAX_OBS 24   /* nc_max + ne_max limit (and N * rows_per_step <= 128) */

typedef struct alipmpc_cfg {
    int32_t N;          /* horizon (reference: step = 3) */
    int32_t nc_max;     /* circle slots per instance (raw count before select_obs) */
    int32_t ne_max;     /* ellipse slots per instance */
    int32_t variant;    /* ALIPMPC_VARIANT_* */
    int32_t max_iter;   /* interior-point iteration cap */
    int32_t precision;  /* ALIPMPC_PREC_FP64 / _FP32 (device arithmetic; host buffers stay fp64).  With
                           FP32 and tol / acceptable_tol still at the fp64 defaults (1e-8 / 1e-6, below
                           fp32 resolution), alipmpc_create uses the fp32 defaults: 1e-4 / 1e-3 for
                           N <= 3, 3e-4 / 3e-3 for N > 3 */
    int32_t select_obs; /* 1: MPCCBF.select_obs range filter (modi) */
    int32_t detour;     /* 1: local-goal detour heuristic of solveMPCCBF (modi, sig_step) */
    double tol;         /* overall KKT tolerance (IPOPT tol, default 1e-8) */
    double acceptable_tol;
    double dt, H, g;    /* step period T, LIP height, gravity */
    double leg2_max;    /* leg length^2 bound */
    double bvx_lo, bvx_hi, bvy_lo, bvy_hi; /* body-frame velocity bounds (DD: v bounds in bvx_*) */
    double dtheta_max;  /* turning bound (DD: omega bound) */
    double q, p, r;     /* cost weights: position, first-step position, heading */
    double gamma;       /* D-CBF decay */
    double s;           /* f_en turning weight */
    double detect_r2;   /* select_obs range^2 */
    double dd_t;        /* DD control-smoothness weight */
    double mu_init;     /* initial barrier parameter */
    int32_t program;    /* device program (no reference counterpart; the arithmetic of the interior point is the
                           same in both): ALIPMPC_PROGRAM_WAVE — one instance per wavefront (solve_kernel,
                           latency-optimised: small batches); ALIPMPC_PROGRAM_LANE — one instance per lane
                           (lane_kernel, throughput-optimised: batches of 10^5+ instances; N = 3 with either
                           ne_max = 0, nc_max <= 6, modi / sig_step, or ne_max >= 1, nc_max + ne_max <= 5, modi — the
                           obstacle-form build, circles and ellipses; otherwise alipmpc_create returns
                           ALIPMPC_EUNSUPPORTED: other N, DD, sig_step with ellipse slots, more slots).  A per-handle
                           choice, never a function of B: an instance's result does not depend on its batch. */
    int32_t goal_singular; /* a planned state exactly on the goal, where the target heading atan2(g - p) has 0 / 0
                           derivatives (the reference's cal_dtar_ang_du, MPC_LIP_modi.py:650-655, returns NaN there):
                           ALIPMPC_GOAL_SINGULAR_ZERO (0, default) — take them as 0 (atan2(0, 0) = 0 held locally
                           constant; a deviation); ALIPMPC_GOAL_SINGULAR_ABORT (1) — the
                           reference's path: IPOPT's gradient check (Eval_Error on a non-finite objective gradient)
                           ends the solve with status ALIPMPC_INVALID_NUMBER_DETECTED (-13) at the first iterate
                           (starting point or accepted step) with such a state, and that iterate is returned.
                           (Fills the struct's tail padding: sizeof(alipmpc_cfg) is unchanged.) */
    int32_t restoration;   /* what follows a failed filter line search (IPOPT's default path; no reference option
                           selects it): ALIPMPC_RESTORATION_IPOPT (0, default) — IPOPT's feasibility restoration phase:
                           the l1 feasibility problem min rho sum(p + n) + zeta/2 |D_R (x - x_R)|^2 s.t. c(x) - s - p + n
                           = 0 (rho = 1000, zeta = sqrt(mu)) solved by the same interior point until an iterate the
                           original filter accepts with 0.9 of the violation, status 2 (Infeasible_Problem_Detected)
                           only when it converges to a point of local infeasibility;
                           ALIPMPC_RESTORATION_SUBSTITUTE (1) — the rounds-1..5 substitute: the shortest trial step,
                           slacks reset onto c(u), filter reset, status 2 after 6 such events.  The DD variant always
                           runs the substitute.  fp64 wave program: split launches run the phase in their second
                           launch (a failed search in the first cuts the instance there).  Lane program (both
                           precisions) and fp32 wave program: an instance whose search fails is handed to the fp64
                           wave program, which solves it from its start (alipmpc_lane_handoffs counts them); the fp64
                           workspace must then fit the LDS too (alipmpc_create: ALIPMPC_EUNSUPPORTED otherwise). */
    int32_t cl_between;    /* what a tick of alipmpc_closed_loop_schedule_batch that does not solve commands (no other
                           entry point reads it): ALIPMPC_CL_BETWEEN_NOMINAL (0, default) — the nominal ALIP foothold;
                           ALIPMPC_CL_BETWEEN_FIRST_ORDER (1) — the last solve's plan moved to first order with the
                           plant, where that solve's sensitivities are valid (see that entry point);
                           ALIPMPC_CL_BETWEEN_GUARDED (3) — mode 1 with every moved plan held against the constraint
                           rows first: an episode whose plan fails re-solves on that tick.  Modes 1 and 3 need the
                           domain of alipmpc_solve_sens_batch: fp32, the lane program, DD or N = 6 make alipmpc_create
                           return ALIPMPC_EUNSUPPORTED; any other value (2 included) ALIPMPC_EINVAL.  (The former
                           reserved_ field: sizeof(alipmpc_cfg) is unchanged.) */
} alipmpc_cfg;

#define ALIPMPC_CL_BETWEEN_NOMINAL 0
#define ALIPMPC_CL_BETWEEN_FIRST_ORDER 1
#define ALIPMPC_CL_BETWEEN_GUARDED 3
/* the guard's bar on a first-order plan's largest constraint violation (mode 3): alipmpc_audit_batch's customary
 * viol_tol and the restoration's local-infeasibility test */
#define ALIPMPC_CL_GUARD_VIOL 1e-4

#define ALIPMPC_GOAL_SINGULAR_ZERO 0
#define ALIPMPC_GOAL_SINGULAR_ABORT 1

#define ALIPMPC_RESTORATION_IPOPT 0
#define ALIPMPC_RESTORATION_SUBSTITUTE 1

/* Fill *out with the reference's constants for a variant and horizon.  nc_max = ne_max = 6, precision
 * fp64, max_iter = the reference's IPOPT cap (modi 30, sig_step 20, DD 40). */
int alipmpc_default_cfg(int32_t variant, int32_t N, alipmpc_cfg* out);

/* Rows per step and total padded rows (m_max) of the fixed constraint layout for cfg. */
int32_t alipmpc_rows_per_step(const alipmpc_cfg* cfg);
int32_t alipmpc_num_vars(const alipmpc_cfg* cfg);

/* device: HIP device ordinal (>= 0).  Returns ALIPMPC_ENODEV when no gfx950 device is visible. */
int alipmpc_create(const alipmpc_cfg* cfg, int device, void** handle);

/*
 * Solve B independent NLP instances.
 *   x0    B x sdim         initial state (MPCCBF.gen_control_test `state`)
 *   goal  B x 2            goal position (MPCCBF `goals`)
 *   leg   B                od_ev = +-1 (the reference passes -leg_ind)
 *   cir   B x nc_max x 3   inflated circles [cx, cy, r]   (cir_cbf); nc[b] of them valid
 *   elp   B x ne_max x 5   inflated ellipses [cx, cy, a, b, phi] (elp_cbf); ne[b] valid (may be NULL if ne_max == 0)
 *   u0    B x n            initial guess (init_guess)
 *   last_u B x 2           DD only: previous control (may be NULL otherwise)
 * Outputs (any output pointer may be NULL except u_out):
 *   u_out    B x n         solution u
 *   foot_out B x 3         p_list[0] = W(u_1 - A x0) (LIP) / first control [v, w, 0] (DD)
 *   x_pred   B x N x sdim  predicted states x_1..x_N (xk_list[1:])
 *   status   B             IPOPT-compatible status
 *   iters    B             interior-point iterations used
 */
int alipmpc_solve_batch(void* handle, int64_t B,
                        const double* x0, const double* goal, const int8_t* leg,
                        const double* cir, const int32_t* nc,
                        const double* elp, const int32_t* ne,
                        const double* u0, const double* last_u,
                        double* u_out, double* foot_out, double* x_pred,
                        int32_t* status, int32_t* iters,
                        void* hip_stream);

/*
 * alipmpc_solve_batch with the plan's first-order sensitivities to the state and the goal, taken from the solve's own
 * KKT system at the accepted iterate: the barrier KKT conditions differentiated with the barrier
 * parameter and the prologue's piecewise-constant decisions (obstacle selection, leg parity, whether the detour fires
 * and to which side) held fixed.  Where the detour fired its chain rule is folded in: the outputs are total
 * derivatives with respect to the caller's x0 and goal.
 *   Inputs and the outputs u_out .. iters as alipmpc_solve_batch; they are that call's, bit for bit.
 *   dfoot   B x 3 x 7      d foot_out / d theta (required)
 *   du      B x 5N x 7     d u_out / d theta, the canonical u_k = x_{k+1} (may be NULL)
 *   sens_ok B              1: the derivatives are valid; 0: the instance did not end with status 0 or 1, or its KKT
 *                          matrix had a non-positive pivot without regularisation — every derivative of the instance
 *                          is NaN (may be NULL)
 * Columns theta: 0-4 the components of x0, 5-6 the goal.
 * One launch of the work-queue form for every B (no split launch).  Wave program, fp64, LIP variants, N <= 5; fp32
 * handles, lane-program handles, DD and N = 6: ALIPMPC_EUNSUPPORTED.  Host / device pointers as alipmpc_solve_batch.
 */
int alipmpc_solve_sens_batch(void* handle, int64_t B,
                             const double* x0, const double* goal, const int8_t* leg,
                             const double* cir, const int32_t* nc,
                             const double* elp, const int32_t* ne,
                             const double* u0, const double* last_u,
                             double* u_out, double* foot_out, double* x_pred,
                             int32_t* status, int32_t* iters,
                             double* dfoot, double* du, int32_t* sens_ok,
                             void* hip_stream);

/* The plan's sensitivities to the obstacles (alipmpc_sens_obs_cols, alipmpc_solve_sens_obs_batch) are declared in an
 * extension header of their own; a translation unit that includes this header has them too. */
#include "alipmpc_sens_obs.h"

/*
 * Evaluate the NLP callbacks and the set-up at given u (parity / oracle hook).  m_max = N*rows_per_step.
 *   f B, grad B x n, c B x m_max, J B x m_max x n, cl/cu B x m_max, goal_eff B x 2 (after detour),
 *   row_active B x m_max.  Any output may be NULL.
 *   Kernels: N = 3 with circle slots only runs the sweep kernel (lane-per-instance set-up, wave-cooperative
 *   J stores), every other shape eval_kernel; both give the same bits.  Dev knobs (environment):
 *   ALIPMPC_EVAL_KERNEL=group (read by alipmpc_create) forces eval_kernel, ALIPMPC_SWEEP_SHAPE=641 (read per
 *   call) the 64-instance sweep shape.
 */
int alipmpc_eval_batch(void* handle, int64_t B,
                       const double* x0, const double* goal, const int8_t* leg,
                       const double* cir, const int32_t* nc,
                       const double* elp, const int32_t* ne,
                       const double* u, const double* last_u,
                       double* f, double* grad, double* c, double* J,
                       double* cl, double* cu, double* goal_eff, int8_t* row_active,
                       void* hip_stream);

/*
 * Closed-loop receding-horizon rollout of B independent episodes for up to S steps on an ideal ALIP plant
 * (the batch harness that replaces the data_log replay loop: main_sim_mpc.py:66-131 driving
 * logger_mpc.py:318-341 gen_nex_foot_input -> MPCCBF.gen_control_test).  Step t: solve every active
 * instance (as alipmpc_solve_batch), execute the first planned step (x <- x_pred[0], the state at the next
 * touchdown = get_next_states over a full step), switch stance (leg <- -leg), warm-start the next solve
 * from the plan (modi: previous x_mpc_tar unshifted, logger_mpc.py:325-331; sig_step: [g2..gN, gN],
 * MPC_LIP_sig_step.py:186-189; DD: previous controls and last_u <- first control), and retire the
 * instance once close_2_goal holds (the episode stops after that step, main_sim_mpc.py:121-131).
 * Inputs as alipmpc_solve_batch (x0/leg/u0/last_u = the first step's).  Outputs (any may be NULL):
 *   foot_traj     B x S x 3        p_list[0] of each step (NaN after the goal)
 *   x_traj        B x (S+1) x sdim touchdown states x^(0) = x0, x^(1), ...
 *   status_traj   B x S            solve status per step (ALIPMPC_ROLLOUT_DONE after the goal)
 *   iters_traj    B x S            interior-point iterations per step
 *   steps_to_goal B                steps taken until close_2_goal (-1: not within S)
 *   u_traj        B x S x n        the plan (solution u) of every step (NaN after the goal); with x_traj it
 *                                  feeds alipmpc_trace_batch for the per-step predicted traces
 * Host pointers when hip_stream == NULL, else device pointers (asynchronous; S solve launches + S small
 * plant-update launches on the stream, no host synchronisation).
 */
int alipmpc_rollout_batch(void* handle, int64_t B, int32_t S,
                          const double* x0, const double* goal, const int8_t* leg,
                          const double* cir, const int32_t* nc,
                          const double* elp, const int32_t* ne,
                          const double* u0, const double* last_u,
                          double* foot_traj, double* x_traj, int32_t* status_traj, int32_t* iters_traj,
                          int32_t* steps_to_goal, double* u_traj, void* hip_stream);

/*
 * Closed loop at the reference's control rate: B episodes of up to S walking steps with f_cyc MPC solves per
 * step (main_sim_mpc.py:41,65-135, f_cyc = 40: one solve per 10 ms tick of a 0.4 s step) on an ALIP plant —
 * the batch harness of Logger.set_stf_head / gen_nex_foot_input (data_procs/logger_mpc.py:270-371).
 * Tick i of step s (rest_t = T - i T / f_cyc, main_sim_mpc.py:78):
 *   i == 0: set_stf_head with the plant heading: nex_turn <- tube_func(nex_turn, hd), hd_input_pr <- avg_hd(hd),
 *           hd_input_cos <- hd (logger_mpc.py:208-215, 270-300; nex_turn = 0 and mpc_hds_list = the initial heading
 *           initially — the Logger's 0 in its robot frame, whose origin is the initial pose, logger_mpc.py:27,90);
 *   x_nex = get_next_states(pos, vel, hd, [stance foot, hd_input_pr], rest_t) (MPC_LIP_modi.py:149-178);
 *   solve at x_nex with od_ev = -leg_ind; warm start [x_nex] x 3 on the episode's first solve, then the
 *   previous plan x_mpc_tar (logger_mpc.py:327-333 with the driver's num_step >= 1; sig_step: [g2..gN, gN]);
 *   nex_turn <- p_list[0][2], mpc_hds_list <- hd_list;
 *   the plant moves dt = T / f_cyc around the stance foot with the heading advancing hd_input_pr dt / T (the
 *   model get_next_states assumes), plus a velocity kick kick * U(-1, 1) per axis from splitmix64(seed,
 *   episode, step, tick, axis) (plant mismatch; kick = 0: the ideal plant);
 *   after the last tick: touchdown — the stance foot becomes p_list[0][0:2] of that solve, leg_ind <- -leg_ind;
 *   the episode stops there if any earlier solve reported close_2_goal (the driver checks real_close at the
 *   foot change before updating it, main_sim_mpc.py:106-135).
 * Inputs: x0 B x 5 plant state at the first touchdown, foot0 B x 2 its stance foot, goal B x 2, leg B leg_ind
 * (the reference starts at -1), obstacles as alipmpc_solve_batch.  Outputs (any may be NULL):
 *   foot_traj B x S x 3 (p_list[0] of each step's last solve, NaN after the stop), x_traj B x (S+1) x 5
 *   (touchdown states), hd_traj B x S x 2 (hd_input_pr, hd_input_cos of each step), status_traj / iters_traj
 *   B x S x f_cyc (ALIPMPC_ROLLOUT_DONE after the stop), steps_to_goal B (-1: not within S), action_traj
 *   B x S x f_cyc x 8: the task-space-controller command of every tick (Logger.gen_nex_foot_input +
 *   gen_tsc_control, logger_mpc.py:318-384: [foot_input x, y, 0, hd_input_pr / f_cyc (i + 4.5) + hd_input_cos,
 *   nex_pos_fot_loc x, y, nex_vel_fot_loc x, 0] in the Logger's robot-global frame = the map frame moved to the
 *   initial pose; vel_des starts at alip_des_vel(0.6, leg_ind) and follows mpc_state_tar as main_sim_mpc.py:54,
 *   88, 112 do; NaN after the stop).
 * LIP variants only (DD: ALIPMPC_EUNSUPPORTED).  Host / device pointers as alipmpc_solve_batch; S * f_cyc solve
 * launches plus two small kernels per tick on the stream.
 */
int alipmpc_closed_loop_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, double kick, uint64_t seed,
                              const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                              const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                              double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                              int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj, void* hip_stream);

/*
 * The closed loop of alipmpc_closed_loop_batch — same arguments, same outputs, bit for bit — that also writes the
 * imitation-learning rows the reference's logger records per MPC call (data_procs/logger_iml.py:377-401 X and
 * y_mpc, :416-428 y_act; sup_learn/X_data.csv, y_mpc_data.csv, y_act_data.csv).  Every tick (b, s, i) whose solve
 * ran (status != ALIPMPC_ROLLOUT_DONE) gives one row; rows are episode-major, then step, then tick, compacted on the
 * device: episode b owns rows row_start[b] .. row_start[b + 1] - 1 (f_cyc per step it entered), row_start[B] is
 * the total.
 *   X          3 nc_max + 5 ne_max + 11 columns: circle slots [cx, cy, r - safe_dis], ellipse slots [cx, cy,
 *              a - safe_dis, b - safe_dis, phi] as passed (slots past nc / ne zero; safe_dis = 0.4 gives back the
 *              raw radii logger_iml.py:67 records), then the plant's CoM position (2), velocity (2) and heading
 *              before the tick, the stance foot (2), the goal (2), leg_ind (the plant's), rest_t = T - i (T / f_cyc);
 *   y_mpc      8: p_list[0][0:2] of the tick's solve, 0, hd_input_pr + hd_input_cos (robot frame, as action_traj
 *              [..., 3] uses it), x_nex[0:2], v_des_map (2) as it stood before this tick's update;
 *   y_act      8, the same for all f_cyc rows of a step: stance foot after the touchdown (2), 0, plant heading,
 *              CoM position (2) and velocity (2) at the touchdown;
 *   row_status int32, the tick's solve status.
 * first_index: the kick stream's episode id is first_index + b, so a shard of a sweep gives the rows the whole
 * sweep gives (0: alipmpc_closed_loop_batch's stream); first_index < 0 or first_index + B > 2^32: ALIPMPC_EINVAL,
 * as are a negative or non-finite safe_dis and max_rows < 0.  max_rows is the capacity of X / y_mpc / y_act /
 * row_status in rows: rows at positions >= max_rows are not written, row_start (B + 1 entries) is complete
 * whatever max_rows is — compare row_start[B] with max_rows; B * S * f_cyc always suffices.  Any of the five may be
 * NULL (row_start alone sizes a second call).  Row contents depend only on the episode's inputs, seed and
 * first_index + b: not on B, the episode groups or the pointer mode.  Device-pointer calls never synchronise with
 * the host.  The rows cost a B x S x f_cyc x 88-byte staging area in the handle's workspace (ALIPMPC_EHIP with the
 * size in the message if it cannot be allocated) and two kernels after the loop.
 */
int alipmpc_closed_loop_dataset_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, double kick, uint64_t seed,
                                      const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                                      const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                                      double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                                      int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj,
                                      int64_t first_index, double safe_dis, int64_t max_rows, double* X, double* y_mpc,
                                      double* y_act, int32_t* row_status, int64_t* row_start, void* hip_stream);

/*
 * Closed loop that solves on scheduled ticks only: the reference's hybrid driver (main_sim_mpc_alip.py:71-130, 20 ticks
 * per step and ONE solve per step at tick s_mpc = 15, Logger.gen_nex_foot_input; every other tick Logger.cal_foot_input,
 * data_procs/logger.py:380-418) on the plant, inputs, outputs, pointer modes, episode groups, kick stream and stop
 * rule of alipmpc_closed_loop_batch.  Bit i of mpc_mask set: tick i of every step solves.  f_cyc outside 1..64 or a
 * mask bit at or above f_cyc: ALIPMPC_EINVAL; DD: ALIPMPC_EUNSUPPORTED.
 *   A solve tick is alipmpc_closed_loop_batch's tick (the all-ones mask gives its outputs bit for bit, with the same
 *   launches when plan_traj is NULL); plan_traj[b, s, i] also receives the solve's u.
 *   A nominal tick (logger.py:380-410, main_sim_mpc_alip.py:96-105, 121-124): set_stf_head at i == 0 as ever; x_nex =
 *   get_next_states(plant, [stance foot, hd_input_pr], rest_t); the foothold target f = cal_foot_with_veldes(x_nex,
 *   v_des_map) = B_vel^-1 (v_des_map - (A x_nex)[2:4]), the one-step deadbeat ALIP law that realises the plan's
 *   desired touchdown velocity; the command is action_traj's with f in place of p_list[0][0:2]; the plant moves
 *   T / f_cyc and takes the kick.  nex_turn, mpc_hds_list, the plan, v_des_map and the close flag stay as the last solve
 *   left them.  status_traj = ALIPMPC_TICK_NOMINAL, iters_traj = 0, the plan_traj row is NaN.
 *   Touchdown on a nominal last tick: stance foot <- f, foot_traj[b, s] = [f, nex_turn as it stands], leg_ind <-
 *   -leg_ind, v_des_map <- plan row 1 [2:4] (row 0 at N = 1; alip_des_vel(0.6, the new leg_ind) before the first
 *   solve), then the stop test.
 * Deviation: only solves set the close flag, and an episode stops at a touchdown after a solve reported
 * close_2_goal — alipmpc_closed_loop_batch's rule, so that the all-ones mask IS that loop; the reference's hybrid
 * driver breaks at the tick itself (main_sim_mpc_alip.py:129).
 * plan_traj: B x S x f_cyc x 5N, may be NULL (NaN after the stop).  Mask 0 is the nominal gait baseline: no solve.
 * Launches: a maximal run of consecutive nominal ticks — it may cross step boundaries — is ONE launch that keeps the
 * episode's state in registers (mask 1 << 15 at f_cyc 20: two small launches and one solve per step; mask 0: one
 * launch per loop); the flow constants of every tick travel in the launch's arguments, so device-pointer calls stay
 * copy-free and allocation-free.  ALIPMPC_CL_FUSE=0 (development, read per call) launches the same kernel once per
 * nominal tick instead: the same bits.
 *
 * First-order ticks (a handle created with cfg.cl_between = ALIPMPC_CL_BETWEEN_FIRST_ORDER; no reference counterpart):
 * state feedback on the MPC plan at every tick, with no further solve.  "Anchor": the last solve of the current step.
 *   A solve tick is the solve tick above, outputs bit for bit.  When a later tick of its step does not solve it runs
 *   as alipmpc_solve_sens_batch's launch (whose solve outputs are the solve's own bits) and keeps the anchor: xa = its
 *   x_nex, ua = its u, du = its sensitivities; the anchor is valid iff sens_ok.  A later solve of the step replaces
 *   the anchor; every touchdown invalidates it (leg parity and the step's constraints change there).
 *   A non-solve tick with a valid anchor: x_nex as on a nominal tick; u_fo = ua + du[:, 0:5] (x_nex - xa) (the goal
 *   does not move in the loop); p_0 = W (u_fo_0 - A x_nex) and x_{k+1} = M_A x_k + M_B u_fo_k as gen_control_test
 *   derives them; and from there the tick is a solve tick whose outputs are these values: plan <- u_fo (the next
 *   solve's warm start), nex_turn, mpc_hds_list, the close flag, the command with p_0, v_des_map from the predicted
 *   states, the plant move, touchdown on p_0.  status_traj = ALIPMPC_TICK_FIRST_ORDER, iters_traj = 0, the plan_traj
 *   row is u_fo.  The anchor itself does not move: every update linearises about the real solve.
 *   A non-solve tick without one (before the step's first solve, or sens_ok = 0) is the nominal tick, as in mode 0.
 * Held fixed by the linearisation, as by the sensitivities: obstacle selection, the detour decision and the barrier
 * parameter.  u_fo is not checked against the constraints: plan_traj holds it for alipmpc_audit_batch.
 * A mode-1 handle behaves as a mode-0 handle in every other entry point, and here with the all-ones mask or mask 0.
 * Launches: after a solve left anchors, a run of non-solve ticks ends with the step and is two launches per episode
 * group — the nominal kernel for the episodes without a valid anchor (so that their ticks have mode 0's bits) and a
 * first-order kernel for the others; before a step's first such solve, the nominal launch alone, as in mode 0.  The
 * anchors (B x (5 + 5N + 35N + 21) doubles) live in the handle's workspace in both pointer modes.
 *
 * Guarded first-order ticks (cfg.cl_between = ALIPMPC_CL_BETWEEN_GUARDED): mode 1, except that a first-order tick is
 * accepted only if its plan passes the constraint rows, and an episode whose plan fails re-solves on that tick.
 *   On a non-solve tick of an episode with a valid anchor, x_nex and u_fo are formed as above and viol = the largest
 *   max(cl - c, c - cu, 0) over the rows alipmpc_eval_batch returns for (x0 = x_nex, u = u_fo, leg = -leg_ind),
 *   obstacles selected at this x_nex: column 0 of alipmpc_audit_batch for those inputs.  The guard fires iff
 *   !(viol <= ALIPMPC_CL_GUARD_VIOL) — a NaN (a plan or state that is not finite) fires.
 *   Not fired: mode 1's first-order tick, bit for bit.
 *   Fired: a solve tick for that episode alone — the projection of a solve tick, warm start = the loop's current plan
 *   (the previous tick's u_fo, or the anchor plan), alipmpc_solve_sens_batch's launch restricted to the fired episodes,
 *   the solve tick's update.  status_traj and iters_traj hold the solve's values and the plan_traj row its u, so a
 *   triggered tick is one whose mask bit is clear and whose status is none of ALIPMPC_ROLLOUT_DONE, ALIPMPC_TICK_NOMINAL
 *   and ALIPMPC_TICK_FIRST_ORDER.  The solve replaces the anchor when sens_ok and a later tick of the step does not
 *   solve by the mask; otherwise the episode has no anchor until the step's next solve and its ticks are nominal.
 *   Episodes without an anchor run the nominal tick with mode 0's bits; a touchdown invalidates the anchor as before.
 * Not guarded: nominal ticks, and the dense trace's clearance (alipmpc_audit_batch's other columns).  There is no cap
 * on the re-solves of a step.  Only this entry point reads the mode: elsewhere a mode-3 handle is a mode-0 handle, and
 * here with the all-ones mask or mask 0 as well.
 * Launches: after a solve left anchors, the non-solve ticks of the step run one at a time, each as the nominal launch
 * (episodes without an anchor), the guard (cl_guard_kernel: the audit's violation pass on 16-lane groups, which marks
 * the fired episodes), the first-order launch (skips them) and the solve tick's launches acting on the fired episodes
 * alone — every one issued whether or not an episode fired: the host never learns the count, and device-pointer calls
 * stay copy-free and synchronisation-free.  Before a step's first anchor the launches are mode 0's.
 * ALIPMPC_CL_GUARD_TOL (development, read per call as ALIPMPC_CL_FUSE is) replaces the bar: a number as strtod reads
 * it; inf never fires on a finite plan, a negative value always fires; empty, unparsable or NaN: the default.
 */
#define ALIPMPC_TICK_NOMINAL (-20)       /* status_traj: the tick ran the nominal ALIP law, no solve */
#define ALIPMPC_TICK_FIRST_ORDER (-21)   /* status_traj: the tick moved the last solve's plan to first order, no solve */
int alipmpc_closed_loop_schedule_batch(void* handle, int64_t B, int32_t S, int32_t f_cyc, uint64_t mpc_mask,
                                       double kick, uint64_t seed,
                                       const double* x0, const double* foot0, const double* goal, const int8_t* leg,
                                       const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                                       double* foot_traj, double* x_traj, double* hd_traj, int32_t* status_traj,
                                       int32_t* iters_traj, int32_t* steps_to_goal, double* action_traj,
                                       double* plan_traj, void* hip_stream);

/* Nominal gait of a batch (replaces MPCCBF.alip_des_vel / cal_foot_with_veldes, MPC_LIP_modi.py:181-194, used by
 * the driver at main_sim_mpc.py:54 and the ALIP-only loggers):
 *   vel_des = alip_des_vel(vx_max, leg_ind) = [sigma vx_max T / 2, 0.5 (-0.5 leg_ind step_gap) beta sinh(beta T) /
 *             (cosh(beta T) + 1)], sigma = beta coth(beta T / 2), step_gap = 0.3 — or the given vel_des_in (B x 2),
 *   foot    = cal_foot_with_veldes(x, vel_des) = B_vel^-1 (vel_des - (A x)[2:4]), B_vel = B[2:4, 0:2].
 * x B x 5 states, leg B leg_ind (ignored when vel_des_in is given), vel_des B x 2 (may be NULL), foot B x 2.
 * Host pointers with hip_stream = NULL (synchronous), device pointers otherwise. */
int alipmpc_nominal_gait_batch(void* handle, int64_t B, double vx_max, const double* x, const int8_t* leg,
                               const double* vel_des_in, double* vel_des, double* foot, void* hip_stream);

/*
 * Generate B Monte-Carlo scenes on the device: instances g = first_index .. first_index + B - 1 of the sweep
 * (seed, fields, n_cir, n_elp, max_candidates).  Every output row is a pure function of those and g — never of B
 * or of the call that produced it — so a rank generates exactly its shard and a sweep is never scattered.  The
 * distribution is the reference's random obstacle fields (rand_obs.py:31-72: random_circle / random_obs, inflated by
 * safe_dis = 0.4 as main_sim_mpc.py:11,14 does) and the initial states of alipmpc/scenes.py; the function itself and
 * its stream have no reference counterpart.  alipmpc/scenes.py: make_batch_counter restates the stream on the host.
 *
 * The stream.  U(id, stream, ctr) in [0, 1) is splitmix64 of a counter: key = (((id * 4 + stream) << 20) | ctr) + 1,
 * z = seed + 0x9E3779B97F4A7C15 * key, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB,
 * z ^= z >> 31, U = (z >> 11) * 2^-53; id < 2^40, ctr < 2^20, stream 0 = field placement, 1 = ellipse shapes, 2 =
 * instance state.  r2(v) = rint(v * 100) / 100 (np.round(v, 2)).  All arithmetic is fp64, every operation rounded on
 * its own, left to right as written (no fused multiply-add).
 *   Field of instance g: id = g % fields (fields == 0: id = g).  placed = [(10, 10, 0.3), (0, 0, 1.0)], spacing = 0.8,
 *   tries = 0.  Candidate c = 0, 1, ...: x = r2(8.5 U(ctr 3c)), y = r2(8.5 U(3c + 1)), r = r2(0.65 U(3c + 2) + 0.35),
 *   accepted when (x-cx)*(x-cx) + (y-cy)*(y-cy) - t*t >= 0 with t = (r + cr) + 2*spacing for every placed (cx, cy, cr);
 *   accept: append, tries = 0; reject: tries += 1, and tries > 2000: spacing *= 0.5, tries = 0.  Stops at n_cir + n_elp
 *   obstacles or after max_candidates candidates (0 = the default 2^18, also the limit; the field then holds fewer
 *   obstacles and nc / ne say how many).  The two seed circles are dropped.
 *   Mix fields (n_elp > 0; needs n_cir = ceil(tot / 2), n_elp = floor(tot / 2)): obstacle i in placement order is circle
 *   slot i / 2 (i even) or ellipse slot j = (i - 1) / 2 (i odd) with a = r, b = r2((a / 2) U(stream 1, ctr 2j) + a / 2),
 *   phi = r2(floor(181 U(stream 1, ctr 2j + 1)) * (pi / 180)).  Inflation: circle r + 0.4, ellipse a + 0.4, b + 0.4.
 *   Slots past the count are zero.
 *   State (stream 2, id = g): pair i = 0, 1, ...: px = 10 U(ctr 2i), py = 10 U(2i + 1), accepted when
 *   (px-10)*(px-10) + (py-10)*(py-10) > 0.25 and dx*dx + dy*dy >= R*R for every inflated obstacle (R = r + 0.2 for a
 *   circle, max(a, b) + 0.2 for an ellipse); after 1024 rejected pairs the last one is used.  leg = U(4096) < 0.5 ? -1
 *   : +1, noise = 0.2 sqrt(-2 log(1 - U(4097))) cos(2 pi U(4098)), vbx = 0.45 + 0.3 U(4099), vby = -leg (0.17 + 0.16
 *   U(4100)), th = atan2(10 - py, 10 - px) + noise, x0 = [px, py, cos(th) vbx - sin(th) vby, sin(th) vbx + cos(th) vby,
 *   th], goal = (10, 10), u0 = [x0] * N.  (x0[2:5] pass through the device's log / sqrt / cos / sin / atan2: equal to the
 *   host restatement to a few ulp, not bit for bit; everything else is.)
 * Outputs, shaped as alipmpc_solve_batch's inputs for the handle's N, nc_max, ne_max (any may be NULL; elp / ne are
 * ignored when ne_max == 0): x0 B x 5, goal B x 2, leg B, cir B x nc_max x 3, nc B, elp B x ne_max x 5, ne B, u0 B x 5N.
 * Host pointers with hip_stream == NULL (staged, synchronous); device pointers otherwise: one kernel launch on that
 * stream (one wavefront per instance), no host synchronisation, no device allocation.
 * ALIPMPC_EINVAL: B < 0, n_cir > nc_max, n_elp > ne_max, a broken mix rule, fields < 0, max_candidates outside
 * [0, 2^18], first_index < 0, first_index + B > 2^40.  LIP variants only (DD: ALIPMPC_EUNSUPPORTED).
 */
int alipmpc_scenes_batch(void* handle, int64_t B, uint64_t seed, int64_t first_index,
                         int32_t n_cir, int32_t n_elp, int64_t fields, int32_t max_candidates,
                         double* x0, double* goal, int8_t* leg, double* cir, int32_t* nc,
                         double* elp, int32_t* ne, double* u0, void* hip_stream);

/* Rows per planned step of alipmpc_trace_batch: 1 + len(np.arange(0, dt + 0.01, 0.01)) (42 at dt = 0.4);
 * 0 for the DD variant. */
int32_t alipmpc_trace_len(const alipmpc_cfg* cfg);

/*
 * Dense CoM traces of plans — the pos_det output of MPCCBF.gen_control_test (MPC_LIP_modi.py:117-122) built
 * by MPCCBF.xk_track_det (MPC_LIP_modi.py:304-322), i.e. the 126 x 2 rows per plan of the reference's
 * data_log *_pred_full_end.pkl at N = 3 (main_sim_mpc.py:117, logger_mpc.py:473).  For each instance and
 * step k = 0..N-1: row 0 = x_k[0:2], then the ALIP flow from x_k around the stance foot p_k at t = 0, 0.01,
 * ..., with x_{k+1} = M_A x_k + M_B u_k and p_k = W(u_k - A x_k) as gen_control_test forms them.
 *   x0 B x 5, u B x 5N (a solve's u_out)  ->  trace B x N x alipmpc_trace_len(cfg) x 2.
 * LIP variants only (DD: ALIPMPC_EUNSUPPORTED).  Host / device pointers as alipmpc_solve_batch.
 */
int alipmpc_trace_batch(void* handle, int64_t B, const double* x0, const double* u, double* trace,
                        void* hip_stream);

/*
 * Plan audit: per instance, how far the plan u violates its constraints and how close its dense CoM trace comes to
 * the obstacles; per call, integer counts of both.  One kernel launch (one instance per 16 lanes), nothing but the
 * outputs below is written.  No reference counterpart: the reference inspects traces by plotting (plot_data_cir.py)
 * and its driver keeps only feasi != 2 (main_sim_mpc.py:118).
 *   Inputs as alipmpc_solve_batch; u B x 5N is the plan to audit (a solve's u_out); status B (may be NULL) the
 *   solve's status, used by the summary's cross table only.
 *   metrics B x ALIPMPC_AUDIT_COLS (may be NULL):
 *     0 viol        max over the active rows of max(cl - c, c - cu, 0) with c, cl, cu, row_active exactly those
 *                   alipmpc_eval_batch returns at u (the reference's rows, f_en included; select_obs and the detour as
 *                   configured); 0 when no row is violated.
 *     1 clear       min over all N x alipmpc_trace_len rows of the plan's dense trace (alipmpc_trace_batch's rows) and
 *                   over all valid obstacles — the nc[b] circles and ne[b] ellipses as passed (inflated as passed,
 *                   NOT filtered by select_obs) — of the radial clearance; +inf without a valid obstacle.
 *     2 clear_knot  the same minimum over the N + 1 knots only: knot k < N is row 0 of step k (x_k), knot N the last
 *                   row of step N - 1 (x_N).
 *     3 goal_1      | knot 1 - goal |  (the goal as passed, not the detour goal)
 *     4 goal_N      | knot N - goal |
 *   Radial clearance of a point p to an obstacle (cx, cy, a, b, phi) — a circle is a = b = r, phi = 0; the semi-axis
 *   a = elp[2] lies along phi, the reference's h_elp convention: d = p - c, Q = ((dx cos phi + dy sin phi) / a)^2 +
 *   ((-dx sin phi + dy cos phi) / b)^2, clearance = |d| (1 - 1 / sqrt(Q)), and -min(a, b) at |d| = 0: the signed
 *   distance to the boundary along the ray from the centre (for a circle |d| - r), negative inside.
 *   where B x ALIPMPC_AUDIT_WHERE int32 (may be NULL):
 *     0 viol_row    padded row index of viol (the smallest among equal violations), -1 when viol == 0
 *     1 clear_row   flat trace row k * alipmpc_trace_len + r of clear
 *     2 clear_obs   obstacle slot of clear: circle j is j, ellipse j is nc_max + j; -1 (with clear_row = -1): no obstacle
 *     Among exactly equal clearances the smallest (row, obs) in row-major order wins (rows 0 and 1 of a step are
 *     the same point).
 *   Non-finite input: if any of x0[b], goal[b], u[b] is not finite (a rollout's plans after the goal are NaN), the
 *   five metrics are NaN, where is -1 and only summary[0], [1] count the instance.
 *   summary alipmpc_audit_summary_len(n_edges) = 6 + (n_edges + 1) + 20 int64 words (may be NULL), ADDED to what the
 *   buffer holds, so one buffer carried through the chunks of a sweep ends as the whole sweep's (integer counts:
 *   independent of chunking and of execution order):
 *     [0] instances  [1] non-finite  [2] viol <= viol_tol  [3] clear >= 0  [4] both  [5] clear < 0 <= clear_knot (an
 *     incursion between touchdowns only); [6 + i], i = 0..n_edges: clearance histogram, bin i counts edges[i - 1] <=
 *     clear < edges[i] (first bin open below, last open above, +inf in the last); then, only when status != NULL
 *     (else left untouched), 20 words indexed cls * 4 + 2 (clear >= 0) + (viol <= viol_tol) with cls = 0, 1, 2, 3, 4
 *     for status 0, 1, -1, 2, other.
 *   edges: n_edges finite, strictly increasing values, ALWAYS a host pointer (copied into the launch).
 * Host / device pointers as alipmpc_solve_batch (edges excepted).  Device pointers: asynchronous on the stream, one
 * launch, no device allocation, no host synchronisation.  Host pointers: summary is staged in, added to, staged out.
 * Every LIP handle, whatever its precision and program (the audit arithmetic is always fp64); DD:
 * ALIPMPC_EUNSUPPORTED.  ALIPMPC_EINVAL: B < 0, n_edges outside [0, ALIPMPC_AUDIT_MAX_EDGES], edges not finite or not
 * strictly increasing, viol_tol negative or not finite, u == NULL, metrics, where and summary all NULL.
 */
#define ALIPMPC_AUDIT_COLS 5
#define ALIPMPC_AUDIT_WHERE 3
#define ALIPMPC_AUDIT_MAX_EDGES 62
int32_t alipmpc_audit_summary_len(int32_t n_edges);   /* ALIPMPC_EINVAL for n_edges outside [0, 62] */
int alipmpc_audit_batch(void* handle, int64_t B,
                        const double* x0, const double* goal, const int8_t* leg,
                        const double* cir, const int32_t* nc, const double* elp, const int32_t* ne,
                        const double* u, const int32_t* status,
                        double* metrics, int32_t* where, double viol_tol,
                        const double* edges, int32_t n_edges, int64_t* summary,
                        void* hip_stream);

/* Instances this handle's solve kernel holds resident on its device at once (solve_kernel: resident
 * workgroups x 4 waves, one instance per wave; lane_kernel: resident waves x instances per wave).  A wave-program
 * batch that fits these slots launches one wave per instance (as a split launch, see alipmpc_solve_launches); a
 * larger one — and every lane-program batch — runs as a persistent grid of the resident workgroups whose waves
 * (lanes) pull instances from a per-launch work queue.  Every form runs the same per-instance arithmetic, so an
 * instance's result does not depend on B (a batch solved whole or in chunks is bit-identical).  0 for the DD
 * variant (always one wave per instance).  No reference counterpart (scheduling of the batched replacement). */
int alipmpc_solve_slots(void* handle, int64_t* slots);

/* Kernel launches one alipmpc_solve_batch of B instances runs on this handle: 2 for a split launch (wave program,
 * 2 <= B <= alipmpc_solve_slots, and ALIPMPC_SPLIT_IT > 0 — phase 1 up to that many iterations, phase 2 resumes the
 * unfinished instances from their exact loop-state records — or, fp64, ALIPMPC_SPLIT_TR > 0), 1 otherwise; *team = the
 * team size (4 waves) when phase 1 also cuts instances by their line-search trial count (ALIPMPC_SPLIT_TR > 0, fp64
 * only) into team records that phase 2 runs on a team each, else 1.
 * fp64 with cfg.restoration = ALIPMPC_RESTORATION_IPOPT, no team records, one row group per lane and 8 workspaces within
 * the LDS (cfg2's shape): phase 2 is the PAIRED form, still one launch — phase 1 lists its records in two classes (cut
 * with a restoration pending / cut at the iteration cap), and phase 2 runs 8-wave workgroups, two waves per SIMD, whose
 * owner waves 0-3 resume the pending-restoration records at top priority and whose filler waves 4-7 resume regular
 * ones, so no SIMD holds two restoration tails while another holds none.  ALIPMPC_SPLIT_PAIR=0 selects the 4-wave
 * phase 2 with the records in cut order (same bits either way).  The closed loop's per-tick solves keep the 4-wave form.
 * It reports the form of an eager launch on a stream that holds, or can still get, a record buffer: a launch
 * captured into a graph on a stream without one, or on a ninth stream, runs the one-phase form (1 launch).
 * Profiling tools use it to turn per-dispatch figures into per-solve ones.  No reference counterpart. */
int alipmpc_solve_launches(void* handle, int64_t B, int32_t* launches, int32_t* team);

/* Lane program (either precision) or fp32 wave program with cfg.restoration = ALIPMPC_RESTORATION_IPOPT: the instances
 * of the last solve on this stream whose line search failed in that program and which were therefore solved, from
 * their start, by the fp64 wave program's restoration-capable work queue (IPOPT's restoration phase: DESIGN.md §2
 * item 4).  Synchronises the stream.  0 for other programs / restoration modes.  The count is read from the stream's
 * current list: a graph captured before the list grew (Conventions) counts into the list it captured, so after its
 * replay this call still reports the last solve issued through the library.  No reference counterpart. */
int alipmpc_lane_handoffs(void* handle, void* hip_stream, int64_t* count);

/* The device program this handle's solves run (cfg.program): "solve_kernel<N,rows/4,type>" (one instance per
 * wavefront; launched as one wave per instance when the batch fits alipmpc_solve_slots, as the persistent
 * work queue otherwise — the same bits per instance either way), "lane_kernel<N,circle slots,modi,type>" (one
 * instance per lane, circles only: the compiled slot count 0, 5 or 6 serving cfg.nc_max),
 * "lane_kernel<3,5,true,Form<type>>" (one instance per lane, the obstacle-form build: 5 form slots serving every
 * cfg.nc_max + cfg.ne_max <= 5 with cfg.ne_max >= 1, modi; a profiler prints that kernel as
 * lane_kernel<3, 5, true, alip::lane::Form<type>>) or "dd_solve_kernel<N,row groups>".  No reference counterpart.  The
 * string is owned by the library. */
const char* alipmpc_solve_program(void* handle);

/* Duration in milliseconds of the most recent solve kernel launch on this handle, measured with HIP
 * events on the launch stream (0 if none). */
double alipmpc_last_kernel_ms(void* handle);

/* Identifier of this library build: 16 hex digits of a sha256 over the sources and compile flags it was built from
 * (alipmpc/build.py).  Profiles and counter records carry it, so tools never attach one build's counters to another
 * build's measurement.  No reference counterpart. */
const char* alipmpc_build_id(void);

const char* alipmpc_last_error(void* handle);
void alipmpc_destroy(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* ALIPMPC_H */
