"""The scheduled closed loop in numpy (alipmpc_closed_loop_schedule_batch, include/alipmpc.h): the hybrid driver of
main_sim_mpc_alip.py:71-130 on an ALIP plant.  Tick i of a step solves the MPC when bit i of the mask is set
(Logger.gen_nex_foot_input) and otherwise takes the foothold that realises the plan's desired touchdown velocity from
the plant's projection (Logger.cal_foot_input, data_procs/logger.py:380-410: cal_foot_with_veldes(x_nex, v_des_map)).

  run     drives the loop with any solver (a callable): the host restatement of the device loop, in either mode of
          cfg.cl_between (nominal, first-order or guarded first-order ticks between the solves)
  replay  recomputes every step of a device loop from the device's own touchdown state x[:, s] and its recorded plans,
          so no drift crosses a step; also returns the solve inputs (x_nex, -leg_ind, u0) of every solved tick

Built from the pieces of alipmpc.tsc (heading tube, command packing) and alipmpc.planner (ALIP matrices); every
expression is written in the operation order of the device kernels (csrc/alipmpc.hip: cl_project_kernel,
cl_update_kernel, cl_nominal_run_kernel, cl_between_run_kernel / cl_first_order_plan, nominal_gait_kernel; the guard of
the guarded mode is csrc/audit.inc's cl_guard_kernel).
"""
import math
from fractions import Fraction

import numpy as np

from . import planner, tsc

TICK_NOMINAL = -20     # ALIPMPC_TICK_NOMINAL
TICK_FIRST_ORDER = -21  # ALIPMPC_TICK_FIRST_ORDER
BETWEEN_NOMINAL, BETWEEN_FIRST_ORDER = 0, 1   # cfg.cl_between
BETWEEN_GUARDED = 3     # ... first-order ticks behind the guard (ALIPMPC_CL_BETWEEN_GUARDED)
GUARD_VIOL = 1e-4       # ALIPMPC_CL_GUARD_VIOL: the guard's bar on a first-order plan's largest violation
ROLLOUT_DONE = -10     # ALIPMPC_ROLLOUT_DONE
VARIANT_MODI, VARIANT_SIG_STEP = 0, 1
MAX_F_CYC = 64

_M64 = (1 << 64) - 1


def mask_of(mpc_ticks, f_cyc=None):
    """The schedule as a 64-bit mask: mpc_ticks is an int mask or an iterable of tick indices.  With f_cyc given,
    ValueError for f_cyc outside 1..64 or a tick at or above f_cyc (the ABI's ALIPMPC_EINVAL cases); without, only
    what 64 bits cannot hold is refused (the library checks the rest)."""
    if isinstance(mpc_ticks, (int, np.integer)):
        m = int(mpc_ticks)
    else:
        m = 0
        for t in mpc_ticks:
            t = int(t)
            if not 0 <= t < MAX_F_CYC:
                raise ValueError(f"tick {t} outside 0..{MAX_F_CYC - 1}")
            m |= 1 << t
    if not 0 <= m <= _M64:
        raise ValueError("mask outside 64 bits")
    if f_cyc is not None:
        F = int(f_cyc)
        if not 1 <= F <= MAX_F_CYC:
            raise ValueError(f"f_cyc {F} outside 1..{MAX_F_CYC}")
        if m >> F:
            raise ValueError(f"mask {m:#x} has a tick at or above f_cyc = {F}")
    return m


def all_ones(f_cyc):
    return (1 << int(f_cyc)) - 1


def cl_uniform(seed, b, s, i, axis):
    """splitmix64 uniform [0, 1) of (episode, step, tick, axis): the plant's velocity kick (cl_uniform of
    csrc/alipmpc.hip, the same integer recipe)."""
    key = ((((b * 1048576 + s) * 1024 + i) * 2 + axis) + 1) & _M64
    z = (seed + 0x9E3779B97F4A7C15 * key) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z = z ^ (z >> 31)
    return (z >> 11) * (1.0 / 9007199254740992.0)


def constants(cfg):
    """The loop's constants of a cfg-like object (N, variant, dt, g, H): ALIP matrices of a whole step
    (planner.alip_constants), alip_des_vel(0.6, .) and cal_foot_with_veldes's B_vel^-1."""
    T = float(cfg.dt)
    k = planner.alip_constants(T, float(cfg.g), float(cfg.H))
    beta = k["beta"]
    sh, ch = math.sinh(beta * T), math.cosh(beta * T)
    return dict(N=int(cfg.N), variant=int(cfg.variant), T=T, beta=beta, A=k["A"], W=k["W"], M_A=k["M_A"],
                M_B=k["M_B"], bsh=sh * beta, ch=ch, ibv=1.0 / (-sh * beta),
                vdx=beta / math.tanh(T * beta / 2) * 0.6 * T / 2, vdy0=(beta * sh) / (ch + 1))


def des_vel(k, leg):
    """alip_des_vel(0.6, leg_ind) per episode (MPC_LIP_modi.py:181-186)."""
    leg = np.asarray(leg, float)
    return np.stack([np.full(leg.shape, k["vdx"]), 0.5 * (-0.5 * leg * 0.3) * k["vdy0"]], -1)


def flow_consts(beta, t):
    """cosh, sinh / beta, beta sinh of the ALIP flow over t."""
    return math.cosh(beta * t), math.sinh(beta * t) / beta, math.sinh(beta * t) * beta


def flow(x, fx, fy, hp, ch, shb, bsh, tt):
    """get_next_states (MPC_LIP_modi.py:149-178): the state x (n, 5) moved around the stance foot (fx, fy) with the
    heading advancing tt * hp."""
    return np.stack([ch * x[:, 0] + shb * x[:, 2] + (1.0 - ch) * fx,
                     ch * x[:, 1] + shb * x[:, 3] + (1.0 - ch) * fy,
                     bsh * x[:, 0] + ch * x[:, 2] - bsh * fx,
                     bsh * x[:, 1] + ch * x[:, 3] - bsh * fy,
                     x[:, 4] + tt * hp], axis=1)


def _fma(a, b, c):
    """a * b + c rounded once, elementwise (exact rational arithmetic): the device's v_fma_f64."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    out = np.empty(a.shape)
    of, af, bf, cf = out.reshape(-1), a.reshape(-1), b.reshape(-1), c.reshape(-1)
    for j in range(of.size):
        of[j] = float(Fraction(float(af[j])) * Fraction(float(bf[j])) + Fraction(float(cf[j])))
    return out


def flow_device(x, fx, fy, hp, ch, shb, bsh, tt, project):
    """flow() with the roundings of the device kernels, which contract cl_flow's expressions into fma's: position
    fma(1 - ch, f, fma(ch, pos, shb vel)) and heading fma(tt, hp, x4) in all; velocity fma(-bsh, f, fma(bsh, pos,
    ch vel)) in cl_project_kernel (project: a solve tick's x_nex) and in the plant moves of cl_update_kernel and
    cl_between_run_kernel (a tick with a plan), and fma(-f, bsh, fma(ch, vel, bsh pos)) in cl_nominal_run_kernel's
    plant move.  (Read off the gfx950 code of the kernels; replay's bit-exact mode.)"""
    omc = 1.0 - ch
    cols = []
    for pos, vel, f in ((x[:, 0], x[:, 2], fx), (x[:, 1], x[:, 3], fy)):
        cols.append(_fma(omc, f, _fma(ch, pos, shb * vel)))
    for pos, vel, f in ((x[:, 0], x[:, 2], fx), (x[:, 1], x[:, 3], fy)):
        cols.append(_fma(-bsh, f, _fma(bsh, pos, ch * vel)) if project else _fma(-f, bsh, _fma(ch, vel, pos * bsh)))
    cols.append(_fma(tt, hp, x[:, 4]))
    return np.stack(cols, axis=1)


def foot_with_veldes(k, xn, vdes):
    """cal_foot_with_veldes (MPC_LIP_modi.py:188-194): B_vel^-1 (v_des - (A x)[2:4])."""
    ax = k["bsh"] * xn[:, 0] + k["ch"] * xn[:, 2]
    ay = k["bsh"] * xn[:, 1] + k["ch"] * xn[:, 3]
    return np.stack([k["ibv"] * (vdes[:, 0] - ax), k["ibv"] * (vdes[:, 1] - ay)], 1)


def plan_outputs(k, xn, u):
    """What gen_control_test derives from a solve's u at x_nex (MPC_LIP_modi.py:102-115): p_list[0] (n, 3) and
    xk_list[1:] (n, N, 5), p_k = W (u_k - A x_k), x_{k+1} = M_A x_k + M_B u_k."""
    N = k["N"]
    u = np.asarray(u, float).reshape(len(xn), N, 5)
    xk = np.asarray(xn, float)
    foot = (u[:, 0] - xk @ k["A"].T) @ k["W"].T
    xp = []
    for j in range(N):
        xk = xk @ k["M_A"].T + u[:, j] @ k["M_B"].T
        xp.append(xk)
    return foot, np.stack(xp, 1)


def first_order_plan(k, xn, xa, ua, du):
    """A first-order tick's plan and what follows from it (cl_first_order_plan of csrc/alipmpc.hip, its operation
    order): u_fo = ua + du[:, :, 0:5] (x_nex - xa) (m, 5N), then p_0 (m, 3) and xk_list[1:] (m, N, 5) as plan_outputs
    states them, every sum from 0.0 in the device's order of terms."""
    N, m = k["N"], len(xn)
    A, W, MA, MB = k["A"], k["W"], k["M_A"], k["M_B"]
    xn = np.asarray(xn, float)
    d = xn - xa
    ua = np.asarray(ua, float).reshape(m, N, 5)
    du = np.asarray(du, float).reshape(m, N, 5, -1)
    u = np.empty((m, N, 5))
    for kk in range(N):
        for c in range(5):
            v = np.zeros(m)
            for j in range(5):
                v = v + du[:, kk, c, j] * d[:, j]
            u[:, kk, c] = ua[:, kk, c] + v
    e = np.empty((m, 5))
    for i in range(5):
        v = np.zeros(m)
        for c in range(5):
            v = v + A[i, c] * xn[:, c]
        e[:, i] = u[:, 0, i] - v
    foot = np.empty((m, 3))
    for i in range(3):
        v = np.zeros(m)
        for c in range(5):
            v = v + W[i, c] * e[:, c]
        foot[:, i] = v
    xk, xp = xn, np.empty((m, N, 5))
    for kk in range(N):
        y = np.empty((m, 5))
        for i in range(5):
            v = np.zeros(m)
            for c in range(5):
                v = v + MA[i, c] * xk[:, c]
            for c in range(5):
                v = v + MB[i, c] * u[:, kk, c]
            y[:, i] = v
        xk = xp[:, kk] = y
    return u.reshape(m, 5 * N), foot, xp


def _rot(th, vx, vy):
    c, s = np.cos(th), np.sin(th)
    return c * vx + s * vy, -s * vx + c * vy


def command(p0, foot, fx, fy, xn, vdes, hd, hp, hcos, i, F):
    """The task-space-controller command of a tick (Logger.gen_nex_foot_input / cal_foot_input + gen_tsc_control):
    foot the next foothold (n, 2) in the map frame, p0 the initial pose (origin and heading of the robot frame)."""
    nsx, nsy = _rot(p0[:, 2], foot[:, 0] - p0[:, 0], foot[:, 1] - p0[:, 1])
    csx, csy = _rot(p0[:, 2], fx - p0[:, 0], fy - p0[:, 1])
    npx, npy = _rot(p0[:, 2], xn[:, 0] - p0[:, 0], xn[:, 1] - p0[:, 1])
    nvx, nvy = _rot(p0[:, 2], vdes[:, 0], vdes[:, 1])
    th = hd - p0[:, 2]
    fi = np.stack(_rot(th, nsx - csx, nsy - csy), -1)
    npf = np.stack(_rot(th, npx - csx, npy - csy), -1)
    nvf = np.stack(_rot(th, nvx, nvy), -1)
    return tsc.gen_tsc_control(fi, npf, nvf, hp, hcos - p0[:, 2], i, F)


def _close(variant, xp, goal):
    """close_2_goal of a plan's predicted states xp (m, N, 5)."""
    d = np.sqrt(((xp[:, :, 0:2] - goal[:, None, :]) ** 2).sum(-1))
    return (d <= 0.35).any(1) if variant == VARIANT_SIG_STEP else d[:, 0] <= 0.15


def _loop(cfg, inp, mask, steps, f_cyc, kick, seed, solve, dev, between=BETWEEN_NOMINAL, sens=None, guard=None):
    k = constants(cfg)
    N, n, variant = k["N"], 5 * k["N"], k["variant"]
    S, F = int(steps), int(f_cyc)
    mask = mask_of(mask, F)
    x = np.array(inp["x0"], np.float64).reshape(-1, 5).copy()
    B = len(x)
    pst = np.array(inp["foot0"], np.float64).reshape(B, 2).copy()
    goal = np.ascontiguousarray(np.broadcast_to(np.asarray(inp["goal"], np.float64), (B, 2)))
    leg = np.array(np.broadcast_to(np.asarray(inp["leg"]), (B,)), np.int8).copy()
    nex_turn, hd_pr, hd_cos = np.zeros(B), np.zeros(B), np.zeros(B)
    mhd = np.repeat(x[:, 4:5], 3, axis=1)      # mpc_hds_list: 0 in the Logger's robot frame = the initial heading
    plan = np.zeros((B, n))
    active = np.ones(B, bool)
    has_plan = np.zeros(B, bool)
    rclose = np.zeros(B, bool)
    beta, T = k["beta"], k["T"]
    dt = T / F
    ch_d, shb_d, bsh_d = flow_consts(beta, dt)
    td = dt / T
    pose0 = np.concatenate([x[:, 0:2], x[:, 4:5]], axis=1).copy()
    vdes = des_vel(k, leg)
    foot = np.full((B, S, 3), np.nan)
    xs = np.zeros((B, S + 1, 5))
    xs[:, 0] = x
    hd = np.zeros((B, S, 2))
    action = np.full((B, S, F, 8), np.nan)
    plans = np.full((B, S, F, n), np.nan)
    target = np.full((B, S, F, 2), np.nan)     # the foothold every tick commands: p_list[0][0:2] or the nominal f
    status = np.full((B, S, F), ROLLOUT_DONE, np.int32)
    iters = np.zeros((B, S, F), np.int32)
    stg = np.full(B, -1, np.int32)
    solves = dict(b=[], s=[], i=[], x_nex=[], leg=[], u0=[])
    # first-order mode: the anchor of every episode (the last solve of the current step: its x_nex, plan, du[:, :, 0:5]
    # and tick), valid where that solve's sens_ok is set and no touchdown came since
    guarded = int(between) == BETWEEN_GUARDED
    fo_mode = int(between) == BETWEEN_FIRST_ORDER or guarded
    exact = dev is not None and dev.get("hd") is not None and dev.get("foot") is not None
    a_x, a_u, a_du = np.zeros((B, 5)), np.zeros((B, n)), np.zeros((B, n, 5))
    a_ok, a_i = np.zeros(B, bool), np.full(B, -1)
    fos = dict(b=[], s=[], i=[], x_nex=[], anchor_i=[])
    anchors = dict(b=[], s=[], i=[], sens_ok=[], du=[])
    trigs = dict(b=[], s=[], i=[], x_nex=[], u0=[])

    def solve_tick(s, i, sel, xn, triggered):
        """The solve tick of the episodes sel (x_nex xn): the whole tick's, or a guarded tick's re-solve.  Returns the
        foothold, the predicted states and close_2_goal."""
        m = len(sel)
        u0 = np.tile(xn, (1, N))
        hp_ = has_plan[sel]
        if variant == VARIANT_SIG_STEP:
            pb = plan[sel].reshape(m, N, 5)
            u0[hp_] = np.concatenate([pb[:, 1:], pb[:, -1:]], axis=1).reshape(m, n)[hp_]
        else:
            u0[hp_] = plan[sel][hp_]
        od = (-leg[sel]).astype(np.int8)
        if dev is not None:
            u = np.asarray(dev["plan"])[sel, s, i]
            ft, xp = plan_outputs(k, xn, u)
            o = dict(u=u, foot=ft, x_pred=xp, status=np.asarray(dev["status"])[sel, s, i], iters=np.zeros(m, np.int32))
            if triggered:
                for key, v in (("b", sel), ("s", np.full(m, s)), ("i", np.full(m, i)), ("x_nex", xn), ("u0", u0)):
                    trigs[key].append(v)
            else:
                for key, v in (("b", sel), ("s", np.full(m, s)), ("i", np.full(m, i)), ("x_nex", xn), ("leg", od),
                               ("u0", u0)):
                    solves[key].append(v)
        else:
            o = solve(xn, od, u0, sel)
        if fo_mode:   # a later tick of the step does not solve: this solve leaves the anchor
            if (all_ones(F) & ~mask) >> (i + 1):
                du_, ok_ = sens(xn, od, u0, sel) if dev is not None else (o["du"], o["sens_ok"])
                ok_ = np.asarray(ok_).reshape(m) != 0
                du_ = np.asarray(du_, np.float64).reshape(m, n, -1)
                a_ok[sel] = ok_
                j = sel[ok_]
                a_x[j], a_u[j], a_du[j], a_i[j] = xn[ok_], np.asarray(o["u"])[ok_], du_[ok_][:, :, 0:5], i
                for key, v in (("b", sel), ("s", np.full(m, s)), ("i", np.full(m, i)), ("sens_ok", ok_), ("du", du_)):
                    anchors[key].append(v)
            else:
                a_ok[sel] = False
        status[sel, s, i] = o["status"]
        iters[sel, s, i] = o["iters"]
        plan[sel] = o["u"]
        plans[sel, s, i] = o["u"]
        has_plan[sel] = True
        nex_turn[sel] = o["foot"][:, 2]
        xp = np.asarray(o["x_pred"]).reshape(m, N, 5)
        mhd[sel, :min(3, N)] = xp[:, :3, 4]
        return np.asarray(o["foot"])[:, 0:2], xp, _close(variant, xp, goal[sel])

    for s in range(S):
        if dev is not None:   # replay: every step from the device's own touchdown state and its set of episodes
            x = np.array(dev["x"][:, s], np.float64)
            active = np.asarray(dev["status"])[:, s, 0] != ROLLOUT_DONE
            if exact and s > 0:   # and from its own stance foot
                pst[active] = dev["foot"][active, s - 1, 0:2]
        for i in range(F):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                continue
            rest = T - i * (T / F)
            ch_r, shb_r, bsh_r = flow_consts(beta, rest)
            tr = rest * (1.0 / T)
            if i == 0:   # set_stf_head (data_procs/logger.py:266-288) with the plant heading
                cur = x[idx, 4]
                hd_cos[idx] = cur
                nex_turn[idx] = tsc.tube_step(nex_turn[idx], cur)
                ssum = nex_turn[idx]
                prev = [cur, mhd[idx, 0], mhd[idx, 1]]
                for j in range(3):
                    ssum = ssum + tsc.angle_a_minus_b(mhd[idx, j], prev[j])
                hd_pr[idx] = ssum / 4.0
                if exact:   # the device's own heading inputs
                    hd_pr[idx], hd_cos[idx] = dev["hd"][idx, s, 0], dev["hd"][idx, s, 1]
                hd[idx, s, 0], hd[idx, s, 1] = hd_pr[idx], hd_cos[idx]
            xi, fx, fy, hp = x[idx], pst[idx, 0], pst[idx, 1], hd_pr[idx]
            solved = bool(mask >> i & 1)
            xn = (flow_device(xi, fx, fy, hp, ch_r, shb_r, bsh_r, tr, True) if exact and solved else
                  flow(xi, fx, fy, hp, ch_r, shb_r, bsh_r, tr))
            # upd: the episodes whose tick has a plan (solved, first-order or re-solved), xp / close: what follows from it
            upd = np.zeros(len(idx), bool)
            xp = np.full((len(idx), N, 5), np.nan)
            close = np.zeros(len(idx), bool)
            fo = np.zeros(len(idx), bool)
            if solved:
                nfoot, xp, close = solve_tick(s, i, idx, xn, False)
                upd[:] = True
            else:
                nfoot = foot_with_veldes(k, xn, vdes[idx])
                status[idx, s, i] = TICK_NOMINAL
                iters[idx, s, i] = 0
                # first-order ticks: the episodes with a valid anchor (replay: the ticks the device ran as such)
                trig = np.zeros(len(idx), bool)
                if fo_mode:
                    st_dev = np.asarray(dev["status"])[idx, s, i] if dev is not None else None
                    fo = st_dev == TICK_FIRST_ORDER if dev is not None else a_ok[idx].copy()
                    if guarded and dev is not None:   # the device recorded a solve on a tick outside the mask
                        trig = ~np.isin(st_dev, (ROLLOUT_DONE, TICK_NOMINAL, TICK_FIRST_ORDER))
                u_fo = None
                if fo.any():
                    j = idx[fo]
                    u_fo, ft, xpf = first_order_plan(k, xn[fo], a_x[j], a_u[j], a_du[j])
                    if guarded and dev is None:   # the guard: the rows at this x_nex, obstacles selected there
                        v = np.asarray(guard["viol"](xn[fo], (-leg[j]).astype(np.int8), u_fo, j), float).reshape(len(j))
                        fired = ~(v <= guard["tol"])
                        trig[np.nonzero(fo)[0][fired]] = True
                        keep = ~fired
                        fo[trig] = False
                        j, u_fo, ft, xpf = j[keep], u_fo[keep], ft[keep], xpf[keep]
                if fo.any():   # a solve tick whose outputs follow from u_fo
                    status[j, s, i] = TICK_FIRST_ORDER
                    # (bit-exact replay: the next solve's warm start is the device's row, the replay's own is returned)
                    plan[j] = np.asarray(dev["plan"])[j, s, i] if exact else u_fo
                    plans[j, s, i] = u_fo
                    nex_turn[j] = ft[:, 2]
                    mhd[j, :min(3, N)] = xpf[:, :3, 4]
                    xp[fo], close[fo], upd[fo] = xpf, _close(variant, xpf, goal[j]), True
                    nfoot[fo] = ft[:, 0:2]
                    for key, v in (("b", j), ("s", np.full(len(j), s)), ("i", np.full(len(j), i)), ("x_nex", xn[fo]),
                                   ("anchor_i", a_i[j])):
                        fos[key].append(v)
                if trig.any():   # guarded mode: the fired episodes' solve tick (the projection of a solve tick)
                    if exact:
                        xn[trig] = flow_device(xi[trig], fx[trig], fy[trig], hp[trig], ch_r, shb_r, bsh_r, tr, True)
                    nfoot[trig], xp[trig], close[trig] = solve_tick(s, i, idx[trig], xn[trig], True)
                    upd[trig] = True
            target[idx, s, i] = nfoot
            action[idx, s, i] = command(pose0[idx], nfoot, fx, fy, xn, vdes[idx], xi[:, 4], hp, hd_cos[idx], i, F)
            if upd.any():   # vel_des <- mpc_state_tar[0][2:4] after a solve, [1][2:4] at touchdown
                kv = 1 if (i == F - 1 and N > 1) else 0
                vdes[idx[upd]] = xp[upd][:, kv, 2:4]
            if exact:   # the plant move to the bit: cl_nominal_run_kernel's form, or the tick kernels' after a plan
                xa = np.empty_like(xi)
                for sel, form in ((upd, True), (~upd, False)):
                    if sel.any():
                        xa[sel] = flow_device(xi[sel], fx[sel], fy[sel], hp[sel], ch_d, shb_d, bsh_d, td, form)
            else:
                xa = flow(xi, fx, fy, hp, ch_d, shb_d, bsh_d, td)
            if kick > 0:
                for ax in (0, 1):
                    kv_ = np.array([2.0 * cl_uniform(seed, int(b), s, i, ax) - 1.0 for b in idx])
                    xa[:, 2 + ax] = _fma(kick, kv_, xa[:, 2 + ax]) if exact else xa[:, 2 + ax] + kick * kv_
            x[idx] = xa
            if i == F - 1:   # touchdown
                pst[idx] = nfoot
                leg[idx] = -leg[idx]
                foot[idx, s, 0:2] = nfoot
                foot[idx, s, 2] = nex_turn[idx]
                if not solved:
                    pl = plan[idx].reshape(len(idx), N, 5)[:, 1 if N > 1 else 0, 2:4]
                    nominal = np.where(has_plan[idx, None], pl, des_vel(k, leg[idx]))
                    vdes[idx] = np.where(upd[:, None], vdes[idx], nominal)   # (a tick with a plan took its own)
                stop = idx[rclose[idx]]
                active[stop] = False
                stg[stop] = s + 1
                a_ok[idx] = False   # the linearisation does not carry over a touchdown
            rclose[idx[upd]] |= close[upd]
        xs[:, s + 1] = x
    out = dict(foot=foot, x=xs, hd=hd, status=status, iters=iters, steps_to_goal=stg, action=action, plan=plans,
               target=target)
    if dev is not None:
        cat = lambda v, shape: np.concatenate(v) if v else np.zeros(shape)   # noqa: E731
        out["solves"] = dict(b=cat(solves["b"], (0,)).astype(np.int64), s=cat(solves["s"], (0,)).astype(np.int64),
                             i=cat(solves["i"], (0,)).astype(np.int64), x_nex=cat(solves["x_nex"], (0, 5)),
                             leg=cat(solves["leg"], (0,)).astype(np.int8), u0=cat(solves["u0"], (0, n)))
        if fo_mode:
            ci = lambda v: cat(v, (0,)).astype(np.int64)   # noqa: E731
            out["fo"] = dict(b=ci(fos["b"]), s=ci(fos["s"]), i=ci(fos["i"]), x_nex=cat(fos["x_nex"], (0, 5)),
                             anchor_i=ci(fos["anchor_i"]))
            out["anchors"] = dict(b=ci(anchors["b"]), s=ci(anchors["s"]), i=ci(anchors["i"]),
                                  sens_ok=cat(anchors["sens_ok"], (0,)).astype(bool),
                                  du=cat(anchors["du"], (0, n, 7)))
        if guarded:
            out["triggered"] = dict(b=ci(trigs["b"]), s=ci(trigs["s"]), i=ci(trigs["i"]),
                                    x_nex=cat(trigs["x_nex"], (0, 5)), u0=cat(trigs["u0"], (0, n)))
    return out


def _between(cfg, between):
    b = int(getattr(cfg, "cl_between", BETWEEN_NOMINAL) if between is None else between)
    if b not in (BETWEEN_NOMINAL, BETWEEN_FIRST_ORDER, BETWEEN_GUARDED):
        raise ValueError(f"between = {b}")
    return b


def run(cfg, inputs, mask, solve=None, steps=8, f_cyc=20, kick=0.0, seed=0, between=None, guard_tol=GUARD_VIOL,
        viol=None):
    """The scheduled loop on the host.  cfg: an object with N, variant, dt, g, H (a Cfg); inputs: dict with x0 (B, 5),
    foot0 (B, 2), goal, leg; mask: int mask or iterable of solved ticks; solve(x_nex (n, 5), od_ev (n,), u0 (n, 5N),
    idx (n,) the episodes) -> dict(u, foot, x_pred, status, iters) — not needed for mask 0.  between: what a tick
    without a solve does, BETWEEN_NOMINAL or BETWEEN_FIRST_ORDER (None: cfg.cl_between, 0 where cfg has none); in
    first-order mode solve's dict also carries du (n, 5N, 7) and sens_ok (n,) (Solver.solve_sens's), and a tick with a
    valid anchor moves the anchor's plan by du[:, :, 0:5] (x_nex - x_nex of the anchor) (status TICK_FIRST_ORDER).
    BETWEEN_GUARDED: the first-order mode with the guard — viol(x_nex (m, 5), od_ev (m,), u (m, 5N), idx (m,)) -> (m,)
    is the largest constraint violation of the moved plan at the tick's x_nex (Solver.audit's column 0; audit.
    audit_reference's on the host); where not viol <= guard_tol (a NaN fires) the episode solves on that tick instead,
    warm-started from its current plan, and the solve leaves the new anchor (or none, as a scheduled solve would).
    Returns the dict of Solver.closed_loop_schedule (plan included, NaN rows on nominal ticks and after the stop) plus
    target (B, S, f_cyc, 2): the foothold every tick commands."""
    if solve is None and mask_of(mask, f_cyc):
        raise ValueError("a schedule with solved ticks needs a solve callable")
    between = _between(cfg, between)
    guard = None
    if between == BETWEEN_GUARDED:
        if viol is None:
            raise ValueError("between = BETWEEN_GUARDED needs a viol callable")
        guard = dict(tol=float(guard_tol), viol=viol)
    return _loop(cfg, inputs, mask, steps, f_cyc, float(kick), int(seed), solve, None, between, guard=guard)


def replay(cfg, inputs, mask, x_traj, plan_traj, status_traj, kick=0.0, seed=0, sens=None, foot_traj=None,
           hd_traj=None, guarded=False):
    """Every step of a device loop recomputed from the device's own touchdown state x_traj[:, s], the episodes it
    still ran (status_traj[:, s, 0]) and the plans it recorded (plan_traj), a solve's foothold and predicted states
    derived from its plan as gen_control_test does (plan_outputs).  Returns foot, hd, x (x[:, s + 1] from
    x_traj[:, s]), action — the values to hold against the device's — and solves: dict(b, s, i, x_nex, leg, u0), the
    inputs of every solved tick.  (iters is not replayed; steps_to_goal follows from status.)
    A first-order loop (a handle with cfg.cl_between = 1) is replayed when sens is given: sens(x_nex, od_ev, u0, idx)
    -> (du (n, 5N, 7), sens_ok (n,)) is called at every replayed solve tick that leaves an anchor; the ticks the device
    recorded as TICK_FIRST_ORDER are recomputed from the anchor (their plan rows are the replay's own, not the
    device's), and the result also holds fo: dict(b, s, i, x_nex, anchor_i), the first-order ticks, and anchors:
    dict(b, s, i, sens_ok, du), the solves that left (or failed to leave) an anchor.
    Bit-exact solve inputs: with the device's foot_traj and hd_traj also given, every step restarts from the device's
    stance foot and heading inputs as well, the plant moves of the nominal ticks and the projection of a solve tick
    round as the device kernels do (flow_device), and the warm start after a first-order tick is the device's recorded
    row — so that up to a step's first solve x_nex and u0 are the device's own bits, and a solve of them on the same
    handle is the device's solve.  The plant moves after a solve or first-order tick round as cl_update_kernel's and
    cl_between_run_kernel's do, so a later solve of the step — a guarded loop's re-solve — has the device's inputs too.
    (The other outputs are compared within a tolerance either way.)
    guarded (with sens; a handle with cfg.cl_between = 3): a tick outside the mask on which the device recorded a solve
    status is replayed as that episode's solve tick — x_nex by the projection's roundings, warm start from the plan as
    it stands, the recorded plan row as its u, the new anchor from sens — and the result also holds triggered: dict(b,
    s, i, x_nex, u0), those ticks with their solve inputs.  anchors then lists the re-solves' anchors too (their i is
    outside the mask)."""
    st = np.asarray(status_traj)
    B, S, F = st.shape
    dev = dict(x=np.asarray(x_traj, np.float64), plan=np.asarray(plan_traj, np.float64).reshape(B, S, F, -1), status=st,
               foot=None if foot_traj is None else np.asarray(foot_traj, np.float64),
               hd=None if hd_traj is None else np.asarray(hd_traj, np.float64))
    if guarded and sens is None:
        raise ValueError("a guarded replay needs sens")
    return _loop(cfg, inputs, mask, S, F, float(kick), int(seed), None, dev,
                 BETWEEN_NOMINAL if sens is None else BETWEEN_GUARDED if guarded else BETWEEN_FIRST_ORDER, sens)
