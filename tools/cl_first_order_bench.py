"""Dev measurement of the first-order ticks of the scheduled closed loop (cfg.cl_between = 1; DESIGN §3.8,
profiles/first_order) on bench.py's cfg2 episodes: S = 8 walking steps of f_cyc = 20 ticks.

  python tools/cl_first_order_bench.py time      loop times, device pointers, B = 4096 (AB_B): mask {15} on a mode-0
        handle (a), the same mask on a mode-1 handle (b), mask {0} on the mode-1 handle (c) and every tick solving (d);
        AB_ROUNDS (4) rounds of one process per mode, alternating, AB_REPS (5) timed loops per mask after a warm-up
        pass.
  python tools/cl_first_order_bench.py error     accuracy, host pointers, B = 512 (AB_EB), mask {0} on the mode-1
        handle, for the kicks 0.01 / 0.02 / 0.05 / 0.1: at every first-order tick a re-solve on the device at the replayed
        x_nex, warm-started from the anchor plan (max_iter 100); over the ticks where anchor and re-solve end with status
        0, per tick index the medians of e1 = |u_fo - u_re|_inf and e0 = |u_anchor - u_re|_inf.
Each ends with one JSON summary line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, F = 8, 20
KICKS = (0.01, 0.02, 0.05, 0.1)


def setup(B):
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    sys.path.insert(0, ROOT)
    import alipmpc
    import bench
    bt = bench.global_inputs("cfg2", 0, B, B, 0, 5, 0, 3)
    mk = lambda **kw: alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0, **kw))   # noqa: E731
    return alipmpc, bt, mk


def time_one(mode):
    """One process, one handle (a second handle's streams would share the hardware queues with the first's episode
    groups): mode 0 times mask {15} (a) and every tick (d), mode 1 mask {15} (b) and mask {0} (c)."""
    import torch
    B, reps = int(os.environ.get("AB_B", "4096")), int(os.environ.get("AB_REPS", "5"))
    alipmpc, bt, mk = setup(B)
    s = mk(cl_between=mode)
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
    inp["leg"], inp["nc"] = inp["leg"].to(torch.int8), inp["nc"].to(torch.int32)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    sol = {"u": torch.empty((B, 15), **f64), "foot": torch.empty((B, 3), **f64)}
    s.solve_device(inp, sol)
    inp["foot0"] = sol["foot"][:, 0:2].contiguous()
    out = dict(foot=torch.zeros((B, S, 3), **f64), x=torch.zeros((B, S + 1, 5), **f64), hd=torch.zeros((B, S, 2), **f64),
               status=torch.zeros((B, S, F), **i32), iters=torch.zeros((B, S, F), **i32),
               steps_to_goal=torch.zeros(B, **i32), action=torch.zeros((B, S, F, 8), **f64))
    kw = dict(f_cyc=F, kick=0.05, seed=7)
    runs = ({"b_tick15_mode1": 1 << 15, "c_tick0_mode1": 1} if mode else
            {"a_tick15_mode0": 1 << 15, "d_every_tick": (1 << F) - 1})
    ms, share = {k: [] for k in runs}, {}
    for _ in range(reps + 1):   # (the first pass warms up)
        for k, mask in runs.items():
            s.closed_loop_schedule_device(inp, out, S, mpc_ticks=mask, **kw)
            ms[k].append(s.last_kernel_ms())
            st = out["status"].cpu().numpy()
            share[k] = round(float((st == -21).sum() / max(1, ((st == -21) | (st == -20)).sum())), 4)
    print(json.dumps({"build_id": alipmpc.build_id(), "B": B, "loop_ms": {k: [round(m, 4) for m in v[1:]] for k, v in ms.items()},
                      "first_order_share_of_non_solve_ticks": share}), flush=True)


def time_loops():
    """Rounds of one process per mode, alternating; medians of the processes' medians and their max - min."""
    import subprocess
    rounds = int(os.environ.get("AB_ROUNDS", "4"))
    recs = []
    for _ in range(rounds):
        for mode in ("0", "1"):
            r = subprocess.run([sys.executable, __file__, "one", mode], timeout=200, capture_output=True, text=True)
            if r.returncode != 0:   # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode)
            recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(recs[-1]), flush=True)
    summ = {"tool": "cl_first_order_bench time", "build_id": recs[0]["build_id"], "B": recs[0]["B"], "S": S, "f_cyc": F,
            "kick": 0.05, "rounds": rounds}
    for k in ("a_tick15_mode0", "b_tick15_mode1", "c_tick0_mode1", "d_every_tick"):
        v = np.array([np.median(r["loop_ms"][k]) for r in recs if k in r["loop_ms"]])
        sh = [r["first_order_share_of_non_solve_ticks"][k] for r in recs if k in r["loop_ms"]][0]
        summ[k] = {"run_medians_ms": v.round(4).tolist(), "median_ms": round(float(np.median(v)), 4),
                   "spread_ms": round(float(v.max() - v.min()), 4), "first_order_share_of_non_solve_ticks": sh}
    print(json.dumps(summ), flush=True)


def errors():
    B = int(os.environ.get("AB_EB", "512"))
    alipmpc, bt, mk = setup(B)
    from alipmpc import schedule
    s1, sre = mk(cl_between=1), mk(max_iter=100)
    x0, goal, leg = bt["x0"], bt["goal"], bt["leg"].astype(np.int8)
    cir, nc = bt["cir"], bt["nc"].astype(np.int32)
    foot0 = s1.solve(x0, goal, leg, cir, nc, u0=bt["u0"])["foot"][:, 0:2].copy()
    e = dict(x0=x0, foot0=foot0, goal=goal, leg=leg, cir=cir, nc=nc)
    rec = {"tool": "cl_first_order_bench error", "build_id": alipmpc.build_id(), "B": B, "S": S, "f_cyc": F,
           "mask": [0], "by_kick": {}}
    for kick in KICKS:
        o = s1.closed_loop_schedule(x0, foot0, goal, leg, cir, nc, steps=S, f_cyc=F, mpc_ticks=(0,), kick=kick, seed=7,
                                    want_plans=True)

        def sens(xn, od, u0, idx):
            r = s1.solve_sens(xn, goal[idx], od, cir[idx], nc[idx], u0=u0)
            return r["du"], r["sens_ok"]
        rp = schedule.replay(s1.cfg, e, [0], o["x"], o["plan"], o["status"], kick=kick, seed=7, sens=sens,
                             foot_traj=o["foot"], hd_traj=o["hd"])
        fo = rp["fo"]
        b, st, i = fo["b"], fo["s"], fo["i"]
        ua, ufo = o["plan"][b, st, 0], o["plan"][b, st, i]
        od = (-leg[b] * (-1) ** st).astype(np.int8)     # od_ev = -leg_ind of step st
        re = sre.solve(fo["x_nex"], goal[b], od, cir[b], nc[b], u0=ua)
        keep = (o["status"][b, st, 0] == 0) & (re["status"] == 0)
        e1 = np.abs(ufo - re["u"]).max(-1)
        e0 = np.abs(ua - re["u"]).max(-1)
        by_tick = {int(t): [float(np.median(e1[keep & (i == t)])), float(np.median(e0[keep & (i == t)]))]
                   for t in range(1, F) if (keep & (i == t)).any()}
        rec["by_kick"][str(kick)] = {
            "first_order_ticks": int(len(b)), "kept": int(keep.sum()),
            "median_e1": float(np.median(e1[keep])), "median_e0": float(np.median(e0[keep])),
            "ratio": float(np.median(e1[keep]) / np.median(e0[keep])),
            "p90_e1": float(np.quantile(e1[keep], 0.9)), "p90_e0": float(np.quantile(e0[keep], 0.9)),
            "median_e1_e0_by_tick": by_tick}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "one":
        time_one(int(sys.argv[2]))
    else:
        {"time": time_loops, "error": errors}[sys.argv[1]]()
