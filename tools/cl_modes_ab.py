"""Dev A/B of the closed loop's host driver (csrc/closed_loop_host.inc) against a parent build, in every cl_between
mode, on bench.py's cfg2 episodes with device pointers (tools/cl_schedule_bench.py's set-up; profiles/closed_loop_host):
rounds of one process per (mode, build), parent and this build alternating.  Mode 0 runs the plain loop, the dataset
call and the masks {15} (with and without plan_traj, fused and ALIPMPC_CL_FUSE=0), {0}, {0, 19}, all ones and 0;
modes 1 and 3 the masks {15}, {0} and {0, 19}.  Per case an md5 of every output (plans and rows included) and the loop
time; the summary has both builds' medians of the runs' medians, their max - min, and whether the digests are equal
(exit status 1 if any differs).

  python tools/cl_modes_ab.py run PARENT.so     AB_B (4096) AB_S (8) AB_ROUNDS (3) AB_REPS (3) AB_MODES (0,1,3)
  python tools/cl_modes_ab.py one MODE          the library ALIPMPC_LIB names (default: the tree's)
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 20
MODES = tuple(os.environ.get("AB_MODES", "0,1,3").split(","))
KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")


def one(mode):
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import alipmpc
    import bench
    B, S = int(os.environ.get("AB_B", "4096")), int(os.environ.get("AB_S", "8"))
    reps = int(os.environ.get("AB_REPS", "3"))
    bt = bench.global_inputs("cfg2", 0, B, B, 0, 5, 0, 3)
    s = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0, cl_between=mode))
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
    plan = torch.zeros((B, S, F, 15), **f64)
    R = B * S * F
    rows = dict(X=torch.zeros((R, 26), **f64), y_mpc=torch.zeros((R, 8), **f64), y_act=torch.zeros((R, 8), **f64),
                row_status=torch.zeros(R, **i32), row_start=torch.zeros(B + 1, dtype=torch.int64, device=dev))
    kw = dict(f_cyc=F, kick=0.05, seed=7)

    def sched(mask, fuse="1", want_plan=True):
        def go():
            os.environ["ALIPMPC_CL_FUSE"] = fuse
            s.closed_loop_schedule_device(inp, dict(out, plan=plan) if want_plan else out, S, mpc_ticks=mask, **kw)
            return (plan,) if want_plan else ()
        return go

    def ds():
        s.closed_loop_dataset_device(inp, dict(out, **rows), S, first=3, **kw)
        return tuple(rows.values())
    m = f"m{mode}_"
    runs = {m + "tick15": sched(1 << 15), m + "tick0": sched(1), m + "ticks_0_19": sched(1 | 1 << 19),
            m + "tick15_no_plan": sched(1 << 15, want_plan=False), m + "tick15_per_tick": sched(1 << 15, "0")}
    if mode == 0:
        runs.update({"plain": lambda: (s.closed_loop_device(inp, out, S, **kw), ())[1], "dataset": ds,
                     "m0_all_ones": sched((1 << F) - 1), "m0_mask0": sched(0)})
    ms, hs = {k: [] for k in runs}, {}
    for r in range(reps + 1):     # (the first pass warms up)
        for k, go in runs.items():
            for t in (*out.values(), plan, *rows.values()):
                t.zero_()
            extra = go()
            ms[k].append(s.last_kernel_ms())
            hs[k] = hashlib.md5(b"".join(t.cpu().numpy().tobytes() for t in (*(out[q] for q in KEYS), *extra))).hexdigest()[:12]
    print(json.dumps({"lib": os.path.basename(os.environ.get("ALIPMPC_LIB", "tree")), "build_id": alipmpc.build_id(),
                      "mode": mode, "B": B, "S": S, "f_cyc": F,
                      "loop_ms": {k: [round(v, 4) for v in w[1:]] for k, w in ms.items()}, "hash": hs}), flush=True)


def run(parent):
    rounds = int(os.environ.get("AB_ROUNDS", "3"))
    recs = {}
    for _ in range(rounds):
        for mode in MODES:
            for lib in (parent, "tree"):
                env = dict(os.environ)
                env.pop("ALIPMPC_CL_FUSE", None)
                if lib != "tree":
                    env["ALIPMPC_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, __file__, "one", mode], env=env, timeout=240, capture_output=True,
                                   text=True)
                if r.returncode != 0:   # (nothing more is started on the GPU after a failed run)
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit(r.returncode if r.returncode > 0 else 1)
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps(rec), flush=True)
                recs.setdefault((mode, lib), []).append(rec)
    summ, ok = {"tool": "cl_modes_ab", "rounds": rounds}, True
    for mode in MODES:
        pa, ne = recs[(mode, parent)], recs[(mode, "tree")]
        for k in pa[0]["loop_ms"]:
            a = np.array([np.median(r["loop_ms"][k]) for r in pa])
            b = np.array([np.median(r["loop_ms"][k]) for r in ne])
            hashes = {r["hash"][k] for r in pa + ne}
            ok &= len(hashes) == 1
            summ[k] = {"parent_median_ms": round(float(np.median(a)), 4), "new_median_ms": round(float(np.median(b)), 4),
                       "parent_spread_ms": round(float(a.max() - a.min()), 4),
                       "new_spread_ms": round(float(b.max() - b.min()), 4), "outputs_equal": len(hashes) == 1,
                       "hash": sorted(hashes)}
    summ["all_outputs_equal"] = bool(ok)
    print(json.dumps(summ), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one(int(sys.argv[2]))
    else:
        run(sys.argv[2])
