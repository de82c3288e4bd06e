"""Dev measurement of the scheduled closed loop (alipmpc_closed_loop_schedule_batch; DESIGN "Scheduled closed loop",
profiles/cl_schedule) on bench.py's cfg2 episodes: B = 4096, S = 8 walking steps, f_cyc = 20, device pointers.

  python tools/cl_schedule_bench.py run [parent.so]   rounds of one process per build, alternating: the parent build's
        closed_loop (a) when a parent library is given, then this build's closed_loop (b), all-ones schedule (c), tick 15
        with fused runs (d), tick 15 with ALIPMPC_CL_FUSE=0 (e) and mask 0 (f), the five alternating inside the process.
        Prints every process's line and a summary: medians in ms per loop, tick-episodes per second, (a)'s run-to-run
        spread, and whether (a), (b), (c) gave the same outputs.
  python tools/cl_schedule_bench.py one                one process of the build ALIPMPC_LIB names (default: the tree's).
Environment: AB_B (4096), AB_S (8), AB_ROUNDS (4), AB_REPS (3).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 20
KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")


def setup():
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import alipmpc
    import bench
    B, S = int(os.environ.get("AB_B", "4096")), int(os.environ.get("AB_S", "8"))
    bt = bench.global_inputs("cfg2", 0, B, B, 0, 5, 0, 3)
    s = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0))
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
    return alipmpc, s, B, S, inp, out


def digest(out):
    return hashlib.md5(b"".join(out[k].cpu().numpy().tobytes() for k in KEYS)).hexdigest()[:12]


def one():
    alipmpc, s, B, S, inp, out = setup()
    reps = int(os.environ.get("AB_REPS", "3"))
    have = hasattr(s._L, "alipmpc_closed_loop_schedule_batch")
    kw = dict(f_cyc=F, kick=0.05, seed=7)

    def sched(mask, fuse="1"):
        def go():
            os.environ["ALIPMPC_CL_FUSE"] = fuse
            s.closed_loop_schedule_device(inp, out, S, mpc_ticks=mask, **kw)
        return go
    runs = {"closed_loop": lambda: s.closed_loop_device(inp, out, S, **kw)}
    if have:
        runs.update({"all_ones": sched((1 << F) - 1), "tick15_fused": sched(1 << 15), "tick15_per_tick": sched(1 << 15, "0"),
                     "mask0": sched(0)})
    ms, hs = {k: [] for k in runs}, {}
    for r in range(reps + 1):     # (the first pass warms up)
        for k, go in runs.items():
            out["hd"].zero_()
            go()
            ms[k].append(s.last_kernel_ms())
            hs[k] = digest(out)
    print(json.dumps({"lib": os.path.basename(os.environ.get("ALIPMPC_LIB", "tree")), "build_id": alipmpc.build_id(), "B": B, "S": S,
                      "f_cyc": F, "loop_ms": {k: [round(m, 4) for m in v[1:]] for k, v in ms.items()}, "hash": hs}),
          flush=True)


def run(parent):
    rounds = int(os.environ.get("AB_ROUNDS", "4"))
    libs = ([parent] if parent else []) + ["tree"]
    recs = {lib: [] for lib in libs}
    for _ in range(rounds):
        for lib in libs:
            env = dict(os.environ)
            env.pop("ALIPMPC_CL_FUSE", None)
            if lib != "tree":
                env["ALIPMPC_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, __file__, "one"], env=env, timeout=280, capture_output=True, text=True)
            if r.returncode != 0:   # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode)
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            recs[lib].append(rec)
    B, S = recs["tree"][0]["B"], recs["tree"][0]["S"]
    med = lambda lib, k: np.array([np.median(r["loop_ms"][k]) for r in recs[lib]])   # noqa: E731
    summ = {"tool": "cl_schedule_bench", "B": B, "S": S, "f_cyc": F, "rounds": rounds}
    names = {"closed_loop": "b_closed_loop", "all_ones": "c_all_ones", "tick15_fused": "d_tick15_fused",
             "tick15_per_tick": "e_tick15_per_tick", "mask0": "f_mask0"}
    cols = {v: med("tree", k) for k, v in names.items()}
    if parent:
        cols = {"a_parent_closed_loop": med(parent, "closed_loop"), **cols}
    for k, v in cols.items():
        m = float(np.median(v))
        summ[k] = {"run_medians_ms": v.round(4).tolist(), "median_ms": round(m, 4), "spread_ms": round(float(v.max() - v.min()), 4),
                   "tick_episodes_per_s": round(B * S * F / (m * 1e-3), 1)}
    hashes = {r["hash"]["closed_loop"] for v in recs.values() for r in v} | {r["hash"]["all_ones"] for r in recs["tree"]}
    summ["existing_path_outputs_equal"] = len(hashes) == 1
    summ["fused_equals_per_tick"] = all(r["hash"]["tick15_fused"] == r["hash"]["tick15_per_tick"] for r in recs["tree"])
    print(json.dumps(summ))
    sys.exit(0 if summ["existing_path_outputs_equal"] and summ["fused_equals_per_tick"] else 1)


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one()
    else:
        run(sys.argv[2] if len(sys.argv) > 2 else None)
