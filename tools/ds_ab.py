"""Dev measurements of the dataset call (profiles/r9/dataset), on bench.py's cfg2 episodes, one walking step, f_cyc = 40.

  python tools/ds_ab.py parent devlib/parent.so [new.so]   A/B of the EXISTING call: alternates the two builds, one
        process per run (>= 4 rounds), hashes every output (they must be equal) and compares the loop time: the
        median difference against the parent's own run-to-run spread.
  python tools/ds_ab.py cost                                one process, this build: alternates the existing call and
        the dataset call (>= 4 pairs); loop ms of both, rows/s.
  python tools/ds_ab.py trace                               one dataset call after a warm-up, to be run under
        rocprofv3 --kernel-trace --stats (the scan and compaction kernels' times).
Environment: AB_B (4096), AB_ROUNDS (4), AB_REPS (3).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 40
KEYS = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")


def setup():
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import alipmpc
    import bench
    B = int(os.environ.get("AB_B", "4096"))
    bt = bench.global_inputs("cfg2", 0, B, B, 0, 5, 0, 3)
    s = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0))
    dev = torch.device("cuda", 0)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
    inp["leg"], inp["nc"] = inp["leg"].to(torch.int8), inp["nc"].to(torch.int32)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    sol = {"u": torch.empty((B, 15), **f64), "foot": torch.empty((B, 3), **f64)}
    s.solve_device(inp, sol)
    inp["foot0"] = sol["foot"][:, 0:2].contiguous()
    out = dict(foot=torch.empty((B, 1, 3), **f64), x=torch.empty((B, 2, 5), **f64), hd=torch.empty((B, 1, 2), **f64),
               status=torch.empty((B, 1, F), **i32), iters=torch.empty((B, 1, F), **i32),
               steps_to_goal=torch.empty(B, **i32), action=torch.empty((B, 1, F, 8), **f64))
    rows = dict(X=torch.empty((B * F, 26), **f64), y_mpc=torch.empty((B * F, 8), **f64),
                y_act=torch.empty((B * F, 8), **f64), row_status=torch.empty(B * F, **i32),
                row_start=torch.empty(B + 1, dtype=torch.int64, device=dev))
    return torch, alipmpc, s, B, inp, out, rows


def digest(out):
    return hashlib.md5(b"".join(out[k].cpu().numpy().tobytes() for k in KEYS)).hexdigest()[:12]


def one_existing():
    torch, alipmpc, s, B, inp, out, _ = setup()
    ms = []
    for _ in range(1 + int(os.environ.get("AB_REPS", "3"))):
        s.closed_loop_device(inp, out, 1, f_cyc=F, kick=0.05, seed=7)
        ms.append(s.last_kernel_ms())
    print(json.dumps({"lib": os.environ.get("ALIPMPC_LIB", "tree"), "build_id": alipmpc.build_id(), "B": B,
                      "loop_ms": [round(m, 4) for m in ms[1:]], "hash": digest(out)}), flush=True)


def parent(libs):
    rounds = int(os.environ.get("AB_ROUNDS", "4"))
    recs = {lib: [] for lib in libs}
    for _ in range(rounds):
        for lib in libs:
            env = dict(os.environ)
            if lib != "tree":
                env["ALIPMPC_LIB"] = os.path.join(ROOT, lib)
            r = subprocess.run([sys.executable, __file__, "one"], env=env, timeout=280, capture_output=True, text=True)
            if r.returncode != 0:   # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode)
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            recs[lib].append(rec)
    a, b = libs[0], libs[-1]
    ma = np.array([np.median(r["loop_ms"]) for r in recs[a]])
    mb = np.array([np.median(r["loop_ms"]) for r in recs[b]])
    hashes = {r["hash"] for v in recs.values() for r in v}
    print(json.dumps({"tool": "ds_ab parent", "parent": a, "new": b, "rounds": rounds,
                      "parent_run_medians_ms": ma.round(4).tolist(), "new_run_medians_ms": mb.round(4).tolist(),
                      "parent_median_ms": round(float(np.median(ma)), 4), "new_median_ms": round(float(np.median(mb)), 4),
                      "median_difference_ms": round(float(np.median(mb) - np.median(ma)), 4),
                      "parent_spread_ms": round(float(ma.max() - ma.min()), 4),
                      "outputs_equal": len(hashes) == 1, "hashes": sorted(hashes)}))
    sys.exit(0 if len(hashes) == 1 else 1)


def cost():
    torch, alipmpc, s, B, inp, out, rows = setup()
    pairs = int(os.environ.get("AB_ROUNDS", "4"))
    ex, ds, hs = [], [], set()
    for k in range(pairs + 1):
        s.closed_loop_device(inp, out, 1, f_cyc=F, kick=0.05, seed=7)
        ex.append(s.last_kernel_ms())
        hs.add(digest(out))
        s.closed_loop_dataset_device(inp, dict(out, **rows), 1, f_cyc=F, kick=0.05, seed=7)
        ds.append(s.last_kernel_ms())
        hs.add(digest(out))
    ex, ds = np.array(ex[1:]), np.array(ds[1:])
    R = int(rows["row_start"][B].item())
    print(json.dumps({"tool": "ds_ab cost", "build_id": alipmpc.build_id(), "B": B, "f_cyc": F, "pairs": pairs,
                      "existing_ms": ex.round(4).tolist(), "dataset_ms": ds.round(4).tolist(),
                      "existing_median_ms": round(float(np.median(ex)), 4),
                      "dataset_median_ms": round(float(np.median(ds)), 4),
                      "median_difference_ms": round(float(np.median(ds) - np.median(ex)), 4),
                      "existing_spread_ms": round(float(ex.max() - ex.min()), 4), "rows": R,
                      "rows_per_s": round(R / (float(np.median(ds)) * 1e-3), 1), "loop_outputs_equal": len(hs) == 1}))


def trace():
    torch, alipmpc, s, B, inp, out, rows = setup()
    for _ in range(2):
        s.closed_loop_dataset_device(inp, dict(out, **rows), 1, f_cyc=F, kick=0.05, seed=7)
    torch.cuda.synchronize()
    print("loop ms", s.last_kernel_ms(), "rows", int(rows["row_start"][B].item()))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "one":
        one_existing()
    elif mode == "parent":
        parent(sys.argv[2:] if len(sys.argv) > 3 else [sys.argv[2], "tree"])
    elif mode == "cost":
        cost()
    else:
        trace()
