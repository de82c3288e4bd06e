"""Dev A/B of the solve's host path: small batches through device pointers, where a call costs more on the host than on
the device (profiles/launch_plan).  Rounds of one process per build, alternating; per build and B the median host time
of a solve_device call (enqueue only) and the wall time per call of the whole run (enqueue, execution, one final
synchronise), each the median over the rounds with its max - min.

  python tools/solve_host_ab.py run PARENT.so [PARENT.so ...]   AB_CALLS (3000) AB_ROUNDS (3); "tree" is always added
  python tools/solve_host_ab.py one                             the library ALIPMPC_LIB names (default: the tree's)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = (2, 64)


def one():
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    import torch
    import alipmpc
    from alipmpc import scenes
    calls = int(os.environ.get("AB_CALLS", "3000"))
    dev = torch.device("cuda", 0)
    s = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0))
    rec = {"lib": os.environ.get("AB_NAME", "tree"), "build_id": alipmpc.build_id(), "calls": calls}
    st = torch.cuda.Stream(device=dev)
    for B in BS:
        bt = scenes.make_batch(B, seed=11, n_cir=5)
        inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
        inp["leg"], inp["nc"] = inp["leg"].to(torch.int8), inp["nc"].to(torch.int32)
        out = {"u": torch.empty((B, 15), dtype=torch.float64, device=dev),
               "foot": torch.empty((B, 3), dtype=torch.float64, device=dev),
               "status": torch.empty(B, dtype=torch.int32, device=dev), "iters": torch.empty(B, dtype=torch.int32, device=dev)}
        for _ in range(50):
            s.solve_device(inp, out, stream=st)
        torch.cuda.synchronize()
        host = np.empty(calls)
        t0 = time.perf_counter()
        for i in range(calls):
            a = time.perf_counter()
            s.solve_device(inp, out, stream=st)
            host[i] = time.perf_counter() - a
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rec[f"B{B}"] = {"host_us_per_call": round(float(np.median(host)) * 1e6, 3), "wall_us_per_call": round(wall / calls * 1e6, 3),
                        "launches": s.solve_launches(B)[0]}
    print(json.dumps(rec), flush=True)


def run(libs):
    rounds = int(os.environ.get("AB_ROUNDS", "3"))
    names = [f"parent{i}" for i in range(len(libs))] + ["tree"]
    recs = {n: [] for n in names}
    for _ in range(rounds):
        for n, lib in zip(names, [*libs, None]):
            env = dict(os.environ, AB_NAME=n)
            if lib:
                env["ALIPMPC_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, __file__, "one"], env=env, timeout=240, capture_output=True, text=True)
            if r.returncode != 0:   # (nothing more is started on the GPU after a failed run)
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(r.returncode if r.returncode > 0 else 1)
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            recs[n].append(rec)
    summ = {"tool": "solve_host_ab", "rounds": rounds}
    for n in names:
        for B in BS:
            for k in ("host_us_per_call", "wall_us_per_call"):
                v = np.array([r[f"B{B}"][k] for r in recs[n]])
                summ[f"{n}_B{B}_{k}"] = {"median": round(float(np.median(v)), 3), "spread": round(float(v.max() - v.min()), 3)}
    print(json.dumps(summ), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one()
    else:
        run(sys.argv[2:])
