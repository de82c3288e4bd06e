"""From (seed, global index range) to imitation-learning dataset shards, all on the device.

Per chunk of episodes: the scenes are generated from (seed, global index) (alipmpc_scenes_batch), one solve at the
initial state gives the first foothold, which is taken as the stance foot (the start bench.py's closed-loop leg
and the GPU tests use), and alipmpc_closed_loop_dataset_batch runs the loop and compacts the rows (X, y_mpc, y_act
as the reference's sup_learn/*.csv, data_procs/logger_iml.py:377-401, 416-428) of the ticks that were run.  The
trimmed rows cross PCIe once and are written as one shard, rows_<first>_<count>.npz (with --csv also a directory
of the reference's three file names).  --first / --episodes select a global index range, so a rank writes its
shards alone and they hold the rows the whole sweep holds.  Prints one JSON line: episodes, rows, loop time (the
library's HIP events, summed over the chunks), rows/s and the counts of the rows' solve statuses.

  timeout 900 python tools/mc_dataset.py --episodes 65536 --chunk 16384 --out shards
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--episodes", type=int, default=65536, help="episodes of this run's range")
    ap.add_argument("--first", type=int, default=0, help="first global index of this run's range")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--f-cyc", type=int, default=8, help="MPC calls per walking step (the recorded dataset: 8)")
    ap.add_argument("--kick", type=float, default=0.0, help="plant velocity kick (alipmpc_closed_loop_batch)")
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--n-cir", type=int, default=5)
    ap.add_argument("--safe-dis", type=float, default=0.4, help="taken off the radii in X (0.4: the raw radii)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="directory of the shards (default: rows are counted, not written)")
    ap.add_argument("--csv", action="store_true", help="also write each shard as the reference's three CSV files")
    ap.add_argument("--check", action="store_true", help="run dataset.check_rows on every shard")
    a = ap.parse_args()
    if a.episodes <= 0 or a.first < 0 or a.chunk <= 0:
        ap.error("--episodes, --chunk > 0 and --first >= 0")

    import torch
    import alipmpc
    from alipmpc import dataset

    cfg = alipmpc.default_cfg(alipmpc.VARIANT_MODI, 3, nc_max=a.n_cir, ne_max=0)
    torch.cuda.set_device(a.device)
    dev = torch.device("cuda", a.device)
    s = alipmpc.Solver(cfg, device=a.device)
    C, S, F = min(a.chunk, a.episodes), a.steps, a.f_cyc
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    inp = dict(x0=torch.empty((C, 5), **f64), goal=torch.empty((C, 2), **f64),
               leg=torch.empty(C, dtype=torch.int8, device=dev), cir=torch.empty((C, a.n_cir, 3), **f64),
               nc=torch.empty(C, **i32), u0=torch.empty((C, s.n), **f64), foot0=torch.empty((C, 2), **f64))
    sol = dict(u=torch.empty((C, s.n), **f64), foot=torch.empty((C, 3), **f64))
    cap = C * S * F
    out = dict(X=torch.empty((cap, s.x_cols()), **f64), y_mpc=torch.empty((cap, 8), **f64),
               y_act=torch.empty((cap, 8), **f64), row_status=torch.empty(cap, **i32),
               row_start=torch.empty(C + 1, dtype=torch.int64, device=dev))
    st = torch.cuda.current_stream()

    def chunk(lo, n):
        i = {k: v[:n] for k, v in inp.items()}
        s.scenes_device(i, seed=a.seed, first=lo, n_cir=a.n_cir, stream=st)
        s.solve_device(i, {k: v[:n] for k, v in sol.items()}, stream=st)
        i["foot0"].copy_(sol["foot"][:n, 0:2])
        o = dict(out, row_start=out["row_start"][:n + 1])
        s.closed_loop_dataset_device(i, o, S, F, kick=a.kick, seed=a.seed, first=lo, safe_dis=a.safe_dis,
                                     max_rows=cap, stream=st)
        rs = o["row_start"].cpu()          # (synchronises: the loop is done)
        ms = s.last_kernel_ms()
        R = int(rs[n])
        rows = {k: out[k][:R].cpu().numpy() for k in ("X", "y_mpc", "y_act", "row_status")}   # the one copy
        return rows, rs.numpy(), ms

    chunk(a.first, min(C, 256))            # warm-up (code-object load, first-launch set-up), not timed or written
    loop_ms, rows_n, nshard, resid = 0.0, 0, 0, {}
    counts = {}
    t0 = time.perf_counter()
    for lo in range(a.first, a.first + a.episodes, C):
        n = min(C, a.first + a.episodes - lo)
        rows, rs, ms = chunk(lo, n)
        loop_ms += ms
        rows_n += len(rows["X"])
        for k, v in zip(*np.unique(rows["row_status"], return_counts=True)):
            counts[int(k)] = counts.get(int(k), 0) + int(v)
        if a.check:
            r = dataset.check_rows(rows["X"], rows["y_mpc"], rows["y_act"], rs, F, a.n_cir, 0, cfg, tol_stance=0.0)
            resid = {k: max(v, resid.get(k, 0.0)) for k, v in r.items()}
        if a.out:
            base = os.path.join(a.out, f"rows_{lo}_{n}")
            dataset.write_npz(base + ".npz", row_start=rs, seed=a.seed, first=lo, episodes=n, steps=S, f_cyc=F,
                              kick=a.kick, safe_dis=a.safe_dis, **rows)
            if a.csv:
                dataset.write_csv(base, rows["X"], rows["y_mpc"], rows["y_act"])
        nshard += 1
    wall = time.perf_counter() - t0
    rec = {"tool": "mc_dataset", "build_id": alipmpc.build_id(), "program": s.solve_program(), "episodes": a.episodes,
           "first": a.first, "seed": a.seed, "steps": S, "f_cyc": F, "kick": a.kick, "chunk": C, "shards": nshard,
           "rows": rows_n, "dense_rows": a.episodes * S * F, "loop_ms": round(loop_ms, 3),
           "rows_per_s": round(rows_n / (loop_ms * 1e-3), 1), "wall_s": round(wall, 3),
           "status_counts": {str(k): counts[k] for k in sorted(counts)}}
    if a.check:
        rec["check_rows"] = {k: float(f"{v:.3g}") for k, v in resid.items()}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
