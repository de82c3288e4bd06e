"""Monte-Carlo sweep with the scenes generated on the device (alipmpc_scenes_batch): by default BASELINE cfg5's
shape — fp32 lane program, N = 3, 5 circles, one obstacle field per instance, 2^20 scenes.

The sweep runs in chunks: each chunk is generated on the device from (seed, global index), solved from the same
device buffers and reduced to a count of feasible instances on the device (status != 2, the driver's rule,
main_sim_mpc.py:118); nothing but that count crosses PCIe.  --first / --count select a global index range, so a
rank runs its shard alone and the shards' rows are those of the whole sweep.  Prints one JSON line: generation
and solve time (HIP events, summed over the chunks), the feasible fraction, and as the host comparison the wall
time of scenes.make_batch_vec for one 16,384-instance chunk.

  timeout 600 python tools/mc_sweep.py                      # cfg5's shape
  timeout 600 python tools/mc_sweep.py --scenes 65536 --n-cir 5 --n-elp 5 --horizon 5 --fields 4096   # dense mix
  timeout 600 python tools/mc_sweep.py --n-cir 3 --n-elp 2                                        # mix on the lane program
The solve is the fp32 lane program where it serves the shape — horizon 3 with circles only (<= 6), or circles and
ellipses with --n-cir + --n-elp <= 5 (its obstacle-form build: 2.5x the fp64 wave program's rate on 3 + 2 mix scenes,
profiles/lane_elp/bench.jsonl) — and the fp64 wave program otherwise.
--audit adds the plan audit (alipmpc_audit_batch) of every chunk's solutions on the same device buffers: one summary
buffer is carried through all chunks and read once at the end; the JSON line gains "audit" (constraint violation x
dense-trace clearance counts, the clearance histogram over --edges, the table by status class) and "audit_ms".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))

HOST_CHUNK = 16384


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=1 << 20, help="size of the whole sweep (global indices 0 .. scenes-1)")
    ap.add_argument("--first", type=int, default=0, help="first global index of this run's range")
    ap.add_argument("--count", type=int, default=None, help="instances of this run's range (default: up to --scenes)")
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n-cir", type=int, default=5)
    ap.add_argument("--n-elp", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=3)
    ap.add_argument("--fields", type=int, default=0, help="distinct obstacle fields (0: one per instance)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gen-only", action="store_true", help="generate only (no solve, no feasible fraction)")
    ap.add_argument("--no-host", action="store_true", help="skip the host generator comparison")
    ap.add_argument("--audit", action="store_true", help="audit every plan on the device (violation, trace clearance)")
    ap.add_argument("--edges", default="-0.2,-0.1,-0.05,0,0.05,0.1,0.2,0.4",
                    help="clearance histogram edges in metres for --audit (comma-separated, increasing)")
    ap.add_argument("--viol-tol", type=float, default=1e-4, help="violation tolerance for --audit")
    a = ap.parse_args()

    import torch
    import alipmpc
    from alipmpc import scenes

    count = a.scenes - a.first if a.count is None else a.count
    if a.first < 0 or count <= 0 or a.first + count > a.scenes:
        ap.error("--first / --count must select a non-empty range within --scenes")
    lane = a.horizon == 3 and (a.n_cir <= 6 if a.n_elp == 0 else a.n_cir + a.n_elp <= 5)
    kw = dict(precision=alipmpc.PREC_FP32, program=alipmpc.PROGRAM_LANE) if lane else {}
    cfg = alipmpc.default_cfg(alipmpc.VARIANT_MODI, a.horizon, nc_max=a.n_cir, ne_max=a.n_elp, **kw)
    torch.cuda.set_device(a.device)
    dev = torch.device("cuda", a.device)
    s = alipmpc.Solver(cfg, device=a.device)
    C = min(a.chunk, count)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    inp = dict(x0=torch.empty((C, 5), **f64), goal=torch.empty((C, 2), **f64),
               leg=torch.empty(C, dtype=torch.int8, device=dev), cir=torch.empty((C, a.n_cir, 3), **f64),
               nc=torch.empty(C, **i32), u0=torch.empty((C, s.n), **f64))
    if a.n_elp:
        inp["elp"], inp["ne"] = torch.empty((C, a.n_elp, 5), **f64), torch.empty(C, **i32)
    out = dict(u=torch.empty((C, s.n), **f64), foot=torch.empty((C, 3), **f64), status=torch.empty(C, **i32),
               iters=torch.empty(C, **i32))
    gen_kw = dict(seed=a.seed, n_cir=a.n_cir, n_elp=a.n_elp, fields=a.fields)
    st = torch.cuda.current_stream()
    infeasible = torch.zeros((), dtype=torch.int64, device=dev)
    do_audit = a.audit and not a.gen_only
    if do_audit:
        from alipmpc import audit
        edges = [float(v) for v in a.edges.split(",") if v.strip()]
        asum = torch.zeros(alipmpc.audit_summary_len(len(edges)), dtype=torch.int64, device=dev)

    def views(d, n):
        return d if n == C else {k: v[:n] for k, v in d.items()}

    def chunk(lo, n, ev):
        i, o = views(inp, n), views(out, n)
        ev[0].record(st)
        s.scenes_device(i, first=lo, stream=st, **gen_kw)
        ev[1].record(st)
        if not a.gen_only:
            s.solve_device(i, o, stream=st)
            ev[2].record(st)
            infeasible.add_((o["status"] == 2).sum())
            if do_audit:
                ev[3].record(st)
                s.audit_device(dict(i, u=o["u"], status=o["status"]), dict(summary=asum), edges=edges,
                               viol_tol=a.viol_tol, stream=st)
                ev[4].record(st)

    def events():
        return [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    # warm-up (code-object load, first-launch set-up): the first chunk's range, not timed
    chunk(a.first, min(C, count), events())
    torch.cuda.synchronize()
    infeasible.zero_()
    if do_audit:
        asum.zero_()
    evs = []
    t0 = time.perf_counter()
    for lo in range(a.first, a.first + count, C):
        evs.append(events())
        chunk(lo, min(C, a.first + count - lo), evs[-1])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    gen_ms = sum(e[0].elapsed_time(e[1]) for e in evs)
    rec = {"tool": "mc_sweep", "build_id": alipmpc.build_id(), "scenes": a.scenes, "first": a.first, "count": count,
           "chunk": C, "chunks": len(evs), "seed": a.seed, "n_cir": a.n_cir, "n_elp": a.n_elp, "horizon": a.horizon,
           "fields": a.fields, "gen_ms": round(gen_ms, 4), "gen_scenes_per_s": round(count / (gen_ms * 1e-3), 1),
           "wall_s": round(wall, 4)}
    if not a.gen_only:
        solve_ms = sum(e[1].elapsed_time(e[2]) for e in evs)
        rec.update(program=s.solve_program(), solve_ms=round(solve_ms, 4),
                   solves_per_s=round(count / (solve_ms * 1e-3), 1), gen_over_solve=round(gen_ms / solve_ms, 5),
                   feasible_fraction=round(1.0 - infeasible.item() / count, 6))
    if do_audit:
        audit_ms = sum(e[3].elapsed_time(e[4]) for e in evs)
        rec.update(audit_ms=round(audit_ms, 4), audit_over_solve=round(audit_ms / solve_ms, 5),
                   audit=audit.describe(asum.cpu().numpy(), len(edges), edges))
    if not a.no_host:
        t0 = time.perf_counter()
        scenes.make_batch_vec(HOST_CHUNK, seed=a.seed, n_cir=a.n_cir, n_elp=a.n_elp, N=a.horizon,
                              fields=a.fields or None)
        host = time.perf_counter() - t0
        rec.update(host_make_batch_vec_16384_s=round(host, 4),
                   host_extrapolated_s=round(host * count / HOST_CHUNK, 2),
                   host_over_gen=round(host * count / HOST_CHUNK / (gen_ms * 1e-3), 1))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
