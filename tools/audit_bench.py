"""Plan audit against what it replaces, on one GPU, alternating runs (plan audit).

Scenes are generated on the device (alipmpc_scenes_batch), solved once, and the solutions are then examined three ways:
  audit  alipmpc_audit_batch over the whole batch: metrics, where, summary — one launch
  a      the feasibility leg of bench.py --full: alipmpc_eval_batch of c, cl, cu, row_active in chunks of 65,536 and
         the torch reduction of bench.feasible_fraction (five element-wise / reduction kernels per chunk)
  b      alipmpc_trace_batch in chunks and a torch reduction of the circle clearances of the dense trace
Every repetition runs audit, a, b in turn and times each with HIP events; the line reports the median and the
minimum, the audit's algorithmic bytes (inputs read + outputs written, from the shapes) over its median time, and
checks that the three agree (the feasible count exactly, the clearance to 1e-9).  N = 3 with circles only.

  timeout 600 python tools/audit_bench.py --B 65536                 # cfg2's shape, fp64 wave handle
  timeout 900 python tools/audit_bench.py --B 1048576 --lane        # cfg5's shape, fp32 lane handle
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))

CHUNK = 65536


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--n-cir", type=int, default=5)
    ap.add_argument("--lane", action="store_true", help="fp32 lane handle (cfg5) instead of the fp64 wave handle (cfg2)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import alipmpc
    from alipmpc import audit

    N, nc = 3, a.n_cir
    kw = dict(precision=alipmpc.PREC_FP32, program=alipmpc.PROGRAM_LANE) if a.lane else {}
    cfg = alipmpc.default_cfg(alipmpc.VARIANT_MODI, N, nc_max=nc, ne_max=0, **kw)
    torch.cuda.set_device(a.device)
    dev = torch.device("cuda", a.device)
    s = alipmpc.Solver(cfg, device=a.device)
    ev64 = alipmpc.Solver(alipmpc.default_cfg(alipmpc.VARIANT_MODI, N, nc_max=nc, ne_max=0), device=a.device)
    B, m, rows = a.B, s.m_max, alipmpc.trace_len(cfg)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    inp = dict(x0=torch.empty((B, 5), **f64), goal=torch.empty((B, 2), **f64),
               leg=torch.empty(B, dtype=torch.int8, device=dev), cir=torch.empty((B, nc, 3), **f64),
               nc=torch.empty(B, **i32), u0=torch.empty((B, s.n), **f64))
    out = dict(u=torch.empty((B, s.n), **f64), status=torch.empty(B, **i32))
    for lo in range(0, B, 1 << 17):
        hi = min(B, lo + (1 << 17))
        s.scenes_device({k: v[lo:hi] for k, v in inp.items()}, seed=a.seed, first=lo, n_cir=nc)
        s.solve_device({k: v[lo:hi] for k, v in inp.items()}, {k: v[lo:hi] for k, v in out.items()})
    torch.cuda.synchronize()
    edges = [-0.2, -0.1, -0.05, 0.0, 0.05, 0.1, 0.2, 0.4]
    ainp = dict(inp, u=out["u"], status=out["status"])
    aout = dict(metrics=torch.empty((B, 5), **f64), where=torch.empty((B, 3), **i32),
                summary=torch.zeros(alipmpc.audit_summary_len(len(edges)), dtype=torch.int64, device=dev))
    C = min(CHUNK, B)
    eo = {"c": torch.empty((C, m), **f64), "cl": torch.empty((C, m), **f64), "cu": torch.empty((C, m), **f64),
          "row_active": torch.empty((C, m), dtype=torch.int8, device=dev)}
    tr = torch.empty((C, N, rows, 2), **f64)
    feas = torch.zeros((), dtype=torch.int64, device=dev)
    clear_b = torch.empty(B, **f64)

    def leg_audit():
        aout["summary"].zero_()
        s.audit_device(ainp, aout, edges=edges)

    def leg_a():
        feas.zero_()
        for lo in range(0, B, C):
            hi = min(B, lo + C)
            n = hi - lo
            sub = {k: v[lo:hi] for k, v in inp.items() if k != "u0"}
            sub["u"] = out["u"][lo:hi]
            o = {k: v[:n] for k, v in eo.items()}
            ev64.eval_device(sub, o)
            v = torch.clamp(torch.maximum(o["cl"] - o["c"], o["c"] - o["cu"]), min=0.0)
            v = torch.where(o["row_active"] != 0, v, torch.zeros_like(v))
            feas.add_((v.amax(dim=1) <= 1e-4).sum())

    def leg_b():
        for lo in range(0, B, C):
            hi = min(B, lo + C)
            n = hi - lo
            s.trace_device(inp["x0"][lo:hi], out["u"][lo:hi], tr[:n])
            p = tr[:n].reshape(n, N * rows, 1, 2)
            c = inp["cir"][lo:hi]
            d = torch.linalg.vector_norm(p - c[:, None, :, 0:2], dim=3) - c[:, None, :, 2]
            valid = torch.arange(nc, device=dev)[None, :] < inp["nc"][lo:hi, None]
            d = torch.where(valid[:, None, :], d, torch.full_like(d, float("inf")))
            clear_b[lo:hi] = d.amin(dim=(1, 2))

    legs = dict(audit=leg_audit, a=leg_a, b=leg_b)
    for f in legs.values():   # warm-up: code objects, allocator
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    met = aout["metrics"]
    summ = aout["summary"].cpu().numpy()
    feas_audit = int((met[:, 0] <= 1e-4).sum().item())
    dclear = float(torch.nan_to_num(met[:, 1] - clear_b, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item())
    in_bytes = 8 * (5 + 2 + 3 * nc + 5 * N) + 1 + 4 + 4
    out_bytes = 8 * 5 + 4 * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = {"tool": "audit_bench", "build_id": alipmpc.build_id(), "B": B, "N": N, "n_cir": nc,
           "handle": s.solve_program(), "reps": a.reps,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "audit_bytes_per_instance": {"read": in_bytes, "written": out_bytes},
           "audit_GBps_algorithmic": round(B * (in_bytes + out_bytes) / (med["audit"] * 1e-3) / 1e9, 2),
           "a_bytes_per_instance_written": m * 25,
           "a_over_audit": round(med["a"] / med["audit"], 2), "b_over_audit": round(med["b"] / med["audit"], 2),
           "feasible_a": int(feas.item()), "feasible_audit": feas_audit, "summary_viol_ok": int(summ[2]),
           "max_abs_clear_minus_b": dclear,
           "audit": audit.describe(summ, len(edges), edges)}
    print(json.dumps(rec))
    assert rec["feasible_a"] == feas_audit == int(summ[2]), (rec["feasible_a"], feas_audit, int(summ[2]))
    assert dclear <= 1e-9, dclear


if __name__ == "__main__":
    main()
