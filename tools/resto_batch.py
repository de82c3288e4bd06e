#!/usr/bin/env python3
"""Study (CPU): the cfg2 bench batch (4096 instances, seed 0, bench.scene_block) solved by the numpy
oracle with the build's restoration substitute and with IPOPT's restoration phase (np_oracle._resto): status mix,
iterations, line-search trials (the work a wave spends; the slowest instances set the split launch's phase 2) and how
the restorations ended.

  python tools/resto_batch.py [--B 4096] [--modes substitute,ipopt] [--prox u,p] [--out profiles/r6/resto/cfg2_batch.json]

--first-failure (CPU only, r7): with IPOPT's restoration phase and proximity "p", also the iteration at which each
instance's line search first fails (np_oracle._resto wrapped) and, per phase-1 cut c of the split launch, the records
phase 1 leaves: pending-restoration ones (first failure before c), regular ones (still running at c) and the regular
wave-iterations left — to profiles/r7/resto/first_failure.json.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
import np_oracle as O  # noqa: E402
from alipmpc import scenes  # noqa: E402

BT = None


def _init(B):
    global BT
    BT = scenes.make_batch(B, seed=0, n_cir=5, N=3)


def one(args):
    i, mode, prox = args
    O.RESTO["proximity"] = prox
    cfg = O.default_cfg(0, 3, nc_max=5, ne_max=0)
    pr = O.Problem(cfg, BT["x0"][i], BT["goal"][i], BT["leg"][i], BT["cir"][i][:BT["nc"][i]], np.zeros((0, 5)))
    st = {}
    u, s, it = O.solve_footholds(pr, BT["u0"][i], stats=st, restoration=mode)
    _, p0 = O.plan(pr, u)
    return p0, int(s), int(it), int(st.get("trials", 0)), int(st.get("restorations", 0)), st.get("resto", []), \
        int(st.get("resto_iters", 0))


def one_first(i):
    """(iterations, status, iteration whose line search first failed or -1) with IPOPT's restoration phase."""
    O.RESTO["proximity"] = "p"
    cfg = O.default_cfg(0, 3, nc_max=5, ne_max=0)
    pr = O.Problem(cfg, BT["x0"][i], BT["goal"][i], BT["leg"][i], BT["cir"][i][:BT["nc"][i]], np.zeros((0, 5)))
    first = []
    inner = O._resto

    def logged(prob, x, s, zl, zu, mu_o, cl, cu, hl, hu, filt_o, theta_R, orig_phi, it, *rest):
        first.append(it - 1)   # (the caller has counted the failed iteration)
        return inner(prob, x, s, zl, zu, mu_o, cl, cu, hl, hu, filt_o, theta_R, orig_phi, it, *rest)
    O._resto = logged
    try:
        _, s, it = O.solve_footholds(pr, BT["u0"][i], restoration="ipopt")
    finally:
        O._resto = inner
    return int(it), int(s), int(first[0]) if first else -1


def first_failure(ex, B, out):
    res = np.array(list(ex.map(one_first, range(B), chunksize=16)))
    its, st, ff = res[:, 0], res[:, 1], res[:, 2]
    cap = int(its.max())
    rest = ff >= 0
    rep = {"B": B,
           "numbering": "iterations count from 0 as the kernel's do: an instance whose search fails in iteration f is "
                        "cut by phase 1 when f < c (np_oracle._resto receives f + 1)",
           "restoring_instances": int(rest.sum()), "restoring_at_cap": int((rest & (its >= cap)).sum()),
           "first_failure_histogram": {str(k): int(v) for k, v in zip(*np.unique(ff[rest], return_counts=True))},
           "iterations_left_after_first_failure_quartiles": [float(q) for q in
                                                             np.percentile((its - ff)[rest], [25, 50, 75, 100])],
           "never_restoring_at_cap": int((~rest & (its >= cap)).sum()),
           "never_restoring_iters_range": [int(its[~rest].min()), int(its[~rest & (its < cap)].max())],
           "status": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
           "per_cut": {}}
    for c in range(8, 21):
        pend = rest & (ff < c)
        reg = ~pend & (its >= c)   # still running at the top of iteration c
        rep["per_cut"][str(c)] = {"pending": int(pend.sum()), "regular": int(reg.sum()),
                                  "regular_wave_iterations_left": int((its - c)[reg].sum())}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print("first_failure", json.dumps(rep), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--modes", default="substitute,ipopt")
    ap.add_argument("--prox", default="u")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6", "resto", "cfg2_batch.json"))
    ap.add_argument("--first-failure", action="store_true",
                    help="only the first-restoration-iteration histogram and the per-cut record table (CPU)")
    ap.add_argument("--first-out", default=os.path.join(ROOT, "profiles", "r7", "resto", "first_failure.json"))
    a = ap.parse_args()
    if a.first_failure:
        with ProcessPoolExecutor(a.jobs, initializer=_init, initargs=(a.B,)) as ex:
            first_failure(ex, a.B, a.first_out)
        return
    rep = {"B": a.B}
    feet = {}
    with ProcessPoolExecutor(a.jobs, initializer=_init, initargs=(a.B,)) as ex:
        for mode in a.modes.split(","):
            for prox in (a.prox.split(",") if mode == "ipopt" else ["u"]):
                t0 = time.time()
                res = list(ex.map(one, [(i, mode, prox) for i in range(a.B)], chunksize=16))
                key = mode if mode != "ipopt" else f"ipopt_prox_{prox}"
                feet[key] = np.array([r[0] for r in res])
                st = np.array([r[1] for r in res])
                its = np.array([r[2] for r in res])
                tr = np.array([r[3] for r in res])
                rest = {}
                for r in res:
                    for e in r[5]:
                        rest[e] = rest.get(e, 0) + 1
                s2 = st == 2
                rep[key] = {"status": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                            "mean_iters": float(its.mean()), "max_iters": int(its.max()),
                            "mean_trials": float(tr.mean()), "max_trials": int(tr.max()),
                            "trials_p99": float(np.percentile(tr, 99)),
                            "status2_mean_iters": float(its[s2].mean()) if s2.any() else 0.0,
                            "status2_mean_trials": float(tr[s2].mean()) if s2.any() else 0.0,
                            "line_search_failures": int(sum(r[4] for r in res)), "resto_outcomes": rest,
                            "resto_iters": int(sum(r[6] for r in res)), "s": round(time.time() - t0, 1)}
                print(key, json.dumps(rep[key]), flush=True)
    keys = list(feet)
    for k in keys[1:]:
        d = np.max(np.abs(feet[k] - feet[keys[0]]), axis=1)
        rep[f"{k}_vs_{keys[0]}_feet_within_1e-4"] = float(np.mean(d <= 1e-4))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rep, fh, indent=1)


if __name__ == "__main__":
    main()
