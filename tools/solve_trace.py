"""Dev: the kernels one solve of each program dispatches, for comparing two library builds launch by launch
(profiles/launch_plan).  `run` executes the cases below in one process, each followed by a marker (a torch cos kernel);
run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python tools/solve_trace.py run` (no
counters, no other tracing), once per library (ALIPMPC_LIB).  `diff A/kt_kernel_trace.csv B/kt_kernel_trace.csv OUT`
writes OUT/kernels_<case>_parent_vs_new.txt: per dispatch the kernel name, grid, workgroup and LDS bytes of both builds
side by side, and exits 1 if any case differs.

Cases: fp64 wave handle at the default cuts, B = 512 and B = slots + 1; fp32 and lane handles with cfg.restoration =
IPOPT (the hand-off); a DD handle; a sensitivity solve; the scheduled closed loop in modes 0, 1 and 3 at
tools/cl_modes_ab.py's shape (cfg2 episodes, B = 4096, S = 8, f_cyc = 20, mask {15}, device pointers), on one episode
group (ALIPMPC_CL_GROUPS=1), so that the dispatches of a call have one order.
"""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("wave_fp64_B512", "wave_fp64_slots_plus_1", "wave_fp32_resto", "lane_resto", "dd", "sens",
         "closed_loop_mode0", "closed_loop_mode1", "closed_loop_mode3")


def run():
    sys.path.insert(0, os.path.join(ROOT, "mujoco-lip-mpc-simulation_amd"))
    sys.path.insert(0, ROOT)
    import torch
    import alipmpc
    import bench
    from alipmpc import scenes
    dev = torch.device("cuda", 0)
    mark = torch.zeros(64, device=dev)

    def done(name):
        torch.cuda.synchronize()
        mark.cos_()
        torch.cuda.synchronize()
        print("case", name, flush=True)

    def solve(s, bt):
        return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=bt["u0"])

    done("start")
    s = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0))
    solve(s, scenes.make_batch(512, seed=3, n_cir=5))
    done(CASES[0])
    B = s.solve_slots() + 1
    solve(s, scenes.make_batch_vec(B, seed=4, n_cir=5, N=3))
    done(CASES[1])
    bt = scenes.make_batch(512, seed=5, n_cir=5)
    solve(alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0, precision=alipmpc.PREC_FP32)), bt)
    done(CASES[2])
    solve(alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0, program=alipmpc.PROGRAM_LANE)), bt)
    done(CASES[3])
    rng = np.random.default_rng(6)
    x0 = np.ascontiguousarray(np.stack([bt["x0"][:, 0], bt["x0"][:, 1], bt["x0"][:, 4]], 1))
    lu = np.ascontiguousarray(np.stack([rng.uniform(0.45, 0.75, 512), rng.uniform(-0.15, 0.15, 512)], 1))
    alipmpc.Solver(alipmpc.default_cfg(2, 3, nc_max=5, ne_max=0)).solve(x0, bt["goal"], None, bt["cir"], bt["nc"],
                                                                        u0=np.tile(lu, (1, 3)), last_u=lu)
    done(CASES[4])
    s.solve_sens(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=bt["u0"])
    done(CASES[5])
    B, S, F = 4096, 8, 20
    os.environ["ALIPMPC_CL_GROUPS"] = "1"
    cb = bench.global_inputs("cfg2", 0, B, B, 0, 5, 0, 3)
    inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cb.items() if v is not None}
    inp["leg"], inp["nc"] = inp["leg"].to(torch.int8), inp["nc"].to(torch.int32)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    for mode, name in zip((0, 1, 3), CASES[6:]):
        c = alipmpc.Solver(alipmpc.default_cfg(0, 3, nc_max=5, ne_max=0, cl_between=mode))
        sol = {"u": torch.empty((B, 15), **f64), "foot": torch.empty((B, 3), **f64)}
        c.solve_device(inp, sol)
        inp["foot0"] = sol["foot"][:, 0:2].contiguous()
        out = dict(foot=torch.zeros((B, S, 3), **f64), x=torch.zeros((B, S + 1, 5), **f64), hd=torch.zeros((B, S, 2), **f64),
                   status=torch.zeros((B, S, F), **i32), iters=torch.zeros((B, S, F), **i32),
                   steps_to_goal=torch.zeros(B, **i32), action=torch.zeros((B, S, F, 8), **f64),
                   plan=torch.zeros((B, S, F, 15), **f64))
        c.closed_loop_schedule_device(inp, out, S, f_cyc=F, mpc_ticks=1 << 15, kick=0.05, seed=7)
        done(name)


def dispatches(path):
    """per case, the process's dispatches in start order as (name, grid, workgroup, LDS) strings"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    cases, cur = [], []
    for r in rows:
        if "cos" in r["Kernel_Name"]:
            cases.append(cur)
            cur = []
        else:
            cur.append(f'{r["Kernel_Name"]} grid {r["Grid_Size_X"]} wg {r["Workgroup_Size_X"]} lds {r["LDS_Block_Size"]}')
    assert len(cases) == len(CASES) + 1, len(cases)   # (the first marker is before the first case)
    return dict(zip(CASES, cases[1:]))


def diff(a, b, out):
    da, db = dispatches(a), dispatches(b)
    os.makedirs(out, exist_ok=True)
    same = True
    for name in CASES:
        ka, kb = da[name], db[name]
        eq = ka == kb
        same &= eq
        with open(os.path.join(out, f"kernels_{name}_parent_vs_new.txt"), "w") as f:
            f.write(f"{name}: {len(ka)} | {len(kb)} dispatches, {'identical' if eq else 'DIFFERENT'}\nparent | new\n")
            for i in range(max(len(ka), len(kb))):
                x, y = (ka[i] if i < len(ka) else "-"), (kb[i] if i < len(kb) else "-")
                f.write(f"{x} | {y}{'' if x == y else '   <<<'}\n")
        print(name, len(ka), len(kb), "identical" if eq else "DIFFERENT", flush=True)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        diff(*sys.argv[2:5])
