"""CPU: host-side pieces — the C ABI library exports, the reference-facing planner helpers, the synthetic
scene generator, and the multi-rank sharding/gather logic (gloo, world size 2)."""
import os
import re
import ctypes

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "alipmpc.h")).read()
    return sorted(set(re.findall(r"\b(alipmpc_[a-z_]+)\s*\(", src)))


def test_library_builds_and_exports_every_header_symbol():
    import alipmpc
    from alipmpc import build
    build.build()                                  # hipcc cross-compiles gfx950 without a GPU
    lib = ctypes.CDLL(build.LIB)
    declared = header_functions()
    assert set(declared) == set(alipmpc.EXPORTS)
    for sym in declared:
        assert hasattr(lib, sym), sym


def test_default_cfg_matches_reference_constants():
    import alipmpc
    c = alipmpc.default_cfg(alipmpc.VARIANT_MODI, 3)
    # MPC_LIP_modi.py:35-41, 397-411
    assert (c.leg2_max, c.bvx_lo, c.bvx_hi, c.bvy_lo, c.bvy_hi) == (0.09, 0.4, 0.8, 0.15, 0.35)
    assert (c.p, c.q, c.r, c.gamma) == (0.0, 1.0, 50.0, 0.2)
    assert abs(c.s - 0.024 * 180 / np.pi) < 1e-15 and abs(c.dtheta_max - np.pi / 16) < 1e-15
    s = alipmpc.default_cfg(alipmpc.VARIANT_SIG_STEP, 3)
    # MPC_LIP_sig_step.py:38, 340-353
    assert (s.bvy_hi, s.p, s.q, s.r, s.gamma, s.select_obs) == (0.30, 2.0, 1.0, 15.0, 0.4, 0)
    assert alipmpc.rows_per_step(c) == 4 + 6 + 6 + 1 and alipmpc.rows_per_step(s) == 4 + 6 + 6
    assert alipmpc.num_vars(c) == 15
    # the reference's IPOPT iteration caps (MPC_LIP_modi.py:287, MPC_LIP_sig_step.py:269)
    assert (c.max_iter, s.max_iter) == (30, 20)


def test_no_device_fails_loudly():
    import torch
    import alipmpc
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="ENODEV"):
        alipmpc.Solver(alipmpc.default_cfg(0, 3))


def test_planner_host_helpers_match_reference(golden):
    from alipmpc import planner
    g = golden("g4_aux")
    beta = np.sqrt(9.81)
    for row, out, trk, ln in zip(g["gns_in"], g["gns_out"], g["trk"], g["trk_len"]):
        xn, det = planner.next_state(beta, 0.4, row[0:2], row[2:4], row[4], row[5:8], row[8])
        assert np.max(np.abs(xn - out)) < 1e-13
        assert det.shape == (ln, 2) and np.max(np.abs(det - trk[:ln])) < 1e-12
    obj = planner._Base.__new__(planner._Base)
    obj.beta, obj.dt, obj.step_gap = beta, 0.4, 0.3
    obj.sigma = beta / np.tanh(0.4 * beta / 2)
    assert abs(obj.sigma - g["sigma"]) < 1e-12
    for vx, leg, ex, ey in g["alip_des_vel"]:
        assert np.allclose(obj.alip_des_vel(vx, leg), [ex, ey], rtol=0, atol=1e-14)
    A, B = planner._alip_matrices(beta, 0.4, 0.4)
    obj.A = A
    obj.inv_B_vel_shr = np.linalg.inv(B[2:4, 0:2])
    for inp, out in zip(g["cfv_in"], g["cfv_out"]):
        assert np.allclose(obj.cal_foot_with_veldes(inp[:5], inp[5:]), out, rtol=0, atol=1e-12)
    for h, v0, out in zip(g["tube_in"], g["tube_init"], g["tube_out"]):
        assert np.allclose(obj.tube_func(h, v0), out, rtol=0, atol=1e-15)


def test_sup_learn_state_projection_is_bit_exact(golden):
    """get_next_states reproduces the logged x_nex of every recorded MPC call exactly."""
    d = golden("g3_sup_learn")
    assert np.max(np.abs(d["x_nex"][:, :2] - d["x_nex_logged"])) == 0.0


def test_scene_generator_distribution():
    from alipmpc import scenes
    bt = scenes.make_batch(200, seed=1, n_cir=5)
    assert bt["cir"].shape == (200, 5, 3) and np.all(bt["nc"] == 5)
    r = bt["cir"][:, :, 2] - scenes.SAFE_DIS
    assert r.min() >= 0.35 - 1e-12 and r.max() <= 1.0 + 1e-12
    assert bt["cir"][:, :, :2].min() >= 0 and bt["cir"][:, :, :2].max() <= 8.5
    for b in range(200):
        c = bt["cir"][b]
        d = np.hypot(*(bt["x0"][b, :2] - c[:, :2]).T)
        assert np.all(d >= c[:, 2] + 0.2 - 1e-12)
        for i in range(5):
            for j in range(i):
                ri, rj = c[i, 2] - 0.4, c[j, 2] - 0.4
                assert np.hypot(*(c[i, :2] - c[j, :2])) >= ri + rj + 1.6 - 1e-9
    vb = np.cos(bt["x0"][:, 4]) * bt["x0"][:, 2] + np.sin(bt["x0"][:, 4]) * bt["x0"][:, 3]
    assert vb.min() >= 0.45 - 1e-12 and vb.max() <= 0.75 + 1e-12
    assert np.array_equal(bt["u0"], np.tile(bt["x0"], (1, 3)))
    mix = scenes.make_batch(20, seed=2, n_cir=5, n_elp=5, N=5)
    assert mix["elp"].shape == (20, 5, 5) and mix["u0"].shape == (20, 25)


def _shard_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from alipmpc import sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    B = 10
    lo, hi = sharding.shard_range(B, rank, world)
    local = torch.arange(lo, hi, dtype=torch.float64).reshape(-1, 1).repeat(1, 3)
    full = sharding.gather_to_root(local, B, rank, world)
    if rank == 0:
        q.put(full.numpy().tolist())
    dist.destroy_process_group()


def test_sharding_and_gather_gloo_world2():
    import multiprocessing as mp
    import socket
    from alipmpc import sharding
    assert [sharding.shard_range(10, r, 3) for r in range(3)] == [(0, 4), (4, 7), (7, 10)]
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    full = np.array(q.get(timeout=120))
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(full[:, 0], np.arange(10))


def _bench_worker(rank, world, port, B_total, q):
    """bench.py's step / gather loop and its quality all-reduce with a stub solver on CPU tensors."""
    import torch
    import torch.distributed as dist
    import bench
    from alipmpc import sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = sharding.shard_range(B_total, rank, world)
    B, n = hi - lo, 15
    out = {"u": torch.empty((B, n), dtype=torch.float64), "foot": torch.empty((B, 3), dtype=torch.float64),
           "status": torch.empty(B, dtype=torch.int32), "iters": torch.empty(B, dtype=torch.int32)}
    calls = []

    def solve():   # stub "solver output": a function of the global instance index
        g = torch.arange(lo, hi, dtype=torch.float64)
        out["u"][:] = g[:, None] * 100 + torch.arange(n, dtype=torch.float64)
        out["foot"][:] = -g[:, None]
        out["status"][:] = (torch.arange(lo, hi) % 3).to(torch.int32) - 1
        out["iters"][:] = torch.arange(lo, hi).to(torch.int32) + 7
        calls.append(1)
    step = bench.make_step(solve, out, n, B_total, rank, world)
    elapsed, ev = bench.timed_loop(step, 1, 3, world, torch.device("cpu"))
    full = step()
    qc = bench.quality_counts(rank + 1, out["status"], torch.device("cpu"), world)
    if rank == 0:
        q.put((full.numpy().tolist(), qc, len(calls), elapsed))
    dist.destroy_process_group()


@pytest.mark.parametrize("B_total", [11, 64])
def test_bench_step_gather_loop_gloo_world2(B_total):
    """bench.py at N = 2 ranks: every step solves the rank's contiguous shard and gathers the packed
    outputs to rank 0 with sharding.gather_to_root (the benched collective), uneven shards padded
    (B_total = 11 -> 6 + 5, as cfg4's total split over ranks that do not divide it); the quality counts
    are summed over ranks."""
    import multiprocessing as mp
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_bench_worker, args=(r, 2, port, B_total, q)) for r in range(2)]
    for p in ps:
        p.start()
    full, qc, ncalls, elapsed = q.get(timeout=180)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    full = np.array(full)
    g = np.arange(B_total, dtype=float)
    assert full.shape == (B_total, 15 + 5)
    assert np.array_equal(full[:, :15], g[:, None] * 100 + np.arange(15))
    assert np.array_equal(full[:, 15:18], np.repeat(-g[:, None], 3, 1))
    assert np.array_equal(full[:, 18], g % 3 - 1)
    assert np.array_equal(full[:, 19], g + 7)
    assert ncalls == 1 + 3 + 1 and elapsed > 0
    st = g % 3 - 1
    assert qc["instances"] == B_total
    assert qc["feasible_fraction"] == pytest.approx(3 / B_total)     # 1 + 2 over the two ranks
    assert qc["converged_fraction"] == pytest.approx(np.isin(st, [0, 1]).mean())
    assert qc["solved_fraction"] == pytest.approx((st == 0).mean())


def _stub_outputs(inp, n):
    """An index-free stand-in for the solver: per-instance outputs computed from the instance's own inputs only."""
    import torch
    x0 = torch.from_numpy(inp["x0"])
    cir = torch.from_numpy(inp["cir"]).reshape(x0.shape[0], -1)
    u = torch.cat([x0, x0 * 2.0, x0 * 3.0], dim=1)[:, :n] + cir.sum(dim=1, keepdim=True)
    foot = torch.stack([cir[:, 0], cir[:, 1], torch.from_numpy(inp["goal"][:, 0])], dim=1)
    status = torch.from_numpy(inp["leg"].astype(np.int32))
    iters = torch.from_numpy(inp["nc"].astype(np.int32)) + 3
    return {"u": u.contiguous(), "foot": foot.contiguous(), "status": status, "iters": iters}


def _world_inputs_worker(rank, world, port, total, block, q):
    """bench.py's strong-scaling input path at world size `world`: the rank's shard from (seed, global index)
    blocks, a stub solve, one gather to rank 0."""
    import torch
    import torch.distributed as dist
    import bench
    from alipmpc import sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = sharding.shard_range(total, rank, world)
    inp = bench.global_inputs("cfg4", lo, hi, block, 0, 5, 0, 3)
    out = _stub_outputs(inp, 15)
    step = bench.make_step(lambda: None, out, 15, total, rank, world)
    full = step()
    if rank == 0:
        q.put(full.numpy().tolist())
    dist.destroy_process_group()


def test_strong_scaling_inputs_identical_across_world_sizes_gloo():
    """SURVEY 8e / VERDICT r2: instances come from (seed, global index), so the gathered world-2 outputs of the
    strong-scaling configs (cfg4 / cfg5 shards) equal the world-1 outputs bit for bit (real scene generator, a
    stub solver that depends only on each instance's inputs).  Uneven shards (101 + 100 of 201) cut a block."""
    import multiprocessing as mp
    import socket
    import bench
    total, block = 201, 64
    ref = _stub_outputs(bench.global_inputs("cfg4", 0, total, block, 0, 5, 0, 3), 15)
    ref = bench.pack_outputs(ref, 15).numpy()
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_world_inputs_worker, args=(r, 2, port, total, block, q)) for r in range(2)]
    for p in ps:
        p.start()
    full = np.array(q.get(timeout=180))
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert full.shape == ref.shape and np.array_equal(full, ref)
    # and every config runs one program whatever the world size
    assert all(c["program"] in ("wave", "lane") for c in bench.CONFIGS.values())


def test_bench_bound_label_from_counters():
    """The bench line's roofline `bound` is read off the profiled build's counters: the
    cfg2 / cfg3 / cfg4 counter shares of profiles/r4/r4h, and the label without counters."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    assert bench.bound_label("wave", {"mfma_busy_share": 0.055, "valu_issue_frac": 0.464}) == "latency"   # cfg2
    assert bench.bound_label("wave", {"mfma_busy_share": 0.089, "valu_issue_frac": 0.646}) == "valu"      # cfg3
    assert bench.bound_label("lane", {"mfma_busy_share": 0.0, "valu_issue_frac": 0.396}) == "latency"     # cfg4
    assert bench.bound_label("wave", {"mfma_busy_share": 0.6, "valu_issue_frac": 0.7}) == "mfma"
    assert bench.bound_label("lane", {}) == "valu" and bench.bound_label("wave", {}) == "latency"


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as float64 DIR/<name>.npy; above the size cap the same fixed, seeded,
    ascending sample of instances of every array (indices in sample_index.npy), identical from run to run."""
    import bench
    B = 50
    arrays = {"u": np.arange(B * 15, dtype=np.float64).reshape(B, 15), "foot": np.ones((B, 3)),
              "status": np.arange(B, dtype=np.int32), "iters": np.full(B, 7, np.int32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert not (tmp_path / "a" / "sample_index.npy").exists()
    for k, v in arrays.items():
        assert got[k].dtype == np.float64 and np.array_equal(got[k], v)
    row = (15 + 3 + 1 + 1 + 1) * 8                    # bytes per instance, the index included
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20 * row + 5)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    idx = np.load(tmp_path / "b" / "sample_index.npy").astype(np.int64)
    assert idx.shape == (20,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    total = 0
    for k, v in arrays.items():
        s = np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(s, v[idx]) and np.array_equal(s, np.load(tmp_path / "c" / (k + ".npy")))
        total += s.nbytes
    assert total + idx.size * 8 <= bench.DUMP_MAX_BYTES
