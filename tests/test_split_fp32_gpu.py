"""The fp32 wave program's split launch with cfg.restoration = IPOPT: zero the record header, zero the hand-off list,
phase 1, phase 2, then the fp64 work queue over the listed instances (csrc/solve_plan.inc).  Phase 1 starts the list and
phase 2 continues it, and the record holds an instance's whole loop state, so status, iters, u, foot and x_pred equal the
one-phase form's (ALIPMPC_SPLIT_IT=0, ALIPMPC_SPLIT_TR=0) bit for bit.  Small batches in which every other instance is a
copy of an infeasible scene, whose line search fails and which is therefore handed off.  modi, N = 3, 5 circle slots,
through the C ABI, a fresh handle per form (the cuts are read when the handle is made)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("status", "iters", "u", "foot", "x_pred")
_big = {}


def _solver(gpu_lib, monkeypatch, split):
    for v in ("ALIPMPC_SPLIT_IT", "ALIPMPC_SPLIT_TR"):
        if split:
            monkeypatch.delenv(v, raising=False)
        else:
            monkeypatch.setenv(v, "0")
    return gpu_lib.Solver(gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0, precision=gpu_lib.PREC_FP32))


def _solve(s, bt):
    return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=bt["u0"])


def _scenes(gpu_lib, monkeypatch):
    """1024 scenes with their one-phase status, computed once for the module"""
    if not _big:
        from alipmpc import scenes
        _big["bt"] = scenes.make_batch(1024, seed=77, n_cir=5)
        _big["status"] = _solve(_solver(gpu_lib, monkeypatch, False), _big["bt"])["status"]
    return _big["bt"], _big["status"]


@pytest.mark.parametrize("B", [9, 64])
def test_fp32_split_with_handoff_equals_one_phase(gpu_lib, monkeypatch, B):
    big, st = _scenes(gpu_lib, monkeypatch)
    bad, good = np.flatnonzero(st == 2), np.flatnonzero(st == 0)
    assert len(bad) >= 1 and len(good) >= B
    idx = np.where(np.arange(B) % 2 == 0, bad[0], good[:B])
    bt = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in big.items()}
    one = _solver(gpu_lib, monkeypatch, False)
    assert one.solve_launches(B)[0] == 1
    ref = _solve(one, bt)
    # status 2 comes out of the restoration phase alone, which the fp32 program does not have: those were handed off
    assert (ref["status"][0::2] == 2).all() and one.lane_handoffs() >= (B + 1) // 2
    two = _solver(gpu_lib, monkeypatch, True)
    assert two.solve_slots() >= B and two.solve_launches(B) == (2, 1)
    o = _solve(two, bt)
    assert two.lane_handoffs() == one.lane_handoffs()
    for k in KEYS:
        assert np.array_equal(o[k], ref[k]), (B, k)
