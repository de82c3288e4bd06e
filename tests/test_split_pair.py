"""The paired phase 2 of the split launch (fp64, cfg.restoration = IPOPT): phase 1 lists its records in two classes
(cut with a restoration pending / cut at the iteration cap) and phase 2 runs 8-wave workgroups whose owner waves 0-3
take the pending records and whose filler waves 4-7 take regular ones.  Which wave resumes a record never changes its
arithmetic: every output equals the one-phase launch's (ALIPMPC_SPLIT_IT=0) and the 4-wave phase 2's
(ALIPMPC_SPLIT_PAIR=0) bit for bit.  All fp64 modi, N = 3, 5 circle slots, through the C ABI."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("status", "iters", "u", "foot", "x_pred")


def _cfg(gpu_lib):
    return gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0)


def _solve(gpu_lib, monkeypatch, bt, cut, pair, check=None):
    """One solve with the given cut (None: the default) and phase-2 form, on a fresh handle (both are read at create)."""
    if cut is None:
        monkeypatch.delenv("ALIPMPC_SPLIT_IT", raising=False)
    else:
        monkeypatch.setenv("ALIPMPC_SPLIT_IT", str(cut))
    monkeypatch.setenv("ALIPMPC_SPLIT_PAIR", "1" if pair else "0")
    monkeypatch.setenv("ALIPMPC_SPLIT_TR", "0")
    s = gpu_lib.Solver(_cfg(gpu_lib))
    if check:
        check(s)
    return s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=bt["u0"])


def _same(o, ref, what):
    for k in KEYS:
        assert np.array_equal(o[k], ref[k]), (what, k)


def _against_both(gpu_lib, monkeypatch, bt, cuts, check=None):
    """The paired form at every cut against the one-phase launch and against the 4-wave phase 2 at the same cut."""
    ref = _solve(gpu_lib, monkeypatch, bt, 0, True)
    for cut in cuts:
        o = _solve(gpu_lib, monkeypatch, bt, cut, True, check)
        _same(o, ref, ("one-phase", cut))
        _same(o, _solve(gpu_lib, monkeypatch, bt, cut, False, check), ("4-wave phase 2", cut))
    return ref


def test_pair_cuts(gpu_lib, monkeypatch):
    """Cut 1: no pending records, every instance a regular one.  Cuts 9 and 11: both classes, and fillers whose own
    search fails later.  Cut 16 and max_iter - 1: mostly pending records."""
    from alipmpc import scenes
    bt = scenes.make_batch(1024, seed=77, n_cir=5)
    max_iter = _cfg(gpu_lib).max_iter
    ref = _against_both(gpu_lib, monkeypatch, bt, (1, 9, 11, 16, max_iter - 1))
    assert (ref["status"] == 2).sum() > 0 and (ref["iters"] > 16).sum() > 0


@pytest.mark.parametrize("B", [2, 5, 9])
def test_pair_small_batches(gpu_lib, monkeypatch, B):
    """The smallest split, a pending count that is no multiple of 4, and one workgroup holding both classes with
    empty waves: B instances of which every other one is a copy of an infeasible scene."""
    from alipmpc import scenes
    big = scenes.make_batch(1024, seed=77, n_cir=5)
    st = _solve(gpu_lib, monkeypatch, big, 0, True)["status"]
    bad, good = np.flatnonzero(st == 2), np.flatnonzero(st == 0)
    assert len(bad) >= B and len(good) >= B
    idx = np.where(np.arange(B) % 2 == 0, bad[:B], good[:B])
    bt = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in big.items()}
    ref = _against_both(gpu_lib, monkeypatch, bt, (3, 11, None))
    assert (ref["status"] == 2).sum() == (B + 1) // 2


def test_pair_no_pending_records(gpu_lib, monkeypatch):
    """No obstacle, no failed search: the owner waves fall through to regular records."""
    from alipmpc import scenes
    bt = scenes.make_batch(300, seed=78, n_cir=0, nc_max=5)
    ref = _against_both(gpu_lib, monkeypatch, bt, (2, 5))
    assert (ref["status"] == 2).sum() == 0 and (ref["iters"] > 5).sum() > 0


def test_pair_pending_outnumber_regular(gpu_lib, monkeypatch):
    """B = 64 copies of one infeasible instance: 64 pending records, no regular one; the launch stays at two
    dispatches and within the slots."""
    from alipmpc import scenes
    big = scenes.make_batch(1024, seed=77, n_cir=5)
    st = _solve(gpu_lib, monkeypatch, big, 0, True)
    B = 64
    # (cut 2 makes regular records of the copies, the later cuts pending ones)
    bad = np.flatnonzero(st["status"] == 2)
    idx = np.full(B, bad[0])
    bt = {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in big.items()}

    def check(s):
        assert s.solve_slots() >= B
        assert s.solve_launches(B)[0] == 2

    ref = _against_both(gpu_lib, monkeypatch, bt, (2, 16, None), check)
    assert (ref["status"] == 2).all() and (ref["iters"] == ref["iters"][0]).all()


def test_pair_graph_capture_keeps_its_records(gpu_lib, monkeypatch):
    """A paired split solve captured into a HIP graph at B = 1000, an eager B = 4000 solve on the capture stream, then
    the replay: the stream's record buffer (records, instance ids and the two class lists, sized once for the slots)
    is still the captured one, and the replay's outputs equal an eager B = 1000 solve's bit for bit."""
    import torch
    from alipmpc import scenes
    monkeypatch.setenv("ALIPMPC_SPLIT_PAIR", "1")
    monkeypatch.setenv("ALIPMPC_SPLIT_TR", "0")
    monkeypatch.delenv("ALIPMPC_SPLIT_IT", raising=False)
    s = gpu_lib.Solver(_cfg(gpu_lib))
    assert s.solve_launches(1000)[0] == 2 and s.solve_launches(4000)[0] == 2
    dev = torch.device("cuda", 0)

    def inputs(B, seed):
        bt = scenes.make_batch_vec(B, seed=seed, n_cir=5, N=3)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in bt.items() if v is not None}
        d["leg"] = d["leg"].to(torch.int8)
        d["nc"] = d["nc"].to(torch.int32)
        return d

    def outputs(B):
        f = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
        return {"u": f(B, 15), "foot": f(B, 3), "x_pred": f(B, 3, 5),
                "status": torch.full((B,), -99, dtype=torch.int32, device=dev),
                "iters": torch.full((B,), -99, dtype=torch.int32, device=dev)}
    small, big = inputs(1000, 61), inputs(4000, 62)
    ref = outputs(1000)
    s.solve_device(small, ref)
    torch.cuda.synchronize()
    assert (ref["status"] == 2).sum() > 0
    st = torch.cuda.Stream()
    og = outputs(1000)
    with torch.cuda.stream(st):
        s.solve_device(small, og)       # the capture stream's first solve: allocates its record buffer
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        s.solve_device(small, og)
    ob = outputs(4000)
    with torch.cuda.stream(st):
        s.solve_device(big, ob)         # a larger batch on the capture stream
        for v in og.values():
            v.fill_(-7)
        g.replay()
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(og[k], ref[k]), k
    assert (ob["status"] != -99).all()
    # the 4-wave phase 2 on another handle computes the same bits
    monkeypatch.setenv("ALIPMPC_SPLIT_PAIR", "0")
    o4 = outputs(1000)
    gpu_lib.Solver(_cfg(gpu_lib)).solve_device(small, o4)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(o4[k], ref[k]), k
