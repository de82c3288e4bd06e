"""The stream and capture contract of device-pointer solves (include/alipmpc.h, Conventions): a solve is asynchronous
and graph-capturable, a captured graph stays valid whatever batch sizes run on its stream afterwards, up to 8 streams
per handle hold a split-launch record buffer and a ninth runs the one-phase form with the same bits, and the handle's
64 work-queue counter pairs are a ring that solves in flight on different streams share.

The per-stream hand-off list (lane programs, fp32 wave program: the instances the fp64 wave program solves from their
start) is the one buffer here that grows.  A list too small for a batch is retired and kept until alipmpc_destroy —
it used to be freed, and a graph captured at B = 512 then wrote its count and instance indices into freed memory once a
B = 2048 solve had run on its stream.  alipmpc_dbg_handoff_lists (a test hook of the library, not part of the ABI)
reports the lists a handle owns for a stream.

Every comparison is bit for bit on u, foot, x_pred, status, iters; every device output is pre-filled with NaN (doubles)
or -99 (ints) before the launch that writes it, so a skipped instance shows.

Measured figures are written under $ALIPMPC_TEST_ARTIFACTS (streams/*.json; profiles/streams/streams.json is their
collection from one MI355X run)."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_resto_gpu import FP32_TOLS, HANDLES, KEYS, ROWS, _batch, _run, _same_rows, _solver, _take  # noqa: F401

gpu = pytest.mark.gpu

SMALL, LARGE = 512, 2048      # the captured batch and the larger eager one (ROWS' own B for rows 1 and 8 is 512)
MIN_HANDOFFS = 100            # below this a hand-off test would hardly touch the list (the oracle restores on >= 100
                              # instances of each row: test_resto_gpu.py::test_oracle_strata_hold_recovered_instances)


# ---------------------------------------------------------------------------------------------------- helpers
def _record(name, obj):
    """A small JSON record of a case's measured numbers under $ALIPMPC_TEST_ARTIFACTS/streams (if set)."""
    d = os.environ.get("ALIPMPC_TEST_ARTIFACTS")
    if d:
        d = os.path.join(d, "streams")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as fh:
            json.dump(obj, fh, indent=1)


_BATCHES = {}


def _row_batch(row, B):
    """_batch(row, B), built once per session and left unchanged."""
    if (row, B) not in _BATCHES:
        _BATCHES[row, B] = _batch(row, B=B)
    return _BATCHES[row, B]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _inputs(bt, idx=None):
    """The batch (or its rows idx, a device index tensor) as device tensors of the ABI's types."""
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(_dev()) for k, v in bt.items() if v is not None}
    d["leg"] = d["leg"].to(torch.int8)
    d["nc"] = d["nc"].to(torch.int32)
    if "ne" in d:
        d["ne"] = d["ne"].to(torch.int32)
    if idx is not None:
        d = {k: v.index_select(0, idx).contiguous() for k, v in d.items()}
    return d


def _outputs(B, N):
    """Sentinel-filled device outputs of a solve: NaN in the doubles, -99 in the ints."""
    import torch
    f = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=_dev())  # noqa: E731
    i = lambda: torch.full((B,), -99, dtype=torch.int32, device=_dev())  # noqa: E731
    return {"u": f(B, 5 * N), "foot": f(B, 3), "x_pred": f(B, N, 5), "status": i(), "iters": i()}


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _no_sentinel(o):
    """No NaN in a double output, no -99 in an int one (numpy dict)."""
    return all(not np.isnan(o[k]).any() for k in ("u", "foot", "x_pred")) and \
        all((o[k] != -99).all() for k in ("status", "iters"))


def _bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _equal_on_device(out, ref, idx=None):
    """The keys of `out` that differ, bit for bit, from `ref` (device tensors; rows idx of ref)."""
    import torch
    bad = []
    for k in KEYS:
        r = ref[k] if idx is None else ref[k].index_select(0, idx)
        if not torch.equal(_bits(out[k]), _bits(r)):
            bad.append(k)
    return bad


def _lists(s, st):
    """[(address, bytes)] of the hand-off lists the handle owns for stream st, the live one first
    (alipmpc_dbg_handoff_lists: host bookkeeping, no device access)."""
    from alipmpc import _lib
    f = s._L.alipmpc_dbg_handoff_lists
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                  ctypes.c_int]
    f.restype = ctypes.c_int
    cap = 16
    a, b = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)()
    n = f(s._h, _lib._stream_arg(st), a, b, cap)
    assert 0 <= n <= cap, n
    return [(int(a[i]), int(b[i])) for i in range(n)]


def _count_at(s, addr):
    """The count word of the hand-off list at device address addr (a list the handle still owns), read with the HIP
    runtime the library itself is linked to.  The caller has synchronised."""
    try:
        f = s._L.hipMemcpy
    except AttributeError:
        f = ctypes.CDLL("libamdhip64.so").hipMemcpy
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    f.restype = ctypes.c_int
    c = ctypes.c_uint32(0xFFFFFFFF)
    rc = f(ctypes.byref(c), ctypes.c_void_p(addr), 4, 2)   # hipMemcpyDeviceToHost
    assert rc == 0, rc
    return int(c.value)


_HOST_REF = {}


def _host_ref(gpu_lib, name, B):
    """(host-mode outputs, lane_handoffs) of the handle's row at batch size B, on a handle of its own; once per
    session."""
    if (name, B) not in _HOST_REF:
        row, kw, _ = HANDLES[name]
        s = _solver(gpu_lib, row, **kw)
        o = _run(s, _row_batch(row, B))
        _HOST_REF[name, B] = (o, s.lane_handoffs())
    return _HOST_REF[name, B]


def _wave_cfg(gpu_lib):
    return gpu_lib.default_cfg(0, 3, nc_max=5, ne_max=0)


_WAVE = {}


def _wave_case(gpu_lib):
    """(batch, host-mode outputs on a handle of its own) of the fp64 wave handle at B = 1000; once per session."""
    if not _WAVE:
        from alipmpc import scenes
        bt = scenes.make_batch_vec(1000, seed=61, n_cir=5, N=3)
        _WAVE["bt"] = bt
        _WAVE["ref"] = _run(gpu_lib.Solver(_wave_cfg(gpu_lib)), bt)
    return _WAVE["bt"], _WAVE["ref"]


# ---------------------------------------------------------------------------------------------------- a. ownership
@gpu
@pytest.mark.parametrize("name", sorted(HANDLES))
def test_handoff_list_a_capture_could_hold_stays_owned(gpu_lib, name):
    """A B = 512 solve on a fresh stream leaves one hand-off list of at least 4 * 513 bytes at address A.  A B = 2048
    solve on that stream needs a larger one: the live list then holds at least 4 * 2049 bytes, A is STILL among the
    handle's lists for the stream (a graph captured in between would hold A), and the retired lists sum to less than
    the live one.  No kernel touches a freed buffer here, whatever the library's policy: the test reads the host's
    bookkeeping.  Both solves equal the host-mode bits."""
    import torch
    row, kw, _ = HANDLES[name]
    N = ROWS[row][1]
    s = _solver(gpu_lib, row, **kw)
    small, big = _inputs(_row_batch(row, SMALL)), _inputs(_row_batch(row, LARGE))
    o1, o2 = _outputs(SMALL, N), _outputs(LARGE, N)
    st = torch.cuda.Stream(device=_dev())
    assert _lists(s, st) == []
    torch.cuda.synchronize()
    s.solve_device(small, o1, stream=st)
    l1 = _lists(s, st)
    assert len(l1) == 1 and l1[0][0] != 0 and l1[0][1] >= 4 * (SMALL + 1), l1
    A = l1[0][0]
    s.solve_device(big, o2, stream=st)
    l2 = _lists(s, st)
    _record(f"owned_{name}", {"handle": name, "row": row, "lists_after_B512": l1, "lists_after_B2048": l2, "calls": 2,
                              "launches": {str(B): s.solve_launches(B)[0] for B in (SMALL, LARGE)}})
    assert l2[0][1] >= 4 * (LARGE + 1), l2
    assert A in [a for a, _ in l2], (A, l2)
    # (an allocator may hand a freed address out again: A counts as owned only as the very list it was — retired
    # behind a new live one, or still live because the first list was large enough and nothing grew)
    assert (l1[0] in l2[1:]) if l2[0] != l1[0] else (l2 == l1), (l1, l2)
    assert len({a for a, _ in l2}) == len(l2), l2
    assert sum(b for _, b in l2[1:]) < l2[0][1], l2
    torch.cuda.synchronize()
    for o, B in ((o1, SMALL), (o2, LARGE)):
        o, ref = _host(o), _host_ref(gpu_lib, name, B)[0]
        assert _no_sentinel(o)
        assert _same_rows(o, ref).all(), (B, np.flatnonzero(~_same_rows(o, ref)))


# ---------------------------------------------------------------------------------------------------- b. the replay
@gpu
@pytest.mark.parametrize("name", sorted(HANDLES))
def test_handoff_graph_capture_keeps_its_list(gpu_lib, name):
    """test_gpu.py::test_split_launch_graph_capture_keeps_its_records for the hand-off list: an eager B = 512 solve on
    a stream, the same solve captured into a graph, an eager B = 2048 solve on the stream (the list grows), the
    captured outputs overwritten with -7, then the replay.  The replay's memset node, lane (or fp32 wave) kernel and
    hand-off kernel hold the list the capture saw, which the handle still owns (the test above): the replayed outputs
    equal the handle's host-mode B = 512 solve on every row, and the count the replay left in ITS list — read at the
    captured address — is that solve's lane_handoffs(), at least 100.  alipmpc_lane_handoffs(st) reads the stream's
    current list (include/alipmpc.h), which the replay does not write: it still reports the B = 2048 solve's count.
    The B = 2048 outputs equal their host-mode solve too, with no sentinel left."""
    import torch
    row, kw, _ = HANDLES[name]
    N = ROWS[row][1]
    s = _solver(gpu_lib, row, **kw)
    bt_s, bt_l = _row_batch(row, SMALL), _row_batch(row, LARGE)
    ref_s = _run(s, bt_s)
    h_s = s.lane_handoffs()
    ref_l = _run(s, bt_l)
    h_l = s.lane_handoffs()
    assert h_s >= MIN_HANDOFFS, h_s
    small, big = _inputs(bt_s), _inputs(bt_l)
    og, ob = _outputs(SMALL, N), _outputs(LARGE, N)
    st = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s.solve_device(small, og)       # the capture stream's first solve: allocates its hand-off list
    st.synchronize()
    assert s.lane_handoffs(st) == h_s and _same_rows(_host(og), ref_s).all()
    captured = _lists(s, st)
    assert len(captured) == 1 and captured[0][1] >= 4 * (SMALL + 1), captured
    for v in og.values():
        v.fill_(float("nan") if v.dtype == torch.float64 else -99)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        s.solve_device(small, og)
    assert _lists(s, st) == captured    # (a capture neither allocates nor retires)
    with torch.cuda.stream(st):
        s.solve_device(big, ob)         # a larger batch on the capture stream: the list grows
        for v in og.values():
            v.fill_(-7)
        g.replay()
    torch.cuda.synchronize()
    after = _lists(s, st)
    count_replayed = _count_at(s, captured[0][0]) if captured[0][0] in [a for a, _ in after] else None
    h_live = s.lane_handoffs(st)
    o_g, o_b = _host(og), _host(ob)
    _record(f"replay_{name}", {"handle": name, "row": row, "handoffs_B512": h_s, "handoffs_B2048": h_l,
                               "count_in_captured_list_after_replay": count_replayed,
                               "lane_handoffs_after_replay": h_live, "lists_at_capture": captured,
                               "lists_after_B2048": after, "calls": 3 + 1,
                               "rows_equal_replay": int(_same_rows(o_g, ref_s).sum()),
                               "launches": {str(B): s.solve_launches(B)[0] for B in (SMALL, LARGE)}})
    assert captured[0] in after[1:] and after[0][1] >= 4 * (LARGE + 1), (captured, after)
    assert _same_rows(o_g, ref_s).all(), np.flatnonzero(~_same_rows(o_g, ref_s))
    assert count_replayed == h_s, (count_replayed, h_s)
    assert h_live == h_l, (h_live, h_l)
    assert _no_sentinel(o_b) and _same_rows(o_b, ref_l).all(), np.flatnonzero(~_same_rows(o_b, ref_l))


# ---------------------------------------------------------------------------------------------------- c. the ring
RING_HANDLES = ("wave_fp64", "lane_fp32")
ROUNDS, CALLS_PER_ROUND = 3, 48     # 48 < 64 in flight (include/alipmpc.h); 144 calls wrap the ring of 64 pairs twice
UNION = 1000


def _ring_case(gpu_lib, which):
    """(fresh handle, fresh reference handle, union batch, N) of a ring test."""
    if which == "wave_fp64":
        from alipmpc import scenes
        bt = scenes.make_batch_vec(UNION, seed=63, n_cir=5, N=3)
        return gpu_lib.Solver(_wave_cfg(gpu_lib)), gpu_lib.Solver(_wave_cfg(gpu_lib)), bt, 3
    row, kw, _ = HANDLES[which]
    return _solver(gpu_lib, row, **kw), _solver(gpu_lib, row, **kw), _row_batch(row, UNION), ROWS[row][1]


@gpu
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("which", RING_HANDLES)
def test_more_solves_than_queue_pairs(gpu_lib, which, streams):
    """Three rounds of 48 device-pointer solves each, issued back to back on 1 or 3 streams of one handle with no
    synchronisation inside a round: 144 calls on a ring of 64 work-queue counter pairs, fewer than 64 in flight.  Per
    stream the calls cycle a fixed list of batch sizes from {64, 300, 1000, solve_slots() + 64} — on the fp64 wave
    handle the split launch and, above the slots, the work queue; on the lane handle a hand-off list that grows while
    launches holding the smaller ones are still queued.  Every call's batch is rows (offset + i) mod 1000 of one
    union batch; an instance's result does not depend on its batch or launch form (include/alipmpc.h), so every
    call's outputs equal those rows of ONE host-mode solve of the union batch on a handle of its own, bit for bit.
    Lane handle: lane_handoffs(stream) after each round is the count of that stream's last batch solved alone.  The
    queues are atomicAdd tickets with a bound check, nothing spin-waits: a wrong ring shows as wrong or missing rows."""
    import torch
    s, sref, bt, N = _ring_case(gpu_lib, which)
    lane = which != "wave_fp64"
    big = s.solve_slots() + 64
    sizes = [64, 300, 1000, 64, 300, big, 1000, 300, 64, 1000, 300, 64, 1000, 64, 300, 1000]
    forms = {B: s.solve_launches(B)[0] for B in sorted(set(sizes))}
    if not lane:
        assert forms[1000] == 2 and forms[big] == 1, forms      # the split launch and the work queue
    ref_np = _run(sref, bt)
    assert _no_sentinel(ref_np)
    ref = {k: torch.from_numpy(np.ascontiguousarray(ref_np[k])).to(_dev()) for k in KEYS}
    full = _inputs(bt)
    per = CALLS_PER_ROUND // streams
    # stream j's c-th call of a round: size and row offset, the same in every round
    plan = [[(sizes[(c + 5 * j) % len(sizes)], 37 * (c * streams + j)) for c in range(per)] for j in range(streams)]
    idx, inp = {}, {}
    for calls in plan:
        for B, off in calls:
            if (B, off) not in idx:
                idx[B, off] = (torch.arange(B, device=_dev()) + off) % UNION
                inp[B, off] = {k: v.index_select(0, idx[B, off]).contiguous() for k, v in full.items()}
    last_alone = {}
    if lane:
        for calls in plan:
            B, off = calls[-1]
            _run(sref, _take(bt, (np.arange(B) + off) % UNION))
            last_alone[B, off] = sref.lane_handoffs()
    sts = [torch.cuda.Stream(device=_dev()) for _ in range(streams)]
    assert len({st.cuda_stream for st in sts}) == streams
    handoffs, lists = [], []
    for rnd in range(ROUNDS):
        outs = [[_outputs(B, N) for B, _ in calls] for calls in plan]
        torch.cuda.synchronize()
        for c in range(per):
            for j, st in enumerate(sts):
                s.solve_device(inp[plan[j][c]], outs[j][c], stream=st)
        torch.cuda.synchronize()
        for j, calls in enumerate(plan):
            for c, key in enumerate(calls):
                bad = _equal_on_device(outs[j][c], ref, idx[key])
                if bad:
                    o = _host(outs[j][c])
                    rows = ~_same_rows(o, {k: ref_np[k][idx[key].cpu().numpy()] for k in KEYS})
                    assert False, (rnd, j, c, key, bad, "sentinel-free" if _no_sentinel(o) else "sentinel left",
                                   int(rows.sum()), np.flatnonzero(rows)[:16])
        if lane:
            got = [s.lane_handoffs(st) for st in sts]
            handoffs.append(got)
            lists.append([_lists(s, st) for st in sts])
            assert got == [last_alone[calls[-1]] for calls in plan], (rnd, got, last_alone)
        del outs
    _record(f"ring_{which}_{streams}", {"handle": which, "streams": streams, "calls": ROUNDS * CALLS_PER_ROUND,
                                        "sizes": sizes, "launches": {str(k): v for k, v in forms.items()},
                                        "lane_handoffs_per_round": handoffs, "lists_per_round": lists})


# ---------------------------------------------------------------------------------------------------- d. nine streams
@gpu
def test_ninth_stream_runs_one_phase_with_the_same_bits(gpu_lib):
    """The fp64 wave handle's B = 1000 solve is a split launch (2 launches).  Eight streams get a record buffer each;
    the ninth has none and runs the one-phase form.  All nine outputs equal the host-mode solve bit for bit, and so do
    second solves on the first and on the ninth stream."""
    import torch
    bt, ref = _wave_case(gpu_lib)
    s = gpu_lib.Solver(_wave_cfg(gpu_lib))
    assert s.solve_launches(1000)[0] == 2
    inp = _inputs(bt)
    sts = [torch.cuda.Stream(device=_dev()) for _ in range(9)]
    assert len({st.cuda_stream for st in sts}) == 9 and all(st.cuda_stream != 0 for st in sts)
    calls = 0
    for j in list(range(9)) + [0, 8]:
        o = _outputs(1000, 3)
        torch.cuda.synchronize()
        s.solve_device(inp, o, stream=sts[j])
        torch.cuda.synchronize()
        calls += 1
        o = _host(o)
        assert _no_sentinel(o) and _same_rows(o, ref).all(), (j, calls, np.flatnonzero(~_same_rows(o, ref)))
    _record("nine_streams", {"handle": "wave_fp64", "B": 1000, "streams": 9, "calls": calls,
                             "launches": {"1000": s.solve_launches(1000)[0]}})


# ---------------------------------------------------------------------------------------------------- e. capture first
@gpu
def test_capture_as_a_streams_first_solve(gpu_lib):
    """A capture on a stream that has never solved records the one-phase form (no allocation inside a capture); its
    replay equals the host-mode bits.  An eager solve on that stream then allocates the record buffer and runs the
    split form; the graph, replayed again, still computes the same bits."""
    import torch
    bt, ref = _wave_case(gpu_lib)
    s = gpu_lib.Solver(_wave_cfg(gpu_lib))
    assert s.solve_launches(1000)[0] == 2
    inp = _inputs(bt)
    og, oe = _outputs(1000, 3), _outputs(1000, 3)
    st = torch.cuda.Stream(device=_dev())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        s.solve_device(inp, og)
    torch.cuda.synchronize()
    assert not _no_sentinel(_host(og))      # (captured, not run)

    def replay():
        with torch.cuda.stream(st):
            for v in og.values():
                v.fill_(float("nan") if v.dtype == torch.float64 else -99)
            g.replay()
        torch.cuda.synchronize()
        o = _host(og)
        assert _no_sentinel(o) and _same_rows(o, ref).all(), np.flatnonzero(~_same_rows(o, ref))

    replay()
    with torch.cuda.stream(st):
        s.solve_device(inp, oe)             # eager: the stream's record buffer, the split form
    torch.cuda.synchronize()
    o = _host(oe)
    assert _no_sentinel(o) and _same_rows(o, ref).all(), np.flatnonzero(~_same_rows(o, ref))
    replay()
    _record("capture_first", {"handle": "wave_fp64", "B": 1000, "calls": 2, "replays": 2,
                              "launches": {"1000": s.solve_launches(1000)[0]}})
