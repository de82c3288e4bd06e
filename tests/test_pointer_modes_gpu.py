"""Host-pointer mode against device-pointer mode of the C ABI, bit for bit, where the other GPU tests leave a gap.

Every entry point takes its arrays either as host pointers (hip_stream NULL: staged through the handle's buffers,
synchronous) or as device pointers (asynchronous on the given stream).  Both run the same kernels on the same values, so
every output must be identical — also with outputs left out, with B = 67 (odd: the 67-byte int8 areas leave the alignment
of every following staged area to the staging code; not a multiple of the four instances per workgroup), without ellipse
slots, for the DD variant, and when one handle's staging buffer grows and is reused across calls of different shapes.

The calls go through the binding's private Solver._L / _lib._ptr / _lib._stream_arg so that outputs can be left out in
host mode too and nominal gait (which has no *_device wrapper) can run on device pointers.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 67
S, F, KICK, SEED = 2, 3, 0.05, 7


class Arr:
    """An array argument: a numpy array or None; `name`: it is an output, returned under that name."""

    def __init__(self, a, name=None):
        self.a = None if a is None else np.ascontiguousarray(a)
        self.name = name


def _abi(s, fn, args, host):
    """Call s._L.<fn>(handle, *args, stream): host=True passes numpy copies and a NULL stream, host=False passes CUDA
    tensors and the current stream.  Returns the outputs as numpy arrays."""
    import torch
    from alipmpc._lib import _ptr, _stream_arg
    keep, outs, cargs = [], {}, []
    for a in args:
        if not isinstance(a, Arr):
            cargs.append(a)
            continue
        if a.a is None:
            cargs.append(None)
            continue
        v = a.a.copy() if host else torch.from_numpy(a.a.copy()).cuda()
        keep.append(v)
        cargs.append(_ptr(v))
        if a.name:
            outs[a.name] = v
    st = None if host else _stream_arg(torch.cuda.current_stream())
    s._check(getattr(s._L, fn)(s._h, *cargs, st), fn)
    if not host:
        torch.cuda.synchronize()
    return {k: (v if host else v.cpu().numpy()) for k, v in outs.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def _both(s, fn, args):
    h, d = _abi(s, fn, args, True), _abi(s, fn, args, False)
    _same(h, d)
    return h


def _z(*shape, dtype=np.float64):
    return np.zeros(shape, dtype)


def _scene(bt, u=None):
    """x0, goal, leg, cir, nc, elp, ne[, u]: the scene inputs in the ABI's order"""
    a = [Arr(bt["x0"]), Arr(bt["goal"]), Arr(bt.get("leg")), Arr(bt["cir"]), Arr(bt["nc"]), Arr(bt.get("elp")),
         Arr(bt.get("ne"))]
    return a if u is None else a + [Arr(u)]


def _solve_args(s, bt, n=None, want=("u", "foot", "x_pred", "status", "iters")):
    n = bt["x0"].shape[0] if n is None else n
    N, sd = s.cfg.N, s.sdim
    o = dict(u=_z(n, s.n), foot=_z(n, 3), x_pred=_z(n, N, sd), status=_z(n, dtype=np.int32), iters=_z(n, dtype=np.int32))
    cut = {k: (None if v is None else v[:n]) for k, v in bt.items()}
    return [n] + _scene(cut, cut["u0"]) + [Arr(cut.get("last_u"))] + \
           [Arr(o[k] if k in want else None, k) for k in ("u", "foot", "x_pred", "status", "iters")]


EVAL_OUT = ("f", "grad", "c", "J", "cl", "cu", "goal_eff", "row_active")


def _eval_args(s, bt, u, want):
    n, mm = bt["x0"].shape[0], s.m_max
    o = dict(f=_z(n), grad=_z(n, s.n), c=_z(n, mm), J=_z(n, mm, s.n), cl=_z(n, mm), cu=_z(n, mm), goal_eff=_z(n, 2),
             row_active=_z(n, mm, dtype=np.int8))
    return [n] + _scene(bt, u) + [Arr(bt.get("last_u"))] + [Arr(o[k] if k in want else None, k) for k in EVAL_OUT]


def _rollout_args(s, bt, want):
    n, sd = bt["x0"].shape[0], s.sdim
    o = dict(foot=_z(n, S, 3), x=_z(n, S + 1, sd), status=_z(n, S, dtype=np.int32), iters=_z(n, S, dtype=np.int32),
             steps_to_goal=_z(n, dtype=np.int32), u=_z(n, S, s.n))
    return [n, S] + _scene(bt, bt["u0"]) + [Arr(bt.get("last_u"))] + \
           [Arr(o[k] if k in want else None, k) for k in ("foot", "x", "status", "iters", "steps_to_goal", "u")]


CL_OUT = ("foot", "x", "hd", "status", "iters", "steps_to_goal", "action")


def _loop_args(bt, foot0, want=CL_OUT):
    n = bt["x0"].shape[0]
    o = dict(foot=_z(n, S, 3), x=_z(n, S + 1, 5), hd=_z(n, S, 2), status=_z(n, S, F, dtype=np.int32),
             iters=_z(n, S, F, dtype=np.int32), steps_to_goal=_z(n, dtype=np.int32), action=_z(n, S, F, 8))
    sc = _scene(bt)
    return [n, S, F, KICK, SEED, sc[0], Arr(foot0)] + sc[1:] + [Arr(o[k] if k in want else None, k) for k in CL_OUT]


@pytest.fixture(scope="module")
def mix(gpu_lib):
    """modi, N = 3, wave program, fp64, two circle slots and one ellipse slot; 67 scenes and the foothold of a first solve"""
    from alipmpc import scenes
    cfg = gpu_lib.default_cfg(gpu_lib.VARIANT_MODI, 3, nc_max=2, ne_max=1)
    bt = scenes.make_batch(B, 11, n_cir=2, n_elp=1)
    s = gpu_lib.Solver(cfg)
    sol = s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], bt["elp"], bt["ne"], u0=bt["u0"])
    return dict(cfg=cfg, s=s, bt=bt, sol=sol, foot0=sol["foot"][:, 0:2].copy())


@pytest.mark.parametrize("want", [EVAL_OUT, tuple(k for k in EVAL_OUT if k != "J"), ("f",)], ids=["all", "no_J", "f"])
def test_eval(mix, want):
    """with J, without J, and f alone: in host mode too the kernel gets a null pointer for an output left out"""
    s, bt = mix["s"], mix["bt"]
    u = bt["u0"] + 0.01 * np.random.default_rng(3).standard_normal(bt["u0"].shape)
    o = _both(s, "alipmpc_eval_batch", _eval_args(s, bt, u, want))
    assert set(o) == set(want) and np.all(np.isfinite(o["f"]))
    if want != EVAL_OUT:   # an output's values do not depend on which others are asked for
        full = _abi(s, "alipmpc_eval_batch", _eval_args(s, bt, u, EVAL_OUT), True)
        _same(o, {k: full[k] for k in o})


def test_solve_u_alone(mix):
    """a solve with every optional output left out: the same u as the full solve, in both modes"""
    s, bt = mix["s"], mix["bt"]
    o = _both(s, "alipmpc_solve_batch", _solve_args(s, bt, want=("u",)))
    assert set(o) == {"u"} and np.array_equal(o["u"], mix["sol"]["u"], equal_nan=True)


@pytest.mark.parametrize("want", [CL_OUT, ("status",)], ids=["all", "status"])
def test_closed_loop(mix, want):
    o = _both(mix["s"], "alipmpc_closed_loop_batch", _loop_args(mix["bt"], mix["foot0"], want))
    assert set(o) == set(want)


@pytest.mark.parametrize("form", ["leg", "vel_des"])
def test_nominal_gait(mix, form):
    s, bt = mix["s"], mix["bt"]
    vin = np.random.default_rng(4).uniform(-0.3, 0.6, (B, 2))
    if form == "leg":
        args = [B, 0.6, Arr(bt["x0"]), Arr(bt["leg"]), Arr(None), Arr(_z(B, 2), "vel_des"), Arr(_z(B, 2), "foot")]
    else:
        args = [B, 0.6, Arr(bt["x0"]), Arr(None), Arr(vin), Arr(None), Arr(_z(B, 2), "foot")]
    o = _both(s, "alipmpc_nominal_gait_batch", args)
    assert np.any(o["foot"] != 0)


@pytest.mark.parametrize("want", [("x0", "goal", "leg", "cir", "nc", "elp", "ne", "u0"), ("x0", "nc")], ids=["all", "x0_nc"])
def test_scenes(mix, want):
    o = dict(x0=_z(B, 5), goal=_z(B, 2), leg=_z(B, dtype=np.int8), cir=_z(B, 2, 3), nc=_z(B, dtype=np.int32),
             elp=_z(B, 1, 5), ne=_z(B, dtype=np.int32), u0=_z(B, 15))
    args = [B, 5, 1000, 2, 1, 0, 0] + [Arr(o[k] if k in want else None, k)
                                       for k in ("x0", "goal", "leg", "cir", "nc", "elp", "ne", "u0")]
    r = _both(mix["s"], "alipmpc_scenes_batch", args)
    assert set(r) == set(want) and np.any(r["x0"] != 0)


@pytest.mark.parametrize("want", [("foot", "x", "status", "iters", "steps_to_goal", "u"), ("steps_to_goal",)],
                         ids=["all", "steps_to_goal"])
def test_rollout(mix, want):
    o = _both(mix["s"], "alipmpc_rollout_batch", _rollout_args(mix["s"], mix["bt"], want))
    assert set(o) == set(want)


def test_no_ellipse_slots(gpu_lib):
    """ne_max = 0: elp / ne are ignored, whether absent or (device pointers) valid arrays of something else"""
    from alipmpc import scenes
    s = gpu_lib.Solver(gpu_lib.default_cfg(gpu_lib.VARIANT_MODI, 3, nc_max=5, ne_max=0))
    bt = scenes.make_batch(B, 12, n_cir=5)
    assert bt["elp"] is None and bt["ne"] is None
    junk = dict(bt, elp=np.random.default_rng(5).uniform(-9, 9, (B, 1, 5)), ne=np.full(B, 3, np.int32))
    sol = _both(s, "alipmpc_solve_batch", _solve_args(s, bt))
    _same(sol, _abi(s, "alipmpc_solve_batch", _solve_args(s, junk), False))
    foot0 = sol["foot"][:, 0:2].copy()
    loop = _both(s, "alipmpc_closed_loop_batch", _loop_args(bt, foot0))
    _same(loop, _abi(s, "alipmpc_closed_loop_batch", _loop_args(junk, foot0), False))


def test_dd(gpu_lib):
    """DD: no leg, last_u given (the recipe of test_gpu._dd_batch at B = 67, in default_cfg(2)'s 6 + 6 slots)"""
    from alipmpc import scenes
    s = gpu_lib.Solver(gpu_lib.default_cfg(gpu_lib.VARIANT_DD))
    sc = scenes.make_batch(B, 13, n_cir=5, nc_max=6, ne_max=6)
    rng = np.random.default_rng(13 + 17)
    last_u = np.stack([rng.uniform(0.45, 0.75, B), rng.uniform(-0.15, 0.15, B)], 1)
    bt = dict(x0=np.stack([sc["x0"][:, 0], sc["x0"][:, 1], sc["x0"][:, 4]], 1), goal=sc["goal"], leg=None, cir=sc["cir"],
              nc=sc["nc"], elp=sc["elp"], ne=sc["ne"], last_u=last_u, u0=np.tile(last_u, (1, 3)))
    o = _both(s, "alipmpc_solve_batch", _solve_args(s, bt))
    assert np.any(o["status"] == 0)
    _both(s, "alipmpc_rollout_batch", _rollout_args(s, bt, ("foot", "x", "status", "iters", "steps_to_goal", "u")))


def test_buffer_growth_and_reuse(gpu_lib, mix):
    """one handle's staging buffer across calls of different shapes and sizes: each result is that of a fresh handle"""
    from alipmpc import scenes
    cfg = mix["cfg"]
    bt = scenes.make_batch(131, 14, n_cir=2, n_elp=1)
    b67 = {k: v[:B] for k, v in bt.items()}
    edges = np.array([0.0, 0.1])
    words = gpu_lib.audit_summary_len(len(edges))
    from alipmpc._lib import _ptr

    def audit_args(sol):
        return [B] + _scene(b67, sol["u"]) + [Arr(sol["status"]), Arr(_z(B, 5), "metrics"),
                                              Arr(_z(B, 3, dtype=np.int32), "where"), 1e-4, _ptr(edges), len(edges),
                                              Arr(np.arange(1, words + 1, dtype=np.int64), "summary")]

    def trace_args(sol):
        return [B, Arr(b67["x0"]), Arr(sol["u"]), Arr(_z(B, 3, gpu_lib.trace_len(cfg), 2), "trace")]

    one = gpu_lib.Solver(cfg)
    sol = _abi(one, "alipmpc_solve_batch", _solve_args(one, bt, B), True)
    calls = [("alipmpc_solve_batch", lambda s: _solve_args(s, bt, B)),
             ("alipmpc_trace_batch", lambda s: trace_args(sol)),
             ("alipmpc_audit_batch", lambda s: audit_args(sol)),
             ("alipmpc_solve_batch", lambda s: _solve_args(s, bt, 131)),
             ("alipmpc_solve_batch", lambda s: _solve_args(s, bt, B))]
    got = [_abi(one, fn, mk(one), True) for fn, mk in calls]
    for (fn, mk), g in zip(calls, got):
        fresh = gpu_lib.Solver(cfg)
        _same(g, _abi(fresh, fn, mk(fresh), True))
        fresh.close()
    _same(got[0], sol)
    _same(got[0], got[4])
    assert np.any(got[2]["summary"] != np.arange(1, words + 1))
