"""ctypes binding of libalipmpc.so (include/alipmpc.h).

This is the reference-side binding a Python caller of the planner would add: plain
ctypes over the C ABI, numpy arrays for host-pointer calls, torch CUDA tensors (+ the current HIP stream)
for device-pointer calls.  There is no fallback: if the library or a gfx950 device is missing, the
calls raise.
"""
import collections
import ctypes
import operator
import os

import numpy as np

from . import build as _build

VARIANT_MODI, VARIANT_SIG_STEP, VARIANT_DD = 0, 1, 2
PREC_FP64, PREC_FP32 = 0, 1
PROGRAM_WAVE, PROGRAM_LANE = 0, 1   # cfg.program: one instance per wavefront / per lane (include/alipmpc.h)
GOAL_SINGULAR_ZERO, GOAL_SINGULAR_ABORT = 0, 1   # cfg.goal_singular (include/alipmpc.h)
RESTORATION_IPOPT, RESTORATION_SUBSTITUTE = 0, 1   # cfg.restoration (include/alipmpc.h)
INVALID_NUMBER_DETECTED = -13

STATUS_NAMES = {0: "Solve_Succeeded", 1: "Solved_To_Acceptable_Level", 2: "Infeasible_Problem_Detected",
                -1: "Maximum_Iterations_Exceeded", -3: "Error_In_Step_Computation",
                -13: "Invalid_Number_Detected (cfg.goal_singular = GOAL_SINGULAR_ABORT)",
                -10: "Rollout_Done (goal reached earlier, not solved)"}
ROLLOUT_DONE = -10
TICK_NOMINAL = -20   # closed_loop_schedule: the tick ran the nominal ALIP law, no solve (ALIPMPC_TICK_NOMINAL)
TICK_FIRST_ORDER = -21   # ... the tick moved the last solve's plan to first order (ALIPMPC_TICK_FIRST_ORDER)
CL_BETWEEN_NOMINAL, CL_BETWEEN_FIRST_ORDER = 0, 1   # cfg.cl_between (include/alipmpc.h)
CL_BETWEEN_GUARDED = 3    # ... first-order ticks held against the constraint rows, re-solve on violation
CL_GUARD_VIOL = 1e-4      # ... its bar on the largest violation (ALIPMPC_CL_GUARD_VIOL)

_ERRORS = {-1: "EINVAL", -2: "ENODEV (no visible gfx950 device)", -3: "EHIP", -4: "EUNSUPPORTED"}


class Cfg(ctypes.Structure):
    """alipmpc_cfg"""
    _fields_ = [(k, ctypes.c_int32) for k in
                ("N", "nc_max", "ne_max", "variant", "max_iter", "precision", "select_obs", "detour")] + \
               [(k, ctypes.c_double) for k in
                ("tol", "acceptable_tol", "dt", "H", "g", "leg2_max", "bvx_lo", "bvx_hi", "bvy_lo", "bvy_hi",
                 "dtheta_max", "q", "p", "r", "gamma", "s", "detect_r2", "dd_t", "mu_init")] + \
               [("program", ctypes.c_int32), ("goal_singular", ctypes.c_int32), ("restoration", ctypes.c_int32),
                ("cl_between", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# ---------------------------------------------------------------- the ABI, one ordered declaration per export
# Every export of include/alipmpc.h is stated here once: its return type and its arguments in the header's order.
# load() sets the ctypes prototypes from this table, Solver._host / Solver._device build every batch call's argument
# vector from it, and tests/test_binding_host.py holds it against the header.  A new entry point is one row here and
# a short method on Solver.
#   Scalar: a by-value argument or a pointer to one value (ctypes type, header name).
#   Array:  a caller-owned buffer, passed as void*.  key: its name in the wrappers' dicts; out: the library writes it;
#           opt: a device-mode dict may leave the key out (NULL); nullable: a host-mode None is passed as NULL;
#           shape: a tuple of ints, names (the solver's n, sdim, m_max, the cfg's N, nc_max, ne_max, the call's scalars
#           by header name, rows, words) and callables of those, or one callable that gives the tuple, or None for NULL;
#           bcast: a host input is broadcast to the shape (otherwise reshaped); host: a host pointer in both modes.
Scalar = collections.namedtuple("Scalar", "ctype name")
Array = collections.namedtuple("Array", "key dtype out opt nullable shape bcast host")
Entry = collections.namedtuple("Entry", "restype args")

_int, _i32, _i64, _u64, _f64, _P = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double,
                                    ctypes.c_void_p)
_f8, _i4, _i1, _i8 = np.float64, np.int32, np.int8, np.int64
_CFG = Scalar(ctypes.POINTER(Cfg), "cfg")
_HANDLE, _STREAM, _B = Scalar(_P, "handle"), Scalar(_P, "hip_stream"), Scalar(_i64, "B")


def _in(key, dtype, *dims, shape=None, opt=False, nullable=None, bcast=False, host=False):
    return Array(key, np.dtype(dtype), False, opt, opt if nullable is None else nullable, shape or dims, bcast, host)


def _out(key, dtype, *dims, shape=None, opt=True):
    return Array(key, np.dtype(dtype), True, opt, False, shape or dims, False, False)


def _elp_shape(d):   # no ellipse slots: elp and ne are NULL in both directions
    return (d["B"], d["ne_max"], 5) if d["ne_max"] else None


def _ne_shape(d):
    return (d["B"],) if d["ne_max"] else None


def _steps1(d):
    return d["S"] + 1


def _obs_cols(d):   # the obstacle columns of solve_sens_obs (alipmpc_sens_obs_cols)
    return 3 * d["nc_max"] + 5 * d["ne_max"]


# x0, goal, leg, cir, nc, elp, ne: the scene block of solve / eval / rollout / audit and, around foot0, the closed loops
_SCENE = (_in("x0", _f8, "B", "sdim"), _in("goal", _f8, "B", 2, bcast=True),
          _in("leg", _i1, "B", nullable=True, bcast=True), _in("cir", _f8, "B", "nc_max", 3, bcast=True),
          _in("nc", _i4, "B", bcast=True),
          _in("elp", _f8, shape=_elp_shape, opt=True, nullable=False, bcast=True),
          _in("ne", _i4, shape=_ne_shape, opt=True, nullable=False, bcast=True))
_LAST_U = _in("last_u", _f8, "B", 2, opt=True, bcast=True)
_SOLVE_IN = _SCENE + (_in("u0", _f8, "B", "n"), _LAST_U)
_SOLVE_OUT = (_out("u", _f8, "B", "n", opt=False), _out("foot", _f8, "B", 3), _out("x_pred", _f8, "B", "N", "sdim"),
              _out("status", _i4, "B"), _out("iters", _i4, "B"))
_CL_HEAD = (_HANDLE, _B, Scalar(_i32, "S"), Scalar(_i32, "f_cyc"))
_CL_IN = _SCENE[:1] + (_in("foot0", _f8, "B", 2),) + _SCENE[1:]
_CL_OUT = (_out("foot", _f8, "B", "S", 3), _out("x", _f8, "B", _steps1, 5), _out("hd", _f8, "B", "S", 2),
           _out("status", _i4, "B", "S", "f_cyc"), _out("iters", _i4, "B", "S", "f_cyc"),
           _out("steps_to_goal", _i4, "B"), _out("action", _f8, "B", "S", "f_cyc", 8))
_KICK_SEED = (Scalar(_f64, "kick"), Scalar(_u64, "seed"))

_ABI = {
    "alipmpc_default_cfg": Entry(_int, (Scalar(_i32, "variant"), Scalar(_i32, "N"), _CFG._replace(name="out"))),
    "alipmpc_rows_per_step": Entry(_i32, (_CFG,)),
    "alipmpc_num_vars": Entry(_i32, (_CFG,)),
    "alipmpc_create": Entry(_int, (_CFG, Scalar(_int, "device"), Scalar(ctypes.POINTER(_P), "handle"))),
    "alipmpc_solve_batch": Entry(_int, (_HANDLE, _B) + _SOLVE_IN + _SOLVE_OUT + (_STREAM,)),
    "alipmpc_solve_sens_batch": Entry(_int, (_HANDLE, _B) + _SOLVE_IN + _SOLVE_OUT + (
        _out("dfoot", _f8, "B", 3, 7, opt=False), _out("du", _f8, "B", "n", 7), _out("sens_ok", _i4, "B"), _STREAM)),
    "alipmpc_eval_batch": Entry(_int, (_HANDLE, _B) + _SCENE + (
        _in("u", _f8, "B", "n"), _LAST_U, _out("f", _f8, "B"), _out("grad", _f8, "B", "n"),
        _out("c", _f8, "B", "m_max"), _out("J", _f8, "B", "m_max", "n"), _out("cl", _f8, "B", "m_max"),
        _out("cu", _f8, "B", "m_max"), _out("goal_eff", _f8, "B", 2), _out("row_active", _i1, "B", "m_max"), _STREAM)),
    "alipmpc_rollout_batch": Entry(_int, (_HANDLE, _B, Scalar(_i32, "S")) + tuple(
        a._replace(opt=True) if a.key == "leg" else a for a in _SOLVE_IN) + (
        _out("foot", _f8, "B", "S", 3), _out("x", _f8, "B", _steps1, "sdim"), _out("status", _i4, "B", "S"),
        _out("iters", _i4, "B", "S"), _out("steps_to_goal", _i4, "B"), _out("u", _f8, "B", "S", "n"), _STREAM)),
    "alipmpc_closed_loop_batch": Entry(_int, _CL_HEAD + _KICK_SEED + _CL_IN + _CL_OUT + (_STREAM,)),
    "alipmpc_closed_loop_dataset_batch": Entry(_int, _CL_HEAD + _KICK_SEED + _CL_IN + _CL_OUT + (
        Scalar(_i64, "first_index"), Scalar(_f64, "safe_dis"), Scalar(_i64, "max_rows"),
        _out("X", _f8, "rows", lambda d: 3 * d["nc_max"] + 5 * d["ne_max"] + 11),
        _out("y_mpc", _f8, "rows", 8), _out("y_act", _f8, "rows", 8), _out("row_status", _i4, "rows"),
        _out("row_start", _i8, lambda d: d["B"] + 1), _STREAM)),
    "alipmpc_closed_loop_schedule_batch": Entry(_int, _CL_HEAD + (Scalar(_u64, "mpc_mask"),) + _KICK_SEED + _CL_IN + (
        *_CL_OUT, _out("plan", _f8, "B", "S", "f_cyc", "n"), _STREAM)),
    "alipmpc_trace_len": Entry(_i32, (_CFG,)),
    "alipmpc_trace_batch": Entry(_int, (_HANDLE, _B, _in("x0", _f8, "B", 5), _in("u", _f8, "B", "n"),
                                        _out("trace", _f8, "B", "N", lambda d: trace_len(d["cfg"]), 2, opt=False),
                                        _STREAM)),
    "alipmpc_nominal_gait_batch": Entry(_int, (
        _HANDLE, _B, Scalar(_f64, "vx_max"), _in("x", _f8, "B", 5), _in("leg", _i1, "B", opt=True, bcast=True),
        _in("vel_des_in", _f8, "B", 2, opt=True, bcast=True), _out("vel_des", _f8, "B", 2),
        _out("foot", _f8, "B", 2), _STREAM)),
    "alipmpc_solve_slots": Entry(_int, (_HANDLE, Scalar(ctypes.POINTER(_i64), "slots"))),
    "alipmpc_solve_launches": Entry(_int, (_HANDLE, _B, Scalar(ctypes.POINTER(_i32), "launches"),
                                           Scalar(ctypes.POINTER(_i32), "team"))),
    "alipmpc_lane_handoffs": Entry(_int, (_HANDLE, _STREAM, Scalar(ctypes.POINTER(_i64), "count"))),
    "alipmpc_solve_program": Entry(ctypes.c_char_p, (_HANDLE,)),
    "alipmpc_last_kernel_ms": Entry(_f64, (_HANDLE,)),
    "alipmpc_build_id": Entry(ctypes.c_char_p, ()),
    "alipmpc_scenes_batch": Entry(_int, (
        _HANDLE, _B, Scalar(_u64, "seed"), Scalar(_i64, "first_index"), Scalar(_i32, "n_cir"), Scalar(_i32, "n_elp"),
        Scalar(_i64, "fields"), Scalar(_i32, "max_candidates"), _out("x0", _f8, "B", 5), _out("goal", _f8, "B", 2),
        _out("leg", _i1, "B"), _out("cir", _f8, "B", "nc_max", 3), _out("nc", _i4, "B"),
        _out("elp", _f8, shape=_elp_shape), _out("ne", _i4, shape=_ne_shape),
        _out("u0", _f8, "B", lambda d: 5 * d["N"]), _STREAM)),
    "alipmpc_audit_summary_len": Entry(_i32, (Scalar(_i32, "n_edges"),)),
    "alipmpc_audit_batch": Entry(_int, (_HANDLE, _B) + _SCENE + (
        _in("u", _f8, "B", "n", opt=True), _in("status", _i4, "B", opt=True, bcast=True),
        _out("metrics", _f8, "B", 5), _out("where", _i4, "B", 3), Scalar(_f64, "viol_tol"),
        _in("edges", _f8, "n_edges", host=True), Scalar(_i32, "n_edges"),
        _out("summary", _i8, "words"), _STREAM)),
    "alipmpc_last_error": Entry(ctypes.c_char_p, (_HANDLE,)),
    "alipmpc_destroy": Entry(None, (_HANDLE,)),
}
EXPORTS = tuple(_ABI)
# The exports of the extension header include/alipmpc_sens_obs.h (which alipmpc.h includes), in the same form: _ABI is
# alipmpc.h's own table, held against that header entry by entry (tests/test_binding_host.py), this one against its
# (tests/test_sens_obs_binding_host.py).
_ABI_EXT = {
    "alipmpc_sens_obs_cols": Entry(_i32, (_CFG,)),
    "alipmpc_solve_sens_obs_batch": Entry(_int, (_HANDLE, _B) + _SOLVE_IN + _SOLVE_OUT + (
        _out("dfoot", _f8, "B", 3, 7), _out("du", _f8, "B", "n", 7), _out("sens_ok", _i4, "B"),
        _out("dfoot_obs", _f8, "B", 3, _obs_cols, opt=False), _out("du_obs", _f8, "B", "n", _obs_cols), _STREAM)),
}
EXPORTS_EXT = tuple(_ABI_EXT)
_ENTRIES = {**_ABI, **_ABI_EXT}   # every entry point, for the call paths


def _shape(a, d):
    """Array a's shape under the names d (None: the array is NULL)."""
    s = a.shape(d) if callable(a.shape) else a.shape
    return s and tuple(d[x] if isinstance(x, str) else x(d) if callable(x) else x for x in s)


def _host_array(a, v, d, skip):
    """What a host-pointer call passes for array a, given v (None: nothing given): the input converted to a's dtype and
    shape, or a zeroed output; None is NULL."""
    if a.out and v is not None:          # the caller's own output buffer (audit's summary)
        return v
    shape = _shape(a, d)
    if shape is None or a.key in skip:
        return None
    if a.out:
        return np.zeros(shape, a.dtype)
    if v is None and a.nullable:
        return None
    if not a.bcast:
        return np.ascontiguousarray(v, a.dtype).reshape(shape)
    if 0 in shape[1:]:                   # no slots (nc_max == 0): nothing of the argument is read
        return np.zeros(shape, a.dtype)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v), shape), a.dtype)


# The exports every build has had.  The others may be absent from an older development build loaded through
# ALIPMPC_LIB for A/B timing: load() sets no prototype for an absent one, and calling it raises AttributeError.
_ALWAYS = frozenset("alipmpc_" + k for k in (
    "default_cfg", "rows_per_step", "num_vars", "create", "solve_batch", "eval_batch", "rollout_batch",
    "closed_loop_batch", "trace_len", "trace_batch", "last_kernel_ms", "last_error", "destroy"))


def _device_plan(args):
    """What Solver._device needs of a batch entry, precomputed so that a call runs no Python loop over its arguments:
    the keys it reads from the inp dict and from the out dict, a getter of the required ones of each (it raises the
    KeyError of a missing one; None: none is required), and `order`, which puts the values gathered as (scalars in
    header order, inp values, out values) into the header's order between (handle, B) and the stream.  A host array
    counts as a scalar: its wrapper passes the host pointer."""
    mid = args[2:-1]
    scalars = [i for i, a in enumerate(mid) if isinstance(a, Scalar) or a.host]
    inps = [i for i, a in enumerate(mid) if i not in scalars and not a.out]
    outs = [i for i, a in enumerate(mid) if i not in scalars and a.out]
    gathered = scalars + inps + outs

    def need(idx):
        required = [mid[i].key for i in idx if not mid[i].opt]
        return operator.itemgetter(*required) if required else None
    return (tuple(mid[i].key for i in inps), tuple(mid[i].key for i in outs), need(inps), need(outs),
            operator.itemgetter(*(gathered.index(i) for i in range(len(mid)))))


_DEVICE_PLAN = {name: _device_plan(e.args) for name, e in _ENTRIES.items() if name.endswith("_batch")}

_lib = None


def lib_path():
    return _build.LIB


def build_id():
    """The loaded library's build id (include/alipmpc.h: alipmpc_build_id; "unknown" for builds without one)."""
    L = load()
    return L.alipmpc_build_id().decode() if hasattr(L, "alipmpc_build_id") else "unknown"


def load(build_if_missing=True):
    """Load libalipmpc.so (building it in-tree with hipcc if it is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ALIPMPC_LIB")          # dev override (e.g. the phase-stamp diagnostic build)
    if path is None:
        if build_if_missing and _build.needs_build():
            _build.build()
        path = _build.LIB
    if not os.path.exists(path):
        raise RuntimeError(f"libalipmpc.so not found at {path}; run alipmpc.build.build()")
    L = ctypes.CDLL(path)
    for name, entry in _ENTRIES.items():
        if name in _ALWAYS or hasattr(L, name):    # an absent symbol gets no prototype; one of _ALWAYS raises here
            f = getattr(L, name)
            f.argtypes = [a.ctype if isinstance(a, Scalar) else _P for a in entry.args]
            f.restype = entry.restype
    _lib = L
    return L


# fp32 solve kernels (cfg.precision = PREC_FP32, BASELINE cfg5): the fp64 tolerance 1e-8 is below fp32
# resolution, so unless the caller sets them the fp32 tolerances are tol 1e-4 / acceptable 1e-3 for N <= 3
# and 3e-4 / 3e-3 for longer horizons, whose decision-space gradients (through A^k) are larger and put the
# fp32 stationarity floor higher.  tools/fp32_study.py (profiles/): N = 3 foothold within 1e-3 of the fp64
# solve on 99.8 % of the instances both converge on, same feasible fraction, 1.5x the fp64 throughput;
# N = 5 with ellipses 99 % within 1e-3, 1.7x.
FP32_TOL, FP32_ACCEPTABLE_TOL = 1e-4, 1e-3
FP32_TOL_LONG, FP32_ACCEPTABLE_TOL_LONG = 3e-4, 3e-3


def default_cfg(variant=VARIANT_MODI, N=3, **overrides):
    c = Cfg()
    rc = load().alipmpc_default_cfg(variant, N, ctypes.byref(c))
    if rc != 0:
        raise ValueError(f"alipmpc_default_cfg({variant}, {N}) -> {rc}")
    if overrides.get("precision") == PREC_FP32:
        long_h = N > 3
        overrides.setdefault("tol", FP32_TOL_LONG if long_h else FP32_TOL)
        overrides.setdefault("acceptable_tol", FP32_ACCEPTABLE_TOL_LONG if long_h else FP32_ACCEPTABLE_TOL)
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def rows_per_step(cfg):
    return int(load().alipmpc_rows_per_step(ctypes.byref(cfg)))


def num_vars(cfg):
    return int(load().alipmpc_num_vars(ctypes.byref(cfg)))


def trace_len(cfg):
    return int(load().alipmpc_trace_len(ctypes.byref(cfg)))


def audit_summary_len(n_edges):
    """Words of an audit summary with n_edges histogram edges: 6 + (n_edges + 1) + 20 (alipmpc_audit_summary_len)."""
    n = int(load().alipmpc_audit_summary_len(int(n_edges)))
    if n < 0:
        raise ValueError(f"alipmpc_audit_summary_len({n_edges}) -> {_ERRORS.get(n, n)}")
    return n


def _edges_arg(edges):
    """(host array kept alive by the caller, pointer or None, count) of the histogram edges: always a host pointer."""
    e = np.ascontiguousarray(np.asarray(edges, np.float64).reshape(-1))
    return e, (_ptr(e) if e.size else None), int(e.size)


STREAM_NULL = ctypes.c_void_p(ctypes.c_size_t(-1).value)   # ALIPMPC_STREAM_NULL


def _stream_arg(st):
    """Device-pointer mode needs a non-NULL stream argument: torch's default stream has handle 0, which the
    ABI reads as host-pointer mode, so it is passed as ALIPMPC_STREAM_NULL."""
    h = int(st.cuda_stream)
    return ctypes.c_void_p(h) if h else STREAM_NULL


def _ptr(a):
    if a is None:
        return None
    data_ptr = getattr(a, "data_ptr", None)          # torch tensor (device mode)
    return _P(data_ptr()) if data_ptr is not None else a.ctypes.data_as(_P)


class _SensObsCalls:
    """The calls of the extension header include/alipmpc_sens_obs.h (_ABI_EXT), on Solver through this base class: the
    plan's sensitivities to the obstacles."""

    @property
    def sens_obs_cols(self):
        """Obstacle columns of solve_sens_obs: 3 nc_max + 5 ne_max (alipmpc_sens_obs_cols)."""
        return int(self._L.alipmpc_sens_obs_cols(ctypes.byref(self.cfg)))

    def solve_sens_obs(self, x0, goal, leg, cir, nc, elp=None, ne=None, u0=None, want_du=True, want_state=True):
        """solve_sens() with the obstacle columns (alipmpc_solve_sens_obs_batch): the dict of solve_sens plus dfoot_obs
        (B, 3, P) and du_obs (B, 5N, P) (None unless want_du), P = sens_obs_cols — columns as
        alipmpc.sensitivity.obs_columns(nc_max, ne_max), by the caller's input slots; exact zeros for a slot past the
        instance's count or dropped by select_obs, NaN rows where the instance's sensitivity is invalid.  want_state =
        False leaves dfoot, du and sens_ok out (None)."""
        skip = (() if want_du else ("du", "du_obs")) + (() if want_state else ("dfoot", "du", "sens_ok"))
        return self._host("alipmpc_solve_sens_obs_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, u0=u0),
                          skip=skip)

    def solve_sens_obs_device(self, inp, out, stream=None):
        """Asynchronous solve with sensitivities and their obstacle columns on device tensors: inp as solve_device; out
        as solve_sens_device (dfoot optional here) plus dfoot_obs (B,3,P) (required) and du_obs (B,5N,P) (optional)."""
        self._device("alipmpc_solve_sens_obs_batch", inp, out, stream, inp["x0"].shape[0])


class Solver(_SensObsCalls):
    """Owns one libalipmpc handle (one config, one device)."""

    def __init__(self, cfg, device=0):
        self.cfg = cfg
        self.device = device
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.alipmpc_create(ctypes.byref(cfg), device, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"alipmpc_create failed: {_ERRORS.get(rc, rc)}")
        self._h = h
        self.n = num_vars(cfg)
        self.rps = rows_per_step(cfg)
        self.m_max = cfg.N * self.rps
        self.sdim = 3 if cfg.variant == VARIANT_DD else 5

    def close(self):
        if getattr(self, "_h", None):
            self._L.alipmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.alipmpc_last_error(self._h).decode()
            raise RuntimeError(f"{what} failed ({_ERRORS.get(rc, rc)}): {msg}")

    def last_kernel_ms(self):
        return float(self._L.alipmpc_last_kernel_ms(self._h))

    def solve_program(self):
        """The device program this handle's solves run (include/alipmpc.h: alipmpc_solve_program)."""
        return self._L.alipmpc_solve_program(self._h).decode()

    def solve_slots(self):
        """Instances the solve kernel holds resident at once; larger batches run the persistent
        work-queue launch (include/alipmpc.h: alipmpc_solve_slots)."""
        v = ctypes.c_int64(0)
        self._check(self._L.alipmpc_solve_slots(self._h, ctypes.byref(v)), "alipmpc_solve_slots")
        return int(v.value)

    def solve_launches(self, B):
        """(kernel launches per solve of B instances, phase-2 team size) — 2 for a split launch
        (include/alipmpc.h: alipmpc_solve_launches)."""
        n, t = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._L.alipmpc_solve_launches(self._h, int(B), ctypes.byref(n), ctypes.byref(t)),
                    "alipmpc_solve_launches")
        return int(n.value), int(t.value)

    def lane_handoffs(self, stream=None):
        """Instances of the last lane-program or fp32 wave-program solve on `stream` (None: the handle's own stream, the
        host-pointer calls) that were handed to the fp64 wave program for IPOPT's restoration phase (include/alipmpc.h)."""
        v = ctypes.c_int64(0)
        st = None if stream is None else _stream_arg(stream)
        self._check(self._L.alipmpc_lane_handoffs(self._h, st, ctypes.byref(v)), "alipmpc_lane_handoffs")
        return int(v.value)

    # ---------------------------------------------------------------- the two call paths, driven by _ABI
    def _host(self, name, given, scalars=(), skip=(), **dims):
        """Host-pointer call of a batch entry: converts the inputs in `given` (key -> array-like) to the table's dtype
        and shape, allocates every output that is neither in `given` nor in `skip` (those are None), calls, checks,
        and returns the outputs as a dict in the table's order.  B is scalars["B"] or the leading size of the
        entry's first array; `dims` adds names for the shape rules (a B there sizes the arrays only).  `given` is the
        caller's own dict: converted arrays replace what it held."""
        cfg, args = self.cfg, _ENTRIES[name].args
        d = dict(n=self.n, sdim=self.sdim, m_max=self.m_max, cfg=cfg, N=cfg.N, nc_max=cfg.nc_max, ne_max=cfg.ne_max,
                 handle=self._h, hip_stream=None)
        d.update(scalars, **dims)
        if "B" not in d:
            d["B"] = self._batch_size(name, given)
        argv, res, keep = [], {}, []
        for a in args:
            if isinstance(a, Scalar):
                argv.append(scalars[a.name] if a.name in scalars else d[a.name])
                continue
            v = given.get(a.key)
            if a.host:
                v, p, _ = _edges_arg(v)
            else:
                v = _host_array(a, v, d, skip)
                p = _ptr(v)
            if a.out:
                res[a.key] = v
            keep.append(v)
            argv.append(p)
        self._check(getattr(self._L, name)(*argv), name)
        return res

    def _batch_size(self, name, given):
        """B of a host call: the leading size of the entry's first array, which is converted here, once, in `given`."""
        lead = next(a for a in _ENTRIES[name].args if isinstance(a, Array))
        x = np.ascontiguousarray(given[lead.key], lead.dtype).reshape(_shape(lead, dict(B=-1, sdim=self.sdim)))
        given[lead.key] = x
        return x.shape[0]

    def _device(self, name, inp, out, stream, B, *scalars):
        """Device-pointer call of a batch entry, asynchronous on `stream` (None: torch's current stream): the pointers
        of the tensors in the dicts `inp` / `out`; a required key that is missing is a KeyError, an optional one NULL.
        `scalars`: the entry's scalars after B (and the host pointer of a host array), in the header's order."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream()
        inp_keys, out_keys, need_inp, need_out, order = _DEVICE_PLAN[name]
        if need_inp:
            need_inp(inp)
        if need_out:
            need_out(out)
        gathered = [*scalars, *map(_ptr, map(inp.get, inp_keys)), *map(_ptr, map(out.get, out_keys))]
        self._check(getattr(self._L, name)(self._h, B, *order(gathered), _stream_arg(stream)), name)

    # ---------------------------------------------------------------- host (numpy) calls
    @staticmethod
    def _scene(x0, goal, leg, cir, nc, elp, ne, **more):
        return dict(x0=x0, goal=goal, leg=leg, cir=cir, nc=nc, elp=elp, ne=ne, **more)

    def solve(self, x0, goal, leg, cir, nc, elp=None, ne=None, u0=None, last_u=None):
        """Solve a batch from host arrays; returns a dict of numpy outputs."""
        return self._host("alipmpc_solve_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, u0=u0, last_u=last_u))

    def solve_sens(self, x0, goal, leg, cir, nc, elp=None, ne=None, u0=None, want_du=True):
        """solve() with the plan's sensitivities (alipmpc_solve_sens_batch): the dict of solve plus dfoot (B, 3, 7),
        du (B, 5N, 7) (None unless want_du) and sens_ok (B,) — columns as alipmpc.sensitivity.COLUMNS (x0's five
        components, then the goal); NaN rows where sens_ok is 0."""
        return self._host("alipmpc_solve_sens_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, u0=u0),
                          skip=() if want_du else ("du",))

    def eval(self, x0, goal, leg, cir, nc, elp=None, ne=None, u=None, last_u=None, want_J=True):
        return self._host("alipmpc_eval_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, u=u, last_u=last_u),
                          skip=() if want_J else ("J",))

    def rollout(self, x0, goal, leg, cir, nc, elp=None, ne=None, u0=None, last_u=None, steps=8):
        """Closed-loop receding-horizon rollout (alipmpc_rollout_batch) from host arrays.  Returns
        dict(foot (B,S,3), x (B,S+1,sdim), status (B,S), iters (B,S), steps_to_goal (B,), u (B,S,n))."""
        return self._host("alipmpc_rollout_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, u0=u0, last_u=last_u),
                          dict(S=int(steps)))

    def closed_loop(self, x0, foot0, goal, leg, cir, nc, elp=None, ne=None, steps=8, f_cyc=40, kick=0.0, seed=0):
        """Closed loop at the reference's control rate (alipmpc_closed_loop_batch): B episodes, up to `steps`
        walking steps, f_cyc solves per step on an ALIP plant with an optional seeded velocity kick.
        Returns dict(foot (B,S,3), x (B,S+1,5), hd (B,S,2), status (B,S,f_cyc), iters (B,S,f_cyc),
        steps_to_goal (B,), action (B,S,f_cyc,8): the controller command of every tick)."""
        return self._host("alipmpc_closed_loop_batch", self._scene(x0, goal, leg, cir, nc, elp, ne, foot0=foot0),
                          dict(S=int(steps), f_cyc=int(f_cyc), kick=float(kick), seed=int(seed)))

    def closed_loop_device(self, inp, out, steps, f_cyc=40, kick=0.0, seed=0, stream=None):
        """Asynchronous closed loop on device tensors: inp x0 (B,5), foot0 (B,2), goal, leg (int8), cir, nc
        [, elp, ne]; out dict with any of foot, x, hd, status, iters, steps_to_goal, action (shapes of
        closed_loop)."""
        self._device("alipmpc_closed_loop_batch", inp, out, stream, inp["x0"].shape[0], int(steps), int(f_cyc),
                     float(kick), int(seed))

    def closed_loop_schedule(self, x0, foot0, goal, leg, cir, nc, elp=None, ne=None, steps=8, f_cyc=20,
                             mpc_ticks=(15,), kick=0.0, seed=0, want_plans=False):
        """Closed loop that solves on scheduled ticks only (alipmpc_closed_loop_schedule_batch): tick i of every step
        solves the MPC if i is in mpc_ticks (an iterable of tick indices, or an int bit mask); every other tick takes
        the nominal ALIP foothold cal_foot_with_veldes(x_nex, v_des) (status TICK_NOMINAL, 0 iterations).  The default
        is the reference's hybrid driver (main_sim_mpc_alip.py: 20 ticks, one solve at tick 15).  Returns the dict of
        closed_loop plus plan: (B, S, f_cyc, 5N) the u of every solved tick, NaN elsewhere (None unless want_plans).
        On a handle whose cfg.cl_between is CL_BETWEEN_FIRST_ORDER, a tick between the solves of a step whose last
        solve has valid sensitivities commands that solve's plan moved to first order with the plant instead, u_fo =
        u + du[:, 0:5] (x_nex - x_nex of the solve): status TICK_FIRST_ORDER (-21), 0 iterations, plan row u_fo; the
        ticks before a step's first solve, and those after a solve without valid sensitivities, stay nominal.
        cfg.cl_between = CL_BETWEEN_GUARDED (3): the same, but u_fo is first held against the constraint rows at the
        tick's x_nex (audit's viol of (x_nex, u_fo, -leg_ind)); where it exceeds CL_GUARD_VIOL the episode re-solves on
        that tick, warm-started from its current plan, and takes a new anchor: the tick then carries the solve's status,
        iterations and plan although it is not in mpc_ticks."""
        from .schedule import mask_of
        sc = dict(S=int(steps), f_cyc=int(f_cyc), mpc_mask=mask_of(mpc_ticks), kick=float(kick), seed=int(seed))
        return self._host("alipmpc_closed_loop_schedule_batch",
                          self._scene(x0, goal, leg, cir, nc, elp, ne, foot0=foot0), sc,
                          skip=() if want_plans else ("plan",))

    def closed_loop_schedule_device(self, inp, out, steps, f_cyc=20, mpc_ticks=(15,), kick=0.0, seed=0, stream=None):
        """Asynchronous scheduled closed loop on device tensors: inp / out as closed_loop_device, out also with plan
        (B, S, f_cyc, 5N) if the plans are wanted.  cfg.cl_between = CL_BETWEEN_FIRST_ORDER: first-order ticks (status
        TICK_FIRST_ORDER, -21) as in closed_loop_schedule; CL_BETWEEN_GUARDED (3): guarded ones, with re-solves on the
        device where the guard fires (no host round trip)."""
        from .schedule import mask_of
        self._device("alipmpc_closed_loop_schedule_batch", inp, out, stream, inp["x0"].shape[0], int(steps), int(f_cyc),
                     mask_of(mpc_ticks), float(kick), int(seed))

    def x_cols(self):
        """Columns of the dataset's X: 3 nc_max + 5 ne_max + 11 (include/alipmpc.h)."""
        return 3 * self.cfg.nc_max + 5 * self.cfg.ne_max + 11

    def closed_loop_dataset(self, x0, foot0, goal, leg, cir, nc, elp=None, ne=None, steps=8, f_cyc=8, kick=0.0,
                            seed=0, first=0, safe_dis=0.4, max_rows=None):
        """closed_loop that also returns the imitation-learning rows of every tick that ran
        (alipmpc_closed_loop_dataset_batch): the dict of closed_loop plus X (R, 3 nc_max + 5 ne_max + 11), y_mpc (R, 8),
        y_act (R, 8), row_status (R,), row_start (B + 1,) — episode b owns rows row_start[b] .. row_start[b + 1] - 1 —
        trimmed to the total R = row_start[B].  `first`: global index of episode 0 (the kick stream's episode id).
        max_rows (default B * steps * f_cyc, which always suffices) caps the rows written; rows past it are lost and
        R = min(row_start[B], max_rows)."""
        given = self._scene(x0, goal, leg, cir, nc, elp, ne, foot0=foot0)
        B = self._batch_size("alipmpc_closed_loop_dataset_batch", given)
        S, F = int(steps), int(f_cyc)
        cap = B * S * F if max_rows is None else int(max_rows)
        n = max(cap, 0)
        out = self._host("alipmpc_closed_loop_dataset_batch", given,
                         dict(S=S, f_cyc=F, kick=float(kick), seed=int(seed), first_index=int(first),
                              safe_dis=float(safe_dis), max_rows=cap), B=B, rows=n)
        R = min(int(out["row_start"][B]), n)
        for k in ("X", "y_mpc", "y_act", "row_status"):
            out[k] = out[k][:R]
        return out

    def closed_loop_dataset_device(self, inp, out, steps, f_cyc=8, kick=0.0, seed=0, first=0, safe_dis=0.4,
                                   max_rows=None, stream=None):
        """Asynchronous closed loop with rows on device tensors: inp / out as closed_loop_device, out also with any
        of X (max_rows, 3 nc_max + 5 ne_max + 11), y_mpc (max_rows, 8), y_act (max_rows, 8), row_status (max_rows,)
        int32, row_start (B + 1,) int64.  max_rows defaults to the leading size of the first row tensor given.  Rows
        at positions >= max_rows are not written; the caller reads row_start[B] once the stream is done."""
        if max_rows is None:
            rows = [out[k] for k in ("X", "y_mpc", "y_act", "row_status") if out.get(k) is not None]
            max_rows = min(t.shape[0] for t in rows) if rows else 0
        self._device("alipmpc_closed_loop_dataset_batch", inp, out, stream, inp["x0"].shape[0], int(steps), int(f_cyc),
                     float(kick), int(seed), int(first), float(safe_dis), int(max_rows))

    def nominal_gait(self, x, leg=None, vx_max=0.6, vel_des=None):
        """Nominal gait (alipmpc_nominal_gait_batch): returns (vel_des (B,2), foot (B,2)) — alip_des_vel(vx_max,
        leg_ind) per instance (or the given vel_des) and cal_foot_with_veldes(x, vel_des)."""
        out = self._host("alipmpc_nominal_gait_batch", dict(x=x, leg=leg, vel_des_in=vel_des),
                         dict(vx_max=float(vx_max)))
        return out["vel_des"], out["foot"]

    def trace(self, x0, u):
        """Dense plan traces (alipmpc_trace_batch): x0 (B,5), u (B,5N) -> (B, N, trace_len, 2)."""
        return self._host("alipmpc_trace_batch", dict(x0=x0, u=u))["trace"]

    def audit(self, x0, goal, leg, cir, nc, elp=None, ne=None, u=None, status=None, edges=(), viol_tol=1e-4,
              summary=None):
        """Plan audit (alipmpc_audit_batch) from host arrays: u (B,5N) the plans (a solve's u), status (B,) optional.
        Returns dict(metrics (B,5), where (B,3), summary (audit_summary_len(len(edges)),) int64) — columns and words
        as alipmpc.audit.COLS / WHERE / SUMMARY_FIELDS (include/alipmpc.h).  The summary counts from zero, or is added
        to a copy of `summary` when one is given (the buffer a chunked sweep carries along)."""
        ne_ = int(np.size(edges))
        words = int(self._L.alipmpc_audit_summary_len(ne_))     # negative for an edge count the call itself refuses
        given = self._scene(x0, goal, leg, cir, nc, elp, ne, u=u, status=status, edges=edges)
        if summary is not None:
            given["summary"] = acc = np.array(summary, np.int64).reshape(-1)
            if words >= 0 and acc.size != words:
                raise ValueError(f"summary has {acc.size} words, {words} expected for {ne_} edges")
        return self._host("alipmpc_audit_batch", given, dict(viol_tol=float(viol_tol), n_edges=ne_),
                          words=max(words, 0))

    def audit_device(self, inp, out, edges=(), viol_tol=1e-4, stream=None):
        """Asynchronous plan audit on device tensors: inp as solve_device's plus u (B,5N) the plans and optionally
        status (B,) int32; out any of metrics (B,5) float64, where (B,3) int32, summary (audit_summary_len(len(edges)),)
        int64 — the summary is ADDED to, so one tensor carried through the chunks of a sweep ends as the sweep's.
        edges is a host sequence (copied into the launch)."""
        e, ep, ne_ = _edges_arg(edges)
        self._device("alipmpc_audit_batch", inp, out, stream, inp["x0"].shape[0], float(viol_tol), ep, ne_)

    def scenes(self, B, seed=0, first=0, n_cir=None, n_elp=0, fields=0, max_candidates=0):
        """Monte-Carlo scenes first .. first + B - 1 of the counter-based stream (alipmpc_scenes_batch), generated
        on the device: the dict of scenes.make_batch (elp / ne None without ellipse slots).  n_cir defaults to the
        handle's nc_max; fields > 0 shares that many obstacle fields (instance g uses field g % fields)."""
        n_cir = self.cfg.nc_max if n_cir is None else n_cir
        return self._host("alipmpc_scenes_batch", {},
                          dict(B=int(B), seed=int(seed), first_index=int(first), n_cir=int(n_cir), n_elp=int(n_elp),
                               fields=int(fields), max_candidates=int(max_candidates)), B=max(int(B), 0))

    # ---------------------------------------------------------------- device (torch) calls
    def scenes_device(self, out, seed=0, first=0, n_cir=None, n_elp=0, fields=0, max_candidates=0, stream=None):
        """Asynchronous scene generation into device tensors: out holds any of x0 (B,5), goal (B,2), leg (int8),
        cir (B,nc_max,3), nc (int32), elp (B,ne_max,5), ne (int32), u0 (B,5N) — the keys of solve_device's inp, so
        the solve reads what this wrote, on the same stream, with no copy.  B is the leading size of out's tensors."""
        B = next(v for v in out.values() if v is not None).shape[0]
        n_cir = self.cfg.nc_max if n_cir is None else n_cir
        self._device("alipmpc_scenes_batch", {}, out, stream, B, int(seed), int(first), int(n_cir), int(n_elp),
                     int(fields), int(max_candidates))

    def rollout_device(self, inp, out, steps, stream=None):
        """Asynchronous rollout on device tensors: inp as solve_device, out dict with any of foot (B,S,3),
        x (B,S+1,sdim), status (B,S), iters (B,S), steps_to_goal (B,), u (B,S,n)."""
        self._device("alipmpc_rollout_batch", inp, out, stream, inp["x0"].shape[0], int(steps))

    def trace_device(self, x0, u, trace, stream=None):
        """Asynchronous dense plan traces on device tensors x0 (B,5), u (B,5N) -> trace (B,N,trace_len,2)."""
        self._device("alipmpc_trace_batch", {"x0": x0, "u": u}, {"trace": trace}, stream, x0.shape[0])

    def solve_device(self, inp, out, stream=None):
        """Asynchronous solve on device tensors.  inp/out: dicts of torch CUDA tensors with the shapes of
        solve(); stream: torch.cuda.Stream (defaults to the current stream)."""
        self._device("alipmpc_solve_batch", inp, out, stream, inp["x0"].shape[0])

    def solve_sens_device(self, inp, out, stream=None):
        """Asynchronous solve with sensitivities on device tensors: inp as solve_device; out as solve_device plus
        dfoot (B,3,7) (required), du (B,5N,7) and sens_ok (B,) int32 (either may be absent)."""
        self._device("alipmpc_solve_sens_batch", inp, out, stream, inp["x0"].shape[0])

    def eval_device(self, inp, out, stream=None):
        self._device("alipmpc_eval_batch", inp, out, stream, inp["x0"].shape[0])
