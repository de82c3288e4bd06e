"""CPU: the ctypes binding (alipmpc/_lib.py) against the header and against itself.

1. The table _ABI, entry by entry, against the prototypes parsed out of include/alipmpc.h.
2. The argument vector and the returned dict of every Solver wrapper, host and device, recorded by a stand-in for the
   library: no handle is created, no library call is made for a batch entry, nothing touches a GPU.  The expectations
   are literals, written from the hand-written wrappers this table replaced.
3. A device-mode dict without a required key is a KeyError, without an optional one a NULL.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
# torch before anything here loads libalipmpc.so: the order conftest's gpu_lib keeps.  This file runs ahead of the GPU
# tests, and torch's bundled HIP runtime finds no device if it is loaded second.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------ 1. table / header
C_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
             "double": ctypes.c_double}
C_ELEMENTS = {"double": "f8", "int32_t": "i4", "int8_t": "i1", "int64_t": "i8"}


def header_prototypes():
    """{name: (return type, [(const, base type, stars, name), ...])} of every alipmpc_* function in the header."""
    src = open(os.path.join(ROOT, "include", "alipmpc.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*$", " ", src, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r"([\w \t\*]+?)\b(alipmpc_\w+)\s*\(([^)]*)\)\s*;", src):
        parsed = []
        for a in (x.strip() for x in args.split(",")):
            if a in ("", "void"):
                continue
            m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*+)?\s*(\w+)", a)
            assert m, (name, a)
            parsed.append((bool(m.group(1)), m.group(2), len(m.group(3) or ""), m.group(4)))
        assert name not in protos, name
        protos[name] = (re.sub(r"\s+", " ", ret).replace(" *", "*").strip(), parsed)
    return protos


def c_to_ctypes(lib, base, stars):
    if base == "void":
        t, stars = ctypes.c_void_p, stars - 1
    elif base == "alipmpc_cfg":
        t = lib.Cfg
    else:
        t = C_SCALARS[base]
    for _ in range(stars):
        t = ctypes.POINTER(t)
    return t


def test_table_matches_header():
    from alipmpc import _lib as lib
    protos = header_prototypes()
    assert len(protos) == 25
    assert set(protos) == set(lib._ABI), set(protos) ^ set(lib._ABI)
    assert lib.EXPORTS == tuple(lib._ABI)
    returns = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "double": ctypes.c_double,
               "const char*": ctypes.c_char_p, "void": None}
    for name, (ret, cargs) in protos.items():
        entry = lib._ABI[name]
        assert entry.restype is returns[ret], name
        assert len(entry.args) == len(cargs), name
        for a, (const, base, stars, cname) in zip(entry.args, cargs):
            where = f"{name}: {cname}"
            if isinstance(a, lib.Scalar):
                assert a.ctype is c_to_ctypes(lib, base, stars) or a.ctype == c_to_ctypes(lib, base, stars), where
                assert a.name == cname, where
            else:
                assert isinstance(a, lib.Array), where
                assert stars == 1 and a.dtype == np.dtype(C_ELEMENTS[base]), where
                assert a.out == (not const), where          # const pointers are inputs, the others outputs
        if name.endswith("_batch"):
            assert entry.args[0] is lib._HANDLE and entry.args[-1] is lib._STREAM, name
            assert cargs[0][1:] == ("void", 1, "handle") and cargs[-1][1:] == ("void", 1, "hip_stream"), name
            inp_keys, out_keys = lib._DEVICE_PLAN[name][:2]
            arrays = [a for a in entry.args if isinstance(a, lib.Array) and not a.host]
            assert list(inp_keys) == [a.key for a in arrays if not a.out], name
            assert list(out_keys) == [a.key for a in arrays if a.out], name
    # edges is a host pointer in both modes, and the only such argument
    hosts = [(n, a.key) for n, e in lib._ABI.items() for a in e.args if isinstance(a, lib.Array) and a.host]
    assert hosts == [("alipmpc_audit_batch", "edges")]


def test_load_sets_every_prototype_from_the_table():
    from alipmpc import _lib as lib
    L = lib.load()
    for name, entry in lib._ABI.items():
        f = getattr(L, name)
        assert f.restype is entry.restype, name
        assert list(f.argtypes) == [a.ctype if isinstance(a, lib.Scalar) else ctypes.c_void_p for a in entry.args], name
    # every data pointer is a void*: _ptr results, raw addresses and None all pass
    assert L.alipmpc_solve_batch.argtypes == [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 15


# ------------------------------------------------------------------------------------------------ 2. argument vectors
HANDLE, STREAM, ROWS = 0x1234, 0x77, 5
B, S, F = 3, 2, 3


class Recorder:
    """Stands in for the loaded library: every function records its positional arguments and returns 0; the dataset
    call also writes row_start[B], which its host wrapper reads back, and alipmpc_audit_summary_len answers as the
    library does (unrecorded)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            if name == "alipmpc_audit_summary_len":
                return 6 + (args[0] + 1) + 20 if 0 <= args[0] <= 62 else -1
            self.calls.append((name, args))
            if name == "alipmpc_closed_loop_dataset_batch" and args[-2] is not None:
                ctypes.c_int64.from_address(args[-2].value + 8 * args[1]).value = ROWS
            return 0
        return f


CFGS = {"A": (0, dict(nc_max=2, ne_max=1)), "A0": (0, dict(nc_max=2, ne_max=0)), "C0": (0, dict(nc_max=0, ne_max=1)),
        "DD": (2, dict(nc_max=2, ne_max=0))}


def make_solver(lib, cfg_name):
    variant, over = CFGS[cfg_name]
    cfg = lib.default_cfg(variant, 3, **over)
    s = lib.Solver.__new__(lib.Solver)
    s.cfg, s.device, s._L, s._h = cfg, 0, Recorder(), ctypes.c_void_p(HANDLE)
    s.n, s.rps = lib.num_vars(cfg), lib.rows_per_step(cfg)
    s.m_max, s.sdim = cfg.N * s.rps, 3 if variant == 2 else 5
    return s


def host_inputs(s):
    """Array-likes of the shapes a caller passes: goal, leg, cir, nc, elp, ne, last_u, vel_des one instance's, to be
    broadcast; every value distinct so that an argument is recognised by its contents."""
    r = np.random.default_rng(5)
    return dict(x0=r.random((B, s.sdim)), goal=np.array([10.0, 9.0]), leg=-1, cir=r.random((s.cfg.nc_max, 3)) + 1, nc=2,
                elp=r.random((max(s.cfg.ne_max, 1), 5)) + 2, ne=1, u0=r.random((B, s.n)) + 3, u=r.random((B, s.n)) + 4,
                last_u=[0.3, 0.1], foot0=r.random((B, 2)) + 5, status=np.array([0, 1, 2]), x=r.random((B, 5)) + 6,
                vel_des_in=np.array([0.5, 0.05]), edges=(0.0, 0.1), summary=np.arange(29))


TORCH_DTYPES = {"f8": "float64", "i4": "int32", "i1": "int8", "i8": "int64"}


def tensors(tokens):
    """{key: CPU tensor} of the "key:dtype:shape" tokens (None tokens: the key is left out)."""
    import torch
    res = {}
    for t in tokens:
        if t is not None:
            key, dt, shape = t.lstrip(">").split(":")
            res[key] = torch.zeros([int(k) for k in shape.split(",")], dtype=getattr(torch, TORCH_DTYPES[dt]))
    return res


def device_dicts(cfg_name, method, case=None):
    """inp: the scene of the config plus every further input of any wrapper; out: the outputs the case (default: the
    first case of `method`) expects."""
    n = 6 if cfg_name == "DD" else 15
    inp = tensors(SCENE[cfg_name] + ["foot0:f8:3,2", f"u0:f8:3,{n}", f"u:f8:3,{n}", "last_u:f8:3,2", "status:i4:3"])
    want = EXPECT[case or [c for c, v in CASES.items() if v[:2] == (cfg_name, method)][0]][1]
    return ({} if method == "scenes_device" else inp), tensors(t for t in want if isinstance(t, str) and t[0] == ">")


def spec_of(a):
    dt = a.dtype.str[1:] if isinstance(a, np.ndarray) else {"float64": "f8", "int32": "i4", "int8": "i1",
                                                           "int64": "i8"}[str(a.dtype).split(".")[-1]]
    return dt + ":" + ",".join(str(k) for k in a.shape)


def symbolic(args, seen, given, outs):
    """One token per positional argument: a scalar as it was passed, None, "handle", "stream:<value>",
    ">key:dtype:shape" for the array returned / given as output `key`, "key:dtype:shape" for an input whose contents
    are given[key]'s (several keys joined with | where an empty array leaves that open)."""
    toks = []
    for p in args:
        if not isinstance(p, ctypes.c_void_p):
            toks.append(p)
            continue
        if p.value == HANDLE:
            toks.append("handle")
            continue
        if p.value not in seen:
            toks.append(f"stream:{p.value:#x}")
            continue
        a = seen[p.value]
        addr = lambda v: v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data   # noqa: E731
        keys = [">" + k for k, v in outs.items() if v is not None and addr(v) == p.value and v.dtype == a.dtype]
        if not keys:
            keys = [k for k, v in given.items() if v is a]
        if not keys:
            for k, v in given.items():
                g = np.asarray(v)
                try:
                    g = g.reshape(a.shape) if g.size == a.size and g.size else np.broadcast_to(g, a.shape)
                except ValueError:
                    continue
                if np.array_equal(g.astype(a.dtype), a):
                    keys.append(k)
        toks.append("|".join(keys) + ":" + spec_of(a))
    return toks


def layout(res):
    if isinstance(res, dict):
        return [k + ":" + ("None" if v is None else spec_of(v)) for k, v in res.items()]
    if isinstance(res, tuple):
        return [spec_of(v) for v in res]
    return None if res is None else spec_of(res)


def run_case(lib, monkeypatch, case):
    """Calls s.<method> as `call(s, given, inp, out)` does; returns (library function, tokens, layout of the result)."""
    cfg_name, method, call = CASES[case]
    s = make_solver(lib, cfg_name)
    seen, orig = {}, lib._ptr

    def ptr(a):
        p = orig(a)
        if p is not None:
            seen[p.value] = a
        return p
    monkeypatch.setattr(lib, "_ptr", ptr)
    given = host_inputs(s)
    inp, out = device_dicts(cfg_name, method, case) if method.endswith("_device") else ({}, {})
    res = call(s, given, inp, out)
    (name, args), = s._L.calls
    if method.endswith("_device"):
        toks = symbolic(args, seen, dict(inp, edges=given["edges"]), out)
    else:
        outs = res if isinstance(res, dict) else dict(vel_des=res[0], foot=res[1]) if isinstance(res, tuple) \
            else dict(trace=res)
        toks = symbolic(args, seen, given, outs)
    s._h = None
    return name, toks, layout(res)


def scene(g):
    return g["x0"], g["goal"], g["leg"], g["cir"], g["nc"], g["elp"], g["ne"]


def cl_scene(g):
    return (g["x0"], g["foot0"]) + scene(g)[1:]


STREAM_OBJ = types.SimpleNamespace(cuda_stream=STREAM)
NULL_STREAM_OBJ = types.SimpleNamespace(cuda_stream=0)

# case -> (cfg, method, call)
CASES = {
    "solve": ("A", "solve", lambda s, g, i, o: s.solve(*scene(g), u0=g["u0"])),
    "solve/ne_max=0": ("A0", "solve", lambda s, g, i, o: s.solve(*scene(g), u0=g["u0"])),
    "solve/nc_max=0": ("C0", "solve", lambda s, g, i, o: s.solve(*scene(g), u0=g["u0"])),
    "solve/DD": ("DD", "solve", lambda s, g, i, o: s.solve(*scene(g), u0=g["u0"], last_u=g["last_u"])),
    "solve_sens": ("A", "solve_sens", lambda s, g, i, o: s.solve_sens(*scene(g), u0=g["u0"])),
    "solve_sens/no du": ("A", "solve_sens", lambda s, g, i, o: s.solve_sens(*scene(g), u0=g["u0"], want_du=False)),
    "eval": ("A", "eval", lambda s, g, i, o: s.eval(*scene(g), u=g["u"])),
    "eval/no J/ne_max=0": ("A0", "eval", lambda s, g, i, o: s.eval(*scene(g), u=g["u"], want_J=False)),
    "eval/DD": ("DD", "eval", lambda s, g, i, o: s.eval(*scene(g), u=g["u"], last_u=g["last_u"])),
    "rollout": ("A", "rollout", lambda s, g, i, o: s.rollout(*scene(g), u0=g["u0"], steps=S)),
    "rollout/DD": ("DD", "rollout", lambda s, g, i, o: s.rollout(*scene(g), u0=g["u0"], last_u=g["last_u"], steps=S)),
    "closed_loop": ("A", "closed_loop",
                    lambda s, g, i, o: s.closed_loop(*cl_scene(g), steps=S, f_cyc=F, kick=0.25, seed=11)),
    "closed_loop/nc_max=0": ("C0", "closed_loop", lambda s, g, i, o: s.closed_loop(*cl_scene(g), steps=S, f_cyc=F)),
    "closed_loop_schedule": ("A", "closed_loop_schedule", lambda s, g, i, o: s.closed_loop_schedule(
        *cl_scene(g), steps=S, f_cyc=F, mpc_ticks=(0, 2), kick=0.25, seed=11, want_plans=True)),
    "closed_loop_schedule/no plans": ("A0", "closed_loop_schedule", lambda s, g, i, o: s.closed_loop_schedule(
        *cl_scene(g), steps=S, f_cyc=F, mpc_ticks=2)),
    "closed_loop_dataset": ("A", "closed_loop_dataset", lambda s, g, i, o: s.closed_loop_dataset(
        *cl_scene(g), steps=S, f_cyc=F, kick=0.25, seed=11, first=100, safe_dis=0.3)),
    "closed_loop_dataset/max_rows": ("A0", "closed_loop_dataset", lambda s, g, i, o: s.closed_loop_dataset(
        *cl_scene(g), steps=S, f_cyc=F, max_rows=4)),
    "nominal_gait": ("A", "nominal_gait", lambda s, g, i, o: s.nominal_gait(g["x"], g["leg"], vx_max=0.5)),
    "nominal_gait/vel_des": ("A", "nominal_gait", lambda s, g, i, o: s.nominal_gait(g["x"], vel_des=g["vel_des_in"])),
    "trace": ("A", "trace", lambda s, g, i, o: s.trace(g["x0"], g["u"])),
    "audit": ("A", "audit", lambda s, g, i, o: s.audit(*scene(g), u=g["u"], status=g["status"], edges=g["edges"],
                                                       viol_tol=1e-3, summary=g["summary"])),
    "audit/no edges/ne_max=0": ("A0", "audit", lambda s, g, i, o: s.audit(*scene(g), u=g["u"])),
    "scenes": ("A", "scenes", lambda s, g, i, o: s.scenes(B, seed=9, first=4, n_elp=1, fields=2, max_candidates=50)),
    "scenes/ne_max=0": ("A0", "scenes", lambda s, g, i, o: s.scenes(B, n_cir=1)),
    "scenes/nc_max=0": ("C0", "scenes", lambda s, g, i, o: s.scenes(B)),
    "solve_device": ("A", "solve_device", lambda s, g, i, o: s.solve_device(i, o, stream=STREAM_OBJ)),
    "solve_device/null stream": ("A", "solve_device", lambda s, g, i, o: s.solve_device(i, o, stream=NULL_STREAM_OBJ)),
    "solve_device/DD": ("DD", "solve_device", lambda s, g, i, o: s.solve_device(i, o, stream=STREAM_OBJ)),
    "solve_sens_device": ("A", "solve_sens_device", lambda s, g, i, o: s.solve_sens_device(i, o, stream=STREAM_OBJ)),
    "eval_device": ("A", "eval_device", lambda s, g, i, o: s.eval_device(i, o, stream=STREAM_OBJ)),
    "rollout_device": ("A", "rollout_device", lambda s, g, i, o: s.rollout_device(i, o, S, stream=STREAM_OBJ)),
    "closed_loop_device": ("A", "closed_loop_device", lambda s, g, i, o: s.closed_loop_device(
        i, o, S, f_cyc=F, kick=0.25, seed=11, stream=STREAM_OBJ)),
    "closed_loop_schedule_device": (
        "A", "closed_loop_schedule_device", lambda s, g, i, o: s.closed_loop_schedule_device(
        i, o, S, f_cyc=F, mpc_ticks=(1,), kick=0.25, seed=11, stream=NULL_STREAM_OBJ)),
    "closed_loop_dataset_device": ("A", "closed_loop_dataset_device", lambda s, g, i, o: s.closed_loop_dataset_device(
        i, o, S, f_cyc=F, kick=0.25, seed=11, first=100, safe_dis=0.3, stream=STREAM_OBJ)),
    "closed_loop_dataset_device/max_rows": ("A", "closed_loop_dataset_device", lambda s, g, i, o:
        s.closed_loop_dataset_device(i, o, S, f_cyc=F, max_rows=6, stream=STREAM_OBJ)),
    "trace_device": (
        "A", "trace_device", lambda s, g, i, o: s.trace_device(i["x0"], i["u"], o["trace"], stream=STREAM_OBJ)),
    "audit_device": ("A", "audit_device", lambda s, g, i, o: s.audit_device(i, o, edges=g["edges"], viol_tol=1e-3,
                                                                            stream=STREAM_OBJ)),
    "audit_device/no edges": ("A", "audit_device", lambda s, g, i, o: s.audit_device(i, o, stream=STREAM_OBJ)),
    "scenes_device": ("A", "scenes_device", lambda s, g, i, o: s.scenes_device(
        o, seed=9, first=4, n_elp=1, fields=2, max_candidates=50, stream=STREAM_OBJ)),
}

# The expectations: (library function, one token per positional argument as symbolic() gives them, result layout).
SCENE = {"A": ["x0:f8:3,5", "goal:f8:3,2", "leg:i1:3", "cir:f8:3,2,3", "nc:i4:3", "elp:f8:3,1,5", "ne:i4:3"],
         "A0": ["x0:f8:3,5", "goal:f8:3,2", "leg:i1:3", "cir:f8:3,2,3", "nc:i4:3", None, None],
         "C0": ["x0:f8:3,5", "goal:f8:3,2", "leg:i1:3", "cir:f8:3,0,3", "nc:i4:3", "elp:f8:3,1,5", "ne:i4:3"],
         "DD": ["x0:f8:3,3", "goal:f8:3,2", "leg:i1:3", "cir:f8:3,2,3", "nc:i4:3", None, None]}
CL_SCENE = {c: v[:1] + ["foot0:f8:3,2"] + v[1:] for c, v in SCENE.items()}
SOLVE_OUT = [">u:f8:3,15", ">foot:f8:3,3", ">x_pred:f8:3,3,5", ">status:i4:3", ">iters:i4:3"]
SOLVE_OUT_DD = [">u:f8:3,6", ">foot:f8:3,3", ">x_pred:f8:3,3,3", ">status:i4:3", ">iters:i4:3"]
EVAL_OUT = [">f:f8:3", ">grad:f8:3,15", ">c:f8:3,24", ">J:f8:3,24,15", ">cl:f8:3,24", ">cu:f8:3,24", ">goal_eff:f8:3,2",
            ">row_active:i1:3,24"]
EVAL_OUT_A0 = [">f:f8:3", ">grad:f8:3,15", ">c:f8:3,21", None, ">cl:f8:3,21", ">cu:f8:3,21", ">goal_eff:f8:3,2",
               ">row_active:i1:3,21"]
EVAL_OUT_DD = [">f:f8:3", ">grad:f8:3,6", ">c:f8:3,9", ">J:f8:3,9,6", ">cl:f8:3,9", ">cu:f8:3,9", ">goal_eff:f8:3,2",
               ">row_active:i1:3,9"]
ROLL_OUT = [">foot:f8:3,2,3", ">x:f8:3,3,5", ">status:i4:3,2", ">iters:i4:3,2", ">steps_to_goal:i4:3", ">u:f8:3,2,15"]
ROLL_OUT_DD = [">foot:f8:3,2,3", ">x:f8:3,3,3", ">status:i4:3,2", ">iters:i4:3,2", ">steps_to_goal:i4:3", ">u:f8:3,2,6"]
CL_OUT = [">foot:f8:3,2,3", ">x:f8:3,3,5", ">hd:f8:3,2,2", ">status:i4:3,2,3", ">iters:i4:3,2,3", ">steps_to_goal:i4:3",
          ">action:f8:3,2,3,8"]
AUDIT_OUT = [">metrics:f8:3,5", ">where:i4:3,3"]
SCENES_OUT = {"A": [">x0:f8:3,5", ">goal:f8:3,2", ">leg:i1:3", ">cir:f8:3,2,3", ">nc:i4:3", ">elp:f8:3,1,5", ">ne:i4:3",
                    ">u0:f8:3,15"],
              "A0": [">x0:f8:3,5", ">goal:f8:3,2", ">leg:i1:3", ">cir:f8:3,2,3", ">nc:i4:3", None, None, ">u0:f8:3,15"],
              "C0": [">x0:f8:3,5", ">goal:f8:3,2", ">leg:i1:3", ">cir:f8:3,0,3", ">nc:i4:3", ">elp:f8:3,1,5",
                     ">ne:i4:3", ">u0:f8:3,15"]}
H, ST, ST0 = "handle", "stream:0x77", "stream:0xffffffffffffffff"


def returned(*outs, **changed):
    """Layout of a host wrapper's dict: the output tokens in order, `changed` where the wrapper trims or leaves out."""
    return [changed.get(t[1:].split(":")[0], t[1:]) for o in outs for t in o]


EXPECT = {
    "solve": (
        "alipmpc_solve_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", None] + SOLVE_OUT + [None], returned(SOLVE_OUT)),
    "solve/ne_max=0": ("alipmpc_solve_batch", [H, 3] + SCENE["A0"] + ["u0:f8:3,15", None] + SOLVE_OUT + [None],
                       returned(SOLVE_OUT)),
    "solve/nc_max=0": ("alipmpc_solve_batch", [H, 3] + SCENE["C0"] + ["u0:f8:3,15", None] + SOLVE_OUT + [None],
                       returned(SOLVE_OUT)),
    "solve/DD": ("alipmpc_solve_batch", [H, 3] + SCENE["DD"] + ["u0:f8:3,6", "last_u:f8:3,2"] + SOLVE_OUT_DD + [None],
                 returned(SOLVE_OUT_DD)),
    "solve_sens": ("alipmpc_solve_sens_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", None] + SOLVE_OUT + [
        ">dfoot:f8:3,3,7", ">du:f8:3,15,7", ">sens_ok:i4:3", None],
        returned(SOLVE_OUT, [">dfoot:f8:3,3,7", ">du:f8:3,15,7", ">sens_ok:i4:3"])),
    "solve_sens/no du": ("alipmpc_solve_sens_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", None] + SOLVE_OUT + [
        ">dfoot:f8:3,3,7", None, ">sens_ok:i4:3", None],
        returned(SOLVE_OUT, [">dfoot:f8:3,3,7", ">du:f8:3,15,7", ">sens_ok:i4:3"], du="du:None")),
    "eval": ("alipmpc_eval_batch", [H, 3] + SCENE["A"] + ["u:f8:3,15", None] + EVAL_OUT + [None], returned(EVAL_OUT)),
    "eval/no J/ne_max=0": ("alipmpc_eval_batch", [H, 3] + SCENE["A0"] + ["u:f8:3,15", None] + EVAL_OUT_A0 + [None],
                           ["f:f8:3", "grad:f8:3,15", "c:f8:3,21", "J:None", "cl:f8:3,21", "cu:f8:3,21",
                            "goal_eff:f8:3,2", "row_active:i1:3,21"]),
    "eval/DD": ("alipmpc_eval_batch", [H, 3] + SCENE["DD"] + ["u:f8:3,6", "last_u:f8:3,2"] + EVAL_OUT_DD + [None],
                returned(EVAL_OUT_DD)),
    "rollout": ("alipmpc_rollout_batch", [H, 3, 2] + SCENE["A"] + ["u0:f8:3,15", None] + ROLL_OUT + [None],
                returned(ROLL_OUT)),
    "rollout/DD": (
        "alipmpc_rollout_batch", [H, 3, 2] + SCENE["DD"] + ["u0:f8:3,6", "last_u:f8:3,2"] + ROLL_OUT_DD + [None],
                   returned(ROLL_OUT_DD)),
    "closed_loop": (
        "alipmpc_closed_loop_batch", [H, 3, 2, 3, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [None], returned(CL_OUT)),
    "closed_loop/nc_max=0": ("alipmpc_closed_loop_batch", [H, 3, 2, 3, 0.0, 0] + CL_SCENE["C0"] + CL_OUT + [None],
                             returned(CL_OUT)),
    "closed_loop_schedule": (
        "alipmpc_closed_loop_schedule_batch", [H, 3, 2, 3, 5, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [
        ">plan:f8:3,2,3,15", None], returned(CL_OUT, [">plan:f8:3,2,3,15"])),
    "closed_loop_schedule/no plans": (
        "alipmpc_closed_loop_schedule_batch", [H, 3, 2, 3, 2, 0.0, 0] + CL_SCENE["A0"] + CL_OUT + [
        None, None], returned(CL_OUT, [">plan:f8:3,2,3,15"], plan="plan:None")),
    # max_rows defaulted: B * S * f_cyc = 18 rows allocated, trimmed to the ROWS = 5 the library reported
    "closed_loop_dataset": ("alipmpc_closed_loop_dataset_batch", [H, 3, 2, 3, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [
        100, 0.3, 18, ">X:f8:18,22", ">y_mpc:f8:18,8", ">y_act:f8:18,8", ">row_status:i4:18", ">row_start:i8:4", None],
        returned(CL_OUT) + ["X:f8:5,22", "y_mpc:f8:5,8", "y_act:f8:5,8", "row_status:i4:5", "row_start:i8:4"]),
    # max_rows = 4 given: 4 rows allocated, R = min(5, 4)
    "closed_loop_dataset/max_rows": (
        "alipmpc_closed_loop_dataset_batch", [H, 3, 2, 3, 0.0, 0] + CL_SCENE["A0"] + CL_OUT + [
        0, 0.4, 4, ">X:f8:4,17", ">y_mpc:f8:4,8", ">y_act:f8:4,8", ">row_status:i4:4", ">row_start:i8:4", None],
        returned(CL_OUT) + ["X:f8:4,17", "y_mpc:f8:4,8", "y_act:f8:4,8", "row_status:i4:4", "row_start:i8:4"]),
    "nominal_gait": ("alipmpc_nominal_gait_batch", [H, 3, 0.5, "x:f8:3,5", "leg:i1:3", None, ">vel_des:f8:3,2",
                                                    ">foot:f8:3,2", None], ["f8:3,2", "f8:3,2"]),
    "nominal_gait/vel_des": ("alipmpc_nominal_gait_batch", [H, 3, 0.6, "x:f8:3,5", None, "vel_des_in:f8:3,2",
                                                            ">vel_des:f8:3,2", ">foot:f8:3,2", None],
                             ["f8:3,2", "f8:3,2"]),
    "trace": ("alipmpc_trace_batch", [H, 3, "x0:f8:3,5", "u:f8:3,15", ">trace:f8:3,3,42,2", None], "f8:3,3,42,2"),
    "audit": ("alipmpc_audit_batch", [H, 3] + SCENE["A"] + ["u:f8:3,15", "status:i4:3"] + AUDIT_OUT + [
        0.001, "edges:f8:2", 2, ">summary:i8:29", None], returned(AUDIT_OUT, [">summary:i8:29"])),
    "audit/no edges/ne_max=0": ("alipmpc_audit_batch", [H, 3] + SCENE["A0"] + ["u:f8:3,15", None] + AUDIT_OUT + [
        0.0001, None, 0, ">summary:i8:27", None], returned(AUDIT_OUT, [">summary:i8:27"])),
    "scenes": ("alipmpc_scenes_batch", [H, 3, 9, 4, 2, 1, 2, 50] + SCENES_OUT["A"] + [None], returned(SCENES_OUT["A"])),
    "scenes/ne_max=0": ("alipmpc_scenes_batch", [H, 3, 0, 0, 1, 0, 0, 0] + SCENES_OUT["A0"] + [None],
                        ["x0:f8:3,5", "goal:f8:3,2", "leg:i1:3", "cir:f8:3,2,3", "nc:i4:3", "elp:None", "ne:None",
                         "u0:f8:3,15"]),
    "scenes/nc_max=0": ("alipmpc_scenes_batch", [H, 3, 0, 0, 0, 0, 0, 0] + SCENES_OUT["C0"] + [None],
                        returned(SCENES_OUT["C0"])),
    "solve_device": (
        "alipmpc_solve_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", "last_u:f8:3,2"] + SOLVE_OUT + [ST], None),
    "solve_device/null stream": (
        "alipmpc_solve_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", "last_u:f8:3,2"] + SOLVE_OUT + [
        ST0], None),
    "solve_device/DD": (
        "alipmpc_solve_batch", [H, 3] + SCENE["DD"] + ["u0:f8:3,6", "last_u:f8:3,2"] + SOLVE_OUT_DD + [ST],
                        None),
    "solve_sens_device": (
        "alipmpc_solve_sens_batch", [H, 3] + SCENE["A"] + ["u0:f8:3,15", "last_u:f8:3,2"] + SOLVE_OUT + [
        ">dfoot:f8:3,3,7", ">du:f8:3,15,7", ">sens_ok:i4:3", ST], None),
    "eval_device": ("alipmpc_eval_batch", [H, 3] + SCENE["A"] + ["u:f8:3,15", "last_u:f8:3,2"] + EVAL_OUT + [ST], None),
    "rollout_device": (
        "alipmpc_rollout_batch", [H, 3, 2] + SCENE["A"] + ["u0:f8:3,15", "last_u:f8:3,2"] + ROLL_OUT + [ST],
                       None),
    "closed_loop_device": ("alipmpc_closed_loop_batch", [H, 3, 2, 3, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [ST], None),
    "closed_loop_schedule_device": (
        "alipmpc_closed_loop_schedule_batch", [H, 3, 2, 3, 2, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [
        ">plan:f8:3,2,3,15", ST0], None),
    # max_rows defaulted: the smallest leading size of the row tensors given (7, 9, 8, 8)
    "closed_loop_dataset_device": (
        "alipmpc_closed_loop_dataset_batch", [H, 3, 2, 3, 0.25, 11] + CL_SCENE["A"] + CL_OUT + [
        100, 0.3, 7, ">X:f8:7,22", ">y_mpc:f8:9,8", ">y_act:f8:8,8", ">row_status:i4:8", ">row_start:i8:4", ST], None),
    "closed_loop_dataset_device/max_rows": (
        "alipmpc_closed_loop_dataset_batch", [H, 3, 2, 3, 0.0, 0] + CL_SCENE["A"] + CL_OUT + [
        0, 0.4, 6, ">X:f8:7,22", ">y_mpc:f8:9,8", ">y_act:f8:8,8", ">row_status:i4:8", ">row_start:i8:4", ST], None),
    "trace_device": ("alipmpc_trace_batch", [H, 3, "x0:f8:3,5", "u:f8:3,15", ">trace:f8:3,3,42,2", ST], None),
    "audit_device": ("alipmpc_audit_batch", [H, 3] + SCENE["A"] + ["u:f8:3,15", "status:i4:3"] + AUDIT_OUT + [
        0.001, "edges:f8:2", 2, ">summary:i8:29", ST], None),
    "audit_device/no edges": ("alipmpc_audit_batch", [H, 3] + SCENE["A"] + ["u:f8:3,15", "status:i4:3"] + AUDIT_OUT + [
        0.0001, None, 0, ">summary:i8:27", ST], None),
    "scenes_device": ("alipmpc_scenes_batch", [H, 3, 9, 4, 2, 1, 2, 50] + SCENES_OUT["A"] + [ST], None),
}


def test_every_wrapper_has_a_case():
    from alipmpc import _lib as lib
    wrappers = {m for m in vars(lib.Solver) if not m.startswith("_") and m not in (
        "close", "last_kernel_ms", "solve_program", "solve_slots", "solve_launches", "lane_handoffs", "x_cols")}
    assert len(wrappers) == 21 and wrappers == {c[1] for c in CASES.values()}
    assert set(CASES) == set(EXPECT)


@pytest.mark.parametrize("case", list(CASES))
def test_wrapper_argument_vector(case, monkeypatch):
    from alipmpc import _lib as lib
    name, toks, res = run_case(lib, monkeypatch, case)
    want_name, want_toks, want_res = EXPECT[case]
    assert name == want_name
    assert len(toks) == len(want_toks)
    for k, (got, want) in enumerate(zip(toks, want_toks)):
        if isinstance(want, str) and ":" in want and not want.startswith("stream:"):
            key, _, spec = want.partition(":")
            gkeys, _, gspec = got.partition(":")
            assert key in gkeys.split("|") and gspec == spec, (k, got, want)
        else:
            assert type(got) is type(want) and got == want, (k, got, want)
    assert res == want_res


# ------------------------------------------------------------------------------------------------ 3. missing keys
@pytest.mark.parametrize("method, key", [("solve_device", "x0"), ("solve_device", "leg"), ("solve_device", "u0"),
                                         ("solve_device", ">u"), ("solve_sens_device", ">dfoot"), ("eval_device", "u"),
                                         ("rollout_device", "u0"), ("closed_loop_device", "foot0"),
                                         ("audit_device", "cir")])
def test_device_call_without_a_required_key_raises(method, key, monkeypatch):
    from alipmpc import _lib as lib
    s = make_solver(lib, "A")
    inp, out = device_dicts("A", method)
    del (out if key[0] == ">" else inp)[key.lstrip(">")]
    args = (inp, out, S) if method in ("rollout_device", "closed_loop_device") else (inp, out)
    with pytest.raises(KeyError):
        getattr(s, method)(*args, stream=STREAM_OBJ)
    assert s._L.calls == []
    s._h = None


def test_device_call_without_optional_keys_passes_null(monkeypatch):
    from alipmpc import _lib as lib
    s = make_solver(lib, "A")
    inp, out = device_dicts("A", "solve_device")
    inp = {k: inp[k] for k in ("x0", "goal", "cir", "nc", "u0")}        # rollout: leg, elp, ne, last_u optional
    s.rollout_device(inp, {}, S, stream=STREAM_OBJ)
    inp["leg"] = None                                       # solve: the key is required, its value may be None
    s.solve_device(inp, {"u": out["u"]}, stream=STREAM_OBJ)
    (_, a), (_, b) = s._L.calls
    assert [p is None for p in a] == [False] * 5 + [True, False, False, True, True, False] + [True] * 7 + [False]
    assert [p is None for p in b] == ([False] * 4 + [True, False, False, True, True, False, True, False] + [True] * 4 +
                                      [False])
    s._h = None


def test_audit_leaves_a_refused_edge_count_to_the_call():
    """More than 62 edges: alipmpc_audit_summary_len has no length for them; the wrapper still makes the call, whose
    EINVAL is the error the caller sees (tests/test_plan_audit_gpu.py::test_errors), and a summary of the wrong
    length for a valid count stays a ValueError before any call."""
    from alipmpc import _lib as lib
    s = make_solver(lib, "A")
    g = host_inputs(s)
    s.audit(*scene(g), u=g["u"], edges=np.linspace(0.0, 1.0, 63))
    (name, args), = s._L.calls
    assert name == "alipmpc_audit_batch" and args[15] == 63 and args[14] is not None and args[16] is not None
    with pytest.raises(ValueError, match="29 expected for 2 edges"):
        s.audit(*scene(g), u=g["u"], edges=(0.0, 1.0), summary=np.zeros(5))
    assert len(s._L.calls) == 1
    s._h = None
