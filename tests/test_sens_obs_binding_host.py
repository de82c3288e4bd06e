"""The binding of the extension header include/alipmpc_sens_obs.h (alipmpc_sens_obs_cols, alipmpc_solve_sens_obs_batch):
what test_binding_host.py holds for alipmpc.h and the table _ABI, held here for that header and the table _ABI_EXT, with
that module's own parser rules, recorder and token comparison.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import test_binding_host as TB

HEADER = os.path.join(TB.ROOT, "include", "alipmpc_sens_obs.h")


def ext_prototypes():
    """header_prototypes of test_binding_host.py, on the extension header"""
    src = open(HEADER).read()
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


def test_ext_table_matches_its_header():
    from alipmpc import _lib as lib
    protos = ext_prototypes()
    assert set(protos) == set(lib._ABI_EXT) == {"alipmpc_sens_obs_cols", "alipmpc_solve_sens_obs_batch"}
    assert lib.EXPORTS_EXT == tuple(lib._ABI_EXT)
    assert not set(lib._ABI_EXT) & set(lib._ABI) and not set(protos) & set(TB.header_prototypes())
    # alipmpc.h brings the extension header along
    assert re.search(r'^#include "alipmpc_sens_obs.h"$', open(os.path.join(TB.ROOT, "include", "alipmpc.h")).read(), re.M)
    returns = {"int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for name, (ret, cargs) in protos.items():
        entry = lib._ABI_EXT[name]
        assert entry.restype is returns[ret], name
        assert len(entry.args) == len(cargs), name
        for a, (const, base, stars, cname) in zip(entry.args, cargs):
            where = f"{name}: {cname}"
            if isinstance(a, lib.Scalar):
                assert a.ctype is TB.c_to_ctypes(lib, base, stars) or a.ctype == TB.c_to_ctypes(lib, base, stars), where
                assert a.name == cname, where
            else:
                assert isinstance(a, lib.Array) and not a.host, where
                assert stars == 1 and a.dtype == np.dtype(TB.C_ELEMENTS[base]), where
                assert a.out == (not const), where
    name = "alipmpc_solve_sens_obs_batch"
    entry, cargs = lib._ABI_EXT[name], protos[name][1]
    assert entry.args[0] is lib._HANDLE and entry.args[-1] is lib._STREAM
    assert cargs[0][1:] == ("void", 1, "handle") and cargs[-1][1:] == ("void", 1, "hip_stream")
    inp_keys, out_keys = lib._DEVICE_PLAN[name][:2]
    arrays = [a for a in entry.args if isinstance(a, lib.Array)]
    assert list(inp_keys) == [a.key for a in arrays if not a.out]
    assert list(out_keys) == [a.key for a in arrays if a.out]
    # solve_sens' arguments, then the two obstacle outputs
    sens = lib._ABI["alipmpc_solve_sens_batch"].args
    assert [getattr(a, "key", a) for a in entry.args[:len(sens) - 1]] == [getattr(a, "key", a) for a in sens[:-1]]
    assert [a.key for a in entry.args[len(sens) - 1:-1]] == ["dfoot_obs", "du_obs"]
    required = [a.key for a in arrays if a.out and not a.opt]
    assert required == ["u", "dfoot_obs"]


def test_load_sets_the_ext_prototypes():
    from alipmpc import _lib as lib
    L = lib.load()
    for name, entry in lib._ABI_EXT.items():
        f = getattr(L, name)
        assert f.restype is entry.restype, name
        assert list(f.argtypes) == [a.ctype if isinstance(a, lib.Scalar) else ctypes.c_void_p for a in entry.args], name
    assert L.alipmpc_solve_sens_obs_batch.argtypes == [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 20
    cfg = lib.default_cfg(0, 3, nc_max=4, ne_max=3)
    assert L.alipmpc_sens_obs_cols(ctypes.byref(cfg)) == 27 and L.alipmpc_sens_obs_cols(None) == 0


H, ST = TB.H, TB.ST
SENS = [">dfoot:f8:3,3,7", ">du:f8:3,15,7", ">sens_ok:i4:3"]
OBS = [">dfoot_obs:f8:3,3,11", ">du_obs:f8:3,15,11"]    # cfg A: 2 circle slots, 1 ellipse slot
CASES = {
    "solve_sens_obs": ("A", "solve_sens_obs", lambda s, g, i, o: s.solve_sens_obs(*TB.scene(g), u0=g["u0"])),
    "solve_sens_obs/obstacle columns only": ("A", "solve_sens_obs", lambda s, g, i, o: s.solve_sens_obs(
        *TB.scene(g), u0=g["u0"], want_du=False, want_state=False)),
    "solve_sens_obs/no du": ("A", "solve_sens_obs", lambda s, g, i, o: s.solve_sens_obs(
        *TB.scene(g), u0=g["u0"], want_du=False)),
    "solve_sens_obs_device": ("A", "solve_sens_obs_device",
                              lambda s, g, i, o: s.solve_sens_obs_device(i, o, stream=TB.STREAM_OBJ)),
}
HEAD = [H, 3] + TB.SCENE["A"] + ["u0:f8:3,15", None] + TB.SOLVE_OUT
EXPECT = {
    "solve_sens_obs": ("alipmpc_solve_sens_obs_batch", HEAD + SENS + OBS + [None], TB.returned(TB.SOLVE_OUT, SENS, OBS)),
    "solve_sens_obs/obstacle columns only": (
        "alipmpc_solve_sens_obs_batch", HEAD + [None, None, None, OBS[0], None, None],
        TB.returned(TB.SOLVE_OUT, SENS, OBS, dfoot="dfoot:None", du="du:None", sens_ok="sens_ok:None",
                    du_obs="du_obs:None")),
    "solve_sens_obs/no du": (
        "alipmpc_solve_sens_obs_batch", HEAD + [SENS[0], None, SENS[2], OBS[0], None, None],
        TB.returned(TB.SOLVE_OUT, SENS, OBS, du="du:None", du_obs="du_obs:None")),
    "solve_sens_obs_device": (
        "alipmpc_solve_sens_obs_batch", [H, 3] + TB.SCENE["A"] + ["u0:f8:3,15", "last_u:f8:3,2"] + TB.SOLVE_OUT + SENS
        + OBS + [ST], None),
}


def test_every_ext_wrapper_has_a_case():
    from alipmpc import _lib as lib
    wrappers = {m for m in vars(lib._SensObsCalls) if not m.startswith("_") and m != "sens_obs_cols"}
    assert wrappers == {c[1] for c in CASES.values()} and set(CASES) == set(EXPECT)
    assert all(callable(getattr(lib.Solver, m)) for m in wrappers) and isinstance(lib.Solver.sens_obs_cols, property)


@pytest.mark.parametrize("case", list(CASES))
def test_ext_wrapper_argument_vector(case, monkeypatch):
    from alipmpc import _lib as lib
    monkeypatch.setitem(TB.CASES, case, CASES[case])     # test_binding_host's run_case reads its own tables
    monkeypatch.setitem(TB.EXPECT, case, EXPECT[case])
    name, toks, res = TB.run_case(lib, monkeypatch, case)
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


def test_device_call_needs_dfoot_obs_only(monkeypatch):
    from alipmpc import _lib as lib
    s = TB.make_solver(lib, "A")
    inp, out = TB.tensors(TB.SCENE["A"] + ["u0:f8:3,15"]), TB.tensors([">u:f8:3,15", OBS[0]])
    s.solve_sens_obs_device(inp, out, stream=TB.STREAM_OBJ)
    (name, args), = s._L.calls
    assert name == "alipmpc_solve_sens_obs_batch" and sum(a is None for a in args) == 9   # last_u, 4 + 3 + 1 outputs
    with pytest.raises(KeyError):
        s.solve_sens_obs_device(inp, {k: v for k, v in out.items() if k != "dfoot_obs"}, stream=TB.STREAM_OBJ)
    s._h = None
