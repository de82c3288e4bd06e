"""GPU: the counter-based scene generator kernel (csrc/scenes.inc, alipmpc_scenes_batch) against its host
restatement (alipmpc/scenes.py: make_batch_counter), its shard invariance, and a solve straight from its buffers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("x0", "goal", "leg", "cir", "nc", "elp", "ne", "u0")
# x0[:, 2:5] pass through log / sqrt / cos / sin / atan2: device and libm results differ by a few ulp on values of
# magnitude <= 5 (<= 1e-14); everything else uses + - * /, rint and comparisons only and matches bit for bit
ATOL_TRANSCENDENTAL = 1e-12


def _same(a, b, lo=None, hi=None):
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k][lo:hi]), k


def _solver(gpu_lib, n_cir, n_elp, N=3, variant=0):
    return gpu_lib.Solver(gpu_lib.default_cfg(variant, N, nc_max=n_cir, ne_max=n_elp))


def _device_buffers(s, B, dev="cuda"):
    import torch
    cfg = s.cfg
    out = dict(x0=torch.full((B, 5), np.nan, dtype=torch.float64, device=dev),
               goal=torch.full((B, 2), np.nan, dtype=torch.float64, device=dev),
               leg=torch.zeros(B, dtype=torch.int8, device=dev),
               cir=torch.full((B, cfg.nc_max, 3), np.nan, dtype=torch.float64, device=dev),
               nc=torch.full((B,), -1, dtype=torch.int32, device=dev),
               u0=torch.full((B, 5 * cfg.N), np.nan, dtype=torch.float64, device=dev))
    if cfg.ne_max:
        out["elp"] = torch.full((B, cfg.ne_max, 5), np.nan, dtype=torch.float64, device=dev)
        out["ne"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    return out


def _to_host(out):
    return {k: out[k].cpu().numpy() if out.get(k) is not None else None for k in KEYS}


@pytest.mark.parametrize("B,n_cir,n_elp,N,kw", [
    (4096, 5, 0, 3, dict(seed=11)),
    (512, 5, 5, 5, dict(seed=12, fields=64)),
    (1000, 5, 0, 3, dict(seed=13, first=123457)),
    (2048, 5, 0, 3, dict(seed=14, max_candidates=8)),
], ids=["circles", "mix_fields64", "first123457", "short_fields"])
def test_device_scenes_match_host_restatement(gpu_lib, B, n_cir, n_elp, N, kw):
    from alipmpc import scenes
    s = _solver(gpu_lib, n_cir, n_elp, N)
    dev = s.scenes(B, n_cir=n_cir, n_elp=n_elp, **kw)
    ref = scenes.make_batch_counter(B, n_cir=n_cir, n_elp=n_elp, N=N, **kw)
    for k in ("leg", "nc", "ne", "cir", "elp", "goal"):
        if ref[k] is None:
            assert dev[k] is None, k
        else:
            assert dev[k].dtype == ref[k].dtype and np.array_equal(dev[k], ref[k]), k
    assert np.array_equal(dev["x0"][:, :2], ref["x0"][:, :2])
    err = np.abs(dev["x0"][:, 2:5] - ref["x0"][:, 2:5]).max()
    print(f"x0[:, 2:5] max |device - host| = {err:.3e}")
    assert err <= ATOL_TRANSCENDENTAL
    u0d, u0r = dev["u0"].reshape(B, N, 5), ref["u0"].reshape(B, N, 5)
    assert np.array_equal(u0d[:, :, :2], u0r[:, :, :2])
    assert np.abs(u0d[:, :, 2:5] - u0r[:, :, 2:5]).max() <= ATOL_TRANSCENDENTAL
    assert np.array_equal(dev["u0"], np.tile(dev["x0"], (1, N)))
    if "max_candidates" in kw:
        assert np.any(dev["nc"] < n_cir) and np.any(dev["nc"] == n_cir)


def test_device_scenes_are_shard_invariant(gpu_lib):
    import torch
    s = _solver(gpu_lib, 5, 5, 5)
    kw = dict(seed=21, n_cir=5, n_elp=5, fields=40)
    whole = s.scenes(700, first=1000, **kw)
    for lo, hi in ((0, 1), (1, 130), (130, 700)):
        _same(s.scenes(hi - lo, first=1000 + lo, **kw), whole, lo, hi)
    # device pointers on a non-default stream: the same bits as the host-pointer form
    out = _device_buffers(s, 570)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())     # the fills above
    with torch.cuda.stream(st):
        s.scenes_device(out, first=1130, stream=st, **kw)
    st.synchronize()
    _same(_to_host(out), whole, 130, 700)
    # ... and on the current (default) stream
    out = _device_buffers(s, 129)
    s.scenes_device(out, first=1001, **kw)
    torch.cuda.synchronize()
    _same(_to_host(out), whole, 1, 130)


def test_solve_from_generated_device_buffers(gpu_lib, coracle):
    import torch
    from test_gpu import _oracle_solve, _compare     # the existing parity comparison, unchanged
    B = 2048
    s = _solver(gpu_lib, 5, 0)
    inp = _device_buffers(s, B)
    out = dict(u=torch.zeros((B, s.n), dtype=torch.float64, device="cuda"),
               foot=torch.zeros((B, 3), dtype=torch.float64, device="cuda"),
               x_pred=torch.zeros((B, 3, 5), dtype=torch.float64, device="cuda"),
               status=torch.zeros(B, dtype=torch.int32, device="cuda"),
               iters=torch.zeros(B, dtype=torch.int32, device="cuda"))
    s.scenes_device(inp, seed=31)
    s.solve_device(inp, out)                 # same stream: reads what the generator wrote, no copy
    torch.cuda.synchronize()
    bt = _to_host(inp)
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    host = s.solve(bt["x0"], bt["goal"], bt["leg"], bt["cir"], bt["nc"], u0=bt["u0"])
    for k in ("u", "foot", "x_pred", "status", "iters"):
        assert np.array_equal(dev[k], host[k], equal_nan=True), k
    bt = {k: v for k, v in bt.items() if v is not None}
    ref = _oracle_solve(coracle, dict(variant=0, N=3, nc_max=5, ne_max=0), bt)
    _compare(dev, ref)


def test_scenes_argument_errors(gpu_lib):
    s = _solver(gpu_lib, 5, 5)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=6)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=5, n_elp=3)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=5, max_candidates=2 ** 18 + 1)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=5, first=-1)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=5, first=2 ** 40 - 7)
    with pytest.raises(RuntimeError, match="EINVAL"):
        s.scenes(8, n_cir=5, fields=-1)
    assert s.scenes(8, n_cir=5, first=2 ** 40 - 8, max_candidates=2 ** 18)["nc"].tolist() == [5] * 8
    assert s.scenes(0, n_cir=5)["x0"].shape == (0, 5)
    dd = gpu_lib.Solver(gpu_lib.default_cfg(2, 3, nc_max=5, ne_max=0))
    with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
        dd.scenes(8, n_cir=5)


def test_scenes_null_optional_outputs(gpu_lib):
    import torch
    s = _solver(gpu_lib, 5, 5, 5)
    kw = dict(seed=41, n_cir=5, n_elp=5, fields=16)
    B = 200
    whole = s.scenes(B, **kw)
    for keep in (("x0", "leg"), ("cir", "nc", "u0"), ("elp", "ne", "goal")):
        out = {k: v for k, v in _device_buffers(s, B).items() if k in keep}
        s.scenes_device(out, **kw)
        torch.cuda.synchronize()
        for k in keep:
            assert np.array_equal(out[k].cpu().numpy(), whole[k]), k
    # the host-pointer form with NULL outputs, through the C ABI directly
    x0, nc = np.zeros((B, 5)), np.zeros(B, np.int32)
    rc = s._L.alipmpc_scenes_batch(s._h, B, 41, 0, 5, 5, 16, 0, x0.ctypes.data, None, None, None, nc.ctypes.data,
                                   None, None, None, None)
    assert rc == 0 and np.array_equal(x0, whole["x0"]) and np.array_equal(nc, whole["nc"])
