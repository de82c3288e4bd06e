"""CPU: the counter-based scene stream's host restatement (alipmpc/scenes.py: counter_uniform,
make_batch_counter; include/alipmpc.h: alipmpc_scenes_batch states the stream)."""
import numpy as np
import pytest

KEYS = ("x0", "goal", "leg", "cir", "nc", "elp", "ne", "u0")


def _same(a, b):
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k]), k


def _cat(parts):
    return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in KEYS}


def _splitmix_uniform(seed, id, stream, ctr):
    """The integer recipe of the stream, written out on its own (include/alipmpc.h)."""
    m = 2 ** 64
    key = (id * 4 + stream) * 2 ** 20 + ctr + 1          # ctr < 2^20: the OR of the recipe is a sum
    z = (seed + 0x9E3779B97F4A7C15 * key) % m
    z = ((z ^ (z // 2 ** 30)) * 0xBF58476D1CE4E5B9) % m
    z = ((z ^ (z // 2 ** 27)) * 0x94D049BB133111EB) % m
    z = z ^ (z // 2 ** 31)
    return (z // 2 ** 11) / 2.0 ** 53


@pytest.mark.parametrize("args", [(0, 0, 0, 0), (1, 1, 1, 1), (7, 123456, 2, 4100), (2 ** 64 - 1, 2 ** 40 - 1, 2, 2 ** 20 - 1),
                                  (0xDEADBEEF, 2 ** 40 - 1, 0, 3 * (2 ** 18 - 1) + 2), (42, 2 ** 33 + 5, 1, 23)])
def test_counter_uniform_is_the_splitmix_recipe(args):
    from alipmpc import scenes
    u = scenes.counter_uniform(*args)
    assert u == _splitmix_uniform(*args) and 0.0 <= u < 1.0
    seed, id, stream, ctr = args
    assert scenes.counter_uniforms(seed, id, stream, [ctr, ctr ^ 1])[0] == u
    assert scenes.counter_uniform(seed, id, stream, ctr ^ 1) == scenes.counter_uniforms(seed, id, stream, [ctr ^ 1])[0] != u


def _pairs_spaced(obs, spacing):
    """Every pair of raw obstacles [x, y, r] keeps r1 + r2 + 2 * spacing."""
    for i in range(len(obs)):
        for j in range(i):
            if np.hypot(*(obs[i, :2] - obs[j, :2])) < obs[i, 2] + obs[j, 2] + 2 * spacing - 1e-9:
                return False
    return True


def test_counter_batch_distribution():
    """The properties test_scene_generator_distribution asserts for make_batch."""
    from alipmpc import scenes
    B = 256
    bt = scenes.make_batch_counter(B, seed=1, n_cir=5)
    assert bt["cir"].shape == (B, 5, 3) and np.all(bt["nc"] == 5) and bt["elp"] is None and bt["ne"] is None
    assert bt["leg"].dtype == np.int8 and set(np.unique(bt["leg"])) == {-1, 1}
    assert np.array_equal(bt["goal"], np.tile([10.0, 10.0], (B, 1)))
    r = bt["cir"][:, :, 2] - scenes.SAFE_DIS
    assert r.min() >= 0.35 - 1e-12 and r.max() <= 1.0 + 1e-12
    assert bt["cir"][:, :, :2].min() >= 0 and bt["cir"][:, :, :2].max() <= 8.5
    for b in range(B):
        c = bt["cir"][b]
        d = np.hypot(*(bt["x0"][b, :2] - c[:, :2]).T)
        assert np.all(d >= c[:, 2] + 0.2 - 1e-12)
        assert np.hypot(*(bt["x0"][b, :2] - 10.0)) > 0.5 - 1e-12
        assert _pairs_spaced(c - [0, 0, scenes.SAFE_DIS], 0.8)
        # the seed circles take part in the rejection
        for sx, sy, sr in ((10.0, 10.0, 0.3), (0.0, 0.0, 1.0)):
            assert np.all(np.hypot(c[:, 0] - sx, c[:, 1] - sy) >= c[:, 2] - 0.4 + sr + 1.6 - 1e-9)
    th = bt["x0"][:, 4]
    vbx = np.cos(th) * bt["x0"][:, 2] + np.sin(th) * bt["x0"][:, 3]
    vby = -np.sin(th) * bt["x0"][:, 2] + np.cos(th) * bt["x0"][:, 3]
    assert vbx.min() >= 0.45 - 1e-12 and vbx.max() <= 0.75 + 1e-12
    assert np.all(-bt["leg"] * vby >= 0.17 - 1e-12) and np.all(-bt["leg"] * vby <= 0.33 + 1e-12)
    # heading towards the goal + N(0, 0.2)
    dev = np.angle(np.exp(1j * (th - np.arctan2(10 - bt["x0"][:, 1], 10 - bt["x0"][:, 0]))))
    assert abs(dev.mean()) < 0.05 and 0.15 < dev.std() < 0.25
    assert np.array_equal(bt["u0"], np.tile(bt["x0"], (1, 3)))
    # coordinates and radii are multiples of 0.01
    assert np.array_equal(np.round(bt["cir"][:, :, :2], 2), bt["cir"][:, :, :2])


def test_counter_batch_mix_shapes():
    from alipmpc import scenes
    mix = scenes.make_batch_counter(24, seed=2, n_cir=5, n_elp=5, N=5)
    assert mix["cir"].shape == (24, 5, 3) and mix["elp"].shape == (24, 5, 5) and mix["u0"].shape == (24, 25)
    assert np.all(mix["nc"] == 5) and np.all(mix["ne"] == 5)
    a, b, phi = mix["elp"][:, :, 2] - 0.4, mix["elp"][:, :, 3] - 0.4, mix["elp"][:, :, 4]
    assert a.min() >= 0.35 - 1e-12 and a.max() <= 1.0 + 1e-12
    assert np.all(b >= a / 2 - 0.005 - 1e-12) and np.all(b <= a + 0.005 + 1e-12)
    assert phi.min() >= 0 and phi.max() <= 3.14 + 1e-12
    for t in range(24):
        raw = np.concatenate([mix["cir"][t] - [0, 0, 0.4], mix["elp"][t][:, :3] - [0, 0, 0.4]])
        assert _pairs_spaced(raw, 0.2)       # 10 obstacles: at most 2 relaxations of the 0.8 spacing
        d = np.hypot(*(mix["x0"][t, :2] - mix["elp"][t][:, :2]).T)
        assert np.all(d >= np.maximum(mix["elp"][t][:, 2], mix["elp"][t][:, 3]) + 0.2 - 1e-12)
    odd = scenes.make_batch_counter(4, seed=2, n_cir=3, n_elp=2)
    assert odd["cir"].shape == (4, 3, 3) and odd["elp"].shape == (4, 2, 5)
    with pytest.raises(ValueError):
        scenes.make_batch_counter(4, n_cir=5, n_elp=3)


def test_counter_batch_is_shard_invariant():
    from alipmpc import scenes
    whole = scenes.make_batch_counter(300, seed=3, n_cir=5)
    parts = [scenes.make_batch_counter(100, seed=3, first=0, n_cir=5),
             scenes.make_batch_counter(200, seed=3, first=100, n_cir=5)]
    _same(whole, _cat(parts))
    assert not np.array_equal(whole["cir"], scenes.make_batch_counter(300, seed=4, n_cir=5)["cir"])
    mix = scenes.make_batch_counter(40, seed=3, n_cir=2, n_elp=2, fields=7)
    _same(mix, _cat([scenes.make_batch_counter(13, seed=3, n_cir=2, n_elp=2, fields=7),
                     scenes.make_batch_counter(27, seed=3, first=13, n_cir=2, n_elp=2, fields=7)]))


def test_counter_batch_shared_fields():
    from alipmpc import scenes
    bt = scenes.make_batch_counter(28, seed=5, n_cir=5, fields=7)
    for g in range(21):
        assert np.array_equal(bt["cir"][g], bt["cir"][g + 7]) and bt["nc"][g] == bt["nc"][g + 7]
        assert not np.array_equal(bt["x0"][g], bt["x0"][g + 7])
    assert len({bt["cir"][g].tobytes() for g in range(7)}) == 7
    # field f of a shared sweep is field f of a one-field-per-instance sweep
    own = scenes.make_batch_counter(7, seed=5, n_cir=5)
    assert np.array_equal(own["cir"], bt["cir"][:7])


def test_counter_batch_short_fields():
    from alipmpc import scenes
    bt = scenes.make_batch_counter(256, seed=6, n_cir=5, max_candidates=8)
    assert bt["nc"].min() >= 0 and bt["nc"].max() <= 5 and np.any(bt["nc"] < 5) and np.any(bt["nc"] == 5)
    for b in range(256):
        k = bt["nc"][b]
        assert np.all(bt["cir"][b, k:] == 0) and np.all(bt["cir"][b, :k, 2] >= 0.75 - 1e-12)
        assert _pairs_spaced(bt["cir"][b, :k] - [0, 0, 0.4], 0.8)
        d = np.hypot(*(bt["x0"][b, :2] - bt["cir"][b, :k, :2]).T)
        assert np.all(d >= bt["cir"][b, :k, 2] + 0.2 - 1e-12)
    # a short field is a prefix of the full one
    full = scenes.make_batch_counter(256, seed=6, n_cir=5)
    for b in range(256):
        k = bt["nc"][b]
        assert np.array_equal(bt["cir"][b, :k], full["cir"][b, :k])
    mix = scenes.make_batch_counter(64, seed=6, n_cir=3, n_elp=3, max_candidates=8)
    placed = mix["nc"] + mix["ne"]
    assert np.any(placed < 6) and np.array_equal(mix["nc"], (placed + 1) // 2) and np.array_equal(mix["ne"], placed // 2)
    for b in range(64):
        assert np.all(mix["elp"][b, mix["ne"][b]:] == 0) and np.all(mix["cir"][b, mix["nc"][b]:] == 0)
