"""Synthetic scenario batches — the distribution of the reference's random obstacle fields.

Obstacles follow rand_obs.random_circle / random_obs (rand_obs.py:31-72): centres ~ U[0, 8.5]^2 rounded
to 0.01, radii ~ U[0.35, 1.0] rounded to 0.01, rejected when any pair is closer than r1 + r2 + 2*0.8
(the seed circles (10,10,0.3) and (0,0,1.0) take part in the rejection and are dropped afterwards);
in 'mix' scenes every second obstacle becomes an ellipse [xc, yc, a=r, b~U[a/2,a], phi=deg(U{0..180})].
Obstacles are inflated by safe_dis = 0.4 as the driver does (main_sim_mpc.py:11,14).
Initial states: position ~ U[0,10]^2 outside every inflated obstacle by 0.2, heading towards the goal
(10, 10) + N(0, 0.2), body velocity vx ~ U[0.45, 0.75], vy = -leg * U[0.17, 0.33] rotated to world,
leg ~ U{-1, +1}, warm start u0 = [x0]*N (logger_mpc.py:327-328).
Unlike the reference's unbounded rejection loop, placement gives up after `max_tries` draws per obstacle
and relaxes the spacing rule (needed for 10-obstacle scenes, which rarely fit the reference's rule).
"""
import numpy as np

SAFE_DIS = 0.4
GOAL = (10.0, 10.0)


def random_circles(rng, num, margin=8.5, radius=1.0, safe_dis=0.8, max_tries=2000):
    placed = [(10.0, 10.0, 0.3), (0.0, 0.0, 1.0)]
    tries = 0
    spacing = safe_dis
    while len(placed) < num + 2:
        x = round(margin * rng.random(), 2)
        y = round(margin * rng.random(), 2)
        r = round((radius - 0.35) * rng.random() + 0.35, 2)
        ok = all((x - c[0]) ** 2 + (y - c[1]) ** 2 - (r + c[2] + 2 * spacing) ** 2 >= 0 for c in placed)
        if ok:
            placed.append((x, y, r))
            tries = 0
        else:
            tries += 1
            if tries > max_tries:
                spacing *= 0.5
                tries = 0
    return np.array(placed[2:], dtype=np.float64)


def to_mix(rng, cir):
    cl, el = [], []
    for i, c in enumerate(cir):
        if i % 2 == 0:
            cl.append(c)
        else:
            a = c[2]
            b = round((a / 2) * rng.random() + a / 2, 2)
            phi = round(int(rng.integers(0, 181)) * np.pi / 180, 2)
            el.append([c[0], c[1], a, b, phi])
    return np.array(cl, np.float64).reshape(-1, 3), np.array(el, np.float64).reshape(-1, 5)


def sample_state(rng, cir_safe, elp_safe, goal=GOAL, clearance=0.2):
    while True:
        pos = rng.uniform(0.0, 10.0, 2)
        ok = np.hypot(pos[0] - goal[0], pos[1] - goal[1]) > 0.5
        for c in cir_safe:
            ok &= np.hypot(*(pos - c[:2])) >= c[2] + clearance
        for e in elp_safe:
            ok &= np.hypot(*(pos - e[:2])) >= max(e[2], e[3]) + clearance
        if ok:
            break
    leg = int(rng.choice([-1, 1]))
    th = np.arctan2(goal[1] - pos[1], goal[0] - pos[0]) + rng.normal(0.0, 0.2)
    vbx = rng.uniform(0.45, 0.75)
    vby = -leg * rng.uniform(0.17, 0.33)
    c, s = np.cos(th), np.sin(th)
    return np.array([pos[0], pos[1], c * vbx - s * vby, s * vbx + c * vby, th]), leg


def make_batch(B, seed=0, n_cir=5, n_elp=0, N=3, nc_max=None, ne_max=None, scenes_per_batch=None,
               in_range=False):
    """Build a batch of B instances.  n_elp > 0 uses 'mix' scenes with n_cir + n_elp obstacles.
    scenes_per_batch: number of distinct obstacle fields (instances cycle over them; default B).
    in_range: place every obstacle within the 4 m detection range of x0 (fixed m for timing)."""
    rng = np.random.default_rng(seed)
    nc_max = n_cir if nc_max is None else nc_max
    ne_max = n_elp if ne_max is None else ne_max
    S = B if scenes_per_batch is None else scenes_per_batch
    x0 = np.zeros((B, 5))
    leg = np.zeros(B, np.int8)
    cir = np.zeros((B, nc_max, 3))
    elp = np.zeros((B, max(ne_max, 0), 5))
    nc = np.zeros(B, np.int32)
    ne = np.zeros(B, np.int32)
    scenes = []
    for _ in range(S):
        tot = n_cir + n_elp
        c = random_circles(rng, tot)
        if n_elp > 0:
            cc, ee = to_mix(rng, c)
        else:
            cc, ee = c, np.zeros((0, 5))
        cs = cc + np.array([0, 0, SAFE_DIS]) if len(cc) else cc
        es = ee + np.array([0, 0, SAFE_DIS, SAFE_DIS, 0]) if len(ee) else ee
        scenes.append((cs, es))
    for b in range(B):
        cs, es = scenes[b % S]
        st, lg = sample_state(rng, cs, es)
        if in_range:
            # shift the scene so its centroid sits ~2 m ahead of the robot
            cen = np.mean(np.concatenate([cs[:, :2], es[:, :2]]) if len(es) else cs[:, :2], axis=0)
            d = st[:2] + 2.0 * np.array([np.cos(st[4]), np.sin(st[4])]) - cen
            cs = cs.copy(); cs[:, :2] += d
            es = es.copy()
            if len(es):
                es[:, :2] += d
        x0[b] = st
        leg[b] = lg
        nc[b] = min(len(cs), nc_max)
        ne[b] = min(len(es), ne_max)
        cir[b, :nc[b]] = np.asarray(cs, float).reshape(-1, 3)[:nc[b]]
        if ne_max:
            elp[b, :ne[b]] = np.asarray(es, float).reshape(-1, 5)[:ne[b]]
    u0 = np.tile(x0, (1, N))
    goal = np.tile(np.array(GOAL), (B, 1))
    return dict(x0=x0, goal=goal, leg=leg, cir=cir, nc=nc, elp=elp if ne_max else None, ne=ne if ne_max else None,
                u0=u0)


def block_path(batch, seed, gap=(0.6, 1.4), lat=0.5):
    """A copy of `batch` (a make_batch dict) with one obstacle per instance moved into the way to the goal, so that its
    D-CBF rows are active at the solution (on the random fields they rarely are, and the plan's obstacle sensitivities
    are zero to rounding).  With d the unit vector from x0's position to the goal and n = (-d_y, d_x), the moved
    obstacle's centre goes to pos + (R + g_b) d + t_b R n, R = r or max(a, b) (inflated, as stored), g_b ~ U(gap) and
    t_b ~ U(-lat, lat) drawn from default_rng(1000 + seed), all g first.  Instance b moves ellipse slot
    (b // 2) % ne[b] if it has ellipses and b is odd, circle slot b % nc[b] otherwise: the rotating slot puts
    obstacles that select_obs drops in front of the moved one."""
    bt = {k: (None if v is None else np.array(v)) for k, v in batch.items()}
    B = bt["x0"].shape[0]
    rng = np.random.default_rng(1000 + seed)
    g = rng.uniform(gap[0], gap[1], B)
    t = rng.uniform(-lat, lat, B)
    pos = bt["x0"][:, 0:2]
    d = np.broadcast_to(bt["goal"], (B, 2)) - pos
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    nrm = np.stack([-d[:, 1], d[:, 0]], axis=1)
    for b in range(B):
        n_elp = int(bt["ne"][b]) if bt.get("ne") is not None else 0
        if n_elp > 0 and b % 2 == 1:
            o = bt["elp"][b, (b // 2) % n_elp]
            R = max(o[2], o[3])
        else:
            o = bt["cir"][b, b % int(bt["nc"][b])]
            R = o[2]
        o[0:2] = pos[b] + (R + g[b]) * d[b] + t[b] * R * nrm[b]
    return bt


def make_batch_vec(B, seed=0, n_cir=5, n_elp=0, N=3, fields=None, max_rounds=4000):
    """Same distribution as make_batch, vectorised over instances, with `fields` distinct obstacle fields
    (default: one PER INSTANCE — the Monte-Carlo sweep of BASELINE cfg5, 1M randomized scenes; instance b
    uses field b % fields).  Every round draws candidates for each unfinished field and accepts the first
    one that passes the same spacing rule (halved after 2000 consecutive rejections, as random_circles);
    initial states are rejection-sampled per instance the same way.  Not stream-identical to make_batch
    (different draw order), distribution-identical."""
    rng = np.random.default_rng(seed)
    tot = n_cir + n_elp
    K = tot + 2
    F = B if fields is None else max(1, min(int(fields), B))
    B_inst, B = B, F
    obs = np.zeros((B, K, 3))
    obs[:, 0] = (10.0, 10.0, 0.3)
    obs[:, 1] = (0.0, 0.0, 1.0)
    cnt = np.full(B, 2)
    spacing = np.full(B, 0.8)
    tries = np.zeros(B, np.int64)
    C = 32   # candidates per field and round; the first acceptable one is taken (= sequential rejection)
    for _ in range(max_rounds * max(tot, 1)):
        todo = np.nonzero(cnt < K)[0]
        if todo.size == 0:
            break
        x = np.round(8.5 * rng.random((todo.size, C)), 2)
        y = np.round(8.5 * rng.random((todo.size, C)), 2)
        r = np.round(0.65 * rng.random((todo.size, C)) + 0.35, 2)
        o = obs[todo]
        slot = np.arange(K)[None, None, :] < cnt[todo, None, None]
        d = (x[:, :, None] - o[:, None, :, 0]) ** 2 + (y[:, :, None] - o[:, None, :, 1]) ** 2 - \
            (r[:, :, None] + o[:, None, :, 2] + 2 * spacing[todo, None, None]) ** 2
        okc = np.all((d >= 0) | ~slot, axis=2)                  # (todo, C)
        first = np.argmax(okc, axis=1)
        anyok = okc[np.arange(todo.size), first]
        # the 2000-rejection relaxation applies within the candidate sequence too
        nrej = np.where(anyok, first, C)
        over = tries[todo] + nrej > 2000
        ok = anyok & ~over
        acc = todo[ok]
        obs[acc, cnt[acc]] = np.stack([x[ok, first[ok]], y[ok, first[ok]], r[ok, first[ok]]], axis=1)
        cnt[acc] += 1
        tries[acc] = 0
        rej = todo[~ok]
        tries[rej] += np.minimum(nrej[~ok], 2001 - tries[rej])
        relax = rej[tries[rej] > 2000]
        spacing[relax] *= 0.5
        tries[relax] = 0
    assert np.all(cnt == K), "obstacle placement did not finish"
    obs = obs[:, 2:]
    if n_elp > 0:   # to_mix: every second obstacle becomes an ellipse
        ci = np.arange(0, tot, 2)
        ei = np.arange(1, tot, 2)
        cir = obs[:, ci]
        a = obs[:, ei, 2]
        b = np.round((a / 2) * rng.random(a.shape) + a / 2, 2)
        phi = np.round(rng.integers(0, 181, a.shape) * np.pi / 180, 2)
        elp = np.concatenate([obs[:, ei, :2], a[..., None], b[..., None], phi[..., None]], axis=2)
        elp = elp + np.array([0, 0, SAFE_DIS, SAFE_DIS, 0])
    else:
        cir, elp = obs, np.zeros((B, 0, 5))
    cir = cir + np.array([0, 0, SAFE_DIS])
    if B_inst != F:   # instance b -> field b % F
        idx = np.arange(B_inst) % F
        cir, elp, B = cir[idx], elp[idx], B_inst
    # initial states outside every inflated obstacle (+0.2) and > 0.5 from the goal
    pos = np.zeros((B, 2))
    todo = np.arange(B)
    while todo.size:
        p = rng.uniform(0.0, 10.0, (todo.size, 2))
        ok = np.hypot(p[:, 0] - GOAL[0], p[:, 1] - GOAL[1]) > 0.5
        ok &= np.all(np.hypot(p[:, None, 0] - cir[todo, :, 0], p[:, None, 1] - cir[todo, :, 1]) >=
                     cir[todo, :, 2] + 0.2, axis=1)
        if elp.shape[1]:
            ok &= np.all(np.hypot(p[:, None, 0] - elp[todo, :, 0], p[:, None, 1] - elp[todo, :, 1]) >=
                         np.maximum(elp[todo, :, 2], elp[todo, :, 3]) + 0.2, axis=1)
        pos[todo[ok]] = p[ok]
        todo = todo[~ok]
    leg = rng.choice(np.array([-1, 1], np.int8), B)
    th = np.arctan2(GOAL[1] - pos[:, 1], GOAL[0] - pos[:, 0]) + rng.normal(0.0, 0.2, B)
    vbx = rng.uniform(0.45, 0.75, B)
    vby = -leg * rng.uniform(0.17, 0.33, B)
    c, s = np.cos(th), np.sin(th)
    x0 = np.stack([pos[:, 0], pos[:, 1], c * vbx - s * vby, s * vbx + c * vby, th], axis=1)
    return dict(x0=x0, goal=np.tile(np.array(GOAL), (B, 1)), leg=leg,
                cir=np.ascontiguousarray(cir), nc=np.full(B, cir.shape[1], np.int32),
                elp=np.ascontiguousarray(elp) if n_elp else None,
                ne=np.full(B, elp.shape[1], np.int32) if n_elp else None,
                u0=np.tile(x0, (1, N)))


# ---------------------------------------------------------------------------------------------------------------
# Counter-based stream (include/alipmpc.h: alipmpc_scenes_batch; csrc/scenes.inc is the device form).
# Every row is a pure function of (seed, global index, fields, n_cir, n_elp, max_candidates), so any index range
# can be generated on its own.  This is the host restatement: the yardstick of the device kernel and a CPU
# fallback for tools, not a fast path.  Same distribution as make_batch, a different stream.
# ---------------------------------------------------------------------------------------------------------------
MAX_CANDIDATES = 1 << 18      # default and limit of max_candidates
MAX_TRIES = 2000              # consecutive rejections before the spacing is halved
STATE_PAIRS = 1024            # initial-state pairs tried before the last one is taken
STREAM_FIELD, STREAM_SHAPE, STREAM_STATE = 0, 1, 2
CTR_LEG = 4096                # stream 2: leg, heading noise (2 draws), vbx, vby follow the position pairs
_M64 = (1 << 64) - 1


def counter_uniform(seed, id, stream, ctr):
    """U(seed, id, stream, ctr) in [0, 1): splitmix64 of the counter (id < 2^40, stream < 4, ctr < 2^20)."""
    key = ((((int(id) * 4 + int(stream)) << 20) | int(ctr)) + 1) & _M64
    z = (int(seed) + 0x9E3779B97F4A7C15 * key) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def counter_uniforms(seed, id, stream, ctr):
    """counter_uniform for an array of counters (uint64 arithmetic wraps as the scalar form masks)."""
    ctr = np.asarray(ctr, np.uint64)
    base = np.uint64((int(id) * 4 + int(stream)) << 20)
    with np.errstate(over="ignore"):
        key = (base | ctr) + np.uint64(1)
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * key
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _r2(v):
    return np.rint(v * 100) / 100          # np.round(v, 2)


def counter_field(seed, fid, tot, max_candidates=MAX_CANDIDATES):
    """Placement of field `fid`: the sequential rejection loop of random_circles on stream 0.  Returns the placed
    obstacles [x, y, r] (fewer than tot when max_candidates ran out), seed circles dropped."""
    placed = [(10.0, 10.0, 0.3), (0.0, 0.0, 1.0)]
    spacing, tries, c, block = 0.8, 0, 0, 32
    while len(placed) < tot + 2 and c < max_candidates:
        n = min(block, max_candidates - c)
        u = counter_uniforms(seed, fid, STREAM_FIELD, np.arange(3 * c, 3 * (c + n)))
        xs, ys = _r2(8.5 * u[0::3]).tolist(), _r2(8.5 * u[1::3]).tolist()
        rs = _r2(0.65 * u[2::3] + 0.35).tolist()
        for x, y, r in zip(xs, ys, rs):
            c += 1
            ok = True
            for cx, cy, cr in placed:
                t = (r + cr) + 2 * spacing
                if not ((x - cx) * (x - cx) + (y - cy) * (y - cy) - t * t >= 0):
                    ok = False
                    break
            if ok:
                placed.append((x, y, r))
                tries = 0
                if len(placed) == tot + 2:
                    break
            else:
                tries += 1
                if tries > MAX_TRIES:
                    spacing *= 0.5
                    tries = 0
        block = min(4 * block, 4096)
    return np.array(placed[2:], np.float64).reshape(-1, 3)


def counter_scene(seed, fid, n_cir, n_elp, max_candidates=MAX_CANDIDATES):
    """Inflated obstacles of field `fid`: (cir (nc, 3), elp (ne, 5))."""
    obs = counter_field(seed, fid, n_cir + n_elp, max_candidates)
    if n_elp > 0:
        cir = obs[0::2].copy()
        odd = obs[1::2]
        j = np.arange(len(odd))
        a = odd[:, 2]
        b = _r2((a / 2) * counter_uniforms(seed, fid, STREAM_SHAPE, 2 * j) + a / 2)
        phi = _r2(np.floor(181 * counter_uniforms(seed, fid, STREAM_SHAPE, 2 * j + 1)) * (np.pi / 180))
        elp = np.stack([odd[:, 0], odd[:, 1], a + SAFE_DIS, b + SAFE_DIS, phi], axis=1)
    else:
        cir, elp = obs.copy(), np.zeros((0, 5))
    cir[:, 2] = cir[:, 2] + SAFE_DIS
    return cir, elp


def counter_state(seed, g, cir, elp):
    """Initial state and leg of instance g (stream 2) among the inflated obstacles cir / elp."""
    ox = np.concatenate([cir[:, 0], elp[:, 0]])
    oy = np.concatenate([cir[:, 1], elp[:, 1]])
    R = np.concatenate([cir[:, 2], np.maximum(elp[:, 2], elp[:, 3])]) + 0.2
    RR = R * R
    px = py = 0.0
    for i0 in range(0, STATE_PAIRS, 64):
        u = counter_uniforms(seed, g, STREAM_STATE, np.arange(2 * i0, 2 * (i0 + 64)))
        qx, qy = 10 * u[0::2], 10 * u[1::2]
        ok = (qx - 10) * (qx - 10) + (qy - 10) * (qy - 10) > 0.25
        dx, dy = qx[:, None] - ox[None, :], qy[:, None] - oy[None, :]
        ok &= np.all(dx * dx + dy * dy >= RR[None, :], axis=1)
        k = int(np.argmax(ok)) if ok.any() else 63
        px, py = float(qx[k]), float(qy[k])
        if ok.any():
            break
    leg = -1 if counter_uniform(seed, g, STREAM_STATE, CTR_LEG) < 0.5 else 1
    noise = 0.2 * np.sqrt(-2 * np.log(1 - counter_uniform(seed, g, STREAM_STATE, CTR_LEG + 1))) * \
        np.cos(2 * np.pi * counter_uniform(seed, g, STREAM_STATE, CTR_LEG + 2))
    vbx = 0.45 + 0.3 * counter_uniform(seed, g, STREAM_STATE, CTR_LEG + 3)
    vby = -leg * (0.17 + 0.16 * counter_uniform(seed, g, STREAM_STATE, CTR_LEG + 4))
    th = np.arctan2(10 - py, 10 - px) + noise
    c, s = np.cos(th), np.sin(th)
    return np.array([px, py, c * vbx - s * vby, s * vbx + c * vby, th]), leg


def make_batch_counter(B, seed=0, first=0, n_cir=5, n_elp=0, N=3, nc_max=None, ne_max=None, fields=0,
                       max_candidates=0):
    """Instances first .. first + B - 1 of the counter-based stream: the dict of make_batch.  fields > 0: instance g
    uses obstacle field g % fields (0: its own).  max_candidates: candidates per field (0: 2^18); a field that runs
    out holds fewer obstacles (nc / ne say how many, the other slots are zero)."""
    nc_max = n_cir if nc_max is None else nc_max
    ne_max = n_elp if ne_max is None else ne_max
    maxc = max_candidates or MAX_CANDIDATES
    tot = n_cir + n_elp
    if B < 0 or first < 0 or first + B > 1 << 40 or fields < 0 or not 0 < maxc <= MAX_CANDIDATES:
        raise ValueError("make_batch_counter: index range, fields or max_candidates out of range")
    if not (0 <= n_cir <= nc_max and 0 <= n_elp <= ne_max) or (n_elp > 0 and (n_cir, n_elp) != ((tot + 1) // 2, tot // 2)):
        raise ValueError("make_batch_counter: n_cir / n_elp do not fit the slots or the mix rule")
    x0 = np.zeros((B, 5))
    leg = np.zeros(B, np.int8)
    cir = np.zeros((B, nc_max, 3))
    elp = np.zeros((B, ne_max, 5))
    nc = np.zeros(B, np.int32)
    ne = np.zeros(B, np.int32)
    cache = {}
    for b in range(B):
        g = first + b
        fid = g % fields if fields else g
        if fid not in cache:
            cache[fid] = counter_scene(seed, fid, n_cir, n_elp, maxc)
        cs, es = cache[fid]
        if not fields:
            del cache[fid]
        nc[b], ne[b] = len(cs), len(es)
        cir[b, :len(cs)] = cs
        elp[b, :len(es)] = es
        x0[b], leg[b] = counter_state(seed, g, cs, es)
    return dict(x0=x0, goal=np.tile(np.array(GOAL), (B, 1)), leg=leg, cir=cir, nc=nc,
                elp=elp if ne_max else None, ne=ne if ne_max else None, u0=np.tile(x0, (1, N)))
