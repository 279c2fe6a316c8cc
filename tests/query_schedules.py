"""Ray orders that stress the refill of the persistent query kernels (find_nearest_kernel, is_occluded_kernel, their KD-tree / grid and two-level forms,
sample_query_kernel), shared by tests/test_gpu_query_lane_reuse.py (device against oracle, the launch bounded to k workgroups with CRT_DEBUG_QUERY_GRID) and
tests/test_query_schedules_cpu.py (the oracle alone: is each order what it claims to be?).

A lane that finishes takes the next ray of the launch-wide cursor and reuses its registers, its LDS stack column and its counters, so what a ray inherits depends
on the ORDER of the rays.  An order here is an array of distinct indices into a pool of rays whose per-ray answers the oracle has given once; the expected result
of a launch over pool[order] is answers[order], whatever the order.  `cost` is the oracle's work per ray: traversed + tested for the queries, random numbers drawn
for Sample.  Everything here is numpy; nothing is recorded data."""
import numpy as np

WAVE = 64                                                                 # lanes of a wavefront = rays of one full draw from the cursor
REFILL = 16                                                               # kQueryRefill: idle lanes that trigger the next draw of the 64-thread kernels
TAILS = (0, 1, 15, 16, 17, 63)                                            # n0 + r: a last draw that ends at n, one lane short of it, either side of REFILL


def base_size(k, sample=False):
    """rays of a launch bounded to k workgroups: 24 per lane of the 64-thread kernels, 8 per lane of sample_query_kernel's 256"""
    return 256 * k * 8 if sample else 64 * k * 24


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rays made on purpose
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def idler_rays(lo, hi, n, seed, up=False, margin=0.25):
    """rays that end in their first trip: origins beyond the +x face of the box (lo, hi), directions with a positive x component, so they leave the box behind
    and miss the root's children / the grid's box.  up: every direction rises (nothing but the sky for Sample; no floor for the occlusion rule)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    O = np.stack([hi[0] + margin + rng.uniform(0.0, 1.0, n), rng.uniform(-0.8, hi[1] + 1.0, n), rng.uniform(lo[2] - 1.0, hi[2] + 1.0, n)], 1)
    D = np.stack([rng.uniform(0.2, 1.0, n), rng.uniform(0.1, 1.0, n) if up else rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)], 1)
    return O.astype(np.float32), unit(D)


def through_box_rays(lo, hi, n, seed):
    """rays from a sphere around the box (lo, hi) through two points of it, the second near the opposite corner region: long walks, the walkers' candidates"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    O = c + d * r
    O[:, 1] = np.maximum(O[:, 1], -0.9)                                   # above the floor
    T = lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo)
    return O.astype(np.float32), unit(T - O)


def zero_components(D, every, seed):
    """a copy of D in which every `every`-th direction has one component (two for every fourth of those) set to exactly 0 and is normalised again: axis-parallel
    rays, infinite reciprocals, NaN slab and plane distances.  Returns (D, flags)."""
    rng = np.random.default_rng(seed)
    D = np.array(D, np.float32)
    flags = np.zeros(len(D), bool)
    for j, i in enumerate(range(0, len(D), every)):
        a = int(rng.integers(0, 3))
        D[i, a] = 0
        if j % 4 == 3:
            D[i, (a + 1) % 3] = 0
        if not D[i].any():
            D[i, (a + 2) % 3] = 1
        flags[i] = True
    D[flags] = unit(D[flags])
    return D, flags


def refused_sample_rays(O, D, seeds):
    """copies of Sample rays made unfit, mixed: seed 0, a NaN direction component, an infinite origin component, D = (0, -0, 0)"""
    O, D, seeds = np.array(O, np.float32), np.array(D, np.float32), np.array(seeds, np.uint32)
    for i in range(len(O)):
        k = i % 4
        if k == 0:
            seeds[i] = 0
        elif k == 1:
            D[i, i % 3] = np.nan
        elif k == 2:
            O[i, i % 3] = np.inf if i % 8 == 2 else -np.inf
        else:
            D[i] = (0.0, -0.0, 0.0)
    return O, D, seeds


def refused(O, D, seeds):
    """crt_sample's refusal rule (crt_abi.h): seed 0, a component of O or D that is not finite, or D = (0, 0, 0)"""
    O, D = np.asarray(O, np.float32), np.asarray(D, np.float32)
    return (np.asarray(seeds) == 0) | ~np.isfinite(O).all(axis=1) | ~np.isfinite(D).all(axis=1) | (D == 0).all(axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# orders: arrays of distinct pool indices
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def shuffled(idx, seed=1):
    """a fixed-seed permutation of idx"""
    idx = np.asarray(idx)
    return idx[np.random.default_rng(seed).permutation(len(idx))]


def ascending(idx, cost):
    """idx by rising cost (cost is indexed by pool index): the lanes of a wavefront finish together, every refill is a full one"""
    idx = np.asarray(idx)
    return idx[np.argsort(np.asarray(cost)[idx], kind="stable")]


def descending(idx, cost):
    return ascending(idx, cost)[::-1].copy()


def walker_among_idlers(idx, cost, idlers, n, group=WAVE):
    """n rays in groups of `group`: position (7 g) mod group of group g holds one of the n / group most expensive rays of idx, the other positions hold idlers, so
    one lane walks for many trips while its neighbours are refilled around it trip after trip.  A permutation of the walkers and idlers it selects."""
    assert n % group == 0
    g = n // group
    idx, idlers = np.asarray(idx), np.asarray(idlers)
    walkers = descending(idx, cost)[:g]
    assert len(idlers) >= g * (group - 1) and len(walkers) == g
    order = np.empty((g, group), idx.dtype)
    fill = idlers[: g * (group - 1)].reshape(g, group - 1)
    for j in range(g):
        p = (7 * j) % group
        order[j, :p] = fill[j, :p]; order[j, p] = walkers[j]; order[j, p + 1:] = fill[j, p:]
    return order.reshape(-1)


def walker_positions(n, group=WAVE):
    return np.array([j * group + (7 * j) % group for j in range(n // group)])


def leading_done_at_refill(leading, idx, n, seed=2):
    """the leading rays (each finished inside the refill itself: quad-occluded shadow rays, refused Sample rays) first, so whole draws leave every lane idle and the
    wavefront has to draw again; ordinary rays of idx follow, shuffled, up to n rays"""
    leading = np.asarray(leading)
    assert len(leading) < n
    return np.concatenate([leading, shuffled(idx, seed)[: n - len(leading)]])


def degenerate_mixed(idx, flags, seed=3):
    """a permutation of idx in which the flagged rays (flags is indexed by pool index: axis-parallel directions, light-only and floor-only rays, inside = 1) sit at
    evenly spaced positions among the others instead of in a block"""
    idx = shuffled(idx, seed)
    f = np.asarray(flags)[idx]
    special, plain = idx[f], idx[~f]
    n, m = len(idx), len(special)
    out = np.empty(n, idx.dtype)
    slots = np.zeros(n, bool)
    if m:
        slots[(np.arange(m) * n) // m] = True
    out[slots] = special; out[~slots] = plain
    return out


def largest_gap(order, flags):
    """the longest run of positions of `order` without a flagged ray"""
    pos = np.flatnonzero(np.asarray(flags)[np.asarray(order)])
    return int(np.diff(np.concatenate([[-1], pos, [len(order)]])).max() - 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# pools: the rays of one (kernel, scene), made once.  ordinary / idlers / leading are index arrays into O, D, last (inside or t) and seeds
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Pool:
    def __init__(self, parts, kmax, sample=False):
        """parts: [(class name, O, D, last)]; the ordinary rays are shuffled once, so that every prefix of them holds every kind of ray"""
        self.kmax, self.sample = kmax, sample
        self.O = np.concatenate([p[1] for p in parts]).astype(np.float32); self.D = np.concatenate([p[2] for p in parts]).astype(np.float32)
        self.last = np.concatenate([p[3] for p in parts])
        at = np.cumsum([0] + [len(p[1]) for p in parts])
        for j, p in enumerate(parts):
            setattr(self, p[0], np.arange(at[j], at[j + 1]))
        self.seeds = None
        self.flags = np.zeros(len(self.O), bool)

    def n0(self, k):
        return base_size(k, self.sample)

    def orders(self, k, cost):
        """name -> order for a launch bounded to k workgroups; `cost` per pool index.  "shuffled" has the longest tail: its prefixes n0 + r are the tail sizes."""
        n0 = self.n0(k)
        idx = self.ordinary[:n0]
        out = {"shuffled": shuffled(self.ordinary[: n0 + max(TAILS)]), "ascending": ascending(idx, cost), "descending": descending(idx, cost),
               "walker_among_idlers": walker_among_idlers(self.ordinary, cost, self.idlers, n0), "degenerate_mixed": degenerate_mixed(idx, self.flags)}
        if hasattr(self, "leading"):
            width = 256 if self.sample else WAVE
            out["leading_done_at_refill"] = leading_done_at_refill(self.leading[: 2 * width * k], self.ordinary, n0)
        return out


def scene_box(o, kind):
    """the box every mesh ray must enter: the BVH root's (FileScene) / the TLAS root's"""
    if kind == 0:
        n = o.bvh(0)["nodes"][0]
        return np.array(n["aabbMin"], np.float32), np.array(n["aabbMax"], np.float32)
    n = o.tlas()[0][0]
    return np.array(n["aabbMin"], np.float32), np.array(n["aabbMax"], np.float32)


def find_nearest_pool(lo, hi, light, kmax=3, ordinary=None, cost_fn=None):
    """FindNearest rays of a scene whose meshes lie in (lo, hi): the parity test's set, rays through the box, rays from beside it up at the light and down at the
    floor, a share of axis-parallel directions, inside = 1 on every fifth; idlers for n0 / 64 groups of 63.  ordinary: (O, D) to use instead.
    cost_fn(O, D) -> the oracle's cost per ray: one ray per group is then the most expensive of 800 000 rays through the box (a scene as small as the cube has
    few rays that walk 20 steps: about one in 7 000 of those)."""
    from test_gpu_parity import _rays
    from test_gpu_scene_queries import up_rays
    m = base_size(kmax) + max(TAILS)
    if ordinary is None:
        a, b = m // 2, m // 4
        c = (m - a - b) // 2; d = m - a - b - c
        O1, D1 = _rays(a, 7)
        O2, D2 = through_box_rays(lo, hi, b, 8)
        beside = (float(hi[0]) + 0.3, float(hi[0]) + 1.5)
        O3, D3 = up_rays(c, 9, light, beside, (float(lo[2]), float(hi[2])), -0.9, light[1] - 0.3, spread=0.45)
        rng = np.random.default_rng(10)
        O4 = np.stack([rng.uniform(*beside, d), rng.uniform(-0.5, 1.0, d), rng.uniform(lo[2], hi[2], d)], 1).astype(np.float32)
        D4 = unit(np.stack([rng.uniform(0.0, 0.5, d), rng.uniform(-1.0, -0.3, d), rng.uniform(-0.5, 0.5, d)], 1))
        O, D = np.concatenate([O1, O2, O3, O4]), np.concatenate([D1, D2, D3, D4])
        D, axis = zero_components(D, 12, 12)
        if cost_fn is not None:                                              # in place of the first rays through the box, as they are
            g = base_size(kmax) // WAVE
            Oc, Dc = through_box_rays(lo, hi, 800000, 15)
            top = np.argsort(-cost_fn(Oc, Dc), kind="stable")[:g]
            O[a:a + g], D[a:a + g], axis[a:a + g] = Oc[top], Dc[top], False
        p = np.random.default_rng(11).permutation(m)
        O, D, axis = O[p], D[p], axis[p]
    else:
        O, D = ordinary
        assert len(O) >= m
        O, D = O[:m], D[:m]
        axis = (D == 0).any(axis=1)
    g = base_size(kmax) // WAVE
    Oi, Di = idler_rays(lo, hi, g * (WAVE - 1), 13)
    inside = (np.arange(m) % 5 == 3).astype(np.int32)
    pool = Pool([("ordinary", O, D, inside), ("idlers", Oi, Di, np.zeros(len(Oi), np.int32))], kmax)
    pool.flags[: m] = axis | (inside != 0)
    return pool


def flag_light_and_floor_only(pool, hits, least):
    """adds to the pool's degenerate flags the ordinary rays that hit the light, and those that hit the floor and walk no further than an idler does"""
    h = hits[pool.ordinary]
    pool.flags[pool.ordinary] |= (h["objIdx"] == 0) | ((h["objIdx"] == 1) & (h["tested"] == 0) & (h["traversed"] == least))


def occlusion_pool(lo, hi, light, kmax=3, ordinary=None):
    """shadow rays that rise from above the floor (so the oracle's FindNearest tells whether a mesh lies on the ray: nothing lies above the light): around the
    meshes, from under / inside them into the quad, vertical ones; t by pick_t (1e34, the quad distance and its two neighbours).  leading: rays into the quad
    with t = 1e34, all quad-occluded.  ordinary: (O, D) to use instead."""
    from test_gpu_scene_queries import up_rays, quad_occluded, pick_t
    assert hi[1] < light[1] - 0.01, "the meshes must lie below the light plane"
    m = base_size(kmax) + max(TAILS)
    xr, zr = (float(lo[0]), float(hi[0])), (float(lo[2]), float(hi[2]))
    if ordinary is None:
        a = m // 2; b = m // 4; c = m - a - b
        O1, D1 = up_rays(a, 5, light, (xr[0] - 0.7, xr[1] + 0.7), (zr[0] - 0.7, zr[1] + 0.7), -0.9, light[1] - 0.3)
        O2, D2 = up_rays(b, 6, light, xr, zr, -0.95, max(float(lo[1] + hi[1]) / 2, -0.5), spread=0.45)
        rng = np.random.default_rng(7)
        O3 = np.stack([rng.uniform(*xr, c), rng.uniform(-0.95, float(hi[1]), c), rng.uniform(*zr, c)], 1).astype(np.float32)
        D3 = np.tile(np.array([[0.0, 1.0, 0.0]], np.float32), (c, 1))      # straight up: two zero components
        D3[::3, 0] = 0.3; D3[::3] = unit(D3[::3])                          # ... and one
        O, D = np.concatenate([O1, O2, O3]), np.concatenate([D1, D2, D3])
        p = np.random.default_rng(11).permutation(m)
        O, D = O[p], D[p]
    else:
        O, D = ordinary
        assert len(O) >= m
        O, D = O[:m], D[:m]
    _, tq = quad_occluded(O, D, np.full(m, 1e34, np.float32), light)
    t = pick_t(tq)
    g = base_size(kmax) // WAVE
    Oi, Di = idler_rays(lo, hi, g * (WAVE - 1), 13, up=True)
    nl = 2 * WAVE * kmax
    Ol, Dl = up_rays(nl, 14, light, (xr[0] - 0.7, xr[1] + 0.7), (zr[0] - 0.7, zr[1] + 0.7), -0.9, light[1] - 0.3, spread=0.45)
    big = lambda n: np.full(n, 1e34, np.float32)                           # noqa: E731
    pool = Pool([("ordinary", O, D, t), ("idlers", Oi, Di, big(len(Oi))), ("leading", Ol, Dl, big(nl))], kmax)
    pool.flags[: m] = (D == 0).any(axis=1)
    return pool


def sample_pool(o, prim, lo=None, hi=None, kmax=3, extra=None):
    """Sample rays of one world (`o`: its oracle, renderer_init done): sample_query_inputs' ray set at the size the launches need, a share of its directions
    axis-parallel; idlers that end in their first trip (triangle scenes: up and away from everything, the sky; the primitive scene's closed room: at the light);
    leading: refused rays.  extra: (O, D, inside, seeds) put in place of ordinary rays at evenly spaced positions, as they are.  pool.seeds holds the seeds; pool.want = (rgb, seeds out) per pool ray by the oracle, the refused rays' by the rule itself."""
    import sample_query_inputs as si
    m = base_size(kmax, True) + max(TAILS)
    g = base_size(kmax, True) // WAVE
    ni, nl = g * (WAVE - 1), 2 * 256 * kmax
    if prim:
        O, D, inside, seeds = si.prim_rays(n=m, seed=7)
        # the light ends a path at once: aim at points where first rays met it
        Oc, Dc, ic, sc = si.prim_rays(n=4096, seed=21)
        _, out, _ = si.oracle_sample(o, Oc, Dc, ic, sc)
        lit = np.flatnonzero((si.draws(sc, out) == 0) & (ic == 0))
        hit = o.find_nearest(Oc[lit], Dc[lit])
        I = Oc[lit] + hit["t"][:, None] * Dc[lit]
        Oi = si.prim_rays(n=2 * ni, seed=22)[0]
        Di = unit(I[np.arange(2 * ni) % len(I)] - Oi)
        _, out, _ = si.oracle_sample(o, Oi, Di, np.zeros(2 * ni, np.int32), si.seeds_for(2 * ni))
        keep = np.flatnonzero(si.draws(si.seeds_for(2 * ni), out) == 0)[:ni]
        assert len(keep) == ni, len(keep)
        Oi, Di = Oi[keep], Di[keep]
    else:
        O, D, inside, seeds = si.triangle_rays(o, n=m, seed=5)
        Oi, Di = idler_rays(lo, hi, ni, 13, up=True)
    D, axis = zero_components(D, 16, 12)
    si_seeds = si.seeds_for(m + ni + nl)
    if extra is not None:
        at = (np.arange(len(extra[0])) * m) // len(extra[0])
        O[at], D[at], inside[at], si_seeds[at], axis[at] = extra[0], extra[1], extra[2], extra[3], False
    Ol, Dl, sl = refused_sample_rays(O[:nl], D[:nl], si_seeds[m + ni:])
    pool = Pool([("ordinary", O, D, inside), ("idlers", Oi, Di, np.zeros(ni, np.int32)), ("leading", Ol, Dl, inside[:nl])], kmax, sample=True)
    pool.seeds = np.concatenate([si_seeds[:m + ni], sl]).astype(np.uint32)
    ok = np.concatenate([pool.ordinary, pool.idlers])
    rgb = np.full((len(pool.O), 3), np.nan, np.float32); out = pool.seeds.copy()
    rgb[ok], out[ok], cnt = si.oracle_sample(o, pool.O[ok], pool.D[ok], pool.last[ok], pool.seeds[ok])
    pool.want = (rgb, out)
    # the counters' growth per ray (a second pass: oracle_sample gives the total only), so that any order's sum is at hand
    pool.counted = {"rays": np.zeros(len(pool.O), np.int64), "mesh_hits": np.zeros(len(pool.O), np.int64)}
    c0 = o.counters()
    for i in ok:
        o.sample(pool.O[i], pool.D[i], int(pool.seeds[i]), int(pool.last[i]))
        c1 = o.counters()
        for k in pool.counted:
            pool.counted[k][i] = c1[k] - c0[k]
        c0 = c1
    assert all(int(pool.counted[k].sum()) == cnt[k] for k in pool.counted) and cnt["primary"] == 0
    pool.cost = np.zeros(len(pool.O), np.int64); pool.cost[ok] = si.draws(pool.seeds[ok], out[ok])
    assert (pool.cost >= 0).all()
    pool.flags[pool.ordinary] = axis | (inside != 0) | (pool.cost[pool.ordinary] == 0)
    return pool


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# cases: a pool with the oracle's answer per pool ray (`want`), its cost, and `walk`, hit records of the walk the cost was taken from
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def hit_cost(h):
    return h["traversed"].astype(np.int64) + h["tested"]


def _case(pool, want, walk, **more):
    c = Case()
    c.pool, c.want, c.walk, c.cost = pool, want, walk, hit_cost(walk)
    c.least = int(walk["traversed"].min())                                # the smallest Ray::traversed this scene's walk reports
    for k, v in more.items():
        setattr(c, k, v)
    return c


def find_nearest_case(orc, xml, kind, assets):
    """find_nearest_kernel: the oracle's FindNearest, all seven fields"""
    from test_gpu_scene_queries import light_of
    o, _ = orc.load_scene(xml, kind, assets)
    lo, hi = scene_box(o, kind)
    pool = find_nearest_pool(lo, hi, light_of(xml), cost_fn=lambda O, D: hit_cost(o.find_nearest(O, D)))
    want = o.find_nearest(pool.O, pool.D, pool.last)
    c = _case(pool, want, want, o=o)
    flag_light_and_floor_only(pool, want, c.least)
    return c


def occlusion_case(orc, xml, kind, assets, light):
    """is_occluded_kernel: Quad::IsOccluded restated | a mesh on the ray by the oracle's FindNearest (rising rays from above the floor: see occlusion_pool)"""
    from test_gpu_scene_queries import quad_occluded
    o, _ = orc.load_scene(xml, kind, assets)
    lo, hi = scene_box(o, kind)
    pool = occlusion_pool(lo, hi, light)
    assert (pool.D[:, 1] > 0).all() and (pool.O[:, 1] > -1).all()
    w = o.find_nearest(pool.O, pool.D)
    assert not (w["objIdx"] == 1).any()                                   # a rising ray above the floor never reaches it
    q, _ = quad_occluded(pool.O, pool.D, pool.last, light)
    return _case(pool, q | (w["objIdx"] >= 2), w, o=o, quad=q)


def alt_cases(orc, xml, kind, assets, light):
    """find_nearest_alt_kernel / is_occluded_alt_kernel over FileScene's KD-tree ("kd") or grid: the oracle's restatement of the accelerator alone over the whole
    ray (`want` of the first case; the BVH answer of the oracle's FindNearest in `bvh`), and Quad::IsOccluded restated | that restatement finds a triangle"""
    from test_gpu_scene_queries import quad_occluded
    o, _ = orc.load_scene(xml, 0, assets)
    lo, hi = scene_box(o, 0)
    a = orc.alt_accel(kind, o.bvh(0)["tris"])
    pool = find_nearest_pool(lo, hi, light)
    w = a.intersect(pool.O, pool.D)
    fn = _case(pool, w, w, o=o, bvh=o.find_nearest(pool.O, pool.D, pool.last))
    flag_light_and_floor_only(pool, fn.bvh, int(fn.bvh["traversed"].min()))
    pool = occlusion_pool(lo, hi, light)
    w = a.intersect(pool.O, pool.D)
    q, _ = quad_occluded(pool.O, pool.D, pool.last, light)
    oc = _case(pool, q | (w["objIdx"] > -1), w, o=o, quad=q)
    a.close()
    return fn, oc


def tlas_alt_cases(orc, xml, kind, assets, light):
    """tlas_alt_query_kernel: tests/tlas_alt_restate.py per ray (Python: one workgroup's worth of rays, kmax = 1), every field / the occlusion flag.  The
    occlusion pool's cost is the oracle's TLAS-BVH walk of the same rays."""
    import tlas_alt_restate as R
    from test_gpu_scene_queries import quad_occluded
    o, _ = orc.load_scene(xml, 1, assets)
    lo, hi = scene_box(o, 1)
    sc = R.Scene(orc, o, kind, light)
    pool = find_nearest_pool(lo, hi, light, kmax=1, ordinary=R.query_rays(o, light, 1600))
    want = sc.find_nearest_many(pool.O, pool.D, orc.HIT_DTYPE)
    fn = _case(pool, want, want, o=o)
    flag_light_and_floor_only(pool, want, fn.least)
    pool = occlusion_pool(lo, hi, light, kmax=1, ordinary=R.query_rays(o, light, 1600, seed=6))
    q, _ = quad_occluded(pool.O, pool.D, pool.last, light)
    oc = _case(pool, sc.is_occluded_many(pool.O, pool.D, pool.last) != 0, o.find_nearest(pool.O, pool.D), o=o, quad=q)
    return fn, oc


def sample_case(o, name):
    """sample_query_kernel in world `name` of tests/test_gpu_sample_query.py (`o`: its oracle): rgb and the returned seed by the oracle's Sample; cost = draws.
    The two-level worlds (tlas_kd, tlas_grid: `o` walks the structure, orc.set_blas_accel) also hold the committed rays of alt_disagreement.py, spread through
    the ordinary rays."""
    prim = name == "prim"
    lo, hi = (None, None) if prim else scene_box(o, 1 if name.startswith("tlas") else 0)
    extra = None
    if name in ("tlas_kd", "tlas_grid"):
        import alt_disagreement as ad
        extra = ad.load(name[5:])[:4]
    pool = sample_pool(o, prim, lo, hi, extra=extra)
    c = Case()
    c.pool, c.want, c.cost, c.o = pool, pool.want, pool.cost, o
    return c
