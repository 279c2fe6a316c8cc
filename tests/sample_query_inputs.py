"""Inputs of the crt_sample tests, shared by tests/test_gpu_sample_query.py (device against oracle) and tests/test_sample_query_cpu.py (the oracle alone: do the
inputs reach every branch of Renderer::Sample?).  One scene description serves FileScene (BVH, KD-tree, grid) and TLASFileScene: the bunny as a dielectric with
absorption, a mirror cube and a diffuse textured cube over the textured floor, under the light quad and the sky.  Everything here is numpy + the CPU oracle."""
import numpy as np

LIGHT = (0.0, 3.0, 1.0)                                                   # write_scene's light position; the floor is the plane y = -1
MATS = [(0.0, 1.0, (0.5, 0.2, 0.1), ""),                                  # 0: dielectric with absorption (the bunny)
        (1.0, 0.0, (0.0, 0.0, 0.0), ""),                                  # 1: mirror
        (0.0, 0.0, (0.0, 0.0, 0.0), "../assets/textures/Defuse_wok.png")]  # 2: diffuse, textured
BUNNY_C, MIRROR_C, DIFFUSE_C = (0.0, -0.35, 2.1), (-1.6, -0.6, 2.2), (1.6, -0.6, 2.2)
EXTRA = [("cube", 1, MIRROR_C, (0.0, 30.0, 0.0), (0.4, 0.4, 0.4)), ("cube", 2, DIFFUSE_C, (0.0, -20.0, 0.0), (0.4, 0.4, 0.4))]
OBJ_MAT = [0, 1, 2]                                                       # material of object k (hit records: objIdx = 2 + k in both scene kinds)
N_RAYS = 4096


def scene_xml(tmp_path):
    from test_gpu_golden_and_edges import write_scene
    return write_scene(tmp_path, "bunny", name="sample.xml", mats=MATS, extra_objects=EXTRA)


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def seeds_for(n):
    """1 + i, and every 13th with the high bit set (never 0)"""
    i = np.arange(n, dtype=np.uint64)
    s = (i + np.uint64(1)).astype(np.uint32)
    hi = (np.uint64(0x80000000) | ((i * np.uint64(2654435761)) & np.uint64(0x7fffffff)) | np.uint64(1)).astype(np.uint32)
    s[::13] = hi[::13]
    return s


def xorshift(s):
    s = s.astype(np.uint32).copy()
    s ^= s << np.uint32(13); s ^= s >> np.uint32(17); s ^= s << np.uint32(5)
    return s


def rnd(s):
    """RandomFloat(seed): (new state, float32 in [0, 1))"""
    s = xorshift(s)
    return s, s.astype(np.float32) * np.float32(2.3283064365387e-10)


def init_seed(base):
    """InitSeed (WangHash((base + 1) * 17)) in uint32 arithmetic"""
    M = np.uint64(0xffffffff)
    s = ((np.asarray(base).astype(np.uint64) + np.uint64(1)) * np.uint64(17)) & M
    s = (s ^ np.uint64(61)) ^ (s >> np.uint64(16)); s = (s * np.uint64(9)) & M; s = s ^ (s >> np.uint64(4)); s = (s * np.uint64(0x27d4eb2d)) & M; s = s ^ (s >> np.uint64(15))
    return s.astype(np.uint32)


def draws(seed_in, seed_out, limit=512):
    """how many xorshift32 steps lead from seed_in to seed_out (-1: more than `limit`)"""
    s = np.asarray(seed_in, np.uint32).copy(); out = np.asarray(seed_out, np.uint32)
    k = np.full(len(s), -1, np.int64); k[s == out] = 0
    for j in range(1, limit + 1):
        s = xorshift(s)
        k[(k < 0) & (s == out)] = j
    return k


def camera_like(n, rng, targets, spread=0.3):
    O = np.tile(np.array([0.0, 0.3, -2.0], np.float32), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    T = np.asarray(targets, np.float32)[np.arange(n) % len(targets)] + rng.normal(scale=spread, size=(n, 3)).astype(np.float32)
    return O, unit(T - O)


def triangle_rays(o, n=N_RAYS, seed=5):
    """the ray set of one triangle-scene world (`o`: an oracle holding scene_xml's scene, used to find points inside the bunny): a quarter each of camera-like rays
    at the three objects and the floor, rays that start just inside the dielectric with inside = 1, rays aimed at the light, rays aimed at the sky.
    Returns O, D [n, 3] float32, inside [n] int32, seeds [n] uint32."""
    rng = np.random.default_rng(seed)
    q = n // 4
    Oa, Da = camera_like(q, rng, [BUNNY_C, MIRROR_C, DIFFUSE_C, (0.0, -1.0, 0.8)])
    # inside the dielectric: where a ray at the bunny enters it, a little further along, in a direction near the ray's
    Ob, Db = camera_like(q, rng, [BUNNY_C], spread=0.2)
    h = o.find_nearest(Ob, Db)
    entered = h["objIdx"] == 2
    I = (Ob + h["t"][:, None] * Db).astype(np.float32)
    Ob = np.where(entered[:, None], I + np.float32(2e-3) * Db, Ob).astype(np.float32)
    Db = np.where(entered[:, None], unit(Db + rng.normal(scale=0.3, size=(q, 3)).astype(np.float32)), Db).astype(np.float32)
    inside_b = entered.astype(np.int32)
    # at the light: from points between floor and light, up at the quad (half size 0.5)
    Oc = np.stack([rng.uniform(-2.0, 2.0, q), rng.uniform(-0.9, 0.5, q), rng.uniform(-0.5, 3.5, q)], 1).astype(np.float32)
    Tc = np.stack([LIGHT[0] + rng.uniform(-0.45, 0.45, q), np.full(q, LIGHT[1]), LIGHT[2] + rng.uniform(-0.45, 0.45, q)], 1).astype(np.float32)
    Dc = unit(Tc - Oc)
    # at the sky
    m = n - 3 * q
    Od = np.tile(np.array([0.0, 0.3, -2.0], np.float32), (m, 1)) + rng.uniform(-0.5, 0.5, (m, 3)).astype(np.float32)
    Dd = unit(np.stack([rng.uniform(-1, 1, m), rng.uniform(0.3, 1.0, m), rng.uniform(-1, 1, m)], 1))
    O = np.concatenate([Oa, Ob, Oc, Od]).astype(np.float32); D = np.concatenate([Da, Db, Dc, Dd]).astype(np.float32)
    inside = np.concatenate([np.zeros(q, np.int32), inside_b, np.zeros(q + m, np.int32)])
    perm = rng.permutation(n)                                             # the classes mixed over the lanes of every wavefront
    return O[perm], D[perm], inside[perm], seeds_for(n)


def two_level_rays(o, kind):
    """the ray set of a two-level world ("kd" / "grid"): triangle_rays plus the committed rays on which tlas_scene.xml's structures disagree (alt_disagreement.py)"""
    import alt_disagreement as ad
    O, D, inside, seeds = triangle_rays(o)
    Oa, Da, ia, sa, _ = ad.load(kind)
    return np.concatenate([O, Oa]), np.concatenate([D, Da]), np.concatenate([inside, ia]).astype(np.int32), np.concatenate([seeds, sa]).astype(np.uint32)


def prim_rays(n=N_RAYS, seed=7):
    """rays inside the PrimitiveScene's room, half of them aimed at the small objects; every fourth with inside = 1"""
    rng = np.random.default_rng(seed)
    O = np.stack([rng.uniform(-2.8, 2.8, n), rng.uniform(-0.9, 1.9, n), rng.uniform(-2.8, 3.8, n)], axis=1).astype(np.float32)
    D = unit(rng.normal(size=(n, 3)))
    targets = np.array([[-1.8, 0.2, 1.0], [1.8, 0.0, 2.5], [-0.25, 0.0, 2.0], [0.0, 1.7, 2.0]], np.float32)
    k = n // 2
    T = targets[rng.integers(0, len(targets), k)] + rng.normal(scale=0.4, size=(k, 3)).astype(np.float32)
    D[:k] = unit(T - O[:k])
    inside = (np.arange(n) % 4 == 1).astype(np.int32)
    return O, D.astype(np.float32), inside, seeds_for(n)


def oracle_sample(o, O, D, inside, seeds):
    """Oracle.sample per ray: (rgb [n, 3] float32, seeds out [n] uint32, the growth of the oracle's counters {name: delta})"""
    c0 = o.counters()
    rgb = np.zeros((len(O), 3), np.float32); out = np.zeros(len(O), np.uint32)
    for i in range(len(O)):
        rgb[i], out[i] = o.sample(O[i], D[i], int(seeds[i]), int(inside[i]))
    c1 = o.counters()
    return rgb, out, {k: c1[k] - c0[k] for k in c1}


def first_hit_classes(o, O, D, inside):
    """counts of the rays by what Sample meets first (the oracle's find_nearest + MATS)"""
    h = o.find_nearest(O, D, inside)
    obj = h["objIdx"]
    mat = np.full(len(obj), -1)
    mesh = obj >= 2
    mat[mesh] = np.asarray(OBJ_MAT)[obj[mesh] - 2]
    refl = np.array([m[0] for m in MATS]); refr = np.array([m[1] for m in MATS])
    mirror = mesh & (refl[mat] > 0)
    diel = mesh & (refl[mat] == 0) & (refr[mat] > 0)
    return dict(mirror=int(mirror.sum()), dielectric_outside=int((diel & (inside == 0)).sum()), dielectric_inside=int((diel & (inside != 0)).sum()),
                diffuse=int(((obj == 1) | (mesh & ~mirror & ~diel)).sum()), diffuse_textured_mesh=int((mesh & (mat == 2)).sum()), light=int((obj == 0).sum()),
                miss=int((obj == -1).sum()))


def assert_branches(o, O, D, inside, seeds, seeds_out):
    """the premise of the parity test: at least 100 rays of every first-hit class, 100 paths that draw nothing and 100 that draw more than 10 numbers"""
    c = first_hit_classes(o, O, D, inside)
    assert all(v >= 100 for v in c.values()), c
    k = draws(seeds, seeds_out)
    assert (k >= 0).all()
    assert int((k == 0).sum()) >= 100 and int((k > 10).sum()) >= 100, (int((k == 0).sum()), int((k > 10).sum()))
    return c, k
