"""The HIP kernels against the float64 brute-force truth of tests/mesh_truth.py, directly: find_nearest / find_nearest_alt / find_nearest_device,
is_occluded(accel) and get_hit_info through the six worlds a mesh scene can be walked by, the scene the host front rebuilds (move_and_rebuild), and every structure
the DEVICE refits or rebuilds (refit_device, build_bvh_device, build_kdtree_device, build_grid_device, update_transforms_device), for which the oracle has no counterpart: the truth over the moved triangles
does not care how the tree was made.  The criterion, its tolerances and its caps are those tests/test_mesh_truth_cpu.py settles on the CPU oracle.

Two behaviours of the reference are not the nearest hit, and are excused exactly where they explain a ray and nowhere else: the two-level KD-tree's lost hits
(only where the oracle, through the same structure, returns the same bits; counted against the CPU test's cap) and BVH::Refit's stale node 1
(mesh_truth.refit_excused)."""
import numpy as np
import pytest

import bvh_build_inputs as B
import mesh_truth as mt
import mesh_truth_scenes as MC
from conftest import ASSETS

torch = pytest.importorskip("torch")

import test_gpu_grid_device as TG                                          # noqa: E402  (helpers only)
from test_gpu_analytic_truth import WORLDS                                 # noqa: E402

pytestmark = pytest.mark.gpu

N_RAYS = 1024
SCENE_OF = {"bvh": ("bunny",), "kd": ("bunny",), "grid": ("bunny",), "tlas": ("tlas", "gen"), "tlas_kd": ("tlas", "gen"), "tlas_grid": ("tlas", "gen")}
CASES = [(w, s) for w in WORLDS for s in SCENE_OF[w]]
HIT_BITS = ("t", "u", "v", "objIdx", "triIdx")


def accel_of(crt, world):
    return {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}.get(world.split("_")[-1], 0)


def host_scene(crt, name, tmp):
    hs = crt.HostScene(MC.scene_xml(name, tmp), MC.SCENES[name], ASSETS)
    if name == "gen":
        for i, T in enumerate(mt.generated_transforms(hs)):
            hs.set_transform(i, T)
    return hs


class Case:
    """a scene as the HOST FRONT loads it (the truth's arrays come from the library's own scene, not from the oracle's), its rays and their truth"""

    def __init__(self, crt, orc, name, tmp):
        self.name, self.kind, self.tmp = name, MC.SCENES[name], tmp
        hs = host_scene(crt, name, tmp)
        self.sc, light, obj_mat, invto = MC.describe(orc, MC.scene_xml(name, tmp))
        self.described = (light, obj_mat, invto)
        self.world = mt.world_of(hs, self.kind, light, obj_mat, invto)
        self.O, self.D, self.cls = mt.make_rays(self.world, N_RAYS, seed=11 + len(name), aim=mt.GEN_AIM if name == "gen" else None)
        self.tr = mt.nearest_truth(self.world, self.O, self.D)
        self.ti = mt.hit_info_truth(self.world, self.O, self.D, self.tr)
        self.t_shadow = mt.shadow_lengths(self.tr, 5)
        self.occ = mt.occluded_truth(self.world, self.O, self.D, self.t_shadow, self.tr)
        self.caps = mt.check_caps(self.tr, name)
        for a in (self.O, self.D, self.t_shadow):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def cases(crt, orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mesh_truth_gpu")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(crt, orc, name, tmp)
        return made[name]
    return get


def open_ctx(crt, c, world):
    hs = host_scene(crt, c.name, c.tmp)
    accel = accel_of(crt, world)
    if accel:
        hs.build_alt(accel)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    if accel:
        hs.upload_alt(ctx, accel)
    return hs, ctx, accel


def nearest_all_ways(crt, ctx, kind, accel, O, D):
    """the hit records of every find-nearest entry that serves (kind, accel): they agree bit for bit; returns one"""
    dev = TG.hits_np(crt, ctx.find_nearest_device(TG.ray_records(crt, O, D), accel=accel))
    torch.cuda.synchronize()
    host = ctx.find_nearest(O, D) if accel == 0 else (ctx.find_nearest_alt(accel, O, D) if kind == 0 else None)
    if host is not None:
        for f in HIT_BITS:
            assert np.array_equal(np.asarray(host[f]).view(np.uint32), np.asarray(dev[f]).view(np.uint32)), ("host and device entries differ", f)
    return dev


def same_bits(a, b, rays):
    return all(np.array_equal(np.asarray(a[f][rays]).view(np.uint32), np.asarray(b[f][rays]).view(np.uint32)) for f in HIT_BITS)


def check_queries(crt, ctx, kind, accel, O, D, tr, ti, ts, occ, what, excused=None, occ_excused=None, occ_oracle=None, occ_cap=0, reached=None):
    """find_nearest (every entry), is_occluded and get_hit_info of `ctx` through `accel` against the truth.  The reference's own behaviours:
    excused / occ_excused    the rays mesh_truth.refit_excused explains (or, excused alone, the two-level KD-tree's violations that are the oracle's bits);
                             with `reached` (mesh_truth.without_node1) they are held to what the refitted walk does reach
    occ_oracle, occ_cap      the oracle's is_occluded through the same two-level KD-tree: a required 1 answered 0 stands only where the oracle answers 0 too,
                             on at most occ_cap rays"""
    hits = nearest_all_ways(crt, ctx, kind, accel, O, D)
    viol = mt.nearest_violations(tr, hits)
    bad = mt.rays_of(viol)
    if excused is not None:
        if reached is not None:
            assert len(mt.refit_violations(reached, O, D, tr, hits, bad[excused[bad]])) == 0, MC.report(what + ", beyond node 1", viol, O, D, hits, tr)
        bad = bad[~excused[bad]]
    assert len(bad) == 0, MC.report(what, {k: v[np.isin(v, bad)] for k, v in viol.items() if np.isin(v, bad).any()}, O, D, hits, tr)
    got = np.asarray(ctx.is_occluded(O, D, ts, accel=accel)) != 0
    ob = mt.occluded_violations(occ[0], occ[1], got)
    if occ_excused is not None:
        lost = occ_excused[ob] & occ[0][ob] & ~got[ob]
        assert len(mt.refit_occluded_violations(reached, O, D, ts, ob[lost])) == 0, (what, "is_occluded, an occluder outside node 1", ob[:8].tolist())
        ob = ob[~lost]
    if occ_oracle is not None:
        lost = occ[0][ob] & ~got[ob] & ~(np.asarray(occ_oracle) != 0)[ob]
        print("%s: is_occluded loses %d required occluders, as the oracle does" % (what, lost.sum()))
        assert lost.sum() <= occ_cap, (what, "is_occluded", int(lost.sum()), occ_cap)
        ob = ob[~lost]
    assert len(ob) == 0, (what, "is_occluded", ob[:8].tolist())
    dev = ctx.is_occluded_device(TG.ray_records(crt, O, D, ts, crt.SHADOW_RAY_DTYPE), accel=accel).cpu().numpy()
    assert np.array_equal(dev != 0, got), (what, "is_occluded_device")
    info = ctx.get_hit_info(O, D, hits)
    hv, n = mt.hit_info_violations(tr, ti, hits, info)                     # (compared wherever the answer names the truth's own hit)
    assert not hv, (what, "get_hit_info", {k: (len(v), v[:4].tolist()) for k, v in hv.items()})
    return hits, n


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the six worlds
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,scene", CASES)
def test_worlds(crt, orc, cases, world, scene):
    c = cases(scene)
    if c.kind == 1:
        assert c.caps["blases"] >= 2
    hs, ctx, accel = open_ctx(crt, c, world)
    excused = occ_oracle = None; occ_cap = 0
    if world == "tlas_kd":
        # the two-level KD-tree's own behaviour: a violation stands only where the oracle, through the same structure, returns the same bits
        o, _, _ = MC.load(orc, scene, c.tmp)
        want = MC.through(orc, o, world).find_nearest(c.O, c.D)
        hits = TG.hits_np(crt, ctx.find_nearest_device(TG.ray_records(crt, c.O, c.D), accel=accel)); torch.cuda.synchronize()
        bad = mt.rays_of(mt.nearest_violations(c.tr, hits))
        assert same_bits(hits, want, bad), (scene, "tlas_kd violations that are not the oracle's", bad[:8].tolist())
        print("%s tlas_kd: %d violations of %d rays" % (scene, len(bad), len(c.O)))
        assert len(bad) <= mt.TLAS_KD_VIOLATIONS[scene][1] * len(c.O), (len(bad), mt.TLAS_KD_VIOLATIONS[scene])
        excused = np.zeros(len(c.O), bool); excused[bad] = True
        occ_oracle = o.is_occluded(c.O, c.D, c.t_shadow); occ_cap = mt.TLAS_KD_VIOLATIONS[scene][1] * len(c.O)
    _, n = check_queries(crt, ctx, c.kind, accel, c.O, c.D, c.tr, c.ti, c.t_shadow, c.occ, "%s through %s" % (scene, world), excused,
                         occ_oracle=occ_oracle, occ_cap=occ_cap)
    assert n >= (0.7 if world == "tlas_kd" else 0.8) * len(c.O)
    assert c.occ[0].sum() >= 50 and (~c.occ[1]).sum() >= 50
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. structures the device refits and rebuilds
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Moved:
    """scene `name` with BVH `bvh` at B.wobble positions: the truth over the MOVED triangles"""

    def __init__(self, crt, c, bvh):
        hs = host_scene(crt, c.name, c.tmp)
        self.bvh, self.n = bvh, hs.bvh_count()
        self.p = B.wobble(TG.positions(hs.bvh(bvh)))
        tris = [MC.moved_records(hs.bvh(i)["tris"], self.p) if i == bvh else hs.bvh(i)["tris"] for i in range(self.n)]
        light, obj_mat, invto = c.described
        tr = [hs.blas_transform(i) for i in range(self.n)] if c.kind == 1 else None
        self.T = np.stack([t[0] for t in tr]) if tr else None
        self.world = mt.World(c.kind, tris, self.T, [t[1] for t in tr] if tr else None, light, obj_mat, invto)
        self.O, self.D, _ = mt.make_rays(self.world, N_RAYS, seed=23)
        self.tr = mt.nearest_truth(self.world, self.O, self.D)
        self.ti = mt.hit_info_truth(self.world, self.O, self.D, self.tr)
        self.ts = mt.shadow_lengths(self.tr, 6)
        self.occ = mt.occluded_truth(self.world, self.O, self.D, self.ts, self.tr)
        mt.check_caps(self.tr, c.name + " moved")
        hs.close()


@pytest.fixture(scope="module")
def moved(crt, cases):
    made = {}

    def get(name, bvh):
        if name not in made:
            made[name] = Moved(crt, cases(name), bvh)
        return made[name]
    return get


@pytest.mark.parametrize("op", ["refit", "bvh", "kd", "grid", "host_rebuild"])
@pytest.mark.parametrize("scene,bvh", [("bunny", 0), ("tlas", 1)])
def test_device_built_structures(crt, orc, cases, moved, scene, bvh, op):
    c = cases(scene); m = moved(scene, bvh)
    world = {"kd": "kd", "grid": "grid"}.get(op, "")
    hs, ctx, accel = open_ctx(crt, c, world)
    before = nearest_all_ways(crt, ctx, c.kind, 0, m.O, m.D)
    t = TG.to_dev(m.p)
    if op == "host_rebuild":                                                # the host front's BVH::Build over the moved triangles (+ TLAS), uploaded afresh
        hs.move_and_rebuild(bvh, m.p); hs.upload(ctx)
    elif op == "bvh":
        ctx.build_bvh_device(bvh, t)
    else:
        ctx.refit_device(bvh, t)
    if c.kind == 1 and op != "host_rebuild":
        ctx.update_transforms_device(TG.to_dev(m.T))
    if op == "kd":
        ctx.build_kdtree_device(bvh, t)
    elif op == "grid":
        ctx.build_grid_device(bvh, t)
    what = "%s after %s" % (scene, op)
    excused = occ_ex = occ_oracle = reached = None; occ_cap = 0
    if op == "refit":
        b = ctx.get_bvh(bvh)
        reached = mt.without_node1(m.world, bvh, b["nodes"], b["indices"])
        excused = mt.refit_excused(m.world, bvh, b["nodes"], b["indices"], m.O, m.D, m.tr)
        occ_ex = mt.refit_excused(m.world, bvh, b["nodes"], b["indices"], m.O, m.D, m.tr, whole_ray=True)
    elif c.kind == 1 and op == "kd":
        o, _ = orc.load_scene(MC.scene_xml(scene, c.tmp), 1, ASSETS)
        o.move_and_refit(bvh, m.p)
        want = MC.through(orc, o, "tlas_kd").find_nearest(m.O, m.D)
        hits = TG.hits_np(crt, ctx.find_nearest_device(TG.ray_records(crt, m.O, m.D), accel=accel)); torch.cuda.synchronize()
        bad = mt.rays_of(mt.nearest_violations(m.tr, hits))
        assert same_bits(hits, want, bad) and len(bad) <= mt.TLAS_KD_VIOLATIONS[scene][1] * len(m.O), (what, bad[:8].tolist())
        excused = np.zeros(len(m.O), bool); excused[bad] = True
        occ_oracle = o.is_occluded(m.O, m.D, m.ts); occ_cap = mt.TLAS_KD_VIOLATIONS[scene][1] * len(m.O)
    hits, _ = check_queries(crt, ctx, c.kind, accel, m.O, m.D, m.tr, m.ti, m.ts, m.occ, what, excused, occ_ex, occ_oracle, occ_cap, reached)
    if excused is not None and op == "refit":
        print("%s: %d rays excused by node 1's stale box" % (what, excused.sum()))
    if c.kind == 1:                                                         # where the moved BLAS is the answer neither before nor after, the answer is unchanged
        others = (before["objIdx"] != 2 + bvh) & (hits["objIdx"] != 2 + bvh) & (~excused if excused is not None else True)
        assert others.sum() >= 300 and same_bits(before, hits, others), what
    ctx.close(); hs.close()


@pytest.mark.parametrize("name", mt.REBUILD_MESHES)
def test_generated_meshes_built_on_the_device(crt, name):
    """uploaded under a leaf root (test_gpu_grid_device.leaf_root_bvh), then each structure built on the device and asked"""
    p = B.mesh(crt, name)
    w = mt.mesh_world(p)
    O, D, _ = mt.make_rays(w, N_RAYS, seed=31, near=mt.AIMED_FROM.get(name))
    tr = mt.nearest_truth(w, O, D); ti = mt.hit_info_truth(w, O, D, tr)
    ts = mt.shadow_lengths(tr, 6); occ = mt.occluded_truth(w, O, D, ts, tr)
    mt.check_caps(tr, name, min_mesh=0 if name == "cluster" else mt.MIN_MESH)
    if name == "cluster":
        assert np.isfinite(tr["mesh_hi"]).sum() <= 0.15 * len(O)             # nearly every |a| is below 1e-4: the truth is "no hit"
    ctx = crt.Context(64, 64)
    TG.upload_described(crt, ctx, TG.leaf_root_bvh(crt, p))
    t = TG.to_dev(p)
    ctx.build_bvh_device(0, t)
    check_queries(crt, ctx, 0, 0, O, D, tr, ti, ts, occ, name + " build_bvh_device")
    ctx.build_kdtree_device(0, t)
    check_queries(crt, ctx, 0, crt.ACCEL_KDTREE, O, D, tr, ti, ts, occ, name + " build_kdtree_device")
    ctx.build_grid_device(0, t)
    check_queries(crt, ctx, 0, crt.ACCEL_GRID, O, D, tr, ti, ts, occ, name + " build_grid_device")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. transforms on the device
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_transforms_with_scale_on_the_device(crt, cases):
    """the generated scene moved by update_transforms_device to new rotations, places and scales >= 1 (see mesh_truth.py on what SetTransform makes of a scale);
    the truth takes T as sent and invT as the library reports it"""
    import tlas_device_inputs as TD
    c = cases("gen")
    hs = host_scene(crt, "gen", c.tmp)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    place = [((-1.0, 0.1, 3.2), (0.3, 0.9, 0.2), 1.0), ((1.0, -0.2, 3.0), (0.1, -0.7, 0.4), 1.5), ((0.1, 0.3, 2.6), (0.5, 0.2, -0.3), 2.5), ((-0.2, -0.3, 2.3), (-0.4, 0.6, 0.1), 1.0)]
    T = np.stack([TD.rigid(p, a) for p, a, _ in place])
    for i, (_, _, s) in enumerate(place):
        T[i, :3, :3] *= np.float32(s)
    hs.set_transforms_device(ctx, TG.to_dev(T))
    tr_ = [hs.blas_transform(i) for i in range(4)]
    assert all(np.array_equal(tr_[i][0].reshape(4, 4), T[i]) for i in range(4))
    light, obj_mat, invto = c.described
    w = mt.World(1, [hs.bvh(i)["tris"] for i in range(4)], T, [t[1] for t in tr_], light, obj_mat, invto)
    assert abs(np.linalg.det(w.invT[2][:3, :3]) - 2.5 ** 3) <= 1e-3           # invT = s R^T: it scales d
    O, D, _ = mt.make_rays(w, N_RAYS, seed=29)
    tr = mt.nearest_truth(w, O, D); ti = mt.hit_info_truth(w, O, D, tr)
    ts = mt.shadow_lengths(tr, 6); occ = mt.occluded_truth(w, O, D, ts, tr)
    seen = mt.check_caps(tr, "gen moved on the device")
    assert seen["blases"] >= 3
    check_queries(crt, ctx, 1, 0, O, D, tr, ti, ts, occ, "update_transforms_device")
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. Sample's first hit
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,scene", CASES)
def test_sample_returns_the_sky_on_the_truths_misses(crt, orc, cases, world, scene):
    """depth limit 0: Sample returns the sky texel for a miss and 0 for any hit (3. PathTracer/renderer.cpp:54-55), so the rays that come back coloured are the
    rays FindNearest missed.  They must hold every ray without a soft candidate and none with a robust one.  (The colour itself is not compared.)"""
    c = cases(scene)
    hs = host_scene(crt, scene, c.tmp)
    accel = accel_of(crt, world)
    if accel:
        hs.build_alt(accel)
    ctx = crt.Context(64, 64, depth_limit=0); hs.upload(ctx)
    if accel:
        hs.upload_alt(ctx, accel)
    seeds = torch.from_numpy(((np.arange(len(c.O), dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)).view(np.int32).copy()).to(TG.dev())
    rgb, _ = ctx.sample_device(TG.ray_records(crt, c.O, c.D), seeds=seeds, accel=accel)
    rgb = rgb.cpu().numpy()
    assert np.isfinite(rgb).all()
    sky = (rgb != 0).any(axis=1)
    must_sky, must_not = c.tr["t_lo"] == np.inf, np.isfinite(c.tr["t_hi"])
    bad = np.flatnonzero((must_sky & ~sky) | (must_not & sky))
    if world == "tlas_kd":                                                  # a lost hit shows the sky: only where the oracle's walk of the same structure misses too
        o, _, _ = MC.load(orc, scene, c.tmp)
        lost = MC.through(orc, o, world).find_nearest(c.O, c.D)["objIdx"] < 0
        assert lost[bad].all() and len(bad) <= mt.TLAS_KD_VIOLATIONS[scene][1] * len(c.O)
    else:
        assert len(bad) == 0, (scene, world, bad[:8].tolist())
    assert must_sky.sum() >= mt.MIN_MISS and sky.sum() >= mt.MIN_MISS
    ctx.close(); hs.close()
