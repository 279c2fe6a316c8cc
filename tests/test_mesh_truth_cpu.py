"""The CPU oracle against the float64 brute-force truth of tests/mesh_truth.py: every query over a triangle mesh, through every structure the oracle can walk a
scene by, on the scene as loaded, refitted and rebuilt.  The truth does not depend on the structure, so a misreading that oracle, host build and kernel share
does not pass here.  tests/test_gpu_mesh_truth.py holds the kernels to the same truth with the same criterion; what is settled here first is that the criterion
itself is met by a correct float32 evaluation (zero violations), that it has teeth (doctored answers are rejected), and the tolerances it asserts.

The host-rebuilt scene (HostScene.move_and_rebuild) cannot be queried without a GPU; here the oracle builds its own tree over the moved triangles, that tree is
asserted equal to the host's build (crt.host_bvh_build), and the GPU module queries the host-rebuilt scene itself."""
import os
import time

import numpy as np
import pytest

import alt_disagreement as AD
import bvh_build_inputs as B
import hit_info_restate as hr
import light_quad_inputs as lq
import mesh_truth as mt
import render_looks_inputs as li
from conftest import ASSETS
from mesh_truth_scenes import SCENES, describe, load, moved_records, report, scene_xml, through

N_RAYS = 4096
WORLDS = {0: ("bvh", "kd", "grid"), 1: ("tlas", "tlas_kd", "tlas_grid")}
CASES = [(s, w) for s, k in SCENES.items() for w in WORLDS[k]]


class Case:
    """a scene, its rays and their truth, computed once per module and never written to"""

    def __init__(self, orc, name, tmp, n=N_RAYS):
        self.name, self.kind = name, SCENES[name]
        self.o, self.sc, self.world = load(orc, name, tmp)
        self.O, self.D, self.cls = mt.make_rays(self.world, n, seed=11 + len(name), aim=mt.GEN_AIM if name == "gen" else None)
        t0 = time.time()
        self.tr = mt.nearest_truth(self.world, self.O, self.D)
        self.seconds = time.time() - t0
        self.ti = mt.hit_info_truth(self.world, self.O, self.D, self.tr)
        self.t_shadow = mt.shadow_lengths(self.tr, 5)
        self.occ = mt.occluded_truth(self.world, self.O, self.D, self.t_shadow, self.tr)
        self.sh = hr.SceneShading(orc, self.o, self.sc, self.kind, ASSETS)
        for a in (self.O, self.D, self.t_shadow):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def cases(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mesh_truth")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(orc, name, tmp)
        return made[name]
    return get


def kd_violations_are_documented(orc, c, hits, viol):
    """every tlas_kd violation is a ray on which the two-level KD-tree parts from the TLAS-BVH in one of the ways tests/alt_disagreement.py documents: it loses
    the BVH's hit (a larger t) or finds a hit the BVH has culled (a smaller t)"""
    bad = mt.rays_of(viol)
    bvh_hits = through(orc, c.o, "tlas").find_nearest(c.O, c.D)
    d, lost, found = AD.differ(bvh_hits, hits)
    assert (d[bad] & (lost[bad] | found[bad])).all(), report("tlas_kd violations that are not a lost or a found hit", viol, c.O, c.D, hits, c.tr)
    return int(lost[bad].sum()), int(found[bad].sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. zero violations
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,world", CASES)
def test_oracle_meets_the_criterion(orc, cases, scene, world):
    c = cases(scene)
    seen = mt.check_caps(c.tr, scene)
    if c.kind == 1:
        assert seen["blases"] >= 2
    o = through(orc, c.o, world)
    hits = o.find_nearest(c.O, c.D)
    viol = mt.nearest_violations(c.tr, hits)
    print(scene, world, "find_nearest:", mt.nearest_deviation(c.tr, hits))
    if world == "tlas_kd":
        n = mt.count(viol)
        lost, found = kd_violations_are_documented(orc, c, hits, viol) if n else (0, 0)
        through(orc, c.o, world)
        print("%s tlas_kd: %d violations of %d rays (%d lost hits, %d culled hits found)" % (scene, n, len(c.O), lost, found))
        recorded, cap = mt.TLAS_KD_VIOLATIONS[scene]
        assert n == recorded, (n, recorded)                                # the table in mesh_truth.py records what the oracle gives
        assert n <= cap * len(c.O)
    else:
        assert not viol, report("%s through %s" % (scene, world), viol, c.O, c.D, hits, c.tr)
    occ = o.is_occluded(c.O, c.D, c.t_shadow)
    bad = mt.occluded_violations(c.occ[0], c.occ[1], occ)
    if world == "tlas_kd":                                                  # a lost hit can turn a required 1 into 0, nothing else
        assert (c.occ[0][bad] & (occ[bad] == 0)).all() and len(bad) <= mt.TLAS_KD_VIOLATIONS[scene][1] * len(c.O), bad[:8].tolist()
    else:
        assert len(bad) == 0, (scene, world, "is_occluded", bad[:8].tolist())
    assert c.occ[0].sum() >= 200 and (~c.occ[1]).sum() >= 200                # both answers are asked for
    info = c.sh.hit_info(c.O, c.D, hits)
    hv, n = mt.hit_info_violations(c.tr, c.ti, hits, info)
    print(scene, world, "hit_info over %d rays:" % n, mt.hit_info_deviation(c.tr, c.ti, hits, info))
    assert n >= (0.7 if world == "tlas_kd" else 0.8) * len(c.O) and not hv, (scene, world, {k: (len(v), v[:4].tolist()) for k, v in hv.items()})


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the tolerance table and the cost
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_tolerance_table(orc, cases):
    """the observed column of mesh_truth.TOL is what the oracle shows when this test runs; the asserted column is 4 x that"""
    worst = dict(t=0.0, u=0.0, v=0.0, I=0.0, N=0.0, uv=0.0)
    for scene, world in CASES:
        if world == "tlas_kd":                                              # (its lost hits are no rounding; everywhere else it returns the TLAS-BVH's bits)
            continue
        c = cases(scene)
        o = through(orc, c.o, world)
        hits = o.find_nearest(c.O, c.D)
        d = mt.nearest_deviation(c.tr, hits)
        d.update(mt.hit_info_deviation(c.tr, c.ti, hits, c.sh.hit_info(c.O, c.D, hits)))
        assert d["n"] >= 0.7 * len(c.O)                                    # the rays with a tight interval are most of them
        for k in worst:
            worst[k] = max(worst[k], d[k])
    print("observed on the oracle:", {k: "%.3g" % v for k, v in worst.items()})
    print("truth of the largest set (tlas_scene.xml, %d rays x %d triangles): %.1f s" % (N_RAYS, sum(len(t) for t in cases("tlas").world.tris), cases("tlas").seconds))
    for k, (observed, asserted) in mt.TOL.items():
        assert worst[k] <= observed * 1.001, (k, worst[k], observed)       # the table is not behind the oracle ...
        assert worst[k] >= observed * 0.5, (k, worst[k], observed)         # ... nor padded
        assert abs(asserted - 4 * observed) <= 0.02 * asserted, k


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the generated scene depends on where |a| >= 1e-4 is evaluated
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_generated_scene_depends_on_the_space_of_the_determinant_test(orc, cases):
    c = cases("gen")
    O = np.concatenate([c.O] + [mt.tiny_cube_rays(c.world, b, 256, 40 + b)[0] for b in (2, 3)])
    D = np.concatenate([c.D] + [mt.tiny_cube_rays(c.world, b, 256, 40 + b)[1] for b in (2, 3)])
    tr = mt.nearest_truth(c.world, O, D)
    invisible, visible = mt.threshold_dependent(c.world, O, D, tr)
    print("rays that pass through a face whose |a| < 1e-4: %d; rays that hit a face only because invT scales d: %d" % (invisible.sum(), visible.sum()))
    assert invisible.sum() >= 20 and visible.sum() >= 20
    assert set(tr["blas"][visible].tolist()) == {2}                         # the tiny cube under the T of scale 2
    for world in ("tlas", "tlas_grid"):                                     # (tlas_kd loses hits on cubes this small: test_oracle_meets_the_criterion counts them)
        hits = through(orc, c.o, world).find_nearest(O, D)
        viol = mt.nearest_violations(tr, hits)
        sel = np.flatnonzero(invisible | visible)
        assert not np.intersect1d(mt.rays_of(viol), sel).size, report(world, viol, O, D, hits, tr)
        assert (hits["objIdx"][visible] == 4).mean() >= 0.9                 # and the oracle does see those faces


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. refitted and rebuilt scenes, generated meshes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def corners_of(tris):
    def il(a, b, c):
        return np.stack([tris[a], tris[b], tris[c]], 1).reshape(len(tris) * 3, -1)
    return il("vertex0", "vertex1", "vertex2"), il("normal0", "normal1", "normal2"), il("uv0", "uv1", "uv2")


def rebuilt_oracle(orc, sc, kind, bvh_tris, T=None):
    """a fresh oracle scene whose BVHs are BUILT over the given triangle records (already in BVH space: the objects are added under the identity, which is
    exact); kind 1: moved to T afterwards"""
    def rp(p):
        return p if os.path.isabs(p) else os.path.normpath(os.path.join(ASSETS, p))
    o = orc.Oracle(kind)
    o.set_light_position(sc["light"])
    o.set_floor_texture(orc.pack_rgb(orc.read_image(rp(sc["plane_texture"])))); o.set_skydome(orc.pack_rgb(orc.read_image(rp(sc["skydome"]))))
    for m in sc["materials"]:
        o.add_material(m["reflectivity"], m["refractivity"], m["absorption"], orc.pack_rgb(orc.read_image(rp(m["texture"]))) if m["texture"] else None)
    if kind == 0:
        (tris,) = bvh_tris
        for k, obj in enumerate(sorted(set(tris["objIdx"].tolist()))):
            assert obj == 2 + k
            o.add_object(corners_of(tris[tris["objIdx"] == obj]), material_idx=sc["objects"][k]["material_idx"])
    else:
        for k, tris in enumerate(bvh_tris):
            o.add_object(corners_of(tris), material_idx=sc["objects"][k]["material_idx"])
    o.build()
    if kind == 1:
        for i in range(len(bvh_tris)):
            o.set_transform(i, T[i])
    return o


def check_all_queries(orc, o, sc, kind, worlds, what, n=1024, refitted=None):
    """zero violations of find_nearest, is_occluded and hit_info through every world of a scene in its current state; returns (world, rays, truth).
    refitted: the BVH that BVH::Refit went over — through the BVH / TLAS its violations are those mesh_truth.refit_excused explains, and no others"""
    _, light, obj_mat, invto = sc["_described"]
    w = mt.world_of(o, kind, light, obj_mat, invto)
    O, D, _ = mt.make_rays(w, n, seed=23)
    tr = mt.nearest_truth(w, O, D); ti = mt.hit_info_truth(w, O, D, tr)
    mt.check_caps(tr, what)
    ts = mt.shadow_lengths(tr, 6); must, may = mt.occluded_truth(w, O, D, ts, tr)
    sh = hr.SceneShading(orc, o, sc, kind, ASSETS)
    for world in worlds:
        through(orc, o, world)
        hits = o.find_nearest(O, D)
        viol = mt.nearest_violations(tr, hits)
        bad = mt.occluded_violations(must, may, o.is_occluded(O, D, ts))
        if refitted is not None and world in ("bvh", "tlas"):
            b = o.bvh(refitted)
            ex = mt.refit_excused(w, refitted, b["nodes"], b["triIndices"], O, D, tr)
            print("%s through %s: %d rays lose their hit to node 1's stale box (of %d excused): %s" % (what, world, mt.count(viol), ex.sum(), mt.rays_of(viol).tolist()))
            occ_ex = mt.refit_excused(w, refitted, b["nodes"], b["triIndices"], O, D, tr, whole_ray=True) & must
            assert ex[mt.rays_of(viol)].all() and occ_ex[bad].all(), report("%s through %s, not node 1" % (what, world), viol, O, D, hits, tr)
            assert mt.count(viol) >= 1                                      # (if Refit ever covers node 1, this test is to be tightened to zero)
            reached = mt.without_node1(w, refitted, b["nodes"], b["triIndices"])       # ... and held to what the walk does reach
            assert len(mt.refit_violations(reached, O, D, tr, hits, mt.rays_of(viol))) == 0, report("%s through %s, beyond node 1" % (what, world), viol, O, D, hits, tr)
            assert len(mt.refit_occluded_violations(reached, O, D, ts, bad)) == 0, (what, world, "is_occluded, an occluder outside node 1", bad[:8].tolist())
        else:
            assert not viol, report("%s through %s" % (what, world), viol, O, D, hits, tr)
            assert len(bad) == 0, (what, world, "is_occluded", bad[:8].tolist())
        hv, _ = mt.hit_info_violations(tr, ti, hits, sh.hit_info(O, D, hits))      # (compared wherever the answer names the truth's own hit)
        assert not hv, (what, world, {k: (len(v), v[:4].tolist()) for k, v in hv.items()})
    return w, O, D, tr


@pytest.mark.parametrize("scene,bvh", [("bunny", 0), ("tlas", 1)])
def test_refitted_and_rebuilt_scenes(crt, orc, tmp_path, scene, bvh):
    kind = SCENES[scene]
    xml = scene_xml(scene, tmp_path)
    o, sc = orc.load_scene(xml, kind, ASSETS)
    sc["_described"] = describe(orc, xml)
    p0 = np.stack([o.bvh(bvh)["tris"][k] for k in ("vertex0", "vertex1", "vertex2")], 1)
    moved = B.wobble(p0)
    worlds = [w for w in WORLDS[kind] if w != "tlas_kd"]
    # Refit: the old topology over the moved triangles; the KD-tree and the grid are built afresh over them (the reference refits neither)
    o.move_and_refit(bvh, moved)
    w, O, D, tr = check_all_queries(orc, o, sc, kind, worlds, scene + " refitted", refitted=bvh)
    assert np.array_equal(w.v[bvh].astype(np.float32), moved)
    # Build over the moved triangles: the oracle's own tree, equal to the host front's build
    tris = [moved_records(o.bvh(i)["tris"], moved) if i == bvh else o.bvh(i)["tris"] for i in range(o.bvh_count())]
    T = [o.blas_transform(i)[0] for i in range(o.bvh_count())] if kind == 1 else None
    o2 = rebuilt_oracle(orc, sc, kind, tris, T)
    b2 = o2.bvh(bvh)
    assert np.array_equal(np.stack([b2["tris"][k] for k in ("vertex0", "vertex1", "vertex2")], 1), moved)
    B.assert_bvh_equal(dict(nodes=b2["nodes"], indices=b2["triIndices"], nodesUsed=b2["nodesUsed"], maxDepth=b2["maxDepth"]), crt.host_bvh_build(moved), "host build")
    assert b2["nodesUsed"] != o.bvh(bvh)["nodesUsed"]                       # another tree than the refitted one
    check_all_queries(orc, o2, sc, kind, worlds, scene + " rebuilt")


def mesh_scene(orc, p):
    """the oracle's FileScene over bare positions, as test_gpu_grid_device.upload_described describes it to the library"""
    w = mt.mesh_world(p)
    o = orc.Oracle(0)
    o.set_light_position((0.0, 3.0, 1.0))
    tex = np.full((4, 4), 0x808080, np.uint32)
    o.set_floor_texture(tex); o.set_skydome(tex); o.add_material()
    o.add_object(corners_of(w.tris[0]))
    o.build()
    sc = dict(light=[0.0, 3.0, 1.0], materials=[dict(reflectivity=0.0, refractivity=0.0, absorption=[0, 0, 0], texture="")], objects=[dict(material_idx=0)])
    return o, sc, w


@pytest.mark.parametrize("name", mt.REBUILD_MESHES)
def test_generated_meshes(crt, orc, name):
    p = B.mesh(crt, name)
    o, sc, w = mesh_scene(orc, p)
    assert np.array_equal(np.stack([o.bvh(0)["tris"][k] for k in ("vertex0", "vertex1", "vertex2")], 1), p)
    O, D, _ = mt.make_rays(w, 1024, seed=31, near=mt.AIMED_FROM.get(name))
    tr = mt.nearest_truth(w, O, D)
    mt.check_caps(tr, name, min_mesh=0 if name == "cluster" else mt.MIN_MESH)
    if name == "cluster":
        # triangles of size <= 0.002: |a| <= 4e-6 for a unit direction, so all 300 are invisible, and so is most of what a ray could see of the 301st
        near = np.abs(O.astype(np.float64) + np.where(np.isfinite(tr["mesh_lo"]), tr["mesh_lo"], 0)[:, None] * D - 10.0).max(1) < 0.2
        assert not (np.isfinite(tr["mesh_lo"]) & ~near).any()               # no candidate at all among the small ones
        free = mt.mesh_candidates(w, O, D, a_min=0.0)
        assert np.isfinite(free["hi"]).sum() >= 300 and np.isfinite(tr["mesh_hi"]).sum() <= 0.15 * len(O)
    ts = mt.shadow_lengths(tr, 6); must, may = mt.occluded_truth(w, O, D, ts, tr)
    for world in WORLDS[0]:
        through(orc, o, world)
        hits = o.find_nearest(O, D)
        viol = mt.nearest_violations(tr, hits)
        assert not viol, report("%s through %s" % (name, world), viol, O, D, hits, tr)
        assert len(mt.occluded_violations(must, may, o.is_occluded(O, D, ts))) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. the criterion has teeth: the oracle's answers, doctored, are rejected
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1 + 1e-4, 1 - 1e-4])
def test_rejects_t_scaled(orc, cases, factor):
    for scene in SCENES:
        c = cases(scene)
        hits = through(orc, c.o, WORLDS[c.kind][0]).find_nearest(c.O, c.D)
        hits["t"] = (hits["t"].astype(np.float64) * factor).astype(np.float32)
        viol = mt.nearest_violations(c.tr, hits)
        far = (hits["objIdx"] >= 0) & (c.tr["t_hi"] - c.tr["t_lo"] <= 1e-9) & (hits["t"] * 1e-4 > 2 * mt.tol("t") * c.tr["scale"])
        assert far.sum() >= 1000 and np.isin(np.flatnonzero(far), mt.rays_of(viol)).all(), scene


def edge_neighbours(tris):
    """for every triangle, one that shares two of its vertices (or -1)"""
    v = np.stack([tris["vertex0"], tris["vertex1"], tris["vertex2"]], 1)
    ids = {}
    key = [[tuple(v[i, k].tolist()) for k in range(3)] for i in range(len(v))]
    for i, ks in enumerate(key):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ids.setdefault(frozenset((ks[a], ks[b])), []).append(i)
    out = np.full(len(v), -1)
    for pair in ids.values():
        if len(pair) >= 2:
            out[pair[0]], out[pair[1]] = pair[1], pair[0]
    return out


def test_rejects_the_neighbour_across_an_edge(orc, cases):
    for scene in ("bunny", "tlas"):
        c = cases(scene)
        hits = through(orc, c.o, WORLDS[c.kind][0]).find_nearest(c.O, c.D)
        assert not mt.nearest_violations(c.tr, hits)
        interior = (c.tr["kind_hi"] == 2) & c.tr["unique"] & ~c.tr["edge"] & ~c.tr["uninformative"]
        changed = np.zeros(len(hits), bool)
        for b, tris in enumerate(c.world.tris):
            nb = edge_neighbours(tris)
            m = interior & (c.tr["blas"] == b)
            m[m] = nb[hits["triIdx"][m]] >= 0
            hits["triIdx"][m] = nb[hits["triIdx"][m]]; changed |= m
        assert changed.sum() >= 400
        viol = mt.nearest_violations(c.tr, hits)
        assert np.array_equal(viol.get("another triangle", []), np.flatnonzero(changed)), scene


def test_rejects_T_in_place_of_invT(orc, cases, tmp_path):
    c = cases("tlas")
    o, _, _ = load(orc, "tlas", tmp_path)
    T = o.blas_transform(1)[0].reshape(4, 4).astype(np.float64)
    o.set_transform(1, np.linalg.inv(T).astype(np.float32))                   # invT of that is T: BLAS 1's rays are carried by T
    assert np.abs(o.blas_transform(1)[1].reshape(4, 4) - T).max() <= 1e-6
    hits = o.find_nearest(c.O, c.D)
    on1 = (c.tr["kind_hi"] == 2) & (c.tr["blas"] == 1) & c.tr["unique"] & ~c.tr["uninformative"]
    bad = mt.rays_of(mt.nearest_violations(c.tr, hits))
    assert on1.sum() >= 200 and np.isin(np.flatnonzero(on1), bad).mean() >= 0.95
    assert not np.isin(np.flatnonzero((c.tr["kind_hi"] == 2) & (c.tr["blas"] != 1) & (hits["objIdx"] != 3)), bad).any()     # the other BLASes' hits stand


def test_rejects_a_deleted_triangle(orc, cases, tmp_path):
    c = cases("bunny")
    hit = (c.tr["kind_hi"] == 2) & c.tr["unique"] & ~c.tr["edge"] & ~c.tr["uninformative"]
    k = int(np.bincount(c.tr["tri"][hit]).argmax())
    on_k = np.flatnonzero(hit & (c.tr["tri"] == k))
    tris = c.o.bvh(0)["tris"].copy()
    tris["vertex1"][k] = tris["vertex0"][k]; tris["vertex2"][k] = tris["vertex0"][k]     # gone, and every other triangle keeps its number
    o = rebuilt_oracle(orc, c.sc, 0, [tris])
    hits = o.find_nearest(c.O, c.D)
    bad = mt.rays_of(mt.nearest_violations(c.tr, hits))
    assert len(on_k) >= 1 and np.array_equal(bad, on_k), (k, on_k.tolist(), bad.tolist())


def test_rejects_the_determinant_threshold_ignored(crt, orc):
    p = B.mesh(crt, "cluster")
    w = mt.mesh_world(p)
    O, D, _ = mt.make_rays(w, 1024, seed=31)
    tr = mt.nearest_truth(w, O, D)
    free = mt.nearest_truth(w, O, D, a_min=0.0)                             # Moeller-Trumbore without `if (a > -0.0001f && a < 0.0001f) return`
    hits = np.zeros(len(O), crt.HIT_DTYPE)
    hits["t"] = np.where(np.isfinite(free["t_hi"]), free["t_hi"], 1e34); hits["objIdx"] = np.where(np.isfinite(free["t_hi"]), free["obj"], -1)
    hits["triIdx"], hits["u"], hits["v"] = free["tri"], free["u"], free["v"]
    differs = np.isfinite(free["mesh_hi"]) & (free["kind_hi"] == 2) & ~(tr["mesh_lo"] <= free["mesh_hi"] + 1e-4)
    bad = mt.rays_of(mt.nearest_violations(tr, hits))
    assert differs.sum() >= 200 and np.isin(np.flatnonzero(differs), bad).all()


def test_rejects_occlusion_bounded_by_the_rays_t(orc, cases):
    for scene in SCENES:
        c = cases(scene)
        hits = through(orc, c.o, WORLDS[c.kind][0]).find_nearest(c.O, c.D)
        assert len(mt.occluded_violations(c.occ[0], c.occ[1], c.o.is_occluded(c.O, c.D, c.t_shadow))) == 0
        behind = ~(c.tr["light"][1] < c.t_shadow * 1.5) & (c.tr["mesh_lo"] > c.t_shadow * 1.5)       # nothing on the segment, and no light: the bounded walk says 0
        doctored = (c.o.is_occluded(c.O, c.D, c.t_shadow) != 0) & ~behind
        beyond = np.isfinite(c.tr["mesh_hi"]) & behind
        bad = mt.occluded_violations(c.occ[0], c.occ[1], doctored)
        assert beyond.sum() >= 200 and np.isin(np.flatnonzero(beyond), bad).all(), scene


def test_rejects_normals_left_as_T_carries_them(orc, cases):
    c = cases("gen")                                                        # BLAS 1 and 2 stand under a T of scale 2
    hits = through(orc, c.o, "tlas").find_nearest(c.O, c.D)
    info = c.sh.hit_info(c.O, c.D, hits)
    assert not mt.hit_info_violations(c.tr, c.ti, hits, info)[0]
    raw = mt.hit_info_truth(c.world, c.O, c.D, c.tr, renormalise=False)
    scaled = c.ti["ok"] & (c.tr["kind"] == 2) & np.isin(c.tr["blas"], (1, 2)) & (hits["objIdx"] == c.tr["obj"]) & (hits["triIdx"] == c.tr["tri"])
    assert scaled.sum() >= 100 and np.allclose(np.linalg.norm(raw["N"][scaled], axis=1), 2.0, atol=1e-6)
    info["N"][scaled] = raw["N"][scaled]
    hv, _ = mt.hit_info_violations(c.tr, c.ti, hits, info)
    assert np.array_equal(hv.get("N", []), np.flatnonzero(scaled & c.ti["sure"]))


def test_rejects_normals_not_flipped(orc, cases):
    for scene in SCENES:
        c = cases(scene)
        hits = through(orc, c.o, WORLDS[c.kind][0]).find_nearest(c.O, c.D)
        info, flipped = c.sh.hit_info(c.O, c.D, hits, with_flip=True)
        info["N"][flipped] = -info["N"][flipped]
        m = flipped & c.ti["ok"] & c.ti["sure"] & (hits["objIdx"] == c.tr["obj"]) & ((c.tr["kind"] != 2) | (hits["triIdx"] == c.tr["tri"]))
        hv, _ = mt.hit_info_violations(c.tr, c.ti, hits, info)
        assert m.sum() >= 50 and np.array_equal(hv.get("N", []), np.flatnonzero(m)), scene     # (a closed mesh turns its normal only for a ray that starts inside)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the light quad of a look: turned, resized (light_quad_inputs.py; the kernels: tests/test_gpu_light_quad.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def quad_base(orc, scene):
    """the file look's light fields, as the library's HostScene.look() gives them (test_render_looks_cpu.py holds that equality)"""
    T = li.translate(np.asarray(orc.read_scene_xml(li.scene_path(li.SCENES[scene][0]))["light"], np.float32))
    return dict(light_T=T.reshape(16), light_invT=li.inverse_no_scale(T).reshape(16), light_size=0.5)


QUAD_CASES = [(s, n) for s in sorted(li.SCENES) for n in ("z25", "zyx", "y45", "quarter_z", "half_x", "zyx_size_0.9") + tuple("size_%g" % x for x in li.SIZES[s])]


@pytest.mark.parametrize("scene,name", QUAD_CASES)
def test_oracle_meets_the_criterion_under_a_quad_look(orc, scene, name):
    """the rays of light_quad_inputs meet the caps, and the oracle with set_light_quad meets the float64 truth on them: nearest hit, occlusion, the light's normal
    from both faces; GetLightPos is the restatement's; on the two quads of exact cells the float32 one-liner predicts the light's t bit for bit"""
    look = li.quad_looks(scene, quad_base(orc, scene))[name]
    xml, kind = li.SCENES[scene]
    o, sc = orc.load_scene(li.scene_path(xml), kind, ASSETS)
    o.set_light_quad(look["light_T"], look["light_invT"], look["light_size"])
    c = lq.Case(orc, scene, name, look, o)
    front, back = c.light_faces()
    assert front >= 100 and back >= 100, (front, back)
    for world in (("bvh", "grid") if kind == 0 else ("tlas", "tlas_grid")):
        hits = through(orc, o, world).find_nearest(c.O, c.D)
        viol = mt.nearest_violations(c.tr, hits)
        assert not viol, report("%s under %s through %s" % (scene, name, world), viol, c.O, c.D, hits, c.tr)
        bad = mt.occluded_violations(c.occ[0], c.occ[1], o.is_occluded(c.O, c.D, c.ts))
        assert len(bad) == 0, (scene, name, world, "is_occluded", bad[:8].tolist())
    through(orc, o, "bvh" if kind == 0 else "tlas")
    sh_cls = c.cls == lq.CLASSES.index("shadow")
    assert (c.occ[0] & sh_cls).sum() >= 40 and (~c.occ[1] & sh_cls).sum() >= 15         # the lengths just beyond / just short of the quad decide
    sh = hr.SceneShading(orc, o, sc, kind, ASSETS)
    full = dict(look, floor_texture=0, sky_texture=1, materials=[(m["reflectivity"], m["refractivity"], tuple(m["absorption"]), -1) for m in sc["materials"]])
    k = 2
    for i, m in enumerate(sc["materials"]):                                  # texture indices as the host scene numbers them
        if m["texture"]:
            full["materials"][i] = full["materials"][i][:3] + (k,); k += 1
    sh.set_look(full)
    info = sh.hit_info(c.O, c.D, hits)
    hv, n = mt.hit_info_violations(c.tr, c.ti, hits, info)
    assert n >= 0.7 * len(c.O) and not hv, (scene, name, {k: (len(v), v[:4].tolist()) for k, v in hv.items()})       # (a fifth of these rays are made to miss)
    q = o.light()
    assert np.array_equal(q["pos"].view(np.uint32), sh.light_pos().view(np.uint32)) and np.array_equal(q["normal"].view(np.uint32), sh.light_normal().view(np.uint32))
    T = np.asarray(look["light_T"], np.float32).reshape(4, 4)
    assert abs(float(q["pos"][1]) - (float(T[1, 3]) - 0.01)) < 1e-6 and np.abs(q["pos"][[0, 2]] - T[[0, 2], 3]).max() < 1e-6       # 0.01 down in WORLD y, whatever the normal
    if name in ("quarter_z", "half_x"):
        assert q["normal"].tolist() == {"quarter_z": [-1.0, 0.0, 0.0], "half_x": [0.0, 1.0, 0.0]}[name]
        cand, t = lq.axis_form(name, T, look["light_size"], c.O, c.D)
        lit = hits["objIdx"] == 0
        assert lit.sum() >= 300 and cand[lit].all() and np.array_equal(hits["t"][lit].view(np.uint32), t[lit].view(np.uint32))
        assert (hits["t"][cand & ~lit] < t[cand & ~lit]).all() and (hits["objIdx"][cand & ~lit] >= 1).all()     # something nearer
        eO, eD = lq.exact_rays(T, look["light_size"], 5)
        eh = o.find_nearest(eO, eD)
        assert not (eh["objIdx"] == 0).any() and not lq.axis_form(name, T, look["light_size"], eO, eD)[0].any()


def test_a_wrong_quad_is_rejected(orc):
    """the criterion has teeth on these rays: the oracle with the rotation transposed, with the size ignored, and with the un-turned quad breaks it.  (y45 is
    not asked to tell R from its transpose: a square turned by +45 and by -45 degrees about its normal is one square; and half_x, the square turned face up onto itself, is
    told from the un-turned quad by nothing a query returns, GetHitInfo's normal being turned towards the ray: it is there for the general form with exact cells.)"""
    scene = "cube"; xml, kind = li.SCENES[scene]
    looks = li.quad_looks(scene, quad_base(orc, scene))
    o, _ = orc.load_scene(li.scene_path(xml), kind, ASSETS)
    for name, wrong in (("zyx", "transposed"), ("z25", "transposed"), ("y45", "unturned"), ("size_0.9", "size"), ("size_0.03125", "size"), ("quarter_z", "unturned")):
        look = looks[name]
        c = lq.Case(orc, scene, name, look, o)
        T = np.asarray(look["light_T"], np.float32).reshape(4, 4).copy(); size = look["light_size"]
        if wrong == "transposed":
            T[:3, :3] = T[:3, :3].T.copy()
        elif wrong == "size":
            size = 0.5
        elif wrong == "unturned":
            T[:3, :3] = np.eye(3)
        o.set_light_quad(T, li.inverse_no_scale(T), size)
        hits = o.find_nearest(c.O, c.D)
        n = mt.count(mt.nearest_violations(c.tr, hits))
        assert n >= 50, (name, wrong, n)
