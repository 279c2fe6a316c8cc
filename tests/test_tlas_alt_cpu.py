"""TLASFileScene built with TLAS_USE_KDTree / TLAS_USE_Grid (tlas_file_scene.cpp:40-90) on the host front, without a GPU: the per-BLAS structures equal the
oracle's builds over the same triangle arrays, their root boxes are the BVH root boxes (so the shared TLAS is the variant's own), and the CPU restatement the GPU
tests compare with (tests/tlas_alt_restate.py) agrees with the oracle's TLAS-BVH where the structures agree, the oracle's own two-level walk (orc.set_blas_accel)
equals that restatement bit for bit, and the committed rays on which the structures disagree (tests/golden/alt_disagreement_rays.npz) still do."""
import os

import numpy as np
import pytest

from conftest import ASSETS, scene_path
from test_gpu_golden_and_edges import write_scene
from test_gpu_scene_queries import light_of, quad_occluded, pick_t, tlas_up_rays
import alt_disagreement as ad
import sample_query_inputs as si
import tlas_alt_restate as R

KINDS = [("kd", 1), ("grid", 2)]


def second_scene(tmp_path):
    """bunny + cube, rotated, non-uniformly scaled"""
    return write_scene(tmp_path, "bunny", name="tlas2.xml", pos=(-0.6, -1.0, 2.5), rot=(10.0, 140.0, 0.0), scale=(1.1, 0.8, 1.3),
                       extra_objects=[("cube", 0, (0.9, -0.7, 2.2), (0.0, 35.0, 20.0), (0.5, 0.3, 0.7))])


@pytest.fixture(params=["tlas", "second"])
def scene_xml(request, tmp_path):
    return scene_path("tlas_scene.xml") if request.param == "tlas" else second_scene(tmp_path)


@pytest.mark.parametrize("kind,code", KINDS)
def test_blas_structures_equal_the_oracle_builds(crt, orc, scene_xml, kind, code):
    hs = crt.HostScene(scene_xml, 1, ASSETS)
    got = hs.build_alt(code)
    o, _ = orc.load_scene(scene_xml, 1, ASSETS)
    assert len(got) == hs.bvh_count() == o.bvh_count() >= 2
    for i in range(hs.bvh_count()):
        tris = o.bvh(i)["tris"]
        assert hs.bvh(i)["tris"].tobytes() == tris.tobytes()
        a = orc.alt_accel(kind, tris); want = a.dump(); a.close()
        assert got[i].keys() == want.keys()
        for k in want:
            assert np.asarray(got[i][k]).tobytes() == np.asarray(want[k]).tobytes(), (i, k)
        assert hs.blas_alt(code, i)["refs"].tobytes() == got[i]["refs"].tobytes()
    hs.close()


@pytest.mark.parametrize("kind,code", KINDS)
def test_root_boxes_are_the_bvh_root_boxes(crt, scene_xml, kind, code):
    hs = crt.HostScene(scene_xml, 1, ASSETS)
    for i, s in enumerate(hs.build_alt(code)):
        root = hs.bvh(i)["nodes"][0]
        lo, hi = (s["nodes"][0]["aabbMin"], s["nodes"][0]["aabbMax"]) if kind == "kd" else (s["boundsMin"], s["boundsMax"])
        assert lo.tobytes() == root["aabbMin"].tobytes() and hi.tobytes() == root["aabbMax"].tobytes(), i
    hs.close()


def test_host_front_refusals(crt, tmp_path):
    hs = crt.HostScene(scene_path("tlas_scene.xml"), 1, ASSETS)
    with pytest.raises(crt.CrtError):
        hs.blas_alt(crt.ACCEL_KDTREE, 0)                                  # not built yet
    hs.build_alt(crt.ACCEL_KDTREE)
    for i in (-1, hs.bvh_count()):
        with pytest.raises(crt.CrtError):
            hs.blas_alt(crt.ACCEL_KDTREE, i)
    with pytest.raises(crt.CrtError):
        hs.build_alt(7)
    hs.close()


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_restatement_agrees_with_the_oracle_tlas_bvh(crt, orc, kind):
    """on rays without zero direction components, the three structures give the same nearest hit: the restatement's (t, u, v, objIdx, triIdx) is the oracle's
    TLAS-BVH FindNearest, bit for bit"""
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    O, D = R.query_rays(o, light, 400, seed=21)
    general = np.all(D != 0, axis=1)
    O, D = O[general], D[general]
    sc = R.Scene(orc, o, kind, light)
    got = sc.find_nearest_many(O, D, crt.HIT_DTYPE)
    want = o.find_nearest(O, D)
    assert (want["objIdx"] >= 2).sum() > 50 and (want["objIdx"] == 1).sum() > 20
    for f in ("t", "u", "v", "objIdx", "triIdx"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_restatement_counters_on_one_instance(crt, orc, tmp_path, kind):
    """one instance (TLAS root = leaf): for rays that hit neither light nor floor, traversed = 1 TLAS step + the standalone structure's count on the
    object-space ray, and tested is the standalone structure's"""
    xml = write_scene(tmp_path, "bunny", name="one.xml", pos=(0.3, -0.8, 2.0), rot=(0.0, 150.0, 0.0), scale=(1.2, 0.9, 1.0))
    light = light_of(xml)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    sc = R.Scene(orc, o, kind, light)
    O, D = R.query_rays(o, light, 400, seed=4)
    keep = []
    with np.errstate(all="ignore"):
        for i in range(len(O)):
            r = R.Ray(O[i], D[i]); sc.light_intersect(r); sc.floor_intersect(r)
            keep.append(r.objIdx == -1)
    keep = np.array(keep)
    O, D = O[keep], D[keep]
    got = sc.find_nearest_many(O, D, crt.HIT_DTYPE)
    assert (got["objIdx"] == 2).sum() > 30 and (got["objIdx"] == -1).sum() > 30
    with np.errstate(all="ignore"):
        obj = [sc.blas[0].object_ray(R.Ray(O[i], D[i])) for i in range(len(O))]
    Oo = np.array([[float(x) for x in r.O] for r in obj], np.float32); Do = np.array([[float(x) for x in r.D] for r in obj], np.float32)
    a = orc.alt_accel(kind, o.bvh(0)["tris"]); w = a.intersect(Oo, Do); a.close()
    assert np.array_equal(got["traversed"], w["traversed"] + 1)
    assert np.array_equal(got["tested"], w["tested"])
    for f in ("t", "u", "v", "triIdx"):
        assert np.array_equal(got[f].view(np.uint32), w[f].view(np.uint32)), f


def test_ray_set_tells_rule_1_apart(crt, orc):
    """the GPU tests' ray set holds rays whose `traversed` differs between BLASKDTree's early return (rule 1) and FileScene's KD-tree rule"""
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    O, D = R.query_rays(o, light)                                         # the set of test_gpu_tlas_alt.py on this scene
    sc = R.Scene(orc, o, "kd", light)
    a = sc.find_nearest_many(O, D, crt.HIT_DTYPE, rule1=True)
    b = sc.find_nearest_many(O, D, crt.HIT_DTYPE, rule1=False)
    assert (a["traversed"] != b["traversed"]).sum() >= 10


def test_real_disagreements_between_the_structures(crt, orc):
    """Rays from the default camera on which the three structures of tlas_scene.xml disagree (tools/query_tlas_alt.py counts such rays), restated here: the
    KD-tree loses the teapot's nearest hit (its `t < tmin + 0.001` / `t > tmax - 0.001` tests skip a child, kdtree.cpp:163-201); KD-tree and grid find the torii
    gate's foot a float step before the floor, where the BVH's box test (tlas_bvh.cpp:72-81) has already culled it.  Image comparisons with the TLAS-BVH render
    (test_gpu_tlas_alt.py) use a camera whose paths meet no such ray."""
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    O = np.zeros((2, 3), np.float32); O[:, 2] = -2
    D = np.array([[0.05717528611421585, -0.15218958258628845, 0.986696183681488], [0.32969576120376587, -0.2006836086511612, 0.9225110411643982]], np.float32)
    bvh = o.find_nearest(O, D)
    kd = R.Scene(orc, o, "kd", light).find_nearest_many(O, D, crt.HIT_DTYPE)
    grid = R.Scene(orc, o, "grid", light).find_nearest_many(O, D, crt.HIT_DTYPE)
    assert bvh["objIdx"][0] == 1 and kd["objIdx"][0] == grid["objIdx"][0] == 3 and kd["t"][0] < bvh["t"][0] and grid["t"][0] == kd["t"][0]
    assert bvh["objIdx"][1] == grid["objIdx"][1] == 4 and bvh["t"][1] == grid["t"][1] and kd["t"][1] > bvh["t"][1]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The C++ oracle's two-level walk (orc.set_blas_accel) against the numpy restatement: two independent restatements of tlas_kdtree.cpp / blas_kdtree.cpp /
# blas_grid.cpp, written at different times in different languages.  This is what pins the oracle the GPU's Sample, render and Whitted tests compare with.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")


def assert_fields(got, want, what, fields=FIELDS):
    for f in fields:
        a, b = got[f].view(np.uint32), want[f].view(np.uint32)
        assert np.array_equal(a, b), (what, f, int((a != b).sum()))


def two_level(orc, o, kind):
    orc.set_blas_accel(o, orc.blas_accels(o, kind))
    return o


def moved(T):
    """the instance motion of test_gpu_tlas_alt.py::test_instance_motion_keeps_the_set: the instance rotated about y by 0.7 and shifted"""
    T = T.reshape(4, 4).copy()
    c, s = np.float32(np.cos(np.float32(0.7))), np.float32(np.sin(np.float32(0.7)))
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[:3, 3] += np.array([-0.4, 0.1, 0.3], np.float32)
    return T


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_oracle_two_level_walk_equals_the_restatement(crt, orc, scene_xml, kind):
    """all seven fields, as bits, on the 2 000 rays of R.query_rays (zero direction components, origins inside instances and floor-first rays included), and
    IsOccluded; then again after one instance moved — the installed set survives orc_set_blas_transform because invT is read per query"""
    light = light_of(scene_xml)
    o, _ = orc.load_scene(scene_xml, 1, ASSETS)
    plain, _ = orc.load_scene(scene_xml, 1, ASSETS)                        # the TLAS-BVH scene: what the walk must NOT be confused with
    two_level(orc, o, kind)
    hs = crt.HostScene(scene_xml, 1, ASSETS)
    for step in ("built", "moved"):
        if step == "moved":
            i = o.bvh_count() - 1
            T = moved(o.blas_transform(i)[0])
            o.set_transform(i, T); plain.set_transform(i, T); hs.set_transform(i, T)
        O, D = R.query_rays(o, light)
        sc = R.Scene(orc, o, kind, light)
        want = sc.find_nearest_many(O, D, crt.HIT_DTYPE)
        got = o.find_nearest(O, D)
        assert (want["objIdx"] >= 2).sum() > 300 and (want["objIdx"] == 1).sum() > 100
        assert_fields(got, want, (kind, step))
        bvh = plain.find_nearest(O, D)
        assert (got["traversed"] != bvh["traversed"]).mean() > 0.5          # the set is walked, not the BVH
        Ou, Du = tlas_up_rays(hs, light, n=1500)
        _, tq = quad_occluded(Ou, Du, np.full(len(Ou), 1e34, np.float32), light)
        t = pick_t(tq)
        occ = sc.is_occluded_many(Ou, Du, t)
        assert 0 < occ.sum() < len(occ)
        assert np.array_equal(o.is_occluded(Ou, Du, t), occ), (kind, step)
    hs.close()


def test_oracle_set_blas_accel_refusals_and_reset(orc):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    O, D = R.query_rays(o, light, 400, seed=2)
    bvh = o.find_nearest(O, D)
    acc = orc.blas_accels(o, "kd")
    with pytest.raises(RuntimeError):
        orc.set_blas_accel(o, acc[:-1])                                     # n must equal orc_bvh_count
    with pytest.raises(RuntimeError):
        orc.set_blas_accel(o, acc[1:] + acc[:1])                            # structures over other triangle arrays
    f, _ = orc.load_scene(scene_path("bunny_scene.xml"), 0, ASSETS)
    with pytest.raises(RuntimeError):
        orc.set_blas_accel(f, orc.blas_accels(f, "kd"))                     # a FileScene
    with pytest.raises(RuntimeError):
        orc.set_render_accel(o, acc[0])                                     # and orc_set_render_accel keeps refusing a two-level scene
    assert_fields(o.find_nearest(O, D), bvh, "refused calls leave the BVH answering")
    orc.set_blas_accel(o, acc)
    kd = o.find_nearest(O, D)
    assert not np.array_equal(kd["traversed"], bvh["traversed"])
    orc.set_blas_accel(o, None)                                             # kind 0 restores the TLAS-BVH
    assert_fields(o.find_nearest(O, D), bvh, "kind 0")
    orc.set_blas_accel(o, acc)
    tris = o.bvh(0)["tris"]
    pos = np.stack([tris["vertex0"], tris["vertex1"], tris["vertex2"]], 1).astype(np.float32) * np.float32(1.01)
    o.move_and_refit(0, pos)                                                # drops the set, as the product does
    p, _ = orc.load_scene(xml, 1, ASSETS); p.move_and_refit(0, pos)
    assert_fields(o.find_nearest(O, D), p.find_nearest(O, D), "refit")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The committed rays on which the structures disagree (tests/golden/alt_disagreement_rays.npz, tests/alt_disagreement.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_disagreement_rays_still_disagree(orc, kind):
    """re-derived from the oracle alone on every run: every committed ray's two-level record differs from the TLAS-BVH record, at least 100 rays per kind drawn
    the three ways a path produces rays, none with a zero direction component, a non-zero seed each; for the KD-tree at least 20 rays on which it loses the BVH's
    hit and 20 on which it finds a hit the BVH culled"""
    b, a = ad.scene_pair(orc, scene_path("tlas_scene.xml"), ASSETS, kind)
    O, D, inside, seeds, cls = ad.load(kind)
    counts = ad.check(kind, O, D, inside, seeds, cls, b.find_nearest(O, D, inside), a.find_nearest(O, D, inside))
    assert counts["rays"] == 180                                           # the counts DESIGN §6 records
    assert (counts["lost"], counts["found"]) == ((90, 90) if kind == "kd" else (0, 180))
    # and a path through them is a different path: Sample through the structure and through the BVH part ways on most of them
    rgb_b, s_b, _ = si.oracle_sample(b, O, D, inside, seeds)
    rgb_a, s_a, _ = si.oracle_sample(a, O, D, inside, seeds)
    assert (s_a != s_b).sum() >= 50, int((s_a != s_b).sum())


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_oracle_equals_the_restatement_on_the_disagreement_rays(crt, orc, kind):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    b, a = ad.scene_pair(orc, xml, ASSETS, kind)
    O, D, inside, _, _ = ad.load(kind)
    want = R.Scene(orc, a, kind, light).find_nearest_many(O, D, crt.HIT_DTYPE)
    assert_fields(a.find_nearest(O, D, inside), want, kind)
    if kind == "kd":                                                       # without rule 1's objIdx condition the walk is another walk on these rays
        other = R.Scene(orc, a, kind, light).find_nearest_many(O, D, crt.HIT_DTYPE, rule1=False)
        assert (other["traversed"] != want["traversed"]).sum() >= 10
