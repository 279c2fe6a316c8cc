"""TLASFileScene built with TLAS_USE_KDTree / TLAS_USE_Grid (tlas_file_scene.cpp:40-90) on the GPU: TLASKDTree over BLASKDTree and TLASGrid over BLASGrid,
uploaded with crt_upload_blas_accel.  Every query record is compared field for field with the CPU restatement (tests/tlas_alt_restate.py), Ray::traversed and
Ray::tested included, and at size (2^16 rays) with the C++ oracle's two-level walk (orc.set_blas_accel, pinned to the restatement by tests/test_tlas_alt_cpu.py).
Renders and Whitted frames are compared with the oracle through the same structure, over frame counts at which that differs from the oracle's TLAS-BVH render,
and (test_render_and_whitted_equal_the_oracle) with the TLAS-BVH render itself on a camera whose paths meet no ray on which the structures disagree."""
import numpy as np
import pytest
import torch

from conftest import ASSETS, scene_path
from test_gpu_scene_queries import light_of, quad_occluded, pick_t, ray_records, shadow_records, hits_np, tlas_up_rays
from test_tlas_alt_cpu import second_scene
import alt_disagreement as ad
import tlas_alt_restate as R

pytestmark = pytest.mark.gpu
KINDS = [("kd", 1), ("grid", 2)]
FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")


def assert_records(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f, int((got[f].view(np.uint32) != want[f].view(np.uint32)).sum()))


def setup(crt, orc, xml, code, W=64, H=64):
    hs = crt.HostScene(xml, 1, ASSETS)
    hs.build_alt(code)
    ctx = crt.Context(W, H)
    hs.upload(ctx); hs.upload_alt(ctx, code)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    return hs, ctx, o


@pytest.fixture(params=["tlas", "second"])
def scene_xml(request, tmp_path):
    return scene_path("tlas_scene.xml") if request.param == "tlas" else second_scene(tmp_path)


@pytest.mark.parametrize("kind,code", KINDS)
def test_queries_equal_the_restatement(crt, orc, scene_xml, kind, code):
    hs, ctx, o = setup(crt, orc, scene_xml, code)
    light = light_of(scene_xml)
    O, D = R.query_rays(o, light)
    sc = R.Scene(orc, o, kind, light)
    want = sc.find_nearest_many(O, D, crt.HIT_DTYPE)
    # what the ray set covers: floor first, several instances, origins inside objects, axis-parallel components, the light
    assert (want["objIdx"] == 1).sum() > 100 and (want["objIdx"] >= 2).sum() > 300 and (want["objIdx"] == 0).sum() > 5
    assert len(set(want["objIdx"][want["objIdx"] >= 2])) == hs.bvh_count()
    assert (D == 0).any(axis=1).sum() >= 150
    got = ctx.find_nearest_alt(code, O, D)
    assert_records(got, want, "host entry")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dh = ctx.find_nearest_device(ray_records(O, D), accel=code)
    side.synchronize()
    assert_records(hits_np(crt, dh), want, "device entry")
    # on general rays the same nearest hits as the TLAS-BVH path
    general = np.all(D != 0, axis=1)
    hb = ctx.find_nearest(O, D)
    for f in ("t", "u", "v", "objIdx", "triIdx"):
        assert np.array_equal(got[f][general].view(np.uint32), hb[f][general].view(np.uint32)), f
    # and the occlusion query
    _, tq = quad_occluded(O, D, np.full(len(O), 1e34, np.float32), light)
    t = pick_t(tq)
    occ = sc.is_occluded_many(O, D, t)
    assert 0 < occ.sum() < len(occ)
    assert np.array_equal(ctx.is_occluded(O, D, t, accel=code), occ)
    assert np.array_equal(ctx.is_occluded_device(shadow_records(O, D, t), accel=code).cpu().numpy(), occ)
    ctx.close(); hs.close()


@pytest.mark.parametrize("kind,code", KINDS)
def test_occlusion_towards_the_light(crt, orc, kind, code):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    hs, ctx, o = setup(crt, orc, xml, code)
    O, D = tlas_up_rays(hs, light, n=1500)
    _, tq = quad_occluded(O, D, np.full(len(O), 1e34, np.float32), light)
    t = pick_t(tq)
    want = R.Scene(orc, o, kind, light).is_occluded_many(O, D, t)
    assert np.array_equal(ctx.is_occluded(O, D, t, accel=code), want)
    assert np.array_equal(ctx.is_occluded(O, D, t), want)                # IsOccluded's answer is the BVH variant's
    ctx.close(); hs.close()


# The three structures of tlas_scene.xml do not return the same nearest hit for every ray (test_tlas_alt_cpu.py::test_real_disagreements_between_the_structures),
# and one such ray shifts the random-number stream of the rest of its tile, so an image comparison with the TLAS-BVH render needs paths that meet none: over
# 5 frames this camera (near the wok, looking past it to the torii gate) meets none, and neither does the default camera of the bunny + cube scene over 70 frames
# x 2 passes.  That the images come from the KD-tree / grid path and not the BVH one is told by the statistics counters: the sequential Sample loop and the
# Whitted kernel count no TLAS steps through a BLAS set, the BVH path does.
CAMERA = ((-0.8, 0.2, 2.0), (-1.6, -0.7, 3.0))


@pytest.mark.parametrize("kind,code", KINDS)
def test_render_and_whitted_equal_the_oracle(crt, orc, tmp_path, kind, code):
    W, H = 96, 64
    for xml, cam, frames, passes in ((scene_path("tlas_scene.xml"), CAMERA, 5, 1), (second_scene(tmp_path), None, 5, 1), (second_scene(tmp_path), None, 70, 2)):
        hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(code)
        ctx = crt.Context(W, H, collect_stats=True); hs.upload(ctx); hs.upload_alt(ctx, code)
        o, _ = orc.load_scene(xml, 1, ASSETS)
        o.renderer_init(W, H); o.set_params(5, passes)
        if cam:
            ctx.set_camera_state(*cam); o.set_camera_state(*cam)
        ctx.set_render_accel(code)
        ctx.render(1, frames, passes); o.render(frames, 8)
        assert np.array_equal(ctx.accumulator(), o.accumulator()), (xml, frames)
        c = ctx.counters()
        assert c["rays"] == o.counters()["rays"] and c["mesh_hits"] > 2000 * frames * passes // 5
        assert c["tlas_iters"] == 0 and c["interior_iters"] == 0, c                # the sequential loop through the BLAS set ran, not the BVH path
        ctx.reset_counters()
        px = ctx.whitted_tick(); o.whitted(8)
        assert np.array_equal(ctx.accumulator(), o.accumulator()) and np.array_equal(px, o.screen())
        assert ctx.counters()["tlas_iters"] == 0
        # the same calls through the BVH path do count TLAS steps (what the two assertions above tell apart)
        ctx.set_render_accel(0); ctx.reset_counters(); ctx.clear()
        ctx.render(1, 1, passes)
        assert ctx.counters()["tlas_iters"] > 0
        ctx.reset_counters(); ctx.whitted_tick()
        assert ctx.counters()["tlas_iters"] > 0
        ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Against the oracle THROUGH THE SAME STRUCTURE (orc.set_blas_accel), on frames where that is not the TLAS-BVH answer
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# (kind, scene state, passes) -> (frames, differing tiles): at 96 x 64 with tlas_scene.xml's default camera, the smallest frame count for which the oracle's
# accumulator through the structure differs from the oracle's accumulator through the TLAS-BVH, and in how many 16 x 16 tiles it then differs.  Found with the
# oracle; the test asserts both numbers on the oracle's two images (one frame fewer: no tile differs), so a comparison that says nothing new cannot pass unnoticed.
# "moved": instance 2 (the teapot) rotated and shifted, as in test_instance_motion_keeps_the_set.
STRUCTURE_FRAMES = {("kd", "built", 1): (2, 1), ("kd", "built", 2): (3, 1), ("kd", "moved", 1): (9, 1),
                    ("grid", "built", 1): (20, 1), ("grid", "built", 2): (24, 1), ("grid", "moved", 1): (20, 1)}
RW, RH = 96, 64


def differing_tiles(a, b):
    d = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    return int(d.reshape(RH // 16, 16, RW // 16, 16).any(axis=(1, 3)).sum())


def moved_transform(T):
    T = T.reshape(4, 4).copy()
    c, s = np.float32(np.cos(np.float32(0.7))), np.float32(np.sin(np.float32(0.7)))
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[:3, 3] += np.array([-0.4, 0.1, 0.3], np.float32)
    return T


def structure_context(crt, xml, code):
    hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(code)
    ctx = crt.Context(RW, RH, collect_stats=True); hs.upload(ctx); hs.upload_alt(ctx, code)
    ctx.set_render_accel(code)
    return hs, ctx


def render_and_whitted_against(ctx, a, b, frames, tiles, passes, what):
    """crt_render x frames and one Whitted Tick of `ctx` against oracle `a` (through the structure); `b` (through the TLAS-BVH) only states the premise"""
    for o in (a, b):
        o.set_params(5, passes); o.clear(); o.reset_counters()
        o.render(frames - 1, 8)
    assert differing_tiles(a.accumulator(), b.accumulator()) == 0, what     # `frames` is the smallest such count
    a.render(1, 8); b.render(1, 8)
    assert differing_tiles(a.accumulator(), b.accumulator()) == tiles >= 1, what
    ctx.clear(); ctx.reset_counters()
    ctx.render(1, frames, passes)
    assert np.array_equal(ctx.accumulator().view(np.uint32), a.accumulator().view(np.uint32)), what
    c, oc = ctx.counters(), a.counters()
    assert c["rays"] == oc["rays"] and c["mesh_hits"] == oc["mesh_hits"] and c["tlas_iters"] == 0, (what, c, oc)
    ctx.reset_counters()
    px = ctx.whitted_tick(); a.whitted(8)                                   # its shadow rays take the ANY form of the walk
    assert np.array_equal(px, a.screen()) and np.array_equal(ctx.accumulator().view(np.uint32), a.accumulator().view(np.uint32)), what
    assert ctx.counters()["tlas_iters"] == 0


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("kind,code", KINDS)
def test_render_through_the_structure_equals_the_oracle_through_it(crt, orc, kind, code, passes):
    xml = scene_path("tlas_scene.xml")
    b, a = ad.scene_pair(orc, xml, ASSETS, kind)
    for o in (a, b):
        o.renderer_init(RW, RH)
    hs, ctx = structure_context(crt, xml, code)
    render_and_whitted_against(ctx, a, b, *STRUCTURE_FRAMES[(kind, "built", passes)], passes, (kind, "built", passes))
    if passes == 1:
        # one instance moves: set_transform + UPDATE_TRANSFORMS keeps the uploaded set (invT is read per query), and so does the device route with the same matrices
        T = moved_transform(hs.blas_transform(2)[0])
        hs.set_transform(2, T); a.set_transform(2, T); b.set_transform(2, T)
        hs.update(ctx, crt.UPDATE_TRANSFORMS)
        frames, tiles = STRUCTURE_FRAMES[(kind, "moved", 1)]
        render_and_whitted_against(ctx, a, b, frames, tiles, 1, (kind, "set_transform + UPDATE_TRANSFORMS"))
        hs2, ctx2 = structure_context(crt, xml, code)
        allT = np.stack([hs.blas_transform(i)[0].reshape(16) for i in range(hs.bvh_count())]).astype(np.float32)
        ctx2.update_transforms_device(torch.from_numpy(allT).cuda())
        render_and_whitted_against(ctx2, a, b, frames, tiles, 1, (kind, "update_transforms_device"))
        ctx2.close(); hs2.close()
    ctx.close(); hs.close()


@pytest.mark.parametrize("kind,code", KINDS)
def test_queries_at_size_equal_the_oracle(crt, orc, kind, code):
    """2^16 rays of R.query_rays plus the committed rays on which the structures disagree: a launch of many workgroups (2 000 rays are a workgroup per 64 rays),
    both FindNearest entries and both occlusion entries against the C++ oracle's two-level walk, all seven fields as bits"""
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    hs, ctx, o = setup(crt, orc, xml, code)
    orc.set_blas_accel(o, orc.blas_accels(o, kind))
    O, D = R.query_rays(o, light, n=65536)
    Oa, Da, _, _, _ = ad.load(kind)
    at = np.linspace(0, len(O), len(Oa), endpoint=False).astype(np.int64)   # spread through the launch
    O = np.insert(O, at, Oa, axis=0); D = np.insert(D, at, Da, axis=0)
    want = o.find_nearest(O, D)
    assert (want["objIdx"] == 1).sum() > 3000 and (want["objIdx"] >= 2).sum() > 10000 and (want["objIdx"] == 0).sum() > 100 and (D == 0).any(axis=1).sum() > 5000
    assert_records(ctx.find_nearest_alt(code, O, D), want, "host entry")
    assert_records(hits_np(crt, ctx.find_nearest_device(ray_records(O, D), accel=code)), want, "device entry")
    _, tq = quad_occluded(O, D, np.full(len(O), 1e34, np.float32), light)
    t = pick_t(tq)
    occ = o.is_occluded(O, D, t)
    assert 1000 < occ.sum() < len(occ) - 1000
    assert np.array_equal(ctx.is_occluded(O, D, t, accel=code), occ != 0)
    assert np.array_equal(ctx.is_occluded_device(shadow_records(O, D, t), accel=code).cpu().numpy(), occ)
    ctx.close(); hs.close()


@pytest.mark.parametrize("kind,code", KINDS)
def test_instance_motion_keeps_the_set(crt, orc, kind, code):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    W, H = 96, 64
    hs, ctx, o = setup(crt, orc, xml, code, W, H)
    o.renderer_init(W, H)
    T = hs.blas_transform(2)[0].reshape(4, 4).copy()
    c, s = np.float32(np.cos(np.float32(0.7))), np.float32(np.sin(np.float32(0.7)))
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    T[:3, 3] += np.array([-0.4, 0.1, 0.3], np.float32)
    hs.set_transform(2, T); o.set_transform(2, T)
    hs.update(ctx, crt.UPDATE_TRANSFORMS)
    O, D = R.query_rays(o, light, 800, seed=9)
    assert_records(ctx.find_nearest_alt(code, O, D), R.Scene(orc, o, kind, light).find_nearest_many(O, D, crt.HIT_DTYPE), "moved")
    ctx.set_camera_state(*CAMERA); o.set_camera_state(*CAMERA)
    ctx.set_render_accel(code)
    ctx.render(1, 3, 1); o.render(3, 8)
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    ctx.close(); hs.close()


@pytest.mark.parametrize("kind,code", KINDS)
def test_refit_drops_the_set(crt, orc, kind, code):
    xml = scene_path("tlas_scene.xml")
    W, H = 96, 64
    hs, ctx, o = setup(crt, orc, xml, code, W, H)
    o.renderer_init(W, H)
    ctx.set_render_accel(code)
    tris = hs.bvh(0)["tris"]
    pos = np.stack([tris["vertex0"], tris["vertex1"], tris["vertex2"]], 1).astype(np.float32) * np.float32(1.01)
    hs.move_and_refit(0, pos); o.move_and_refit(0, pos)
    hs.update(ctx, crt.UPDATE_BOUNDS)
    with pytest.raises(crt.CrtError) as e:
        ctx.find_nearest_alt(code, np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32))
    assert e.value.code == -5
    with pytest.raises(crt.CrtError):
        ctx.set_render_accel(code)
    ctx.render(1, 3, 1); o.render(3, 8)                                   # back on the BVH
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    ctx.close(); hs.close()


def test_upload_refusals_leave_the_set_answering(crt, orc, tmp_path):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    hs = crt.HostScene(xml, 1, ASSETS)
    structs = hs.build_alt(crt.ACCEL_KDTREE)
    tris = [hs.bvh(i)["tris"] for i in range(hs.bvh_count())]
    ctx = crt.Context(64, 64)
    with pytest.raises(crt.CrtError) as e:
        ctx.upload_blas_accel(crt.ACCEL_KDTREE, structs, tris)            # no scene yet
    assert e.value.code == -5
    fs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    fctx = crt.Context(64, 64); fs.upload(fctx)
    with pytest.raises(crt.CrtError) as e:
        fctx.upload_blas_accel(crt.ACCEL_KDTREE, structs, tris)           # a FILE scene
    assert e.value.code == -5
    fctx.close(); fs.close()
    hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    O, D = R.query_rays(o, light, 300, seed=13)
    before = ctx.find_nearest_alt(crt.ACCEL_KDTREE, O, D)
    bad = []
    bad.append(("blasCount", crt.ACCEL_KDTREE, structs[:-1], tris[:-1], -1))
    bad.append(("kind", crt.ACCEL_GRID, structs, tris, -1))
    t2 = [t.copy() for t in tris]; t2[1]["objIdx"] += 1
    bad.append(("objIdx", crt.ACCEL_KDTREE, structs, t2, -1))
    s2 = [dict(s) for s in structs]; s2[0]["nodes"] = s2[0]["nodes"].copy(); s2[0]["nodes"][0]["aabbMax"][1] = np.nextafter(s2[0]["nodes"][0]["aabbMax"][1], np.float32(np.inf))
    bad.append(("root box", crt.ACCEL_KDTREE, s2, tris, -1))
    for what, kind, st, tr, code in bad:
        with pytest.raises(crt.CrtError) as e:
            if what == "kind":                                             # a set of kind grid whose structures are KD-trees
                arr = (crt.AltAccelS * len(st))(*[crt.alt_desc(crt.ACCEL_KDTREE, t, s) for t, s in zip(tr, st)])
                ctx._ck(ctx.L.crt_upload_blas_accel(ctx.h, kind, arr, len(st)))
            else:
                ctx.upload_blas_accel(kind, st, tr)
        assert e.value.code == code, what
        assert_records(ctx.find_nearest_alt(crt.ACCEL_KDTREE, O, D), before, what)
    ctx.close(); hs.close()


def test_tick_sequence_equals_render_readback_resolve(crt):
    W, H = 96, 64
    xml = scene_path("tlas_scene.xml")
    out = []
    for use_tick in (True, False):
        hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
        ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE); ctx.set_render_accel(crt.ACCEL_KDTREE)
        res = []
        for spp in range(1, 6):
            if use_tick:
                res.append(ctx.tick(spp, 1))
            else:
                ctx.render(spp, 1, 1)
                acc = ctx.accumulator()
                px, e = ctx.resolve_screen(1.0 / (spp + 1))
                res.append((px, acc, e))
        out.append(res)
        ctx.close(); hs.close()
    for a, b in zip(*out):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
