"""crt_update_look: the live scene's look — materials, floor texture, skydome, light quad — changed in place.  After the call every entry that shades must give bit
for bit what a FRESH context gives that uploaded the scene's description with that look (HostScene.set_look + upload, followed by the same alternative-accelerator
uploads), and what the oracle gives for a scene built with that look (render_looks_inputs.make_oracle).  The looks are
tests/render_looks_inputs.py's; tests/test_render_looks_cpu.py holds, without a GPU, that each of them changes the image."""
import ctypes as C

import numpy as np
import pytest

import render_looks_inputs as li
from conftest import ASSETS, scene_path
from test_gpu_render_looks import Rig, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = li.W, li.H
INVALID, UNSUPPORTED, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def rigs(crt, orc):
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = Rig(crt, orc, scene)
        return cache[scene]
    yield get
    for r in cache.values():
        r.close()


def one(scene, name, frames=3):
    return li.Case(scene, [name], None, 1, frames, 1)


def primary(ctx_w, ctx_h, orc_scene, camera):
    """the primary rays through every fourth pixel centre"""
    orc_scene.set_camera_state(*camera)
    xs, ys = np.meshgrid(np.arange(0, ctx_w, 4, dtype=np.float32) + 0.5, np.arange(0, ctx_h, 4, dtype=np.float32) + 0.5)
    return orc_scene.primary_rays(np.stack([xs.ravel(), ys.ravel()], axis=1))


# 1: crt_render (a small launch: render_tiles_kernel) after every look, against the fresh upload and the oracle
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_render_after_every_look(rigs, scene):
    r = rigs(scene)
    cam = li.CAMERAS[scene]
    base = r.fresh_loop(one(scene, "base"))[0]
    for name in r.looks:
        c = one(scene, name)
        r.ctx.update_look(r.rec[name])
        r.ctx.set_camera_state(*cam); r.ctx.clear(); r.ctx.render(c.spp_first, c.frames, c.passes)
        got = r.ctx.accumulator()
        assert same(got, r.fresh_loop(c)[0]), (scene, name, "fresh upload")
        for a in r.oracle_views(c).values():
            assert same(got, a), (scene, name, "oracle")
        assert same(got, base) == (name == "base"), (scene, name)            # every look changes the image
    r.ctx.update_look(r.rec["base"])


# 2: a job routed to the pool kernel
@pytest.mark.parametrize("scene,name", [("cube", "all"), ("tlas", "all"), ("tlas", "glass")])
def test_pool_kernel_after_a_look(crt, orc, monkeypatch, rigs, scene, name):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    r = rigs(scene)
    a, b = crt.Context(W, H, max_frames_per_launch=4096), crt.Context(W, H, max_frames_per_launch=4096)
    r.hs.upload(a); r.upload_fresh(name, b)
    a.update_look(r.rec[name])
    out = []
    for ctx in (a, b):
        ctx.set_camera_state(*li.CAMERAS[scene]); ctx.render(1, 64, 1)
        t = ctx.timing()
        assert t["render_launches"] == 1 and t["pool_launches"] == 1, t
        out.append(ctx.accumulator())
    assert same(out[0], out[1])
    assert same(out[0], r.oracle_views(one(scene, name, 64))[0])
    a.close(); b.close()


# 3: crt_tick across the update: the Ticks before it (frames are rendered ahead by then), the update, then Ticks
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_tick_across_the_update(crt, rigs, scene):
    r = rigs(scene)
    a, b = crt.Context(W, H), crt.Context(W, H)
    r.hs.upload(a); r.upload_fresh("base", b)
    for ctx in (a, b):
        ctx.set_camera_state(*li.CAMERAS[scene])
    for spp in (1, 2, 3, 4):
        pa, ra, ea = a.tick(spp); pb, rb, eb = b.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    a.update_look(r.rec["all"])                                              # drops the frames rendered ahead with the old look
    r.upload_fresh("all", b)                                                 # (an upload keeps the camera and the accumulator)
    b.set_camera_state(*li.CAMERAS[scene])
    for spp in (5, 6, 7):
        pa, ra, ea = a.tick(spp); pb, rb, eb = b.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    old = crt.Context(W, H); r.upload_fresh("base", old); old.set_camera_state(*li.CAMERAS[scene])
    for spp in range(1, 8):
        last = old.tick(spp)
    assert not same(last[1], ra)                                             # ... and the new look is in the later Ticks
    for ctx in (a, b, old):
        ctx.close()


# 4: the other entries that shade
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_queries_after_a_look(crt, orc, rigs, scene):
    r = rigs(scene)
    cam = li.CAMERAS[scene]
    O, D = primary(W, H, li.make_oracle(orc, scene, r.looks["base"]), cam)
    base_light = r.ctx.get_light()[0]
    for name in ("all", "glass", "sky"):
        a, b = r.ctx, r.fresh
        a.update_look(r.rec[name]); r.upload_fresh(name)
        for ctx in (a, b):
            ctx.set_camera_state(*cam)
        assert np.array_equal(a.whitted_tick(), b.whitted_tick()), name
        seeds = (np.arange(len(O), dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
        sa, sb = a.sample(O, D, seeds.copy()), b.sample(O, D, seeds.copy())
        assert all(same(x, y) for x, y in zip(sa, sb)), name
        rays = np.zeros(len(O), crt.RAY_DTYPE); rays["O"], rays["D"] = O, D
        assert same(a.trace(rays), b.trace(rays)), name
        hits = a.find_nearest(O, D)
        assert hits.tobytes() == b.find_nearest(O, D).tobytes()
        assert a.get_hit_info(O, D, hits).tobytes() == b.get_hit_info(O, D, hits).tobytes(), name
        assert same(a.get_sky_color(D), b.get_sky_color(D)), name
        la, lb = a.get_light(), b.get_light()
        assert same(la[0], lb[0]) and same(la[1], lb[1]) and same(la[0], base_light) == (name != "all")
        ol = li.make_oracle(orc, scene, r.looks[name])                       # the oracle's Sample, ray by ray
        for i in range(0, len(O), 7):
            want, seed = ol.sample(O[i], D[i], int(seeds[i]))
            assert same(sa[0][i], want) and int(sa[1][i]) == seed, (name, i)
    r.ctx.update_look(r.rec["base"])


# 5: crt_render through the KD-tree and the grid: the structures are kept, they hold no appearance
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_render_through_kd_and_grid(crt, rigs, scene):
    r = rigs(scene)
    xml, kind = li.SCENES[scene]
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    for accel in (crt.ACCEL_KDTREE, crt.ACCEL_GRID):
        hs.set_look(r.rec["base"]); hs.build_alt(accel)
        a, b = crt.Context(W, H), crt.Context(W, H)
        hs.upload(a); hs.upload_alt(a, accel); a.set_render_accel(accel)
        a.update_look(r.rec["all"])                                          # behind the accelerator's upload
        hs.set_look(r.rec["all"]); hs.upload(b); hs.upload_alt(b, accel); b.set_render_accel(accel)
        for ctx in (a, b):
            ctx.set_camera_state(*li.CAMERAS[scene]); ctx.clear(); ctx.render(1, 3, 1)
        assert same(a.accumulator(), b.accumulator()), accel
        hs.set_look(r.rec["base"]); hs.upload(b); hs.upload_alt(b, accel); b.set_render_accel(accel)
        b.set_camera_state(*li.CAMERAS[scene]); b.clear(); b.render(1, 3, 1)
        assert not same(a.accumulator(), b.accumulator()), accel              # ... and not what the old look renders through it
        a.close(); b.close()


# 6: a render enqueued before the update keeps the old look
def test_a_render_enqueued_before_the_update_keeps_the_old_look(crt, rigs):
    r = rigs("tlas")
    c_old, c_new = one("tlas", "base", 64), one("tlas", "all", 64)
    want_old, want_new = r.fresh_loop(c_old)[0], r.fresh_loop(c_new)[0]
    assert not same(want_old, want_new)
    a = crt.Context(W, H, max_frames_per_launch=4096); r.hs.upload(a)
    a.set_camera_state(*li.CAMERAS["tlas"])
    a.render(1, 64, 1)                                                       # asynchronous: still in flight when the look changes
    a.update_look(r.rec["all"])
    assert same(a.accumulator(), want_old)
    a.clear(); a.render(1, 64, 1)
    assert same(a.accumulator(), want_new)
    a.close()


# 7: the refusals leave the scene intact
def test_refusals_leave_the_scene_intact(crt, rigs):
    r = rigs("tlas"); L = r.ctx.L
    a = crt.Context(W, H)
    rec = r.rec["all"]
    p = lambda x: x.ctypes.data_as(C.c_void_p)                               # noqa: E731
    assert L.crt_update_look(a.h, p(rec)) == STATE                           # no scene
    r.hs.upload(a); a.set_camera_state(*li.CAMERAS["tlas"])
    a.render(1, 2, 1); before, light = a.accumulator(), a.get_light()
    assert L.crt_update_look(a.h, None) == INVALID
    for word, value, field in ((33, -1, "floorTexture"), (33, 3, "floorTexture"), (34, 3, "skyTexture"), (34, -1, "skyTexture"), (36 + 5, -2, "material 0"), (36 + 17, 3, "material 2")):
        bad = rec.copy(); bad.view(np.int32)[word] = value                   # the rest of the record is the "all" look: nothing of it may arrive
        assert L.crt_update_look(a.h, p(bad)) == INVALID, field
        assert field in L.crt_last_error(a.h).decode(), field
    a.clear(); a.render(1, 2, 1)
    assert same(a.accumulator(), before) and all(same(x, y) for x, y in zip(a.get_light(), light))
    a.update_look(rec)                                                       # ... and the good record is taken
    a.clear(); a.render(1, 2, 1)
    assert not same(a.accumulator(), before)
    a.close()
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    assert L.crt_update_look(pc.h, p(rec)) == UNSUPPORTED
    pc.close()
