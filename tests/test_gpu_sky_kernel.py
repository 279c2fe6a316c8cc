"""render_sky_kernel (device/render_sky.hip): a pool launch that has the tile-class table leaves the order's kTileSky tail to one straight-line
launch beside it.  Which kernel rendered a tile must not show: every render is held to the oracle bit for bit and to the same render without the table
(CRT_DEBUG_NO_TILE_CLASS: one pool launch renders every tile) — with two passes, a last window of 8 frames, a second launch that continues the first, tile
partitions, a camera change that turns sky tiles into mesh tiles, an image of sky tiles only, an image without one, and a statistics context (no sky launch).
Every test asserts the class counts it relies on and whether a sky launch ran (crt_debug_sky_launches: launches of the context so far)."""
import ctypes as C

import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H = 160, 96
BUNNY = "bunny_scene.xml"
NEAR = ((0.0, 0.3, -0.4), (0.0, -0.3, 2.0))                 # test_gpu_tile_class.py's: close to the mesh, it covers tiles that were sky; 4 sky tiles stay
ALL_SKY = ((0.0, 0.0, -6.0), (8.0, 8.0, 2.0))               # 32x32: up and sideways, the mesh and the light in front of the eye but outside the view
FLOOR = ((0.0, 2.5, -1.5), (0.0, -1.0, 1.0))                # 160x96: down at the floor from above, every ray can hit it


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


def sky_launches(ctx):
    ctx.L.crt_debug_sky_launches.restype = C.c_int
    ctx.L.crt_debug_sky_launches.argtypes = [C.c_void_p]
    return ctx.L.crt_debug_sky_launches(ctx.h)


def host_table(crt, ctx, w, h):
    """crt_debug_tile_classes_host (the CPU function) on the context's Scene block: root pair, camera, light offsets, floor"""
    out = np.zeros(16 + 22, np.float32); cam = np.zeros(12, np.float32); lf = np.zeros(4, np.float32)
    ctx.L.crt_debug_primary_block.restype = C.c_int
    ctx.L.crt_debug_primary_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert ctx.L.crt_debug_primary_block(ctx.h, out.ctypes.data, cam.ctypes.data, lf.ctypes.data) == 0
    return crt.tile_classes_host(cam, (lf[1], lf[0], lf[2]), 0.5, lf[3], out[:16], w, h)      # Quad(0, 1): size 0.5


def oracle_of(orc, w, h, frames, passes=1, camera=None):
    o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
    o.renderer_init(w, h); o.set_params(5, passes)
    if camera: o.set_camera_state(*camera)
    o.render(frames, 8)
    acc = o.accumulator(); acc.setflags(write=False)
    return acc, o.counters()


@pytest.fixture(scope="module")
def oracle(orc):
    """the oracle's renders of the default view: rendered once, shared, never written to"""
    return {(192, 1): oracle_of(orc, W, H, 192, 1), (192, 2): oracle_of(orc, W, H, 192, 2), (200, 1): oracle_of(orc, W, H, 200, 1)}


def open_bunny(crt, w=W, h=H, **ctx_args):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(w, h, max_frames_per_launch=4096, **ctx_args)
    hs.upload(ctx)
    return hs, ctx


def every_kind_of_tile(crt, cls):
    return (cls == crt.TILE_SKY).sum() >= 10 and (cls & crt.TILE_NO_TREE == 0).sum() >= 4 and ((cls != crt.TILE_SKY) & (cls != 0)).any()


@pytest.mark.parametrize("passes", [1, 2])
def test_equals_oracle_and_the_launch_without_the_table(crt, oracle, monkeypatch, passes):
    want_acc, want_cnt = oracle[(192, passes)]
    _, ctx = open_bunny(crt)
    cls = ctx.tile_classes()
    assert every_kind_of_tile(crt, cls)
    ctx.render(1, 192, passes)
    acc, cnt, tm = ctx.accumulator(), ctx.counters(), ctx.timing()
    assert sky_launches(ctx) == 1 and tm["pool_launches"] == tm["render_launches"] == 1
    ctx.close()
    monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
    _, ctx = open_bunny(crt)
    ctx.render(1, 192, passes)
    acc_off, cnt_off, tm_off = ctx.accumulator(), ctx.counters(), ctx.timing()
    assert sky_launches(ctx) == 0 and tm_off["pool_launches"] == 1
    ctx.close()
    assert np.array_equal(acc, want_acc), "sky launch + pool launch != oracle"
    assert np.array_equal(acc, acc_off), "sky launch + pool launch != one pool launch without the table"
    assert cnt["rays"] == want_cnt["rays"] == cnt_off["rays"] and cnt["primary"] == want_cnt["primary"] == cnt_off["primary"]


def test_partial_group(crt, oracle):
    """200 frames: the last 64-frame window has 8 lanes; and 128 + 72 frames, the second launch starting at spp 129"""
    want_acc, want_cnt = oracle[(200, 1)]
    _, ctx = open_bunny(crt)
    assert every_kind_of_tile(crt, ctx.tile_classes())
    ctx.render(1, 200, 1)
    assert sky_launches(ctx) == 1
    assert np.array_equal(ctx.accumulator(), want_acc)
    cnt = ctx.counters()
    assert cnt["rays"] == want_cnt["rays"] and cnt["primary"] == want_cnt["primary"]
    ctx.clear(); ctx.reset_counters(); ctx.timing()
    ctx.render(1, 128, 1); ctx.render(129, 72, 1)
    tm = ctx.timing()
    # (once the first job's tile costs have arrived a launch may be planned with a block table, and a job that needs one keeps its sky tiles in the pool launch)
    assert tm["pool_launches"] == tm["render_launches"] == 2 and sky_launches(ctx) == 3 - tm["split_launches"]
    assert np.array_equal(ctx.accumulator(), want_acc)
    cnt = ctx.counters()
    assert cnt["rays"] == want_cnt["rays"] and cnt["primary"] == want_cnt["primary"]
    ctx.close()


def test_tile_ownership(crt, oracle):
    """the three owners of an interleaved partition: each has sky tiles of its own, and their accumulators sum to the whole image"""
    want_acc, _ = oracle[(192, 1)]
    total = np.zeros_like(want_acc)
    for r in range(3):
        first, stride, count = crt.tile_partition(r, 3, 60)
        _, ctx = open_bunny(crt, tile_first=first, tile_stride=stride, tile_count=count)
        cls = ctx.tile_classes()
        assert len(cls) == count == 20 and (cls == crt.TILE_SKY).sum() >= 6 and (cls != crt.TILE_SKY).sum() >= 10
        ctx.render(1, 192, 1)
        assert sky_launches(ctx) == 1 and ctx.timing()["pool_launches"] == 1
        total += ctx.accumulator()
        ctx.close()
    assert np.array_equal(total, want_acc)


def test_former_sky_tiles_reach_the_tree_after_a_camera_change(crt, orc):
    _, ctx = open_bunny(crt)
    o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
    o.renderer_init(W, H)
    before = ctx.tile_classes()
    assert every_kind_of_tile(crt, before)
    ctx.render(1, 128, 1); o.render(128, 8)
    assert sky_launches(ctx) == 1
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    ctx.set_camera_state(*NEAR); o.set_camera_state(*NEAR)
    after = ctx.tile_classes()
    assert ((before == crt.TILE_SKY) & (after & crt.TILE_NO_TREE == 0)).sum() >= 4 and (after == crt.TILE_SKY).sum() >= 1
    ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
    ctx.render(1, 128, 1); o.render(128, 8)
    assert sky_launches(ctx) == 2
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    got, want = ctx.counters(), o.counters()
    assert got["rays"] == want["rays"] and got["primary"] == want["primary"]
    ctx.close()


def test_an_image_of_sky_tiles_only(crt, orc):
    want_acc, want_cnt = oracle_of(orc, 32, 32, 192, 1, ALL_SKY)
    _, ctx = open_bunny(crt, 32, 32)
    ctx.set_camera_state(*ALL_SKY)
    table = host_table(crt, ctx, 32, 32)
    assert len(table) == 4 and (table == crt.TILE_SKY).all() and np.array_equal(ctx.tile_classes(), table)
    ctx.render(1, 192, 1)
    tm = ctx.timing()
    assert sky_launches(ctx) == 1 and tm["pool_launches"] == 0 and tm["render_launches"] == 1       # only the sky launch ran
    assert np.array_equal(ctx.accumulator(), want_acc)
    cnt = ctx.counters()
    assert cnt["rays"] == want_cnt["rays"] == cnt["primary"] == want_cnt["primary"] == 32 * 32 * 192
    ctx.close()


def test_an_image_without_a_sky_tile(crt, orc):
    want_acc, want_cnt = oracle_of(orc, W, H, 192, 1, FLOOR)
    _, ctx = open_bunny(crt)
    ctx.set_camera_state(*FLOOR)
    table = host_table(crt, ctx, W, H)
    assert len(table) == 60 and not (table == crt.TILE_SKY).any() and table.any() and np.array_equal(ctx.tile_classes(), table)
    ctx.render(1, 192, 1)
    assert sky_launches(ctx) == 0 and ctx.timing()["pool_launches"] == 1
    assert np.array_equal(ctx.accumulator(), want_acc)
    cnt = ctx.counters()
    assert cnt["rays"] == want_cnt["rays"] and cnt["primary"] == want_cnt["primary"]
    ctx.close()


def test_statistics_context_runs_no_sky_launch(crt, oracle):
    """its pool build counts the root step of every primary ray, a sky tile's included"""
    want_acc, want_cnt = oracle[(192, 1)]
    _, ctx = open_bunny(crt, collect_stats=True)
    assert every_kind_of_tile(crt, ctx.tile_classes())
    ctx.render(1, 192, 1)
    assert sky_launches(ctx) == 0 and ctx.timing()["pool_launches"] == 1
    assert ctx.counters() == want_cnt
    assert np.array_equal(ctx.accumulator(), want_acc)
    ctx.close()
