"""render_pool_kernel's floor class (device/layout.h kTileFloor; DESIGN.md section 5, "Floor tiles"): in a tile whose primary rays are all proven to miss the light
and the tree and to hit the floor, the END pass parks the primary ray through floor_ray, a straight form of new_ray that sends every lane to the BOUNCE queue with
the same D, t, seed and meta.  No sample may change, so every render is held to the oracle bit for bit — and to the same launch with the bit cleared at upload
(CRT_DEBUG_NO_FLOOR_CLASS) — with the refill inside one wavefront, with two passes, in the statistics build (every counter: the skipped root step is still
counted), on a two-level scene, across a camera change, and at depth limit 0, where a floor hit ends the path and the kernel must take the general form.
160x96 with 192 frames: the smallest shape with every kind of tile and a refill."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H = 160, 96
BUNNY, TLAS = "bunny_scene.xml", "tlas_scene.xml"
BELOW = ((0.3, -3.0, -2.0), (0.0, -1.0, 2.0))                # test_tile_class_cpu.py's "below_the_floor": num < 0, the floor is hit from underneath
DEFAULT = ((0.0, 0.0, -2.0), (0.0, 0.0, 0.0))


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


@pytest.fixture(scope="module")
def bunny_oracle(orc):
    """the oracle's 192 frames of the bunny at 160x96 (depth limit 5 with one and two passes, depth limit 0): rendered once, shared, never written to"""
    out = {}
    for depth, passes in ((5, 1), (5, 2), (0, 1)):
        o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
        o.renderer_init(W, H); o.set_params(depth, passes)
        o.render(192, 8)
        acc = o.accumulator(); acc.setflags(write=False)
        out[depth, passes] = (acc, o.counters())
    return out


def render_bunny(crt, frames, passes, **ctx_args):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(W, H, **ctx_args)
    hs.upload(ctx)
    ctx.render(1, frames, passes)
    out = ctx.accumulator(), ctx.counters(), ctx.timing(), ctx.tile_classes(ex=True), ctx.tile_classes()
    ctx.close()
    return out


def every_kind(crt, cls):
    floor = ((cls & crt.TILE_FLOOR) == crt.TILE_FLOOR).sum()
    return floor >= 4 and (cls & crt.TILE_NO_TREE == 0).sum() >= 4 and (cls == crt.TILE_SKY).sum() >= 10


@pytest.mark.parametrize("wave,passes", [(None, 1), (256, 1), (None, 2)], ids=["planned", "refill_in_one_wave", "two_passes"])
def test_bunny_equals_oracle_and_class_off(crt, bunny_oracle, monkeypatch, wave, passes):
    if wave: monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", str(wave))           # 192 frames in one wavefront of 128 slots: 64 refills, in floor tiles through floor_ray
    acc, cnt, tm, cls, old = render_bunny(crt, 192, passes, max_frames_per_launch=4096)
    assert tm["pool_launches"] >= 1
    assert every_kind(crt, cls), np.bincount(cls, minlength=16).tolist()
    assert np.array_equal(old, cls & np.uint8(7))                           # the older entry: the kTileNo* bits of the same table
    monkeypatch.setenv("CRT_DEBUG_NO_FLOOR_CLASS", "1")
    acc_off, cnt_off, tm_off, cls_off, _ = render_bunny(crt, 192, passes, max_frames_per_launch=4096)
    assert tm_off["pool_launches"] >= 1
    assert not (cls_off & crt.TILE_FLOOR_SURE).any() and np.array_equal(cls_off, cls & np.uint8(7))
    want_acc, want_cnt = bunny_oracle[5, passes]
    assert np.array_equal(acc, want_acc), "floor class on != oracle"
    assert np.array_equal(acc_off, want_acc), "floor class off != oracle"
    assert np.array_equal(acc, acc_off)
    assert cnt["rays"] == cnt_off["rays"] == want_cnt["rays"] and cnt["primary"] == cnt_off["primary"] == want_cnt["primary"]


@pytest.mark.parametrize("per_launch", [64, 4096], ids=["64_slots", "128_slots"])
def test_statistics_context_counts_what_the_oracle_counts(crt, bunny_oracle, per_launch):
    """floor_ray still counts the root step the reference takes; both stream counts of the statistics build"""
    acc, cnt, tm, cls, _ = render_bunny(crt, 192, 1, collect_stats=True, max_frames_per_launch=per_launch)
    assert tm["pool_launches"] == tm["render_launches"] >= (3 if per_launch == 64 else 1)
    assert every_kind(crt, cls)
    want_acc, want_cnt = bunny_oracle[5, 1]
    assert len(want_cnt) == 8 and cnt == want_cnt
    assert np.array_equal(acc, want_acc)


def load_pair(crt, orc, xml, kind, **ctx_args):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W, H, max_frames_per_launch=4096, **ctx_args)
    hs.upload(ctx)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H)
    return hs, ctx, o


def test_two_level_scene_equals_oracle(crt, orc):
    hs, ctx, o = load_pair(crt, orc, TLAS, 1, collect_stats=True)
    cls = ctx.tile_classes(ex=True)
    print("two-level scene, tiles by class:", np.bincount(cls, minlength=16).tolist())
    assert ((cls & crt.TILE_FLOOR) == crt.TILE_FLOOR).any() and (cls & crt.TILE_NO_TREE == 0).any()
    ctx.render(1, 192, 1); o.render(192, 8)
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    assert ctx.counters() == o.counters()
    ctx.close()


def test_camera_change_after_a_render(crt, orc):
    """below the floor (the plane is hit from underneath: num < 0, D.y > 0), then back: the table follows, each render equals the oracle"""
    hs, ctx, o = load_pair(crt, orc, BUNNY, 0)
    ctx.render(1, 128, 1)
    first = ctx.tile_classes(ex=True)
    tables = []
    for view in (BELOW, DEFAULT):
        ctx.set_camera_state(*view); o.set_camera_state(*view)
        tables.append(ctx.tile_classes(ex=True))
        assert (tables[-1] & crt.TILE_FLOOR_SURE).any()
        ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
        ctx.render(1, 192, 1); o.render(192, 8)
        assert np.array_equal(ctx.accumulator(), o.accumulator()), view
        got, want = ctx.counters(), o.counters()
        assert got["rays"] == want["rays"] and got["primary"] == want["primary"], view
    assert not np.array_equal(first, tables[0]) and not np.array_equal(tables[0], tables[1])
    ctx.close()


def test_depth_limit_zero(crt, bunny_oracle):
    """crt_create accepts depthLimit 0: a floor hit at depth 0 ends the path (END, not BOUNCE), so the kernel drops the class and takes new_ray's general form"""
    acc, cnt, tm, cls, _ = render_bunny(crt, 192, 1, depth_limit=0, max_frames_per_launch=4096)
    assert tm["pool_launches"] >= 1 and every_kind(crt, cls)
    want_acc, want_cnt = bunny_oracle[0, 1]
    assert np.array_equal(acc, want_acc)
    assert cnt["rays"] == want_cnt["rays"] == cnt["primary"]                # no ray bounces
