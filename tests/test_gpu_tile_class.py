"""render_pool_kernel with the tile classes (device/tile_class.h; DESIGN.md section 5, "tile classes"): a set bit only skips a test whose outcome the host has
proven, so every render is held to the oracle bit for bit — and to the same launch with the table off (CRT_DEBUG_NO_TILE_CLASS) — with the refill inside the
specialised END pass, with two passes, in the statistics build (every counter), on a two-level scene, and after every kind of write that makes the table stale:
a camera change, a host-side scene update, a TLAS rebuilt on the device.  The table on the device is the CPU function's."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the library loads the HIP runtime: the transforms of the device-side TLAS rebuild live in a torch tensor

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H = 160, 96
BUNNY, TLAS = "bunny_scene.xml", "tlas_scene.xml"


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


@pytest.fixture(scope="module")
def bunny_oracle(orc):
    """the oracle's 192 frames of the bunny at 160x96, one and two passes: rendered once, shared, never written to"""
    out = {}
    for passes in (1, 2):
        o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
        o.renderer_init(W, H); o.set_params(5, passes)
        o.render(192, 8)
        acc = o.accumulator(); acc.setflags(write=False)
        out[passes] = (acc, o.counters())
    return out


def render_bunny(crt, frames, passes, **ctx_args):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(W, H, **ctx_args)
    hs.upload(ctx)
    ctx.render(1, frames, passes)
    acc, cnt, tm, cls = ctx.accumulator(), ctx.counters(), ctx.timing(), ctx.tile_classes()
    ctx.close()
    return acc, cnt, tm, cls


@pytest.mark.parametrize("wave,passes", [(None, 1), (256, 1), (None, 2)], ids=["planned", "refill_in_one_wave", "two_passes"])
def test_bunny_equals_oracle_and_table_off(crt, bunny_oracle, monkeypatch, wave, passes):
    if wave: monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", str(wave))           # 192 frames in one wavefront of 128 slots: 64 refills, in sky tiles inside the short pass
    acc, cnt, tm, cls = render_bunny(crt, 192, passes, max_frames_per_launch=4096)
    assert tm["pool_launches"] >= 1
    assert (cls == crt.TILE_SKY).sum() >= 10 and (cls & crt.TILE_NO_TREE == 0).sum() >= 4 and ((cls != crt.TILE_SKY) & (cls != 0)).any()   # every kind of tile is in the image
    monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
    acc_off, cnt_off, tm_off, _ = render_bunny(crt, 192, passes, max_frames_per_launch=4096)
    assert tm_off["pool_launches"] >= 1
    want_acc, want_cnt = bunny_oracle[passes]
    assert np.array_equal(acc, want_acc), "table on != oracle"
    assert np.array_equal(acc_off, want_acc), "table off != oracle"
    assert cnt["rays"] == cnt_off["rays"] == want_cnt["rays"] and cnt["primary"] == cnt_off["primary"] == want_cnt["primary"]


@pytest.mark.parametrize("per_launch", [64, 4096], ids=["64_slots", "128_slots"])
def test_statistics_context_counts_what_the_oracle_counts(crt, bunny_oracle, per_launch):
    """a skipped root test still counts its interior step; both stream counts of the statistics build"""
    acc, cnt, tm, cls = render_bunny(crt, 192, 1, collect_stats=True, max_frames_per_launch=per_launch)
    assert tm["pool_launches"] == tm["render_launches"] >= (3 if per_launch == 64 else 1)
    want_acc, want_cnt = bunny_oracle[1]
    assert cnt == want_cnt
    assert np.array_equal(acc, want_acc)


def load_pair(crt, orc, xml, kind, **ctx_args):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W, H, max_frames_per_launch=4096, **ctx_args)
    hs.upload(ctx)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H)
    return hs, ctx, o


def same_after(ctx, o, frames, what):
    ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
    ctx.render(1, frames, 1); o.render(frames, 8)
    assert np.array_equal(ctx.accumulator(), o.accumulator()), what
    got, want = ctx.counters(), o.counters()
    assert got["rays"] == want["rays"] and got["primary"] == want["primary"], what


def test_two_level_scene_equals_oracle(crt, orc):
    hs, ctx, o = load_pair(crt, orc, TLAS, 1, collect_stats=True)
    cls = ctx.tile_classes()
    print("two-level scene, tiles by class:", np.bincount(cls, minlength=8).tolist())
    assert cls.any() and (cls & crt.TILE_NO_TREE == 0).any()
    ctx.render(1, 128, 1); o.render(128, 8)
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    assert ctx.counters() == o.counters()


# ---- staleness: the table follows every write of the Scene's camera-relative block ----
def test_camera_change_after_a_render(crt, orc):
    hs, ctx, o = load_pair(crt, orc, BUNNY, 0)
    ctx.render(1, 128, 1)
    before = ctx.tile_classes()
    near = ((0.0, 0.3, -0.4), (0.0, -0.3, 2.0))                              # close to the mesh: it now covers tiles that were sky
    ctx.set_camera_state(*near); o.set_camera_state(*near)
    after = ctx.tile_classes()
    assert ((before == crt.TILE_SKY) & (after & crt.TILE_NO_TREE == 0)).sum() >= 4
    same_after(ctx, o, 128, "camera")


def test_scene_update_after_a_render(crt, orc):
    hs, ctx, o = load_pair(crt, orc, BUNNY, 0)
    ctx.render(1, 128, 1)
    before = ctx.tile_classes()
    t = hs.bvh(0)["tris"]
    moved = (np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1) + np.array([0, 1.2, 0], np.float32)).astype(np.float32)     # the mesh rises into the sky half
    hs.move_and_refit(0, moved); o.move_and_refit(0, moved)
    hs.update(ctx, crt.UPDATE_BOUNDS)
    after = ctx.tile_classes()
    assert ((before == crt.TILE_SKY) & (after & crt.TILE_NO_TREE == 0)).sum() >= 4
    same_after(ctx, o, 128, "scene update")


def test_transforms_on_the_device_after_a_render(crt, orc):
    hs, ctx, o = load_pair(crt, orc, TLAS, 1)
    ctx.render(1, 128, 1)
    before = ctx.tile_classes()
    T = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(hs.bvh_count())]).astype(np.float32)
    T[:, 1, 3] += np.float32(1.3)                                           # every instance rises
    dev_T = torch.from_numpy(np.ascontiguousarray(T)).to(torch.device("cuda", 0)); torch.cuda.synchronize()
    ctx.update_transforms_device(dev_T)
    for i in range(len(T)): o.set_transform(i, T[i])
    after = ctx.tile_classes()
    print("tiles whose class changed:", int((before != after).sum()), "of", len(before))
    assert before.any()
    same_after(ctx, o, 128, "transforms on the device")


# ---- the table on the device is the CPU function's ----
def primary_block(ctx):
    out = np.zeros(16 + 22, np.float32); cam = np.zeros(12, np.float32); lf = np.zeros(4, np.float32)
    ctx.L.crt_debug_primary_block.restype = C.c_int
    ctx.L.crt_debug_primary_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert ctx.L.crt_debug_primary_block(ctx.h, out.ctypes.data, cam.ctypes.data, lf.ctypes.data) == 0
    return out[:16], cam, lf


def host_table(crt, ctx, w, h, part=None):
    pair, cam, lf = primary_block(ctx)
    first, stride, count = part if part else (0, 1, -1)
    return crt.tile_classes_host(cam, (lf[1], lf[0], lf[2]), 0.5, lf[3], pair, w, h, first, stride, count)      # Quad(0, 1): size 0.5


def test_read_back_is_the_cpu_table(crt):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(W, H)
    assert not ctx.tile_classes().any()                                     # no scene: nothing is known
    hs.upload(ctx)
    a = ctx.tile_classes()
    assert len(a) == 60 and a.any() and np.array_equal(a, host_table(crt, ctx, W, H))
    ctx.set_camera_state((1.5, 0.7, -3.0), (0.2, -0.1, 2.0))
    b = ctx.tile_classes()
    assert not np.array_equal(a, b) and np.array_equal(b, host_table(crt, ctx, W, H))
    ctx.render(1, 2, 1)
    assert np.array_equal(ctx.tile_classes(), b)
    ctx.close()
    # a tile partition of a larger image
    tiles = (1280 // 16) * (720 // 16)
    part = crt.tile_partition(1, 8, tiles)
    ctx = crt.Context(1280, 720, tile_first=part[0], tile_stride=part[1], tile_count=part[2])
    hs.upload(ctx)
    got = ctx.tile_classes()
    assert len(got) == part[2] and (got == crt.TILE_SKY).sum() >= 1400 // 8 and np.array_equal(got, host_table(crt, ctx, 1280, 720, part))
    ctx.close()
