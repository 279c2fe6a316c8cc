"""The compact sample slab (device/sample_body.h): every render kernel stores 12-byte samples, a sky launch whose accumulate follows at
once stores the 4-byte sky texel instead, and accumulate_kernel / commit_frame_kernel read both.  Nothing of that may show: every accumulator here is held to the
oracle's bit for bit (np.array_equal), `rays` and `primary` to the oracle's counters — pool + sky launches with 1, 2 and 3 passes (3 passes: 2 304-byte rows, 12-byte
samples across every power-of-two boundary), a last window of 8 frames, two launches, the launch without the class table, a split job, render_tiles_kernel alone,
a tile partition, images of sky tiles only and without one, a camera change with no synchronisation between two renders, a bound accumulator whose w channel
holds -0.0, 5.0 and a NaN, crt_tick's commits across a window boundary, the 32-bit pool form, and the sequential kernel (Sample through the KD-tree).
Shapes are tests/test_gpu_sky_kernel.py's: the bunny at 160x96 in the default view has sky, floor-only and mesh tiles."""
import ctypes as C

import numpy as np
import pytest

from conftest import ASSETS, scene_path

torch = pytest.importorskip("torch")       # (at collection, as the other device-buffer tests: the bound accumulator is a torch tensor)

pytestmark = pytest.mark.gpu

W, H = 160, 96
BUNNY = "bunny_scene.xml"
NEAR = ((0.0, 0.3, -0.4), (0.0, -0.3, 2.0))                 # close to the mesh: it covers tiles that were sky; 4 sky tiles stay
ALL_SKY = ((0.0, 0.0, -6.0), (8.0, 8.0, 2.0))               # 32x32: every tile is a sky tile
FLOOR = ((0.0, 2.5, -1.5), (0.0, -1.0, 1.0))                # 160x96: no sky tile
SPLIT_FRAMES = 72                                           # two windows: the smallest job; the planner splits it once a 128-frame measuring job has delivered the tile costs


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


def sky_launches(ctx):
    ctx.L.crt_debug_sky_launches.restype = C.c_int
    ctx.L.crt_debug_sky_launches.argtypes = [C.c_void_p]
    return ctx.L.crt_debug_sky_launches(ctx.h)


def frozen(a):
    a.setflags(write=False)
    return a


def oracle_steps(orc, w, h, steps, passes=1, camera=None, xml=BUNNY, kind=0):
    """one oracle Renderer; {frames: (accumulator, counters)} after each of the ascending frame counts in `steps`"""
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(w, h); o.set_params(5, passes)
    if camera: o.set_camera_state(*camera)
    out, done = {}, 0
    for n in steps:
        o.render(n - done, 8); done = n
        out[n] = (frozen(o.accumulator()), o.counters())
    return out


@pytest.fixture(scope="module")
def oracle(orc):
    """the oracle's renders of the default view: rendered once, shared, never written to.  Key: (frames, passes)"""
    out = {(n, 1): v for n, v in oracle_steps(orc, W, H, sorted({64, 128, 192, 200, SPLIT_FRAMES})).items()}
    out[(192, 2)] = oracle_steps(orc, W, H, [192], 2)[192]
    out[(192, 3)] = oracle_steps(orc, W, H, [192], 3)[192]
    return out


def open_bunny(crt, w=W, h=H, **ctx_args):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(w, h, max_frames_per_launch=4096, **ctx_args)
    hs.upload(ctx)
    return hs, ctx


def every_kind_of_tile(crt, cls):
    return (cls == crt.TILE_SKY).sum() >= 10 and (cls & crt.TILE_NO_TREE == 0).sum() >= 4 and ((cls != crt.TILE_SKY) & (cls != 0)).any()


def same_counts(got, want):
    return got["rays"] == want["rays"] and got["primary"] == want["primary"]


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_pool_and_sky_launch_with_and_without_the_table(crt, oracle, monkeypatch, passes):
    want_acc, want_cnt = oracle[(192, passes)]
    _, ctx = open_bunny(crt)
    assert every_kind_of_tile(crt, ctx.tile_classes())
    ctx.render(1, 192, passes)
    acc, cnt, tm = ctx.accumulator(), ctx.counters(), ctx.timing()
    assert sky_launches(ctx) == 1 and tm["pool_launches"] == tm["render_launches"] == 1
    ctx.close()
    monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")              # the sky tiles go through the pool kernel, in the 12-byte form
    _, ctx = open_bunny(crt)
    ctx.render(1, 192, passes)
    acc_off, cnt_off = ctx.accumulator(), ctx.counters()
    assert sky_launches(ctx) == 0 and ctx.timing()["pool_launches"] == 1
    ctx.close()
    assert np.array_equal(acc, want_acc), "sky launch (texel form) + pool launch != oracle"
    assert np.array_equal(acc_off, want_acc) and np.array_equal(acc, acc_off), "one pool launch without the table != the launch with the sky launch"
    assert same_counts(cnt, want_cnt) and same_counts(cnt_off, want_cnt)


@pytest.mark.parametrize("table", [True, False], ids=["table", "table_off"])
def test_partial_window_and_two_launches(crt, oracle, monkeypatch, table):
    """200 frames: the last window has 8 frames (the texel rows' and the sample rows' tails stay unread); then 128 + 72 frames as two launches"""
    if not table: monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
    want_acc, want_cnt = oracle[(200, 1)]
    _, ctx = open_bunny(crt)
    ctx.render(1, 200, 1)
    assert sky_launches(ctx) == (1 if table else 0)
    assert np.array_equal(ctx.accumulator(), want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.clear(); ctx.reset_counters(); ctx.timing()
    ctx.render(1, 128, 1); ctx.render(129, 72, 1)
    acc, tm = ctx.accumulator(), ctx.timing()
    assert tm["pool_launches"] == tm["render_launches"] == 2
    assert sky_launches(ctx) == ((3 - tm["split_launches"]) if table else 0)     # (a job planned with a block table keeps its sky tiles in the pool launch)
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()


def test_split_job(crt, oracle):
    """pool launch + block-table render_tiles_kernel launch into one slab: after a measuring job has delivered the tile costs"""
    want_acc, want_cnt = oracle[(SPLIT_FRAMES, 1)]
    _, ctx = open_bunny(crt)
    ctx.render(1, 128, 1)                                           # the measuring job
    assert np.array_equal(ctx.accumulator(), oracle[(128, 1)][0])   # (read back: its costs have arrived)
    ctx.clear(); ctx.reset_counters(); ctx.timing()
    ctx.render(1, SPLIT_FRAMES, 1)
    acc, tm = ctx.accumulator(), ctx.timing()
    assert tm["split_launches"] == 1 and tm["pool_launches"] == 1, tm
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()


def test_render_tiles_kernel_alone(crt, orc, monkeypatch):
    monkeypatch.delenv("CRT_RENDER_KERNEL")
    want = oracle_steps(orc, 64, 48, [10, 64])
    for frames in (64, 10):
        _, ctx = open_bunny(crt, 64, 48)
        ctx.render(1, frames, 1)
        acc, tm = ctx.accumulator(), ctx.timing()
        assert tm["pool_launches"] == 0 and tm["render_launches"] == 1 and sky_launches(ctx) == 0
        assert np.array_equal(acc, want[frames][0]) and same_counts(ctx.counters(), want[frames][1]), frames
        ctx.close()


def test_tile_partition(crt, oracle):
    """tile_first = r, tile_stride = 3: every pixel is rendered by one rank, and the three accumulators together are the oracle's image"""
    want_acc, want_cnt = oracle[(192, 1)]
    total, owners, cnt = np.zeros_like(want_acc), np.zeros((H, W), np.int32), {"rays": 0, "primary": 0}
    for r in range(3):
        first, stride, count = crt.tile_partition(r, 3, 60)
        _, ctx = open_bunny(crt, tile_first=first, tile_stride=stride, tile_count=count)
        if r == 1: assert (first, stride) == (1, 3)
        cls = ctx.tile_classes()
        assert len(cls) == count == 20 and (cls == crt.TILE_SKY).sum() >= 6 and (cls != crt.TILE_SKY).sum() >= 10
        ctx.render(1, 192, 1)
        assert sky_launches(ctx) == 1 and ctx.timing()["pool_launches"] == 1
        acc, c = ctx.accumulator(), ctx.counters()
        ctx.close()
        owners += (acc[..., :3] != 0).any(axis=2)
        total += acc
        cnt = {k: cnt[k] + c[k] for k in cnt}
    assert (owners <= 1).all() and (owners == (want_acc[..., :3] != 0).any(axis=2)).all()
    assert np.array_equal(total, want_acc) and same_counts(cnt, want_cnt)


def test_sky_only_and_floor_images(crt, orc):
    want_acc, want_cnt = oracle_steps(orc, 32, 32, [192], 1, ALL_SKY)[192]
    _, ctx = open_bunny(crt, 32, 32)
    ctx.set_camera_state(*ALL_SKY)
    assert (ctx.tile_classes() == crt.TILE_SKY).all()
    ctx.render(1, 192, 1)
    acc, tm = ctx.accumulator(), ctx.timing()
    assert sky_launches(ctx) == 1 and tm["pool_launches"] == 0 and tm["render_launches"] == 1       # the sky launch is the whole job
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()
    want_acc, want_cnt = oracle_steps(orc, W, H, [192], 1, FLOOR)[192]
    _, ctx = open_bunny(crt)
    ctx.set_camera_state(*FLOOR)
    assert not (ctx.tile_classes() == crt.TILE_SKY).any()
    ctx.render(1, 192, 1)
    acc = ctx.accumulator()
    assert sky_launches(ctx) == 0 and ctx.timing()["pool_launches"] == 1
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()


def test_unsynchronised_camera_change(crt, orc, oracle):
    """two renders with a camera change and NO synchronisation between them: the second call re-uploads the class table and the tile order, in which former sky
    tiles are mesh tiles, while the first accumulate — which reads the sky launch's ranks of the OLD order — may still be queued.  Both images land in one
    accumulator: the default view's 128 frames, then NEAR's 128 frames on top; the oracle adds the same samples in the same order.  The first image alone is
    oracle[(128, 1)] (test_split_job's read-back), the second alone is rendered after a clear and compared with the oracle's render of NEAR."""
    o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
    o.renderer_init(W, H); o.render(128, 8)
    assert np.array_equal(o.accumulator(), oracle[(128, 1)][0])
    o.set_camera_state(*NEAR); o.set_spp(1); o.render(128, 8)
    _, ctx = open_bunny(crt)
    before = ctx.tile_classes()
    assert every_kind_of_tile(crt, before)
    ctx.render(1, 128, 1)
    ctx.set_camera_state(*NEAR)
    ctx.render(1, 128, 1)
    both = ctx.accumulator()
    after = ctx.tile_classes()
    assert ((before == crt.TILE_SKY) & (after & crt.TILE_NO_TREE == 0)).sum() >= 4 and (after == crt.TILE_SKY).sum() >= 1
    assert sky_launches(ctx) == 2
    assert np.array_equal(both, o.accumulator())
    o.clear(); o.set_spp(1); o.reset_counters(); o.render(128, 8)
    ctx.clear(); ctx.reset_counters()
    ctx.render(1, 128, 1)
    assert np.array_equal(ctx.accumulator(), o.accumulator()) and same_counts(ctx.counters(), o.counters())
    ctx.close()


def test_bound_accumulator_keeps_the_w_rule(crt, oracle):
    """the float4 slab added its stored 0.0f to w once per sample: -0.0 becomes +0.0, everything else — 5.0, a NaN's payload — stays.  In a sky tile (texel form)
    and in a mesh tile (sample form)."""
    want_acc, want_cnt = oracle[(64, 1)]
    _, ctx = open_bunny(crt)
    cls = ctx.tile_classes()
    sky_tile, mesh_tile = int(np.flatnonzero(cls == crt.TILE_SKY)[0]), int(np.flatnonzero(cls & crt.TILE_NO_TREE == 0)[0])
    w = np.zeros((H, W), np.uint32)
    NEG0, FIVE, NAN = 0x80000000, 0x40A00000, 0x7FC12345
    for t in (sky_tile, mesh_tile):
        x0, y0 = (t % (W // 16)) * 16, (t // (W // 16)) * 16
        w[y0 + 1, x0 + 2], w[y0 + 7, x0 + 15], w[y0 + 15, x0] = NEG0, FIVE, NAN
    host = np.zeros((H, W, 4), np.float32)
    host[..., 3] = w.view(np.float32)
    acc = torch.from_numpy(host).to("cuda:0")
    ctx.bind_accumulator(acc.data_ptr())
    ctx.render(1, 64, 1)
    ctx.sync()
    assert sky_launches(ctx) == 1
    got, cnt = acc.cpu().numpy(), ctx.counters()
    ctx.close()
    assert np.array_equal(got[..., :3], want_acc[..., :3]) and same_counts(cnt, want_cnt)
    want_w = w.copy(); want_w[w == NEG0] = 0
    assert (want_w == FIVE).sum() == (want_w == NAN).sum() == 2 and (w == NEG0).sum() == 2
    assert np.array_equal(got[..., 3].view(np.uint32), want_w)


def test_tick_commits_across_a_window_boundary(crt, orc):
    """crt_tick at 64x48: Ticks 1 and 2 are plain; the second still Tick renders frames 3..66 ahead, the next launch 128 frames (67..194), whose first window ends
    at frame 130: commit_frame_kernel reads 12-byte samples of both windows, sky tiles included (a render-ahead launch never writes the texel form)"""
    w, h = 64, 48
    _, ctx = open_bunny(crt, w, h)
    assert (ctx.tile_classes() == crt.TILE_SKY).sum() >= 1
    o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
    o.renderer_init(w, h)
    checks, done = {1, 2, 3, 66, 67, 129, 130, 131, 132, 136}, 0
    for k in range(1, 137):
        read = k in checks
        _, acc, _ = ctx.tick(k, 1, pixels=False, accumulator=read)
        if read:
            o.render(k - done, 8); done = k
            assert np.array_equal(acc, o.accumulator()), k
            if k == 1: assert same_counts(ctx.counters(), o.counters())   # (from the second still Tick on the counters include frames rendered ahead and not yet committed)
    assert sky_launches(ctx) >= 2                                  # the render-ahead launches had sky tiles, and a sky launch each
    ctx.close()


def test_wide_pool_form(crt, oracle, monkeypatch):
    monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    want_acc, want_cnt = oracle[(192, 1)]
    _, ctx = open_bunny(crt)
    assert ctx.pool_lds(192)[2] == 32
    ctx.render(1, 192, 1)
    acc = ctx.accumulator()
    assert sky_launches(ctx) == 1 and ctx.timing()["pool_launches"] == 1
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()


def test_sequential_kernel_writes_the_sample_form(crt, orc):
    """render_seq_kernel (Sample through FileScene's KD-tree; the PrimitiveScene's renders run the same kernel) stores through the same helper and is read by the
    same accumulate: 64x48, 3 passes, 70 frames — two windows, the second of 6 frames"""
    w, h, frames, passes = 64, 48, 70, 3
    o, _ = orc.load_scene(scene_path(BUNNY), 0, ASSETS)
    o.renderer_init(w, h); o.set_params(5, passes)
    kd = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, kd)
    o.render(frames, 8)
    want_acc, want_cnt = o.accumulator(), o.counters()
    orc.set_render_accel(o, None); kd.close()
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    hs.build_alt(crt.ACCEL_KDTREE)
    ctx = crt.Context(w, h); hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
    ctx.set_render_accel(crt.ACCEL_KDTREE)
    ctx.render(1, frames, passes)
    acc = ctx.accumulator()
    assert np.array_equal(acc, want_acc) and same_counts(ctx.counters(), want_cnt)
    ctx.close()
