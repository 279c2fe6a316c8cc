"""crt_tick: one Renderer::Tick per call, served from frames rendered ahead while the camera and the scene stay put.  Every Tick must be bit for bit
what the plain path leaves — crt_render(spp, 1, passes) + crt_read_accumulator + crt_resolve_screen on a second context — and, where the oracle
renders the same sequence, what the oracle's Renderer leaves."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

SCENES = [("bunny_scene.xml", 0), ("tlas_scene.xml", 1)]


def scale_of(spp, passes):
    return float(np.float32(1) / np.float32(spp + passes))           # renderer.cpp:119 in float, as crt_tick and the facade form it


def plain_tick(ctx, spp, passes=1, read=True):
    ctx.render(spp, 1, passes)
    if not read:
        return None
    acc = ctx.accumulator()
    px, e = ctx.resolve_screen(scale_of(spp, passes))
    return px, acc, e


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def pair(crt, xml, kind, W, H, **kw):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ca, cb = crt.Context(W, H, **kw), crt.Context(W, H, **kw)
    hs.upload(ca); hs.upload(cb)
    return hs, ca, cb


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("xml,kind", SCENES)
def test_static_camera_matches_oracle_and_plain_path(crt, orc, xml, kind, passes):
    W, H = 128, 80
    _, ctx, plain = pair(crt, xml, kind, W, H)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H); o.set_params(5, passes)
    checks, done = {1, 2, 63, 64, 65, 130}, 0
    for k in range(1, 131):
        spp = 1 + (k - 1) * passes
        got = ctx.tick(spp, passes)
        assert same(got, plain_tick(plain, spp, passes)), k
        if k in checks:
            o.render(k - done, 8); done = k
            assert o.spp() == spp + passes
            assert np.array_equal(got[1], o.accumulator()), k
            assert np.array_equal(got[0], o.screen()), k
            assert got[2] == o.energy(), k
    assert ctx.timing()["render_launches"] <= 10


def test_full_size_matches_plain_path(crt):
    W, H = 1280, 720
    _, ctx, plain = pair(crt, "bunny_scene.xml", 0, W, H)
    checks = {1, 2, 3, 64, 65, 66, 130, 193, 194, 200}
    for k in range(1, 201):
        read = k in checks
        got = ctx.tick(k, 1, pixels=read, accumulator=read)
        want = plain_tick(plain, k, 1, read)
        if read:
            assert same(got, want), k
    assert ctx.timing()["render_launches"] <= 10


def test_camera_moves(crt):
    W, H = 128, 80
    _, ctx, plain = pair(crt, "bunny_scene.xml", 0, W, H)
    pos0, tgt = (0.0, 0.0, -2.0), (0.0, 0.0, 0.0)
    spp = 1
    seq = [("still", pos0)] * 6 + [("move", (0.4, 0.3, -2.4))] + [("still", (0.4, 0.3, -2.4))] * 70
    for k, (what, pos) in enumerate(seq):
        for c in (ctx, plain):
            c.set_camera_state(pos, tgt)                           # re-sent every Tick, as PushCamera does
            if what == "move":
                c.clear()                                          # the facade's ClearAccumulator; spp keeps counting
        assert same(ctx.tick(spp), plain_tick(plain, spp)), k
        spp += 1
    assert ctx.timing()["render_launches"] <= 12
    plain.timing()
    # a camera that changes every Tick: same images, and exactly the plain path's launches (nothing rendered ahead)
    for k in range(20):
        pos = (0.02 * k, 0.1, -2.2 - 0.01 * k)
        for c in (ctx, plain):
            c.set_camera_state(pos, tgt); c.clear()
        assert same(ctx.tick(spp), plain_tick(plain, spp)), k
        spp += 1
    assert ctx.timing()["render_launches"] == plain.timing()["render_launches"] == 20


def test_scene_update_mid_sequence(crt):
    from test_gpu_scene_update import rigid
    W, H = 128, 80
    hs, ctx, plain = pair(crt, "tlas_scene.xml", 1, W, H)
    T0 = hs.blas_transform(1)[0].reshape(4, 4)
    for k in range(1, 81):
        if k == 30:
            hs.set_transform(1, rigid(0.5, T0[:3, 3] + np.array([0.3, 0.1, -0.2], np.float32)))
            hs.update(ctx, crt.UPDATE_TRANSFORMS); hs.update(plain, crt.UPDATE_TRANSFORMS)
        assert same(ctx.tick(k), plain_tick(plain, k)), k


def test_ring_wraps_under_jumps_passes_renders_and_clears(crt):
    W, H = 128, 80
    _, ctx, plain = pair(crt, "bunny_scene.xml", 0, W, H, max_frames_per_launch=64)
    spp, passes = 1, 1

    def ticks(n):
        nonlocal spp
        for _ in range(n):
            assert same(ctx.tick(spp, passes), plain_tick(plain, spp, passes)), (spp, passes)
            spp += passes

    ticks(140)                       # three render-ahead launches of 64 frames
    spp += 10; ticks(5)              # spp jump
    passes = 2; ticks(70)            # passes change
    for c in (ctx, plain):
        c.render(spp, 512, passes)   # eight launches through the ring while frames were queued
    spp += 512 * passes; ticks(70)
    for c in (ctx, plain):
        c.clear()                    # frames rendered ahead stay valid
    ticks(70)


def test_tile_subset_contexts(crt):
    W, H = 128, 80
    n = (W // 16) * (H // 16)
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    for rank in range(2):
        first, stride, count = crt.tile_partition(rank, 2, n)
        ctx = crt.Context(W, H, tile_first=first, tile_stride=stride, tile_count=count)
        plain = crt.Context(W, H, tile_first=first, tile_stride=stride, tile_count=count)
        hs.upload(ctx); hs.upload(plain)
        for k in range(1, 71):
            got, want = ctx.tick(k), plain_tick(plain, k)
            assert same(got, want), (rank, k)
        assert ctx.timing()["render_launches"] <= 10


def test_unspeculated_paths(crt):
    W, H = 96, 64
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    hs.build_alt(crt.ACCEL_KDTREE)
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.3)
    for what in ("kd", "prim", "stats"):
        ctxs = []
        for _ in range(2):
            c = crt.Context(W, H, collect_stats=(what == "stats"))
            if what == "prim":
                ps.upload(c)
            else:
                hs.upload(c)
            if what == "kd":
                hs.upload_alt(c, crt.ACCEL_KDTREE); c.set_render_accel(crt.ACCEL_KDTREE)
            ctxs.append(c)
        ctx, plain = ctxs
        for k in range(1, 9):
            assert same(ctx.tick(k), plain_tick(plain, k)), (what, k)
        if what == "stats":
            assert ctx.timing()["render_launches"] == 8
            assert ctx.counters() == plain.counters()


def test_facade_tick_matches_oracle(crt, orc):
    W, H = 96, 64
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    r = crt.HostRenderer(hs, W, H); r.init()
    o, _ = orc.load_scene(scene_path("bunny_scene.xml"), 0, ASSETS)
    o.renderer_init(W, H)
    r.context().timing()
    for k in range(70):
        r.tick(16.0); o.render(1, 4)
        assert r.spp == o.spp() == k + 2
        assert np.array_equal(r.accumulator(), o.accumulator()), k
        assert np.array_equal(r.screen(), o.screen()), k
        assert r.energy == o.energy(), k
    assert r.context().timing()["render_launches"] <= 10
    # an `animating` Tick clears the accumulator first (SetTime changes nothing on the device): frames rendered ahead stay valid
    a, b = crt.HostRenderer(hs, W, H), crt.HostRenderer(hs, W, H)
    a.init(); b.init()
    for k in range(70):
        a.clear(); a.tick(16.0)
        b.clear(); b.render(1)
        assert a.spp == b.spp and np.array_equal(a.accumulator(), b.accumulator()) and np.array_equal(a.screen(), b.screen()) and a.energy == b.energy, k


def test_null_outputs_and_errors(crt):
    W, H = 64, 48
    ctx = crt.Context(W, H)
    with pytest.raises(crt.CrtError) as e:
        ctx.tick(1)
    assert e.value.code == -5                                        # CRT_ERR_STATE: before an upload
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    hs.upload(ctx)
    plain = crt.Context(W, H); hs.upload(plain)
    for bad in (0, 5):
        with pytest.raises(crt.CrtError) as e:
            ctx.tick(1, bad)
        assert e.value.code == -1                                    # CRT_ERR_INVALID: passes outside 1..4
    for k in range(1, 71):
        px, acc, energy = ctx.tick(k, 1, pixels=(k % 3 == 0), accumulator=(k % 2 == 0))
        want = plain_tick(plain, k)
        assert energy == want[2], k
        assert (px is None) == (k % 3 != 0) and (acc is None) == (k % 2 != 0)
        if px is not None:
            assert np.array_equal(px, want[0]), k
        if acc is not None:
            assert np.array_equal(acc, want[1]), k
    assert same(ctx.tick(71), plain_tick(plain, 71))
