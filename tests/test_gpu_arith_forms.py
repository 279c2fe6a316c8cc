"""The short arithmetic forms of the render kernels' hot paths (dev_common.h: slab_accept behind tray_tame, div_short = div_by_rcp with a reciprocal of its own
behind the tame-operand guard, sky_angles with its widened guard) held to the forms they stand for, bit for bit.  Every item is an identity of IEEE arithmetic, so nothing here has a tolerance:
the probe (crt_debug_arith_forms) evaluates old and new side by side on the device and returns the number of differing records and the first of them.  The renders
follow tests/test_gpu_factor_path.py: 32 x 32, 192 frames = 3 windows forced through the pool kernel (128 slots and a refilled partial range), equal to the oracle
bit for bit, counters included."""
import itertools

import numpy as np
import pytest

from conftest import ASSETS, scene_path
from test_arith_forms_cpu import boundary_values

pytestmark = pytest.mark.gpu

PRED, DIV, SKY, DIV_SWEEP = range(4)


@pytest.fixture(scope="module")
def ctx(crt):
    c = crt.Context(64, 64)
    yield c
    c.close()


def expect_none(res, what):
    bad, first, ops, old, new = res
    print("%s: %d differing records" % (what, bad))
    assert bad == 0, "%s: %d records differ; first %s: operands %s old %s new %s" % (what, bad, first, [hex(x) for x in ops], [hex(x) for x in old], [hex(x) for x in new])


def cross(k):
    v = boundary_values().view(np.uint32)
    return np.array(list(itertools.product(v, repeat=k)), np.uint32)


def test_predicate(ctx):
    t = cross(3)
    expect_none(ctx.arith_forms(PRED, t, len(t) + (1 << 24), seed=11), "predicate")


def test_quotients(ctx, what=DIV):
    # the boundary pairs: nearly every wavefront holds an operand that is not tame, and the guard sends it to the IEEE division
    p = cross(2)
    expect_none(ctx.arith_forms(what, p), "boundary pairs")
    # the tame boundary values alone in their wavefronts (1e-4 and 1, both signs), so that the short form runs on them
    v = boundary_values()
    tame = v[(np.abs(v) >= np.float32(2.0 ** -40)) & (np.abs(v) <= np.float32(2.0 ** 40))]
    assert len(tame) == 4
    q = np.repeat(np.array(list(itertools.product(tame.view(np.uint32), repeat=2)), np.uint32), 64, axis=0)
    expect_none(ctx.arith_forms(what, q), "tame boundary pairs")
    expect_none(ctx.arith_forms(what, None, 1 << 26, seed=3), "2^26 random tame pairs")


def test_quotients_over_all_mantissas_of_the_divisor(ctx, what=DIV_SWEEP):
    # b = 1.m x 2^0 and -1.m x 2^-7 over all 2^23 m, against three numerators each (one just below a power of two, one just above, one ordinary)
    for b_bits, nums in ((0x3f800000, (1.9999999, 1.0000001, -3.1415927)), (0xbc000000, (0.99999994, 1048577.0, 7.3e-5))):
        head = np.concatenate([np.array([b_bits], np.uint32), np.array(nums, np.float32).view(np.uint32)])
        expect_none(ctx.arith_forms(what, head, 3 << 23), "mantissa sweep %#x" % b_bits)


def special_directions():
    """a component at +-0, the smallest denormal, 2^-70 and 1 (not tame, or next to it), components of equal magnitude (the quotient 1 of crt_atan_pos's middle
    range), each alone in a wavefront and in one lane of a wavefront of ordinary directions"""
    zero, one, den, tiny = np.float32(0), np.float32(1), np.array([1], np.uint32).view(np.float32)[0], np.float32(2.0 ** -70)
    r = np.float32(np.sqrt(0.5))
    rows = []
    for s in (one, -one):
        for c in (zero, den, tiny, one):
            c = c * s
            rows += [[c, np.float32(0.6), np.float32(0.8)], [np.float32(0.8), c, np.float32(0.6)], [np.float32(0.6), np.float32(0.8), c], [c, np.float32(0.3), c], [c, c, c]]
        rows += [[r * s, zero, r], [r, np.float32(0.1), r * s], [np.float32(0.5) * s, r, np.float32(-0.5)], [np.float32(2.0 ** -40) * s, zero, one], [one, zero, np.float32(2.0 ** -41) * s]]
    return np.array(rows, np.float32)


def test_sky_angles(ctx):
    S = special_directions()
    alone = np.repeat(S, 64, axis=0)
    rng = np.random.default_rng(29)
    U = rng.standard_normal((64 * len(S), 3)).astype(np.float32)
    U = (U / np.sqrt((U * U).sum(axis=1, keepdims=True), dtype=np.float32)).astype(np.float32)
    mixed = U.copy()
    mixed[np.arange(len(S)) * 64 + (np.arange(len(S)) * 7) % 64] = S
    D = np.concatenate([alone, mixed, U]).view(np.uint32)
    expect_none(ctx.arith_forms(SKY, D, len(D) + (1 << 24), seed=7), "sky_angles")


# ---- renders ----
W, H, FRAMES = 32, 32, 192
SCENES = [("bunny_scene.xml", 0), ("cube_scene.xml", 0), ("tlas_scene.xml", 1)]
CASES = [(xml, kind, d, p) for xml, kind in SCENES for d in (0, 1, 5) for p in (1, 2)]


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's accumulator and counters of every case, rendered once (one oracle per scene) and left unchanged"""
    out = {}
    for xml, kind in SCENES:
        o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
        o.renderer_init(W, H)
        for x, k, depth, passes in CASES:
            if x != xml:
                continue
            o.set_params(depth, passes)
            o.clear(); o.reset_counters()
            o.render(FRAMES, 4)
            acc = o.accumulator(); acc.setflags(write=False)
            out[(xml, depth, passes)] = (acc, o.counters())
    return out


@pytest.fixture(scope="module")
def host_scenes(crt):
    return {xml: crt.HostScene(scene_path(xml), kind, ASSETS) for xml, kind in SCENES}


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
@pytest.mark.parametrize("xml,kind,depth,passes", CASES)
def test_renders_match_oracle(crt, want, host_scenes, monkeypatch, xml, kind, depth, passes, stats):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    ctx = crt.Context(W, H, depth_limit=depth, collect_stats=stats, max_frames_per_launch=4096)
    try:
        host_scenes[xml].upload(ctx)
        ctx.render(1, FRAMES, passes)
        acc = ctx.accumulator()
        assert ctx.timing()["pool_launches"] == 1
        ref, cnt = want[(xml, depth, passes)]
        assert np.array_equal(acc, ref)
        if stats:
            assert ctx.counters() == cnt
        else:
            assert ctx.counters()["rays"] == cnt["rays"]
    finally:
        ctx.close()


def test_sky_tiles_through_both_slab_forms(crt, orc, monkeypatch):
    """the bunny at 160 x 96 has sky, floor-only and mesh tiles: with the tile-class table the sky tiles go through render_sky_kernel (sky_angles per sample, the
    texel form of the slab), without it through the pool kernel's END pass (the 12-byte form); both are the oracle's image"""
    import ctypes as C
    w, h = 160, 96
    o, _ = orc.load_scene(scene_path("bunny_scene.xml"), 0, ASSETS)
    o.renderer_init(w, h)
    o.render(FRAMES, 8)
    ref = o.accumulator()
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    for table in (True, False):
        if not table:
            monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
        ctx = crt.Context(w, h, max_frames_per_launch=4096)
        try:
            hs.upload(ctx)
            if table:
                assert (ctx.tile_classes() == crt.TILE_SKY).sum() >= 10
            ctx.render(1, FRAMES, 1)
            ctx.L.crt_debug_sky_launches.restype = C.c_int
            ctx.L.crt_debug_sky_launches.argtypes = [C.c_void_p]
            assert ctx.L.crt_debug_sky_launches(ctx.h) == (1 if table else 0) and ctx.timing()["pool_launches"] == 1
            assert np.array_equal(ctx.accumulator(), ref), "table" if table else "no table"
            assert ctx.counters()["rays"] == o.counters()["rays"]
        finally:
            ctx.close()
