"""Planned render_pool_kernel launches — a wave table with a range length per tile rank, a short part behind it, a sky launch beside it, a block-table head in
front of it — from GIVEN tile costs (Context.set_job_costs: the installing half of the library's own cost adoption), at image sizes a test controls.  The
recipes are tests/planned_launch_inputs.py's; tests/test_planned_launch_cpu.py holds each to the plan it was made for.

Every case: context, scene, costs, ONE job — then the accumulator bit for bit against the oracle's sequential render, the ray count, the resolved pixels and
energy, and the launch shape (wavefronts that own more than 128 frames, split launches, sky launches) against what crt_debug_sky_split predicts from the context's
own tile classes.  Which wavefront renders a (tile, frame) changes nothing about its samples, so all plans of one scene and shape give one image: the oracle renders
once per (scene, size, frames, passes)."""
import ctypes as C

import numpy as np
import pytest

import planned_launch_inputs as I
from conftest import ASSETS, scene_path
from planned_launch_inputs import S, SKY

pytestmark = pytest.mark.gpu

BUNNY_SMALL, BUNNY, CUBE, TLAS, BUNNY4 = (("bunny_scene.xml", 0, 64, 48), ("bunny_scene.xml", 0, 96, 64), ("cube_scene.xml", 0, 32, 32), ("tlas_scene.xml", 1, 64, 48),
                                          ("bunny4_scene.xml", 0, 96, 64))
FRAMES = 1189                                     # 1024 + 128 + 37: a long part, then two short groups, the last a partial window with fewer streams than slots
ERR_INVALID, ERR_STATE = -1, -5                   # include/crt_abi.h
CAMERA_2 = ((0.6, 0.5, -2.4), (0.0, 0.0, 1.0))    # case 10's second camera


def long_waves(ctx):
    ctx.L.crt_debug_pool_long_waves.restype = C.c_int; ctx.L.crt_debug_pool_long_waves.argtypes = [C.c_void_p]
    return ctx.L.crt_debug_pool_long_waves(ctx.h)


def sky_launches(ctx):
    ctx.L.crt_debug_sky_launches.restype = C.c_int; ctx.L.crt_debug_sky_launches.argtypes = [C.c_void_p]
    return ctx.L.crt_debug_sky_launches(ctx.h)


@pytest.fixture(scope="module")
def oracle(orc):
    """(accumulator, rays, pixels, energy) of the oracle's sequential render, once per (scene, kind, W, H, frames, passes, camera); read-only"""
    cache = {}

    def get(scene, frames, passes=1, camera=None):
        key = (scene, frames, passes, camera)
        if key not in cache:
            xml, kind, w, h = scene
            o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
            o.renderer_init(w, h); o.set_params(5, passes)
            if camera: o.set_camera_state(*camera)
            o.render(frames, 8)
            acc, px = o.accumulator().copy(), o.screen().copy()
            acc.setflags(write=False); px.setflags(write=False)
            cache[key] = (acc, o.counters()["rays"], px, np.float32(o.energy()))
        return cache[key]
    return get


@pytest.fixture(autouse=True)
def planned_env(monkeypatch):
    monkeypatch.delenv("CRT_SKY_PLACEMENT", raising=False)
    for k, v in I.ENV.items(): monkeypatch.setenv(k, v)


def context(crt, scene, **kw):
    xml, kind, w, h = scene
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(w, h, max_frames_per_launch=4096, **kw)
    hs.upload(ctx)
    return ctx


def recipe_plan(crt, ctx, recipe, frames, **kw):
    """the recipe's costs for the context's own tiles and the plan the library makes of them: (plan, (cost, pool ticks, sky ticks))"""
    cls = ctx.tile_classes()
    costs = recipe(cls, frames, **kw)
    return I.plan(crt, cls, *((costs[0], frames) + costs[1:])), costs


def install(crt, ctx, recipe, frames, **kw):
    """... installed; returns (plan, cost)"""
    p, costs = recipe_plan(crt, ctx, recipe, frames, **kw)
    ctx.set_job_costs(*costs)
    got, pt, st = ctx.job_costs()
    assert np.array_equal(got, costs[0]) and (pt, st) == costs[1:]
    return p, costs[0]


def job(ctx, frames, passes=1):
    """one job from a cleared accumulator; returns the sky launches it made"""
    ctx.clear(); ctx.reset_counters(); ctx.timing()
    before = sky_launches(ctx)
    ctx.render(1, frames, passes)
    return sky_launches(ctx) - before


def check_image(ctx, want, frames, passes=1):
    acc, rays, px, energy = want
    assert np.array_equal(ctx.accumulator(), acc)
    assert ctx.counters()["rays"] == rays
    got_px, got_energy = ctx.resolve_screen(1.0 / (1 + frames * passes))
    assert np.array_equal(got_px, px) and np.float32(got_energy) == energy


def check_shape(ctx, p, sky):
    """the launch the context reports is the launch the plan predicts"""
    t = ctx.timing()
    assert t["render_launches"] == 1 and t["pool_launches"] == 1, t
    assert long_waves(ctx) == p["long_waves"] and t["split_launches"] == p["split_launches"] and sky == p["sky_launches"], (long_waves(ctx), t, sky, p)


def planned_job(crt, oracle, scene, recipe, frames=FRAMES, passes=1, ctx_kw={}, **kw):
    ctx = context(crt, scene, **ctx_kw)
    p, _ = install(crt, ctx, recipe, frames, **kw)
    assert p["long_waves"] > 0 and p["blocks"] > 0                       # (a wave table: test_planned_launch_cpu.py's precondition, on this context's classes)
    I.replay(p, frames)
    sky = job(ctx, frames, passes)
    check_shape(ctx, p, sky)
    check_image(ctx, oracle(scene, frames, passes), frames, passes)
    return ctx, p


def test_recorded_tile_classes_are_the_contexts(crt):
    """what test_planned_launch_cpu.py checks the recipes on"""
    for scene in (BUNNY_SMALL, BUNNY, CUBE, TLAS, BUNNY4):
        ctx = context(crt, scene)
        assert ctx.tile_classes().tolist() == I.CLASSES[(scene[0], scene[2], scene[3])], scene
        ctx.close()


# 1. mixed lengths with a sky launch, behind the pool launch and ahead of it
@pytest.mark.parametrize("placement", ["behind", "ahead"])
def test_mixed_lengths_with_a_sky_launch(crt, oracle, monkeypatch, placement):
    if placement == "ahead": monkeypatch.setenv("CRT_SKY_PLACEMENT", "ahead")
    ctx, p = planned_job(crt, oracle, BUNNY_SMALL, I.mixed)
    cls = ctx.tile_classes()
    assert (cls == SKY).sum() >= 2 and (cls == I.FLOOR_ONLY).sum() >= 2 and ((cls & I.NO_TREE) == 0).sum() >= 4
    assert sorted(I.lengths(p)) == [S, 2 * S, 4 * S, 8 * S] and p["sky"] >= 2 and p["head"] == 0


# 2. the same image from other plans
@pytest.mark.parametrize("recipe,kw", [(I.uniform_long, {}), (I.last_rank_only, {}), (I.mixed, {"reverse": True})], ids=["same_length", "last_rank_only", "reversed"])
def test_other_plans_same_image(crt, oracle, recipe, kw):
    ctx, p = planned_job(crt, oracle, BUNNY_SMALL, recipe, **kw)
    if recipe is I.uniform_long: assert (p["wf"] == 8 * S).all()
    if recipe is I.last_rank_only: assert (p["wf"][:-1] == S).all() and p["wf"][-1] > S
    if kw: assert not np.array_equal(p["order"], np.arange(p["n"])) and (ctx.tile_classes()[p["order"][-p["sky"]:]] == SKY).all() and p["order"][-1] != p["n"] - 1


# 3. no short part: the grid is the table's blocks
@pytest.mark.parametrize("frames", [1024, 2048])
def test_jobs_without_a_short_part(crt, oracle, frames):
    ctx, p = planned_job(crt, oracle, BUNNY_SMALL, I.mixed, frames=frames, span=I.SPAN_NO_SHORT_PART)
    assert p["long_frames"] == frames
    if frames == 2048: assert set((frames // p["wf"]).tolist()) >= {2, 16}


# 4. a block-table head and a wave table behind it in the descriptor buffer
def test_head_and_wave_table_in_one_job(crt, oracle):
    ctx, p = planned_job(crt, oracle, BUNNY, I.head_and_table, ctx_kw={"render_streams": 3})
    assert p["head"] == 2 and p["split_launches"] == 1 and p["sky_launches"] == 0 and (ctx.tile_classes() == SKY).sum() >= 2


# 5. two passes, four tiles, four lengths
def test_two_passes_four_lengths(crt, oracle):
    ctx, p = planned_job(crt, oracle, CUBE, I.mixed, passes=2)
    assert p["wf"].tolist() == [S, 2 * S, 4 * S, 8 * S]


# 6. the two-level scene
def test_two_level_scene(crt, oracle):
    ctx, p = planned_job(crt, oracle, TLAS, I.mixed)
    assert len(I.lengths(p)) == 4


# 7. 32-bit pool references
def test_wide_pool_references(crt, oracle):
    ctx, p = planned_job(crt, oracle, BUNNY4, I.mixed)
    assert ctx.pool_lds(FRAMES)[2] == 32 and len(I.lengths(p)) == 4


# 8. the trial: planned, plain, then whichever was faster
def test_trial_of_the_plan(crt, oracle, monkeypatch):
    monkeypatch.delenv("CRT_PLAN_NO_TRIAL")
    ctx = context(crt, BUNNY_SMALL)
    p, _ = install(crt, ctx, I.mixed, FRAMES)
    want = oracle(BUNNY_SMALL, FRAMES)
    seen = []
    for i in range(4):
        job(ctx, FRAMES)
        seen.append(long_waves(ctx))
        check_image(ctx, want, FRAMES)
    assert seen[0] == p["long_waves"] > 0 and seen[1] == 0 and seen[2] == seen[3] and seen[2] in (0, p["long_waves"]), seen


# 9. two strided owners, each with costs for its own tiles
def test_tile_ownership(crt, oracle):
    xml, kind, w, h = BUNNY
    tiles = (w // 16) * (h // 16)
    want = oracle(BUNNY, FRAMES)
    total, rays = np.zeros((h, w, 4), np.float32), 0
    for r in range(2):
        first, stride, count = crt.tile_partition(r, 2, tiles)
        ctx = context(crt, BUNNY, tile_first=first, tile_stride=stride, tile_count=count)
        p, _ = install(crt, ctx, I.mixed, FRAMES, reverse=bool(r))
        assert p["long_waves"] > 0 and p["n"] == count
        sky = job(ctx, FRAMES)
        check_shape(ctx, p, sky)
        acc = ctx.accumulator()
        mine = np.zeros((h, w), bool)
        for t in range(first, first + count * stride, stride):
            mine[t // (w // 16) * 16:t // (w // 16) * 16 + 16, t % (w // 16) * 16:t % (w // 16) * 16 + 16] = True
        assert not acc[~mine].any() and np.array_equal(acc[mine], want[0][mine])
        total += acc; rays += ctx.counters()["rays"]
        ctx.close()
    assert np.array_equal(total, want[0]) and rays == want[1]


# 10. what drops measured costs drops installed ones; installed costs survive a measurement in flight
def test_invalidation(crt, oracle):
    ctx, p = planned_job(crt, oracle, BUNNY_SMALL, I.mixed)
    ctx.set_camera_state(*CAMERA_2)
    with pytest.raises(crt.CrtError) as e: ctx.job_costs()
    assert e.value.code == ERR_STATE
    want = oracle(BUNNY_SMALL, FRAMES, 1, CAMERA_2)
    p2, costs2 = recipe_plan(crt, ctx, I.mixed, FRAMES, reverse=True)     # (for the new camera's classes)
    assert p2["long_waves"] > 0
    job(ctx, FRAMES)                                                      # plain, and it measures: its costs are on their way when the next ones are installed
    assert long_waves(ctx) == 0
    ctx.set_job_costs(*costs2)                                            # (nothing has waited for the job in between)
    check_image(ctx, want, FRAMES)
    sky = job(ctx, FRAMES)
    check_shape(ctx, p2, sky)
    check_image(ctx, want, FRAMES)
    assert np.array_equal(ctx.job_costs()[0], costs2[0])
    ctx.set_camera_state((0.0, 0.0, -2.0), (0.0, 0.0, 0.0))               # ... and a camera change drops them again
    with pytest.raises(crt.CrtError): ctx.job_costs()


# 11. refusals write nothing
def test_refusals(crt, oracle):
    L = crt.lib()
    L.crt_debug_set_job_costs.restype = C.c_int; L.crt_debug_set_job_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double]
    some = np.full(64, 1000, np.uint32)
    assert L.crt_debug_set_job_costs(None, some.ctypes.data, I.P, 0.0) == ERR_INVALID
    xml, kind, w, h = BUNNY_SMALL
    bare = crt.Context(w, h)
    with pytest.raises(crt.CrtError) as e: bare.set_job_costs(some[:bare.tiles], I.P)
    assert e.value.code == ERR_STATE
    hs = crt.HostScene(scene_path(xml), kind, ASSETS); hs.upload(bare)    # the refused context is as good as new
    job(bare, FRAMES); assert long_waves(bare) == 0
    check_image(bare, oracle(BUNNY_SMALL, FRAMES), FRAMES)
    bare.close()
    stats = context(crt, BUNNY_SMALL, collect_stats=True)
    with pytest.raises(crt.CrtError) as e: stats.set_job_costs(some[:stats.tiles], I.P)
    assert e.value.code == ERR_STATE
    with pytest.raises(crt.CrtError): stats.job_costs()
    job(stats, FRAMES); assert long_waves(stats) == 0
    check_image(stats, oracle(BUNNY_SMALL, FRAMES), FRAMES)
    stats.close()
    ctx = context(crt, BUNNY_SMALL)
    with pytest.raises(crt.CrtError) as e: ctx.set_job_costs(None, I.P)
    assert e.value.code == ERR_INVALID
    with pytest.raises(crt.CrtError): ctx.set_job_costs(some[:ctx.tiles], float("nan"))
    with pytest.raises(crt.CrtError): ctx.job_costs()                     # nothing was installed
    job(ctx, FRAMES); assert long_waves(ctx) == 0
    check_image(ctx, oracle(BUNNY_SMALL, FRAMES), FRAMES)
