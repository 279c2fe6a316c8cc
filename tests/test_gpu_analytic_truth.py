"""The HIP kernels against closed-form ground truth (tests/analytic_truth.py), directly: the same scenes, seeds, sample counts and criterion as
tests/test_analytic_truth_cpu.py holds the oracle to.  sample_query_kernel (Context.sample) through every structure a scene can be walked by, the three render
kernels (render_tiles_kernel, render_pool_kernel + render_sky_kernel, the 32-bit pool form), whitted_tick, and find_nearest over the PrimitiveScene.  Every test
also asserts bit equality with the oracle on these scenes, which no other test renders."""
import ctypes as C
import os

import numpy as np
import pytest

import analytic_truth as at
import render_looks_inputs as li
from conftest import ASSETS
from test_gpu_golden_and_edges import write_scene
from test_gpu_primitive_scene import _rays

pytestmark = pytest.mark.gpu

WORLDS = ["bvh", "tlas", "kd", "grid", "tlas_kd", "tlas_grid"]
N_BITS = 4096                                      # samples of every case that are also compared with the oracle's, bit for bit


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    return at.write_scenes(tmp_path_factory.mktemp("truth"), write_scene)


@pytest.fixture(scope="module")
def flat_sky(orc, scenes):
    return orc.read_image(os.path.join(os.path.dirname(scenes["S0"]), "sky.tga"))


@pytest.fixture(scope="module")
def oracle_images(orc, scenes):
    """the oracle's renders of S0, made once and never written to: the default view and the view up at the light"""
    o, _ = orc.load_scene(scenes["S0"], 0, ASSETS); o.renderer_init(at.W, at.H)
    o.render(at.FRAMES, 8); view = o.accumulator(); view.setflags(write=False)
    o.clear(); o.set_camera_state(*at.LIGHT_CAMERA); o.render(at.LIGHT_FRAMES, 8); light = o.accumulator(); light.setflags(write=False)
    return view, light


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_world(crt, orc, xml, world, depth_limit=5):
    """(context, oracle, accel code) of scene `xml` walked through `world`'s structure"""
    kind = 1 if world.startswith("tlas") else 0
    name = world.split("_")[-1]
    accel = {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}.get(name, 0)
    hs = crt.HostScene(xml, kind, ASSETS)
    if accel:
        hs.build_alt(accel)
    ctx = crt.Context(at.W, at.H, depth_limit=depth_limit); hs.upload(ctx)
    if accel:
        hs.upload_alt(ctx, accel)
    o, _ = orc.load_scene(xml, kind, ASSETS); o.renderer_init(at.W, at.H); o.set_params(depth_limit, 1)
    if accel and kind == 0:
        o._alt = orc.alt_accel(name, o.bvh(0)["tris"]); orc.set_render_accel(o, o._alt)
    elif accel:
        orc.set_blas_accel(o, orc.blas_accels(o, name))
    return ctx, o, accel


def sample_one_ray(ctx, o, accel, O, D, seeds, what):
    """Context.sample of one ray under every seed; the first N_BITS equal the oracle's through the same structure"""
    n = len(seeds)
    rgb, _ = ctx.sample(np.broadcast_to(O, (n, 3)), np.broadcast_to(D, (n, 3)), seeds, accel=accel)
    want = at.oracle_samples(o, O, D, seeds[:N_BITS])
    assert np.array_equal(bits(rgb[:N_BITS]), bits(want)), what
    return rgb


@pytest.mark.parametrize("world", WORLDS)
def test_sample_floor_points(crt, orc, scenes, world):
    ctx, o, accel = open_world(crt, orc, scenes["S0"], world)
    for k in range(len(at.FLOOR_POINTS)):
        O, D, mean, second, seeds = at.floor_case(k)
        what = "floor point %d through %s" % (k, world)
        at.check_mean(sample_one_ray(ctx, o, accel, O, D, seeds, what), mean, second, what)
    ctx.close()


# not through tlas_kd: KDTree::IntersectKDTree (kdtree.cpp:164-203) visits one child where the ray runs parallel to a split plane, a BLAS is walked in object
# space, and there a ray at normal incidence on a cube's face is parallel to two axes: that walk does not see the slab at all (test_gpu_tlas_alt.py and
# test_gpu_sample_query.py hold it to the oracle on such rays).  The floor points go through every structure.
@pytest.mark.parametrize("world,depth_limit", [(w, 5) for w in WORLDS if w != "tlas_kd"] + [("bvh", 1), ("bvh", 3), ("tlas", 3)])
def test_sample_slab(crt, orc, scenes, world, depth_limit):
    ctx, o, accel = open_world(crt, orc, scenes["S2"], world, depth_limit)
    O, D, _, _, seeds, _, t0 = at.slab_case(depth_limit)
    h = ctx.find_nearest(O, D)
    assert h["objIdx"][0] == 2 and abs(float(h["t"][0]) - t0) <= 1e-5
    what = "slab through %s, depth limit %d" % (world, depth_limit)
    at.check_slab(sample_one_ray(ctx, o, accel, O, D, seeds, what), depth_limit, what)
    ctx.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_sample_mirror(crt, orc, scenes, kind):
    sky = orc.read_image(ASSETS + "/sky_gradient.png")
    O, D, want, axis, _ = at.mirror_case(kind, sky)
    assert (axis == 1).sum() >= 100 and (axis != 1).sum() >= 100
    ctx, o, _ = open_world(crt, orc, scenes["S1"], "tlas" if kind else "bvh")
    rgb, _ = ctx.sample(O, D, 1 + np.arange(len(O), dtype=np.uint32))
    assert (np.abs(rgb - want) <= 1e-6 * np.maximum(np.abs(want), 1e-3)).all()
    assert np.array_equal(bits(rgb), bits(np.stack([o.sample(O[i], D[i], 1 + i)[0] for i in range(len(O))])))
    ctx.close()


def sky_launches(ctx):
    ctx.L.crt_debug_sky_launches.restype = C.c_int
    ctx.L.crt_debug_sky_launches.argtypes = [C.c_void_p]
    return ctx.L.crt_debug_sky_launches(ctx.h)


@pytest.mark.parametrize("mode", ["tiles", "pool", "pool32"])
def test_render_of_the_floor(crt, scenes, flat_sky, oracle_images, monkeypatch, mode):
    """S0 at 64 x 64: sky pixels, floor-tile means against pixel_truth, the pixels that see only the light quad; through render_tiles_kernel (launches of 64
    frames), through render_pool_kernel with the sky tiles from render_sky_kernel, and through the pool kernel's 32-bit form"""
    if mode != "tiles":
        monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    if mode == "pool32":
        monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    hs = crt.HostScene(scenes["S0"], 0, ASSETS)
    ctx = crt.Context(at.W, at.H, max_frames_per_launch=64 if mode == "tiles" else 4096); hs.upload(ctx)
    ctx.render(1, at.FRAMES, 1)
    acc, tm = ctx.accumulator(), ctx.timing()
    if mode == "tiles":
        assert tm["pool_launches"] == 0 and tm["render_launches"] == at.FRAMES // 64
    else:
        assert tm["pool_launches"] >= 1 and ctx.pool_lds(at.FRAMES)[2] == (32 if mode == "pool32" else 16)
    if mode == "pool":
        assert sky_launches(ctx) == 1                                      # the 8 sky tiles came from render_sky_kernel
    at.check_render(acc, at.FRAMES, flat_sky, mode)
    assert np.array_equal(acc, oracle_images[0]), mode
    ctx.clear(); ctx.set_camera_state(*at.LIGHT_CAMERA); ctx.render(1, at.LIGHT_FRAMES, 1)
    acc = ctx.accumulator()
    at.check_light_pixels(acc, at.LIGHT_FRAMES, mode)
    assert np.array_equal(acc, oracle_images[1]), mode
    ctx.close()


@pytest.mark.parametrize("scene,kind", [("S0", 0), ("S1", 0), ("S1", 1)])
def test_whitted_floor(crt, orc, scenes, scene, kind):
    hs = crt.HostScene(scenes[scene], kind, ASSETS)
    ctx = crt.Context(at.W, at.H); hs.upload(ctx)
    px = ctx.whitted_tick()
    acc = ctx.accumulator()
    at.check_whitted(acc, [at.Box(**at.MIRROR)] if scene == "S1" else [], "whitted_tick %s kind %d" % (scene, kind), shadow=scene == "S1")
    o, _ = orc.load_scene(scenes[scene], kind, ASSETS); o.renderer_init(at.W, at.H); o.whitted(4)
    assert np.array_equal(acc, o.accumulator()) and np.array_equal(px, o.screen())
    ctx.close()


@pytest.mark.parametrize("t", [0.0, 1.3, 7.77])
def test_primitive_scene(crt, orc, t):
    O, D = _rays(20000, 11)
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(t)
    ctx = crt.Context(64, 64); ps.upload(ctx)
    h = ctx.find_nearest(O, D)
    tw, iw, margin = at.prim_truth(O, D, t)
    at.prim_check(h["t"], h["objIdx"], tw, iw, margin)
    g = orc.primitive_scene(ASSETS, t).find_nearest(O, D)
    assert np.array_equal(h["objIdx"], g["objIdx"]) and np.array_equal(bits(h["t"]), bits(g["t"]))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the light quad of a look, turned and resized (analytic_truth.QUAD_LOOKS), applied by update_look and as one render_looks job
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LOOK_NAMES = sorted(at.QUAD_LOOKS)


def look_record(crt, hs, name):
    T, half = at.look_cells(name)
    return crt.look_records([dict(li.with_light(crt.look_dicts(hs.look())[0], T.reshape(4, 4)), light_size=float(half))])[0]


def look_oracle(orc, xml, kind, name):
    o, _ = orc.load_scene(xml, kind, ASSETS); o.renderer_init(at.W, at.H)
    T, half = at.look_cells(name)
    o.set_light_quad(T, li.inverse_no_scale(T), half)
    return o


@pytest.mark.parametrize("world", ["bvh", "tlas"])
@pytest.mark.parametrize("name", LOOK_NAMES)
def test_sample_floor_points_under_a_quad_look(crt, orc, scenes, name, world):
    kind = 1 if world == "tlas" else 0
    hs = crt.HostScene(scenes["S0"], kind, ASSETS)
    ctx = crt.Context(at.W, at.H); hs.upload(ctx)
    ctx.update_look(look_record(crt, hs, name))
    o = look_oracle(orc, scenes["S0"], kind, name)
    q = at.look_quad(name)
    for k in range(len(at.QUAD_FLOOR_POINTS)):
        O, D, mean, second, seeds = at.floor_case(k, q, salt=LOOK_NAMES.index(name))
        what = "%s, floor point %d through %s" % (name, k, world)
        at.check_mean(sample_one_ray(ctx, o, 0, O, D, seeds, what), mean, second, what)
    ctx.close()


@pytest.mark.parametrize("mode", ["tiles", "pool", "pool32"])
@pytest.mark.parametrize("name", LOOK_NAMES)
def test_render_of_the_floor_under_quad_looks(crt, orc, scenes, flat_sky, monkeypatch, name, mode):
    """per look: floor-tile means against the expectation and the oracle's bits; under the 0.9 quad, looking up: every pixel inside its projection and wholly
    outside the 0.5 quad's is exactly the light's colour (tiles a classifier blind to lightSize would prove free of the light)"""
    if mode != "tiles":
        monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    if mode == "pool32":
        monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    hs = crt.HostScene(scenes["S0"], 0, ASSETS)
    ctx = crt.Context(at.W, at.H, max_frames_per_launch=64 if mode == "tiles" else 4096); hs.upload(ctx)
    ctx.update_look(look_record(crt, hs, name))
    ctx.render(1, at.FRAMES, 1)
    acc, tm = ctx.accumulator(), ctx.timing()
    assert (tm["pool_launches"] == 0) == (mode == "tiles"), tm
    at.check_render(acc, at.FRAMES, flat_sky, "%s under %s" % (mode, name), quad=at.look_quad(name), key=name)
    o = look_oracle(orc, scenes["S0"], 0, name); o.render(at.FRAMES, 8)
    assert np.array_equal(acc, o.accumulator()), (mode, name)
    if name == "size_0.9":
        ctx.clear(); ctx.set_camera_state(*at.LIGHT_CAMERA); ctx.render(1, at.LIGHT_FRAMES, 1)
        ring = at.check_light_pixels(ctx.accumulator(), at.LIGHT_FRAMES, mode + ", the ring round the 0.5 quad", quad=(at.QUAD[0], 0.9), beyond=at.QUAD)
        assert ring >= 200
    ctx.close()


def test_whitted_floor_under_quad_looks(crt, orc, scenes):
    hs = crt.HostScene(scenes["S0"], 0, ASSETS)
    ctx = crt.Context(at.W, at.H); hs.upload(ctx)
    for name in LOOK_NAMES:
        ctx.update_look(look_record(crt, hs, name))
        px = ctx.whitted_tick(); acc = ctx.accumulator()
        at.check_whitted(acc, [], "whitted_tick under %s" % name, shadow=name == "z25", quad=at.look_quad(name), tol=at.WHITTED_QUAD_TOL)
        o = look_oracle(orc, scenes["S0"], 0, name); o.whitted(4)
        assert np.array_equal(acc, o.accumulator()) and np.array_equal(px, o.screen()), name
    ctx.close()


def test_one_render_looks_job_of_the_quad_looks(crt, scenes, flat_sky):
    """the five looks as one job through the default camera: per view the floor-tile means of its own look (the live look stays the file's)"""
    hs = crt.HostScene(scenes["S0"], 0, ASSETS)
    ctx = crt.Context(at.W, at.H, max_frames_per_launch=4096); hs.upload(ctx)
    cams = crt.camera_records(at.W, at.H, [((0.0, 0.0, -2.0), (0.0, 0.0, 0.0))] * len(LOOK_NAMES))          # Camera(): camera.h:14-22
    acc = ctx.render_looks(cams, np.stack([look_record(crt, hs, n) for n in LOOK_NAMES]), 1, at.FRAMES, 1)
    for k, name in enumerate(LOOK_NAMES):
        at.check_render(acc[k], at.FRAMES, flat_sky, "render_looks view %d (%s)" % (k, name), quad=at.look_quad(name), key=name)
    ctx.clear(); ctx.render(1, at.FRAMES, 1)
    at.check_render(ctx.accumulator(), at.FRAMES, flat_sky, "the live look after the job")
    ctx.close()
