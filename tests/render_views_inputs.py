"""The cameras, shapes and worlds of the crt_render_views tests (test_gpu_render_views.py on the GPU, test_render_views_cpu.py for what it assumes of the oracle).
Cameras are (position, target) pairs: both sides turn them into the reference Camera with set_camera_state.  Every shape is small: the tests are about where a
view-frame lands — which window, which lane, which view's sum — not about the image."""
import math

W, H = 32, 16                                   # two tiles
CUBE_CENTRE, TLAS_CENTRE = (0.0, 0.0, 3.0), (0.0, -0.3, 3.3)


def ring(n, centre=CUBE_CENTRE, radius=4.0, total=None):
    """camera k of `total` on a circle round `centre`, each a little higher than the one before: no two alike, all looking at the mesh"""
    total = n if total is None else total
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / total
        out.append(((centre[0] + radius * math.cos(a), centre[1] + 0.4 + 0.01 * k, centre[2] + radius * math.sin(a)), centre))
    return out


def prim_cameras(n):
    """inside PrimitiveScene's room, round the default camera position, looking at the objects"""
    return [((0.5 * math.cos(1.1 * k), 0.2 * math.sin(0.7 * k), -2.0 + 0.1 * k), (0.0, 0.3, 2.0)) for k in range(n)]


# name -> (cameras, spp_first, frames, passes): the cube through its BVH, 32 x 16
CASES = {
    "identity": (ring(1), 1, 1, 1),
    "start_and_passes": (ring(3), 5, 2, 2),                              # a non-zero start and the pass order
    "lanes_64": (ring(64, total=130), 1, 1, 1),                          # one full window, a camera per lane
    "lanes_65": (ring(65, total=130), 1, 1, 1),                          # ... and a last window of one lane
    "lanes_130": (ring(130), 1, 1, 1),                                   # two windows and a bit
    "straddle_3": (ring(43), 1, 3, 1),                                   # view 21 = view-frames 63..65, view 42 = 126..128: windows 0|1 and 1|2
    "straddle_70": (ring(2), 1, 70, 1),                                  # a view longer than a window
}

# case 6: every world at K = 3, frames = 2
WORLDS = ("bvh", "tlas", "kd", "grid", "tlas_kd", "prim")
WORLD_SHAPE = (1, 2, 1)                                                  # spp_first, frames, passes


def world_cameras(world):
    if world == "prim":
        return prim_cameras(3)
    return ring(3, TLAS_CENTRE, 5.0) if world.startswith("tlas") else ring(3)


def scene_of(world):
    """(scene file or None for the PrimitiveScene, kind)"""
    if world == "prim":
        return None, 0
    return ("tlas_scene.xml", 1) if world.startswith("tlas") else ("cube_scene.xml", 0)


def make_oracle(orc, assets, scene_path, world, width=W, height=H):
    """the oracle of a world, its renderer initialised; the alternative structures stay referenced from the returned object"""
    xml, kind = scene_of(world)
    if xml is None:
        o = orc.primitive_scene(assets, 0.0)
    else:
        o, _ = orc.load_scene(scene_path(xml), kind, assets)
        if world in ("kd", "grid"):
            o._views_acc = orc.alt_accel(world, o.bvh(0)["tris"]); orc.set_render_accel(o, o._views_acc)
        if world == "tlas_kd":
            orc.set_blas_accel(o, orc.blas_accels(o, "kd"))
    o.renderer_init(width, height)
    return o


def oracle_view(o, camera, spp_first, frames, passes, threads=4):
    """(accumulator, counters) of one view: set_camera_state, set_spp, set_params, render"""
    o.set_camera_state(*camera)
    o.clear(); o.set_spp(spp_first); o.set_params(5, passes)
    o.reset_counters()
    o.render(frames, threads)
    return o.accumulator(), o.counters()
