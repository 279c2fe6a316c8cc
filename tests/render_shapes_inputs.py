"""The scenes, shapes, transforms and cameras of the crt_render_shapes tests (test_gpu_render_shapes.py on the GPU, test_render_shapes_cpu.py for what it assumes of
the oracle).  A shape of a mesh is `deform` of tests/test_oracle_pinning.py with a factor of its own: p + a_s * (p.yzx * p.zxy), float32 products and sums only;
shape 0 is the uploaded positions.  Scenes: cube_scene.xml, the teapot, a mesh of two triangles whose root is a leaf, and the two-level sets of
tests/tlas_device_inputs.py with one BLAS — never instance 0 — deforming while every instance moves (tests/render_poses_inputs.py `poses`).  Cameras are (position,
target) pairs.  Every shape is small: the tests are about which image a lane walks, not about the picture."""
import os

import numpy as np

import render_poses_inputs as pi
import tlas_device_inputs as inp
from conftest import ASSETS, scene_path
from render_views_inputs import ring
from test_gpu_golden_and_edges import write_scene

W, H = 32, 16                                   # two tiles
F = np.float32
FILE_SCENES = ("cube", "teapot", "tiny")

TINY_OBJ = """v -0.5 -0.5 0.0
v 0.5 -0.5 0.0
v 0.0 0.5 0.2
v 0.1 -0.4 0.5
v 0.9 -0.4 0.5
v 0.5 0.6 0.4
vn 0.0 0.0 -1.0
vt 0.0 0.0
f 1/1/1 2/1/1 3/1/1
f 4/1/1 5/1/1 6/1/1
"""


def scene_xml(tmp_path, scene):
    """(scene file, kind) of `scene`: a FileScene of the cube, the teapot or the two-triangle mesh, or one of tlas_device_inputs' two-level sets"""
    if scene == "cube":
        return scene_path("cube_scene.xml"), 0
    if scene == "teapot":
        return write_scene(tmp_path, "teapot", name="teapot.xml"), 0
    if scene == "tiny":
        obj = tmp_path / "tiny.obj"
        obj.write_text(TINY_OBJ)
        rel = os.path.relpath(str(obj)[:-4], ASSETS)                 # write_scene names a mesh relative to the assets
        return write_scene(tmp_path, rel, name="tiny.xml", pos=(0.0, -0.3, 2.5), rot=(0.0, 0.0, 0.0)), 0
    return inp.scene_xml(tmp_path, scene), 1


def positions(src, bvh):
    """[triCount, 3, 3] float32: the vertices of BVH `bvh` as `src` (a HostScene or an oracle) holds them, the reference's triangle order"""
    t = src.bvh(bvh)["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(F)


def deform_by(p, a):
    p = np.asarray(p, F)
    return (p + F(a) * (p[..., [1, 2, 0]] * p[..., [2, 0, 1]])).astype(F)


def shapes(p0, factors):
    """[S, triCount, 3, 3]: shape s = deform_by(p0, factors[s]); a factor of 0 is p0 itself, bit for bit"""
    return np.stack([np.asarray(p0, F) if a == 0 else deform_by(p0, a) for a in factors])


def factors(count, step):
    out = [step * s for s in range(count)]
    assert len(set(out)) == count and out[0] == 0
    return out


class Case:
    def __init__(self, scene, bvh, pos, T, cameras, view_shape, spp_first, frames, passes):
        self.scene, self.bvh, self.pos, self.T, self.cameras, self.view_shape = scene, bvh, pos, T, cameras, view_shape
        self.spp_first, self.frames, self.passes = spp_first, frames, passes
        assert len(cameras) == (len(pos) if view_shape is None else len(view_shape))
        assert T is None or len(T) == len(pos)

    def shape_of(self, k):
        return k if self.view_shape is None else int(self.view_shape[k])

    def reversed(self):
        """the same job with the shapes (and their views) in the opposite order"""
        assert self.view_shape is None
        return Case(self.scene, self.bvh, self.pos[::-1].copy(), None if self.T is None else self.T[::-1].copy(), self.cameras[::-1], None, self.spp_first, self.frames, self.passes)


def _round(p0, n, total=None):
    """n cameras on a circle round the mesh, far enough to see all of it"""
    lo, hi = p0.reshape(-1, 3).min(0).astype(np.float64), p0.reshape(-1, 3).max(0).astype(np.float64)
    c = (lo + hi) / 2
    return ring(n, (float(c[0]), float(c[1]), float(c[2])), float(max(2.0, 2.5 * (hi - lo).max())), total)


def _in_front(p0, n):
    """n cameras side by side on the -z side of the mesh, looking at its middle (a flat mesh seen face on)"""
    c = (p0.reshape(-1, 3).min(0).astype(np.float64) + p0.reshape(-1, 3).max(0).astype(np.float64)) / 2
    return [((float(c[0]) + 0.4 * k - 0.4, float(c[1]) + 0.3 + 0.05 * k, float(c[2]) - 2.5), (float(c[0]), float(c[1]), float(c[2]))) for k in range(n)]


def _at_instance(T, bvh, view_shape, n):
    """n cameras in front of the scene, camera k looking at where its shape's transforms put the deforming instance"""
    out = []
    for k in range(n):
        t = T[k if view_shape is None else view_shape[k]][bvh, :3, 3].astype(np.float64)
        out.append(((float(t[0]) + 0.25 * k - 0.3, float(t[1]) + 0.9 + 0.05 * k, float(t[2]) - 2.2), (float(t[0]), float(t[1]), float(t[2]))))
    return out


TLAS_BVH = dict(tlas3=2, ring40=1)              # the BLAS that deforms: never instance 0


def case(name, src, passes=None):
    """the named case over the scene `src` (a HostScene or an oracle of scene_xml(case_scene(name))) holds"""
    scene = case_scene(name)
    if scene in FILE_SCENES:
        p0 = positions(src, 0)
        if name in ("cube_loop", "teapot_loop"):        # 1: K = S = 3, a non-zero start, two frames
            return Case(scene, 0, shapes(p0, factors(3, 0.08)), None, _round(p0, 3), None, 5, 2, passes or 1)
        if name == "lanes_69":                          # 2: a shape per lane, one full window and a partial one
            return Case(scene, 0, shapes(p0, factors(69, 0.004)), None, _round(p0, 69), None, 1, 1, 1)
        if name == "windows_48":                        # 3: three views of 48 frames over two shapes: views straddle windows
            return Case(scene, 0, shapes(p0, factors(2, 0.1)), None, _round(p0, 3), [1, 0, 1], 1, 48, 1)
        if name == "stale_node1":                       # 4: shapes that grow far out of the boxes the upload left
            return Case(scene, 0, shapes(p0, [0, 0.35, 0.6]), None, _round(p0, 3), None, 1, 2, 1)
        if name == "leaf_root":
            return Case(scene, 0, shapes(p0, factors(3, 0.3)), None, _in_front(p0, 3), None, 1, 2, 1)
    else:
        bvh = TLAS_BVH[scene]
        p0 = positions(src, bvh)
        if name == "tlas3_loop":                        # 1: the two-level scene, every instance moving, BLAS 2 deforming
            T = pi.poses("tlas3", 3)
            return Case(scene, bvh, shapes(p0, factors(3, 0.15)), T, _at_instance(T, bvh, None, 3), None, 5, 2, passes or 1)
        if name == "tlas3_windows":                     # 3, two-level
            T = pi.poses("tlas3", 2)
            return Case(scene, bvh, shapes(p0, factors(2, 0.2)), T, _at_instance(T, bvh, [1, 0, 1], 3), [1, 0, 1], 1, 48, 1)
        if name == "mixed_heights":                     # 5: a ring pose and a line pose of forty instances
            T = np.stack([inp.transforms("ring40"), pi.line40()])
            return Case(scene, bvh, shapes(p0, factors(2, 0.5)), T, _at_instance(T, bvh, None, 2), None, 1, 2, 1)
        if name == "bad_shape":                         # 8: non-finite positions as shape 1 of 3: BLAS 2's box is NaN, no partner is found
            T = pi.poses("tlas3", 3)
            pos = shapes(p0, factors(3, 0.15)); pos[1] = F(np.nan)
            return Case(scene, bvh, pos, T, _at_instance(T, bvh, None, 3), None, 1, 1, 1)
    raise KeyError(name)


CASE_SCENE = dict(cube_loop="cube", teapot_loop="teapot", lanes_69="cube", windows_48="cube", stale_node1="cube", leaf_root="tiny", tlas3_loop="tlas3", tlas3_windows="tlas3",
                  mixed_heights="ring40", bad_shape="tlas3")
LOOP_CASES = ("cube_loop", "teapot_loop", "tlas3_loop")
ALL_RENDERED = LOOP_CASES + ("lanes_69", "windows_48", "tlas3_windows", "stale_node1", "leaf_root", "mixed_heights")


def case_scene(name):
    return CASE_SCENE[name]


def make_oracle(orc, tmp_path, scene, width=W, height=H):
    xml, kind = scene_xml(tmp_path, scene)
    o, _ = orc.load_scene(xml, kind, ASSETS)
    o.renderer_init(width, height)
    return o


def oracle_shape(o, c, s):
    """shape s of the case on the oracle: move_and_refit of the BVH, then for a two-level scene set_transform for every instance"""
    o.move_and_refit(c.bvh, c.pos[s])
    if c.T is not None:
        for i in range(len(c.T[s])):
            o.set_transform(i, c.T[s][i])


def oracle_view(o, c, k, threads=4):
    """(accumulator, counters) of view k of case c"""
    oracle_shape(o, c, c.shape_of(k))
    o.set_camera_state(*c.cameras[k])
    o.clear(); o.set_spp(c.spp_first); o.set_params(5, c.passes)
    o.reset_counters()
    o.render(c.frames, threads)
    return o.accumulator(), o.counters()
