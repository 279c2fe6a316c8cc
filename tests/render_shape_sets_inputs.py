"""The scenes, shape sets, transforms and cameras of the crt_render_shape_sets tests (test_gpu_render_shape_sets.py on the GPU, test_render_shape_sets_cpu.py for what it
assumes of the oracle).  A case names the BLASes of a two-level scene that deform (`bvhs`, in the order the job is given them) and, per BLAS, S shapes of it:
render_shapes_inputs.deform_by with a factor of its own per (shape, mesh), so that sub-images of equal size — the forty cubes of ring40 — cannot be swapped unnoticed.
Every instance moves per shape (render_poses_inputs.poses); cameras look at the deforming instances."""
import os

import numpy as np

import render_poses_inputs as pi
import render_shapes_inputs as si
import tlas_device_inputs as inp
from conftest import ASSETS
from test_gpu_golden_and_edges import write_scene

W, H = si.W, si.H                               # two tiles
F = np.float32
TINY3_AT = ((-1.1, -0.3, 2.5), (0.0, -0.2, 2.9), (1.1, -0.3, 2.5))


def scene_xml(tmp_path, scene):
    """(scene file, kind): tlas_device_inputs' sets, or `tiny3` — three instances of render_shapes_inputs.TINY_OBJ's two-triangle mesh, whose BVH root is a leaf"""
    if scene != "tiny3":
        return inp.scene_xml(tmp_path, scene), 1
    obj = tmp_path / "tiny.obj"
    obj.write_text(si.TINY_OBJ)
    rel = os.path.relpath(str(obj)[:-4], ASSETS)                     # write_scene names a mesh relative to the assets
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    return write_scene(tmp_path, rel, name="tiny3.xml", pos=TINY3_AT[0], rot=zero, extra_objects=[(rel, 0, p, zero, one) for p in TINY3_AT[1:]]), 1


def tiny3_poses(count):
    """[count, 3, 4, 4]: pose 0 is the scene file's; pose p shifts instance i by an amount of its own"""
    return np.stack([np.stack([inp.rigid((x + 0.07 * p * (i - 1), y + 0.05 * p, z + 0.04 * p * i)) for i, (x, y, z) in enumerate(TINY3_AT)]) for p in range(count)]).astype(F)


def make_oracle(orc, tmp_path, scene, width=W, height=H):
    xml, kind = scene_xml(tmp_path, scene)
    o, _ = orc.load_scene(xml, kind, ASSETS)
    o.renderer_init(width, height)
    return o


class Case:
    def __init__(self, scene, bvhs, factors, p0, T, cameras, view_shape, spp_first, frames, passes):
        """factors: [S, M]; p0: the uploaded positions of bvhs[m], per m.  pos[m] = [S, triCount_m, 3, 3]"""
        self.scene, self.bvhs, self.factors, self.p0, self.T, self.cameras, self.view_shape = scene, list(bvhs), np.asarray(factors, np.float64), p0, T, cameras, view_shape
        self.spp_first, self.frames, self.passes = spp_first, frames, passes
        S, M = self.factors.shape
        assert M == len(self.bvhs) == len(p0) and len(set(self.bvhs)) == M and len(T) == S
        assert len(set(self.factors.reshape(-1).tolist())) == S * M          # a factor of its own per (shape, mesh)
        assert len(cameras) == (S if view_shape is None else len(view_shape))
        self.pos = [np.stack([si.deform_by(p0[m], self.factors[s, m]) for s in range(S)]) for m in range(M)]

    def shape_of(self, k):
        return k if self.view_shape is None else int(self.view_shape[k])

    def set_positions(self):
        """[S, setTris, 9]: per shape the BVHs' blocks in the order of bvhs — what the C entry takes"""
        return np.ascontiguousarray(np.concatenate([p.reshape(p.shape[0], p.shape[1], 9) for p in self.pos], axis=1))

    def with_factors(self, factors):
        return Case(self.scene, self.bvhs, factors, self.p0, self.T, self.cameras, self.view_shape, self.spp_first, self.frames, self.passes)

    def reversed(self):
        """the same job with the shapes (and their views) in the opposite order"""
        assert self.view_shape is None
        return Case(self.scene, self.bvhs, self.factors[::-1], self.p0, self.T[::-1].copy(), self.cameras[::-1], None, self.spp_first, self.frames, self.passes)


def _at_set(T, bvhs, view_shape, n, back=2.6, up=0.9):
    """n cameras in front of the scene, camera k looking at the middle of where its shape's transforms put the deforming instances"""
    out = []
    for k in range(n):
        t = T[k if view_shape is None else view_shape[k]][list(bvhs), :3, 3].astype(np.float64).mean(0)
        out.append(((float(t[0]) + 0.25 * (k % 7) - 0.3, float(t[1]) + up + 0.05 * (k % 5) + 0.01 * (k // 7), float(t[2]) - back), (float(t[0]), float(t[1]), float(t[2]))))
    return out


def _grid(S, M, first, step):
    """[S, M] factors, every one different"""
    return first + step * np.arange(S * M, dtype=np.float64).reshape(S, M)


RING5 = [7, 5, 9, 6, 8]                         # five neighbours of the ring, in no order
RING_ALL = list(range(20, 40)) + list(range(20))
CASE_SCENE = dict(tlas3_two="tlas3", tlas3_all="tlas3", ring40_five="ring40", ring40_all="ring40", windows_48="tlas3", stale_node1="tlas3", leaf_root="tiny3", bad_mesh="tlas3")
LOOP_CASES = ("tlas3_two", "tlas3_all")
ALL_RENDERED = LOOP_CASES + ("ring40_five", "ring40_all", "windows_48", "stale_node1", "leaf_root")
CASE_BVHS = dict(tlas3_two=[0, 2], tlas3_all=[2, 0, 1], ring40_five=RING5, ring40_all=RING_ALL, windows_48=[1, 2], stale_node1=[0, 2], leaf_root=[2, 0], bad_mesh=[0, 2])


def case_scene(name):
    return CASE_SCENE[name]


def case(name, src, passes=None):
    """the named case over the scene `src` (a HostScene or an oracle of scene_xml(case_scene(name))) holds"""
    scene, bvhs = CASE_SCENE[name], CASE_BVHS[name]
    p0 = [si.positions(src, b) for b in bvhs]
    M = len(bvhs)
    if name in ("tlas3_two", "tlas3_all"):              # the loop cases: K = S = 3, a non-zero start, two frames; tlas3_two lets instance 0 deform
        T = pi.poses("tlas3", 3)
        return Case(scene, bvhs, _grid(3, M, 0.05, 0.04), p0, T, _at_set(T, bvhs, None, 3), None, 5, 2, passes or 1)
    if name == "ring40_five":                           # a shape per lane: one full window and a partial one
        T = pi.poses("ring40", 69)
        return Case(scene, bvhs, _grid(69, M, 0.05, 0.002), p0, T, _at_set(T, bvhs, None, 69, back=2.2, up=0.7), None, 1, 1, 1)
    if name == "ring40_all":                            # every BLAS deforms; a ring pose and a line pose (TLASes of different heights)
        T = np.stack([inp.transforms("ring40"), pi.line40()])
        cams = [((0.0, 7.5, 4.0), (0.0, -0.2, 4.5)), ((0.4, 1.2, 0.8), (1.2, -0.3, 5.0))]
        return Case(scene, bvhs, _grid(2, M, 0.3, 0.008), p0, T, cams, None, 1, 2, 1)
    if name == "windows_48":                            # three views of 48 frames over two shapes: views straddle windows
        T = pi.poses("tlas3", 2)
        return Case(scene, bvhs, _grid(2, M, 0.1, 0.07), p0, T, _at_set(T, bvhs, [1, 0, 1], 3), [1, 0, 1], 1, 48, 1)
    if name == "stale_node1":                           # both meshes grow far out of the node-1 boxes the upload left
        T = pi.poses("tlas3", 3)
        return Case(scene, bvhs, [[0.35, 0.4], [0.6, 0.5], [0.8, 0.7]], p0, T, _at_set(T, bvhs, None, 3, back=3.2), None, 1, 2, 1)
    if name == "leaf_root":                             # the root of both deforming BVHs is a leaf: no node pair at all
        T = tiny3_poses(3)
        return Case(scene, bvhs, _grid(3, M, 0.2, 0.15), p0, T, _at_set(T, bvhs, None, 3, back=2.5, up=0.3), None, 1, 2, 1)
    if name == "bad_mesh":                              # non-finite positions in ONE mesh (the second of the set) of shape 1 of 3
        T = pi.poses("tlas3", 3)
        c = Case(scene, bvhs, _grid(3, M, 0.05, 0.04), p0, T, _at_set(T, bvhs, None, 3), None, 1, 1, 1)
        c.pos[1][1] = F(np.nan)
        return c
    raise KeyError(name)


def oracle_shape(o, c, s, only=None):
    """shape s of the case on the oracle: move_and_refit of every BVH of the set (only: of that one; the others at their uploaded positions), then set_transform"""
    for m, b in enumerate(c.bvhs):
        o.move_and_refit(b, c.pos[m][s] if only is None or only == m else c.p0[m])
    for i in range(len(c.T[s])):
        o.set_transform(i, c.T[s][i])


def oracle_view(o, c, k, threads=4, shape=None, only=None):
    """(accumulator, counters) of view k of case c (shape: under that shape instead of its own)"""
    oracle_shape(o, c, c.shape_of(k) if shape is None else shape, only)
    o.set_camera_state(*c.cameras[k])
    o.clear(); o.set_spp(c.spp_first); o.set_params(5, c.passes)
    o.reset_counters()
    o.render(c.frames, threads)
    return o.accumulator(), o.counters()
