"""The scenes, poses, cameras and shapes of the crt_render_poses tests (test_gpu_render_poses.py on the GPU, test_render_poses_cpu.py for what it assumes of the
oracle).  Scenes and base transforms are tests/tlas_device_inputs.py's; a further pose is those transforms perturbed by a small rigid motion per instance
(`rigid`), so every pose of a case is a different TLAS over the same BLASes.  Cameras are (position, target) pairs, as in tests/render_views_inputs.py.
Every shape is small: the tests are about which pose a lane walks, not about the image."""
import math

import numpy as np

import tlas_device_inputs as inp
from render_views_inputs import ring, TLAS_CENTRE

W, H = 32, 16                                   # two tiles
F = np.float32


def poses(name, count, spread=0.25):
    """[count, N, 4, 4] float32: pose 0 is transforms(name); pose p > 0 shifts instance i by up to `spread` and turns it where it stands, each by an amount of its own"""
    base = inp.transforms(name)
    out = [base]
    for p in range(1, count):
        T = base.copy()
        for i in range(len(base)):
            a = 0.7 * p + 1.3 * i
            turn = inp.rigid((0.0, 0.0, 0.0), (0.05 * math.sin(a), 0.11 * p + 0.03 * i, 0.0))
            T[i, :3, :3] = (turn[:3, :3].astype(np.float64) @ base[i, :3, :3].astype(np.float64)).astype(F)
            T[i, :3, 3] = base[i, :3, 3] + np.array([spread * math.sin(a), 0.5 * spread * math.cos(1.7 * a), spread * math.cos(a)], F)
        out.append(T)
    return np.stack(out).astype(F)


def same_poses(count):
    """same8: every instance of a pose gets the SAME transform (every area ties in every pose), a different one per pose"""
    return np.stack([np.stack([inp.rigid((0.2 * p, 0.05 * p, 4.0 + 0.1 * p), (0.0, 0.5 + 0.2 * p, 0.0))] * 8) for p in range(count)]).astype(F)


def line40():
    """forty instances along x at growing distances: the agglomeration makes a caterpillar, far taller than the ring's tree"""
    return np.stack([inp.rigid((-1.0 + 1.4 ** i, -0.3, 5.0), (0.0, 0.2 * i, 0.0)) for i in range(40)]).astype(F)


def looking_at(T, n, eye=(0.0, 0.6, -1.0)):
    """n cameras round `eye`, looking at the middle of pose T's first instances"""
    c = T[: min(len(T), 4), :3, 3].astype(np.float64).mean(0)
    return [((eye[0] + 0.3 * k, eye[1] + 0.05 * k, eye[2]), (float(c[0]), float(c[1]), float(c[2]))) for k in range(n)]


class Case:
    def __init__(self, scene, T, cameras, view_pose, spp_first, frames, passes):
        self.scene, self.T, self.cameras, self.view_pose = scene, T, cameras, view_pose
        self.spp_first, self.frames, self.passes = spp_first, frames, passes
        assert len(cameras) == (len(T) if view_pose is None else len(view_pose))

    def pose_of(self, k):
        return k if self.view_pose is None else int(self.view_pose[k])


def _tlas_ring(n, total=None):
    return ring(n, TLAS_CENTRE, 5.0, total)


_T130 = None


def _poses130():
    global _T130
    if _T130 is None:
        _T130 = poses("tlas3", 130, spread=0.35)
    return _T130


def case(name):
    """the named case (built on demand: the scenes are files the caller writes with tlas_device_inputs.scene_xml)"""
    if name == "loop_3":                        # 1: K = P = 3, a non-zero start, two frames, two passes
        return Case("tlas3", poses("tlas3", 3), _tlas_ring(3), None, 5, 2, 2)
    if name == "loop_5_of_2":                   # 1: five views over two poses
        return Case("tlas3", poses("tlas3", 2), _tlas_ring(5), [1, 0, 1, 1, 0], 5, 2, 2)
    if name in ("lanes_64", "lanes_65", "lanes_130"):   # 2: a pose per lane, full and partial windows
        n = int(name.split("_")[1])
        return Case("tlas3", _poses130()[:n], _tlas_ring(n, 130), None, 1, 1, 1)
    if name == "straddle_3":                    # 3: view 21 = view-frames 63..65
        return Case("tlas3", poses("tlas3", 4), _tlas_ring(43), [k % 4 for k in range(43)], 1, 3, 1)
    if name == "mixed_heights":                 # 4: a ring pose and a line pose of forty instances
        T = np.stack([inp.transforms("ring40"), line40()])
        return Case("ring40", T, [looking_at(T[0], 1)[0], looking_at(T[1], 1, eye=(0.5, 0.4, 0.0))[0]], None, 1, 2, 1)
    if name in ("one", "two"):                  # 5: the list extremes
        T = poses(name, 2)
        return Case(name, T, looking_at(T[0], 2), None, 1, 1, 1)
    if name == "same8":
        T = same_poses(2)
        return Case(name, T, looking_at(T[0], 2), None, 1, 1, 1)
    if name == "rand256":
        T = poses(name, 2)
        return Case(name, T, [((0.0, 1.5, -2.0), (0.0, 1.0, 8.0)), ((1.0, 2.0, -2.0), (-0.5, 1.0, 8.0))], None, 1, 1, 1)
    if name == "bad_pose":                      # 6: the NaN set as pose 1 of 3 (the good ones: its instance 5 put somewhere finite, and a perturbation of that)
        nan = inp.transforms("nan")
        good = nan.copy(); good[5] = inp.rigid((0.0, 0.0, 5.0))
        other = good.copy(); other[:, :3, 3] += F(0.2)
        T = np.stack([good, nan, other])
        return Case("nan", T, looking_at(good, 3), None, 1, 1, 1)
    raise KeyError(name)


LOOP_CASES = ("loop_3", "loop_5_of_2")
LANE_CASES = ("lanes_64", "lanes_65", "lanes_130")
EXTREMES = ("one", "two", "same8", "rand256")
ALL_RENDERED = LOOP_CASES + LANE_CASES + ("straddle_3", "mixed_heights") + EXTREMES


def good_views(c):
    """the views of a case whose pose builds (bad_pose: views 0 and 2)"""
    return [k for k in range(len(c.cameras)) if np.isfinite(c.T[c.pose_of(k)]).all()]


def make_oracle(orc, assets, xml, width=W, height=H):
    o, _ = orc.load_scene(xml, 1, assets)
    o.renderer_init(width, height)
    return o


def oracle_view(o, c, k, threads=4):
    """(accumulator, counters) of view k of case c: set_transform for every instance, set_camera_state, render"""
    T = c.T[c.pose_of(k)]
    for i in range(len(T)):
        o.set_transform(i, T[i])
    o.set_camera_state(*c.cameras[k])
    o.clear(); o.set_spp(c.spp_first); o.set_params(5, c.passes)
    o.reset_counters()
    o.render(c.frames, threads)
    return o.accumulator(), o.counters()
