"""Inputs of the crt_update_transforms_device tests, and a numpy restatement of the build as the kernel does it (device/tlas_build.hip): SetTransform per BLAS,
then TLASBVH::Build (tlas_bvh.cpp:17-70) with FindBestMatch as an argmin over a fixed-size open list.

Every set is a scene of cubes (12 triangles each, so loading stays cheap) plus the transforms the test moves its instances to; `tlas3` is tlas_scene.xml.
    one, two        the smallest lists: node 0 is the leaf's copy / a single merge
    tlas3           tlas_scene.xml, its three BLAS moved
    ring40          forty instances in a ring, every one moved and rotated
    lattice64       4 x 4 x 4 identical cubes (corners at +-0.25) at integer translations: merged areas tie exactly
    same8           eight identical transforms: every area ties
    rand256         the maximum, random placement   } both reach the case where A, the last entry, lies outside the shortened list
    line256         the maximum, along a line       }
    nan             one transform with a NaN translation: a FindBestMatch call without a candidate while more than one node is open
"""
import math

import numpy as np

from conftest import scene_path
from test_gpu_golden_and_edges import write_scene

SETS = ("one", "two", "tlas3", "ring40", "lattice64", "same8", "rand256", "line256", "nan")
COUNT = dict(one=1, two=2, tlas3=3, ring40=40, lattice64=64, same8=8, rand256=256, line256=256, nan=8)
TLAS_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("leftRight", "<u4"), ("aabbMax", "<f4", 3), ("BLAS", "<u4")])
F = np.float32


def scene_xml(tmp_path, name):
    """the scene file of set `name`: COUNT[name] cubes in a ring in front of the camera (the transforms the scene starts with; the tests move them)"""
    if name == "tlas3":
        return scene_path("tlas_scene.xml")
    n = COUNT[name]
    s = 0.25 if name in ("lattice64", "same8") else 0.3            # 0.25: the cube's corners are exact in float32 and stay so at integer translations

    def place(i):
        a = 2 * math.pi * i / max(n, 1)
        r = 2.5 + 0.5 * (i % 3)
        return ("cube", 0, (round(r * math.sin(a), 3), round(-0.5 + 0.3 * (i % 4), 3), round(4.0 + r * math.cos(a), 3)), (0.0, round(37.0 * i % 360, 1), 0.0), (s, s, s))
    first = place(0)
    return write_scene(tmp_path, "cube", name=name + ".xml", pos=first[2], rot=first[3], scale=first[4], extra_objects=[place(i) for i in range(1, n)])


def rigid(pos, angles=(0.0, 0.0, 0.0)):
    """Translate * RotateY * RotateX * RotateZ as a row-major float32 mat4 (no scale)"""
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ rz
    m[:3, 3] = pos
    return m.astype(F)


def transforms(name):
    """the (N, 4, 4) float32 transforms of set `name`"""
    n = COUNT[name]
    rng = np.random.default_rng(1000 + SETS.index(name))
    if name == "one":
        T = [rigid((0.3, -0.2, 4.0), (0.2, 0.7, 0.1))]
    elif name == "two":
        T = [rigid((-0.8, -0.3, 4.0), (0.0, 0.5, 0.0)), rigid((0.9, 0.2, 5.0), (0.3, -0.4, 0.2))]
    elif name == "tlas3":
        T = [rigid((-1.2, -1.0, 3.5), (0.0, 0.9, 0.0)), rigid((0.6, -1.0, 5.0), (0.0, 2.8, 0.0)), rigid((1.1, -0.8, 2.6), (0.1, -1.0, 0.05))]
    elif name == "ring40":
        T = [rigid((2.8 * math.sin(2 * math.pi * i / 40 + 0.3), -0.4 + 0.25 * (i % 5), 4.5 + 2.8 * math.cos(2 * math.pi * i / 40 + 0.3)), (0.1 * (i % 7), 0.37 * i, 0.05 * (i % 3)))
             for i in range(40)]
    elif name == "lattice64":
        T = [rigid((x - 2.0, y - 1.0, z + 4.0)) for z in range(4) for y in range(4) for x in range(4)]
    elif name == "same8":
        T = [rigid((0.0, 0.0, 4.0), (0.0, 0.5, 0.0))] * 8
    elif name == "rand256":
        T = [rigid((rng.uniform(-5, 5), rng.uniform(-0.8, 3.0), rng.uniform(3, 13)), tuple(rng.uniform(-3, 3, 3))) for _ in range(256)]
    elif name == "line256":
        T = [rigid((-8.0 + 0.0625 * i + 0.01 * math.sin(1.7 * i), 0.3 * math.sin(0.4 * i), 6.0 + 0.02 * i), (0.0, 0.11 * i, 0.0)) for i in range(256)]
    else:                                                           # nan
        T = [rigid((rng.uniform(-2, 2), rng.uniform(-0.5, 1.0), rng.uniform(3, 7)), tuple(rng.uniform(-3, 3, 3))) for _ in range(8)]
        T[5][0, 3] = np.nan
    T = np.stack(T).astype(F)
    assert T.shape == (n, 4, 4)
    return T


def aimed_rays(T, n=2000, seed=3):
    """n rays from in front of the scene towards the instances' origins (jittered, so that some miss)"""
    rng = np.random.default_rng(seed)
    centres = np.nan_to_num(T[:, :3, 3].astype(np.float64))
    tgt = centres[rng.integers(0, len(centres), n)] + rng.uniform(-0.35, 0.35, (n, 3))
    O = np.array([0.0, 0.6, -1.0]) + rng.uniform(-0.3, 0.3, (n, 3))
    D = tgt - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return O.astype(F), D.astype(F)


def _lesser(a, b):
    return np.where(a < b, a, b)        # tmplmath.h:122: a < b ? a : b


def _greater(a, b):
    return np.where(a > b, a, b)


def set_transform(boxes, T):
    """BLASBVH::SetTransform for every BLAS (blas_bvh.cpp:363-374): boxes = (N, 2, 3) node-0 boxes, T = (N, 4, 4).  Returns (invT (N, 16), world boxes (N, 2, 3)), float32
    operation for operation."""
    T = np.ascontiguousarray(T, F).reshape(-1, 16)
    n = len(T)
    with np.errstate(all="ignore"):
        inv = np.zeros((n, 16), F)
        inv[:, 15] = 1
        for r in range(3):
            for c in range(3):
                inv[:, 4 * r + c] = T[:, 4 * c + r]
        for r in range(3):
            inv[:, 4 * r + 3] = -((T[:, 3] * inv[:, 4 * r] + T[:, 7] * inv[:, 4 * r + 1]) + T[:, 11] * inv[:, 4 * r + 2])
        lo = np.full((n, 3), 1e34, F)
        hi = np.full((n, 3), -1e34, F)
        boxes = np.asarray(boxes, F)
        for i in range(8):
            c = [boxes[:, 1 if i & (1 << k) else 0, k] for k in range(3)]
            for k in range(3):
                p = ((T[:, 4 * k] * c[0] + T[:, 4 * k + 1] * c[1]) + T[:, 4 * k + 2] * c[2]) + T[:, 4 * k + 3] * F(1.0)
                lo[:, k] = _lesser(lo[:, k], p)
                hi[:, k] = _greater(hi[:, k], p)
    return inv, np.stack([lo, hi], axis=1)


def build(world):
    """TLASBVH::Build over world = (N, 2, 3) instance boxes, as the kernel does it.  Returns dict(nodes (2N TLAS_DTYPE records, the reference layout), height,
    searches, stale_a (merges after which A lay outside the list), ties (searches whose smallest area was reached by more than one candidate), no_candidate (the
    FindBestMatch call, counted from 1, that found nobody while more than one node was open; None if there was none: then nodes is complete))."""
    n = len(world)
    lo = np.zeros((2 * n, 3), F)
    hi = np.zeros((2 * n, 3), F)
    lr = np.zeros(2 * n, np.uint32)
    blas = np.zeros(2 * n, np.uint32)
    height = np.zeros(2 * n, np.int64)
    lo[1:n + 1], hi[1:n + 1] = world[:, 0], world[:, 1]
    blas[1:n + 1] = np.arange(n)
    lst = np.zeros(256, np.int64)                                  # the fixed-size list: entries past `open` keep what they held
    lst[:n] = np.arange(1, n + 1)
    stats = dict(searches=0, stale_a=0, ties=0, no_candidate=None)
    open_ = n

    def partner(A):
        stats["searches"] += 1
        B = np.arange(open_)
        B = B[B != A]
        ia, ib = lst[A], lst[B]
        with np.errstate(all="ignore"):
            e = _greater(hi[ia], hi[ib]) - _lesser(lo[ia], lo[ib])
            area = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
            ok = area < F(1e30)                                    # a NaN area is never below the running minimum
        if not ok.any():
            if open_ > 1 and stats["no_candidate"] is None:
                stats["no_candidate"] = stats["searches"]
            return -1
        cand, a = B[ok], area[ok]
        if (a == a.min()).sum() > 1:
            stats["ties"] += 1
        return int(cand[np.argmin(a)])                             # the lowest list index among the candidates of smallest area

    used, A = n + 1, 0
    B = partner(A)
    while open_ > 1 and stats["no_candidate"] is None:
        C = partner(B)
        if C < 0:
            break
        if A != C:
            A, B = B, C
            continue
        ia, ib = lst[A], lst[B]
        lo[used], hi[used] = _lesser(lo[ia], lo[ib]), _greater(hi[ia], hi[ib])
        lr[used] = ia + (ib << 16)
        height[used] = max(height[ia], height[ib]) + 1
        lst[A] = used
        lst[B] = lst[open_ - 1]
        if A == open_ - 1:
            stats["stale_a"] += 1
        used += 1
        open_ -= 1
        B = partner(A)
    nodes = np.zeros(2 * n, TLAS_DTYPE)
    if stats["no_candidate"] is None:
        root = lst[A]
        lo[0], hi[0], lr[0], blas[0], height[0] = lo[root], hi[root], lr[root], blas[root], height[root]
        nodes["aabbMin"], nodes["aabbMax"], nodes["leftRight"], nodes["BLAS"] = lo, hi, lr, blas
    return dict(nodes=nodes, height=int(height[0]), **stats)


def restate(boxes, T):
    """SetTransform for every BLAS + Build: dict(invT, world, nodes, height, searches, stale_a, ties, no_candidate)"""
    inv, world = set_transform(boxes, T)
    return dict(invT=inv, world=world, **build(world))
