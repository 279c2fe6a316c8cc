"""Rays that drive every LDS traversal stack to the last entry the library allots, the scenes they need, and float32 restatements of the reference's walks that
also report how many stack entries a ray holds.  Shared by tests/test_stack_fill_cpu.py (the criterion, settled on the oracle) and tests/test_gpu_stack_fill.py
(every kernel that owns a stack, at its bound).  Not collected by pytest.

THE GAP.  crt_upload_scene allots bvhStack = the tallest BVH's height and stackDepth = bvhStack + TLAS height + 1 return marker, with no slack, and every walking
kernel keeps live data right behind the last entry.  The shipped scenes' rays stay far below that: measured with the walks below, the default camera's 64 x 64
primary rays on bunny_scene.xml (height 15, 15 entries allotted) hold at most 6 entries, and 1200 rays aimed from a sphere at the centres of its eight deepest
leaves at most 11.  (Recorded, not asserted.)

THE SCENES.  A ray that descends near-child-first to the deepest leaf without visiting a leaf on the way still has t = 1e30 when it gets there, so the sibling at
every level was pushed: height entries.  Triangle i of the meshes lies in the plane x = X[i] with vertices (x, 0, 0) (x, 0, .5) (x, 1, 1); a ray along +x through
(y, z) with z outside [y, .5 + .5 y] is inside every box and misses every triangle.
  chain      bvh_build_inputs.chain(): 24 triangles at x = 8^i, height 18                         FileScene through upload_desc
  deep       20 triangles at x = 2^i, height 8 (tests/golden/stack_deep.obj)                      FileScene, and the BLAS of `tlas_deep`
  compact    20 triangles at x = 2^-i, height 8 (tests/golden/stack_compact.obj)                  FileScene, and the BLAS of `tlas_compact`
  tlas_deep     seven instances of `deep` at x = 0 and 2^21 * 4^i: the TLAS is a chain of height 6; 8 + 6 + 1 = 15 entries.  tlas_deep_flat: the same
                instances on a 4 x 2 lattice in y, z (TLAS height 3), the placement update_transforms_device moves the line from and back to
  tlas_compact  seven instances of `compact` at x = 0, 1.1, 2.24, 3.436, 4.7104, 6.0946, 7.6324: TLAS height 3, 12 entries; small enough for a camera

OCCUPANCY.  The walks count `held`, the entries on the stack after a push, as the render kernels lay a two-level walk out in one column: the TLAS entries pending
when an instance is entered, plus 1 for the return marker, plus the BLAS walk's own entries.  The query kernels (find_nearest_seq, tlas_walk) keep the TLAS entries
in a part of their own above the bvhStack BLAS entries and push no marker: `blas_held` and `tlas_held` are the two parts.  The device's highest WRITTEN slot is
what matters for an out-of-range store, and the kernels differ from the reference in two ways:
  * the tiles and the pool kernel store the far child at slot `sp` BEFORE the push is decided (a dead store unless it is pushed).  At every interior node the slot
    behind the entries held is therefore written: `written` = max over interior visits of (entries held + 1), which is >= held.  At an interior node of depth d
    at most d entries of its own tree are held, and d <= height - 1, so written <= the allotted number; a ray that holds `allotted` entries has written exactly
    that slot by a push, and `written == held == allotted`.
  * the pool kernel takes a primary ray's first step from the root's child pair in its kernel arguments and stores the far root child at entry 1 (dead unless
    hit): the same slot the walk from the root reference writes, so the occupancy is the same with and without CRT_DEBUG_NO_ROOTPAIR.
For the sequential kernels (no dead store) the highest written slot is `held` itself.  The KD walks push (far child, plane distance) pairs only where both
children are visited; the library allots height + 1 such entries (kdStack), and at most height can be pending (one per interior node of a root-to-leaf path).

SENSITIVITY.  `lost=N` walks as a device would whose store into entry N (counted as above) falls outside its allocation: LDS drops the store and the later load
returns 0, i.e. node 0, which is walked again before the entry below is popped.  (A push made while that happens lands at or above entry N and is lost alike; the
walk is cut off after LOST_LIMIT times the steps of the honest one and then counts as changed.)

ALLOTTED.  allotted(ctx, accel) reads stackDepth and bvhStack from crt_debug_geometry's words.  Nothing reads the KD sizing back, so kdStack is derived as the
library derives it: the tallest live KD-tree's height (Context.get_kdtree) + 1.
"""
import os

import numpy as np

import bvh_build_inputs as B
import tlas_alt_restate as R
from conftest import GOLDEN

f32 = np.float32
MISS = f32(1e30)
LOST_LIMIT = 8
N_TRI = 20
MIN_FILLING = 16


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# meshes and scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def plane_mesh(xs):
    return np.array([[[x, 0, 0], [x, 0, 0.5], [x, 1, 1]] for x in xs], np.float32)


def mesh(name):
    if name == "chain":
        return B.chain()
    return plane_mesh([2.0 ** i for i in range(N_TRI)] if name == "deep" else [2.0 ** -i for i in range(N_TRI)])


def obj_text(p):
    """the mesh as an OBJ: three `v` lines per triangle (every coordinate is a dyadic number, written out in full), one normal, one uv"""
    v = "".join("v %s %s %s\n" % tuple(("%.25f" % float(c)).rstrip("0").rstrip(".") for c in corner) for tri in p for corner in tri)
    f = "".join("f %d/1/1 %d/1/1 %d/1/1\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(len(p)))
    return "# generated by tests/stack_fill.py\n" + v + "vn 0 0 -1\nvt 0 0\n" + f


def obj_model(name):
    """the `mesh` argument of write_scene (a path below assets/, without .obj) for tests/golden/stack_<name>.obj"""
    return "../tests/golden/stack_" + name


def obj_path(name):
    return os.path.join(GOLDEN, "stack_%s.obj" % name)


DEEP_X = [0.0] + [2.0 ** 21 * 4.0 ** i for i in range(6)]
COMPACT_X = [0.0, 1.1, 2.24, 3.436, 4.7104, 6.0946, 7.6324]
FLAT_YZ = [(0.0, 0.0), (2.0, 0.0), (4.0, 0.0), (6.0, 0.0), (0.0, 2.0), (2.0, 2.0), (4.0, 2.0)]
LIGHT = (0.0, 3.0, 1.0)


def write_file_scene(tmp_path, write_scene, name):
    """`deep` / `compact` as a FileScene under the identity"""
    return write_scene(tmp_path, obj_model(name), name="stack_%s.xml" % name, pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0), light=LIGHT)


def write_tlas_scene(tmp_path, write_scene, name):
    """seven instances of the mesh, all at the origin in the file; transforms(name) places them"""
    m = obj_model(name.split("_")[1])
    ob = [(m, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))] * 6
    return write_scene(tmp_path, m, name="stack_%s.xml" % name, pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0), extra_objects=ob, light=LIGHT)


def transforms(name):
    """float32 row-major mat4 translations of the seven instances: tlas_deep, tlas_deep_flat, tlas_compact"""
    out = np.tile(np.eye(4, dtype=np.float32), (7, 1, 1))
    if name == "tlas_deep_flat":
        for i, (y, z) in enumerate(FLAT_YZ):
            out[i, 1, 3], out[i, 2, 3] = y, z
    else:
        out[:, 0, 3] = np.array(DEEP_X if name == "tlas_deep" else COMPACT_X, np.float32)
    return out


def place(scene, name):
    """set_transform as mesh_truth.generated_transforms' users do (the oracle's scene and the host front's alike)"""
    for i, T in enumerate(transforms(name)):
        scene.set_transform(i, T)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _outside(rng, n, lo=0.05, hi=0.95):
    """(y, z) in the unit square, clear of the triangle z in [y, .5 + .5 y] by 0.04 and of the box faces"""
    out = []
    while len(out) < n:
        y, z = rng.uniform(lo, hi, 2)
        if z < y - 0.04 or z > 0.54 + 0.5 * y:
            out.append((y, z))
    return np.array(out)


def axis_rays(n, seed, tilt, x0=-3.0, lo=0.05, hi=0.95):
    """n rays from x = x0 along +x that pass inside every box and miss every triangle; the first two are the issue's (.9, .1) and (.6, .5); D's y and z are random in
    [-tilt, tilt] before D is normalised (Sample and Trace want unit directions), never zero"""
    rng = np.random.default_rng(seed)
    yz = _outside(rng, n, lo, hi); yz[0] = (0.9, 0.1); yz[1] = (0.6, 0.5)
    O = np.stack([np.full(n, x0), yz[:, 0], yz[:, 1]], 1).astype(np.float32)
    d = rng.uniform(-1.0, 1.0, (n, 2)) * tilt
    d = np.where(d == 0, tilt, d)
    D = np.stack([np.ones(n), d[:, 0], d[:, 1]], 1)
    return O, (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)


def short_rays(n, seed=9):
    """rays whose walk ends at the root and holds nothing, so that a lane takes its next ray while its neighbour holds a full stack: from the filling rays'
    origins away from the meshes (-x: the sky), down onto the floor, and up towards the light"""
    O, _ = axis_rays(n, seed, 1e-3)
    D = np.tile(np.float64([[-1, 0.01, 0.02], [0.01, -1, 0.02], [-0.3, 1, 0.1]]), (n // 3 + 1, 1))[:n]
    return O, (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)


FILL = {"chain": dict(tilt=1e-24, x0=-1.0), "deep": dict(tilt=1e-13), "compact": dict(tilt=1e-3),
        "tlas_deep": dict(tilt=1e-13), "tlas_compact": dict(tilt=0.02, lo=0.3, hi=0.7)}


def fill_rays(name, n=64, seed=7):
    """the candidate stack-filling rays of a world"""
    k = dict(FILL[name]); tilt = k.pop("tilt")
    return axis_rays(n, seed, tilt, **k)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the restated walks
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Occ:
    """what a walk reports beside the hit: see OCCUPANCY in the module's head"""

    def __init__(self):
        self.held = self.written = self.blas_held = self.tlas_held = self.kd_held = 0
        self.steps = 0
        self.cut = False

    def push(self, base, own):
        self.held = max(self.held, base + own)

    def interior(self, base, own):
        self.written = max(self.written, base + own + 1)


class Cut(Exception):
    pass


class Bvh:
    """one BVH / BLASBVH from the oracle's arrays: nodes, triangleIndices, Tri records; obj = the BLAS's objIdx (None: Tri::objIdx)"""

    def __init__(self, b, obj=None, invT=None):
        n = b["nodes"]
        self.lo = [tuple(f32(x) for x in r) for r in n["aabbMin"]]; self.hi = [tuple(f32(x) for x in r) for r in n["aabbMax"]]
        self.leftFirst = [int(x) for x in n["leftFirst"]]; self.triCount = [int(x) for x in n["triCount"]]
        self.idx = [int(x) for x in b["triIndices"]]
        t = b["tris"]
        self.tris = [tuple(tuple(f32(x) for x in r[k]) for k in ("vertex0", "vertex1", "vertex2")) for r in t]
        self.objs = [int(x) for x in t["objIdx"]] if obj is None else [int(obj)] * len(t)
        self.invT = None if invT is None else [[f32(x) for x in np.asarray(invT, np.float32).reshape(4, 4)[r]] for r in range(3)]
        d = B.depths(n[:b["nodesUsed"]])
        self.height = int(d.max())

    def walk(self, ray, occ, base=0, stop=False, lost=None, limit=None):
        """BVH::Intersect, infra/bvh.cpp:224-258: near child first, the far child pushed if it is hit.  stop: the occlusion form, which ends at the first hit.
        Returns True if it stopped."""
        node = 0; stack = []
        while True:
            ray.traversed += 1; occ.steps += 1
            if limit is not None and occ.steps > limit:
                raise Cut()
            if self.triCount[node] > 0:
                for i in range(self.triCount[node]):
                    ti = self.idx[self.leftFirst[node] + i]
                    ray.tested += 1
                    R._tri(ray, self.tris[ti], ti, self.objs[ti])
                    if stop and ray.objIdx > -1:
                        return True
                if not stack:
                    return False
                node = stack.pop(); continue
            occ.interior(base, len(stack))
            c1, c2 = self.leftFirst[node], self.leftFirst[node] + 1
            h1, t1, _ = R._aabb(ray, self.lo[c1], self.hi[c1]); h2, t2, _ = R._aabb(ray, self.lo[c2], self.hi[c2])
            d1 = t1 if h1 else MISS; d2 = t2 if h2 else MISS
            if d1 > d2:
                d1, d2, c1, c2 = d2, d1, c2, c1
            if d1 == MISS:
                if not stack:
                    return False
                node = stack.pop()
            else:
                node = c1
                if d2 != MISS:
                    stack.append(0 if (lost is not None and base + len(stack) + 1 >= lost) else c2)
                    occ.push(base, len(stack)); occ.blas_held = max(occ.blas_held, len(stack))


def object_ray(ray, M):
    """BLASBVH::Intersect's transform (blas_bvh.cpp:376-381; TransformPosition_SSE / TransformVector_SSE: (x + y) + (z + w) / (x + y) + z), Ray(const Ray&)"""
    O, D = ray.O, ray.D
    Oo = tuple((O[0] * M[r][0] + O[1] * M[r][1]) + (O[2] * M[r][2] + f32(1) * M[r][3]) for r in range(3))
    Do = tuple((D[0] * M[r][0] + D[1] * M[r][1]) + D[2] * M[r][2] for r in range(3))
    tr = R.Ray(Oo, Do, ray.t)
    tr.objIdx, tr.triIdx, tr.u, tr.v, tr.traversed, tr.tested = ray.objIdx, ray.triIdx, ray.u, ray.v, ray.traversed, ray.tested
    return tr


def _back(ray, tr):
    ray.t, ray.objIdx, ray.triIdx, ray.u, ray.v, ray.traversed, ray.tested = tr.t, tr.objIdx, tr.triIdx, tr.u, tr.v, tr.traversed, tr.tested


class Kd:
    """one KDTree / BLASKDTree from the oracle's dump"""

    def __init__(self, dump, tris, obj=None, invT=None):
        self.n = [dict(lo=tuple(f32(x) for x in n["aabbMin"]), hi=tuple(f32(x) for x in n["aabbMax"]), left=int(n["left"]), right=int(n["right"]),
                       split=f32(n["splitDistance"]), axis=int(n["splitAxis"]), first=int(n["firstTri"]), count=int(n["triCount"])) for n in dump["nodes"]]
        self.refs = [int(r) for r in dump["refs"]]
        self.tris = [tuple(tuple(f32(x) for x in r[k]) for k in ("vertex0", "vertex1", "vertex2")) for r in tris]
        self.objs = [int(x) for x in tris["objIdx"]]
        self.obj = None if obj is None else int(obj)
        self.invT = None if invT is None else [[f32(x) for x in np.asarray(invT, np.float32).reshape(4, 4)[r]] for r in range(3)]
        self.height = self._height(0)

    def _height(self, i):
        n = self.n[i]
        return 0 if n["left"] < 0 else 1 + max(self._height(n["left"]), self._height(n["right"]))

    def walk(self, ray, occ, tlas_pending=0, stop=False):
        """KDTree::IntersectKDTree (infra/kdtree.cpp:143-202) / BLASKDTree::IntersectKDTree (blas_kdtree.cpp:336-398, rule 1 when self.obj is set), the recursion
        as the device's stack of (far child, plane distance): an entry per frame that visits both children, the caller's `if (ray.t < t) return` at pop time"""
        node = 0; stack = []
        while True:
            descend = False
            ray.traversed += 1
            nd = self.n[node]
            hit, tmin, tmax = R._aabb(ray, nd["lo"], nd["hi"])
            if hit:
                if nd["left"] < 0:
                    for k in range(nd["count"]):
                        ti = self.refs[nd["first"] + k]
                        R._tri(ray, self.tris[ti], ti, self.objs[ti] if self.obj is None else self.obj)
                        ray.tested += 1
                        if stop and ray.objIdx > -1:
                            return True
                else:
                    axis = nd["axis"]
                    t = (nd["lo"][axis] + nd["split"] - ray.O[axis]) / ray.D[axis]
                    first, second = (nd["left"], nd["right"]) if ray.D[axis] > 0 else (nd["right"], nd["left"])
                    if float(t) < float(tmin) + 0.001:
                        node = second
                    elif float(t) > float(tmax) - 0.001:
                        node = first
                    else:
                        stack.append((second, t)); node = first
                        occ.kd_held = max(occ.kd_held, len(stack)); occ.push(tlas_pending, len(stack))
                    descend = True
            if descend:
                continue
            found = False
            while stack:
                second, t = stack.pop()
                if (ray.objIdx == self.obj and ray.t < t) if self.obj is not None else (ray.t < t):
                    continue
                node = second; found = True; break
            if not found:
                return False


class World:
    """a scene of the oracle `o` walked by `accel`: "bvh" (BVH / TLAS over BLASBVH) or "kd" (KDTree / TLAS over BLASKDTree).  The light quad and the floor are
    tlas_alt_restate's."""
    light_intersect, light_occludes, floor_intersect = R.Scene.light_intersect, R.Scene.light_occludes, R.Scene.floor_intersect
    _quad_t, _quad_inside = R.Scene._quad_t, R.Scene._quad_inside

    def __init__(self, orc, o, accel="bvh", light=LIGHT):
        self.kind, self.accel = o.kind, accel
        self.qc = [[f32(1), f32(0), f32(0), -f32(light[0])], [f32(0), f32(1), f32(0), -f32(light[1])], [f32(0), f32(0), f32(1), -f32(light[2])]]
        self.qsize = f32(0.5); self.floorN, self.floorD = (f32(0), f32(1), f32(0)), f32(1)
        self.parts = []
        for i in range(o.bvh_count()):
            b = o.bvh(i)
            invT = o.blas_transform(i)[1] if self.kind == 1 else None
            obj = b["tris"]["objIdx"][0] if self.kind == 1 else None
            if accel == "bvh":
                self.parts.append(Bvh(b, obj, invT))
            else:
                a = orc.alt_accel("kd", b["tris"]); dump = a.dump(); a.close()
                self.parts.append(Kd(dump, b["tris"], obj, invT))
        self.bvh_height = max(p.height for p in self.parts)
        if self.kind == 1:
            self.tlas = o.tlas()[0]
            self.tlas_height = self._tlas_height(0)

    def _tlas_height(self, i):
        lr = int(self.tlas[i]["leftRight"])
        return 0 if lr == 0 else 1 + max(self._tlas_height(lr & 0xffff), self._tlas_height(lr >> 16))

    def entries(self):
        """what the reference's structure needs at most, as the library sizes it: BVH: height (+ TLAS height + 1); KD: height + 1 entries (kdStack)"""
        own = self.bvh_height if self.accel == "bvh" else self.bvh_height + 1
        return own if self.kind == 0 else own + self.tlas_height + 1

    def structure(self, ray, occ, stop=False, lost=None, limit=None):
        if self.kind == 0:
            p = self.parts[0]
            return p.walk(ray, occ, 0, stop, lost, limit) if self.accel == "bvh" else p.walk(ray, occ, 0, stop)
        # TLASBVH::Intersect, infra/tlas_bvh.cpp:83-111 (tlas_kdtree.cpp is the same text)
        nodes = self.tlas; node = 0; stack = []
        while True:
            ray.traversed += 1; occ.steps += 1
            if limit is not None and occ.steps > limit:
                raise Cut()
            nd = nodes[node]
            if int(nd["leftRight"]) == 0:
                p = self.parts[int(nd["BLAS"])]
                tr = object_ray(ray, p.invT)
                if self.accel == "bvh":
                    occ.push(len(stack), 1)                                 # the return marker
                    done = p.walk(tr, occ, len(stack) + 1, stop, lost, limit)
                else:
                    done = p.walk(tr, occ, len(stack), stop)
                _back(ray, tr)
                if done or not stack:
                    return done
                node = stack.pop(); continue
            if self.accel == "bvh":
                occ.interior(0, len(stack))
            c1, c2 = int(nd["leftRight"]) & 0xffff, int(nd["leftRight"]) >> 16
            h1, t1, _ = R._aabb(ray, tuple(f32(x) for x in nodes[c1]["aabbMin"]), tuple(f32(x) for x in nodes[c1]["aabbMax"]))
            h2, t2, _ = R._aabb(ray, tuple(f32(x) for x in nodes[c2]["aabbMin"]), tuple(f32(x) for x in nodes[c2]["aabbMax"]))
            d1 = t1 if h1 else MISS; d2 = t2 if h2 else MISS
            if d1 > d2:
                d1, d2, c1, c2 = d2, d1, c2, c1
            if d1 == MISS:
                if not stack:
                    return False
                node = stack.pop()
            else:
                node = c1
                if d2 != MISS:
                    stack.append(0 if (lost is not None and len(stack) + 1 >= lost) else c2)
                    occ.push(0, len(stack)); occ.tlas_held = max(occ.tlas_held, len(stack))

    def find_nearest(self, O, D, lost=None, limit=None):
        """FileScene / TLASFileScene::FindNearest: light, floor, structure.  Returns (hit tuple, Occ)."""
        occ = Occ()
        with np.errstate(all="ignore"):
            ray = R.Ray(O, D)
            self.light_intersect(ray); self.floor_intersect(ray)
            try:
                self.structure(ray, occ, lost=lost, limit=limit)
            except Cut:
                occ.cut = True
        return (ray.t, ray.u, ray.v, ray.objIdx, ray.triIdx, ray.traversed, ray.tested), occ

    def is_occluded(self, O, D, t, stop=True):
        """IsOccluded: the light quad bounded by t, then the structure over the whole ray (shadow.t = 1e34f).  stop: the device's form, which ends at the first hit
        (the answer is the same; the entries held are those up to that hit)"""
        occ = Occ()
        with np.errstate(all="ignore"):
            if self.light_occludes(R.Ray(O, D, t)):
                return 1, occ
            shadow = R.Ray(O, D)
            self.structure(shadow, occ, stop=stop)
        return (1 if shadow.objIdx > -1 else 0), occ

    def find_nearest_many(self, O, D, hit_dtype, lost=None, limits=None):
        hits = np.zeros(len(O), hit_dtype); occs = []
        for i in range(len(O)):
            h, occ = self.find_nearest(O[i], D[i], lost, None if limits is None else int(limits[i]))
            hits[i] = h; occs.append(occ)
        return hits, occs

    def is_occluded_many(self, O, D, t, stop=True):
        r = [self.is_occluded(O[i], D[i], t[i], stop) for i in range(len(O))]
        return np.array([a for a, _ in r], np.int32), [b for _, b in r]


def diag_rays(n=48, seed=2):
    """rays for the KD-trees of the `compact` mesh, whose splits cycle through y, z, x towards the corner (0, 0, 0): from 0.9 in front of that corner along
    (1, a, b), 0.6 <= a <= 0.93, 0.45 a <= b <= 0.9 a (so z < y: below every triangle), crossing a plane of every axis inside every nested cell"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.6, 0.93, n)
    d = np.stack([np.ones(n), a, a * rng.uniform(0.45, 0.9, n)], 1)
    d[0] = (1, .9, .6)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P = np.stack([np.full(n, 2.0 ** -19), rng.uniform(0, 2.0 ** -12, n), np.zeros(n)], 1); P[:, 2] = P[:, 1] * 0.5
    return (P - 0.9 * d).astype(np.float32), d.astype(np.float32)


WORLDS = ("chain", "deep", "compact", "tlas_deep", "tlas_compact")
KIND = {"chain": 0, "deep": 0, "compact": 0, "tlas_deep": 1, "tlas_compact": 1}
# the entries the BVH worlds allot = the entries their filling rays hold (tests/test_stack_fill_cpu.py): height (+ TLAS height + 1)
BVH_ENTRIES = {"chain": 18, "deep": 8, "compact": 8, "tlas_deep": 15, "tlas_compact": 12}
# KD worlds: (kdStack = height + 1, the most (far child, plane) entries a ray of kd_rays holds).  kdStack - 1 is the most any ray can hold.  On the compact mesh
# the search stays below it: its KD-tree halves y, z, x in turn down to cells of 2^-7, and the walk's `t < tmin + 0.001` / `t > tmax - 0.001` visit one child
# only once a cell's stretch of the ray is that short; of 6 400 random and aimed rays none held more than 14 entries, the diagonal family below holds 13.
KD_ENTRIES = {"chain": (21, 20), "deep": (19, 18), "compact": (21, 13), "tlas_deep": (19, 18), "tlas_compact": (21, 13)}
KD_TLAS_HELD = {"tlas_deep": 6, "tlas_compact": 3}                        # TLAS entries pending above the KD part (TLAS height: all of them)
CAMERA = dict(W=32, H=32, pos=(-1.0, 0.5, 0.5), target=(0.0, 0.5, 0.5))  # on the x axis, looking along +x


def kd_rays(name):
    """the rays of the KD worlds: the filling rays of the BVH world and, on the compact mesh, the diagonal family"""
    O, D = fill_rays(name)
    if "compact" in name:
        O2, D2 = diag_rays()
        O, D = np.concatenate([O, O2]), np.concatenate([D, D2])
    return O, D


def mesh_oracle(orc, p):
    """the oracle's FileScene over bare positions, as test_gpu_grid_device.upload_described describes it to the library (test_mesh_truth_cpu.mesh_scene)"""
    tris = np.zeros(len(p), orc.TRI_DTYPE)
    tris["vertex0"], tris["vertex1"], tris["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    for k in ("normal0", "normal1", "normal2"):
        tris[k] = [0, 0, -1]
    o = orc.Oracle(0)
    o.set_light_position(LIGHT)
    tex = np.full((4, 4), 0x808080, np.uint32)                             # (the floor: 100 texels wide, so that file_scene.cpp:16's texW / 100 is the 1 upload_desc passes)
    o.set_floor_texture(np.full((4, 100), 0x808080, np.uint32)); o.set_skydome(tex); o.add_material()
    o.add_object((p.reshape(-1, 3), np.tile(np.float32([0, 0, -1]), (3 * len(p), 1)), np.zeros((3 * len(p), 2), np.float32)))
    o.build()
    return o


def scene_file(name, tmp):
    from test_gpu_golden_and_edges import write_scene
    return write_file_scene(tmp, write_scene, name) if KIND[name] == 0 else write_tlas_scene(tmp, write_scene, "tlas_" + name.split("_")[1])


def load_oracle(orc, name, tmp, placement=None):
    """the oracle's scene of a world; placement: another of transforms()'s names"""
    from conftest import ASSETS
    if name == "chain":
        return mesh_oracle(orc, mesh("chain"))
    o, _ = orc.load_scene(scene_file(name, tmp), KIND[name], ASSETS)
    if KIND[name] == 1:
        place(o, placement or name)
    return o


def through(orc, o, accel):
    """the oracle walks `accel` ("bvh" / "kd") from now on (mesh_truth_scenes.through)"""
    if accel == "kd":
        if o.kind == 0:
            o._alt = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, o._alt)
        else:
            orc.set_blas_accel(o, orc.blas_accels(o, "kd"))
    elif o.kind == 0:
        orc.set_render_accel(o, None)
    else:
        orc.set_blas_accel(o, None)
    return o


def camera_pixels(o, W, H):
    """the unjittered primary ray of every pixel of the oracle's camera (pixel corners, as Camera::GetPrimaryRay(x, y) is given them before the jitter)"""
    xy = np.stack(np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)), -1).reshape(-1, 2)
    return o.primary_rays(xy)


def kd_height(nodes):
    """the height of a flat pre-order KD-tree (KD_NODE_DTYPE; left < 0: a leaf)"""
    def h(i):
        return 0 if nodes["left"][i] < 0 else 1 + max(h(int(nodes["left"][i])), h(int(nodes["right"][i])))
    return h(0)


FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")


def same_hits(a, b):
    return np.all([np.asarray(a[f]).view(np.uint32) == np.asarray(b[f]).view(np.uint32) for f in FIELDS], axis=0)


def kept(world, O, D, hit_dtype, entries):
    """the stack-filling rays kept for the GPU tests: those that hold exactly `entries` entries AND on which a walker that loses the store into entry `entries`
    changes `traversed` or the hit.  Returns dict(fill: mask of the filling rays, keep: mask, hits: the honest records, occ)."""
    hits, occs = world.find_nearest_many(O, D, hit_dtype)
    held = np.array([o.held for o in occs])
    fill = held == entries
    lost, locc = world.find_nearest_many(O, D, hit_dtype, lost=entries, limits=LOST_LIMIT * np.maximum(hits["traversed"], 8))
    changed = ~same_hits(hits, lost) | np.array([o.cut for o in locc])
    return dict(fill=fill, keep=fill & changed, hits=hits, occ=occs, held=held)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the library allots
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def scene_words(ctx):
    """crt_debug_geometry's words: ..., stackDepth (8), bvhStack (9), poolRefBits (10), ldsBytes (11)"""
    import ctypes as C
    words = np.zeros(24, np.uint32); size = C.c_ulonglong()
    ctx._ck(ctx.L.crt_debug_geometry(ctx.h, words.ctypes.data_as(C.c_void_p), C.byref(size), None))
    return words


def allotted(ctx, accel="bvh", n_bvh=1):
    """dict(entries, bvh, tlas): the stack entries per lane the library allots for walks through `accel`.  bvh: the BVH part (bvhStack) or, for "kd", kdStack =
    the tallest live KD-tree's height + 1 (derived from get_kdtree: nothing reads the context's kdStack back); tlas: stackDepth - bvhStack = TLAS height + 1
    marker (0 for a FileScene); entries = their sum."""
    w = scene_words(ctx)
    depth, bvh = int(w[8]), int(w[9])
    if accel == "kd":
        own = max(ctx.get_kdtree(i)["height"] for i in range(n_bvh)) + 1
    else:
        own = bvh
    return dict(entries=own + depth - bvh, bvh=own, tlas=depth - bvh)
