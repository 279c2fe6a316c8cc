"""A CPU restatement of TLASFileScene::FindNearest / IsOccluded built with TLAS_USE_KDTree or TLAS_USE_Grid (infra/scene/tlas_file_scene.cpp:40-90, 201-218):
TLASKDTree / TLASGrid over BLASKDTree / BLASGrid.  This module restates them in float32, one ray at a time, operation for operation, so the GPU's records can be
compared field for field, Ray::traversed and Ray::tested included.  The C++ oracle has its own two-level walk (orc.set_blas_accel, written later and from the
reference text, not from this file); tests/test_tlas_alt_cpu.py holds the two to each other bit for bit, which is what pins the oracle's walk.

Its data come from the oracle only: o.tlas() (the TLAS the BVH variant built; the KD / grid variants' SetTransform takes the same world bounds from the same root
box), o.blas_transform(i) (invT), o.bvh(i)["tris"] (BLAS i's object-space triangles, reference order), orc.alt_accel(kind, tris).dump() (the structure KDTree /
Grid build over them: BLASKDTree::Build / BLASGrid::Build are the same builds, blas_kdtree.cpp:82-104, 227-301, blas_grid.cpp:82-131).

Numerics: numpy float32 scalars, rounded after every operation, no fused operations; the KD traversal's two mixed comparisons (`t < tmin + 0.001`) in double.
Not collected by pytest (no test_ prefix)."""
import numpy as np

f32 = np.float32
INF_T = f32(1e34)
BOX_MISS = f32(1e30)


def _dot(a, b):                               # tmplmath.h dot: (x*x + y*y) + z*z
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _min(a, b):                               # std::min(a, b)
    return b if b < a else a


def _max(a, b):                               # std::max(a, b)
    return b if a < b else a


class Ray:
    """template/ray.h: O, D, rD = 1 / D, t, objIdx, triIdx, barycentric, traversed; `tested` counts the whole query (the project's documented deviation)"""

    def __init__(self, O, D, t=INF_T):
        self.O = tuple(f32(x) for x in O); self.D = tuple(f32(x) for x in D)
        self.rD = (f32(1) / self.D[0], f32(1) / self.D[1], f32(1) / self.D[2])
        self.t = f32(t); self.objIdx = -1; self.triIdx = -1; self.u = f32(0); self.v = f32(0)
        self.traversed = 0; self.tested = 0


def _aabb(ray, bmin, bmax):
    """IntersectAABB of blas_kdtree.cpp:303-314 / blas_grid.cpp:133-142 / tlas_bvh.cpp:72-81: (hit, tmin, tmax)"""
    O, rD = ray.O, ray.rD
    tx1 = (bmin[0] - O[0]) * rD[0]; tx2 = (bmax[0] - O[0]) * rD[0]
    tmin = _min(tx1, tx2); tmax = _max(tx1, tx2)
    ty1 = (bmin[1] - O[1]) * rD[1]; ty2 = (bmax[1] - O[1]) * rD[1]
    tmin = _max(tmin, _min(ty1, ty2)); tmax = _min(tmax, _max(ty1, ty2))
    tz1 = (bmin[2] - O[2]) * rD[2]; tz2 = (bmax[2] - O[2]) * rD[2]
    tmin = _max(tmin, _min(tz1, tz2)); tmax = _min(tmax, _max(tz1, tz2))
    return (tmax >= tmin and tmin < ray.t and tmax > 0), tmin, tmax


def _tri(ray, tri, triIdx, objIdx):
    """BLASKDTree::IntersectTri / BLASGrid::IntersectTri, blas_kdtree.cpp:316-334, blas_grid.cpp:144-163"""
    v0, v1, v2 = tri
    edge1 = _sub(v1, v0); edge2 = _sub(v2, v0)
    h = _cross(ray.D, edge2)
    a = _dot(edge1, h)
    if a > f32(-0.0001) and a < f32(0.0001):
        return False
    f = f32(1) / a
    s = _sub(ray.O, v0)
    u = f * _dot(s, h)
    if u < 0 or u > 1:
        return False
    q = _cross(s, edge1)
    v = f * _dot(ray.D, q)
    if v < 0 or u + v > 1:
        return False
    t = f * _dot(edge2, q)
    if t > f32(0.0001):
        if t < ray.t:
            ray.t = _min(ray.t, t); ray.objIdx = objIdx; ray.triIdx = triIdx; ray.u = u; ray.v = v
        return True
    return False


class Blas:
    """one BLASKDTree / BLASGrid: its object-space triangles, its invT, its objIdx and the dumped structure"""

    def __init__(self, kind, tris, invT, objIdx, dump):
        self.kind, self.objIdx, self.s = kind, int(objIdx), dump
        self.tris = [tuple(tuple(f32(x) for x in t[k]) for k in ("vertex0", "vertex1", "vertex2")) for t in tris]
        self.invT = [[f32(x) for x in np.asarray(invT, np.float32).reshape(4, 4)[r]] for r in range(3)]
        if kind == "kd":
            self.nodes = [dict(lo=tuple(f32(x) for x in n["aabbMin"]), hi=tuple(f32(x) for x in n["aabbMax"]), left=int(n["left"]), right=int(n["right"]),
                               split=f32(n["splitDistance"]), axis=int(n["splitAxis"]), first=int(n["firstTri"]), count=int(n["triCount"])) for n in dump["nodes"]]
            self.refs = [int(r) for r in dump["refs"]]
        else:
            self.res = [int(r) for r in dump["resolution"]]; self.cell = [f32(x) for x in dump["cellSize"]]
            self.lo = tuple(f32(x) for x in dump["boundsMin"]); self.hi = tuple(f32(x) for x in dump["boundsMax"])
            self.start = [int(x) for x in dump["cellStart"]]; self.refs = [int(x) for x in dump["refs"]]

    # BLASKDTree::IntersectKDTree, blas_kdtree.cpp:336-398 (rule 1: the caller frame returns only if the ray's nearest hit is this BLAS's)
    def _kd(self, ray, ni, rule1, stop):
        node = self.nodes[ni]
        ray.traversed += 1
        hit, tmin, tmax = _aabb(ray, node["lo"], node["hi"])
        if not hit:
            return False
        if node["left"] < 0:
            for k in range(node["count"]):
                ti = self.refs[node["first"] + k]
                _tri(ray, self.tris[ti], ti, self.objIdx)
                ray.tested += 1
                if stop and ray.objIdx > -1:
                    return True
            return False
        axis = node["axis"]
        splitPos = node["lo"][axis] + node["split"]
        t = (splitPos - ray.O[axis]) / ray.D[axis]
        early = (lambda: ray.objIdx == self.objIdx and ray.t < t) if rule1 else (lambda: ray.t < t)
        near, far = (node["left"], node["right"]) if ray.D[axis] > 0 else (node["right"], node["left"])
        if float(t) < float(tmin) + 0.001:
            return self._kd(ray, far, rule1, stop)
        if float(t) > float(tmax) - 0.001:
            return self._kd(ray, near, rule1, stop)
        if self._kd(ray, near, rule1, stop):
            return True
        if early():
            return False
        return self._kd(ray, far, rule1, stop)

    # BLASGrid::IntersectGrid, blas_grid.cpp:180-231 (3D-DDA)
    def _grid(self, ray, stop):
        hit, _, _ = _aabb(ray, self.lo, self.hi)
        if not hit:
            return False
        ext, step, cell, deltaT, nxt = [0] * 3, [0] * 3, [0] * 3, [f32(0)] * 3, [f32(0)] * 3
        for i in range(3):
            roc = ray.O[i] - self.lo[i]
            fl = np.floor(roc / self.cell[i])
            c = 0 if np.isnan(fl) else (int(fl) if np.isfinite(fl) else (1 << 31 if fl > 0 else -(1 << 31)))
            cell[i] = min(max(c, 0), self.res[i] - 1)
            if ray.D[i] < 0:
                deltaT[i] = -self.cell[i] * ray.rD[i]; nxt[i] = (f32(cell[i]) * self.cell[i] - roc) * ray.rD[i]; ext[i] = -1; step[i] = -1
            else:
                deltaT[i] = self.cell[i] * ray.rD[i]; nxt[i] = (f32(cell[i] + 1) * self.cell[i] - roc) * ray.rD[i]; ext[i] = self.res[i]; step[i] = 1
        amap = (2, 1, 2, 1, 2, 2, 0, 0)
        while True:
            ray.traversed += 1
            index = cell[0] + cell[1] * self.res[0] + cell[2] * self.res[0] * self.res[1]
            for k in range(self.start[index], self.start[index + 1]):
                ti = self.refs[k]
                ray.tested += 1
                _tri(ray, self.tris[ti], ti, self.objIdx)
                if stop and ray.objIdx > -1:
                    return True
            k = (int(nxt[0] < nxt[1]) << 2) + (int(nxt[0] < nxt[2]) << 1) + int(nxt[1] < nxt[2])
            axis = amap[k]
            if ray.t < nxt[axis]:
                break
            cell[axis] += step[axis]
            if cell[axis] == ext[axis]:
                break
            nxt[axis] = nxt[axis] + deltaT[axis]
        return False

    def object_ray(self, ray):
        """BLASKDTree::Intersect / BLASGrid::Intersect's transform (blas_kdtree.cpp:420-433, blas_grid.cpp:233-248): TransformPosition_SSE / TransformVector_SSE
        (template/tmplmath.cpp:170-191: (x + y) + (z + w) / (x + y) + z), rD = 1 / D"""
        O, D, M = ray.O, ray.D, self.invT
        Oo = tuple((O[0] * M[r][0] + O[1] * M[r][1]) + (O[2] * M[r][2] + f32(1) * M[r][3]) for r in range(3))
        Do = tuple((D[0] * M[r][0] + D[1] * M[r][1]) + D[2] * M[r][2] for r in range(3))
        tr = Ray(Oo, Do, ray.t)
        tr.objIdx, tr.triIdx, tr.u, tr.v, tr.traversed, tr.tested = ray.objIdx, ray.triIdx, ray.u, ray.v, ray.traversed, ray.tested
        return tr

    def intersect(self, ray, rule1=True, stop=False):
        """Ray(const Ray&) copies t, objIdx, triIdx, barycentric and traversed (template/ray.h:10-14); O / D / rD are restored afterwards"""
        tr = self.object_ray(ray)
        done = self._kd(tr, 0, rule1, stop) if self.kind == "kd" else self._grid(tr, stop)
        ray.t, ray.objIdx, ray.triIdx, ray.u, ray.v, ray.traversed, ray.tested = tr.t, tr.objIdx, tr.triIdx, tr.u, tr.v, tr.traversed, tr.tested
        return done


class Scene:
    """TLASFileScene with TLAS_USE_KDTree ("kd") or TLAS_USE_Grid ("grid") over the oracle's state `o` (an orc.Oracle of kind 1)"""

    def __init__(self, orc, o, kind, light):
        self.kind = kind
        self.tlas, _ = o.tlas()
        self.blas = []
        for i in range(o.bvh_count()):
            tris = o.bvh(i)["tris"]
            a = orc.alt_accel(kind, tris); dump = a.dump(); a.close()
            _, invT, _, _ = o.blas_transform(i)
            self.blas.append(Blas(kind, tris, invT, tris["objIdx"][0], dump))
        # the light quad Quad(0, 1) with T = Translate(lightPos) (tlas_file_scene.cpp:15-18): invT = identity rotation, translation -lightPos; size 0.5
        self.qc = [[f32(1), f32(0), f32(0), -f32(light[0])], [f32(0), f32(1), f32(0), -f32(light[1])], [f32(0), f32(0), f32(1), -f32(light[2])]]
        self.qsize = f32(0.5)
        self.floorN, self.floorD = (f32(0), f32(1), f32(0)), f32(1)          # Plane(1, float3(0, 1, 0), 1, ...)

    def _quad_t(self, ray):
        c = self.qc
        Oy = ((c[1][0] * ray.O[0] + c[1][1] * ray.O[1]) + c[1][2] * ray.O[2]) + c[1][3]
        Dy = (c[1][0] * ray.D[0] + c[1][1] * ray.D[1]) + c[1][2] * ray.D[2]
        return Oy / -Dy

    def _quad_inside(self, ray, t):
        c = self.qc
        Ox = ((c[0][0] * ray.O[0] + c[0][1] * ray.O[1]) + c[0][2] * ray.O[2]) + c[0][3]
        Oz = ((c[2][0] * ray.O[0] + c[2][1] * ray.O[1]) + c[2][2] * ray.O[2]) + c[2][3]
        Dx = (c[0][0] * ray.D[0] + c[0][1] * ray.D[1]) + c[0][2] * ray.D[2]
        Dz = (c[2][0] * ray.D[0] + c[2][1] * ray.D[1]) + c[2][2] * ray.D[2]
        Ix = Ox + t * Dx; Iz = Oz + t * Dz
        s = self.qsize
        return Ix > -s and Ix < s and Iz > -s and Iz < s

    def light_intersect(self, ray):                                       # Quad::Intersect, template/primitives.h:331-346
        t = self._quad_t(ray)
        if t < ray.t and t > 0 and self._quad_inside(ray, t):
            ray.t = t; ray.objIdx = 0

    def light_occludes(self, ray):                                        # Quad::IsOccluded, primitives.h:347-362
        t = self._quad_t(ray)
        return bool(t < ray.t and t > 0 and self._quad_inside(ray, t))

    def floor_intersect(self, ray):                                       # Plane::Intersect, primitives.h:107-111
        t = -(_dot(ray.O, self.floorN) + self.floorD) / _dot(ray.D, self.floorN)
        if t < ray.t and t > 0:
            ray.t = t; ray.objIdx = 1

    def tlas_intersect(self, ray, rule1=True, stop=False):
        """TLASKDTree::Intersect / TLASGrid::Intersect = TLASBVH::Intersect's loop (tlas_bvh.cpp:83-111) over the shared node array"""
        nodes = self.tlas
        node = 0; stack = []
        while True:
            ray.traversed += 1
            nd = nodes[node]
            if int(nd["leftRight"]) == 0:                                  # isLeaf
                if self.blas[int(nd["BLAS"])].intersect(ray, rule1, stop):
                    return
                if not stack:
                    return
                node = stack.pop(); continue
            c1, c2 = int(nd["leftRight"]) & 0xffff, int(nd["leftRight"]) >> 16
            h1, t1, _ = _aabb(ray, tuple(f32(x) for x in nodes[c1]["aabbMin"]), tuple(f32(x) for x in nodes[c1]["aabbMax"]))
            h2, t2, _ = _aabb(ray, tuple(f32(x) for x in nodes[c2]["aabbMin"]), tuple(f32(x) for x in nodes[c2]["aabbMax"]))
            d1 = t1 if h1 else BOX_MISS; d2 = t2 if h2 else BOX_MISS
            if d1 > d2:
                d1, d2, c1, c2 = d2, d1, c2, c1
            if d1 == BOX_MISS:
                if not stack:
                    return
                node = stack.pop()
            else:
                node = c1
                if d2 != BOX_MISS:
                    stack.append(c2)

    def find_nearest(self, O, D, rule1=True):
        """TLASFileScene::FindNearest (tlas_file_scene.cpp:201-206): light, floor, TLAS; one HIT_DTYPE-like tuple per ray"""
        with np.errstate(all="ignore"):
            ray = Ray(O, D)
            self.light_intersect(ray); self.floor_intersect(ray); self.tlas_intersect(ray, rule1)
        return (ray.t, ray.u, ray.v, ray.objIdx, ray.triIdx, ray.traversed, ray.tested)

    def is_occluded(self, O, D, t):
        """TLASFileScene::IsOccluded (tlas_file_scene.cpp:208-218) for Ray(O, D, t) (objIdx -1): the light quad bounded by t, then the TLAS with shadow.t = 1e34f"""
        with np.errstate(all="ignore"):
            ray = Ray(O, D, t)
            if self.light_occludes(ray):
                return 1
            shadow = Ray(O, D)
            self.tlas_intersect(shadow)
            return 1 if shadow.objIdx > -1 else 0

    def find_nearest_many(self, O, D, hit_dtype, rule1=True):
        out = np.zeros(len(O), hit_dtype)
        for i in range(len(O)):
            out[i] = self.find_nearest(O[i], D[i], rule1)
        return out

    def is_occluded_many(self, O, D, t):
        return np.array([self.is_occluded(O[i], D[i], t[i]) for i in range(len(O))], np.int32)


def query_rays(o, light, n=2000, seed=5):
    """rays for the two-level KD / grid queries, from the oracle's state: camera-like rays that hit the floor first or pass through several instances, rays from
    inside each instance's bounds, upward rays towards the light, and a share with a direction component that is exactly 0"""
    rng = np.random.default_rng(seed)
    nodes, _ = o.tlas()
    lo, hi = nodes[0]["aabbMin"].astype(np.float64), nodes[0]["aabbMax"].astype(np.float64)
    k = n // 4
    # from in front of the scene at eye height, through its bounds (many go down into the floor, many cross several instances)
    O1 = np.stack([rng.uniform(lo[0] - 1, hi[0] + 1, k), rng.uniform(-0.5, 1.5, k), np.full(k, lo[2] - 2.5)], 1)
    T1 = np.stack([rng.uniform(lo[0], hi[0], k), rng.uniform(lo[1] - 0.3, hi[1], k), rng.uniform(lo[2], hi[2], k)], 1)
    # along the row of instances (x direction), low: several instances per ray
    O2 = np.stack([np.full(k, lo[0] - 1.5), rng.uniform(lo[1] + 0.02, hi[1], k), rng.uniform(lo[2], hi[2], k)], 1)
    T2 = O2 + np.stack([np.full(k, 3.0), rng.uniform(-0.2, 0.1, k), rng.uniform(-0.6, 0.6, k)], 1)
    # from inside each instance's world bounds, in all directions
    sets_O, sets_T = [O1, O2], [T1, T2]
    nb = o.bvh_count(); m = max(k // nb, 8)
    for i in range(nb):
        _, _, blo, bhi = o.blas_transform(i)
        blo, bhi = blo.astype(np.float64), bhi.astype(np.float64)
        Oi = blo + rng.uniform(0.2, 0.8, (m, 3)) * (bhi - blo)
        sets_O.append(Oi); sets_T.append(Oi + rng.normal(size=(m, 3)))
    # up towards the light from above the floor
    r = n - sum(len(s) for s in sets_O)
    O4 = np.stack([rng.uniform(lo[0], hi[0], r), rng.uniform(-0.9, 0.5, r), rng.uniform(lo[2], hi[2], r)], 1)
    T4 = np.stack([light[0] + rng.uniform(-1, 1, r), np.full(r, light[1]), light[2] + rng.uniform(-1, 1, r)], 1)
    sets_O.append(O4); sets_T.append(T4)
    O = np.concatenate(sets_O).astype(np.float32)
    D = np.concatenate(sets_T) - np.concatenate(sets_O)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    sel = rng.permutation(n)[: n // 10]                                  # axis-parallel components
    D[sel[0::3], 0] = 0; D[sel[1::3], 1] = 0; D[sel[2::3], 2] = 0
    return O, D
