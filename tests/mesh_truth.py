"""Float64 brute-force ground truth for every query over a triangle-mesh scene (FileScene, kind 0; TLASFileScene, kind 1): FindNearest, IsOccluded, GetHitInfo.

The nearest hit does not depend on the structure a scene is walked by, so one truth judges the BVH, the TLAS, the KD-tree, the grid, their two-level forms, and
every structure refitted or rebuilt on the host or on the device.  Nothing here imports the oracle or the library: the inputs are plain arrays (per BVH the Tri
records; per BLAS the float32 T and invT the scene holds; the light's position; the rays), and the test modules hand the answers in.  Not collected by pytest.

Derived from the reference's lines as mathematics:
  candidates   Moeller-Trumbore as infra/bvh.cpp:203-222 and infra/blas_bvh.cpp:281-300 state it, for every triangle of every BVH, in the space the reference
               evaluates it in: world space for a FileScene, object space for a BLAS, o = invT O, d = invT D, NOT renormalised (blas_bvh.cpp:376-389), so the
               ray parameter t is the world's.  Conditions: |a| >= 1e-4, 0 <= u, 0 <= v, u + v <= 1, t > 1e-4.  The two absolute thresholds are behaviour.
  floor        Plane(1, (0, 1, 0), 1): t = -(O.N + 1) / D.N, t > 0 (template/primitives.h:107-111)
  light        Quad(0, 2 half, T), T rigid = (R | c): the plane through the centre c with normal R's y column, t > 0, and the hit point's coordinates along R's
               x and z columns within +-half (primitives.h:321-367 as geometry).  The scene files give T = Translate(light position), half = 0.5; a look
               (crt_update_look) any rigid T and any half size: World(light_T=, light_half=)
  IsOccluded   the light bounded by the ray's t; then the structure over the WHOLE ray (shadow.t = 1e34f); the floor is skipped (file_scene.cpp:177-187)
  GetHitInfo   N = normalize(w n0 + u n1 + v n2) (bvh.cpp:290-297), carried by T and renormalised for a BLAS (blas_bvh.cpp:391-398), turned towards the ray
               (file_scene.cpp:211); uv interpolated alike; material 2 + matIdx; the floor's N, uv = frac(I.xz * invto) and the light's N = -(R's y column), turned
               towards the ray like every other.

THE CRITERION.  float32 arithmetic may decide a borderline condition either way, so every ray gets two candidate sets:
  ROBUST  every condition holds with slack;   SOFT  every condition holds when relaxed by the same slack;
  t_hi = the nearest robust candidate, t_lo = the nearest soft candidate (floor and light included).
Any correct float32 evaluation returns t in [t_lo - tol, t_hi + tol]; it returns a miss only if there is no robust candidate at all, and floor or light only
where that object has a soft candidate at the returned t.  NO ray is excluded from this: one with a borderline candidate in front is merely constrained loosely.
Where the soft candidates within ID_BAND of t_lo belong to exactly one triangle, the returned (objIdx, triIdx) is that triangle and u, v agree with the truth's.

The slack, per candidate (eps = 2^-24; emax the longer edge, s = o - vertex0; O, D and the vertices ARE float32 numbers, so s and the edges carry one rounding):
  u, v, u + v   EPS + 8 eps cond,  cond = (|s| + omag / 2) |d| emax / |a|      EPS = 1e-4, plus a first-order bound on the rounding of u = dot(s, h) / a, h = cross(d, e2):
                one rounding in s and in e2, three in h, five in the dot product: at most 7 eps |s| |h| / |a|, |h| <= |d| |e2|; the same for v and a's own part.
                omag: a BLAS's o = invT O is itself rounded, four times at the magnitude |invT| |O| + |invT's translation|: 4 eps omag; 0 for a FileScene
  |a|           REL * 1e-4 + 8 eps |d| |e1| |e2|                 REL = 1e-3, plus the same bound on the triple product
  t > 1e-4      REL * 1e-4 + TOL["t"] * scale (the answer's own tolerance);   the floor's and the light's t > 0: TOL["t"] * scale;   the quad's half size: EPS

A ray is UNINFORMATIVE if t_hi - t_lo exceeds ID_BAND * scale, or if its nearest soft candidates belong to several triangles although the nearest lies in a
triangle's interior (coincident or crossing triangles; two triangles that meet at a shared edge are expected and not counted).  Caps on every ray set keep the
check from being vacuous: at most MAX_UNINFORMATIVE of the rays, at least MIN_MESH / MIN_PRIM / MIN_MISS robust mesh hits / floor-or-light answers / misses.

TOLERANCES.  Measured on the CPU oracle (never on the HIP path) by tests/test_mesh_truth_cpu.py::test_tolerance_table over the 4 096-ray sets of the three
scenes and their worlds (bvh, kd, grid; tlas, tlas_grid), on rays with a tight interval (t_hi - t_lo <= 1e-9 scale) whose answer names the truth's triangle; asserted = 4 x observed (the project's practice, PRIM_TOLERANCE of analytic_truth.py: room for the
rays a later edit would draw; the kernels return the oracle's bits).  t and I are scaled by scale = max(1, |t|, |O|, mesh extent); u, v, N and the interpolated
uv by 1 + cond, the conditioning of that triangle under that ray (so those rows are in units of a rounding, 2^-24 = 6e-8); the floor's uv by scale.
  This DEPARTS from "scale every tolerance by max(1, |t|, |O|, extent)": u = dot(s, h) / a loses digits as |s| |d| emax / |a| grows (a grazing ray, a thin or
  distant triangle), which none of those magnitudes sees, and a bound in them that the oracle meets on a grazing ray would be vacuous on a head-on one.  What
  it allows, on the rays where a u / v check actually runs (the answer names the truth's unique triangle):
    set (rays checked)                 median cond    99th percentile    largest    u allowed at the median / at the largest
    bunny_scene.xml (2 604 of 4 096)        145            1 645           2 709       5.3e-5 / 9.9e-4
    tlas_scene.xml  (2 038)                 800            7 814          16 506       2.9e-4 / 6.0e-3
    generated scene (2 413)                  32            3 335           7 821       1.2e-5 / 2.8e-3
    three (644 of 1 024)                     13            1 529          48 610       4.8e-6 / 1.8e-2
    spanner (653)                           301            5 936           7 887       1.1e-4 / 2.9e-3
    sliver (557)                            387           13 616          30 889       1.4e-4 / 1.1e-2
    bunny_moved (647)                       175            1 404           2 195       6.4e-5 / 8.0e-4
  The identity of the triangle, which needs no tolerance, is what catches a wrong hit; u and v at these tolerances catch a swapped or mirrored pair.

COST.  The truth of the largest set (tlas_scene.xml, 12 460 triangles, 4 096 rays) takes 10 to 11 s of numpy on one core, 2.6 s for the 1 024 rays of the GPU
module; every test module computes it once per scene and shares it.
"""
import numpy as np

import analytic_truth as at

A_MIN = 1e-4                                       # bvh.cpp:209
T_MIN = 1e-4                                       # bvh.cpp:218
EPS = 1e-4
REL = 1e-3
EPS32 = 2.0 ** -24
ID_BAND = 1e-4
INF = np.inf
MAX_UNINFORMATIVE = 0.01
MIN_MESH, MIN_PRIM, MIN_MISS = 500, 100, 100

#   quantity: (observed on the oracle, asserted = 4 x observed)        [test_tolerance_table prints the first column]
TOL = {
    "t": (7.43e-6, 2.97e-5),
    "u": (9.10e-8, 3.64e-7),
    "v": (1.02e-7, 4.08e-7),
    "I": (6.51e-6, 2.60e-5),
    "N": (7.02e-8, 2.81e-7),
    "uv": (5.14e-8, 2.06e-7),
}
# the two-level KD-tree (TLASKDTree over BLASKDTree) does not return the nearest hit on every ray: the reference's own behaviour, tests/alt_disagreement.py.
# (violations observed on the oracle over the 4 096 rays of tlas_scene.xml / of the generated scene, the cap asserted on the share = 2 x observed).  All are LOST
# hits.  The generated scene's are rays at its two cubes of edge 0.009 and 0.013 (57 and 25), and the cause is the walk's `t < tmin + 0.001` / `t > tmax - 0.001`
# tests (blas_kdtree.cpp:365-389), which drop a child whose stretch of the ray is shorter than 0.001 — a fifth of such a cube: of the first 80 of them, 72 find their
# hit when tests/tlas_alt_restate.py walks the same trees with those two margins at 0.  The other 8 stay lost: the build's own 0.001 (blas_kdtree.cpp:262) keeps a
# triangle that reaches less than that across a split plane on one side only.  On the GPU the cap is not what holds a kernel: a violation stands only where
# the oracle's walk of the same trees returns the same bits.
TLAS_KD_VIOLATIONS = {"tlas": (2, 2 * 2 / 4096), "gen": (82, 2 * 82 / 4096)}

# Left out of the generated meshes of the rebuild tests (bvh_build_inputs.GENERATED): `ulp` and `chain`, whose coordinates of 2^20 and 8^23 leave float32 no
# digits to resolve a band of 1e-4; `single`, `pair`, `flat`, `margin`, `zeros-*` add nothing to `three` for a nearest hit.
REBUILD_MESHES = ("three", "spanner", "sliver", "cluster", "bunny_moved")
# `sliver`: triangles 0.01 wide and 1.56 long.  From the sphere round the mesh (126 away) cond = 126 * 1.56 / (0.0156 cos): a slack of 0.006 / cos of a barycentric
# at each of three edges, so its aimed rays start 2 from the centroid they aim at (cond 200 / cos, a slack of 1.1e-4)
AIMED_FROM = {"sliver": 2.0}


def tol(name):
    return TOL[name][1]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the world
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class World:
    """kind 0: one BVH in world space.  kind 1: one BLAS per object with its float32 T and invT as the scene holds them.  light: the quad's centre;
    light_T (the float32 cells, rotation | centre) and light_half: a look's quad instead of Translate(light), 0.5.
    obj_mat: the material index of every object of the scene file.  floor_invto: 1 / (floor texture width // 100) (file_scene.cpp:16)."""

    def __init__(self, kind, tris, T=None, invT=None, light=(0.0, 3.0, 1.0), obj_mat=(0,), floor_invto=1.0, light_T=None, light_half=None):
        self.kind = int(kind)
        self.tris = [np.array(t) for t in tris]
        n = len(self.tris)
        self.T = [np.eye(4) if T is None else np.asarray(T[i], np.float32).astype(np.float64).reshape(4, 4) for i in range(n)]
        self.invT = [np.eye(4) if invT is None else np.asarray(invT[i], np.float32).astype(np.float64).reshape(4, 4) for i in range(n)]
        self.light = np.asarray(light, np.float32).astype(np.float64)
        self.light_R, self.light_half = np.eye(3), float(at.LIGHT_HALF if light_half is None else np.float32(light_half))
        if light_T is not None:                                             # the look's float32 cells, 3 x 4 or 4 x 4, row-major: rotation | centre
            M = np.asarray(light_T, np.float32).astype(np.float64).reshape(-1, 4)
            self.light_R, self.light = M[:3, :3].copy(), M[:3, 3].copy()
            assert np.abs(self.light_R @ self.light_R.T - np.eye(3)).max() < 1e-6, "a rigid light transform"
        self.obj_mat = list(obj_mat)
        self.floor_invto = float(floor_invto)
        self.v = [np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], 1).astype(np.float64) for t in self.tris]          # [n, 3, 3] per BVH
        # where the triangles APPEAR in the world: x with invT x = p
        self.world_v = [(v.reshape(-1, 3) - M[:3, 3]) @ np.linalg.inv(M[:3, :3]).T for v, M in zip(self.v, self.invT)]
        allv = np.concatenate(self.world_v)
        self.extent = float(np.abs(allv).max())
        self.first = np.cumsum([0] + [len(v) for v in self.v])                                                           # global triangle numbers

    def obj_idx(self, blas, tri):
        """the objIdx FindNearest reports for triangle `tri` of BVH `blas`: Tri::objIdx (bvh.cpp:220) or the BLAS's own (blas_bvh.cpp:298)"""
        out = np.full(len(blas), -1, np.int64)
        for b in range(len(self.tris)):
            m = blas == b
            out[m] = self.tris[b]["objIdx"][tri[m]] if self.kind == 0 else 2 + b
        return out


def world_of(scene, kind, light, obj_mat, floor_invto, light_T=None, light_half=None):
    """the plain arrays of anything that answers bvh_count(), bvh(i)["tris"] and blas_transform(i) (the oracle's scene and the host front's alike)"""
    n = scene.bvh_count()
    tris = [scene.bvh(i)["tris"] for i in range(n)]
    if kind == 0:
        return World(0, tris, light=light, obj_mat=obj_mat, floor_invto=floor_invto, light_T=light_T, light_half=light_half)
    tr = [scene.blas_transform(i) for i in range(n)]
    return World(1, tris, [t[0] for t in tr], [t[1] for t in tr], light, obj_mat, floor_invto, light_T, light_half)


def mesh_world(p, light=(0.0, 3.0, 1.0)):
    """a FileScene of bare positions (n, 3, 3) as test_gpu_grid_device.upload_described uploads it: normals (0, 0, -1), objIdx 2, one material"""
    t = np.zeros(len(p), at_tri_dtype())
    t["vertex0"], t["vertex1"], t["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    for k in ("normal0", "normal1", "normal2"):
        t[k] = [0, 0, -1]
    t["objIdx"] = 2
    return World(0, [t], light=light, obj_mat=[0], floor_invto=1.0)


def at_tri_dtype():
    return np.dtype([("vertex0", "<f4", 3), ("vertex1", "<f4", 3), ("vertex2", "<f4", 3), ("normal0", "<f4", 3), ("normal1", "<f4", 3), ("normal2", "<f4", 3),
                     ("uv0", "<f4", 2), ("uv1", "<f4", 2), ("uv2", "<f4", 2), ("centroid", "<f4", 3), ("objIdx", "<i4")])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def moller_trumbore(o, d, v):
    """a, u, v, t [rays, triangles] of bvh.cpp:205-217 in float64, and |s|"""
    v0 = v[:, 0]; e1 = v[:, 1] - v0; e2 = v[:, 2] - v0
    h = _cross(d[:, None, :], e2[None])
    a = (e1[None] * h).sum(-1)
    with np.errstate(all="ignore"):
        f = 1.0 / a
        s = o[:, None, :] - v0[None]
        u = f * (s * h).sum(-1)
        q = _cross(s, e1[None])
        w = f * (d[:, None, :] * q).sum(-1)
        t = f * (e2[None] * q).sum(-1)
    return a, u, w, t, np.sqrt((s * s).sum(-1))


def _scale(world, O, t):
    return np.maximum(np.maximum(1.0, np.where(np.isfinite(t), np.abs(t), 0.0)), np.maximum(np.linalg.norm(O, axis=1), world.extent))


def mesh_candidates(world, O, D, a_min=A_MIN, chunk=96):
    """per ray, over every triangle of every BVH: dict of
       hi, lo          the nearest robust / soft mesh candidate's t (inf: none)
       blas, tri, u, v the nearest soft candidate; slack: its u, v slack; edge: it lies within 10 slacks of one of its triangle's edges
       second          the next soft candidate's t (another triangle)
    a_min: the |a| threshold (0 = ignored: the doctored form of the test)"""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    n = len(O)
    out = dict(hi=np.full(n, INF), lo=np.full(n, INF), second=np.full(n, INF), blas=np.full(n, -1), tri=np.full(n, -1), u=np.zeros(n), v=np.zeros(n),
               slack=np.full(n, EPS), cond=np.zeros(n), edge=np.zeros(n, bool))
    tscale = np.maximum(1.0, np.maximum(np.linalg.norm(O, axis=1), world.extent))           # (|t| joins in where t is known: a t > 1e-4 test is about small t)
    t_band = REL * T_MIN + tol("t") * tscale
    for b, v in enumerate(world.v):
        M = world.invT[b]
        o_all = O @ M[:3, :3].T + M[:3, 3]; d_all = D @ M[:3, :3].T
        omag_all = (np.linalg.norm(M[:3, :3], 2) * np.linalg.norm(O, axis=1) + np.linalg.norm(M[:3, 3])) if world.kind == 1 else np.zeros(n)
        v0 = v[:, 0]; e1 = v[:, 1] - v0; e2 = v[:, 2] - v0
        l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        emax = np.maximum(l1, l2)
        for c0 in range(0, n, chunk):
            sl = slice(c0, min(n, c0 + chunk)); o, d = o_all[sl], d_all[sl]
            a, u, w, t, ls = moller_trumbore(o, d, v)
            ld = np.linalg.norm(d, axis=1)[:, None]
            with np.errstate(all="ignore"):
                cond = (ls + 0.5 * omag_all[sl, None]) * ld * emax[None] / np.abs(a)
            e_uv = EPS + 8 * EPS32 * cond
            e_a = (REL * a_min + 8 * EPS32 * ld * (l1 * l2)[None]) if a_min > 0 else 0.0
            tb = t_band[sl, None]
            with np.errstate(invalid="ignore"):
                rob = (np.abs(a) >= a_min + e_a) & (u >= e_uv) & (w >= e_uv) & (u + w <= 1 - e_uv) & (t > T_MIN + tb)
                soft = (np.abs(a) >= a_min - e_a) & (np.abs(a) > 0) & (u >= -e_uv) & (w >= -e_uv) & (u + w <= 1 + e_uv) & (t > T_MIN - tb)
            rows = np.arange(t.shape[0])
            hi = np.where(rob, t, INF).min(1)
            ts = np.where(soft, t, INF)
            k = ts.argmin(1); t1 = ts[rows, k]
            ts[rows, k] = INF
            t2 = ts.min(1)
            better = t1 < out["lo"][sl]
            # the second nearest overall: the loser of this comparison, or the runner-up inside this BVH
            out["second"][sl] = np.minimum(np.where(better, np.minimum(out["lo"][sl], t2), np.minimum(out["second"][sl], t1)), out["second"][sl])
            for key, val in (("lo", t1), ("blas", b), ("tri", k), ("u", u[rows, k]), ("v", w[rows, k]), ("slack", e_uv[rows, k]), ("cond", cond[rows, k])):
                out[key][sl] = np.where(better, val, out[key][sl])
            out["hi"][sl] = np.minimum(out["hi"][sl], hi)
    with np.errstate(invalid="ignore"):
        out["edge"] = np.minimum(np.minimum(out["u"], out["v"]), 1 - out["u"] - out["v"]) < 10 * out["slack"]
    return out


def floor_candidate(world, O, D, band):
    """(robust t, soft t) of the floor plane y = -1"""
    with np.errstate(all="ignore"):
        t = -(O[:, 1] + 1.0) / D[:, 1]
    t = np.where(np.isfinite(t), t, -INF)
    return np.where(t > band, t, INF), np.where(t > -band, t, INF)


def light_candidate(world, O, D, band):
    """(robust t, soft t) of the light quad"""
    R = world.light_R
    o = O - world.light
    with np.errstate(all="ignore"):
        t = (o @ R[:, 1]) / -(D @ R[:, 1])                                  # the plane through the centre with normal R's y column
    t = np.where(np.isfinite(t), t, -INF)
    tt = np.where(np.isfinite(t), t, 0.0)
    P = o + tt[:, None] * D
    edge = world.light_half - np.maximum(np.abs(P @ R[:, 0]), np.abs(P @ R[:, 2]))   # inside the square spanned by R's x and z columns
    return np.where((t > band) & (edge > EPS), t, INF), np.where((t > -band) & (edge > -EPS), t, INF)


def nearest_truth(world, O, D, a_min=A_MIN):
    """everything the criterion needs, per ray (see the module's head); kind: 0 light, 1 floor, 2 mesh, -1 nothing = the nearest SOFT candidate's"""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    m = mesh_candidates(world, O, D, a_min)
    s0 = np.maximum(1.0, np.maximum(np.linalg.norm(O, axis=1), world.extent))
    band0 = tol("t") * s0
    fr, fs = floor_candidate(world, O, D, band0)
    lr, ls = light_candidate(world, O, D, band0)
    t_hi = np.minimum(np.minimum(m["hi"], fr), lr)
    t_lo = np.minimum(np.minimum(m["lo"], fs), ls)
    kind = np.where(t_lo == INF, -1, np.where(m["lo"] == t_lo, 2, np.where(fs == t_lo, 1, 0)))
    kind_hi = np.where(t_hi == INF, -1, np.where(m["hi"] == t_hi, 2, np.where(fr == t_hi, 1, 0)))
    scale = _scale(world, O, t_hi)
    band = ID_BAND * scale
    # the nearest soft candidate's rivals: another triangle, the floor, the light
    rival = np.full(len(O), INF)
    rival = np.where(kind == 2, np.minimum(m["second"], np.minimum(fs, ls)), rival)
    rival = np.where(kind == 1, np.minimum(m["lo"], ls), rival)
    rival = np.where(kind == 0, np.minimum(m["lo"], fs), rival)
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        unique = (kind >= 0) & (rival - t_lo > band)
    wide = np.isfinite(t_hi) != np.isfinite(t_lo)
    with np.errstate(invalid="ignore"):
        wide |= np.isfinite(t_hi) & (t_hi - t_lo > band)
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        crowded = (kind == 2) & ~unique & ~m["edge"] & (m["second"] - t_lo <= band)
    obj = np.where(kind == 2, world.obj_idx(m["blas"], np.maximum(m["tri"], 0)), kind)
    return dict(t_hi=t_hi, t_lo=t_lo, kind=kind, kind_hi=kind_hi, unique=unique, uninformative=wide | crowded, scale=scale, obj=obj, blas=m["blas"], tri=m["tri"],
                u=m["u"], v=m["v"], slack=m["slack"], cond=1.0 + np.where(np.isfinite(m["cond"]), m["cond"], 0.0), mesh_hi=m["hi"], mesh_lo=m["lo"], floor=(fr, fs), light=(lr, ls), edge=m["edge"])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def nearest_violations(tr, hits):
    """the rays on which the hit records (fields t, u, v, objIdx, triIdx) break the criterion: {reason: indices}"""
    t = np.asarray(hits["t"], np.float64); obj = np.asarray(hits["objIdx"]); tri = np.asarray(hits["triIdx"])
    miss = obj < 0
    tt = tol("t") * tr["scale"]
    cond = tr["cond"]
    bad = {}
    bad["miss in front of a robust candidate"] = miss & np.isfinite(tr["t_hi"])
    bad["t beyond the nearest robust candidate"] = ~miss & (t > tr["t_hi"] + tt)
    bad["t in front of every soft candidate"] = ~miss & (t < tr["t_lo"] - tt)
    fs, ls = tr["floor"][1], tr["light"][1]
    bad["floor where the floor is not"] = (obj == 1) & ~(np.abs(t - fs) <= tt)
    bad["light where the light is not"] = (obj == 0) & ~(np.abs(t - ls) <= tt)
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        ident = tr["unique"] & ~miss & (tr["t_hi"] - tr["t_lo"] <= ID_BAND * tr["scale"])
    bad["another object"] = ident & (obj != tr["obj"])
    mesh = ident & (tr["kind"] == 2) & (obj == tr["obj"])
    bad["another triangle"] = mesh & (tri != tr["tri"])
    same = mesh & (tri == tr["tri"])
    bad["u"] = same & (np.abs(np.asarray(hits["u"], np.float64) - tr["u"]) > tol("u") * cond)
    bad["v"] = same & (np.abs(np.asarray(hits["v"], np.float64) - tr["v"]) > tol("v") * cond)
    return {k: np.flatnonzero(v) for k, v in bad.items() if v.any()}


def count(viol):
    return len(set(np.concatenate([v for v in viol.values()]).tolist())) if viol else 0


def rays_of(viol):
    return np.array(sorted(set(np.concatenate([v for v in viol.values()]).tolist())), np.int64) if viol else np.zeros(0, np.int64)


def nearest_deviation(tr, hits):
    """the observed deviations on rays with a tight interval and a unique identity the answer shares: {quantity: max of |got - truth| / its scale}"""
    t = np.asarray(hits["t"], np.float64); obj = np.asarray(hits["objIdx"]); tri = np.asarray(hits["triIdx"])
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        tight = tr["unique"] & (obj == tr["obj"]) & (tr["t_hi"] - tr["t_lo"] <= 1e-9 * tr["scale"])
    mesh = tight & (tr["kind"] == 2) & (tri == tr["tri"])
    cond = tr["cond"]
    out = dict(t=float((np.abs(t - tr["t_hi"]) / tr["scale"])[tight].max()) if tight.any() else 0.0, n=int(tight.sum()))
    for f in ("u", "v"):
        out[f] = float((np.abs(np.asarray(hits[f], np.float64) - tr[f]) / cond)[mesh].max()) if mesh.any() else 0.0
    return out


def check_caps(tr, what, min_mesh=MIN_MESH):
    """the conditions on a ray set; min_mesh = 0 only for `cluster`, whose truth is "no hit" on almost every ray"""
    n = len(tr["t_hi"])
    seen = dict(rays=n, uninformative=int(tr["uninformative"].sum()), mesh=int((tr["kind_hi"] == 2).sum()), prim=int(np.isin(tr["kind_hi"], (0, 1)).sum()),
                miss=int((tr["t_lo"] == INF).sum()), blases=len(set(tr["blas"][tr["kind_hi"] == 2].tolist())))
    print("%s: %s" % (what, seen))
    assert seen["uninformative"] <= MAX_UNINFORMATIVE * n, (what, seen)
    assert seen["mesh"] >= min_mesh and seen["prim"] >= MIN_PRIM and seen["miss"] >= MIN_MISS, (what, seen)
    return seen


def occluded_truth(world, O, D, t, tr=None):
    """(must be 1, may be 1) per shadow ray (O, D, t)"""
    O, D, t = np.asarray(O, np.float64), np.asarray(D, np.float64), np.asarray(t, np.float64)
    tr = tr if tr is not None else nearest_truth(world, O, D)
    band = tol("t") * tr["scale"]
    lr, ls = tr["light"]
    must = (lr < t - band) | np.isfinite(tr["mesh_hi"])
    may = (ls < t + band) | np.isfinite(tr["mesh_lo"])
    return must, may


def occluded_violations(must, may, got):
    got = np.asarray(got).astype(bool)
    return np.flatnonzero((must & ~got) | (~may & got))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# BVH::Refit
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def under_node1(nodes, tri_indices, n_tris):
    """the triangles in node 1's subtree"""
    under = np.zeros(n_tris, bool)
    stack = [1] if len(nodes) >= 2 else []
    while stack:
        k = stack.pop()
        if nodes["triCount"][k] > 0:
            under[tri_indices[nodes["leftFirst"][k]:nodes["leftFirst"][k] + nodes["triCount"][k]]] = True
        else:
            stack += [int(nodes["leftFirst"][k]), int(nodes["leftFirst"][k]) + 1]
    return under


def refit_excused(world, bvh, nodes, tri_indices, O, D, tr, whole_ray=False):
    """BVH::Refit (infra/bvh.cpp:26-43) skips node 1 (`if (i != 1)`), the root's left child here, so that node keeps the box it had before the vertices moved and
    a refitted tree does NOT return every nearest hit: the reference's own behaviour, which host, device and oracle refits restate.  A ray is excused from the
    criterion exactly where that explains it: the truth's nearest hit is a triangle under node 1, and the ray's segment up to that hit does not meet node 1's
    stale box (in the BVH's own space; 1e-5 * scale of overlap is left to float32), so the walk never reaches the triangle.  whole_ray (IsOccluded, which asks
    for ANY hit): the whole ray does not meet that box, so the walk reaches nothing under node 1.  An excused ray is not let go: refit_violations and
    refit_occluded_violations hold it to what the walk does reach.  Returns the mask."""
    n = len(O)
    if len(nodes) < 2:
        return np.zeros(n, bool)
    under = under_node1(nodes, tri_indices, len(world.v[bvh]))
    M = world.invT[bvh]
    o = np.asarray(O, np.float64) @ M[:3, :3].T + M[:3, 3]; d = np.asarray(D, np.float64) @ M[:3, :3].T
    with np.errstate(all="ignore"):
        t1 = (nodes["aabbMin"][1].astype(np.float64) - o) / d; t2 = (nodes["aabbMax"][1].astype(np.float64) - o) / d
    tmin, tmax = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
    t_hit = np.where(np.isfinite(tr["mesh_lo"]), tr["mesh_lo"], 0.0)
    overlap = np.minimum(tmax, t_hit) - np.maximum(tmin, 0.0)
    if whole_ray:
        return np.isfinite(tr["mesh_lo"]) & ~(tmax - np.maximum(tmin, 0.0) > 1e-5 * tr["scale"])
    mine = (tr["kind"] == 2) & (tr["blas"] == bvh)
    mine[mine] = under[tr["tri"][mine]]
    return mine & ~(overlap > 1e-5 * tr["scale"])


def without_node1(world, bvh, nodes, tri_indices):
    """the world a walk sees that never enters node 1 of BVH `bvh`: that subtree's triangles collapsed to a point (|a| = 0: no candidate; the others keep
    their numbers)"""
    tris = [np.array(t) for t in world.tris]
    under = under_node1(nodes, tri_indices, len(tris[bvh]))
    tris[bvh]["vertex1"][under] = tris[bvh]["vertex0"][under]; tris[bvh]["vertex2"][under] = tris[bvh]["vertex0"][under]
    return World(world.kind, tris, world.T if world.kind else None, world.invT if world.kind else None, world.light, world.obj_mat, world.floor_invto)


def refit_violations(reached, O, D, tr, hits, rays):
    """the rays among `rays` (excused by refit_excused: the segment up to the truth's hit does not meet node 1's stale box) whose answer the stale box does not
    explain either.  Beyond the lost hit the ray may still enter the box, so a farther triangle under node 1 may be the answer; but everything outside node 1 is
    walked as ever: the answer is not beyond the nearest robust candidate of `reached` (without_node1), a miss only where that world has none, and never in
    front of the full truth's nearest soft candidate."""
    rays = np.asarray(rays, np.int64)
    if not len(rays):
        return rays
    t2 = nearest_truth(reached, O[rays], D[rays])
    t = np.asarray(hits["t"], np.float64)[rays]; miss = np.asarray(hits["objIdx"])[rays] < 0
    tt = tol("t") * tr["scale"][rays]
    bad = (miss & np.isfinite(t2["t_hi"])) | (~miss & (t > t2["t_hi"] + tt)) | (~miss & (t < tr["t_lo"][rays] - tt))
    return rays[bad]


def refit_occluded_violations(reached, O, D, ts, rays):
    """the rays among `rays` (must be 1, answered 0, the whole ray clear of node 1's stale box) that have a robust occluder outside node 1: not explained"""
    rays = np.asarray(rays, np.int64)
    if not len(rays):
        return rays
    must, _ = occluded_truth(reached, O[rays], D[rays], np.asarray(ts)[rays])
    return rays[must]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GetHitInfo
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def hit_info_truth(world, O, D, tr, renormalise=True, flip=True):
    """GetHitInfo of the truth's own nearest hit, on the rays where it is unique and tight: dict(ok, I, N, uv, material, sure: the flip is not a coin toss,
    cond).  renormalise / flip = False: the doctored forms of the test."""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    n = len(O)
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        ok = tr["unique"] & np.isfinite(tr["t_hi"]) & (tr["t_hi"] - tr["t_lo"] <= ID_BAND * tr["scale"])
    t = np.where(ok, tr["t_hi"], 0.0)
    I = O + t[:, None] * D
    N = np.zeros((n, 3)); uv = np.zeros((n, 2)); mat = np.full(n, -1, np.int64)
    m = ok & (tr["kind"] == 0)
    N[m] = -world.light_R[:, 1]; mat[m] = 0                               # Quad::GetNormal: -(T's y column)
    m = ok & (tr["kind"] == 1)
    N[m] = [0.0, 1.0, 0.0]; mat[m] = 1
    f = I[m][:, [0, 2]] * world.floor_invto
    uv[m] = f - np.floor(f)
    for b, tris in enumerate(world.tris):
        m = ok & (tr["kind"] == 2) & (tr["blas"] == b)
        if not m.any():
            continue
        rec = tris[tr["tri"][m]]
        u, v = tr["u"][m, None], tr["v"][m, None]; w = 1.0 - u - v
        nn = w * rec["normal0"].astype(np.float64) + u * rec["normal1"] + v * rec["normal2"]
        uv[m] = w * rec["uv0"].astype(np.float64) + u * rec["uv1"] + v * rec["uv2"]
        if world.kind == 1:
            if not renormalise:                                             # the doctored form: a unit normal carried by T and left at that
                nn = nn / np.maximum(np.linalg.norm(nn, axis=1, keepdims=True), 1e-300)
            nn = nn @ world.T[b][:3, :3].T
            mat[m] = 2 + world.obj_mat[b]
        else:
            mat[m] = 2 + np.asarray(world.obj_mat)[rec["objIdx"] - 2]
        ln = np.linalg.norm(nn, axis=1, keepdims=True)
        N[m] = nn / np.maximum(ln, 1e-300) if (renormalise or world.kind == 0) else nn
        ok[np.flatnonzero(m)[ln[:, 0] < 1e-3]] = False                      # no normal to speak of
    dot = (N * D).sum(1)
    if flip:
        N = np.where((dot > 0)[:, None], -N, N)
    return dict(ok=ok, I=I, N=N, uv=uv, material=mat, sure=np.abs(dot) > 1e-3, cond=tr["cond"])


def hit_info_violations(tr, ti, hits, info):
    """the rays on which crt_hit_info records (fields I, N, u, v, material) break the truth's, where the hit records name the truth's own hit"""
    obj = np.asarray(hits["objIdx"]); tri = np.asarray(hits["triIdx"])
    m = ti["ok"] & (obj == tr["obj"]) & ((tr["kind"] != 2) | (tri == tr["tri"]))
    N = np.asarray(info["N"], np.float64); uv = np.stack([info["u"], info["v"]], 1).astype(np.float64)
    duv = np.abs(uv - ti["uv"]); duv = np.where(tr["kind"][:, None] == 1, np.minimum(duv, 1.0 - duv), duv)          # the floor's frac(): 0 and 1 are one place
    scale_uv = np.where(tr["kind"] == 1, tr["scale"], ti["cond"])
    bad = {}
    bad["I"] = m & (np.abs(np.asarray(info["I"], np.float64) - ti["I"]).max(1) > tol("I") * tr["scale"])
    bad["N"] = m & ti["sure"] & (np.abs(N - ti["N"]).max(1) > tol("N") * ti["cond"])
    bad["N up to its sign"] = m & ~ti["sure"] & (np.minimum(np.abs(N - ti["N"]).max(1), np.abs(N + ti["N"]).max(1)) > tol("N") * ti["cond"])
    bad["uv"] = m & (duv.max(1) > tol("uv") * scale_uv)
    bad["material"] = m & (np.asarray(info["material"]) != ti["material"])
    return {k: np.flatnonzero(v) for k, v in bad.items() if v.any()}, int(m.sum())


def hit_info_deviation(tr, ti, hits, info):
    obj = np.asarray(hits["objIdx"]); tri = np.asarray(hits["triIdx"])
    with np.errstate(invalid="ignore"):                                  # (inf - inf where a ray has no candidate at all: NaN compares false)
        m = ti["ok"] & ti["sure"] & (obj == tr["obj"]) & ((tr["kind"] != 2) | (tri == tr["tri"])) & (tr["t_hi"] - tr["t_lo"] <= 1e-9 * tr["scale"])
    if not m.any():
        return dict(I=0.0, N=0.0, uv=0.0)
    uv = np.stack([info["u"], info["v"]], 1).astype(np.float64)
    duv = np.abs(uv - ti["uv"]); duv = np.where(tr["kind"][:, None] == 1, np.minimum(duv, 1.0 - duv), duv)
    scale_uv = np.where(tr["kind"] == 1, tr["scale"], ti["cond"])
    return dict(I=float((np.abs(np.asarray(info["I"], np.float64) - ti["I"]).max(1) / tr["scale"])[m].max()),
                N=float((np.abs(np.asarray(info["N"], np.float64) - ti["N"]).max(1) / ti["cond"])[m].max()),
                uv=float((duv.max(1) / scale_uv)[m].max()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------------------------------------
CLASSES = ("aimed", "camera", "bounce", "shadow")
SHARES = (0.62, 0.12, 0.13, 0.13)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _as_rays(O, D):
    """float32 rays without a zero direction component (the KD walk treats axis-parallel rays specially)"""
    D = _unit(np.asarray(D, np.float64))
    D = np.where(np.abs(D) < 1e-4, np.where(D < 0, -1e-4, 1e-4), D)
    D = _unit(D).astype(np.float32)
    assert (D != 0).all()
    return np.asarray(O, np.float32), D


def make_rays(world, n, seed, near=None, aim=None):
    """(O, D float32 [n, 3], class [n]) for a world: aimed rays from a sphere round the meshes towards triangle centroids (a fifth of them pushed aside so that
    some miss), camera rays with sub-pixel jitter, bounce rays that start 1e-3 off a hit surface in random directions, shadow rays towards the light quad.
    aim: the share of the aimed rays per BVH (default: by its share of the triangles).
    near: the aimed rays start this far from the centroid they aim at instead (AIMED_FROM: a mesh whose triangles are too thin to be judged from the sphere).
    Where 1e-3 is within four times t's own tolerance at the magnitudes in play (a mesh 100 across), the bounce and shadow rays start that far off instead: a ray
    that starts within the tolerance of the surface it left has that surface as a soft candidate at t = 0 and says nothing."""
    rng = np.random.default_rng(seed)
    wv = np.concatenate(world.world_v).reshape(-1, 3, 3)
    cen = wv.mean(1)
    c0 = 0.5 * (cen.min(0) + cen.max(0)); r = max(float(np.linalg.norm(cen - c0, axis=1).max()), 0.05)
    counts = [int(round(s * n)) for s in SHARES]; counts[0] += n - sum(counts)
    # aimed
    k = counts[0]
    d = _unit(rng.normal(size=(k, 3))); d[:, 1] = np.abs(d[:, 1]) * 0.8 + 0.05
    if aim is None:
        tgt = cen[rng.integers(0, len(cen), k)]
    else:
        sizes = np.diff(world.first)
        tgt = cen[rng.choice(len(cen), k, p=np.repeat(np.asarray(aim, np.float64) / sizes, sizes))]
    Oa = c0 + (2.5 * r + 1.0) * _unit(d) if near is None else tgt + near * _unit(d)
    Oa[:, 1] = np.maximum(Oa[:, 1], -0.8)
    aside = rng.random(k) < 0.2
    push = _unit(rng.normal(size=(k, 3))); push[:, 1] = np.abs(push[:, 1])                 # upwards: towards the sky rather than the floor
    tgt = tgt + aside[:, None] * push * rng.uniform(0.4, 1.6, (k, 1)) * r
    Da = tgt - Oa
    # camera: looking at the meshes from in front and a little above, 64 x 64 pixels, jittered
    k = counts[1]
    cam = at.camera_state(c0 + [0.0, 0.4 * r + 0.3, -(2.0 * r + 1.5)], c0, 64, 64)
    Dc = at.primary_dirs(cam, 64, 64, rng.uniform(0, 64, k), rng.uniform(0, 64, k))
    Oc = np.broadcast_to(cam[0], (k, 3))
    O1, D1 = _as_rays(np.concatenate([Oa, Oc]), np.concatenate([Da, Dc]))
    first = nearest_truth(world, O1, D1)
    # surface points: the robust unique mesh hits of those rays, and floor points
    hit = np.flatnonzero((first["kind_hi"] == 2) & first["unique"] & ~first["uninformative"])
    if len(hit) >= 16:
        g = world.first[first["blas"][hit]] + first["tri"][hit]
        P = O1[hit].astype(np.float64) + first["t_hi"][hit, None] * D1[hit].astype(np.float64)
        Ng = _unit(_cross(wv[g, 1] - wv[g, 0], wv[g, 2] - wv[g, 0]))
        Ng = np.where(((Ng * D1[hit]).sum(1) > 0)[:, None], -Ng, Ng)
        off = np.maximum(1e-3, 4 * (REL * T_MIN + tol("t") * np.maximum(np.maximum(1.0, np.linalg.norm(P, axis=1)), world.extent)))
        P = P + off[:, None] * Ng
    else:                                                                   # a mesh that is all but invisible (`cluster`): points beside its triangles
        hit = np.arange(64)
        P = cen[rng.integers(0, len(cen), 64)] + 1e-3 * _unit(rng.normal(size=(64, 3)))
    k = counts[2]
    pick = rng.integers(0, len(hit), k)
    Ob, Db = P[pick], _unit(rng.normal(size=(k, 3)))
    k = counts[3]
    half = k // 2
    pick = rng.integers(0, len(hit), half)
    fl = np.stack([c0[0] + rng.uniform(-2 * r - 1, 2 * r + 1, k - half), np.full(k - half, -1.0 + 1e-3), c0[2] + rng.uniform(-2 * r - 1, 2 * r + 1, k - half)], 1)
    Os = np.concatenate([P[pick], fl])
    Ds = world.light + np.stack([rng.uniform(-0.7, 0.7, k), np.zeros(k), rng.uniform(-0.7, 0.7, k)], 1) - Os
    O2, D2 = _as_rays(np.concatenate([Ob, Os]), np.concatenate([Db, Ds]))
    cls = np.repeat(np.arange(4), counts)
    return np.concatenate([O1, O2]), np.concatenate([D1, D2]), cls


def shadow_lengths(tr, seed):
    """a `t` per ray for IsOccluded: before the nearest robust candidate, beyond it, or far away, a third each"""
    rng = np.random.default_rng(seed)
    base = np.where(np.isfinite(tr["t_hi"]), tr["t_hi"], 10.0)
    return (base * rng.choice([0.5, 2.0, 100.0], len(base))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the generated two-level scene
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# cube.obj (corners +-1).  The reference bakes an object's SCALE into its BLAS's vertices and keeps T = Translate * Rotate rigid (tlas_file_scene.cpp:46-51), so
# a scene file alone never makes invT scale d.  SetTransform does (blas_bvh.cpp:363-366: invT = FastInvertedTransformNoScale(T), the transposed 3 x 3 part): under
# T = Translate * R * Scale(s) it is s R^T, NOT T's inverse — the BLAS appears at 1 / s of its size, d is s long, and every |a| is s times the world's.  The TLAS
# keeps the box of T (s times the BLAS), which holds what appears only for s >= 1: s = 2 is used, and 0.3 is a scale of the scene file.
#   0  a cube of scale 0.3, turned about all three axes
#   1  a cube of scale 0.5 under a T of scale 2: it appears with half size 0.25
#   2  a cube of scale 0.0045 (edge 0.009, |a| <= 8.1e-5 for a unit d) under a T of scale 2: it appears with half size 0.00225; in object space |a| doubles to
#      <= 1.62e-4, so a face is VISIBLE where the ray's cosine to it is above 0.617 — in world units |a| <= 2.0e-5, below the threshold everywhere
#   3  a cube of scale 0.0065 (|a| <= 1.69e-4 for a unit d) under a rigid T: a face is visible where the cosine is above 0.59, and INVISIBLE below it
GEN_OBJECTS = [dict(position=(-1.3, -0.2, 3.0), rotation=(20.0, 35.0, 10.0), scale=0.3), dict(position=(0.9, -0.3, 3.4), rotation=(0.0, 50.0, 15.0), scale=0.5),
               dict(position=(0.0, 0.2, 2.5), rotation=(10.0, 20.0, 30.0), scale=0.0045), dict(position=(-0.3, -0.4, 2.2), rotation=(25.0, -15.0, 5.0), scale=0.0065)]
GEN_T_SCALE = (1.0, 2.0, 2.0, 1.0)
GEN_LIGHT = (0.0, 3.0, 2.5)
GEN_AIM = (0.45, 0.45, 0.05, 0.05)             # a tenth of the aimed rays go to the two tiny cubes (tiny_cube_rays adds what the threshold test needs), so that
#                                                the two-level KD-tree, which loses hits on cubes that small, is held to the truth on most of the set


def write_generated(tmp_path, write_scene):
    ob = [("cube", 0, o["position"], o["rotation"], (o["scale"],) * 3) for o in GEN_OBJECTS]
    return write_scene(tmp_path, "cube", name="mesh_truth_gen.xml", pos=ob[0][2], rot=ob[0][3], scale=ob[0][4], extra_objects=ob[1:], light=GEN_LIGHT)


def generated_transforms(scene):
    """the transforms the generated scene is moved to: what the scene file gave, times Scale(GEN_T_SCALE[i]) — float32 row-major mat4s"""
    out = []
    for i, s in enumerate(GEN_T_SCALE):
        T = np.array(scene.blas_transform(i)[0], np.float32).reshape(4, 4)
        T[:3, :3] *= np.float32(s)
        out.append(T)
    return np.stack(out)


def tiny_cube_rays(world, blas, n, seed):
    """n rays from all round towards points inside the box that BLAS `blas` appears as"""
    rng = np.random.default_rng(seed)
    wv = world.world_v[blas]
    c = 0.5 * (wv.min(0) + wv.max(0)); h = 0.5 * (wv.max(0) - wv.min(0)).max()
    d = _unit(rng.normal(size=(n, 3))); d[:, 1] = np.abs(d[:, 1])
    O = c + 1.5 * d
    return _as_rays(O, c + rng.uniform(-0.4, 0.4, (n, 3)) * h - O)


def threshold_dependent(world, O, D, tr):
    """the rays whose answer depends on WHERE |a| >= 1e-4 is evaluated: without the threshold their nearest candidate is nearer than with it (a face is
    invisible), or a face they robustly hit has |a| below 1e-4 for the unit world direction (it is visible only because invT scales d)"""
    free = mesh_candidates(world, O, D, a_min=0.0)
    invisible = np.isfinite(free["hi"]) & ~(tr["mesh_lo"] <= free["hi"] + ID_BAND)
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    wv = np.concatenate(world.world_v).reshape(-1, 3, 3)
    hit = (tr["kind_hi"] == 2) & tr["unique"]
    g = world.first[np.maximum(tr["blas"], 0)] + np.maximum(tr["tri"], 0)
    a_world = np.abs((_cross(D, wv[g, 2] - wv[g, 0]) * (wv[g, 1] - wv[g, 0])).sum(1))
    visible = hit & (a_world < A_MIN * (1 - REL))
    return invisible, visible
