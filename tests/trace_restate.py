"""float32 restatement of the Whitted renderer's Trace ("2. WhittedStyle/renderer.cpp":21-91, DirectIllumination :105-126) for ARRAYS of rays, operation by
operation in np.float32 with nothing fused.  The oracle has no per-ray Trace (orc_whitted_render traces its camera's pixels only), so the recursion is written out
here over what the oracle does export:

    orc_find_nearest        scene.FindNearest                    (the nearest hit, Ray::traversed / Ray::tested)
    orc_is_occluded         scene.IsOccluded                     (DirectIllumination's shadow ray)
    orc_probe_expected      the deterministic expf               (the medium's absorption)
    hit_info_restate        GetHitInfo, GetAlbedo, GetSkyColor   (itself pinned to the oracle by tests/test_hit_info_cpu.py)

A level of the recursion is one batch: every ray of the level through FindNearest at once, then the child rays of the level — all refracted / mirrored rays, then
all Fresnel reflections — as the next batches.  Trace is deterministic, so the order in which the children are evaluated does not change a value; the sums are
formed in the reference's order, out = ((0 + cA * Trace(a)) + cB * Trace(b)) + C, return medium * out.

tests/test_trace_restate_cpu.py pins this module to orc_whitted_render bit for bit; tests/test_gpu_trace_query.py then uses it as the yardstick for rays no camera
produces.  Nothing here touches the library under test."""
import numpy as np

import hit_info_restate as hr
from hit_info_restate import EPS, F, INVPI, dot, f32

LIGHT_COLOR = f32([24, 24, 22])
AMBIENT = f32([0.3, 0.3, 0.3])


def _m(a, b):
    return (a * b).astype(F)


def _col(s):
    return s[:, None]


class Tracer:
    """Trace over the scene `o` (an orc.Oracle, FileScene or TLASFileScene) that `sh` (hit_info_restate.SceneShading) describes"""

    def __init__(self, orc, o, sh, depth_limit=5):
        self.orc, self.o, self.sh, self.depth_limit = orc, o, sh, int(depth_limit)
        mats = sh.materials
        # per crt_hit_info.material: 0 the light, 1 the floor (a plain textured material), 2 + k the scene file's material k
        self.refl = f32([0, 0] + [m["reflectivity"] for m in mats])
        self.refr = f32([0, 0] + [m["refractivity"] for m in mats])
        self.absorb = f32([[0, 0, 0], [0, 0, 0]] + [m["absorption"] for m in mats]).reshape(-1, 3)
        self.light_pos = sh.light_pos()

    def expf(self, x):
        x = np.ascontiguousarray(x, F)
        return self.orc.probe_expected("EXPF", x.reshape(-1, 1)).view(F)[:, 0].reshape(x.shape)

    def direct(self, I, N):
        """DirectIllumination (renderer.cpp:105-126)"""
        n = len(I)
        irr = np.zeros((n, 3), F)
        if n == 0:
            return irr
        with np.errstate(all="ignore"):
            L = (self.light_pos[None, :] - I).astype(F)
            dist = np.sqrt(dot(L, L)).astype(F)
            L = _m(L, _col((F(1) / dist).astype(F)))
            ndotl = dot(N, L)
            go = ~(ndotl < EPS)
            if go.any():
                org = (I[go] + _m(L[go], EPS)).astype(F)
                t = (dist[go] - _m(F(2), EPS)).astype(F)
                free = self.o.is_occluded(org, L[go], t) == 0
                att = (F(1) / _m(dist[go], dist[go])).astype(F)
                inr = _m(LIGHT_COLOR[None, :], _col(att))
                lit = _m(inr, _col(dot(N[go], L[go])))
                lit[~free] = 0
                irr[go] = lit
        return irr

    def trace(self, O, D, inside=None, depth=0, counts=None):
        """Trace(Ray(O, D) with ray.inside, depth) per ray -> [n, 3] float32.  counts: a dict that receives the depth-0 rays' "traversed" / "tested" and "cost",
        the FindNearest calls of each ray's whole tree."""
        O, D = f32(O).reshape(-1, 3), f32(D).reshape(-1, 3)
        n = len(O)
        inside = np.zeros(n, bool) if inside is None else np.broadcast_to(np.asarray(inside) != 0, (n,)).copy()
        res = np.zeros((n, 3), F)
        cost = np.zeros(n, np.int64)
        if counts is not None and depth == 0:
            counts["traversed"] = np.zeros(n, np.int32); counts["tested"] = np.zeros(n, np.int32)
        if depth > self.depth_limit or n == 0:                                # if (depth > depthLimit) return float3(0), ahead of the trace
            if counts is not None:
                counts["cost"] = cost
            return res
        hits = self.o.find_nearest(O, D, inside.astype(np.int32))
        cost += 1
        if counts is not None and depth == 0:
            counts["traversed"], counts["tested"] = hits["traversed"].copy(), hits["tested"].copy()
        info = self.sh.hit_info(O, D, hits)
        mat = info["material"]
        miss, light = mat == hr.MATERIAL_MISS, mat == 0
        res[miss] = info["albedo"][miss]                                      # scene.GetSkyColor(ray)
        res[light] = LIGHT_COLOR
        s = np.flatnonzero(mat >= 1)
        if len(s):
            with np.errstate(all="ignore"):
                Ds, I, N, alb, ins, t = D[s], info["I"][s], info["N"][s], info["albedo"][s], inside[s], f32(hits["t"][s])
                refl, refr = self.refl[mat[s]], self.refr[mat[s]]
                diffuseness = (F(1) - (refl + refr).astype(F)).astype(F)
                out = np.zeros((len(s), 3), F)
                R = (Ds - _m(_m(F(2), N), _col(dot(N, Ds)))).astype(F)         # reflect(ray.D, N) = D - 2.0f * N * dot(N, D)
                RO = (I + _m(R, EPS)).astype(F)
                sub = {}
                a = refl > 0                                                  # renderer.cpp:49-54
                if a.any():
                    c = {}
                    tr = self.trace(RO[a], R[a], np.zeros(int(a.sum()), bool), depth + 1, c)
                    out[a] = (out[a] + _m(_m(_col(refl[a]), alb[a]), tr)).astype(F)
                    sub[("a", 0)] = (a, c["cost"])
                b = ~a & (refr > 0)                                           # renderer.cpp:55-72
                if b.any():
                    one = np.ones(int(b.sum()), F)
                    n1 = np.where(ins[b], F(1.2), F(1)).astype(F); n2 = np.where(ins[b], F(1), F(1.2)).astype(F)
                    eta = (n1 / n2).astype(F); cosi = dot(-Ds[b], N[b])
                    cost2 = (F(1) - _m(_m(eta, eta), (one - _m(cosi, cosi)).astype(F))).astype(F)
                    go = cost2 > 0
                    Fr = np.ones(int(b.sum()), F)
                    aa, bb = (n1 - n2).astype(F), (n1 + n2).astype(F)
                    R0 = (_m(aa, aa) / _m(bb, bb)).astype(F); cc = (one - cosi).astype(F)
                    Fr[go] = (R0 + _m((one - R0).astype(F), _m(_m(_m(_m(cc, cc), cc), cc), cc))).astype(F)[go]
                    T = (_m(_col(eta), Ds[b]) + _m(_col((_m(eta, cosi) - np.sqrt(np.abs(cost2)).astype(F)).astype(F)), N[b])).astype(F)
                    ob = out[b]
                    bi = np.flatnonzero(b)
                    if go.any():
                        c = {}
                        tr = self.trace((I[b][go] + _m(T[go], EPS)).astype(F), T[go], ~ins[b][go], depth + 1, c)
                        ob[go] = (ob[go] + _m(_m(alb[b][go], _col((one - Fr).astype(F)[go])), tr)).astype(F)
                        m = np.zeros(len(s), bool); m[bi[go]] = True
                        sub[("b", 0)] = (m, c["cost"])
                    c = {}
                    tr = self.trace(RO[b], R[b], np.zeros(int(b.sum()), bool), depth + 1, c)
                    ob = (ob + _m(_m(alb[b], _col(Fr)), tr)).astype(F)
                    out[b] = ob
                    sub[("b", 1)] = (b, c["cost"])
                d = diffuseness > 0                                           # renderer.cpp:74-80
                if d.any():
                    irr = self.direct(I[d], N[d])
                    brdf = _m(alb[d], INVPI)
                    out[d] = (out[d] + _m(_m(_col(diffuseness[d]), brdf), (irr + AMBIENT[None, :]).astype(F))).astype(F)
                medium = np.ones((len(s), 3), F)
                if ins.any():
                    medium[ins] = self.expf(_m(self.absorb[mat[s]][ins], _col(-t[ins])))
                res[s] = _m(medium, out)
                for m, c in sub.values():
                    cost[s[m]] += c
        if counts is not None:
            counts["cost"] = cost
        return res


def pixel_rays(o, W, H):
    """Trace(camera.GetPrimaryRay((float)x, (float)y)) of Renderer::Tick, row-major"""
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.float32)
    return o.primary_rays(xy)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(a, b):
    """rows in which two float32 arrays differ as bit patterns (any NaN equals any NaN)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return np.flatnonzero(((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))).reshape(len(a), -1).any(axis=1))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the two scenes of the Trace tests and their cameras
# ---------------------------------------------------------------------------------------------------------------------------------------------------
W, H = 64, 48
# a FileScene of three cubes on the floor: a full mirror, a dielectric with absorption, a half mirror (the other half diffuse)
MATS = [(1.0, 0.0, (0.0, 0.0, 0.0), ""),
        (0.0, 1.0, (0.5, 0.2, 0.1), ""),
        (0.5, 0.0, (0.0, 0.0, 0.0), "")]
MIRROR_C, GLASS_C, HALF_C = (-1.3, -0.5, 2.6), (0.0, -0.5, 2.0), (1.3, -0.5, 2.6)
EXTRA = [("cube", 1, GLASS_C, (0.0, 20.0, 0.0), (0.5, 0.5, 0.5)), ("cube", 2, HALF_C, (0.0, -35.0, 0.0), (0.5, 0.5, 0.5))]
# cameras chosen with the oracle alone (a search over positions and targets for the largest smallest class; test_trace_restate_cpu.py asserts what each image
# holds): the light quad, the sky, the floor and every mesh material in one 64 x 48 image
CAMERAS = {"cubes": ((0.6, 2.0, -2.1), (0.7, 1.9, -1.1)), "tlas": ((1.4, 0.4, -2.0), (1.0, 0.5, -1.0))}


def cubes_xml(tmp_path):
    from test_gpu_golden_and_edges import write_scene
    return write_scene(tmp_path, "cube", name="trace_cubes.xml", pos=MIRROR_C, rot=(0.0, 30.0, 0.0), scale=(0.5, 0.5, 0.5), mats=MATS, extra_objects=EXTRA)


def scene_of(name, tmp_path, assets_scenes):
    """(xml path, scene kind) of scene `name`: "cubes" (FileScene, written to tmp_path) or "tlas" (assets/scenes/tlas_scene.xml as a TLASFileScene)"""
    import os
    return (cubes_xml(tmp_path), 0) if name == "cubes" else (os.path.join(assets_scenes, "tlas_scene.xml"), 1)


def load(orc, xml, kind, assets, name, depth_limit=5):
    """the oracle of the scene with the renderer at W x H and the scene's camera, its shading restatement and its Tracer"""
    o, sc = orc.load_scene(xml, kind, assets)
    o.renderer_init(W, H)
    o.set_camera_state(*CAMERAS[name])
    o.set_params(depth_limit=depth_limit, passes=1)
    sh = hr.SceneShading(orc, o, sc, kind, assets)
    return o, sh, Tracer(orc, o, sh, depth_limit)


def pixel_classes(tr, o):
    """what the primary rays of the W x H image hit: counts of sky, floor, light, and per material class mirror (reflectivity 1), dielectric, half mirror, diffuse"""
    O, D = pixel_rays(o, W, H)
    info = tr.sh.hit_info(O, D, o.find_nearest(O, D))
    mat = info["material"]
    refl, refr = tr.refl[np.maximum(mat, 0)], tr.refr[np.maximum(mat, 0)]
    mesh = mat >= 2
    return dict(sky=int((mat == -1).sum()), light=int((mat == 0).sum()), floor=int((mat == 1).sum()), mirror=int((mesh & (refl == 1)).sum()),
                half_mirror=int((mesh & (refl > 0) & (refl < 1)).sum()), dielectric=int((mesh & (refr > 0) & (refl == 0)).sum()), diffuse=int((mesh & (refl == 0) & (refr == 0)).sum()))
