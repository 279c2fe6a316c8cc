"""float32 restatement of the reference's shading queries, operation by operation in np.float32 with nothing fused:

    BaseScene::GetHitInfo       infra/scene/file_scene.cpp:189-214, infra/scene/tlas_file_scene.cpp:220-260
    Material::GetAlbedo(uv)     template/material.h (the material's texture at uv, or float3(1))
    BaseScene::GetSkyColor      infra/scene/file_scene.cpp:142-154
    Trace's diffuse arm and DirectIllumination of the Whitted renderer, as oracle/crt_oracle.cpp:1465-1526 restates "2. WhittedStyle/renderer.cpp":21-126

Its inputs are the oracle's: o.bvh(i)["tris"] (normals, uvs, objIdx), o.blas_transform(i), the scene file's materials, orc.read_image + orc.texture_sample (the
oracle's Texture::Sample, pinned to the real texture.h by tests/test_oracle_pinning.py).  tests/test_hit_info_cpu.py pins this module to the oracle's Whitted
image and to its Sample of a miss on the CPU; the GPU tests then use it as the yardstick for crt_get_hit_info / crt_get_sky_color.

Nothing here touches the library under test."""
import os

import numpy as np

F = np.float32
PI = F(3.14159265358979323846264)            # template/common.h:8
INVPI = F(0.31830988618379067153777)         # :9
INV2PI = F(0.15915494309189533576888)        # :10
EPS = F(0.001)                               # renderer.h:12
MATERIAL_MISS, MATERIAL_INVALID = -1, -2
HIT_INFO_DTYPE = np.dtype([("I", "<f4", 3), ("material", "<i4"), ("N", "<f4", 3), ("u", "<f4"), ("albedo", "<f4", 3), ("v", "<f4")])


def f32(x):
    return np.asarray(x, F)


def dot(a, b):
    """dot(float3, float3) = a.x * b.x + a.y * b.y + a.z * b.z, summed left to right (tmplmath.h:458)"""
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def normalize(v):
    """normalize(float3) = v * (1 / sqrtf(dot(v, v))) (tmplmath.h:480 with rsqrtf = 1 / sqrtf, tmplmath.h:124)"""
    with np.errstate(all="ignore"):
        inv = (F(1) / np.sqrt(dot(v, v)).astype(F)).astype(F)
    return (v * inv[..., None]).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the deterministic atan2 / acos GetSkyColor goes through (oracle/crt_oracle.cpp:110-166; DESIGN.md "numerics")
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _atan_pos(x):
    x = f32(x)
    with np.errstate(all="ignore"):
        big, mid = x > F(2.414213562373095), x > F(0.4142135623730950)
        y0 = np.where(big, F(1.5707963267948966), np.where(mid, F(0.7853981633974483), F(0))).astype(F)
        t = np.where(big, -(F(1) / x).astype(F), np.where(mid, ((x - F(1)).astype(F) / (x + F(1)).astype(F)).astype(F), x)).astype(F)
        z = (t * t).astype(F)
        p = np.full(x.shape, F(8.05374449538e-2), F)
        p = ((p * z).astype(F) - F(1.38776856032e-1)).astype(F)
        p = ((p * z).astype(F) + F(1.99777106478e-1)).astype(F)
        p = ((p * z).astype(F) - F(3.33329491539e-1)).astype(F)
        p = (((p * z).astype(F) * t).astype(F) + t).astype(F)
        return (y0 + p).astype(F)


def det_atan2(y, x):
    y, x = f32(y), f32(x)
    sy = y.view(np.uint32) & np.uint32(0x80000000)
    sx = (x.view(np.uint32) & np.uint32(0x80000000)) != 0
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        a = _atan_pos((ay / ax).astype(F))
        r = np.where(sx, (PI - a).astype(F), a).astype(F)
        r = np.where(np.isinf(ax) & np.isinf(ay), np.where(sx, F(2.356194490192345), F(0.7853981633974483)), r).astype(F)
        r = np.where(ax == 0, F(1.5707963267948966), r).astype(F)
        r = np.where(ay == 0, np.where(sx, PI, F(0)), r).astype(F)
    r = (r.view(np.uint32) | sy).view(F)
    return np.where(np.isnan(x) | np.isnan(y), (x + y).astype(F), r).astype(F)


def _asin_small(x):
    z = (x * x).astype(F)
    p = np.full(x.shape, F(4.2163199048e-2), F)
    p = ((p * z).astype(F) + F(2.4181311049e-2)).astype(F)
    p = ((p * z).astype(F) + F(4.5470025998e-2)).astype(F)
    p = ((p * z).astype(F) + F(7.4953002686e-2)).astype(F)
    p = ((p * z).astype(F) + F(1.6666752422e-1)).astype(F)
    return (((p * z).astype(F) * x).astype(F) + x).astype(F)


def det_acos(x):
    x = f32(x)
    with np.errstate(all="ignore"):
        hi, lo = x > F(0.5), x < F(-0.5)
        s_hi = np.sqrt((F(0.5) * (F(1) - x).astype(F)).astype(F)).astype(F)
        s_lo = np.sqrt((F(0.5) * (F(1) + x).astype(F)).astype(F)).astype(F)
        r = np.where(hi, (F(2) * _asin_small(s_hi)).astype(F),
                     np.where(lo, (PI - (F(2) * _asin_small(s_lo)).astype(F)).astype(F), (F(1.5707963267948966) - _asin_small(x)).astype(F))).astype(F)
        r = np.where((x > F(1)) | (x < F(-1)), F(np.nan), r).astype(F)
    return np.where(np.isnan(x), x, r).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the scene as GetHitInfo sees it
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class SceneShading:
    """What GetHitInfo / GetAlbedo / GetSkyColor read of a FileScene (kind 0) or TLASFileScene (kind 1) `o` that orc.load_scene built from the description `sc`.
    set_look: the scene under a look of crt_update_look / crt_render_looks instead of the file's own."""

    def __init__(self, orc, o, sc, kind, base_dir):
        def rp(p):
            return p if os.path.isabs(p) else os.path.normpath(os.path.join(base_dir, p))
        self.orc, self.kind = orc, int(kind)
        self.floor_tex = orc.pack_rgb(orc.read_image(rp(sc["plane_texture"])))
        self.sky_tex = orc.pack_rgb(orc.read_image(rp(sc["skydome"])))
        self.mat_tex = [orc.pack_rgb(orc.read_image(rp(m["texture"]))) if m["texture"] else None for m in sc["materials"]]
        self.materials = sc["materials"]
        self.obj_mat = [ob["material_idx"] for ob in sc["objects"]]          # models[i]->matIdx (FileScene) / blas[i]->matIdx (two-level)
        self.light = f32(sc["light"])
        self.light_T = np.eye(4, dtype=F)                                    # T = Translate(light position), file_scene.cpp:18
        self.light_T[0, 3], self.light_T[1, 3], self.light_T[2, 3] = self.light
        self.tris = [o.bvh(i)["tris"] for i in range(o.bvh_count())]
        self.refresh_transforms(o)
        self.floor_n = f32([0, 1, 0])                                        # Plane floor(1, float3(0, 1, 0), 1, texW / 100), file_scene.cpp:16
        self.floor_invto = F(1) / F(self.floor_tex.shape[1] // 100)          # invto = 1 / (float)(texW / 100), the division an integer one
        self.objects = len(sc["objects"])

    def refresh_transforms(self, o):
        self.T = [o.blas_transform(i)[0].reshape(4, 4) for i in range(o.bvh_count())] if self.kind == 1 else None

    def set_look(self, look):
        """the look's light T, and its floor, sky and material textures by index into the scene's texture list ([0] the file's floor texture, [1] its skydome,
        then the materials' in file order).  The floor plane's uv scale is NOT part of a look: floor_invto stays the uploaded floor texture's
        (file_scene.cpp:16 runs once, at construction), whatever width the selected texture has."""
        if not hasattr(self, "textures"):
            self.textures = [self.floor_tex, self.sky_tex] + [t for t in self.mat_tex if t is not None]
        self.light_T = f32(look["light_T"]).reshape(4, 4).copy()
        self.light = self.light_T[:3, 3].copy()
        self.floor_tex, self.sky_tex = self.textures[look["floor_texture"]], self.textures[look["sky_texture"]]
        assert len(look["materials"]) == len(self.materials)
        self.mat_tex = [self.textures[t] if t >= 0 else None for _, _, _, t in look["materials"]]
        self.materials = [dict(reflectivity=a, refractivity=b, absorption=c) for a, b, c, _ in look["materials"]]

    def light_normal(self):
        """Quad::GetNormal (primitives.h:363-367): (-T[1], -T[5], -T[9]) of the quad's T"""
        T = self.light_T
        return f32([-T[0, 1], -T[1, 1], -T[2, 1]])

    def light_pos(self):
        """GetLightPos (file_scene.cpp:156-162): (c1 + c2) * 0.5f - (0, 0.01f, 0), the corners through the scalar TransformPosition"""
        T = self.light_T                                                     # (the corners are +-0.5 whatever the quad's size, and 0.01 down in WORLD y)

        def tp(a):
            return f32([(((T[r, 0] * a[0]).astype(F) + (T[r, 1] * a[1]).astype(F)).astype(F) + (T[r, 2] * a[2]).astype(F)).astype(F) + (T[r, 3] * F(1)).astype(F) for r in range(3)])
        c1, c2 = tp(f32([-0.5, 0, -0.5])), tp(f32([0.5, 0, 0.5]))
        return (((c1 + c2).astype(F) * F(0.5)).astype(F) - f32([0, 0.01, 0])).astype(F)

    def sky(self, D):
        """GetSkyColor (file_scene.cpp:142-154)"""
        D = f32(D).reshape(-1, 3)
        phi = (det_atan2(-D[:, 2], D[:, 0]) + PI).astype(F)
        theta = det_acos(-D[:, 1])
        uv = np.stack([(phi * INV2PI).astype(F), (theta * INVPI).astype(F)], 1)
        return self.orc.texture_sample(self.sky_tex, uv)

    def albedo(self, tex, uv):
        """Material::GetAlbedo(uv)"""
        if tex is None:
            return np.ones((len(uv), 3), F)
        return self.orc.texture_sample(tex, uv)

    def hit_info(self, O, D, hits, with_flip=False):
        """crt_hit_info records (HIT_INFO_DTYPE) for rays O / D and their hit records (fields t, u, v, objIdx, triIdx); with_flip: also the mask of the records
        whose normal GetHitInfo turned round (it faced away from the ray's origin)"""
        O, D = f32(O).reshape(-1, 3), f32(D).reshape(-1, 3)
        n = len(O)
        out = np.zeros(n, HIT_INFO_DTYPE)
        obj = np.asarray(hits["objIdx"]); tri = np.asarray(hits["triIdx"])
        t, bu, bv = f32(hits["t"]), f32(hits["u"]), f32(hits["v"])
        N = np.zeros((n, 3), F); uv = np.zeros((n, 2), F); alb = np.zeros((n, 3), F); mat = np.full(n, MATERIAL_MISS, np.int32)
        with np.errstate(all="ignore"):
            I = (O + (t[:, None] * D).astype(F)).astype(F)                      # float3 I = ray.O + ray.t * ray.D
        miss = obj == -1
        I[miss] = 0
        if miss.any():
            alb[miss] = self.sky(D[miss])                                        # what Trace / Sample return for a miss
        m = obj == 0                                                             # case 0: the light
        N[m] = self.light_normal(); mat[m] = 0; alb[m] = 1                       # primitiveMaterials[0] has no texture
        m = obj == 1                                                             # case 1: the floor, Plane::GetNormal / GetUV (primitives.h:112-133)
        if m.any():
            N[m] = self.floor_n; mat[m] = 1
            if self.floor_n[1] == 1:
                u = (I[m, 0] * self.floor_invto).astype(F); v = (I[m, 2] * self.floor_invto).astype(F)
                uv[m, 0] = (u - np.floor(u)).astype(F); uv[m, 1] = (v - np.floor(v)).astype(F)
            alb[m] = self.albedo(self.floor_tex, uv[m])
        mesh = obj >= 2
        for b in range(len(self.tris)):                                          # default: BVH::GetNormal / GetUV (bvh.cpp:290-305), BLASBVH's (blas_bvh.cpp:391-406)
            m = mesh & ((obj - 2 == b) if self.kind == 1 else True)
            if not m.any():
                continue
            tr = self.tris[b][tri[m]]
            w = ((F(1) - bu[m]).astype(F) - bv[m]).astype(F)                     # 1 - barycentric.x - barycentric.y
            Nn = (((w[:, None] * tr["normal0"]).astype(F) + (bu[m, None] * tr["normal1"]).astype(F)).astype(F) + (bv[m, None] * tr["normal2"]).astype(F)).astype(F)
            uv[m] = (((w[:, None] * tr["uv0"]).astype(F) + (bu[m, None] * tr["uv1"]).astype(F)).astype(F) + (bv[m, None] * tr["uv2"]).astype(F)).astype(F)
            if self.kind == 1:                                                   # TransformVector(N, T) = make_float3(float4(N, 0) * T): row sums left to right
                T = self.T[b]
                Nn = np.stack([((((T[r, 0] * Nn[:, 0]).astype(F) + (T[r, 1] * Nn[:, 1]).astype(F)).astype(F) + (T[r, 2] * Nn[:, 2]).astype(F)).astype(F)
                                + (T[r, 3] * F(0)).astype(F)).astype(F) for r in range(3)], 1)
                mi = np.full(int(m.sum()), self.obj_mat[b], np.int64)            # materials[bvh->matIdx]
            else:
                mi = np.asarray(self.obj_mat, np.int64)[tr["objIdx"] - 2]        # materials[models[acc.triangles[triIdx].objIdx - 2]->matIdx]
            N[m] = normalize(Nn)
            mat[m] = 2 + mi
            a = np.ones((len(mi), 3), F)
            for k in np.unique(mi):
                sel = mi == k
                a[sel] = self.albedo(self.mat_tex[k], uv[m][sel])
            alb[m] = a
        flip = dot(N, D) > 0                                                     # if (dot(hitInfo.normal, ray.D) > 0) hitInfo.normal = -hitInfo.normal
        N[flip] = -N[flip]
        out["I"], out["material"], out["N"], out["u"], out["albedo"], out["v"] = I, mat, N, uv[:, 0], alb, uv[:, 1]
        return (out, flip) if with_flip else out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the Whitted renderer's Trace for scenes whose materials are all diffuse (oracle/crt_oracle.cpp:1465-1526), assembled from the queries
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def shadow_rays(info, light_pos):
    """DirectIllumination's shadow ray per record (crt_oracle.cpp:1467-1472): returns (origin, L, t = dist - 2 eps, dist, dot(N, L))"""
    I, N = info["I"], info["N"]
    with np.errstate(all="ignore"):
        L = (light_pos[None, :] - I).astype(F)
        dist = np.sqrt(dot(L, L)).astype(F)
        L = (L * (F(1) / dist).astype(F)[:, None]).astype(F)
        ndotl = dot(N, L)
        org = (I + (L * EPS).astype(F)).astype(F)
        t = (dist - (F(2) * EPS).astype(F)).astype(F)
    return org, L, t, dist, ndotl


def whitted_diffuse(info, occluded, light_pos):
    """Trace of a primary ray (depth 0, ray.inside false) in a scene whose materials are all diffuse, from its hit-info record and the occlusion of its shadow ray:
    sky for a miss, (24, 24, 22) for the light, else out = 0 + diffuseness * brdf * (irr + ambient) with diffuseness = 1 - (0 + 0); medium = 1."""
    n = len(info)
    _, L, _, dist, ndotl = shadow_rays(info, light_pos)
    alb, N = info["albedo"], info["N"]
    with np.errstate(all="ignore"):
        att = (F(1) / (dist * dist).astype(F)).astype(F)
        inr = (f32([24, 24, 22])[None, :] * att[:, None]).astype(F)
        irr = (inr * dot(N, L)[:, None]).astype(F)
    irr[(ndotl < EPS) | occluded] = 0
    diffuseness = F(1) - (F(0) + F(0))
    brdf = (alb * INVPI).astype(F)
    lit = (F(0) + ((diffuseness * brdf).astype(F) * (irr + f32([0.3, 0.3, 0.3])[None, :]).astype(F)).astype(F)).astype(F)
    out = (f32([1, 1, 1])[None, :] * lit).astype(F)                              # return medium * out
    mat = info["material"]
    out[mat == 0] = f32([24, 24, 22])
    out[mat == MATERIAL_MISS] = alb[mat == MATERIAL_MISS]
    acc = np.zeros((n, 4), F)
    acc[:, :3] = out
    return acc
