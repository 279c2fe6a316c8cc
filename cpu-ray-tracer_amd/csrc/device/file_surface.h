// file_surface.h — FileSurface<KIND>: GetHitInfo + Material::GetAlbedo of a triangle scene (file_scene.cpp:189-214, tlas_file_scene.cpp:220-260) for a hit on the floor
// plane or on a mesh triangle.  One definition for the sequential Sample loop's worlds (render_seq.hip) and for the hit-info query (shade_query.hip), so that what
// Sample shades with and what crt_get_hit_info reports cannot drift apart.
#pragma once
#include "seq_sample.h"

namespace crt {

struct SurfExtra { float u, v; int mat; };                 // HitInfo::uv; index into Scene::mats ([0] light, [1] floor, 2.. the scene's)

// the hit's surface in a triangle scene: the floor plane or a mesh triangle (KIND 1: the normal goes through the instance's T)
template <int KIND>
struct FileSurface {
    static constexpr bool kMeshHits = true;
    __device__ __forceinline__ f3 miss(const Scene& sc, f3 D) const { return sky_color(sc, D); }        // GetSkyColor, file_scene.cpp:142-154
    // h.triIdx is the GLOBAL shade index (what LeafTri::shadeIdx carries).  x: also HitInfo::uv and the material's index in Scene::mats, for the hit-info query
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D, SurfExtra* x = nullptr) const
    {
        const char* __restrict__ geom = sc.geom;
        Surf s; f3 N; float tu = 0, tv = 0; uint32_t tOff; int tW, tH;
        int mat = 1;
        if (h.objIdx == 1) {                                                   // floor: Plane::GetNormal / GetUV (primitives.h:112-133)
            N = mk3(sc.floorN[0], sc.floorN[1], sc.floorN[2]);
            if (N.y == 1) {
                float uu = I.x, vw = I.z;
                uu *= sc.floorInvto; vw *= sc.floorInvto;
                tu = uu - __builtin_floorf(uu); tv = vw - __builtin_floorf(vw);
            }
            s.refl = sc.floorMat.reflectivity; s.refr = sc.floorMat.refractivity;
            s.absorb = mk3(sc.floorMat.absorption[0], sc.floorMat.absorption[1], sc.floorMat.absorption[2]);
            tOff = sc.floorMat.texOffset; tW = sc.floorMat.texW; tH = sc.floorMat.texH;
        } else {                                                               // mesh: GetNormal / GetUV (bvh.cpp:290-305, blas_bvh.cpp:391-406)
            const uint32_t so = sc.shadeOff + (uint32_t)h.triIdx * 64u;
            const rec4 s0 = ldg(geom, so), s1 = ldg(geom, so + 16u), s2 = ldg(geom, so + 32u), s3 = ldg(geom, so + 48u);
            const f3 n0 = mk3(s0.x, s0.y, s0.z), n1 = mk3(s0.w, s1.x, s1.y), n2 = mk3(s1.z, s1.w, s2.x);
            const float w = 1 - h.u - h.v;
            const f3 Nn = w * n0 + h.u * n1 + h.v * n2;
            tu = w * s2.y + h.u * s2.w + h.v * s3.y;
            tv = w * s2.z + h.u * s3.x + h.v * s3.z;
            mat = (int)asu(s3.w);
            const rec4* mp = reinterpret_cast<const rec4*>(sc.mats + mat);
            const rec4 m0 = mp[0], m1 = mp[1];
            s.refl = m0.x; s.refr = m0.y; s.absorb = mk3(m0.z, m0.w, m1.x);
            tOff = asu(m1.y); tW = (int)asu(m1.z); tH = (int)asu(m1.w);
            if (KIND == 0) N = normalize3(Nn);
            else {
                const uint32_t io = sc.instOff + (uint32_t)(h.objIdx - 2) * 128u + 64u;   // Instance::T rows
                const rec4 r0 = ldg(geom, io), r1 = ldg(geom, io + 16), r2 = ldg(geom, io + 32);
                N = normalize3(mk3(r0.x * Nn.x + r0.y * Nn.y + r0.z * Nn.z + r0.w * 0.0f,
                                   r1.x * Nn.x + r1.y * Nn.y + r1.z * Nn.z + r1.w * 0.0f,
                                   r2.x * Nn.x + r2.y * Nn.y + r2.z * Nn.z + r2.w * 0.0f));
            }
        }
        if (dot3(N, D) > 0) N = -N;
        s.N = N;
        s.c = mk3(1.0f, 1.0f, 1.0f);
        if (tW > 0) s.c = tex_sample(sc, tOff, tW, tH, tu, tv);              // Material::GetAlbedo
        if (x) { x->u = tu; x->v = tv; x->mat = mat; }
        return s;
    }
};

} // namespace crt
