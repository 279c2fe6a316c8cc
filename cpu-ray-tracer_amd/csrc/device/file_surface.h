// file_surface.h — FileSurface<KIND>: GetHitInfo + Material::GetAlbedo of a triangle scene (file_scene.cpp:189-214, tlas_file_scene.cpp:220-260) for a hit on the floor
// plane or on a mesh triangle.  One definition for the sequential Sample loop's worlds (render_seq.hip) and for the hit-info query (shade_query.hip), so that what
// Sample shades with and what crt_get_hit_info reports cannot drift apart.  The normal, uv and material words are sample_body.h's floor_point / mesh_point / face_ray:
// the functions render_pool_kernel and render_tiles_kernel shade with, not a copy; this class only loads the records and fetches the albedo.
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
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D, SurfExtra* x = nullptr) const { return surface_of(sc, h, I, D, sc.geom, sc.instOff, x); }
    // ... with the Instance records (KIND 1: their T rows) at instGeom + instOff: the live scene's (above), or a job-local pose's image of them (render_poses.h)
    __device__ __forceinline__ Surf surface_of(const Scene& sc, const Hit& h, f3 I, f3 D, const char* instGeom, uint32_t instOff, SurfExtra* x = nullptr) const
    {
        const char* __restrict__ geom = sc.geom;
        SurfPoint p;
        if (h.objIdx == 1) p = floor_point(mk3(sc.floorN[0], sc.floorN[1], sc.floorN[2]), sc.floorInvto, sc.floorMat, I);
        else {
            const uint32_t so = sc.shadeOff + (uint32_t)h.triIdx * 64u;
            const rec4 s0 = ldg(geom, so), s1 = ldg(geom, so + 16u), s2 = ldg(geom, so + 32u), s3 = ldg(geom, so + 48u);
            p = mesh_point<KIND>(s0, s1, s2, s3, h.u, h.v, h.objIdx, instGeom, instOff, sc.mats);
        }
        Surf s; s.N = face_ray(p.N, D); s.refl = p.refl; s.refr = p.refr; s.absorb = p.absorb;
        s.c = mk3(1.0f, 1.0f, 1.0f);
        if (p.tW > 0) s.c = tex_sample(sc, p.tOff, p.tW, p.tH, p.tu, p.tv);   // Material::GetAlbedo
        if (x) { x->u = p.tu; x->v = p.tv; x->mat = p.mat; }
        return s;
    }
};

} // namespace crt
