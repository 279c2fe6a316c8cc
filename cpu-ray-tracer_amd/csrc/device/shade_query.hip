// shade_query.hip — the shading queries of the lower seam on record buffers (crt_abi.h "scene queries"): BaseScene::GetHitInfo + Material::GetAlbedo
// (hit_info_kernel) and BaseScene::GetSkyColor (sky_color_kernel).
//
// A gather, not a walk: one record per lane, 64-lane blocks in a grid-stride loop.  Per record 56 B in (crt_ray + crt_hit, 28-byte AoS records loaded as
// find_nearest_kernel loads crt_ray), up to 64 B ShadeTri + 32 B Material + 48 B of Instance::T + one texel, and 48 B out in three 16-byte stores.  No LDS, no
// atomics, no cursor: every record costs the same but for the four-way branch miss / light / floor / mesh, whose arms are short.
// The surface is FileSurface<KIND>::surface (file_surface.h) and the sky dev_common.h's sky_color — the functions Sample shades with, not a copy.
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).
#include "file_surface.h"
#include "launch.h"

namespace crt {

struct ShadeRayIn { float O[3]; float D[3]; int32_t inside; };                                  // crt_ray
struct ShadeHitIn { float t, u, v; int32_t objIdx, triIdx, traversed, tested; };                // crt_hit
constexpr int32_t kMaterialMiss = -1, kMaterialInvalid = -2;                                     // CRT_MATERIAL_MISS / CRT_MATERIAL_INVALID
constexpr uint32_t kShadeWavesPerCu = 32u;                                                       // no LDS and few registers: every wave slot of a CU

// out[3 i .. 3 i + 2] = crt_hit_info i: {I, material} {N, u} {albedo, v}.  objects / fileTris: hit_record_ok's bounds (fileTris: the FileScene's triangle count;
// a two-level scene's BLAS carries its own in Instance::triCount).  A record that fails the predicate reads nothing of the scene.
template <int KIND>
__global__ __launch_bounds__(64) void hit_info_kernel(const Scene sc, const ShadeRayIn* __restrict__ rays, const ShadeHitIn* __restrict__ hits, rec4* __restrict__ out,
                                                      uint32_t n, uint32_t objects, uint32_t fileTris)
{
    const char* __restrict__ g = sc.geom;
    const FileSurface<KIND> world{};
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
        const ShadeRayIn r = rays[i];
        const ShadeHitIn hr = hits[i];
        const f3 O = mk3(r.O[0], r.O[1], r.O[2]), D = mk3(r.D[0], r.D[1], r.D[2]);
        rec4 o0 = {0.0f, 0.0f, 0.0f, asf((uint32_t)kMaterialInvalid)}, o1 = {0.0f, 0.0f, 0.0f, 0.0f}, o2 = o1;
        rec4 ids = {0.0f, 0.0f, 0.0f, 0.0f};                              // KIND 1: the instance's {shadeBase, rootRef16, rootRef, objIdx}
        const bool ok = hit_record_ok(hr.objIdx, hr.triIdx, objects, [&](uint32_t k) -> uint32_t {
            if (KIND == 0) return fileTris;
            const uint32_t io = sc.instOff + k * 128u;
            ids = ldg(g, io + 48u);
            return asu(ldg(g, io + 112u).x);                              // Instance::triCount
        });
        if (ok) {
            if (hr.objIdx == -1) {                                        // what Trace / Sample return for a miss
                const f3 c = world.miss(sc, D);
                o0.w = asf((uint32_t)kMaterialMiss);
                o2.x = c.x; o2.y = c.y; o2.z = c.z;
            } else {
                const f3 I = O + hr.t * D;
                f3 N, c; SurfExtra x; x.u = 0; x.v = 0; x.mat = 0;
                if (hr.objIdx == 0) {                                     // the light quad: Quad::GetNormal, primitiveMaterials[0] (no texture)
                    N = mk3(sc.lightNrm[0], sc.lightNrm[1], sc.lightNrm[2]);
                    if (dot3(N, D) > 0) N = -N;
                    c = mk3(1.0f, 1.0f, 1.0f);
                } else {
                    Hit h; h.t = hr.t; h.u = hr.u; h.v = hr.v; h.objIdx = hr.objIdx;
                    h.triIdx = (KIND == 0) ? hr.triIdx : (int)(asu(ids.x) + (uint32_t)hr.triIdx);   // Instance::shadeBase + the BLAS-local index
                    const Surf s = world.surface(sc, h, I, D, &x);
                    N = s.N; c = s.c;
                }
                o0.x = I.x; o0.y = I.y; o0.z = I.z; o0.w = asf((uint32_t)x.mat);
                o1.x = N.x; o1.y = N.y; o1.z = N.z; o1.w = x.u;
                o2.x = c.x; o2.y = c.y; o2.z = c.z; o2.w = x.v;
            }
        }
        rec4* __restrict__ op = out + (size_t)i * 3u;
        op[0] = o0; op[1] = o1; op[2] = o2;
    }
}

// rgb[3 i .. 3 i + 2] = GetSkyColor(rays[i]): only D is read
__global__ __launch_bounds__(64) void sky_color_kernel(const Scene sc, const ShadeRayIn* __restrict__ rays, float* __restrict__ rgb, uint32_t n)
{
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
        const f3 c = sky_color(sc, mk3(rays[i].D[0], rays[i].D[1], rays[i].D[2]));
        float* __restrict__ op = rgb + (size_t)i * 3u;
        op[0] = c.x; op[1] = c.y; op[2] = c.z;
    }
}

static dim3 shade_grid(uint32_t n)
{
    const uint32_t need = (n + 63u) / 64u, fill = 256u * kShadeWavesPerCu;   // the device full once, never more blocks than the records need (as the other query launches)
    return dim3(need < fill ? need : fill);
}

} // namespace crt

extern "C" hipError_t crt_launch_hit_info(const crt::Scene* sc, const void* rays, const void* hits, void* out, uint32_t n, uint32_t objects, uint32_t fileTris, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (sc->kind == 0) hipLaunchKernelGGL(crt::hit_info_kernel<0>, crt::shade_grid(n), dim3(64), 0, stream, *sc, (const crt::ShadeRayIn*)rays, (const crt::ShadeHitIn*)hits, (crt::rec4*)out, n, objects, fileTris);
    else hipLaunchKernelGGL(crt::hit_info_kernel<1>, crt::shade_grid(n), dim3(64), 0, stream, *sc, (const crt::ShadeRayIn*)rays, (const crt::ShadeHitIn*)hits, (crt::rec4*)out, n, objects, fileTris);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_sky_color(const crt::Scene* sc, const void* rays, float* rgb, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(crt::sky_color_kernel, crt::shade_grid(n), dim3(64), 0, stream, *sc, (const crt::ShadeRayIn*)rays, rgb, n);
    return hipGetLastError();
}
