// render_seq.hip — the FileScene / TLASFileScene worlds of render_seq_kernel (seq_sample.h), the sequential per-lane Sample loop:
//   BvhWorld<KIND>   FindNearest through the BVH / TLAS (file_scene.cpp:170-175 / tlas_file_scene.cpp:201-206) in the reference's order (dev_common.h find_nearest_seq):
//                    the latency mode's cost probe
//   KdWorld          FindNearest through FileScene's KD-tree (kd_intersect) — the accelerator the reference's shipped FileScene traces through (file_scene.h:10-12)
//   GridWorld        ... through its uniform grid (grid_intersect)
//   TlasKdWorld      TLASFileScene::FindNearest built with TLAS_USE_KDTree (TLASKDTree over BLASKDTree: tlas_alt_intersect<1>)
//   TlasGridWorld    ... with TLAS_USE_Grid (TLASGrid over BLASGrid: tlas_alt_intersect<2>)
// The issue-bound renders of these scenes are render_pool_kernel / render_tiles_kernel; this form exists for the probe and for parity with the alternative
// accelerators (crt_set_render_accel).
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).  No MFMA: pointer chasing + slab / Möller–Trumbore tests.
#include "alt_common.h"
#include "seq_sample.h"

namespace crt {

// the hit's surface in a triangle scene: the floor plane or a mesh triangle (KIND 1: the normal goes through the instance's T)
template <int KIND>
struct FileSurface {
    static constexpr bool kMeshHits = true;
    __device__ __forceinline__ f3 miss(const Scene& sc, f3 D) const { return sky_color(sc, D); }        // GetSkyColor, file_scene.cpp:142-154
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D) const
    {
        const char* __restrict__ geom = sc.geom;
        Surf s; f3 N; float tu = 0, tv = 0; uint32_t tOff; int tW, tH;
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
            const rec4* mp = reinterpret_cast<const rec4*>(sc.mats + (int)asu(s3.w));
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
        return s;
    }
};

template <int KIND>
struct BvhWorld : FileSurface<KIND> {
    __device__ __host__ uint32_t stack_words(const Scene& sc) const { return sc.stackDepth; }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
        int traversed = 0, tested = 0;
        find_nearest_seq(sc, O, D, rD, h, stk, cn, traversed, tested);
        return cn.interior + cn.tri + cn.tlas;
    }
};

// FileScene::FindNearest through an alternative accelerator: light quad, floor plane, then the structure
struct KdWorld : FileSurface<0> {
    AltAccelDev acc;
    __device__ __host__ uint32_t stack_words(const Scene&) const { return acc.kdStack * 2u; }          // (far child, plane distance) per entry
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        int traversed = 0, tested = 0;
        hit_light_floor(sc, O, D, h);
        kd_intersect(acc, O, D, rD, h, stk, traversed, tested);
        return 0u;
    }
};
struct GridWorld : FileSurface<0> {
    AltAccelDev acc;
    __device__ __host__ uint32_t stack_words(const Scene&) const { return 0u; }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t*) const
    {
        int traversed = 0, tested = 0;
        hit_light_floor(sc, O, D, h);
        grid_intersect(acc, O, D, rD, h, traversed, tested);
        return 0u;
    }
};

// TLASFileScene::FindNearest (tlas_file_scene.cpp:201-206) built with TLAS_USE_KDTree / TLAS_USE_Grid: light quad, floor plane, then TLASKDTree / TLASGrid over
// the BLAS set of crt_upload_blas_accel; shading is the BVH variant's (GetHitInfo, :236-253: triangle records carry the global shade index)
template <int ACCEL>
struct TlasAltWorld : FileSurface<1> {
    TlasAltDev tl;
    __device__ __host__ uint32_t stack_words(const Scene& sc) const { return tlas_alt_stack_words(sc, tl); }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        int traversed = 0, tested = 0;
        hit_light_floor(sc, O, D, h);
        tlas_alt_intersect<ACCEL>(sc, tl, O, D, rD, h, stk, traversed, tested);
        return 0u;
    }
};
using TlasKdWorld = TlasAltWorld<1>;
using TlasGridWorld = TlasAltWorld<2>;

} // namespace crt

// the latency mode's cost probe: kProbeWaves wavefronts per owned tile, 64 paths each, step counts summed into tileCost[tile]
extern "C" uint32_t crt_probe_paths() { return 64u * crt::kProbeWaves; }
extern "C" hipError_t crt_launch_probe(const crt::Scene* sc, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t* tileCost, hipStream_t stream)
{
    if (tileCount == 0 || !tileCost || tileCount > 0x10000u) return hipSuccess;
    const uint32_t nProbe = tileCount * crt::kProbeWaves;
    dim3 grid((nProbe + crt::kSeqWaves - 1u) / crt::kSeqWaves), block(64u * crt::kSeqWaves);
    const uint32_t ldsBytes = crt::seq_lds_bytes(sc->stackDepth);
    if (hipMemsetAsync(tileCost, 0, (size_t)tileCount * 4, stream) != hipSuccess) return hipGetLastError();
    if (sc->kind == 0) hipLaunchKernelGGL((crt::render_seq_kernel<crt::BvhWorld<0>, true>), grid, block, ldsBytes, stream, *sc, crt::BvhWorld<0>{}, (float4*)nullptr, (crt::Counters*)nullptr, tileFirst, tileStride, tileCount, tilesX, 1u, 64u, 1u, nProbe, tileCost);
    else hipLaunchKernelGGL((crt::render_seq_kernel<crt::BvhWorld<1>, true>), grid, block, ldsBytes, stream, *sc, crt::BvhWorld<1>{}, (float4*)nullptr, (crt::Counters*)nullptr, tileFirst, tileStride, tileCount, tilesX, 1u, 64u, 1u, nProbe, tileCost);
    return hipGetLastError();
}

// Renderer::Sample through the KD-tree (accel 1) or uniform grid (accel 2) — FileScene's (acc), or a two-level scene's BLAS set (tl): one wavefront per (owned tile,
// 64-frame window) of the launch, lane = frame
extern "C" hipError_t crt_launch_render_alt(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, void* slab, crt::Counters* counters, uint32_t tileFirst,
                                            uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, hipStream_t stream)
{
    if (tileCount == 0 || frames == 0) return hipSuccess;
    if (accel != 1 && accel != 2) return hipErrorInvalidValue;
    const uint32_t windows = (frames + 63u) / 64u;
    if ((unsigned long long)tileCount * windows > 0x7fffffffull || tileCount > 0x10000u || windows > 64u) return hipErrorInvalidValue;
    if (sc->kind != 0) {
        if (crt::seq_lds_bytes(crt::tlas_alt_stack_words(*sc, *tl)) > 64u * 1024u) return hipErrorInvalidValue;
        if (accel == 1) return crt::launch_render_seq(sc, crt::TlasKdWorld{{}, *tl}, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, stream);
        return crt::launch_render_seq(sc, crt::TlasGridWorld{{}, *tl}, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, stream);
    }
    if (accel == 1) {
        const crt::KdWorld kd{{}, *acc};
        if (crt::seq_lds_bytes(kd.stack_words(*sc)) > 64u * 1024u) return hipErrorInvalidValue;
        return crt::launch_render_seq(sc, kd, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, stream);
    }
    return crt::launch_render_seq(sc, crt::GridWorld{{}, *acc}, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, stream);
}
