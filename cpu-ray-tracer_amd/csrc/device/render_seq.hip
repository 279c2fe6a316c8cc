// render_seq.hip — the FileScene / TLASFileScene worlds of render_seq_kernel (seq_sample.h), the sequential per-lane Sample loop:
//   BvhWorld<KIND>   FindNearest through the BVH / TLAS (file_scene.cpp:170-175 / tlas_file_scene.cpp:201-206) in the reference's order (dev_common.h find_nearest_seq):
//                    the latency mode's cost probe
//   KdWorld          FindNearest through FileScene's KD-tree (kd_intersect) — the accelerator the reference's shipped FileScene traces through (file_scene.h:10-12)
//   GridWorld        ... through its uniform grid (grid_intersect)
//   TlasKdWorld      TLASFileScene::FindNearest built with TLAS_USE_KDTree (TLASKDTree over BLASKDTree: tlas_alt_intersect<1>)
//   TlasGridWorld    ... with TLAS_USE_Grid (TLASGrid over BLASGrid: tlas_alt_intersect<2>)
// The issue-bound renders of these scenes are render_pool_kernel / render_tiles_kernel; this form exists for the probe and for parity with the alternative
// accelerators (crt_set_render_accel).  The same worlds serve sample_query_kernel (sample_query.h): Renderer::Sample for a caller's rays and seeds, and
// render_views_kernel (render_views.h): the frames of many cameras in one launch (crt_render_views), whose per-view sums views_accumulate_kernel below forms.
// render_poses_kernel (render_poses.h) is that kernel over job-local poses of a two-level scene's instances (crt_render_poses); it is launched from here too.
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).  No MFMA: pointer chasing + slab / Möller–Trumbore tests.
#include "alt_common.h"
#include "file_surface.h"
#include "launch.h"
#include "sample_query.h"
#include "render_views.h"
#include "render_poses.h"

namespace crt {

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

// views_accumulate_kernel: for every view with view-frames in [jFirst, jFirst + nj), owned tile and pixel, the view's samples of this launch added channel by channel in
// frame order, then pass order — accumulate_kernel's chain after crt_clear.  Block = (owned tile, view of the launch), views of a tile side by side (they share the slab's lines), thread = pixel (v * 16 + u, the slab's order).  A
// view whose first frame lies in this launch starts from +0; one that began in an earlier launch continues from what that launch left in out_rgba.  The sum follows the
// view across the tile blocks of the windows it straddles (slab_position with the launch's view-frame as the frame).  w: +0 plus 0.0f per launch, so +0.  The screen
// pixel (rgb8_pixel) is written with the view's last frame.  Every addition of a channel happens in one thread, in order; no atomics.
__global__ __launch_bounds__(256) void views_accumulate_kernel(const char* __restrict__ slab, float4* __restrict__ outRgba, uint32_t* __restrict__ outPixels, uint32_t tileFirst,
                                                                uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t W, uint32_t H, uint32_t frames, uint32_t passes,
                                                                uint32_t jFirst, uint32_t nj, uint32_t nViews, float scale)
{
    const uint32_t viewFirst = jFirst / frames, view = viewFirst + blockIdx.x % nViews, tl = blockIdx.x / nViews, pix = threadIdx.x;
    if (tl >= tileCount) return;
    const unsigned long long vBegin = (unsigned long long)view * frames, vEnd = vBegin + frames, jEnd = (unsigned long long)jFirst + nj;
    const uint32_t ja = (uint32_t)(vBegin > jFirst ? vBegin : jFirst), jb = (uint32_t)(vEnd < jEnd ? vEnd : jEnd);     // this view's view-frames of the launch
    if (ja >= jb) return;
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t x0 = (tile % tilesX) * 16u, y0 = (tile / tilesX) * 16u;
    const size_t i = (size_t)view * W * H + (x0 + (pix & 15u)) + (size_t)(y0 + (pix >> 4)) * W;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ja != vBegin) a = outRgba[i];
    const uint32_t rowLen = 64u * passes;
    for (uint32_t j = ja; j < jb; j++) {
        const size_t at = slab_position(j - jFirst, tileCount, tl, pix, rowLen, passes, 0u);
        for (uint32_t p = 0; p < passes; p++) { const Sample3 t = load_sample(slab, at + p * kSampleBytes); a.x += t.x; a.y += t.y; a.z += t.z; }
    }
    a.w += 0.0f;
    outRgba[i] = a;
    if (outPixels && jb == vEnd) outPixels[i] = rgb8_pixel(a.x, a.y, a.z, scale);
}

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
    if (sc->kind == 0) hipLaunchKernelGGL((crt::render_seq_kernel<crt::BvhWorld<0>, true>), grid, block, ldsBytes, stream, *sc, crt::BvhWorld<0>{}, (char*)nullptr, (crt::Counters*)nullptr, tileFirst, tileStride, tileCount, tilesX, 1u, 64u, 1u, nProbe, tileCost);
    else hipLaunchKernelGGL((crt::render_seq_kernel<crt::BvhWorld<1>, true>), grid, block, ldsBytes, stream, *sc, crt::BvhWorld<1>{}, (char*)nullptr, (crt::Counters*)nullptr, tileFirst, tileStride, tileCount, tilesX, 1u, 64u, 1u, nProbe, tileCost);
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

// Renderer::Sample for a buffer of rays with a seed each (crt_sample / crt_sample_device): accel 0 = the scene's BVH / TLAS, 1 / 2 = the KD-tree / grid (FileScene's
// `acc`, or a two-level scene's BLAS set `tl`).  A world whose LDS columns exceed 64 KB per workgroup is refused (hipErrorInvalidValue), as crt_launch_render_alt does.
// residentLanes != null: only report the lanes a full launch holds.
extern "C" hipError_t crt_launch_sample_query(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, const void* rays, uint32_t* seeds, float* rgb,
                                              uint32_t n, crt::Counters* counters, uint32_t* cursor, uint32_t* residentLanes, hipStream_t stream)
{
    if (accel < 0 || accel > 2) return hipErrorInvalidValue;
    if (accel == 0) {
        if (sc->kind == 0) return crt::launch_sample_query(sc, crt::BvhWorld<0>{}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
        return crt::launch_sample_query(sc, crt::BvhWorld<1>{}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
    }
    if (sc->kind != 0) {
        if (accel == 1) return crt::launch_sample_query(sc, crt::TlasKdWorld{{}, *tl}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
        return crt::launch_sample_query(sc, crt::TlasGridWorld{{}, *tl}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
    }
    if (accel == 1) return crt::launch_sample_query(sc, crt::KdWorld{{}, *acc}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
    return crt::launch_sample_query(sc, crt::GridWorld{{}, *acc}, rays, seeds, rgb, n, counters, cursor, residentLanes, stream);
}

// crt_render_views: the view-frames [jFirst, jFirst + nj) of a job (render_views.h) through accel 0 = the scene's BVH / TLAS, 1 / 2 = the KD-tree / grid (FileScene's
// `acc`, or a two-level scene's BLAS set `tl`).  A world whose LDS columns exceed 64 KB per workgroup is refused (hipErrorInvalidValue), as crt_launch_render_alt does.
extern "C" hipError_t crt_launch_render_views(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, const float* cams, void* slab, crt::Counters* counters,
                                              uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst,
                                              uint32_t nj, hipStream_t stream)
{
    if (accel < 0 || accel > 2) return hipErrorInvalidValue;
    if (accel == 0) {
        if (sc->kind == 0) return crt::launch_render_views(sc, crt::BvhWorld<0>{}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
        return crt::launch_render_views(sc, crt::BvhWorld<1>{}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
    }
    if (sc->kind != 0) {
        if (accel == 1) return crt::launch_render_views(sc, crt::TlasKdWorld{{}, *tl}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
        return crt::launch_render_views(sc, crt::TlasGridWorld{{}, *tl}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
    }
    if (accel == 1) return crt::launch_render_views(sc, crt::KdWorld{{}, *acc}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
    return crt::launch_render_views(sc, crt::GridWorld{{}, *acc}, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, stream);
}

// crt_render_poses: the same launch over the poses of a pose table (render_poses.h).  sc: the context's Scene with the JOB's stackDepth (the tallest pose's).
extern "C" hipError_t crt_launch_render_poses(const crt::Scene* sc, const crt::PoseTableDev* pt, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst,
                                              uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj,
                                              hipStream_t stream)
{
    const uint32_t ldsBytes = crt::seq_lds_bytes(sc->stackDepth);
    const unsigned long long entries = (unsigned long long)tileCount * ((nj + 63u) / 64u);
    if (sc->kind != 1 || ldsBytes > 64u * 1024u || entries > 0x7fffffffull || frames == 0) return hipErrorInvalidValue;
    if (entries == 0) return hipSuccess;
    hipLaunchKernelGGL(crt::render_poses_kernel, dim3((uint32_t)((entries + crt::kSeqWaves - 1u) / crt::kSeqWaves)), dim3(64u * crt::kSeqWaves), ldsBytes, stream, *sc, *pt, cams, (char*)slab,
                       counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, (uint32_t)entries);
    return hipGetLastError();
}

// ... and the per-view sums of that launch's slab into the caller's images (views_accumulate_kernel)
extern "C" hipError_t crt_launch_views_accumulate(const void* slab, float* outRgba, uint32_t* outPixels, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t W,
                                                  uint32_t H, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, float scale, hipStream_t stream)
{
    if (tileCount == 0 || nj == 0) return hipSuccess;
    if (frames == 0) return hipErrorInvalidValue;
    const uint32_t nViews = (uint32_t)(((unsigned long long)jFirst + nj - 1u) / frames) - jFirst / frames + 1u;
    if ((unsigned long long)nViews * tileCount > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::views_accumulate_kernel, dim3(nViews * tileCount), dim3(256), 0, stream, (const char*)slab, (float4*)outRgba, outPixels, tileFirst, tileStride, tileCount, tilesX, W, H,
                       frames, passes, jFirst, nj, nViews, scale);
    return hipGetLastError();
}
