// render_shapes.hip — the two instantiations of render_shapes_kernel (render_shapes.h) and their launch: crt_render_views' launch over the shapes of a shape table
// (crt_render_shapes); render_shape_sets_kernel (render_shape_sets.h) and its launch, the same over a set's table (crt_render_shape_sets).  The per-view sums are
// crt_launch_views_accumulate's (render_seq.hip).
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).  No MFMA: pointer chasing + slab / Möller–Trumbore tests.
#include "launch.h"
#include "render_shape_sets.h"

// sc: the context's Scene with the JOB's stackDepth (a two-level scene: the tallest shape's TLAS).
extern "C" hipError_t crt_launch_render_shapes(const crt::Scene* sc, const crt::ShapeTableDev* t, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst,
                                               uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj,
                                               hipStream_t stream)
{
    const uint32_t ldsBytes = crt::seq_lds_bytes(sc->stackDepth);
    const unsigned long long entries = (unsigned long long)tileCount * ((nj + 63u) / 64u);
    if ((sc->kind != 0 && sc->kind != 1) || ldsBytes > 64u * 1024u || entries > 0x7fffffffull || frames == 0) return hipErrorInvalidValue;
    if (entries == 0) return hipSuccess;
    const dim3 grid((uint32_t)((entries + crt::kSeqWaves - 1u) / crt::kSeqWaves)), block(64u * crt::kSeqWaves);
    if (sc->kind == 0)
        hipLaunchKernelGGL(crt::render_shapes_kernel<0>, grid, block, ldsBytes, stream, *sc, *t, cams, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes,
                           jFirst, nj, (uint32_t)entries);
    else
        hipLaunchKernelGGL(crt::render_shapes_kernel<1>, grid, block, ldsBytes, stream, *sc, *t, cams, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes,
                           jFirst, nj, (uint32_t)entries);
    return hipGetLastError();
}

// sc: the context's two-level Scene with the JOB's stackDepth.
extern "C" hipError_t crt_launch_render_shape_sets(const crt::Scene* sc, const crt::ShapeSetTableDev* t, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst,
                                                   uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj,
                                                   hipStream_t stream)
{
    const uint32_t ldsBytes = crt::seq_lds_bytes(sc->stackDepth);
    const unsigned long long entries = (unsigned long long)tileCount * ((nj + 63u) / 64u);
    if (sc->kind != 1 || ldsBytes > 64u * 1024u || entries > 0x7fffffffull || frames == 0) return hipErrorInvalidValue;
    if (entries == 0) return hipSuccess;
    const dim3 grid((uint32_t)((entries + crt::kSeqWaves - 1u) / crt::kSeqWaves)), block(64u * crt::kSeqWaves);
    hipLaunchKernelGGL(crt::render_shape_sets_kernel, grid, block, ldsBytes, stream, *sc, *t, cams, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes,
                       jFirst, nj, (uint32_t)entries);
    return hipGetLastError();
}
