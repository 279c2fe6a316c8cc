// render_looks.hip — crt_render_looks: render_looks_kernel (render_looks.h) for the two triangle scene kinds, and its launch.  The job's look table comes from
// look_build.hip; the per-view sums are crt_launch_views_accumulate's (render_seq.hip).
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).  No MFMA: pointer chasing + slab / Möller–Trumbore tests.
#include "launch.h"
#include "render_looks.h"

// the view-frames [jFirst, jFirst + nj) of a job over the looks of a look table; sc: the context's Scene (a look changes no tree, so its stack depth is the job's)
extern "C" hipError_t crt_launch_render_looks(const crt::Scene* sc, const crt::LookTableDev* lt, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst,
                                              uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj,
                                              hipStream_t stream)
{
    const uint32_t ldsBytes = crt::seq_lds_bytes(sc->stackDepth);
    const unsigned long long entries = (unsigned long long)tileCount * ((nj + 63u) / 64u);
    if ((sc->kind != 0 && sc->kind != 1) || ldsBytes > 64u * 1024u || entries > 0x7fffffffull || frames == 0) return hipErrorInvalidValue;
    if (entries == 0) return hipSuccess;
    const dim3 grid((uint32_t)((entries + crt::kSeqWaves - 1u) / crt::kSeqWaves)), block(64u * crt::kSeqWaves);
    if (sc->kind == 0)
        hipLaunchKernelGGL(crt::render_looks_kernel<0>, grid, block, ldsBytes, stream, *sc, *lt, cams, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes,
                           jFirst, nj, (uint32_t)entries);
    else
        hipLaunchKernelGGL(crt::render_looks_kernel<1>, grid, block, ldsBytes, stream, *sc, *lt, cams, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes,
                           jFirst, nj, (uint32_t)entries);
    return hipGetLastError();
}
