// render_views.h — crt_render_views: the frames of MANY cameras in one launch.  render_seq_kernel (seq_sample.h) with "frame" generalised to the VIEW-FRAME
// j = view * frames + frame of a job of K * frames of them: one wavefront per (owned tile, window of 64 consecutive j), lane = j in the window.  A one-frame render
// runs its 3 600 serial RNG streams as one-lane wavefronts; here the other 63 lanes hold the same tile's stream for other cameras (frames == 1: 64 cameras per
// wavefront) or other frames (frames >= 64: one camera per wavefront).  A lane's stream is the reference's: it starts at stream_seed(tx, ty, W, sppFirst, frame, passes),
// walks the tile's 256 x passes items with primary_target / sample_step / sample_unwind (sample_body.h, seq_sample.h: the one definition, over the same worlds as
// render_seq_kernel) and reads its camera — crt_set_camera's twelve floats — from cams[view].  The samples go to a slab of the sample form (sample_body.h) whose
// "frame" axis is j - jFirst; views_accumulate_kernel folds them per view.
//
//   render_views_kernel<World>   instantiated beside the worlds: render_seq.hip (BvhWorld, KdWorld, GridWorld, TlasAltWorld), render_prim.hip (PrimWorld)
//   views_accumulate_kernel      render_seq.hip
//
// A job is cut into launches by whole windows (abi.cpp crt_render_views_device): a launch covers the view-frames [jFirst, jFirst + nj), jFirst a multiple of 64.
//
// Numerics: seq_sample.h's (-ffp-contract=off, IEEE + - * / sqrt).  No MFMA.
#pragma once
#include "launch.h"
#include "seq_sample.h"

namespace crt {

// the screen pixel of an accumulator value at `scale` (renderer.cpp:119,127; RGBF32_to_RGB8's scalar branch, template/precomp.h:336-340): the expression
// resolve_kernel and commit_frame_kernel (kernels.hip) evaluate
__device__ __forceinline__ uint32_t rgb8_pixel(float ax, float ay, float az, float scale)
{
    const float px = ax * scale, py = ay * scale, pz = az * scale;
    const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, px)), g = (uint32_t)(255.0f * min_std(1.0f, py)), bb = (uint32_t)(255.0f * min_std(1.0f, pz));
    return (r << 16) + (g << 8) + bb;
}

// entry = tile rank * windows + window, windows = ceil(nj / 64).  The camera is read again for every pixel (twelve loads, L1 / L2 hits, next to a whole path):
// held in registers across the pixel loop it is twelve VGPRs per lane the traversal then spills for.
template <class World>
__global__ __launch_bounds__(256, 4) void render_views_kernel(const Scene sc, const World world, const float* __restrict__ cams, char* __restrict__ slab,
                                                             Counters* __restrict__ counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                             uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, uint32_t nEntries)
{
    extern __shared__ uint32_t ldsAll[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t entry = blockIdx.x * kSeqWaves + wave;
    if (entry >= nEntries) return;
    const uint32_t windows = (nj + 63u) / 64u;
    const uint32_t tl = entry / windows, win = entry % windows;
    if (tl >= tileCount) return;
    const uint32_t jl = win * 64u + lane;                                         // view-frame of the launch
    if (jl >= nj) return;
    const uint32_t j = jFirst + jl, view = j / frames, frame = j - view * frames;
    slab += slab_block_position(win, tileCount, tl, 64u * passes);                // this tile's block of this window's region of the sample slab
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    // this lane's LDS columns: the traversal stack, then the throughput factors
    const uint32_t stackWords = world.stack_words(sc);
    uint32_t* stk = ldsAll + wave * (stackWords + 15u) * 64u + lane;
    float* fst = reinterpret_cast<float*>(stk + stackWords * 64u);

    uint32_t nRays = 0, nPrimary = 0, nMesh = 0, steps = 0;
    const uint32_t items = 256u * passes;                                         // (pixel, pass) pairs in stream order
    uint32_t seed = stream_seed(tx, ty, (uint32_t)sc.W, sppFirst, frame, passes); // renderer.cpp:120
    const float* __restrict__ cam = cams + (size_t)view * 12u;                    // camPos, topLeft, topRight, bottomLeft
    const kernarg_f inv = scene_floats(offsetof(Scene, invW));
    const float invW = inv[0], invH = inv[1];

    for (uint32_t item = 0; item < items; item++) {
        // ---------------- ProcessTile + Camera::GetPrimaryRay (renderer.cpp:125-126, camera.h:23-30) ----------------
        const uint32_t pix = (passes == 1u) ? item : item / passes;
        const f3 camPos = mk3(cam[0], cam[1], cam[2]);
        const f3 TL = mk3(cam[3], cam[4], cam[5]), TR = mk3(cam[6], cam[7], cam[8]), BL = mk3(cam[9], cam[10], cam[11]);
        const f3 v = primary_target(camPos, TL, TR - TL, BL - TL, invW, invH, tx, ty, pix, seed);
        f3 O = camPos, D = v * rcp_exact(sqrt_exact(dot3(v, v)));                 // normalize()
        bool inside = false; int depth = 0;
        nPrimary++;
        f3 L = mk3(0, 0, 0);
        while (!sample_step<World, false>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {}
        sample_unwind(fst, depth, L);                                             // unwind the recursion, store the sample
        uint32_t pass = 0;
        if (passes != 1u) pass = item - pix * passes;
        store_sample(slab, slab_sample_offset(lane, pix, 64u * passes, passes, pass), L);
    }
    atomicAdd(&counters->v[0], (unsigned long long)nRays);
    atomicAdd(&counters->v[1], (unsigned long long)nPrimary);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

// what a launch over every (owned tile, window of the view-frames [jFirst, jFirst + nj)) needs; the callers check their own limits first
template <class World>
hipError_t launch_render_views(const Scene* sc, const World& world, const float* cams, void* slab, Counters* counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount,
                               uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream)
{
    const uint32_t ldsBytes = seq_lds_bytes(world.stack_words(*sc));
    const unsigned long long entries = (unsigned long long)tileCount * ((nj + 63u) / 64u);
    if (ldsBytes > 64u * 1024u || entries > 0x7fffffffull || frames == 0) return hipErrorInvalidValue;
    if (entries == 0) return hipSuccess;
    hipLaunchKernelGGL((render_views_kernel<World>), dim3((uint32_t)((entries + kSeqWaves - 1u) / kSeqWaves)), dim3(64u * kSeqWaves), ldsBytes, stream, *sc, world, cams, (char*)slab,
                       counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, (uint32_t)entries);
    return hipGetLastError();
}

} // namespace crt
