// seq_sample.h — render_seq_kernel: Renderer::ProcessTile + Sample ("3. PathTracer/renderer.cpp":117-131, Sample :50-100) as a plain per-lane path loop — the
// SEQUENTIAL form: one wavefront per (tile, 64-frame window), lane = frame, no phases, no queues.  It serves everything that is not issue-bound:
//   * the latency mode's cost probe (PROBE: render_seq.hip, abi.cpp probe_tile_costs);
//   * Sample through FileScene's KD-tree / uniform grid (crt_set_render_accel; render_seq.hip);
//   * Sample over the PrimitiveScene (render_prim.hip).
// The per-path part (sample_step: one FindNearest + the Sample branch + the factor store; sample_unwind: the return path) is also what sample_query_kernel
// (sample_query.h: Sample for a caller's rays and seeds) runs.  The branch itself — medium, the rnd draw, mirror / dielectric / diffuse, the throughput factor, the
// primary ray, the return path — is sample_body.h's: the functions render_pool_kernel and render_tiles_kernel shade with, not a copy.
// What differs between them is the "world" the loop runs in, a small policy class:
//   uint32_t trace(sc, O, D, rD, h, stk)   scene.FindNearest into `h`; returns the traversal steps the probe counts (interior + triangle + TLAS steps; 0 where never probed)
//   Surf surface(sc, h, I, D)              normal (already facing the ray), albedo, reflectivity, refractivity and absorption at the hit
//   f3 miss(sc, D)                         scene.GetSkyColor
//   kMeshHits                              hits of objects >= 2 are counted into Counters::v[7]
//   stack_words(sc)                        dwords per lane of the LDS traversal stack `stk` (column layout: entry i at stk[i * 64])
// Per stream everything is the reference's: the rnd draws in its order and every float expression as written there (-ffp-contract=off, dev_common.h), so the
// samples are bit-identical to render_pool_kernel's, render_tiles_kernel's and the CPU oracle's.
#pragma once
#include "sample_body.h"

namespace crt {

struct Surf { f3 N, c; float refl, refr; f3 absorb; };

constexpr uint32_t kSeqWaves = 4u;                         // wavefronts per workgroup, each an entry of its own
constexpr uint32_t kProbeWaves = 8u;                       // cost probe: wavefronts (of 64 one-path lanes) per tile

__device__ __host__ __forceinline__ uint32_t seq_lds_bytes(uint32_t stackWords) { return kSeqWaves * (stackWords + 15u) * 64u * 4u; }   // traversal stack + 15 throughput factors per lane

// One trip of Renderer::Sample's recursion (renderer.cpp:50-100) for the path this lane holds: scene.FindNearest for the ray (O, D), then the branch.  Returns true when
// the path has ended (L = the radiance of its last ray: sky, light, or black at the depth limit); otherwise the bounce's throughput factor is stored in this lane's
// factor column `fst` (slot `depth`), depth is advanced and (O, D, inside) is the next ray.  Shared by render_seq_kernel and sample_query_kernel (sample_query.h): the
// rnd draws in the reference's order and every float expression as written there.  `steps`: the cost probe's traversal + weighted shading steps (PROBE only).
template <class World, bool PROBE>
__device__ __forceinline__ bool sample_step(const Scene& sc, const World& world, uint32_t* stk, float* fst, f3& O, f3& D, bool& inside, int& depth, uint32_t& seed, f3& L,
                                            uint32_t& nRays, uint32_t& nMesh, uint32_t& steps)
{
    const f3 rD = rcp_exact3(D);
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    nRays++;
    const uint32_t traceSteps = world.trace(sc, O, D, rD, h, stk);
    if (PROBE) steps += traceSteps + 3u;                                          // a shading step weighs about three traversal steps
    if (World::kMeshHits && h.objIdx >= 2) nMesh++;
    // ---------------- Renderer::Sample (renderer.cpp:50-100) ----------------
    if (h.objIdx == -1) { L = world.miss(sc, D); return true; }
    if (depth >= sc.depthLimit) { L = mk3(0, 0, 0); return true; }
    if (h.objIdx == 0) { L = mk3(24, 24, 22); return true; }                       // the light
    const f3 I = O + h.t * D;
    const Surf s = world.surface(sc, h, I, D);
    const f3 N = s.N, c = s.c;
    const f3 medium = medium_of(inside, s.absorb, h.t);
    const Bounce b = draw_bounce(seed, D, N, inside, s.refl, s.refr);
    const f3 nv = b.branch == kDiffuse ? b.v * rcp_exact(sqrt_exact(dot3(b.v, b.v))) : b.v;   // normalize(R)
    const f3 factor = bounce_factor(b.branch, c, medium, nv, N);
    // the bounce's throughput factor (albedo*medium*... multiplies on return: depth <= 4 here)
    float* fd = fst + (uint32_t)(3 * depth) * 64u;
    fd[0] = factor.x; fd[64] = factor.y; fd[128] = factor.z;
    depth++;
    O = I + nv * CRT_EPS; D = nv; inside = b.newInside;
    return false;
}

// entry = tile rank * windows + window.  PROBE = true is the cost probe of the latency mode: kProbeWaves entries per tile, lane l of entry q traces ONE path through
// pixel (4 l + q) % 256 of the tile with a seed of its own (256 paths per tile per four entries), nothing is stored, and every wavefront adds the number of traversal /
// shading steps its 64 paths took to tileCost[tile] (zeroed by the host) — an estimate of what the tile's streams will cost (a stream = 256 such paths), available well
// under a millisecond after a camera or scene change instead of after a first full render.
template <class World, bool PROBE>
__global__ __launch_bounds__(256, 4) void render_seq_kernel(const Scene sc, const World world, char* __restrict__ slab, Counters* __restrict__ counters,
                                                           uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                           uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t nEntries, uint32_t* __restrict__ tileCost)
{
    extern __shared__ uint32_t ldsAll[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t entry = blockIdx.x * kSeqWaves + wave;
    if (entry >= nEntries) return;
    const uint32_t windows = (frames + 63u) / 64u;
    const uint32_t tl = PROBE ? entry / kProbeWaves : entry / windows, win = PROBE ? 0u : entry % windows;
    if (tl >= tileCount) return;
    sppFirst += win * 64u * passes;
    frames = (frames - win * 64u < 64u) ? frames - win * 64u : 64u;               // frames of THIS window (the last one may be partial)
    if (lane >= frames) return;
    if (!PROBE) slab += slab_block_position(win, tileCount, tl, 64u * passes);     // this tile's block of this window's region of the sample slab
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    // this lane's LDS columns: the traversal stack, then the throughput factors
    const uint32_t stackWords = world.stack_words(sc);
    uint32_t* stk = ldsAll + wave * (stackWords + 15u) * 64u + lane;
    float* fst = reinterpret_cast<float*>(stk + stackWords * 64u);

    uint32_t nRays = 0, nPrimary = 0, nMesh = 0;
    const uint32_t items = PROBE ? 1u : 256u * passes;                            // (pixel, pass) pairs in stream order
    uint32_t seed = init_seed(tx + ty * (uint32_t)sc.W + (sppFirst + lane * passes) * 1799u);   // renderer.cpp:120
    if (PROBE) seed = init_seed(0x9e3779b9u ^ ((tile * kProbeWaves + entry % kProbeWaves) * 64u + lane));
    uint32_t steps = 0;                                                           // probe: traversal + weighted shading steps of this lane's path

    const kernarg_f cam = scene_floats(offsetof(Scene, camPos));                  // camPos, topLeft, topRight, bottomLeft, invW, invH
    const f3 camPos = mk3(cam[0], cam[1], cam[2]);
    const f3 TL = mk3(cam[3], cam[4], cam[5]), TR = mk3(cam[6], cam[7], cam[8]), BL = mk3(cam[9], cam[10], cam[11]);
    const float invW = cam[12], invH = cam[13];

    for (uint32_t item = 0; item < items; item++) {
        // ---------------- ProcessTile + Camera::GetPrimaryRay (renderer.cpp:125-126, camera.h:23-30) ----------------
        const uint32_t pix = PROBE ? ((lane * 4u + entry % kProbeWaves) & 255u) : ((passes == 1u) ? item : item / passes);
        const f3 v = primary_target(camPos, TL, TR - TL, BL - TL, invW, invH, tx, ty, pix, seed);
        f3 O = camPos, D = v * rcp_exact(sqrt_exact(dot3(v, v)));                 // normalize()
        bool inside = false; int depth = 0;
        nPrimary++;
        f3 L = mk3(0, 0, 0);
        while (!sample_step<World, PROBE>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {}
        sample_unwind(fst, depth, L);                                             // unwind the recursion, store the sample
        if (!PROBE) {
            uint32_t pass = 0;
            if (passes != 1u) pass = item - pix * passes;
            store_sample(slab, slab_sample_offset(lane, pix, 64u * passes, passes, pass), L);   // (`slab`: the tile's block of the window)
        } else if (L.x != L.x) steps++;                                            // (keeps the probe's shading arithmetic alive)
    }
    if (PROBE) { const uint32_t sum = wave_sum(steps); if (lane == 0) atomicAdd(&tileCost[tl], sum); return; }
    atomicAdd(&counters->v[0], (unsigned long long)nRays);
    atomicAdd(&counters->v[1], (unsigned long long)nPrimary);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

// what a launch over every (owned tile, 64-frame window) needs (render_seq.hip / render_prim.hip: the callers check their own limits first)
template <class World>
hipError_t launch_render_seq(const Scene* sc, const World& world, void* slab, Counters* counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                             uint32_t sppFirst, uint32_t frames, uint32_t passes, hipStream_t stream)
{
    const uint32_t entries = tileCount * ((frames + 63u) / 64u);
    hipLaunchKernelGGL((render_seq_kernel<World, false>), dim3((entries + kSeqWaves - 1u) / kSeqWaves), dim3(64u * kSeqWaves), seq_lds_bytes(world.stack_words(*sc)), stream,
                       *sc, world, (char*)slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, entries, (uint32_t*)nullptr);
    return hipGetLastError();
}

} // namespace crt
