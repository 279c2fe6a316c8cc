// sample_query.h — sample_query_kernel: Renderer::Sample(ray, seed, 0) ("3. PathTracer/renderer.cpp":50-100) for an ARRAY of rays, each with a seed of its own
// (crt_sample / crt_sample_device).  The path itself is seq_sample.h's sample_step / sample_unwind, the one sequential Sample body, over the same worlds as
// render_seq_kernel; what differs is where a lane's work comes from.  A tile's stream is a chain (pixel k + 1 starts from the seed pixel k left), a query's rays are
// independent and 1 to depthLimit + 1 rays long, so the launch is PERSISTENT like the find-nearest query kernels: the grid is what the device holds at once, and a
// lane whose path has ended takes the next ray index from the launch-wide cursor — one atomicAdd per wavefront and trip, shared out by ballot + mbcnt ranks.  A trip
// of the wave's loop is one sample_step (one FindNearest + its shading) for every lane that holds a path; the wavefront ends when the cursor is exhausted and no lane
// holds one.  Per lane: the traversal stack column and the 15 throughput factors in LDS (seq_lds_bytes), as in render_seq_kernel.
//
// A ray is NOT traced — three quiet NaNs, its seed left alone — when its seed is 0 (xorshift32 maps 0 to 0: every draw would be 0 and diffusereflection's rejection loop
// would never end), when a component of O or D is not finite, or when D is (0, 0, 0).  The test sits in the refill, the only way a lane comes to hold a path, ahead of
// the lane's first draw; a non-zero xorshift32 state never becomes 0.
//
// Numerics: seq_sample.h's (-ffp-contract=off, IEEE + - * / sqrt, crt_expf / crt_atan2f / crt_acosf).  No MFMA.
#pragma once
#include "launch.h"
#include "seq_sample.h"

namespace crt {

struct SampleRay { float O[3]; float D[3]; int32_t inside; };           // = crt_ray, 28 bytes

template <class World>
__global__ __launch_bounds__(256, 4) void sample_query_kernel(const Scene sc, const World world, const SampleRay* __restrict__ rays, uint32_t* __restrict__ seeds,
                                                             float* __restrict__ rgb, uint32_t n, Counters* __restrict__ counters, uint32_t* __restrict__ cursor)
{
    extern __shared__ uint32_t ldsAll[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // this lane's LDS columns: the traversal stack, then the throughput factors
    const uint32_t stackWords = world.stack_words(sc);
    uint32_t* stk = ldsAll + wave * (stackWords + 15u) * 64u + lane;
    float* fst = reinterpret_cast<float*>(stk + stackWords * 64u);

    uint32_t nRays = 0, nMesh = 0, steps = 0;
    // the path in this lane
    bool active = false;
    uint32_t idx = 0, seed = 0;
    f3 O = mk3(0, 0, 0), D = O;
    bool inside = false; int depth = 0;
    bool more = true;                                                     // wave-uniform: the cursor has rays left
    for (;;) {
        // ---------------- refill: idle lanes draw the next rays ----------------
        const uint64_t mIdle = __builtin_amdgcn_ballot_w64(!active);
        if (more && mIdle != 0ull) {
            const uint32_t nIdle = (uint32_t)__popcll(mIdle);
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, nIdle);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            more = base + nIdle < n;                                      // base <= n + 64 * wavefronts of the launch: no wrap (n < 2^31)
            const uint32_t my = base + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mIdle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mIdle, 0u));
            if (!active && my < n) {
                const SampleRay r = rays[my];
                const uint32_t s0 = seeds[my];
                const bool traced = s0 != 0u && finite_bits(r.O[0]) && finite_bits(r.O[1]) && finite_bits(r.O[2]) && finite_bits(r.D[0]) && finite_bits(r.D[1]) &&
                                    finite_bits(r.D[2]) && !(r.D[0] == 0.0f && r.D[1] == 0.0f && r.D[2] == 0.0f);
                if (traced) {
                    idx = my; seed = s0;
                    O = mk3(r.O[0], r.O[1], r.O[2]); D = mk3(r.D[0], r.D[1], r.D[2]);
                    inside = r.inside != 0; depth = 0;
                    active = true;
                } else {                                                  // not traced: quiet NaNs, seeds[my] stays as it is
                    const float qnan = __uint_as_float(0x7fc00000u);
                    rgb[3 * (size_t)my] = qnan; rgb[3 * (size_t)my + 1] = qnan; rgb[3 * (size_t)my + 2] = qnan;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
            if (!more) break;                                             // nothing in flight, nothing left to draw
            continue;                                                     // every ray drawn was refused: draw again
        }
        // ---------------- one trip: FindNearest + the Sample branch for every lane that holds a path ----------------
        if (active) {
            f3 L = mk3(0, 0, 0);
            if (sample_step<World, false>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {
                sample_unwind(fst, depth, L);
                rgb[3 * (size_t)idx] = L.x; rgb[3 * (size_t)idx + 1] = L.y; rgb[3 * (size_t)idx + 2] = L.z;
                seeds[idx] = seed;
                active = false;
            }
        }
    }
    if (nRays) atomicAdd(&counters->v[0], (unsigned long long)nRays);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

// blocks of sample_query_kernel<World> the device holds at once with `ldsBytes` of LDS each (registers, LDS and the wave slots decide); 0 on error
template <class World>
uint32_t sample_query_resident_blocks(uint32_t ldsBytes)
{
    int perCu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, sample_query_kernel<World>, 64 * kSeqWaves, ldsBytes) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || perCu <= 0 || cus <= 0) { (void)hipGetLastError(); return 0u; }
    return (uint32_t)perCu * (uint32_t)cus;
}

// the persistent launch: the device full once, never more blocks than the rays need; `cursor` is zeroed on the stream ahead of it.  residentLanes (may be null): the
// lanes of a full launch, for the tools and tests that want an n just above it
template <class World>
hipError_t launch_sample_query(const Scene* sc, const World& world, const void* rays, uint32_t* seeds, float* rgb, uint32_t n, Counters* counters, uint32_t* cursor,
                               uint32_t* residentLanes, hipStream_t stream)
{
    const uint32_t ldsBytes = seq_lds_bytes(world.stack_words(*sc));
    if (ldsBytes > 64u * 1024u) return hipErrorInvalidValue;
    const uint32_t resident = sample_query_resident_blocks<World>(ldsBytes);
    if (resident == 0u) return hipErrorLaunchFailure;
    if (residentLanes) { *residentLanes = resident * 64u * kSeqWaves; return hipSuccess; }
    if (n == 0) return hipSuccess;
    if (!cursor || !counters) return hipErrorInvalidValue;
    if (hipMemsetAsync(cursor, 0, 4, stream) != hipSuccess) return hipGetLastError();
    const uint32_t need = (n + 64u * kSeqWaves - 1u) / (64u * kSeqWaves);
    hipLaunchKernelGGL((sample_query_kernel<World>), dim3(bounded_query_grid(need < resident ? need : resident)), dim3(64u * kSeqWaves), ldsBytes, stream, *sc, world,
                       (const SampleRay*)rays, seeds, rgb, n, counters, cursor);
    return hipGetLastError();
}

} // namespace crt
