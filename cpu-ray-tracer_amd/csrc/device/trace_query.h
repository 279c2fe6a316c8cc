// trace_query.h — trace_query_kernel: the Whitted integrator's Renderer::Trace(ray, 0) ("2. WhittedStyle/renderer.cpp":21-91) for an ARRAY of rays
// (crt_trace / crt_trace_device).  The per-ray body is trace_body.h's, the one whitted_kernel runs; what differs is where a lane's work comes from.  A pixel grid
// gives every lane one tree and the block waits for its longest; a caller's rays are independent and their trees are 1 (sky) to 2^(depthLimit + 1) - 1 (dielectrics)
// FindNearest calls long, so the launch is PERSISTENT like sample_query_kernel: the grid is what the device holds at once, and a lane whose tree has ended takes the
// next ray index from the launch-wide cursor — one atomicAdd per wavefront and trip, shared out by ballot + mbcnt ranks.
//
// One trip of the wave's loop is one trace_descend per lane that holds a tree: one FindNearest, its shading and at most one shadow walk.  The lane then runs its
// return steps (no traversal: a handful of multiply-adds on its frames) in the same trip, and the depth test of a child past depthLimit with them, until it needs
// another traversal or its root frame completes — so every trip carries a traversal for each active lane.  The wavefront ends when the cursor is exhausted and
// no lane holds a tree.
//
// Per lane: the traversal stack column in LDS (four wavefronts per workgroup, `stackWords` dwords per lane by crt_launch_whitted's rules), the 7 frames
// (kWhittedMaxDepth x WFrame = 616 bytes, indexed by the tree's depth) in private memory, as in whitted_kernel.
//
// A ray is NOT traced — three quiet NaNs, -1 in both counts — when a component of O or D is not finite or D is (0, 0, 0); the test sits in the refill, the only
// way a lane comes to hold a tree.  D is used as given (not normalised), depth starts at 0, inspection is off.
//
// Numerics: trace_body.h's (-ffp-contract=off, IEEE + - * / sqrt, crt_expf).  No MFMA.
#pragma once
#include "launch.h"
#include "trace_body.h"

namespace crt {

struct TraceRay { float O[3]; float D[3]; int32_t inside; };            // = crt_ray, 28 bytes
constexpr uint32_t kTraceWaves = 4;                                     // wavefronts per workgroup

template <int ACCEL, class ALT>
__global__ __launch_bounds__(64 * kTraceWaves, 4) void trace_query_kernel(const Scene sc, const ALT alt, const TraceRay* __restrict__ rays, float* __restrict__ rgb,
                                                                          int32_t* __restrict__ travOut, int32_t* __restrict__ testedOut, uint32_t n, uint32_t stackWords,
                                                                          Counters* __restrict__ counters, uint32_t* __restrict__ cursor)
{
    extern __shared__ uint32_t ldsAll[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t* stk = ldsAll + wave * stackWords * 64u + lane;             // this lane's traversal stack column
    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    // the tree in this lane
    WFrame fr[kWhittedMaxDepth];
    TraceState t;
    trace_begin(t, mk3(0, 0, 0), mk3(0, 0, 0), false);
    bool active = false;
    uint32_t idx = 0;
    int32_t primTraversed = 0, primTested = 0;
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
                const TraceRay r = rays[my];
                const bool traced = finite_bits(r.O[0]) && finite_bits(r.O[1]) && finite_bits(r.O[2]) && finite_bits(r.D[0]) && finite_bits(r.D[1]) && finite_bits(r.D[2]) &&
                                    !(r.D[0] == 0.0f && r.D[1] == 0.0f && r.D[2] == 0.0f);
                if (traced) {
                    idx = my;
                    trace_begin(t, mk3(r.O[0], r.O[1], r.O[2]), mk3(r.D[0], r.D[1], r.D[2]), r.inside != 0);
                    primTraversed = 0; primTested = 0;
                    active = true;
                } else {                                                  // not traced: quiet NaNs, -1 in the counts
                    const float qnan = __uint_as_float(0x7fc00000u);
                    rgb[3 * (size_t)my] = qnan; rgb[3 * (size_t)my + 1] = qnan; rgb[3 * (size_t)my + 2] = qnan;
                    if (travOut) travOut[my] = -1;
                    if (testedOut) testedOut[my] = -1;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
            if (!more) break;                                             // nothing in flight, nothing left to draw
            continue;                                                     // every ray drawn was refused: draw again
        }
        // ---------------- one trip: one descend step for every lane that holds a tree, then its return steps ----------------
        if (active) {
            trace_descend<ACCEL, true>(sc, alt, stk, cn, t, fr, primTraversed, primTested);
            for (;;) {
                if (t.descend) { if (!trace_depth_cut(sc, t)) break; }    // the next traversal waits for the next trip; a child past depthLimit returns 0 here
                else if (trace_return(t, fr)) {
                    rgb[3 * (size_t)idx] = t.res.x; rgb[3 * (size_t)idx + 1] = t.res.y; rgb[3 * (size_t)idx + 2] = t.res.z;
                    if (travOut) travOut[idx] = primTraversed;
                    if (testedOut) testedOut[idx] = primTested;
                    active = false;
                    break;
                }
            }
        }
    }
    // whitted_kernel's counters for the same rays; `primary` stays 0: these are a caller's rays
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t s = wave_sum(vals[k]);
        if (lane == 0 && s) atomicAdd(&counters->v[k], (unsigned long long)s);
    }
}

// blocks of trace_query_kernel<ACCEL, ALT> the device holds at once with `ldsBytes` of LDS each (registers, LDS and the wave slots decide); 0 on error
template <int ACCEL, class ALT>
uint32_t trace_query_resident_blocks(uint32_t ldsBytes)
{
    int perCu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, trace_query_kernel<ACCEL, ALT>, 64 * kTraceWaves, ldsBytes) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || perCu <= 0 || cus <= 0) { (void)hipGetLastError(); return 0u; }
    return (uint32_t)perCu * (uint32_t)cus;
}

// the persistent launch: the device full once, never more blocks than the rays need; `cursor` is zeroed on the stream ahead of it.  stackWords: dwords of traversal
// stack per lane.  residentLanes (may be null): the lanes of a full launch, for the tools and tests that want an n just above it — then nothing is launched
template <int ACCEL, class ALT>
hipError_t launch_trace_query(const Scene* sc, const ALT& alt, uint32_t stackWords, const void* rays, float* rgb, int32_t* trav, int32_t* tested, uint32_t n, Counters* counters,
                              uint32_t* cursor, uint32_t* residentLanes, hipStream_t stream)
{
    const uint64_t lds = (uint64_t)stackWords * 64u * 4u * kTraceWaves;
    if (lds > 64u * 1024u) return hipErrorInvalidValue;
    const uint32_t ldsBytes = (uint32_t)lds;
    const uint32_t resident = trace_query_resident_blocks<ACCEL, ALT>(ldsBytes);
    if (resident == 0u) return hipErrorLaunchFailure;
    if (residentLanes) { *residentLanes = resident * 64u * kTraceWaves; return hipSuccess; }
    if (n == 0) return hipSuccess;
    if (!cursor || !counters) return hipErrorInvalidValue;
    if (hipMemsetAsync(cursor, 0, 4, stream) != hipSuccess) return hipGetLastError();
    const uint32_t need = (n + 64u * kTraceWaves - 1u) / (64u * kTraceWaves);
    hipLaunchKernelGGL((trace_query_kernel<ACCEL, ALT>), dim3(bounded_query_grid(need < resident ? need : resident)), dim3(64u * kTraceWaves), ldsBytes, stream, *sc, alt,
                       (const TraceRay*)rays, rgb, trav, tested, n, stackWords, counters, cursor);
    return hipGetLastError();
}

} // namespace crt
