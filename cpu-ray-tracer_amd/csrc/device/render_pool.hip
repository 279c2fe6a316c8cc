// render_pool.hip — render_pool_kernel: the path tracer's per-tile sample loop ("3. PathTracer/renderer.cpp":117-131, Sample :50-100,
// FindNearest infra/scene/file_scene.cpp:170-175 / tlas_file_scene.cpp:201-206, IntersectBVH infra/bvh.cpp:224-258) as a STREAM POOL.
//
// The unit of work is the reference's RNG stream: one xorshift32 stream per (tile, frame), consumed serially over the tile's 256
// pixels (renderer.cpp:120-126).  A wavefront has S > 64 stream SLOTS and owns a range [frame0, frame0 + n) of one tile's frames: the first min(n, S) streams
// start in the slots, and a slot whose stream has rendered its 256 pixels takes the range's next frame (REFILL, in the END pass), so the wavefront's population stays
// at S until the range runs out instead of falling from S to 0 over the last part of every 128 frames.  Which slot renders a stream has no influence on its samples:
// the seed and the slab position depend on the frame alone.  A wavefront has only 64 lanes, and a stream is not tied to a lane:
//   * a stream that is WALKING the acceleration structure is resident in a lane: its ray, nearest hit, node reference and
//     pre-loaded node / triangle record live in that lane's registers, its traversal stack in the lane's LDS column;
//   * a stream that WAITS for shading is parked in LDS (ray, hit, RNG state, pixel counter, the path's throughput factors —
//     14 dwords; the path's throughput factors in a global scratch area) and queued by what it needs next: the END queue (the path ended: sky lookup or light / depth limit, unwind the
//     throughput factors, store the sample, generate the next pixel's primary ray) or the BOUNCE queue (surface hit: normal,
//     uv, albedo, mirror / dielectric / rejection-sampled diffuse direction);
//   * a shading pass takes up to 64 streams from ONE queue — all lanes run the same branch of Renderer::Sample — starts each
//     stream's next FindNearest (light quad, floor plane, the root step from the kernel arguments) and queues the stream as
//     READY to walk, or, when the ray misses both root children, straight back into a shading queue;
//   * lanes whose stream finished walking take the next READY stream.
// So the traversal phases run on lanes that are (nearly) all walking and the shading passes on (nearly) full wavefronts, instead
// of every phase running on the sub-set of 64 fixed streams that happens to be in that state (render_tiles_kernel).  Per stream
// nothing changes: every ray visits the reference's nodes in the reference's order and every float expression is evaluated as
// written there, so the image is bit-identical to render_tiles_kernel's and to the CPU oracle's.
//
// The Sample body — the surface of a hit, medium, the bounce and its factor, the primary ray, the ordered two-child step — is sample_body.h's: the functions
// render_tiles_kernel and the sequential kernels shade with, not a copy.  This file decides where the operands come from and when their loads are issued.
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only (dev_common.h).  No MFMA: pointer chasing + slab / Möller–Trumbore tests.
#include <type_traits>
#include "launch.h"
#include "sample_body.h"

namespace crt {

// parked stream state, SoA in LDS: field f of stream s at st[f * S + s]
enum : uint32_t {
    F_OX = 0, F_OY, F_OZ, F_DX, F_DY, F_DZ,                      // ray origin, direction (world space)
    F_RX, F_RY, F_RZ,                                            // reciprocal direction: needed until the walk is over (swap-in, return from a BLAS)
    F_T,                                                         // nearest hit distance: after the quad / plane tests, then FindNearest's result
    F_SEED, F_META,                                              // RNG state; item | depth << 11 | inside << 14 | fresh << 15 | (hit objIdx + 1) << 16
    F_U, F_V,                                                    // barycentrics of a mesh hit (after the walk)
    F_COUNT,                                                     // 14 dwords = 56 bytes per parked stream
    // slots with two lives:
    F_CUR = F_U, F_PEND = F_V,                                   // what a READY stream needs before the walk: node reference to start at, far root child to push (0 = none)
    F_TRI = F_RX                                                 // after the walk: the hit triangle's global shade index
};
// The path's throughput factors (albedo*medium*... of each bounce, multiplied on unwind: 15 floats, written once per bounce, read once
// per path) live in a global scratch area behind the launch's sample slab instead of LDS — 8 KB per wave that buy a third wave per SIMD:
// component j of depth k of stream s of block b at fac[(b * 15 + 3k + j) * S + s].
constexpr uint32_t kMetaItemMask = 0x7ffu, kMetaDepthShift = 11u, kMetaInside = 1u << 14, kMetaFresh = 1u << 15, kMetaObjShift = 16u, kMetaLowMask = 0xffffu;
constexpr uint32_t kQueueMask = 127u;                            // queues are rings of 128 one-byte stream ids (S <= 128)

#ifndef CRT_POOL_MIN_WAVES
#define CRT_POOL_MIN_WAVES 4         // waves per SIMD the register budget must allow (<= 128 VGPRs)
#endif
#ifndef CRT_POOL_WIDE_MIN_WAVES
#define CRT_POOL_WIDE_MIN_WAVES 4    // ... of the 32-bit-reference form (LDS allows 3 - 4: DESIGN.md 3a)
#endif
#ifndef CRT_POOL_NODE_STEPS
#define CRT_POOL_NODE_STEPS 2     // NODE steps per trip of the lanes that stay at interior nodes
#endif
#ifndef CRT_POOL_NODE2_MIN
#define CRT_POOL_NODE2_MIN 16     // ... as long as at least this many lanes take the further step
#endif
#ifndef CRT_POOL_STARVE
#define CRT_POOL_STARVE 40        // a shading pass waits for a full queue (64 streams) unless fewer than this many streams are walking or ready to walk
#endif

#ifdef CRT_POOL_STAMPS
// diagnostic build only (-DCRT_POOL_STAMPS, tools/pool_stamps.py): shader-clock time of the sections of the loop, summed over all waves:
// [0] walk phases + swap out (incl. the wait for the records), [1] swap in + record loads + pass decision, [2] END pass up to its new_ray, [3] END's new_ray, [4] END tail (unwind, store),
// [5] BOUNCE up to the material draw, [6] material draw + rejection loop, [7] normalise + factor store, [8] BOUNCE's new_ray, [9] trips, [10] END passes, [11] BOUNCE passes
__device__ unsigned long long g_poolStamps[16];
#define CRT_PSTAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory")
#define CRT_PACC(i, a, b) (pst[i] += (b) - (a))
#else
#define CRT_PSTAMP(var)
#define CRT_PACC(i, a, b)
#endif
#ifdef CRT_POOL_DENS
// diagnostic build only (-DCRT_POOL_DENS, tools/pool_density.py): how often every section of the loop runs and with how many lanes, summed over all waves
// [32 + 4 * k + b]: by the wave's LIVE streams (slots whose stream has not yet rendered its 256 pixels; bucket b: 0 = >= 112, 1 = 96..111, 2 = 64..95, 3 = < 64)
//   k = 0 trips, 1 END passes, 2 BOUNCE passes, 3 wall-clock ticks (100 MHz) of the wave's life
// [30], [31]: the trips and the shading passes (END + BOUNCE) of the wavefronts whose tile carries kTileFloor
__device__ unsigned long long g_poolDens[48];
#define CRT_DENS(i, v) (dens[i] += (uint32_t)(v))
#define CRT_DENS_MASK(i, pred) (dens[i] += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(pred)))
#define CRT_LIVE_BUCKET(n) ((n) >= 112u ? 0u : (n) >= 96u ? 1u : (n) >= 64u ? 2u : 3u)
#else
#define CRT_DENS(i, v)
#define CRT_DENS_MASK(i, pred)
#endif
#ifdef CRT_POOL_TIMELINE
// diagnostic build only (-DCRT_POOL_TIMELINE, tools/pool_timeline.py): start / end wall clock (100 MHz) and compute unit of every wavefront of the last launch
__device__ unsigned long long* g_poolTimeline = nullptr;
#endif
// Lane sets of the loop are explicit 64-bit scalar masks (mRes: lanes holding a resident stream; mNode / mTri / mTlas: what each resident lane is at) and a
// per-lane predicate is `lane_in(mask)` = the mask used directly as the execution / select mask (amdgcn inverse ballot): no v_cndmask + v_cmp round trip per
// ballot, and `resident` never has to be re-derived from lane state.
__device__ __forceinline__ bool lane_in(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// lanes (of the active ones) whose three components are all finite: three compares straight into scalar masks.  |x| < inf is false for inf and NaN alike, i.e. it is
// finite3's "exponent not all ones"; the compare builtin returns the lane mask itself, where the ballot of a bool goes through a VGPR (v_cndmask 0 / 1 + v_cmp_ne).
__device__ __forceinline__ uint64_t finite3_mask(f3 v)
{
    const float inf = __builtin_inff();
    return __builtin_amdgcn_fcmpf(__builtin_fabsf(v.x), inf, 4) & __builtin_amdgcn_fcmpf(__builtin_fabsf(v.y), inf, 4) & __builtin_amdgcn_fcmpf(__builtin_fabsf(v.z), inf, 4);   // 4 = ordered and less than
}
// The loop's wave-uniform decisions are scalar compares in front of scalar branches: nested `if`s on 32-bit counts, no `bool` carried across a join (the
// compiler materialises such a flag as a 64-bit lane mask: s_cselect_b64 -1 / 0, s_and / s_or_b64, s_andn2_b64 vcc, exec + s_cbranch_vccnz).  pop32: a mask's
// population as a 32-bit scalar the compiler cannot widen again; CRT_CTL_SEQ: an empty statement that keeps two nested uniform `if`s from being merged back into
// one flag expression.
#define CRT_CTL_SEQ() asm volatile("")
__device__ __forceinline__ bool ctl_free(uint64_t mRes) { CRT_CTL_SEQ(); return mRes != ~0ull; }      // any lane without a stream? (as the inner of two nested tests)
// a launch constant as a value the compiler must compare where it is asked about: a test of it is then s_cmp + s_cbranch_scc at the place of use, not a 64-bit
// flag formed in front of the loop, kept in (spilled) SGPRs for the wavefront's life and negated through a VGPR (v_cndmask 0 / 1 + v_cmp_ne) where its opposite is wanted
__device__ __forceinline__ uint32_t fresh(uint32_t x) { asm("" : "+s"(x)); return x; }
__device__ __forceinline__ uint32_t pop32(uint64_t m) { uint32_t n = (uint32_t)__builtin_popcountll(m); asm("" : "+s"(n)); return n; }
// Lane sets straight from a compare of values every lane holds (a lane without a stream holds the value that keeps it out of the set): the compare builtins return
// the lane mask, where the ballot of a `bool` that was assigned under a divergent `if` goes through a VGPR (v_cndmask 0 / 1 + v_cmp_ne, both half rate).
__device__ __forceinline__ uint64_t mask_ne(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 33); }    // LLVM's integer predicates: 32 eq, 33 ne,
__device__ __forceinline__ uint64_t mask_eq(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 32); }    // 36 unsigned <, 37 unsigned <=, 39 signed >=
__device__ __forceinline__ uint64_t mask_ult(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 36); }
__device__ __forceinline__ uint64_t mask_ule(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 37); }
__device__ __forceinline__ uint64_t mask_sge(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 39); }
// lanes (of the active ones) whose walk may run the short slab test (dev_common.h box_short): finite reciprocal direction AND a tray the short accept predicate
// holds for (tray_tame: bit pattern >= 2 as a signed integer).  A stream's tray is set when it is swapped in and falls only to accepted triangle hits (t > 1e-4),
// so a lane that is tame when it enters a walk stays tame, and one that is not (a light / floor hit at a denormal t) accepts nothing and stays as it is.
__device__ __forceinline__ uint64_t short_slab_mask(f3 rD, float tray) { return finite3_mask(rD) & mask_sge((int)asu(tray), 2); }
__device__ __forceinline__ uint32_t rank_in(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }   // set bits below this lane

// REFBITS: the width of the scene's pool references (layout.h: 16 or 32) — of `cur`, of the stack entries and of the constants that classify them
template <int KIND, bool COUNT, int S, int REFBITS = 16>
__global__ __launch_bounds__(64, REFBITS == 32 ? CRT_POOL_WIDE_MIN_WAVES : CRT_POOL_MIN_WAVES) void render_pool_kernel(const Scene sc, char* __restrict__ slab, float* __restrict__ facScratch, Counters* __restrict__ counters,
                                                             unsigned long long* __restrict__ tileClocks, const uint32_t* __restrict__ tileOrder,
                                                             uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                             uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t groups, uint32_t waveFrames, const uint32_t* __restrict__ waveTab, uint32_t tabBlocks, uint32_t longFrames,
                                                             uint32_t rankFirst, uint32_t* __restrict__ tileCost, unsigned long long* __restrict__ launchClk, const uint8_t* __restrict__ tileClass)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
#ifdef CRT_POOL_TIMELINE
    const unsigned long long tl0 = wall_clock64();
#endif
    const unsigned long long clk0 = (COUNT || tileCost) ? wall_clock64() : 0ull;
    if (launchClk && lane == 0) { atomicMax(&launchClk[0], ~clk0); atomicMax(&launchClk[1], clk0); }     // first / last wavefront start of a measuring job (abi.cpp adopt_job_costs)
    // block -> (tile rank, frame range), rank-major: all wavefronts of the expensive tiles (listed first by the host) are dispatched first;
    // rankFirst > 0: the tiles before it in the order are rendered by a concurrent render_tiles_kernel launch (a split job, abi.cpp).
    // Every tile the same range length (waveFrames, `groups` wavefronts per tile), or a plan (abi.cpp pool_wave_plan) in two parts.  The first tabBlocks wavefronts render
    // the frames [0, longFrames) of every tile with a range length per rank: waveTab[2 r] = first block and waveTab[2 r + 1] = range length of rank rankFirst + r (a
    // divisor of longFrames) — searched once per wavefront, on the scalar unit (the block index is wave-uniform).  The wavefronts behind them render the frames
    // [longFrames, frames) with S frames each, `groups` per tile, rank-major again: the short wavefronts that fill the launch's end.
    uint32_t rank0, grp, wf = waveFrames, first = 0u, limit = frames;
    if (waveTab) {
        if (blockIdx.x < tabBlocks) {
            uint32_t lo = 0u, hi = tileCount - rankFirst;                         // the last rank whose first block is <= this block
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (waveTab[2u * mid] <= blockIdx.x) lo = mid; else hi = mid; }
            rank0 = lo; grp = blockIdx.x - waveTab[2u * lo]; wf = waveTab[2u * lo + 1u]; limit = longFrames;
        } else { const uint32_t b = blockIdx.x - tabBlocks; rank0 = b / groups; grp = b - rank0 * groups; wf = (uint32_t)S; first = longFrames; }
    } else { rank0 = blockIdx.x / groups; grp = blockIdx.x - rank0 * groups; }
    const uint32_t rank = rank0 + rankFirst;
    if (rank >= tileCount) return;
    const uint32_t tl = tileOrder ? tileOrder[rank] : rank;
    const uint32_t frame0 = first + grp * wf;                                    // first frame (of the launch) of this wave's range
    if (frame0 >= limit) return;
    const uint32_t nOwn = (limit - frame0 < wf) ? limit - frame0 : wf;           // frames of the range
    const uint32_t nStreams = nOwn < (uint32_t)S ? nOwn : (uint32_t)S;           // ... of which this many start now, one per slot
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    // what the tile's primary rays cannot hit (layout.h kTileNo*, proven on the host: tile_class.h), one scalar for the wavefront's life; 0 = every test runs.
    // Only new_ray's primary form and the END pass look at it, and only to skip, under a scalar branch, a test whose outcome is known
    // kTileFloorSure (every primary ray hits the floor: floor_ray, below) is dropped here, once, when the depth limit is 0: a floor hit at depth 0 then ends the path
    // instead of bouncing, which is new_ray's general form
    const uint32_t tcls = tileClass ? __builtin_amdgcn_readfirstlane((uint32_t)tileClass[tl] & (sc.depthLimit > 0 ? ~0u : ~kTileFloorSure)) : 0u;
    // "not a sky tile" is compared afresh by each test that asks (fresh(), above)
    auto not_sky = [&]() -> bool { return fresh(tcls) != kTileSky; };
    const char* __restrict__ geom = sc.geom;
    float* __restrict__ fac = facScratch + (size_t)blockIdx.x * (15u * (uint32_t)S);

    // `cur` and the stack entries of this kernel are pool references (layout.h: ref16 — the children's are stored next to the offset form in every
    // NodePair), REFBITS wide.  A scene that fits the 16-bit form gets 2 bytes per stack entry instead of 4, which is what lets 128 parked streams + the stacks
    // fit 4 waves per SIMD; every other scene is in the 32-bit form: 4 bytes per entry, a wave per SIMD less on deep trees, the same walk.
    // Traversal stack of the stream resident in a lane: entry i (1 .. stackDepth) at LDS byte  kEntryB * lane + kLevelB * i;  entry 0 is a dummy below the bottom, so
    // the speculative read of the top and the dead store above it need no bounds logic, and the stack pointer IS the byte address of the top entry (`spB`).
    constexpr PoolRefForm R = pool_ref_form((uint32_t)REFBITS);
    using StackEntry = std::conditional_t<REFBITS == 32, uint32_t, uint16_t>;
    constexpr uint32_t kEntryB = (uint32_t)sizeof(StackEntry), kLevelB = 64u * kEntryB;   // bytes per entry, per stack level of the wavefront
    char* const ldsB = reinterpret_cast<char*>(lds);
    const uint32_t laneB = lane * kEntryB;
    uint32_t* st = lds + (sc.stackDepth + 1u) * (kLevelB / 4u);                  // parked stream state (behind (stackDepth + 1) * 64 stack entries)
    float* stf = reinterpret_cast<float*>(st);
    uint8_t* qEnd = reinterpret_cast<uint8_t*>(st + F_COUNT * S);
    uint8_t* qBnc = qEnd + 128, * qRdy = qEnd + 256;
    uint16_t* slotFrame = reinterpret_cast<uint16_t*>(qEnd + 384);               // S > 64 only: frame (relative to frame0) of the stream in each slot
    auto stk_top = [&](uint32_t at) -> uint32_t { return *reinterpret_cast<const StackEntry*>(ldsB + at); };
    auto stk_put = [&](uint32_t at, uint32_t v) { *reinterpret_cast<StackEntry*>(ldsB + at) = (StackEntry)v; };

    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    uint32_t trips = 0;
#ifdef CRT_POOL_DENS
    uint32_t dens[48]; for (int i = 0; i < 48; i++) dens[i] = 0;
    uint32_t live = nStreams; unsigned long long liveClk = wall_clock64();
#endif
    const uint32_t items = 256u * passes;                                        // (pixel, pass) pairs in stream order
    const uint32_t rowLen = 64u * passes;                                        // samples per pixel row of the slab
    const f3 nil3 = mk3(0.0f, 0.0f, 0.0f);                                       // placeholder of values no lane reads

    // every stream starts in the END queue as "fresh": the pass only generates its first primary ray
    for (uint32_t s = lane; s < nStreams; s += 64u) {
        st[F_SEED * S + s] = stream_seed(tx, ty, (uint32_t)sc.W, sppFirst, frame0 + s, passes);
        st[F_META * S + s] = kMetaFresh;
        qEnd[s] = (uint8_t)s;
        if (S > 64) slotFrame[s] = (uint16_t)s;
    }
    // streams of the wavefront that have not rendered their 256 pixels yet — walking or in a queue; falls only in the END pass, when a stream's last path ends and no
    // frame is left for its slot.  The loop ends when it reaches zero: one scalar compare at the foot of a trip.  (That is the moment the walking lanes and the three
    // queues are all empty.)
    uint32_t nLive = nStreams;
    uint32_t nextFrame = nStreams;                                               // the range's next frame (relative to frame0) without a slot (wave-uniform; only grows)
    uint32_t endH = 0, endT = nStreams, bncH = 0, bncT = 0, rdyH = 0, rdyT = 0;  // queue heads / tails (wave-uniform)

    // The stream resident in this lane (if any: mRes).  Invariant at the top of a trip: a resident stream is walking (cur != done) — streams whose walk ended
    // leave their lane in the trip that ended it, and only streams with a walk ahead are ever READY.
    uint64_t mRes = 0ull;                                                        // lanes holding a stream
    uint64_t mFinite = ~0ull;                                                    // ... whose reciprocal direction is finite in all components and whose tray is tame (short_slab_mask: the v_min / v_max slab test is exact)
    uint32_t sid = 0, cur = kRefDone, spB = laneB, metaLo = 0u;
    f3 tO = nil3, tD = nil3, trD = nil3;
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    rec4 q0 = {0, 0, 0, 0}, q1 = q0, q2 = q0, q3 = q0;

    // ---- the start of a stream's next scene.FindNearest, shared by both shading passes: normalise, reciprocal direction, light quad,
    // floor plane, root step; parks the new ray and queues the stream (READY, or END / BOUNCE when the ray never enters the tree)
    // `primary` (a compile-time tag): the ray starts at the camera (the END pass), and the operands that depend on the origin alone come from the Scene's
    // camera-relative block (layout.h: primRoot, primLight, primFloor, formed on the host) instead of being recomputed by every lane.
    // The tile class applies to these rays only.
    // mAct: the lanes with a new ray, as the caller's scalar mask
    auto new_ray = [&](auto primary, uint64_t mAct, uint32_t s, f3 v, bool norm, f3 O, uint32_t seed, uint32_t meta) {
        constexpr bool PRIM = decltype(primary)::value;
        const bool act = lane_in(mAct);
        // a sky tile (all three bits): the ray misses light, floor and tree, so FindNearest is over before it starts and the stream goes straight back to the END queue.
        // Parked is only what that pass reads of a missed path: the direction (sky lookup), the RNG state, meta with depth 0 and object field 0 (= miss).
        const bool noLight = PRIM && (tcls & kTileNoLight) != 0u, noFloor = PRIM && (tcls & kTileNoFloor) != 0u, noTree = PRIM && (tcls & kTileNoTree) != 0u;
        f3 D = v, rD = v; Hit nh; nh.t = 1e34f; nh.u = 0; nh.v = 0; nh.objIdx = -1; nh.triIdx = -1;
        uint32_t ncur = kRefDone, pend = 0u;
        if (act) {
            const float inv = rcp_exact(sqrt_exact(dot3(v, v)));                  // normalize(): v * (1 / sqrtf(dot(v, v)))
            D = norm ? v * inv : v;
            cn.rays++;
            if (!PRIM || not_sky()) {
                rD = rcp_exact3(D);
                hit_light_floor<PRIM>(light_floor_from_kernarg<PRIM>(), O, D, nh, noLight, noFloor);
            }
            if (noTree) {
                // both slab tests are known to fail: ncur = done, nothing pending; the reference's root step is still counted
                if (COUNT) { if (KIND == 0) cn.interior++; else cn.tlas++; }
            } else if (sc.rootIsPair) {
                // bvh.cpp:244-257 / tlas_bvh.cpp:96-110 at the root with an empty stack, from the child pair in the kernel arguments
                const kernarg_f rp = scene_floats(offsetof(Scene, rootPair));
                const rec4 a0 = {rp[0], rp[1], rp[2], rp[3]}, a1 = {rp[4], rp[5], rp[6], rp[7]};
                const rec4 b0 = {rp[8], rp[9], rp[10], rp[11]}, b1 = {rp[12], rp[13], rp[14], rp[15]};
                float d1, d2;
                const bool allFinite = (__builtin_amdgcn_ballot_w64(true) & ~short_slab_mask(rD, nh.t)) == 0ull;
                const float tp = tray_pred(nh.t);
                if constexpr (PRIM) {
                    // rp[16 ..]: primRoot, the four corners minus the camera position (behind rootPair in the Scene)
                    const f3 ra0 = mk3(rp[16], rp[17], rp[18]), ra1 = mk3(rp[19], rp[20], rp[21]), rb0 = mk3(rp[22], rp[23], rp[24]), rb1 = mk3(rp[25], rp[26], rp[27]);
                    if (allFinite) { d1 = box_short_rel(ra0, ra1, rD, tp); d2 = box_short_rel(rb0, rb1, rD, tp); }
                    else { d1 = box_exact_rel(ra0, ra1, rD, nh.t); d2 = box_exact_rel(rb0, rb1, rD, nh.t); }
                } else if (allFinite) { d1 = box_short(a0, a1, O, rD, tp); d2 = box_short(b0, b1, O, rD, tp); }
                else { d1 = box_exact(a0, a1, O, rD, nh.t); d2 = box_exact(b0, b1, O, rD, nh.t); }
                const Ordered o = ordered_step(d1, d2, asu(a1.w), asu(b1.w));        // the children's ref16
                pend = o.push ? o.farRef : 0u;
                ncur = o.hitN ? o.nearRef : kRefDone;
                if (COUNT) { if (KIND == 0) cn.interior++; else cn.tlas++; }
            } else ncur = sc.rootRef16;
            if (COUNT && KIND == 0 && (ncur & R.tagMask) == 0u && ncur != kRefDone) cn.leaf++;
            if (!PRIM || not_sky()) {
                stf[F_OX * S + s] = O.x; stf[F_OY * S + s] = O.y; stf[F_OZ * S + s] = O.z;
                stf[F_RX * S + s] = rD.x; stf[F_RY * S + s] = rD.y; stf[F_RZ * S + s] = rD.z;
                stf[F_T * S + s] = nh.t;
                st[F_CUR * S + s] = ncur; st[F_PEND * S + s] = pend;
            }
            stf[F_DX * S + s] = D.x; stf[F_DY * S + s] = D.y; stf[F_DZ * S + s] = D.z;
            st[F_SEED * S + s] = seed; st[F_META * S + s] = meta | ((uint32_t)(nh.objIdx + 1) << kMetaObjShift);
        }
        // queue: the walk is needed only when the ray enters the tree; otherwise FindNearest is already over (renderer.cpp:52-55, 69).  Every set is the ballot of ONE
        // comparison combined with scalar logic.  (A sky tile: every new ray is a finished path — one set, no further ballots.)
        uint64_t mW = 0ull, mE = mAct, mB = 0ull;
        if (!PRIM || not_sky()) {
            const uint32_t depth = (meta >> kMetaDepthShift) & 7u;
            mW = mAct & mask_ne(ncur, kRefDone);                               // (ncur, nh.objIdx and depth are defined on every lane)
            const uint64_t mStop = mask_ule((uint32_t)(nh.objIdx + 1), 1u) | mask_sge((int)depth, sc.depthLimit);   // miss, light, or depth limit
            mE = mAct & ~mW & mStop; mB = mAct & ~mW & ~mStop;
            if (lane_in(mW)) qRdy[(rdyT + rank_in(mW)) & kQueueMask] = (uint8_t)s;
            if (lane_in(mB)) qBnc[(bncT + rank_in(mB)) & kQueueMask] = (uint8_t)s;
            rdyT += (uint32_t)__popcll(mW); bncT += (uint32_t)__popcll(mB);
        }
        CRT_DENS(20, __popcll(mAct)); CRT_DENS(19, __popcll(mW));
        if (lane_in(mE)) qEnd[(endT + rank_in(mE)) & kQueueMask] = (uint8_t)s;
        endT += (uint32_t)__popcll(mE);
    };
    // ---- the primary form of new_ray in a kTileFloor wavefront (layout.h; the host's proof: tile_class.h): every primary ray misses the light quad and both root
    // children and passes the floor plane's test, and the depth limit is above 0 (tcls, above), so the outcome of new_ray's general form is known for every lane:
    // nh = {t = -primFloor / D.y (hit_light_floor<true>'s floorAxisY expression), objIdx 1}, ncur = done, and the stream goes to the BOUNCE queue.  What is left is
    // what that pass reads of a floor hit: O, D, t, the RNG state and meta with the floor's object field.  The reciprocal direction, CUR and PEND (alias F_TRI, F_U,
    // F_V) feed a root test and a walk that do not happen; the BOUNCE pass loads those slots but uses them for mesh hits only.
    auto floor_ray = [&](uint64_t mAct, uint32_t s, f3 v, f3 O, uint32_t seed, uint32_t meta) {
        if (lane_in(mAct)) {
            const float inv = rcp_exact(sqrt_exact(dot3(v, v)));                  // normalize(): v * (1 / sqrtf(dot(v, v)))
            const f3 D = v * inv;
            cn.rays++;
            if (COUNT) { if (KIND == 0) cn.interior++; else cn.tlas++; }           // the reference's root step is still counted
            const kernarg_f pf = scene_floats(offsetof(Scene, primFloor));
            const float t = -pf[0] / D.y;
            stf[F_OX * S + s] = O.x; stf[F_OY * S + s] = O.y; stf[F_OZ * S + s] = O.z;
            stf[F_DX * S + s] = D.x; stf[F_DY * S + s] = D.y; stf[F_DZ * S + s] = D.z;
            stf[F_T * S + s] = t;
            st[F_SEED * S + s] = seed; st[F_META * S + s] = meta | (2u << kMetaObjShift);
            qBnc[(bncT + rank_in(mAct)) & kQueueMask] = (uint8_t)s;
        }
        CRT_DENS(20, __popcll(mAct));
        bncT += (uint32_t)__popcll(mAct);
    };
    // back to the world-space ray when a BLAS is finished (two-level scenes): the parked copy is the world-space ray
    auto world_ray = [&]() {
        tO = mk3(stf[F_OX * S + sid], stf[F_OY * S + sid], stf[F_OZ * S + sid]);
        tD = mk3(stf[F_DX * S + sid], stf[F_DY * S + sid], stf[F_DZ * S + sid]);
        trD = mk3(stf[F_RX * S + sid], stf[F_RY * S + sid], stf[F_RZ * S + sid]);
    };

    // ---------------- NODE step (infra/bvh.cpp:244-257 / tlas_bvh.cpp:96-110) of the lanes in m, on their pre-loaded NodePair ----------------
    // Which slab test the step runs — the v_min / v_max form with the short accept predicate (box_short), exact while every stepping lane is in mFinite, or the ordered-compare form — is a
    // property of the trip: the walk tests it once, on the lanes of the first step (mFinite changes in swap-in, at a TLAS leaf and at a BLAS return only, none of which
    // lies between a trip's NODE steps for the lanes that step), and calls the steps with the answer as a compile-time tag.  The exact form is then one out-of-line
    // region of the loop instead of a uniform branch inside every step's divergent region.
    uint64_t mNode2 = 0ull;
    auto node_step = [&](auto exactTag, uint64_t m) {
        constexpr bool allFinite = !decltype(exactTag)::value;
        if (lane_in(m)) {
            if (COUNT) { if (KIND == 1 && (cur & R.tlasBit) != 0u) cn.tlas++; else cn.interior++; }
            const uint32_t top = stk_top(spB);                               // speculative: lands during the slab arithmetic (the dummy entry when the stack is empty)
            float d1, d2;
            if constexpr (allFinite) { const float tp = tray_pred(h.t); d1 = box_short(q0, q1, tO, trD, tp); d2 = box_short(q2, q3, tO, trD, tp); }
            else { d1 = box_exact(q0, q1, tO, trD, h.t); d2 = box_exact(q2, q3, tO, trD, h.t); }
            const Ordered o = ordered_step(d1, d2, asu(q1.w), asu(q3.w));    // the children's ref16
            stk_put(spB + kLevelB, o.farRef);                                   // dead store unless `push`
            const bool pop = !o.hitN && spB != laneB;
            cur = o.hitN ? o.nearRef : (pop ? top : kRefDone);
            spB = spB + (o.push ? kLevelB : 0u) - (pop ? kLevelB : 0u);
            if (COUNT && (cur & R.tagMask) == 0u && cur != kRefDone) cn.leaf++;
        }
    };
    // where the record of `cur` lies in geom: record offset of a pool reference = index * record size + section base (layout.h)
    auto record_offset = [&]() -> uint32_t {
        const uint32_t idx = cur & R.indexMask;
        const bool inter = (cur & R.interior) != 0u;
        uint32_t oa = idx * (inter ? 64u : 48u) + (inter ? 0u : sc.leafOff - 48u);             // NodePair | LeafTri (one multiply-add on selected operands: no divergent arms)
        if (KIND == 1 && (cur & R.tlasBit) != 0u)
            oa = (cur & R.interior) ? sc.instOff + idx * 128u : sc.tlasPairOff + idx * 64u;   // TLAS leaf: Instance {invT rows, ids} | TLAS interior: its child pair
        return oa;
    };
    // the record of `cur` into q0..q3 for the lanes in m (the others keep theirs)
    auto load_records = [&](uint64_t m) {
        const uint32_t oa = record_offset();
        if (lane_in(m)) { q0 = ldp<0>(geom, oa); q1 = ldp<1>(geom, oa); q2 = ldp<2>(geom, oa); q3 = ldp<3>(geom, oa); }
    };

    // ---------------- TRI step of the lanes in m: one triangle of the current leaf (infra/bvh.cpp:203-222, 232-243), on the pre-loaded LeafTri ----------------
    auto tri_step = [&](uint64_t m) {
        CRT_DENS(3, 1); CRT_DENS(4, __popcll(m));
        if (lane_in(m)) {
            if (COUNT) cn.tri++;
            const uint32_t top = stk_top(spB);
            hit_tri(q0, q1, q2, tO, tD, h);
            const bool more = asu(q2.w) > 1u;                                // the leaf's next LeafTri is the next index
            const bool pop = !more && spB != laneB;
            const uint32_t next = more ? cur + 1u : (pop ? top : kRefDone);
            spB -= pop ? kLevelB : 0u;
            if (COUNT && !more && (next & R.tagMask) == 0u && next != kRefDone) cn.leaf++;
            cur = next;
        }
    };

#ifdef CRT_POOL_STAMPS
    unsigned long long pst[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    for (;;) {
        CRT_PSTAMP(p0);
        if (mRes != 0ull) {
            // ---------------- D. walk: the phases of the resident streams (TLAS leaf / NODE / TRI), on the records loaded by the previous trip ----------------
            // what each resident lane is at, from its pool reference: 10 = BVH interior, 00 = leaf triangle (never 0 here), 01 = TLAS interior, 11 = TLAS leaf
            uint64_t mNode, mTlas = 0ull;
            if (KIND == 0) mNode = mRes & __builtin_amdgcn_ballot_w64(cur > R.interior - 1u);
            else { mTlas = mRes & __builtin_amdgcn_ballot_w64(cur >= R.tlasLeaf); mNode = mRes & __builtin_amdgcn_ballot_w64(cur - R.tlasBit < R.interior); }
            const uint64_t mTri = mRes & ~(mNode | mTlas);
            // The record loads issued at the end of the previous trip are first needed here.  Naming all four tuples in one
            // empty asm keeps the register allocator from splitting a loaded tuple across the back-edge.
            asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3));
            CRT_DENS(22, __popcll(mRes));
            if (mNode) { CRT_DENS(1, 1); CRT_DENS(2, __popcll(mNode)); }

            if (KIND == 1 && mTlas) { CRT_DENS(23, 1); CRT_DENS(24, __popcll(mTlas)); }
            uint64_t mBack = 0ull;                                                 // lanes that popped the return marker: BLAS finished, back to the TLAS level
            if (KIND == 1 && mTlas != 0ull) {
                if (lane_in(mTlas)) {
                    // ---------------- TLAS leaf (infra/tlas_bvh.cpp:91-95) -> enter the BLAS (BLASBVH::Intersect, blas_bvh.cpp:376-381) ----------
                    if (COUNT) { cn.tlas++; cn.visits++; }
                    const f3 O = mk3(stf[F_OX * S + sid], stf[F_OY * S + sid], stf[F_OZ * S + sid]);
                    const f3 D = mk3(stf[F_DX * S + sid], stf[F_DY * S + sid], stf[F_DZ * S + sid]);
                    to_object_space(q0, q1, q2, O, D, tO, tD, trD);
                    spB += kLevelB; stk_put(spB, R.ret);
                    const uint32_t next = asu(q3.y);                                 // Instance::rootRef16
                    if (COUNT && (next & R.tagMask) == 0u && next != kRefDone) cn.leaf++;
                    cur = next;
                }
                mFinite = (mFinite & ~mTlas) | (mTlas & short_slab_mask(trD, h.t));
            }
            uint64_t mLeafNow = 0ull;                                              // lanes that reached a leaf in an earlier step of this trip and have its first triangle loaded
            auto node_phase = [&](auto exactTag) {
                if (mNode != 0ull) node_step(exactTag, mNode);
#if CRT_POOL_NODE_STEPS > 1
                // ---------------- further NODE steps in the same trip (while-while): the fixed part of a trip — swap out / in, queue bookkeeping, the pass decision — is
                // paid once for several node steps of the lanes that stay at interior nodes.  The lanes that just stepped fetch their next record now (an interior pair, or
                // the first triangle of a leaf, which then joins THIS trip's TRI phase); everyone else keeps the record the previous trip loaded.
#pragma unroll
                for (int rep = 1; rep < CRT_POOL_NODE_STEPS; rep++) {
                    const uint64_t mStepped = rep == 1 ? mNode : mNode2;
                    mNode2 = mStepped & (KIND == 0 ? __builtin_amdgcn_ballot_w64(cur > R.interior - 1u) : __builtin_amdgcn_ballot_w64(cur - R.tlasBit < R.interior));
                    if (pop32(mNode2) < (uint32_t)CRT_POOL_NODE2_MIN) { mNode2 = 0ull; break; }
                    const uint64_t mLeaf = mStepped & __builtin_amdgcn_ballot_w64((cur & R.tagMask) == 0u) & ~__builtin_amdgcn_ballot_w64(cur == kRefDone);
                    load_records(mNode2 | mLeaf);
                    mLeafNow |= mLeaf;
                    CRT_DENS(28, 1); CRT_DENS(29, __popcll(mNode2));
                    node_step(exactTag, mNode2);
                }
#endif
            };
            if (mNode != 0ull) {
                // two `if`s, not if / else: an else arm holding divergent regions comes back as a second, dead branch on a saved flag
                uint64_t mInf = mNode & ~mFinite, mInf2 = mInf;
                asm("" : "+s"(mInf2));
                if (__builtin_expect(mInf == 0ull, 1)) node_phase(std::false_type{});
                if (__builtin_expect(mInf2 != 0ull, 0)) node_phase(std::true_type{});
            }
            const uint64_t mTriAll = mTri | mLeafNow;
            if (mTriAll != 0ull) tri_step(mTriAll);
            if (KIND == 1) {
                // a popped return marker: the BLAS is finished — back to the world-space ray, pop the TLAS entry below (rare: once per BLAS visit)
                mBack = (mNode | mTriAll) & __builtin_amdgcn_ballot_w64(cur == R.ret);
                if (mBack != 0ull) {
                    if (lane_in(mBack)) {
                        world_ray();
                        const bool pop = spB != laneB;
                        const uint32_t top = stk_top(spB);
                        cur = pop ? top : kRefDone; spB -= pop ? kLevelB : 0u;
                        if (COUNT && (cur & R.tagMask) == 0u && cur != kRefDone) cn.leaf++;
                    }
                    mFinite = (mFinite & ~mBack) | (mBack & short_slab_mask(trD, h.t));
                }
            }
            asm volatile("" ::: "memory");          // (the sections exchange stream state through LDS across lanes: nothing is carried over in registers)
            // ---------------- A. swap out: streams whose walk is over park their hit and queue for shading ------------------------------
            const uint64_t mFin = mRes & __builtin_amdgcn_ballot_w64(cur == kRefDone);
            if (mFin != 0ull) {
                CRT_DENS(5, 1); CRT_DENS(6, __popcll(mFin));
                const uint32_t depth = (metaLo >> kMetaDepthShift) & 7u;
                const uint64_t mStop = __builtin_amdgcn_ballot_w64((uint32_t)(h.objIdx + 1) <= 1u) | __builtin_amdgcn_ballot_w64((int)depth >= sc.depthLimit);   // miss, light, or depth limit
                const uint64_t mE = mFin & mStop, mB = mFin & ~mStop;
                if (lane_in(mFin)) {
                    stf[F_T * S + sid] = h.t; stf[F_U * S + sid] = h.u; stf[F_V * S + sid] = h.v;
                    st[F_TRI * S + sid] = (uint32_t)h.triIdx;
                    st[F_META * S + sid] = metaLo | ((uint32_t)(h.objIdx + 1) << kMetaObjShift);
                }
                if (lane_in(mE)) qEnd[(endT + rank_in(mE)) & kQueueMask] = (uint8_t)sid;
                if (lane_in(mB)) qBnc[(bncT + rank_in(mB)) & kQueueMask] = (uint8_t)sid;
                endT += (uint32_t)__popcll(mE); bncT += (uint32_t)__popcll(mB);
                mRes &= ~mFin;
            }
            asm volatile("" ::: "memory");
        }
        CRT_PSTAMP(p1); CRT_PACC(0, p0, p1);
        if (COUNT) trips++;
        CRT_DENS(0, 1); CRT_DENS(30, tcls == kTileFloor);
#ifdef CRT_POOL_STAMPS
        pst[9]++;
#endif
#ifdef CRT_POOL_DENS
        dens[32u + CRT_LIVE_BUCKET(live)]++;
#endif
        // ---------------- C. swap in: free lanes take the next READY streams; E. the record loads (consumed by the next trip's walk) ----
        {
            const uint32_t nRdy = rdyT - rdyH;
            const uint64_t mFree = ~mRes;
            if (nRdy != 0u) if (ctl_free(mRes)) {
                const uint32_t myRank = rank_in(mFree);
                const uint64_t mTake = mFree & __builtin_amdgcn_ballot_w64(myRank < nRdy);      // the first min(nRdy, free) free lanes
                CRT_DENS(7, 1); CRT_DENS(8, __popcll(mTake));
                if (lane_in(mTake)) {
                    sid = qRdy[(rdyH + myRank) & kQueueMask];
                    tO = mk3(stf[F_OX * S + sid], stf[F_OY * S + sid], stf[F_OZ * S + sid]);
                    tD = mk3(stf[F_DX * S + sid], stf[F_DY * S + sid], stf[F_DZ * S + sid]);
                    trD = mk3(stf[F_RX * S + sid], stf[F_RY * S + sid], stf[F_RZ * S + sid]);
                    const uint32_t meta = st[F_META * S + sid];
                    h.t = stf[F_T * S + sid]; h.objIdx = (int)(meta >> kMetaObjShift) - 1; h.u = 0; h.v = 0; h.triIdx = -1;
                    metaLo = meta & kMetaLowMask;
                    cur = st[F_CUR * S + sid];
                    const uint32_t pend = st[F_PEND * S + sid];
                    stk_put(laneB + kLevelB, pend);                                     // a dead store unless the far root child was hit
                    spB = laneB + (pend ? kLevelB : 0u);
                }
                mFinite = (mFinite & ~mTake) | (mTake & short_slab_mask(trD, h.t));
                mRes |= mTake;
                rdyH += (uint32_t)__popcll(mTake);
            }
            if (mRes != 0ull) {
                CRT_DENS(21, 1);
                uint32_t oa = record_offset();
                if (!lane_in(mRes)) oa = 0u;                                         // lanes without a stream re-read record 0
                q0 = ldp<0>(geom, oa); q1 = ldp<1>(geom, oa); q2 = ldp<2>(geom, oa); q3 = ldp<3>(geom, oa);
            }
        }
        asm volatile("" ::: "memory");
        // ---------------- B. shading passes (their latency-free arithmetic also covers the record loads just issued) --------------------
        const uint32_t nEnd = endT - endH, nBnc = bncT - bncH;
        // a shading pass waits for a full wavefront of streams unless the walking side runs dry
        // "A queue is full, or the wave is starving" is ONE scalar compare in front of ONE branch round both passes: the walking side's population, replaced by 0 when
        // a queue is full (64 is a power of two: either count >= 64 <=> the OR is), against the starving threshold.  No pass due — the common case — costs ten scalar
        // instructions, the branch included.  (The loop holds divergent regions, so the compiler structurises it as a whole, and every further early way out of this
        // section — nested tests, a `continue` — comes back as a saved 64-bit flag and a second branch.)
        uint32_t walking = pop32(mRes) + (rdyT - rdyH), fullest = nEnd | nBnc;
        asm("" : "+s"(walking));                                                  // (a select of two values at hand, not a branch round the sum)
        walking = fullest >= 64u ? 0u : walking;
        asm("" : "+s"(walking), "+s"(fullest));                                   // (and inside, the rare side, a compare of its own: no flag kept from this one)
        if (walking < (uint32_t)CRT_POOL_STARVE) {
            // Which pass, as one 32-bit word: runEnd = its low byte, runBnc = the bits above.  A full queue runs its pass (rings hold <= 128, so n >> 6 != 0 <=> n >= 64),
            // and then the starving arms add nothing: the queue that is not full is the shorter one.  Otherwise the starving wave runs the longer queue's pass, END on a
            // tie, none when both are empty (nEnd < 64 fits the byte).
            const uint32_t run = fullest >= 64u ? (nEnd >> 6) | ((nBnc >> 6) << 8) : (nEnd >= nBnc ? nEnd : nBnc << 8);
            const uint32_t runEnd = run & 0xffu, runBnc = run >> 8;

            CRT_PSTAMP(p2b); CRT_PACC(1, p1, p2b);
            if (runEnd != 0u) {
                // ---------------- B1. END pass: the path of each stream ended (renderer.cpp:54-55, 69) or has not begun ----------------
                const uint32_t n = nEnd < 64u ? nEnd : 64u;
                const uint64_t mActE = mask_ult(lane, n);
                const bool act = lane_in(mActE);
                const uint32_t s = act ? qEnd[(endH + lane) & kQueueMask] : 0u;
                endH += n;
                uint32_t meta = 0, seed = 0; int obj = -1; f3 D = nil3;
                if (act) { meta = st[F_META * S + s]; seed = st[F_SEED * S + s]; obj = (int)(meta >> kMetaObjShift) - 1; D = mk3(stf[F_DX * S + s], stf[F_DY * S + s], stf[F_DZ * S + s]); }
                const int depth = (int)((meta >> kMetaDepthShift) & 7u);
                uint32_t item = meta & kMetaItemMask;
                // the pass's lane sets as scalar masks (meta is 0 on a lane without a stream: neither fresh nor a hit)
                const uint64_t mFirst = mask_ne(meta & kMetaFresh, 0u), mEnded = mActE & ~mFirst, mMiss = mEnded & mask_eq(meta >> kMetaObjShift, 0u);
                const bool first = lane_in(mFirst), ended = lane_in(mEnded), miss = lane_in(mMiss);
#ifdef CRT_POOL_DENS
                dens[36u + CRT_LIVE_BUCKET(live)]++;
#endif
                CRT_DENS(9, 1); CRT_DENS(31, tcls == kTileFloor); CRT_DENS(10, n); CRT_DENS_MASK(11, miss); CRT_DENS_MASK(13, act && first); CRT_DENS_MASK(25, ended && depth > 0); CRT_DENS_MASK(26, ended && depth > 1); CRT_DENS_MASK(27, ended && depth > 2);
                if (ended && obj >= 2) cn.meshhits++;
                // the path's throughput factors: fetched now, needed after the sky lookup.  They were written by this wavefront's BOUNCE passes, possibly from another
                // lane, and by nobody else: a workgroup is this one wavefront and the rows are the block's own.  So the accesses are relaxed atomics of WORKGROUP scope:
                // LLVM's gfx942 / gfx950 memory model asks for no cache bypass at that scope, because all lanes of a workgroup go through one vector L1 — which holds as
                // long as the kernel is not built for threadgroup-split mode, and it is not.  (At agent scope every one of these loads and stores carries sc1 and goes
                // past the L2 of its XCD.)
                // Level k + 1 is fetched inside level k's region (depth > k + 1 implies depth > k): most paths end at depth 0..2, and the first level no lane reaches
                // skips all the deeper ones with one branch.  "Not a sky tile" is asked once, round the nest (a sky tile's paths all end at depth 0: no factor was ever
                // written, the fetch and the unwind below are skipped as a whole).  The 15 registers start as whatever they hold — a definition without an instruction:
                // a lane reads a level in the unwind only where it loaded it here.
                float fk[15];
                asm("" : "=v"(fk[0]), "=v"(fk[1]), "=v"(fk[2]), "=v"(fk[3]), "=v"(fk[4]), "=v"(fk[5]), "=v"(fk[6]), "=v"(fk[7]), "=v"(fk[8]), "=v"(fk[9]), "=v"(fk[10]), "=v"(fk[11]), "=v"(fk[12]), "=v"(fk[13]), "=v"(fk[14]));
                auto fetch_level = [&](int k) {
#pragma unroll
                    for (int j = 0; j < 3; j++) fk[3 * k + j] = __hip_atomic_load(fac + (3 * k + j) * S + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                };
                if (not_sky()) {
                    if (ended && depth > 0) { fetch_level(0);
                        if (depth > 1) { fetch_level(1);
                            if (depth > 2) { fetch_level(2);
                                if (depth > 3) { fetch_level(3);
                                    if (depth > 4) fetch_level(4); } } } }
                }
                // GetSkyColor (file_scene.cpp:142-154): the texel fetch is issued here and consumed after the next ray has been set up — the skydome is far
                // larger than the caches, and the (long) latency of this one load is then covered by the arithmetic of ray generation and new_ray
                uint32_t skyTexel = 0u;
                if (miss) {
                    float phi, theta; sky_angles(D, phi, theta);
                    const kernarg_f sk = scene_floats(offsetof(Scene, skyOffset));   // skyOffset, skyW, skyH
                    skyTexel = sc.texels[tex_index(asu(sk[0]), (int)asu(sk[1]), (int)asu(sk[2]), phi * CRT_INV2PI, theta * CRT_INVPI)];
                }
                bool gen = act && first;
                size_t sampleAt = 0;
                if (ended) {
                    uint32_t pix = item, pass = 0;
                    if (fresh(passes) != 1u) { pix = item / passes; pass = item - pix * passes; }
                    const uint32_t fr = frame0 + (S > 64 ? (uint32_t)slotFrame[s] : s);   // frame of the launch -> (64-frame window, sample row position)
                    sampleAt = slab_position(fr, tileCount, tl, pix, rowLen, passes, pass);
                    item++;
                    gen = item < items;                                            // else: the stream has rendered its 256 pixels
                }
                // REFILL: the slots whose stream has just rendered its last pixel take the range's next frames (none left: the slot stays empty and the population
                // falls).  The finished path's sample position is computed above, from the old frame; its radiance is stored below as for every ended path.
                // (the set of lanes that generate a ray is one mask: the fresh streams, the ended ones with pixels left — `item` was stepped on those lanes only —
                // and, below, the refilled slots.  A stream renders its last pixel once per 256 paths, so the test of mDone skips all of it nearly always.)
                uint64_t mGen = mFirst | (mEnded & mask_ult(item, items));
                const uint64_t mDone = mEnded & ~mGen;
                if (mDone != 0ull) {
                    uint64_t mTake = 0ull;
                    if (S > 64) if (nextFrame < nOwn) {
                        const uint32_t f = nextFrame + rank_in(mDone);
                        mTake = mDone & mask_ult(f, nOwn);
                        if (lane_in(mTake)) {
                            slotFrame[s] = (uint16_t)f;
                            seed = stream_seed(tx, ty, (uint32_t)sc.W, sppFirst, frame0 + f, passes);   // as at the wave's start
                            item = 0u;
                        }
                        nextFrame += pop32(mTake);
                        mGen |= mTake;
                    }
                    nLive -= pop32(mDone & ~mTake);
                }
                gen = lane_in(mGen);
#ifdef CRT_POOL_DENS
                {
                    const uint32_t gone = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ended) & ~__builtin_amdgcn_ballot_w64(gen));
                    if (gone) { const unsigned long long now = wall_clock64(); dens[44u + CRT_LIVE_BUCKET(live)] += (uint32_t)(now - liveClk); liveClk = now; live -= gone; }
                }
#endif
                // the camera (camPos, topLeft, topRight, bottomLeft: 12 floats of the Scene block) is read here, not held in registers across the loop
                const kernarg_f cam = scene_floats(offsetof(Scene, camPos));
                const f3 camPos = mk3(cam[0], cam[1], cam[2]);
                f3 v = camPos;
                if (gen) {                                                         // ProcessTile + Camera::GetPrimaryRay (renderer.cpp:125-126, camera.h:23-30)
                    const uint32_t pix = (fresh(passes) == 1u) ? item : item / passes;
                    const f3 TL = mk3(cam[3], cam[4], cam[5]);
                    constexpr size_t pc = (offsetof(Scene, primRight) - offsetof(Scene, camPos)) / 4;   // primRight[3], primDown[3]: TR - TL and BL - TL, formed on the host
                    const f3 right = mk3(cam[pc], cam[pc + 1], cam[pc + 2]), down = mk3(cam[pc + 3], cam[pc + 4], cam[pc + 5]);
                    v = primary_target(camPos, TL, right, down, cam[12], cam[13], tx, ty, pix, seed);   // invW, invH follow the camera in the Scene block
                    cn.primary++;
                }
                CRT_DENS_MASK(12, gen);
                CRT_PSTAMP(e1); CRT_PACC(2, p2b, e1);
                // (two `if`s on one scalar, not if / else: as at the walk's node_phase)
                if (fresh(tcls) != kTileFloor) new_ray(std::true_type{}, mGen, s, v, true, camPos, seed, item);   // depth 0, outside, not fresh
                if (fresh(tcls) == kTileFloor) floor_ray(mGen, s, v, camPos, seed, item);
                CRT_PSTAMP(e2); CRT_PACC(3, e1, e2);
                if (ended) {
                    // the finished path's radiance: sky colour / light (24,24,22) / 0 at the depth limit (renderer.cpp:54-55, 69; GetLightColor file_scene.cpp:164-167), times the
                    // throughput factors in recursion order (innermost first: albedo*medium*Sample(...) multiplies on return)
                    f3 L = miss ? tex_unpack(skyTexel) : ((depth >= sc.depthLimit) ? mk3(0, 0, 0) : mk3(24, 24, 22));
                    // (nested as the fetch is: a lane at depth d multiplies by the factors d - 1 ... 0, in that order, and the first level no lane reaches skips the deeper ones)
                    auto fk3 = [&](int k) -> f3 { return mk3(fk[3 * k], fk[3 * k + 1], fk[3 * k + 2]); };
                    if (not_sky()) {
                        if (depth > 0) {
                            if (depth > 1) {
                                if (depth > 2) {
                                    if (depth > 3) {
                                        if (depth > 4) L = fk3(4) * L;
                                        L = fk3(3) * L; }
                                    L = fk3(2) * L; }
                                L = fk3(1) * L; }
                            L = fk3(0) * L; }
                    }
                    store_sample(slab, sampleAt, L);
                }
                // every load of this pass is named as consumed here, at its end, on every path: the registers they wrote are re-used by the next sections, and a load
                // the compiler cannot prove finished would put a wait for ALL outstanding loads — the record loads in flight included — in front of that first re-use
#ifdef CRT_POOL_STAMPS
                { CRT_PSTAMP(e3); CRT_PACC(4, e2, e3); pst[10]++; }
#endif
                asm volatile("" :: "v"(fk[0]), "v"(fk[1]), "v"(fk[2]), "v"(fk[3]), "v"(fk[4]), "v"(fk[5]), "v"(fk[6]), "v"(fk[7]), "v"(fk[8]), "v"(fk[9]), "v"(fk[10]), "v"(fk[11]), "v"(fk[12]), "v"(fk[13]), "v"(fk[14]), "v"(skyTexel));
            }
            CRT_PSTAMP(p3);
            asm volatile("" ::: "memory");
            if (runBnc != 0u) {
                // ---------------- B2. BOUNCE pass: surface hit (floor or mesh) below the depth limit (renderer.cpp:56-99) ----------------
                const uint32_t n = nBnc < 64u ? nBnc : 64u;
                const uint64_t mActB = mask_ult(lane, n);
                const bool act = lane_in(mActB);
                const uint32_t s = act ? qBnc[(bncH + lane) & kQueueMask] : 0u;
                bncH += n;
                f3 O = nil3, D = nil3; float ht = 0, hu = 0, hv = 0; int obj = 1; uint32_t tri = 0, seed = 0, meta = 0;
                if (act) {
                    tri = st[F_TRI * S + s];
                    O = mk3(stf[F_OX * S + s], stf[F_OY * S + s], stf[F_OZ * S + s]);
                    D = mk3(stf[F_DX * S + s], stf[F_DY * S + s], stf[F_DZ * S + s]);
                    ht = stf[F_T * S + s]; hu = stf[F_U * S + s]; hv = stf[F_V * S + s];
                    seed = st[F_SEED * S + s]; meta = st[F_META * S + s]; obj = (int)(meta >> kMetaObjShift) - 1;
                }
                const bool mesh = act && obj >= 2;
#ifdef CRT_POOL_DENS
                dens[40u + CRT_LIVE_BUCKET(live)]++;
#endif
                CRT_DENS(14, 1); CRT_DENS(31, tcls == kTileFloor); CRT_DENS(15, n); CRT_DENS_MASK(16, mesh);
                rec4 s0 = {0, 0, 0, 0}, s1 = s0, s2 = s0, s3 = s0;                 // the hit triangle's ShadeTri
                if (mesh) { const uint32_t so = sc.shadeOff + tri * 64u; s0 = ldp<0>(geom, so); s1 = ldp<1>(geom, so); s2 = ldp<2>(geom, so); s3 = ldp<3>(geom, so); cn.meshhits++; }
                const bool inside = (meta & kMetaInside) != 0u;
                const int depth = (int)((meta >> kMetaDepthShift) & 7u);
                const uint32_t item = meta & kMetaItemMask;
                f3 v = O; bool newInside = false;
                if (act) {
                    const f3 I = O + ht * D;
                    SurfPoint p;
                    if (obj == 1) {
                        const kernarg_f fl = scene_floats(offsetof(Scene, floorN));      // floorN[3], floorD, floorInvto
                        const kernarg_f fm = scene_floats(offsetof(Scene, floorMat));    // Material: reflectivity, refractivity, absorption[3], texOffset, texW, texH
                        const rec4 m0 = {fm[0], fm[1], fm[2], fm[3]}, m1 = {fm[4], fm[5], fm[6], fm[7]};
                        p = floor_point(mk3(fl[0], fl[1], fl[2]), fl[4], m0, m1, I);
                    } else p = mesh_point<KIND>(s0, s1, s2, s3, hu, hv, obj, geom, sc.instOff, sc.mats);
                    const f3 N = face_ray(p.N, D);
                    // Material::GetAlbedo: the texel fetch is issued here and consumed after the direction has been drawn (its latency hides behind the rejection loop)
                    uint32_t texel = 0x00ffffffu;
                    if (p.tW > 0) texel = sc.texels[tex_index(p.tOff, p.tW, p.tH, p.tu, p.tv)];
                    const f3 medium = medium_of(inside, p.absorb, ht);
                    CRT_PSTAMP(b1); CRT_PACC(5, p3, b1);
                    const Bounce b = draw_bounce(seed, D, N, inside, p.refl, p.refr);
                    newInside = b.newInside;
                    // albedo (1,1,1 untextured: 0xffffff * (1/255) == 1 exactly)
                    const f3 c = (p.tW > 0) ? tex_unpack(texel) : mk3(1.0f, 1.0f, 1.0f);
                    CRT_PSTAMP(b2); CRT_PACC(6, b1, b2);
                    // normalize(R) of the diffuse branch; the bounce's throughput factor and the new origin use the normalised direction
                    const float inv = rcp_exact(sqrt_exact(dot3(b.v, b.v)));
                    const f3 nv = b.branch == kDiffuse ? b.v * inv : b.v;
                    v = nv;
                    const f3 factor = bounce_factor(b.branch, c, medium, nv, N);
                    float* fd = fac + (3 * depth) * S + s;                         // depth <= 4 here; workgroup scope: read back by this wavefront alone (the END pass's fetch)
                    __hip_atomic_store(fd, factor.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(fd + S, factor.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(fd + 2 * S, factor.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    O = I + nv * CRT_EPS;
                    CRT_PSTAMP(b3); CRT_PACC(7, b2, b3);
                }
                CRT_PSTAMP(b4);
                new_ray(std::false_type{}, mActB, s, v, false, O, seed, item | ((uint32_t)(depth + 1) << kMetaDepthShift) | (newInside ? kMetaInside : 0u));
#ifdef CRT_POOL_STAMPS
                { CRT_PSTAMP(b5); CRT_PACC(8, b4, b5); pst[11]++; }
#endif
                asm volatile("" :: "v"(s0), "v"(s1), "v"(s2), "v"(s3));            // (as at the end of the END pass)
            }
        }
        if (nLive == 0u) break;                                                   // every stream has rendered its 256 pixels
    }
#ifdef CRT_POOL_STAMPS
    if (lane == 0) for (int i = 0; i < 12; i++) atomicAdd(&g_poolStamps[i], pst[i]);
#endif
#ifdef CRT_POOL_DENS
    dens[44u + CRT_LIVE_BUCKET(live)] += (uint32_t)(wall_clock64() - liveClk);
    if (lane == 0) for (int i = 0; i < 48; i++) if (dens[i]) atomicAdd(&g_poolDens[i], (unsigned long long)dens[i]);
#endif

#ifdef CRT_POOL_TIMELINE
    if (lane == 0 && g_poolTimeline) { uint32_t hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw)); g_poolTimeline[3 * (size_t)blockIdx.x] = tl0; g_poolTimeline[3 * (size_t)blockIdx.x + 1] = wall_clock64(); g_poolTimeline[3 * (size_t)blockIdx.x + 2] = hw; }
#endif
    // what this tile costs (100 MHz ticks): this wavefront's duration per 64 streams (close to what the tile's one-stream-per-lane wavefront takes on an idle chip);
    // wavefronts of exactly S frames only — one with fewer runs them less densely, one with more (refill) more densely.  The host orders and plans later jobs with it (abi.cpp plan_job).
    if (tileCost && lane == 0 && nOwn == (uint32_t)S) atomicMax(&tileCost[tl], (uint32_t)((wall_clock64() - clk0) * 64ull / (uint32_t)S));
    // ... and how much of this wavefront ran after the launch's last wavefront had started (the launch's drain: abi.cpp adopt_job_costs)
    if (launchClk && lane == 0) { const unsigned long long now = wall_clock64(), last = __hip_atomic_load(&launchClk[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), from = last > clk0 ? last : clk0; if (now > from) atomicAdd(&launchClk[2], now - from); }
    if (COUNT && tileClocks && lane == 0 && nOwn == frames) {                   // instrumentation: per-tile wall time + loop trips (one wavefront per tile only)
        tileClocks[2 * tl] = wall_clock64() - clk0;        // 100 MHz constant clock
        tileClocks[2 * tl + 1] = trips;
    }
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (!COUNT && i >= 2 && i != 7) continue;
        uint32_t sum = wave_sum(vals[i]);
        if (lane == 0 && sum) atomicAdd(&counters->v[i], (unsigned long long)sum);
    }
}

} // namespace crt

// streams per wavefront: 128 for jobs of >= 128 frames, 64 (streams = lanes) for shorter ones
#ifndef CRT_POOL_STREAMS
#define CRT_POOL_STREAMS 128
#endif
extern "C" uint32_t crt_pool_streams(uint32_t frames) { return frames > 64u ? (uint32_t)CRT_POOL_STREAMS : 64u; }
// LDS of one wavefront: traversal stacks ((stackDepth + 1 dummy) entries of refBits / 8 bytes per lane) + parked stream state + the three one-byte ring queues
// + (more slots than lanes: wavefronts that may refill) the two-byte frame of every slot.  128 slots, 16-bit references, at a stack depth of <= 17: <= 10 240 bytes,
// 16 wavefronts per CU; 32-bit references add (stackDepth + 1) * 128 bytes.
extern "C" uint32_t crt_pool_lds_bytes(uint32_t stackDepth, uint32_t streams, uint32_t refBits) { return (stackDepth + 1u) * 64u * (refBits / 8u) + crt::F_COUNT * streams * 4u + 3u * 128u + (streams > 64u ? 2u * streams : 0u); }
// the most LDS a pool wavefront may ask for: what the device grants one workgroup, and never more than the 64 KiB that bound the other render kernels' stacks (abi.cpp)
extern "C" uint32_t crt_pool_lds_limit(int device)
{
    static uint32_t known[64] = {};                                             // asked once per device (the launch wrapper checks every launch against it)
    if (device >= 0 && device < 64 && known[device]) return known[device];
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || v <= 0) { (void)hipGetLastError(); return 0u; }
    const uint32_t limit = (uint32_t)v < 64u * 1024u ? (uint32_t)v : 64u * 1024u;
    if (device >= 0 && device < 64) known[device] = limit;
    return limit;
}
// bytes of throughput-factor scratch a launch of `windows` 64-frame windows needs behind its sample slab (15 floats per stream; a wave's
// group of streams may reach past the last window, hence 128 stream slots per window)
extern "C" size_t crt_pool_scratch_bytes_per_window(uint32_t tileCount) { return (size_t)tileCount * 128u * 15u * 4u; }

#ifdef CRT_POOL_STAMPS
extern "C" int crt_debug_pool_stamps(unsigned long long* out, int reset)       // after a sync: the section clocks summed over every pool wave since the last reset
{
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(crt::g_poolStamps), 128) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(crt::g_poolStamps), z, 128) != hipSuccess) return -1; }
    return 0;
}
#endif
#ifdef CRT_POOL_DENS
extern "C" int crt_debug_pool_density(unsigned long long* out, int reset)      // after a sync: the 48 section counters summed over every pool wave since the last reset
{
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(crt::g_poolDens), 384) != hipSuccess) return -1;
    if (reset) { unsigned long long z[48] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(crt::g_poolDens), z, 384) != hipSuccess) return -1; }
    return 0;
}
#endif
#ifdef CRT_POOL_TIMELINE
static unsigned long long* g_timelineHost = nullptr; static size_t g_timelineCount = 0;
extern "C" size_t crt_debug_pool_timeline(unsigned long long* out, size_t cap)        // after a sync: 3 words per wavefront of the last pool launch
{
    const size_t n = g_timelineCount < cap ? g_timelineCount : cap;
    if (out && n) (void)hipMemcpy(out, g_timelineHost, n * 24, hipMemcpyDeviceToHost);
    return g_timelineCount;
}
#endif
extern "C" hipError_t crt_launch_render_pool(const crt::Scene* sc, void* slab, void* facScratch, crt::Counters* counters, unsigned long long* tileClocks, const uint32_t* tileOrder,
                                             uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst,
                                             uint32_t frames, uint32_t passes, int collectStats, uint32_t rankFirst, uint32_t rankEnd, uint32_t waveFrames, const uint32_t* waveTab, uint32_t tabBlocks, uint32_t longFrames,
                                             uint32_t* tileCost, unsigned long long* launchClk, const uint8_t* tileClass, uint32_t extraLds, hipStream_t stream)
{
    if (tileCount == 0 || frames == 0) return hipSuccess;
    if (sc->poolRefBits != 16u && sc->poolRefBits != 32u) return hipErrorInvalidValue;   // a scene without pool references: the host launches render_tiles_kernel
    const uint32_t S = crt_pool_streams(frames);
    // frames per wavefront: S (waveFrames == 0), or a multiple of S, at most 0xff80 (the slots' 16-bit frames) — one for all tiles; or per rank from waveTab for the
    // frames [0, longFrames) (tabBlocks wavefronts in all) and S for the rest
    const uint32_t wf = (S == 64u || waveFrames < S) ? S : waveFrames;
    if (wf % S != 0u || wf > 0xff80u) return hipErrorInvalidValue;
    if (S == 64u) waveTab = nullptr;
    if (waveTab && (tabBlocks == 0u || longFrames == 0u || longFrames > frames)) return hipErrorInvalidValue;
    const uint32_t groups = waveTab ? (frames - longFrames + S - 1u) / S : (frames + wf - 1u) / wf;
    if ((unsigned long long)tileCount * ((frames + S - 1u) / S) > 0x7fffffffull) return hipErrorInvalidValue;
    // the ranks [rankFirst, rankEnd) of the order: the grid ends with rankEnd's wavefronts (both parts of the launch are rank-major), and a wave table says of
    // the ranks behind them that their first block is tabBlocks — the kernel's search, which runs over all tileCount - rankFirst entries, never lands there
    if (rankEnd > tileCount) return hipErrorInvalidValue;
    if (rankFirst >= rankEnd) return hipSuccess;
    dim3 grid(waveTab ? tabBlocks + (rankEnd - rankFirst) * groups : (rankEnd - rankFirst) * groups), block(64);
#ifdef CRT_POOL_TIMELINE
    { static unsigned long long* buf = nullptr; static size_t cap = 0;
      if (cap < (size_t)grid.x) { if (buf) (void)hipFree(buf); (void)hipMalloc((void**)&buf, (size_t)grid.x * 24); cap = grid.x; (void)hipMemcpyToSymbol(HIP_SYMBOL(crt::g_poolTimeline), &buf, sizeof(buf)); }
      (void)hipMemsetAsync(buf, 0, (size_t)grid.x * 24, stream); g_timelineHost = buf; g_timelineCount = grid.x; }
#endif
    const uint32_t ldsBytes = crt_pool_lds_bytes(sc->stackDepth, S, sc->poolRefBits) + extraLds;
    { int dev = 0; if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError(); if (ldsBytes > crt_pool_lds_limit(dev)) return hipErrorInvalidValue; }   // (the host routes such a scene to render_tiles_kernel)
#define CRT_LAUNCH(K, C, SS) do { if (sc->poolRefBits == 32u) CRT_LAUNCH_R(K, C, SS, 32); else CRT_LAUNCH_R(K, C, SS, 16); } while (0)
#define CRT_LAUNCH_R(K, C, SS, RB) hipLaunchKernelGGL((crt::render_pool_kernel<K, C, SS, RB>), grid, block, ldsBytes, stream, *sc, (char*)slab, (float*)facScratch, counters, tileClocks, tileOrder, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, groups, wf, waveTab, tabBlocks, longFrames, rankFirst, tileCost, launchClk, tileClass)
#define CRT_LAUNCH_S(K, C) do { if (S == 64u) CRT_LAUNCH(K, C, 64); else CRT_LAUNCH(K, C, CRT_POOL_STREAMS); } while (0)
    if (sc->kind == 0) { if (collectStats) CRT_LAUNCH_S(0, true); else CRT_LAUNCH_S(0, false); }
    else { if (collectStats) CRT_LAUNCH_S(1, true); else CRT_LAUNCH_S(1, false); }
#undef CRT_LAUNCH_S
#undef CRT_LAUNCH
#undef CRT_LAUNCH_R
    return hipGetLastError();
}
