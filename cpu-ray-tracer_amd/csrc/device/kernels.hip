// kernels.hip — hand-written gfx950 (CDNA4) kernels of the path-tracing hot path.
//
//   render_tiles_kernel   one 64-lane wavefront per (16x16 image tile, 64-frame window); lane f owns the RNG stream of frame f
//                         of that tile (the reference seeds one xorshift32 stream per (tile, frame) and consumes it serially
//                         over the tile's 256 pixels — "3. PathTracer/renderer.cpp":117-131).  One grid covers every window
//                         of a crt_render job, expensive tiles first.  The wave is a small wavefront pipeline of its own:
//                         every lane is a state machine {needs shading / ray-gen, at a TLAS node, at a BVH interior node, at
//                         a leaf triangle}, and each trip of the wave's loop runs the phases that have lanes waiting
//                         (ballot population counts).  Lanes never wait for the longest ray of the wave: a lane whose path
//                         ends regenerates its next pixel's primary ray and re-enters traversal while its neighbours keep
//                         walking.  Traversal stacks and the paths' throughput factors are per-lane columns in LDS.
//                         Finished paths write their radiance sample to the sample slab in HBM.
//   accumulate_kernel     adds the slab's samples to the float4 accumulator in (window, frame, pass) order (bit-exact with the
//                         reference's `accumulator[..] +=` order, renderer.cpp:124), streaming the slab at HBM rate — no float
//                         atomics anywhere.
//   find_nearest_kernel   scene.FindNearest for a ray buffer (parity / query entry).
//   whitted_kernel        the Whitted-style integrator ("2. WhittedStyle/renderer.cpp":21-157), one thread per pixel.
//   trace_query_kernel    the same integrator's Trace for a caller's ray array, persistent and cursor-fed (trace_query.h; the body of both: trace_body.h).
//   inspect_primary_kernel / inspect_color_kernel   the Whitted renderer's traversal / intersection heat maps and per-Tick metrics
//                         (renderer.cpp:38-39, 147-152): primary rays' counts + metrics, then exclusive prefix maximum + colour.
//   resolve_kernel        screen pixels + per-tile energy sums (renderer.cpp:119,127-129).
//   commit_frame_kernel   crt_tick: one rendered-ahead frame's samples into the accumulator + the screen, in one pass.
//
// Numerics: compiled with -ffp-contract=off; only IEEE + - * / sqrt, so results are bit-identical with a scalar
// CPU evaluation of the same expressions.  min/max follow the reference's std::min/std::max operand order.
// No MFMA: the path is pointer chasing + slab / Möller–Trumbore tests.
// render_tiles_kernel's Sample body — the surface of a hit, medium, the bounce and its factor, the primary ray, the return path, the light / floor operands, the
// ordered two-child step — and whitted_kernel's surface are sample_body.h's: the functions render_pool_kernel and the sequential kernels shade with, not a copy.
// One repeat stays written out in render_tiles_kernel: its second NODE step.  The two steps as one local lambda called twice took its latency mode (one render
// of 64 frames) from 20.09 to 20.74 ms, past the parent's 20.29 + 0.07 (profiles/sample_body.json, tiles_kernel_pieces).
#include "alt_common.h"
#include "launch.h"
#include "sample_body.h"
#include "trace_body.h"
#include "trace_query.h"

namespace crt {

// ------------------------------------------------------------------------------------------------------------
// render_tiles_kernel<KIND, COUNT>: grid = (tiles owned by this ctx) x (64-frame windows of the launch), block = one wavefront (lane = frame).
// slab layout (sample_body.h, the 12-byte sample form): [window][tileLocal][pixel 0..255][sample 0..64*passes), sample = frame*passes + pass (a partial
// last window leaves the tail of its rows unused).  Pixel-major: the lanes of a wave are the consecutive samples of a pixel, so lanes that finish the same
// pixel write neighbouring 12-byte pieces of one row and the L2 merges them into whole lines before they leave for HBM; accumulate_kernel
// transposes through LDS on the read side.
//
// Per-lane traversal state is ONE packed reference `cur` (layout.h), the 64-byte record it names — already
// PRE-LOADED into registers q0..q3 by the trip that produced it — and a stack in a per-lane LDS column:
//     cur == 0 (done)      -> SHADE phase: shade the hit with the pre-loaded ShadeTri (or end the path: unwind, write the
//                             sample, generate the next pixel's primary ray), start FindNearest for the new ray (quad,
//                             plane, first traversal step from the root's child pair in the kernel arguments)
//     BVH interior         -> NODE phase: two slab tests on the pre-loaded NodePair, ordered descend / push / pop
//     BVH leaf             -> TRI phase: ONE Möller–Trumbore test on the pre-loaded LeafTri, next triangle or pop
//     TLAS interior        -> NODE phase as well (two-level scenes): its two child TlasNodes are fetched into the NodePair layout
//     TLAS leaf            -> TLAS phase: enter the BLAS through the pre-loaded invT rows (return marker on the stack)
// One trip of the wave's loop = ballot the states, run each phase that has enough lanes (thresholds below: SHADE waits
// for 24 lanes unless nothing else can run, the others run whenever populated), then issue the record loads: four 16-byte loads at
// `geom + 32-bit offset`.  The loads fly while the next trip's ballots and the other phases' arithmetic execute, and a
// lane only ever pays for its own ray's length, never for the longest ray in the wave.
// ------------------------------------------------------------------------------------------------------------
#ifndef CRT_SHADE_BATCH
#define CRT_SHADE_BATCH 24          // lanes the SHADE phase waits for in a launch of few windows (latency matters: its heaviest tile ends it)
#endif
#ifndef CRT_SHADE_BATCH_JOB
#define CRT_SHADE_BATCH_JOB 40      // ... and in a many-window job, where fuller SHADE runs buy throughput (measured: -2.7 % per window, +7 % latency)
#endif
#ifndef CRT_TRI_BATCH
#define CRT_TRI_BATCH 1
#endif
#ifndef CRT_NODE_BATCH
#define CRT_NODE_BATCH 1
#endif

#ifndef CRT_TILES_NODE_STEPS
#define CRT_TILES_NODE_STEPS 2     // NODE steps per trip of the lanes that stay at interior nodes
#endif
#ifndef CRT_MIN_WAVES
#define CRT_MIN_WAVES 5      // waves per SIMD the register budget must allow (<= 96 VGPRs)
#endif
template <int KIND, bool COUNT>
__global__ __launch_bounds__(64, CRT_MIN_WAVES) void render_tiles_kernel(const Scene sc, char* __restrict__ slab,
                                                           Counters* __restrict__ counters, unsigned long long* __restrict__ tileClocks,
                                                           const uint32_t* __restrict__ tileOrder,
                                                           uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                           uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t windows,
                                                           const uint32_t* __restrict__ blockDesc, uint32_t* __restrict__ tileCost, uint32_t rankCount, unsigned long long* __restrict__ launchClk)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const unsigned long long clk0 = (COUNT || tileCost) ? wall_clock64() : 0ull;
    // a job that measures: when did the first and the last wavefront of the launch start (the host derives the launch's machine time from it, abi.cpp adopt_job_costs)
    if (launchClk && lane == 0) { atomicMax(&launchClk[0], ~clk0); atomicMax(&launchClk[1], clk0); }
    // block -> tile.  The kernel's duration is set by its most expensive tiles (one serial RNG stream per lane), so the host
    // lists the tiles whose pixels can see the meshes FIRST (tileOrder): the dispatcher starts them first and they are dealt
    // round-robin over the 8 XCDs / 256 CUs instead of piling up on the XCDs that own the image rows of the model.  The
    // geometry fits every XCD's L2, so nothing is lost by not giving an XCD a contiguous run of tiles (measured: a
    // contiguous-per-XCD mapping is 7-14 % slower).  Speed only; any bijection gives the same image.
    // One launch covers `windows` consecutive 64-frame windows of the progressive render (block = (tile rank, window), rank-major):
    // all windows of the expensive tiles are dispatched first and the cheap tiles fill the machine behind them, so a long job is
    // one grid whose duration is total work / machine throughput instead of a sequence of launches that each end on their
    // heaviest tile.
    // Latency mode (a launch of ONE window with a block table): the launch ends on its most expensive tile — one serial stream per lane, and every
    // trip of that wave pays for all the phases its 64 lanes populate (NODE and TRI nearly always; a lone wave issues one instruction per 6 - 9 cycles
    // whatever its lane count, tools/microbench/lone_wave.hip).  The host therefore measures the tiles (tileCost, below) and gives the expensive ones
    // to SEVERAL wavefronts of fewer lanes each: fewer phases are populated per trip, so each stream's serial chain advances faster, and the idle part of the
    // chip takes the extra wavefronts.  blockDesc[block] = local tile index | first frame << 16 | log2(lanes) << 22 | window << 25; blocks are listed most expensive tile first.  (A job of
    // several windows uses the same table form for its most expensive tiles, abi.cpp build_job_table.)
    uint32_t rank, win = 0u, laneBase = 0u, myLanes = 64u;
    if (blockDesc) { const uint32_t d = blockDesc[blockIdx.x]; rank = d & 0xffffu; laneBase = (d >> 16) & 63u; myLanes = 1u << ((d >> 22) & 7u); win = d >> 25; }
    else { rank = blockIdx.x / windows; win = blockIdx.x - rank * windows; }
    if (rank >= (blockDesc ? tileCount : rankCount)) return;                        // rankCount <= tileCount: only the first tiles of the order (a split job, abi.cpp)
    const uint32_t tl = blockDesc ? rank : (tileOrder ? tileOrder[rank] : rank);       // (a block table names local tile indices itself)
    sppFirst += win * 64u * passes;
    frames = (frames - win * 64u < 64u) ? frames - win * 64u : 64u;               // frames of THIS window (the last one may be partial)
    if (blockDesc) frames = frames > laneBase ? ((frames - laneBase < myLanes) ? frames - laneBase : myLanes) : 0u;
    slab += slab_block_position(win, tileCount, tl, 64u * passes);                 // this tile's block of this window's region of the sample slab
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    uint32_t* stk = lds + lane;
    const char* __restrict__ geom = sc.geom;

    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    uint32_t trips = 0;
    const bool narrowWave = myLanes < 64u;
    const int shadeBatch = narrowWave ? (int)((myLanes * 3u + 7u) / 8u) : (windows >= 8u ? CRT_SHADE_BATCH_JOB : CRT_SHADE_BATCH);   // (24 of 64 lanes, scaled to a narrow wavefront)
#ifdef CRT_STAMPS
    // diagnostic build (-DCRT_STAMPS): shader-clock time per phase of this wave; never compiled into the product
    unsigned long long stT[6] = {0, 0, 0, 0, 0, 0}; uint32_t stN[4] = {0, 0, 0, 0}; uint32_t stL[4] = {0, 0, 0, 0};
#define CRT_STAMP(var) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory")
#else
#define CRT_STAMP(var)
#endif
    const uint32_t items = 256u * passes;                                     // (pixel, pass) pairs in stream order
    const f3 nil3 = mk3(0.0f, 0.0f, 0.0f);                                    // placeholder of values no lane reads (the camera is read where a primary ray is generated)

    bool live = lane < frames;
    uint64_t liveMask = __builtin_amdgcn_ballot_w64(live);                    // lanes whose stream still has pixels to render
    uint32_t seed = init_seed(tx + ty * (uint32_t)sc.W + (sppFirst + (laneBase + lane) * passes) * 1799u);   // renderer.cpp:120
    uint32_t item = 0;
    // world-space ray of the current path segment, its nearest hit so far, path state
    f3 O = nil3, D = nil3, rD = nil3; bool inside = false; int depth = 0;
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    // throughput factors of depths 0..4 (albedo*medium*... of each bounce, multiplied on unwind): written once per bounce and read once
    // per path, so they live in a per-lane LDS column behind the traversal stack (component j of depth k at fst[(3k + j) * 64]) instead
    // of 15 registers — the kernel then fits 5 waves per SIMD — and a bounce stores through a computed address instead of a select chain
    float* fst = reinterpret_cast<float*>(lds + sc.stackDepth * 64u + lane);
    // traversal state; (tO, tD, trD) = ray in the space of the structure being walked (object space inside a BLAS)
    uint32_t cur = kRefDone, sp = 0;
    f3 tO = nil3, tD = nil3, trD = nil3;
    bool rayFinite = true;                                                    // all of trD finite -> v_min/v_max slab test is exact
    bool fresh = true;                                                        // true: SHADE phase must generate a primary ray
    rec4 q0 = {0, 0, 0, 0}, q1 = q0, q2 = q0, q3 = q0;                        // pre-loaded record of `cur`

    // Traversal stack: one LDS column per lane, entry i at stk[i * 64]; `sp` = number of entries.  The hot phases are
    // written branch-free: the current top is read speculatively at the start of a phase (it arrives while the slab /
    // triangle arithmetic runs), a push always stores to slot sp (a dead store when the far child was missed) and
    // only the pointer moves under a select.
#define CRT_TOP() (stk[(sp ? sp - 1u : 0u) * 64u])
    // where the 64-byte record a lane fetches next lies in geom, as two 32-byte halves: the hit's ShadeTri (`shade`: the walk is over) | NodePair / LeafTri of `cur` |
    // TLAS leaf: Instance {invT rows, ids} | TLAS interior: its two child nodes
    auto record_offsets = [&](bool shade, uint32_t& oa, uint32_t& ob) {
        oa = shade ? sc.shadeOff + (uint32_t)h.triIdx * 64u : (cur & kRefOffsetMask) << 4; ob = oa + 32u;
        if (KIND == 1 && !shade && (cur & kRefTlasBit) != 0u) {
            if (cur & kRefInterior) { oa = sc.instOff + (cur & 0xffffu) * 128u; ob = oa + 32u; }
            else { oa = sc.tlasOff + (cur & 0x7fffu) * 32u; ob = sc.tlasOff + ((cur >> 15) & 0x7fffu) * 32u; }
        }
    };
    // two-level scenes: a popped return marker — the BLAS is finished: back to the world-space ray, pop the TLAS entry below
    auto leave_blas = [&](uint32_t next) -> uint32_t {
        if (KIND == 1 && next == kRefReturn) {
            tO = O; tD = D; trD = rD; rayFinite = finite3(rD);
            const bool pop = sp != 0u; const uint32_t top = CRT_TOP();
            next = pop ? top : kRefDone; sp -= pop ? 1u : 0u;
        }
        return next;
    };

    for (;;) {
        // state ballots: the compares write their lane masks straight into scalar registers; `liveMask` (maintained below) removes
        // finished lanes with one scalar AND instead of a per-lane predicate round trip
        const uint64_t mDone = __builtin_amdgcn_ballot_w64(cur == kRefDone) & liveMask;
        // (two-level scenes: a TLAS interior node is walked by the NODE phase too — its two child TlasNodes arrive in q0..q3 in the NodePair
        // layout {lo, ref, hi, -} x 2, and the ordered descend / push / pop is the same code; only TLAS leaves need the TLAS phase)
        const uint64_t mNode = __builtin_amdgcn_ballot_w64(KIND == 1 ? (((cur >> 31) ^ (cur >> 30)) & 1u) != 0u : (cur & 0xC0000000u) == kRefInterior) & liveMask;
        const uint64_t mTri = __builtin_amdgcn_ballot_w64(cur != kRefDone && (cur & 0xC0000000u) == 0u) & liveMask;
        const uint64_t mTlas = (KIND == 1) ? (__builtin_amdgcn_ballot_w64((cur & 0xC0000000u) == kRefTlasLeaf) & liveMask) : 0ull;
        const bool isDone = live && cur == kRefDone;
        const bool isNode = live && (KIND == 1 ? (((cur >> 31) ^ (cur >> 30)) & 1u) != 0u : (cur & 0xC0000000u) == kRefInterior);
        const bool isTri = live && cur != kRefDone && (cur & 0xC0000000u) == 0u;
        const bool isTlas = (KIND == 1) && live && (cur & 0xC0000000u) == kRefTlasLeaf;
        const int nDone = __popcll(mDone), nNode = __popcll(mNode), nTri = __popcll(mTri);
        const int nTlas = (KIND == 1) ? __popcll(mTlas) : 0;
        if (nDone + nNode + nTri + nTlas == 0) break;
        if (COUNT) trips++;
        // a phase runs when enough lanes wait for it; when no phase reaches its batch size the most populated one runs
        const bool bigNode = nNode >= CRT_NODE_BATCH, bigTri = nTri >= CRT_TRI_BATCH, bigShade = nDone >= shadeBatch;
        const bool none = !bigNode && !bigTri && !bigShade && nTlas == 0;
        const bool runTlas = nTlas > 0;
        const bool runNode = bigNode || (none && nNode > 0 && nNode >= nTri && nNode >= nDone);
        const bool runTri = bigTri || (none && nTri > 0 && nTri > nNode && nTri >= nDone);
        const bool runShade = bigShade || (none && nDone > 0 && nDone > nNode && nDone > nTri);
        // The record loads issued at the end of the previous trip are first needed here.  Naming all four tuples in one
        // empty asm keeps the register allocator from splitting a loaded tuple across the back-edge (it otherwise copies one
        // component right behind the loads, which puts a vmcnt wait — the whole fetch latency — at the end of every trip).
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3));
#ifdef CRT_STAMPS
        CRT_STAMP(s0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        CRT_STAMP(s1);
        stT[0] += s1 - s0;
        if (runShade) { stN[0]++; stL[0] += nDone; } if (runNode) { stN[1]++; stL[1] += nNode; } if (runTri) { stN[2]++; stL[2] += nTri; }
        stN[3]++;
#endif

        if (runShade && isDone) {
            // ---------------- SHADE / RAY-GEN phase: one step of Renderer::Sample ("3. PathTracer/renderer.cpp":50-100) ----------
            // Written as a sequence of stages that as many lanes as possible share, instead of one if/else tree per outcome: the
            // sky / floor / mesh texel fetch is ONE site, the direction normalisation of a diffuse bounce and of a new primary ray
            // is ONE site, and the new ray's reciprocal direction, quad / plane tests and root step are ONE site.  Every lane
            // still evaluates exactly the reference's expressions in the reference's order.
            // stage 1: what did FindNearest return (renderer.cpp:52-55, 69)
            // (Scene fields only this phase needs are read from the kernel-argument segment here instead of living in scalar registers across the loop: dev_common.h scene_floats)
            const kernarg_f cam = scene_floats(offsetof(Scene, camPos));          // camPos, topLeft, topRight, bottomLeft, invW, invH
            const f3 camPos = mk3(cam[0], cam[1], cam[2]);
            const bool first = fresh;                                             // no path yet: only generate the first primary ray
            const bool miss = !first && h.objIdx == -1;                           // -> GetSkyColor
            const bool stop = !first && h.objIdx != -1 && (depth >= sc.depthLimit || h.objIdx == 0);   // depth limit -> 0, light -> (24,24,22)
            const bool surf = !first && !miss && !stop;                           // floor or mesh: the path bounces
            if (!first && h.objIdx >= 2) cn.meshhits++;
            // stage 2: texture coordinates + surface data
            const kernarg_f sk = scene_floats(offsetof(Scene, skyOffset));        // skyOffset, skyW, skyH
            float tu = 0, tv = 0; uint32_t tOff = asu(sk[0]); int tW = (int)asu(sk[1]), tH = (int)asu(sk[2]);
            f3 I = O, N = O, absorb = O; float refl = 0, refr = 0;
            if (miss) {                                                           // GetSkyColor, file_scene.cpp:142-154
                const float phi = crt_atan2f(-D.z, D.x) + CRT_PI, theta = crt_acosf(-D.y);
                tu = phi * CRT_INV2PI; tv = theta * CRT_INVPI;
            }
            if (surf) {
                I = O + h.t * D;
                SurfPoint p;
                if (h.objIdx == 1) {
                    const kernarg_f fl = scene_floats(offsetof(Scene, floorN));     // floorN[3], floorD, floorInvto
                    const kernarg_f fm = scene_floats(offsetof(Scene, floorMat));   // Material: reflectivity, refractivity, absorption[3], texOffset, texW, texH
                    const rec4 m0 = {fm[0], fm[1], fm[2], fm[3]}, m1 = {fm[4], fm[5], fm[6], fm[7]};
                    p = floor_point(mk3(fl[0], fl[1], fl[2]), fl[4], m0, m1, I);
                } else p = mesh_point<KIND>(q0, q1, q2, q3, h.u, h.v, h.objIdx, geom, sc.instOff, sc.mats);   // (q0..q3) = the hit's ShadeTri
                N = face_ray(p.N, D);
                tu = p.tu; tv = p.tv; refl = p.refl; refr = p.refr; absorb = p.absorb; tOff = p.tOff; tW = p.tW; tH = p.tH;
            }
            // stage 3: the one texel fetch (Texture::Sample) — sky colour of a miss, albedo of a textured surface
            f3 c = mk3(1.0f, 1.0f, 1.0f);
            if (miss || (surf && tW > 0)) c = tex_sample(sc, tOff, tW, tH, tu, tv);
            // stage 4a: the bounce (renderer.cpp:76-99).  `v` = outgoing direction (a diffuse one still to be normalised); its throughput factor
            // follows in stage 5, once the direction is normalised
            f3 v = O, medium = O; bool norm = false, newInside = false; Branch branch = kMirror;
            if (surf) {
                medium = medium_of(inside, absorb, h.t);
                const Bounce b = draw_bounce(seed, D, N, inside, refl, refr);
                v = b.v; branch = b.branch; newInside = b.newInside; norm = b.branch == kDiffuse;
            }
            // stage 4b: the path ended: unwind the recursion (innermost factor first: albedo*medium*Sample(...) multiplies on return),
            // store the sample, move on to the stream's next pixel
            bool gen = first;
            if (miss || stop) {
                f3 L = miss ? c : ((depth >= sc.depthLimit) ? mk3(0, 0, 0) : mk3(24, 24, 22));   // GetLightColor, file_scene.cpp:164-167
                sample_unwind(fst, depth, L);                                     // most paths end at depth 0..2: a level is read only when some lane of the wave is that deep
                uint32_t pix = item, pass = 0;
                if (passes != 1u) { pix = item / passes; pass = item - pix * passes; }
                store_sample(slab, slab_sample_offset(laneBase + lane, pix, 64u * passes, passes, pass), L);   // (`slab`: the tile's block of the window)
                item++;
                gen = true;
                if (item >= items) { live = false; gen = false; }
            }
            if (gen) {                                                            // ProcessTile + Camera::GetPrimaryRay (renderer.cpp:125-126, camera.h:23-30)
                const uint32_t pix = (passes == 1u) ? item : item / passes;
                const f3 TL = mk3(cam[3], cam[4], cam[5]), TR = mk3(cam[6], cam[7], cam[8]), BL = mk3(cam[9], cam[10], cam[11]);
                v = primary_target(camPos, TL, TR - TL, BL - TL, cam[12], cam[13], tx, ty, pix, seed); norm = true;
                inside = false; depth = 0; fresh = false;
                cn.primary++;
            }
            // stage 5: the new ray (bounce or primary) and the start of its scene.FindNearest: light quad, floor plane, root step
            if (live) {
                const float inv = rcp_exact(sqrt_exact(dot3(v, v)));              // normalize(): v * (1 / sqrtf(dot(v, v)))
                const f3 nv = norm ? v * inv : v;
                if (surf) {
                    const f3 factor = bounce_factor(branch, c, medium, nv, N);
                    float* fd = fst + depth * 192;                                // depth <= 4 here: a surface hit at depth >= depthLimit (<= 5) ended the path
                    fd[0] = factor.x; fd[64] = factor.y; fd[128] = factor.z;
                    depth++;
                    O = I + nv * CRT_EPS; inside = newInside;
                } else O = camPos;
                D = nv; rD = rcp_exact3(nv);
                cn.rays++;
                h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
                hit_light_floor(light_floor_from_kernarg<false>(), O, D, h);
                tO = O; tD = D; trD = rD; rayFinite = finite3(rD);
                sp = 0;
                if (sc.rootIsPair) {
                    // the root's two children travel in the kernel arguments (scalar registers): the first traversal step
                    // (bvh.cpp:244-257 / tlas_bvh.cpp:96-110 at the root, empty stack) happens here, at this phase's lane
                    // density, and a ray that misses both boxes never leaves the SHADE state
                    const kernarg_f rp = scene_floats(offsetof(Scene, rootPair));
                    const rec4 a0 = {rp[0], rp[1], rp[2], rp[3]}, a1 = {rp[4], rp[5], rp[6], rp[7]};
                    const rec4 b0 = {rp[8], rp[9], rp[10], rp[11]}, b1 = {rp[12], rp[13], rp[14], rp[15]};
                    float d1, d2;
                    if (__builtin_amdgcn_ballot_w64(!rayFinite) == 0ull) { d1 = box_fast(a0, a1, O, rD, h.t); d2 = box_fast(b0, b1, O, rD, h.t); }
                    else { d1 = box_exact(a0, a1, O, rD, h.t); d2 = box_exact(b0, b1, O, rD, h.t); }
                    const Ordered o = ordered_step(d1, d2, asu(a0.w), asu(b0.w));
                    stk[0] = o.farRef;                                            // dead store unless pushed
                    sp = o.push ? 1u : 0u;
                    cur = o.hitN ? o.nearRef : kRefDone;
                    if (COUNT) { if (KIND == 0) cn.interior++; else cn.tlas++; }
                } else cur = sc.rootRef;
                if (COUNT && KIND == 0 && (cur & 0xC0000000u) == 0u && cur != kRefDone) cn.leaf++;
            }
        }
        if (runShade) liveMask = __builtin_amdgcn_ballot_w64(live);             // streams end only in the SHADE phase
#ifdef CRT_STAMPS
        CRT_STAMP(s2); stT[1] += s2 - s1;
#endif
        if (KIND == 1 && runTlas && isTlas) {
            // ---------------- TLAS phase: a TLAS leaf (infra/tlas_bvh.cpp:91-95) -> enter the BLAS (BLASBVH::Intersect, blas_bvh.cpp:376-381):
            // object-space ray through the pre-loaded invT rows, return marker on the stack, BLAS root
            if (COUNT) { cn.tlas++; cn.visits++; }
            to_object_space(q0, q1, q2, O, D, tO, tD, trD);
            rayFinite = finite3(trD);
            stk[sp * 64u] = kRefReturn; sp++;
            const uint32_t next = asu(q3.z);                                      // Instance::rootRef
            if (COUNT && (next & 0xC0000000u) == 0u && next != kRefDone) cn.leaf++;
            cur = next;
        }
#ifdef CRT_STAMPS
        CRT_STAMP(s3);
#endif
        if (runNode) {
            // ---------------- NODE phase (infra/bvh.cpp:244-257) -------------------------------------------------
            const bool allFinite = __builtin_amdgcn_ballot_w64(isNode && !rayFinite) == 0ull;
            if (isNode) {
                if (COUNT) { if (KIND == 1 && (cur & kRefTlasBit) != 0u) cn.tlas++; else cn.interior++; }
                uint32_t top = CRT_TOP();                                            // speculative: lands during the slab arithmetic
                float d1, d2;
                if (allFinite) { d1 = box_fast(q0, q1, tO, trD, h.t); d2 = box_fast(q2, q3, tO, trD, h.t); }
                else { d1 = box_exact(q0, q1, tO, trD, h.t); d2 = box_exact(q2, q3, tO, trD, h.t); }
                const Ordered o = ordered_step(d1, d2, asu(q0.w), asu(q2.w));             // near child first
                stk[sp * 64u] = o.farRef;                                             // dead store unless `push`
                bool pop = !o.hitN && sp != 0u;
                uint32_t next = o.hitN ? o.nearRef : (pop ? top : kRefDone);
                sp = sp + (o.push ? 1u : 0u) - (pop ? 1u : 0u);
                next = leave_blas(next);
                if (COUNT && (next & 0xC0000000u) == 0u && next != kRefDone) cn.leaf++;
                cur = next;
            }
        }
        // ---------------- a second NODE step in the same trip (while-while, round 3): the lanes that just stepped and are still at an interior node fetch their next
        // pair now and step again, so the trip's fixed part (state ballots, phase selection, the other phases' skeleton) is paid once per two node steps; a lane that
        // just reached a leaf fetches its first triangle with them and joins THIS trip's TRI phase.  Same steps in the same order per lane.
        bool triNow = isTri;
#if CRT_TILES_NODE_STEPS > 1
        if (runNode) {
            const bool node2 = isNode && (KIND == 1 ? (((cur >> 31) ^ (cur >> 30)) & 1u) != 0u : (cur & 0xC0000000u) == kRefInterior);
            const bool leaf2 = isNode && cur != kRefDone && (cur & 0xC0000000u) == 0u;
            const uint64_t mNode2 = __builtin_amdgcn_ballot_w64(node2);
            if (mNode2 != 0ull) {
                if (node2 || leaf2) {
                    uint32_t oa, ob; record_offsets(false, oa, ob);
                    q0 = ldg(geom, oa); q1 = ldg(geom, oa + 16u); q2 = ldg(geom, ob); q3 = ldg(geom, ob + 16u);
                }
                triNow = isTri || leaf2;
                const bool allFinite2 = __builtin_amdgcn_ballot_w64(node2 && !rayFinite) == 0ull;
                if (node2) {
                    if (COUNT) { if (KIND == 1 && (cur & kRefTlasBit) != 0u) cn.tlas++; else cn.interior++; }
                    uint32_t top = CRT_TOP();
                    float d1, d2;
                    if (allFinite2) { d1 = box_fast(q0, q1, tO, trD, h.t); d2 = box_fast(q2, q3, tO, trD, h.t); }
                    else { d1 = box_exact(q0, q1, tO, trD, h.t); d2 = box_exact(q2, q3, tO, trD, h.t); }
                    const Ordered o = ordered_step(d1, d2, asu(q0.w), asu(q2.w));             // near child first
                    stk[sp * 64u] = o.farRef;
                    bool pop = !o.hitN && sp != 0u;
                    uint32_t next = o.hitN ? o.nearRef : (pop ? top : kRefDone);
                    sp = sp + (o.push ? 1u : 0u) - (pop ? 1u : 0u);
                    next = leave_blas(next);
                    if (COUNT && (next & 0xC0000000u) == 0u && next != kRefDone) cn.leaf++;
                    cur = next;
                }
            }
        }
#endif
#ifdef CRT_STAMPS
        CRT_STAMP(s4); stT[2] += s4 - s3;
#endif
        if ((runTri || triNow != isTri) && triNow) {
            // ---------------- TRI phase: one triangle of the current leaf (infra/bvh.cpp:203-222, 232-243) -----------
            if (COUNT) cn.tri++;
            uint32_t top = CRT_TOP();                                                // speculative, as in the NODE phase
            hit_tri(q0, q1, q2, tO, tD, h);
            const bool more = asu(q2.w) > 1u;                                        // next LeafTri of this leaf (48 B = 3 units)
            bool pop = !more && sp != 0u;
            uint32_t next = more ? cur + 3u : (pop ? top : kRefDone);
            sp -= pop ? 1u : 0u;
            next = leave_blas(next);
            if (COUNT && !more && (next & 0xC0000000u) == 0u && next != kRefDone) cn.leaf++;
            cur = next;
        }
#ifdef CRT_STAMPS
        CRT_STAMP(s5); stT[3] += s5 - s4;
#endif
        // ---------------- issue the record loads of every lane that moved (consumed by a later trip) ---------------
        {
            const bool doneNow = cur == kRefDone;
            uint32_t oa, ob; record_offsets(doneNow, oa, ob);
            // unconditional per lane on purpose: a lane that did not move re-fetches its record (an L1 hit) and a lane with nothing to
            // fetch reads record 0, so q0..q3 are plain loop-carried load results and nothing has to wait for them here.  Only when NO
            // lane of the wave has a record to fetch (tiles that see only sky and floor: every ray ends at the root step) the loads —
            // and the memory round trip the next trip would wait for — are skipped altogether.
            const bool nothing = !live || (doneNow && h.objIdx < 2);
            if (nothing) { oa = 0u; ob = 32u; }
            if (__builtin_amdgcn_ballot_w64(!nothing) != 0ull) { q0 = ldg(geom, oa); q1 = ldg(geom, oa + 16u); q2 = ldg(geom, ob); q3 = ldg(geom, ob + 16u); }
        }
#ifdef CRT_STAMPS
        CRT_STAMP(s6); stT[4] += s6 - s5; stT[5] += s6 - s0;
#endif
    }
#undef CRT_TOP

    // what this tile cost (100 MHz wall clock ticks; the longest of its wavefronts): the host's latency mode sizes the next launch's wavefronts with it
    if (tileCost && lane == 0) atomicMax(&tileCost[tl], (uint32_t)(wall_clock64() - clk0));
    // ... and how much of this wavefront ran after the launch's last wavefront had started (the launch's drain: abi.cpp adopt_job_costs)
    if (launchClk && lane == 0) { const unsigned long long now = wall_clock64(), last = __hip_atomic_load(&launchClk[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), from = last > clk0 ? last : clk0; if (now > from) atomicAdd(&launchClk[2], now - from); }
    if (COUNT && tileClocks && lane == 0 && windows == 1u) {                 // instrumentation build only: per-tile wall time + loop trips
        tileClocks[2 * tl] = wall_clock64() - clk0;        // 100 MHz constant clock
        tileClocks[2 * tl + 1] = trips;
#ifdef CRT_STAMPS
        unsigned long long* dbg = tileClocks + 2 * (size_t)tileCount + 16 * (size_t)tl;
        for (int i = 0; i < 6; i++) dbg[i] = stT[i];
        for (int i = 0; i < 4; i++) dbg[6 + i] = stN[i];
        for (int i = 0; i < 4; i++) dbg[10 + i] = stL[i];
#endif
    }
    // wave-level reduction of the counters, one atomic per counter per wave
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (!COUNT && i >= 2 && i != 7) continue;
        uint32_t s = wave_sum(vals[i]);
        if (lane == 0 && s) atomicAdd(&counters->v[i], (unsigned long long)s);
    }
}

// ------------------------------------------------------------------------------------------------------------
// accumulate_kernel: accumulator[pixel] += the slab's samples in (window, frame, pass) order — the reference's
// `accumulator[..] +=` order, renderer.cpp:124.  The slab is pixel-major (sample_body.h: [window][tile][pixel][sample], 12-byte samples); this kernel
// streams it with fully coalesced 768-byte loads and transposes through LDS:
//   block = one owned tile, 4 wavefronts; wavefront w owns the tile's image rows 4w .. 4w+3 (16 pixels each) and never talks to the others;
//   per (row, window, block of 64 samples): lane l fetches sample l of each of the row's 16 pixels (16 loads of 768 bytes per wave in flight),
//   parks them in the wave's LDS region, then lane (pixel j = l / 4, channel = l % 4) adds its 64 values IN ORDER to its running sum.
// The running sums of a row are 64 consecutive floats of the accumulator (one 256-byte line).  Every addition of a channel happens
// in one lane, in frame order; no float atomics anywhere.
// Blocks [texelFirst, tileCount) — the ranks a render_sky_kernel launch wrote for THIS accumulate, a fact of the launch and uniform over the block — hold the
// texel form instead: per (row, window) the 16 pixels' passes x 64 packed texels are 4 096 x passes contiguous bytes; they are parked in the order of the
// additions, and the channel lanes unpack each with tex_unpack — the sample the 12-byte form would have held — and add it in (frame, pass) order.
// The w channel: a float4 slab carried a 0.0f per sample and the w lanes added it.  x + 0.0f any number of times (>= 1) leaves the bits one such addition leaves
// (-0.0f becomes +0.0f, a signalling NaN its quiet form, everything else itself), so the w lanes add 0.0f ONCE per row — a launch has at least one sample —
// and a bound accumulator (crt_bind_accumulator: caller memory, any w) ends with the same bits as before.
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kAccRowW = 64u * 3u + 3u;         // floats per pixel row in LDS, sample form: 64 samples + 1 pad (pixel j, channel c at bank 3j + c: the channel-wise reads spread)
                                                     // texel form: 64 x passes + 1 dwords per pixel row (pixel j at bank j)
constexpr uint32_t kAccWaveLds = 64u * 65u * 4u;     // bytes per wavefront: a texel trip's pixel rows (passes 1: 64 x 65 dwords = 16 640; 2: 32 x 129; 3: 16 x 193; 4: 16 x 257); the sample form needs 16 x kAccRowW x 4 = 12 480
__device__ __forceinline__ float texel_channel(uint32_t texel, uint32_t ch) { const f3 L = tex_unpack(texel); return ch == 1u ? L.y : (ch == 2u ? L.z : L.x); }

// The texel blocks of accumulate_kernel, for one wavefront's four tile rows.  A sky tile's rows are contiguous ([pixel][pass][frame]), so a trip takes G whole rows
// of the wavefront — 4 with one pass, 2 with two, else 1: 64 (48 with three passes) loads of 256 bytes, 16 KB (12 KB) in flight per wavefront as in the sample form —
// parks every texel at its pixel's [frame x passes + pass], the order of the additions, and each lane then runs its G rows' chains of additions side by side.
template <uint32_t PASSES>
__device__ __forceinline__ void accumulate_texel_rows(const char* __restrict__ slab, float* __restrict__ acc, uint32_t* lds, uint32_t tl, uint32_t tileCount, uint32_t wave, uint32_t lane,
                                                      uint32_t x0, uint32_t y0, uint32_t W, uint32_t frames, size_t winStride)
{
    constexpr uint32_t G = PASSES == 1u ? 4u : (PASSES == 2u ? 2u : 1u), U = 16u * G * PASSES, rowLen = 64u * PASSES, pitch = rowLen + 1u;
    const uint32_t pj = lane >> 2, ch = lane & 3u;
    for (uint32_t r = 0; r < 4u; r += G) {
        const uint32_t v = wave * 4u + r;                                      // first row of the trip
        float* ap[G]; float a0[G], a[G];
#pragma unroll
        for (uint32_t g = 0; g < G; g++) { ap[g] = acc + ((size_t)(x0 + (size_t)(y0 + v + g) * W)) * 4u + lane; a0[g] = a[g] = *ap[g]; }
        const char* __restrict__ base = slab + slab_texel_position(lane, tileCount, tl, v * 16u, rowLen, PASSES, 0u);   // lane = frame of the window
        for (uint32_t f0 = 0; f0 < frames; f0 += 64u, base += winStride) {
            const uint32_t S = ((frames - f0 < 64u) ? frames - f0 : 64u) * PASSES;   // valid texels of this window's rows (a row's tail is inside the block: fetched, never added)
            uint32_t t[U];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) t[u] = load_texel(base, slab_texel_offset(0u, u / PASSES, PASSES, u % PASSES));
#pragma unroll
            for (uint32_t u = 0; u < U; u++) lds[(u / PASSES) * pitch + lane * PASSES + u % PASSES] = t[u];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // wave-private region: LDS executes a wave's operations in order
            const uint32_t* myT = lds + pj * pitch;
            uint32_t s = 0;
            for (; s + 4u <= S; s += 4u) {
                uint32_t x[G][4];
#pragma unroll
                for (uint32_t g = 0; g < G; g++)
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) x[g][k] = myT[g * 16u * pitch + s + k];
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
                    for (uint32_t g = 0; g < G; g++) a[g] += texel_channel(x[g][k], ch);
            }
            for (; s < S; s++)
#pragma unroll
                for (uint32_t g = 0; g < G; g++) a[g] += texel_channel(myT[g * 16u * pitch + s], ch);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (uint32_t g = 0; g < G; g++) *ap[g] = ch == 3u ? a0[g] + 0.0f : a[g];
    }
}

__global__ __launch_bounds__(256) void accumulate_kernel(const char* __restrict__ slab, float* __restrict__ acc, const uint32_t* __restrict__ tileOrder, uint32_t texelFirst,
                                                          uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                          uint32_t W, uint32_t frames, uint32_t passes)
{
    extern __shared__ float accLds[];
    const uint32_t rank = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (rank >= tileCount) return;
    const uint32_t tl = tileOrder ? tileOrder[rank] : rank;
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t x0 = (tile % tilesX) * 16u, y0 = (tile / tilesX) * 16u;
    const uint32_t rowLen = 64u * passes;                                      // samples per pixel row of the slab
    const size_t winStride = slab_window_bytes(tileCount, passes);
    float* myLds = accLds + wave * (kAccWaveLds / 4u);
    if (rank >= texelFirst) {                                                  // (uniform over the block)
        uint32_t* myU = reinterpret_cast<uint32_t*>(myLds);
        if (passes == 1u) accumulate_texel_rows<1>(slab, acc, myU, tl, tileCount, wave, lane, x0, y0, W, frames, winStride);
        else if (passes == 2u) accumulate_texel_rows<2>(slab, acc, myU, tl, tileCount, wave, lane, x0, y0, W, frames, winStride);
        else if (passes == 3u) accumulate_texel_rows<3>(slab, acc, myU, tl, tileCount, wave, lane, x0, y0, W, frames, winStride);
        else accumulate_texel_rows<4>(slab, acc, myU, tl, tileCount, wave, lane, x0, y0, W, frames, winStride);
        return;
    }
    const uint32_t pj = lane >> 2, ch = lane & 3u, chR = ch == 3u ? 0u : ch;    // (a w lane reads along with x and drops the sum)
    const float* myF = myLds + pj * kAccRowW + chR;
    for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t v = wave * 4u + r;                                      // row of the tile
        float* __restrict__ ap = acc + ((size_t)(x0 + (size_t)(y0 + v) * W)) * 4u + lane;   // 16 pixels x 4 channels = 64 consecutive floats
        const float a0 = *ap;
        float a = a0;
        const char* __restrict__ rowBase = slab + slab_position(0u, tileCount, tl, v * 16u, rowLen, passes, 0u);
        for (uint32_t f0 = 0; f0 < frames; f0 += 64u, rowBase += winStride) {
            const uint32_t S = ((frames - f0 < 64u) ? frames - f0 : 64u) * passes;   // valid samples of this window's rows
            for (uint32_t b = 0; b < S; b += 64u) {
                const uint32_t n = (S - b < 64u) ? S - b : 64u;
                Sample3 t[16];
                if (lane < n) {
#pragma unroll
                    for (uint32_t j = 0; j < 16u; j++) t[j] = load_sample(rowBase, slab_row_offset(j, rowLen, b + lane));
#pragma unroll
                    for (uint32_t j = 0; j < 16u; j++) { float* d = myLds + j * kAccRowW + lane * 3u; d[0] = t[j].x; d[1] = t[j].y; d[2] = t[j].z; }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // wave-private region: LDS executes a wave's operations in order
                uint32_t s = 0;
                for (; s + 8u <= n; s += 8u) {
                    float x[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) x[k] = myF[(s + k) * 3u];
#pragma unroll
                    for (int k = 0; k < 8; k++) a += x[k];
                }
                for (; s < n; s++) a += myF[s * 3u];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
        *ap = ch == 3u ? a0 + 0.0f : a;
    }
}

// ------------------------------------------------------------------------------------------------------------
// find_nearest_kernel: scene.FindNearest for a buffer of rays in the reference's traversal order (reports Ray::traversed / tested as bvh.cpp:224-258 and
// tlas_bvh.cpp:83-111 count their loop trips).  Persistent-wave form (round 3; before: one ray per lane for the whole launch, 19 % of the lanes busy): a wavefront
// draws rays from a launch-wide cursor, a lane whose ray is finished takes the next one as soon as a quarter of the wavefront is idle, and a trip of the loop runs
// each kind of step once for the lanes that are at it — TLAS node / leaf, BVH node, ONE triangle of a leaf — exactly the steps of find_nearest_seq (dev_common.h),
// which the render kernels' sequential forms still call.
// ------------------------------------------------------------------------------------------------------------
struct RayIn { float O[3]; float D[3]; int32_t inside; };
struct HitOut { float t, u, v; int32_t objIdx, triIdx, traversed, tested; };
constexpr uint32_t kQueryRefill = 16u;                                   // idle lanes that trigger the next draw from the cursor

__global__ __launch_bounds__(64) void find_nearest_kernel(const Scene sc, const RayIn* __restrict__ rays,
                                                           HitOut* __restrict__ hits, uint32_t n, Counters* __restrict__ counters, uint32_t* __restrict__ cursor)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const char* __restrict__ g = sc.geom;
    uint32_t* stk = lds + lane;                                           // BVH entries of this lane's column: entry i at [i * 64]
    uint32_t* tstk = stk + sc.bvhStack * 64;                              // TLAS entries above them
    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    // the ray in this lane
    uint32_t mode = 0u;                                                   // 0 idle, 1 at a BVH reference (`cur`), 2 inside a leaf (`leafAt`), 3 at a TLAS reference (`tcur`), 4 finished
    uint32_t idx = 0; f3 O = mk3(0, 0, 0), D = O, rD = O, Oo = O, Do = O, rDo = O;   // world-space ray; the ray the BVH is walked with (object space inside a BLAS)
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    int traversed = 0, tested = 0;
    uint32_t cur = 0, sp = 0, tcur = 0, tsp = 0, leafAt = 0;
    bool more = true;                                                     // wave-uniform: the cursor has rays left
    for (;;) {
        // ---------------- refill: idle lanes draw the next rays ----------------
        const uint64_t mIdle = __builtin_amdgcn_ballot_w64(mode == 0u);
        const uint32_t nIdle = (uint32_t)__popcll(mIdle);
        if (more && nIdle >= kQueryRefill) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, nIdle);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            more = base + nIdle < n;
            const uint32_t my = base + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mIdle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mIdle, 0u));
            if (mode == 0u && my < n) {
                idx = my;
                const RayIn r = rays[idx];
                O = mk3(r.O[0], r.O[1], r.O[2]); D = mk3(r.D[0], r.D[1], r.D[2]);
                rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);                      // Ray ctor, template/ray.h:15-24
                h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1; traversed = 0; tested = 0;
                cn.rays++;
                hit_light_floor(sc, O, D, h);
                if (sc.kind == 0) { Oo = O; Do = D; rDo = rD; cur = sc.rootRef; sp = 0; mode = 1u; }
                else { tcur = sc.rootRef; tsp = 0; mode = 3u; }
            }
        }
        if (__builtin_amdgcn_ballot_w64(mode != 0u) == 0ull) break;       // nothing in flight, nothing left to draw
        // ---------------- TLAS step (tlas_bvh.cpp:83-111): a leaf enters its BLAS, an interior node orders its children ----------------
        if (mode == 3u) {
            traversed++; cn.tlas++;
            bool pop = false;
            if ((tcur & kRefTlasLeaf) == kRefTlasLeaf) {
                cn.visits++;
                const uint32_t io = sc.instOff + (tcur & 0xffffu) * 128u;
                const rec4 r0 = ldg(g, io), r1 = ldg(g, io + 16), r2 = ldg(g, io + 32), ids = ldg(g, io + 48);
                to_object_space(r0, r1, r2, O, D, Oo, Do, rDo);
                cur = asu(ids.z); sp = 0; mode = 1u;
            } else {
                const uint32_t o1 = sc.tlasOff + (tcur & 0x7fffu) * 32u, o2 = sc.tlasOff + ((tcur >> 15) & 0x7fffu) * 32u;
                const rec4 alo = ldg(g, o1), ahi = ldg(g, o1 + 16), blo = ldg(g, o2), bhi = ldg(g, o2 + 16);
                float d1 = box_exact(alo, ahi, O, rD, h.t), d2 = box_exact(blo, bhi, O, rD, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) pop = true;
                else { tcur = r1; if (d2 != 1e30f) { tstk[tsp * 64] = r2; tsp++; } }
            }
            if (pop) { if (tsp == 0) mode = 4u; else tcur = tstk[(--tsp) * 64]; }
        }
        // ---------------- BVH step (bvh.cpp:224-258): an interior node orders its children, a leaf starts its triangle list ----------------
        bool back = false;                                                // this lane pops the BVH stack
        if (mode == 1u) {
            traversed++;
            const uint32_t off = (cur & kRefOffsetMask) << 4;
            if (cur & kRefInterior) {
                cn.interior++;
                const rec4 alo = ldg(g, off), ahi = ldg(g, off + 16), blo = ldg(g, off + 32), bhi = ldg(g, off + 48);
                float d1 = box_exact(alo, ahi, Oo, rDo, h.t), d2 = box_exact(blo, bhi, Oo, rDo, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) back = true;
                else { cur = r1; if (d2 != 1e30f) { stk[sp * 64] = r2; sp++; } }
            } else { cn.leaf++; leafAt = off; mode = 2u; }
        }
        // ---------------- one triangle of the leaf (bvh.cpp:232-243) ----------------
        if (mode == 2u) {
            const rec4 a = ldg(g, leafAt), b = ldg(g, leafAt + 16), c = ldg(g, leafAt + 32);
            tested++; cn.tri++;
            hit_tri(a, b, c, Oo, Do, h);
            if (asu(c.w) <= 1u) { back = true; mode = 1u; } else leafAt += 48;
        }
        if (back) {
            if (sp != 0) cur = stk[(--sp) * 64];
            else if (sc.kind == 0) mode = 4u;                              // the BVH is done
            else if (tsp == 0) mode = 4u;                                  // the BLAS is done: back to the TLAS loop, tlas_bvh.cpp:95
            else { tcur = tstk[(--tsp) * 64]; mode = 3u; }
        }
        if (mode == 4u) {                                                  // finished: the result record, and the lane is free
            if (h.objIdx >= 2) cn.meshhits++;
            int triIdx = h.triIdx;
            if (sc.kind != 0 && h.objIdx >= 2) triIdx -= (int)asu(ldg(g, sc.instOff + (uint32_t)(h.objIdx - 2) * 128u + 48u).x);   // - Instance::shadeBase
            HitOut o; o.t = h.t; o.u = h.u; o.v = h.v; o.objIdx = h.objIdx; o.triIdx = triIdx; o.traversed = traversed; o.tested = tested;
            hits[idx] = o;
            mode = 0u;
        }
    }
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t s = wave_sum(vals[k]);
        if (lane == 0 && s) atomicAdd(&counters->v[k], (unsigned long long)s);
    }
}

// ------------------------------------------------------------------------------------------------------------
// is_occluded_kernel: scene.IsOccluded for a buffer of shadow rays (file_scene.cpp:177-187, tlas_file_scene.cpp:208-218) over the BVH / TLAS, in
// find_nearest_kernel's persistent-wave form.  The light quad bounded by the ray's t first (a lane whose ray it occludes is done without a walk), then the
// reference's walk over the whole ray (shadow.t = 1e34f, no floor) in its order, STOPPED at the first successful triangle test: until that test the
// reference's nearest-hit walk has ray.t == 1e34f, so every box decision up to it is this walk's; after it objIdx > -1 for good (DESIGN.md "Scene queries").
// Counts nothing (the reference's IsOccluded does not count on its copy of the ray).
// ------------------------------------------------------------------------------------------------------------
struct ShadowRayIn { float O[3]; float D[3]; float t; };

__global__ __launch_bounds__(64) void is_occluded_kernel(const Scene sc, const ShadowRayIn* __restrict__ rays, int32_t* __restrict__ occluded, uint32_t n,
                                                          uint32_t* __restrict__ cursor)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const char* __restrict__ g = sc.geom;
    uint32_t* stk = lds + lane;                                           // as find_nearest_kernel: BVH entries of this lane's column, TLAS entries above them
    uint32_t* tstk = stk + sc.bvhStack * 64;
    uint32_t mode = 0u;                                                   // 0 idle, 1 at a BVH reference, 2 inside a leaf, 3 at a TLAS reference, 4 finished
    uint32_t idx = 0; f3 O = mk3(0, 0, 0), D = O, rD = O, Oo = O, Do = O, rDo = O;
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    uint32_t cur = 0, sp = 0, tcur = 0, tsp = 0, leafAt = 0;
    bool more = true;
    for (;;) {
        const uint64_t mIdle = __builtin_amdgcn_ballot_w64(mode == 0u);
        const uint32_t nIdle = (uint32_t)__popcll(mIdle);
        if (more && nIdle >= kQueryRefill) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, nIdle);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            more = base + nIdle < n;
            const uint32_t my = base + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mIdle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mIdle, 0u));
            if (mode == 0u && my < n) {
                idx = my;
                const ShadowRayIn r = rays[idx];
                O = mk3(r.O[0], r.O[1], r.O[2]); D = mk3(r.D[0], r.D[1], r.D[2]);
                if (quad_occluded(sc, O, D, r.t)) occluded[idx] = 1;      // the lane stays idle
                else {
                    rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);                  // Ray shadow(O, D) ctor, template/ray.h:15-24
                    h.t = 1e34f; h.objIdx = -1;
                    if (sc.kind == 0) { Oo = O; Do = D; rDo = rD; cur = sc.rootRef; sp = 0; mode = 1u; }
                    else { tcur = sc.rootRef; tsp = 0; mode = 3u; }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(mode != 0u) == 0ull) {
            if (!more) break;
            continue;                                                     // every drawn ray was quad-occluded: draw again
        }
        // ---------------- TLAS step (tlas_bvh.cpp:83-111) ----------------
        if (mode == 3u) {
            bool pop = false;
            if ((tcur & kRefTlasLeaf) == kRefTlasLeaf) {
                const uint32_t io = sc.instOff + (tcur & 0xffffu) * 128u;
                const rec4 r0 = ldg(g, io), r1 = ldg(g, io + 16), r2 = ldg(g, io + 32), ids = ldg(g, io + 48);
                to_object_space(r0, r1, r2, O, D, Oo, Do, rDo);
                cur = asu(ids.z); sp = 0; mode = 1u;
            } else {
                const uint32_t o1 = sc.tlasOff + (tcur & 0x7fffu) * 32u, o2 = sc.tlasOff + ((tcur >> 15) & 0x7fffu) * 32u;
                const rec4 alo = ldg(g, o1), ahi = ldg(g, o1 + 16), blo = ldg(g, o2), bhi = ldg(g, o2 + 16);
                float d1 = box_exact(alo, ahi, O, rD, h.t), d2 = box_exact(blo, bhi, O, rD, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) pop = true;
                else { tcur = r1; if (d2 != 1e30f) { tstk[tsp * 64] = r2; tsp++; } }
            }
            if (pop) { if (tsp == 0) mode = 4u; else tcur = tstk[(--tsp) * 64]; }
        }
        // ---------------- BVH step (bvh.cpp:224-258) ----------------
        bool back = false;
        if (mode == 1u) {
            const uint32_t off = (cur & kRefOffsetMask) << 4;
            if (cur & kRefInterior) {
                const rec4 alo = ldg(g, off), ahi = ldg(g, off + 16), blo = ldg(g, off + 32), bhi = ldg(g, off + 48);
                float d1 = box_exact(alo, ahi, Oo, rDo, h.t), d2 = box_exact(blo, bhi, Oo, rDo, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) back = true;
                else { cur = r1; if (d2 != 1e30f) { stk[sp * 64] = r2; sp++; } }
            } else { leafAt = off; mode = 2u; }
        }
        // ---------------- one triangle of the leaf (bvh.cpp:232-243); the first success ends the walk ----------------
        if (mode == 2u) {
            const rec4 a = ldg(g, leafAt), b = ldg(g, leafAt + 16), c = ldg(g, leafAt + 32);
            hit_tri(a, b, c, Oo, Do, h);
            if (h.objIdx > -1) mode = 4u;
            else if (asu(c.w) <= 1u) { back = true; mode = 1u; } else leafAt += 48;
        }
        if (back) {
            if (sp != 0) cur = stk[(--sp) * 64];
            else if (sc.kind == 0) mode = 4u;
            else if (tsp == 0) mode = 4u;
            else { tcur = tstk[(--tsp) * 64]; mode = 3u; }
        }
        if (mode == 4u) {
            occluded[idx] = h.objIdx > -1 ? 1 : 0;
            mode = 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// whitted_kernel: the reference's second front-end ("2. WhittedStyle/renderer.cpp":21-157) behind the same boundary.
// Deterministic (no RNG), so one thread per pixel.  The per-ray body — Trace()'s explicit post-order frame machine, its
// descend and return steps, whitted_occluded — is trace_body.h's, the one definition trace_query_kernel (trace_query.h)
// runs too; here a lane steps its own pixel's tree to the end.
// ------------------------------------------------------------------------------------------------------------

// ACCEL: 0 = the scene's BVH / TLAS, 1 / 2 = the KD-tree / uniform grid (crt_set_render_accel) for both the nearest-hit and the shadow queries: FileScene's
// (ALT = AltAccelDev) or a two-level scene's BLASKDTree / BLASGrid set (ALT = TlasAltDev)
// One Tick's metrics over the primary rays ("2. WhittedStyle/renderer.cpp":147-152) as the device collects them: exact integer sums and this Tick's maxima
// (crt_whitted_metrics' layout; the host raises the maxima by the peaks passed in).  Zeroed before every launch.
struct InspectSums { unsigned long long hits, traversal, tests; int32_t maxTraversal, maxTests; };
static_assert(sizeof(InspectSums) == 32, "crt_whitted_metrics is read back from this record");

__device__ __forceinline__ int32_t wave_max(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) { const int32_t t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
// the primary ray's record into the per-pixel count images and, one atomic per wavefront and figure, into the Tick's metrics (every lane of the wavefront calls
// this; lanes beyond the image pass zeros).  Integer add / max only: the result does not depend on the order the wavefronts arrive in.
__device__ __forceinline__ void inspect_reduce(uint32_t lane, int32_t traversed, int32_t tested, InspectSums* __restrict__ sums)
{
    const uint32_t hits = wave_sum(traversed > 0 ? 1u : 0u), st = wave_sum((uint32_t)traversed), ss = wave_sum((uint32_t)tested);
    const int32_t mt = wave_max(traversed), ms = wave_max(tested);
    if (lane == 0) {
        if (hits) atomicAdd(&sums->hits, (unsigned long long)hits);
        if (st) atomicAdd(&sums->traversal, (unsigned long long)st);
        if (ss) atomicAdd(&sums->tests, (unsigned long long)ss);
        if (mt) atomicMax(&sums->maxTraversal, mt);
        if (ms) atomicMax(&sums->maxTests, ms);
    }
}

// EXTRA: nothing (crt_whitted_tick), or one InspectOut (crt_whitted_tick_inspect, CRT_INSPECT_NONE): the same Tick, and the depth-0 ray's traversed / tested go to
// the count images and the metrics.  A parameter pack so that the instantiations without it keep their parameter list and their code.
struct InspectOut { int32_t* traversed; int32_t* tested; InspectSums* sums; };
__device__ __forceinline__ const InspectOut& inspect_out(const InspectOut& o) { return o; }
template <int ACCEL, class ALT = AltAccelDev, class... EXTRA>
__global__ __launch_bounds__(64) void whitted_kernel(const Scene sc, const ALT alt, float4* __restrict__ acc, uint32_t* __restrict__ pixels, Counters* __restrict__ counters, const EXTRA... extra)
{
    constexpr bool COUNTS = sizeof...(EXTRA) != 0;
    extern __shared__ uint32_t lds[];
    [[maybe_unused]] int32_t primTraversed = 0, primTested = 0;
    const uint32_t lane = threadIdx.x;
    const uint32_t idx = blockIdx.x * 64u + lane;
    const uint32_t W = (uint32_t)sc.W, H = (uint32_t)sc.H;
    uint32_t* stk = lds + lane;
    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    if (idx < W * H) {
        const uint32_t x = idx % W, y = idx / W;
        const f3 camPos = mk3(sc.camPos[0], sc.camPos[1], sc.camPos[2]);
        const f3 TL = mk3(sc.topLeft[0], sc.topLeft[1], sc.topLeft[2]);
        const f3 TR = mk3(sc.topRight[0], sc.topRight[1], sc.topRight[2]);
        const f3 BL = mk3(sc.bottomLeft[0], sc.bottomLeft[1], sc.bottomLeft[2]);
        const float u = (float)x * sc.invW, v = (float)y * sc.invH;                   // GetPrimaryRay((float)x, (float)y), no jitter
        const f3 P = TL + u * (TR - TL) + v * (BL - TL);
        const f3 O = camPos, D = normalize3(P - camPos); const bool inside = false;
        cn.primary++;
        WFrame fr[kWhittedMaxDepth];
        TraceState t;
        trace_begin(t, O, D, inside);
        for (;;) {
            if (t.descend) trace_descend<ACCEL, COUNTS>(sc, alt, stk, cn, t, fr, primTraversed, primTested);
            else if (trace_return(t, fr)) break;
        }
        const f3 res = t.res;
        acc[idx] = make_float4(res.x, res.y, res.z, 0.0f);
        const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, res.x)), g = (uint32_t)(255.0f * min_std(1.0f, res.y)), bb = (uint32_t)(255.0f * min_std(1.0f, res.z));
        pixels[idx] = (r << 16) + (g << 8) + bb;
        if constexpr (COUNTS) { const InspectOut& o = inspect_out(extra...); o.traversed[idx] = primTraversed; o.tested[idx] = primTested; }
    }
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t s = wave_sum(vals[k]);
        if (lane == 0 && s) atomicAdd(&counters->v[k], (unsigned long long)s);
    }
    if constexpr (COUNTS) inspect_reduce(lane, primTraversed, primTested, inspect_out(extra...).sums);
}

// ------------------------------------------------------------------------------------------------------------
// The Whitted renderer's "Inspect traversal" / "Inspect intersection" views (renderer.cpp:38-39, infra/helper.h:104-120): Trace returns
// GetTraverseCountColor(count, peak) for a primary ray that hits anything, the sky colour otherwise, with `peak` as the pixels before it in row-major order left it:
//     peakIn(i) = max(peak carried into the Tick, max over j < i of count(j)),  i = x + y * W
// Two launches, no host round trip: inspect_primary_kernel traces one ray per pixel and leaves the counts, the metrics and one maximum per kInspectBlock pixels;
// inspect_color_kernel forms the exclusive prefix maximum (carry-in from the earlier blocks' maxima, scan in the block) and colours.
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kInspectBlock = 1024;            // pixels per block of inspect_color_kernel (= per entry of blockMax)
constexpr uint32_t kInspectPending = 0xff000000u;   // screen value of a hit pixel between the two passes (a finished pixel is below 2^24)

template <int ACCEL, class ALT = AltAccelDev>
__global__ __launch_bounds__(64) void inspect_primary_kernel(const Scene sc, const ALT alt, float4* __restrict__ acc, uint32_t* __restrict__ pixels, Counters* __restrict__ counters,
                                                             int32_t* __restrict__ travOut, int32_t* __restrict__ testedOut, InspectSums* __restrict__ sums,
                                                             int32_t* __restrict__ blockMax, int useTested)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t idx = blockIdx.x * 64u + lane;
    const uint32_t W = (uint32_t)sc.W, H = (uint32_t)sc.H;
    uint32_t* stk = lds + lane;
    Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
    int traversed = 0, tested = 0;
    if (idx < W * H) {
        const uint32_t x = idx % W, y = idx / W;
        const f3 camPos = mk3(sc.camPos[0], sc.camPos[1], sc.camPos[2]);
        const f3 TL = mk3(sc.topLeft[0], sc.topLeft[1], sc.topLeft[2]);
        const f3 TR = mk3(sc.topRight[0], sc.topRight[1], sc.topRight[2]);
        const f3 BL = mk3(sc.bottomLeft[0], sc.bottomLeft[1], sc.bottomLeft[2]);
        const float u = (float)x * sc.invW, v = (float)y * sc.invH;                   // whitted_kernel's primary ray
        const f3 P = TL + u * (TR - TL) + v * (BL - TL);
        const f3 O = camPos, D = normalize3(P - camPos);
        cn.primary++;
        Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
        const f3 rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);
        if (ACCEL == 0) find_nearest_seq(sc, O, D, rD, h, stk, cn, traversed, tested);
        else {
            cn.rays++;
            hit_light_floor(sc, O, D, h);
            alt_walk<ACCEL>(sc, alt, O, D, rD, h, stk, traversed, tested);
            if (h.objIdx >= 2) cn.meshhits++;
        }
        travOut[idx] = traversed; testedOut[idx] = tested;
        if (h.objIdx == -1) {                                                          // a miss is the sky in every mode (renderer.cpp:27): finished here
            const f3 res = sky_color(sc, D);
            acc[idx] = make_float4(res.x, res.y, res.z, 0.0f);
            const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, res.x)), g = (uint32_t)(255.0f * min_std(1.0f, res.y)), bb = (uint32_t)(255.0f * min_std(1.0f, res.z));
            pixels[idx] = (r << 16) + (g << 8) + bb;
        } else pixels[idx] = kInspectPending;
    }
    uint32_t vals[8] = {cn.rays, cn.primary, cn.interior, cn.leaf, cn.tri, cn.tlas, cn.visits, cn.meshhits};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t s = wave_sum(vals[k]);
        if (lane == 0 && s) atomicAdd(&counters->v[k], (unsigned long long)s);
    }
    inspect_reduce(lane, traversed, tested, sums);
    const int32_t m = wave_max(useTested ? tested : traversed);                        // 64 | kInspectBlock: a wavefront's pixels lie in one block of the scan
    if (lane == 0 && m) atomicMax(&blockMax[idx / kInspectBlock], m);
}

// GetTraverseCountColor (infra/helper.h:104-120), operation for operation in float32: a true division, separate multiply and add (the tree builds with -ffp-contract=off)
__device__ __forceinline__ f3 traverse_count_color(int32_t traversed, int32_t peak)
{
    const float invMax = 1 / 255.f;
    const f3 green = mk3(179 * invMax, 255 * invMax, 174 * invMax);
    const f3 red = mk3(255 * invMax, 50 * invMax, 50 * invMax);
    if (peak < 10) return green;
    traversed = traversed < 0 ? 0 : (traversed > peak ? peak : traversed);
    const float blend = traversed / (float)peak;
    return mk3(green.x + blend * (red.x - green.x), green.y + blend * (red.y - green.y), green.z + blend * (red.z - green.z));
}

__global__ __launch_bounds__(1024) void inspect_color_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ blockMax, int32_t peakIn, uint32_t n,
                                                             float4* __restrict__ acc, uint32_t* __restrict__ pixels)
{
    __shared__ int32_t carryPart[16], waveMax[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t idx = blockIdx.x * kInspectBlock + tid;
    // carry-in: the peak passed in, raised by every earlier block
    int32_t c = peakIn;
    for (uint32_t j = tid; j < blockIdx.x; j += kInspectBlock) { const int32_t t = blockMax[j]; c = t > c ? t : c; }
    c = wave_max(c);
    // inclusive maximum over the wavefront's pixels up to this lane
    const int32_t own = idx < n ? count[idx] : 0;
    int32_t incl = own;
    for (int o = 1; o < 64; o <<= 1) { const int32_t t = __shfl_up(incl, o, 64); if (lane >= (uint32_t)o && t > incl) incl = t; }
    if (lane == 0) carryPart[wave] = c;
    if (lane == 63) waveMax[wave] = incl;
    __syncthreads();
    int32_t peak = carryPart[0];
#pragma unroll
    for (uint32_t w = 1; w < 16; w++) { const int32_t t = carryPart[w]; peak = t > peak ? t : peak; }
    for (uint32_t w = 0; w < wave; w++) { const int32_t t = waveMax[w]; peak = t > peak ? t : peak; }
    const int32_t before = __shfl_up(incl, 1, 64);                                     // exclusive: the lanes before this one
    if (lane > 0 && before > peak) peak = before;
    if (idx < n && pixels[idx] == kInspectPending) {
        const f3 res = traverse_count_color(own, peak);
        acc[idx] = make_float4(res.x, res.y, res.z, 0.0f);
        const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, res.x)), g = (uint32_t)(255.0f * min_std(1.0f, res.y)), bb = (uint32_t)(255.0f * min_std(1.0f, res.z));
        pixels[idx] = (r << 16) + (g << 8) + bb;
    }
}

// ------------------------------------------------------------------------------------------------------------
// resolve_kernel: one thread per owned tile; pixels in ProcessTile order so the per-tile energy sum is bit-exact
// (renderer.cpp:119,127-129; RGBF32_to_RGB8 scalar branch, template/precomp.h:336-340)
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void resolve_kernel(const float4* __restrict__ acc, uint32_t* __restrict__ pixels, float* __restrict__ tileSums,
                                                      uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                      uint32_t W, float scale)
{
    const uint32_t tl = blockIdx.x * blockDim.x + threadIdx.x;
    if (tl >= tileCount) return;
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t x0 = (tile % tilesX) * 16u, y0 = (tile / tilesX) * 16u;
    float sum = 0;
    for (uint32_t v = 0; v < 16; v++) for (uint32_t u = 0; u < 16; u++) {
        const size_t i = (x0 + u) + (size_t)(y0 + v) * W;
        const float4 a = acc[i];
        const float px = a.x * scale, py = a.y * scale, pz = a.z * scale;
        sum += px + py + pz;
        const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, px)), g = (uint32_t)(255.0f * min_std(1.0f, py)), bb = (uint32_t)(255.0f * min_std(1.0f, pz));
        pixels[i] = (r << 16) + (g << 8) + bb;
    }
    tileSums[tile] = sum;
}

// ------------------------------------------------------------------------------------------------------------
// commit_frame_kernel: crt_tick's hit — ONE rendered-ahead frame into the accumulator, then the screen: accumulate_kernel for that frame
// followed by resolve_kernel, in one pass.  Block = one owned tile, thread = pixel (v * 16 + u, the slab's pixel order).  Each channel gets the
// frame's `passes` samples in pass order (accumulate_kernel's chain of adds); the pixel is formed from the new value as resolve_kernel forms it.
// The tile's energy is summed by one lane over the 256 parked values in ProcessTile (v, u) order, so it is bit-exact (renderer.cpp:119,127-129).
// slabWindow = the launch's window that holds the frame ([tileLocal][pixel][frame * passes + pass], the 12-byte sample form of sample_body.h: a render-ahead
// launch never writes the texel form — its frames are read here after the tile order may have changed).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void commit_frame_kernel(const char* __restrict__ slabWindow, uint32_t frameInWindow, uint32_t passes,
                                                            float4* __restrict__ acc, uint32_t* __restrict__ pixels, float* __restrict__ tileSums,
                                                            uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                            uint32_t W, float scale)
{
    __shared__ float tileE[256];
    const uint32_t tl = blockIdx.x, pix = threadIdx.x;
    if (tl >= tileCount) return;
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t x0 = (tile % tilesX) * 16u, y0 = (tile / tilesX) * 16u;
    const size_t i = (x0 + (pix & 15u)) + (size_t)(y0 + (pix >> 4)) * W;
    const size_t at = slab_position(frameInWindow, tileCount, tl, pix, 64u * passes, passes, 0u);   // (frame-in-window: the window is in `slabWindow`)
    float4 a = acc[i];
    for (uint32_t p = 0; p < passes; p++) { const Sample3 t = load_sample(slabWindow, at + p * kSampleBytes); a.x += t.x; a.y += t.y; a.z += t.z; }
    a.w += 0.0f;                                                                // as accumulate_kernel's w lanes: once for the frame's >= 1 samples
    acc[i] = a;
    const float px = a.x * scale, py = a.y * scale, pz = a.z * scale;
    tileE[pix] = px + py + pz;
    const uint32_t r = (uint32_t)(255.0f * min_std(1.0f, px)), g = (uint32_t)(255.0f * min_std(1.0f, py)), bb = (uint32_t)(255.0f * min_std(1.0f, pz));
    pixels[i] = (r << 16) + (g << 8) + bb;
    __syncthreads();
    if (pix == 0) {
        float sum = 0;
        for (uint32_t k = 0; k < 256u; k++) sum += tileE[k];
        tileSums[tile] = sum;
    }
}

} // namespace crt

// ------------------------------------------------------------------------------------------------------------
// launch wrappers (called from abi.cpp)
// ------------------------------------------------------------------------------------------------------------
// self-check of dev_common.h's short reciprocals on the device at hand (tests/test_gpu_reciprocal.py through crt_debug_check_reciprocals): every one of the
// 2^32 float bit patterns through rcp_exact / rcp_exact_large / rcp_exact3 against the IEEE division, bit for bit (two NaNs count as equal).
// out = {inputs, rcp_exact differences, rcp_exact_large differences among |x| >= 1e-4 and NaN, rcp_exact3 differences}
namespace crt {
__device__ __forceinline__ bool same_bits(float a, float b) { return asu(a) == asu(b) || (a != a && b != b); }
__global__ __launch_bounds__(256) void check_reciprocals_kernel(unsigned long long* out)
{
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, nthreads = gridDim.x * 256u;
    unsigned long long n = 0, bad1 = 0, bad2 = 0, bad3 = 0;
    for (uint64_t b = tid; b < (1ull << 32); b += nthreads) {
        const float x = asf((uint32_t)b), want = 1.0f / x;
        n++;
        if (!same_bits(rcp_exact(x), want)) bad1++;
        if (!(__builtin_fabsf(x) < 0.0001f) && !same_bits(rcp_exact_large(x), want)) bad2++;
        // the other two components: a value from another part of the number line, and one that leaves the guard range now and then
        const float y = asf((uint32_t)b * 2654435761u), z = asf(((uint32_t)b >> 7) * 40503u + 0x3f000000u);
        const f3 r = rcp_exact3(mk3(x, y, z));
        if (!same_bits(r.x, want) || !same_bits(r.y, 1.0f / y) || !same_bits(r.z, 1.0f / z)) bad3++;
    }
    atomicAdd(&out[0], n); atomicAdd(&out[1], bad1); atomicAdd(&out[2], bad2); atomicAdd(&out[3], bad3);
}
} // namespace crt
extern "C" hipError_t crt_launch_check_reciprocals(unsigned long long* out, hipStream_t stream)
{
    hipLaunchKernelGGL(crt::check_reciprocals_kernel, dim3(4096), dim3(256), 0, stream, out);
    return hipGetLastError();
}

// the same self-check for dev_common.h's short square root (tests/test_gpu_pool_diet.py through crt_debug_check_sqrt): every one of the 2^32 float bit patterns
// through sqrt_exact against __builtin_sqrtf, bit for bit (two NaNs count as equal).  Consecutive bit patterns share a wavefront, so most wavefronts take the short
// form and the ones at the edges of its range (and all of the negative half) the compiler's.  out = {inputs, differences}
namespace crt {
__global__ __launch_bounds__(256) void check_sqrt_kernel(unsigned long long* out)
{
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, nthreads = gridDim.x * 256u;
    unsigned long long n = 0, bad = 0;
    for (uint64_t b = tid; b < (1ull << 32); b += nthreads) {
        const float x = asf((uint32_t)b);
        n++;
        if (!same_bits(sqrt_exact(x), __builtin_sqrtf(x))) bad++;
    }
    atomicAdd(&out[0], n); atomicAdd(&out[1], bad);
}
} // namespace crt
extern "C" hipError_t crt_launch_check_sqrt(unsigned long long* out, hipStream_t stream)
{
    hipLaunchKernelGGL(crt::check_sqrt_kernel, dim3(4096), dim3(256), 0, stream, out);
    return hipGetLastError();
}

// blockDesc / nBlocks: block table (see the kernel; the launch renders exactly the table's blocks), else nullptr / 0; tileCost: nullptr or one uint32 per tile, atomicMax'ed
extern "C" hipError_t crt_launch_render(const crt::Scene* sc, void* slab, crt::Counters* counters, unsigned long long* tileClocks, const uint32_t* tileOrder,
                                        uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst,
                                        uint32_t frames, uint32_t passes, uint32_t ldsBytes, int collectStats, const uint32_t* blockDesc, uint32_t nBlocks, uint32_t* tileCost, uint32_t rankCount, unsigned long long* launchClk, hipStream_t stream)
{
    if (tileCount == 0 || frames == 0) return hipSuccess;
    const uint32_t windows = (frames + 63u) / 64u;                      // one 64-lane wavefront per (tile, 64-frame window)
    if ((unsigned long long)tileCount * windows > 0x7fffffffull) return hipErrorInvalidValue;
    if (collectStats || nBlocks == 0u) blockDesc = nullptr;
    if (blockDesc && (tileCount > 0x10000u || windows > 64u)) return hipErrorInvalidValue;
    if (rankCount == 0u || rankCount > tileCount) rankCount = tileCount;          // the first rankCount tiles of the order only (all windows)
    dim3 grid(blockDesc ? nBlocks : rankCount * windows), block(64);
#define CRT_LAUNCH(K, C) hipLaunchKernelGGL((crt::render_tiles_kernel<K, C>), grid, block, ldsBytes + 15u * 64u * 4u /* throughput-factor columns */, stream, *sc, (char*)slab, counters, tileClocks, tileOrder, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, windows, blockDesc, tileCost, rankCount, launchClk)
    if (sc->kind == 0) { if (collectStats) CRT_LAUNCH(0, true); else CRT_LAUNCH(0, false); }
    else { if (collectStats) CRT_LAUNCH(1, true); else CRT_LAUNCH(1, false); }
#undef CRT_LAUNCH
    return hipGetLastError();
}

// how many wavefronts of render_tiles_kernel the device holds at once (registers: 5 per SIMD; LDS: the stack columns) — the size the latency tuner fits its block tables to
extern "C" uint32_t crt_render_resident_waves(int device, int kind, uint32_t ldsBytes)
{
    int perCu = 0, cus = 0;
    const size_t lds = (size_t)ldsBytes + 15u * 64u * 4u;
    hipError_t e = kind == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, crt::render_tiles_kernel<0, false>, 64, lds)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, crt::render_tiles_kernel<1, false>, 64, lds);
    if (e != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || perCu <= 0 || cus <= 0) { (void)hipGetLastError(); return 5120u; }
    return (uint32_t)perCu * (uint32_t)cus;
}

extern "C" size_t crt_slab_window_bytes(uint32_t tileCount, uint32_t passes) { return crt::slab_window_bytes(tileCount, passes); }

extern "C" void crt_slab_layout_probe(int texel, uint32_t frames, uint32_t tileCount, uint32_t passes, unsigned long long* pos, unsigned long long* sizes)
{
    for (uint32_t fr = 0; fr < frames; fr++)
        for (uint32_t tl = 0; tl < tileCount; tl++)
            for (uint32_t pix = 0; pix < 256u; pix++)
                for (uint32_t pass = 0; pass < passes; pass++)
                    *pos++ = texel ? crt::slab_texel_position(fr, tileCount, tl, pix, 64u * passes, passes, pass) : crt::slab_position(fr, tileCount, tl, pix, 64u * passes, passes, pass);
    sizes[0] = crt::slab_window_bytes(tileCount, passes);
    sizes[1] = crt::slab_tile_bytes(passes);
}

extern "C" hipError_t crt_launch_accumulate(const void* slab, void* acc, const uint32_t* tileOrder, uint32_t texelFirst, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount,
                                            uint32_t tilesX, uint32_t W, uint32_t frames, uint32_t passes, hipStream_t stream)
{
    if (tileCount == 0 || frames == 0) return hipSuccess;
    if (passes < 1u || passes > 4u || (texelFirst < tileCount && !tileOrder)) return hipErrorInvalidValue;   // (the LDS region holds 4 passes of texel rows; texel blocks are ranks of an order)
    dim3 grid(tileCount), block(256);
    hipLaunchKernelGGL(crt::accumulate_kernel, grid, block, 4u * crt::kAccWaveLds, stream, (const char*)slab, (float*)acc, tileOrder, texelFirst, tileFirst, tileStride, tileCount, tilesX, W, frames,
                       passes);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_find_nearest(const crt::Scene* sc, const void* rays, void* hits, uint32_t n, crt::Counters* counters,
                                              uint32_t ldsBytes, uint32_t* cursor, hipStream_t stream)
{
    hipError_t e; if (!crt::query_launch_begin(n, cursor, stream, &e)) return e;       // no rays: nothing to do; the cursor zeroed on the stream (launch.h)
    dim3 grid(crt::query_grid(n, ldsBytes)), block(64);                 // persistent wavefronts (launch.h)
    hipLaunchKernelGGL(crt::find_nearest_kernel, grid, block, ldsBytes, stream, *sc, (const crt::RayIn*)rays, (crt::HitOut*)hits, n, counters, cursor);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_is_occluded(const crt::Scene* sc, const void* rays, int32_t* occluded, uint32_t n, uint32_t ldsBytes, uint32_t* cursor, hipStream_t stream)
{
    hipError_t e; if (!crt::query_launch_begin(n, cursor, stream, &e)) return e;       // no rays: nothing to do; the cursor zeroed on the stream (launch.h)
    dim3 grid(crt::query_grid(n, ldsBytes)), block(64);
    hipLaunchKernelGGL(crt::is_occluded_kernel, grid, block, ldsBytes, stream, *sc, (const crt::ShadowRayIn*)rays, occluded, n, cursor);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_whitted(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, void* acc, uint32_t* pixels, crt::Counters* counters, uint32_t ldsBytes,
                                         hipStream_t stream)
{
    const uint32_t n = (uint32_t)sc->W * (uint32_t)sc->H;
    dim3 grid((n + 63u) / 64u), block(64);
    if (accel != 0 && sc->kind != 0) {                                    // a two-level scene's BLASKDTree / BLASGrid set (crt_upload_blas_accel)
        const uint32_t bytes = crt::tlas_alt_stack_words(*sc, *tl) * 64u * 4u;
        if (bytes > 64u * 1024u) return hipErrorInvalidValue;
        if (accel == 1) hipLaunchKernelGGL((crt::whitted_kernel<1, crt::TlasAltDev>), grid, block, bytes, stream, *sc, *tl, (float4*)acc, pixels, counters);
        else hipLaunchKernelGGL((crt::whitted_kernel<2, crt::TlasAltDev>), grid, block, bytes, stream, *sc, *tl, (float4*)acc, pixels, counters);
        return hipGetLastError();
    }
    if (accel == 1) hipLaunchKernelGGL(crt::whitted_kernel<1>, grid, block, alt->kdStack * 128u * 4u, stream, *sc, *alt, (float4*)acc, pixels, counters);
    else if (accel == 2) hipLaunchKernelGGL(crt::whitted_kernel<2>, grid, block, 256u, stream, *sc, *alt, (float4*)acc, pixels, counters);
    else { const crt::AltAccelDev none{}; hipLaunchKernelGGL(crt::whitted_kernel<0>, grid, block, ldsBytes, stream, *sc, none, (float4*)acc, pixels, counters); }
    return hipGetLastError();
}

// crt_trace / crt_trace_device (trace_query.h).  Dwords of traversal stack per lane, by crt_launch_whitted's rules: the scene's own stack, a FileScene's KD stack (two
// words per entry) or the grid's single word, a two-level set's KD + TLAS stack
extern "C" uint32_t crt_trace_query_stack_words(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl)
{
    if (accel == 0) return sc->stackDepth;
    if (sc->kind != 0) return crt::tlas_alt_stack_words(*sc, *tl);
    return accel == 1 ? alt->kdStack * 2u : 1u;
}

extern "C" hipError_t crt_launch_trace_query(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, const void* rays, float* rgb, int32_t* trav,
                                             int32_t* tested, uint32_t n, crt::Counters* counters, uint32_t* cursor, uint32_t* residentLanes, hipStream_t stream)
{
    const uint32_t words = crt_trace_query_stack_words(sc, accel, alt, tl);
    if (accel != 0 && sc->kind != 0) {                                    // a two-level scene's BLASKDTree / BLASGrid set (crt_upload_blas_accel)
        if (accel == 1) return crt::launch_trace_query<1>(sc, *tl, words, rays, rgb, trav, tested, n, counters, cursor, residentLanes, stream);
        return crt::launch_trace_query<2>(sc, *tl, words, rays, rgb, trav, tested, n, counters, cursor, residentLanes, stream);
    }
    if (accel == 1) return crt::launch_trace_query<1>(sc, *alt, words, rays, rgb, trav, tested, n, counters, cursor, residentLanes, stream);
    if (accel == 2) return crt::launch_trace_query<2>(sc, *alt, words, rays, rgb, trav, tested, n, counters, cursor, residentLanes, stream);
    const crt::AltAccelDev none{};
    return crt::launch_trace_query<0>(sc, none, words, rays, rgb, trav, tested, n, counters, cursor, residentLanes, stream);
}

// crt_whitted_tick_inspect.  work = InspectSums followed by one int32 per kInspectBlock pixels; zeroed here, on the stream.  inspect 0: whitted_kernel's Tick with the
// counts (one launch); 1 / 2: the primary pass and the scan + colour pass.
template <int ACCEL, class ALT>
static hipError_t launch_whitted_inspect(const crt::Scene& sc, const ALT& alt, uint32_t ldsBytes, int inspect, int32_t peakIn, float4* acc, uint32_t* pixels, crt::Counters* counters,
                                         int32_t* trav, int32_t* tested, crt::InspectSums* sums, int32_t* blockMax, hipStream_t stream)
{
    const uint32_t n = (uint32_t)sc.W * (uint32_t)sc.H;
    dim3 grid((n + 63u) / 64u), block(64);
    if (inspect == 0) {
        const crt::InspectOut out{trav, tested, sums};
        hipLaunchKernelGGL((crt::whitted_kernel<ACCEL, ALT, crt::InspectOut>), grid, block, ldsBytes, stream, sc, alt, acc, pixels, counters, out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((crt::inspect_primary_kernel<ACCEL, ALT>), grid, block, ldsBytes, stream, sc, alt, acc, pixels, counters, trav, tested, sums, blockMax, inspect == 2 ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::inspect_color_kernel, dim3((n + crt::kInspectBlock - 1u) / crt::kInspectBlock), dim3(crt::kInspectBlock), 0, stream,
                       inspect == 2 ? tested : trav, blockMax, peakIn, n, acc, pixels);
    return hipGetLastError();
}

extern "C" size_t crt_whitted_inspect_work_bytes(uint32_t pixelCount) { return sizeof(crt::InspectSums) + (size_t)((pixelCount + crt::kInspectBlock - 1u) / crt::kInspectBlock) * 4u; }

extern "C" hipError_t crt_launch_whitted_inspect(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, int inspect, int32_t peakIn, void* acc, uint32_t* pixels,
                                                 crt::Counters* counters, int32_t* trav, int32_t* tested, void* work, uint32_t ldsBytes, hipStream_t stream)
{
    if (inspect < 0 || inspect > 2 || peakIn < 0 || !trav || !tested || !work) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)sc->W * (uint32_t)sc->H;
    uint32_t bytes = 0;
    if (accel != 0 && sc->kind != 0) {                                    // the stack check of crt_launch_whitted, before anything is written
        bytes = crt::tlas_alt_stack_words(*sc, *tl) * 64u * 4u;
        if (bytes > 64u * 1024u) return hipErrorInvalidValue;
    }
    if (hipMemsetAsync(work, 0, crt_whitted_inspect_work_bytes(n), stream) != hipSuccess) return hipGetLastError();
    crt::InspectSums* sums = (crt::InspectSums*)work;
    int32_t* blockMax = (int32_t*)(sums + 1);
    if (accel != 0 && sc->kind != 0) {
        if (accel == 1) return launch_whitted_inspect<1>(*sc, *tl, bytes, inspect, peakIn, (float4*)acc, pixels, counters, trav, tested, sums, blockMax, stream);
        return launch_whitted_inspect<2>(*sc, *tl, bytes, inspect, peakIn, (float4*)acc, pixels, counters, trav, tested, sums, blockMax, stream);
    }
    if (accel == 1) return launch_whitted_inspect<1>(*sc, *alt, alt->kdStack * 128u * 4u, inspect, peakIn, (float4*)acc, pixels, counters, trav, tested, sums, blockMax, stream);
    if (accel == 2) return launch_whitted_inspect<2>(*sc, *alt, 256u, inspect, peakIn, (float4*)acc, pixels, counters, trav, tested, sums, blockMax, stream);
    const crt::AltAccelDev none{};
    return launch_whitted_inspect<0>(*sc, none, ldsBytes, inspect, peakIn, (float4*)acc, pixels, counters, trav, tested, sums, blockMax, stream);
}

extern "C" hipError_t crt_launch_resolve(const void* acc, uint32_t* pixels, float* tileSums, uint32_t tileFirst, uint32_t tileStride,
                                         uint32_t tileCount, uint32_t tilesX, uint32_t W, float scale, hipStream_t stream)
{
    if (tileCount == 0) return hipSuccess;
    dim3 grid((tileCount + 63u) / 64u), block(64);
    hipLaunchKernelGGL(crt::resolve_kernel, grid, block, 0, stream, (const float4*)acc, pixels, tileSums, tileFirst, tileStride, tileCount, tilesX, W, scale);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_commit_frame(const void* slabWindow, uint32_t frameInWindow, uint32_t passes, void* acc, uint32_t* pixels, float* tileSums,
                                              uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t W, float scale, hipStream_t stream)
{
    if (tileCount == 0) return hipSuccess;
    if (frameInWindow >= 64u || passes < 1u || passes > 4u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::commit_frame_kernel, dim3(tileCount), dim3(256), 0, stream, (const char*)slabWindow, frameInWindow, passes, (float4*)acc, pixels, tileSums,
                       tileFirst, tileStride, tileCount, tilesX, W, scale);
    return hipGetLastError();
}
