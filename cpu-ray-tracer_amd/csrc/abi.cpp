// abi.cpp — implementation of include/crt_abi.h: context, scene flattening + upload, launches, read-back.
// Host-only logic; the kernels live in device/*.hip, behind the launch wrappers that device/launch.h declares, and take the structs of device/layout.h.
// There is NO CPU rendering path in this library: without a HIP device crt_create fails with CRT_ERR_NO_DEVICE.
#include "../../include/crt_abi.h"
#include "device/launch.h"
#include "device/tile_class.h"
#include "device/build_common.h"
#include "host/grid_resolution.h"

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <algorithm>
#include <vector>
#include <chrono>

static_assert(sizeof(crt_bvh_node) == 32 && sizeof(crt_tri) == 112 && sizeof(crt_tlas_node) == 32, "reference layouts");
static_assert(sizeof(crt::NodePair) == 64 && sizeof(crt::LeafTri) == 48 && sizeof(crt::ShadeTri) == 64 && sizeof(crt::TlasNode) == 32 &&
              sizeof(crt::Instance) == 128 && sizeof(crt::Material) == 32 && offsetof(crt::Instance, T) == 64, "device layouts");
static_assert(sizeof(crt_counters) == sizeof(crt::Counters), "counter layout");
static_assert(sizeof(crt_kd_node) == 48 && sizeof(crt::KdNode) == sizeof(crt_kd_node) && sizeof(crt::AltTri) == 48, "flat KD node (uploaded as it comes), alternative accelerators' triangle record");
static_assert(offsetof(crt::PrimDev, red) == 536 && sizeof(crt::PrimDev) == 552, "PrimDev: 134 floats, then the two texel pointers");
static_assert(sizeof(crt::BlasAltDesc) == 72, "BLAS descriptor");
static_assert(sizeof(crt_shadow_ray) == 28 && sizeof(crt_ray) == 28 && sizeof(crt_hit) == 28, "query records");
static_assert(sizeof(crt_hit_info) == 48 && offsetof(crt_hit_info, material) == 12 && offsetof(crt_hit_info, N) == 16 && offsetof(crt_hit_info, albedo) == 32 && offsetof(crt_hit_info, v) == 44, "crt_hit_info: three 16-byte pieces");
static_assert(sizeof(crt::Instance) == 128 && offsetof(crt::Instance, triCount) == 112, "Instance record");

namespace {

thread_local std::string g_createError;

// Test / diagnostic switches (CRT_RENDER_KERNEL, CRT_LAT_*, CRT_SPLIT_*, CRT_DEBUG_*, CRT_PLAN_*) are environment variables that are looked at
// ONLY after the process has called crt_debug_enable_hooks(1) — the test suite and the tools do, a host application never does, so a variable that happens to be
// exported in its environment cannot change what the library does.
bool g_hooks = false;
inline const char* hook(const char* name) { return g_hooks ? getenv(name) : nullptr; }

struct EventPair { hipEvent_t a, b; int mode = -1; bool seen = false; };   // mode: latency-mode stage of a single-window launch, 100 / 101 a plain / planned job trial, -1 otherwise (harvest_tuning)

} // namespace

// CRT_DEBUG_QUERY_GRID=<k>, k >= 1: every persistent query launch (find-nearest, is-occluded, their KD-tree / grid and two-level forms, Sample, Trace) uses at most k
// workgroups, so a few thousand rays are enough for every lane to take ray after ray from the cursor (tests/test_gpu_query_lane_reuse.py).  Read on every launch
// by the wrappers in device/*.hip (launch.h bounded_query_grid); unset or 0: the launch's own grid.  crt_debug_sample_resident_lanes / crt_debug_trace_resident_lanes are not launches and ignore it.
extern "C" uint32_t crt_debug_query_grid(void)
{
    const char* e = hook("CRT_DEBUG_QUERY_GRID");
    const long k = e ? strtol(e, nullptr, 10) : 0;
    return k > 0 ? (uint32_t)(k > 0x7fffffffL ? 0x7fffffffL : k) : 0u;
}

struct crt_ctx {
    crt_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    int tilesX = 0, tilesY = 0;
    uint32_t tileFirst = 0, tileStride = 1, tileCount = 0;
    // device memory
    void* dAccOwned = nullptr; void* dAcc = nullptr;
    // Render launches (independent: different spp windows) rotate over `streams` so that consecutive crt_render calls overlap on
    // the GPU; the ordered accumulate kernels run on the main stream behind events.  Their sample slabs are regions of ONE pool
    // handed out as a ring: launch order = accumulate order = release order, so the oldest region is always the next to free.
    std::vector<hipStream_t> streams; uint64_t launchSeq = 0;
    // freed: recorded on the main stream behind the region's accumulate.  held: the region of a crt_tick render-ahead launch whose frames are not all committed
    // or discarded yet — its `freed` is not recorded, so take_region must never wait on it
    struct Region { size_t off, bytes; hipEvent_t freed; bool held = false; };
    std::deque<Region> inflight;
    char* pool = nullptr; size_t poolBytes = 0, poolHead = 0; bool poolCapped = false;   // capped: already as large as the HBM budget allows
    hipEvent_t mustWait = nullptr;                                // `freed` of the newest region whose space was handed out again
    std::vector<hipEvent_t> freeEvents;
    std::vector<hipEvent_t> doneEvents;                           // recycled end events of render-ahead launches
    // crt_tick's render-ahead queue (see crt_tick): launches of the frames after the last Tick, valid for one state epoch and the next (spp, passes)
    struct Ahead { hipEvent_t end; size_t off; const char* slab; uint64_t epoch; uint32_t sppFirst, nf, passes, used; };   // used: frames committed so far
    std::deque<Ahead> ahead;
    uint64_t epoch = 1;                   // bumped by every change the samples depend on: camera, scene upload / update, render accelerator
    uint64_t tickEpoch = 0; uint32_t tickNextSpp = 0, tickPasses = 0;   // the previous crt_tick: its epoch (0: none), spp + passes, passes
    uint32_t aheadFrames = 0;             // frames of the newest render-ahead launch (doubles while Ticks hit)
    hipStream_t aheadStream = nullptr;    // low-priority stream of the render-ahead launches
    hipStream_t skyStream = nullptr;      // low-priority stream of the sky launches submitted behind their job's pool launch (launch_render_kernels)
    crt::Scene hScene{};
    crt::Counters* dCounters = nullptr;
    uint32_t* dQueryCursor = nullptr;      // the ray cursor of the persistent query kernels (zeroed by each launch)
    // crt_whitted_tick_inspect: the primary rays' traversed / tested images (two int32 per pixel) and the metrics record + per-block maxima; allocated by the first call
    int32_t* dInspectCounts = nullptr; void* dInspectWork = nullptr; size_t inspectCap = 0;
    uint32_t* dPixels = nullptr; float* dTileSums = nullptr;
    unsigned long long* dTileClocks = nullptr;
    std::vector<void*> sceneAllocs;
    // dispatch-order heuristic: owned tiles that can see the scene's meshes come first (see render_tiles_kernel)
    float meshLo[3] = {0, 0, 0}, meshHi[3] = {0, 0, 0}; bool orderDirty = true;
    uint32_t* dTileOrder = nullptr;
    uint32_t* hTileOrder[2] = {nullptr, nullptr}; hipEvent_t orderCopied[2] = {nullptr, nullptr}; hipEvent_t orderReady = nullptr; int orderFlip = 0;
    // render_pool_kernel's tile classes (device/tile_class.h): one byte per owned tile, stale from every write of the Scene's camera-relative block (primary_changed)
    // until the next crt_render classifies again (update_tile_class); a launch never sees a stale table (launch_render_kernels passes none)
    bool classDirty = true;
    uint8_t* dTileClass = nullptr;
    uint8_t* hTileClass[2] = {nullptr, nullptr}; hipEvent_t classCopied[2] = {nullptr, nullptr}; int classFlip = 0;
    // The kTileSky tiles of that table (hostClass: the host's copy of it; skyTiles of them) are the TAIL of every tile order (sky_to_tail), and a pool launch that has
    // the table leaves that tail to one render_sky_kernel launch of the same job (sky_split, launch_render_kernels).  skyLaunches: those launches so far
    // (crt_debug_sky_launches); skyWindowTicks: what one window of them took in the measuring job (adopt_job_costs; 0: unknown)
    std::vector<uint8_t> hostClass; uint32_t skyTiles = 0, skyLaunches = 0; double skyWindowTicks = 0;
    bool haveScene = false;
    // what crt_update_scene needs of the last upload: a host mirror of the geometry buffer and where each BVH's records start
    struct Flat { int32_t kind = 0; uint64_t leafOff = 0, tlasOff = 0, tlasPairOff = 0, instOff = 0, shadeOff = 0; uint32_t tlasNodeCount = 0, maxHeight = 0;
                  uint32_t objects = 0;           // objCount (FileScene) / bvhCount (two-level): the objIdx a hit record may carry is below 2 + objects
                  std::vector<uint64_t> pairBase, triBase; std::vector<uint32_t> nodesUsed, triCount, height; std::vector<char> geom;   // height: every BVH's deepest leaf, in edges
                  std::vector<float> rootBox;
                  uint32_t materialCount = 0; std::vector<crt::TexDesc> tex; } flat;   // crt_update_look / crt_render_looks: the scene's material count, its texture table (dTex: the device's copy)
    const crt::TexDesc* dTex = nullptr;     // rootBox: every BVH's node 0 box (min xyz, max xyz), what crt_upload_blas_accel checks the BLAS structures against
    char* hStage[2] = {nullptr, nullptr}; size_t stageBytes[2] = {0, 0}; hipEvent_t stageCopied[2] = {nullptr, nullptr}; int stageFlip = 0;
    hipEvent_t sceneReady = nullptr, writeFence = nullptr;   // the scene-write protocol (begin_scene_write): the last write's `done` event, the protocol's own fence
    bool havePrim = false; crt::PrimDev prim{}; uint32_t* dPrimTex = nullptr;       // crt_upload_primitive_scene: PrimitiveScene instead of a triangle scene
    int renderAccel = 0;                  // crt_set_render_accel: 0 = the scene's BVH / TLAS, CRT_ACCEL_KDTREE / CRT_ACCEL_GRID = Sample and Trace go through that structure
    crt::AltAccelDev alt{}; bool haveKd = false, haveGrid = false; std::vector<void*> altAllocs[2]; crt::AltTri* altTris = nullptr; uint32_t altTriCount = 0;   // KD-tree [0] / grid [1] buffers
    // crt_upload_blas_accel: a two-level scene's BLASKDTree [0] / BLASGrid [1] set.  haveBlas is cleared by CRT_UPDATE_BOUNDS without a host wait; the buffers
    // go with the next upload of the kind or of a scene, which wait for the queries first
    crt::TlasAltDev blasAlt[2]{}; bool haveBlas[2] = {false, false}; std::vector<void*> blasAllocs[2];
    bool hasAlt(int kind) const { return (kind == CRT_ACCEL_KDTREE && (haveKd || haveBlas[0])) || (kind == CRT_ACCEL_GRID && (haveGrid || haveBlas[1])); }
    char* dStage = nullptr; size_t stageCap = 0;   // device staging of the host-buffer query entries (stage()): one call's records in and out, then the call synchronises
    // Device-buffer queries (crt_find_nearest_device / crt_is_occluded_device) on callers' streams: each launch draws its rays from a cursor word of its own
    // (slot k at dQuerySlots + 16k, one cache line each), handed out as a ring; `done` is recorded on the caller's stream behind the launch, and a slot is
    // reused only after its event has completed.  The same events order later scene writes behind the queries still in flight (order_behind_queries).
    static constexpr int kQuerySlots = 64;
    uint32_t* dQuerySlots = nullptr;
    struct QuerySlot { hipEvent_t done = nullptr; bool pending = false; } qslot[kQuerySlots];
    int qslotNext = 0;
    // crt_render_views / crt_render_views_device: the sample slab of their launches, scratch of the entries' own (whole windows, grown on demand, kept until
    // crt_destroy) — the slab pool and crt_tick's held regions are not touched; viewsDone: behind the last call's last accumulate, on that call's stream (the next
    // call's stream waits for it before it writes the slab again)
    char* dViewsSlab = nullptr; size_t viewsSlabCap = 0; hipEvent_t viewsDone = nullptr; bool viewsPending = false;
    // (crt_render_shapes / crt_render_shapes_device keep their shape table, layout.h ShapeJobHeader, and its pinned copy in the same four: a job-local table either way)
    // crt_render_poses / crt_render_poses_device: the job's pose table (device/layout.h PoseJobHeader: P build headers, P images of [tlasOff, shadeOff)), scratch of the
    // entries' own like dViewsSlab and ordered by the same event (the job's launches read it to the end); hPoseBack: the pinned copy of the headers (and, for
    // tlas_out, of the images' node sections), poseBack: behind that read-back (the entries' one host wait)
    char* dPoseTable = nullptr; size_t poseTableCap = 0; char* hPoseBack = nullptr; size_t poseBackCap = 0; hipEvent_t poseBack = nullptr;
    // crt_refit_device: per BVH the bottom-up plan of refit_box_kernel (device/refit.hip), built from the mirror's references by the first refit of that BVH and
    // freed with the scene; the root's pair + node 0's box come back through `hBack` (pinned) behind the kernels, and `done` is what sceneReady then names
    struct RefitPlan { void* dPlan = nullptr; uint32_t* dLevelOff = nullptr; uint32_t levels = 0, rootCode = 0; bool built = false; };
    std::vector<RefitPlan> refitPlans; std::vector<void*> refitAllocs;
    struct Refit {
        float* dBack = nullptr; float* hBack = nullptr; hipEvent_t done = nullptr;
        void release() { if (done) (void)hipEventDestroy(done); (void)hipFree(dBack); (void)hipHostFree(hBack); *this = Refit{}; }
    } refit;
    // crt_update_transforms_device (device/tlas_build.hip): every BLAS's node-0 box on the device (6 floats each; written at upload, by CRT_UPDATE_BOUNDS and by
    // crt_refit_device on its stream, freed with the scene), the kernel's result block and its pinned copy (TlasBuildHeader + an image of [tlasOff, shadeOff)),
    // and the events: `back` behind the read-back (the one host wait), `done` behind the copy into the geometry buffer (what sceneReady then names)
    float* dRootBox = nullptr;
    struct TlasBuild {
        char* dBuild = nullptr; char* hBack = nullptr; size_t bytes = 0;
        hipEvent_t back = nullptr, done = nullptr, t0 = nullptr, t1 = nullptr; bool timed = false;
        void release() { for (hipEvent_t e : {back, done, t0, t1}) if (e) (void)hipEventDestroy(e); (void)hipFree(dBuild); (void)hipHostFree(hBack); *this = TlasBuild{}; }
    } tlasBuild;
    // What crt_build_grid_device and crt_build_kdtree_device keep alike between calls: `back` behind each read-back (the host waits), `done` behind the build
    // (sceneReady names it; the next build of the kind, which reuses the scratch, waits for it), t0 / t1 round the build under the debug hooks, and the workgroups
    // the device holds at once (crt_grid_build_blocks)
    struct AccelBuild {
        hipEvent_t back = nullptr, done = nullptr, t0 = nullptr, t1 = nullptr; bool built = false, timed = false; uint32_t blocks = 0;
        void releaseEvents() { for (hipEvent_t e : {back, done, t0, t1}) if (e) (void)hipEventDestroy(e); }
    };
    // crt_build_grid_device (device/grid_build.hip): the kernels' state block and its pinned copy, scratch (the scan's chunk sums, the fill's cursors and unsorted
    // references, grown on demand; capacities in bytes); two read-backs, so two host waits
    struct GridBuild : AccelBuild {
        crt::GridBuildState* dState = nullptr; crt::GridBuildState* hState = nullptr;
        unsigned long long* dChunks = nullptr; void* dCursor = nullptr; void* dUnsorted = nullptr; size_t cursorCap = 0, unsortedCap = 0;
        double waitMs[2] = {0, 0};        // wall time of the last call's two host waits (crt_debug_grid_build_ms)
        void release() { releaseEvents(); for (void* p : {(void*)dState, (void*)dChunks, dCursor, dUnsorted}) (void)hipFree(p); (void)hipHostFree(hState); *this = GridBuild{}; }
    } gridBuild;
    // A structure the build replaces may still be read by launches enqueued earlier: its buffers go to `retired` with an event recorded on the main stream
    // once that is ordered behind those launches, and are freed by a later call that finds the event complete (or with the scene, which drains first).
    struct Retired { std::vector<void*> ptrs; void* pinned = nullptr; hipEvent_t unread = nullptr; };
    std::deque<Retired> retired; std::vector<hipEvent_t> retiredEvents;
    uint32_t gridRefCount = 0;            // references of the FileScene's live grid (uploaded or built on the device)
    // crt_build_kdtree_device (device/kd_build.hip): the kernels' state block and its pinned copy; per level the nodes, the references and their owner nodes, kept
    // until the finalise pass; the triangle boxes, the two scan arrays and the chunk sums — all grown on demand and kept between calls; one read-back (host wait) per level
    struct KdBuild : AccelBuild {
        static constexpr uint32_t kLevels = crt::kKdMaxDepth + 1u;
        crt::KdBuildState* dState = nullptr; crt::KdBuildState* hState = nullptr;
        struct Level { void* nodes = nullptr; void* refs = nullptr; void* owner = nullptr; size_t nodeCap = 0, refCap = 0, ownerCap = 0; } lv[kLevels];
        void* dTriBox = nullptr; void* dNodeItems = nullptr; void* dRefItems = nullptr; void* dChunks = nullptr; size_t triBoxCap = 0, nodeItemCap = 0, refItemCap = 0, chunkCap = 0;
        uint32_t waits = 0, levels = 0; double waitMs = 0;    // the last call's host waits, its levels, the wall time of the waits together (crt_debug_kdtree_build_ms)
        void release()
        {
            releaseEvents();
            for (Level& l : lv) for (void* p : {l.nodes, l.refs, l.owner}) (void)hipFree(p);
            for (void* p : {(void*)dState, dTriBox, dNodeItems, dRefItems, dChunks}) (void)hipFree(p);
            (void)hipHostFree(hState); *this = KdBuild{};
        }
    } kdBuild;
    // crt_build_bvh_device (device/bvh_build.hip): the kernels' state block and its pinned copy; the node records and box keys of all levels (at most 2n - 1 nodes),
    // the centroids, triangleIndices and owners (double-buffered: a level's partition writes the next level's), `remain`, the triangles' objIdx, the two scan arrays,
    // the chunk sums and one level's bins — grown on demand and kept between calls; one read-back (host wait) per level, and the read-back of the new records
    struct BvhBuild : AccelBuild {
        crt::BvhBuildState* dState = nullptr; crt::BvhBuildState* hState = nullptr;
        static constexpr int kBufs = 13;      // nodes, keys, cen, idx x 2, owner x 2, remain, objOf, leftItems, nodeItems, chunks, bins
        void* buf[kBufs] = {}; size_t cap[kBufs] = {};
        uint32_t waits = 0, levels = 0; double waitMs = 0, readBackMs = 0;      // the last call's host waits per level, its levels, the waits' wall time, the mirror read-back's
        void release() { releaseEvents(); for (void* p : buf) (void)hipFree(p); (void)hipFree(dState); (void)hipHostFree(hState); *this = BvhBuild{}; }
    } bvhBuild;
    uint32_t kdNodeCount = 0, kdRefCount = 0;   // nodes / leaf references of the FileScene's live KD-tree (uploaded or built on the device)
    // The two-level KD [0] / grid [1] set as the device holds it, uploaded or rebuilt per BLAS: the descriptors; per BLAS the elements of its part of the kind's two
    // arrays (count[0]: KD nodes / cells + 1, count[1]: KD / cell references) and its height (KD only); and whether BLAS i's part is of its current vertices (an
    // upload sets all, CRT_UPDATE_BOUNDS clears all, crt_refit_device clears its BLAS's, the kind's device build sets its BLAS's): the set is live (haveBlas[k]) iff
    // every flag is set.  Kept while the set is dropped: the buffers are still held (`held`), and a rebuild carries the other BLASes' parts over.
    struct BlasSet {
        std::vector<crt::BlasAltDesc> desc; std::vector<uint32_t> count[2], height; std::vector<uint8_t> current; bool held = false;
        void stale(uint32_t bvh) { if (bvh < current.size()) current[bvh] = 0; }
        bool allCurrent() const { for (uint8_t k : current) if (!k) return false; return true; }
    } blasSet[2];
    hipEvent_t altReady = nullptr;        // recorded behind the last crt_upload_alt_accel's copies (device queries on other streams wait for it)
    // Latency mode of single-window launches (render_tiles_kernel's block table), driven by measurement — see next_block_table.  Stage 0 = the table solved from the cost probe's
    // estimates (one wavefront per tile when there was no probe); stages 1 .. kLatStages = tables solved from the tile costs the stage before measured; afterwards the fastest stage is used
    // (HIP event durations of the launches themselves; identical pixels whatever the table).
    static constexpr int kLatStages = 4;       // (round 3: the stages are solved, not stepped, and agree within launch-to-launch scatter from stage 1 on; round 2's stepping tuner needed 6)
    double tuneMs[kLatStages + 1] = {}; int tuneCount[kLatStages + 1] = {};
    hipEvent_t lastRenderEnd = nullptr;   // end event of the most recent render launch (owned by the timing lists)
    int latStage = 0;              // stage of the table on the device (0: none yet)
    int latBest = 0;               // fastest stage so far
    bool latDone = false;          // all stages measured, the fastest one's table is (being) installed
    bool latConfirming = false; std::vector<int> latQueue;      // after the last stage: the two fastest stages are timed once more
    bool latWarm = false;          // stage 0 has been measured once already (the first launch after an upload runs cold: it is measured twice)
    uint32_t latSlots = 0;         // wavefronts of render_tiles_kernel the device holds at once (0: not asked yet)
    bool latProbed = false;        // the cost probe has run for this camera / scene: stage 0 is a block table built from its estimates (latL[0]), not one wavefront per tile
    std::vector<uint8_t> latL[kLatStages + 1];          // lanes per wavefront of every tile, per stage ([0]: all 64)
    std::vector<uint32_t> latCost[kLatStages + 1];      // measured tile costs, per stage
    uint32_t* dTileCost = nullptr; uint32_t* hTileCost = nullptr; hipEvent_t costCopied = nullptr; bool costPending = false; int costStage = 0;
    uint32_t* dBlockDesc = nullptr; uint32_t* hBlockDesc = nullptr; uint32_t nBlocks = 0, descCap = 0; hipEvent_t descReady = nullptr;   // the table of render_tiles_kernel
    // Jobs (launches of several windows): what each tile costs is measured once per camera / scene by the first job launch (every wavefront's duration, scaled to
    // 64 streams); later launches dispatch the tiles most expensive first and SPLIT: see split_point
    uint32_t* dJobCost = nullptr; uint32_t* hJobCost = nullptr; hipEvent_t jobCostCopied = nullptr; bool jobCostPending = false, jobCostValid = false;
    uint32_t recWaves = 0, recResident = 0, recWindows = 0; bool recPool = false;     // the measuring launch: wavefronts, how many the chip holds, windows, kernel
    double poolWindowTicks = 0;             // machine time of ONE window of this image under the pool, 100 MHz ticks (0: unknown)
    std::vector<uint32_t> jobCost;          // per local tile, 100 MHz ticks; sorted view = the tile order on the device once jobCostValid
    std::vector<uint32_t> jobOrder;
    uint32_t* dJobDesc = nullptr; uint32_t* hJobDesc = nullptr; uint32_t jobDescCap = 0, jobBlocks = 0, jobHead = 0; hipEvent_t jobDescReady = nullptr;
    uint32_t planWindows = 0, planFrames = 0, planSky = 0, planSkyAsked = 0; bool planPool = false, planValid = false;       // what the table on the device was planned for (planSky: sky ranks left out)
    double jobTrialMs[2] = {0, 0};          // this plan's shape timed [0] plain (cost-ordered, no table) and [1] planned: the faster one is kept (planner_prepare)
    // the plan's pool launch: frames per wavefront by tile rank (pool_wave_plan), behind the block table in dJobDesc — jobWaveBlocks wavefronts (0: every wavefront S frames,
    // no table), jobLongWaves of them with more than S frames; lastLongWaves: what the last pool launch had of those (crt_debug_pool_long_waves)
    uint32_t jobWaveOff = 0, jobWaveBlocks = 0, jobLongFrames = 0, jobLongWaves = 0, lastLongWaves = 0;
    std::vector<hipEvent_t> splitEvents;    // end events of the second kernel of split launches (recycled round-robin)
    size_t splitSeq = 0; uint32_t splitLaunches = 0;
    uint64_t poolMinWaves = 65000; // launches of fewer (tile, 64-frame window) pairs run render_tiles_kernel: see crt_render
    bool usePool = true;          // render_pool_kernel (stream pool); CRT_RENDER_KERNEL=tiles selects render_tiles_kernel (one stream per lane)
    uint32_t ldsBytes = 0;
    uint32_t extraLds = 0;        // CRT_DEBUG_EXTRA_LDS: unused LDS bytes per wavefront (part of ldsBytes; the pool launch adds it to its own need)
    uint32_t poolLdsLimit = 0;    // crt_pool_lds_limit of the device (0: not asked yet)
    // timing of the last crt_render
    std::vector<EventPair> evPool; size_t evUsedRender = 0, evUsedAcc = 0;
    std::deque<EventPair> evRender, evAcc;                        // launches not yet folded into the totals below (oldest first)
    double foldedRenderMs = 0, foldedAccMs = 0; uint32_t foldedLaunches = 0, poolLaunches = 0;

    int fail(int code, const char* fmt, ...)
    {
        char buf[1024];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
        err = buf; return code;
    }
    int hip(hipError_t e, const char* what)
    {
        if (e == hipSuccess) return 0;
        (void)hipGetLastError();          // the runtime keeps a failed call's code until it is read: a launch wrapper's hipGetLastError() of a LATER call must not find it
        return fail(CRT_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
    }
    void freeAlt()
    {
        for (auto& v : altAllocs) { for (void* p : v) (void)hipFree(p); v.clear(); }
        if (altTris) (void)hipFree(altTris);
        altTris = nullptr; altTriCount = 0; haveKd = haveGrid = false; alt = crt::AltAccelDev{}; renderAccel = 0;
        for (int k = 0; k < 2; k++) { for (void* p : blasAllocs[k]) (void)hipFree(p); blasAllocs[k].clear(); haveBlas[k] = false; blasAlt[k] = crt::TlasAltDev{}; }
        for (BlasSet& b : blasSet) b = BlasSet{};
        gridRefCount = 0; kdNodeCount = kdRefCount = 0;
        freeRetired(true);                // the callers have drained every stream
    }
    void freeRetired(bool all)
    {
        while (!retired.empty()) {
            Retired& r = retired.front();
            if (!all && hipEventQuery(r.unread) != hipSuccess) { (void)hipGetLastError(); break; }     // oldest first: the events complete in order on the main stream
            for (void* p : r.ptrs) (void)hipFree(p);
            if (r.pinned) (void)hipHostFree(r.pinned);
            retiredEvents.push_back(r.unread); retired.pop_front();
        }
    }
    void freeScene()
    {
        for (void* p : sceneAllocs) (void)hipFree(p);
        sceneAllocs.clear(); haveScene = false; dRootBox = nullptr; dTex = nullptr;
        for (void* p : refitAllocs) (void)hipFree(p);
        refitAllocs.clear(); refitPlans.clear();
        if (dPrimTex) { (void)hipFree(dPrimTex); dPrimTex = nullptr; }
        havePrim = false;
        freeAlt();                        // the alternative accelerators index the scene's triangles
    }
};

#define HIPCK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (ctx)->hip(e_, #call); } while (0)

namespace {

template <class T>
int upload(crt_ctx* c, const std::vector<T>& v, const T** out)
{
    *out = nullptr;
    if (v.empty()) return 0;
    void* d = nullptr;
    HIPCK(c, hipMalloc(&d, v.size() * sizeof(T)));
    c->sceneAllocs.push_back(d);
    HIPCK(c, hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));   // v is a temporary of the caller
    *out = reinterpret_cast<const T*>(d);
    return 0;
}

// one array of an accelerator: a device allocation of its own, noted in `allocs`, filled by a synchronous copy; *out = the view's typed pointer (null: empty array)
template <class T>
int upload_array(crt_ctx* c, std::vector<void*>& allocs, const void* src, size_t bytes, const T** out)
{
    *out = nullptr; if (!bytes) return 0;
    void* d = nullptr; HIPCK(c, hipMalloc(&d, bytes)); allocs.push_back(d);
    HIPCK(c, hipMemcpy(d, src, bytes, hipMemcpyHostToDevice)); *out = static_cast<const T*>(d); return 0;
}

// height of the tree below node 0 in pushes: the ordered traversal pushes at most one sibling per interior level
int bvh_height(crt_ctx* c, const crt_bvh& b, uint32_t* heightOut)
{
    std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u});
    uint32_t h = 0; size_t visited = 0;
    while (!st.empty()) {
        auto [n, d] = st.back(); st.pop_back();
        if (++visited > (size_t)b.nodesUsed) return c->fail(CRT_ERR_INVALID, "BVH node graph is not a tree");
        const crt_bvh_node& nd = b.nodes[n];
        if (nd.triCount > 0) { if (d > h) h = d; continue; }
        if (nd.leftFirst == 0 || nd.leftFirst + 1 >= b.nodesUsed) return c->fail(CRT_ERR_INVALID, "BVH child index out of range (node %u)", n);
        st.push_back({nd.leftFirst, d + 1}); st.push_back({nd.leftFirst + 1, d + 1});
    }
    *heightOut = h;
    return 0;
}

// device queries on callers' streams that may still read the scene / accelerator buffers: the host waits for them (before buffers are freed or rewritten
// by a synchronous copy); an in-place write makes the main stream wait instead (order_behind_queries)
int wait_queries(crt_ctx* c)
{
    for (auto& q : c->qslot) if (q.pending) { HIPCK(c, hipEventSynchronize(q.done)); q.pending = false; }
    return 0;
}

// an event field that is created by its first use
hipError_t ensure_event(hipEvent_t* e, unsigned flags = hipEventDisableTiming) { return *e ? hipSuccess : hipEventCreateWithFlags(e, flags); }

// before the scene's or an accelerator set's buffers are freed: every launch that may still read them has finished (render streams first: the main stream's accumulates wait on them)
int drain_all(crt_ctx* c)
{
    for (auto st : c->streams) HIPCK(c, hipStreamSynchronize(st));
    if (c->aheadStream) HIPCK(c, hipStreamSynchronize(c->aheadStream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return wait_queries(c);
}

} // namespace

extern "C" {

int crt_abi_version(void) { return CRT_ABI_VERSION; }

void crt_debug_enable_hooks(int on) { g_hooks = on != 0; }

// Every write of a context's camera-relative block goes through here: what a tile's primary rays can hit depends on exactly the values set_primary reads (camera,
// light / floor block, root pair), so the tile classes are stale from the same moment.
static void primary_changed(crt_ctx* c) { crt::set_primary(c->hScene); c->classDirty = true; }

int crt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* crt_last_error(crt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int crt_create(crt_ctx** out, const crt_config* cfg)
{
    if (!out || !cfg) { g_createError = "crt_create: null argument"; return CRT_ERR_INVALID; }
    *out = nullptr;
    // independent launches overlap on several HIP streams; ROCm multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues
    // (default 4) and serialises kernels that share one.  Only effective when the HIP runtime has not initialised yet
    // (a host that already uses HIP sets the variable itself); never overrides the user's value.
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    if (cfg->width < 16 || cfg->height < 16) { g_createError = "crt_create: width and height must be at least one 16x16 tile"; return CRT_ERR_INVALID; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_createError = "crt_create: no HIP device visible (this library has no CPU path)";
        return CRT_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_createError = "crt_create: device ordinal out of range"; return CRT_ERR_INVALID; }
    crt_ctx* c = new crt_ctx();
    c->cfg = *cfg;
    if (const char* k = hook("CRT_RENDER_KERNEL")) {             // tests / A-B runs: "tiles" = never the stream pool, "pool_always" = also for launches of <= 64 frames
        c->usePool = strcmp(k, "tiles") != 0;
        if (!strcmp(k, "pool_always")) c->poolMinWaves = 0;
    }
    if (c->cfg.depthLimit < 0) c->cfg.depthLimit = 5;
    if (c->cfg.depthLimit > 5) { g_createError = "crt_create: depthLimit > 5 unsupported (throughput stack holds 5 factors; reference default is 5)"; delete c; return CRT_ERR_UNSUPPORTED; }
    if (c->cfg.maxFramesPerLaunch <= 0) c->cfg.maxFramesPerLaunch = c->cfg.collectStats ? 64 : 4096;   // 64 windows of 64 frames; per-tile clocks of a statistics context describe ONE window
    if (c->cfg.maxFramesPerLaunch > 64) c->cfg.maxFramesPerLaunch = c->cfg.maxFramesPerLaunch / 64 * 64;   // whole windows (< 64: one partial window per launch)
    if (c->cfg.renderStreams < 0) c->cfg.renderStreams = 0;
    c->tilesX = cfg->width / 16; c->tilesY = cfg->height / 16;      // truncating, as renderer.cpp:151
    const int tiles = c->tilesX * c->tilesY;
    int first = cfg->tileFirst, stride = cfg->tileStride <= 0 ? 1 : cfg->tileStride, count = cfg->tileCount;
    if (count < 0) { first = 0; stride = 1; count = tiles; }
    if (first < 0 || (count > 0 && (long long)first + (long long)(count - 1) * stride >= tiles)) {
        g_createError = "crt_create: tile range exceeds the image"; delete c; return CRT_ERR_INVALID;
    }
    c->tileFirst = (uint32_t)first; c->tileStride = (uint32_t)stride; c->tileCount = (uint32_t)count;

    auto bail = [&](hipError_t he, const char* what) {
        g_createError = std::string("crt_create: ") + what + ": " + hipGetErrorString(he);
        crt_destroy(c); return CRT_ERR_DEVICE;
    };
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    const size_t px = (size_t)cfg->width * cfg->height;
    if ((e = hipMalloc(&c->dAccOwned, px * 16)) != hipSuccess) return bail(e, "hipMalloc(accumulator)");
    c->dAcc = c->dAccOwned;
    if ((e = hipMemsetAsync(c->dAcc, 0, px * 16, c->stream)) != hipSuccess) return bail(e, "hipMemset(accumulator)");
    if ((e = hipMalloc((void**)&c->dPixels, px * 4)) != hipSuccess) return bail(e, "hipMalloc(pixels)");
    if ((e = hipMemsetAsync(c->dPixels, 0, px * 4, c->stream)) != hipSuccess) return bail(e, "hipMemset(pixels)");
    if ((e = hipMalloc((void**)&c->dTileSums, (size_t)tiles * 4)) != hipSuccess) return bail(e, "hipMalloc(tileSums)");
    if ((e = hipMemsetAsync(c->dTileSums, 0, (size_t)tiles * 4, c->stream)) != hipSuccess) return bail(e, "hipMemset(tileSums)");
    if ((e = hipMalloc((void**)&c->dCounters, sizeof(crt::Counters))) != hipSuccess) return bail(e, "hipMalloc(counters)");
    if ((e = hipMemsetAsync(c->dCounters, 0, sizeof(crt::Counters), c->stream)) != hipSuccess) return bail(e, "hipMemset(counters)");
    if ((e = hipMalloc((void**)&c->dQueryCursor, 64)) != hipSuccess) return bail(e, "hipMalloc(query cursor)");
    if ((e = hipMalloc((void**)&c->dQuerySlots, crt_ctx::kQuerySlots * 64)) != hipSuccess) return bail(e, "hipMalloc(query cursor slots)");
    if (c->cfg.collectStats && count > 0) {
        if ((e = hipMalloc((void**)&c->dTileClocks, (size_t)count * 144)) != hipSuccess) return bail(e, "hipMalloc(tileClocks)");
        if ((e = hipMemsetAsync(c->dTileClocks, 0, (size_t)count * 144, c->stream)) != hipSuccess) return bail(e, "hipMemset(tileClocks)");
    }
    // Camera() defaults, template/camera.h:14-22
    memset(&c->hScene, 0, sizeof(c->hScene));
    const float aspect = (float)cfg->width / (float)cfg->height;
    crt::Scene& s = c->hScene;
    s.camPos[0] = 0; s.camPos[1] = 0; s.camPos[2] = -2;
    s.topLeft[0] = -aspect; s.topLeft[1] = 1; s.topLeft[2] = 0;
    s.topRight[0] = aspect; s.topRight[1] = 1; s.topRight[2] = 0;
    s.bottomLeft[0] = -aspect; s.bottomLeft[1] = -1; s.bottomLeft[2] = 0;
    s.W = cfg->width; s.H = cfg->height; s.invW = 1.0f / cfg->width; s.invH = 1.0f / cfg->height;
    s.depthLimit = c->cfg.depthLimit;
    primary_changed(c);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    *out = c;
    return CRT_OK;
}

void crt_destroy(crt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    for (auto st : c->streams) (void)hipStreamSynchronize(st);
    if (c->aheadStream) (void)hipStreamSynchronize(c->aheadStream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& q : c->qslot) if (q.done) { if (q.pending) (void)hipEventSynchronize(q.done); (void)hipEventDestroy(q.done); }   // device queries on callers' streams
    if (c->dQuerySlots) (void)hipFree(c->dQuerySlots);
    if (c->viewsDone) { if (c->viewsPending) (void)hipEventSynchronize(c->viewsDone); (void)hipEventDestroy(c->viewsDone); }
    if (c->dViewsSlab) (void)hipFree(c->dViewsSlab);
    if (c->poseBack) (void)hipEventDestroy(c->poseBack);
    if (c->dPoseTable) (void)hipFree(c->dPoseTable);
    if (c->hPoseBack) (void)hipHostFree(c->hPoseBack);
    if (c->altReady) (void)hipEventDestroy(c->altReady);
    if (c->writeFence) (void)hipEventDestroy(c->writeFence);
    c->refit.release(); c->tlasBuild.release();
    c->freeScene();
    c->gridBuild.release();
    c->kdBuild.release();
    c->bvhBuild.release();
    for (hipEvent_t e : c->retiredEvents) (void)hipEventDestroy(e);
    for (auto& a : c->ahead) (void)hipEventDestroy(a.end);
    if (c->aheadStream) (void)hipStreamDestroy(c->aheadStream);
    if (c->skyStream) (void)hipStreamDestroy(c->skyStream);          // (every sky launch was joined into a render stream: nothing of its own to wait for)
    for (auto& ev : c->evPool) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto& ev : c->evRender) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto& ev : c->evAcc) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    if (c->dAccOwned) (void)hipFree(c->dAccOwned);
    for (auto st : c->streams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (auto& r : c->inflight) (void)hipEventDestroy(r.freed);
    for (auto e : c->freeEvents) (void)hipEventDestroy(e);
    if (c->mustWait) (void)hipEventDestroy(c->mustWait);
    if (c->pool) (void)hipFree(c->pool);
    for (auto e : c->doneEvents) (void)hipEventDestroy(e);
    if (c->dPixels) (void)hipFree(c->dPixels);
    if (c->dTileSums) (void)hipFree(c->dTileSums);
    if (c->dCounters) (void)hipFree(c->dCounters);
    if (c->dQueryCursor) (void)hipFree(c->dQueryCursor);
    if (c->dInspectCounts) (void)hipFree(c->dInspectCounts);
    if (c->dInspectWork) (void)hipFree(c->dInspectWork);
    if (c->dTileClocks) (void)hipFree(c->dTileClocks);
    if (c->dTileOrder) (void)hipFree(c->dTileOrder);
    if (c->dTileClass) (void)hipFree(c->dTileClass);
    if (c->dTileCost) (void)hipFree(c->dTileCost);
    if (c->dJobCost) (void)hipFree(c->dJobCost);
    if (c->dJobDesc) (void)hipFree(c->dJobDesc);
    if (c->hJobDesc) (void)hipHostFree(c->hJobDesc);
    if (c->jobDescReady) (void)hipEventDestroy(c->jobDescReady);
    if (c->hJobCost) (void)hipHostFree(c->hJobCost);
    if (c->jobCostCopied) (void)hipEventDestroy(c->jobCostCopied);
    for (auto e : c->splitEvents) (void)hipEventDestroy(e);
    if (c->hTileCost) (void)hipHostFree(c->hTileCost);
    if (c->costCopied) (void)hipEventDestroy(c->costCopied);
    if (c->dBlockDesc) (void)hipFree(c->dBlockDesc);
    if (c->hBlockDesc) (void)hipHostFree(c->hBlockDesc);
    if (c->descReady) (void)hipEventDestroy(c->descReady);
    if (c->dStage) (void)hipFree(c->dStage);
    for (int k = 0; k < 2; k++) { if (c->hTileOrder[k]) (void)hipHostFree(c->hTileOrder[k]); if (c->orderCopied[k]) (void)hipEventDestroy(c->orderCopied[k]); }
    for (int k = 0; k < 2; k++) { if (c->hTileClass[k]) (void)hipHostFree(c->hTileClass[k]); if (c->classCopied[k]) (void)hipEventDestroy(c->classCopied[k]); }
    for (int k = 0; k < 2; k++) { if (c->hStage[k]) (void)hipHostFree(c->hStage[k]); if (c->stageCopied[k]) (void)hipEventDestroy(c->stageCopied[k]); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The light block of a Scene from a description's (or a look's) lightT / lightInvT / lightSize: the one writer, for crt_upload_scene and crt_update_look, so the two
// cannot differ by a bit.
static void set_light_block(crt::Scene& s, const float* lightT, const float* lightInvT, float lightSize)
{
    memcpy(s.lightInvT, lightInvT, 48);
    s.lightNrm[0] = -lightT[1]; s.lightNrm[1] = -lightT[5]; s.lightNrm[2] = -lightT[9];   // Quad::GetNormal, primitives.h:363-367
    s.lightSize = lightSize;
    {   // GetLightPos (file_scene.cpp:156-162): middle of the quad's two corners, 0.01 below; scalar TransformPosition order
        const float* m = lightT;
        const float ax = -0.5f, ay = 0.0f, az = -0.5f, bx = 0.5f, by = 0.0f, bz = 0.5f;
        const float c1[3] = {m[0] * ax + m[1] * ay + m[2] * az + m[3] * 1.0f, m[4] * ax + m[5] * ay + m[6] * az + m[7] * 1.0f, m[8] * ax + m[9] * ay + m[10] * az + m[11] * 1.0f};
        const float c2[3] = {m[0] * bx + m[1] * by + m[2] * bz + m[3] * 1.0f, m[4] * bx + m[5] * by + m[6] * bz + m[7] * 1.0f, m[8] * bx + m[9] * by + m[10] * bz + m[11] * 1.0f};
        s.lightPos[0] = (c1[0] + c2[0]) * 0.5f - 0.0f; s.lightPos[1] = (c1[1] + c2[1]) * 0.5f - 0.01f; s.lightPos[2] = (c1[2] + c2[2]) * 0.5f - 0.0f;
    }
    // what FileScene / TLASFileScene always build: a translated, unrotated quad
    const float* m = lightInvT;
    s.lightAxis = (m[0] == 1.0f && m[1] == 0.0f && m[2] == 0.0f && m[4] == 0.0f && m[5] == 1.0f && m[6] == 0.0f && m[8] == 0.0f && m[9] == 0.0f && m[10] == 1.0f) ? 1u : 0u;
    if (hook("CRT_DEBUG_GENERAL_PRIMS")) s.lightAxis = 0u;                        // tests: the general quad expressions on the standard scenes
}

int crt_upload_scene(crt_ctx* c, const crt_scene_desc* sd)
{
    if (!c || !sd) return CRT_ERR_INVALID;
    c->epoch++;                                                       // frames rendered ahead by crt_tick are of the old scene
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (sd->kind != CRT_SCENE_FILE && sd->kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_INVALID, "unknown scene kind %d", sd->kind);
    if (!sd->bvhs || sd->bvhCount == 0) return c->fail(CRT_ERR_INVALID, "scene has no acceleration structure");
    if (sd->kind == CRT_SCENE_FILE && sd->bvhCount != 1) return c->fail(CRT_ERR_INVALID, "CRT_SCENE_FILE takes exactly one BVH (FileScene::acc)");
    if (sd->kind == CRT_SCENE_TLAS && (sd->bvhCount > 256 || !sd->tlasNodes || sd->tlasNodeCount < 2 * sd->bvhCount))
        return c->fail(CRT_ERR_INVALID, "TLAS scene needs <= 256 BLAS (tlas_bvh.cpp:21) and 2*blasCount TLAS nodes");
    if (sd->textureCount == 0 || !sd->textures) return c->fail(CRT_ERR_INVALID, "floor and skydome textures are required");
    if (sd->floorTexture < 0 || sd->floorTexture >= (int)sd->textureCount || sd->skyTexture < 0 || sd->skyTexture >= (int)sd->textureCount)
        return c->fail(CRT_ERR_INVALID, "floor/sky texture index out of range");
    for (uint32_t i = 0; i < sd->textureCount; i++)
        if (!sd->textures[i].pixels || sd->textures[i].width <= 0 || sd->textures[i].height <= 0) return c->fail(CRT_ERR_INVALID, "texture %u is empty", i);
    if (sd->materialCount > 0 && !sd->materials) return c->fail(CRT_ERR_INVALID, "materialCount is %u but materials is NULL", sd->materialCount);
    for (uint32_t i = 0; i < sd->materialCount; i++)
        if (sd->materials[i].texture >= (int)sd->textureCount) return c->fail(CRT_ERR_INVALID, "material %u: texture index out of range", i);
    if (sd->kind == CRT_SCENE_FILE) {
        if (!sd->objMatIdx || sd->objCount == 0) return c->fail(CRT_ERR_INVALID, "CRT_SCENE_FILE needs objMatIdx");
        for (uint32_t i = 0; i < sd->objCount; i++)
            if (sd->objMatIdx[i] < 0 || sd->objMatIdx[i] >= (int)sd->materialCount) return c->fail(CRT_ERR_INVALID, "objMatIdx entry out of range");
    }

    // ---- sizes of the sections of the geometry buffer: pairs | leaf tris (+1 pad record) | TLAS nodes | instances | shade records ----
    uint64_t nPairs = 0, nTris = 0;
    uint32_t maxHeight = 0; std::vector<uint32_t> heights;
    for (uint32_t bi = 0; bi < sd->bvhCount; bi++) {
        const crt_bvh& b = sd->bvhs[bi];
        if (!b.nodes || !b.triangles || !b.triangleIndices || b.nodesUsed == 0 || b.triCount == 0) return c->fail(CRT_ERR_INVALID, "BVH %u is empty", bi);
        if ((b.nodesUsed & 1u) == 0) return c->fail(CRT_ERR_INVALID, "BVH %u: nodesUsed must be odd (root + child pairs)", bi);
        if (sd->kind == CRT_SCENE_TLAS && (b.matIdx < 0 || b.matIdx >= (int)sd->materialCount)) return c->fail(CRT_ERR_INVALID, "BLAS %u: matIdx out of range", bi);
        if (sd->kind == CRT_SCENE_TLAS && b.objIdx != (int)bi + 2)
            return c->fail(CRT_ERR_INVALID, "BLAS %u: objIdx must be %u (TLASFileScene numbers objects from 2, tlas_file_scene.cpp:13,51-53)", bi, bi + 2);
        uint32_t h = 0; int r = bvh_height(c, b, &h); if (r) return r;
        if (h > maxHeight) maxHeight = h;
        heights.push_back(h);
        nPairs += b.nodesUsed / 2; nTris += b.triCount;
    }
    const uint64_t pairBytes = nPairs ? nPairs * 64 : 64;                   // offset 0 must never be a leaf record (ref 0 = "done")
    const uint64_t leafOffB = pairBytes, leafBytes = (nTris + 1) * 48;       // +1: record fetches read 64 B from a 48-B LeafTri
    const uint64_t tlasOffB = (leafOffB + leafBytes + 63) & ~63ull;
    const uint64_t tlasBytes = (sd->kind == CRT_SCENE_TLAS) ? (uint64_t)sd->tlasNodeCount * 32 : 0;
    const uint64_t tlasPairOffB = (tlasOffB + tlasBytes + 63) & ~63ull;      // one NodePair-shaped record per TLAS interior node (at most tlasNodeCount / 2)
    const uint64_t tlasPairBytes = (sd->kind == CRT_SCENE_TLAS) ? (uint64_t)sd->tlasNodeCount * 32 : 0;
    const uint64_t instOffB = (tlasPairOffB + tlasPairBytes + 127) & ~127ull;
    const uint64_t instBytes = (sd->kind == CRT_SCENE_TLAS) ? (uint64_t)sd->bvhCount * 128 : 0;
    const uint64_t shadeOffB = (instOffB + instBytes + 63) & ~63ull;
    const uint64_t total = shadeOffB + nTris * 64;
    if (total >= crt::kMaxGeomBytes) return c->fail(CRT_ERR_UNSUPPORTED, "scene geometry needs %llu bytes; this build addresses 4 GiB", (unsigned long long)total);
    if (sd->kind == CRT_SCENE_TLAS && sd->tlasNodeCount > 0x7fffu) return c->fail(CRT_ERR_UNSUPPORTED, "TLAS node index exceeds 15 bits");

    std::vector<char> geom((size_t)total, 0);
    crt::NodePair* pairs = reinterpret_cast<crt::NodePair*>(geom.data());
    crt::LeafTri* leaf = reinterpret_cast<crt::LeafTri*>(geom.data() + leafOffB);
    crt::TlasNode* tlas = reinterpret_cast<crt::TlasNode*>(geom.data() + tlasOffB);
    crt::NodePair* tlasPairs = reinterpret_cast<crt::NodePair*>(geom.data() + tlasPairOffB);
    // The width the scene's pool references are written in (layout.h): 16 bits where every index fits, else 32 — whose index limit is what kMaxGeomBytes imposes
    // on the records anyway (index * 64 and leafOff + index * 48 below 2^32), checked here all the same; a scene beyond it has no pool form (render_tiles_kernel).
    const bool ref16ok = nPairs <= crt::kRef16MaxIndex && nTris <= crt::kRef16MaxIndex && !hook("CRT_DEBUG_NO_REF16");   // (tests: a scene that fits, treated as one that does not)
    const bool refWideOk = nPairs <= crt::kRefWideMaxIndex && nTris < crt::kRefWideMaxIndex && nPairs * 64 < crt::kMaxGeomBytes && leafOffB + nTris * 48 < crt::kMaxGeomBytes;
    const uint32_t poolRefBits = ref16ok ? 16u : (refWideOk ? 32u : 0u);
    const crt::PoolRefForm PR = crt::pool_ref_form(poolRefBits);
    crt::Instance* inst = reinterpret_cast<crt::Instance*>(geom.data() + instOffB);
    crt::ShadeTri* shade = reinterpret_cast<crt::ShadeTri*>(geom.data() + shadeOffB);

    uint64_t pairBase = 0, triBase = 0; uint32_t rootRef0 = 0, rootRef0_16 = 0;
    for (uint32_t bi = 0; bi < sd->bvhCount; bi++) {
        const crt_bvh& b = sd->bvhs[bi];
        // packed reference of node n (layout.h): interior -> offset of its child pair, leaf -> offset of its first LeafTri, both in 16-byte units
        auto ref_of = [&](uint32_t n, uint32_t* ref) -> int {
            const crt_bvh_node& nd = b.nodes[n];
            if (nd.triCount > 0) {
                if ((uint64_t)nd.leftFirst + nd.triCount > b.triCount) return c->fail(CRT_ERR_INVALID, "leaf range out of bounds (BVH %u node %u)", bi, n);
                *ref = (uint32_t)((leafOffB + (triBase + nd.leftFirst) * 48) >> 4);
            } else {
                if ((nd.leftFirst & 1u) == 0) return c->fail(CRT_ERR_INVALID, "interior node %u: children must be allocated pairwise starting at an odd index", n);
                *ref = crt::kRefInterior | (uint32_t)(((pairBase + ((nd.leftFirst - 1u) >> 1)) * 64) >> 4);
            }
            return 0;
        };
        // the same reference in the pool form (layout.h), in the scene's width: record INDEX instead of offset; only meaningful when poolRefBits != 0
        auto ref16_of = [&](uint32_t n) -> uint32_t {
            const crt_bvh_node& nd = b.nodes[n];
            if (nd.triCount > 0) return (uint32_t)((triBase + nd.leftFirst + 1) & PR.indexMask);
            return PR.interior | (uint32_t)((pairBase + ((nd.leftFirst - 1u) >> 1)) & PR.indexMask);
        };
        int r;
        for (uint32_t n = 1; n + 1 < b.nodesUsed; n += 2) {
            crt::NodePair& p = pairs[pairBase + ((n - 1) >> 1)];
            for (int k = 0; k < 2; k++) {
                const crt_bvh_node& nd = b.nodes[n + k];
                memcpy(p.c[k].lo, nd.aabbMin, 12); memcpy(p.c[k].hi, nd.aabbMax, 12);
                if ((r = ref_of(n + k, &p.c[k].ref))) return r;
                p.c[k].ref16 = ref16_of(n + k);
            }
        }
        uint32_t rootRef = 0; if ((r = ref_of(0, &rootRef))) return r;
        const uint32_t rootRef16 = ref16_of(0);
        // `remain` of every leaf slot: triangles left in its leaf including itself
        std::vector<uint32_t> remain(b.triCount, 1u);
        for (uint32_t n = 0; n < b.nodesUsed; n++) {
            const crt_bvh_node& nd = b.nodes[n];
            if (nd.triCount == 0) continue;
            for (uint32_t i = 0; i < nd.triCount; i++) remain[nd.leftFirst + i] = nd.triCount - i;
        }
        for (uint32_t j = 0; j < b.triCount; j++) {                       // leaf order: triangleIndices resolved here
            const uint32_t ti = b.triangleIndices[j];
            if (ti >= b.triCount) return c->fail(CRT_ERR_INVALID, "BVH %u: triangleIndices[%u] out of range", bi, j);
            const crt_tri& t = b.triangles[ti];
            crt::LeafTri& lt = leaf[triBase + j];
            for (int k = 0; k < 3; k++) { lt.v0[k] = t.vertex0[k]; lt.e1[k] = t.vertex1[k] - t.vertex0[k]; lt.e2[k] = t.vertex2[k] - t.vertex0[k]; }
            lt.shadeIdx = (uint32_t)(triBase + ti);
            lt.objIdx = (sd->kind == CRT_SCENE_TLAS) ? b.objIdx : t.objIdx;
            lt.remain = remain[j];
            if (sd->kind == CRT_SCENE_FILE && (t.objIdx < 2 || (uint32_t)(t.objIdx - 2) >= sd->objCount))
                return c->fail(CRT_ERR_INVALID, "triangle %u: objIdx %d has no entry in objMatIdx", ti, t.objIdx);
        }
        for (uint32_t ti = 0; ti < b.triCount; ti++) {                    // shading records in the reference's triIdx order
            const crt_tri& t = b.triangles[ti];
            if (sd->kind == CRT_SCENE_FILE && (t.objIdx < 2 || (uint32_t)(t.objIdx - 2) >= sd->objCount))   // every triangle, not only those triangleIndices reaches
                return c->fail(CRT_ERR_INVALID, "triangle %u: objIdx %d has no entry in objMatIdx", ti, t.objIdx);
            crt::ShadeTri& s = shade[triBase + ti];
            memcpy(s.n0, t.normal0, 12); memcpy(s.n1, t.normal1, 12); memcpy(s.n2, t.normal2, 12);
            memcpy(s.uv0, t.uv0, 8); memcpy(s.uv1, t.uv1, 8); memcpy(s.uv2, t.uv2, 8);
            // materials[models[tri.objIdx - 2]->matIdx] (file_scene.cpp:207) / materials[blas->matIdx] (tlas_file_scene.cpp:240); +2: [0] light, [1] floor
            s.mat = 2 + ((sd->kind == CRT_SCENE_TLAS) ? b.matIdx : sd->objMatIdx[t.objIdx - 2]);
        }
        if (sd->kind == CRT_SCENE_TLAS) {
            crt::Instance& in = inst[bi];
            memcpy(in.invT, b.invT, 48); memcpy(in.T, b.T, 48);
            in.shadeBase = (uint32_t)triBase; in.rootRef16 = rootRef16; in.rootRef = rootRef; in.objIdx = b.objIdx; in.triCount = b.triCount;
        } else { rootRef0 = rootRef; rootRef0_16 = rootRef16; }
        pairBase += b.nodesUsed / 2; triBase += b.triCount;
    }
    leaf[nTris].remain = 1;                                                 // pad record
    uint32_t tlasHeight = 0, tlasRoot = 0, tlasRoot16 = 0;
    if (sd->kind == CRT_SCENE_TLAS) {
        uint32_t nTlasPairs = 0;
        for (uint32_t i = 0; i < sd->tlasNodeCount; i++) {      // device copy carries each node's packed reference instead of leftRight / BLAS
            const crt_tlas_node& nd = sd->tlasNodes[i];
            memcpy(tlas[i].lo, nd.aabbMin, 12); memcpy(tlas[i].hi, nd.aabbMax, 12);
            tlas[i].ref = nd.leftRight ? (crt::kRefTlasInterior | (nd.leftRight & 0x7fffu) | (((nd.leftRight >> 16) & 0x7fffu) << 15))
                                       : (crt::kRefTlasLeaf | (nd.BLAS & 0xffffu));
            tlas[i].ref16 = nd.leftRight ? (PR.tlasBit | nTlasPairs++) : (PR.tlasLeaf | (nd.BLAS & PR.indexMask));   // interior nodes number their child pairs
        }
        std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u}); size_t visited = 0;
        while (!st.empty()) {
            auto [n, d] = st.back(); st.pop_back();
            if (++visited > (size_t)sd->tlasNodeCount) return c->fail(CRT_ERR_INVALID, "TLAS node graph is not a tree");
            const crt_tlas_node& nd = sd->tlasNodes[n];
            if (nd.leftRight == 0) { if (nd.BLAS >= sd->bvhCount) return c->fail(CRT_ERR_INVALID, "TLAS leaf references BLAS %u", nd.BLAS); if (d > tlasHeight) tlasHeight = d; continue; }
            const uint32_t l = nd.leftRight & 0xffffu, r = nd.leftRight >> 16;
            if (l >= sd->tlasNodeCount || r >= sd->tlasNodeCount) return c->fail(CRT_ERR_INVALID, "TLAS child index out of range");
            st.push_back({l, d + 1}); st.push_back({r, d + 1});
        }
        // the child pair of every TLAS interior node, side by side in the NodePair layout (render_pool_kernel fetches it with one 64-byte record load)
        for (uint32_t i = 0; i < sd->tlasNodeCount; i++) {
            const crt_tlas_node& nd = sd->tlasNodes[i];
            if (nd.leftRight == 0) continue;
            crt::NodePair& p = tlasPairs[tlas[i].ref16 & PR.indexMask];
            memcpy(&p.c[0], &tlas[nd.leftRight & 0xffffu], 32); memcpy(&p.c[1], &tlas[nd.leftRight >> 16], 32);
        }
        tlasRoot = tlas[0].ref; tlasRoot16 = tlas[0].ref16;
    }
    // texel pool + materials ([0] light, [1] floor, then the scene's — file_scene.cpp:10-12, 30-38); each carries its texture descriptor
    std::vector<uint32_t> texOff(sd->textureCount); uint64_t texels = 0;
    for (uint32_t i = 0; i < sd->textureCount; i++) {
        texOff[i] = (uint32_t)texels;
        texels += (uint64_t)sd->textures[i].width * sd->textures[i].height;
        if (texels > 0xffffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "texture pool exceeds 2^32 texels");
    }
    auto bindTex = [&](crt::Material& m, int t) {
        if (t < 0) { m.texOffset = 0; m.texW = 0; m.texH = 0; }
        else { m.texOffset = texOff[t]; m.texW = sd->textures[t].width; m.texH = sd->textures[t].height; }
    };
    std::vector<crt::Material> mats(2 + sd->materialCount);
    memset(mats.data(), 0, mats.size() * sizeof(crt::Material));
    bindTex(mats[0], -1);
    bindTex(mats[1], sd->floorTexture);
    for (uint32_t i = 0; i < sd->materialCount; i++) {
        crt::Material& m = mats[2 + i];
        m.reflectivity = sd->materials[i].reflectivity; m.refractivity = sd->materials[i].refractivity;
        memcpy(m.absorption, sd->materials[i].absorption, 12);
        bindTex(m, sd->materials[i].texture);
    }

    { const int r = drain_all(c); if (r) return r; }                     // launches still in flight read the previous scene's buffers
    c->freeScene();
    uint32_t* dTexels = nullptr;
    HIPCK(c, hipMalloc((void**)&dTexels, (size_t)texels * 4)); c->sceneAllocs.push_back(dTexels);
    for (uint32_t i = 0; i < sd->textureCount; i++)
        HIPCK(c, hipMemcpyAsync(dTexels + texOff[i], sd->textures[i].pixels, (size_t)sd->textures[i].width * sd->textures[i].height * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));

    crt::Scene& s = c->hScene;
    s.kind = sd->kind;
    set_light_block(s, sd->lightT, sd->lightInvT, sd->lightSize);
    memcpy(s.floorN, sd->floorN, 12); s.floorD = sd->floorD; s.floorInvto = sd->floorInvto;
    {   // what FileScene / TLASFileScene always build: the y-up floor plane
        s.floorAxisY = (sd->floorN[0] == 0.0f && sd->floorN[1] == 1.0f && sd->floorN[2] == 0.0f) ? 1u : 0u;
        if (hook("CRT_DEBUG_GENERAL_PRIMS")) s.floorAxisY = 0u;                   // tests: the general quad / plane expressions on the standard scenes (the light's: set_light_block)
    }
    s.floorMat = mats[1];
    s.skyOffset = texOff[sd->skyTexture]; s.skyW = sd->textures[sd->skyTexture].width; s.skyH = sd->textures[sd->skyTexture].height;
    s.texels = dTexels;
    int r;
    const char* dGeom = nullptr;
    if ((r = upload(c, geom, &dGeom))) return r;
    s.geom = dGeom;
    s.tlasOff = (uint32_t)tlasOffB; s.instOff = (uint32_t)instOffB; s.shadeOff = (uint32_t)shadeOffB;
    s.leafOff = (uint32_t)leafOffB; s.tlasPairOff = (uint32_t)tlasPairOffB;
    s.rootRef16 = (sd->kind == CRT_SCENE_TLAS) ? tlasRoot16 : rootRef0_16;
    s.poolRefBits = poolRefBits;
    if ((r = upload(c, mats, &s.mats))) return r;
    std::vector<crt::TexDesc> texTable(sd->textureCount);                     // what a texture index becomes in a Material: crt_update_look, crt_render_looks' build launch
    for (uint32_t i = 0; i < sd->textureCount; i++) texTable[i] = crt::TexDesc{texOff[i], sd->textures[i].width, sd->textures[i].height, 0u};
    if ((r = upload(c, texTable, &c->dTex))) return r;
    if (sd->kind == CRT_SCENE_TLAS) {                                     // every BLAS's node-0 box, where crt_update_transforms_device takes SetTransform's corners from
        std::vector<float> boxes;
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) { const crt_bvh_node& n0 = sd->bvhs[bi].nodes[0]; boxes.insert(boxes.end(), n0.aabbMin, n0.aabbMin + 3); boxes.insert(boxes.end(), n0.aabbMax, n0.aabbMax + 3); }
        const float* d = nullptr;
        if ((r = upload(c, boxes, &d))) return r;
        c->dRootBox = const_cast<float*>(d);
    }
    s.rootRef = (sd->kind == CRT_SCENE_TLAS) ? tlasRoot : rootRef0;
    // Traversal stack entries (LDS is what limits the waves per SIMD, so no slack): the ordered traversal keeps at most one pending sibling per level
    // below the root, i.e. <= height entries, and its dead store (the far child is written to slot sp before the push is decided) happens at an
    // interior node, where sp <= height - 1.  Two-level scenes add the TLAS entries and the return marker below the BLAS part.
    s.bvhStack = maxHeight > 0 ? maxHeight : 1;
    // the root's two children also travel in the kernel arguments: the render kernel takes every ray's first traversal step from scalar registers
    s.rootIsPair = 0; memset(s.rootPair, 0, sizeof(s.rootPair));
    if (sd->kind == CRT_SCENE_TLAS) {
        if ((tlasRoot & 0xC0000000u) == crt::kRefTlasInterior) {
            memcpy(s.rootPair, &tlas[tlasRoot & 0x7fffu], 32); memcpy(s.rootPair + 8, &tlas[(tlasRoot >> 15) & 0x7fffu], 32);
            s.rootIsPair = 1;
        }
    } else if (rootRef0 & crt::kRefInterior) {
        memcpy(s.rootPair, geom.data() + ((size_t)(rootRef0 & crt::kRefOffsetMask) << 4), 64);
        s.rootIsPair = 1;
    }
    if (hook("CRT_DEBUG_NO_ROOTPAIR")) s.rootIsPair = 0;                            // tests: every ray starts at the root reference instead
    primary_changed(c);                                                             // new light / floor block and rootPair: the camera-relative block follows
    s.stackDepth = s.bvhStack + ((sd->kind == CRT_SCENE_TLAS) ? tlasHeight + 1 : 0);   // + TLAS pushes + the return marker
    c->ldsBytes = s.stackDepth * 64u * 4u; c->latSlots = 0;
    c->extraLds = 0;
    if (const char* e = hook("CRT_DEBUG_EXTRA_LDS")) { c->extraLds = (uint32_t)atoi(e); c->ldsBytes += c->extraLds; }   // occupancy experiments and tests: unused LDS on top, for every render kernel
    if (c->ldsBytes + 15u * 256u > 64u * 1024u) return c->fail(CRT_ERR_UNSUPPORTED, "tree height %u (+TLAS %u) needs %u bytes of LDS traversal stack per wave (> 64 KiB)", maxHeight, tlasHeight, c->ldsBytes);
    // world-space bounds of all meshes (FileScene: root box of the BVH; TLAS: root box of the TLAS) for the dispatch-order heuristic
    {
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        auto grow = [&](const float* mn, const float* mx) { for (int k = 0; k < 3; k++) { if (mn[k] < lo[k]) lo[k] = mn[k]; if (mx[k] > hi[k]) hi[k] = mx[k]; } };
        if (sd->kind == CRT_SCENE_TLAS) grow(sd->tlasNodes[0].aabbMin, sd->tlasNodes[0].aabbMax);
        else grow(sd->bvhs[0].nodes[0].aabbMin, sd->bvhs[0].nodes[0].aabbMax);
        memcpy(c->meshLo, lo, 12); memcpy(c->meshHi, hi, 12); c->orderDirty = true;
    }
    {   // keep what crt_update_scene needs
        crt_ctx::Flat& f = c->flat;
        f.kind = sd->kind; f.leafOff = leafOffB; f.tlasOff = tlasOffB; f.tlasPairOff = tlasPairOffB; f.instOff = instOffB; f.shadeOff = shadeOffB;
        f.tlasNodeCount = (sd->kind == CRT_SCENE_TLAS) ? sd->tlasNodeCount : 0; f.maxHeight = maxHeight;
        f.objects = (sd->kind == CRT_SCENE_TLAS) ? sd->bvhCount : sd->objCount;
        f.pairBase.clear(); f.triBase.clear(); f.nodesUsed.clear(); f.triCount.clear(); f.rootBox.clear();
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) { const crt_bvh_node& r = sd->bvhs[bi].nodes[0]; f.rootBox.insert(f.rootBox.end(), r.aabbMin, r.aabbMin + 3); f.rootBox.insert(f.rootBox.end(), r.aabbMax, r.aabbMax + 3); }
        uint64_t pb = 0, tb = 0;
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) { f.pairBase.push_back(pb); f.triBase.push_back(tb); f.nodesUsed.push_back(sd->bvhs[bi].nodesUsed); f.triCount.push_back(sd->bvhs[bi].triCount); pb += sd->bvhs[bi].nodesUsed / 2; tb += sd->bvhs[bi].triCount; }
        f.geom.swap(geom); f.height.swap(heights);
        f.materialCount = sd->materialCount; f.tex.swap(texTable);
    }
    c->haveScene = true;
    return CRT_OK;
}

// ---- the scene-write protocol ----
// The geometry buffer, the node-0 boxes and the accelerator sets are read by launches on many streams and rewritten without a host wait for any of them.
//   A WRITER brackets what it enqueues on its stream `st` with begin_scene_write(c, st) ... end_scene_write(c, st, done): begin orders the write behind everything
//   submitted so far that may read the old bytes, end records `done` behind it and publishes it.  (crt_build_grid_device replaces buffers instead: it builds as a
//   reader, then order_behind_readers, publish_scene_write, and the old buffers are retired behind an event recorded on the main stream after that.)
//   A READER calls wait_scene(c, st) before it enqueues anything on `st` that reads the scene.
// `sceneReady` names the `done` event of the last write; every write is ordered behind the one before it, so waiting for the last is waiting for all.  The main
// stream is the meeting point: it is already behind every crt_render launch (each launch's accumulate waits for it there) and carries the host-buffer queries, so a
// writer starts from it (`writeFence`) and hands back to it, and its own consumers see the write without a wait of their own.

// Writes on the main stream of data the render kernels read (tile order, block tables, job plans, scene writes) assume it is ordered behind every render launch
// submitted so far — not true for crt_tick's render-ahead launches, which nothing on it waits for until their frames are committed: it waits for them here first.
static int order_behind_ahead(crt_ctx* c)
{
    for (const auto& a : c->ahead) HIPCK(c, hipStreamWaitEvent(c->stream, a.end, 0));
    return 0;
}

// ... and for the device queries still in flight on callers' streams (no host wait; wait_queries is the host's form)
static int order_behind_queries(crt_ctx* c)
{
    for (auto& q : c->qslot) {
        if (!q.pending) continue;
        const hipError_t e = hipEventQuery(q.done);
        if (e == hipSuccess) { q.pending = false; continue; }
        if (e != hipErrorNotReady) return c->hip(e, "hipEventQuery(query)");
        HIPCK(c, hipStreamWaitEvent(c->stream, q.done, 0));
    }
    return 0;
}

static int wait_scene(crt_ctx* c, hipStream_t st)
{
    if (c->sceneReady) HIPCK(c, hipStreamWaitEvent(st, c->sceneReady, 0));
    return 0;
}

// The main stream behind every launch submitted so far that may read the scene.  The epoch is bumped HERE, the one place every writer passes before its first byte
// changes: an entry that fails later has already invalidated crt_tick's rendered-ahead frames, and a write refused after this point costs those frames only.
static int order_behind_readers(crt_ctx* c)
{
    int r;
    if ((r = order_behind_ahead(c)) || (r = order_behind_queries(c))) return r;
    c->epoch++;
    return 0;
}

static int begin_scene_write(crt_ctx* c, hipStream_t st)
{
    const int r = order_behind_readers(c);
    if (r || st == c->stream) return r;                                    // (the main stream is behind the previous write already)
    HIPCK(c, ensure_event(&c->writeFence));
    HIPCK(c, hipEventRecord(c->writeFence, c->stream));                    // a wait takes the event as recorded at the call: one fence serves every write
    HIPCK(c, hipStreamWaitEvent(st, c->writeFence, 0));
    return wait_scene(c, st);
}

// `done`, recorded on `st` behind the write, is what readers wait for from now on, and the main stream follows
static int publish_scene_write(crt_ctx* c, hipStream_t st, hipEvent_t done)
{
    c->sceneReady = done;
    if (st != c->stream) HIPCK(c, hipStreamWaitEvent(c->stream, done, 0));
    return 0;
}

static int end_scene_write(crt_ctx* c, hipStream_t st, hipEvent_t done)
{
    HIPCK(c, hipEventRecord(done, st));
    return publish_scene_write(c, st, done);
}

// fills the TLAS sections of a host geometry image from the reference's TLASBVHNode array: per-node records with both reference forms, and the child
// pair of every interior node side by side (NodePair layout).  Returns the TLAS height, or a negative status.
static int flatten_tlas(crt_ctx* c, const crt_tlas_node* nodes, uint32_t count, uint32_t bvhCount, crt::TlasNode* tlas, crt::NodePair* tlasPairs, uint32_t* heightOut)
{
    const crt::PoolRefForm PR = crt::pool_ref_form(c->hScene.poolRefBits);      // the pool references stay in the width the scene was uploaded in
    uint32_t nTlasPairs = 0;
    for (uint32_t i = 0; i < count; i++) {      // device copy carries each node's packed reference instead of leftRight / BLAS
        const crt_tlas_node& nd = nodes[i];
        memcpy(tlas[i].lo, nd.aabbMin, 12); memcpy(tlas[i].hi, nd.aabbMax, 12);
        tlas[i].ref = nd.leftRight ? (crt::kRefTlasInterior | (nd.leftRight & 0x7fffu) | (((nd.leftRight >> 16) & 0x7fffu) << 15))
                                   : (crt::kRefTlasLeaf | (nd.BLAS & 0xffffu));
        tlas[i].ref16 = nd.leftRight ? (PR.tlasBit | nTlasPairs++) : (PR.tlasLeaf | (nd.BLAS & PR.indexMask));   // interior nodes number their child pairs
    }
    std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u}); size_t visited = 0; uint32_t height = 0;
    while (!st.empty()) {
        auto [n, d] = st.back(); st.pop_back();
        if (++visited > (size_t)count) return c->fail(CRT_ERR_INVALID, "TLAS node graph is not a tree");
        const crt_tlas_node& nd = nodes[n];
        if (nd.leftRight == 0) { if (nd.BLAS >= bvhCount) return c->fail(CRT_ERR_INVALID, "TLAS leaf references BLAS %u", nd.BLAS); if (d > height) height = d; continue; }
        const uint32_t l = nd.leftRight & 0xffffu, r = nd.leftRight >> 16;
        if (l >= count || r >= count) return c->fail(CRT_ERR_INVALID, "TLAS child index out of range");
        st.push_back({l, d + 1}); st.push_back({r, d + 1});
    }
    for (uint32_t i = 0; i < count; i++) {
        const crt_tlas_node& nd = nodes[i];
        if (nd.leftRight == 0) continue;
        crt::NodePair& p = tlasPairs[tlas[i].ref16 & PR.indexMask];
        memcpy(&p.c[0], &tlas[nd.leftRight & 0xffffu], 32); memcpy(&p.c[1], &tlas[nd.leftRight >> 16], 32);
    }
    *heightOut = height;
    return 0;
}

// the Scene block's view of the root: its child pair travels in the kernel arguments (see render kernels), plus the dispatch-order bounds
static void set_root(crt_ctx* c, int kind, const float* lo, const float* hi)
{
    crt::Scene& s = c->hScene; const crt_ctx::Flat& f = c->flat;
    s.rootIsPair = 0; memset(s.rootPair, 0, sizeof(s.rootPair));
    if (kind == CRT_SCENE_TLAS) {
        const crt::TlasNode* tlas = reinterpret_cast<const crt::TlasNode*>(f.geom.data() + f.tlasOff);
        const uint32_t root = tlas[0].ref;
        s.rootRef = root; s.rootRef16 = tlas[0].ref16;
        if ((root & 0xC0000000u) == crt::kRefTlasInterior) { memcpy(s.rootPair, &tlas[root & 0x7fffu], 32); memcpy(s.rootPair + 8, &tlas[(root >> 15) & 0x7fffu], 32); s.rootIsPair = 1; }
    } else if (s.rootRef & crt::kRefInterior) {
        memcpy(s.rootPair, f.geom.data() + ((size_t)(s.rootRef & crt::kRefOffsetMask) << 4), 64);
        s.rootIsPair = 1;
    }
    if (hook("CRT_DEBUG_NO_ROOTPAIR")) s.rootIsPair = 0;
    primary_changed(c);
    memcpy(c->meshLo, lo, 12); memcpy(c->meshHi, hi, 12); c->orderDirty = true;
}

// LDS of one render_pool_kernel wavefront of a launch of `frames` frames on the current scene, CRT_DEBUG_EXTRA_LDS included (crt_launch_render_pool asks for the same)
static uint32_t pool_lds_need(const crt_ctx* c, uint32_t frames)
{
    return crt_pool_lds_bytes(c->hScene.stackDepth, crt_pool_streams(frames), c->hScene.poolRefBits) + c->extraLds;
}
// Can render_pool_kernel render the current scene at all: its references have a pool form (16 or 32 bits wide, layout.h) and a wavefront's LDS stays within what the
// device grants a workgroup.  Otherwise the launch is render_tiles_kernel's, whatever CRT_RENDER_KERNEL says.
static bool pool_can_run(crt_ctx* c, uint32_t frames)
{
    if (c->hScene.poolRefBits == 0u) return false;
    if (!c->poolLdsLimit) c->poolLdsLimit = crt_pool_lds_limit(c->cfg.device);
    return pool_lds_need(c, frames) <= c->poolLdsLimit;
}

// a TLAS of this height on top of the scene's BLASes: does the traversal stack (BVH part + TLAS pushes + the return marker) fit the LDS budget of the render kernels?
static int check_tlas_height(crt_ctx* c, uint32_t tlasHeight)
{
    if ((c->hScene.bvhStack + tlasHeight + 1) * 64u * 4u + 15u * 256u > 64u * 1024u)
        return c->fail(CRT_ERR_UNSUPPORTED, "TLAS height %u needs %u bytes of LDS traversal stack per wave (> 64 KiB)", tlasHeight, (c->hScene.bvhStack + tlasHeight + 1) * 256u);
    return 0;
}

// what a rebuilt TLAS changes in the context besides the geometry buffer (crt_update_scene, crt_update_transforms_device), once the mirror holds the new TLAS
// sections: the stack depth and its LDS, the root reference and pair in the kernel arguments, the dispatch-order bounds (node 0's box)
static void adopt_tlas(crt_ctx* c, uint32_t tlasHeight, const float* lo, const float* hi)
{
    crt::Scene& s = c->hScene;
    s.stackDepth = s.bvhStack + tlasHeight + 1;
    c->ldsBytes = s.stackDepth * 64u * 4u; c->latSlots = 0;
    set_root(c, CRT_SCENE_TLAS, lo, hi);
}

// the reference has no Refit for BLASKDTree / BLASGrid: a refit (CRT_UPDATE_BOUNDS, crt_refit_device) drops the two-level KD-tree / grid sets (their buffers are
// freed by the next upload)
static void drop_blas_sets(crt_ctx* c)
{
    for (int k = 0; k < 2; k++) if (c->haveBlas[k]) { c->haveBlas[k] = false; if (c->renderAccel == k + 1) c->renderAccel = 0; }
}

int crt_update_scene(crt_ctx* c, const crt_scene_desc* sd, uint32_t what)
{
    if (!c || !sd) return CRT_ERR_INVALID;
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_update_scene before crt_upload_scene");
    crt_ctx::Flat& f = c->flat;
    if (sd->kind != f.kind || sd->bvhCount != f.nodesUsed.size() || !sd->bvhs) return c->fail(CRT_ERR_INVALID, "crt_update_scene: scene kind / BVH count differ from the uploaded scene");
    if ((what & ~(uint32_t)(CRT_UPDATE_TRANSFORMS | CRT_UPDATE_BOUNDS)) || what == 0) return c->fail(CRT_ERR_INVALID, "crt_update_scene: unknown update flags");
    if ((what & CRT_UPDATE_TRANSFORMS) && f.kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_INVALID, "CRT_UPDATE_TRANSFORMS applies to two-level scenes (a FileScene bakes its transforms into the triangles)");
    HIPCK(c, hipSetDevice(c->cfg.device));
    for (uint32_t bi = 0; bi < sd->bvhCount; bi++)
        if (sd->bvhs[bi].nodesUsed != f.nodesUsed[bi] || sd->bvhs[bi].triCount != f.triCount[bi] || !sd->bvhs[bi].nodes || !sd->bvhs[bi].triangles || !sd->bvhs[bi].triangleIndices)
            return c->fail(CRT_ERR_INVALID, "crt_update_scene: BVH %u changed its topology (node / triangle count); upload the scene again", bi);
    // ---- every check first: a refused update leaves the host mirror (and so the next successful update) untouched ----
    if (f.kind == CRT_SCENE_TLAS && (!sd->tlasNodes || sd->tlasNodeCount != f.tlasNodeCount))
        return c->fail(CRT_ERR_INVALID, "crt_update_scene: a two-level scene needs the node array of the TLASBVH::Build that followed the change (tlasNodes, %u nodes as uploaded)", f.tlasNodeCount);
    if (what & CRT_UPDATE_BOUNDS) {
        const crt::LeafTri* leaf = reinterpret_cast<const crt::LeafTri*>(f.geom.data() + f.leafOff);
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) {
            const crt_bvh& b = sd->bvhs[bi];
            for (uint32_t j = 0; j < b.triCount; j++) {
                const uint32_t ti = b.triangleIndices[j];
                if (ti >= b.triCount) return c->fail(CRT_ERR_INVALID, "BVH %u: triangleIndices[%u] out of range", bi, j);
                if (leaf[f.triBase[bi] + j].shadeIdx != (uint32_t)(f.triBase[bi] + ti)) return c->fail(CRT_ERR_INVALID, "BVH %u: triangleIndices changed; Refit keeps the leaf order — upload the scene again", bi);
            }
        }
    }
    uint32_t tlasHeight = 0;
    std::vector<char> tlasImage;                                            // the TLAS sections (nodes + child pairs), flattened aside and copied in once they are known to be valid
    if (f.kind == CRT_SCENE_TLAS) {
        tlasImage.assign((size_t)(f.instOff - f.tlasOff), 0);
        int r = flatten_tlas(c, sd->tlasNodes, sd->tlasNodeCount, sd->bvhCount, reinterpret_cast<crt::TlasNode*>(tlasImage.data()),
                             reinterpret_cast<crt::NodePair*>(tlasImage.data() + (f.tlasPairOff - f.tlasOff)), &tlasHeight);
        if (r || (r = check_tlas_height(c, tlasHeight))) return r;
    }
    // ---- apply ----
    size_t lo = SIZE_MAX, hi = 0;                                         // byte range of the geometry buffer to rewrite
    auto touch = [&](size_t a, size_t b) { if (a < lo) lo = a; if (b > hi) hi = b; };
    if (what & CRT_UPDATE_BOUNDS) {
        // BVH::Refit / BLASBVH::Refit (bvh.cpp:26-43): same tree, new boxes and vertex positions.  References, leaf order and shading records stay.
        crt::NodePair* pairs = reinterpret_cast<crt::NodePair*>(f.geom.data());
        crt::LeafTri* leaf = reinterpret_cast<crt::LeafTri*>(f.geom.data() + f.leafOff);
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) {
            const crt_bvh& b = sd->bvhs[bi];
            for (uint32_t n = 1; n + 1 < b.nodesUsed; n += 2) {
                crt::NodePair& p = pairs[f.pairBase[bi] + ((n - 1) >> 1)];
                for (int k = 0; k < 2; k++) { memcpy(p.c[k].lo, b.nodes[n + k].aabbMin, 12); memcpy(p.c[k].hi, b.nodes[n + k].aabbMax, 12); }
            }
            for (uint32_t j = 0; j < b.triCount; j++) {
                const crt_tri& t = b.triangles[b.triangleIndices[j]];
                crt::LeafTri& lt = leaf[f.triBase[bi] + j];
                for (int k = 0; k < 3; k++) { lt.v0[k] = t.vertex0[k]; lt.e1[k] = t.vertex1[k] - t.vertex0[k]; lt.e2[k] = t.vertex2[k] - t.vertex0[k]; }
            }
        }
        touch(0, (size_t)f.tlasOff);
        for (uint32_t bi = 0; bi < sd->bvhCount; bi++) { memcpy(&f.rootBox[6 * bi], sd->bvhs[bi].nodes[0].aabbMin, 12); memcpy(&f.rootBox[6 * bi + 3], sd->bvhs[bi].nodes[0].aabbMax, 12); }
    }
    if (f.kind == CRT_SCENE_TLAS) {
        if (what & CRT_UPDATE_TRANSFORMS) {
            crt::Instance* inst = reinterpret_cast<crt::Instance*>(f.geom.data() + f.instOff);
            for (uint32_t bi = 0; bi < sd->bvhCount; bi++) { memcpy(inst[bi].invT, sd->bvhs[bi].invT, 48); memcpy(inst[bi].T, sd->bvhs[bi].T, 48); }   // BLASBVH::SetTransform, blas_bvh.cpp:363-374
        }
        // TLASBVH::Build (tlas_bvh.cpp:17-55) ran on the host after SetTransform / Refit: new node array of the same size
        memcpy(f.geom.data() + f.tlasOff, tlasImage.data(), tlasImage.size());
        touch((size_t)f.tlasOff, (size_t)f.shadeOff);
    }
    if (lo >= hi) return CRT_OK;
    // In-place rewrite on the main stream (the scene-write protocol), no allocation of device memory and no host wait for the GPU.  Pinned staging buffers alternate
    // and grow on demand; one is reused only after its own copy.
    const int k = c->stageFlip ^= 1;
    const size_t boxBytes = ((what & CRT_UPDATE_BOUNDS) && c->dRootBox) ? f.rootBox.size() * 4u : 0u;   // the device copy of the node-0 boxes rides behind the range
    const size_t geomBytes = hi - lo, bytes = geomBytes + boxBytes;
    if (c->stageBytes[k] < bytes) {
        if (c->hStage[k]) { HIPCK(c, hipEventSynchronize(c->stageCopied[k])); HIPCK(c, hipHostFree(c->hStage[k])); c->hStage[k] = nullptr; }
        HIPCK(c, hipHostMalloc((void**)&c->hStage[k], bytes, hipHostMallocDefault)); c->stageBytes[k] = bytes;
        HIPCK(c, ensure_event(&c->stageCopied[k]));
    } else HIPCK(c, hipEventSynchronize(c->stageCopied[k]));
    memcpy(c->hStage[k], f.geom.data() + lo, geomBytes);
    if (boxBytes) memcpy(c->hStage[k] + geomBytes, f.rootBox.data(), boxBytes);
    { const int r = begin_scene_write(c, c->stream); if (r) return r; }
    if (what & CRT_UPDATE_BOUNDS) {
        for (crt_ctx::BlasSet& b : c->blasSet) std::fill(b.current.begin(), b.current.end(), (uint8_t)0);   // every BLAS's KD-tree and grid are of the old vertices
        drop_blas_sets(c);                                                 // (may reset renderAccel: behind the epoch's bump)
    }
    HIPCK(c, hipMemcpyAsync(const_cast<char*>(c->hScene.geom) + lo, c->hStage[k], geomBytes, hipMemcpyHostToDevice, c->stream));
    if (boxBytes) HIPCK(c, hipMemcpyAsync(c->dRootBox, c->hStage[k] + geomBytes, boxBytes, hipMemcpyHostToDevice, c->stream));
    { const int r = end_scene_write(c, c->stream, c->stageCopied[k]); if (r) return r; }
    if (f.kind == CRT_SCENE_TLAS) adopt_tlas(c, tlasHeight, sd->tlasNodes[0].aabbMin, sd->tlasNodes[0].aabbMax);
    else set_root(c, f.kind, sd->bvhs[0].nodes[0].aabbMin, sd->bvhs[0].nodes[0].aabbMax);
    return CRT_OK;
}

uint32_t crt_look_words(uint32_t materialCount) { return CRT_LOOK_HEADER_WORDS + CRT_LOOK_MATERIAL_WORDS * materialCount; }

// a look's texture indices against the uploaded texture table (crt_update_look; crt_render_looks' host entry, which names the look): 0, or the refusal
static int check_look(crt_ctx* c, const uint32_t* look, const char* what, const char* where)
{
    const crt_ctx::Flat& f = c->flat;
    const crt_look_header* h = reinterpret_cast<const crt_look_header*>(look);
    const int32_t n = (int32_t)f.tex.size();
    if (h->floorTexture < 0 || h->floorTexture >= n) return c->fail(CRT_ERR_INVALID, "%s: %sfloorTexture %d lies outside [0, %d)", what, where, h->floorTexture, n);
    if (h->skyTexture < 0 || h->skyTexture >= n) return c->fail(CRT_ERR_INVALID, "%s: %sskyTexture %d lies outside [0, %d)", what, where, h->skyTexture, n);
    const crt_material* m = reinterpret_cast<const crt_material*>(look + CRT_LOOK_HEADER_WORDS);
    for (uint32_t i = 0; i < f.materialCount; i++)
        if (m[i].texture < -1 || m[i].texture >= n) return c->fail(CRT_ERR_INVALID, "%s: %smaterial %u: texture %d lies outside [-1, %d)", what, where, i, m[i].texture, n);
    return 0;
}

int crt_update_look(crt_ctx* c, const void* look)
{
    if (!c) return CRT_ERR_INVALID;
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "crt_update_look: the PrimitiveScene's materials are part of its code (primitive_scene.cpp); it has no look");
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_update_look before crt_upload_scene");
    if (!look) return c->fail(CRT_ERR_INVALID, "crt_update_look: NULL look");
    const crt_ctx::Flat& f = c->flat;
    const uint32_t* words = static_cast<const uint32_t*>(look);
    { const int r = check_look(c, words, "crt_update_look", ""); if (r) return r; }
    HIPCK(c, hipSetDevice(c->cfg.device));
    const crt_look_header* h = reinterpret_cast<const crt_look_header*>(words);
    const crt_material* lm = reinterpret_cast<const crt_material*>(words + CRT_LOOK_HEADER_WORDS);
    // ---- the Material table as crt_upload_scene writes it ([0] light, [1] floor, then the scene's), into a pinned staging buffer (crt_update_scene's pair) ----
    const size_t bytes = (size_t)(2u + f.materialCount) * sizeof(crt::Material);
    const int k = c->stageFlip ^= 1;
    if (c->stageBytes[k] < bytes) {
        if (c->hStage[k]) { HIPCK(c, hipEventSynchronize(c->stageCopied[k])); HIPCK(c, hipHostFree(c->hStage[k])); c->hStage[k] = nullptr; c->stageBytes[k] = 0; }
        HIPCK(c, hipHostMalloc((void**)&c->hStage[k], bytes, hipHostMallocDefault)); c->stageBytes[k] = bytes;
        HIPCK(c, ensure_event(&c->stageCopied[k]));
    } else HIPCK(c, hipEventSynchronize(c->stageCopied[k]));
    crt::Material* mats = reinterpret_cast<crt::Material*>(c->hStage[k]);
    memset(mats, 0, bytes);
    auto bindTex = [&](crt::Material& m, int t) {
        if (t < 0) { m.texOffset = 0; m.texW = 0; m.texH = 0; }
        else { m.texOffset = f.tex[(size_t)t].offset; m.texW = f.tex[(size_t)t].w; m.texH = f.tex[(size_t)t].h; }
    };
    bindTex(mats[0], -1);
    bindTex(mats[1], h->floorTexture);
    for (uint32_t i = 0; i < f.materialCount; i++) {
        crt::Material& m = mats[2 + i];
        m.reflectivity = lm[i].reflectivity; m.refractivity = lm[i].refractivity;
        memcpy(m.absorption, lm[i].absorption, 12);
        bindTex(m, lm[i].texture);
    }
    // ---- apply: the records in place under the scene-write protocol; the Scene block travels by value with every later launch ----
    { const int r = begin_scene_write(c, c->stream); if (r) return r; }
    HIPCK(c, hipMemcpyAsync(const_cast<crt::Material*>(c->hScene.mats), mats, bytes, hipMemcpyHostToDevice, c->stream));
    { const int r = end_scene_write(c, c->stream, c->stageCopied[k]); if (r) return r; }
    crt::Scene& s = c->hScene;
    set_light_block(s, h->lightT, h->lightInvT, h->lightSize);
    s.floorMat = mats[1];
    const crt::TexDesc& sky = f.tex[(size_t)h->skyTexture];
    s.skyOffset = sky.offset; s.skyW = sky.w; s.skyH = sky.h;
    primary_changed(c);                                                   // new light block: the camera-relative block and the tile classes follow
    c->orderDirty = true;                                                 // ... and what a camera change invalidates: the dispatch order, the probe and the job costs behind it
    return CRT_OK;
}

int crt_set_camera(crt_ctx* c, const float camPos[3], const float tl[3], const float tr[3], const float bl[3])
{
    if (!c || !camPos || !tl || !tr || !bl) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    crt::Scene& s = c->hScene;
    if (!memcmp(s.camPos, camPos, 12) && !memcmp(s.topLeft, tl, 12) && !memcmp(s.topRight, tr, 12) && !memcmp(s.bottomLeft, bl, 12)) return CRT_OK;   // unchanged (a per-frame PushCamera)
    memcpy(s.camPos, camPos, 12); memcpy(s.topLeft, tl, 12); memcpy(s.topRight, tr, 12); memcpy(s.bottomLeft, bl, 12);
    primary_changed(c);
    c->orderDirty = true; c->epoch++;
    return CRT_OK;      // the Scene block travels by value in every launch's kernel arguments
}

// the dispatch order of the tiles (local indices) to the device.  No host synchronisation: the copy runs on the main stream, which is ordered behind every render
// launch submitted so far (it waits for each launch's end event before that launch's accumulate), so the previous order is no longer read when it is overwritten;
// later launches wait for `orderReady` on their own stream.  The staging buffers are pinned and alternate; one is reused only after its own copy.
static int upload_tile_order(crt_ctx* c, const std::vector<uint32_t>& order)
{
    if (!c->dTileOrder) HIPCK(c, hipMalloc((void**)&c->dTileOrder, (size_t)c->tileCount * 4));
    { const int r = order_behind_ahead(c); if (r) return r; }
    const int k = c->orderFlip ^= 1;
    if (!c->hTileOrder[k]) {
        HIPCK(c, hipHostMalloc((void**)&c->hTileOrder[k], (size_t)c->tileCount * 4, hipHostMallocDefault));
        HIPCK(c, ensure_event(&c->orderCopied[k]));
    } else HIPCK(c, hipEventSynchronize(c->orderCopied[k]));
    memcpy(c->hTileOrder[k], order.data(), order.size() * 4);
    HIPCK(c, hipMemcpyAsync(c->dTileOrder, c->hTileOrder[k], order.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->orderCopied[k], c->stream));
    c->orderReady = c->orderCopied[k];
    return 0;
}

// Every tile order ends with the tiles whose CURRENT class is kTileSky (cls: one byte per local tile, or none known), in the relative order they had: the ranks in
// front of that tail are what a pool launch with a sky launch beside it renders (sky_split).  Returns the tail's length.
static uint32_t sky_to_tail(const std::vector<uint8_t>& cls, std::vector<uint32_t>& order)
{
    if (cls.size() != order.size()) return 0u;
    const auto tail = std::stable_partition(order.begin(), order.end(), [&](uint32_t i) { return cls[i] != crt::kTileSky; });
    return (uint32_t)(order.end() - tail);
}

// Tiles (local indices 0..tileCount) ordered so that those inside the screen-space bounding rectangle of the meshes' world box come first
// (the stream-pool kernel and wide launches dispatch in this order).  Pure scheduling heuristic: the projection uses the pin-hole camera of crt_set_camera in double precision and is conservative on failure
// (a corner behind the eye makes every tile a candidate).
static int update_tile_order(crt_ctx* c)
{
    if (!c->orderDirty || c->tileCount == 0) return 0;
    const crt::Scene& s = c->hScene;
    double R[3], Dn[3], N[3];
    for (int k = 0; k < 3; k++) { R[k] = (double)s.topRight[k] - s.topLeft[k]; Dn[k] = (double)s.bottomLeft[k] - s.topLeft[k]; }
    N[0] = R[1] * Dn[2] - R[2] * Dn[1]; N[1] = R[2] * Dn[0] - R[0] * Dn[2]; N[2] = R[0] * Dn[1] - R[1] * Dn[0];
    const double rr = R[0] * R[0] + R[1] * R[1] + R[2] * R[2], dd = Dn[0] * Dn[0] + Dn[1] * Dn[1] + Dn[2] * Dn[2];
    double E[3]; for (int k = 0; k < 3; k++) E[k] = (double)s.topLeft[k] - s.camPos[k];
    const double num = E[0] * N[0] + E[1] * N[1] + E[2] * N[2];
    // screen rectangle (in tiles, one tile of margin) of 8 world-space corners; false when a corner is behind the eye
    auto rect_of = [&](const float* P8, int r[4]) -> bool {
        double u0 = 1e30, u1 = -1e30, v0 = 1e30, v1 = -1e30;
        for (int i = 0; i < 8; i++) {
            const float* P = P8 + 3 * i;
            double d[3] = {P[0] - s.camPos[0], P[1] - s.camPos[1], P[2] - s.camPos[2]};
            const double den = d[0] * N[0] + d[1] * N[1] + d[2] * N[2];
            const double t = den != 0 ? num / den : -1;
            if (!(t > 0) || rr == 0 || dd == 0) return false;
            double Q[3]; for (int k = 0; k < 3; k++) Q[k] = s.camPos[k] + t * d[k] - s.topLeft[k];
            const double u = (Q[0] * R[0] + Q[1] * R[1] + Q[2] * R[2]) / rr, v = (Q[0] * Dn[0] + Q[1] * Dn[1] + Q[2] * Dn[2]) / dd;
            if (u < u0) u0 = u; if (u > u1) u1 = u; if (v < v0) v0 = v; if (v > v1) v1 = v;
        }
        r[0] = (int)floor(u0 * c->cfg.width / 16.0) - 1; r[1] = (int)floor(u1 * c->cfg.width / 16.0) + 1;
        r[2] = (int)floor(v0 * c->cfg.height / 16.0) - 1; r[3] = (int)floor(v1 * c->cfg.height / 16.0) + 1;
        return true;
    };
    float world[24];
    for (int i = 0; i < 8; i++) { world[3 * i] = (i & 1) ? c->meshHi[0] : c->meshLo[0]; world[3 * i + 1] = (i & 2) ? c->meshHi[1] : c->meshLo[1]; world[3 * i + 2] = (i & 4) ? c->meshHi[2] : c->meshLo[2]; }
    int wr[4] = {0, c->tilesX - 1, 0, c->tilesY - 1};
    (void)rect_of(world, wr);                                     // on failure wr stays the whole image
    std::vector<uint32_t> first, second, rest;
    for (uint32_t i = 0; i < c->tileCount; i++) {
        const uint32_t tile = c->tileFirst + i * c->tileStride;
        const int tx = (int)(tile % (uint32_t)c->tilesX), ty = (int)(tile / (uint32_t)c->tilesX);
        const bool inRect = tx >= wr[0] && tx <= wr[1] && ty >= wr[2] && ty <= wr[3];
        if (inRect) first.push_back(i); else rest.push_back(i);
    }
    // a new camera / scene: the latency mode measures again (see next_block_table)
    for (int k = 0; k <= crt_ctx::kLatStages; k++) { c->tuneCount[k] = 0; c->tuneMs[k] = 0; }
    c->latStage = 0; c->latBest = 0; c->latDone = false; c->latWarm = false; c->latConfirming = false; c->latQueue.clear(); c->costPending = false; c->latProbed = false;
    first.insert(first.end(), rest.begin(), rest.end());
    (void)sky_to_tail(c->hostClass, first);
    c->jobCostValid = false; c->jobCostPending = false; c->planValid = false; c->skyWindowTicks = 0;
    { const int r = upload_tile_order(c, first); if (r) return r; }
    c->orderDirty = false;
    return 0;
}

// The tile classes of the Scene block as it stands (device/tile_class.h), to the device under the tile order's protocol (upload_tile_order): the copy runs on the
// main stream behind every render launch submitted so far, so a launch in flight keeps reading the table it was launched with; later launches wait for
// `orderReady`, which names the newest of the two tables' copies (one stream: behind it, both have landed).
static int update_tile_class(crt_ctx* c)
{
    if (!c->classDirty || c->tileCount == 0) return 0;
    if (!c->dTileClass) HIPCK(c, hipMalloc((void**)&c->dTileClass, (size_t)c->tileCount));
    { const int r = order_behind_ahead(c); if (r) return r; }
    const int k = c->classFlip ^= 1;
    if (!c->hTileClass[k]) {
        HIPCK(c, hipHostMalloc((void**)&c->hTileClass[k], (size_t)c->tileCount, hipHostMallocDefault));
        HIPCK(c, ensure_event(&c->classCopied[k]));
    } else HIPCK(c, hipEventSynchronize(c->classCopied[k]));
    crt::classify_tiles(c->hScene, c->cfg.width, c->cfg.height, (uint32_t)c->tilesX, c->tileFirst, c->tileStride, c->tileCount, c->hTileClass[k]);
    if (hook("CRT_DEBUG_NO_FLOOR_CLASS"))                           // tests / A-B: the table as it was before kTileFloorSure (the floor tiles take new_ray's general form)
        for (uint32_t i = 0; i < c->tileCount; i++) c->hTileClass[k][i] &= (uint8_t)~crt::kTileFloorSure;
    {
        // a changed set of sky tiles: the order on the device no longer ends with it, so a new one is made before the next launch (crt_render: update_tile_order
        // runs behind this function) — and with it the costs are measured again, as after a camera change
        const uint8_t* cls = c->hTileClass[k];
        bool same = c->hostClass.size() == c->tileCount; uint32_t sky = 0;
        for (uint32_t i = 0; i < c->tileCount; i++) { const bool s = cls[i] == crt::kTileSky; sky += s ? 1u : 0u; if (same && s != (c->hostClass[i] == crt::kTileSky)) same = false; }
        c->hostClass.assign(cls, cls + c->tileCount); c->skyTiles = sky;
        if (!same) c->orderDirty = true;
    }
    HIPCK(c, hipMemcpyAsync(c->dTileClass, c->hTileClass[k], (size_t)c->tileCount, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->classCopied[k], c->stream));
    c->orderReady = c->classCopied[k];
    c->classDirty = false;
    return 0;
}

// bytes one 64-frame window of a launch takes in the slab pool: its 12-byte samples (device/sample_body.h: the kernels' own size function) + (stream-pool
// kernel) the throughput-factor scratch.  A launch's region = [samples of all its windows][scratch of all its windows]; a window of samples is a multiple of
// 196 608 bytes, so the scratch behind them stays 4-byte aligned.
static size_t sample_bytes_per_window(const crt_ctx* c, uint32_t passes) { return crt_slab_window_bytes(c->tileCount, passes); }
static size_t window_bytes(const crt_ctx* c, uint32_t passes) { return sample_bytes_per_window(c, passes) + (c->usePool ? crt_pool_scratch_bytes_per_window(c->tileCount) : 0); }

// Latency mode: block tables of single-window launches from measured tile costs (100 MHz ticks of a tile's slowest wavefront).  A launch ends on its slowest
// wavefront, and a wavefront's speed is set by how many phases (NODE / TRI / SHADE) its lanes populate per trip, not by its lane count — so a tile given to
// 64 / L wavefronts of L lanes runs its streams' serial chains faster, at the price of 64 / L times the instruction issue.  Measured on the bunny's heaviest
// tiles (tools/latency_probe.py, everything else one wave per tile): time(L) / time(64) = 0.93 (32), 0.88 (16), 0.79 (8), 0.69 (4), 0.57 (2), 0.48 (1) — but the
// ratio differs from tile to tile (phase mix) and shrinks when the extra wavefronts compete for instruction issue, so the tables are found by FEEDBACK: each
// stage starts from the fastest stage so far (its lanes per tile and the costs measured under it), aims at `aim` x that stage's slowest tile, narrows every tile
// the model says would miss the aim and widens every tile that would make it with wavefronts twice as wide; crt_render times each stage and keeps the fastest.
// CRT_LAT_POLICY="share:lanes,.." replaces stage 1 by fixed steps (tiles costing >= share x the slowest get `lanes`) and stops there.
// one entry of a block table: local tile | first frame << 16 | log2(lanes) << 22 | window << 25 (render_tiles_kernel)
static uint32_t block_desc(uint32_t tile, uint32_t laneBase, uint32_t lanes, uint32_t window) { uint32_t lg = 0; while ((1u << lg) < lanes) lg++; return tile | (laneBase << 16) | (lg << 22) | (window << 25); }
static const uint32_t kLatLanes[7] = {64u, 32u, 16u, 8u, 4u, 2u, 1u};
static const double kLatG[7] = {1.0, 0.93, 0.88, 0.79, 0.69, 0.57, 0.48};
static int lat_index(uint32_t L) { int k = 0; while (k < 6 && kLatLanes[k] != L) k++; return k; }

// one feedback step of the latency tuner for one tile: it ran `lanes`-wide wavefronts and its slowest one took `cost`; the widest width whose modelled duration meets T
static uint8_t next_lanes(uint8_t lanes, uint32_t cost, double T)
{
    int k = lat_index(lanes); const double unit = (double)cost / kLatG[k];                     // the model's one-wave cost of this tile
    while (k < 6 && unit * kLatG[k] > T) k++;                                                  // narrower until the model meets the aim
    while (k > 0 && unit * kLatG[k - 1] <= 0.9 * T) k--;                                        // wider while twice as wide still makes it comfortably
    return (uint8_t)kLatLanes[k];
}
// tests (no GPU needed): next_lanes for n tiles
extern "C" int crt_debug_next_lanes(const uint8_t* lanes, const uint32_t* cost, uint32_t n, double T, uint8_t* out)
{
    if (!lanes || !cost || !out) return CRT_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) { if (lanes[i] == 0 || lanes[i] > 64 || (64 % lanes[i]) != 0) return CRT_ERR_INVALID; out[i] = next_lanes(lanes[i], cost[i], T); }
    return CRT_OK;
}

// The table of a stage, solved instead of stepped (round 3): every tile ran `lanes[i]`-wide wavefronts and its slowest took `cost[i]` (or: lanes 64 and the probe's estimate).
// A narrower table is a faster launch as long as the device holds ALL its wavefronts at once — a wavefront that has to wait for a slot starts its chain late — so the aim
// T is the LOWEST one whose table fits `budget` wavefronts (bisection; waves(T) falls as T rises), but not below what the most expensive tile takes as one-lane wavefronts,
// which bounds the launch anyway: cheaper tiles are not split to beat a time nothing can reach.  Returns T.
static double solve_block_table(const std::vector<uint8_t>& lanes, const std::vector<uint32_t>& cost, double budget, std::vector<uint8_t>& out)
{
    const size_t n = cost.size();
    double topUnit = 0; for (size_t i = 0; i < n; i++) topUnit = std::max(topUnit, (double)cost[i] / kLatG[lat_index(lanes[i])]);
    out.assign(n, 64);
    if (topUnit <= 0) return 0;
    auto waves = [&](double T) { double w = 0; for (size_t i = 0; i < n; i++) w += 64.0 / next_lanes(lanes[i], cost[i], T); return w; };
    double lo = kLatG[6] * topUnit, hi = topUnit;
    if (waves(lo) > budget) { for (int it = 0; it < 14; it++) { const double mid = 0.5 * (lo + hi); if (waves(mid) <= budget) hi = mid; else lo = mid; } lo = hi; }
    for (size_t i = 0; i < n; i++) out[i] = next_lanes(lanes[i], cost[i], lo);
    return lo;
}
// tests (no GPU needed): the solved table for n tiles and a wavefront budget; returns the aim through *T
extern "C" int crt_debug_solve_block_table(const uint8_t* lanes, const uint32_t* cost, uint32_t n, double budget, uint8_t* out, double* T)
{
    if (!lanes || !cost || !out) return CRT_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) if (lanes[i] == 0 || lanes[i] > 64 || (64 % lanes[i]) != 0) return CRT_ERR_INVALID;
    std::vector<uint8_t> L; const double t = solve_block_table(std::vector<uint8_t>(lanes, lanes + n), std::vector<uint32_t>(cost, cost + n), budget, L);
    if (n) memcpy(out, L.data(), n);
    if (T) *T = t;
    return CRT_OK;
}
static double lat_budget(crt_ctx* c)
{
    if (!c->latSlots) c->latSlots = crt_render_resident_waves(c->cfg.device, c->hScene.kind, c->ldsBytes);
    double share = 0.98;
    if (const char* e = hook("CRT_LAT_BUDGET")) { const double v = atof(e); if (v > 0) share = v; }
    return share * (double)c->latSlots;
}

static int upload_block_table(crt_ctx* c, const std::vector<uint8_t>& lanes, const std::vector<uint32_t>& cost)
{
    const uint32_t n = c->tileCount;
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });      // issued most expensive tile first
    std::vector<uint32_t> table; table.reserve((size_t)n * 2);
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t tl = order[r], L = lanes[tl];
        for (uint32_t base = 0; base < 64u; base += L) table.push_back(block_desc(tl, base, L, 0u));
    }
    if (table.size() > 0x7fffffffull) return c->fail(CRT_ERR_INVALID, "block table too large");
    if (hook("CRT_LAT_VERBOSE")) fprintf(stderr, "[crt] latency table: %zu wavefronts for %u tiles (slowest tile of the base stage %.2f ms)\n", table.size(), n, n ? cost[order[0]] * 1e-5 : 0.0);
    if (c->descCap < table.size()) {
        if (c->dBlockDesc) (void)hipFree(c->dBlockDesc);
        if (c->hBlockDesc) (void)hipHostFree(c->hBlockDesc);
        c->dBlockDesc = nullptr; c->hBlockDesc = nullptr; c->descCap = 0;
        const size_t cap = table.size() + table.size() / 2;
        HIPCK(c, hipMalloc((void**)&c->dBlockDesc, cap * 4));
        HIPCK(c, hipHostMalloc((void**)&c->hBlockDesc, cap * 4, hipHostMallocDefault));
        c->descCap = (uint32_t)cap;
    } else if (c->descReady) HIPCK(c, hipEventSynchronize(c->descReady));     // the staging buffer's previous copy (long done)
    HIPCK(c, ensure_event(&c->descReady));
    memcpy(c->hBlockDesc, table.data(), table.size() * 4);
    { const int r = order_behind_ahead(c); if (r) return r; }
    // on the main stream: ordered behind every launch submitted so far (each launch's accumulate waits for it there), so the previous table is no longer read
    HIPCK(c, hipMemcpyAsync(c->dBlockDesc, c->hBlockDesc, table.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->descReady, c->stream));
    c->nBlocks = (uint32_t)table.size();
    return 0;
}

// the costs of stage `c->costStage` have arrived in hTileCost: remember them, then build and install the next stage's table (or, after the last stage, the fastest one's)
static int next_block_table(crt_ctx* c)
{
    const uint32_t n = c->tileCount; const int K = crt_ctx::kLatStages;
    const int s = c->costStage;
    if (s == 0 && !c->latWarm && !c->latProbed) { c->latWarm = true; return 0; }          // measure the one-wave launch once more, warm (a probed stage 0 is not the base of anything: every stage is solved from the one before it)
    c->latCost[s].assign(c->hTileCost, c->hTileCost + n);
    if (s == 0 && !c->latProbed) c->latL[0].assign(n, 64);
    if (c->tuneCount[s] && (c->latBest == s || !c->tuneCount[c->latBest] || c->tuneMs[s] < c->tuneMs[c->latBest])) c->latBest = s;
    bool last = s >= K;
    std::vector<std::pair<double, uint32_t>> steps;
    if (const char* e = hook("CRT_LAT_POLICY")) {
        for (const char* p = e; *p;) {
            char* q = nullptr; const double sh = strtod(p, &q); if (q == p || *q != ':') break;
            const long L = strtol(q + 1, &q, 10); if (L < 1 || L > 64 || (64 % L) != 0) break;
            steps.push_back({sh, (uint32_t)L});
            p = (*q == ',') ? q + 1 : q; if (*q != ',') break;
        }
        if (s >= 1) last = true;
    }
    auto install = [&](int stage) -> int {                                  // the table of an earlier stage back onto the device (an unprobed stage 0 needs none)
        if ((stage != 0 || c->latProbed) && stage != c->latStage) { const int r = upload_block_table(c, c->latL[stage], c->latCost[stage]); if (r) return r; }
        c->latStage = stage; return 0;
    };
    auto fastest = [&](int except) { int b = -1; for (int k = 0; k <= K; k++) if (k != except && c->tuneCount[k] && (b < 0 || c->tuneMs[k] < c->tuneMs[b])) b = k; return b; };
    auto finish = [&]() -> int {
        c->latDone = true; c->latConfirming = false;
        const int b = fastest(-1); c->latBest = b < 0 ? 0 : b;
        if (hook("CRT_LAT_FORCE")) c->latBest = s;                       // diagnostics: keep the last table whatever its time
        if (hook("CRT_LAT_VERBOSE")) { fprintf(stderr, "[crt] latency stages:"); for (int k = 0; k <= K; k++) if (c->tuneCount[k]) fprintf(stderr, " %d: %.2f ms", k, c->tuneMs[k]); fprintf(stderr, " -> %d\n", c->latBest); }
        return install(c->latBest);
    };
    if (c->latConfirming) {                                               // a confirmation launch of stage s has been timed (harvest_tuning keeps each stage's minimum)
        if (!c->latQueue.empty()) c->latQueue.erase(c->latQueue.begin());
        if (!c->latQueue.empty()) return install(c->latQueue.front());
        return finish();
    }
    if (last) {
        // every stage has ONE timing so far, and launch durations scatter by a few per cent: the two fastest stages run once more before the choice is final
        const int a = fastest(-1), b2 = fastest(a);
        if (hook("CRT_LAT_FORCE") || a < 0 || b2 < 0) return finish();
        c->latQueue = {a, b2}; c->latConfirming = true;
        return install(a);
    }
    const int b = c->latBest;                                              // base: the fastest stage so far
    const std::vector<uint8_t>& baseL = c->latL[b]; const std::vector<uint32_t>& baseC = c->latCost[b];
    uint32_t top = 0; for (uint32_t i = 0; i < n; i++) top = baseC[i] > top ? baseC[i] : top;
    std::vector<uint8_t>& L = c->latL[s + 1]; L = baseL;
    if (!steps.empty()) {
        for (uint32_t i = 0; i < n; i++)
            for (const auto& st : steps) if (top > 0 && (double)baseC[i] >= st.first * (double)top) { L[i] = (uint8_t)st.second; break; }
    } else {
        // solved from the LATEST stage's measurement (each tile's cost at the width it just ran is the best estimate of its one-wave cost there is, whether or not
        // that stage was the fastest); keeping the fastest stage guards the choice
        const double T = solve_block_table(c->latL[s], c->latCost[s], lat_budget(c), L);
        if (hook("CRT_LAT_VERBOSE")) fprintf(stderr, "[crt] stage %d: aim %.2f ms\n", s + 1, T * 1e-5);
    }
    const int r = upload_block_table(c, L, steps.empty() ? c->latCost[s] : baseC);
    if (r) return r;
    c->latStage = s + 1;
    return 0;
}

// Timing pairs of launches that have completed are folded into running totals and recycled, so a host that renders forever and never
// asks for the timing (an interactive Tick loop) keeps a bounded number of HIP events alive.
// latency-mode auto-tuning: durations of completed single-window launches, by mode (each launch is looked at once)
static void harvest_tuning(crt_ctx* c)
{
    for (auto& ev : c->evRender) {
        if (ev.mode < 0 || ev.seen) continue;
        if (hipEventQuery(ev.b) != hipSuccess) break;                   // launches complete in order per stream; stop at the first unfinished one
        float t = 0;
        if (hipEventElapsedTime(&t, ev.a, ev.b) == hipSuccess) {
            if (ev.mode >= 100) { double& m = c->jobTrialMs[ev.mode - 100]; m = (m > 0 && m < t) ? m : t; }      // a job of the current plan's shape: plain (100) / planned (101)
            else { c->tuneMs[ev.mode] = c->tuneCount[ev.mode] ? (c->tuneMs[ev.mode] < t ? c->tuneMs[ev.mode] : t) : t; c->tuneCount[ev.mode]++; }
        }
        ev.seen = true;
    }
}

static void fold_completed(crt_ctx* c, std::deque<EventPair>& list, double* ms, uint32_t* count)
{
    while (list.size() > 64 && hipEventQuery(list.front().b) == hipSuccess) {
        float t = 0;
        if (hipEventElapsedTime(&t, list.front().a, list.front().b) == hipSuccess) *ms += t;
        if (count) (*count)++;
        c->evPool.push_back(list.front()); list.pop_front();
    }
}

static int take_event(crt_ctx* c, std::deque<EventPair>& list, EventPair* out)
{
    EventPair ev;
    if (c->evPool.empty()) {
        HIPCK(c, hipEventCreate(&ev.a)); HIPCK(c, hipEventCreate(&ev.b));
    } else { ev = c->evPool.back(); c->evPool.pop_back(); }
    ev.mode = -1; ev.seen = false;
    list.push_back(ev); *out = ev;
    return 0;
}

// Sizes the sample-slab pool for a crt_render of `frames` frames and returns the frames per launch to use (*maxFOut).
// One launch renders up to cfg.maxFramesPerLaunch frames = that many / 64 windows; its samples need windowBytes per window.  The pool
// grows to the high-water mark only (hipMalloc synchronises the device and takes seconds for tens of GB): room for the largest
// launch — for two of them when a call needs several launches — and for at least eight windows (consecutive single-window calls
// overlap on the streams), never more than half of the free HBM.
// The region of render-ahead launch `a` is free once the main stream has passed `a`'s end (a committed launch: behind its last commit)
static int release_ahead_region(crt_ctx* c, const crt_ctx::Ahead& a)
{
    for (auto& r : c->inflight)
        if (r.held && r.off == a.off) { HIPCK(c, hipEventRecord(r.freed, c->stream)); r.held = false; return 0; }
    return c->fail(CRT_ERR_DEVICE, "render-ahead region at %zu is not in the slab ring", a.off);
}

// Drops crt_tick's render-ahead queue.  Kernels of a discarded launch keep running, so the main stream waits for each launch's end before the region's
// `freed` is recorded there (releases stay ordered on the main stream, which take_region's mustWait relies on).
static int discard_ahead(crt_ctx* c)
{
    while (!c->ahead.empty()) {
        const crt_ctx::Ahead a = c->ahead.front(); c->ahead.pop_front();
        HIPCK(c, hipStreamWaitEvent(c->stream, a.end, 0));
        c->doneEvents.push_back(a.end);
        const int r = release_ahead_region(c, a); if (r) return r;
    }
    c->aheadFrames = 0;
    return 0;
}

static int ensure_pool(crt_ctx* c, uint32_t frames, uint32_t passes, uint32_t* maxFOut)
{
    const size_t windowBytes = window_bytes(c, passes);
    uint32_t maxF = (uint32_t)c->cfg.maxFramesPerLaunch;
    uint32_t maxW = maxF >= 64u ? maxF / 64u : 1u;
    const uint32_t wantW = (frames + 63u) / 64u;                                          // (an upper bound when maxF < 64)
    const uint32_t callW = wantW < maxW ? wantW : maxW;                                   // windows of this call's largest launch
    size_t want = (size_t)callW * windowBytes * (wantW > callW ? 2u : 1u);
    if (want < 8 * windowBytes) want = 8 * windowBytes;
    if (want > c->poolBytes && !(c->poolCapped && windowBytes <= c->poolBytes)) {
        { const int r = discard_ahead(c); if (r) return r; }
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (auto st : c->streams) HIPCK(c, hipStreamSynchronize(st));
        if (c->aheadStream) HIPCK(c, hipStreamSynchronize(c->aheadStream));
        for (auto& r : c->inflight) c->freeEvents.push_back(r.freed);
        c->inflight.clear(); c->poolHead = 0;
        if (c->pool) { HIPCK(c, hipFree(c->pool)); c->pool = nullptr; c->poolBytes = 0; }
        size_t freeB = 0, totalB = 0;
        HIPCK(c, hipMemGetInfo(&freeB, &totalB));
        const size_t budget = freeB / 2;
        if (budget < windowBytes) return c->fail(CRT_ERR_DEVICE, "not enough free HBM for one 64-frame sample slab (%zu bytes needed, %zu free)", windowBytes, freeB);
        c->poolCapped = want > budget;
        if (want > budget) want = budget;
        want = want / windowBytes * windowBytes;
        HIPCK(c, hipMalloc((void**)&c->pool, want));
        c->poolBytes = want;
    }
    {   // launches must fit the pool; when the call needs several launches leave room for two in flight
        uint32_t fitW = (uint32_t)(c->poolBytes / windowBytes);
        if (wantW > fitW && fitW >= 2) fitW /= 2;
        if (maxW > fitW) maxW = fitW;
    }
    if (maxF >= 64u) maxF = maxW * 64u;
    *maxFOut = maxF;
    return 0;
}

int crt_reserve(crt_ctx* c, uint32_t frames, uint32_t passes)
{
    if (!c) return CRT_ERR_INVALID;
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "passes must be 1..4");
    HIPCK(c, hipSetDevice(c->cfg.device));
    { const int r = discard_ahead(c); if (r) return r; }
    if (c->tileCount == 0 || frames == 0) return CRT_OK;
    uint32_t maxF = 0;
    return ensure_pool(c, frames, passes, &maxF);
}

// a region of `need` bytes of the slab pool for a launch on stream `st`; regions still in use are waited for on the GPU (never on the host).
// Returns 1 (nothing taken) when the space would have to come from a held render-ahead region.
static int take_region(crt_ctx* c, size_t need, hipStream_t st, size_t* offOut)
{
    for (;;) {
        bool ok = false; size_t off = 0;
        if (c->inflight.empty()) { off = 0; ok = need <= c->poolBytes; }
        else {
            const size_t tail = c->inflight.front().off;                     // oldest region still held
            if (c->poolHead > tail) {                                        // free: [head, end) and [0, tail)
                if (c->poolBytes - c->poolHead >= need) { off = c->poolHead; ok = true; }
                else if (tail >= need) { off = 0; ok = true; }
            } else if (c->poolHead < tail && tail - c->poolHead >= need) { off = c->poolHead; ok = true; }
        }
        if (ok) {
            // every launch is ordered behind the release of ALL space handed out again so far (releases are ordered on the main stream)
            if (c->mustWait) HIPCK(c, hipStreamWaitEvent(st, c->mustWait, 0));
            c->poolHead = off + need; *offOut = off;
            return 0;
        }
        if (c->inflight.empty()) return c->fail(CRT_ERR_DEVICE, "slab pool of %zu bytes cannot hold a launch of %zu bytes", c->poolBytes, need);
        if (c->inflight.front().held) return 1;
        if (c->mustWait) c->freeEvents.push_back(c->mustWait);
        c->mustWait = c->inflight.front().freed;
        c->inflight.pop_front();
    }
}

// the job-cost buffer: one uint32 per tile, then (8-byte aligned) three uint64: ~(first wavefront's start clock), last wavefront's start clock, wave time after it;
// then two of the job's sky launch (render_sky_kernel): ~(first wavefront's start clock), last wavefront's end clock
static size_t job_cost_clk_offset(const crt_ctx* c) { return (((size_t)c->tileCount + 1u) & ~(size_t)1u) * 4u; }
static size_t job_cost_bytes(const crt_ctx* c) { return job_cost_clk_offset(c) + 40u; }

// How many ranks at the end of the tile order a launch leaves to render_sky_kernel: the order's sky tail, when the launch runs the pool kernel of a non-statistics
// context (the statistics build counts the root step of every primary ray) and the class table the order was made with is the current one.  0: one kernel renders
// every tile, as a launch without the table does (stale, or CRT_DEBUG_NO_TILE_CLASS; CRT_DEBUG_NO_SKY_KERNEL keeps the table and drops only the sky launch: A/B runs;
// CRT_POOL_WAVE_FRAMES, the tests' forced range length, describes a pool launch of every tile and gets one).
// Where the sky launch goes: on the next stream, submitted behind the pool launch — its many short wavefronts run in that launch's drain (the default: measured
// faster); CRT_SKY_PLACEMENT=ahead (A/B runs): on the launch's own stream in front of the pool launch.
static bool sky_behind() { const char* e = hook("CRT_SKY_PLACEMENT"); return !(e && !strcmp(e, "ahead")); }
static uint32_t sky_split(const crt_ctx* c, bool pool)
{
    if (!pool || c->cfg.collectStats || c->classDirty || !c->dTileClass || c->hostClass.size() != c->tileCount) return 0u;
    if (hook("CRT_DEBUG_NO_TILE_CLASS") || hook("CRT_DEBUG_NO_SKY_KERNEL")) return 0u;
    if (hook("CRT_POOL_WAVE_FRAMES")) return 0u;                       // (that switch forces a range length "for every tile": the pool launch it describes renders them all)
    return c->skyTiles;
}

// A job's tile costs have arrived (hJobCost): dispatch order = most expensive tile first from now on; and what ONE window of this image costs the machine under
// the pool — the planner's yardstick.  The sum of the wavefront durations is no measure of it (waves that share a SIMD with four others last longer; the
// expensive tiles' wavefronts, which outlive the crowd, do not), so it comes from the launch's dispatch: a launch that oversubscribes the chip keeps every wavefront
// slot busy until its last wavefront starts (S0 = last start - first start), and drains afterwards — the wave time spent after S0, summed by the wavefronts
// themselves, divided by the slots.  One-stream-per-lane launches need 1.2x the pool's machine time (4.24 against 3.52 ms per window on the bunny).
// (the order itself: most expensive first, ties in index order, the sky tiles behind all others)
static uint32_t job_order(const std::vector<uint32_t>& cost, const std::vector<uint8_t>& cls, std::vector<uint32_t>& order)
{
    order.resize(cost.size());
    for (uint32_t i = 0; i < (uint32_t)cost.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    return sky_to_tail(cls, order);
}
// ... in two steps: what the measuring launch left in hJobCost (the costs, its clocks) as the planner's three inputs, and their installation.  The second step
// alone is crt_debug_set_job_costs' (tests: a plan from GIVEN costs — the clocks of a small launch never lead to one).
static void measured_job_costs(const crt_ctx* c, std::vector<uint32_t>& cost, double* poolWindowTicks, double* skyWindowTicks)
{
    const uint32_t n = c->tileCount;
    cost.assign(c->hJobCost, c->hJobCost + n);
    {
        const unsigned long long* clk = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(c->hJobCost) + job_cost_clk_offset(c));
        const double s0 = (clk[0] && clk[1] && clk[1] > ~clk[0]) ? (double)(clk[1] - ~clk[0]) : 0.0;
        const double drain = (double)clk[2] / (double)(c->recResident ? c->recResident : 1u);
        *poolWindowTicks = 0;
        if (c->recWindows && (double)c->recWaves >= 1.5 * (double)c->recResident && s0 > 0) *poolWindowTicks = (s0 + drain) / (double)c->recWindows / (c->recPool ? 1.0 : 1.2);
        if (hook("CRT_LAT_VERBOSE")) fprintf(stderr, "[crt] measured %u windows with %s: %u wavefronts, last one started %.2f ms after the first, then %.2f ms of drain -> %.3f ms of machine time per window under the pool\n", c->recWindows, c->recPool ? "the pool" : "one stream per lane", c->recWaves, s0 * 1e-5, drain * 1e-5, *poolWindowTicks * 1e-5);
    }
    {
        // the job's sky launch, if it had one: its span on the device per window (it shared the machine with the pool launch; the planner adds it to its makespan aim)
        const unsigned long long* clk = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(c->hJobCost) + job_cost_clk_offset(c)) + 3;
        *skyWindowTicks = (c->recWindows && clk[0] && clk[1] > ~clk[0]) ? (double)(clk[1] - ~clk[0]) / (double)c->recWindows : 0.0;
        if (hook("CRT_LAT_VERBOSE")) fprintf(stderr, "[crt] the sky launch of the measuring job: %.3f ms per window\n", *skyWindowTicks * 1e-5);
    }
}
// (the order's copy runs on the main stream behind every launch submitted so far and behind the frames rendered ahead: upload_tile_order)
static int install_job_costs(crt_ctx* c, std::vector<uint32_t>&& cost, double poolWindowTicks, double skyWindowTicks)
{
    c->jobCost = std::move(cost); c->poolWindowTicks = poolWindowTicks; c->skyWindowTicks = skyWindowTicks;
    job_order(c->jobCost, c->hostClass, c->jobOrder);
    c->jobCostValid = true; c->planValid = false;
    return upload_tile_order(c, c->jobOrder);
}
static int adopt_job_costs(crt_ctx* c)
{
    std::vector<uint32_t> cost; double poolWindowTicks = 0, skyWindowTicks = 0;
    measured_job_costs(c, cost, &poolWindowTicks, &skyWindowTicks);
    return install_job_costs(c, std::move(cost), poolWindowTicks, skyWindowTicks);
}

// Plan of a job (one launch of `windows` windows) once the tile costs are known.  A launch ends on its slowest wavefront, and how long a wavefront runs is set by
// the serial chains of its streams: per tile and window, a stream-pool wavefront (128 streams on 64 lanes; the fewest instructions per sample) runs 2.4x as long
// as a one-stream-per-lane wavefront of render_tiles_kernel, and that one can be cut further by handing the tile's 64 streams to 64 / L wavefronts of L lanes
// (kLatG; at 64 / L times the instruction issue).  A job many times longer than its slowest pool wavefront should be all pool; a short one (few windows, or one
// rank's share of a multi-GPU tile split) ends on those wavefronts with the chip nearly empty (tools/pool_timeline.py: 20 windows of the bunny, 4 096 waves in
// flight until 65 ms, then a tail to 83 ms).  The plan is the smallest makespan T for which every tile can take the CHEAPEST class whose wavefronts last <= T
//     pool (2.4 c, if this launch may use the pool) | one wavefront per window (1.1 c under load) | 64 / L wavefronts per window (g(L) c)
// and the machine time of all of them (wave time / wavefronts the chip advances at once) still fits T.  Tiles are sorted by cost, so the classes are contiguous:
// the first `head` tiles of the order go to a block table (render_tiles_kernel, dispatched first), the rest to the pool launch — or, in a launch without the pool,
// everything goes to the table as soon as one tile needs narrow wavefronts.  Returns the table's blocks in `table` (empty: no table needed).
// nSky: the last nSky ranks of the order are the job's sky launch (sky_split) — the plan sees the n ranks in front of them only, and skyTicks, that launch's
// machine time, as time the makespan must hold besides.
static void plan_job(const crt_ctx* c, uint32_t windows, uint32_t frames, bool pool, std::vector<uint32_t>& table, uint32_t* head, uint32_t nSky = 0u, double skyTicks = 0.0)
{
    table.clear(); *head = 0;
    if (nSky >= c->tileCount) return;                                   // an image of sky tiles only: no pool launch, nothing to plan
    const uint32_t n = c->tileCount - nSky;
    if (!c->jobCostValid || windows < 2u || windows > 64u || c->tileCount > 0x10000u || c->cfg.collectStats || hook("CRT_SPLIT_OFF")) return;
    if (pool && c->streams.size() < 2) return;
    if (const char* e = hook("CRT_SPLIT_FORCE")) {                      // tests: the first h tiles through the table, alternating wavefront widths
        const uint32_t h = std::min<uint32_t>((uint32_t)atoi(e), pool ? n - 1u : n);
        static const uint32_t Ls[4] = {64u, 16u, 2u, 1u};
        for (uint32_t r = 0; r < (pool ? h : n); r++) { const uint32_t L = r < h ? Ls[r & 3u] : 64u; for (uint32_t w = 0; w < windows; w++) for (uint32_t b0 = 0; b0 < 64u; b0 += L) table.push_back(block_desc(c->jobOrder[r], b0, L, w)); }
        *head = h; return;
    }
    // cost unit: a pool wavefront's duration per 64 streams while the costs were measured (render_pool_kernel).  In a saturated job the wavefronts of the most expensive
    // tiles run 1.2x longer than that (82 ms against 68 ms on the bunny); one-stream-per-lane wavefronts need 1.2x the machine time of the pool's.
    double poolLong = 2.4, wideLoad = 1.1, poolSlots = 4096.0, wideMt = 1.2, narrowSlots = 3500.0;
    if (const char* e = hook("CRT_PLAN_NARROW_SLOTS")) narrowSlots = atof(e);
    const double K = (double)windows;
    // machine time of one window's pool wavefront of a tile, per unit of its cost: from the measured machine time per window when the measuring launch
    // oversubscribed the chip (adopt_job_costs), else from the wavefront durations (which then ran without much competition)
    double costSum = 0; for (uint32_t v : c->jobCost) costSum += (double)v;
    const double perCost = (c->poolWindowTicks > 0 && costSum > 0) ? c->poolWindowTicks / costSum : 1.0 / poolSlots;
    // machine time (ticks) of tile cost v in the cheapest class that lasts <= T; cls: 0 pool, 1 wide, 2 + k narrow (kLatLanes[k])
    auto cheapest = [&](double v, double T, int* cls) -> double {
        if (pool && poolLong * v <= T) { *cls = 0; return K * v * perCost; }
        if (wideLoad * v <= T) { *cls = 1; return K * wideMt * v * perCost; }
        int k = 1; while (k < 6 && kLatG[k] * v > T) k++;
        *cls = 2 + k; return K * (64.0 / kLatLanes[k]) * kLatG[k] * v / narrowSlots;
    };
    std::vector<uint8_t> planned(c->tileCount, 0); for (uint32_t r = 0; r < n; r++) planned[c->jobOrder[r]] = 1;      // (summed in tile order, whatever the ranks)
    auto machine = [&](double T) { double m = 0; int cls; for (uint32_t i = 0; i < c->tileCount; i++) if (planned[i]) m += cheapest((double)c->jobCost[i], T, &cls); return m + skyTicks; };
    const double top = (double)c->jobCost[c->jobOrder[0]];
    double lo = top * kLatG[6], hi = std::max(poolLong * top, machine(1e30)) * 1.01;
    if (machine(lo) <= lo) hi = lo;
    else for (int it = 0; it < 50; it++) { const double mid = 0.5 * (lo + hi); if (machine(mid) <= mid) hi = mid; else lo = mid; }
    const double T = hi;
    uint32_t h = 0, narrow = 0; std::vector<uint8_t> lanes(n, 64);
    for (uint32_t r = 0; r < n; r++) {
        int cls; (void)cheapest((double)c->jobCost[c->jobOrder[r]], T, &cls);
        if (cls != 0) h = r + 1u;
        if (cls >= 2) { lanes[r] = (uint8_t)kLatLanes[cls - 2]; narrow++; }
    }
    if (pool && h >= n) h = n - 1u;
    if (hook("CRT_LAT_VERBOSE")) fprintf(stderr, "[crt] job of %u windows, %u tiles: makespan aim %.1f ms (most expensive tile %.2f ms); %u tiles to the block table, %u of them narrow, %s\n", windows, n, T * 1e-5, top * 1e-5, pool ? h : (narrow ? n : 0u), narrow, pool ? "rest to the pool" : "no pool");
    if (pool ? h == 0u : narrow == 0u) return;
    const uint32_t upto = pool ? h : n;
    for (uint32_t r = 0; r < upto; r++) {
        const uint32_t L = lanes[r];
        for (uint32_t w = 0; w < windows; w++) {
            const uint32_t fw = std::min(64u, frames - w * 64u);               // frames of this window: no wavefronts for frames past the end
            for (uint32_t b0 = 0; b0 < fw; b0 += L) table.push_back(block_desc(c->jobOrder[r], b0, L, w));
        }
    }
    if (table.size() > (4u << 20)) { table.clear(); *head = 0; return; }          // (never seen: the machine-time bound keeps narrow tiles few; a plain launch is always valid)
    *head = pool ? h : 0u;
}

// Frames per pool wavefront, by tile rank.  A wavefront that owns S frames of a tile spends the last part of its life with its population falling from S to 0; one that
// owns more refills its slots (render_pool_kernel) and pays that ramp-down once per range instead of once per S frames.  But a launch ends on its last wavefront, a
// range of S 2^k frames lasts 2^k times as long, and fewer, longer wavefronts pack the launch's end worse.  So the launch has two parts.  The LONG part renders the frames
// [0, longFrames) of every tile, longFrames = the whole multiples of 8 S frames within `share` of the job: the tile at rank r (dispatch order: most expensive first) is
// expected to start when the machine has worked off the long part of the tiles before it — startTicks + the sum of their machine time, longFrames / 64 x cost x perCost —
// and its wavefronts last poolLong x cost x frames / 128 (plan_job's term: 2.4 = 2 x the 1.2 under load); it gets the largest k <= 3 for which  start + safety x duration <= aim
// (the job's makespan aim: the machine time of everything).  The SHORT part renders the remaining frames of every tile with S frames per wavefront, as a launch without
// refill does, dispatched behind the long part in the same tile order: its many short wavefronts fill the launch's end, and a tile's last wavefront takes the remainder.
// Nothing is lengthened when costs are unknown (cost == nullptr), or when the launch would keep fewer than guard x resident wavefronts — the chip must stay oversubscribed
// for the dispatch order to fill the tail: k is capped lower until it does.  Measured: a 64-window 720p plan that keeps 14 x 4096 wavefronts gains 2 %, a 20-window plan
// that kept 6 x 4096 lost 37 % (it grew the tail the split had removed); the guard is 12.  Needs no GPU (tests:
// crt_debug_pool_wave_plan).  Returns the wavefronts of the launch; wf[r] = frames per wavefront of rank r in the long part, start[r] its expected start; *longFrames = 0:
// every wavefront owns S frames.
// tailTicks / tailWaves: machine time and wavefronts of a launch dispatched BEHIND this one inside the same job (the sky launch: short wavefronts that fill this
// launch's end as its own short part does) — the time is part of the makespan aim, the wavefronts count towards the guard (in this launch's units: S frames each).
struct PoolWaveTerms { double poolLong = 2.4, load = 1.0, safety = 1.0, guard = 12.0, share = 1.0, tailTicks = 0.0, tailWaves = 0.0; };   // (poolLong is the duration UNDER LOAD: it holds the 1.2, plan_job)
static uint64_t pool_wave_plan(const uint32_t* cost, uint32_t nr, uint32_t frames, uint32_t S, double perCost, double startTicks, uint32_t resident, const PoolWaveTerms& tm,
                               std::vector<uint32_t>& wf, uint32_t* longFrames, std::vector<double>* start, double* aimOut)
{
    wf.assign(nr, S); *longFrames = 0;
    if (start) start->assign(nr, 0.0);
    if (aimOut) *aimOut = 0;
    const uint64_t perTile = (frames + S - 1u) / S, plain = (uint64_t)nr * perTile;
    if (!cost || S <= 64u || nr == 0u) return plain;
    const uint32_t F1 = (uint32_t)((double)frames * std::min(tm.share, 1.0)) / (8u * S) * (8u * S);
    if (F1 == 0u) return plain;
    double aim = startTicks, m = startTicks;
    std::vector<double> st(nr);
    for (uint32_t r = 0; r < nr; r++) { st[r] = m; m += (double)(F1 / 64u) * (double)cost[r] * perCost; aim += (double)((frames + 63u) / 64u) * (double)cost[r] * perCost; }
    aim += tm.tailTicks;
    if (start) *start = st;
    if (aimOut) *aimOut = aim;
    if ((double)plain + tm.tailWaves < tm.guard * (double)resident) return plain;
    const uint64_t shortWaves = (uint64_t)nr * ((frames - F1 + S - 1u) / S);
    for (int kMax = 3; kMax >= 1; kMax--) {
        uint64_t waves = shortWaves; bool any = false;
        for (uint32_t r = 0; r < nr; r++) {
            int k = kMax;
            while (k > 0 && st[r] + tm.safety * tm.poolLong * tm.load * (double)cost[r] * (double)((uint64_t)S << k) / 128.0 > aim) k--;
            wf[r] = S << k; any = any || k > 0;
            waves += F1 / wf[r];
        }
        if (!any) break;
        if ((double)waves + tm.tailWaves >= tm.guard * (double)resident) { *longFrames = F1; return waves; }
    }
    wf.assign(nr, S);
    return plain;
}
// the table of the long part of such a launch: first block and frames per wavefront of every rank (render_pool_kernel's waveTab); returns its wavefronts
static uint32_t pool_wave_table(const std::vector<uint32_t>& wf, uint32_t longFrames, uint32_t S, std::vector<uint32_t>& tab, uint32_t* longWaves)
{
    tab.resize(2 * wf.size()); uint32_t b = 0, lw = 0;
    for (size_t r = 0; r < wf.size(); r++) {
        tab[2 * r] = b; tab[2 * r + 1] = wf[r];
        b += longFrames / wf[r];
        if (wf[r] > S) lw += longFrames / wf[r];
    }
    if (longWaves) *longWaves = lw;
    return b;
}
static bool pool_wave_terms(PoolWaveTerms& tm)
{
    if (const char* e = hook("CRT_POOL_REFILL_SAFETY")) { const double v = atof(e); if (v > 0) tm.safety = v; }
    if (const char* e = hook("CRT_POOL_REFILL_GUARD")) { const double v = atof(e); if (v > 0) tm.guard = v; }
    if (const char* e = hook("CRT_POOL_REFILL_SHARE")) { const double v = atof(e); if (v > 0) tm.share = v; }
    return !hook("CRT_POOL_REFILL_OFF");
}
// tests / A-B runs: CRT_POOL_WAVE_FRAMES=<n> forces n frames per pool wavefront for every tile (rounded down to whole groups of S; n = 128 is the launch without refill)
static uint32_t forced_wave_frames(uint32_t S)
{
    const char* e = hook("CRT_POOL_WAVE_FRAMES");
    if (!e) return 0u;
    const long v = atol(e);
    if (v < (long)S) return S;
    return (uint32_t)std::min<long>(v, 8192) / S * S;
}

// The plan of a job's pool launch: pool_wave_plan for the ranks [head, tileCount - nSky) of the order, the head's tiles (block table, dispatched first) as time spent
// before them and the sky launch (skyTicks of machine time; the wavefronts its ranks would have in this launch) as the launch's tail — or, when the sky launch is
// submitted ahead (sky_behind), as time spent before them too.  Appends the wave table to `table` when any wavefront owns
// more than S frames: one entry per rank from `head` to the END of the order, because the kernel's search runs over all of them — a rank of the sky tail gets
// `blocks` as its first block, which no wavefront of the long part reaches.
struct PoolWavePlan { uint32_t off = 0, blocks = 0, longFrames = 0, longWaves = 0, ranks = 0; double aim = 0; };
static PoolWavePlan plan_pool_waves(const crt_ctx* c, uint32_t windows, uint32_t frames, uint32_t head, uint32_t nSky, double skyTicks, std::vector<uint32_t>& table)
{
    PoolWavePlan p;
    PoolWaveTerms terms;
    const uint32_t S = crt_pool_streams(frames);
    if (!c->jobCostValid || c->cfg.collectStats || head + nSky >= c->tileCount || !pool_wave_terms(terms) || forced_wave_frames(S)) return p;
    const uint32_t nr = c->tileCount - nSky - head;
    p.ranks = nr;
    std::vector<uint32_t> cost(nr), wf, tab;
    double costSum = 0; for (uint32_t v : c->jobCost) costSum += (double)v;
    const double perCost = (c->poolWindowTicks > 0 && costSum > 0) ? c->poolWindowTicks / costSum : 1.0 / 4096.0;
    double startTicks = 0;
    if (sky_behind()) { terms.tailTicks = skyTicks; terms.tailWaves = (double)nSky * (double)((frames + S - 1u) / S); } else startTicks = skyTicks;
    for (uint32_t r = 0; r < head; r++) startTicks += (double)windows * 1.2 * (double)c->jobCost[c->jobOrder[r]] * perCost;      // (one stream per lane: 1.2 x the pool's machine time)
    for (uint32_t r = 0; r < nr; r++) cost[r] = c->jobCost[c->jobOrder[head + r]];
    uint32_t F1 = 0, lw = 0, blocks = 0;
    pool_wave_plan(cost.data(), nr, frames, S, perCost, startTicks, 4096u, terms, wf, &F1, nullptr, &p.aim);
    if (F1) blocks = pool_wave_table(wf, F1, S, tab, &lw);
    if (lw) {
        for (uint32_t r = 0; r < nSky; r++) { tab.push_back(blocks); tab.push_back(S); }
        p.off = (uint32_t)table.size(); p.blocks = blocks; p.longFrames = F1; p.longWaves = lw;
        table.insert(table.end(), tab.begin(), tab.end());
    }
    if (hook("CRT_LAT_VERBOSE")) {
        uint32_t cnt[4] = {0, 0, 0, 0}; double share[4] = {0, 0, 0, 0}, sum = 0;
        for (uint32_t r = 0; r < nr; r++) { int k = 0; while ((S << k) < wf[r]) k++; cnt[k]++; share[k] += cost[r]; sum += cost[r]; }
        fprintf(stderr, "[crt] pool launch of %u ranks x %u frames (%u sky ranks behind them: %.2f ms): aim %.1f ms, most expensive tile %.2f ms, long part %u frames in %u wavefronts, %u of them own more than %u frames (safety %.2f, guard %.1f x 4096, share %.2f); tiles by frames per wavefront (share of the cost):",
                nr, frames, nSky, skyTicks * 1e-5, p.aim * 1e-5, nr ? cost[0] * 1e-5 : 0.0, F1, blocks, lw, S, terms.safety, terms.guard, terms.share);
        for (int k = 0; k < 4; k++) fprintf(stderr, " %u: %u (%.3f)", S << k, cnt[k], sum > 0 ? share[k] / sum : 0.0);
        fprintf(stderr, "\n");
    }
    return p;
}

// Machine time of a job's sky launch, for the planner's makespan aim: what the measuring job's sky launch took per window (adopt_job_costs).  0 when that job had
// none — it ran one stream per lane, below the pool's size: the sky tiles' costs it measured bound the sky launch from above, but an aim raised by them made the plan
// slower than the parent's, so nothing is assumed about a launch that was not measured.
static double sky_launch_ticks(const crt_ctx* c, uint32_t windows, uint32_t nSky)
{
    return (nSky && c->jobCostValid) ? c->skyWindowTicks * (double)windows : 0.0;
}

// ... and its table on the device (cached for launches of the same shape)
static int install_job_plan(crt_ctx* c, uint32_t windows, uint32_t frames, bool pool)
{
    const uint32_t asked = sky_split(c, pool);
    if (c->planValid && c->planWindows == windows && c->planFrames == frames && c->planPool == pool && c->planSkyAsked == asked) return 0;
    uint32_t nSky = asked;
    double skyTicks = sky_launch_ticks(c, windows, nSky);
    std::vector<uint32_t> table; uint32_t head = 0;
    plan_job(c, windows, frames, pool, table, &head, nSky, skyTicks);
    if (head && nSky) {
        // A job that needs the block table ends on its most expensive tiles' wavefronts, not on machine time, and there a sky launch beside the pool launch was
        // measured to COST its own duration (20 windows of the bunny: +5 %, whatever its placement or priority): such a job keeps its sky tiles
        // in the pool launch, at the end of its dispatch order, as before.
        nSky = 0; skyTicks = 0;
        plan_job(c, windows, frames, pool, table, &head);
    }
    c->planValid = true; c->planWindows = windows; c->planFrames = frames; c->planPool = pool; c->planSkyAsked = asked; c->planSky = nSky; c->jobHead = head; c->jobBlocks = (uint32_t)table.size();
    c->jobTrialMs[0] = c->jobTrialMs[1] = 0;
    c->jobWaveOff = c->jobWaveBlocks = c->jobLongFrames = c->jobLongWaves = 0;
    if (pool) {
        const PoolWavePlan p = plan_pool_waves(c, windows, frames, head, nSky, skyTicks, table);
        c->jobWaveOff = p.off; c->jobWaveBlocks = p.blocks; c->jobLongFrames = p.longFrames; c->jobLongWaves = p.longWaves;
    }
    if (table.empty()) return 0;
    if (c->jobDescCap < table.size()) {
        if (c->dJobDesc) (void)hipFree(c->dJobDesc);
        if (c->hJobDesc) (void)hipHostFree(c->hJobDesc);
        c->dJobDesc = nullptr; c->hJobDesc = nullptr; c->jobDescCap = 0;
        const size_t cap = table.size() + table.size() / 2;
        HIPCK(c, hipMalloc((void**)&c->dJobDesc, cap * 4));
        HIPCK(c, hipHostMalloc((void**)&c->hJobDesc, cap * 4, hipHostMallocDefault));
        c->jobDescCap = (uint32_t)cap;
    } else if (c->jobDescReady) HIPCK(c, hipEventSynchronize(c->jobDescReady));
    HIPCK(c, ensure_event(&c->jobDescReady));
    memcpy(c->hJobDesc, table.data(), table.size() * 4);
    { const int r = order_behind_ahead(c); if (r) return r; }
    HIPCK(c, hipMemcpyAsync(c->dJobDesc, c->hJobDesc, table.size() * 4, hipMemcpyHostToDevice, c->stream));      // main stream: behind every launch submitted so far
    HIPCK(c, hipEventRecord(c->jobDescReady, c->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// One render launch of crt_render = the three steps below, each owning its part of the context:
//   tuner_prepare     single-window launches (8 .. 64 frames): the LATENCY tuner — owns lat*, cost*, dBlockDesc / nBlocks* (probe, stages, confirmation: next_block_table)
//   planner_prepare   jobs (> 64 frames): tile-cost measurement and the PLANNER — owns jobCost*, rec*, plan*, dJobDesc / jobBlocks*, jobTrial* (plan_job, install_job_plan)
//   launch_render_kernels   the LAUNCHER: render_pool_kernel / render_tiles_kernel on their streams, joined before the launch's end event
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct Launch {
    hipStream_t st = nullptr; EventPair ev{}; void* slab = nullptr; uint32_t sppFirst = 0, nf = 0, passes = 1, windows = 1;
    const uint32_t* blockDesc = nullptr; uint32_t nBlocks = 0;      // the latency mode's table (single-window launch), or none
    bool wantCost = false, wantJobCost = false, pool = false;
    uint32_t head = 0, jobBlocks = 0; unsigned long long* jobClk = nullptr;      // a planned job: table blocks + first tile rank of the pool launch
    uint32_t waveFrames = 0, waveBlocks = 0, longFrames = 0, longWaves = 0; const uint32_t* waveTab = nullptr;   // the pool launch's frames per wavefront: one for all (0: S), or per rank (table of waveBlocks wavefronts)
    uint32_t sky = 0;                                               // ranks at the end of the order that go to render_sky_kernel (sky_split); the pool launch renders the ranks in front of them
    // the sky launch writes its tiles' blocks in the texel form (device/sample_body.h) and the launch's accumulate reads the ranks [tileCount - sky, tileCount) as
    // such: only where that accumulate follows at once (launch_frames) — never a render-ahead launch, whose frames are committed after the order may have changed
    bool skyTexels = false;
};

static int next_block_table(crt_ctx* c);
static int probe_tile_costs(crt_ctx* c, hipStream_t st);

static int tuner_prepare(crt_ctx* c, Launch& L)
{
    int r;
    // ... only when the GPU is idle at submission: a caller that queues launch after launch wants throughput, and narrow wavefronts buy latency with issue
    // slots (56 queued single-window calls: 6.4 ms each with one wave per tile, 12.4 ms with the tuned table)
    const bool gpuIdle = !c->lastRenderEnd || hipEventQuery(c->lastRenderEnd) == hipSuccess;
    if (L.nf <= 64u && L.nf >= 8u && gpuIdle && !c->cfg.collectStats && c->tileCount <= 0x10000u && !hook("CRT_LAT_OFF")) {
        if (c->costPending && hipEventQuery(c->costCopied) == hipSuccess) { c->costPending = false; harvest_tuning(c); if ((r = next_block_table(c))) return r; }
        if (c->latStage == 0 && !c->latProbed && !c->latWarm && !c->costPending && L.nf == 64u && !hook("CRT_LAT_POLICY") && !hook("CRT_LAT_NO_PROBE")) { if ((r = probe_tile_costs(c, L.st))) return r; }
        const int stage = c->latStage;
        if (stage || c->latProbed) { L.blockDesc = c->dBlockDesc; L.nBlocks = c->nBlocks; HIPCK(c, hipStreamWaitEvent(L.st, c->descReady, 0)); }
        L.wantCost = (!c->latDone && !c->costPending) || (c->latDone && hook("CRT_LAT_RECORD"));      // (the latter: diagnostics, crt_debug_tile_costs)
        c->evRender.back().mode = c->latDone ? -1 : stage;
        if (L.wantCost && !c->latDone) c->costStage = stage;
    }
    if (L.wantCost) {
        if (!c->dTileCost) {
            HIPCK(c, hipMalloc((void**)&c->dTileCost, (size_t)c->tileCount * 4));
            HIPCK(c, hipHostMalloc((void**)&c->hTileCost, (size_t)c->tileCount * 4, hipHostMallocDefault));
            HIPCK(c, ensure_event(&c->costCopied));
        }
        else HIPCK(c, hipStreamWaitEvent(L.st, c->costCopied, 0));          // behind an earlier measurement (possibly on another stream) that a camera change abandoned
        HIPCK(c, hipMemsetAsync(c->dTileCost, 0, (size_t)c->tileCount * 4, L.st));
    }
    return 0;
}

static int planner_prepare(crt_ctx* c, Launch& L)
{
    int r;
    // jobs: measure the tile costs once per camera / scene (first job launch), adopt them when they have arrived
    if (L.nf > 64u && !c->cfg.collectStats) {
        if (c->jobCostPending && hipEventQuery(c->jobCostCopied) == hipSuccess) { c->jobCostPending = false; if ((r = adopt_job_costs(c))) return r; HIPCK(c, hipStreamWaitEvent(L.st, c->orderReady, 0)); }
        L.wantJobCost = !c->jobCostValid && !c->jobCostPending && L.nf >= 128u;       // (a pool launch records full 128-stream wavefronts only)
        if (L.wantJobCost) {
            if (!c->dJobCost) {
                HIPCK(c, hipMalloc((void**)&c->dJobCost, job_cost_bytes(c)));
                HIPCK(c, hipHostMalloc((void**)&c->hJobCost, job_cost_bytes(c), hipHostMallocDefault));
                HIPCK(c, ensure_event(&c->jobCostCopied));
            } else HIPCK(c, hipStreamWaitEvent(L.st, c->jobCostCopied, 0));      // behind an earlier measurement that a camera change abandoned
            HIPCK(c, hipMemsetAsync(c->dJobCost, 0, job_cost_bytes(c), L.st));
        }
    }
    // Which render kernel: the stream pool executes a third fewer instructions per sample, but its wavefronts own 128 streams for 64 lanes, so the most
    // expensive tiles take about twice as long per wavefront; a launch that is not many times larger than the machine (4 096 - 5 120 wavefronts in
    // flight) ends on those and is faster with one stream per lane.  Measured cross-over (tools/crossover.py, bench.py --steps): bunny 1280x720 at 17 - 20
    // windows (20 windows: 81.0 ms pool, 87.6 ms tiles), TLAS scene at ~28, watch-tower 1920x1080 at 7 — 56 000 ... 100 000 (tile, window) pairs; the
    // threshold sits at the low end of that range.
    // With the tile costs known (most expensive first + split, see plan_job) the pool is never slower than one stream per lane from ~12 windows of 720p on
    // (tools/split_probe.py: bunny 14 windows 57.8 against 59.6 ms, two-level scene 16 windows 79 against 94 ms, watch-tower 1080p 7 windows 155.6 against 161.1 ms).
    // A scene in the 32-bit pool-reference form (layout.h; 4-byte stack entries: 13 KB of LDS per wavefront at a stack depth of 20, 3 waves per SIMD): the pool did not
    // beat one stream per lane at any job size measured (14-bunny scene 1280x720, tools/pool_wide_bench.py, profiles/pool_wide.json: 12 / 20 / 64 windows 249.3 /
    // 413.7 / 1299.9 ms against 245.9 / 407.8 / 1293.1 ms, scatter <= 0.2 %), so by default such a scene is rendered by render_tiles_kernel at every size and the
    // pool is reached through CRT_RENDER_KERNEL=pool_always alone.  (Scene-dependent: on the 4-bunny scenes the 32-bit pool is 7 - 11 % faster)
    const bool poolByDefault = c->hScene.poolRefBits == 16u || c->poolMinWaves == 0;
    const uint64_t minWaves = c->poolMinWaves != 65000u ? c->poolMinWaves : (c->jobCostValid ? 43000u : 65000u);
    L.pool = c->usePool && poolByDefault && pool_can_run(c, L.nf) && (uint64_t)c->tileCount * L.windows >= minWaves && (c->poolMinWaves == 0 || L.nf > 64u);
    L.sky = sky_split(c, L.pool);
    if (L.nf > 64u && c->jobCostValid) {
        if ((r = install_job_plan(c, L.windows, L.nf, L.pool))) return r;
        // The plan is a MODEL (machine time within ~15 %): for a job shape that repeats (a progressive render) it is checked by measurement — the first launch of the
        // shape runs planned, the second plain (same kernel choice, cost-ordered, no table), and whichever was faster is kept: "planned is never slower than the
        // plain launch" holds by construction from the third launch on (tags 100 / 101 of the timing pairs, harvest_tuning).
        int use = 1;                                                           // 1 planned, 0 plain
        if ((c->jobBlocks || c->jobLongWaves) && !hook("CRT_PLAN_NO_TRIAL")) {
            if (c->jobTrialMs[1] > 0 && c->jobTrialMs[0] > 0) use = c->jobTrialMs[1] <= c->jobTrialMs[0] ? 1 : 0;
            else if (c->jobTrialMs[1] > 0 && c->jobTrialMs[0] == 0) use = 0;   // the planned launch has been timed: time the plain one
            c->evRender.back().mode = 100 + use;
        }
        if (use) L.sky = c->planSky;                                        // (the planned launch: what its table was made for — none beside a block table)
        if (use) { L.head = c->jobHead; L.jobBlocks = c->jobBlocks; if (L.pool && c->jobLongWaves) { L.waveTab = c->dJobDesc + c->jobWaveOff; L.waveBlocks = c->jobWaveBlocks; L.longFrames = c->jobLongFrames; L.longWaves = c->jobLongWaves; } }
    }
    if (L.pool) if (const uint32_t S = crt_pool_streams(L.nf); const uint32_t n = forced_wave_frames(S)) {
        L.waveFrames = n; L.waveTab = nullptr; L.waveBlocks = 0;
        L.longWaves = n > S ? (c->tileCount - L.sky - L.head) * (L.nf / n + ((L.nf % n) > S ? 1u : 0u)) : 0u;
    }
    if (L.jobBlocks || L.waveTab) HIPCK(c, hipStreamWaitEvent(L.st, c->jobDescReady, 0));
    if (L.wantJobCost) {                                                 // what adopt_job_costs needs to know about the measuring launch
        L.jobClk = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(c->dJobCost) + job_cost_clk_offset(c));
        c->recPool = L.pool; c->recWindows = L.windows;
        const uint32_t perWave = L.pool ? std::max(crt_pool_streams(L.nf), L.waveFrames) : 64u;
        c->recWaves = L.pool ? (c->tileCount - L.sky) * ((L.nf + perWave - 1u) / perWave) : c->tileCount * L.windows;
        c->recResident = L.pool ? 4096u : 5120u;                            // 4 / 5 wavefronts per SIMD (render_pool_kernel / render_tiles_kernel)
        if (L.pool && c->hScene.poolRefBits == 32u)                         // the 32-bit-reference form: what its LDS leaves of those 4 (160 KiB per CU of 4 SIMDs)
            c->recResident = 256u * std::min(16u, (160u * 1024u) / std::max(1u, pool_lds_need(c, L.nf)));
    }
    return 0;
}

static hipError_t launch_render_kernels(crt_ctx* c, const Launch& L)
{
    hipStream_t st = L.st;
    hipError_t le = hipSuccess;
    // a second kernel of the same launch on another stream: released by the launch's start event, joined before its end event
    auto join = [&](hipStream_t other) -> hipError_t {
        if (other == st) return hipSuccess;
        hipError_t e = hipSuccess;
        if (c->splitEvents.size() < 32) { hipEvent_t ne; e = hipEventCreateWithFlags(&ne, hipEventDisableTiming); if (e == hipSuccess) c->splitEvents.push_back(ne); }
        if (e == hipSuccess) { hipEvent_t je = c->splitEvents[c->splitSeq++ % c->splitEvents.size()]; e = hipEventRecord(je, other); if (e == hipSuccess) e = hipStreamWaitEvent(st, je, 0); }
        return e;
    };
    // a block table: render_tiles_kernel on this launch's stream
    auto launch_table = [&](const uint32_t* desc, uint32_t nBlocks, uint32_t* cost) -> hipError_t {
        return crt_launch_render(&c->hScene, L.slab, c->dCounters, c->dTileClocks, c->dTileOrder, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX,
                                 L.sppFirst, L.nf, L.passes, c->ldsBytes, 0, desc, nBlocks, cost, 0u, nullptr, st);
    };
    if (L.pool) {
        void* scratch = (char*)L.slab + (size_t)L.windows * sample_bytes_per_window(c, L.passes);
        hipStream_t st2 = st;
        // The order's sky tail goes to render_sky_kernel, inside the launch's event pair and joined in front of its end event (placement: sky_behind)
        const bool skyBehind = sky_behind();
        auto launch_sky = [&](hipStream_t s) -> hipError_t {
            return crt_launch_render_sky(&c->hScene, L.slab, c->dCounters, c->dTileOrder, c->tileCount - L.sky, L.sky, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX,
                                         L.sppFirst, L.nf, L.passes, L.skyTexels ? 1 : 0, L.jobClk ? L.jobClk + 3 : nullptr, s);
        };
        if (L.sky && !skyBehind) { le = launch_sky(st); if (le == hipSuccess) c->skyLaunches++; }
        if (le != hipSuccess) return le;
        if (L.jobBlocks) {
            // the expensive tiles first, through the block table, on this launch's stream; the pool for the rest on the next stream, released by the same start event
            le = launch_table(c->dJobDesc, L.jobBlocks, nullptr);
            st2 = c->streams[(size_t)(c->launchSeq++ % c->streams.size())];
            if (le == hipSuccess && st2 != st) le = hipStreamWaitEvent(st2, L.ev.a, 0);
        }
        if (le == hipSuccess)
            le = crt_launch_render_pool(&c->hScene, L.slab, scratch, c->dCounters, c->dTileClocks, c->dTileOrder, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX,
                                        L.sppFirst, L.nf, L.passes, c->cfg.collectStats, L.jobBlocks ? L.head : 0u, c->tileCount - L.sky, L.waveFrames, L.waveTab, L.waveBlocks, L.longFrames,
                                        L.wantJobCost ? c->dJobCost : nullptr, L.jobClk,
                                        (c->classDirty || hook("CRT_DEBUG_NO_TILE_CLASS")) ? nullptr : c->dTileClass /* tests / A-B: the kernel without the table */, c->extraLds, st2);
        if (le == hipSuccess) c->lastLongWaves = L.longWaves;
        if (L.jobBlocks && le == hipSuccess) le = join(st2);
        if (L.sky && skyBehind && le == hipSuccess) {
            // ... on a stream of the lowest priority: "behind" is a dispatch preference, not an order — at equal priority the sky launch's wavefronts are dispatched
            // beside the pool launch's first ones and a short job, which ends on its most expensive tiles' wavefronts, ends later by the sky launch's whole duration
            // (CRT_SKY_PRIORITY=normal: the next render stream; the A/B of DESIGN.md section 5)
            if (!c->skyStream && !hook("CRT_SKY_PRIORITY")) {
                int least = 0, greatest = 0;
                le = hipDeviceGetStreamPriorityRange(&least, &greatest);
                if (le == hipSuccess) le = hipStreamCreateWithPriority(&c->skyStream, hipStreamNonBlocking, least);
                if (le != hipSuccess) return le;
            }
            hipStream_t st3 = c->skyStream;
            if (hook("CRT_SKY_PRIORITY")) { st3 = c->streams[(size_t)(c->launchSeq++ % c->streams.size())]; if (st3 == st2 && c->streams.size() > 1) st3 = c->streams[(size_t)(c->launchSeq++ % c->streams.size())]; }
            if (st3 != st) le = hipStreamWaitEvent(st3, L.ev.a, 0);
            if (le == hipSuccess) le = launch_sky(st3);
            if (le == hipSuccess) { c->skyLaunches++; le = join(st3); }
        }
    } else if (L.jobBlocks) {
        le = launch_table(c->dJobDesc, L.jobBlocks, nullptr);
    } else if (L.blockDesc && L.nBlocks) {
        le = launch_table(L.blockDesc, L.nBlocks, L.wantCost ? c->dTileCost : nullptr);
    } else {
        le = crt_launch_render(&c->hScene, L.slab, c->dCounters, c->dTileClocks, c->dTileOrder, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX,
                               L.sppFirst, L.nf, L.passes, c->ldsBytes, c->cfg.collectStats, nullptr, 0u,
                               L.wantCost ? c->dTileCost : (L.wantJobCost ? c->dJobCost : nullptr), 0u, L.jobClk, st);
    }
    if (L.jobBlocks && le == hipSuccess) c->splitLaunches++;
    return le;
}

// The first single-window launch after a camera / scene change used to run one wavefront per tile (34 ms for the 720p bunny) because nothing was known about the
// tiles.  Now a probe launch (render_seq_kernel<.., true>: 512 paths per tile, two through every pixel, one per lane) counts the steps those paths take and stage 0 of the latency mode is a
// block table solved from that estimate (solve_block_table).  The call waits for the probe (the only host wait of crt_render, once per camera / scene).
static int probe_tile_costs(crt_ctx* c, hipStream_t st)
{
    const uint32_t n = c->tileCount;
    if (!c->dTileCost) {
        HIPCK(c, hipMalloc((void**)&c->dTileCost, (size_t)n * 4));
        HIPCK(c, hipHostMalloc((void**)&c->hTileCost, (size_t)n * 4, hipHostMallocDefault));
        HIPCK(c, ensure_event(&c->costCopied));
    } else HIPCK(c, hipEventSynchronize(c->costCopied));                   // an earlier measurement that a camera change abandoned
    const auto tp0 = std::chrono::steady_clock::now();
    HIPCK(c, crt_launch_probe(&c->hScene, c->tileFirst, c->tileStride, n, (uint32_t)c->tilesX, c->dTileCost, st));
    HIPCK(c, hipMemcpyAsync(c->hTileCost, c->dTileCost, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCK(c, hipEventRecord(c->costCopied, st));
    HIPCK(c, hipStreamSynchronize(st));
    // steps of the probe's paths -> an estimate in the units the tuner's model uses: only ratios matter (aims are fractions of the most expensive tile)
    const auto tp1 = std::chrono::steady_clock::now();
    std::vector<uint32_t>& est = c->latCost[0]; est.assign(c->hTileCost, c->hTileCost + n);
    // measured (tools/probe_quality.py; bunny, watch-tower, two-level scene): a tile's one-wavefront duration is AFFINE in the probe's step count — 84 - 113 ticks per step
    // plus 3.7 - 4.8 ms that every tile pays for its 16 384 paths whatever they hit (ray generation, the sky lookup, the sample store): 15 - 22 steps' worth per probed path.
    // With the constant added the estimate ranks the expensive tiles to 6 - 9 % (without: 10 - 20 %, the cheap half of them overrated).
    for (uint32_t i = 0; i < n; i++) est[i] += 18u * crt_probe_paths();
    std::vector<uint8_t>& L = c->latL[0]; L.assign(n, 64);
    solve_block_table(std::vector<uint8_t>(n, 64), est, lat_budget(c), L);
    c->latProbed = true;
    bool any = false; for (uint32_t i = 0; i < n; i++) any = any || L[i] != 64;
    if (!any) { c->latProbed = false; return 0; }                           // nothing to narrow: stage 0 stays one wavefront per tile
    const auto tp2 = std::chrono::steady_clock::now();
    const int r = upload_block_table(c, L, est);
    if (hook("CRT_LAT_VERBOSE")) { const auto tp3 = std::chrono::steady_clock::now(); auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[crt] cost probe: launch + wait %.3f ms, table solved in %.3f ms, uploaded in %.3f ms\n", ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3)); }
    return r;
}

// One render launch of frames [sppFirst, sppFirst + nf * passes) on stream `st`: a slab region, tuner_prepare, planner_prepare, launch_render_kernels.
// ahead == nullptr: a launch of crt_render — the ordered accumulate follows on the main stream and the region is released behind it.  Otherwise a
// render-ahead launch of crt_tick: no accumulate; the region stays held and *ahead describes the launch (its end event recorded on `st`).
// Returns 1 (nothing launched) when a render-ahead launch finds no room in the ring short of a held region.
static int launch_frames(crt_ctx* c, uint32_t sppFirst, uint32_t nf, uint32_t passes, hipStream_t st, crt_ctx::Ahead* ahead)
{
    const size_t windowBytes = window_bytes(c, passes);
    size_t off = 0; int r;
    if ((r = take_region(c, (size_t)((nf + 63u) / 64u) * windowBytes, st, &off))) return r;
    if (c->orderReady) HIPCK(c, hipStreamWaitEvent(st, c->orderReady, 0));
    if ((r = wait_scene(c, st))) return r;
    void* slab = c->pool + off;
    EventPair ev;
    harvest_tuning(c);
    fold_completed(c, c->evRender, &c->foldedRenderMs, &c->foldedLaunches); fold_completed(c, c->evAcc, &c->foldedAccMs, nullptr);
    if ((r = take_event(c, c->evRender, &ev))) return r;
    // the pair is in the timing list from here on; any error exit before its end event is recorded takes it back (a half-recorded pair would make every
    // later crt_get_timing fail in hipEventElapsedTime)
    struct PairGuard { crt_ctx* c; bool armed; ~PairGuard() { if (armed && !c->evRender.empty()) { c->evPool.push_back(c->evRender.back()); c->evRender.pop_back(); } } } pairGuard{c, true};
    Launch L; L.st = st; L.ev = ev; L.slab = slab; L.sppFirst = sppFirst; L.nf = nf; L.passes = passes; L.windows = (nf + 63u) / 64u;
    if ((r = tuner_prepare(c, L))) return r;                       // single-window launches: latency mode (block table, tile-cost measurement)
    if ((r = planner_prepare(c, L))) return r;                     // jobs: tile-cost measurement, kernel choice, plan (block table + pool split) or plain launch
    L.skyTexels = ahead == nullptr;                                // (the accumulate below reads the sky launch's ranks; crt_tick's commits could not tell them later)
    HIPCK(c, hipEventRecord(ev.a, st));
    const bool pool = L.pool, wantCost = L.wantCost, wantJobCost = L.wantJobCost;
    const hipError_t le = hook("CRT_DEBUG_FAIL_LAUNCH") ? hipErrorInvalidConfiguration /* tests: the runtime refuses the launch */ : launch_render_kernels(c, L);
    if (le != hipSuccess) {
        // a launch that failed has rendered nothing: its timing pair goes back (pairGuard), the accumulator and the region bookkeeping stay untouched —
        // the frames before it are in, this one and the rest are not — and the error is reported
        return c->hip(le, pool ? "launch of render_pool_kernel" : "launch of render_tiles_kernel");
    }
    if (pool && L.sky < c->tileCount) c->poolLaunches++;           // (an image of sky tiles only: the sky launch was the whole job)
    HIPCK(c, hipEventRecord(ev.b, st));
    pairGuard.armed = false;
    c->lastRenderEnd = ev.b;
    if (wantJobCost) {
        HIPCK(c, hipMemcpyAsync(c->hJobCost, c->dJobCost, job_cost_bytes(c), hipMemcpyDeviceToHost, st));
        HIPCK(c, hipEventRecord(c->jobCostCopied, st));
        c->jobCostPending = true;
    }
    if (wantCost && !pool && !c->latDone) {                                                // the tile costs travel to the host behind the launch; looked at by a later crt_render
        HIPCK(c, hipMemcpyAsync(c->hTileCost, c->dTileCost, (size_t)c->tileCount * 4, hipMemcpyDeviceToHost, st));
        HIPCK(c, hipEventRecord(c->costCopied, st));
        c->costPending = true;
    }
    crt_ctx::Region reg; reg.off = off; reg.bytes = (size_t)((nf + 63u) / 64u) * windowBytes;
    if (c->freeEvents.empty()) HIPCK(c, hipEventCreateWithFlags(&reg.freed, hipEventDisableTiming));
    else { reg.freed = c->freeEvents.back(); c->freeEvents.pop_back(); }
    if (ahead) {                                                    // render-ahead: the frames are committed one by one by later crt_tick calls
        hipEvent_t end = nullptr;
        if (c->doneEvents.empty()) { const hipError_t e = hipEventCreateWithFlags(&end, hipEventDisableTiming); if (e != hipSuccess) { c->freeEvents.push_back(reg.freed); return c->hip(e, "hipEventCreate"); } }
        else { end = c->doneEvents.back(); c->doneEvents.pop_back(); }
        const hipError_t e = hipEventRecord(end, st);
        if (e != hipSuccess) { c->doneEvents.push_back(end); c->freeEvents.push_back(reg.freed); return c->hip(e, "hipEventRecord"); }
        reg.held = true;
        c->inflight.push_back(reg);
        *ahead = crt_ctx::Ahead{end, off, (const char*)slab, c->epoch, sppFirst, nf, passes, 0u};
        return 0;
    }
    // ordered accumulation on the main stream (frame order = launch order), behind this launch.
    // Which of the launch's tile blocks hold the texel form is told in RANKS of the tile order: the sky launch's [tileCount - sky, tileCount).  Invariant: this
    // accumulate reads the order the launch's kernels read.  Every copy to dTileOrder (upload_tile_order, from update_tile_order in crt_render and from
    // adopt_job_costs in planner_prepare above) is enqueued on the main stream: one made before this point is in front of this accumulate and is the one the
    // render kernels waited for (orderReady); a later one is enqueued behind this accumulate on the same stream.  The class table (update_tile_class) and the job
    // table follow the same protocol and are not read here at all.
    HIPCK(c, hipStreamWaitEvent(c->stream, ev.b, 0));
    if ((r = take_event(c, c->evAcc, &ev))) return r;
    HIPCK(c, hipEventRecord(ev.a, c->stream));
    const uint32_t texelFirst = (L.pool && L.skyTexels) ? c->tileCount - L.sky : c->tileCount;     // (launch_render_kernels: a sky launch runs beside a pool launch only)
    HIPCK(c, crt_launch_accumulate(slab, c->dAcc, c->dTileOrder, texelFirst, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, nf, passes, c->stream));
    HIPCK(c, hipEventRecord(ev.b, c->stream));
    HIPCK(c, hipEventRecord(reg.freed, c->stream));
    c->inflight.push_back(reg);
    return 0;
}

int crt_render(crt_ctx* c, uint32_t spp_first, uint32_t frames, uint32_t passes)
{
    if (!c) return CRT_ERR_INVALID;
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "crt_render before crt_upload_scene");
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "passes must be 1..4 (the reference's UI range, renderer.cpp:178)");
    HIPCK(c, hipSetDevice(c->cfg.device));
    { int r = discard_ahead(c); if (r) return r; }                 // (a held region must never be handed out again: see take_region)
    if (c->tileCount == 0 || frames == 0) return CRT_OK;
    { int r = update_tile_class(c); if (r) return r; }            // (first: the order ends with the table's sky tiles)
    { int r = update_tile_order(c); if (r) return r; }
    if (c->streams.empty()) {
        int n = c->cfg.renderStreams;
        if (n <= 0) n = 7;
        if (n > 16) n = 16;
        if (c->cfg.collectStats) n = 1;                       // per-tile clocks of a statistics context describe ONE launch
        c->streams.resize((size_t)n);
        for (auto& st : c->streams) HIPCK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
    uint32_t maxF = 0;
    { int r = ensure_pool(c, frames, passes, &maxF); if (r) return r; }
    const size_t windowBytes = window_bytes(c, passes);
    if (c->renderAccel != 0 || c->havePrim) {
        // Renderer::Sample through FileScene's KD-tree / grid, or over the PrimitiveScene (crt_set_render_accel): the sequential form — one wavefront per (tile, window), lane = frame — on the
        // main stream, followed by the ordered accumulate; no planning, no latency mode (the BASELINE configurations are BVH-SAH; this path exists for parity
        // with the reference's shipped FileScene, which traces through its KD-tree: file_scene.h:10-12)
        for (uint32_t f0 = 0; f0 < frames; f0 += maxF) {
            const uint32_t nf = (frames - f0 < maxF) ? frames - f0 : maxF;
            size_t off = 0; int r;
            if ((r = take_region(c, (size_t)((nf + 63u) / 64u) * windowBytes, c->stream, &off))) return r;
            if ((r = wait_scene(c, c->stream))) return r;
            void* slab = c->pool + off;
            if (c->havePrim) HIPCK(c, crt_launch_render_prim(&c->hScene, &c->prim, slab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, spp_first + f0 * passes, nf, passes, c->stream));
            else HIPCK(c, crt_launch_render_alt(c->renderAccel, &c->hScene, &c->alt, &c->blasAlt[c->renderAccel - 1], slab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, spp_first + f0 * passes, nf, passes, c->stream));
            HIPCK(c, crt_launch_accumulate(slab, c->dAcc, nullptr, c->tileCount, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, nf, passes, c->stream));
            crt_ctx::Region reg; reg.off = off; reg.bytes = (size_t)((nf + 63u) / 64u) * windowBytes;
            if (c->freeEvents.empty()) HIPCK(c, hipEventCreateWithFlags(&reg.freed, hipEventDisableTiming));
            else { reg.freed = c->freeEvents.back(); c->freeEvents.pop_back(); }
            HIPCK(c, hipEventRecord(reg.freed, c->stream));
            c->inflight.push_back(reg);
        }
        return CRT_OK;
    }
    for (uint32_t f0 = 0; f0 < frames; f0 += maxF) {
        const uint32_t nf = (frames - f0 < maxF) ? frames - f0 : maxF;
        const int r = launch_frames(c, spp_first + f0 * passes, nf, passes, c->streams[(size_t)(c->launchSeq++ % c->streams.size())], nullptr);
        if (r) return r > 0 ? c->fail(CRT_ERR_DEVICE, "slab ring blocked by a render-ahead region") : r;
    }
    return CRT_OK;
}

int crt_sync(crt_ctx* c)
{
    if (!c) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipStreamSynchronize(c->stream));          // every render launch is followed by its accumulate on this stream
    for (auto st : c->streams) HIPCK(c, hipStreamSynchronize(st));
    if (c->aheadStream) HIPCK(c, hipStreamSynchronize(c->aheadStream));
    return CRT_OK;
}

int crt_clear(crt_ctx* c)
{
    if (!c) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemsetAsync(c->dAcc, 0, (size_t)c->cfg.width * c->cfg.height * 16, c->stream));
    return CRT_OK;
}

int crt_read_accumulator(crt_ctx* c, float* host)
{
    if (!c || !host) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemcpyAsync(host, c->dAcc, (size_t)c->cfg.width * c->cfg.height * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

// the screen and the energy a resolve left on the device, to the host (waits for the main stream)
static int read_screen(crt_ctx* c, uint32_t* hostPixels, float* energy)
{
    const int tiles = c->tilesX * c->tilesY;
    if (hostPixels) HIPCK(c, hipMemcpyAsync(hostPixels, c->dPixels, (size_t)c->cfg.width * c->cfg.height * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> sums(tiles);
    HIPCK(c, hipMemcpyAsync(sums.data(), c->dTileSums, (size_t)tiles * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (energy) { float e = 0; for (int i = 0; i < tiles; i++) e += sums[i]; *energy = e; }   // renderer.cpp:155-157, tile order
    return CRT_OK;
}

int crt_resolve_screen(crt_ctx* c, float scale, uint32_t* hostPixels, float* energy)
{
    if (!c) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, crt_launch_resolve(c->dAcc, c->dPixels, c->dTileSums, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, scale, c->stream));
    return read_screen(c, hostPixels, energy);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// crt_tick: one Renderer::Tick.  A frame's samples depend on its tile, spp, passes, camera, scene, depthLimit and render accelerator — never on the
// accumulator — so while none of those change, the frames after a Tick can be rendered AHEAD as ordinary render launches (no accumulate; their slab
// regions stay held) and a later Tick only commits its frame's samples (commit_frame_kernel: accumulate + resolve in one pass) and reads back.
// The queue is valid for one state epoch (crt_set_camera with new values, crt_update_scene, crt_upload_*, crt_set_render_accel bump it) and the next
// (spp, passes); any other request discards it and renders its frame as crt_render(spp, 1, passes).  Speculation starts once a Tick follows a Tick of the
// same epoch with spp = previous + passes, so a camera that moves every Tick renders exactly as before: one launch per Tick, no slab held.
// Depth: the first launch renders one 64-frame window, each later one twice as many frames as the one before, up to kAheadMaxFrames;
// at most two launches are queued, on a low-priority stream so that a miss's own launch is dispatched first.
// ---------------------------------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t kAheadMaxFrames = 256;

// queues a render-ahead launch whose first frame has spp `sppFirst`
static int launch_ahead(crt_ctx* c, uint32_t sppFirst, uint32_t passes)
{
    if (!c->aheadStream) {
        int least = 0, greatest = 0;
        HIPCK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCK(c, hipStreamCreateWithPriority(&c->aheadStream, hipStreamNonBlocking, least));
    }
    uint32_t nf = c->aheadFrames ? std::min(2u * c->aheadFrames, kAheadMaxFrames) : 64u;
    if (nf > (uint32_t)c->cfg.maxFramesPerLaunch) nf = (uint32_t)c->cfg.maxFramesPerLaunch;
    const uint32_t poolW = (uint32_t)(c->poolBytes / window_bytes(c, passes));      // the pool as the miss's crt_render sized it: two launches must fit
    if (nf > poolW / 2u * 64u) nf = poolW / 2u * 64u;
    if (nf == 0 || c->streams.empty()) return 0;
    hipStream_t st = hook("CRT_AHEAD_NORMAL_PRIORITY") ? c->streams[(size_t)(c->launchSeq++ % c->streams.size())] : c->aheadStream;   // A/B of the stream priority
    crt_ctx::Ahead a{};
    const int r = launch_frames(c, sppFirst, nf, passes, st, &a);
    if (r < 0) return r;
    if (r > 0) return 0;                                            // no room in the ring short of a held region: a later hit tries again
    c->ahead.push_back(a); c->aheadFrames = nf;
    return 0;
}

int crt_tick(crt_ctx* c, uint32_t spp, uint32_t passes, uint32_t* hostPixels, float* hostRgba, float* energy)
{
    if (!c) return CRT_ERR_INVALID;
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "crt_tick before crt_upload_scene");
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "passes must be 1..4 (the reference's UI range, renderer.cpp:178)");
    HIPCK(c, hipSetDevice(c->cfg.device));
    const float scale = 1.0f / (float)(spp + passes);                                          // renderer.cpp:119
    // statistics contexts (per-tile clocks of ONE launch), the KD-tree / grid path and the PrimitiveScene are served by the plain path only
    const bool eligible = !c->cfg.collectStats && c->renderAccel == 0 && !c->havePrim && c->tileCount > 0;
    const bool streak = eligible && c->tickEpoch == c->epoch && spp == c->tickNextSpp && passes == c->tickPasses;
    c->tickEpoch = c->epoch; c->tickNextSpp = spp + passes; c->tickPasses = passes;
    const bool hit = !c->ahead.empty() && c->ahead.front().epoch == c->epoch && c->ahead.front().passes == passes &&
                     spp == c->ahead.front().sppFirst + c->ahead.front().used * passes;
    int r;
    if (hit) {
        crt_ctx::Ahead& a = c->ahead.front();
        const uint32_t f = a.used++;
        HIPCK(c, hipStreamWaitEvent(c->stream, a.end, 0));
        HIPCK(c, crt_launch_commit_frame(a.slab + (size_t)(f / 64u) * sample_bytes_per_window(c, passes), f % 64u, passes, c->dAcc, c->dPixels, c->dTileSums,
                                         c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, scale, c->stream));
        if (a.used == a.nf) {                                                                  // the launch's last frame: its region is free behind this commit
            const crt_ctx::Ahead done = a; c->ahead.pop_front();
            c->doneEvents.push_back(done.end);
            if ((r = release_ahead_region(c, done))) return r;
        }
        if (c->ahead.size() < 2u) {                                                            // top up while the read-back runs
            const uint32_t next = c->ahead.empty() ? spp + passes : c->ahead.back().sppFirst + c->ahead.back().nf * passes;
            if ((r = launch_ahead(c, next, passes))) return r;
        }
    } else {
        if ((r = crt_render(c, spp, 1, passes))) return r;                                     // (discards the queue)
        HIPCK(c, crt_launch_resolve(c->dAcc, c->dPixels, c->dTileSums, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, scale, c->stream));
    }
    if (hostRgba) HIPCK(c, hipMemcpyAsync(hostRgba, c->dAcc, (size_t)c->cfg.width * c->cfg.height * 16, hipMemcpyDeviceToHost, c->stream));
    if ((r = read_screen(c, hostPixels, energy))) return r;
    // a second still Tick in a row: render ahead, after the read-back (the GPU is idle, so a single-window launch takes the latency mode)
    if (!hit && streak && (r = launch_ahead(c, spp + passes, passes))) return r;
    return CRT_OK;
}

int crt_whitted_tick(crt_ctx* c, uint32_t* hostPixels)
{
    if (!c) return CRT_ERR_INVALID;
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_whitted_tick before crt_upload_scene");
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, crt_launch_whitted(&c->hScene, c->renderAccel, &c->alt, c->renderAccel ? &c->blasAlt[c->renderAccel - 1] : nullptr, c->dAcc, c->dPixels, c->dCounters, c->ldsBytes, c->stream));
    if (hostPixels) HIPCK(c, hipMemcpyAsync(hostPixels, c->dPixels, (size_t)c->cfg.width * c->cfg.height * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_whitted_tick_inspect(crt_ctx* c, int inspect, int32_t peakTraversalIn, int32_t peakTestsIn, uint32_t* hostPixels, int32_t* hostTraversed, int32_t* hostTested, crt_whitted_metrics* metrics)
{
    if (!c) return CRT_ERR_INVALID;
    if (inspect < CRT_INSPECT_NONE || inspect > CRT_INSPECT_TESTS) return c->fail(CRT_ERR_INVALID, "crt_whitted_tick_inspect: inspect must be CRT_INSPECT_NONE, _TRAVERSAL or _TESTS");
    if (peakTraversalIn < 0 || peakTestsIn < 0) return c->fail(CRT_ERR_INVALID, "crt_whitted_tick_inspect: a peak cannot be negative");
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_whitted_tick_inspect before crt_upload_scene");
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (n > c->inspectCap) {                                               // first use (the image size is the context's): kept until crt_destroy
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (c->dInspectCounts) (void)hipFree(c->dInspectCounts);
        if (c->dInspectWork) (void)hipFree(c->dInspectWork);
        c->dInspectCounts = nullptr; c->dInspectWork = nullptr; c->inspectCap = 0;
        HIPCK(c, hipMalloc((void**)&c->dInspectCounts, n * 2 * sizeof(int32_t)));
        HIPCK(c, hipMalloc(&c->dInspectWork, crt_whitted_inspect_work_bytes((uint32_t)n)));
        c->inspectCap = n;
    }
    int32_t* dTrav = c->dInspectCounts; int32_t* dTested = c->dInspectCounts + n;
    HIPCK(c, crt_launch_whitted_inspect(&c->hScene, c->renderAccel, &c->alt, c->renderAccel ? &c->blasAlt[c->renderAccel - 1] : nullptr, inspect,
                                        inspect == CRT_INSPECT_TESTS ? peakTestsIn : peakTraversalIn, c->dAcc, c->dPixels, c->dCounters, dTrav, dTested, c->dInspectWork, c->ldsBytes, c->stream));
    static_assert(sizeof(crt_whitted_metrics) == 32, "crt::InspectSums (kernels.hip) is read back into this record");
    crt_whitted_metrics m;                                                 // the device record has this layout, with this Tick's maxima in the peaks
    if (hostPixels) HIPCK(c, hipMemcpyAsync(hostPixels, c->dPixels, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (hostTraversed) HIPCK(c, hipMemcpyAsync(hostTraversed, dTrav, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (hostTested) HIPCK(c, hipMemcpyAsync(hostTested, dTested, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (metrics) HIPCK(c, hipMemcpyAsync(&m, c->dInspectWork, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (metrics) {
        if (m.peakTraversal < peakTraversalIn) m.peakTraversal = peakTraversalIn;
        if (m.peakTests < peakTestsIn) m.peakTests = peakTestsIn;
        *metrics = m;
    }
    return CRT_OK;
}

// ---- the host-buffer query entries: records in, one launch on the main stream, records out, synchronise.  Their device staging is ONE allocation, grown to the high-water
// mark (hipMalloc synchronises the device; 16-byte aligned and more); every entry returns only after hipStreamSynchronize, so each lays its sub-buffers out from offset 0 ----
static int stage(crt_ctx* c, size_t bytes)
{
    if (bytes <= c->stageCap) return 0;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (c->dStage) (void)hipFree(c->dStage);
    c->dStage = nullptr; c->stageCap = 0;
    HIPCK(c, hipMalloc((void**)&c->dStage, bytes));
    c->stageCap = bytes;
    return 0;
}

// FindNearest (crt_hit records) / IsOccluded (occl: int32 flags) for n rays in device memory: THE choice of launcher, for host and device entries, after their checks.  accel 0 = the
// scene's own structure (BVH / TLAS, or the PrimitiveScene's eleven primitives), else the uploaded KD-tree / grid: FileScene's structure, or a two-level scene's BLAS set.
static hipError_t launch_query(crt_ctx* c, bool occl, int accel, const void* rays, void* out, uint32_t n, uint32_t* cursor, hipStream_t st)
{
    if (accel != 0) {
        if (c->hScene.kind == CRT_SCENE_TLAS) return crt_launch_tlas_alt_query(accel, occl, &c->hScene, &c->blasAlt[accel - 1], rays, out, n, cursor, st);
        if (occl) return crt_launch_is_occluded_alt(accel, &c->hScene, &c->alt, rays, static_cast<int32_t*>(out), n, cursor, st);
        return crt_launch_find_nearest_alt(accel, &c->hScene, &c->alt, rays, out, n, cursor, st);
    }
    if (occl) return crt_launch_is_occluded(&c->hScene, rays, static_cast<int32_t*>(out), n, c->ldsBytes, cursor, st);
    if (c->havePrim) return crt_launch_find_nearest_prim(&c->prim, rays, out, n, st);
    return crt_launch_find_nearest(&c->hScene, rays, out, n, c->dCounters, c->ldsBytes, cursor, st);
}

// crt_find_nearest / crt_find_nearest_alt / crt_is_occluded after their own checks (n >= 1): a ray and a shadow ray are 28 bytes alike
static int query_host(crt_ctx* c, bool occl, int accel, const void* rays, void* out, size_t n)
{
    const size_t outSize = occl ? sizeof(int32_t) : sizeof(crt_hit);
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (const int r = stage(c, n * (sizeof(crt_ray) + outSize))) return r;
    char* dRays = c->dStage; char* dOut = dRays + n * sizeof(crt_ray);
    HIPCK(c, hipMemcpyAsync(dRays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, launch_query(c, occl, accel, dRays, dOut, (uint32_t)n, c->dQueryCursor, c->stream));
    HIPCK(c, hipMemcpyAsync(out, dOut, n * outSize, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_find_nearest(crt_ctx* c, const crt_ray* rays, crt_hit* hits, size_t n)
{
    if (!c || (n && (!rays || !hits))) return CRT_ERR_INVALID;
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "crt_find_nearest before crt_upload_scene");
    if (n == 0) return CRT_OK;
    if (n > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "at most 2^31-1 rays per call");
    return query_host(c, false, 0, rays, hits, n);
}

// the alternative accelerators' triangle record.  triIdx = what a hit reports: the triangle's index (crt_upload_alt_accel) / its global shade index, shadeBase + BLAS-local index (_blas_accel)
static crt::AltTri alt_tri(const crt_tri& t, uint32_t triIdx)
{
    crt::AltTri o{};                                                       // pad = 0
    for (int k = 0; k < 3; k++) { o.v0[k] = t.vertex0[k]; o.e1[k] = t.vertex1[k] - t.vertex0[k]; o.e2[k] = t.vertex2[k] - t.vertex0[k]; }
    o.triIdx = triIdx; o.objIdx = t.objIdx;
    return o;
}

// LDS of the single-wavefront kernels (the find-nearest / is-occluded queries, Whitted): `words` dwords of traversal stack per lane must fit one workgroup's 64 KiB
static bool wave_stack_fits(uint64_t words) { return words * 64u * 4u <= 64u * 1024u; }

// the checks of one KD-tree / grid description (crt_upload_alt_accel, and every BLAS's of crt_upload_blas_accel); kdHeight: the KD-tree's height
static int check_alt_accel(crt_ctx* c, const crt_alt_accel* a, uint32_t* kdHeightOut)
{
    if (a->kind != CRT_ACCEL_KDTREE && a->kind != CRT_ACCEL_GRID) return c->fail(CRT_ERR_INVALID, "unknown accelerator kind %d", a->kind);
    if (!a->triangles || a->triCount == 0) return c->fail(CRT_ERR_INVALID, "accelerator has no triangles");
    uint32_t kdHeight = 0;
    if (a->kind == CRT_ACCEL_KDTREE) {
        if (!a->kdNodes || a->kdNodeCount == 0 || (a->kdTriIndexCount && !a->kdTriIndices)) return c->fail(CRT_ERR_INVALID, "KD-tree arrays missing");
        std::vector<std::pair<uint32_t, uint32_t>> st; st.push_back({0u, 0u}); size_t visited = 0;
        while (!st.empty()) {
            auto [n, d] = st.back(); st.pop_back();
            if (++visited > (size_t)a->kdNodeCount) return c->fail(CRT_ERR_INVALID, "KD node graph is not a tree");
            const crt_kd_node& nd = a->kdNodes[n];
            if (d > kdHeight) kdHeight = d;
            if (nd.left < 0) { if ((uint64_t)nd.firstTri + nd.triCount > a->kdTriIndexCount) return c->fail(CRT_ERR_INVALID, "KD leaf %u: triangle range out of bounds", n); continue; }
            if (nd.right < 0 || (uint32_t)nd.left >= a->kdNodeCount || (uint32_t)nd.right >= a->kdNodeCount || nd.splitAxis < 0 || nd.splitAxis > 2)
                return c->fail(CRT_ERR_INVALID, "KD node %u: child index / split axis out of range", n);
            st.push_back({(uint32_t)nd.left, d + 1}); st.push_back({(uint32_t)nd.right, d + 1});
        }
        for (uint32_t i = 0; i < a->kdTriIndexCount; i++) if (a->kdTriIndices[i] >= a->triCount) return c->fail(CRT_ERR_INVALID, "kdTriIndices[%u] out of range", i);
        if (!wave_stack_fits((uint64_t)(kdHeight + 1) * 2u)) return c->fail(CRT_ERR_UNSUPPORTED, "KD-tree height %u exceeds the LDS traversal stack", kdHeight);
    } else {
        uint64_t cells = 1;
        for (int k = 0; k < 3; k++) { if (a->gridResolution[k] < 1 || a->gridResolution[k] > 128) return c->fail(CRT_ERR_INVALID, "grid resolution must be 1..128 per axis (grid.cpp:22)"); cells *= (uint64_t)a->gridResolution[k]; }
        if (!a->gridCellStart || (a->gridCellTriCount && !a->gridCellTris)) return c->fail(CRT_ERR_INVALID, "grid arrays missing");
        if (a->gridCellStart[0] != 0 || a->gridCellStart[cells] != a->gridCellTriCount) return c->fail(CRT_ERR_INVALID, "gridCellStart must run from 0 to gridCellTriCount");
        for (uint64_t i = 0; i < cells; i++) if (a->gridCellStart[i] > a->gridCellStart[i + 1]) return c->fail(CRT_ERR_INVALID, "gridCellStart is not monotone at cell %llu", (unsigned long long)i);
        for (uint32_t i = 0; i < a->gridCellTriCount; i++) if (a->gridCellTris[i] < 0 || (uint32_t)a->gridCellTris[i] >= a->triCount) return c->fail(CRT_ERR_INVALID, "gridCellTris[%u] out of range", i);
    }
    *kdHeightOut = kdHeight;
    return 0;
}

// FileScene's KD-tree / uniform grid over the scene's triangles, for crt_find_nearest_alt
int crt_upload_alt_accel(crt_ctx* c, const crt_alt_accel* a)
{
    if (!c || !a) return CRT_ERR_INVALID;
    if (!c->haveScene || c->hScene.kind != CRT_SCENE_FILE) return c->fail(CRT_ERR_STATE, "crt_upload_alt_accel needs an uploaded CRT_SCENE_FILE scene (light quad, floor plane, materials)");
    uint32_t kdHeight = 0;
    { const int r = check_alt_accel(c, a, &kdHeight); if (r) return r; }
    c->epoch++;
    HIPCK(c, hipSetDevice(c->cfg.device));
    const int slot = a->kind == CRT_ACCEL_KDTREE ? 0 : 1;
    HIPCK(c, hipStreamSynchronize(c->stream));                            // queries of the previous structure
    { const int r = wait_queries(c); if (r) return r; }                  // ... also those on callers' streams
    std::vector<void*>& allocs = c->altAllocs[slot];
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    if (slot == 0) c->haveKd = false; else c->haveGrid = false;
    if (c->renderAccel == a->kind) c->renderAccel = 0;
    int r;
    // Möller–Trumbore operands in the reference's triangle order (one array shared by both structures)
    if (!c->altTris || c->altTriCount != a->triCount) {
        if (c->altTris) { (void)hipFree(c->altTris); c->altTris = nullptr; }
        HIPCK(c, hipMalloc((void**)&c->altTris, (size_t)a->triCount * sizeof(crt::AltTri))); c->altTriCount = a->triCount;
    }
    {
        std::vector<crt::AltTri> rec(a->triCount);
        for (uint32_t i = 0; i < a->triCount; i++) rec[i] = alt_tri(a->triangles[i], i);
        HIPCK(c, hipMemcpy(c->altTris, rec.data(), rec.size() * sizeof(crt::AltTri), hipMemcpyHostToDevice));
        c->alt.tris = c->altTris;
    }
    if (slot == 0) {
        if ((r = upload_array(c, allocs, a->kdNodes, (size_t)a->kdNodeCount * sizeof(crt::KdNode), &c->alt.kdNodes))) return r;
        if ((r = upload_array(c, allocs, a->kdTriIndices, (size_t)a->kdTriIndexCount * 4, &c->alt.kdRefs))) return r;
        c->alt.kdStack = kdHeight + 1; c->haveKd = true; c->kdNodeCount = a->kdNodeCount; c->kdRefCount = a->kdTriIndexCount;
    } else {
        uint64_t cells = (uint64_t)a->gridResolution[0] * a->gridResolution[1] * a->gridResolution[2];
        if ((r = upload_array(c, allocs, a->gridCellStart, (size_t)(cells + 1) * 4, &c->alt.cellStart))) return r;
        if ((r = upload_array(c, allocs, a->gridCellTris, (size_t)a->gridCellTriCount * 4, &c->alt.cellRefs))) return r;
        for (int k = 0; k < 3; k++) { c->alt.res[k] = a->gridResolution[k]; c->alt.cell[k] = a->gridCellSize[k]; c->alt.lo[k] = a->gridMin[k]; c->alt.hi[k] = a->gridMax[k]; }
        c->haveGrid = true; c->gridRefCount = a->gridCellTriCount;
    }
    HIPCK(c, ensure_event(&c->altReady));
    HIPCK(c, hipEventRecord(c->altReady, nullptr));                       // behind the copies above (null stream): device queries on other streams wait for it
    return CRT_OK;
}

// TLASFileScene built with TLAS_USE_KDTree / TLAS_USE_Grid: one BLASKDTree / BLASGrid per BLAS of the uploaded two-level scene, for the queries and the render path
int crt_upload_blas_accel(crt_ctx* c, int kind, const crt_alt_accel* blas, uint32_t blasCount)
{
    if (!c) return CRT_ERR_INVALID;
    if (!c->haveScene || c->hScene.kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_STATE, "crt_upload_blas_accel needs an uploaded CRT_SCENE_TLAS scene");
    if (kind != CRT_ACCEL_KDTREE && kind != CRT_ACCEL_GRID) return c->fail(CRT_ERR_INVALID, "unknown accelerator kind %d", kind);
    const crt_ctx::Flat& f = c->flat;
    if (!blas || blasCount != (uint32_t)f.triCount.size()) return c->fail(CRT_ERR_INVALID, "crt_upload_blas_accel: %u structures for a scene of %zu BLAS", blasCount, f.triCount.size());
    // ---- every check first: a refused upload leaves the previous set answering ----
    const crt::Instance* inst = reinterpret_cast<const crt::Instance*>(f.geom.data() + f.instOff);
    uint32_t maxKd = 0; uint64_t nNodes = 0, nRefs = 0, nTris = 0, nCells = 0, nCellRefs = 0; std::vector<uint32_t> kdHeights(blasCount, 0u);
    for (uint32_t b = 0; b < blasCount; b++) {
        const crt_alt_accel& a = blas[b];
        if (a.kind != kind) return c->fail(CRT_ERR_INVALID, "BLAS %u: structure of kind %d in a set of kind %d", b, a.kind, kind);
        uint32_t h = 0;
        { const int r = check_alt_accel(c, &a, &h); if (r) return r; }
        kdHeights[b] = h;
        if (a.triCount != f.triCount[b]) return c->fail(CRT_ERR_INVALID, "BLAS %u: %u triangles, the uploaded BLAS has %u", b, a.triCount, f.triCount[b]);
        for (uint32_t t = 0; t < a.triCount; t++)
            if (a.triangles[t].objIdx != inst[b].objIdx) return c->fail(CRT_ERR_INVALID, "BLAS %u: triangle %u has objIdx %d, the BLAS %d", b, t, a.triangles[t].objIdx, inst[b].objIdx);
        // SetTransform takes the world bounds from this box (blas_kdtree.cpp:407-418, blas_grid.cpp:267-278): the shared TLAS is the variant's only if it is the BVH's
        float box[6];
        if (kind == CRT_ACCEL_KDTREE) { memcpy(box, a.kdNodes[0].aabbMin, 12); memcpy(box + 3, a.kdNodes[0].aabbMax, 12); }
        else { memcpy(box, a.gridMin, 12); memcpy(box + 3, a.gridMax, 12); }
        if (memcmp(box, &f.rootBox[6 * b], 24) != 0) return c->fail(CRT_ERR_INVALID, "BLAS %u: root box differs from the BLAS's BVH root box (the TLAS is shared)", b);
        if (kind == CRT_ACCEL_KDTREE) { if (h + 1 > maxKd) maxKd = h + 1; nNodes += a.kdNodeCount; nRefs += a.kdTriIndexCount; }
        else { nCells += (uint64_t)a.gridResolution[0] * a.gridResolution[1] * a.gridResolution[2] + 1; nCellRefs += a.gridCellTriCount; }
        nTris += a.triCount;
    }
    const uint32_t words = maxKd * 2u + (c->hScene.stackDepth - c->hScene.bvhStack);      // KD stack + TLAS entries + the return marker, per lane
    if (!wave_stack_fits(words)) return c->fail(CRT_ERR_UNSUPPORTED, "TLAS + KD-tree traversal stack of %u dwords per lane exceeds the LDS budget", words);
    if (nNodes > 0xffffffffull || nRefs > 0xffffffffull || nTris > 0xffffffffull || nCells > 0xffffffffull || nCellRefs > 0xffffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "BLAS set too large");
    // ---- flatten: concatenated arrays + one descriptor per BLAS ----
    std::vector<crt::BlasAltDesc> desc(blasCount);
    std::vector<crt_kd_node> nodes; std::vector<uint32_t> refs, cellStart; std::vector<int32_t> cellRefs; std::vector<crt::AltTri> tris((size_t)nTris);
    uint32_t tb = 0;
    for (uint32_t b = 0; b < blasCount; b++) {
        const crt_alt_accel& a = blas[b];
        crt::BlasAltDesc& d = desc[b]; memset(&d, 0, sizeof(d));
        d.nodeBase = (uint32_t)nodes.size(); d.refBase = (uint32_t)refs.size(); d.triBase = tb; d.cellBase = (uint32_t)cellStart.size(); d.cellRefBase = (uint32_t)cellRefs.size();
        d.objIdx = inst[b].objIdx;
        if (kind == CRT_ACCEL_KDTREE) { nodes.insert(nodes.end(), a.kdNodes, a.kdNodes + a.kdNodeCount); refs.insert(refs.end(), a.kdTriIndices, a.kdTriIndices + a.kdTriIndexCount); }
        else {
            const uint64_t cells = (uint64_t)a.gridResolution[0] * a.gridResolution[1] * a.gridResolution[2];
            cellStart.insert(cellStart.end(), a.gridCellStart, a.gridCellStart + cells + 1); cellRefs.insert(cellRefs.end(), a.gridCellTris, a.gridCellTris + a.gridCellTriCount);
            for (int k = 0; k < 3; k++) { d.res[k] = a.gridResolution[k]; d.cell[k] = a.gridCellSize[k]; d.lo[k] = a.gridMin[k]; d.hi[k] = a.gridMax[k]; }
        }
        for (uint32_t i = 0; i < a.triCount; i++) tris[(size_t)tb + i] = alt_tri(a.triangles[i], inst[b].shadeBase + i);
        tb += a.triCount;
    }
    // ---- replace the set of this kind (synchronous): queries and render launches that read the previous one finish first ----
    HIPCK(c, hipSetDevice(c->cfg.device));
    { const int r = drain_all(c); if (r) return r; }
    // the new set goes into buffers of its own; only once every copy has succeeded does it replace the previous one (a failed allocation or copy keeps that)
    std::vector<void*> allocs;
    crt::TlasAltDev tl{};
    int r;
    if ((r = upload_array(c, allocs, desc.data(), desc.size() * sizeof(crt::BlasAltDesc), &tl.desc)) || (r = upload_array(c, allocs, tris.data(), tris.size() * sizeof(crt::AltTri), &tl.tris)) ||
        (r = upload_array(c, allocs, nodes.data(), nodes.size() * sizeof(crt_kd_node), &tl.kdNodes)) || (r = upload_array(c, allocs, refs.data(), refs.size() * 4, &tl.kdRefs)) ||
        (r = upload_array(c, allocs, cellStart.data(), cellStart.size() * 4, &tl.cellStart)) || (r = upload_array(c, allocs, cellRefs.data(), cellRefs.size() * 4, &tl.cellRefs))) {
        for (void* p : allocs) (void)hipFree(p);
        return r;
    }
    tl.kdStack = maxKd;
    const int slot = kind - 1;
    c->epoch++;
    for (void* p : c->blasAllocs[slot]) (void)hipFree(p);
    c->blasAllocs[slot].swap(allocs); c->blasAlt[slot] = tl; c->haveBlas[slot] = true;
    crt_ctx::BlasSet& S = c->blasSet[slot];                               // what the kind's device build and crt_get_kdtree / crt_get_grid need of the set
    S.desc = desc; S.count[0].resize(blasCount); S.count[1].resize(blasCount); S.height = kdHeights; S.current.assign(blasCount, (uint8_t)1); S.held = true;
    for (uint32_t b = 0; b < blasCount; b++) {
        const crt_alt_accel& a = blas[b];
        S.count[0][b] = slot ? (uint32_t)a.gridResolution[0] * (uint32_t)a.gridResolution[1] * (uint32_t)a.gridResolution[2] + 1u : a.kdNodeCount;
        S.count[1][b] = slot ? a.gridCellTriCount : a.kdTriIndexCount;
    }
    if (c->renderAccel == kind) c->renderAccel = 0;                       // as crt_upload_alt_accel: the render goes back to the BVH until crt_set_render_accel
    HIPCK(c, ensure_event(&c->altReady));
    HIPCK(c, hipEventRecord(c->altReady, nullptr));                       // behind the copies above: device queries on other streams wait for it
    return CRT_OK;
}

int crt_upload_primitive_scene(crt_ctx* c, const crt_primitive_scene* ps)
{
    if (!c || !ps) return CRT_ERR_INVALID;
    c->epoch++;
    HIPCK(c, hipSetDevice(c->cfg.device));
    for (const crt_texture* t : {&ps->red, &ps->blue})
        if (t->pixels && (t->width != 512 || t->height != 512)) return c->fail(CRT_ERR_INVALID, "PrimitiveScene wall images are 512 x 512 (Plane::GetAlbedo masks the texel coordinates with 511)");
    { const int r = drain_all(c); if (r) return r; }
    c->freeScene();
    crt::PrimDev& p = c->prim; p = crt::PrimDev{};
    memcpy(p.quadInvT, ps->quadInvT, 48); p.quadNrm[0] = -ps->quadT[1]; p.quadNrm[1] = -ps->quadT[5]; p.quadNrm[2] = -ps->quadT[9]; p.quadSize = ps->quadSize;   // Quad::GetNormal, primitives.h:363-367
    memcpy(p.spherePos, ps->spherePos, 12);
    memcpy(p.cubeInvM, ps->cubeInvM, 48); memcpy(p.cubeM, ps->cubeM, 48); memcpy(p.cubeMin, ps->cubeMin, 12); memcpy(p.cubeMax, ps->cubeMax, 12);
    memcpy(p.torusInvT, ps->torusInvT, 48); memcpy(p.torusT, ps->torusT, 48); p.rt2 = ps->torusRt2; p.rc2 = ps->torusRc2; p.r2 = ps->torusR2;
    memcpy(p.refl, ps->reflectivity, 44); memcpy(p.refr, ps->refractivity, 44); memcpy(p.absorb, ps->absorption, 132);
    HIPCK(c, hipMalloc((void**)&c->dPrimTex, 2u * 512u * 512u * 4u));
    HIPCK(c, hipMemsetAsync(c->dPrimTex, 0, 2u * 512u * 512u * 4u, c->stream));
    if (ps->red.pixels) HIPCK(c, hipMemcpyAsync(c->dPrimTex, ps->red.pixels, 512u * 512u * 4u, hipMemcpyHostToDevice, c->stream));
    if (ps->blue.pixels) HIPCK(c, hipMemcpyAsync(c->dPrimTex + 512u * 512u, ps->blue.pixels, 512u * 512u * 4u, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    p.red = c->dPrimTex; p.blue = c->dPrimTex + 512u * 512u;
    c->havePrim = true; c->orderDirty = false;
    return CRT_OK;
}

// the sequential Sample kernels' LDS columns (render_seq_kernel, sample_query_kernel: device/seq_sample.h seq_lds_bytes).  Dwords of traversal stack per lane when Sample traces
// through `accel`: 0 = the scene's BVH / TLAS (none for the PrimitiveScene), else the uploaded KD-tree / grid
static uint32_t sample_stack_words(const crt_ctx* c, int accel)
{
    if (c->havePrim) return 0u;
    if (accel == 0) return c->hScene.stackDepth;
    if (c->hScene.kind == CRT_SCENE_TLAS) return c->blasAlt[accel - 1].kdStack * 2u + (c->hScene.stackDepth - c->hScene.bvhStack);
    return accel == CRT_ACCEL_KDTREE ? c->alt.kdStack * 2u : 0u;
}
// the stack + 15 throughput factors per lane, four wavefronts per workgroup, within a workgroup's 64 KiB
static bool sample_lds_fits(uint32_t words) { return ((uint64_t)words + 15u) * 64u * 4u * 4u <= 64u * 1024u; }

int crt_set_render_accel(crt_ctx* c, int kind)
{
    if (!c) return CRT_ERR_INVALID;
    if (kind != 0 && kind != CRT_ACCEL_KDTREE && kind != CRT_ACCEL_GRID) return c->fail(CRT_ERR_INVALID, "crt_set_render_accel: unknown accelerator kind %d", kind);
    if (kind != 0 && !c->hasAlt(kind)) return c->fail(CRT_ERR_STATE, "crt_set_render_accel: no such accelerator uploaded (kind %d)", kind);
    if (kind != 0 && c->hScene.kind == CRT_SCENE_TLAS) {
        const uint32_t words = sample_stack_words(c, kind);
        if (!sample_lds_fits(words)) return c->fail(CRT_ERR_UNSUPPORTED, "TLAS + KD-tree stack of %u dwords exceeds the render kernel's LDS stack", words);
    } else if (kind != 0 && !sample_lds_fits(sample_stack_words(c, CRT_ACCEL_KDTREE)))        // a FileScene's grid is held to its KD-tree's stack too, as it always was
        return c->fail(CRT_ERR_UNSUPPORTED, "KD-tree height %u exceeds the render kernel's LDS stack", c->alt.kdStack);
    c->renderAccel = kind; c->epoch++;
    return CRT_OK;
}

int crt_find_nearest_alt(crt_ctx* c, int kind, const crt_ray* rays, crt_hit* hits, size_t n)
{
    if (!c || (n && (!rays || !hits))) return CRT_ERR_INVALID;
    if (!c->hasAlt(kind)) return c->fail(CRT_ERR_STATE, "crt_find_nearest_alt: no such accelerator uploaded (kind %d)", kind);
    if (n == 0) return CRT_OK;
    if (n > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "at most 2^31-1 rays per call");
    return query_host(c, false, kind, rays, hits, n);
}

// ---- scene queries: IsOccluded on host buffers, FindNearest / IsOccluded on device buffers (crt_abi.h "scene queries") ----
// what every query entry checks, before n == 0 returns (as crt_find_nearest / crt_find_nearest_alt): a known accelerator, a scene that has it, at most 2^31-1 rays
static int query_check(crt_ctx* c, int accel, bool occl, size_t n, const char* what)
{
    if (accel != 0 && accel != CRT_ACCEL_KDTREE && accel != CRT_ACCEL_GRID) return c->fail(CRT_ERR_INVALID, "%s: unknown accelerator kind %d", what, accel);
    if (accel == 0) {
        if (occl && c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: IsOccluded over the PrimitiveScene is not supported (crt_whitted_tick refuses it too)", what);
        if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    } else if (!c->hasAlt(accel)) {
        return c->fail(CRT_ERR_STATE, "%s: no such accelerator uploaded (kind %d)", what, accel);
    }
    if (n > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 rays per call", what);
    return 0;
}

// a caller's buffer of `bytes` bytes must be device (or managed) memory of cfg.device, first and last byte alike, and 4-byte aligned
static int check_device_buffer(crt_ctx* c, const void* p, size_t bytes, const char* what)
{
    if (!p) return c->fail(CRT_ERR_INVALID, "%s: NULL buffer", what);
    if (reinterpret_cast<uintptr_t>(p) & 3u) return c->fail(CRT_ERR_INVALID, "%s: buffer %p is not 4-byte aligned", what, p);
    const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + bytes - 1};
    for (const char* q : ends) {
        hipPointerAttribute_t a{};
        const hipError_t e = hipPointerGetAttributes(&a, q);
        if (e != hipSuccess) { (void)hipGetLastError(); return c->fail(CRT_ERR_INVALID, "%s: %p is not device memory (%s)", what, (const void*)q, hipGetErrorString(e)); }
        if (!(a.type == hipMemoryTypeDevice || a.isManaged)) return c->fail(CRT_ERR_INVALID, "%s: %p is not device memory (a host pointer: use the host entry)", what, (const void*)q);
        if (a.device != c->cfg.device) return c->fail(CRT_ERR_INVALID, "%s: %p lives on device %d, the context on device %d", what, (const void*)q, a.device, c->cfg.device);
    }
    return 0;
}

// the stream a device entry was given: a hipStream_t of the context's device (checked), NULL = the ctx's own
static int caller_stream(crt_ctx* c, void* stream, const char* what, hipStream_t* stOut)
{
    *stOut = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (stream) {
        hipDevice_t dev = -1;
        HIPCK(c, hipStreamGetDevice(*stOut, &dev));
        if (dev != c->cfg.device) return c->fail(CRT_ERR_INVALID, "%s: the stream belongs to device %d, the context to device %d", what, dev, c->cfg.device);
    }
    return 0;
}

// what every entry on device buffers starts with, once its arguments are known to fit the scene: the context's device, every buffer checked, the stream
static int device_entry(crt_ctx* c, const char* what, std::initializer_list<std::pair<const void*, size_t>> bufs, void* stream, hipStream_t* stOut)
{
    HIPCK(c, hipSetDevice(c->cfg.device));
    for (const auto& b : bufs) { const int r = check_device_buffer(c, b.first, b.second, what); if (r) return r; }
    return caller_stream(c, stream, what, stOut);
}

// `bytes` of device memory to the host behind everything on `st`, and the host waits for them (`ev` is recorded behind the copy; *waitMs: the wall time of the wait)
static int read_back(crt_ctx* c, hipStream_t st, hipEvent_t ev, void* dst, const void* src, size_t bytes, double* waitMs = nullptr)
{
    HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCK(c, hipEventRecord(ev, st));
    const auto t0 = std::chrono::steady_clock::now();
    HIPCK(c, hipEventSynchronize(ev));
    if (waitMs) *waitMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// what crt_refit_device and crt_build_grid_device ask of their arguments: a triangle scene, `bvh` one of its BVHs, of `triCount` triangles (tail: the entry's own words)
static int check_bvh_arg(crt_ctx* c, const char* me, const char* primLacks, uint32_t bvh, uint32_t triCount, const char* tail)
{
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no %s", me, primLacks);
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", me);
    const std::vector<uint32_t>& tc = c->flat.triCount;
    if (bvh >= tc.size()) return c->fail(CRT_ERR_INVALID, "%s: BVH %u of a scene with %zu", me, bvh, tc.size());
    if (triCount != tc[bvh]) return c->fail(CRT_ERR_INVALID, "%s: %u triangles, the uploaded BVH %u has %u%s", me, triCount, bvh, tc[bvh], tail);
    return 0;
}

// a cursor slot whose previous launch has completed (all 64 in flight: the host waits for the next one in ring order)
static int take_query_slot(crt_ctx* c, int* out)
{
    for (int i = 0; i < crt_ctx::kQuerySlots; i++) {
        const int k = (c->qslotNext + i) % crt_ctx::kQuerySlots;
        crt_ctx::QuerySlot& q = c->qslot[k];
        if (q.pending) {
            const hipError_t e = hipEventQuery(q.done);
            if (e == hipErrorNotReady) continue;
            if (e != hipSuccess) return c->hip(e, "hipEventQuery(query)");
            q.pending = false;
        }
        HIPCK(c, ensure_event(&q.done));
        c->qslotNext = (k + 1) % crt_ctx::kQuerySlots; *out = k;
        return 0;
    }
    const int k = c->qslotNext;
    HIPCK(c, hipEventSynchronize(c->qslot[k].done)); c->qslot[k].pending = false;
    c->qslotNext = (k + 1) % crt_ctx::kQuerySlots; *out = k;
    return 0;
}

// what every device query shares behind its stream: wait_scene (a reader of the scene-write protocol), a slot of the ring (take_query_slot), and the slot's event
// ... recorded behind the launch (order_behind_queries / wait_queries look at it; so does the slot's next use)
static int end_device_query(crt_ctx* c, int k, hipStream_t st)
{
    HIPCK(c, hipEventRecord(c->qslot[k].done, st));
    c->qslot[k].pending = true;
    return CRT_OK;
}

static int query_device(crt_ctx* c, bool occl, int accel, const void* dRays, void* dOut, size_t n, void* stream, const char* what)
{
    int r;
    if ((r = query_check(c, accel, occl, n, what))) return r;
    if (n == 0) return CRT_OK;
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{dRays, n * 28}, {dOut, n * (occl ? 4u : 28u)}}, stream, &st)) || (r = wait_scene(c, st)) || (r = take_query_slot(c, &k))) return r;
    if (accel != 0 && c->altReady) HIPCK(c, hipStreamWaitEvent(st, c->altReady, 0));     // the accelerators' copies ran on the null stream
    HIPCK(c, launch_query(c, occl, accel, dRays, dOut, (uint32_t)n, c->dQuerySlots + 16 * k, st));
    return end_device_query(c, k, st);
}

int crt_find_nearest_device(crt_ctx* c, int accel, const crt_ray* d_rays, crt_hit* d_hits, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    return query_device(c, false, accel, d_rays, d_hits, n, stream, "crt_find_nearest_device");
}

int crt_is_occluded_device(crt_ctx* c, int accel, const crt_shadow_ray* d_rays, int32_t* d_occluded, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    return query_device(c, true, accel, d_rays, d_occluded, n, stream, "crt_is_occluded_device");
}

// ---- crt_refit_device: BVH::Refit / BLASBVH::Refit of one BVH on the device, from positions in device memory (device/refit.hip) ----
// the bottom-up plan of BVH `b`, from the mirror's references (which no update ever changes): every node pair with what its two children are, sorted deepest first
static int build_refit_plan(crt_ctx* c, uint32_t b)
{
    const crt_ctx::Flat& f = c->flat;
    const uint32_t np = f.nodesUsed[b] / 2, nt = f.triCount[b];
    const crt::NodePair* pairs = reinterpret_cast<const crt::NodePair*>(f.geom.data()) + f.pairBase[b];
    const uint32_t rootRef = (f.kind == CRT_SCENE_TLAS) ? reinterpret_cast<const crt::Instance*>(f.geom.data() + f.instOff)[b].rootRef : c->hScene.rootRef;
    bool bad = false;
    auto code_of = [&](uint32_t ref) -> uint32_t {
        const uint64_t off = (uint64_t)(ref & crt::kRefOffsetMask) << 4;
        if (ref & crt::kRefInterior) { const uint64_t i = off / 64u - f.pairBase[b]; if (i >= np) bad = true; return crt::kPlanInterior | (uint32_t)i; }
        const uint64_t j = (off - f.leafOff) / 48u - f.triBase[b]; if (j >= nt) bad = true;
        return (uint32_t)j;
    };
    crt_ctx::RefitPlan P;
    P.rootCode = code_of(rootRef);
    std::vector<uint32_t> depth(np, 0u), count;
    std::vector<std::pair<uint32_t, uint32_t>> st; size_t visited = 0;
    if (P.rootCode & crt::kPlanInterior) st.push_back({P.rootCode & ~crt::kPlanInterior, 0u});
    while (!st.empty() && !bad) {
        auto [p, d] = st.back(); st.pop_back();
        if (++visited > np) { bad = true; break; }
        depth[p] = d; if (count.size() <= d) count.resize(d + 1, 0u);
        count[d]++;
        for (int k = 0; k < 2; k++) { const uint32_t cc = code_of(pairs[p].c[k].ref); if (!bad && (cc & crt::kPlanInterior)) st.push_back({cc & ~crt::kPlanInterior, d + 1}); }
    }
    if (bad || visited != np) return c->fail(CRT_ERR_INVALID, "crt_refit_device: the references of BVH %u do not form its tree", b);
    P.levels = (uint32_t)count.size();
    std::vector<uint32_t> levelOff(P.levels + 1, 0u);                         // level 0 of the plan = the deepest pairs
    for (uint32_t l = 0; l < P.levels; l++) levelOff[l + 1] = levelOff[l] + count[P.levels - 1 - l];
    std::vector<crt::RefitPlanRec> recs(np); std::vector<uint32_t> fill(levelOff.begin(), levelOff.end() - 1);
    for (uint32_t p = 0; p < np; p++) recs[fill[P.levels - 1 - depth[p]]++] = crt::RefitPlanRec{p, {code_of(pairs[p].c[0].ref), code_of(pairs[p].c[1].ref)}, 0u};
    if (np) {
        HIPCK(c, hipMalloc(&P.dPlan, (size_t)np * sizeof(crt::RefitPlanRec))); c->refitAllocs.push_back(P.dPlan);
        HIPCK(c, hipMalloc((void**)&P.dLevelOff, levelOff.size() * 4)); c->refitAllocs.push_back(P.dLevelOff);
        HIPCK(c, hipMemcpy(P.dPlan, recs.data(), (size_t)np * sizeof(crt::RefitPlanRec), hipMemcpyHostToDevice));
        HIPCK(c, hipMemcpy(P.dLevelOff, levelOff.data(), levelOff.size() * 4, hipMemcpyHostToDevice));
    }
    P.built = true;
    c->refitPlans[b] = P;
    return 0;
}

int crt_refit_device(crt_ctx* c, uint32_t bvh, const float* d_positions, uint32_t triCount, void* stream, float rootBox[6])
{
    const char* const me = "crt_refit_device";
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = check_bvh_arg(c, me, "BVH to refit", bvh, triCount, " (Refit keeps the topology)"))) return r;
    crt_ctx::Flat& f = c->flat; crt_ctx::Refit& R = c->refit;
    hipStream_t st = nullptr;
    if ((r = device_entry(c, me, {{d_positions, (size_t)triCount * 36u}}, stream, &st))) return r;
    if (c->refitPlans.size() != f.triCount.size()) c->refitPlans.assign(f.triCount.size(), crt_ctx::RefitPlan{});
    if (!c->refitPlans[bvh].built && (r = build_refit_plan(c, bvh))) return r;
    const crt_ctx::RefitPlan& P = c->refitPlans[bvh];
    if (!R.dBack) HIPCK(c, hipMalloc((void**)&R.dBack, 128));
    if (!R.hBack) HIPCK(c, hipHostMalloc((void**)&R.hBack, 128, hipHostMallocDefault));
    HIPCK(c, ensure_event(&R.done));
    // In place, on the caller's stream: a write of the scene-write protocol.  The read-back rides inside it (`done` is recorded behind both copies), so the entry's
    // one host wait is for the event that end_scene_write has just published.
    if ((r = begin_scene_write(c, st))) return r;
    HIPCK(c, crt_launch_refit(const_cast<char*>(c->hScene.geom), (uint32_t)f.leafOff, (uint32_t)f.pairBase[bvh], (uint32_t)f.triBase[bvh], triCount, d_positions,
                              P.dPlan, P.dLevelOff, P.levels, P.rootCode, R.dBack, st));
    HIPCK(c, hipMemcpyAsync(R.hBack, R.dBack, 88, hipMemcpyDeviceToHost, st));
    if (c->dRootBox) HIPCK(c, hipMemcpyAsync(c->dRootBox + 6 * (size_t)bvh, R.dBack + 16, 24, hipMemcpyDeviceToDevice, st));   // the box pass's node-0 box, for crt_update_transforms_device
    if ((r = end_scene_write(c, st, R.done))) return r;
    // the one host wait: Scene::rootPair travels in the kernel arguments of every later launch, so the refitted pair has to be on the host before this call returns
    HIPCK(c, hipEventSynchronize(R.done));
    const float* back = R.hBack;
    memcpy(&f.rootBox[6 * (size_t)bvh], back + 16, 24);
    if (P.rootCode & crt::kPlanInterior) memcpy(f.geom.data() + (size_t)(f.pairBase[bvh] + (P.rootCode & ~crt::kPlanInterior)) * 64u, back, 64);   // the mirror's copy of the root's pair
    if (f.kind == CRT_SCENE_FILE) set_root(c, CRT_SCENE_FILE, back + 16, back + 19);      // rootPair from the mirror, dispatch-order bounds; a BLAS's box reaches the TLAS through the caller
    for (crt_ctx::BlasSet& b : c->blasSet) b.stale(bvh);                   // crt_build_kdtree_device(bvh) / crt_build_grid_device(bvh) make it current again
    drop_blas_sets(c);
    if (rootBox) memcpy(rootBox, back + 16, 24);
    return CRT_OK;
}

// a built image's node section in the reference layout again (TLASBVH::tlasNode): leftRight / BLAS from the packed reference
static void unpack_tlas_nodes(const crt::TlasNode* nodes, uint32_t count, crt_tlas_node* out)
{
    for (uint32_t i = 0; i < count; i++) {
        const crt::TlasNode& n = nodes[i]; crt_tlas_node& o = out[i];
        memcpy(o.aabbMin, n.lo, 12); memcpy(o.aabbMax, n.hi, 12);
        const bool leaf = (n.ref & 0xC0000000u) == crt::kRefTlasLeaf;
        o.leftRight = leaf ? 0u : ((n.ref & 0x7fffu) | (((n.ref >> 15) & 0x7fffu) << 16));
        o.BLAS = leaf ? (n.ref & 0xffffu) : 0u;
    }
}

// ---- crt_update_transforms_device: SetTransform of every BLAS + TLASBVH::Build on the device, from transforms in device memory (device/tlas_build.hip) ----
int crt_update_transforms_device(crt_ctx* c, const float* d_T, uint32_t blasCount, void* stream, crt_tlas_node* tlasOut)
{
    const char* const me = "crt_update_transforms_device";
    if (!c) return CRT_ERR_INVALID;
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no instances", me);
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", me);
    crt_ctx::Flat& f = c->flat; crt_ctx::TlasBuild& B = c->tlasBuild; int r;
    if (f.kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_INVALID, "crt_update_transforms_device applies to two-level scenes (a FileScene bakes its transforms into the triangles)");
    const uint32_t N = (uint32_t)f.triCount.size();
    if (blasCount != N) return c->fail(CRT_ERR_INVALID, "crt_update_transforms_device: %u transforms, the uploaded scene has %u BLAS", blasCount, N);
    if (f.tlasNodeCount != 2u * N) return c->fail(CRT_ERR_UNSUPPORTED, "crt_update_transforms_device: the scene was uploaded with %u TLAS nodes, TLASBVH::Build makes %u", f.tlasNodeCount, 2u * N);
    hipStream_t st = nullptr;
    if ((r = device_entry(c, me, {{d_T, (size_t)N * 64u}}, stream, &st))) return r;
    const size_t imageBytes = (size_t)(f.shadeOff - f.tlasOff), backBytes = sizeof(crt::TlasBuildHeader) + imageBytes;
    if (B.bytes < backBytes) {                                              // a larger scene than the last one: nothing of an earlier call is in flight in these (see below)
        if (B.done) HIPCK(c, hipEventSynchronize(B.done));
        if (B.dBuild) { HIPCK(c, hipFree(B.dBuild)); B.dBuild = nullptr; }
        if (B.hBack) { HIPCK(c, hipHostFree(B.hBack)); B.hBack = nullptr; }
        B.bytes = 0;
        HIPCK(c, hipMalloc((void**)&B.dBuild, backBytes));
        HIPCK(c, hipHostMalloc((void**)&B.hBack, backBytes, hipHostMallocDefault));
        HIPCK(c, hipMemset(B.dBuild, 0, backBytes));                        // the padding between the image's sections stays zero, as in the host's image: the kernel writes records only
        B.bytes = backBytes;
    }
    for (hipEvent_t* e : {&B.back, &B.done}) HIPCK(c, ensure_event(e));
    if (g_hooks) for (hipEvent_t* e : {&B.t0, &B.t1}) HIPCK(c, ensure_event(e, hipEventDefault));
    // The build is a reader: it reads only the Instance records and the node-0 boxes as the last write left them, and writes only the context's result block, which
    // the commit copy of an earlier call may still be reading on another stream — all behind sceneReady, so it waits for that alone, not for earlier renders or queries.
    if ((r = wait_scene(c, st))) return r;
    if (g_hooks) HIPCK(c, hipEventRecord(B.t0, st));
    HIPCK(c, crt_launch_tlas_build(c->hScene.geom, (uint32_t)f.instOff, d_T, c->dRootBox, N, (uint32_t)(f.tlasPairOff - f.tlasOff), (uint32_t)(f.instOff - f.tlasOff), c->hScene.poolRefBits, B.dBuild, st));
    if (g_hooks) { HIPCK(c, hipEventRecord(B.t1, st)); B.timed = true; }
    // the one host wait: the root's pair and the stack depth travel in the kernel arguments of every later launch, and only a build that passed is committed
    if ((r = read_back(c, st, B.back, B.hBack, B.dBuild, backBytes))) return r;
    const crt::TlasBuildHeader& h = *reinterpret_cast<const crt::TlasBuildHeader*>(B.hBack);
    const char* image = B.hBack + sizeof(crt::TlasBuildHeader);
    if (h.status == crt::kTlasBuildNoCandidate)
        return c->fail(CRT_ERR_INVALID, "crt_update_transforms_device: FindBestMatch call %u found no partner while more than one node was open (a non-finite transform or box, or areas >= 1e30; the reference reads list[-1] there)", h.step);
    if (h.status != crt::kTlasBuildOk) return c->fail(CRT_ERR_INVALID, "crt_update_transforms_device: the build had not ended after %u FindBestMatch calls", h.step);
    if ((r = check_tlas_height(c, h.height))) return r;
    // ---- commit: the write proper, in place on the caller's stream ----
    if ((r = begin_scene_write(c, st))) return r;
    HIPCK(c, hipMemcpyAsync(const_cast<char*>(c->hScene.geom) + f.tlasOff, B.dBuild + sizeof(crt::TlasBuildHeader), imageBytes, hipMemcpyDeviceToDevice, st));
    if ((r = end_scene_write(c, st, B.done))) return r;
    memcpy(f.geom.data() + f.tlasOff, image, imageBytes);                  // the mirror: a later CRT_UPDATE_BOUNDS rewrites [tlasOff, shadeOff) from it
    const crt::TlasNode* nodes = reinterpret_cast<const crt::TlasNode*>(image);
    adopt_tlas(c, h.height, nodes[0].lo, nodes[0].hi);
    if (tlasOut) unpack_tlas_nodes(nodes, 2u * N, tlasOut);
    return CRT_OK;
}

// ---- crt_build_grid_device / crt_build_kdtree_device: one BVH's uniform grid / KD-tree rebuilt on the device from positions in device memory, into FRESH buffers
// that replace the live ones.  The two entries differ in the kernels they launch and in the arrays they name; what surrounds the kernels is AccelReplace ----
// scratch of a build that grows on demand; the previous build of the kind may still be using it, so the host waits for that build first (earlier work only)
static int grow_scratch(crt_ctx* c, const crt_ctx::AccelBuild& B, void** p, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return 0;
    if (B.built) HIPCK(c, hipEventSynchronize(B.done));
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return c->fail(CRT_ERR_DEVICE, "device build scratch: hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    *cap = bytes;
    return 0;
}

// What a replaced buffer set's retirement takes, once `done` is recorded on `st` behind the build: the replaced buffers are still read by launches enqueued earlier, on
// any stream, and by the build's own copies.  The main stream goes behind all those readers and behind the build (`done` published: launches enqueued from now on
// wait for it), and old.unread, recorded on it then, says when the old buffers are unread.  The caller fills old.ptrs and pushes `old` onto c->retired.
static int retire_behind_readers(crt_ctx* c, hipStream_t st, hipEvent_t done, crt_ctx::Retired& old)
{
    if (c->retiredEvents.empty()) { hipEvent_t e = nullptr; HIPCK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->retiredEvents.push_back(e); }
    old.unread = c->retiredEvents.back(); c->retiredEvents.pop_back();
    int r;
    if ((r = order_behind_readers(c)) || (r = publish_scene_write(c, st, done)) || (r = c->hip(hipEventRecord(old.unread, c->stream), "hipEventRecord(retired)"))) {
        c->retiredEvents.push_back(old.unread); old.unread = nullptr;
    }
    return r;
}

// One replacement, slot 0: the KD-tree, 1: the grid (as blasAlt / haveBlas / blasAllocs).  The kind's arrays are numbered 0: KD nodes / cellStart, 1: KD references /
// cellRefs, 2: the AltTri records.  A FileScene's structure is the arrays alone; a two-level scene's is BLAS `bvh`'s part of the set's concatenated arrays, and the
// other BLASes' parts are carried over.  The entry calls begin, prepare, its kernels up to the sizes it reads back, place + alloc per array, carry, the kernels that
// write the result, commit — and then names the new arrays in AltAccelDev / TlasAltDev.  After the first alloc every failure frees what the call allocated (undo).
struct AccelReplace {
    crt_ctx* c; const char* me; int slot; crt_ctx::AccelBuild& B; uint32_t bvh;
    hipStream_t st = nullptr; bool tlas = false; uint32_t N = 0;
    std::vector<void*> fresh; void* pinned = nullptr;
    uint64_t base[3] = {0, 0, 0}, all[3] = {0, 0, 0}; uint32_t part[3] = {0, 0, 0};     // place(): where the new part starts in array k, the array's elements, the part's
    std::vector<crt::BlasAltDesc> desc; crt::BlasAltDesc* newDesc = nullptr;          // the set's descriptors re-based by place(); on the device after carry()

    crt_ctx::BlasSet& set() const { return c->blasSet[slot]; }
    uint32_t crt::BlasAltDesc::* base_of(int k) const
    {
        return k == 2 ? &crt::BlasAltDesc::triBase : slot ? (k ? &crt::BlasAltDesc::cellRefBase : &crt::BlasAltDesc::cellBase) : (k ? &crt::BlasAltDesc::refBase : &crt::BlasAltDesc::nodeBase);
    }
    const std::vector<uint32_t>& counts(int k) const { return k == 2 ? c->flat.triCount : set().count[k]; }
    void undo() { (void)hipStreamSynchronize(st); for (void* p : fresh) (void)hipFree(p); if (pinned) (void)hipHostFree(pinned); }
    int hip(hipError_t e, const char* what) { if (e == hipSuccess) return 0; undo(); return c->hip(e, what); }
    int drop(int r) { if (r) undo(); return r; }
#define REPLCK(R, call) do { if (const int r_ = (R).hip((call), #call)) return r_; } while (0)

    // the entry checks, and the buffers retired by earlier calls that are unread by now
    int begin(const float* d_positions, uint32_t triCount, void* stream)
    {
        int r;
        if ((r = check_bvh_arg(c, me, "triangles", bvh, triCount, ""))) return r;
        tlas = c->flat.kind == CRT_SCENE_TLAS; N = (uint32_t)c->flat.triCount.size();
        if (triCount == 0 || triCount > 0x7fffffffu / 3u) return c->fail(CRT_ERR_UNSUPPORTED, "%s: 1 .. (2^31-1)/3 triangles", me);
        if (tlas && (!set().held || set().desc.size() != N))
            return c->fail(CRT_ERR_STATE, "%s: a two-level scene needs a %s set uploaded earlier (crt_upload_blas_accel(%s)): the other BLASes' parts are carried over", me,
                           slot ? "grid" : "KD", slot ? "CRT_ACCEL_GRID" : "CRT_ACCEL_KDTREE");
        if ((r = device_entry(c, me, {{d_positions, (size_t)triCount * 36u}}, stream, &st))) return r;
        c->freeRetired(false);
        if (tlas) desc = set().desc;
        return 0;
    }
    // Fresh buffers, so the build is a reader: it reads the caller's positions and the LeafTri id words (which no write changes) and waits for the last scene write
    // and for the previous build (whose scratch it reuses).  Earlier renders and queries are not waited for until the old structure is retired.
    int prepare()
    {
        if (!B.blocks && !(B.blocks = crt_grid_build_blocks(c->cfg.device))) return c->fail(CRT_ERR_DEVICE, "%s: the device's compute units / occupancy could not be asked", me);
        for (hipEvent_t* e : {&B.back, &B.done}) HIPCK(c, ensure_event(e));
        if (g_hooks) for (hipEvent_t* e : {&B.t0, &B.t1}) HIPCK(c, ensure_event(e, hipEventDefault));
        if (const int r = wait_scene(c, st)) return r;
        if (B.built) HIPCK(c, hipStreamWaitEvent(st, B.done, 0));
        if (g_hooks) HIPCK(c, hipEventRecord(B.t0, st));
        return 0;
    }
    // array k with the new part `count` elements long: the part alone (FileScene), or at its re-based place among the other BLASes' parts
    void place(int k, uint32_t count)
    {
        part[k] = count; base[k] = 0; all[k] = count;
        if (!tlas) return;
        all[k] = 0;
        for (uint32_t b = 0; b < N; b++) { if (b == bvh) base[k] = all[k]; desc[b].*base_of(k) = (uint32_t)all[k]; all[k] += b == bvh ? count : counts(k)[b]; }
    }
    int alloc(size_t bytes, void** out)
    {
        *out = nullptr; if (!bytes) return 0;
        const hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; undo(); return c->fail(CRT_ERR_DEVICE, "%s: hipMalloc(%zu): %s", me, bytes, hipGetErrorString(e)); }
        fresh.push_back(*out); return 0;
    }
    // the other BLASes' parts of the three arrays, device to device (dst: the new arrays, src: the live set's, elem: bytes per element), and the re-based descriptors
    int carry(void* const dst[3], const void* const src[3], const size_t elem[3])
    {
        if (!tlas) return 0;
        for (uint32_t b = 0; b < N; b++)
            for (int k = 0; k < 3 && b != bvh; k++) {
                const size_t n = counts(k)[b], to = desc[b].*base_of(k), from = set().desc[b].*base_of(k);
                if (n) REPLCK(*this, hipMemcpyAsync((char*)dst[k] + to * elem[k], (const char*)src[k] + from * elem[k], n * elem[k], hipMemcpyDeviceToDevice, st));
            }
        if (const int r = alloc(desc.size() * sizeof(crt::BlasAltDesc), (void**)&newDesc)) return r;
        REPLCK(*this, hipHostMalloc(&pinned, desc.size() * sizeof(crt::BlasAltDesc), hipHostMallocDefault));     // read by the copy below after this call has returned: retired with the old set
        memcpy(pinned, desc.data(), desc.size() * sizeof(crt::BlasAltDesc));
        REPLCK(*this, hipMemcpyAsync(newDesc, pinned, desc.size() * sizeof(crt::BlasAltDesc), hipMemcpyHostToDevice, st));
        return 0;
    }
    // `done` behind the build, the structure it replaces retired, the new buffers the context's
    int commit(crt::AltTri* newTris)
    {
        if (g_hooks) { REPLCK(*this, hipEventRecord(B.t1, st)); B.timed = true; }
        REPLCK(*this, hipEventRecord(B.done, st));
        B.built = true;
        crt_ctx::Retired old;                                              // (what it replaces is also read by this build's own copies: the other BLASes' parts, the pinned descriptors)
        if (const int r = retire_behind_readers(c, st, B.done, old)) return drop(r);
        old.pinned = pinned;
        if (tlas) {
            crt_ctx::BlasSet& S = set();
            old.ptrs.swap(c->blasAllocs[slot]); c->blasAllocs[slot] = fresh;
            S.desc = desc; S.count[0][bvh] = part[0]; S.count[1][bvh] = part[1]; S.current[bvh] = 1;
            c->haveBlas[slot] = S.allCurrent();                            // live again once every BLAS's part is of its current vertices
        } else {
            old.ptrs.swap(c->altAllocs[slot]);
            for (void* p : fresh) if (p != (void*)newTris) c->altAllocs[slot].push_back(p);              // (newTris is not an accelerator array: it becomes altTris)
            if (c->altTris) old.ptrs.push_back(c->altTris);
            c->altTris = newTris; c->altTriCount = part[2]; c->alt.tris = newTris;
            // the other structure shares altTris and is of the old positions: the entry marks it absent, as a refit marks a two-level set (its arrays go with its next upload or build)
            if (c->renderAccel == (slot ? CRT_ACCEL_KDTREE : CRT_ACCEL_GRID)) c->renderAccel = 0;
        }
        c->retired.push_back(std::move(old));
        return 0;
    }
};

int crt_build_grid_device(crt_ctx* c, uint32_t bvh, const float* d_positions, uint32_t triCount, void* stream)
{
    const char* const me = "crt_build_grid_device";
    if (!c) return CRT_ERR_INVALID;
    crt_ctx::Flat& f = c->flat; crt_ctx::GridBuild& G = c->gridBuild;
    AccelReplace R{c, me, 1, G, bvh};
    int r;
    if ((r = R.begin(d_positions, triCount, stream))) return r;
    hipStream_t st = R.st;
    if (!G.dState) HIPCK(c, hipMalloc((void**)&G.dState, sizeof(crt::GridBuildState)));
    if (!G.hState) HIPCK(c, hipHostMalloc((void**)&G.hState, sizeof(crt::GridBuildState), hipHostMallocDefault));
    if (!G.dChunks) HIPCK(c, hipMalloc((void**)&G.dChunks, crt_grid_scan_chunks(128u * 128u * 128u) * 8u));
    if ((r = R.prepare())) return r;
    // ---- a. bounds + finiteness; THE FIRST HOST WAIT: the resolution is computed on the host from the bounds ----
    HIPCK(c, crt_launch_grid_bounds(d_positions, triCount, G.dState, G.blocks, st));
    if ((r = read_back(c, st, G.back, G.hState, G.dState, sizeof(crt::GridBuildState), &G.waitMs[0]))) return r;
    if (G.hState->nonFinite) return c->fail(CRT_ERR_INVALID, "%s: a position component is not finite", me);
    // ---- b. localBounds as aabb::Grow folds them from +-1e34, then the resolution lines shared with the host build ----
    crt::GridParams gp{}; float hi[3], size[3], cell[3]; int res[3];
    for (int k = 0; k < 3; k++) {
        const float lo = crt::bound_of_key(G.hState->key[k]), up = crt::bound_of_key(G.hState->key[3 + k]);
        gp.lo[k] = 1e34f < lo ? 1e34f : lo; hi[k] = -1e34f > up ? -1e34f : up;
        size[k] = hi[k] - gp.lo[k];
    }
    crt::grid_resolution(size, (int)triCount, res, cell);
    for (int k = 0; k < 3; k++) { gp.res[k] = res[k]; gp.cell[k] = cell[k]; }
    const uint32_t cells = (uint32_t)res[0] * (uint32_t)res[1] * (uint32_t)res[2];
    // ---- cellStart is allocated between the waits: the count kernel writes it ----
    R.place(0, cells + 1u);
    if (R.all[0] > 0xffffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the grid set has too many cells", me);
    uint32_t* newStart = nullptr;
    if ((r = R.alloc((size_t)R.all[0] * 4u, (void**)&newStart))) return r;
    // ---- c, d. count + exclusive scan; THE SECOND HOST WAIT: cellRefs is sized from the total ----
    REPLCK(R, crt_launch_grid_count(d_positions, triCount, &gp, cells, newStart + R.base[0], G.dChunks, G.dState, G.blocks, st));
    if ((r = R.drop(read_back(c, st, G.back, G.hState, G.dState, sizeof(crt::GridBuildState), &G.waitMs[1])))) return r;
    const unsigned long long total64 = G.hState->total;
    const uint32_t total = (uint32_t)total64;
    R.place(1, total); R.place(2, triCount);
    if (total64 > 0x7fffffffull || R.all[1] > 0xffffffffull) { R.undo(); return c->fail(CRT_ERR_UNSUPPORTED, "%s: %llu cell references (at most 2^31-1)", me, total64); }
    int32_t* newRefs = nullptr; crt::AltTri* newTris = nullptr;
    if ((r = R.alloc((size_t)R.all[1] * 4u, (void**)&newRefs)) || (r = R.alloc((size_t)R.all[2] * sizeof(crt::AltTri), (void**)&newTris))) return r;
    if ((r = R.drop(grow_scratch(c, G, &G.dCursor, &G.cursorCap, (size_t)cells * 4u))) || (r = R.drop(grow_scratch(c, G, &G.dUnsorted, &G.unsortedCap, (size_t)total * 4u)))) return r;
    if (R.tlas) { crt::BlasAltDesc& nd = R.desc[bvh]; for (int k = 0; k < 3; k++) { nd.res[k] = res[k]; nd.cell[k] = cell[k]; nd.lo[k] = gp.lo[k]; nd.hi[k] = hi[k]; } }
    const crt::TlasAltDev& live = c->blasAlt[1];
    void* const dst[3] = {newStart, newRefs, newTris}; const void* const src[3] = {live.cellStart, live.cellRefs, live.tris}; const size_t elem[3] = {4u, 4u, sizeof(crt::AltTri)};
    if ((r = R.carry(dst, src, elem))) return r;
    // ---- e, f. fill, sort every cell ascending, the AltTri records ----
    REPLCK(R, crt_launch_grid_fill(d_positions, triCount, &gp, cells, newStart + R.base[0], (uint32_t*)G.dCursor, (int32_t*)G.dUnsorted, newRefs ? newRefs + R.base[1] : nullptr, total,
                                   c->hScene.geom, (uint32_t)f.leafOff, (uint32_t)f.triBase[bvh], R.tlas ? 1 : 0, newTris + R.base[2], G.blocks, st));
    if ((r = R.commit(newTris))) return r;
    if (R.tlas) {
        crt::TlasAltDev& tl = c->blasAlt[1];
        tl.desc = R.newDesc; tl.tris = newTris; tl.cellStart = newStart; tl.cellRefs = newRefs; tl.kdNodes = nullptr; tl.kdRefs = nullptr; tl.kdStack = 0;
    } else {
        crt::AltAccelDev& a = c->alt;
        a.cellStart = newStart; a.cellRefs = newRefs;
        for (int k = 0; k < 3; k++) { a.res[k] = res[k]; a.cell[k] = cell[k]; a.lo[k] = gp.lo[k]; a.hi[k] = hi[k]; }
        c->haveGrid = true; c->gridRefCount = total;
        c->haveKd = false; a.kdNodes = nullptr; a.kdRefs = nullptr; a.kdStack = 0;       // the KD-tree: absent
    }
    return CRT_OK;
}

// what crt_get_grid and crt_get_kdtree check first; *tlas: the structure is BLAS bvh's part of a two-level scene's set
static int get_accel_head(crt_ctx* c, const char* me, int slot, uint32_t bvh, bool* tlas)
{
    if (!c) return CRT_ERR_INVALID;
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", me);
    if (bvh >= c->flat.triCount.size()) return c->fail(CRT_ERR_INVALID, "%s: BVH %u of a scene with %zu", me, bvh, c->flat.triCount.size());
    *tlas = c->flat.kind == CRT_SCENE_TLAS;
    if (*tlas ? !(c->haveBlas[slot] && c->blasSet[slot].held) : !(slot ? c->haveGrid : c->haveKd))
        return c->fail(CRT_ERR_STATE, "%s: no live %s (not uploaded, or dropped by a refit and not rebuilt)", me, slot ? "grid" : "KD-tree");
    return 0;
}
// ... and before they copy the arrays: a device build still running (an uploaded structure's copies were synchronous)
static int get_accel_wait(crt_ctx* c, const crt_ctx::AccelBuild& B)
{
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (B.built) HIPCK(c, hipEventSynchronize(B.done));
    return 0;
}

int crt_get_grid(crt_ctx* c, uint32_t bvh, int32_t res[3], float cellSize[3], float gridMin[3], float gridMax[3], uint32_t* cellCount, uint32_t* refCount, uint32_t* cellStart, int32_t* cellRefs)
{
    bool tlas; int rc;
    if ((rc = get_accel_head(c, "crt_get_grid", 1, bvh, &tlas))) return rc;
    const int32_t* r; const float *cs, *lo, *hi; uint32_t cells, refs; const uint32_t* dStart; const int32_t* dRefs;
    if (tlas) {
        const crt_ctx::BlasSet& S = c->blasSet[1]; const crt::BlasAltDesc& d = S.desc[bvh];
        r = d.res; cs = d.cell; lo = d.lo; hi = d.hi; cells = S.count[0][bvh] - 1u; refs = S.count[1][bvh];
        dStart = c->blasAlt[1].cellStart + d.cellBase; dRefs = c->blasAlt[1].cellRefs ? c->blasAlt[1].cellRefs + d.cellRefBase : nullptr;
    } else {
        const crt::AltAccelDev& a = c->alt;
        r = a.res; cs = a.cell; lo = a.lo; hi = a.hi; cells = (uint32_t)a.res[0] * (uint32_t)a.res[1] * (uint32_t)a.res[2]; refs = c->gridRefCount;
        dStart = a.cellStart; dRefs = a.cellRefs;
    }
    for (int k = 0; k < 3; k++) { if (res) res[k] = r[k]; if (cellSize) cellSize[k] = cs[k]; if (gridMin) gridMin[k] = lo[k]; if (gridMax) gridMax[k] = hi[k]; }
    if (cellCount) *cellCount = cells;
    if (refCount) *refCount = refs;
    if (!cellStart && !cellRefs) return CRT_OK;
    if ((rc = get_accel_wait(c, c->gridBuild))) return rc;
    if (cellStart) HIPCK(c, hipMemcpy(cellStart, dStart, ((size_t)cells + 1u) * 4u, hipMemcpyDeviceToHost));
    if (cellRefs && refs) HIPCK(c, hipMemcpy(cellRefs, dRefs, (size_t)refs * 4u, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_build_kdtree_device(crt_ctx* c, uint32_t bvh, const float* d_positions, uint32_t triCount, void* stream)
{
    const char* const me = "crt_build_kdtree_device";
    if (!c) return CRT_ERR_INVALID;
    crt_ctx::Flat& f = c->flat; crt_ctx::KdBuild& K = c->kdBuild;
    AccelReplace R{c, me, 0, K, bvh};
    int r;
    if ((r = R.begin(d_positions, triCount, stream))) return r;
    hipStream_t st = R.st;
    if (!K.dState) HIPCK(c, hipMalloc((void**)&K.dState, sizeof(crt::KdBuildState)));
    if (!K.hState) HIPCK(c, hipHostMalloc((void**)&K.hState, sizeof(crt::KdBuildState), hipHostMallocDefault));
    crt_ctx::KdBuild::Level* lv = K.lv;
    if ((r = grow_scratch(c, K, &K.dTriBox, &K.triBoxCap, (size_t)triCount * 24u)) || (r = grow_scratch(c, K, &lv[0].nodes, &lv[0].nodeCap, sizeof(crt::KdBuildNode))) ||
        (r = grow_scratch(c, K, &lv[0].refs, &lv[0].refCap, (size_t)triCount * 4u)) || (r = grow_scratch(c, K, &lv[0].owner, &lv[0].ownerCap, (size_t)triCount * 4u))) return r;
    if ((r = R.prepare())) return r;
    K.waits = 0; K.waitMs = 0; K.levels = 0;
    // ---- a. bounds + finiteness, the triangle boxes, level 0 (no wait of its own: level 0's read-back carries the flag) ----
    HIPCK(c, crt_launch_kd_begin(d_positions, triCount, K.dState, (float*)K.dTriBox, (crt::KdBuildNode*)lv[0].nodes, (uint32_t*)lv[0].refs, (uint32_t*)lv[0].owner, K.blocks, st));
    // ---- b. level by level; ONE HOST WAIT PER LEVEL: the next level's node and reference counts size its buffers ----
    uint32_t nodeCount[crt_ctx::KdBuild::kLevels] = {1u}, refCount[crt_ctx::KdBuild::kLevels] = {triCount};
    uint32_t levels = 0; uint64_t allNodes64 = 0, leafRefs64 = 0;
    for (uint32_t d = 0; d < crt_ctx::KdBuild::kLevels; d++) {
        const uint32_t m = nodeCount[d], t = refCount[d];
        if ((r = grow_scratch(c, K, &K.dNodeItems, &K.nodeItemCap, ((size_t)m + 1u) * 8u)) || (r = grow_scratch(c, K, &K.dRefItems, &K.refItemCap, ((size_t)t + 1u) * 8u)) ||
            (r = grow_scratch(c, K, &K.dChunks, &K.chunkCap, crt_kd_scan_chunks(m > t ? m : t) * 8u))) return r;
        HIPCK(c, crt_launch_kd_level((crt::KdBuildNode*)lv[d].nodes, m, d, (const uint32_t*)lv[d].owner, (const uint32_t*)lv[d].refs, t, (const float*)K.dTriBox,
                                     (unsigned long long*)K.dNodeItems, (unsigned long long*)K.dRefItems, (unsigned long long*)K.dChunks, K.dState, K.blocks, st));
        double ms = 0;
        if ((r = read_back(c, st, K.back, K.hState, K.dState, sizeof(crt::KdBuildState), &ms))) return r;
        K.waits++; K.waitMs += ms;
        if (d == 0 && K.hState->bounds.nonFinite) return c->fail(CRT_ERR_INVALID, "%s: a position component is not finite", me);
        const uint64_t splits = K.hState->nodeTotal & 0xffffffffull, leafRefs = K.hState->nodeTotal >> 32;
        const uint64_t next = (K.hState->refTotal & 0xffffffffull) + (K.hState->refTotal >> 32);
        allNodes64 += m; leafRefs64 += leafRefs; levels = d + 1u;
        if (leafRefs64 > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: more than 2^31-1 leaf references", me);
        if (splits == 0) break;
        if (next > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: level %u has %llu references (at most 2^31-1)", me, d + 1u, (unsigned long long)next);
        if (d + 1u >= crt_ctx::KdBuild::kLevels || splits > m) return c->fail(CRT_ERR_DEVICE, "%s: the level kernels reported %llu split nodes of %u at depth %u", me, (unsigned long long)splits, m, d);
        nodeCount[d + 1u] = (uint32_t)(2u * splits); refCount[d + 1u] = (uint32_t)next;
        if ((r = grow_scratch(c, K, &lv[d + 1u].nodes, &lv[d + 1u].nodeCap, (size_t)nodeCount[d + 1u] * sizeof(crt::KdBuildNode))) ||
            (r = grow_scratch(c, K, &lv[d + 1u].refs, &lv[d + 1u].refCap, (size_t)next * 4u)) || (r = grow_scratch(c, K, &lv[d + 1u].owner, &lv[d + 1u].ownerCap, (size_t)next * 4u))) return r;
        HIPCK(c, crt_launch_kd_split((crt::KdBuildNode*)lv[d].nodes, m, (const unsigned long long*)K.dNodeItems, (const uint32_t*)lv[d].owner, (const uint32_t*)lv[d].refs, t,
                                     (const unsigned long long*)K.dRefItems, (crt::KdBuildNode*)lv[d + 1u].nodes, nodeCount[d + 1u], (uint32_t*)lv[d + 1u].refs, (uint32_t*)lv[d + 1u].owner,
                                     refCount[d + 1u], K.blocks, st));
    }
    K.levels = levels;
    const uint32_t height = levels - 1u, newNodes = (uint32_t)allNodes64, newRefs = (uint32_t)leafRefs64;
    // ---- the new tree's arrays, allocated after the last wait; a set's deepest tree sizes the traversal stack ----
    R.place(0, newNodes); R.place(1, newRefs); R.place(2, triCount);
    uint32_t maxKd = height + 1u;
    if (R.tlas) {
        const crt_ctx::BlasSet& S = c->blasSet[0];
        for (uint32_t b = 0; b < R.N; b++) if (b != bvh && S.height[b] + 1u > maxKd) maxKd = S.height[b] + 1u;
        if (R.all[0] > 0xffffffffull || R.all[1] > 0xffffffffull || R.all[2] > 0xffffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the KD set is too large", me);
        const uint32_t words = maxKd * 2u + (c->hScene.stackDepth - c->hScene.bvhStack);      // as crt_upload_blas_accel
        if (!wave_stack_fits(words)) return c->fail(CRT_ERR_UNSUPPORTED, "%s: TLAS + KD-tree traversal stack of %u dwords per lane exceeds the LDS budget", me, words);
    }
    crt::KdNode* newNodeArr = nullptr; uint32_t* newRefArr = nullptr; crt::AltTri* newTris = nullptr;
    if ((r = R.alloc((size_t)R.all[0] * sizeof(crt::KdNode), (void**)&newNodeArr)) || (r = R.alloc((size_t)R.all[1] * 4u, (void**)&newRefArr)) ||
        (r = R.alloc((size_t)R.all[2] * sizeof(crt::AltTri), (void**)&newTris))) return r;
    const crt::TlasAltDev& live = c->blasAlt[0];
    void* const dst[3] = {newNodeArr, newRefArr, newTris}; const void* const src[3] = {live.kdNodes, live.kdRefs, live.tris}; const size_t elem[3] = {sizeof(crt::KdNode), 4u, sizeof(crt::AltTri)};
    if ((r = R.carry(dst, src, elem))) return r;
    // ---- c. finalise: subtree sizes bottom-up, pre-order places top-down, the records and the leaf references; the AltTri records ----
    {
        crt::KdBuildNode* ln[crt_ctx::KdBuild::kLevels]; const uint32_t* lr[crt_ctx::KdBuild::kLevels]; const uint32_t* lo[crt_ctx::KdBuild::kLevels];
        for (uint32_t d = 0; d < levels; d++) { ln[d] = (crt::KdBuildNode*)lv[d].nodes; lr[d] = (const uint32_t*)lv[d].refs; lo[d] = (const uint32_t*)lv[d].owner; }
        REPLCK(R, crt_launch_kd_finalise(ln, lr, lo, nodeCount, refCount, levels, newNodeArr + R.base[0], newNodes, newRefArr ? newRefArr + R.base[1] : nullptr, newRefs, K.blocks, st));
    }
    REPLCK(R, crt_launch_alt_tris(d_positions, triCount, c->hScene.geom, (uint32_t)f.leafOff, (uint32_t)f.triBase[bvh], R.tlas ? 1 : 0, newTris + R.base[2], st));
    if ((r = R.commit(newTris))) return r;
    if (R.tlas) {
        crt::TlasAltDev& tl = c->blasAlt[0];
        tl.desc = R.newDesc; tl.tris = newTris; tl.kdNodes = newNodeArr; tl.kdRefs = newRefArr; tl.cellStart = nullptr; tl.cellRefs = nullptr; tl.kdStack = maxKd;
        c->blasSet[0].height[bvh] = height;
        if (c->renderAccel == CRT_ACCEL_KDTREE && !sample_lds_fits(sample_stack_words(c, CRT_ACCEL_KDTREE))) c->renderAccel = 0;   // (a set rebuilt while live, now deeper than the render stack)
    } else {
        crt::AltAccelDev& a = c->alt;
        a.kdNodes = newNodeArr; a.kdRefs = newRefArr; a.kdStack = height + 1u;
        c->haveKd = true; c->kdNodeCount = newNodes; c->kdRefCount = newRefs;
        c->haveGrid = false; a.cellStart = nullptr; a.cellRefs = nullptr; c->gridRefCount = 0;     // the grid: absent
        for (int k = 0; k < 3; k++) { a.res[k] = 0; a.cell[k] = 0.0f; a.lo[k] = 0.0f; a.hi[k] = 0.0f; }
    }
    return CRT_OK;
}
#undef REPLCK

int crt_get_kdtree(crt_ctx* c, uint32_t bvh, uint32_t* nodeCount, uint32_t* refCount, uint32_t* height, crt_kd_node* nodes, uint32_t* refs)
{
    bool tlas; int rc;
    if ((rc = get_accel_head(c, "crt_get_kdtree", 0, bvh, &tlas))) return rc;
    uint32_t nn, nr, h; const crt::KdNode* dNodes; const uint32_t* dRefs;
    if (tlas) {
        const crt_ctx::BlasSet& S = c->blasSet[0]; const crt::BlasAltDesc& d = S.desc[bvh];
        nn = S.count[0][bvh]; nr = S.count[1][bvh]; h = S.height[bvh];
        dNodes = static_cast<const crt::KdNode*>(c->blasAlt[0].kdNodes) + d.nodeBase; dRefs = c->blasAlt[0].kdRefs ? c->blasAlt[0].kdRefs + d.refBase : nullptr;
    } else { nn = c->kdNodeCount; nr = c->kdRefCount; h = c->alt.kdStack - 1u; dNodes = c->alt.kdNodes; dRefs = c->alt.kdRefs; }
    if (nodeCount) *nodeCount = nn;
    if (refCount) *refCount = nr;
    if (height) *height = h;
    if (!nodes && !refs) return CRT_OK;
    if ((rc = get_accel_wait(c, c->kdBuild))) return rc;
    if (nodes) HIPCK(c, hipMemcpy(nodes, dNodes, (size_t)nn * sizeof(crt::KdNode), hipMemcpyDeviceToHost));
    if (refs && nr) HIPCK(c, hipMemcpy(refs, dRefs, (size_t)nr * 4u, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// tools/kdtree_device_cost.py: the last crt_build_kdtree_device's duration on its stream (HIP events, first launch to last; it includes the host round trips in
// between), the number of its host waits and their wall time together, and its levels (debug hooks only)
extern "C" int crt_debug_kdtree_build_ms(crt_ctx* c, float* streamMs, double* waitMs, uint32_t* waits, uint32_t* levels)
{
    if (!c || !streamMs || !waitMs || !waits || !levels) return CRT_ERR_INVALID;
    const crt_ctx::KdBuild& K = c->kdBuild;
    if (!K.timed) return c->fail(CRT_ERR_STATE, "crt_debug_kdtree_build_ms: no timed crt_build_kdtree_device (debug hooks off?)");
    HIPCK(c, hipEventSynchronize(K.t1));
    HIPCK(c, hipEventElapsedTime(streamMs, K.t0, K.t1));
    *waitMs = K.waitMs; *waits = K.waits; *levels = K.levels;
    return CRT_OK;
}

// ---- crt_build_bvh_device: BVH::Build / BLASBVH::Build of one BVH on the device, from positions in device memory (device/bvh_build.hip).  The tree's size changes, so
// the pair section does, and every section behind it moves: the result is a FRESH geometry buffer — the rebuilt BVH's pairs and leaf triangles written by the kernels,
// the other BVHs' pairs re-based, everything else copied device to device — which replaces the live one as crt_build_grid_device replaces a grid ----
int crt_build_bvh_device(crt_ctx* c, uint32_t bvh, const float* d_positions, uint32_t triCount, void* stream, float rootBox[6])
{
    const char* const me = "crt_build_bvh_device";
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = check_bvh_arg(c, me, "BVH to rebuild", bvh, triCount, " (a rebuild keeps the triangles)"))) return r;
    crt_ctx::Flat& f = c->flat; crt_ctx::BvhBuild& B = c->bvhBuild;
    const uint32_t n = triCount, N = (uint32_t)f.triCount.size();
    if (n == 0 || n > 0x7fffffffu / 3u) return c->fail(CRT_ERR_UNSUPPORTED, "%s: 1 .. (2^31-1)/3 triangles", me);
    hipStream_t st = nullptr;
    if ((r = device_entry(c, me, {{d_positions, (size_t)n * 36u}}, stream, &st))) return r;
    c->freeRetired(false);
    if (!B.dState) HIPCK(c, hipMalloc((void**)&B.dState, sizeof(crt::BvhBuildState)));
    if (!B.hState) HIPCK(c, hipHostMalloc((void**)&B.hState, sizeof(crt::BvhBuildState), hipHostMallocDefault));
    enum { kNodes, kKeys, kCen, kIdx0, kIdx1, kOwner0, kOwner1, kRemain, kObj, kLeft, kSplit, kChunks, kBins };
    const size_t need[crt_ctx::BvhBuild::kBufs - 1] = {2u * (size_t)n * sizeof(crt::BvhBuildNode), 2u * (size_t)n * 48u, (size_t)n * 12u, (size_t)n * 4u, (size_t)n * 4u, (size_t)n * 4u,
                                                       (size_t)n * 4u, (size_t)n * 4u, (size_t)n * 4u, ((size_t)n + 1u) * 4u, ((size_t)n + 1u) * 4u, crt::scan_chunks((size_t)n + 1u) * 8u};
    for (int k = 0; k < crt_ctx::BvhBuild::kBufs - 1; k++) if ((r = grow_scratch(c, B, &B.buf[k], &B.cap[k], need[k]))) return r;
    crt::BvhBuildNode* nodes = (crt::BvhBuildNode*)B.buf[kNodes]; unsigned long long* keys = (unsigned long long*)B.buf[kKeys];
    uint32_t* idx[2] = {(uint32_t*)B.buf[kIdx0], (uint32_t*)B.buf[kIdx1]}; uint32_t* owner[2] = {(uint32_t*)B.buf[kOwner0], (uint32_t*)B.buf[kOwner1]};
    // Fresh buffer, so the build is a reader (as AccelReplace::prepare): it reads the caller's positions and the LeafTri id words and waits for the last scene write
    // and for the previous build, whose scratch it reuses
    if (!B.blocks && !(B.blocks = crt_grid_build_blocks(c->cfg.device))) return c->fail(CRT_ERR_DEVICE, "%s: the device's compute units / occupancy could not be asked", me);
    for (hipEvent_t* e : {&B.back, &B.done}) HIPCK(c, ensure_event(e));
    if (g_hooks) for (hipEvent_t* e : {&B.t0, &B.t1}) HIPCK(c, ensure_event(e, hipEventDefault));
    if ((r = wait_scene(c, st))) return r;
    if (B.built) HIPCK(c, hipStreamWaitEvent(st, B.done, 0));
    if (g_hooks) HIPCK(c, hipEventRecord(B.t0, st));
    B.waits = 0; B.levels = 0; B.waitMs = 0; B.readBackMs = 0;
    HIPCK(c, crt_launch_bvh_begin(d_positions, n, c->hScene.geom, (uint32_t)f.leafOff, (uint32_t)f.triBase[bvh], (float*)B.buf[kCen], idx[0], owner[0], (int32_t*)B.buf[kObj], nodes, keys,
                                  B.dState, B.blocks, st));
    // ---- level by level; ONE HOST WAIT PER LEVEL: the number of nodes that split sizes the next level.  The bound of the loop is the traversal stack: a level d
    // with nodes means a leaf at depth >= d, and crt_upload_scene refuses a tree whose stack does not fit the LDS ----
    const uint32_t tlasPart = c->hScene.stackDepth - c->hScene.bvhStack;          // TLAS pushes + the return marker (0 for a FileScene)
    uint32_t otherHeight = 0;
    for (uint32_t b = 0; b < N; b++) if (b != bvh && f.height[b] > otherHeight) otherHeight = f.height[b];
    auto stack_of = [&](uint32_t h) { const uint32_t m = h > otherHeight ? h : otherHeight; return (m ? m : 1u) + tlasPart; };
    auto lds_fits = [&](uint32_t h) { return (uint64_t)stack_of(h) * 256u + c->extraLds + 15u * 256u <= 64u * 1024u; };
    std::vector<uint32_t> levelOff{0u, 1u};
    uint32_t cur = 0, levels = 0;
    for (uint32_t d = 0;; d++) {
        const uint32_t m = levelOff[d + 1u] - levelOff[d];
        if ((r = grow_scratch(c, B, &B.buf[kBins], &B.cap[kBins], (size_t)m * crt::kBvhNodeBinWords * 4u))) return r;
        HIPCK(c, crt_launch_bvh_level(d_positions, (const float*)B.buf[kCen], idx[cur], owner[cur], n, nodes + levelOff[d], keys + 6u * (size_t)levelOff[d], m, (uint32_t*)B.buf[kBins],
                                      (uint32_t*)B.buf[kLeft], (uint32_t*)B.buf[kSplit], (unsigned long long*)B.buf[kChunks], B.dState, d == 0u, B.blocks, st));
        double ms = 0;
        if ((r = read_back(c, st, B.back, B.hState, B.dState, sizeof(crt::BvhBuildState), &ms))) return r;
        B.waits++; B.waitMs += ms; levels = d + 1u;
        if (d == 0u && B.hState->nonFinite) return c->fail(CRT_ERR_INVALID, "%s: a position component is not finite", me);
        const uint64_t splits = B.hState->splits;
        if (splits > m || (uint64_t)levelOff[d + 1u] + 2u * splits > 2u * (uint64_t)n - 1u)
            return c->fail(CRT_ERR_DEVICE, "%s: the level kernels reported %llu split nodes of %u at depth %u", me, (unsigned long long)splits, m, d);
        if (splits && !lds_fits(d + 1u))
            return c->fail(CRT_ERR_UNSUPPORTED, "%s: the tree is taller than %u, its traversal stack (+TLAS %u) exceeds the 64 KiB of LDS per wave", me, d, tlasPart);
        const uint32_t nextM = (uint32_t)(2u * splits);
        HIPCK(c, crt_launch_bvh_split(nodes + levelOff[d], m, (const uint32_t*)B.buf[kSplit], owner[cur], idx[cur], (const uint32_t*)B.buf[kLeft], n, nodes + levelOff[d + 1u],
                                      keys + 6u * (size_t)levelOff[d + 1u], nextM, idx[cur ^ 1u], owner[cur ^ 1u], (uint32_t*)B.buf[kRemain], B.blocks, st));
        cur ^= 1u;
        if (!splits) break;
        levelOff.push_back(levelOff[d + 1u] + nextM);
    }
    B.levels = levels;
    const uint32_t height = levels - 1u, nodesUsed = levelOff.back(), np = nodesUsed / 2u, oldNp = f.nodesUsed[bvh] / 2u;
    // ---- the new buffer's sections, as crt_upload_scene lays them out ----
    uint64_t oldPairs = 0; for (uint32_t b = 0; b < N; b++) oldPairs += f.nodesUsed[b] / 2u;
    const uint64_t nPairs = oldPairs - oldNp + np, nTris = f.triBase[N - 1u] + f.triCount[N - 1u];
    const bool tlas = f.kind == CRT_SCENE_TLAS;
    const uint64_t leafOffB = nPairs ? nPairs * 64 : 64, tlasOffB = (leafOffB + (nTris + 1) * 48 + 63) & ~63ull, tlasBytes = tlas ? (uint64_t)f.tlasNodeCount * 32 : 0;
    const uint64_t tlasPairOffB = (tlasOffB + tlasBytes + 63) & ~63ull, instOffB = (tlasPairOffB + tlasBytes + 127) & ~127ull, instBytes = tlas ? (uint64_t)N * 128 : 0;
    const uint64_t shadeOffB = (instOffB + instBytes + 63) & ~63ull, total = shadeOffB + nTris * 64;
    if (total >= crt::kMaxGeomBytes) return c->fail(CRT_ERR_UNSUPPORTED, "%s: scene geometry needs %llu bytes; this build addresses 4 GiB", me, (unsigned long long)total);
    const uint32_t bits = c->hScene.poolRefBits;                           // pairs <= triangles - 1: the triangle count decided the width at upload, a rebuild cannot change it
    if ((bits == 16u && nPairs > crt::kRef16MaxIndex) || (bits == 32u && nPairs > crt::kRefWideMaxIndex)) return c->fail(CRT_ERR_DEVICE, "%s: %llu node pairs do not fit the scene's %u-bit pool references", me, (unsigned long long)nPairs, bits);
    const crt::PoolRefForm PR = crt::pool_ref_form(bits);
    char* fresh = nullptr;
    { const hipError_t e = hipMalloc((void**)&fresh, (size_t)total); if (e != hipSuccess) { (void)hipGetLastError(); return c->fail(CRT_ERR_DEVICE, "%s: hipMalloc(%llu): %s", me, (unsigned long long)total, hipGetErrorString(e)); } }
    std::vector<char> mirror;
    auto undo = [&](int rc) { (void)hipStreamSynchronize(st); (void)hipFree(fresh); return rc; };
#define BVHCK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return undo(c->hip(e_, #call)); } while (0)
    const char* old = c->hScene.geom;
    const uint64_t pb = f.pairBase[bvh], tb = f.triBase[bvh];
    BVHCK(hipMemsetAsync(fresh, 0, (size_t)shadeOffB, st));                 // the padding between the sections, and the 64 bytes of a scene without pairs
    const crt::BvhFlatten F{(uint32_t)pb, np, (uint32_t)tb, (uint32_t)leafOffB, PR.interior, PR.indexMask};
    BVHCK(crt_launch_bvh_flatten(nodes, levelOff.data(), levels, d_positions, idx[cur], (const uint32_t*)B.buf[kRemain], (const int32_t*)B.buf[kObj], n, &F, fresh, B.blocks, st));
    auto copy = [&](uint64_t to, uint64_t from, uint64_t bytes) { return bytes ? hipMemcpyAsync(fresh + to, old + from, (size_t)bytes, hipMemcpyDeviceToDevice, st) : hipSuccess; };
    BVHCK(copy(leafOffB, f.leafOff, tb * 48));                             // the other BVHs' leaf triangles and the pad record
    BVHCK(copy(leafOffB + (tb + n) * 48, f.leafOff + (tb + n) * 48, (nTris + 1 - tb - n) * 48));
    BVHCK(copy(tlasOffB, f.tlasOff, tlasBytes)); BVHCK(copy(tlasPairOffB, f.tlasPairOff, tlasBytes)); BVHCK(copy(instOffB, f.instOff, instBytes)); BVHCK(copy(shadeOffB, f.shadeOff, nTris * 64));
    const crt::BvhRelocate RL{(uint32_t)oldPairs, (uint32_t)pb, oldNp, (int32_t)np - (int32_t)oldNp, (int32_t)(((int64_t)leafOffB - (int64_t)f.leafOff) / 16), PR.interior, PR.indexMask};
    const bool rootSplits = levels > 1u;
    const uint32_t newRoot = rootSplits ? (crt::kRefInterior | (uint32_t)((pb * 64) >> 4)) : (uint32_t)((leafOffB + tb * 48) >> 4);
    const uint32_t newRoot16 = rootSplits ? (PR.interior | ((uint32_t)pb & PR.indexMask)) : ((uint32_t)(tb + 1) & PR.indexMask);
    BVHCK(crt_launch_bvh_relocate(old, fresh, &RL, (uint32_t)instOffB, tlas ? N : 0u, bvh, newRoot, newRoot16, B.blocks, st));
    if (g_hooks) { BVHCK(hipEventRecord(B.t1, st)); B.timed = true; }
    // ---- the host mirror of everything in front of the shade records, read back from the new buffer (the last host wait; the shade records are the old mirror's) ----
    mirror.resize((size_t)total);
    {
        const auto t0 = std::chrono::steady_clock::now();                  // (the whole copy: into pageable memory the call itself blocks, not the wait behind it)
        if ((r = read_back(c, st, B.back, mirror.data(), fresh, (size_t)shadeOffB))) return undo(r);
        B.readBackMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    memcpy(mirror.data() + shadeOffB, f.geom.data() + f.shadeOff, (size_t)(nTris * 64));
    const float* box = B.hState->rootBox;
    // ---- commit.  Node 0's box on the device is rewritten in place (crt_update_transforms_device reads it), so that copy is a write of the protocol; the buffer is
    // replaced: launches enqueued earlier keep the old one, which is retired behind them ----
    if (c->dRootBox) {
        if ((r = begin_scene_write(c, st))) return undo(r);
        BVHCK(hipMemcpyAsync(c->dRootBox + 6 * (size_t)bvh, B.dState->rootBox, 24, hipMemcpyDeviceToDevice, st));
    }
    BVHCK(hipEventRecord(B.done, st));
    B.built = true;
    crt_ctx::Retired gone;
    if ((r = retire_behind_readers(c, st, B.done, gone))) return undo(r);
#undef BVHCK
    gone.ptrs.push_back(const_cast<char*>(old));
    for (void*& p : c->sceneAllocs) if (p == (void*)old) p = fresh;
    if (bvh < c->refitPlans.size() && c->refitPlans[bvh].built) {          // the plan of the old topology goes with the old buffer (a refit enqueued earlier may still read it)
        for (void* p : {c->refitPlans[bvh].dPlan, (void*)c->refitPlans[bvh].dLevelOff})
            if (p) { gone.ptrs.push_back(p); c->refitAllocs.erase(std::remove(c->refitAllocs.begin(), c->refitAllocs.end(), p), c->refitAllocs.end()); }
        c->refitPlans[bvh] = crt_ctx::RefitPlan{};
    }
    c->retired.push_back(std::move(gone));
    f.geom.swap(mirror);
    f.leafOff = leafOffB; f.tlasOff = tlasOffB; f.tlasPairOff = tlasPairOffB; f.instOff = instOffB; f.shadeOff = shadeOffB;
    f.nodesUsed[bvh] = nodesUsed; f.height[bvh] = height;
    { uint64_t p = 0; for (uint32_t b = 0; b < N; b++) { f.pairBase[b] = p; p += f.nodesUsed[b] / 2u; } }
    f.maxHeight = height > otherHeight ? height : otherHeight;
    memcpy(&f.rootBox[6 * (size_t)bvh], box, 24);
    crt::Scene& s = c->hScene;
    s.geom = fresh; s.leafOff = (uint32_t)leafOffB; s.tlasOff = (uint32_t)tlasOffB; s.tlasPairOff = (uint32_t)tlasPairOffB; s.instOff = (uint32_t)instOffB; s.shadeOff = (uint32_t)shadeOffB;
    s.bvhStack = f.maxHeight ? f.maxHeight : 1u; s.stackDepth = s.bvhStack + tlasPart;
    c->ldsBytes = s.stackDepth * 64u * 4u + c->extraLds; c->latSlots = 0;
    if (tlas) { float lo[3], hi[3]; memcpy(lo, c->meshLo, 12); memcpy(hi, c->meshHi, 12); set_root(c, CRT_SCENE_TLAS, lo, hi); }   // (the TLAS is the caller's next step, as after BLASBVH::Build)
    else { s.rootRef = newRoot; s.rootRef16 = newRoot16; set_root(c, CRT_SCENE_FILE, box, box + 3); }
    for (crt_ctx::BlasSet& b : c->blasSet) b.stale(bvh);                   // as crt_refit_device: the KD-tree / grid of this BLAS are of the old vertices
    drop_blas_sets(c);
    if (rootBox) memcpy(rootBox, box, 24);
    return CRT_OK;
}

// one BVH in the reference's form again, from the live geometry buffer: node 0 from its kept box and the root reference; nodes 2k + 1 and 2k + 2 are pair k's
// children; a leaf slot's triangle is shadeIdx - shadeBase
int crt_get_bvh(crt_ctx* c, uint32_t bvh, uint32_t* nodesUsed, uint32_t* maxDepth, uint32_t* height, crt_bvh_node* nodes, uint32_t* triangleIndices)
{
    const char* const me = "crt_get_bvh";
    if (!c) return CRT_ERR_INVALID;
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no BVH", me);
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", me);
    const crt_ctx::Flat& f = c->flat;
    if (bvh >= f.triCount.size()) return c->fail(CRT_ERR_INVALID, "%s: BVH %u of a scene with %zu", me, bvh, f.triCount.size());
    const uint32_t used = f.nodesUsed[bvh], np = used / 2u, nt = f.triCount[bvh], h = f.height[bvh];
    if (nodesUsed) *nodesUsed = used;
    if (height) *height = h;
    if (maxDepth) *maxDepth = h ? h - 1u : 0u;                             // the deepest node that split is the deepest leaf's parent
    if (!nodes && !triangleIndices) return CRT_OK;
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->sceneReady) HIPCK(c, hipEventSynchronize(c->sceneReady));       // a refit, rebuild or update still running
    std::vector<crt::NodePair> pairs(np); std::vector<crt::LeafTri> leaf(nt);
    if (np) HIPCK(c, hipMemcpy(pairs.data(), c->hScene.geom + f.pairBase[bvh] * 64, (size_t)np * 64u, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(leaf.data(), c->hScene.geom + f.leafOff + f.triBase[bvh] * 48, (size_t)nt * 48u, hipMemcpyDeviceToHost));
    if (triangleIndices) for (uint32_t j = 0; j < nt; j++) triangleIndices[j] = leaf[j].shadeIdx - (uint32_t)f.triBase[bvh];
    if (!nodes) return CRT_OK;
    bool bad = false;
    auto fill = [&](crt_bvh_node& o, const float* lo, const float* hi, uint32_t ref) {
        memcpy(o.aabbMin, lo, 12); memcpy(o.aabbMax, hi, 12);
        const uint64_t off = (uint64_t)(ref & crt::kRefOffsetMask) << 4;
        if (ref & crt::kRefInterior) { const uint64_t k = off / 64u - f.pairBase[bvh]; if (k >= np) bad = true; o.leftFirst = (uint32_t)(2u * k + 1u); o.triCount = 0u; }
        else { const uint64_t j = (off - f.leafOff) / 48u - f.triBase[bvh]; if (j >= nt) { bad = true; return; } o.leftFirst = (uint32_t)j; o.triCount = leaf[j].remain; }
    };
    const uint32_t rootRef = f.kind == CRT_SCENE_TLAS ? reinterpret_cast<const crt::Instance*>(f.geom.data() + f.instOff)[bvh].rootRef : c->hScene.rootRef;
    fill(nodes[0], &f.rootBox[6 * (size_t)bvh], &f.rootBox[6 * (size_t)bvh + 3], rootRef);
    for (uint32_t k = 0; k < np; k++) for (int i = 0; i < 2; i++) fill(nodes[2u * k + 1u + i], pairs[k].c[i].lo, pairs[k].c[i].hi, pairs[k].c[i].ref);
    if (bad) return c->fail(CRT_ERR_DEVICE, "%s: the references of BVH %u do not form its tree", me, bvh);
    return CRT_OK;
}

// tests: the closed form of the partition loop as bvh_scatter_kernel applies it (bvh_partition_dest, build_common.h: the same lines, compiled for the host) over one
// segment of n slots; left[p] != 0: slot p's element goes left.  out[dest] = p; returns leftCount, or -1 where two slots map to one place or a place lies outside
extern "C" int crt_debug_bvh_partition(const uint8_t* left, uint32_t n, uint32_t* out)
{
    if (!left || !out || n == 0 || n > (1u << 20)) return -1;
    std::vector<uint32_t> S((size_t)n + 1u, 0u);
    for (uint32_t p = 0; p < n; p++) { S[p + 1u] = S[p] + (left[p] ? 1u : 0u); out[p] = 0xffffffffu; }
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t d = crt::bvh_partition_dest(S.data(), 0u, n, S[n], p);
        if (d >= n || out[d] != 0xffffffffu) return -1;
        out[d] = p;
    }
    return (int)S[n];
}

// tests: the live geometry buffer (every section: pairs, leaf triangles, TLAS nodes and pairs, instances, shade records) and the words of the Scene block that
// describe it — what a device rebuild must leave exactly as a fresh upload does.  words[24]: leafOff, tlasOff, tlasPairOff, instOff, shadeOff, rootRef, rootRef16,
// rootIsPair, stackDepth, bvhStack, poolRefBits, ldsBytes, then the 12 box floats of rootPair (lo / hi of both children) as bits.  dst == NULL: *bytes alone.
extern "C" int crt_debug_geometry(crt_ctx* c, uint32_t words[24], unsigned long long* bytes, void* dst)
{
    if (!c || !bytes) return CRT_ERR_INVALID;
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_debug_geometry before crt_upload_scene");
    const crt::Scene& s = c->hScene;
    *bytes = c->flat.geom.size();
    if (words) {
        const uint32_t w[12] = {s.leafOff, s.tlasOff, s.tlasPairOff, s.instOff, s.shadeOff, s.rootRef, s.rootRef16, s.rootIsPair, s.stackDepth, s.bvhStack, s.poolRefBits, c->ldsBytes};
        memcpy(words, w, sizeof(w));
        for (int k = 0; k < 2; k++) { memcpy(words + 12 + 6 * k, s.rootPair + 8 * k, 12); memcpy(words + 15 + 6 * k, s.rootPair + 8 * k + 4, 12); }
    }
    if (!dst) return CRT_OK;
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->sceneReady) HIPCK(c, hipEventSynchronize(c->sceneReady));
    HIPCK(c, hipMemcpy(dst, s.geom, c->flat.geom.size(), hipMemcpyDeviceToHost));
    return CRT_OK;
}

// tools/bvh_device_cost.py: the last crt_build_bvh_device's duration on its stream (HIP events, first launch to the last kernel; it includes the host round trips in
// between), the number of its per-level host waits and their wall time together, its levels, and the wall time of the mirror's read-back (debug hooks only)
extern "C" int crt_debug_bvh_build_ms(crt_ctx* c, float* streamMs, double* waitMs, uint32_t* waits, uint32_t* levels, double* readBackMs)
{
    if (!c || !streamMs || !waitMs || !waits || !levels || !readBackMs) return CRT_ERR_INVALID;
    const crt_ctx::BvhBuild& B = c->bvhBuild;
    if (!B.timed) return c->fail(CRT_ERR_STATE, "crt_debug_bvh_build_ms: no timed crt_build_bvh_device (debug hooks off?)");
    HIPCK(c, hipEventSynchronize(B.t1));
    HIPCK(c, hipEventElapsedTime(streamMs, B.t0, B.t1));
    *waitMs = B.waitMs; *waits = B.waits; *levels = B.levels; *readBackMs = B.readBackMs;
    return CRT_OK;
}

// tests: what crt_set_render_accel last selected, after the calls that reset it (an upload of the kind, a refit that drops a set, a grid rebuild that marks the KD-tree absent)
extern "C" int crt_debug_render_accel(crt_ctx* c) { return c ? c->renderAccel : CRT_ERR_INVALID; }

// tools/grid_device_cost.py: the last crt_build_grid_device's duration on its stream (HIP events, first launch to last; it includes the two host round trips in
// between) and the wall time of its two host waits (debug hooks only)
extern "C" int crt_debug_grid_build_ms(crt_ctx* c, float* streamMs, double waitMs[2])
{
    if (!c || !streamMs || !waitMs) return CRT_ERR_INVALID;
    const crt_ctx::GridBuild& G = c->gridBuild;
    if (!G.timed) return c->fail(CRT_ERR_STATE, "crt_debug_grid_build_ms: no timed crt_build_grid_device (debug hooks off?)");
    HIPCK(c, hipEventSynchronize(G.t1));
    HIPCK(c, hipEventElapsedTime(streamMs, G.t0, G.t1));
    waitMs[0] = G.waitMs[0]; waitMs[1] = G.waitMs[1];
    return CRT_OK;
}

// the host front's read of a caller's device buffer (host_abi.cpp, which includes no HIP header): behind everything `stream` holds, synchronous
extern "C" int crt_internal_read_device(crt_ctx* c, void* dst, const void* d_src, size_t bytes, void* stream)
{
    if (!c || !dst) return CRT_ERR_INVALID;
    int r; hipStream_t st = nullptr;
    if ((r = device_entry(c, "crt_internal_read_device", {{d_src, bytes}}, stream, &st))) return r;
    HIPCK(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st));
    HIPCK(c, hipStreamSynchronize(st));
    return CRT_OK;
}

// tools/tlas_device_cost.py: the duration of the last crt_update_transforms_device's kernel (HIP events on its stream; debug hooks only)
extern "C" int crt_debug_tlas_build_ms(crt_ctx* c, float* ms)
{
    if (!c || !ms) return CRT_ERR_INVALID;
    if (!c->tlasBuild.timed) return c->fail(CRT_ERR_STATE, "crt_debug_tlas_build_ms: no timed crt_update_transforms_device (debug hooks off?)");
    HIPCK(c, hipEventSynchronize(c->tlasBuild.t1));
    HIPCK(c, hipEventElapsedTime(ms, c->tlasBuild.t0, c->tlasBuild.t1));
    return CRT_OK;
}

int crt_is_occluded(crt_ctx* c, int accel, const crt_shadow_ray* rays, int32_t* occluded, size_t n)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = query_check(c, accel, true, n, "crt_is_occluded"))) return r;
    if (n == 0) return CRT_OK;
    if (!rays || !occluded) return c->fail(CRT_ERR_INVALID, "crt_is_occluded: NULL buffer");
    return query_host(c, true, accel, rays, occluded, n);
}

// ---- shading queries: GetHitInfo + GetAlbedo, GetSkyColor, GetLightPos / GetLightColor (crt_abi.h "scene queries") ----
// query_check's checks for them (the scene's own records: accel 0); the PrimitiveScene has a sky (black) and no hit info
static int shade_check(crt_ctx* c, bool hitInfo, size_t n, const char* what)
{
    if (hitInfo && c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: GetHitInfo of the PrimitiveScene is not served (crt_abi.h)", what);
    return query_check(c, 0, false, n, what);
}

// hit_record_ok's bounds for the uploaded scene
static uint32_t file_tri_count(const crt_ctx* c) { return c->flat.kind == CRT_SCENE_FILE ? c->flat.triCount[0] : 0u; }

int crt_get_hit_info(crt_ctx* c, const crt_ray* rays, const crt_hit* hits, crt_hit_info* out, size_t n)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = shade_check(c, true, n, "crt_get_hit_info"))) return r;
    if (n == 0) return CRT_OK;
    if (!rays || !hits || !out) return c->fail(CRT_ERR_INVALID, "crt_get_hit_info: NULL buffer");
    // objIdx / triIdx index device memory: every record is checked here, before anything is copied or launched (the kernel applies the same predicate per lane)
    const crt_ctx::Flat& f = c->flat;
    for (size_t i = 0; i < n; i++)
        if (!crt::hit_record_ok(hits[i].objIdx, hits[i].triIdx, f.objects, [&](uint32_t k) { return f.triCount[f.kind == CRT_SCENE_TLAS ? k : 0]; }))
            return c->fail(CRT_ERR_INVALID, "crt_get_hit_info: record %zu names objIdx %d, triIdx %d; the scene has objects -1 .. %u and that object's BVH fewer triangles", i, hits[i].objIdx, hits[i].triIdx, f.objects + 1);
    HIPCK(c, hipSetDevice(c->cfg.device));
    if ((r = stage(c, n * (sizeof(crt_hit_info) + sizeof(crt_ray) + sizeof(crt_hit))))) return r;
    char* dOut = c->dStage; char* dRays = dOut + n * sizeof(crt_hit_info); char* dHits = dRays + n * sizeof(crt_ray);
    HIPCK(c, hipMemcpyAsync(dRays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dHits, hits, n * sizeof(crt_hit), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, crt_launch_hit_info(&c->hScene, dRays, dHits, dOut, (uint32_t)n, f.objects, file_tri_count(c), c->stream));
    HIPCK(c, hipMemcpyAsync(out, dOut, n * sizeof(crt_hit_info), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_get_hit_info_device(crt_ctx* c, const crt_ray* d_rays, const crt_hit* d_hits, crt_hit_info* d_out, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_get_hit_info_device";
    int r;
    if ((r = shade_check(c, true, n, what))) return r;
    if (n == 0) return CRT_OK;
    HIPCK(c, hipSetDevice(c->cfg.device));
    if ((r = check_device_buffer(c, d_rays, n * sizeof(crt_ray), what)) || (r = check_device_buffer(c, d_hits, n * sizeof(crt_hit), what)) ||
        (r = check_device_buffer(c, d_out, n * sizeof(crt_hit_info), what))) return r;
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return c->fail(CRT_ERR_INVALID, "%s: the output buffer %p is not 16-byte aligned", what, (void*)d_out);
    hipStream_t st = nullptr; int k = 0;                                    // (device_entry's steps by hand: the refusal above comes before the stream's)
    if ((r = caller_stream(c, stream, what, &st)) || (r = wait_scene(c, st)) || (r = take_query_slot(c, &k))) return r;       // the slot's cursor word is unused: a record per lane, nothing to draw
    HIPCK(c, crt_launch_hit_info(&c->hScene, d_rays, d_hits, d_out, (uint32_t)n, c->flat.objects, file_tri_count(c), st));
    return end_device_query(c, k, st);
}

int crt_get_sky_color(crt_ctx* c, const crt_ray* rays, float* rgb, size_t n)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = shade_check(c, false, n, "crt_get_sky_color"))) return r;
    if (n == 0) return CRT_OK;
    if (!rays || !rgb) return c->fail(CRT_ERR_INVALID, "crt_get_sky_color: NULL buffer");
    if (c->havePrim) { memset(rgb, 0, n * 12); return CRT_OK; }                // PrimitiveScene::GetSkyColor
    HIPCK(c, hipSetDevice(c->cfg.device));
    if ((r = stage(c, n * (12 + sizeof(crt_ray))))) return r;
    float* dOut = reinterpret_cast<float*>(c->dStage); char* dRays = c->dStage + n * 12;
    HIPCK(c, hipMemcpyAsync(dRays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, crt_launch_sky_color(&c->hScene, dRays, dOut, (uint32_t)n, c->stream));
    HIPCK(c, hipMemcpyAsync(rgb, dOut, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_get_sky_color_device(crt_ctx* c, const crt_ray* d_rays, float* d_rgb, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_get_sky_color_device";
    int r;
    if ((r = shade_check(c, false, n, what))) return r;
    if (n == 0) return CRT_OK;
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_rays, n * sizeof(crt_ray)}, {d_rgb, n * 12}}, stream, &st)) || (r = wait_scene(c, st)) || (r = take_query_slot(c, &k))) return r;
    if (c->havePrim) HIPCK(c, hipMemsetAsync(d_rgb, 0, n * 12, st));          // PrimitiveScene::GetSkyColor
    else HIPCK(c, crt_launch_sky_color(&c->hScene, d_rays, d_rgb, (uint32_t)n, st));
    return end_device_query(c, k, st);
}

// ---- crt_sample / crt_sample_device: Renderer::Sample(ray, seed, 0) per ray of a buffer (device/sample_query.h) ----
// query_check's checks + the world's LDS columns (traversal stack + 15 throughput factors per lane, four wavefronts per workgroup), as crt_set_render_accel refuses them
static int sample_check(crt_ctx* c, int accel, size_t n, const char* what)
{
    int r;
    if ((r = query_check(c, accel, false, n, what))) return r;
    const uint32_t words = sample_stack_words(c, accel);
    if (!sample_lds_fits(words)) return c->fail(CRT_ERR_UNSUPPORTED, "%s: a traversal stack of %u dwords per lane exceeds the kernel's LDS", what, words);
    return 0;
}

static hipError_t launch_sample(crt_ctx* c, int accel, const void* rays, uint32_t* seeds, float* rgb, uint32_t n, uint32_t* cursor, uint32_t* residentLanes, hipStream_t st)
{
    if (c->havePrim) return crt_launch_sample_query_prim(&c->hScene, &c->prim, rays, seeds, rgb, n, c->dCounters, cursor, residentLanes, st);
    return crt_launch_sample_query(accel, &c->hScene, &c->alt, accel ? &c->blasAlt[accel - 1] : nullptr, rays, seeds, rgb, n, c->dCounters, cursor, residentLanes, st);
}

int crt_sample(crt_ctx* c, int accel, const crt_ray* rays, uint32_t* seeds, float* rgb, size_t n)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = sample_check(c, accel, n, "crt_sample"))) return r;
    if (n == 0) return CRT_OK;
    if (!rays || !seeds || !rgb) return c->fail(CRT_ERR_INVALID, "crt_sample: NULL buffer");
    HIPCK(c, hipSetDevice(c->cfg.device));
    if ((r = stage(c, n * (12 + sizeof(crt_ray) + 4)))) return r;
    float* dRgb = reinterpret_cast<float*>(c->dStage); char* dRays = c->dStage + n * 12; uint32_t* dSeeds = reinterpret_cast<uint32_t*>(dRays + n * sizeof(crt_ray));
    HIPCK(c, hipMemcpyAsync(dRays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dSeeds, seeds, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, launch_sample(c, accel, dRays, dSeeds, dRgb, (uint32_t)n, c->dQueryCursor, nullptr, c->stream));
    HIPCK(c, hipMemcpyAsync(rgb, dRgb, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipMemcpyAsync(seeds, dSeeds, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_sample_device(crt_ctx* c, int accel, const crt_ray* d_rays, uint32_t* d_seeds, float* d_rgb, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_sample_device";
    int r;
    if ((r = sample_check(c, accel, n, what))) return r;
    if (n == 0) return CRT_OK;
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_rays, n * sizeof(crt_ray)}, {d_seeds, n * 4}, {d_rgb, n * 12}}, stream, &st)) || (r = wait_scene(c, st)) || (r = take_query_slot(c, &k))) return r;
    if (accel != 0 && c->altReady) HIPCK(c, hipStreamWaitEvent(st, c->altReady, 0));     // the accelerators' copies ran on the null stream
    HIPCK(c, launch_sample(c, accel, d_rays, d_seeds, d_rgb, (uint32_t)n, c->dQuerySlots + 16 * k, nullptr, st));
    return end_device_query(c, k, st);
}

// ---- crt_render_views / crt_render_views_device: the frames of K cameras in one job of K x frames view-frames (device/render_views.h) ----
// the checks that need no buffer, in the order crt_abi.h lists the refusals
static int views_check(crt_ctx* c, uint32_t K, uint32_t frames, uint32_t passes, const char* what)
{
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "%s: passes must be 1..4 (the reference's UI range, renderer.cpp:178)", what);
    if ((uint64_t)K * frames > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 view-frames per call (%u views x %u frames)", what, K, frames);
    const uint32_t words = sample_stack_words(c, c->renderAccel);
    if (!sample_lds_fits(words)) return c->fail(CRT_ERR_UNSUPPORTED, "%s: a traversal stack of %u dwords per lane exceeds the kernel's LDS", what, words);
    return 0;
}

// windows of 64 view-frames one launch of the job renders: what cfg.maxFramesPerLaunch allows (as crt_render's launches), within 4 GiB of slab, within the scratch —
// which grows to that here (the one host wait: for the previous call, before its slab is freed) and never beyond half of the free HBM
static int views_scratch(crt_ctx* c, uint32_t totalWindows, size_t windowBytes, uint32_t* launchWindows)
{
    uint32_t wl = c->cfg.maxFramesPerLaunch >= 64 ? (uint32_t)c->cfg.maxFramesPerLaunch / 64u : 1u;
    const size_t byBytes = ((size_t)4 << 30) / windowBytes;
    if (wl > byBytes) wl = byBytes ? (uint32_t)byBytes : 1u;
    if (wl > totalWindows) wl = totalWindows;
    if ((size_t)wl * windowBytes > c->viewsSlabCap) {
        if (c->viewsPending) { HIPCK(c, hipEventSynchronize(c->viewsDone)); c->viewsPending = false; }
        if (c->dViewsSlab) { HIPCK(c, hipFree(c->dViewsSlab)); c->dViewsSlab = nullptr; c->viewsSlabCap = 0; }
        size_t freeB = 0, totalB = 0;
        HIPCK(c, hipMemGetInfo(&freeB, &totalB));
        if (freeB / 2 < windowBytes) return c->fail(CRT_ERR_DEVICE, "not enough free HBM for one 64-view-frame sample slab (%zu bytes needed, %zu free)", windowBytes, freeB);
        size_t want = (size_t)wl * windowBytes;
        if (want > freeB / 2) want = freeB / 2 / windowBytes * windowBytes;
        HIPCK(c, hipMalloc((void**)&c->dViewsSlab, want));
        c->viewsSlabCap = want;
    }
    const size_t fit = c->viewsSlabCap / windowBytes;
    *launchWindows = wl > fit ? (uint32_t)fit : wl;
    return 0;
}

// the job on `st`, after every check: launches of whole windows, each followed by its per-view sums into the caller's images
// (poses: crt_render_poses' job — the launches read every lane's TLAS and Instance records from its view's pose in that table, with jobScene's stack depth)
// (shapes: crt_render_shapes' job — ... every lane's refitted BVH, and a two-level scene's TLAS and Instance records, from its view's shape in that table)
// (sets: crt_render_shape_sets' job — ... the refitted BVHs of the set, the TLAS and the Instance records, from its view's shape in that table)
// (looks: crt_render_looks' job — the launches read every lane's light quad, floor material, sky and Material records from its view's look in that table)
static int views_run(crt_ctx* c, const float* dCams, uint32_t K, uint32_t sppFirst, uint32_t frames, uint32_t passes, float scale, float* dRgba, uint32_t* dPixels, hipStream_t st,
                     const crt::Scene* jobScene = nullptr, const crt::PoseTableDev* poses = nullptr, const crt::ShapeTableDev* shapes = nullptr, const crt::ShapeSetTableDev* sets = nullptr, const crt::LookTableDev* looks = nullptr)
{
    if (c->tileCount == 0) return 0;
    const uint32_t total = K * frames, totalWindows = (total + 63u) / 64u;
    uint32_t wl = 0; int r;
    if ((r = views_scratch(c, totalWindows, crt_slab_window_bytes(c->tileCount, passes), &wl))) return r;
    HIPCK(c, ensure_event(&c->viewsDone));
    if (c->viewsPending) HIPCK(c, hipStreamWaitEvent(st, c->viewsDone, 0));
    if ((r = wait_scene(c, st))) return r;
    if (c->renderAccel != 0 && c->altReady) HIPCK(c, hipStreamWaitEvent(st, c->altReady, 0));   // the accelerators' copies ran on the null stream
    for (uint32_t j0 = 0; j0 < total; j0 += wl * 64u) {
        const uint32_t nj = (total - j0 < wl * 64u) ? total - j0 : wl * 64u;
        if (looks) HIPCK(c, crt_launch_render_looks(jobScene, looks, dCams, c->dViewsSlab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        else if (sets) HIPCK(c, crt_launch_render_shape_sets(jobScene, sets, dCams, c->dViewsSlab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        else if (shapes) HIPCK(c, crt_launch_render_shapes(jobScene, shapes, dCams, c->dViewsSlab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        else if (poses) HIPCK(c, crt_launch_render_poses(jobScene, poses, dCams, c->dViewsSlab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        else if (c->havePrim) HIPCK(c, crt_launch_render_views_prim(&c->hScene, &c->prim, dCams, c->dViewsSlab, c->dCounters, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        else HIPCK(c, crt_launch_render_views(c->renderAccel, &c->hScene, &c->alt, c->renderAccel ? &c->blasAlt[c->renderAccel - 1] : nullptr, dCams, c->dViewsSlab, c->dCounters, c->tileFirst,
                                              c->tileStride, c->tileCount, (uint32_t)c->tilesX, sppFirst, frames, passes, j0, nj, st));
        HIPCK(c, crt_launch_views_accumulate(c->dViewsSlab, dRgba, dPixels, c->tileFirst, c->tileStride, c->tileCount, (uint32_t)c->tilesX, (uint32_t)c->cfg.width, (uint32_t)c->cfg.height, frames,
                                             passes, j0, nj, scale, st));
    }
    HIPCK(c, hipEventRecord(c->viewsDone, st));
    c->viewsPending = true;
    return 0;
}

// The host entries' staging (the context's, stage()): the K images, the K screens where wanted, then `extraBytes` for the entry's inputs (cameras, ...).
// The job writes the owned tiles' pixels only.  A context that owns every tile of an image whose width the tiling does not truncate writes whole rows — the first
// 16 * tilesY of every view — and only those travel back; any other context's staging starts from the caller's images, so every other pixel returns as it came.
struct ViewsStage { float* dRgba; uint32_t* dPix; char* extra; size_t px, rowsPx; };
static int views_stage_in(crt_ctx* c, uint32_t K, const float* out_rgba, const uint32_t* out_pixels, size_t extraBytes, ViewsStage* S)
{
    const size_t W = (size_t)c->cfg.width, px = W * c->cfg.height;
    const size_t pixOff = K * px * 16, extraOff = pixOff + (out_pixels ? K * px * 4 : 0);
    int r;
    if ((r = stage(c, extraOff + extraBytes))) return r;
    S->dRgba = reinterpret_cast<float*>(c->dStage); S->dPix = out_pixels ? reinterpret_cast<uint32_t*>(c->dStage + pixOff) : nullptr; S->extra = c->dStage + extraOff;
    const bool wholeRows = c->tileFirst == 0 && c->tileStride == 1 && c->tileCount == (uint32_t)(c->tilesX * c->tilesY) && (size_t)c->tilesX * 16u == W;
    S->px = px; S->rowsPx = wholeRows ? W * 16u * (size_t)c->tilesY : px;
    if (!wholeRows) {
        HIPCK(c, hipMemcpyAsync(S->dRgba, out_rgba, K * px * 16, hipMemcpyHostToDevice, c->stream));
        if (S->dPix) HIPCK(c, hipMemcpyAsync(S->dPix, out_pixels, K * px * 4, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}
// ... and the way back, behind the job on the context's stream; the call synchronises
static int views_stage_out(crt_ctx* c, uint32_t K, float* out_rgba, uint32_t* out_pixels, const ViewsStage& S)
{
    const size_t px = S.px;
    if (S.rowsPx == px) {
        HIPCK(c, hipMemcpyAsync(out_rgba, S.dRgba, K * px * 16, hipMemcpyDeviceToHost, c->stream));
        if (S.dPix) HIPCK(c, hipMemcpyAsync(out_pixels, S.dPix, K * px * 4, hipMemcpyDeviceToHost, c->stream));
    } else for (uint32_t k = 0; k < K; k++) {
        HIPCK(c, hipMemcpyAsync(out_rgba + k * px * 4, S.dRgba + k * px * 4, S.rowsPx * 16, hipMemcpyDeviceToHost, c->stream));
        if (S.dPix) HIPCK(c, hipMemcpyAsync(out_pixels + k * px, S.dPix + k * px, S.rowsPx * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->viewsPending = false;
    return CRT_OK;
}

int crt_render_views_device(crt_ctx* c, const float* d_cams, uint32_t K, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba, uint32_t* d_out_pixels, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_views_device";
    int r;
    if ((r = views_check(c, K, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    if (reinterpret_cast<uintptr_t>(d_out_rgba) & 15u) return c->fail(CRT_ERR_INVALID, "%s: d_out_rgba %p is not 16-byte aligned", what, (void*)d_out_rgba);
    hipStream_t st = nullptr; int k = 0;
    if (d_out_pixels) r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_out_rgba, K * px * 16}, {d_out_pixels, K * px * 4}}, stream, &st);
    else r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_out_rgba, K * px * 16}}, stream, &st);
    if (r || (r = take_query_slot(c, &k))) return r;
    if ((r = views_run(c, d_cams, K, spp_first, frames, passes, scale, d_out_rgba, d_out_pixels, st))) return r;
    return end_device_query(c, k, st);
}

int crt_render_views(crt_ctx* c, const float* cams, uint32_t K, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* out_rgba, uint32_t* out_pixels)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = views_check(c, K, frames, passes, "crt_render_views"))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    if (!cams || !out_rgba) return c->fail(CRT_ERR_INVALID, "crt_render_views: NULL buffer");
    HIPCK(c, hipSetDevice(c->cfg.device));
    ViewsStage S;
    if ((r = views_stage_in(c, K, out_rgba, out_pixels, (size_t)K * 48, &S))) return r;
    float* dCams = reinterpret_cast<float*>(S.extra);
    HIPCK(c, hipMemcpyAsync(dCams, cams, (size_t)K * 48, hipMemcpyHostToDevice, c->stream));
    if ((r = views_run(c, dCams, K, spp_first, frames, passes, scale, S.dRgba, S.dPix, c->stream))) return r;
    return views_stage_out(c, K, out_rgba, out_pixels, S);
}

// the job table and the pinned copy of what the one host wait reads, each grown when the job needs more, and `st` behind the previous job's launches
static int job_table(crt_ctx* c, size_t tableBytes, size_t backBytes, hipStream_t st)
{
    // the table is read by the previous job's launches to their end: viewsDone, on that job's stream
    HIPCK(c, ensure_event(&c->viewsDone));
    HIPCK(c, ensure_event(&c->poseBack));
    if (tableBytes > c->poseTableCap) {
        if (c->viewsPending) { HIPCK(c, hipEventSynchronize(c->viewsDone)); c->viewsPending = false; }
        if (c->dPoseTable) { HIPCK(c, hipFree(c->dPoseTable)); c->dPoseTable = nullptr; c->poseTableCap = 0; }
        HIPCK(c, hipMalloc((void**)&c->dPoseTable, tableBytes));
        c->poseTableCap = tableBytes;
    }
    if (backBytes > c->poseBackCap) {                                       // (no copy into it is in flight: every call waits for its own)
        if (c->hPoseBack) { HIPCK(c, hipHostFree(c->hPoseBack)); c->hPoseBack = nullptr; c->poseBackCap = 0; }
        HIPCK(c, hipHostMalloc((void**)&c->hPoseBack, backBytes, hipHostMallocDefault));
        c->poseBackCap = backBytes;
    }
    if (c->viewsPending) HIPCK(c, hipStreamWaitEvent(st, c->viewsDone, 0));
    return 0;
}

// ---- crt_render_poses / crt_render_poses_device: the frames of K cameras over P job-local poses of a two-level scene's instances (device/render_poses.h) ----
// where a job's pose table keeps what (device/layout.h PoseJobHeader)
struct PoseLayout {
    size_t imageBytes, headBytes, tableBytes; uint32_t imagesOff, imageStride;
    PoseLayout(const crt_ctx::Flat& f, uint32_t P)
    {
        imageBytes = (size_t)(f.shadeOff - f.tlasOff);
        imageStride = (uint32_t)((imageBytes + 127u) & ~(size_t)127u);
        headBytes = sizeof(crt::PoseJobHeader) + (size_t)P * sizeof(crt::TlasBuildHeader);
        imagesOff = (uint32_t)((headBytes + 127u) & ~(size_t)127u);        // (poses_check refuses a table beyond 4 GiB before anything uses the 32-bit fields)
        tableBytes = ((headBytes + 127u) & ~(size_t)127u) + (size_t)P * imageStride;
    }
};

// the checks that need no buffer, in the order crt_abi.h lists the refusals
static int poses_check(crt_ctx* c, uint32_t K, uint32_t P, uint32_t blasCount, bool viewPose, uint32_t frames, uint32_t passes, const char* what)
{
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no instances", what);
    const crt_ctx::Flat& f = c->flat;
    if (f.kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_INVALID, "%s applies to two-level scenes (a FileScene bakes its transforms into the triangles)", what);
    const uint32_t N = (uint32_t)f.triCount.size();
    if (blasCount != N) return c->fail(CRT_ERR_INVALID, "%s: %u transforms per pose, the uploaded scene has %u BLAS", what, blasCount, N);
    if (f.tlasNodeCount != 2u * N) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the scene was uploaded with %u TLAS nodes, TLASBVH::Build makes %u", what, f.tlasNodeCount, 2u * N);
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "%s: passes must be 1..4 (the reference's UI range, renderer.cpp:178)", what);
    if ((uint64_t)K * frames > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 view-frames per call (%u views x %u frames)", what, K, frames);
    if (c->renderAccel != 0) return c->fail(CRT_ERR_UNSUPPORTED, "%s: poses of the KD-tree / grid BLAS sets are not supported (crt_set_render_accel(0) first)", what);
    if (K > 0 && P == 0) return c->fail(CRT_ERR_INVALID, "%s: %u views and no pose", what, K);
    if (!viewPose && P != K) return c->fail(CRT_ERR_INVALID, "%s: without view_pose view k renders pose k, so P (%u) must equal K (%u)", what, P, K);
    if (PoseLayout(f, P).tableBytes > crt::kMaxGeomBytes)
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: %u poses of %zu bytes each exceed the 4 GiB the kernel's 32-bit offsets address; split the job", what, P, PoseLayout(f, P).imageBytes);
    return 0;
}

// The job on `st`, after the checks that need no launch: the P builds in one launch, the read-back of their headers and of the view_pose flag (THE host wait),
// the checks of what came back, tlasOut, then crt_render_views' launches over the table.  dViewPose may be nullptr (view k renders pose k).
static int poses_run(crt_ctx* c, const float* dCams, uint32_t K, const float* dT, uint32_t P, const int32_t* dViewPose, uint32_t sppFirst, uint32_t frames, uint32_t passes, float scale,
                     float* dRgba, uint32_t* dPixels, crt_tlas_node* tlasOut, hipStream_t st, const char* what)
{
    const crt_ctx::Flat& f = c->flat;
    const uint32_t N = (uint32_t)f.triCount.size();
    const PoseLayout L(f, P);
    const size_t nodeBytes = (size_t)2u * N * sizeof(crt::TlasNode), backBytes = L.headBytes + (tlasOut ? (size_t)P * nodeBytes : 0);
    // The builds are readers, as crt_update_transforms_device's: the Instance records and the node-0 boxes as the last write left them.
    int r;
    if ((r = wait_scene(c, st))) return r;
    if ((r = job_table(c, L.tableBytes, backBytes, st))) return r;
    HIPCK(c, hipMemsetAsync(c->dPoseTable, 0xff, sizeof(uint32_t), st));    // PoseJobHeader::badView = kPoseNoBadView
    HIPCK(c, crt_launch_tlas_build_poses(c->hScene.geom, (uint32_t)f.instOff, dT, c->dRootBox, N, (uint32_t)(f.tlasPairOff - f.tlasOff), (uint32_t)(f.instOff - f.tlasOff), c->hScene.poolRefBits,
                                         c->dPoseTable, L.imagesOff, L.imageStride, P, dViewPose, K, st));
    if (tlasOut) HIPCK(c, hipMemcpy2DAsync(c->hPoseBack + L.headBytes, nodeBytes, c->dPoseTable + L.imagesOff, L.imageStride, nodeBytes, P, hipMemcpyDeviceToHost, st));
    // the one host wait: the launches' LDS stack is sized by the tallest pose's TLAS, and a job with a failed build or a view_pose entry out of range does not run
    if ((r = read_back(c, st, c->poseBack, c->hPoseBack, c->dPoseTable, L.headBytes))) return r;
    const crt::PoseJobHeader& job = *reinterpret_cast<const crt::PoseJobHeader*>(c->hPoseBack);
    const crt::TlasBuildHeader* heads = reinterpret_cast<const crt::TlasBuildHeader*>(c->hPoseBack + sizeof(crt::PoseJobHeader));
    if (job.badView != crt::kPoseNoBadView) return c->fail(CRT_ERR_INVALID, "%s: view_pose[%u] lies outside [0, %u)", what, job.badView, P);
    uint32_t tallest = 0, tallestPose = 0;
    for (uint32_t p = 0; p < P; p++) {
        const crt::TlasBuildHeader& h = heads[p];
        if (h.status == crt::kTlasBuildNoCandidate)
            return c->fail(CRT_ERR_INVALID, "%s: pose %u: FindBestMatch call %u found no partner while more than one node was open (a non-finite transform or box, or areas >= 1e30; the reference reads list[-1] there)", what, p, h.step);
        if (h.status != crt::kTlasBuildOk) return c->fail(CRT_ERR_INVALID, "%s: pose %u: the build had not ended after %u FindBestMatch calls", what, p, h.step);
        if (h.height > tallest) { tallest = h.height; tallestPose = p; }
    }
    crt::Scene job_scene = c->hScene;                                       // the launches' by-value Scene: the context's, with the job's stack depth.  c->hScene stays as it is
    job_scene.stackDepth = job_scene.bvhStack + tallest + 1;
    if ((r = check_tlas_height(c, tallest))) return r;
    if (!sample_lds_fits(job_scene.stackDepth))
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: pose %u: a TLAS of height %u makes the traversal stack %u dwords per lane, which exceeds the kernel's LDS", what, tallestPose, tallest, job_scene.stackDepth);
    const crt::PoseTableDev pt{c->dPoseTable, dViewPose, L.imagesOff, L.imageStride, (uint32_t)(f.instOff - f.tlasOff)};
    if ((r = views_run(c, dCams, K, sppFirst, frames, passes, scale, dRgba, dPixels, st, &job_scene, &pt))) return r;
    // tlasOut last, once nothing can refuse the job any more (the pinned copy is the call's own until it returns): a refused call writes nothing
    if (tlasOut)
        for (uint32_t p = 0; p < P; p++) unpack_tlas_nodes(reinterpret_cast<const crt::TlasNode*>(c->hPoseBack + L.headBytes + p * nodeBytes), 2u * N, tlasOut + (size_t)p * 2u * N);
    return 0;
}

int crt_render_poses_device(crt_ctx* c, const float* d_cams, uint32_t K, const float* d_T, uint32_t P, uint32_t blasCount, const int32_t* d_view_pose, uint32_t spp_first, uint32_t frames,
                            uint32_t passes, float scale, float* d_out_rgba, uint32_t* d_out_pixels, crt_tlas_node* tlas_out, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_poses_device";
    int r;
    if ((r = poses_check(c, K, P, blasCount, d_view_pose != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    if (reinterpret_cast<uintptr_t>(d_out_rgba) & 15u) return c->fail(CRT_ERR_INVALID, "%s: d_out_rgba %p is not 16-byte aligned", what, (void*)d_out_rgba);
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_T, (size_t)P * blasCount * 64}, {d_out_rgba, K * px * 16}}, stream, &st))) return r;
    if (d_out_pixels && (r = check_device_buffer(c, d_out_pixels, K * px * 4, what))) return r;
    if (d_view_pose && (r = check_device_buffer(c, d_view_pose, (size_t)K * 4, what))) return r;
    if ((r = take_query_slot(c, &k))) return r;
    if ((r = poses_run(c, d_cams, K, d_T, P, d_view_pose, spp_first, frames, passes, scale, d_out_rgba, d_out_pixels, tlas_out, st, what))) return r;
    return end_device_query(c, k, st);
}

int crt_render_poses(crt_ctx* c, const float* cams, uint32_t K, const float* T, uint32_t P, uint32_t blasCount, const int32_t* view_pose, uint32_t spp_first, uint32_t frames, uint32_t passes,
                     float scale, float* out_rgba, uint32_t* out_pixels, crt_tlas_node* tlas_out)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_poses";
    int r;
    if ((r = poses_check(c, K, P, blasCount, view_pose != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    if (!cams || !T || !out_rgba) return c->fail(CRT_ERR_INVALID, "%s: NULL buffer", what);
    if (view_pose)
        for (uint32_t k = 0; k < K; k++)
            if (view_pose[k] < 0 || (uint32_t)view_pose[k] >= P) return c->fail(CRT_ERR_INVALID, "%s: view_pose[%u] = %d lies outside [0, %u)", what, k, view_pose[k], P);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t camBytes = (size_t)K * 48, tBytes = (size_t)P * blasCount * 64;
    ViewsStage S;
    if ((r = views_stage_in(c, K, out_rgba, out_pixels, camBytes + tBytes + (view_pose ? (size_t)K * 4 : 0), &S))) return r;
    float* dCams = reinterpret_cast<float*>(S.extra); float* dT = reinterpret_cast<float*>(S.extra + camBytes);
    int32_t* dViewPose = view_pose ? reinterpret_cast<int32_t*>(S.extra + camBytes + tBytes) : nullptr;
    HIPCK(c, hipMemcpyAsync(dCams, cams, camBytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dT, T, tBytes, hipMemcpyHostToDevice, c->stream));
    if (dViewPose) HIPCK(c, hipMemcpyAsync(dViewPose, view_pose, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    if ((r = poses_run(c, dCams, K, dT, P, dViewPose, spp_first, frames, passes, scale, S.dRgba, S.dPix, tlas_out, c->stream, what))) return r;
    return views_stage_out(c, K, out_rgba, out_pixels, S);
}

// ---- crt_render_looks / crt_render_looks_device: the frames of K cameras over L job-local looks of the live scene (device/look_build.hip, render_looks.h) ----
// where a job's look table keeps what (device/layout.h LookJobHeader, LookDev)
struct LookLayout {
    size_t tableBytes; uint32_t looksOff, lookStride, recordWords;
    LookLayout(const crt_ctx::Flat& f, uint32_t L)
    {
        recordWords = crt_look_words(f.materialCount);
        lookStride = (uint32_t)((sizeof(crt::LookDev) + (size_t)(2u + f.materialCount) * sizeof(crt::Material) + 127u) & ~(size_t)127u);
        looksOff = 128u;                                                    // behind the LookJobHeader
        tableBytes = looksOff + (size_t)L * lookStride;
    }
};

// the checks that need no buffer, in the order crt_abi.h lists the refusals
static int looks_check(crt_ctx* c, uint32_t K, uint32_t L, bool viewLook, uint32_t frames, uint32_t passes, const char* what)
{
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene's materials are part of its code; it has no look", what);
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "%s: passes must be 1..4 (the reference's UI range, renderer.cpp:178)", what);
    if ((uint64_t)K * frames > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 view-frames per call (%u views x %u frames)", what, K, frames);
    if (c->renderAccel != 0) return c->fail(CRT_ERR_UNSUPPORTED, "%s: looks through the KD-tree / grid are not supported (crt_set_render_accel(0) first)", what);
    if (K > 0 && L == 0) return c->fail(CRT_ERR_INVALID, "%s: %u views and no look", what, K);
    if (!viewLook && L != K) return c->fail(CRT_ERR_INVALID, "%s: without view_look view k renders look k, so L (%u) must equal K (%u)", what, L, K);
    const LookLayout Y(c->flat, L);
    if (Y.tableBytes > crt::kMaxGeomBytes || (uint64_t)L * Y.recordWords > 0x3fffffffull)
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: %u looks of %u bytes each exceed the 4 GiB the kernel's 32-bit offsets address; split the job", what, L, Y.lookStride);
    if (!sample_lds_fits(c->hScene.stackDepth)) return c->fail(CRT_ERR_UNSUPPORTED, "%s: a traversal stack of %u dwords per lane exceeds the kernel's LDS", what, c->hScene.stackDepth);
    return 0;
}

// The job on `st`, after the checks that need no launch: the build launch, the read-back of its status header (THE host wait), the checks of what came back, then
// crt_render_views' launches over the table.  dViewLook may be nullptr (view k renders look k).
static int looks_run(crt_ctx* c, const float* dCams, uint32_t K, const void* dLooks, uint32_t L, const int32_t* dViewLook, uint32_t sppFirst, uint32_t frames, uint32_t passes, float scale,
                     float* dRgba, uint32_t* dPixels, hipStream_t st, const char* what)
{
    const crt_ctx::Flat& f = c->flat;
    const LookLayout Y(f, L);
    int r;
    if ((r = wait_scene(c, st))) return r;
    if ((r = job_table(c, Y.tableBytes, sizeof(crt::LookJobHeader), st))) return r;
    HIPCK(c, hipMemsetAsync(c->dPoseTable, 0xff, sizeof(crt::LookJobHeader), st));     // badView = kPoseNoBadView, badField = kLookNoBadField
    const crt::LookBuildDev b{static_cast<const uint32_t*>(dLooks), L, f.materialCount, c->dTex, (uint32_t)f.tex.size(), c->dPoseTable, Y.looksOff, Y.lookStride, dViewLook, K};
    HIPCK(c, crt_launch_look_build(&b, st));
    // the one host wait: a job with a texture index or a view_look entry out of range does not run
    if ((r = read_back(c, st, c->poseBack, c->hPoseBack, c->dPoseTable, sizeof(crt::LookJobHeader)))) return r;
    const crt::LookJobHeader& job = *reinterpret_cast<const crt::LookJobHeader*>(c->hPoseBack);
    if (job.badField != crt::kLookNoBadField) {
        const uint32_t look = (uint32_t)(job.badField >> 32), field = (uint32_t)job.badField;
        if (field == crt::kLookFieldFloor) return c->fail(CRT_ERR_INVALID, "%s: look %u: floorTexture lies outside [0, %zu)", what, look, f.tex.size());
        if (field == crt::kLookFieldSky) return c->fail(CRT_ERR_INVALID, "%s: look %u: skyTexture lies outside [0, %zu)", what, look, f.tex.size());
        return c->fail(CRT_ERR_INVALID, "%s: look %u: material %u: texture lies outside [-1, %zu)", what, look, field - crt::kLookFieldMaterial, f.tex.size());
    }
    if (job.badView != crt::kPoseNoBadView) return c->fail(CRT_ERR_INVALID, "%s: view_look[%u] lies outside [0, %u)", what, job.badView, L);
    const crt::LookTableDev lt{c->dPoseTable, dViewLook, Y.looksOff, Y.lookStride};
    return views_run(c, dCams, K, sppFirst, frames, passes, scale, dRgba, dPixels, st, &c->hScene, nullptr, nullptr, nullptr, &lt);
}

int crt_render_looks_device(crt_ctx* c, const float* d_cams, uint32_t K, const void* d_looks, uint32_t L, const int32_t* d_view_look, uint32_t spp_first, uint32_t frames, uint32_t passes,
                            float scale, float* d_out_rgba, uint32_t* d_out_pixels, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_looks_device";
    int r;
    if ((r = looks_check(c, K, L, d_view_look != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    if (reinterpret_cast<uintptr_t>(d_out_rgba) & 15u) return c->fail(CRT_ERR_INVALID, "%s: d_out_rgba %p is not 16-byte aligned", what, (void*)d_out_rgba);
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_looks, (size_t)L * LookLayout(c->flat, L).recordWords * 4}, {d_out_rgba, K * px * 16}}, stream, &st))) return r;
    if (d_out_pixels && (r = check_device_buffer(c, d_out_pixels, K * px * 4, what))) return r;
    if (d_view_look && (r = check_device_buffer(c, d_view_look, (size_t)K * 4, what))) return r;
    if ((r = take_query_slot(c, &k))) return r;
    if ((r = looks_run(c, d_cams, K, d_looks, L, d_view_look, spp_first, frames, passes, scale, d_out_rgba, d_out_pixels, st, what))) return r;
    return end_device_query(c, k, st);
}

int crt_render_looks(crt_ctx* c, const float* cams, uint32_t K, const void* looks, uint32_t L, const int32_t* view_look, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                     float* out_rgba, uint32_t* out_pixels)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_looks";
    int r;
    if ((r = looks_check(c, K, L, view_look != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    if (!cams || !looks || !out_rgba) return c->fail(CRT_ERR_INVALID, "%s: NULL buffer", what);
    const LookLayout Y(c->flat, L);
    for (uint32_t l = 0; l < L; l++) {                                      // the build launch's checks, on the host first: nothing is staged for a job that will not run
        char where[32]; snprintf(where, sizeof(where), "look %u: ", l);
        if ((r = check_look(c, static_cast<const uint32_t*>(looks) + (size_t)l * Y.recordWords, what, where))) return r;
    }
    if (view_look)
        for (uint32_t k = 0; k < K; k++)
            if (view_look[k] < 0 || (uint32_t)view_look[k] >= L) return c->fail(CRT_ERR_INVALID, "%s: view_look[%u] = %d lies outside [0, %u)", what, k, view_look[k], L);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t camBytes = (size_t)K * 48, lookBytes = (size_t)L * Y.recordWords * 4;
    ViewsStage S;
    if ((r = views_stage_in(c, K, out_rgba, out_pixels, camBytes + lookBytes + (view_look ? (size_t)K * 4 : 0), &S))) return r;
    float* dCams = reinterpret_cast<float*>(S.extra); void* dLooks = S.extra + camBytes;
    int32_t* dViewLook = view_look ? reinterpret_cast<int32_t*>(S.extra + camBytes + lookBytes) : nullptr;
    HIPCK(c, hipMemcpyAsync(dCams, cams, camBytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dLooks, looks, lookBytes, hipMemcpyHostToDevice, c->stream));
    if (dViewLook) HIPCK(c, hipMemcpyAsync(dViewLook, view_look, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    if ((r = looks_run(c, dCams, K, dLooks, L, dViewLook, spp_first, frames, passes, scale, S.dRgba, S.dPix, c->stream, what))) return r;
    return views_stage_out(c, K, out_rgba, out_pixels, S);
}

// ---- crt_render_shapes / crt_render_shapes_device: the frames of K cameras over S job-local shapes of one refitted BVH (device/shape_build.hip, render_shapes.h) ----
// where a job's shape table keeps what (device/layout.h ShapeJobHeader)
struct ShapeLayout {
    bool tlas; uint32_t N, rowFloats, pairCount, triCount;
    size_t headBytes, poseBytes, tableBytes; uint32_t headsOff, rowsOff, imagesOff, imageStride, leafRel, poseRel;
    ShapeLayout(const crt_ctx::Flat& f, uint32_t bvh, uint32_t S)
    {
        tlas = f.kind == CRT_SCENE_TLAS; N = (uint32_t)f.triCount.size();
        rowFloats = tlas ? 6u * N : 6u;
        pairCount = f.nodesUsed[bvh] / 2; triCount = f.triCount[bvh];
        headsOff = (uint32_t)sizeof(crt::ShapeJobHeader);
        headBytes = headsOff + (tlas ? (size_t)S * sizeof(crt::TlasBuildHeader) : 0);      // what the one host wait reads: the flag and the build headers
        const size_t rowsAt = headBytes, imagesAt = (rowsAt + (size_t)S * rowFloats * 4u + 127u) & ~(size_t)127u;
        const size_t leafAt = (size_t)(pairCount ? pairCount : 1u) * 64u, poseAt = (leafAt + (size_t)triCount * 48u + 127u) & ~(size_t)127u;
        poseBytes = tlas ? (size_t)(f.shadeOff - f.tlasOff) : 0;
        const size_t stride = (poseAt + poseBytes + 127u) & ~(size_t)127u;
        tableBytes = imagesAt + (size_t)S * stride + 64u;                   // (+ 64: a fetch of 64 bytes at the last record's last row stays inside)
        // shapes_check refuses a table beyond 4 GiB before anything uses the 32-bit fields
        rowsOff = (uint32_t)rowsAt; imagesOff = (uint32_t)imagesAt; imageStride = (uint32_t)stride; leafRel = (uint32_t)leafAt; poseRel = (uint32_t)poseAt;
    }
};

// the checks that need no buffer, in the order crt_abi.h lists the refusals
static int shapes_check(crt_ctx* c, uint32_t K, uint32_t bvh, uint32_t S, uint32_t triCount, bool haveT, uint32_t blasCount, bool viewShape, uint32_t frames, uint32_t passes, const char* what)
{
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no BVH to refit", what);
    const crt_ctx::Flat& f = c->flat;
    const uint32_t N = (uint32_t)f.triCount.size();
    if (bvh >= N) return c->fail(CRT_ERR_INVALID, "%s: BVH %u of a scene with %u", what, bvh, N);
    if (triCount != f.triCount[bvh]) return c->fail(CRT_ERR_INVALID, "%s: %u triangles per shape, the uploaded BVH %u has %u (Refit keeps the topology)", what, triCount, bvh, f.triCount[bvh]);
    if (f.kind != CRT_SCENE_TLAS) {
        if (haveT || blasCount != 0) return c->fail(CRT_ERR_INVALID, "%s: a FileScene has no instances (T must be NULL and blasCount 0)", what);
    } else {
        if (!haveT || blasCount != N) return c->fail(CRT_ERR_INVALID, "%s: %u transforms per shape%s, the uploaded scene has %u BLAS", what, blasCount, haveT ? "" : " (T is NULL)", N);
        if (f.tlasNodeCount != 2u * N) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the scene was uploaded with %u TLAS nodes, TLASBVH::Build makes %u", what, f.tlasNodeCount, 2u * N);
    }
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "%s: passes must be 1..4 (the reference's UI range, renderer.cpp:178)", what);
    if ((uint64_t)K * frames > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 view-frames per call (%u views x %u frames)", what, K, frames);
    if (c->renderAccel != 0) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the KD-tree / grid structures have no refit (crt_set_render_accel(0) first; crt_refit_device drops those sets too)", what);
    if (K > 0 && S == 0) return c->fail(CRT_ERR_INVALID, "%s: %u views and no shape", what, K);
    if (!viewShape && S != K) return c->fail(CRT_ERR_INVALID, "%s: without view_shape view k renders shape k, so S (%u) must equal K (%u)", what, S, K);
    const ShapeLayout L(f, bvh, S);
    if (L.tableBytes > crt::kMaxGeomBytes)
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: %u shapes of %u bytes each exceed the 4 GiB the kernel's 32-bit offsets address; split the job", what, S, L.imageStride);
    return 0;
}

// what the S TLAS builds of a shape job reported: a failed build refuses the job; the tallest TLAS sizes the launches' LDS stack (jobScene->stackDepth)
static int shape_tlas_heads(crt_ctx* c, const crt::TlasBuildHeader* heads, uint32_t S, crt::Scene* jobScene, const char* what)
{
    uint32_t tallest = 0, tallestShape = 0; int r;
    for (uint32_t s = 0; s < S; s++) {
        const crt::TlasBuildHeader& h = heads[s];
        if (h.status == crt::kTlasBuildNoCandidate)
            return c->fail(CRT_ERR_INVALID, "%s: shape %u: FindBestMatch call %u found no partner while more than one node was open (a non-finite transform, position or box, or areas >= 1e30; the reference reads list[-1] there)", what, s, h.step);
        if (h.status != crt::kTlasBuildOk) return c->fail(CRT_ERR_INVALID, "%s: shape %u: the build had not ended after %u FindBestMatch calls", what, s, h.step);
        if (h.height > tallest) { tallest = h.height; tallestShape = s; }
    }
    jobScene->stackDepth = jobScene->bvhStack + tallest + 1;
    if ((r = check_tlas_height(c, tallest))) return r;
    if (!sample_lds_fits(jobScene->stackDepth))
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: shape %u: a TLAS of height %u makes the traversal stack %u dwords per lane, which exceeds the kernel's LDS", what, tallestShape, tallest, jobScene->stackDepth);
    return 0;
}

// The job on `st`, after the checks that need no launch: the S shapes (leaf launch, box launch, for a two-level scene the S TLAS builds), the read-back of the
// view_shape flag and the build headers (THE host wait; with root_box_out / tlas_out the boxes / node sections too), the checks of what came back, then
// crt_render_views' launches over the table.  dViewShape may be nullptr (view k renders shape k); dT is nullptr for a FileScene.
static int shapes_run(crt_ctx* c, const float* dCams, uint32_t K, uint32_t bvh, const float* dPos, uint32_t S, const float* dT, const int32_t* dViewShape, uint32_t sppFirst, uint32_t frames,
                      uint32_t passes, float scale, float* dRgba, uint32_t* dPixels, float* rootBoxOut, crt_tlas_node* tlasOut, hipStream_t st, const char* what)
{
    const crt_ctx::Flat& f = c->flat;
    const ShapeLayout L(f, bvh, S);
    const uint32_t N = L.N;
    int r;
    if (c->refitPlans.size() != f.triCount.size()) c->refitPlans.assign(f.triCount.size(), crt_ctx::RefitPlan{});
    if (!c->refitPlans[bvh].built && (r = build_refit_plan(c, bvh))) return r;
    const crt_ctx::RefitPlan& P = c->refitPlans[bvh];
    const size_t nodeBytes = (size_t)2u * N * sizeof(crt::TlasNode);
    const size_t boxesAt = L.headBytes, nodesAt = boxesAt + (rootBoxOut ? (size_t)S * 24u : 0), backBytes = nodesAt + (tlasOut && L.tlas ? (size_t)S * nodeBytes : 0);
    // The builds are readers, as crt_render_poses': the live pairs, leaf records, Instance records and node-0 boxes as the last write left them.
    if ((r = wait_scene(c, st))) return r;
    if ((r = job_table(c, L.tableBytes, backBytes, st))) return r;
    char* table = c->dPoseTable;
    HIPCK(c, hipMemsetAsync(table, 0xff, sizeof(uint32_t), st));            // ShapeJobHeader::badView = kPoseNoBadView
    const crt::ShapeBuildDev sb{c->hScene.geom, (uint32_t)f.leafOff, (uint32_t)f.pairBase[bvh], L.pairCount, (uint32_t)f.triBase[bvh], L.triCount, dPos,
                                L.tlas ? c->dRootBox : nullptr, L.rowFloats, L.tlas ? bvh : 0u, table, L.rowsOff, L.imagesOff, L.imageStride, L.leafRel, S};
    HIPCK(c, crt_launch_shape_build(&sb, P.dPlan, P.dLevelOff, P.levels, P.rootCode, dViewShape, K, st));
    if (L.tlas)
        HIPCK(c, crt_launch_tlas_build_shapes(c->hScene.geom, (uint32_t)f.instOff, dT, reinterpret_cast<const float*>(table + L.rowsOff), N, (uint32_t)(f.tlasPairOff - f.tlasOff),
                                              (uint32_t)(f.instOff - f.tlasOff), c->hScene.poolRefBits, table, L.headsOff, L.imagesOff + L.poseRel, L.imageStride, S, st));
    if (rootBoxOut) HIPCK(c, hipMemcpy2DAsync(c->hPoseBack + boxesAt, 24, table + L.rowsOff + (size_t)sb.bvh * 24u, (size_t)L.rowFloats * 4u, 24, S, hipMemcpyDeviceToHost, st));
    if (tlasOut && L.tlas) HIPCK(c, hipMemcpy2DAsync(c->hPoseBack + nodesAt, nodeBytes, table + L.imagesOff + L.poseRel, L.imageStride, nodeBytes, S, hipMemcpyDeviceToHost, st));
    // the one host wait: a job with a view_shape entry out of range or a failed build does not run, and the launches' LDS stack is sized by the tallest shape's TLAS
    if ((r = read_back(c, st, c->poseBack, c->hPoseBack, table, L.headBytes))) return r;
    const crt::ShapeJobHeader& job = *reinterpret_cast<const crt::ShapeJobHeader*>(c->hPoseBack);
    if (job.badView != crt::kPoseNoBadView) return c->fail(CRT_ERR_INVALID, "%s: view_shape[%u] lies outside [0, %u)", what, job.badView, S);
    crt::Scene job_scene = c->hScene;                                       // the launches' by-value Scene: the context's, with the job's stack depth.  c->hScene stays as it is
    if (L.tlas) {
        if ((r = shape_tlas_heads(c, reinterpret_cast<const crt::TlasBuildHeader*>(c->hPoseBack + L.headsOff), S, &job_scene, what))) return r;
    } else if (!sample_lds_fits(job_scene.stackDepth))
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: a traversal stack of %u dwords per lane exceeds the kernel's LDS", what, job_scene.stackDepth);
    // node 0 of the refitted BVH as the image names it (shape_build.hip image_ref)
    const uint32_t rootRef = (P.rootCode & crt::kPlanInterior) ? (crt::kRefInterior | ((P.rootCode & ~crt::kPlanInterior) * 4u)) : ((L.leafRel + P.rootCode * 48u) >> 4);
    const crt::ShapeTableDev tb{table, dViewShape, L.imagesOff, L.imageStride, rootRef, bvh, L.poseRel, (uint32_t)(f.instOff - f.tlasOff)};
    if ((r = views_run(c, dCams, K, sppFirst, frames, passes, scale, dRgba, dPixels, st, &job_scene, nullptr, &tb))) return r;
    // the host outputs last, once nothing can refuse the job any more (the pinned copy is the call's own until it returns): a refused call writes nothing
    if (rootBoxOut) memcpy(rootBoxOut, c->hPoseBack + boxesAt, (size_t)S * 24u);
    if (tlasOut && L.tlas)
        for (uint32_t s = 0; s < S; s++) unpack_tlas_nodes(reinterpret_cast<const crt::TlasNode*>(c->hPoseBack + nodesAt + s * nodeBytes), 2u * N, tlasOut + (size_t)s * 2u * N);
    return 0;
}

int crt_render_shapes_device(crt_ctx* c, const float* d_cams, uint32_t K, uint32_t bvh, const float* d_positions, uint32_t S, uint32_t triCount, const float* d_T, uint32_t blasCount,
                             const int32_t* d_view_shape, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba, uint32_t* d_out_pixels, float* root_box_out,
                             crt_tlas_node* tlas_out, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_shapes_device";
    int r;
    if ((r = shapes_check(c, K, bvh, S, triCount, d_T != nullptr, blasCount, d_view_shape != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    if (reinterpret_cast<uintptr_t>(d_out_rgba) & 15u) return c->fail(CRT_ERR_INVALID, "%s: d_out_rgba %p is not 16-byte aligned", what, (void*)d_out_rgba);
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_positions, (size_t)S * triCount * 36}, {d_out_rgba, K * px * 16}}, stream, &st))) return r;
    if (d_T && (r = check_device_buffer(c, d_T, (size_t)S * blasCount * 64, what))) return r;
    if (d_out_pixels && (r = check_device_buffer(c, d_out_pixels, K * px * 4, what))) return r;
    if (d_view_shape && (r = check_device_buffer(c, d_view_shape, (size_t)K * 4, what))) return r;
    if ((r = take_query_slot(c, &k))) return r;
    if ((r = shapes_run(c, d_cams, K, bvh, d_positions, S, d_T, d_view_shape, spp_first, frames, passes, scale, d_out_rgba, d_out_pixels, root_box_out, tlas_out, st, what))) return r;
    return end_device_query(c, k, st);
}

int crt_render_shapes(crt_ctx* c, const float* cams, uint32_t K, uint32_t bvh, const float* positions, uint32_t S, uint32_t triCount, const float* T, uint32_t blasCount,
                      const int32_t* view_shape, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* out_rgba, uint32_t* out_pixels, float* root_box_out,
                      crt_tlas_node* tlas_out)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_shapes";
    int r;
    if ((r = shapes_check(c, K, bvh, S, triCount, T != nullptr, blasCount, view_shape != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    if (!cams || !positions || !out_rgba) return c->fail(CRT_ERR_INVALID, "%s: NULL buffer", what);
    if (view_shape)
        for (uint32_t k = 0; k < K; k++)
            if (view_shape[k] < 0 || (uint32_t)view_shape[k] >= S) return c->fail(CRT_ERR_INVALID, "%s: view_shape[%u] = %d lies outside [0, %u)", what, k, view_shape[k], S);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t camBytes = (size_t)K * 48, posBytes = ((size_t)S * triCount * 36 + 15u) & ~(size_t)15u, tBytes = (size_t)S * blasCount * 64;
    ViewsStage G;
    if ((r = views_stage_in(c, K, out_rgba, out_pixels, camBytes + posBytes + tBytes + (view_shape ? (size_t)K * 4 : 0), &G))) return r;
    float* dCams = reinterpret_cast<float*>(G.extra); float* dPos = reinterpret_cast<float*>(G.extra + camBytes);
    float* dT = T ? reinterpret_cast<float*>(G.extra + camBytes + posBytes) : nullptr;
    int32_t* dViewShape = view_shape ? reinterpret_cast<int32_t*>(G.extra + camBytes + posBytes + tBytes) : nullptr;
    HIPCK(c, hipMemcpyAsync(dCams, cams, camBytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dPos, positions, (size_t)S * triCount * 36, hipMemcpyHostToDevice, c->stream));
    if (dT) HIPCK(c, hipMemcpyAsync(dT, T, tBytes, hipMemcpyHostToDevice, c->stream));
    if (dViewShape) HIPCK(c, hipMemcpyAsync(dViewShape, view_shape, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    if ((r = shapes_run(c, dCams, K, bvh, dPos, S, dT, dViewShape, spp_first, frames, passes, scale, G.dRgba, G.dPix, root_box_out, tlas_out, c->stream, what))) return r;
    return views_stage_out(c, K, out_rgba, out_pixels, G);
}

// ---- crt_render_shape_sets / crt_render_shape_sets_device: the same over shapes in which M BLASes of a two-level scene deform (device/render_shape_sets.h) ----
// where a set job's table keeps what (device/layout.h ShapeSetMesh): ShapeLayout's head and rows, the two tables the kernels read, then the images, each the M
// sub-images in the order of `bvhs` and the pose image.  With M = 1 an image is ShapeLayout's.
struct ShapeSetLayout {
    uint32_t N, rowFloats;
    size_t headBytes, tableBytes; uint32_t headsOff, rowsOff, meshOff, instRootOff, imagesOff, imageStride, poseRel, setTris;
    std::vector<crt::ShapeSetMesh> mesh;          // plan, levelOff, levels, rootCode: filled by shape_sets_run
    ShapeSetLayout(const crt_ctx::Flat& f, const uint32_t* bvhs, uint32_t M, uint32_t S)
    {
        N = (uint32_t)f.triCount.size(); rowFloats = 6u * N;
        headsOff = (uint32_t)sizeof(crt::ShapeJobHeader);
        headBytes = headsOff + (size_t)S * sizeof(crt::TlasBuildHeader);
        const size_t meshAt = (headBytes + (size_t)S * rowFloats * 4u + 15u) & ~(size_t)15u, rootsAt = meshAt + (size_t)M * sizeof(crt::ShapeSetMesh);
        const size_t imagesAt = (rootsAt + (size_t)N * 4u + 127u) & ~(size_t)127u;
        size_t at = 0, tris = 0;
        for (uint32_t m = 0; m < M; m++) {
            crt::ShapeSetMesh d{};
            d.bvh = bvhs[m]; d.pairBase = (uint32_t)f.pairBase[d.bvh]; d.pairCount = f.nodesUsed[d.bvh] / 2; d.triBase = (uint32_t)f.triBase[d.bvh]; d.triCount = f.triCount[d.bvh];
            d.triFirst = (uint32_t)tris; d.pairRel = (uint32_t)at; d.leafRel = (uint32_t)(at + (size_t)(d.pairCount ? d.pairCount : 1u) * 64u);
            at = (d.leafRel + (size_t)d.triCount * 48u + 63u) & ~(size_t)63u;
            tris += d.triCount;
            mesh.push_back(d);
        }
        const size_t poseAt = (at + 127u) & ~(size_t)127u, stride = (poseAt + (size_t)(f.shadeOff - f.tlasOff) + 127u) & ~(size_t)127u;
        tableBytes = imagesAt + (size_t)S * stride + 64u;                   // (+ 64: a fetch of 64 bytes at the last record's last row stays inside)
        // shape_sets_check refuses a table beyond 4 GiB before anything uses the 32-bit fields (one image is below 4 GiB: it is smaller than the geometry buffer)
        rowsOff = (uint32_t)headBytes; meshOff = (uint32_t)meshAt; instRootOff = (uint32_t)rootsAt; imagesOff = (uint32_t)imagesAt; imageStride = (uint32_t)stride;
        poseRel = (uint32_t)poseAt; setTris = (uint32_t)tris;
    }
};

// the checks that need no buffer, in the order crt_abi.h lists the refusals
static int shape_sets_check(crt_ctx* c, uint32_t K, const uint32_t* bvhs, uint32_t M, uint32_t S, uint32_t setTris, bool haveT, uint32_t blasCount, bool viewShape, uint32_t frames,
                            uint32_t passes, const char* what)
{
    if (!c->haveScene && !c->havePrim) return c->fail(CRT_ERR_STATE, "%s before crt_upload_scene", what);
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the PrimitiveScene has no BVH to refit", what);
    const crt_ctx::Flat& f = c->flat;
    if (f.kind != CRT_SCENE_TLAS) return c->fail(CRT_ERR_INVALID, "%s applies to two-level scenes; a FileScene has one BVH (crt_render_shapes)", what);
    const uint32_t N = (uint32_t)f.triCount.size();
    if (!bvhs) return c->fail(CRT_ERR_INVALID, "%s: bvhs is NULL", what);
    if (M == 0 && K > 0) return c->fail(CRT_ERR_INVALID, "%s: %u views and no BVH in the set", what, K);
    std::vector<uint8_t> named(N, 0);
    uint64_t tris = 0;
    for (uint32_t m = 0; m < M; m++) {
        if (bvhs[m] >= N) return c->fail(CRT_ERR_INVALID, "%s: bvhs[%u] = %u of a scene with %u BLAS", what, m, bvhs[m], N);
        if (named[bvhs[m]]) return c->fail(CRT_ERR_INVALID, "%s: bvhs[%u] = %u is named twice", what, m, bvhs[m]);
        named[bvhs[m]] = 1; tris += f.triCount[bvhs[m]];
    }
    if (setTris != tris) return c->fail(CRT_ERR_INVALID, "%s: %u triangles per shape, the %u uploaded BVHs of the set have %llu (Refit keeps the topology)", what, setTris, M, (unsigned long long)tris);
    if (!haveT || blasCount != N) return c->fail(CRT_ERR_INVALID, "%s: %u transforms per shape%s, the uploaded scene has %u BLAS", what, blasCount, haveT ? "" : " (T is NULL)", N);
    if (f.tlasNodeCount != 2u * N) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the scene was uploaded with %u TLAS nodes, TLASBVH::Build makes %u", what, f.tlasNodeCount, 2u * N);
    if (passes < 1 || passes > 4) return c->fail(CRT_ERR_INVALID, "%s: passes must be 1..4 (the reference's UI range, renderer.cpp:178)", what);
    if ((uint64_t)K * frames > 0x7fffffffull) return c->fail(CRT_ERR_UNSUPPORTED, "%s: at most 2^31-1 view-frames per call (%u views x %u frames)", what, K, frames);
    if (c->renderAccel != 0) return c->fail(CRT_ERR_UNSUPPORTED, "%s: the KD-tree / grid structures have no refit (crt_set_render_accel(0) first; crt_refit_device drops those sets too)", what);
    if (K > 0 && S == 0) return c->fail(CRT_ERR_INVALID, "%s: %u views and no shape", what, K);
    if (!viewShape && S != K) return c->fail(CRT_ERR_INVALID, "%s: without view_shape view k renders shape k, so S (%u) must equal K (%u)", what, S, K);
    const ShapeSetLayout L(f, bvhs, M, S);
    if (L.tableBytes > crt::kMaxGeomBytes)
        return c->fail(CRT_ERR_UNSUPPORTED, "%s: %u shapes of %u bytes each exceed the 4 GiB the kernel's 32-bit offsets address; split the job", what, S, L.imageStride);
    return 0;
}

// The job on `st`, after the checks that need no launch: shapes_run's with the set's two tables enqueued in front of the ONE leaf launch and the ONE box launch.
// The tables travel from the tail of the pinned block the read-back uses; the call waits for that read-back, which is behind the copy on `st`.
static int shape_sets_run(crt_ctx* c, const float* dCams, uint32_t K, const uint32_t* bvhs, uint32_t M, const float* dPos, uint32_t S, const float* dT, const int32_t* dViewShape,
                          uint32_t sppFirst, uint32_t frames, uint32_t passes, float scale, float* dRgba, uint32_t* dPixels, float* rootBoxOut, crt_tlas_node* tlasOut, hipStream_t st,
                          const char* what)
{
    const crt_ctx::Flat& f = c->flat;
    ShapeSetLayout L(f, bvhs, M, S);
    const uint32_t N = L.N;
    int r;
    if (c->refitPlans.size() != f.triCount.size()) c->refitPlans.assign(f.triCount.size(), crt_ctx::RefitPlan{});
    std::vector<uint32_t> instRoot(N, crt::kInstLive);
    for (crt::ShapeSetMesh& d : L.mesh) {
        if (!c->refitPlans[d.bvh].built && (r = build_refit_plan(c, d.bvh))) return r;
        const crt_ctx::RefitPlan& P = c->refitPlans[d.bvh];
        d.plan = reinterpret_cast<const crt::RefitPlanRec*>(P.dPlan); d.levelOff = P.dLevelOff; d.levels = P.levels; d.rootCode = P.rootCode;
        // node 0 of the refitted BVH as the image names it (shape_build.hip image_ref)
        instRoot[d.bvh] = (P.rootCode & crt::kPlanInterior) ? (crt::kRefInterior | ((d.pairRel >> 4) + (P.rootCode & ~crt::kPlanInterior) * 4u)) : ((d.leafRel + P.rootCode * 48u) >> 4);
    }
    const size_t nodeBytes = (size_t)2u * N * sizeof(crt::TlasNode), meshBytes = (size_t)M * sizeof(crt::ShapeSetMesh);
    const size_t boxesAt = L.headBytes, nodesAt = boxesAt + (rootBoxOut ? (size_t)S * M * 24u : 0), tablesAt = (nodesAt + (tlasOut ? (size_t)S * nodeBytes : 0) + 15u) & ~(size_t)15u;
    const size_t backBytes = tablesAt + meshBytes + (size_t)N * 4u;
    // The builds are readers, as crt_render_shapes': the live pairs, leaf records, Instance records and node-0 boxes as the last write left them.
    if ((r = wait_scene(c, st))) return r;
    if ((r = job_table(c, L.tableBytes, backBytes, st))) return r;
    char* table = c->dPoseTable;
    HIPCK(c, hipMemsetAsync(table, 0xff, sizeof(uint32_t), st));            // ShapeJobHeader::badView = kPoseNoBadView
    memcpy(c->hPoseBack + tablesAt, L.mesh.data(), meshBytes); memcpy(c->hPoseBack + tablesAt + meshBytes, instRoot.data(), (size_t)N * 4u);
    HIPCK(c, hipMemcpyAsync(table + L.meshOff, c->hPoseBack + tablesAt, meshBytes + (size_t)N * 4u, hipMemcpyHostToDevice, st));      // (instRootOff = meshOff + meshBytes)
    const crt::ShapeSetBuildDev sb{c->hScene.geom, (uint32_t)f.leafOff, dPos, L.setTris, c->dRootBox, L.rowFloats, table, L.rowsOff, L.meshOff, L.instRootOff, L.imagesOff, L.imageStride, S, M};
    HIPCK(c, crt_launch_shape_set_build(&sb, L.mesh.data(), instRoot.data(), dViewShape, K, st));
    HIPCK(c, crt_launch_tlas_build_shapes(c->hScene.geom, (uint32_t)f.instOff, dT, reinterpret_cast<const float*>(table + L.rowsOff), N, (uint32_t)(f.tlasPairOff - f.tlasOff),
                                          (uint32_t)(f.instOff - f.tlasOff), c->hScene.poolRefBits, table, L.headsOff, L.imagesOff + L.poseRel, L.imageStride, S, st));
    if (rootBoxOut)
        for (uint32_t m = 0; m < M; m++)                                    // entry bvhs[m] of every row -> box (s, m)
            HIPCK(c, hipMemcpy2DAsync(c->hPoseBack + boxesAt + (size_t)m * 24u, (size_t)M * 24u, table + L.rowsOff + (size_t)bvhs[m] * 24u, (size_t)L.rowFloats * 4u, 24, S, hipMemcpyDeviceToHost, st));
    if (tlasOut) HIPCK(c, hipMemcpy2DAsync(c->hPoseBack + nodesAt, nodeBytes, table + L.imagesOff + L.poseRel, L.imageStride, nodeBytes, S, hipMemcpyDeviceToHost, st));
    // the one host wait: a job with a view_shape entry out of range or a failed build does not run, and the launches' LDS stack is sized by the tallest shape's TLAS
    if ((r = read_back(c, st, c->poseBack, c->hPoseBack, table, L.headBytes))) return r;
    const crt::ShapeJobHeader& job = *reinterpret_cast<const crt::ShapeJobHeader*>(c->hPoseBack);
    if (job.badView != crt::kPoseNoBadView) return c->fail(CRT_ERR_INVALID, "%s: view_shape[%u] lies outside [0, %u)", what, job.badView, S);
    crt::Scene job_scene = c->hScene;                                       // the launches' by-value Scene: the context's, with the job's stack depth.  c->hScene stays as it is
    if ((r = shape_tlas_heads(c, reinterpret_cast<const crt::TlasBuildHeader*>(c->hPoseBack + L.headsOff), S, &job_scene, what))) return r;
    const crt::ShapeSetTableDev tb{table, dViewShape, L.imagesOff, L.imageStride, L.instRootOff, L.poseRel, (uint32_t)(f.instOff - f.tlasOff)};
    if ((r = views_run(c, dCams, K, sppFirst, frames, passes, scale, dRgba, dPixels, st, &job_scene, nullptr, nullptr, &tb))) return r;
    // the host outputs last, once nothing can refuse the job any more (the pinned copy is the call's own until it returns): a refused call writes nothing
    if (rootBoxOut) memcpy(rootBoxOut, c->hPoseBack + boxesAt, (size_t)S * M * 24u);
    if (tlasOut)
        for (uint32_t s = 0; s < S; s++) unpack_tlas_nodes(reinterpret_cast<const crt::TlasNode*>(c->hPoseBack + nodesAt + s * nodeBytes), 2u * N, tlasOut + (size_t)s * 2u * N);
    return 0;
}

int crt_render_shape_sets_device(crt_ctx* c, const float* d_cams, uint32_t K, const uint32_t* bvhs, uint32_t M, const float* d_positions, uint32_t S, uint32_t setTris, const float* d_T,
                                 uint32_t blasCount, const int32_t* d_view_shape, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba,
                                 uint32_t* d_out_pixels, float* root_box_out, crt_tlas_node* tlas_out, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_shape_sets_device";
    int r;
    if ((r = shape_sets_check(c, K, bvhs, M, S, setTris, d_T != nullptr, blasCount, d_view_shape != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    if (reinterpret_cast<uintptr_t>(d_out_rgba) & 15u) return c->fail(CRT_ERR_INVALID, "%s: d_out_rgba %p is not 16-byte aligned", what, (void*)d_out_rgba);
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_cams, (size_t)K * 48}, {d_positions, (size_t)S * setTris * 36}, {d_T, (size_t)S * blasCount * 64}, {d_out_rgba, K * px * 16}}, stream, &st))) return r;
    if (d_out_pixels && (r = check_device_buffer(c, d_out_pixels, K * px * 4, what))) return r;
    if (d_view_shape && (r = check_device_buffer(c, d_view_shape, (size_t)K * 4, what))) return r;
    if ((r = take_query_slot(c, &k))) return r;
    if ((r = shape_sets_run(c, d_cams, K, bvhs, M, d_positions, S, d_T, d_view_shape, spp_first, frames, passes, scale, d_out_rgba, d_out_pixels, root_box_out, tlas_out, st, what))) return r;
    return end_device_query(c, k, st);
}

int crt_render_shape_sets(crt_ctx* c, const float* cams, uint32_t K, const uint32_t* bvhs, uint32_t M, const float* positions, uint32_t S, uint32_t setTris, const float* T, uint32_t blasCount,
                          const int32_t* view_shape, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* out_rgba, uint32_t* out_pixels, float* root_box_out,
                          crt_tlas_node* tlas_out)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_render_shape_sets";
    int r;
    if ((r = shape_sets_check(c, K, bvhs, M, S, setTris, T != nullptr, blasCount, view_shape != nullptr, frames, passes, what))) return r;
    if (K == 0 || frames == 0) return CRT_OK;
    if (!cams || !positions || !out_rgba) return c->fail(CRT_ERR_INVALID, "%s: NULL buffer", what);
    if (view_shape)
        for (uint32_t k = 0; k < K; k++)
            if (view_shape[k] < 0 || (uint32_t)view_shape[k] >= S) return c->fail(CRT_ERR_INVALID, "%s: view_shape[%u] = %d lies outside [0, %u)", what, k, view_shape[k], S);
    HIPCK(c, hipSetDevice(c->cfg.device));
    const size_t camBytes = (size_t)K * 48, posBytes = ((size_t)S * setTris * 36 + 15u) & ~(size_t)15u, tBytes = (size_t)S * blasCount * 64;
    ViewsStage G;
    if ((r = views_stage_in(c, K, out_rgba, out_pixels, camBytes + posBytes + tBytes + (view_shape ? (size_t)K * 4 : 0), &G))) return r;
    float* dCams = reinterpret_cast<float*>(G.extra); float* dPos = reinterpret_cast<float*>(G.extra + camBytes);
    float* dT = reinterpret_cast<float*>(G.extra + camBytes + posBytes);
    int32_t* dViewShape = view_shape ? reinterpret_cast<int32_t*>(G.extra + camBytes + posBytes + tBytes) : nullptr;
    HIPCK(c, hipMemcpyAsync(dCams, cams, camBytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dPos, positions, (size_t)S * setTris * 36, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(dT, T, tBytes, hipMemcpyHostToDevice, c->stream));
    if (dViewShape) HIPCK(c, hipMemcpyAsync(dViewShape, view_shape, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    if ((r = shape_sets_run(c, dCams, K, bvhs, M, dPos, S, dT, dViewShape, spp_first, frames, passes, scale, G.dRgba, G.dPix, root_box_out, tlas_out, c->stream, what))) return r;
    return views_stage_out(c, K, out_rgba, out_pixels, G);
}

// tools / tests: the lanes a full sample-query launch of this scene and accelerator holds at once (the grid is that many lanes, or fewer when the rays need fewer)
extern "C" int crt_debug_sample_resident_lanes(crt_ctx* c, int accel, uint32_t* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    int r;
    if ((r = sample_check(c, accel, 0, "crt_debug_sample_resident_lanes"))) return r;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_sample(c, accel, nullptr, nullptr, nullptr, 0u, nullptr, out, c->stream));
    return CRT_OK;
}

// ---- crt_trace / crt_trace_device: the Whitted Renderer::Trace(ray, 0) per ray of a buffer (device/trace_query.h) ----
// query_check's checks, the PrimitiveScene refused as crt_whitted_tick refuses it, and the traversal stack's LDS columns for the four wavefronts of a workgroup
static int trace_check(crt_ctx* c, int accel, size_t n, const char* what)
{
    if (accel != 0 && accel != CRT_ACCEL_KDTREE && accel != CRT_ACCEL_GRID) return c->fail(CRT_ERR_INVALID, "%s: unknown accelerator kind %d", what, accel);
    if (c->havePrim) return c->fail(CRT_ERR_UNSUPPORTED, "%s: Trace over the PrimitiveScene is not supported (crt_whitted_tick refuses it too)", what);
    int r;
    if ((r = query_check(c, accel, false, n, what))) return r;
    const uint32_t words = crt_trace_query_stack_words(&c->hScene, accel, &c->alt, accel ? &c->blasAlt[accel - 1] : nullptr);
    if ((uint64_t)words * 64u * 4u * 4u > 64u * 1024u) return c->fail(CRT_ERR_UNSUPPORTED, "%s: a traversal stack of %u dwords per lane exceeds the kernel's LDS", what, words);
    return 0;
}

static hipError_t launch_trace(crt_ctx* c, int accel, const void* rays, float* rgb, int32_t* trav, int32_t* tested, uint32_t n, uint32_t* cursor, uint32_t* residentLanes, hipStream_t st)
{
    return crt_launch_trace_query(&c->hScene, accel, &c->alt, accel ? &c->blasAlt[accel - 1] : nullptr, rays, rgb, trav, tested, n, c->dCounters, cursor, residentLanes, st);
}

int crt_trace(crt_ctx* c, int accel, const crt_ray* rays, float* rgb, int32_t* traversed, int32_t* tested, size_t n)
{
    if (!c) return CRT_ERR_INVALID;
    int r;
    if ((r = trace_check(c, accel, n, "crt_trace"))) return r;
    if (n == 0) return CRT_OK;
    if (!rays || !rgb) return c->fail(CRT_ERR_INVALID, "crt_trace: NULL buffer");
    HIPCK(c, hipSetDevice(c->cfg.device));
    if ((r = stage(c, n * (12 + sizeof(crt_ray) + 8)))) return r;
    float* dRgb = reinterpret_cast<float*>(c->dStage); char* dRays = c->dStage + n * 12;
    int32_t* dTrav = reinterpret_cast<int32_t*>(dRays + n * sizeof(crt_ray)); int32_t* dTested = dTrav + n;
    HIPCK(c, hipMemcpyAsync(dRays, rays, n * sizeof(crt_ray), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, launch_trace(c, accel, dRays, dRgb, traversed ? dTrav : nullptr, tested ? dTested : nullptr, (uint32_t)n, c->dQueryCursor, nullptr, c->stream));
    HIPCK(c, hipMemcpyAsync(rgb, dRgb, n * 12, hipMemcpyDeviceToHost, c->stream));
    if (traversed) HIPCK(c, hipMemcpyAsync(traversed, dTrav, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (tested) HIPCK(c, hipMemcpyAsync(tested, dTested, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_trace_device(crt_ctx* c, int accel, const crt_ray* d_rays, float* d_rgb, int32_t* d_traversed, int32_t* d_tested, size_t n, void* stream)
{
    if (!c) return CRT_ERR_INVALID;
    const char* what = "crt_trace_device";
    int r;
    if ((r = trace_check(c, accel, n, what))) return r;
    if (n == 0) return CRT_OK;
    hipStream_t st = nullptr; int k = 0;
    if ((r = device_entry(c, what, {{d_rays, n * sizeof(crt_ray)}, {d_rgb, n * 12}}, stream, &st))) return r;
    if (d_traversed && (r = check_device_buffer(c, d_traversed, n * 4, what))) return r;          // the optional outputs: checked where given
    if (d_tested && (r = check_device_buffer(c, d_tested, n * 4, what))) return r;
    if ((r = wait_scene(c, st)) || (r = take_query_slot(c, &k))) return r;
    if (accel != 0 && c->altReady) HIPCK(c, hipStreamWaitEvent(st, c->altReady, 0));     // the accelerators' copies ran on the null stream
    HIPCK(c, launch_trace(c, accel, d_rays, d_rgb, d_traversed, d_tested, (uint32_t)n, c->dQuerySlots + 16 * k, nullptr, st));
    return end_device_query(c, k, st);
}

// tools / tests: the lanes a full trace-query launch of this scene and accelerator holds at once (the grid is that many lanes, or fewer when the rays need fewer)
extern "C" int crt_debug_trace_resident_lanes(crt_ctx* c, int accel, uint32_t* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    int r;
    if ((r = trace_check(c, accel, 0, "crt_debug_trace_resident_lanes"))) return r;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, launch_trace(c, accel, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, out, c->stream));
    return CRT_OK;
}

int crt_get_light(crt_ctx* c, float pos[3], float color[3])
{
    if (!c || !pos || !color) return CRT_ERR_INVALID;
    if (!c->haveScene) return c->fail(c->havePrim ? CRT_ERR_UNSUPPORTED : CRT_ERR_STATE, "crt_get_light needs a triangle scene (crt_upload_scene)");
    memcpy(pos, c->hScene.lightPos, 12);
    color[0] = 24.0f; color[1] = 24.0f; color[2] = 22.0f;                      // GetLightColor, file_scene.cpp:164-168
    return CRT_OK;
}

int crt_get_counters(crt_ctx* c, crt_counters* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemcpyAsync(out, c->dCounters, sizeof(crt::Counters), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_reset_counters(crt_ctx* c)
{
    if (!c) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemsetAsync(c->dCounters, 0, sizeof(crt::Counters), c->stream));
    return CRT_OK;
}

int crt_get_timing(crt_ctx* c, crt_timing* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (auto st : c->streams) HIPCK(c, hipStreamSynchronize(st));
    if (c->aheadStream) HIPCK(c, hipStreamSynchronize(c->aheadStream));
    harvest_tuning(c);                                         // the latency mode's stage timings, before the pairs are recycled
    memset(out, 0, sizeof(*out));
    out->render_kernel_ms = (float)c->foldedRenderMs; out->resolve_kernel_ms = (float)c->foldedAccMs;
    for (auto& ev : c->evRender) { float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, ev.a, ev.b)); out->render_kernel_ms += ms; }
    for (auto& ev : c->evAcc) { float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, ev.a, ev.b)); out->resolve_kernel_ms += ms; }
    out->render_launches = (uint32_t)c->evRender.size() + c->foldedLaunches;
    out->pool_launches = c->poolLaunches; out->split_launches = c->splitLaunches;
    c->foldedRenderMs = c->foldedAccMs = 0; c->foldedLaunches = 0; c->poolLaunches = 0; c->splitLaunches = 0;
    for (auto& ev : c->evRender) c->evPool.push_back(ev);      // the figures cover every launch since the previous crt_get_timing
    for (auto& ev : c->evAcc) c->evPool.push_back(ev);
    c->evRender.clear(); c->evAcc.clear();
    return CRT_OK;
}

int crt_get_tile_clocks(crt_ctx* c, uint64_t* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    if (!c->dTileClocks) return c->fail(CRT_ERR_STATE, "tile clocks are recorded only by a collectStats context");
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemcpyAsync(out, c->dTileClocks, (size_t)c->tileCount * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

// diagnostic builds (-DCRT_STAMPS) only: 16 extra words per tile behind the tile clocks (not part of the public ABI)
// tests: HIP timing events currently held by the context (bounded: completed launches are folded into totals, see fold_completed)
// LDS bytes one render_pool_kernel wavefront of a launch of `frames` frames on the current scene asks for, the per-workgroup limit it is held to, and the width of
// the scene's pool references (0: none).  -1: no context / no scene.
extern "C" int crt_debug_pool_lds(crt_ctx* c, uint32_t frames, uint32_t* bytes, uint32_t* limit, uint32_t* refBits)
{
    if (!c || !c->haveScene) return -1;
    if (!c->poolLdsLimit) c->poolLdsLimit = crt_pool_lds_limit(c->cfg.device);
    if (bytes) *bytes = c->hScene.poolRefBits ? pool_lds_need(c, frames) : 0u;
    if (limit) *limit = c->poolLdsLimit;
    if (refBits) *refBits = c->hScene.poolRefBits;
    return 0;
}
extern "C" int crt_debug_live_events(crt_ctx* c) { return c ? (int)(2 * (c->evRender.size() + c->evAcc.size() + c->evPool.size())) : -1; }

// tests: the device's short reciprocals (dev_common.h rcp_exact*) against the IEEE division over all 2^32 inputs; out[4] = {inputs, differences x 3}
extern "C" int crt_debug_check_reciprocals(crt_ctx* c, uint64_t* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    unsigned long long* d = nullptr;
    HIPCK(c, hipMalloc(&d, 32));
    hipError_t e = hipMemsetAsync(d, 0, 32, c->stream);
    if (e == hipSuccess) e = crt_launch_check_reciprocals(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCK(c, e);
    return CRT_OK;
}

// tests: the device's short square root (dev_common.h sqrt_exact) against the compiler's IEEE sequence over all 2^32 inputs; out[2] = {inputs, differences}
extern "C" int crt_debug_check_sqrt(crt_ctx* c, uint64_t* out)
{
    if (!c || !out) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    unsigned long long* d = nullptr;
    HIPCK(c, hipMalloc(&d, 16));
    hipError_t e = hipMemsetAsync(d, 0, 16, c->stream);
    if (e == hipSuccess) e = crt_launch_check_sqrt(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCK(c, e);
    return CRT_OK;
}

// tests: what the context's Scene block holds for primary rays: out[16 + kPrimFloats] = rootPair, then the camera-relative block (layout.h set_primary); the
// optional others: camera[12] = camPos, topLeft, topRight, bottomLeft; lightFloor[4] = lightInvT[7], [3], [11], floorD
extern "C" int crt_debug_primary_block(crt_ctx* c, float* out, float* camera, float* lightFloor)
{
    if (!c || !out) return CRT_ERR_INVALID;
    const crt::Scene& s = c->hScene;
    static_assert(offsetof(crt::Scene, primRoot) == offsetof(crt::Scene, rootPair) + 64 && offsetof(crt::Scene, primDown) + 12 == offsetof(crt::Scene, rootPair) + 64 + 4 * crt::kPrimFloats, "primary block");
    memcpy(out, s.rootPair, 64 + 4 * crt::kPrimFloats);
    if (camera) memcpy(camera, s.camPos, 48);
    if (lightFloor) { lightFloor[0] = s.lightInvT[7]; lightFloor[1] = s.lightInvT[3]; lightFloor[2] = s.lightInvT[11]; lightFloor[3] = s.floorD; }
    return CRT_OK;
}
// tests (no GPU needed): the same on a context that holds nothing but a Scene block, through the block's writers in the order of a session.  op 0 = a new context's
// defaults, then upload's light / floor block and root pair (in = lightInvT[12], floorD, rootPair[16]); op 1 = the camera setter's part (in = camPos, topLeft,
// topRight, bottomLeft); op 2 = a rebuilt root pair (in = rootPair[16]), what set_root does after a refit / TLAS rebuild.  out as crt_debug_primary_block's.
extern "C" int crt_debug_primary_block_host(int op, const float* in, float* out)
{
    static crt::Scene s{};
    if (!in || !out || op < 0 || op > 2) return CRT_ERR_INVALID;
    if (op == 0) {
        s = crt::Scene{};
        s.camPos[2] = -2; s.topLeft[0] = -1; s.topLeft[1] = 1; s.topRight[0] = 1; s.topRight[1] = 1; s.bottomLeft[0] = -1; s.bottomLeft[1] = -1;
        memcpy(s.lightInvT, in, 48); s.floorD = in[12]; memcpy(s.rootPair, in + 13, 64); s.rootIsPair = 1;
    } else if (op == 1) { memcpy(s.camPos, in, 12); memcpy(s.topLeft, in + 3, 12); memcpy(s.topRight, in + 6, 12); memcpy(s.bottomLeft, in + 9, 12); }
    else memcpy(s.rootPair, in, 64);
    crt::set_primary(s);
    memcpy(out, s.rootPair, 64 + 4 * crt::kPrimFloats);
    return CRT_OK;
}

// tests / tools: the context's tile classes as the device holds them, out[min(cap, tiles owned)] (classified first if the Scene block changed since the last
// crt_render).  Returns the number of owned tiles, or a negative error code.
// (_ex: the whole byte, layout.h kTileFloorSure included; the older entry keeps returning the three kTileNo* bits)
extern "C" int crt_debug_tile_classes_ex(crt_ctx* c, uint8_t* out, uint32_t cap)
{
    if (!c || (!out && cap)) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    { const int r = update_tile_class(c); if (r) return r; }
    const uint32_t n = cap < c->tileCount ? cap : c->tileCount;
    if (n) {
        HIPCK(c, hipMemcpyAsync(out, c->dTileClass, n, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    return (int)c->tileCount;
}
extern "C" int crt_debug_tile_classes(crt_ctx* c, uint8_t* out, uint32_t cap)
{
    const int r = crt_debug_tile_classes_ex(c, out, cap);
    for (uint32_t i = 0; r > 0 && i < cap && i < (uint32_t)r; i++) out[i] &= (uint8_t)crt::kTileNoMask;
    return r;
}
// tests (no GPU needed): classify_tiles on a bare Scene block filled the way a session fills it.  in[33] = camPos, topLeft, topRight, bottomLeft; lightInvT[3], [7],
// [11]; lightSize; floorD; rootPair[16].  flags: 1 = lightAxis, 2 = floorAxisY, 4 = rootIsPair.  out[tileCount], the tiles tileFirst + i * tileStride of a W x H image.
// (_ex: the whole byte, layout.h kTileFloorSure included; the older entry keeps returning the three kTileNo* bits)
extern "C" int crt_debug_tile_classes_host_ex(const float* in, uint32_t flags, int W, int H, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint8_t* out);
extern "C" int crt_debug_tile_classes_host(const float* in, uint32_t flags, int W, int H, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint8_t* out)
{
    const int r = crt_debug_tile_classes_host_ex(in, flags, W, H, tileFirst, tileStride, tileCount, out);
    for (uint32_t i = 0; r == CRT_OK && i < tileCount; i++) out[i] &= (uint8_t)crt::kTileNoMask;
    return r;
}
extern "C" int crt_debug_tile_classes_host_ex(const float* in, uint32_t flags, int W, int H, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint8_t* out)
{
    if (!in || !out || W < 16 || H < 16 || tileStride == 0) return CRT_ERR_INVALID;
    const uint32_t tilesX = (uint32_t)(W / 16), tiles = tilesX * (uint32_t)(H / 16);
    if (tileCount && (unsigned long long)tileFirst + (unsigned long long)(tileCount - 1) * tileStride >= tiles) return CRT_ERR_INVALID;
    crt::Scene s{};
    memcpy(s.camPos, in, 12); memcpy(s.topLeft, in + 3, 12); memcpy(s.topRight, in + 6, 12); memcpy(s.bottomLeft, in + 9, 12);
    s.W = W; s.H = H; s.invW = 1.0f / W; s.invH = 1.0f / H;
    s.lightInvT[0] = s.lightInvT[5] = s.lightInvT[10] = 1.0f; s.lightInvT[3] = in[12]; s.lightInvT[7] = in[13]; s.lightInvT[11] = in[14];
    s.lightSize = in[15]; s.floorN[1] = 1.0f; s.floorD = in[16];
    memcpy(s.rootPair, in + 17, 64);
    s.lightAxis = flags & 1u; s.floorAxisY = (flags >> 1) & 1u; s.rootIsPair = (flags >> 2) & 1u;
    crt::set_primary(s);
    crt::classify_tiles(s, W, H, tilesX, tileFirst, tileStride, tileCount, out);
    return CRT_OK;
}

// tests: dev_common.h's fp32 building blocks (device/probe.hip) and the torus' fp64 ones (end of device/render_prim.hip) on the device at hand, one element per
// thread: host buffers in and out, one launch.  Ops and record layouts: the table at the top of device/probe.hip.  n <= 2^25 records per call.
static int device_probe(crt_ctx* c, int op, const void* in, void* out, uint32_t n)
{
    static const uint8_t words[18][2] = {{1, 1}, {1, 1}, {2, 1}, {1, 1}, {2, 1}, {6, 7}, {1, 18}, {4, 1}, {5, 3}, {13, 2}, {16, 4}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {4, 2}, {2, 1}, {5, 3}};
    if (!c || !in || !out || op < 0 || op > 17 || n > (1u << 25)) return CRT_ERR_INVALID;
    if (n == 0) return CRT_OK;
    const size_t inBytes = (size_t)n * words[op][0] * 4, outBytes = (size_t)n * words[op][1] * 4;
    HIPCK(c, hipSetDevice(c->cfg.device));
    char* d = nullptr;
    HIPCK(c, hipMalloc((void**)&d, inBytes + outBytes));               // inBytes is a multiple of 8 for the fp64 ops: both halves stay aligned
    hipError_t e = hipMemcpyAsync(d, in, inBytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = (op <= 10 || op == 17) ? crt_launch_probe_f32(op, d, d + inBytes, n, c->stream) : crt_launch_probe_f64(op, d, d + inBytes, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + inBytes, outBytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCK(c, e);
    return CRT_OK;
}
extern "C" int crt_debug_device_probe(crt_ctx* c, int op, const void* in, void* out, uint32_t n) { return (op > 16) ? CRT_ERR_INVALID : device_probe(c, op, in, out, n); }
// tests: op 8's lookup through sky_angles, the guarded form the render kernels and the sky query call (probe.hip op 17; records as op 8's)
extern "C" int crt_debug_sky_probe(crt_ctx* c, const void* in, void* out, uint32_t n) { return device_probe(c, 17, in, out, n); }
// tests: the short arithmetic forms of dev_common.h against the forms they stand for, side by side on the device (device/probe.hip probe_arith_kernel: `what`, the
// record layouts and the generated records are listed there).  in: nIn records (sweeps: their 4-word header); n: records in all, the ones behind nIn generated from
// `seed`.  out[9] = {differing records, the lowest of them (0xffffffff: none), its operands [3], old result [2], new result [2]}
extern "C" int crt_debug_arith_forms(crt_ctx* c, int what, const void* in, uint32_t nIn, uint32_t n, uint32_t seed, uint32_t* out)
{
    static const uint8_t words[4] = {3, 2, 3, 0};
    if (!c || !out || what < 0 || what > 3 || nIn > n || (nIn && !in) || (what == 3 && !in)) return CRT_ERR_INVALID;
    for (int k = 0; k < 9; k++) out[k] = 0u;
    out[1] = 0xffffffffu;
    if (n == 0) return CRT_OK;
    const size_t inBytes = what == 3 ? 16 : (size_t)nIn * words[what] * 4;
    HIPCK(c, hipSetDevice(c->cfg.device));
    char* d = nullptr;
    HIPCK(c, hipMalloc((void**)&d, 64 + inBytes));
    hipError_t e = hipMemcpyAsync(d, out, 36, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && inBytes) e = hipMemcpyAsync(d + 64, in, inBytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = crt_launch_probe_arith(what, d + 64, nIn, n, seed, 0xffffffffu, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && out[0] != 0u) {                                       // the lowest differing record once more, for its operands and results
        e = crt_launch_probe_arith(what, d + 64, nIn, n, seed, out[1], d, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out + 2, d + 8, 28, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(d);
    HIPCK(c, e);
    return CRT_OK;
}

// tests (no GPU needed): the planner's decision for given tile costs — plan_job on a context that holds nothing but the costs.  table[] receives the block
// descriptors (tile | first frame << 16 | log2(lanes) << 22 | window << 25), order[] the dispatch order, *head the number of leading tiles of it that go to the table
// when the rest goes to the pool.  Returns the number of blocks, or a negative error code.
extern "C" int crt_debug_plan_job(const uint32_t* cost, uint32_t n, uint32_t windows, uint32_t frames, int pool, double poolWindowTicks,
                                  uint32_t* table, uint32_t tableCap, uint32_t* head, uint32_t* order)
{
    if (!cost || !n || !table || !head || !order) return CRT_ERR_INVALID;
    crt_ctx c;
    c.tileCount = n; c.jobCostValid = true; c.poolWindowTicks = poolWindowTicks;
    c.streams.assign(2, nullptr);
    c.jobCost.assign(cost, cost + n);
    c.jobOrder.resize(n);
    for (uint32_t i = 0; i < n; i++) c.jobOrder[i] = i;
    std::stable_sort(c.jobOrder.begin(), c.jobOrder.end(), [&](uint32_t a, uint32_t b) { return c.jobCost[a] > c.jobCost[b]; });
    std::vector<uint32_t> t; uint32_t h = 0;
    plan_job(&c, windows, frames, pool != 0, t, &h);
    c.streams.clear();
    if (t.size() > tableCap) return CRT_ERR_INVALID;
    memcpy(table, t.data(), t.size() * 4); memcpy(order, c.jobOrder.data(), (size_t)n * 4); *head = h;
    return (int)t.size();
}

// tests (no GPU needed): pool_wave_plan for tile costs given in dispatch order (cost == nullptr: unknown).  wf[nr] receives the frames per wavefront of every rank in the
// long part [0, *longFrames) of the launch (the rest of the frames: S per wavefront), start[nr] (optional) its expected start and *aim (optional) the makespan aim, both in
// the cost's ticks; safety / guard / share <= 0: the built-in terms.  Returns the launch's wavefronts.
extern "C" long long crt_debug_pool_wave_plan(const uint32_t* cost, uint32_t nr, uint32_t frames, double perCost, double startTicks, uint32_t resident, double safety, double guard,
                                              double share, uint32_t* wf, uint32_t* longFrames, double* start, double* aim)
{
    if (!nr || !frames || !wf || !longFrames) return CRT_ERR_INVALID;
    PoolWaveTerms tm; if (safety > 0) tm.safety = safety; if (guard > 0) tm.guard = guard; if (share > 0) tm.share = share;
    std::vector<uint32_t> w; std::vector<double> st;
    const uint64_t waves = pool_wave_plan(cost, nr, frames, crt_pool_streams(frames), perCost, startTicks, resident, tm, w, longFrames, &st, aim);
    memcpy(wf, w.data(), (size_t)nr * 4);
    if (start) memcpy(start, st.data(), (size_t)nr * 8);
    return (long long)waves;
}
// tests (no GPU needed): how the host splits a job's ranks between its pool launch and its sky launch, for tile classes cls[n] (layout.h kTileNo* bits) and tile costs
// cost[n] (nullptr: not measured yet — the order is the tile order with the sky tiles moved behind).  order[n] receives the dispatch order; *skyFirst the first rank of
// its sky tail (render_sky_kernel renders the ranks [*skyFirst, n)); *head the leading ranks the plan gives to the block table; *planRanks the ranks the pool launch's
// wave plan covers (they follow the head).  waveTab[2 n] receives that launch's wave table — (first block, frames per wavefront) per rank from *head to n, the kernel's
// search range — when the plan lengthens wavefronts (*tabBlocks > 0: its wavefronts, *longFrames: the frames of the long part).  Returns the sky tiles.
// (The split as sky_split asks for it.  install_job_plan plans a job again WITHOUT a sky launch when this plan has a head: *head > 0 here means the job keeps one pool launch.)
extern "C" int crt_debug_sky_split(const uint32_t* cost, const uint8_t* cls, uint32_t n, uint32_t windows, uint32_t frames, double poolWindowTicks, double skyWindowTicks,
                                   uint32_t* order, uint32_t* skyFirst, uint32_t* head, uint32_t* planRanks, uint32_t* waveTab, uint32_t* tabBlocks, uint32_t* longFrames)
{
    if (!cls || !n || !order || !skyFirst || !head || !planRanks || !waveTab || !tabBlocks || !longFrames) return CRT_ERR_INVALID;
    crt_ctx c;
    c.tileCount = n; c.poolWindowTicks = poolWindowTicks; c.skyWindowTicks = skyWindowTicks;
    c.hostClass.assign(cls, cls + n);
    *head = *planRanks = *tabBlocks = *longFrames = 0;
    if (!cost) {
        c.jobOrder.resize(n); for (uint32_t i = 0; i < n; i++) c.jobOrder[i] = i;
        c.skyTiles = sky_to_tail(c.hostClass, c.jobOrder);
    } else {
        c.jobCost.assign(cost, cost + n); c.jobCostValid = true;
        c.skyTiles = job_order(c.jobCost, c.hostClass, c.jobOrder);
        c.streams.assign(2, nullptr);
        const double skyTicks = c.skyTiles ? skyWindowTicks * (double)windows : 0.0;
        std::vector<uint32_t> table;
        plan_job(&c, windows, frames, true, table, head, c.skyTiles, skyTicks);
        table.clear();
        const PoolWavePlan p = plan_pool_waves(&c, windows, frames, *head, c.skyTiles, skyTicks, table);
        c.streams.clear();
        *planRanks = p.ranks; *tabBlocks = p.blocks; *longFrames = p.longFrames;
        if (table.size() > 2u * (size_t)n) return CRT_ERR_INVALID;
        memcpy(waveTab, table.data(), table.size() * 4);
    }
    memcpy(order, c.jobOrder.data(), (size_t)n * 4);
    *skyFirst = n - c.skyTiles;
    return (int)c.skyTiles;
}
// tests: render_sky_kernel launches of this context so far (never reset)
extern "C" int crt_debug_sky_launches(crt_ctx* c) { return c ? (int)c->skyLaunches : -1; }
// tests (no device needed): where the kernels put the samples of a launch of `frames` frames over tileCount tiles — device/sample_body.h's own position and size
// functions, evaluated on the host.  pos[frame][tile][pixel][pass] = byte position in the slab, of the sample form or (texel != 0) of the texel form;
// sizes = {bytes per window of samples, bytes per tile block}
extern "C" int crt_debug_slab_layout(int texel, uint32_t frames, uint32_t tileCount, uint32_t passes, unsigned long long* pos, unsigned long long* sizes)
{
    if (!pos || !sizes || passes < 1 || passes > 4 || tileCount == 0 || frames == 0) return CRT_ERR_INVALID;
    crt_slab_layout_probe(texel, frames, tileCount, passes, pos, sizes);
    return CRT_OK;
}
// tools: the tile costs the planner works with (100 MHz ticks per local tile, as the measuring job left them: 0 for a tile its sky launch rendered), and the
// machine time per window of the measuring job's pool launch and of its sky launch.  CRT_ERR_STATE until a measuring job's costs have been adopted (or
// crt_debug_set_job_costs has installed some), and again once a camera or scene change has condemned them.
extern "C" int crt_debug_job_costs(crt_ctx* c, uint32_t* out, double* poolWindowTicks, double* skyWindowTicks)
{
    if (!c || !out) return CRT_ERR_INVALID;
    if (!c->jobCostValid || c->orderDirty || c->jobCost.size() != c->tileCount) return CRT_ERR_STATE;      // (orderDirty: the next crt_render drops them, update_tile_order)
    memcpy(out, c->jobCost.data(), (size_t)c->tileCount * 4);
    if (poolWindowTicks) *poolWindowTicks = c->poolWindowTicks;
    if (skyWindowTicks) *skyWindowTicks = c->skyWindowTicks;
    return CRT_OK;
}
// tests: tile costs (100 MHz ticks per local tile, cost[tileCount]) and the two machine-time figures installed as if a measuring job had left them — the second
// half of adopt_job_costs, so the planner's whole input can be GIVEN (its own comes from device clocks, and a launch small enough for a test never oversubscribes
// the chip).  First the context is brought to the state the next crt_render would start from (class table and tile order of the current camera and scene: a change
// still pending would drop the costs again, as it drops measured ones) and a measurement in flight is settled, so that a late adoption cannot replace what is
// installed here.  Refused, with nothing written: a context without a scene (CRT_ERR_STATE), a statistics context (CRT_ERR_STATE: it never plans).
extern "C" int crt_debug_set_job_costs(crt_ctx* c, const uint32_t* cost, double poolWindowTicks, double skyWindowTicks)
{
    if (!c || !cost) return CRT_ERR_INVALID;
    if (!(poolWindowTicks >= 0) || !(skyWindowTicks >= 0)) return c->fail(CRT_ERR_INVALID, "crt_debug_set_job_costs: the window ticks must be >= 0");
    if (!c->haveScene) return c->fail(CRT_ERR_STATE, "crt_debug_set_job_costs before crt_upload_scene");
    if (c->cfg.collectStats) return c->fail(CRT_ERR_STATE, "crt_debug_set_job_costs: a statistics context never plans");
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->tileCount == 0) return CRT_OK;
    { int r = update_tile_class(c); if (r) return r; }
    { int r = update_tile_order(c); if (r) return r; }
    if (c->jobCostPending) { HIPCK(c, hipEventSynchronize(c->jobCostCopied)); c->jobCostPending = false; }
    return install_job_costs(c, std::vector<uint32_t>(cost, cost + c->tileCount), poolWindowTicks, skyWindowTicks);
}
// tests: wavefronts of the last render_pool_kernel launch that owned more than S frames (and so refilled their slots)
extern "C" int crt_debug_pool_long_waves(crt_ctx* c) { return c ? (int)c->lastLongWaves : -1; }
// the built-in terms of pool_wave_plan: {poolLong, load, safety, guard, share}
extern "C" void crt_debug_pool_wave_terms(double* out) { const PoolWaveTerms tm; out[0] = tm.poolLong; out[1] = tm.load; out[2] = tm.safety; out[3] = tm.guard; out[4] = tm.share; }

// diagnostics (tools/latency_probe.py): the tile costs the last recording single-window launch left on the device (100 MHz ticks, longest wavefront per tile)
extern "C" int crt_debug_tile_costs(crt_ctx* c, uint32_t* out)
{
    if (!c || !out || !c->dTileCost) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipDeviceSynchronize());
    HIPCK(c, hipMemcpy(out, c->dTileCost, (size_t)c->tileCount * 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// diagnostics (tools/probe_quality.py): lanes per wavefront and tile costs of one stage of the latency tuner ([0]: the probe's estimates when latProbed); returns the installed stage
extern "C" int crt_debug_lat_stage(crt_ctx* c, int stage, uint8_t* lanes, uint32_t* cost)
{
    if (!c || stage < 0 || stage > crt_ctx::kLatStages) return CRT_ERR_INVALID;
    if (c->latL[stage].size() != c->tileCount || c->latCost[stage].size() != c->tileCount) return CRT_ERR_STATE;
    if (lanes) memcpy(lanes, c->latL[stage].data(), c->tileCount);
    if (cost) memcpy(cost, c->latCost[stage].data(), (size_t)c->tileCount * 4);
    return c->latStage;
}

extern "C" int crt_debug_tile_stamps(crt_ctx* c, uint64_t* out)
{
    if (!c || !out || !c->dTileClocks) return CRT_ERR_INVALID;
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipMemcpyAsync(out, c->dTileClocks + 2 * (size_t)c->tileCount, (size_t)c->tileCount * 128, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return CRT_OK;
}

int crt_bind_accumulator(crt_ctx* c, void* p)
{
    if (!c) return CRT_ERR_INVALID;
    if (p && ((uintptr_t)p & 15u)) return c->fail(CRT_ERR_INVALID, "accumulator pointer must be 16-byte aligned");
    HIPCK(c, hipSetDevice(c->cfg.device));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->dAcc = p ? p : c->dAccOwned;
    return CRT_OK;
}

int crt_accumulator_device_ptr(crt_ctx* c, void** p)
{
    if (!c || !p) return CRT_ERR_INVALID;
    *p = c->dAcc; return CRT_OK;
}

} // extern "C"
