// launch.h — the seam between the host (abi.cpp) and the device units (device/*.hip): every extern "C" launch wrapper and sizing helper a .hip file defines and
// abi.cpp calls, declared ONCE.  abi.cpp includes this header and so does every .hip file that defines one of these functions, so a definition that drifts from
// its declaration is a compile error ("conflicting types") instead of a transposed argument at run time; extern "C" symbols carry no types for the linker to check.
// Host-includable: no device code.  The by-value kernel argument structs (Scene, AltAccelDev, TlasAltDev, PrimDev) are layout.h's.
#pragma once
#include "layout.h"

#include <hip/hip_runtime.h>

extern "C" {

// ---- kernels.hip ----
hipError_t crt_launch_check_reciprocals(unsigned long long* out, hipStream_t stream);
hipError_t crt_launch_check_sqrt(unsigned long long* out, hipStream_t stream);
hipError_t crt_launch_render(const crt::Scene* sc, void* slab, crt::Counters* counters, unsigned long long* tileClocks, const uint32_t* tileOrder, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t ldsBytes, int collectStats, const uint32_t* blockDesc, uint32_t nBlocks, uint32_t* tileCost,
    uint32_t rankCount, unsigned long long* launchClk, hipStream_t stream);
uint32_t crt_render_resident_waves(int device, int kind, uint32_t ldsBytes);
size_t crt_slab_window_bytes(uint32_t tileCount, uint32_t passes);     // one 64-frame window of samples (sample_body.h slab_window_bytes)
hipError_t crt_launch_accumulate(const void* slab, void* acc, const uint32_t* tileOrder /* block -> local tile, or nullptr: the identity */,
    uint32_t texelFirst /* the blocks [texelFirst, tileCount) hold the texel form (a sky launch's ranks); tileCount: none */, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount,
    uint32_t tilesX, uint32_t W, uint32_t frames, uint32_t passes, hipStream_t stream);
// the layout test's host-only view of sample_body.h's position functions (crt_debug_slab_layout): pos[frame][tile][pixel][pass], sizes = {window, tile block} bytes
void crt_slab_layout_probe(int texel, uint32_t frames, uint32_t tileCount, uint32_t passes, unsigned long long* pos, unsigned long long* sizes);
hipError_t crt_launch_find_nearest(const crt::Scene* sc, const void* rays, void* hits, uint32_t n, crt::Counters* counters, uint32_t ldsBytes, uint32_t* cursor, hipStream_t stream);
hipError_t crt_launch_is_occluded(const crt::Scene* sc, const void* rays, int32_t* occluded, uint32_t n, uint32_t ldsBytes, uint32_t* cursor, hipStream_t stream);
hipError_t crt_launch_whitted(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, void* acc, uint32_t* pixels, crt::Counters* counters, uint32_t ldsBytes,
    hipStream_t stream);
size_t crt_whitted_inspect_work_bytes(uint32_t pixelCount);
hipError_t crt_launch_whitted_inspect(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, int inspect, int32_t peakIn, void* acc, uint32_t* pixels,
    crt::Counters* counters, int32_t* trav, int32_t* tested, void* work, uint32_t ldsBytes, hipStream_t stream);
uint32_t crt_trace_query_stack_words(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl);   // dwords per lane; four wavefronts share a workgroup's 64 KiB
hipError_t crt_launch_trace_query(const crt::Scene* sc, int accel, const crt::AltAccelDev* alt, const crt::TlasAltDev* tl, const void* rays, float* rgb, int32_t* trav /* or nullptr */,
    int32_t* tested /* or nullptr */, uint32_t n, crt::Counters* counters, uint32_t* cursor, uint32_t* residentLanes /* not nullptr: the lanes of a full launch, and no launch */,
    hipStream_t stream);
hipError_t crt_launch_resolve(const void* acc, uint32_t* pixels, float* tileSums, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t W, float scale,
    hipStream_t stream);
hipError_t crt_launch_commit_frame(const void* slabWindow, uint32_t frameInWindow, uint32_t passes, void* acc, uint32_t* pixels, float* tileSums, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t W, float scale, hipStream_t stream);

// ---- render_pool.hip (the crt_debug_pool_* entries exist only in builds with CRT_POOL_STAMPS / _DENS / _TIMELINE; the tools look them up by name) ----
uint32_t crt_pool_streams(uint32_t frames);
size_t crt_pool_scratch_bytes_per_window(uint32_t tileCount);
hipError_t crt_launch_render_pool(const crt::Scene* sc, void* slab, void* facScratch, crt::Counters* counters, unsigned long long* tileClocks, const uint32_t* tileOrder, uint32_t tileFirst,
    uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, int collectStats, uint32_t rankFirst,
    uint32_t rankEnd /* the launch renders the ranks [rankFirst, rankEnd) of tileOrder; tileCount stays the slab's */, uint32_t waveFrames,
    const uint32_t* waveTab /* tileCount - rankFirst entries */, uint32_t tabBlocks, uint32_t longFrames, uint32_t* tileCost, unsigned long long* launchClk,
    const uint8_t* tileClass /* one byte per local tile (layout.h kTileNo*), or nullptr: every test runs */, uint32_t extraLds /* unused LDS bytes per wavefront on top (tests) */,
    hipStream_t stream);
uint32_t crt_pool_lds_bytes(uint32_t stackDepth, uint32_t streams, uint32_t refBits /* Scene::poolRefBits: 16 or 32 */);
uint32_t crt_pool_lds_limit(int device);
int crt_debug_pool_stamps(unsigned long long* out, int reset);
int crt_debug_pool_density(unsigned long long* out, int reset);
size_t crt_debug_pool_timeline(unsigned long long* out, size_t cap);

// ---- render_sky.hip: the kTileSky tiles of a job, ranks [rankFirst, rankFirst + skyTiles) of tileOrder, one wavefront per (tile, 64-frame window) ----
hipError_t crt_launch_render_sky(const crt::Scene* sc, void* slab, crt::Counters* counters, const uint32_t* tileOrder, uint32_t rankFirst, uint32_t skyTiles, uint32_t tileFirst,
    uint32_t tileStride, uint32_t tileCount /* of the slab: all local tiles */, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes,
    int texels /* the tiles' blocks in the texel form (sample_body.h): the launch's accumulate must be told the same ranks */,
    unsigned long long* launchClk /* a measuring job: ~first start, last end (100 MHz), or nullptr */, hipStream_t stream);

// ---- render_seq.hip ----
uint32_t crt_probe_paths(void);
hipError_t crt_launch_probe(const crt::Scene* sc, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t* tileCost, hipStream_t stream);
hipError_t crt_launch_render_alt(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, hipStream_t stream);
hipError_t crt_launch_sample_query(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, const void* rays, uint32_t* seeds, float* rgb, uint32_t n,
    crt::Counters* counters, uint32_t* cursor, uint32_t* residentLanes, hipStream_t stream);
// crt_render_views (render_views.h): one launch renders the view-frames [jFirst, jFirst + nj) of a job of K x frames (jFirst a multiple of 64) into a slab of
// ceil(nj / 64) windows, cams = K records of twelve floats; crt_launch_views_accumulate sums that slab per view into the caller's images (outPixels may be nullptr)
hipError_t crt_launch_render_views(int accel, const crt::Scene* sc, const crt::AltAccelDev* acc, const crt::TlasAltDev* tl, const float* cams, void* slab, crt::Counters* counters,
    uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
// crt_render_poses (render_poses.h): crt_launch_render_views' launch with every lane's TLAS and Instance records taken from its view's pose in the table `pt` names;
// sc->stackDepth is the job's.  The per-view sums are crt_launch_views_accumulate's.
hipError_t crt_launch_render_poses(const crt::Scene* sc, const crt::PoseTableDev* pt, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
// crt_render_shapes (render_shapes.h, render_shapes.hip): the same launch with every lane's refitted BVH (and, two-level, its TLAS and Instance records) taken from its
// view's shape in the table `t` names; sc->stackDepth is the job's.  The per-view sums are crt_launch_views_accumulate's.
hipError_t crt_launch_render_shapes(const crt::Scene* sc, const crt::ShapeTableDev* t, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
// crt_render_shape_sets (render_shape_sets.h): the same with the instances that walk the lane's image named by the table's instRoot words; two-level scenes only
hipError_t crt_launch_render_shape_sets(const crt::Scene* sc, const crt::ShapeSetTableDev* t, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
// crt_render_looks (render_looks.h, render_looks.hip): the same launch with every lane's light quad, floor material, sky and Material records taken from its view's look
// in the table `lt` names (look_build.hip: the build of that table from the job's look records, and the check of the K view -> look indices; the caller sets the
// table's LookJobHeader to all ones on the stream first).  BVH / TLAS only.
hipError_t crt_launch_look_build(const crt::LookBuildDev* b, hipStream_t stream);
hipError_t crt_launch_render_looks(const crt::Scene* sc, const crt::LookTableDev* lt, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
hipError_t crt_launch_views_accumulate(const void* slab, float* outRgba, uint32_t* outPixels, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t W,
    uint32_t H, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, float scale, hipStream_t stream);

// ---- render_prim.hip ----
hipError_t crt_launch_render_views_prim(const crt::Scene* sc, const crt::PrimDev* p, const float* cams, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride,
    uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, hipStream_t stream);
hipError_t crt_launch_find_nearest_prim(const crt::PrimDev* p, const void* rays, void* hits, uint32_t n, hipStream_t stream);
hipError_t crt_launch_render_prim(const crt::Scene* sc, const crt::PrimDev* p, void* slab, crt::Counters* counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
    uint32_t sppFirst, uint32_t frames, uint32_t passes, hipStream_t stream);
hipError_t crt_launch_sample_query_prim(const crt::Scene* sc, const crt::PrimDev* p, const void* rays, uint32_t* seeds, float* rgb, uint32_t n, crt::Counters* counters, uint32_t* cursor,
    uint32_t* residentLanes, hipStream_t stream);
hipError_t crt_launch_probe_f64(int op, const void* in, void* out, uint32_t n, hipStream_t stream);

// ---- alt_accel.hip, tlas_alt.hip ----
hipError_t crt_launch_find_nearest_alt(int kind, const crt::Scene* sc, const crt::AltAccelDev* acc, const void* rays, void* hits, uint32_t n, uint32_t* cursor, hipStream_t stream);
hipError_t crt_launch_is_occluded_alt(int kind, const crt::Scene* sc, const crt::AltAccelDev* acc, const void* rays, int32_t* occluded, uint32_t n, uint32_t* cursor, hipStream_t stream);
hipError_t crt_launch_tlas_alt_query(int kind, bool occl, const crt::Scene* sc, const crt::TlasAltDev* tl, const void* rays, void* out, uint32_t n, uint32_t* cursor, hipStream_t stream);

// ---- shade_query.hip, refit.hip, probe.hip ----
hipError_t crt_launch_hit_info(const crt::Scene* sc, const void* rays, const void* hits, void* out, uint32_t n, uint32_t objects, uint32_t fileTris, hipStream_t stream);
hipError_t crt_launch_sky_color(const crt::Scene* sc, const void* rays, float* rgb, uint32_t n, hipStream_t stream);
hipError_t crt_launch_refit(char* geom, uint32_t leafOff, uint32_t pairBase, uint32_t triBase, uint32_t triCount, const float* pos, const void* plan, const uint32_t* levelOff, uint32_t levels,
    uint32_t rootCode, float* out, hipStream_t stream);
hipError_t crt_launch_probe_f32(int op, const void* in, void* out, uint32_t n, hipStream_t stream);
hipError_t crt_launch_probe_arith(int what, const void* in, uint32_t nIn, uint32_t n, uint32_t seed, uint32_t dumpAt, void* out, hipStream_t stream);

// ---- grid_build.hip ----
uint32_t crt_grid_build_blocks(int device);
size_t crt_grid_scan_chunks(uint32_t cells);
hipError_t crt_launch_grid_bounds(const float* pos, uint32_t triCount, crt::GridBuildState* state, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_grid_count(const float* pos, uint32_t triCount, const crt::GridParams* g, uint32_t cells, uint32_t* counts, unsigned long long* chunkSums, crt::GridBuildState* state,
    uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_grid_fill(const float* pos, uint32_t triCount, const crt::GridParams* g, uint32_t cells, const uint32_t* cellStart, uint32_t* cursor, int32_t* unsorted, int32_t* refs,
    uint32_t total, const char* geom, uint32_t leafOff, uint32_t triBase, int globalIdx, crt::AltTri* tris, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_alt_tris(const float* pos, uint32_t triCount, const char* geom, uint32_t leafOff, uint32_t triBase, int globalIdx, crt::AltTri* tris, hipStream_t stream);

// ---- kd_build.hip ----
size_t crt_kd_scan_chunks(uint32_t n);
hipError_t crt_launch_kd_begin(const float* pos, uint32_t triCount, crt::KdBuildState* state, float* triBox, crt::KdBuildNode* root, uint32_t* refs, uint32_t* owner, uint32_t maxBlocks,
    hipStream_t stream);
hipError_t crt_launch_kd_level(crt::KdBuildNode* nodes, uint32_t nodeCount, uint32_t depth, const uint32_t* owner, const uint32_t* refs, uint32_t refCount, const float* triBox,
    unsigned long long* nodeItems, unsigned long long* refItems, unsigned long long* chunkSums, crt::KdBuildState* state, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_kd_split(crt::KdBuildNode* nodes, uint32_t nodeCount, const unsigned long long* nodeScan, const uint32_t* owner, const uint32_t* refs, uint32_t refCount,
    const unsigned long long* refScan, crt::KdBuildNode* next, uint32_t nextNodes, uint32_t* nextRefs, uint32_t* nextOwner, uint32_t nextRefCount, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_kd_finalise(crt::KdBuildNode* const* nodes, const uint32_t* const* refs, const uint32_t* const* owner, const uint32_t* nodeCount, const uint32_t* refCount, uint32_t levels,
    crt::KdNode* outNodes, uint32_t outNodeCount, uint32_t* outRefs, uint32_t outRefCount, uint32_t maxBlocks, hipStream_t stream);

// ---- bvh_build.hip ----
hipError_t crt_launch_bvh_begin(const float* pos, uint32_t triCount, const char* geom, uint32_t leafOff, uint32_t triBase, float* cen, uint32_t* idx, uint32_t* owner, int32_t* objOf,
    crt::BvhBuildNode* root, unsigned long long* rootKeys, crt::BvhBuildState* state, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_bvh_level(const float* pos, const float* cen, const uint32_t* idx, const uint32_t* owner, uint32_t triCount, crt::BvhBuildNode* nodes, unsigned long long* keys,
    uint32_t m, uint32_t* bins, uint32_t* leftItems, uint32_t* nodeItems, unsigned long long* chunkSums, crt::BvhBuildState* state, int isRoot, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_bvh_split(crt::BvhBuildNode* nodes, uint32_t m, const uint32_t* splitScan, const uint32_t* owner, const uint32_t* idx, const uint32_t* leftScan, uint32_t triCount,
    crt::BvhBuildNode* next, unsigned long long* nextKeys, uint32_t nextM, uint32_t* idxOut, uint32_t* ownerOut, uint32_t* remain, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_bvh_flatten(crt::BvhBuildNode* nodes, const uint32_t* levelOff, uint32_t levels, const float* pos, const uint32_t* idx, const uint32_t* remain, const int32_t* objOf,
    uint32_t triCount, const crt::BvhFlatten* F, char* geom, uint32_t maxBlocks, hipStream_t stream);
hipError_t crt_launch_bvh_relocate(const char* oldGeom, char* geom, const crt::BvhRelocate* R, uint32_t instOff, uint32_t blasCount, uint32_t bvh, uint32_t rootRef, uint32_t rootRef16,
    uint32_t maxBlocks, hipStream_t stream);

// ---- tlas_build.hip ----
hipError_t crt_launch_tlas_build(const char* geom, uint32_t instOff, const float* T, const float* rootBox, uint32_t blasCount, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits,
    void* out, hipStream_t stream);
// P such builds in one launch, one workgroup each, over T + 16 blasCount p into header p / image p of a pose table (layout.h PoseJobHeader), and the check of the K
// view -> pose indices (viewPose may be nullptr); the caller sets PoseJobHeader::badView to kPoseNoBadView on the stream first
hipError_t crt_launch_tlas_build_poses(const char* geom, uint32_t instOff, const float* T, const float* rootBox, uint32_t blasCount, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits,
    void* table, uint32_t imagesOff, uint32_t imageStride, uint32_t P, const int32_t* viewPose, uint32_t K, hipStream_t stream);
// S such builds, each from its own row of node-0 boxes, into the pose images of a shape table (layout.h ShapeJobHeader); posesOff: the first image's pose image
hipError_t crt_launch_tlas_build_shapes(const char* geom, uint32_t instOff, const float* T, const float* rootBoxRows, uint32_t blasCount, uint32_t pairRel, uint32_t instRel,
    uint32_t poolRefBits, void* table, uint32_t headsOff, uint32_t posesOff, uint32_t imageStride, uint32_t S, hipStream_t stream);

// ---- shape_build.hip ----
// crt_render_shapes: BVH::Refit of one BVH for b->S sets of positions into the images of a shape table, the rows of node-0 boxes, and the check of the K view -> shape
// indices (viewShape may be nullptr); the caller sets ShapeJobHeader::badView to kPoseNoBadView on the stream first.  plan / levelOff / levels / rootCode: crt_launch_refit's
hipError_t crt_launch_shape_build(const crt::ShapeBuildDev* b, const void* plan, const uint32_t* levelOff, uint32_t levels, uint32_t rootCode, const int32_t* viewShape, uint32_t K,
    hipStream_t stream);
// crt_render_shape_sets: the same for b->M BVHs of a two-level scene per shape, in one leaf launch and one box launch of a workgroup per (shape, mesh).  meshes / instRoot:
// the host's copy of the two tables the caller has enqueued to b->meshOff / b->instRootOff of the table (layout.h ShapeSetMesh)
hipError_t crt_launch_shape_set_build(const crt::ShapeSetBuildDev* b, const crt::ShapeSetMesh* meshes, const uint32_t* instRoot, const int32_t* viewShape, uint32_t K, hipStream_t stream);

// abi.cpp's test switch CRT_DEBUG_QUERY_GRID=<k>: an upper bound on the workgroups of a persistent query launch (0: none).  Host side only: each wrapper passes its grid through it.
uint32_t crt_debug_query_grid(void);

} // extern "C"

namespace crt {

inline uint32_t bounded_query_grid(uint32_t grid) { const uint32_t k = crt_debug_query_grid(); return (k != 0u && k < grid) ? k : grid; }

// ---- the launch geometry of the persistent find-nearest / is-occluded kernels (kernels.hip, alt_accel.hip, tlas_alt.hip), one wavefront per workgroup ----
// Workgroups of a launch over n rays whose wavefronts take ldsBytes of LDS each: the device filled several times over (they hide each other's fetch latency), never more than the rays need.
// 4 wavefronts per SIMD, LDS stacks permitting (measured: 8 per SIMD is no faster for the grid and 17 % slower for the BVH), on the MI355X's 256 CUs.
inline uint32_t query_grid(uint32_t n, uint32_t ldsBytes)
{
    uint32_t perCu = ldsBytes ? (160u * 1024u) / ldsBytes : 16u; if (perCu > 16u) perCu = 16u; if (perCu < 4u) perCu = 4u;
    const uint32_t need = (n + 63u) / 64u, fill = 256u * perCu;
    return bounded_query_grid(need < fill ? need : fill);
}

// What the wrappers do before such a launch: nothing for no rays; the ray cursor the lanes draw from must exist and is zeroed on the stream, ahead of the kernel.
// true: launch.  false: return *status (hipSuccess for n == 0).
inline bool query_launch_begin(uint32_t n, uint32_t* cursor, hipStream_t stream, hipError_t* status)
{
    *status = hipSuccess;
    if (n == 0) return false;
    if (!cursor) { *status = hipErrorInvalidValue; return false; }
    if (hipMemsetAsync(cursor, 0, 4, stream) != hipSuccess) { *status = hipGetLastError(); return false; }
    return true;
}

} // namespace crt
