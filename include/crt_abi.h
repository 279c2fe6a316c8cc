/*
 * crt_abi.h — C ABI of the MI355X path-tracing back end (libcrt_amd.so).
 *
 * The reference (willake/cpu-ray-tracer) has no plugin/FFI seam: the path tracer is compiled into the
 * application.  The two seams it does have are
 *     upper:  TheApp::Init / Tick(float) and the public Renderer members (accumulator, spp, passes, energy, …)
 *             — template/precomp.h:344-361, "3. PathTracer/renderer.h":27-53
 *     lower:  BaseScene::FindNearest / GetHitInfo / GetSkyColor and the public members of the accel classes
 *             (bvhNodes, triangles, triangleIndices, nodesUsed, T, invT, blas) — infra/scene/base_scene.h:16-32,
 *             infra/bvh.h:37-43, infra/blas_bvh.h:48-57, infra/tlas_bvh.h:27-31
 * This header is what a binding behind those seams calls.  The host application keeps loading scenes and
 * building the SAH-BVH / TLAS on the CPU exactly as today; it hands the BUILT arrays (reference layouts,
 * borrowed pointers, copied during the call) to crt_upload_scene once, and replaces the body of
 * Renderer::Tick's tile loop by crt_render.  INTEGRATION.md shows the binding.
 *
 * Conventions: every function returns 0 on success or a negative crt_status; no function throws or exits
 * (the reference's FatalError/exit and std::runtime_error — template/opencl.cpp:14-27, infra/blas_bvh.cpp:11-14 —
 * become error codes + crt_last_error).  Plain pointers and sizes only; no C++ or torch types.
 * One host thread drives one ctx; work is asynchronous on the ctx's HIP stream until crt_sync / a read.
 */
#ifndef CRT_ABI_H
#define CRT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 3

typedef enum crt_status {
    CRT_OK = 0,
    CRT_ERR_INVALID = -1,      /* bad argument / inconsistent scene description            */
    CRT_ERR_DEVICE = -2,       /* HIP runtime error (message in crt_last_error)            */
    CRT_ERR_NO_DEVICE = -3,    /* no gfx950 device visible: the product never falls back to a CPU path */
    CRT_ERR_UNSUPPORTED = -4,  /* valid input outside this build's limits (stated in the message) */
    CRT_ERR_STATE = -5,        /* call order (e.g. render before upload)                   */
    CRT_ERR_IO = -6            /* host loader: file missing / malformed                    */
} crt_status;

typedef struct crt_ctx crt_ctx;

/* ---- reference record layouts (bit-compatible with the reference structs) ------------------------- */

/* BVHNode — infra/blas_bvh.h:13-20 (32 bytes).  Leaf iff triCount > 0; children at leftFirst, leftFirst+1. */
typedef struct crt_bvh_node { float aabbMin[3], aabbMax[3]; uint32_t leftFirst, triCount; } crt_bvh_node;

/* Tri — infra/helper.h:6-26 (112 bytes AoS). */
typedef struct crt_tri {
    float vertex0[3], vertex1[3], vertex2[3];
    float normal0[3], normal1[3], normal2[3];
    float uv0[2], uv1[2], uv2[2];
    float centroid[3];
    int32_t objIdx;
} crt_tri;

/* TLASBVHNode — infra/tlas_bvh.h:7-14 (32 bytes).  Leaf iff leftRight == 0; children = lo/hi 16 bits. */
typedef struct crt_tlas_node { float aabbMin[3]; uint32_t leftRight; float aabbMax[3]; uint32_t BLAS; } crt_tlas_node;

/* Texture — template/texture.h:15-48: 0x00RRGGBB texels, row 0 = top of the image. */
typedef struct crt_texture { const uint32_t* pixels; int32_t width, height; } crt_texture;

/* Material — template/material.h:6-46.  texture = index into crt_scene_desc.textures or -1. */
typedef struct crt_material { float reflectivity, refractivity; float absorption[3]; int32_t texture; } crt_material;

/* One acceleration structure: BVH (infra/bvh.h) for CRT_SCENE_FILE, BLASBVH (infra/blas_bvh.h) for CRT_SCENE_TLAS. */
typedef struct crt_bvh {
    const crt_bvh_node* nodes;         /* bvhNodes.data()                                              */
    uint32_t nodesUsed;                /* nodesUsed (root = 0, node 1.. allocated pairwise)            */
    const crt_tri* triangles;          /* triangles.data()                                             */
    uint32_t triCount;                 /* triangles.size()                                             */
    const uint32_t* triangleIndices;   /* triangleIndices.data()                                       */
    int32_t objIdx;                    /* BLASBVH::objIdx (hit id written by IntersectTri); ignored for CRT_SCENE_FILE */
    int32_t matIdx;                    /* BLASBVH::matIdx; ignored for CRT_SCENE_FILE                  */
    float T[16], invT[16];             /* BLASBVH::T / invT, row-major mat4; ignored for CRT_SCENE_FILE */
} crt_bvh;

typedef enum crt_scene_kind { CRT_SCENE_FILE = 0 /* FileScene, USE_BVH */, CRT_SCENE_TLAS = 1 /* TLASFileScene, TLAS_USE_BVH */ } crt_scene_kind;

typedef struct crt_scene_desc {
    int32_t kind;
    const crt_bvh* bvhs; uint32_t bvhCount;              /* FILE: exactly 1 (FileScene::acc); TLAS: tlas.blas[]            */
    const crt_tlas_node* tlasNodes; uint32_t tlasNodeCount; /* TLAS only: tlasNode[0 .. 2*blasCount)                         */
    const int32_t* objMatIdx; uint32_t objCount;         /* FILE only: models[i]->matIdx for object id i+2                 */
    const crt_material* materials; uint32_t materialCount;
    const crt_texture* textures; uint32_t textureCount;
    int32_t floorTexture;                                /* primitiveMaterials[1].textureDiffuse (index into textures)      */
    int32_t skyTexture;                                  /* skydome                                                          */
    float lightT[16], lightInvT[16], lightSize;          /* Quad light (template/primitives.h:321-375): T, invT, size       */
    float floorN[3], floorD, floorInvto;                 /* Plane floor (primitives.h:100-179): N, d, invto                 */
} crt_scene_desc;

typedef struct crt_config {
    int32_t width, height;       /* SCRWIDTH / SCRHEIGHT (template/camera.h:4-5)                                      */
    int32_t depthLimit;          /* Renderer::depthLimit (renderer.h:53), default 5                                   */
    int32_t device;              /* HIP device ordinal                                                                  */
    /* image tiles owned by this ctx: tile = tileFirst + i*tileStride, i in [0, tileCount); tileCount < 0 = all.
     * Tiles are numbered x-major as in Renderer::Tick (renderer.cpp:151-152).  Other pixels are never touched. */
    int32_t tileFirst, tileStride, tileCount;
    int32_t maxFramesPerLaunch;  /* frames rendered per kernel launch; 0 = default (4096 = 64 windows of 64 frames, one wavefront
                                    per (tile, window)); values > 64 are rounded down to whole windows; the sample-slab pool
                                    (at most half of the free HBM) may lower it                                            */
    int32_t collectStats;        /* !=0: kernels also count node iterations / triangle tests / BLAS visits / mesh hits   */
    int32_t renderStreams;       /* HIP streams the render launches rotate over, so that independent launches (consecutive crt_render
                                    calls, or the pieces of one long call) overlap on the GPU; 0 = default (7), 1 = one at a time */
} crt_config;

typedef struct crt_ray { float O[3]; float D[3]; int32_t inside; } crt_ray;
typedef struct crt_hit {
    float t; float u, v; int32_t objIdx; int32_t triIdx;
    int32_t traversed;   /* node iterations, as Ray::traversed (bvh.cpp:231, tlas_bvh.cpp:89)                      */
    int32_t tested;      /* triangle tests over the whole query                                                     */
} crt_hit;

typedef struct crt_counters {
    uint64_t rays;            /* FindNearest calls = primary + secondary rays                                       */
    uint64_t primary;
    uint64_t interior_iters;  /* I   (valid when collectStats)                                                      */
    uint64_t leaf_iters;
    uint64_t tri_tests;       /* T                                                                                   */
    uint64_t tlas_iters;
    uint64_t blas_visits;     /* V                                                                                   */
    uint64_t mesh_hits;       /* H                                                                                   */
} crt_counters;

typedef struct crt_timing {                /* covers every launch since the previous crt_get_timing call                       */
    float render_kernel_ms;   /* Σ duration of the path-tracing kernel launches (HIP events on the stream each was launched on; launches on
                                 different render streams overlap, so this sum can exceed wall time)                 */
    float resolve_kernel_ms;  /* Σ duration of the ordered accumulate kernels                                        */
    uint32_t render_launches; /* number of path-tracing kernel launches                                              */
    uint32_t pool_launches;   /* ... of which render_pool_kernel (stream pool; the others are render_tiles_kernel)   */
    uint32_t split_launches;  /* ... of which split: the most expensive tiles by a concurrent render_tiles_kernel    */
    uint32_t reserved;
} crt_timing;

/* ---- life cycle ----------------------------------------------------------------------------------- */
int  crt_abi_version(void);
int  crt_device_count(void);                                   /* number of visible HIP devices (0 = none)          */
int  crt_create(crt_ctx** out, const crt_config* cfg);
void crt_destroy(crt_ctx* ctx);
const char* crt_last_error(crt_ctx* ctx);                      /* ctx may be NULL: error of the last failed crt_create on this thread */

/* ---- scene / camera (lower seam) -------------------------------------------------------------------- */
/* Flattens to the device layout and copies; host pointers are not kept.  The node references the stream-pool render kernel walks are written 16 bits wide
 * when the scene has <= 16382 node pairs and <= 16382 triangles over all its BVHs, 32 bits wide otherwise; the stream-pool kernel can render the scene either way
 * (which kernel does: see crt_render), and the in-place writes (crt_update_scene, crt_refit_device, crt_update_transforms_device, crt_build_grid_device) keep the width. */
int  crt_upload_scene(crt_ctx* ctx, const crt_scene_desc* scene);
/* In-place update of an uploaded scene for animation (renderer.cpp:147 `animating`), same description as at upload, same topology:
 *   CRT_UPDATE_TRANSFORMS  two-level scenes: every BLAS's T / invT as BLASBVH::SetTransform left them (blas_bvh.cpp:363-374) and the node array of the
 *                          TLASBVH::Build that followed (tlas_bvh.cpp:17-55) — instance motion;
 *   CRT_UPDATE_BOUNDS      every BVH's node boxes and triangle vertices as BVH::Refit / BLASBVH::Refit left them (bvh.cpp:26-43; node / triangle counts,
 *                          child indices and triangleIndices unchanged) and, for two-level scenes, the rebuilt TLAS.
 * Only the affected sections of the device geometry buffer are rewritten (a few KB for transforms): no device allocation, no host wait for the GPU;
 * frames submitted earlier still see the old scene, frames submitted later the new one. */
#define CRT_UPDATE_TRANSFORMS 1u
#define CRT_UPDATE_BOUNDS     2u
int  crt_update_scene(crt_ctx* ctx, const crt_scene_desc* scene, uint32_t what);
/* A LOOK: everything of an uploaded triangle scene's appearance that can change without touching geometry or texels, as one block of 4-byte words (so it can live in
 * a host array or in a device tensor): a crt_look_header — the light quad and the floor / skydome texture, the crt_scene_desc members of the same names, same meaning
 * and units, invT supplied by the caller exactly as at upload — followed by materialCount crt_material records (six words each), materialCount being the uploaded
 * scene's.  A look SELECTS AMONG THE UPLOADED TEXTURES BY INDEX (materials: -1 = untextured); texels are never part of a look.  crt_look_words(materialCount) is the
 * stride of an array of looks, in words.  ABI version 3 still: additions, detected by symbol.
 * lightT must be rigid (rotation and translation) and lightInvT its FastInvertedTransformNoScale, as at upload; anything else is the caller's error. */
typedef struct crt_look_header { float lightT[16], lightInvT[16], lightSize; int32_t floorTexture, skyTexture; uint32_t pad; } crt_look_header;
#define CRT_LOOK_HEADER_WORDS   36u
#define CRT_LOOK_MATERIAL_WORDS 6u
uint32_t crt_look_words(uint32_t materialCount);               /* CRT_LOOK_HEADER_WORDS + CRT_LOOK_MATERIAL_WORDS * materialCount */
/* In-place change of the live scene's look (CRT_SCENE_FILE and CRT_SCENE_TLAS): a material sweep, relighting, a moving light, without the re-flatten, re-allocation and
 * synchronising copy of crt_upload_scene.  Rewrites the device Material records, the floor material, the sky words and the light block (and what derives from it: the
 * camera-relative block, the tile classes, the dispatch order and the planner / probe state a camera change also invalidates).  Afterwards every entry that shades —
 * crt_render through either render kernel and through crt_set_render_accel, crt_tick, crt_whitted_tick, crt_sample*, crt_trace*, crt_get_hit_info*,
 * crt_get_sky_color*, crt_get_light — gives bit for bit what a fresh crt_upload_scene of the same description with that look gives (followed by the same
 * alternative-accelerator uploads).  The KD-tree / grid structures are kept: they hold no appearance.  Frames crt_tick rendered ahead are dropped.
 * Ordering, as crt_update_scene: the Material records are rewritten on the context's stream behind every launch submitted earlier that may read them (renders,
 * frames rendered ahead, queries on any stream), so those still see the old look, and every launch submitted later sees the new one; no device allocation, no host
 * wait for the GPU beyond what CRT_UPDATE_TRANSFORMS has (a pinned staging buffer's previous copy).
 * Refused with nothing modified: no scene CRT_ERR_STATE; a PrimitiveScene CRT_ERR_UNSUPPORTED; look NULL, floorTexture / skyTexture outside [0, textureCount), a
 * material's texture outside [-1, textureCount) CRT_ERR_INVALID (crt_last_error names the field). */
int  crt_update_look(crt_ctx* ctx, const void* look /* crt_look_words(materialCount) words, host */);
/* BVH::Refit / BLASBVH::Refit (bvh.cpp:26-61) of ONE uploaded BVH on the device, from vertex positions that already live in device memory (skinning, a cloth step,
 * an optimiser over vertices): no copy of the positions to the host, no CPU refit, no staging of the geometry sections.  ABI version 3 still: an addition,
 * detected by symbol.  d_positions = vertex0, vertex1, vertex2 of every triangle in the reference's triangles[] order (9 floats each; the array
 * crt_host_scene_bvh_move_and_refit takes), device memory of cfg.device (checked as the device query entries check theirs); `stream` as there, NULL = the ctx's.
 * Works on CRT_SCENE_FILE (bvh = 0) and on every BLAS of a CRT_SCENE_TLAS scene.  What it leaves on the device is exactly what Refit followed by
 * crt_update_scene(CRT_UPDATE_BOUNDS) leaves for that BVH, bit for bit: every leaf triangle gets vertex0, vertex1 - vertex0, vertex2 - vertex0; every node box is
 * what the reference's backward loop gives, INCLUDING ITS QUIRK that node 1 is skipped (`if (i != 1)`, bvh.cpp:28): the root's left child keeps the box it had,
 * and that stale box still feeds node 0's.  Normals, uvs, materials, references and the leaf order stay (Refit touches none of them).
 * rootBox (may be NULL) receives node 0's refitted aabbMin, aabbMax.  Two-level scenes: the call does NOT rebuild the TLAS (neither does BLASBVH::Refit); the caller
 * either
 * calls crt_update_transforms_device next, which rebuilds the TLAS on the device from the refitted node-0 box with nothing from the host in between, or puts rootBox
 * into its BLAS's node 0, runs SetTransform + TLASBVH::Build on the host as after any Refit and sends the result with crt_update_scene(CRT_UPDATE_TRANSFORMS) —
 * rootBox is what makes the host route possible without reading the device.  (crt_host_scene_bvh_refit_device takes the host route.)
 * Ordering, as crt_update_scene and the device queries: the refit kernels run on `stream` behind every launch submitted earlier that reads the geometry (renders,
 * frames rendered ahead, queries on any stream), so earlier renders still see the old scene; every launch submitted later waits for the refit.  THE ONE HOST WAIT:
 * the root's child pair travels in the kernel arguments of the render launches, so the call reads that pair and node 0's box back (88 bytes, pinned) and returns
 * once they have landed — it waits for `stream` up to the refit (and so for the earlier readers the refit is ordered behind), for nothing submitted later.
 * Like CRT_UPDATE_BOUNDS it drops a two-level scene's KD-tree / grid sets (crt_build_kdtree_device / crt_build_grid_device of the refitted BLAS bring them back) and
 * the frames crt_tick rendered ahead.
 * Refused with nothing modified: no scene (CRT_ERR_STATE), a PrimitiveScene (CRT_ERR_UNSUPPORTED), bvh out of range, triCount different from the uploaded BVH's,
 * d_positions NULL / a host pointer / memory of another device, a stream of another device (CRT_ERR_INVALID).  The caller's host arrays of that BVH (and a later
 * CRT_UPDATE_BOUNDS built from them) are its own business: an update rewrites both sections from whatever it is given. */
int  crt_refit_device(crt_ctx* ctx, uint32_t bvh, const float* d_positions /* 9 * triCount, device */, uint32_t triCount, void* stream,
                      float rootBox[6] /* out: node 0's aabbMin, aabbMax; may be NULL */);
/* Instance motion of a two-level scene from transforms that already live in device memory (a physics step, an optimiser over poses): BLASBVH::SetTransform for
 * EVERY BLAS (blas_bvh.cpp:363-374) and the TLASBVH::Build that follows (tlas_bvh.cpp:17-70), on the device, in one kernel launch.  ABI version 3 still: an
 * addition, detected by symbol.  d_T[16 i .. 16 i + 15] = BLASBVH::T of BLAS i, a row-major mat4 as crt_bvh.T; only cells 0..11 are read; no scale (as
 * FastInvertedTransformNoScale assumes); device memory of cfg.device, 4-byte aligned, checked as the device query entries check theirs; `stream` as there.
 * What the call leaves on the device is exactly what crt_host_scene_set_transform for every BLAS followed by crt_update_scene(CRT_UPDATE_TRANSFORMS) leaves, byte
 * for byte: the Instance records' T / invT rows, the TLAS nodes, the TLAS child pairs, the root reference and pair, the stack depth.  The world box of BLAS i is
 * grown from the node-0 box of BLAS i AS THE DEVICE HOLDS IT: the one uploaded, sent by the last CRT_UPDATE_BOUNDS, or refitted by crt_refit_device — so
 * crt_refit_device followed by this call needs no value from the host in between.  The build keeps the reference's quirks (FindBestMatch's first strict minimum
 * below 1e30f; the list shortened before the search that follows a merge, so that the new node can meet its own copy).
 * tlasOut (may be NULL) receives TLASBVH::tlasNode[0 .. 2 * blasCount) in the reference layout, byte for byte.
 * Ordering: the build runs on `stream` into scratch of the context's.  THE ONE HOST WAIT, as crt_refit_device's: the root's pair and the stack depth travel in the
 * kernel arguments of later launches, so the call reads the result back (status, height, the TLAS and Instance sections: 64 KB at most, pinned) and returns once
 * that has landed.  Only a build that passed every check is then copied into the geometry buffer, on `stream`, behind every launch submitted earlier that reads
 * the geometry (renders, frames rendered ahead, queries on any stream: they still see the old scene); every launch submitted later waits for the copy.
 * Otherwise as CRT_UPDATE_TRANSFORMS: frames crt_tick rendered ahead are dropped, KD-tree / grid BLAS sets are kept (they live in object space).
 * Refused with nothing modified: no scene (CRT_ERR_STATE); a CRT_SCENE_FILE scene (CRT_ERR_INVALID); a PrimitiveScene (CRT_ERR_UNSUPPORTED); blasCount different
 * from the uploaded bvhCount, d_T NULL / misaligned / a host pointer / memory of another device, a stream of another device (CRT_ERR_INVALID); a TLAS whose
 * traversal stack exceeds the LDS budget (CRT_ERR_UNSUPPORTED, as crt_update_scene); a build in which FindBestMatch finds no candidate while more than one node is
 * open — the reference's list[-1], reached with non-finite transforms or boxes of area >= 1e30 (CRT_ERR_INVALID; crt_last_error names the FindBestMatch call);
 * a scene uploaded with more than 2 * bvhCount TLAS nodes (CRT_ERR_UNSUPPORTED). */
int  crt_update_transforms_device(crt_ctx* ctx, const float* d_T /* 16 * blasCount, device */, uint32_t blasCount, void* stream,
                                  crt_tlas_node* tlasOut /* host, 2 * blasCount; may be NULL */);
/* Grid::Build / BLASGrid::Build (infra/grid.cpp:4-50) for ONE uploaded BVH's triangle array on the device, from vertex positions that already live in device memory:
 * the uniform grid rebuilt from scratch, so that the structures that have no Refit follow deforming geometry without a host round trip.  ABI version 3 still: both
 * entries are additions, detected by symbol.  d_positions is the array crt_refit_device takes (vertex0, vertex1, vertex2 per triangle, the reference's triangles[]
 * order); the pointer and `stream` are checked as there.  What the call leaves on the device equals, byte for byte, what Grid::Build over those triangles followed by
 * crt_upload_alt_accel / crt_upload_blas_accel would leave: resolution, cellSize, gridMin / gridMax (signed zeros as the reference's _mm_min_ps / _mm_max_ps fold
 * leaves them: of -0 and +0 tying for an extreme, the last in (triangle, vertex) order), cellStart (x-major cells, prefix array), cellRefs with every cell's triangle
 * indices ascending, and the triangle records (v0, v1 - v0, v2 - v0; the ids a hit reports are the uploaded scene's).  A rebuilt grid has the quality of a fresh build.
 * CRT_SCENE_FILE (bvh = 0): works with or without an earlier crt_upload_alt_accel(CRT_ACCEL_GRID); the grid becomes the scene's CRT_ACCEL_GRID structure and
 * crt_set_render_accel(CRT_ACCEL_GRID) stays selected (the per-frame loop is refit, rebuild, render).  The KD-tree shares the triangle records and its boxes belong to
 * the old positions, so a successful call marks it absent: a query with CRT_ACCEL_KDTREE is CRT_ERR_STATE, crt_set_render_accel goes back to 0 if it named the KD-tree.
 * CRT_SCENE_TLAS (bvh = a BLAS): needs a grid set uploaded earlier through crt_upload_blas_accel(CRT_ACCEL_GRID, ..), else CRT_ERR_STATE (its buffers are still held
 * after a refit dropped the set; the other BLASes' parts are carried over device to device, the descriptors re-based).  The context keeps a "grid current" flag per
 * BLAS: an upload sets all, CRT_UPDATE_BOUNDS clears all, crt_refit_device(b) clears b's, this call sets b's; the grid set is live iff every flag is set.  So after a
 * refit of BLAS b the set is dropped exactly as before, and is live again (queries; crt_set_render_accel must be called again) once crt_build_grid_device(b) has run.
 * The KD set has flags of its own and is brought back by crt_build_kdtree_device.  The test of crt_upload_blas_accel that the grid's bounds equal the BVH root box is not applied: after Refit node 0's box legitimately
 * differs from the true bounds (node 1 is skipped).  THE CALL TOUCHES NEITHER THE BVH, THE INSTANCES NOR THE TLAS: on a two-level scene the caller runs
 * crt_refit_device (+ crt_update_transforms_device) for the same positions, otherwise the TLAS boxes cull for the old geometry.
 * Ordering, as crt_refit_device / crt_update_transforms_device: the build runs on `stream` into buffers of its own; the grid it replaces keeps answering for
 * everything enqueued earlier, on any stream, and everything submitted later sees the new one.  Retired buffers are freed by a later call, once an event recorded
 * behind their last readers (the earlier launches and this build's own copies out of the old set) has completed.  Freeing them, and growing the build's scratch for
 * a larger grid than any before, goes through hipFree, which may synchronise the whole device: such a call can also wait for work submitted after the earlier build.
 * The promise "nothing submitted later is waited for" is that of the two waits below.  THE TWO HOST WAITS: the call reads the bounds back (the host computes resolution / cellSize from them, with the code the
 * host build uses) and then the total reference count (the host sizes cellRefs from it); each waits for `stream` up to that point, for nothing submitted later.
 * Refused with nothing modified, the previous grid still answering: no scene (CRT_ERR_STATE); a PrimitiveScene (CRT_ERR_UNSUPPORTED); bvh out of range, triCount
 * different from the uploaded BVH's, d_positions NULL / a host pointer / memory of another device, a stream of another device, a non-finite position component
 * (found by the bounds pass) (CRT_ERR_INVALID); more than 2^31-1 cell references (CRT_ERR_UNSUPPORTED); a failed device allocation (CRT_ERR_DEVICE).
 * Cost: a cell's references are sorted by rank, quadratic in the cell's length, one wavefront per cell of more than 32.  A FLAT mesh (cloth at rest, a ground plane: an
 * extent of 0 on an axis) gets resolution (1, 1, 1) from Grid::Build, so ALL its triangles are one cell: about n^2 / 64 steps per lane of a single wavefront — 10 k
 * triangles a few milliseconds, 100 k about 1.6e8 steps (seconds), 1 M minutes of one kernel.  Such a grid is useless for traversal too (every ray tests every
 * triangle); build those on the host or keep them on the BVH.  Meshes with volume have about 5 references per cell and do not meet this. */
int  crt_build_grid_device(crt_ctx* ctx, uint32_t bvh, const float* d_positions /* 9 * triCount, device */, uint32_t triCount, void* stream);
/* The live grid of a FileScene (bvh = 0) or of one BLAS of a two-level scene's set, uploaded or device-built: sizes first (any output may be NULL), then the arrays
 * where the pointers are non-NULL (cellStart: cellCount + 1 entries, cellRefs: refCount).  Synchronous (it waits for a device build still running).  CRT_ERR_STATE
 * when there is no live grid; bvh out of range is CRT_ERR_INVALID.  What lets a caller keep a host mirror of a device-built grid. */
int  crt_get_grid(crt_ctx* ctx, uint32_t bvh, int32_t res[3], float cellSize[3], float gridMin[3], float gridMax[3], uint32_t* cellCount, uint32_t* refCount,
                  uint32_t* cellStart /* cellCount + 1, or NULL */, int32_t* cellRefs /* refCount, or NULL */);
int  crt_set_camera(crt_ctx* ctx, const float camPos[3], const float topLeft[3], const float topRight[3], const float bottomLeft[3]);
                                                                /* Camera members used by GetPrimaryRay (camera.h:23-30) */

/* ---- rendering (upper seam: the tile loop of Renderer::Tick) --------------------------------------- */
/* Renders `frames` consecutive Ticks: frame k uses spp = spp_first + k*passes for its tile seeds
 * (renderer.cpp:120,167) and adds passes samples per pixel into the accumulator in frame order.
 * Asynchronous: the call is cut into launches of up to cfg.maxFramesPerLaunch frames (one grid covers all their 64-frame windows);
 * launches rotate over cfg.renderStreams HIP streams and overlap with those of earlier crt_render calls; the accumulation order
 * is kept by events.  crt_sync / any read waits for everything.
 * Which kernel renders a launch — same samples either way: a scene with 16-bit node references (crt_upload_scene) gets render_pool_kernel (128 RNG streams per
 * wavefront) for launches of many windows and render_tiles_kernel (one stream per lane) for smaller ones.  A scene with 32-bit node references gets
 * render_tiles_kernel at every size: the pool kernel's 32-bit instantiation (4-byte traversal-stack entries, (stack depth + 1) * 128 bytes more LDS per
 * wavefront) renders it too, but measured no faster on the scene the default was decided on (faster on others: DESIGN.md section 5), and runs only where the diagnostic switch CRT_RENDER_KERNEL=pool_always asks for it.
 * A scene whose pool wavefront would need more LDS than a workgroup may have is rendered by render_tiles_kernel whatever the switch says.
 * crt_timing.pool_launches counts pool launches of either width. */
int  crt_render(crt_ctx* ctx, uint32_t spp_first, uint32_t frames, uint32_t passes);
int  crt_sync(crt_ctx* ctx);
/* Optional: sizes the device-side sample-slab pool for an upcoming crt_render(.., frames, passes) now (allocating tens of GB takes
 * seconds and synchronises the device; without this call the first crt_render that needs a larger pool pays for it). */
int  crt_reserve(crt_ctx* ctx, uint32_t frames, uint32_t passes);
int  crt_clear(crt_ctx* ctx);                                   /* Renderer::ClearAccumulator (renderer.cpp:15-18)    */
int  crt_read_accumulator(crt_ctx* ctx, float* host_rgba /* float4[width*height] */);
/* screen->pixels and Renderer::energy as ProcessTile/Tick leave them (renderer.cpp:119,127-129,155-157):
 * pixel = accumulator * scale, scale = 1/(spp+passes) of the LAST rendered frame.  Either output may be NULL. */
int  crt_resolve_screen(crt_ctx* ctx, float scale, uint32_t* host_pixels /* width*height */, float* energy);
/* One Renderer::Tick (renderer.cpp:144-168): exactly crt_render(ctx, spp, 1, passes), then crt_read_accumulator(ctx, host_rgba) if host_rgba != NULL,
 * then crt_resolve_screen(ctx, 1/(spp+passes), host_pixels, energy) — bit for bit the same accumulator, screen pixels, energy and untouched non-owned
 * tiles.  Synchronous; any output may be NULL.  Argument checks and error codes are crt_render's.
 * Render-ahead: a frame's samples do not depend on the accumulator, so once a Tick follows a Tick with spp = previous spp + passes and nothing the
 * samples depend on has changed in between (crt_set_camera with different values, crt_update_scene, any crt_upload_*, crt_set_render_accel), the
 * following frames are rendered ahead in multi-frame launches and a later Tick of that sequence only adds its frame's samples, resolves and reads
 * back.  Any other call order is served as above (crt_render and crt_reserve drop the frames rendered ahead; crt_clear and crt_bind_accumulator keep
 * them).  The counters and crt_get_timing include every frame rendered ahead, also those later dropped.  Contexts with collectStats, the KD-tree /
 * grid path (crt_set_render_accel != 0, FileScene's and a two-level scene's BLAS set alike) and the PrimitiveScene never render ahead. */
int  crt_tick(crt_ctx* ctx, uint32_t spp, uint32_t passes, uint32_t* host_pixels /* width*height */, float* host_rgba /* float4[width*height] */, float* energy);

/* ---- Whitted-style integrator ("2. WhittedStyle/renderer.cpp":21-157): one deterministic Tick -------------------
 * Every pixel of the image (rows are not tile-truncated in this renderer) gets accumulator = float4(Trace(primary), 0)
 * and screen pixel = RGBF32_to_RGB8 of it; host_pixels may be NULL.  Synchronous. */
int  crt_whitted_tick(crt_ctx* ctx, uint32_t* host_pixels /* width*height or NULL */);
/* The Whitted renderer's traversal inspection and per-Tick metrics (renderer.cpp:38-39, 147-152, 164-189; infra/helper.h:104-120 GetTraverseCountColor).
 * One Tick as crt_whitted_tick's, which also reports, over the W*H PRIMARY rays, Ray::traversed / Ray::tested per pixel and the Tick's metrics.  In an inspect
 * mode Trace returns, for a primary ray that hits anything (light quad and floor included; before the isLight test and any recursion, so exactly one ray per
 * pixel is traced), GetTraverseCountColor(count, peak) with count = traversed / tested and `peak` the renderer's m_peakTraversal / m_peakTests AS IT STANDS
 * WHEN THAT PIXEL IS TRACED; a miss is the sky colour in every mode.  The reference raises the peaks from unsynchronised OpenMP threads, so only its
 * single-threaded order defines a picture; that order is served:
 *     peakIn(i) = max(peak passed in, max over pixels j < i of count(j)),  i = x + y * width   (an exclusive prefix maximum in row-major order)
 *     pixel(i)  = hit ? GetTraverseCountColor(count(i), peakIn(i)) : sky;   peak < 10 gives green, else green + (count clamped to [0, peak]) / (float)peak * (red - green)
 * in float32 operation for operation (true division, no fused multiply-add).  The peaks are the caller's state (the reference resets them when the camera
 * changes, not per Tick): passed in, returned raised.  The context keeps none, so the call is a function of scene, camera, crt_set_render_accel and its arguments.
 * Every mode writes accumulator = float4(colour, 0) and the screen pixel for all W*H pixels; CRT_INSPECT_NONE leaves exactly crt_whitted_tick's.  Works through
 * whatever crt_set_render_accel selects.  Synchronous; any output may be NULL.  CRT_ERR_INVALID for a mode outside 0..2 or a negative peak; without a triangle
 * scene as crt_whitted_tick; a failed call writes nothing.  crt_counters: an inspect mode counts its one ray per pixel, CRT_INSPECT_NONE what crt_whitted_tick counts.
 * Deviations: `tested` is crt_hit.tested (tests over the whole query, as everywhere in this ABI); the reference keeps its totals in float and adds ray by ray,
 * which is order-dependent beyond 2^24 — the totals here are the exact integers (average = (float)total / (float)rayHitCount).
 * Device scratch (two int32 per pixel, one int32 per 1024 pixels) is allocated by the first call and freed by crt_destroy. */
#define CRT_INSPECT_NONE      0   /* the shaded image of crt_whitted_tick, plus the metrics          */
#define CRT_INSPECT_TRAVERSAL 1   /* m_inspectTraversal:        heat map of Ray::traversed           */
#define CRT_INSPECT_TESTS     2   /* m_inspectIntersectionTest: heat map of Ray::tested              */
typedef struct crt_whitted_metrics {
    uint64_t rayHitCount;                 /* primary rays with traversed > 0                          */
    uint64_t totalTraversal, totalTests;  /* exact sums over all W*H primary rays                     */
    int32_t  peakTraversal, peakTests;    /* max(value passed in, this Tick's maximum)                */
} crt_whitted_metrics;
int  crt_whitted_tick_inspect(crt_ctx* ctx, int inspect, int32_t peakTraversalIn, int32_t peakTestsIn,
                              uint32_t* host_pixels   /* W*H or NULL */,
                              int32_t* host_traversed /* W*H or NULL */, int32_t* host_tested /* W*H or NULL */,
                              crt_whitted_metrics* metrics /* or NULL */);

/* ---- query entry = scene.FindNearest(ray) ------------------------------------------------------------ */
int  crt_find_nearest(crt_ctx* ctx, const crt_ray* rays, crt_hit* hits, size_t n);

/* ---- FileScene's alternative accelerators: KDTree (infra/kdtree.cpp — the one the reference ships enabled, infra/scene/file_scene.h:10-12)
 * and Grid (infra/grid.cpp), built on the host exactly as there and attached to an uploaded CRT_SCENE_FILE scene.  The reference's KDTreeNode is
 * pointer-linked with a std::vector per node (infra/blas_kdtree.h:15-24), so there is no layout to be bit-compatible with: nodes are passed flattened in
 * PRE-ORDER (node, left subtree, right subtree), leaves naming a range of kdTriIndices; Grid's cells (x-major: ix + iy*rx + iz*rx*ry) as a prefix array.
 * crt_find_nearest_alt = scene.FindNearest with that accelerator in place of the BVH (light quad, floor plane, accelerator: file_scene.cpp:170-175);
 * crt_hit.traversed / tested count as Ray::traversed / Ray::tested do there.  The render kernels walk the SAH-BVH only. */
#define CRT_ACCEL_KDTREE 1
#define CRT_ACCEL_GRID   2
typedef struct crt_kd_node {
    float aabbMin[3]; int32_t left;          /* KDTreeNode::aabbMin; index of node->left, < 0 = leaf (isLeaf)                    */
    float aabbMax[3]; int32_t right;
    float splitDistance; int32_t splitAxis;  /* interior: splitPos = aabbMin[splitAxis] + splitDistance (kdtree.cpp:161-162)       */
    uint32_t firstTri, triCount;             /* leaf: triIndices = kdTriIndices[firstTri .. firstTri + triCount)                    */
} crt_kd_node;
typedef struct crt_alt_accel {
    int32_t kind;                                                    /* CRT_ACCEL_KDTREE or CRT_ACCEL_GRID                          */
    const crt_tri* triangles; uint32_t triCount;                     /* KDTree::triangles / Grid::triangles (= FileScene's triangle array) */
    const crt_kd_node* kdNodes; uint32_t kdNodeCount;                /* KD-tree: pre-order nodes, root = 0                          */
    const uint32_t* kdTriIndices; uint32_t kdTriIndexCount;
    int32_t gridResolution[3]; float gridCellSize[3];                /* Grid::resolution, cellSize                                  */
    float gridMin[3], gridMax[3];                                    /* Grid::localBounds                                           */
    const uint32_t* gridCellStart;                                   /* rx*ry*rz + 1 entries: cell c holds gridCellTris[start[c] .. start[c+1]) */
    const int32_t* gridCellTris; uint32_t gridCellTriCount;
} crt_alt_accel;
int  crt_upload_alt_accel(crt_ctx* ctx, const crt_alt_accel* accel);   /* after crt_upload_scene of a CRT_SCENE_FILE scene; one structure per kind is kept */
int  crt_find_nearest_alt(crt_ctx* ctx, int kind, const crt_ray* rays, crt_hit* hits, size_t n);
/* ABI 3: which structure crt_render (Renderer::Sample) and crt_whitted_tick (Renderer::Trace, incl. its shadow rays) trace through: 0 = the scene's BVH / TLAS
 * (default), CRT_ACCEL_KDTREE / CRT_ACCEL_GRID = the uploaded alternative accelerator — what the reference's FileScene does when built with USE_KDTree (its shipped
 * setting, infra/scene/file_scene.h:10-12, file_scene.cpp:170-187) / USE_Grid.  Bug-compatible: the KD traversal loses hits for rays with a direction component of
 * exactly 0 (kdtree.cpp:161-201).  The sequential form (one wavefront per tile and 64-frame window); reset by crt_upload_scene / crt_upload_alt_accel /
 * crt_upload_blas_accel of the kind, and by a CRT_UPDATE_BOUNDS update that drops a two-level scene's set. */
int  crt_set_render_accel(crt_ctx* ctx, int kind);
/* Two-level scenes built with TLAS_USE_KDTree / TLAS_USE_Grid (tlas_file_scene.cpp:40-90): TLASKDTree over BLASKDTree / TLASGrid over BLASGrid.  After
 * crt_upload_scene of a CRT_SCENE_TLAS scene, blas[i] is BLAS i's KD-tree / grid over its own object-space triangle array (BLASKDTree::Build = KDTree's build,
 * BLASGrid::Build = Grid's; blasCount = the scene's bvhCount).  Checked as crt_upload_alt_accel checks one structure, and also: the triangle count and every
 * triangle's objIdx are BLAS i's, and the root box (KD nodes[0], grid gridMin / gridMax) equals BLAS i's BVH root box bit for bit — the TLAS and the instance
 * records of the BVH variant are shared (SetTransform takes the world bounds from that box) — else CRT_ERR_INVALID; a traversal stack (TLAS height + deepest
 * KD-tree + 1) beyond the LDS budget is CRT_ERR_UNSUPPORTED.  A failed call changes nothing (a refused description, and also a failed device allocation or
 * copy: the new set is built in buffers of its own and replaces the previous one only once complete).  One set per kind is kept; the call is synchronous (it
 * waits for the queries and render launches that read the previous set); a successful call resets crt_set_render_accel to 0 if it named this kind.  Then accel = CRT_ACCEL_KDTREE / CRT_ACCEL_GRID works on the TLAS scene in
 * crt_find_nearest_alt, crt_is_occluded, the device query entries and crt_set_render_accel (crt_render, crt_whitted_tick); records as the TLAS-BVH path's
 * (objIdx >= 2 = the BLAS's, triIdx BLAS-local, traversed = TLAS steps + every BLAS's steps, tested over the query).  The KD walk keeps BLASKDTree's early
 * return `if (ray.objIdx == objIdx && ray.t < t) return;` (blas_kdtree.cpp:377, 396), so `traversed` differs from FileScene's KD-tree for rays that hit something
 * else first.  CRT_UPDATE_TRANSFORMS keeps the set (it lives in object space); CRT_UPDATE_BOUNDS drops it (the reference has no Refit for these structures:
 * the render goes back to the BVH, a query with that accel is CRT_ERR_STATE); crt_upload_scene / crt_upload_primitive_scene drop it; crt_upload_alt_accel on
 * a TLAS scene stays CRT_ERR_STATE. */
int  crt_upload_blas_accel(crt_ctx* ctx, int kind, const crt_alt_accel* blas, uint32_t blasCount);
/* KDTree::Build / BLASKDTree::Build (infra/kdtree.cpp:4-108) for ONE uploaded BVH's triangle array on the device, from vertex positions that already live in device
 * memory: the KD-tree — the accelerator the reference's FileScene ships enabled — rebuilt from scratch without a host round trip, beside crt_refit_device (BVH),
 * crt_update_transforms_device (TLAS) and crt_build_grid_device (grid).  ABI version 3 still: both entries are additions, detected by symbol.  d_positions, triCount
 * and `stream` are exactly crt_build_grid_device's (the same array, the same pointer / device / stream checks, NULL = the context's stream).
 * What the call leaves on the device equals, byte for byte, what KDTree::Build over those triangles followed by crt_upload_alt_accel / crt_upload_blas_accel would
 * leave: the crt_kd_node records in the host build's pre-order (node, left subtree, right subtree); every box derived from the root box (a child takes its parent's
 * box with one component replaced by splitPos; the root box's signed zeros as the reference's fold leaves them); left / right -1 on leaves; splitAxis and
 * splitDistance set on interior nodes, 0 on leaves; firstTri of EVERY node = the leaf references that precede it in pre-order; triCount 0 on interior nodes; the leaf
 * reference array in pre-order of the leaves, each list in the order the recursion keeps; the triangle records as crt_build_grid_device writes them; the KD stack =
 * height + 1, as the upload derives it.  The split is the spatial median of the longest axis (not SAH); recursion stops at <= 2 triangles or at depth 20; the
 * comparison `bmin > splitPos - 0.001` is evaluated in double, as the reference's expression is.  Two runs over the same input give identical bytes.
 * CRT_SCENE_FILE (bvh = 0): works with or without an earlier crt_upload_alt_accel(CRT_ACCEL_KDTREE); the tree becomes the scene's CRT_ACCEL_KDTREE structure and
 * crt_set_render_accel(CRT_ACCEL_KDTREE) stays selected (the per-frame loop is refit, rebuild, render).  The build replaces the triangle records, which the grid
 * shares, and the grid's cells belong to the old positions, so a successful call marks the grid absent — the mirror of what crt_build_grid_device does to the
 * KD-tree: a query with CRT_ACCEL_GRID is CRT_ERR_STATE, crt_set_render_accel goes back to 0 if it named the grid.  Keeping both live from one set of positions is
 * not offered.
 * CRT_SCENE_TLAS (bvh = a BLAS): needs a KD set uploaded earlier through crt_upload_blas_accel(CRT_ACCEL_KDTREE, ..), else CRT_ERR_STATE.  The context keeps a "kd
 * current" flag per BLAS, next to the grid's: an upload sets all, CRT_UPDATE_BOUNDS clears all, crt_refit_device(b) clears b's, this call sets b's; the set is live
 * iff every flag is set (crt_set_render_accel must be called again after the set has been dropped).  The other BLASes' parts are carried over device to device and
 * the descriptors re-based (nodeBase, refBase, triBase); the set's KD stack becomes the deepest tree's height + 1.  The upload's root-box test is not applied, for
 * the reason given at crt_build_grid_device.  The call touches neither the BVH, the instances nor the TLAS.
 * Ordering and lifetime are crt_build_grid_device's: the build runs on `stream` into buffers of its own (a reader of the scene-write protocol); the tree it replaces
 * keeps answering for everything enqueued earlier, on any stream, and is retired once its last readers have completed; a refusal or failure leaves it answering.
 * THE HOST WAITS: the tree grows level by level (depth 0 .. 20), and the host sizes each level's buffers, so the call makes ONE WAIT PER LEVEL, at most 21: a small
 * pinned read-back (the level's split-node, leaf-reference and child-reference counts) that waits for `stream` up to that point only, for nothing submitted later.
 * The first of them also carries the bounds pass's non-finite flag, and the last one (the level without a split) gives the final counts and the height, so there
 * is no separate wait for either.  Growing the build's scratch beyond any earlier build's goes through hipFree / hipMalloc, as the grid build's.
 * Refused with nothing modified, the previous tree still answering: no scene, a two-level scene without an uploaded KD set (CRT_ERR_STATE); a PrimitiveScene, a
 * level or the leaf total with more than 2^31-1 references, a two-level traversal stack beyond the LDS budget (CRT_ERR_UNSUPPORTED); bvh out of range, triCount
 * different from the uploaded BVH's, d_positions NULL / a host pointer / memory of another device, a stream of another device, a non-finite position component
 * (found by the bounds pass) (CRT_ERR_INVALID); a failed device allocation (CRT_ERR_DEVICE).
 * Cost: a triangle that straddles a split plane is referenced on both sides, and where triangles overlap no plane separates them, so they are duplicated down to
 * the depth limit — the reference's behaviour, not the build's.  Measured (tools/kdtree_device_cost.py, profiles/kdtree_device.json, one MI355X):
 * the bunny's 4 968 triangles give 154429 nodes and 216127 leaf references in 21 levels, 10.9 ms by the host route (copy, Refit, KDTree::Build, upload) and 1.4 ms by this
 * call, of which 0.24 ms are its 21 host waits; the eight overlapping triangles of the tests' `zeros` mesh give 247 189 nodes and 383 255 references. */
int  crt_build_kdtree_device(crt_ctx* ctx, uint32_t bvh, const float* d_positions /* 9 * triCount, device */, uint32_t triCount, void* stream);
/* The live KD-tree of a FileScene (bvh = 0) or of one BLAS of a two-level scene's set, uploaded or device-built: sizes first (any output may be NULL; height = the
 * deepest leaf's depth), then the arrays where the pointers are non-NULL (nodes: nodeCount records, refs: refCount leaf references, BLAS-local).  Synchronous (it
 * waits for a device build still running).  CRT_ERR_STATE when there is no live tree; bvh out of range is CRT_ERR_INVALID. */
int  crt_get_kdtree(crt_ctx* ctx, uint32_t bvh, uint32_t* nodeCount, uint32_t* refCount, uint32_t* height, crt_kd_node* nodes /* nodeCount, or NULL */,
                    uint32_t* refs /* refCount, or NULL */);
/* BVH::Build / BLASBVH::Build (bvh.cpp:4-24, 63-178: binned SAH, 8 bins) of ONE uploaded BVH on the device, from vertex positions that already live in device memory:
 * where crt_refit_device keeps the rest pose's topology — boxes overlap more with every frame of a deformation — this call gives the tree a fresh build has.  ABI
 * version 3 still: an addition, detected by symbol.  d_positions, triCount, `stream`, rootBox as crt_refit_device takes them; CRT_SCENE_FILE (bvh = 0) and every BLAS
 * of a CRT_SCENE_TLAS scene.  Afterwards the scene is exactly what crt_upload_scene gives for the same description with that BVH rebuilt on the host (triangles moved,
 * centroids (v0 + v1 + v2) * 0.3333f, Build), byte for byte: node pairs, leaf triangles, both forms of every packed reference, the section offsets (the pair section
 * changes size, so everything behind it moves), the root reference and pair, the stack depth.  Shade records, materials, textures, the TLAS and the transforms are
 * untouched.  Like BLASBVH::Build the call does NOT rebuild the TLAS: crt_update_transforms_device next (it reads the new node-0 box on the device), or the host route
 * through rootBox, as after crt_refit_device.
 * The build is level-synchronous (device/bvh_build.hip): ONE SHORT HOST WAIT PER LEVEL of the tree for the number of nodes that split, then one read-back of the new
 * pair and leaf sections into the context's host mirror.  The result is a fresh geometry buffer; the old one is retired behind its readers: launches enqueued earlier
 * keep the old tree, later ones wait for the new one.  It drops what crt_refit_device drops (a two-level scene's KD-tree / grid sets until their device builds of
 * this BLAS, the frames crt_tick rendered ahead) and that BVH's refit plan.
 * Refused with nothing modified, with crt_refit_device's codes; also: a position component that is not finite (CRT_ERR_INVALID), a tree whose traversal stack would
 * exceed the LDS budget crt_upload_scene enforces, geometry beyond 4 GiB (CRT_ERR_UNSUPPORTED), a failed device allocation (CRT_ERR_DEVICE). */
int  crt_build_bvh_device(crt_ctx* ctx, uint32_t bvh, const float* d_positions /* 9 * triCount, device */, uint32_t triCount, void* stream,
                          float rootBox[6] /* out: node 0's aabbMin, aabbMax; may be NULL */);
/* One BVH of the live scene in the reference's form again, reconstructed from the device's geometry buffer (after an upload, an update, a refit or a device
 * rebuild): sizes first (any output may be NULL; maxDepth = the deepest depth at which a node split, what BVH::Build reports; height = the deepest leaf, in edges),
 * then nodes (nodesUsed records: children 2k + 1 and 2k + 2 are pair k's) and triangleIndices (triCount) where the pointers are non-NULL.  Synchronous (it waits for a
 * scene write still running).  No scene: CRT_ERR_STATE; a PrimitiveScene: CRT_ERR_UNSUPPORTED; bvh out of range: CRT_ERR_INVALID. */
int  crt_get_bvh(crt_ctx* ctx, uint32_t bvh, uint32_t* nodesUsed, uint32_t* maxDepth, uint32_t* height, crt_bvh_node* nodes /* nodesUsed, or NULL */,
                 uint32_t* triangleIndices /* triCount, or NULL */);

/* ---- scene queries: BaseScene::IsOccluded, and both queries on device buffers (base_scene.h:16-32) ------------------------------------------------
 * accel: 0 = the scene's own structure (BVH / TLAS; for the nearest-hit query also the PrimitiveScene), CRT_ACCEL_KDTREE / CRT_ACCEL_GRID = the uploaded
 * alternative accelerator (FileScene built with USE_KDTree / USE_Grid; a TLASFileScene built with TLAS_USE_KDTree / TLAS_USE_Grid: crt_upload_blas_accel).
 *
 * IsOccluded (FileScene::IsOccluded / TLASFileScene::IsOccluded, file_scene.cpp:177-187, tlas_file_scene.cpp:208-218), bug-compatible: the light quad is tested
 * bounded by ray.t (Quad::IsOccluded, primitives.h:347-362); then the acceleration structure is intersected over the WHOLE ray (shadow.t = 1e34f, not clipped at
 * ray.t); the floor plane is not tested.  occluded[i] = 1 or 0.  The walk stops at the first successful triangle test, which gives exactly the answer of the
 * reference's full nearest-hit walk (DESIGN.md "Scene queries").  A binding implements `bool IsOccluded(const Ray& ray)` as one crt_shadow_ray {ray.O, ray.D,
 * ray.t} through crt_is_occluded.  The occlusion entries count nothing in crt_counters (the reference's IsOccluded never touches the caller's ray counters);
 * PrimitiveScene: CRT_ERR_UNSUPPORTED.
 *
 * Device entries: d_* are device pointers on cfg.device (checked; a host or other-device pointer is CRT_ERR_INVALID); `stream` is a hipStream_t of that device
 * (void* here, as this header takes no HIP types), NULL = the ctx's own stream.  They return once the work is enqueued and never wait on the host (except that
 * a call which finds 64 device queries of this ctx still running waits for the oldest).  crt_find_nearest_device writes bit for bit the records of
 * crt_find_nearest / crt_find_nearest_alt and counts into crt_counters as they do.
 * Ordering contract of the device entries:
 *   - a query sees the scene as of the last crt_upload_* / crt_update_scene call made before it (the caller's stream waits for those copies);
 *   - a later crt_update_scene, crt_upload_scene / crt_upload_primitive_scene, crt_upload_alt_accel or crt_destroy does not rewrite or free memory that an
 *     enqueued query still reads: crt_update_scene orders its copy behind every query in flight (no host wait), the others wait for them on the host;
 *   - queries may be in flight on several streams at once (each launch draws its rays from a cursor of its own);
 *   - the outputs are ready in stream order on `stream`: the caller orders its consumers (a kernel on the same stream needs no host synchronisation).
 * All entries: n == 0 is a no-op; n > 2^31-1 is CRT_ERR_UNSUPPORTED; no scene, or an accelerator that was not uploaded, is CRT_ERR_STATE. */
/* A crt_shadow_ray carries no objIdx: IsOccluded is defined for a ray whose objIdx is -1, as Ray(O, D, t) builds it.  (On a two-level scene's KD-tree set a
 * caller ray with objIdx >= 2 could differ: BLASKDTree's early return compares ray.objIdx — only where that instance's object-space direction has a component
 * that is exactly 0.) */
typedef struct crt_shadow_ray { float O[3]; float D[3]; float t; } crt_shadow_ray;   /* Ray with ray.t = t: the argument of IsOccluded (28 bytes, as crt_ray) */
int  crt_is_occluded(crt_ctx* ctx, int accel, const crt_shadow_ray* rays, int32_t* occluded, size_t n);                       /* host pointers, synchronous */
int  crt_find_nearest_device(crt_ctx* ctx, int accel, const crt_ray* d_rays, crt_hit* d_hits, size_t n, void* stream);
int  crt_is_occluded_device(crt_ctx* ctx, int accel, const crt_shadow_ray* d_rays, int32_t* d_occluded, size_t n, void* stream);

/* The shading queries of BaseScene (base_scene.h:16-32): GetHitInfo + Material::GetAlbedo, GetSkyColor, GetLightPos / GetLightColor.  With FindNearest and
 * IsOccluded above they are what every integrator of the reference begins with (FindNearest; miss -> GetSkyColor; I = O + t * D; GetHitInfo; GetAlbedo —
 * "2. WhittedStyle/renderer.cpp":24-32, "3. PathTracer/renderer.cpp":52-61), so a caller can write Trace / Sample outside the library, on device buffers.
 * ABI version 3 still: the entries are additions, detected by symbol (as crt_whitted_tick_inspect).
 *
 * crt_get_hit_info: out[i] from rays[i] (O, D) and hits[i] (t, u, v, objIdx, triIdx), by hits[i].objIdx (file_scene.cpp:189-214, tlas_file_scene.cpp:220-260):
 *     -1 (miss)             I = N = 0, u = v = 0, material = CRT_MATERIAL_MISS, albedo = GetSkyColor(ray): what Trace / Sample return for a miss
 *      0 (light quad)       N = Quad::GetNormal = (-T[1], -T[5], -T[9]) (primitives.h:363-367), u = v = 0, material 0, albedo (1, 1, 1) (primitiveMaterials[0], no texture)
 *      1 (floor plane)      N = floor.N, uv = Plane::GetUV(I) (primitives.h:116-133, with its N.y == 1 test), material 1, albedo = the floor texture at uv (texture.h:61-96)
 *      >= 2, FileScene      N = normalize((1-u-v) n0 + u n1 + v n2) of triangle triIdx (bvh.cpp:290-305), uv by the same weights, material 2 + models[tri.objIdx-2]->matIdx
 *      >= 2, TLASFileScene  the same in BLAS objIdx-2 with the BLAS-LOCAL triIdx that crt_hit reports, then N = normalize(TransformVector(N, T)) (blas_bvh.cpp:391-398),
 *                           material 2 + blas->matIdx
 * albedo = material->GetAlbedo(uv): the material's texture at uv, or (1, 1, 1); then `if (dot(N, ray.D) > 0) N = -N`, so N faces the ray.  I = ray.O + t * ray.D for
 * every hit.  t, u, v come from the hit record: a record of ANY find-nearest entry (BVH, KD-tree, grid, the two-level variants) can be fed straight in, and the
 * query depends neither on crt_set_render_accel nor on the accelerator that produced the hit.  The arithmetic is the render kernels' (the same device functions):
 * bit for bit what Sample and Trace shade with.
 * Bad records do not become bad addresses.  objIdx must lie in -1 .. objects + 1 (objects = objCount of a FileScene, bvhCount of a two-level scene) and, for
 * objIdx >= 2, triIdx in 0 .. the triangle count of that object's BVH - 1.  The host entry checks every record first and returns CRT_ERR_INVALID (the message names
 * the first bad record) with nothing written; the device entry cannot, so the kernel applies the same test per record and writes material =
 * CRT_MATERIAL_INVALID, every other field 0, without reading the scene for it.  NaN or out-of-range t, u, v are arithmetic only and pass through: Texture::Sample
 * clamps uv with clamp(f, 0, 1) = max(0, min(f, 1)), whose comparisons are false for a NaN, so min gives 1, the clamp 1, and a NaN u reads the last column /
 * a NaN v (1 - 1 = 0) row 0 — a texel inside the texture; the float -> int conversions only ever see values in [0, width] / [0, height].
 * crt_get_sky_color: rgb[3i .. 3i+2] = GetSkyColor(rays[i]) (file_scene.cpp:142-154; only D is read) for rays without a hit record.
 * crt_get_light: GetLightPos() (file_scene.cpp:156-162) and GetLightColor() = (24, 24, 22) of the uploaded triangle scene.
 * Host entries: host pointers, synchronous.  Device entries: as the device entries above (pointers checked, `stream`, the ordering contract — a later
 * crt_update_scene is ordered behind them, freeing / re-uploading calls wait for them); d_out of crt_get_hit_info_device must also be 16-byte aligned (three
 * 16-byte stores per record).  n == 0 is a no-op; n > 2^31-1 is CRT_ERR_UNSUPPORTED; no scene is CRT_ERR_STATE.  Nothing is counted in crt_counters and crt_tick's
 * render-ahead is not disturbed.  PrimitiveScene: crt_get_sky_color* gives 0 (PrimitiveScene::GetSkyColor, primitive_scene.cpp:82-85); crt_get_hit_info* and
 * crt_get_light are CRT_ERR_UNSUPPORTED — the repo's oracle exports neither the normals nor the albedo overrides of that scene, so nothing could check them. */
#define CRT_MATERIAL_MISS    (-1)
#define CRT_MATERIAL_INVALID (-2)
typedef struct crt_hit_info {          /* 48 bytes; arrays of it 16-byte aligned: three 16-byte stores per record */
    float I[3];      int32_t material; /* I = ray.O + ray.t * ray.D.  material: 0 = light (primitiveMaterials[0], isLight), 1 = floor
                                          (primitiveMaterials[1]), 2 + k = crt_scene_desc.materials[k], or one of the two values above */
    float N[3];      float u;          /* GetHitInfo's normal, already flipped to face the ray; HitInfo::uv.x                          */
    float albedo[3]; float v;          /* material->GetAlbedo(uv); HitInfo::uv.y                                                        */
} crt_hit_info;
int  crt_get_hit_info(crt_ctx* ctx, const crt_ray* rays, const crt_hit* hits, crt_hit_info* out, size_t n);                   /* host pointers, synchronous */
int  crt_get_hit_info_device(crt_ctx* ctx, const crt_ray* d_rays, const crt_hit* d_hits, crt_hit_info* d_out, size_t n, void* stream);
int  crt_get_sky_color(crt_ctx* ctx, const crt_ray* rays, float* rgb /* 3 * n */, size_t n);                                  /* host pointers, synchronous */
int  crt_get_sky_color_device(crt_ctx* ctx, const crt_ray* d_rays, float* d_rgb /* 3 * n */, size_t n, void* stream);
int  crt_get_light(crt_ctx* ctx, float pos[3], float color[3]);

/* Renderer::Sample(ray, seed, 0) — the path tracer's integrator ("3. PathTracer/renderer.cpp":50-100) — for n rays of the caller's with a seed each: light
 * probes, irradiance baking, a camera of the caller's own, importance-sampled pixels, training sets.  ABI version 3 still: an addition, detected by symbol.
 * rgb[3i .. 3i+2] = the radiance of the path that starts with rays[i]; seeds[i] is in/out: the xorshift32 state before / after the path, so a caller can chain
 * paths exactly as Renderer::ProcessTile does (draw the y jitter, then the x jitter, build the primary ray, Sample).
 * Per ray: O, D and inside are used as given — D is NOT normalised (the reference hands Sample unit directions; so should the caller), rD = 1 / D per component,
 * depth starts at 0, depthLimit is crt_config's, every rnd draw is made in the reference's order and the throughput factors multiply innermost first: radiance and
 * returned seed are bit for bit what the render entries compute for the same ray and seed.
 * accel: as for crt_find_nearest_device — 0 = the BVH of a CRT_SCENE_FILE scene, the TLAS of a CRT_SCENE_TLAS scene, or the PrimitiveScene; CRT_ACCEL_KDTREE /
 * CRT_ACCEL_GRID = the uploaded alternative structure (a two-level scene's per-BLAS sets included).  crt_set_render_accel is not consulted: the argument decides.
 * Rays that are NOT traced come back as quiet NaN in all three channels, their seed untouched, and affect no other ray: a seed of 0 (xorshift32 maps 0 to 0, every
 * draw would be 0 and the diffuse bounce's rejection loop would never end; a non-zero state never becomes 0), a non-finite component of O or D, or D = (0, 0, 0).
 * The host entry applies the same rule per ray; it does not refuse the call.
 * Counters: crt_counters.rays grows by the FindNearest calls made (mesh_hits as the render entries count it); `primary` is not touched.
 * crt_sample_device: as the device entries above — d_rays (28 n bytes), d_seeds (4 n) and d_rgb (12 n) are device pointers on cfg.device, 4-byte aligned (NULL,
 * misaligned, host or other-device memory: CRT_ERR_INVALID), `stream` a hipStream_t of that device or NULL; the ordering contract is theirs (a later
 * crt_update_scene / crt_refit_device is ordered behind the launch).  crt_sample: host pointers, synchronous, through staging buffers the context keeps.
 * Refusals (nothing is modified, crt_last_error says why): no scene or no such accelerator CRT_ERR_STATE; unknown accel CRT_ERR_INVALID; n > 2^31-1
 * CRT_ERR_UNSUPPORTED; a structure whose traversal stack does not fit the kernel's LDS CRT_ERR_UNSUPPORTED (as crt_set_render_accel).  n == 0 is a no-op after
 * the checks that need no buffer. */
int  crt_sample(crt_ctx* ctx, int accel, const crt_ray* rays, uint32_t* seeds, float* rgb /* 3 * n */, size_t n);                          /* host pointers, synchronous */
int  crt_sample_device(crt_ctx* ctx, int accel, const crt_ray* d_rays, uint32_t* d_seeds, float* d_rgb /* 3 * n */, size_t n, void* stream); /* device pointers, no host wait */

/* Renderer::Trace(ray, 0) — the Whitted integrator ("2. WhittedStyle/renderer.cpp":21-91), the deterministic one — for n rays of the caller's: light probes, a second
 * camera, reflection captures, a training set without noise.  crt_whitted_tick traces the pixel grid of the context's camera with the same body; these entries
 * serve it for any ray array.  ABI version 3 still: additions, detected by symbol.
 * rgb[3i .. 3i+2] = Trace's return value for rays[i].  traversed[i] / tested[i] (each may be NULL) = Ray::traversed / Ray::tested of the depth-0 ray after Trace,
 * the figures Renderer::Tick reads off primaryRay for its metrics — so a caller can rebuild Tick with its metrics outside the library.
 * Per ray: O, D and inside are used as given — D is NOT normalised, rD = 1 / D per component; depth starts at 0; depthLimit is crt_config's, with the reference's
 * `depth > depthLimit` test ahead of the trace; the inspection modes are off.  Radiance and counts are bit for bit what crt_whitted_tick[_inspect] computes for the same ray.
 * accel: as for crt_sample_device — 0 = the BVH / TLAS, CRT_ACCEL_KDTREE / CRT_ACCEL_GRID = the uploaded alternative structure (a two-level scene's per-BLAS sets
 * included), for the nearest-hit and the shadow queries alike.  crt_set_render_accel is not consulted: the argument decides.
 * Rays that are NOT traced come back as quiet NaN in all three channels and -1 in both counts, and affect no other ray: a non-finite component of O or D, or
 * D = (0, 0, 0).  The host entry applies the same rule per ray; it does not refuse the call.
 * Counters: everything crt_whitted_tick counts for the same rays, except `primary`, which is not touched.  crt_tick's rendered-ahead frames are not disturbed.
 * crt_trace_device: as the device entries above — d_rays (28 n bytes), d_rgb (12 n) and, where not NULL, d_traversed / d_tested (4 n each) are device pointers on
 * cfg.device, 4-byte aligned (a NULL d_rays / d_rgb, misaligned, host or other-device memory: CRT_ERR_INVALID), `stream` a hipStream_t of that device or NULL; no
 * host wait; the ordering contract is theirs (a later crt_update_scene / crt_refit_device / device rebuild is ordered behind the launch).  crt_trace: host
 * pointers, synchronous, through staging buffers the context keeps.
 * Refusals (nothing is modified, crt_last_error says why): no scene or no such accelerator CRT_ERR_STATE; unknown accel CRT_ERR_INVALID; the PrimitiveScene
 * CRT_ERR_UNSUPPORTED (as crt_whitted_tick); n > 2^31-1 CRT_ERR_UNSUPPORTED; a traversal stack of more than 64 dwords per lane (four wavefronts share a
 * workgroup's 64 KiB of LDS) CRT_ERR_UNSUPPORTED.  n == 0 is a no-op after the checks that need no buffer. */
int  crt_trace(crt_ctx* ctx, int accel, const crt_ray* rays, float* rgb /* 3 * n */, int32_t* traversed /* n or NULL */, int32_t* tested /* n or NULL */, size_t n);
int  crt_trace_device(crt_ctx* ctx, int accel, const crt_ray* d_rays, float* d_rgb /* 3 * n */, int32_t* d_traversed /* n or NULL */, int32_t* d_tested /* n or NULL */,
                      size_t n, void* stream);

/* The frames of MANY cameras in one render job: a turntable, a replayed camera path, an offline animation, the views of a training set — whenever the cameras are
 * known before the frames are needed.  A one-frame crt_render runs a tile's serial RNG stream in one lane of a wavefront; here the other 63 lanes carry the same
 * tile for other cameras or other frames (device/render_views.h).  ABI version 3 still: additions, detected by symbol.
 * cams: K records of 12 floats — camPos, topLeft, topRight, bottomLeft, exactly crt_set_camera's arguments.  For every view k and every pixel of a tile this
 * context owns, out_rgba[k] (W * H float4) is bit for bit what crt_set_camera(cams[k]); crt_clear; crt_render(spp_first, frames, passes); crt_read_accumulator
 * leaves there, w = 0 included, and out_pixels[k] (W * H, may be NULL) is bit for bit crt_resolve_screen(scale, ..)'s pixel of that accumulator.  No other pixel
 * of the outputs is touched: not the tiles the context does not own, not the rows and columns the 16-pixel tiling truncates.  The energy is not offered.
 * The job renders through whatever crt_set_render_accel has selected — the BVH / TLAS, the KD-tree or grid (a two-level scene's BLAS sets included) — or over the
 * PrimitiveScene, with crt_config's depthLimit and tile ownership.
 * It does NOT change the context's camera, accumulator (owned or bound), tile order, tuner or planner tables.  crt_tick: the frames rendered ahead SURVIVE — the
 * job's samples live in scratch of the entries' own (whole windows of 64 view-frames, at most cfg.maxFramesPerLaunch / 64 of them and 4 GiB per launch, kept
 * until crt_destroy), not in the slab pool — so a crt_tick sequence around the call returns the pixels it returns without it.
 * Counters: crt_counters.rays, primary and mesh_hits grow as they would for the K renders; the collectStats detail counters and tile clocks are not fed.
 * crt_render_views_device: d_cams (48 K bytes), d_out_rgba (16 K W H, 16-byte aligned) and, where not NULL, d_out_pixels (4 K W H) are device pointers on
 * cfg.device, checked as crt_sample_device checks its buffers; `stream` a hipStream_t of that device or NULL; no host wait (except to grow the scratch).  The
 * launches are readers under the scene-write protocol: a later crt_update_scene, refit or device rebuild is ordered behind them, a freeing call waits for them.
 * crt_render_views: host pointers, synchronous, through staging the context keeps.
 * Refusals (nothing is modified, crt_last_error says why): no scene CRT_ERR_STATE; passes outside 1..4 CRT_ERR_INVALID (as crt_render); K * frames > 2^31-1
 * CRT_ERR_UNSUPPORTED; a traversal stack beyond the sequential kernels' LDS bound CRT_ERR_UNSUPPORTED (crt_set_render_accel's rule); NULL, misaligned, host or
 * other-device memory, a stream of another device CRT_ERR_INVALID; a failed device allocation CRT_ERR_DEVICE.  K == 0 or frames == 0 is a no-op after the checks
 * that need no buffer.
 * When to use it (one MI355X, 1280x720, profiles/render_views.json): with one frame per view, 64 views take 85 ms (bunny) / 232 ms (tlas_scene.xml) against 916 /
 * 1 982 ms for the loop crt_set_camera, crt_clear, crt_render(1, 1, 1), crt_sync — 10.7x / 8.6x.  The job costs about 0.26 / 0.39 ms per view-frame however they are
 * split into views, while the loop's renders get cheaper per frame as they grow: at 64 frames per view the entry is still 1.36x / 1.87x faster, at 128 1.05x / 1.57x,
 * at 256 the loop wins (0.54x / 0.80x: its renders are then jobs of the pool kernel).  So: up to 128 frames per view call this entry; from 256 on, loop crt_render. */
int  crt_render_views(crt_ctx* ctx, const float* cams, uint32_t K, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                      float* out_rgba /* K * W*H float4 */, uint32_t* out_pixels /* K * W*H or NULL */);                                    /* host pointers, synchronous */
int  crt_render_views_device(crt_ctx* ctx, const float* d_cams, uint32_t K, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                             float* d_out_rgba, uint32_t* d_out_pixels /* or NULL */, void* stream);                                          /* device pointers, no host wait */

/* The frames of MANY cameras over MANY POSES of a two-level scene's instances in one render job: physics playback, a turntable of a moving assembly, a pose
 * optimiser's candidates, the views of a training set in which the objects move.  crt_render_views renders K cameras over the one live scene; the loop that moves
 * the instances between views — crt_update_transforms_device (one lone-wavefront build + one host wait per pose), crt_set_camera, crt_clear, crt_render, crt_read_accumulator —
 * pays the one-frame render and the lone build K times.  Here the P builds run side by side in ONE launch (device/tlas_build.hip), each into a job-local pose: an
 * image of the TLAS nodes, the TLAS child pairs and the Instance records; and every lane of crt_render_views' launch walks the TLAS of its own view's pose
 * (device/render_poses.h).  The BLAS trees are shared.  ABI version 3 still: additions, detected by symbol.
 * cams: K records of 12 floats, crt_set_camera's arguments.  T: P * blasCount row-major mat4s, pose p's at T + 16 * blasCount * p, each exactly what
 * crt_update_transforms_device takes as d_T (cells 0..11 read, no scale).  view_pose: K indices into the poses, or NULL: view k renders pose k, and P must equal K.
 * For every view k, with p = view_pose[k], and every pixel of a tile this context owns: out_rgba[k] (W * H float4) is bit for bit what
 * crt_update_transforms_device(T[p]); crt_set_camera(cams[k]); crt_clear; crt_render(spp_first, frames, passes); crt_read_accumulator leaves there, w = 0
 * included; out_pixels[k] (W * H, may be NULL) is crt_resolve_screen(scale)'s pixel of that accumulator; tlas_out[p] (host memory in BOTH entries, 2 * blasCount
 * nodes per pose, may be NULL) is byte for byte the tlasOut of crt_update_transforms_device(T[p]).  No other pixel of the outputs is touched.
 * THE LIVE SCENE IS NOT CHANGED: the Instance records, the TLAS, the root, the stack depth, the host mirror and the epoch stay as they are, and so do crt_tick's
 * rendered-ahead frames, the context's camera, the accumulator, the tuner and planner tables.  Poses are job-local: they live in scratch of the entries' own (kept
 * until crt_destroy, like crt_render_views' slab), at most 4 GiB of it (about 256 * blasCount bytes per pose).
 * World boxes come from the node-0 boxes as the device holds them — as uploaded, as sent by CRT_UPDATE_BOUNDS, or as refitted by crt_refit_device — so a refit
 * followed by this call needs nothing from the host.  The builds keep the reference's quirks, as crt_update_transforms_device's.
 * Counters: crt_counters.rays, primary and mesh_hits grow as they would for the K renders.
 * Ordering: the call is a reader under the scene-write protocol, exactly like crt_render_views_device: later writes are ordered behind it.  THE ONE HOST WAIT (both
 * entries; besides growing scratch): the launches' LDS traversal stack is sized by the tallest pose's TLAS, and a job with a failed build or a view_pose entry out
 * of range must not run — so the call reads the P build headers and the view_pose flag back (64 (P + 1) bytes, pinned; with tlas_out the node sections too) and
 * returns from that wait before it enqueues the render launches.  crt_render_poses_device: d_cams (48 K bytes), d_T (64 P blasCount), d_view_pose (4 K, or NULL),
 * d_out_rgba (16 K W H, 16-byte aligned), d_out_pixels (4 K W H, or NULL) are device pointers on cfg.device, checked as crt_render_views_device checks its
 * buffers; `stream` a hipStream_t of that device or NULL.  crt_render_poses: host pointers, synchronous, through staging the context keeps.
 * Refusals (nothing is written, crt_last_error says why): no scene CRT_ERR_STATE; a PrimitiveScene CRT_ERR_UNSUPPORTED; a CRT_SCENE_FILE scene CRT_ERR_INVALID;
 * blasCount different from the uploaded bvhCount CRT_ERR_INVALID; passes outside 1..4 CRT_ERR_INVALID; K * frames > 2^31-1 CRT_ERR_UNSUPPORTED;
 * crt_set_render_accel != 0 CRT_ERR_UNSUPPORTED (the KD-tree / grid BLAS sets live in object space and could be posed the same way: not built yet); P == 0 with
 * K > 0, or view_pose NULL with P != K, CRT_ERR_INVALID; a pose table beyond 4 GiB, or a scene uploaded with more than 2 * bvhCount TLAS nodes (as
 * crt_update_transforms_device), CRT_ERR_UNSUPPORTED; NULL, misaligned, host or other-device memory, a stream
 * of another device CRT_ERR_INVALID; a view_pose entry outside [0, P) CRT_ERR_INVALID (the host entry looks before anything runs; the device entry checks in the
 * build launch and learns of it with the headers); a pose whose build has a FindBestMatch without a candidate while more than one node is open CRT_ERR_INVALID
 * (crt_last_error names the first such pose and the call); a pose whose TLAS height puts the traversal stack beyond the sequential kernels' LDS bound
 * CRT_ERR_UNSUPPORTED; a failed device allocation CRT_ERR_DEVICE.  K == 0 or frames == 0 is a no-op after the checks that need no buffer.
 * When to use it (one MI355X, 1280x720, tlas_scene.xml, profiles/render_poses.json): 64 poses of one frame each take 225 ms against 1 983 ms for the loop above (8.8x) and
 * no longer than crt_render_views takes for the same cameras over a static scene (229 ms); 16 poses x 64 frames take 424 ms against 760 ms (1.79x; static: 400 ms).  The
 * builds by themselves: 64 poses of 40 / 256 instances cost 0.26 / 0.64 ms inside the entry against 11.7 / 64.9 ms for 64 crt_update_transforms_device calls.  The entry
 * beat the loop at every shape measured; crt_render_views' rule (from 256 frames per view on, loop crt_render) was not measured again for poses. */
int  crt_render_poses(crt_ctx* ctx, const float* cams /* K * 12 */, uint32_t K, const float* T /* P * blasCount * 16 */, uint32_t P, uint32_t blasCount,
                      const int32_t* view_pose /* K, or NULL */, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                      float* out_rgba /* K * W*H float4 */, uint32_t* out_pixels /* K * W*H or NULL */,
                      crt_tlas_node* tlas_out /* host, P * 2 * blasCount, or NULL */);                                                       /* host pointers, synchronous */
int  crt_render_poses_device(crt_ctx* ctx, const float* d_cams, uint32_t K, const float* d_T, uint32_t P, uint32_t blasCount, const int32_t* d_view_pose /* or NULL */,
                             uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba, uint32_t* d_out_pixels /* or NULL */,
                             crt_tlas_node* tlas_out /* host, or NULL */, void* stream);                                                      /* device pointers, one host wait */

/* The frames of MANY cameras over MANY LOOKS of the live scene in one render job: a material sweep, a relighting turntable, a moving light, the candidates of a
 * derivative-free optimiser over material parameters, a training set with randomised appearance.  The loop that changes the look between views — crt_update_look,
 * crt_set_camera, crt_clear, crt_render, crt_read_accumulator — renders every variant one lane wide.  Here one build launch (device/look_build.hip) turns the L look
 * records into a job-local table of device Material records and one light / floor-material / sky block per look, and every lane of crt_render_views' launch shades
 * with the look of its own view (device/render_looks.h).  Geometry, trees and texels are shared.  ABI version 3 still: additions, detected by symbol.
 * cams: K records of 12 floats, crt_set_camera's arguments.  looks: L records of crt_look_words(materialCount) words each (crt_update_look's argument).  view_look:
 * K indices into the looks, or NULL: view k renders look k, and L must equal K.
 * For every view k, with l = view_look[k], and every pixel of a tile this context owns: out_rgba[k] (W * H float4) is bit for bit what crt_update_look(looks[l]);
 * crt_set_camera(cams[k]); crt_clear; crt_render(spp_first, frames, passes); crt_read_accumulator leaves there, w = 0 included; out_pixels[k] (W * H, may be NULL) is
 * crt_resolve_screen(scale)'s pixel of that accumulator.  No other pixel of the outputs is touched.
 * THE LIVE SCENE IS NOT CHANGED: its look, the context's camera, the accumulator, the epoch and crt_tick's rendered-ahead frames stay as they are.  Looks are
 * job-local: they live in the scratch crt_render_poses keeps its poses in, at most 4 GiB of it (128 + 32 (2 + materialCount) bytes per look, rounded up to 128).
 * Counters: crt_counters.rays, primary and mesh_hits grow as they would for the K renders.
 * Ordering: the call is a reader under the scene-write protocol, exactly like crt_render_views_device.  THE ONE HOST WAIT (both entries; besides growing scratch): a
 * job with a texture index or a view_look entry out of range must not run, so the call reads the build's 64-byte status header back (pinned) and returns from that
 * wait before it enqueues the render launches.  crt_render_looks_device: d_cams (48 K bytes), d_looks (4 L crt_look_words bytes), d_view_look (4 K, or NULL),
 * d_out_rgba (16 K W H, 16-byte aligned), d_out_pixels (4 K W H, or NULL) are device pointers on cfg.device, checked as crt_render_views_device checks its buffers;
 * the records are never read on the host.  crt_render_looks: host pointers, synchronous, through staging the context keeps; it checks the records on the host first.
 * Refusals (nothing is written, crt_last_error says why): no scene CRT_ERR_STATE; a PrimitiveScene CRT_ERR_UNSUPPORTED; passes outside 1..4 CRT_ERR_INVALID;
 * K * frames > 2^31-1 CRT_ERR_UNSUPPORTED; crt_set_render_accel != 0 CRT_ERR_UNSUPPORTED (looks through the KD-tree / grid: not built); L == 0 with K > 0, or
 * view_look NULL with L != K, CRT_ERR_INVALID; a look table beyond 4 GiB CRT_ERR_UNSUPPORTED; NULL, misaligned, host or other-device memory, a stream of another
 * device CRT_ERR_INVALID; a view_look entry outside [0, L) CRT_ERR_INVALID; a floorTexture / skyTexture outside [0, textureCount) or a material's texture outside
 * [-1, textureCount) in ANY look, used by a view or not, CRT_ERR_INVALID (crt_last_error names the lowest such look and its first such field); a failed device
 * allocation CRT_ERR_DEVICE.  K == 0 or frames == 0 is a no-op after the checks that need no buffer. */
int  crt_render_looks(crt_ctx* ctx, const float* cams /* K * 12 */, uint32_t K, const void* looks /* L * crt_look_words(materialCount) words */, uint32_t L,
                      const int32_t* view_look /* K, or NULL */, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                      float* out_rgba /* K * W*H float4 */, uint32_t* out_pixels /* K * W*H or NULL */);                                     /* host pointers, synchronous */
int  crt_render_looks_device(crt_ctx* ctx, const float* d_cams, uint32_t K, const void* d_looks, uint32_t L, const int32_t* d_view_look /* or NULL */,
                             uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba, uint32_t* d_out_pixels /* or NULL */,
                             void* stream);                                                                                                    /* device pointers, one host wait */

/* The frames of MANY cameras over MANY SHAPES of one refitted BVH in one render job: skinning, cloth, the candidates of an optimiser over vertices — callers whose
 * vertex positions already live in device memory.  crt_render_views renders K cameras over the one live scene and crt_render_poses moves a two-level scene's
 * instances; the loop that deforms a mesh between views — crt_refit_device (one host wait), for a two-level scene crt_update_transforms_device (another),
 * crt_set_camera, crt_clear, crt_render, crt_read_accumulator — pays the one-frame render and the waits K times, and can hold only one shape at a time because the
 * live BVH is refitted in place.  Here the S shapes are built side by side (device/shape_build.hip: a leaf launch over (leaf slot, shape) and a box launch of one
 * workgroup per shape, then for a two-level scene the S TLAS builds in one launch), each into a job-local image: the refitted node pairs and leaf triangles of BVH
 * `bvh`, and for a two-level scene a pose as crt_render_poses keeps it; every lane of crt_render_views' launch walks the image of its own view's shape
 * (device/render_shapes.h).  Shading records, the other BVHs and the textures are shared.  ABI version 3 still: additions, detected by symbol.  ONE BVH deforms
 * per job here; a two-level scene in which several BLASes deform at the same time goes to crt_render_shape_sets, below.
 * cams: K records of 12 floats, crt_set_camera's arguments.  positions: S * triCount * 9 floats, shape s's at positions + 9 * triCount * s, each exactly what
 * crt_refit_device takes as d_positions (vertex0, vertex1, vertex2 per triangle in the reference's triangle order; not validated, as there).  T: S * blasCount
 * row-major mat4s, shape s's at T + 16 * blasCount * s, each what crt_update_transforms_device takes; NULL with blasCount 0 for a CRT_SCENE_FILE scene.
 * view_shape: K indices into the shapes, or NULL: view k renders shape k, and S must equal K.
 * For every view k, with s = view_shape[k], and every pixel of a tile this context owns: out_rgba[k] (W * H float4) is bit for bit what
 * crt_refit_device(bvh, positions[s]); for a two-level scene crt_update_transforms_device(T[s]); crt_set_camera(cams[k]); crt_clear; crt_render(spp_first, frames,
 * passes); crt_read_accumulator leaves there on a context in the same live state, w = 0 included; out_pixels[k] (W * H, may be NULL) is crt_resolve_screen(scale)'s
 * pixel of that accumulator; root_box_out[s] (host memory in BOTH entries, 6 floats per shape, may be NULL) is crt_refit_device's rootBox; tlas_out[s] (host memory
 * in both entries, 2 * blasCount nodes per shape, may be NULL; not written for a CRT_SCENE_FILE scene) is byte for byte crt_update_transforms_device's tlasOut.
 * No other pixel of the outputs is touched.  Refit's quirk is kept: node 1 keeps the box THE LIVE SCENE holds, and that box feeds node 0's.  No refit ever writes
 * node 1, so the shapes of a job do not depend on each other or on their order.
 * THE LIVE SCENE IS NOT CHANGED: the geometry, the node-0 boxes, the TLAS, the KD-tree / grid sets, the host mirror and the epoch stay as they are, and so do
 * crt_tick's rendered-ahead frames, the context's camera and the accumulator.  Shapes are job-local: they live in the scratch crt_render_poses keeps its poses in
 * (kept until crt_destroy), at most 4 GiB of it (64 bytes per node pair + 48 per triangle, + about 256 * blasCount per shape of a two-level scene).
 * Counters: crt_counters.rays, primary and mesh_hits grow as they would for the K renders.
 * Ordering: the call is a reader under the scene-write protocol, exactly like crt_render_poses_device.  THE ONE HOST WAIT (both entries; besides growing scratch
 * and the BVH's refit plan, built by the first call as crt_refit_device builds it): a job with a view_shape entry out of range or a failed TLAS build must not run,
 * and the launches' LDS stack is sized by the tallest shape's TLAS — so the call reads the flag and, for a two-level scene, the S build headers back (64 (S + 1)
 * bytes, pinned; with root_box_out the boxes, with tlas_out the node sections too) and returns from that wait before it enqueues the render launches.
 * crt_render_shapes_device: d_cams (48 K bytes), d_positions (36 S triCount), d_T (64 S blasCount, or NULL), d_view_shape (4 K, or NULL), d_out_rgba (16 K W H,
 * 16-byte aligned), d_out_pixels (4 K W H, or NULL) are device pointers on cfg.device, checked as crt_render_views_device checks its buffers; `stream` a
 * hipStream_t of that device or NULL.  crt_render_shapes: host pointers, synchronous, through staging the context keeps.
 * Refusals (nothing is written, crt_last_error says why), in this order: no scene CRT_ERR_STATE; a PrimitiveScene CRT_ERR_UNSUPPORTED; `bvh` out of range, or
 * triCount different from the uploaded BVH's, CRT_ERR_INVALID; a CRT_SCENE_FILE scene with T != NULL or blasCount != 0 CRT_ERR_INVALID; a two-level scene with
 * T == NULL or blasCount != bvhCount CRT_ERR_INVALID; a two-level scene uploaded with a TLAS node count other than 2 * bvhCount CRT_ERR_UNSUPPORTED; passes outside
 * 1..4 CRT_ERR_INVALID; K * frames > 2^31-1 CRT_ERR_UNSUPPORTED; crt_set_render_accel != 0 CRT_ERR_UNSUPPORTED (a refit drops those sets anyway); S == 0 with
 * K > 0, or view_shape NULL with S != K, CRT_ERR_INVALID; a shape table beyond 4 GiB CRT_ERR_UNSUPPORTED; NULL, misaligned, host or other-device memory, a stream of
 * another device CRT_ERR_INVALID; a view_shape entry outside [0, S) CRT_ERR_INVALID (the host entry looks before anything runs; the device entry checks in the
 * build launch and learns of it with the header); a shape whose TLAS build has a FindBestMatch without a candidate while more than one node is open
 * CRT_ERR_INVALID (crt_last_error names the first such shape and the call); a TLAS height that puts the traversal stack beyond the sequential kernels' LDS bound
 * CRT_ERR_UNSUPPORTED; a failed device allocation CRT_ERR_DEVICE.  K == 0 or frames == 0 is a no-op after the checks that need no buffer.
 * When to use it (one MI355X, 1280x720, profiles/render_shapes.json): 64 shapes of one frame each take 212 ms against 1 415 ms for the loop above on the bunny
 * FileScene (6.7x) and 223 ms against 1 986 ms on tlas_scene.xml (8.9x).  The advantage shrinks with the frames per view: 16 shapes x 64 frames 466 against 504 ms
 * (bunny, 1.08x) and 404 against 758 ms (two-level, 1.88x); at 8 x 128 the loop is the better call on the bunny (380 against 435 ms) and the entry still on the
 * two-level scene (382 against 606 ms); at 4 x 256 the loop wins on both (190 against 382 ms, 303 against 363 ms).  So: up to 64 frames per view call the entry, from
 * 256 on loop crt_refit_device + crt_render, in between measure.  The 64 shape builds by themselves cost 0.21 ms (bunny, 4 968 triangles) / 0.20 ms (a BLAS of
 * 2 992 triangles + 64 TLAS builds) inside the entry against 7.3 / 12.1 ms for 64 crt_refit_device (+ crt_update_transforms_device) calls. */
int  crt_render_shapes(crt_ctx* ctx, const float* cams /* K * 12 */, uint32_t K, uint32_t bvh, const float* positions /* S * triCount * 9 */, uint32_t S, uint32_t triCount,
                       const float* T /* S * blasCount * 16; NULL for a CRT_SCENE_FILE scene */, uint32_t blasCount, const int32_t* view_shape /* K, or NULL */,
                       uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* out_rgba /* K * W*H float4 */, uint32_t* out_pixels /* K * W*H or NULL */,
                       float* root_box_out /* host, S * 6, or NULL */, crt_tlas_node* tlas_out /* host, S * 2 * blasCount, or NULL */);         /* host pointers, synchronous */
int  crt_render_shapes_device(crt_ctx* ctx, const float* d_cams, uint32_t K, uint32_t bvh, const float* d_positions, uint32_t S, uint32_t triCount, const float* d_T /* or NULL */,
                              uint32_t blasCount, const int32_t* d_view_shape /* or NULL */, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* d_out_rgba,
                              uint32_t* d_out_pixels /* or NULL */, float* root_box_out /* host, or NULL */, crt_tlas_node* tlas_out /* host, or NULL */,
                              void* stream);                                                                                                   /* device pointers, one host wait */

/* The same job with SEVERAL deforming meshes: M >= 1 BLASes of a two-level scene deform per shape — two skinned characters, a cloth on a body, an optimiser over the
 * vertices of more than one object.  A crt_render_shapes job per BLAS cannot put them into one image, and the loop pays crt_refit_device's host wait once per mesh.
 * bvhs (HOST memory in both entries): M distinct BLAS indices, in any order.  setTris: the sum over m of the uploaded triCount of bvhs[m].  positions: S * setTris * 9
 * floats, shape s's at positions + 9 * setTris * s: BVH bvhs[0]'s triangles first, then bvhs[1]'s, and so on, each block exactly what crt_refit_device takes for
 * that BVH.  cams, T, view_shape, spp_first, frames, passes, scale, out_rgba, out_pixels: crt_render_shapes' (T is never NULL: two-level scenes only).
 * The contract is crt_render_shapes' with "the BVH" replaced by "every BVH of the set": for view k with s = view_shape[k], out_rgba[k] is bit for bit what
 * crt_refit_device(bvhs[m], its block of positions[s]) for every m (in any order); crt_update_transforms_device(T[s]); crt_set_camera(cams[k]); crt_clear;
 * crt_render(spp_first, frames, passes); crt_read_accumulator leaves on a context in the same live state; out_pixels[k] is crt_resolve_screen(scale)'s pixel of
 * that; root_box_out[(s * M + m) * 6 ..] (host, may be NULL) is that refit's rootBox; tlas_out[s] (host, may be NULL) is byte for byte
 * crt_update_transforms_device's tlasOut.  Refit's skipped node 1 is kept PER BVH: node 1 of each deforming BVH keeps the box the live scene holds.  The live scene,
 * crt_tick's rendered-ahead frames, the camera and the accumulator are not changed; counters grow as crt_render_shapes' do; the job is a reader under the
 * scene-write protocol; the one host wait is crt_render_shapes' (the job header plus the S build headers, with the boxes and nodes when asked for; besides growing
 * scratch and the refit plans of the set's BVHs, each built by the first call that names it).  Scratch is the table crt_render_poses / crt_render_shapes keep, at
 * most 4 GiB: per shape 64 bytes per node pair and 48 per triangle of every BVH of the set + about 256 * blasCount.  With M = 1 the entry gives bit for bit what
 * crt_render_shapes gives for the same job.
 * How: device/shape_build.hip refits the M * S BVHs side by side in ONE leaf launch over (leaf slot of the set, shape) and ONE box launch of a workgroup per
 * (shape, mesh), whatever M is; workgroup (s, m) writes entry bvhs[m] of shape s's row of node-0 boxes, over which the S TLAS builds run as they do for
 * crt_render_shapes.  An image holds the M sub-images and the pose; references in every sub-image are relative to the image's first byte, so a lane still needs one
 * offset.  The render kernel (device/render_shape_sets.h) looks an instance up in a table of blasCount words: the image-relative root of its BVH, or "walk the
 * live geometry".
 * Refusals (nothing is written, crt_last_error says why), in this order: no scene CRT_ERR_STATE; a PrimitiveScene CRT_ERR_UNSUPPORTED; a CRT_SCENE_FILE scene
 * CRT_ERR_INVALID (it has one BVH: crt_render_shapes); bvhs NULL, or M == 0 with K > 0, CRT_ERR_INVALID; a bvhs entry out of range or named twice CRT_ERR_INVALID
 * (crt_last_error names the entry); setTris different from the sum of the uploaded counts CRT_ERR_INVALID; then the remaining refusals of crt_render_shapes in its
 * order: T == NULL or blasCount != bvhCount CRT_ERR_INVALID; a TLAS node count other than 2 * bvhCount CRT_ERR_UNSUPPORTED; passes outside 1..4 CRT_ERR_INVALID;
 * K * frames > 2^31-1 CRT_ERR_UNSUPPORTED; crt_set_render_accel != 0 CRT_ERR_UNSUPPORTED; S == 0 with K > 0, or view_shape NULL with S != K, CRT_ERR_INVALID; a table
 * beyond 4 GiB CRT_ERR_UNSUPPORTED; NULL, misaligned, host or other-device memory, a stream of another device CRT_ERR_INVALID; a view_shape entry outside [0, S)
 * CRT_ERR_INVALID; a shape whose TLAS build finds no candidate (non-finite positions of any mesh of the shape among the causes) CRT_ERR_INVALID, crt_last_error
 * names the shape; a TLAS too tall for the LDS stack CRT_ERR_UNSUPPORTED; a failed device allocation CRT_ERR_DEVICE.  K == 0 or frames == 0 is a no-op after the
 * checks that need no buffer.
 * When to use it (one MI355X, 1280x720, tlas_scene.xml with all three BLASes deforming, profiles/render_shape_sets.json): 64 shapes of one frame each take 252 ms against 2 261 ms for the loop
 * (9.0x: 3 crt_refit_device + crt_update_transforms_device, crt_set_camera, crt_clear, crt_render, crt_sync per shape); 16 shapes x 64 frames 478 against 831 ms (1.74x);
 * at 4 x 256 the loop wins (338 against 436 ms).  So, as for crt_render_shapes: up to 64 frames per view call the entry, from 256 on loop crt_refit_device + crt_render, in
 * between measure.  The 64 x 3 shape builds by themselves cost 0.18 ms inside the entry against 26.2 ms for the 64 x 4 calls.  The per-instance lookup is not visible in the
 * wall time: with M = 1 the entry takes 215.4 ms against 211.0 ms for crt_render_shapes of the parent commit at 64 x 1 (1.02x, each side spreading over 192 - 243 ms) and
 * 396.9 against 403.4 ms at 16 x 64 (0.98x). */
int  crt_render_shape_sets(crt_ctx* ctx, const float* cams /* K * 12 */, uint32_t K, const uint32_t* bvhs /* host, M */, uint32_t M, const float* positions /* S * setTris * 9 */,
                           uint32_t S, uint32_t setTris, const float* T /* S * blasCount * 16 */, uint32_t blasCount, const int32_t* view_shape /* K, or NULL */,
                           uint32_t spp_first, uint32_t frames, uint32_t passes, float scale, float* out_rgba /* K * W*H float4 */, uint32_t* out_pixels /* K * W*H or NULL */,
                           float* root_box_out /* host, S * M * 6, or NULL */, crt_tlas_node* tlas_out /* host, S * 2 * blasCount, or NULL */);     /* host pointers, synchronous */
int  crt_render_shape_sets_device(crt_ctx* ctx, const float* d_cams, uint32_t K, const uint32_t* bvhs /* host, M */, uint32_t M, const float* d_positions, uint32_t S, uint32_t setTris,
                                  const float* d_T, uint32_t blasCount, const int32_t* d_view_shape /* or NULL */, uint32_t spp_first, uint32_t frames, uint32_t passes, float scale,
                                  float* d_out_rgba, uint32_t* d_out_pixels /* or NULL */, float* root_box_out /* host, or NULL */, crt_tlas_node* tlas_out /* host, or NULL */,
                                  void* stream);                                                                                               /* device pointers, one host wait */

/* ---- PrimitiveScene (second half): infra/scene/primitive_scene.cpp — the reference's hard-coded demo room (six walls, swinging light quad,
 * bouncing mirror ball, "rounded corners" sphere, spinning glass cube, glass torus; template/primitives.h Sphere :31, Cube :187, Quad :321, Torus :380; the
 * SPEEDTRIX / single-light configuration its headers select).  The binding passes the scene as its constructor + SetTime(t) leave it: the members below.
 * After crt_upload_primitive_scene, crt_render (Renderer::Sample), crt_find_nearest (objIdx 0 .. 10, u = v = 0, triIdx = -1) and the accumulator entry points
 * work on this scene (it replaces an uploaded triangle scene; crt_whitted_tick, crt_update_scene and the alternative accelerators do not apply).
 * PARITY UNPINNED: checked bit for bit against the repo's oracle only (the reference files need MSVC); the torus' double-precision cos(acos(x) / 3) is a
 * deterministic fdlibm-style evaluation on both sides, so its hit distances can differ from a Windows build of the reference in the last place. */
typedef struct crt_primitive_scene {
    float quadT[16], quadInvT[16]; float quadSize;             /* Quad quad: T, invT (FastInvertedTransformNoScale), size (= 0.5)            */
    float spherePos[3];                                        /* Sphere sphere (r = 0.6): pos; sphere2 is constant (0, 2.5, -3.07), r = 8      */
    float cubeMin[3], cubeMax[3], cubeM[16], cubeInvM[16];     /* Cube cube: b[0], b[1], M, invM                                               */
    float torusT[16], torusInvT[16];                           /* Torus torus: T, invT (mat4::Inverted)                                        */
    float torusRt2, torusRc2, torusR2;                         /*              rt2, rc2, r2                                                     */
    float reflectivity[11], refractivity[11], absorption[11][3];   /* Material materials[11] (isLight: index 0; isAlbedoOverridden: 4, 5, 6)   */
    crt_texture red, blue;                                     /* Plane::GetAlbedo's "../assets/red.png" / "blue.png" as Surface loads them (0x00RRGGBB, 512 x 512); pixels may be NULL */
} crt_primitive_scene;
int  crt_upload_primitive_scene(crt_ctx* ctx, const crt_primitive_scene* scene);

/* ---- instrumentation ---------------------------------------------------------------------------------- */
int  crt_get_counters(crt_ctx* ctx, crt_counters* out);        /* cumulative since create / crt_reset_counters       */
int  crt_reset_counters(crt_ctx* ctx);
int  crt_get_timing(crt_ctx* ctx, crt_timing* out);            /* syncs the stream                                   */
/* collectStats contexts only: for each owned tile i of the LAST render launch, out[2i] = wall time of the tile's
 * wavefront and out[2i+1] = its start stamp, both in ticks of the 100 MHz constant clock (load-balance map). */
int  crt_get_tile_clocks(crt_ctx* ctx, uint64_t* out /* 2 * tileCount */);

/* ---- multi-GPU plumbing ---------------------------------------------------------------------------------
 * The accumulator can live in caller-owned device memory (e.g. a torch tensor that torch.distributed/RCCL
 * reduces over xGMI).  Must be width*height*16 bytes, 16-byte aligned, on cfg.device.  NULL = back to internal. */
int  crt_bind_accumulator(crt_ctx* ctx, void* device_ptr);
int  crt_accumulator_device_ptr(crt_ctx* ctx, void** device_ptr);

#ifdef __cplusplus
}
#endif
#endif
