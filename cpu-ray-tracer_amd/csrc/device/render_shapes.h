// render_shapes.h — crt_render_shapes: the frames of many cameras over many SHAPES of one refitted BVH in one job.  render_views_kernel (render_views.h) with one
// difference: a lane's world is not the launch's but one the lane builds for its view's shape.  A shape is an image in the job's shape table (shape_build.hip,
// layout.h ShapeJobHeader): the refitted NodePairs and LeafTris of the one BVH that deforms and, for a two-level scene, a pose image of the TLAS built over that
// shape's root box (tlas_build.hip tlas_build_shapes_kernel).  Shading records, the other BVHs and the textures are the same for every shape and stay in Scene::geom.
//
//   ShapeWorld<0>   trace:   hit_light_floor, then traverse_bvh_seq (dev_common.h) over the lane's image — find_nearest_seq's order, the functions it calls;
//   ShapeWorld<1>   trace:   hit_light_floor, then tlas_walk over the image's TLAS nodes and Instance records (PoseWorld's, render_poses.h); the ONE instance whose BLAS
//                            deforms is walked in the lane's image, every other instance in Scene::geom;
//                   surface: FileSurface<KIND>'s (KIND 1: mesh_point<1>'s Instance T rows read from the image's records);  miss: FileSurface<KIND>'s.
//
// Relocation: references inside a node pair are absolute 16-byte offsets into Scene::geom.  The box kernel rewrites them image-relative while it copies the pairs
// (it touches every pair anyway), so ONE per-lane delta — the image's offset in the table — serves interior and leaf references alike: a record's offset is
// image + (ref << 4), one v_lshl_add_u32 where the walk over the geometry buffer has one v_lshlrev_b32.  A dense image of the pairs and leaves as they are would need
// two deltas and a select on the interior bit in front of every fetch.
// Addressing: the table is one allocation of at most kMaxGeomBytes, so every load is scalar base + 32-bit per-lane offset, as PoseWorld's.
// LDS: the by-value Scene of the launch is a copy of the context's whose stackDepth is the JOB's — bvhStack + the tallest shape's TLAS height + 1 (a FileScene's: the
// context's own; Refit keeps the topology).
//
// Numerics: seq_sample.h's (-ffp-contract=off, IEEE + - * / sqrt; box_exact, hit_tri, rcp_exact through the shared walk).  No MFMA.
#pragma once
#include "file_surface.h"
#include "render_views.h"

namespace crt {

// where traverse_bvh_seq finds a lane's BVH (dev_common.h)
struct ShapeBvh { const char* table; uint32_t image; };
__device__ __forceinline__ const char* bvh_base(const ShapeBvh& w) { return w.table; }
__device__ __forceinline__ uint32_t bvh_record(const ShapeBvh& w, uint32_t ref) { return w.image + ((ref & kRefOffsetMask) << 4); }

template <int KIND>
struct ShapeWorld : FileSurface<KIND> {
    static constexpr int kind = KIND;
    const char* table;                    // the shape table (wave-uniform)
    uint32_t image;                       // this lane's shape: its image's offset in the table
    uint32_t rootRef, bvh;                // the refitted BVH's node 0 (image-relative) and, KIND 1, the instance that walks it (both wave-uniform)
    uint32_t tlas, inst, tlasRoot;        // KIND 1: the image's TLAS nodes, its Instance records, node 0's reference
    __device__ __host__ uint32_t stack_words(const Scene& sc) const { return sc.stackDepth; }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
        int traversed = 0, tested = 0;
        const ShapeBvh mine{table, image};
        hit_light_floor(sc, O, D, h);
        if constexpr (KIND == 0) traverse_bvh_seq(mine, rootRef, O, D, rD, h, stk, cn, traversed, tested);
        else {
            // TLAS entries live above the BVH part of this lane's column, as in find_nearest_seq
            tlas_walk(*this, O, D, rD, h, stk + sc.bvhStack * 64, cn, traversed, [&](uint32_t instance, rec4 ids, f3 Oo, f3 Do, f3 rDo) __attribute__((always_inline)) {
                if (instance == bvh) traverse_bvh_seq(mine, rootRef, Oo, Do, rDo, h, stk, cn, traversed, tested);
                else traverse_bvh_seq(sc, asu(ids.z), Oo, Do, rDo, h, stk, cn, traversed, tested);
            });
        }
        return 0u;
    }
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D) const
    {
        if constexpr (KIND == 0) return this->surface_of(sc, h, I, D, sc.geom, sc.instOff);
        else return this->surface_of(sc, h, I, D, table, inst);
    }
};

// where tlas_walk finds a lane's TLAS (dev_common.h)
__device__ __forceinline__ const char* tlas_base(const ShapeWorld<1>& w) { return w.table; }
__device__ __forceinline__ uint32_t tlas_nodes(const ShapeWorld<1>& w) { return w.tlas; }
__device__ __forceinline__ uint32_t tlas_insts(const ShapeWorld<1>& w) { return w.inst; }
__device__ __forceinline__ uint32_t tlas_root(const ShapeWorld<1>& w) { return w.tlasRoot; }

// the shape of `view`: an index the build launch has found to lie in [0, S) before this kernel is launched
template <class WORLD>
__device__ __forceinline__ WORLD world_of(const ShapeTableDev& t, uint32_t view)
{
    constexpr int KIND = WORLD::kind;
    const uint32_t s = t.viewShape ? (uint32_t)t.viewShape[view] : view;
    WORLD w;
    w.table = t.table; w.image = t.imagesOff + s * t.imageStride; w.rootRef = t.rootRef; w.bvh = t.bvh;
    w.tlas = w.image + t.poseRel; w.inst = w.tlas + t.instRel;
    w.tlasRoot = 0u;
    if constexpr (KIND == 1) w.tlasRoot = asu(ldg(t.table, w.tlas).w);               // TlasNode 0: {lo, ref}
    return w;
}

// render_views_kernel's launch shape, slab, seeds and camera handling (render_views.h: entry = tile rank * windows + window, lane = view-frame, the camera read again
// per pixel); the path itself is sample_step / sample_unwind over the lane's ShapeWorld.
// (the body of render_shapes_kernel and of render_shape_sets_kernel, render_shape_sets.h: WORLD is the lane's world, world_of(st, view) makes it)
template <class WORLD, class TABLE>
__device__ __forceinline__ void render_shape_lanes(const Scene& sc, const TABLE& st, const float* __restrict__ cams, char* __restrict__ slab, Counters* __restrict__ counters,
                                                   uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes,
                                                   uint32_t jFirst, uint32_t nj, uint32_t nEntries)
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
    const WORLD world = world_of<WORLD>(st, view);
    // this lane's LDS columns: the traversal stack (the job's depth), then the throughput factors
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
        const uint32_t pix = (passes == 1u) ? item : item / passes;
        const f3 camPos = mk3(cam[0], cam[1], cam[2]);
        const f3 TL = mk3(cam[3], cam[4], cam[5]), TR = mk3(cam[6], cam[7], cam[8]), BL = mk3(cam[9], cam[10], cam[11]);
        const f3 v = primary_target(camPos, TL, TR - TL, BL - TL, invW, invH, tx, ty, pix, seed);
        f3 O = camPos, D = v * rcp_exact(sqrt_exact(dot3(v, v)));                 // normalize()
        bool inside = false; int depth = 0;
        nPrimary++;
        f3 L = mk3(0, 0, 0);
        while (!sample_step<WORLD, false>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {}
        sample_unwind(fst, depth, L);
        uint32_t pass = 0;
        if (passes != 1u) pass = item - pix * passes;
        store_sample(slab, slab_sample_offset(lane, pix, 64u * passes, passes, pass), L);
    }
    atomicAdd(&counters->v[0], (unsigned long long)nRays);
    atomicAdd(&counters->v[1], (unsigned long long)nPrimary);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

template <int KIND>
__global__ __launch_bounds__(256, 4) void render_shapes_kernel(const Scene sc, const ShapeTableDev st, const float* __restrict__ cams, char* __restrict__ slab,
                                                              Counters* __restrict__ counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                              uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, uint32_t nEntries)
{
    render_shape_lanes<ShapeWorld<KIND>>(sc, st, cams, slab, counters, tileFirst, tileStride, tileCount, tilesX, sppFirst, frames, passes, jFirst, nj, nEntries);
}

} // namespace crt
