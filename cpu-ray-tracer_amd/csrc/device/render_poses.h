// render_poses.h — crt_render_poses: the frames of many cameras over many POSES of a two-level scene's instances in one job.  render_views_kernel (render_views.h)
// with one difference: a lane's world is not the launch's but one the lane builds for its view's pose.  A pose is a result block of the batched TLAS build
// (tlas_build.hip tlas_build_poses_kernel): an image of the geometry buffer's TLAS node, TLAS child pair and Instance sections, complete and relocatable because the
// BLAS trees, their triangles and the shading records are the same for every pose and stay where they are, in Scene::geom.
//
//   PoseWorld   trace:   hit_light_floor, then tlas_walk (dev_common.h) over the pose's TLAS nodes and Instance records, traverse_bvh_seq per instance over Scene::geom —
//                        find_nearest_seq's order, the functions it calls;
//               surface: FileSurface<1>'s, with mesh_point<1>'s Instance T rows read from the pose's records;
//               miss:    FileSurface<1>'s.
//
// Addressing: the table is one allocation of at most kMaxGeomBytes, so a lane names its pose by a 32-bit byte offset and every load is scalar base + per-lane offset
// (global_load_dwordx4 v, v_off, s[base:base+1]), exactly the form the walk uses on the geometry buffer; a per-lane 64-bit base would cost two registers per lane and a
// 64-bit add per fetch.  A lane keeps two words: the image's offset and node 0's reference (read once, at the top of the kernel).
// LDS: the by-value Scene of the launch is a copy of the context's whose stackDepth is the JOB's — bvhStack + the tallest pose's TLAS height + 1 — so every lane's
// column fits every pose of the job.
//
// Numerics: seq_sample.h's (-ffp-contract=off, IEEE + - * / sqrt).  No MFMA.
#pragma once
#include "file_surface.h"
#include "render_views.h"

namespace crt {

struct PoseWorld : FileSurface<1> {
    const char* table;                    // the pose table (wave-uniform)
    uint32_t image, inst, rootRef;        // this lane's pose: its image's offset in the table, its Instance records' offset, node 0's reference
    __device__ __host__ uint32_t stack_words(const Scene& sc) const { return sc.stackDepth; }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
        int traversed = 0, tested = 0;
        hit_light_floor(sc, O, D, h);
        // TLAS entries live above the BVH part of this lane's column, as in find_nearest_seq
        tlas_walk(*this, O, D, rD, h, stk + sc.bvhStack * 64, cn, traversed, [&](uint32_t, rec4 ids, f3 Oo, f3 Do, f3 rDo) __attribute__((always_inline)) {
            traverse_bvh_seq(sc, asu(ids.z), Oo, Do, rDo, h, stk, cn, traversed, tested);
        });
        return 0u;
    }
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D) const { return surface_of(sc, h, I, D, table, inst); }
};

// where tlas_walk finds a lane's TLAS (dev_common.h)
__device__ __forceinline__ const char* tlas_base(const PoseWorld& w) { return w.table; }
__device__ __forceinline__ uint32_t tlas_nodes(const PoseWorld& w) { return w.image; }
__device__ __forceinline__ uint32_t tlas_insts(const PoseWorld& w) { return w.inst; }
__device__ __forceinline__ uint32_t tlas_root(const PoseWorld& w) { return w.rootRef; }

// the pose of `view`: an index the build launch has found to lie in [0, P) before this kernel is launched
__device__ __forceinline__ PoseWorld pose_world(const PoseTableDev& pt, uint32_t view)
{
    const uint32_t p = pt.viewPose ? (uint32_t)pt.viewPose[view] : view;
    PoseWorld w;
    w.table = pt.table; w.image = pt.imagesOff + p * pt.imageStride; w.inst = w.image + pt.instRel;
    w.rootRef = asu(ldg(pt.table, w.image).w);                                       // TlasNode 0: {lo, ref}
    return w;
}

// render_views_kernel's launch shape, slab, seeds and camera handling (render_views.h: entry = tile rank * windows + window, lane = view-frame, the camera read again
// per pixel); the path itself is sample_step / sample_unwind over the lane's PoseWorld.
__global__ __launch_bounds__(256, 4) void render_poses_kernel(const Scene sc, const PoseTableDev pt, const float* __restrict__ cams, char* __restrict__ slab,
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
    const PoseWorld world = pose_world(pt, view);
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
        while (!sample_step<PoseWorld, false>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {}
        sample_unwind(fst, depth, L);
        uint32_t pass = 0;
        if (passes != 1u) pass = item - pix * passes;
        store_sample(slab, slab_sample_offset(lane, pix, 64u * passes, passes, pass), L);
    }
    atomicAdd(&counters->v[0], (unsigned long long)nRays);
    atomicAdd(&counters->v[1], (unsigned long long)nPrimary);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

} // namespace crt
