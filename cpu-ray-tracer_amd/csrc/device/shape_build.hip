// shape_build.hip — crt_render_shapes: BVH::Refit (infra/bvh.cpp:26-61) of ONE BVH for S sets of vertex positions at once, each into a job-local image of the BVH's
// node pairs and leaf triangles (layout.h ShapeJobHeader).  refit.hip does this in place, so only one shape can exist at a time; here the live geometry buffer is
// only read, and the S shapes are built side by side in two launches:
//
//   shape_leaf_kernel  one lane per (leaf slot, shape): the live LeafTri with v0, v1 - v0, v2 - v0 from positions[s], stored into image s (refit_leaf_kernel's
//                      arithmetic; the fourth dword of each row as the live record has it).
//   shape_box_kernel   ONE workgroup per shape.  It copies the BVH's live pairs into the image — boxes as they are, so node 1 keeps the box the live scene holds
//                      (bvh.cpp:28), references rewritten image-relative — and then runs refit_box_kernel's level-by-level pass over the context's plan inside the
//                      image, with __syncthreads() between the levels.  Leaf boxes come from the caller's positions and the LIVE leaf records' remain / shadeIdx
//                      words, which no refit changes: the two kernels do not depend on each other.  Thread 0 then writes node 0's box into the shape's row of
//                      root boxes — the live row with this BVH's entry replaced: what crt_update_transforms_device finds in dRootBox after crt_refit_device.
//                      The same launch looks at the job's view -> shape indices (workgroup s takes every S-th group of 1024): an index outside [0, S) lowers
//                      ShapeJobHeader::badView to its view (atomicMin on the word the host set to kPoseNoBadView).
//
// crt_render_shape_sets deforms M BLASes of a two-level scene per shape (layout.h ShapeSetMesh).  Its two kernels run the same device functions — shape_leaf, shape_refit,
// shape_root_box: ONE definition of the arithmetic — over per-mesh descriptors read from the table, still in two launches whatever M is:
//
//   shape_set_leaf_kernel  one lane per (leaf slot of the set, shape); the slot's mesh by a binary search over the descriptors.
//   shape_set_box_kernel   ONE workgroup per (shape, mesh): sub-image m of image s, references relative to the IMAGE's first byte, and entry bvhs[m] of the shape's
//                          row; mesh 0's workgroup copies the live boxes of the instances that do not deform.  The view -> shape check strides over all workgroups.
//
// No refit ever writes node 1, so the S shapes are independent of each other and of their order.  No kernel here writes the geometry buffer.
// The comparison forms and node_box are refit_common.h's: one definition for this file and refit.hip.  -ffp-contract=off as everywhere.
#include "launch.h"
#include "refit_common.h"

namespace crt {

constexpr uint32_t kShapeBoxThreads = 1024u;

// one leaf slot of one shape of one BVH: the live LeafTri `j` of the BVH with its vertices from `pos` (the shape's triangles of this BVH), stored as record j of `leaves`
__device__ __forceinline__ void shape_leaf(const char* geom, uint32_t leafOff, uint32_t triBase, uint32_t triCount, const float* pos, char* leaves, uint32_t j)
{
    const row4* lt = reinterpret_cast<const row4*>(geom + leafOff + (size_t)(triBase + j) * 48u);
    row4* out = reinterpret_cast<row4*>(leaves + (size_t)j * 48u);
    row4 r0 = lt[0], r1 = lt[1], r2 = lt[2];
    const uint32_t tri = __float_as_uint(r0.w) - triBase;
    if (tri < triCount) {                                                          // (else the record as it is: refit_leaf_kernel leaves such a slot alone)
        const float* v = pos + (size_t)tri * 9u;
        const float v0x = v[0], v0y = v[1], v0z = v[2];
        r0.x = v0x; r0.y = v0y; r0.z = v0z;
        r1.x = v[3] - v0x; r1.y = v[4] - v0y; r1.z = v[5] - v0z;
        r2.x = v[6] - v0x; r2.y = v[7] - v0y; r2.z = v[8] - v0z;
    }
    out[0] = r0; out[1] = r1; out[2] = r2;
}

__global__ __launch_bounds__(256) void shape_leaf_kernel(const ShapeBuildDev b, uint32_t blocksPerShape)
{
    const uint32_t s = blockIdx.x / blocksPerShape, j = (blockIdx.x - s * blocksPerShape) * 256u + threadIdx.x;
    if (s >= b.S || j >= b.triCount) return;
    shape_leaf(b.geom, b.leafOff, b.triBase, b.triCount, b.pos + (size_t)s * b.triCount * 9u, b.table + b.imagesOff + (size_t)s * b.imageStride + b.leafRel, j);
}

// the same for a set (crt_render_shape_sets): one lane per (leaf slot of the set, shape); slot j belongs to the last mesh whose triFirst is <= j
__global__ __launch_bounds__(256) void shape_set_leaf_kernel(const ShapeSetBuildDev b, uint32_t blocksPerShape)
{
    const uint32_t s = blockIdx.x / blocksPerShape, j = (blockIdx.x - s * blocksPerShape) * 256u + threadIdx.x;
    if (s >= b.S || j >= b.setTris) return;
    const ShapeSetMesh* meshes = reinterpret_cast<const ShapeSetMesh*>(b.table + b.meshOff);
    uint32_t lo = 0, hi = b.M;                                                     // triFirst[lo] <= j < triFirst[hi] (triFirst[0] = 0, triFirst[M] = setTris)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (meshes[mid].triFirst <= j) lo = mid; else hi = mid;
    }
    const ShapeSetMesh d = meshes[lo];
    if (j - d.triFirst >= d.triCount) return;
    shape_leaf(b.geom, b.leafOff, d.triBase, d.triCount, b.pos + ((size_t)s * b.setTris + d.triFirst) * 9u, b.table + b.imagesOff + (size_t)s * b.imageStride + d.leafRel, j - d.triFirst);
}

// the live BVH a workgroup refits and where in an image it goes: its pairs at pairRel, its leaves at leafRel, both from the image's first byte
struct ShapeMesh { uint32_t pairBase, pairCount, triBase, triCount, pairRel, leafRel; };

// a live reference of this BVH as the image's: the record's 16-byte offset from the image's first byte
__device__ __forceinline__ uint32_t image_ref(const ShapeMesh& m, uint32_t leafOff, uint32_t ref)
{
    if (ref & kRefInterior) return ref - m.pairBase * 4u + (m.pairRel >> 4);
    if (ref == kRefDone) return ref;
    return ref - ((leafOff + m.triBase * 48u) >> 4) + (m.leafRel >> 4);
}

// One workgroup, one shape of one BVH: the live pairs into the image — boxes as they are, references image-relative —, then refit_box_kernel's level-by-level pass
// inside the image.  pos: the shape's triangles of this BVH.
__device__ __forceinline__ void shape_refit(const char* geom, uint32_t leafOff, const ShapeMesh& m, char* image, const float* pos, const RefitPlanRec* __restrict__ plan,
                                            const uint32_t* __restrict__ levelOff, uint32_t levels)
{
    char* pairs = image + m.pairRel;
    // the live pairs, child by child: box and pool-form word as they are, the reference image-relative
    const row4* live = reinterpret_cast<const row4*>(geom + (size_t)m.pairBase * 64u);
    for (uint32_t i = threadIdx.x; i < 2u * m.pairCount; i += kShapeBoxThreads) {
        row4 lo = live[2 * i]; const row4 hi = live[2 * i + 1];
        lo.w = __uint_as_float(image_ref(m, leafOff, __float_as_uint(lo.w)));
        reinterpret_cast<row4*>(pairs)[2 * i] = lo; reinterpret_cast<row4*>(pairs)[2 * i + 1] = hi;
    }
    __syncthreads();
    for (uint32_t lvl = 0; lvl < levels; lvl++) {
        const uint32_t end = levelOff[lvl + 1];
        for (uint32_t i = levelOff[lvl] + threadIdx.x; i < end; i += kShapeBoxThreads) {
            const RefitPlanRec r = plan[i];
            if (r.pair >= m.pairCount) continue;                                    // (a plan never names a pair past the BVH; neither does this loop)
            row4* p = reinterpret_cast<row4*>(pairs + (size_t)r.pair * 64u);
            for (uint32_t k = 0; k < 2; k++) {
                if (r.pair == 0 && k == 0) continue;                               // node 1 = child 0 of the BVH's first pair: bvh.cpp:28
                if ((r.child[k] & kPlanInterior) && (r.child[k] & ~kPlanInterior) >= m.pairCount) continue;
                const Box x = node_box(pairs, geom, leafOff, 0u, m.triBase, m.triCount, pos, r.child[k]);
                row4 lo = p[2 * k], hi = p[2 * k + 1];                              // .w: ref / ref16 stay
                lo.x = x.lo[0]; lo.y = x.lo[1]; lo.z = x.lo[2]; hi.x = x.hi[0]; hi.y = x.hi[1]; hi.z = x.hi[2];
                p[2 * k] = lo; p[2 * k + 1] = hi;
            }
        }
        __syncthreads();                                                           // the next level reads what this one stored (same workgroup, same CU)
    }
}

// node 0's box of the refitted BVH into its entry of the shape's row of node-0 boxes (one thread, after shape_refit)
__device__ __forceinline__ void shape_root_box(const char* geom, uint32_t leafOff, const ShapeMesh& m, const char* image, const float* pos, uint32_t rootCode, float* entry)
{
    const bool ok = !(rootCode & kPlanInterior) || (rootCode & ~kPlanInterior) < m.pairCount;
    Box x;
    if (ok) x = node_box(image + m.pairRel, geom, leafOff, 0u, m.triBase, m.triCount, pos, rootCode);
    else for (int k = 0; k < 3; k++) { x.lo[k] = 1e30f; x.hi[k] = -1e30f; }
    for (int k = 0; k < 3; k++) { entry[k] = x.lo[k]; entry[3 + k] = x.hi[k]; }
}

__global__ __launch_bounds__(kShapeBoxThreads) void shape_box_kernel(const ShapeBuildDev b, const RefitPlanRec* __restrict__ plan, const uint32_t* __restrict__ levelOff, uint32_t levels,
                                                                     uint32_t rootCode, const int32_t* __restrict__ viewShape, uint32_t K)
{
    const uint32_t s = blockIdx.x;
    if (s >= b.S) return;
    if (viewShape)
        for (unsigned long long k = (unsigned long long)s * kShapeBoxThreads + threadIdx.x; k < K; k += (unsigned long long)b.S * kShapeBoxThreads)
            if ((uint32_t)viewShape[k] >= b.S) atomicMin(&reinterpret_cast<ShapeJobHeader*>(b.table)->badView, (uint32_t)k);
    char* image = b.table + b.imagesOff + (size_t)s * b.imageStride;
    const float* pos = b.pos + (size_t)s * b.triCount * 9u;
    const ShapeMesh m{b.pairBase, b.pairCount, b.triBase, b.triCount, 0u, b.leafRel};
    shape_refit(b.geom, b.leafOff, m, image, pos, plan, levelOff, levels);
    // the shape's row of node-0 boxes: the live ones, this BVH's from the image
    float* row = reinterpret_cast<float*>(b.table + b.rowsOff) + (size_t)s * b.rowFloats;
    if (b.liveRootBox)
        for (uint32_t i = threadIdx.x; i < b.rowFloats; i += kShapeBoxThreads)
            if (i / 6u != b.bvh) row[i] = b.liveRootBox[i];
    if (threadIdx.x == 0) shape_root_box(b.geom, b.leafOff, m, image, pos, rootCode, row + 6u * b.bvh);
}

// the same for a set: ONE workgroup per (shape, mesh), which refits mesh m's sub-image of image s and writes entry bvhs[m] of the shape's row.  Mesh 0's workgroup
// also copies the live boxes of the instances that do not deform, once per row.  The view -> shape check strides over all S M workgroups.
__global__ __launch_bounds__(kShapeBoxThreads) void shape_set_box_kernel(const ShapeSetBuildDev b, const int32_t* __restrict__ viewShape, uint32_t K)
{
    const uint32_t s = blockIdx.x / b.M, mi = blockIdx.x - s * b.M;
    if (s >= b.S) return;
    if (viewShape)
        for (unsigned long long k = (unsigned long long)blockIdx.x * kShapeBoxThreads + threadIdx.x; k < K; k += (unsigned long long)b.S * b.M * kShapeBoxThreads)
            if ((uint32_t)viewShape[k] >= b.S) atomicMin(&reinterpret_cast<ShapeJobHeader*>(b.table)->badView, (uint32_t)k);
    const ShapeSetMesh d = reinterpret_cast<const ShapeSetMesh*>(b.table + b.meshOff)[mi];
    char* image = b.table + b.imagesOff + (size_t)s * b.imageStride;
    const float* pos = b.pos + ((size_t)s * b.setTris + d.triFirst) * 9u;
    const ShapeMesh m{d.pairBase, d.pairCount, d.triBase, d.triCount, d.pairRel, d.leafRel};
    shape_refit(b.geom, b.leafOff, m, image, pos, d.plan, d.levelOff, d.levels);
    float* row = reinterpret_cast<float*>(b.table + b.rowsOff) + (size_t)s * b.rowFloats;
    if (mi == 0u) {
        const uint32_t* instRoot = reinterpret_cast<const uint32_t*>(b.table + b.instRootOff);
        for (uint32_t i = threadIdx.x; i < b.rowFloats; i += kShapeBoxThreads)
            if (instRoot[i / 6u] == kInstLive) row[i] = b.liveRootBox[i];
    }
    if (threadIdx.x == 0) shape_root_box(b.geom, b.leafOff, m, image, pos, d.rootCode, row + 6u * d.bvh);
}

} // namespace crt

// The S shapes of a job: the leaf launch and the box launch.  The caller has set ShapeJobHeader::badView to kPoseNoBadView on the stream and holds the table to
// rowsOff + 4 S rowFloats <= imagesOff, imagesOff + S imageStride <= kMaxGeomBytes, leafRel + 48 triCount <= imageStride.
extern "C" hipError_t crt_launch_shape_build(const crt::ShapeBuildDev* b, const void* plan, const uint32_t* levelOff, uint32_t levels, uint32_t rootCode, const int32_t* viewShape, uint32_t K,
                                             hipStream_t stream)
{
    if (b->S == 0u || (b->imagesOff & 127u) || (b->imageStride & 127u) || (b->leafRel & 63u) || b->leafRel < 64u || b->leafRel < (unsigned long long)b->pairCount * 64u) return hipErrorInvalidValue;
    if ((unsigned long long)b->imagesOff + (unsigned long long)b->S * b->imageStride > crt::kMaxGeomBytes) return hipErrorInvalidValue;   // the render kernel's 32-bit offsets into the table
    if ((unsigned long long)b->leafRel + (unsigned long long)b->triCount * 48u > b->imageStride) return hipErrorInvalidValue;
    if ((unsigned long long)b->rowsOff + (unsigned long long)b->S * b->rowFloats * 4u > b->imagesOff || 6u * b->bvh + 6u > b->rowFloats) return hipErrorInvalidValue;
    const uint32_t blocksPerShape = (b->triCount + 255u) / 256u;
    const unsigned long long blocks = (unsigned long long)blocksPerShape * b->S;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (blocks) {
        hipLaunchKernelGGL(crt::shape_leaf_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, *b, blocksPerShape);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crt::shape_box_kernel, dim3(b->S), dim3(crt::kShapeBoxThreads), 0, stream, *b, (const crt::RefitPlanRec*)plan, levelOff, levels, rootCode, viewShape, K);
    return hipGetLastError();
}

// The S shapes of a set job: ONE leaf launch over (leaf slot of the set, shape) and ONE box launch of a workgroup per (shape, mesh).  meshes / instRoot: the host's copy
// of the two tables the caller has put at b->meshOff / b->instRootOff on the stream (the bounds below are checked on it); the caller has set badView as above.
extern "C" hipError_t crt_launch_shape_set_build(const crt::ShapeSetBuildDev* b, const crt::ShapeSetMesh* meshes, const uint32_t* instRoot, const int32_t* viewShape, uint32_t K,
                                                 hipStream_t stream)
{
    const uint32_t N = b->rowFloats / 6u;
    if (b->S == 0u || b->M == 0u || b->M > N || b->rowFloats != 6u * N || !b->liveRootBox || (b->imagesOff & 127u) || (b->imageStride & 127u) || (b->meshOff & 15u) || (b->instRootOff & 3u))
        return hipErrorInvalidValue;
    if ((unsigned long long)b->imagesOff + (unsigned long long)b->S * b->imageStride > crt::kMaxGeomBytes) return hipErrorInvalidValue;   // the render kernel's 32-bit offsets into the table
    if ((unsigned long long)b->rowsOff + (unsigned long long)b->S * b->rowFloats * 4u > b->meshOff || (unsigned long long)b->meshOff + (unsigned long long)b->M * sizeof(crt::ShapeSetMesh) > b->instRootOff ||
        (unsigned long long)b->instRootOff + 4ull * N > b->imagesOff) return hipErrorInvalidValue;
    unsigned long long at = 0, tris = 0; uint32_t named = 0;
    for (uint32_t m = 0; m < b->M; m++) {                                          // sub-images in order, none over another, each inside the image
        const crt::ShapeSetMesh& d = meshes[m];
        if ((d.pairRel & 63u) || (d.leafRel & 15u) || d.pairRel < at || d.leafRel < 64u || d.leafRel < (unsigned long long)d.pairRel + (unsigned long long)d.pairCount * 64u) return hipErrorInvalidValue;
        at = (unsigned long long)d.leafRel + (unsigned long long)d.triCount * 48u;
        if (at > b->imageStride || d.triFirst != tris || d.bvh >= N || instRoot[d.bvh] == crt::kInstLive) return hipErrorInvalidValue;
        tris += d.triCount;
    }
    for (uint32_t i = 0; i < N; i++) named += instRoot[i] != crt::kInstLive;
    if (tris != b->setTris || named != b->M) return hipErrorInvalidValue;          // M distinct BVHs, every row entry written by exactly one workgroup or the copy
    const uint32_t blocksPerShape = (b->setTris + 255u) / 256u;
    const unsigned long long blocks = (unsigned long long)blocksPerShape * b->S, groups = (unsigned long long)b->S * b->M;
    if (blocks > 0x7fffffffull || groups > 0x7fffffffull) return hipErrorInvalidValue;
    if (blocks) {
        hipLaunchKernelGGL(crt::shape_set_leaf_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, *b, blocksPerShape);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crt::shape_set_box_kernel, dim3((uint32_t)groups), dim3(crt::kShapeBoxThreads), 0, stream, *b, viewShape, K);
    return hipGetLastError();
}
