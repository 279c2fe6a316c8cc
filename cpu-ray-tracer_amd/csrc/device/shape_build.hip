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
// No refit ever writes node 1, so the S shapes are independent of each other and of their order.  Neither kernel writes the geometry buffer.
// The comparison forms and node_box are refit_common.h's: one definition for this file and refit.hip.  -ffp-contract=off as everywhere.
#include "launch.h"
#include "refit_common.h"

namespace crt {

constexpr uint32_t kShapeBoxThreads = 1024u;

__global__ __launch_bounds__(256) void shape_leaf_kernel(const ShapeBuildDev b, uint32_t blocksPerShape)
{
    const uint32_t s = blockIdx.x / blocksPerShape, j = (blockIdx.x - s * blocksPerShape) * 256u + threadIdx.x;
    if (s >= b.S || j >= b.triCount) return;
    const row4* lt = reinterpret_cast<const row4*>(b.geom + b.leafOff + (size_t)(b.triBase + j) * 48u);
    row4* out = reinterpret_cast<row4*>(b.table + b.imagesOff + (size_t)s * b.imageStride + b.leafRel + (size_t)j * 48u);
    row4 r0 = lt[0], r1 = lt[1], r2 = lt[2];
    const uint32_t tri = __float_as_uint(r0.w) - b.triBase;
    if (tri < b.triCount) {                                                        // (else the record as it is: refit_leaf_kernel leaves such a slot alone)
        const float* v = b.pos + ((size_t)s * b.triCount + tri) * 9u;
        const float v0x = v[0], v0y = v[1], v0z = v[2];
        r0.x = v0x; r0.y = v0y; r0.z = v0z;
        r1.x = v[3] - v0x; r1.y = v[4] - v0y; r1.z = v[5] - v0z;
        r2.x = v[6] - v0x; r2.y = v[7] - v0y; r2.z = v[8] - v0z;
    }
    out[0] = r0; out[1] = r1; out[2] = r2;
}

// a live reference of this BVH as the image's: the record's 16-byte offset from the image's first byte
__device__ __forceinline__ uint32_t image_ref(const ShapeBuildDev& b, uint32_t ref)
{
    if (ref & kRefInterior) return ref - b.pairBase * 4u;
    if (ref == kRefDone) return ref;
    return ref - ((b.leafOff + b.triBase * 48u) >> 4) + (b.leafRel >> 4);
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
    // the live pairs, child by child: box and pool-form word as they are, the reference image-relative
    const row4* live = reinterpret_cast<const row4*>(b.geom + (size_t)b.pairBase * 64u);
    for (uint32_t i = threadIdx.x; i < 2u * b.pairCount; i += kShapeBoxThreads) {
        row4 lo = live[2 * i]; const row4 hi = live[2 * i + 1];
        lo.w = __uint_as_float(image_ref(b, __float_as_uint(lo.w)));
        reinterpret_cast<row4*>(image)[2 * i] = lo; reinterpret_cast<row4*>(image)[2 * i + 1] = hi;
    }
    __syncthreads();
    for (uint32_t lvl = 0; lvl < levels; lvl++) {
        const uint32_t end = levelOff[lvl + 1];
        for (uint32_t i = levelOff[lvl] + threadIdx.x; i < end; i += kShapeBoxThreads) {
            const RefitPlanRec r = plan[i];
            if (r.pair >= b.pairCount) continue;                                    // (a plan never names a pair past the BVH; neither does this loop)
            row4* p = reinterpret_cast<row4*>(image + (size_t)r.pair * 64u);
            for (uint32_t k = 0; k < 2; k++) {
                if (r.pair == 0 && k == 0) continue;                               // node 1 = child 0 of the BVH's first pair: bvh.cpp:28
                if ((r.child[k] & kPlanInterior) && (r.child[k] & ~kPlanInterior) >= b.pairCount) continue;
                const Box x = node_box(image, b.geom, b.leafOff, 0u, b.triBase, b.triCount, pos, r.child[k]);
                row4 lo = p[2 * k], hi = p[2 * k + 1];                              // .w: ref / ref16 stay
                lo.x = x.lo[0]; lo.y = x.lo[1]; lo.z = x.lo[2]; hi.x = x.hi[0]; hi.y = x.hi[1]; hi.z = x.hi[2];
                p[2 * k] = lo; p[2 * k + 1] = hi;
            }
        }
        __syncthreads();                                                           // the next level reads what this one stored (same workgroup, same CU)
    }
    // the shape's row of node-0 boxes: the live ones, this BVH's from the image
    float* row = reinterpret_cast<float*>(b.table + b.rowsOff) + (size_t)s * b.rowFloats;
    if (b.liveRootBox)
        for (uint32_t i = threadIdx.x; i < b.rowFloats; i += kShapeBoxThreads)
            if (i / 6u != b.bvh) row[i] = b.liveRootBox[i];
    if (threadIdx.x == 0) {
        const bool ok = !(rootCode & kPlanInterior) || (rootCode & ~kPlanInterior) < b.pairCount;
        Box x;
        if (ok) x = node_box(image, b.geom, b.leafOff, 0u, b.triBase, b.triCount, pos, rootCode);
        else for (int k = 0; k < 3; k++) { x.lo[k] = 1e30f; x.hi[k] = -1e30f; }
        for (int k = 0; k < 3; k++) { row[6u * b.bvh + k] = x.lo[k]; row[6u * b.bvh + 3 + k] = x.hi[k]; }
    }
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
