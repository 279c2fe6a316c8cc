// refit.hip — BVH::Refit / BLASBVH::Refit (infra/bvh.cpp:26-61) on the device, from vertex positions that live in device memory (crt_refit_device).
// Rewrites, in place, the LeafTri vertices and the NodeChild boxes of ONE BVH of the geometry buffer; references, leaf order and shading records stay.
//
//   refit_leaf_kernel  one lane per leaf slot: gathers the 36 bytes of its triangle (slot j holds triangle shadeIdx - triBase) and stores the three 16-byte
//                      rows of the LeafTri again, the fourth dword of each row as it was read.
//   refit_box_kernel   ONE workgroup per BVH walks the node pairs bottom-up, level by level (deepest first), with __syncthreads() between the levels:
//                      producer and consumer of a box are waves of the same CU, so workgroup scope orders them and no cross-workgroup protocol exists.
//                      The order comes from a plan the host builds once per BVH from its mirror of the references (RefitPlanRec, 32-bit indices).
//
// The comparison forms and a node's box (node_box) are refit_common.h's, shared with shape_build.hip (crt_render_shapes: the same refit into job-local images).
// Bit for bit the reference's loop: a leaf's box is UpdateNodeBounds (starts from +-1e30, triangles in leaf order, vertices 0, 1, 2, taken from the caller's
// positions — never from v0 + e1, which rounds), an interior node's box is min / max of its children, both as `a < b ? a : b` / `a > b ? a : b` in the
// reference's operand order (tmplmath.h:122-123; fminf / fmaxf and the min / max instructions differ on NaN and on +-0), and NODE 1 IS SKIPPED
// (bvh.cpp:28 `if (i != 1)`): the root's left child keeps the box it had, and that stale box still feeds node 0's.  -ffp-contract=off as everywhere.
#include "launch.h"
#include "refit_common.h"

namespace crt {

constexpr uint32_t kRefitBoxThreads = 1024u;

__global__ __launch_bounds__(256) void refit_leaf_kernel(char* geom, uint32_t leafOff, uint32_t triBase, uint32_t triCount, const float* __restrict__ pos)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= triCount) return;
    row4* lt = reinterpret_cast<row4*>(geom + leafOff + (size_t)(triBase + j) * 48u);
    row4 r0 = lt[0], r1 = lt[1], r2 = lt[2];
    const uint32_t tri = __float_as_uint(r0.w) - triBase;
    if (tri >= triCount) return;
    const float* v = pos + (size_t)tri * 9u;
    const float v0x = v[0], v0y = v[1], v0z = v[2];
    r0.x = v0x; r0.y = v0y; r0.z = v0z;
    r1.x = v[3] - v0x; r1.y = v[4] - v0y; r1.z = v[5] - v0z;
    r2.x = v[6] - v0x; r2.y = v[7] - v0y; r2.z = v[8] - v0z;
    lt[0] = r0; lt[1] = r1; lt[2] = r2;
}

// out: 16 floats = the root's NodePair as refitted (zeros for a leaf root), then node 0's box (min xyz, max xyz)
__global__ __launch_bounds__(kRefitBoxThreads) void refit_box_kernel(char* geom, uint32_t leafOff, uint32_t pairBase, uint32_t triBase, uint32_t triCount, const float* pos,
                                                                     const RefitPlanRec* plan, const uint32_t* levelOff, uint32_t levels, uint32_t rootCode, float* out)
{
    for (uint32_t lvl = 0; lvl < levels; lvl++) {
        const uint32_t end = levelOff[lvl + 1];
        for (uint32_t i = levelOff[lvl] + threadIdx.x; i < end; i += kRefitBoxThreads) {
            const RefitPlanRec r = plan[i];
            row4* p = reinterpret_cast<row4*>(geom + (size_t)(pairBase + r.pair) * 64u);
            for (uint32_t k = 0; k < 2; k++) {
                if (r.pair == 0 && k == 0) continue;                               // node 1 = child 0 of the BVH's first pair: bvh.cpp:28
                const Box b = node_box(geom, geom, leafOff, pairBase, triBase, triCount, pos, r.child[k]);
                row4 lo = p[2 * k], hi = p[2 * k + 1];                              // .w: ref / ref16 stay
                lo.x = b.lo[0]; lo.y = b.lo[1]; lo.z = b.lo[2]; hi.x = b.hi[0]; hi.y = b.hi[1]; hi.z = b.hi[2];
                p[2 * k] = lo; p[2 * k + 1] = hi;
            }
        }
        __syncthreads();                                                           // the next level reads what this one stored (same workgroup, same CU)
    }
    if (threadIdx.x == 0) {
        const Box b = node_box(geom, geom, leafOff, pairBase, triBase, triCount, pos, rootCode);
        row4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        row4* o = reinterpret_cast<row4*>(out);
        const row4* p = reinterpret_cast<const row4*>(geom + (size_t)(pairBase + (rootCode & ~kPlanInterior)) * 64u);
        const bool pair = (rootCode & kPlanInterior) != 0;
        for (int k = 0; k < 4; k++) o[k] = pair ? p[k] : z;
        for (int k = 0; k < 3; k++) { out[16 + k] = b.lo[k]; out[19 + k] = b.hi[k]; }
    }
}

} // namespace crt

extern "C" hipError_t crt_launch_refit(char* geom, uint32_t leafOff, uint32_t pairBase, uint32_t triBase, uint32_t triCount, const float* pos,
                                       const void* plan, const uint32_t* levelOff, uint32_t levels, uint32_t rootCode, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(crt::refit_leaf_kernel, dim3((triCount + 255u) / 256u), dim3(256), 0, stream, geom, leafOff, triBase, triCount, pos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::refit_box_kernel, dim3(1), dim3(crt::kRefitBoxThreads), 0, stream, geom, leafOff, pairBase, triBase, triCount, pos,
                       (const crt::RefitPlanRec*)plan, levelOff, levels, rootCode, out);
    return hipGetLastError();
}
