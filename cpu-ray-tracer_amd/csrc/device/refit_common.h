// refit_common.h — what BVH::Refit's box pass is made of (infra/bvh.cpp:26-61), for the two files that run it: refit.hip (in place, on the live geometry buffer) and
// shape_build.hip (into the job-local images of crt_render_shapes).  One definition of the comparison forms and of a node's box.
#pragma once
#include "layout.h"

namespace crt {

typedef float row4 __attribute__((ext_vector_type(4)));

// tmplmath.h:122-123 in the reference's operand order; fminf / fmaxf and the min / max instructions differ on NaN and on +-0
__device__ __forceinline__ float lesser(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float greater(float a, float b) { return a > b ? a : b; }

struct Box { float lo[3], hi[3]; };

// the box of the node a child code names: UpdateNodeBounds for a leaf, the union of the two children for an interior node (whose pair an earlier level wrote).
// The node pairs are read at pairGeom + 64 (pairBase + index), the LeafTri records (remain, shadeIdx: what no refit changes) at leafGeom + leafOff + 48 (triBase + slot):
// refit.hip names the geometry buffer twice, shape_build.hip an image's pairs and the live leaves.
__device__ __forceinline__ Box node_box(const char* pairGeom, const char* leafGeom, uint32_t leafOff, uint32_t pairBase, uint32_t triBase, uint32_t triCount, const float* pos,
                                        uint32_t code)
{
    Box b;
    if (code & kPlanInterior) {
        const row4* p = reinterpret_cast<const row4*>(pairGeom + (size_t)(pairBase + (code & ~kPlanInterior)) * 64u);
        const row4 llo = p[0], lhi = p[1], rlo = p[2], rhi = p[3];
        b.lo[0] = lesser(llo.x, rlo.x); b.lo[1] = lesser(llo.y, rlo.y); b.lo[2] = lesser(llo.z, rlo.z);
        b.hi[0] = greater(lhi.x, rhi.x); b.hi[1] = greater(lhi.y, rhi.y); b.hi[2] = greater(lhi.z, rhi.z);
        return b;
    }
    for (int k = 0; k < 3; k++) { b.lo[k] = 1e30f; b.hi[k] = -1e30f; }
    if (code >= triCount) return b;
    const char* leaf = leafGeom + leafOff + (size_t)(triBase + code) * 48u;
    uint32_t n = reinterpret_cast<const uint32_t*>(leaf)[11];                      // LeafTri::remain of the leaf's first slot
    if (n > triCount - code) n = triCount - code;                                  // (a plan never names a slot past the BVH; neither does this loop)
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t tri = reinterpret_cast<const uint32_t*>(leaf + (size_t)i * 48u)[3] - triBase;   // LeafTri::shadeIdx = triBase + the reference's triangle index
        if (tri >= triCount) continue;
        const float* v = pos + (size_t)tri * 9u;
        for (int c = 0; c < 3; c++) for (int k = 0; k < 3; k++) b.lo[k] = lesser(b.lo[k], v[3 * c + k]);
        for (int c = 0; c < 3; c++) for (int k = 0; k < 3; k++) b.hi[k] = greater(b.hi[k], v[3 * c + k]);
    }
    return b;
}

} // namespace crt
