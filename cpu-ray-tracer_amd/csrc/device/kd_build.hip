// kd_build.hip — KDTree::Build / BLASKDTree::Build (infra/kdtree.cpp:4-108) on the device, from vertex positions that live in device memory (crt_build_kdtree_device).
// The reference recurses; here the tree grows level by level (at most 21 levels: depth 0 .. 20), and a finalise pass puts the nodes into the recursion's pre-order.
// The build is not SAH: the split is the spatial median of the longest axis and a triangle goes left, right or both by two comparisons on its box, so every step
// is a map, a stable partition or a prefix sum over integers, and the result is the host build's byte for byte.
//
//   (grid_bounds_kernel)     the root box and the non-finite flag: the grid build's 64-bit key reduction (crt_launch_grid_bounds), signed zeros as the reference's fold
//   kd_root_kernel           level 0: the root node from the bound keys (aabb::Grow from +-1e34)
//   kd_tri_box_kernel        one lane per triangle: its box (only the VALUES are compared later, so signed zeros do not matter), and level 0's references 0 .. n - 1
//   per level d:
//   kd_node_kernel           one lane per node: leaf (d >= 20 or <= 2 references) or split — axis (both comparisons strict), distance, splitPos in float32;
//                            writes the node's scan item: 1 for a split node | its reference count << 32 for a leaf
//   kd_classify_kernel       one lane per reference: left (bmax < splitPos), else right ((double)bmin > (double)splitPos - 0.001, kdtree.cpp:71), else both;
//                            its scan item: goes left | goes right << 32
//   scan_*_kernel<64-bit>    exclusive prefix of either item array in place, both halves at once (build_common.h: multi-block); the total goes behind the items
//                            and to the state block, which the host reads to size the next level
//   kd_split_kernel          one lane per node: the two children (the parent's box with one component replaced by splitPos) at 2 * (split nodes before it) in the next
//                            level; one lane per reference: its place(s) in the next level's array — [left list][right list] per split node in level order, each list
//                            in the parent's order — are sums of prefix values, so no atomic's arrival order reaches the output
//   finalise:
//   kd_sizes_kernel          bottom-up, a launch per level: nodes and leaf references of every subtree
//   kd_emit_kernel           top-down, a launch per level: pre-order index (left = self + 1, right = left + size(left)) and firstTri (leaf references before the node in
//                            pre-order, what the host's emit writes) handed to the children; the KdNode record goes to its pre-order place, a leaf's references to
//                            [firstTri, firstTri + count) in the order the level kept
//   (grid_tris_kernel)       the AltTri records (crt_launch_alt_tris)
//
// The height is the index of the last level: the host knows it without a reduction.  No floating-point atomics, no atomics at all; -ffp-contract=off as everywhere.
#include "launch.h"
#include "build_common.h"

namespace crt {

typedef float row4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kKdThreads = kBuildThreads;

__device__ __forceinline__ float kd_pick(float x, float y, float z, int axis) { return axis == 0 ? x : (axis == 1 ? y : z); }

__global__ __launch_bounds__(64) void kd_root_kernel(const KdBuildState* __restrict__ st, uint32_t triCount, KdBuildNode* root)
{
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    KdBuildNode n{};
    for (int k = 0; k < 3; k++) {
        const float lo = bound_of_key(st->bounds.key[k]), up = bound_of_key(st->bounds.key[3 + k]);
        n.lo[k] = 1e34f < lo ? 1e34f : lo; n.hi[k] = -1e34f > up ? -1e34f : up;    // aabb::Grow from +-1e34 (the host's fold of the same bounds)
    }
    n.first = 0u; n.count = triCount; n.axis = -1;
    *root = n;
}

__global__ __launch_bounds__(kKdThreads) void kd_tri_box_kernel(const float* __restrict__ pos, uint32_t triCount, float* __restrict__ triBox, uint32_t* __restrict__ refs,
                                                                uint32_t* __restrict__ owner)
{
    for (uint32_t t = blockIdx.x * kKdThreads + threadIdx.x; t < triCount; t += gridDim.x * kKdThreads) {
        const float* v = pos + (size_t)t * 9u;
        float* b = triBox + (size_t)t * 6u;
        for (int k = 0; k < 3; k++) {
            b[k] = lesser(lesser(lesser(1e34f, v[k]), v[3 + k]), v[6 + k]);
            b[3 + k] = greater(greater(greater(-1e34f, v[k]), v[3 + k]), v[6 + k]);
        }
        refs[t] = t; owner[t] = 0u;
    }
}

// Subdivide's head (kdtree.cpp:47-59) for every node of the level
__global__ __launch_bounds__(kKdThreads) void kd_node_kernel(KdBuildNode* nodes, uint32_t nodeCount, uint32_t depth, unsigned long long* __restrict__ item)
{
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < nodeCount; i += gridDim.x * kKdThreads) {
        row4* rec = reinterpret_cast<row4*>(nodes + i);
        const row4 a = rec[0], b = rec[1];
        const uint32_t count = __float_as_uint(b.w);
        if (depth >= kKdMaxDepth || count <= 2u) {
            row4 s; s.x = 0.0f; s.y = 0.0f; s.z = __int_as_float(-1); s.w = __uint_as_float(0u);
            row4 z; z.x = __uint_as_float(1u); z.y = __uint_as_float(count); z.z = 0.0f; z.w = 0.0f;       // a leaf's subtree: itself, its references
            rec[2] = s; rec[3] = z;
            item[i] = (unsigned long long)count << 32;
            continue;
        }
        const float ex = b.x - a.x, ey = b.y - a.y, ez = b.z - a.z;
        int axis = 0;
        if (ey > ex) axis = 1;
        if (ez > kd_pick(ex, ey, ez, axis)) axis = 2;
        const float distance = kd_pick(ex, ey, ez, axis) * 0.5f;
        const float splitPos = kd_pick(a.x, a.y, a.z, axis) + distance;
        row4 s; s.x = splitPos; s.y = distance; s.z = __int_as_float(axis); s.w = __uint_as_float(0u);
        rec[2] = s;
        item[i] = 1ull;
    }
}

// Subdivide's loop body (kdtree.cpp:64-80) for every reference of the level
__global__ __launch_bounds__(kKdThreads) void kd_classify_kernel(const KdBuildNode* __restrict__ nodes, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ refs,
                                                                 const float* __restrict__ triBox, uint32_t refCount, unsigned long long* __restrict__ item)
{
    for (uint32_t j = blockIdx.x * kKdThreads + threadIdx.x; j < refCount; j += gridDim.x * kKdThreads) {
        const row4 s = reinterpret_cast<const row4*>(nodes + owner[j])[2];
        const int axis = __float_as_int(s.z);
        unsigned long long v = 0ull;
        if (axis >= 0) {
            const float* b = triBox + (size_t)refs[j] * 6u;
            const float bmin = b[axis], bmax = b[3 + axis], splitPos = s.x;
            if (bmax < splitPos) v = 1ull;
            else if ((double)bmin > (double)splitPos - 0.001) v = 1ull << 32;
            else v = 1ull | (1ull << 32);
        }
        item[j] = v;
    }
}

// Subdivide's tail (kdtree.cpp:82-100) from the two prefixes: nodeScan[i] & 0xffffffff = split nodes before node i; refScan[j] = references before j that go
// left | right << 32.  Lanes below nodeCount make the children, lanes below refCount place their reference.
__global__ __launch_bounds__(kKdThreads) void kd_split_kernel(KdBuildNode* nodes, uint32_t nodeCount, const unsigned long long* __restrict__ nodeScan,
                                                              const uint32_t* __restrict__ owner, const uint32_t* __restrict__ refs, uint32_t refCount,
                                                              const unsigned long long* __restrict__ refScan, KdBuildNode* next, uint32_t nextNodes, uint32_t* __restrict__ nextRefs,
                                                              uint32_t* __restrict__ nextOwner, uint32_t nextRefCount)
{
    const uint32_t items = nodeCount > refCount ? nodeCount : refCount;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < items; i += gridDim.x * kKdThreads) {
        if (i < nodeCount) {
            row4* rec = reinterpret_cast<row4*>(nodes + i);
            const row4 a = rec[0], b = rec[1]; row4 s = rec[2];
            const int axis = __float_as_int(s.z);
            const uint32_t child = 2u * (uint32_t)nodeScan[i];
            const uint32_t f = __float_as_uint(a.w), e = f + __float_as_uint(b.w);
            if (axis >= 0 && child + 1u < nextNodes && e <= refCount && e >= f) {
                const unsigned long long sf = refScan[f], se = refScan[e];
                const uint32_t leftCount = (uint32_t)se - (uint32_t)sf, rightCount = (uint32_t)(se >> 32) - (uint32_t)(sf >> 32);
                const uint32_t base = (uint32_t)sf + (uint32_t)(sf >> 32);
                row4 la = a, lb = b, ra = a, rb = b;
                if (axis == 0) { lb.x = s.x; ra.x = s.x; } else if (axis == 1) { lb.y = s.x; ra.y = s.x; } else { lb.z = s.x; ra.z = s.x; }
                la.w = __uint_as_float(base); lb.w = __uint_as_float(leftCount);
                ra.w = __uint_as_float(base + leftCount); rb.w = __uint_as_float(rightCount);
                row4* l = reinterpret_cast<row4*>(next + child); row4* r = reinterpret_cast<row4*>(next + child + 1u);
                l[0] = la; l[1] = lb; r[0] = ra; r[1] = rb;
                s.w = __uint_as_float(child); rec[2] = s;
            }
        }
        if (i < refCount) {
            const uint32_t o = owner[i];
            const KdBuildNode* nd = nodes + o;
            const row4 a = reinterpret_cast<const row4*>(nd)[0], b = reinterpret_cast<const row4*>(nd)[1];
            const unsigned long long here = refScan[i], after = refScan[i + 1u];
            const bool goesLeft = (uint32_t)after != (uint32_t)here, goesRight = (uint32_t)(after >> 32) != (uint32_t)(here >> 32);
            if (goesLeft || goesRight) {                                              // (a leaf's references have no items)
                const uint32_t f = __float_as_uint(a.w), e = f + __float_as_uint(b.w);
                if (e > refCount || e < f) continue;
                const uint32_t child = 2u * (uint32_t)nodeScan[o], t = refs[i];
                if (goesLeft) { const uint32_t p = (uint32_t)(refScan[f] >> 32) + (uint32_t)here; if (p < nextRefCount) { nextRefs[p] = t; nextOwner[p] = child; } }
                if (goesRight) { const uint32_t p = (uint32_t)refScan[e] + (uint32_t)(here >> 32); if (p < nextRefCount) { nextRefs[p] = t; nextOwner[p] = child + 1u; } }
            }
        }
    }
}

// bottom-up: the subtree sizes of a level's split nodes from their children's (leaves were given theirs by kd_node_kernel)
__global__ __launch_bounds__(kKdThreads) void kd_sizes_kernel(KdBuildNode* nodes, uint32_t nodeCount, const KdBuildNode* __restrict__ next, uint32_t nextNodes)
{
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < nodeCount; i += gridDim.x * kKdThreads) {
        row4* rec = reinterpret_cast<row4*>(nodes + i);
        const row4 s = rec[2];
        const uint32_t child = __float_as_uint(s.w);
        if (__float_as_int(s.z) < 0 || child + 1u >= nextNodes) continue;
        const row4 l = reinterpret_cast<const row4*>(next + child)[3], r = reinterpret_cast<const row4*>(next + child + 1u)[3];
        row4 z = rec[3];
        z.x = __uint_as_float(1u + __float_as_uint(l.x) + __float_as_uint(r.x)); z.y = __uint_as_float(__float_as_uint(l.y) + __float_as_uint(r.y));
        rec[3] = z;
    }
}

// top-down: every node of the level to its pre-order place, its children told theirs; every reference of a leaf to the leaf's range
__global__ __launch_bounds__(kKdThreads) void kd_emit_kernel(const KdBuildNode* __restrict__ nodes, uint32_t nodeCount, KdBuildNode* next, uint32_t nextNodes,
                                                             const uint32_t* __restrict__ owner, const uint32_t* __restrict__ refs, uint32_t refCount, KdNode* outNodes,
                                                             uint32_t outNodeCount, uint32_t* __restrict__ outRefs, uint32_t outRefCount)
{
    const uint32_t items = nodeCount > refCount ? nodeCount : refCount;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < items; i += gridDim.x * kKdThreads) {
        if (i < nodeCount) {
            const row4* rec = reinterpret_cast<const row4*>(nodes + i);
            const row4 a = rec[0], b = rec[1], s = rec[2], z = rec[3];
            const int axis = __float_as_int(s.z);
            const uint32_t child = __float_as_uint(s.w), pre = __float_as_uint(z.z), firstRef = __float_as_uint(z.w);
            row4 o0 = a, o1 = b, o2;
            if (axis >= 0 && child + 1u < nextNodes) {
                row4* l = reinterpret_cast<row4*>(next + child); row4* r = reinterpret_cast<row4*>(next + child + 1u);
                row4 lz = l[3], rz = r[3];
                const uint32_t left = pre + 1u, right = left + __float_as_uint(lz.x);
                lz.z = __uint_as_float(left); lz.w = __uint_as_float(firstRef);
                rz.z = __uint_as_float(right); rz.w = __uint_as_float(firstRef + __float_as_uint(lz.y));
                l[3] = lz; r[3] = rz;
                o0.w = __int_as_float((int)left); o1.w = __int_as_float((int)right);
                o2.x = s.y; o2.y = __int_as_float(axis); o2.z = __uint_as_float(firstRef); o2.w = __uint_as_float(0u);
            } else {
                o0.w = __int_as_float(-1); o1.w = __int_as_float(-1);
                o2.x = 0.0f; o2.y = __int_as_float(0); o2.z = __uint_as_float(firstRef); o2.w = b.w;
            }
            if (pre < outNodeCount) { row4* o = reinterpret_cast<row4*>(outNodes + pre); o[0] = o0; o[1] = o1; o[2] = o2; }
        }
        if (i < refCount) {
            const row4* rec = reinterpret_cast<const row4*>(nodes + owner[i]);
            if (__float_as_int(rec[2].z) < 0) {
                const uint32_t p = __float_as_uint(rec[3].w) + (i - __float_as_uint(rec[0].w));
                if (p < outRefCount) outRefs[p] = refs[i];
            }
        }
    }
}

} // namespace crt

// chunk sums the scan of n items needs (64-bit words)
extern "C" size_t crt_kd_scan_chunks(uint32_t n) { return crt::scan_chunks(n ? n : 1u); }

// bounds (state->bounds), the triangle boxes (6 floats each), level 0: the root node and the references 0 .. triCount - 1
extern "C" hipError_t crt_launch_kd_begin(const float* pos, uint32_t triCount, crt::KdBuildState* state, float* triBox, crt::KdBuildNode* root, uint32_t* refs, uint32_t* owner,
                                          uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e = crt_launch_grid_bounds(pos, triCount, &state->bounds, maxBlocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::kd_root_kernel, dim3(1), dim3(64), 0, stream, state, triCount, root);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::kd_tri_box_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), dim3(crt::kKdThreads), 0, stream, pos, triCount, triBox, refs, owner);
    return hipGetLastError();
}

// One level's decisions: which nodes split and where every reference goes.  nodeItems: nodeCount + 1 words, refItems: refCount + 1 words, both come back as the
// exclusive prefixes kd_split reads, each with its total behind it; chunkSums: crt_kd_scan_chunks(max(nodeCount, refCount)) words.  state->nodeTotal / refTotal receive the totals.
extern "C" hipError_t crt_launch_kd_level(crt::KdBuildNode* nodes, uint32_t nodeCount, uint32_t depth, const uint32_t* owner, const uint32_t* refs, uint32_t refCount, const float* triBox,
                                          unsigned long long* nodeItems, unsigned long long* refItems, unsigned long long* chunkSums, crt::KdBuildState* state, uint32_t maxBlocks,
                                          hipStream_t stream)
{
    hipError_t e;
    hipLaunchKernelGGL(crt::kd_node_kernel, dim3(crt::blocks_for(nodeCount, maxBlocks)), dim3(crt::kKdThreads), 0, stream, nodes, nodeCount, depth, nodeItems);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = crt::scan(nodeItems, nodeCount, (uint32_t)crt_kd_scan_chunks(nodeCount), chunkSums, nodeItems + nodeCount, &state->nodeTotal, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::kd_classify_kernel, dim3(crt::blocks_for(refCount, maxBlocks)), dim3(crt::kKdThreads), 0, stream, nodes, owner, refs, triBox, refCount, refItems);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return crt::scan(refItems, refCount, (uint32_t)crt_kd_scan_chunks(refCount), chunkSums, refItems + refCount, &state->refTotal, stream);
}

// the next level's nodes and references from this level's prefixes
extern "C" hipError_t crt_launch_kd_split(crt::KdBuildNode* nodes, uint32_t nodeCount, const unsigned long long* nodeScan, const uint32_t* owner, const uint32_t* refs, uint32_t refCount,
                                          const unsigned long long* refScan, crt::KdBuildNode* next, uint32_t nextNodes, uint32_t* nextRefs, uint32_t* nextOwner, uint32_t nextRefCount,
                                          uint32_t maxBlocks, hipStream_t stream)
{
    const uint32_t items = nodeCount > refCount ? nodeCount : refCount;
    hipLaunchKernelGGL(crt::kd_split_kernel, dim3(crt::blocks_for(items, maxBlocks)), dim3(crt::kKdThreads), 0, stream, nodes, nodeCount, nodeScan, owner, refs, refCount, refScan, next,
                       nextNodes, nextRefs, nextOwner, nextRefCount);
    return hipGetLastError();
}

// levels: the levels' node arrays, reference arrays, owners and sizes (level 0 first); the finished tree goes to outNodes (pre-order) / outRefs
extern "C" hipError_t crt_launch_kd_finalise(crt::KdBuildNode* const* nodes, const uint32_t* const* refs, const uint32_t* const* owner, const uint32_t* nodeCount, const uint32_t* refCount,
                                             uint32_t levels, crt::KdNode* outNodes, uint32_t outNodeCount, uint32_t* outRefs, uint32_t outRefCount, uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e;
    for (uint32_t d = levels - 1u; d-- > 0u;) {
        hipLaunchKernelGGL(crt::kd_sizes_kernel, dim3(crt::blocks_for(nodeCount[d], maxBlocks)), dim3(crt::kKdThreads), 0, stream, nodes[d], nodeCount[d], nodes[d + 1u], nodeCount[d + 1u]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (uint32_t d = 0; d < levels; d++) {
        const bool last = d + 1u == levels;
        const uint32_t items = nodeCount[d] > refCount[d] ? nodeCount[d] : refCount[d];
        hipLaunchKernelGGL(crt::kd_emit_kernel, dim3(crt::blocks_for(items, maxBlocks)), dim3(crt::kKdThreads), 0, stream, nodes[d], nodeCount[d], last ? nullptr : nodes[d + 1u],
                           last ? 0u : nodeCount[d + 1u], owner[d], refs[d], refCount[d], outNodes, outNodeCount, outRefs, outRefCount);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
