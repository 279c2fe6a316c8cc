// bvh_build.hip — BVH::Build / BLASBVH::Build (infra/bvh.cpp:4-24, 63-178; host/accel.cpp BuildSAH) on the device, from vertex positions that live in device memory
// (crt_build_bvh_device).  The reference recurses depth first; here the tree grows level by level over ONE triangleIndices array, and a finalise pass gives the
// nodes the recursion's numbering.  A level is an array of node records (first, count, box) in level order; `owner` names every slot's node of the level
// (kBvhNone: the slot's node became a leaf on an earlier level).  One lane per slot in every per-triangle kernel, so a node of thousands of triangles spreads
// over many workgroups and a level of thousands of small nodes packs 256 slots into each.
//
//   bvh_begin_kernel         centroids ((v0 + v1 + v2) * 0.3333f), the non-finite flag, triangleIndices = 0 .. n - 1, every triangle's objIdx from the live LeafTri
//                            records, the root record
//   per level:
//   bvh_fill_bins_kernel     the level's 3 x 8 bins emptied (count 0, boxes +-1e34)
//   bvh_bounds_kernel        Builder::fit of every node of the level: 64-bit keys (value, position, sign of a zero — build_common.h) folded with integer min / max,
//                            position = 3 * slot + vertex COMPLEMENTED: Builder::fit keeps the earlier operand, so the first of -0 and +0 in slot order wins; and the centroid bounds per
//                            axis of the nodes with more than 2 triangles (ordered 32-bit keys: only their values are used)
//   bvh_bin_kernel           every triangle of those nodes into its bin on each axis: `kBins / (cmax - cmin)`, x86's float -> int, count and box (ordered keys)
//   bvh_plane_kernel         one lane per node: the boxes back from their keys, the 21 planes in the host's order and expressions, the leaf test
//   bvh_classify_kernel      one lane per slot: centroid[axis] < pos, then scan_*_kernel<uint32_t> over the slots (build_common.h)
//   bvh_decide_kernel        one lane per node: leftCount from the prefix; the node splits iff 0 < leftCount < count; scan over the nodes; the host reads the number
//                            of split nodes (THE LEVEL'S ONE HOST WAIT) and sizes the next level
//   bvh_children_kernel      the two children of every split node at 2 * (split nodes before it)
//   bvh_scatter_kernel       the reference's in-place partition loop in closed form (below), applied to EVERY node that chose a plane — a node whose leftCount is 0
//                            or count stays a leaf with its slots permuted, as on the host; next level's owners; `remain` of the slots of finished leaves
//   finalise:
//   bvh_sizes_kernel         bottom-up, a launch per level: split nodes per subtree
//   bvh_emit_kernel          top-down, a launch per level: a split node's child pair is number (split nodes before it in depth-first pre-order) — children 2k + 1 and
//                            2k + 2 — and is written as NodePair k with both reference forms
//   bvh_leaf_kernel          the LeafTri records in triangleIndices order
//   commit (abi.cpp):
//   bvh_relocate_kernel      the other BVHs' pairs into the new geometry buffer, references re-based; bvh_instances_kernel: the instances' root references
//
// In both LDS paths a workgroup whose 256 slots belong to one node accumulates in LDS and merges once; other workgroups go to global memory directly (small nodes:
// few lanes per address).  Integer atomics on ordered keys only, no kernel waits for another workgroup; -ffp-contract=off as everywhere.
#include "launch.h"
#include "build_common.h"

namespace crt {

constexpr uint32_t kBvhThreads = kBuildThreads;

__device__ __forceinline__ uint32_t ord32(float v) { const uint32_t b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float val32(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// a fresh node: Builder::fit's +-1e30 as keys that lose every tie, the centroid bounds' +-1e30 (choosePlane)
__device__ __forceinline__ void bvh_init_node(BvhBuildNode* nd, unsigned long long* key, uint32_t first, uint32_t count)
{
    BvhBuildNode n{};
    n.first = first; n.count = count; n.axis = -1; n.child = kBvhNone;
    for (int k = 0; k < 3; k++) { n.ckey[k] = ord32(1e30f); n.ckey[3 + k] = ord32(-1e30f); }
    *nd = n;
    for (int k = 0; k < 3; k++) { key[k] = ((unsigned long long)ord32(1e30f) << 32) | 0xfffffffeull; key[3 + k] = (unsigned long long)ord32(-1e30f) << 32; }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_begin_kernel(const float* __restrict__ pos, uint32_t n, const char* __restrict__ geom, uint32_t leafOff, uint32_t triBase,
                                                                float* __restrict__ cen, uint32_t* __restrict__ idx, uint32_t* __restrict__ owner, int32_t* __restrict__ objOf,
                                                                BvhBuildNode* root, unsigned long long* rootKeys, BvhBuildState* st)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) bvh_init_node(root, rootKeys, 0u, n);
    bool bad = false;
    for (uint32_t t = blockIdx.x * kBvhThreads + threadIdx.x; t < n; t += gridDim.x * kBvhThreads) {
        const float* v = pos + (size_t)t * 9u;
        for (int k = 0; k < 9; k++) bad = bad || (__float_as_uint(v[k]) & 0x7f800000u) == 0x7f800000u;
        for (int k = 0; k < 3; k++) cen[(size_t)t * 3u + k] = (v[k] + v[3 + k] + v[6 + k]) * 0.3333f;
        idx[t] = t; owner[t] = 0u;
        const uint32_t* lt = reinterpret_cast<const uint32_t*>(geom + leafOff + (size_t)(triBase + t) * 48u);    // slot t of the live tree: (shadeIdx, objIdx)
        const uint32_t tri = lt[3] - triBase;
        if (tri < n) objOf[tri] = (int32_t)lt[7];
    }
    if (bad) atomicOr(&st->nonFinite, 1u);
}

__global__ __launch_bounds__(kBvhThreads) void bvh_fill_bins_kernel(uint32_t* __restrict__ bins, size_t words)
{
    for (size_t w = (size_t)blockIdx.x * kBvhThreads + threadIdx.x; w < words; w += (size_t)gridDim.x * kBvhThreads) {
        const uint32_t f = (uint32_t)(w % kBvhBinWords);
        bins[w] = f == 0u ? 0u : (f < 4u ? ord32(1e34f) : ord32(-1e34f));
    }
}

// owners are whole segments in ascending order: a chunk of slots whose first and last owner agree belongs to that one node
__device__ __forceinline__ bool bvh_chunk_uniform(const uint32_t* __restrict__ owner, uint32_t base, uint32_t n, uint32_t* o)
{
    const uint32_t last = base + kBvhThreads - 1u < n ? base + kBvhThreads - 1u : n - 1u;
    *o = owner[base];
    return *o != kBvhNone && *o == owner[last];
}

__global__ __launch_bounds__(kBvhThreads) void bvh_bounds_kernel(const float* __restrict__ pos, const float* __restrict__ cen, const uint32_t* __restrict__ idx,
                                                                 const uint32_t* __restrict__ owner, uint32_t n, BvhBuildNode* nodes, uint32_t m, unsigned long long* keys)
{
    __shared__ unsigned long long sk[6];
    __shared__ uint32_t sc[6];
    for (uint32_t base = blockIdx.x * kBvhThreads; base < n; base += gridDim.x * kBvhThreads) {
        uint32_t oF; const bool uniform = bvh_chunk_uniform(owner, base, n, &oF) && oF < m;
        if (uniform) {
            if (threadIdx.x < 6u) { sk[threadIdx.x] = threadIdx.x < 3u ? ~0ull : 0ull; sc[threadIdx.x] = threadIdx.x < 3u ? 0xffffffffu : 0u; }
            __syncthreads();
        }
        const uint32_t p = base + threadIdx.x;
        const uint32_t o = p < n ? owner[p] : kBvhNone;
        if (o < m && idx[p] < n) {
            const uint32_t t = idx[p];
            const float* v = pos + (size_t)t * 9u;
            const bool wantC = nodes[o].count > 2u;
            unsigned long long* gk = keys + (size_t)o * 6u;
            uint32_t* gc = nodes[o].ckey;
            for (int k = 0; k < 3; k++) {
                unsigned long long mn = ~0ull, mx = 0ull;
                for (uint32_t j = 0; j < 3u; j++) {
                    unsigned long long a, b; bound_keys(v[3u * j + k], 0x7fffffffu - (p * 3u + j), &a, &b);      // (complemented: the FIRST tying vertex wins, as Builder::fit)
                    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
                }
                const uint32_t c = ord32(cen[(size_t)t * 3u + k]);
                if (uniform) {
                    atomicMin(&sk[k], mn); atomicMax(&sk[3 + k], mx);
                    if (wantC) { atomicMin(&sc[k], c); atomicMax(&sc[3 + k], c); }
                } else {
                    atomicMin(&gk[k], mn); atomicMax(&gk[3 + k], mx);
                    if (wantC) { atomicMin(&gc[k], c); atomicMax(&gc[3 + k], c); }
                }
            }
        }
        if (uniform) {
            __syncthreads();
            if (threadIdx.x < 3u) { atomicMin(&keys[(size_t)oF * 6u + threadIdx.x], sk[threadIdx.x]); atomicMin(&nodes[oF].ckey[threadIdx.x], sc[threadIdx.x]); }
            else if (threadIdx.x < 6u) { atomicMax(&keys[(size_t)oF * 6u + threadIdx.x], sk[threadIdx.x]); atomicMax(&nodes[oF].ckey[threadIdx.x], sc[threadIdx.x]); }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_bin_kernel(const float* __restrict__ pos, const float* __restrict__ cen, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ owner, uint32_t n, const BvhBuildNode* __restrict__ nodes, uint32_t m, uint32_t* bins)
{
    __shared__ uint32_t sb[kBvhNodeBinWords];
    for (uint32_t base = blockIdx.x * kBvhThreads; base < n; base += gridDim.x * kBvhThreads) {
        uint32_t oF; const bool uniform = bvh_chunk_uniform(owner, base, n, &oF) && oF < m;
        if (uniform) {
            if (threadIdx.x < kBvhNodeBinWords) { const uint32_t f = threadIdx.x % kBvhBinWords; sb[threadIdx.x] = f == 0u ? 0u : (f < 4u ? ord32(1e34f) : ord32(-1e34f)); }
            __syncthreads();
        }
        const uint32_t p = base + threadIdx.x;
        const uint32_t o = p < n ? owner[p] : kBvhNone;
        if (o < m && nodes[o].count > 2u && idx[p] < n) {
            const BvhBuildNode& nd = nodes[o];
            const uint32_t t = idx[p];
            const float* v = pos + (size_t)t * 9u;
            uint32_t blo[3], bhi[3];
            for (int k = 0; k < 3; k++) {                                            // aabb::Grow's values (the keys' fold takes care of the +-1e34 start)
                blo[k] = ord32(lesser(lesser(v[k], v[3 + k]), v[6 + k])); bhi[k] = ord32(greater(greater(v[k], v[3 + k]), v[6 + k]));
            }
            for (int a = 0; a < 3; a++) {
                const float cmin = val32(nd.ckey[a]), cmax = val32(nd.ckey[3 + a]);
                if (cmin == cmax) continue;
                const float scale = 8.0f / (cmax - cmin);
                int b = x86_int((cen[(size_t)t * 3u + a] - cmin) * scale);
                if (b > 7) b = 7;
                if (b < 0) b = 0;                                                     // (the host indexes out of bounds here: a NaN or overflowed scale)
                const uint32_t w = ((uint32_t)a * kBvhBins + (uint32_t)b) * kBvhBinWords;
                if (uniform) {
                    atomicAdd(&sb[w], 1u);
                    for (int k = 0; k < 3; k++) { atomicMin(&sb[w + 1 + k], blo[k]); atomicMax(&sb[w + 4 + k], bhi[k]); }
                } else {
                    uint32_t* B = bins + (size_t)o * kBvhNodeBinWords + w;
                    atomicAdd(B, 1u);
                    for (int k = 0; k < 3; k++) { atomicMin(B + 1 + k, blo[k]); atomicMax(B + 4 + k, bhi[k]); }
                }
            }
        }
        if (uniform) {
            __syncthreads();
            if (threadIdx.x < kBvhNodeBinWords) {
                const uint32_t f = threadIdx.x % kBvhBinWords; uint32_t* g = bins + (size_t)oF * kBvhNodeBinWords + threadIdx.x;
                if (f == 0u) { if (sb[threadIdx.x]) atomicAdd(g, sb[threadIdx.x]); } else if (f < 4u) atomicMin(g, sb[threadIdx.x]); else atomicMax(g, sb[threadIdx.x]);
            }
            __syncthreads();
        }
    }
}

struct BvhBox { float lo[3], hi[3]; };
__device__ __forceinline__ void bvh_grow(BvhBox& a, const float* lo, const float* hi) { for (int k = 0; k < 3; k++) { a.lo[k] = lesser(a.lo[k], lo[k]); a.hi[k] = greater(a.hi[k], hi[k]); } }
__device__ __forceinline__ float bvh_area(const BvhBox& b)                            // aabb::Area
{
    const float e0 = b.hi[0] - b.lo[0], e1 = b.hi[1] - b.lo[1], e2 = b.hi[2] - b.lo[2];
    const float a = e0 * e1 + e0 * e2 + e1 * e2;
    return (0.0f < a) ? a : 0.0f;
}

// Builder::choosePlane and the leaf test of Builder::run for every node of the level
__global__ __launch_bounds__(kBvhThreads) void bvh_plane_kernel(BvhBuildNode* nodes, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ bins, uint32_t m,
                                                                BvhBuildState* st, int isRoot)
{
    for (uint32_t i = blockIdx.x * kBvhThreads + threadIdx.x; i < m; i += gridDim.x * kBvhThreads) {
        BvhBuildNode& nd = nodes[i];
        float lo[3], hi[3];
        for (int k = 0; k < 3; k++) { lo[k] = bound_of_key(keys[(size_t)i * 6u + k]); hi[k] = bound_of_key(keys[(size_t)i * 6u + 3 + k]); nd.lo[k] = lo[k]; nd.hi[k] = hi[k]; }
        if (isRoot && i == 0u) for (int k = 0; k < 3; k++) { st->rootBox[k] = lo[k]; st->rootBox[3 + k] = hi[k]; }
        const uint32_t count = nd.count;
        if (count <= 2u) continue;
        float best = 1e30f, pos = 0.0f; int axis = 0;
        for (int a = 0; a < 3; a++) {
            const float cmin = val32(nd.ckey[a]), cmax = val32(nd.ckey[3 + a]);
            if (cmin == cmax) continue;
            const uint32_t* B = bins + (size_t)i * kBvhNodeBinWords + (uint32_t)a * kBvhBins * kBvhBinWords;
            float areaL[7], areaR[7]; int nL[7], nR[7];
            BvhBox accL, accR; for (int k = 0; k < 3; k++) { accL.lo[k] = accR.lo[k] = 1e34f; accL.hi[k] = accR.hi[k] = -1e34f; }
            int sumL = 0, sumR = 0;
            for (int b = 0; b < 7; b++) {
                const uint32_t* l = B + b * kBvhBinWords; const uint32_t* r = B + (7 - b) * kBvhBinWords;
                float blo[3], bhi[3];
                for (int k = 0; k < 3; k++) { blo[k] = val32(l[1 + k]); bhi[k] = val32(l[4 + k]); }
                sumL += (int)l[0]; nL[b] = sumL; bvh_grow(accL, blo, bhi); areaL[b] = bvh_area(accL);
                for (int k = 0; k < 3; k++) { blo[k] = val32(r[1 + k]); bhi[k] = val32(r[4 + k]); }
                sumR += (int)r[0]; nR[6 - b] = sumR; bvh_grow(accR, blo, bhi); areaR[6 - b] = bvh_area(accR);
            }
            const float scale = (cmax - cmin) / 8.0f;
            for (int b = 0; b < 7; b++) {
                const float cost = (float)nL[b] * areaL[b] + (float)nR[b] * areaR[b];
                if (cost < best) { axis = a; pos = cmin + scale * (float)(b + 1); best = cost; }
            }
        }
        const float e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
        const float leafCost = (float)count * (e0 * e1 + e1 * e2 + e2 * e0);
        if (best >= leafCost) continue;
        nd.axis = axis; nd.pos = pos;
    }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_classify_kernel(const float* __restrict__ cen, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ owner, uint32_t n,
                                                                   const BvhBuildNode* __restrict__ nodes, uint32_t m, uint32_t* __restrict__ item)
{
    for (uint32_t p = blockIdx.x * kBvhThreads + threadIdx.x; p < n; p += gridDim.x * kBvhThreads) {
        const uint32_t o = owner[p];
        uint32_t v = 0u;
        if (o < m && nodes[o].axis >= 0 && idx[p] < n) v = cen[(size_t)idx[p] * 3u + (uint32_t)nodes[o].axis] < nodes[o].pos ? 1u : 0u;
        item[p] = v;
    }
}

// leftScan[x] = slots before x whose triangle goes left
__global__ __launch_bounds__(kBvhThreads) void bvh_decide_kernel(BvhBuildNode* nodes, uint32_t m, const uint32_t* __restrict__ leftScan, uint32_t n, uint32_t* __restrict__ item)
{
    for (uint32_t i = blockIdx.x * kBvhThreads + threadIdx.x; i < m; i += gridDim.x * kBvhThreads) {
        BvhBuildNode& nd = nodes[i];
        uint32_t split = 0u;
        const uint32_t f = nd.first, e = f + nd.count;
        if (nd.axis >= 0 && e <= n && e >= f) {
            const uint32_t nLeft = leftScan[e] - leftScan[f];
            nd.nLeft = nLeft;
            split = (nLeft > 0u && nLeft < nd.count) ? 1u : 0u;
        }
        item[i] = split;
    }
}

__device__ __forceinline__ bool bvh_splits(const BvhBuildNode& nd) { return nd.axis >= 0 && nd.nLeft > 0u && nd.nLeft < nd.count; }

__global__ __launch_bounds__(kBvhThreads) void bvh_children_kernel(BvhBuildNode* nodes, uint32_t m, const uint32_t* __restrict__ splitScan, BvhBuildNode* next, unsigned long long* nextKeys,
                                                                   uint32_t nextM)
{
    for (uint32_t i = blockIdx.x * kBvhThreads + threadIdx.x; i < m; i += gridDim.x * kBvhThreads) {
        BvhBuildNode& nd = nodes[i];
        if (!bvh_splits(nd)) continue;
        const uint32_t child = 2u * splitScan[i];
        if (child + 1u >= nextM) continue;
        nd.child = child;
        bvh_init_node(next + child, nextKeys + (size_t)child * 6u, nd.first, nd.nLeft);
        bvh_init_node(next + child + 1u, nextKeys + (size_t)(child + 1u) * 6u, nd.first + nd.nLeft, nd.count - nd.nLeft);
    }
}

// (the partition loop in closed form: bvh_partition_dest, build_common.h — host-includable, so that the test of the form runs the kernel's own lines)
__global__ __launch_bounds__(kBvhThreads) void bvh_scatter_kernel(const BvhBuildNode* __restrict__ nodes, uint32_t m, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ idx,
                                                                  const uint32_t* __restrict__ leftScan, uint32_t n, uint32_t* __restrict__ idxOut, uint32_t* __restrict__ ownerOut,
                                                                  uint32_t* __restrict__ remain)
{
    for (uint32_t p = blockIdx.x * kBvhThreads + threadIdx.x; p < n; p += gridDim.x * kBvhThreads) {
        const uint32_t o = owner[p];
        if (o >= m) { idxOut[p] = idx[p]; ownerOut[p] = kBvhNone; continue; }
        const BvhBuildNode& nd = nodes[o];
        const uint32_t f = nd.first, count = nd.count;
        uint32_t dest = p;
        if (nd.axis >= 0 && f + count <= n && p >= f && p - f < count) dest = bvh_partition_dest(leftScan, f, count, nd.nLeft, p);
        if (dest >= n || dest < f || dest - f >= count) continue;
        idxOut[dest] = idx[p];
        if (nd.child != kBvhNone) ownerOut[dest] = nd.child + (dest - f >= nd.nLeft ? 1u : 0u);
        else { ownerOut[dest] = kBvhNone; remain[dest] = count - (dest - f); }
    }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_sizes_kernel(BvhBuildNode* nodes, uint32_t m, const BvhBuildNode* __restrict__ next, uint32_t nextM)
{
    for (uint32_t i = blockIdx.x * kBvhThreads + threadIdx.x; i < m; i += gridDim.x * kBvhThreads) {
        const uint32_t child = nodes[i].child;
        if (child == kBvhNone || child + 1u >= nextM) continue;
        nodes[i].subSplits = 1u + next[child].subSplits + next[child + 1u].subSplits;
    }
}

__device__ __forceinline__ void bvh_child_record(const BvhBuildNode& c, const BvhFlatten& F, NodeChild* out)
{
    NodeChild r;
    for (int k = 0; k < 3; k++) { r.lo[k] = c.lo[k]; r.hi[k] = c.hi[k]; }
    if (c.child != kBvhNone) {
        r.ref = kRefInterior | (uint32_t)((((unsigned long long)F.pairBase + c.pair) * 64ull) >> 4);
        r.ref16 = F.interior16 | ((F.pairBase + c.pair) & F.mask16);
    } else {
        r.ref = (uint32_t)(((unsigned long long)F.leafOff + ((unsigned long long)F.triBase + c.first) * 48ull) >> 4);
        r.ref16 = (F.triBase + c.first + 1u) & F.mask16;
    }
    *out = r;
}

__global__ __launch_bounds__(kBvhThreads) void bvh_emit_kernel(const BvhBuildNode* __restrict__ nodes, uint32_t m, BvhBuildNode* next, uint32_t nextM, BvhFlatten F, char* geom)
{
    for (uint32_t i = blockIdx.x * kBvhThreads + threadIdx.x; i < m; i += gridDim.x * kBvhThreads) {
        const BvhBuildNode& nd = nodes[i];
        const uint32_t child = nd.child, k = nd.pair;
        if (child == kBvhNone || child + 1u >= nextM || k >= F.pairs) continue;
        BvhBuildNode& l = next[child]; BvhBuildNode& r = next[child + 1u];
        l.pair = k + 1u; r.pair = k + 1u + l.subSplits;
        NodePair* out = reinterpret_cast<NodePair*>(geom) + F.pairBase + k;
        bvh_child_record(l, F, &out->c[0]); bvh_child_record(r, F, &out->c[1]);
    }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_leaf_kernel(const float* __restrict__ pos, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ remain,
                                                               const int32_t* __restrict__ objOf, uint32_t n, BvhFlatten F, char* geom)
{
    for (uint32_t j = blockIdx.x * kBvhThreads + threadIdx.x; j < n; j += gridDim.x * kBvhThreads) {
        const uint32_t t = idx[j];
        if (t >= n) continue;
        const float* v = pos + (size_t)t * 9u;
        LeafTri lt;
        for (int k = 0; k < 3; k++) { lt.v0[k] = v[k]; lt.e1[k] = v[3 + k] - v[k]; lt.e2[k] = v[6 + k] - v[k]; }
        lt.shadeIdx = F.triBase + t; lt.objIdx = objOf[t]; lt.remain = remain[j];
        *reinterpret_cast<LeafTri*>(geom + F.leafOff + (size_t)(F.triBase + j) * 48u) = lt;
    }
}

// a reference of another BVH's pairs or of its Instance, carried into the new buffer: `later` = the BVH lies behind the rebuilt one (its pairs moved by pairDelta)
__device__ __forceinline__ void bvh_rebase(uint32_t* ref, uint32_t* ref16, const BvhRelocate& R, bool later)
{
    if ((*ref & 0xC0000000u) == kRefInterior) {
        if (later) { *ref = kRefInterior | ((*ref + (uint32_t)(R.pairDelta * 4)) & kRefOffsetMask); *ref16 = R.interior16 | ((*ref16 + (uint32_t)R.pairDelta) & R.mask16); }
    } else *ref = (*ref + (uint32_t)R.leafDelta16) & kRefOffsetMask;
}

__global__ __launch_bounds__(kBvhThreads) void bvh_relocate_kernel(const char* __restrict__ oldGeom, char* geom, BvhRelocate R)
{
    for (uint32_t q = blockIdx.x * kBvhThreads + threadIdx.x; q < R.oldPairs; q += gridDim.x * kBvhThreads) {
        if (q >= R.firstPair && q - R.firstPair < R.pairCount) continue;
        const bool later = q >= R.firstPair;
        NodePair p = reinterpret_cast<const NodePair*>(oldGeom)[q];
        for (int k = 0; k < 2; k++) bvh_rebase(&p.c[k].ref, &p.c[k].ref16, R, later);
        reinterpret_cast<NodePair*>(geom)[later ? (uint32_t)((int32_t)q + R.pairDelta) : q] = p;
    }
}

__global__ __launch_bounds__(kBvhThreads) void bvh_instances_kernel(char* geom, uint32_t instOff, uint32_t blasCount, uint32_t bvh, uint32_t rootRef, uint32_t rootRef16, BvhRelocate R)
{
    const uint32_t b = blockIdx.x * kBvhThreads + threadIdx.x;
    if (b >= blasCount) return;
    Instance* in = reinterpret_cast<Instance*>(geom + instOff) + b;
    if (b == bvh) { in->rootRef = rootRef; in->rootRef16 = rootRef16; }
    else bvh_rebase(&in->rootRef, &in->rootRef16, R, b > bvh);
}

} // namespace crt

extern "C" hipError_t crt_launch_bvh_begin(const float* pos, uint32_t triCount, const char* geom, uint32_t leafOff, uint32_t triBase, float* cen, uint32_t* idx, uint32_t* owner, int32_t* objOf,
                                           crt::BvhBuildNode* root, unsigned long long* rootKeys, crt::BvhBuildState* state, uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(state, 0, sizeof(crt::BvhBuildState), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_begin_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), dim3(crt::kBvhThreads), 0, stream, pos, triCount, geom, leafOff, triBase, cen, idx, owner, objOf, root,
                       rootKeys, state);
    return hipGetLastError();
}

// One level's decisions.  nodes / keys: the level's m records and 6 * m box keys; bins: kBvhNodeBinWords * m words; leftItems: triCount + 1 words, nodeItems: m + 1 words, both
// come back as exclusive prefixes with their totals behind them; chunkSums: scan_chunks(max(triCount, m)) words.  state->splits receives the number of nodes that split.
extern "C" hipError_t crt_launch_bvh_level(const float* pos, const float* cen, const uint32_t* idx, const uint32_t* owner, uint32_t triCount, crt::BvhBuildNode* nodes, unsigned long long* keys,
                                           uint32_t m, uint32_t* bins, uint32_t* leftItems, uint32_t* nodeItems, unsigned long long* chunkSums, crt::BvhBuildState* state, int isRoot,
                                           uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e;
    const dim3 T(crt::kBvhThreads), slots(crt::blocks_for(triCount, maxBlocks)), perNode(crt::blocks_for(m, maxBlocks));
    const size_t words = (size_t)m * crt::kBvhNodeBinWords;
    hipLaunchKernelGGL(crt::bvh_fill_bins_kernel, dim3(crt::blocks_for(words > 0xffffff00ull ? 0xffffff00u : (uint32_t)words, maxBlocks)), T, 0, stream, bins, words);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_bounds_kernel, slots, T, 0, stream, pos, cen, idx, owner, triCount, nodes, m, keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_bin_kernel, slots, T, 0, stream, pos, cen, idx, owner, triCount, nodes, m, bins);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_plane_kernel, perNode, T, 0, stream, nodes, keys, bins, m, state, isRoot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_classify_kernel, slots, T, 0, stream, cen, idx, owner, triCount, nodes, m, leftItems);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = crt::scan(leftItems, triCount, (uint32_t)crt::scan_chunks(triCount), chunkSums, leftItems + triCount, &state->lefts, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(crt::bvh_decide_kernel, perNode, T, 0, stream, nodes, m, leftItems, triCount, nodeItems);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return crt::scan(nodeItems, m, (uint32_t)crt::scan_chunks(m), chunkSums, nodeItems + m, &state->splits, stream);
}

// the next level's nodes, triangleIndices and owners from this level's prefixes (nextM = 2 * split nodes; 0: the last level — the partition's side effect alone)
extern "C" hipError_t crt_launch_bvh_split(crt::BvhBuildNode* nodes, uint32_t m, const uint32_t* splitScan, const uint32_t* owner, const uint32_t* idx, const uint32_t* leftScan,
                                           uint32_t triCount, crt::BvhBuildNode* next, unsigned long long* nextKeys, uint32_t nextM, uint32_t* idxOut, uint32_t* ownerOut, uint32_t* remain,
                                           uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e;
    if (nextM) {
        hipLaunchKernelGGL(crt::bvh_children_kernel, dim3(crt::blocks_for(m, maxBlocks)), dim3(crt::kBvhThreads), 0, stream, nodes, m, splitScan, next, nextKeys, nextM);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crt::bvh_scatter_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), dim3(crt::kBvhThreads), 0, stream, nodes, m, owner, idx, leftScan, triCount, idxOut, ownerOut, remain);
    return hipGetLastError();
}

// levelOff: levels + 1 offsets of the levels in `nodes`; the pairs and the leaf triangles go to `geom` (the new geometry buffer) as F places them
extern "C" hipError_t crt_launch_bvh_flatten(crt::BvhBuildNode* nodes, const uint32_t* levelOff, uint32_t levels, const float* pos, const uint32_t* idx, const uint32_t* remain,
                                             const int32_t* objOf, uint32_t triCount, const crt::BvhFlatten* F, char* geom, uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e;
    const dim3 T(crt::kBvhThreads);
    for (uint32_t d = levels - 1u; d-- > 0u;) {
        const uint32_t m = levelOff[d + 1u] - levelOff[d], nm = levelOff[d + 2u] - levelOff[d + 1u];
        hipLaunchKernelGGL(crt::bvh_sizes_kernel, dim3(crt::blocks_for(m, maxBlocks)), T, 0, stream, nodes + levelOff[d], m, nodes + levelOff[d + 1u], nm);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (uint32_t d = 0; d + 1u < levels; d++) {
        const uint32_t m = levelOff[d + 1u] - levelOff[d], nm = levelOff[d + 2u] - levelOff[d + 1u];
        hipLaunchKernelGGL(crt::bvh_emit_kernel, dim3(crt::blocks_for(m, maxBlocks)), T, 0, stream, nodes + levelOff[d], m, nodes + levelOff[d + 1u], nm, *F, geom);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crt::bvh_leaf_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), T, 0, stream, pos, idx, remain, objOf, triCount, *F, geom);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_bvh_relocate(const char* oldGeom, char* geom, const crt::BvhRelocate* R, uint32_t instOff, uint32_t blasCount, uint32_t bvh, uint32_t rootRef, uint32_t rootRef16,
                                              uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e;
    if (R->oldPairs > R->pairCount) {
        hipLaunchKernelGGL(crt::bvh_relocate_kernel, dim3(crt::blocks_for(R->oldPairs, maxBlocks)), dim3(crt::kBvhThreads), 0, stream, oldGeom, geom, *R);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!blasCount) return hipSuccess;
    hipLaunchKernelGGL(crt::bvh_instances_kernel, dim3((blasCount + crt::kBvhThreads - 1u) / crt::kBvhThreads), dim3(crt::kBvhThreads), 0, stream, geom, instOff, blasCount, bvh, rootRef, rootRef16,
                       *R);
    return hipGetLastError();
}
