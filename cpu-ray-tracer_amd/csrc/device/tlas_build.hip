// tlas_build.hip — BLASBVH::SetTransform for every instance (infra/blas_bvh.cpp:363-374) and the TLASBVH::Build that follows (infra/tlas_bvh.cpp:17-70) on the
// device, from transforms that live in device memory (crt_update_transforms_device).  ONE launch of ONE 64-lane wavefront writes a result block (TlasBuildHeader +
// an image of the geometry buffer's TLAS node, TLAS child pair and Instance sections); the host reads it back, checks it and copies the image into the geometry
// buffer.  The kernel never writes the geometry buffer itself.  crt_render_poses runs the same build for P sets of transforms at once, one workgroup (of that one
// wavefront) per set, into the P result blocks of a pose table (tlas_build_poses_kernel): such a block is a complete, relocatable pose of the scene's instances.
// crt_render_shapes runs it per SHAPE of a refitted BLAS, each build over its own row of node-0 boxes (tlas_build_shapes_kernel).
//
//   phase 1  one lane per BLAS (four rounds for 256): invT = T.FastInvertedTransformNoScale(), the world box grown over the eight corners of the BLAS's node-0
//            box (the context's device array of root boxes) through TransformPosition, the TLAS leaf node, and the Instance record with its T / invT rows renewed.
//   phase 2  the agglomerative clustering, with the open list (256 node indices) and the node boxes (512 x 6 floats) in LDS.  Each FindBestMatch is an argmin over
//            the open list: four entries per lane, then a cross-lane butterfly on (area, list index).  The A / B / C chain around it is the reference's, taken by
//            every lane alike; the merge itself is written by lanes 0..5.
//   phase 3  one lane per node: both reference forms, the child pairs side by side, the header.
//
// Why one wavefront and not a 256-thread workgroup: the build is a chain of about 3.6 N searches, each a few dozen instructions long, and every search needs the
// result of the one before.  With four wavefronts each search would cross two workgroup barriers and a second reduction stage through LDS; with one, the
// reduction is six cross-lane steps, LDS traffic is in program order, and __syncthreads() in a workgroup of one wavefront is no s_barrier at all (the compiler
// lowers it to the LDS wait alone).  Occupancy is of no use to a dependent chain: the other three wavefronts would only add latency to each link.
//
// Bit for bit the host's arithmetic: comparisons are `a < b ? a : b` / `a > b ? a : b` in the reference's operand order (tmplmath.h:122-123), sums are associated
// as written there, -ffp-contract=off as everywhere.  FindBestMatch takes the first B in list order whose area is strictly below the running minimum (1e30f at the
// start): as a reduction, the lowest list index among the candidates of smallest area, candidates being those with area < 1e30f (a NaN area never is).  After a
// merge the reference shortens the list BEFORE the next search: when A was the last entry it then lies outside the list, list[A] (the new node) is still read and
// no entry is excluded by `B != A`, so the new node can be paired with its own copy — kept.
#include "launch.h"

namespace crt {

typedef float row4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTlasLanes = 64u;
constexpr int kNoSlot = 0x7fffffff;

__device__ __forceinline__ float tlas_lesser(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float tlas_greater(float a, float b) { return a > b ? a : b; }

struct TlasLds {
    float box[6][2 * kTlasMaxBlas];       // per node: aabbMin xyz, aabbMax xyz (one array per component: consecutive nodes fall into consecutive banks)
    uint32_t leftRight[2 * kTlasMaxBlas]; // TLASBVHNode::leftRight (0 = leaf)
    uint32_t height[2 * kTlasMaxBlas];    // deepest leaf below the node, in edges
    uint32_t list[kTlasMaxBlas];          // the open list: node indices
};

// FindBestMatch(list, n, A): the list index of A's best partner, or -1.  A may be n (see above); it is always below kTlasMaxBlas.
__device__ __forceinline__ int tlas_partner(const TlasLds& s, int A, int n, uint32_t lane)
{
    const uint32_t ia = s.list[A];
    float alo[3], ahi[3];
    for (int k = 0; k < 3; k++) { alo[k] = s.box[k][ia]; ahi[k] = s.box[3 + k][ia]; }
    float best = 1e30f; int slot = kNoSlot;
    for (uint32_t r = 0; r < kTlasMaxBlas / kTlasLanes; r++) {
        const int B = (int)(lane + r * kTlasLanes);
        if (B >= n || B == A) continue;
        const uint32_t ib = s.list[B];
        float e[3];
        for (int k = 0; k < 3; k++) e[k] = tlas_greater(ahi[k], s.box[3 + k][ib]) - tlas_lesser(alo[k], s.box[k][ib]);
        const float area = e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
        if (area < best) { best = area; slot = B; }
    }
    for (int m = 1; m < (int)kTlasLanes; m <<= 1) {
        const float ob = __shfl_xor(best, m); const int os = __shfl_xor(slot, m);
        if (ob < best || (ob == best && os < slot)) { best = ob; slot = os; }
    }
    return slot == kNoSlot ? -1 : slot;
}

// what the geometry buffer holds for TLAS node i (TlasNode / NodeChild layout): box + both forms of the node's reference.  Interior nodes number their child
// pairs in node-index order, node 0 first (flatten_tlas): the interior nodes are node 0 and nodes n + 1 .. 2n - 1, so node i > 0 owns pair i - n.
__device__ __forceinline__ void tlas_record(const TlasLds& s, uint32_t i, uint32_t n, const PoolRefForm R, row4* lo, row4* hi)
{
    const uint32_t lr = s.leftRight[i], blas = i ? i - 1u : 0u;
    const uint32_t ref = lr ? (kRefTlasInterior | (lr & 0x7fffu) | (((lr >> 16) & 0x7fffu) << 15)) : (kRefTlasLeaf | (blas & 0xffffu));
    const uint32_t ref16 = lr ? (R.tlasBit | (i ? i - n : 0u)) : (R.tlasLeaf | (blas & R.indexMask));   // the pool form, in the scene's width
    *lo = row4{s.box[0][i], s.box[1][i], s.box[2][i], __uint_as_float(ref)};
    *hi = row4{s.box[3][i], s.box[4][i], s.box[5][i], __uint_as_float(ref16)};
}

// The three phases, for the one wavefront of a workgroup: the build over the n transforms at T into `head` and `image` (node section at 0, child pairs at pairRel,
// Instance records at instRel: the geometry buffer's offsets minus tlasOff).  One definition for the two kernels below.
__device__ __forceinline__ void tlas_build_pose(TlasLds& s, const char* __restrict__ geom, uint32_t instOff, const float* __restrict__ T, const float* __restrict__ rootBox, uint32_t n,
                                                uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits, TlasBuildHeader* __restrict__ head, char* __restrict__ image)
{
    const uint32_t lane = threadIdx.x;
    if (n == 0u || n > kTlasMaxBlas) return;

    // ---- phase 1: SetTransform per BLAS, leaf nodes, Instance records ----
    for (uint32_t i = lane; i < n; i += kTlasLanes) {
        float m[12];
        for (int k = 0; k < 12; k++) m[k] = T[16u * i + k];
        float r[12];                                                             // FastInvertedTransformNoScale, tmplmath.h:745-768
        r[0] = m[0]; r[1] = m[4]; r[2] = m[8];
        r[4] = m[1]; r[5] = m[5]; r[6] = m[9];
        r[8] = m[2]; r[9] = m[6]; r[10] = m[10];
        r[3] = -(m[3] * r[0] + m[7] * r[1] + m[11] * r[2]);
        r[7] = -(m[3] * r[4] + m[7] * r[5] + m[11] * r[6]);
        r[11] = -(m[3] * r[8] + m[7] * r[9] + m[11] * r[10]);
        float lo[3], hi[3], wlo[3] = {1e34f, 1e34f, 1e34f}, whi[3] = {-1e34f, -1e34f, -1e34f};
        for (int k = 0; k < 3; k++) { lo[k] = rootBox[6u * i + k]; hi[k] = rootBox[6u * i + 3 + k]; }
        for (int c = 0; c < 8; c++) {
            const float x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
            const float p[3] = {m[0] * x + m[1] * y + m[2] * z + m[3] * 1.0f, m[4] * x + m[5] * y + m[6] * z + m[7] * 1.0f, m[8] * x + m[9] * y + m[10] * z + m[11] * 1.0f};
            for (int k = 0; k < 3; k++) { wlo[k] = tlas_lesser(wlo[k], p[k]); whi[k] = tlas_greater(whi[k], p[k]); }
        }
        for (int k = 0; k < 3; k++) { s.box[k][1u + i] = wlo[k]; s.box[3 + k][1u + i] = whi[k]; }
        s.leftRight[1u + i] = 0u; s.height[1u + i] = 0u; s.list[i] = 1u + i;
        const row4* src = reinterpret_cast<const row4*>(geom + instOff + (size_t)i * 128u);
        row4* dst = reinterpret_cast<row4*>(image + instRel + (size_t)i * 128u);
        const row4 ids = src[3], tail = src[7];                                  // shadeBase, rootRef16, rootRef, objIdx / triCount, pad: as uploaded
        for (int k = 0; k < 3; k++) { dst[k] = row4{r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]}; dst[4 + k] = row4{m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]}; }
        dst[3] = ids; dst[7] = tail;
    }
    __syncthreads();

    // ---- phase 2: TLASBVH::Build ----
    uint32_t used = 1u + n, searches = 0u, staleA = 0u, status = kTlasBuildOk, step = 0u;
    const uint32_t bound = 16u * n + 16u;                                        // about 3.6 n searches happen; a chain that has not ended by then never will
    int open = (int)n, A = 0;
    int B = tlas_partner(s, A, open, lane); searches++;
    while (open > 1) {
        if (B < 0) { status = kTlasBuildNoCandidate; step = searches; break; }
        const int C = tlas_partner(s, B, open, lane); searches++;
        if (C < 0) { status = kTlasBuildNoCandidate; step = searches; break; }   // the reference goes on with B = -1 and reads list[-1]
        if (searches > bound) { status = kTlasBuildNoEnd; step = searches; break; }
        if (A != C) { A = B; B = C; continue; }
        __syncthreads();
        const uint32_t ia = s.list[A], ib = s.list[B], last = s.list[open - 1];
        __syncthreads();
        if (lane < 3u) s.box[lane][used] = tlas_lesser(s.box[lane][ia], s.box[lane][ib]);
        else if (lane < 6u) s.box[lane][used] = tlas_greater(s.box[lane][ia], s.box[lane][ib]);
        else if (lane == 6u) {
            const uint32_t ha = s.height[ia], hb = s.height[ib];
            s.leftRight[used] = ia + (ib << 16); s.height[used] = (ha > hb ? ha : hb) + 1u;
            s.list[A] = used; s.list[B] = (A == open - 1) ? used : last;          // list[A] = new; list[B] = list[N-1], in that order
        }
        if (A == open - 1) staleA++;
        used++; open--;
        __syncthreads();
        B = tlas_partner(s, A, open, lane); searches++;
    }
    if (lane == 0u) {
        TlasBuildHeader* h = head;
        h->status = status; h->step = step; h->height = (status == kTlasBuildOk) ? s.height[s.list[A]] : 0u; h->searches = searches; h->staleA = staleA;
    }
    if (status != kTlasBuildOk) return;

    // ---- phase 3: node 0 = the last open node; records, child pairs ----
    const uint32_t root = s.list[A];
    __syncthreads();
    if (lane < 6u) s.box[lane][0] = s.box[lane][root];
    else if (lane == 6u) { s.leftRight[0] = s.leftRight[root]; s.height[0] = s.height[root]; }
    __syncthreads();
    row4* nodes = reinterpret_cast<row4*>(image);
    row4* pairs = reinterpret_cast<row4*>(image + pairRel);
    const PoolRefForm R = pool_ref_form(poolRefBits);
    for (uint32_t i = lane; i < 2u * n; i += kTlasLanes) {
        row4 lo, hi; tlas_record(s, i, n, R, &lo, &hi);
        nodes[2u * i] = lo; nodes[2u * i + 1u] = hi;
        const uint32_t lr = s.leftRight[i];
        if (!lr) continue;
        row4* p = pairs + 4u * (i ? i - n : 0u);
        tlas_record(s, lr & 0xffffu, n, R, &p[0], &p[1]);
        tlas_record(s, lr >> 16, n, R, &p[2], &p[3]);
    }
    if (n == 1u && lane < 4u) pairs[lane] = row4{0.0f, 0.0f, 0.0f, 0.0f};        // the one pair slot of a single-instance scene stays empty
}

// crt_update_transforms_device.  out: TlasBuildHeader, then the image
__global__ __launch_bounds__(kTlasLanes) void tlas_build_kernel(const char* __restrict__ geom, uint32_t instOff, const float* __restrict__ T, const float* __restrict__ rootBox,
                                                                uint32_t n, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits, char* __restrict__ out)
{
    __shared__ TlasLds s;
    tlas_build_pose(s, geom, instOff, T, rootBox, n, pairRel, instRel, poolRefBits, reinterpret_cast<TlasBuildHeader*>(out), out + sizeof(TlasBuildHeader));
}

// crt_render_poses: P builds in one launch, workgroup p the build over T + 16 n p into header p and image p of a pose table (layout.h PoseJobHeader).  The chains are
// independent, so they run side by side on P compute units in the time of one.  The same launch looks at the job's view -> pose indices (viewPose, K of them, or
// nullptr: the identity): workgroup p takes every P-th group of 64, and an index outside [0, P) lowers PoseJobHeader::badView to its view (atomicMin on the word the
// host set to kPoseNoBadView: the lowest such view remains).
__global__ __launch_bounds__(kTlasLanes) void tlas_build_poses_kernel(const char* __restrict__ geom, uint32_t instOff, const float* __restrict__ T, const float* __restrict__ rootBox,
                                                                      uint32_t n, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits, char* __restrict__ table, uint32_t imagesOff,
                                                                      uint32_t imageStride, uint32_t P, const int32_t* __restrict__ viewPose, uint32_t K)
{
    __shared__ TlasLds s;
    const uint32_t p = blockIdx.x;
    if (viewPose)
        for (unsigned long long k = (unsigned long long)p * kTlasLanes + threadIdx.x; k < K; k += (unsigned long long)P * kTlasLanes)
            if ((uint32_t)viewPose[k] >= P) atomicMin(&reinterpret_cast<PoseJobHeader*>(table)->badView, (uint32_t)k);
    tlas_build_pose(s, geom, instOff, T + (size_t)p * 16u * n, rootBox, n, pairRel, instRel, poolRefBits, reinterpret_cast<TlasBuildHeader*>(table + sizeof(PoseJobHeader)) + p,
                    table + imagesOff + (size_t)p * imageStride);
}

// crt_render_shapes: S builds in one launch, workgroup s the build over T + 16 n s with ITS OWN row of node-0 boxes (shape_build.hip writes the rows: the live boxes
// with the refitted BVH's replaced) into header s and the pose image inside image s of a shape table (layout.h ShapeJobHeader).  The view -> shape indices are the
// box launch's to check.
__global__ __launch_bounds__(kTlasLanes) void tlas_build_shapes_kernel(const char* __restrict__ geom, uint32_t instOff, const float* __restrict__ T, const float* __restrict__ rootBoxRows,
                                                                       uint32_t n, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits, char* __restrict__ table, uint32_t headsOff,
                                                                       uint32_t posesOff, uint32_t imageStride)
{
    __shared__ TlasLds s;
    const uint32_t p = blockIdx.x;
    tlas_build_pose(s, geom, instOff, T + (size_t)p * 16u * n, rootBoxRows + (size_t)p * 6u * n, n, pairRel, instRel, poolRefBits, reinterpret_cast<TlasBuildHeader*>(table + headsOff) + p,
                    table + posesOff + (size_t)p * imageStride);
}

} // namespace crt

extern "C" hipError_t crt_launch_tlas_build(const char* geom, uint32_t instOff, const float* T, const float* rootBox, uint32_t blasCount, uint32_t pairRel, uint32_t instRel, uint32_t poolRefBits,
                                            void* out, hipStream_t stream)
{
    if (blasCount == 0u || blasCount > crt::kTlasMaxBlas) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::tlas_build_kernel, dim3(1), dim3(crt::kTlasLanes), 0, stream, geom, instOff, T, rootBox, blasCount, pairRel, instRel, poolRefBits, static_cast<char*>(out));
    return hipGetLastError();
}

// P builds into a pose table (layout.h PoseJobHeader): one workgroup each.  The caller has set PoseJobHeader::badView to kPoseNoBadView on the stream.
extern "C" hipError_t crt_launch_tlas_build_poses(const char* geom, uint32_t instOff, const float* T, const float* rootBox, uint32_t blasCount, uint32_t pairRel, uint32_t instRel,
                                                  uint32_t poolRefBits, void* table, uint32_t imagesOff, uint32_t imageStride, uint32_t P, const int32_t* viewPose, uint32_t K, hipStream_t stream)
{
    if (blasCount == 0u || blasCount > crt::kTlasMaxBlas || P == 0u || (imagesOff & 63u) || (imageStride & 127u)) return hipErrorInvalidValue;
    if ((unsigned long long)imagesOff + (unsigned long long)P * imageStride > crt::kMaxGeomBytes) return hipErrorInvalidValue;     // the render kernel's 32-bit offsets into the table
    hipLaunchKernelGGL(crt::tlas_build_poses_kernel, dim3(P), dim3(crt::kTlasLanes), 0, stream, geom, instOff, T, rootBox, blasCount, pairRel, instRel, poolRefBits, static_cast<char*>(table),
                       imagesOff, imageStride, P, viewPose, K);
    return hipGetLastError();
}

// S builds into the pose images of a shape table (layout.h ShapeJobHeader), each from its own row of 6 blasCount node-0 boxes: one workgroup each.  posesOff: the
// first image's pose image (imagesOff + poseRel).
extern "C" hipError_t crt_launch_tlas_build_shapes(const char* geom, uint32_t instOff, const float* T, const float* rootBoxRows, uint32_t blasCount, uint32_t pairRel, uint32_t instRel,
                                                   uint32_t poolRefBits, void* table, uint32_t headsOff, uint32_t posesOff, uint32_t imageStride, uint32_t S, hipStream_t stream)
{
    if (blasCount == 0u || blasCount > crt::kTlasMaxBlas || S == 0u || (headsOff & 63u) || (posesOff & 127u) || (imageStride & 127u)) return hipErrorInvalidValue;
    if ((unsigned long long)posesOff + (unsigned long long)S * imageStride > crt::kMaxGeomBytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::tlas_build_shapes_kernel, dim3(S), dim3(crt::kTlasLanes), 0, stream, geom, instOff, T, rootBoxRows, blasCount, pairRel, instRel, poolRefBits, static_cast<char*>(table),
                       headsOff, posesOff, imageStride);
    return hipGetLastError();
}
