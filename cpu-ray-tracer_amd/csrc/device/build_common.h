// build_common.h — what the device builds of the uniform grid (grid_build.hip), the KD-tree (kd_build.hip) and the BVH (bvh_build.hip) share.  The first part is host-includable (abi.cpp
// turns the grid's bound keys back into floats with the function the KD-tree's root kernel uses); the kernels below it exist for the .hip files only, and each
// of them instantiates its own copy for its item type, so no relocatable device code is needed.
#pragma once
#include <cstring>
#include "layout.h"

namespace crt {

// one bound from its key (grid_bounds_kernel): the ordered value back to the float's bits, the sign of a zero from the low bit
CRT_HOST_DEVICE inline float bound_of_key(unsigned long long key)
{
    const uint32_t ord = (uint32_t)(key >> 32);
    uint32_t bits = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
    if (bits == 0u && (key & 1ull)) bits = 0x80000000u;
    float v; memcpy(&v, &bits, 4);
    return v;
}

constexpr uint32_t kBuildThreads = 256u;
constexpr uint32_t kScanItems = 8u, kScanChunk = kBuildThreads * kScanItems;      // items per block of the scan kernels

// chunk sums the scan of n items needs (64-bit words)
inline size_t scan_chunks(size_t n) { return (n + kScanChunk - 1u) / kScanChunk; }

// The partition loop `while (i <= j) if (left(idx[i])) i++; else swap(idx[i], idx[j--]);` over a segment of `count` slots, as a map from a slot to where its
// element ends (tests/test_bvh_device_cpu.py holds these lines to the loop through crt_debug_bvh_partition).  S = leftScan, f = the segment's first slot, nLeft = its left elements.
//   a left element below nLeft stays;  the left element with k lefts behind it in [nLeft, count) takes the place of the k-th right element of [0, nLeft);
//   right element number k of [0, nLeft) goes to count - 1 (k = 0) or just below the (k-1)-th left element from the back;
//   the right element at nLeft goes just below the last paired left element (or to count - 1 when there is no pair);  a right element above nLeft moves down one.
CRT_HOST_DEVICE inline uint32_t bvh_select_left(const uint32_t* S, uint32_t f, uint32_t count, uint32_t rank)      // the slot of left element `rank` (ascending, from 0)
{
    uint32_t lo = f, hi = f + count - 1u;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (S[mid + 1u] - S[f] >= rank + 1u) hi = mid; else lo = mid + 1u; }
    return lo;
}
CRT_HOST_DEVICE inline uint32_t bvh_select_right(const uint32_t* S, uint32_t f, uint32_t count, uint32_t rank)
{
    uint32_t lo = f, hi = f + count - 1u;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((mid + 1u - f) - (S[mid + 1u] - S[f]) >= rank + 1u) hi = mid; else lo = mid + 1u; }
    return lo;
}
CRT_HOST_DEVICE inline uint32_t bvh_partition_dest(const uint32_t* S, uint32_t f, uint32_t count, uint32_t nLeft, uint32_t p)
{
    const uint32_t q = p - f, lb = S[p] - S[f];
    if (S[p + 1u] != S[p]) return q < nLeft ? p : bvh_select_right(S, f, count, nLeft - 1u - lb);
    if (q > nLeft) return p - 1u;
    if (q < nLeft) { const uint32_t k = q - lb; return k == 0u ? f + count - 1u : bvh_select_left(S, f, count, nLeft - k) - 1u; }
    const uint32_t pairs = nLeft - (S[f + nLeft] - S[f]);
    return pairs == 0u ? f + count - 1u : bvh_select_left(S, f, count, nLeft - pairs) - 1u;
}

} // namespace crt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace crt {

__device__ __forceinline__ float lesser(float a, float b) { return a < b ? a : b; }     // tmplmath.h:122 / _mm_min_ps operand order
__device__ __forceinline__ float greater(float a, float b) { return a > b ? a : b; }

// static_cast<int>(float) as the host builds' x86 code performs it (cvttss2si): the "integer indefinite" value for NaN and for every value outside int's range
__device__ __forceinline__ int x86_int(float q) { return (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : (int)0x80000000; }

// The keys of one finite component at position `at` (< 2^31) of a fold `acc = lesser(acc, v)` / `acc = greater(acc, v)`, which keeps the LATER operand on a tie: the
// value as an ordered integer with -0 and +0 on one key, the position (complemented for the minimum, so that the last tying component wins both), the sign the
// winner had in the low bit.  Integer min of *kmin and max of *kmax are then the fold in any order; bound_of_key turns either back into the float.
__device__ __forceinline__ void bound_keys(float v, uint32_t at, unsigned long long* kmin, unsigned long long* kmax)
{
    uint32_t b = __float_as_uint(v);
    const uint32_t sign = b >> 31;
    if ((b << 1) == 0u) b = 0u;
    const unsigned long long ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    *kmin = (ord << 32) | ((unsigned long long)(0x7fffffffu - at) << 1) | sign; *kmax = (ord << 32) | ((unsigned long long)at << 1) | sign;
}

static uint32_t blocks_for(uint32_t items, uint32_t maxBlocks)
{
    const uint32_t need = (items + kBuildThreads - 1u) / kBuildThreads;
    return need < maxBlocks ? (need ? need : 1u) : maxBlocks;
}

// ---- the exclusive prefix over n items of type T in place, multi-block: sums per chunk, one block over the chunk sums, apply.  T = uint32_t: the grid's cell
// counters.  T = unsigned long long: the KD-tree's items, two 32-bit sums side by side (neither half can carry: see KdBuildState).  The chunk sums and the pass
// over them are 64-bit for both; the pass inside a chunk runs in T ----
template <class T>
__global__ __launch_bounds__(kBuildThreads) void scan_sums_kernel(const T* __restrict__ item, uint32_t n, unsigned long long* chunkSums)
{
    __shared__ unsigned long long s[kBuildThreads];
    const uint32_t first = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < kScanItems; i++) if (first + i < n) sum += item[first + i];
    s[threadIdx.x] = sum; __syncthreads();
    for (uint32_t off = kBuildThreads / 2u; off > 0u; off >>= 1) { if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off]; __syncthreads(); }
    if (threadIdx.x == 0u) chunkSums[blockIdx.x] = s[0];
}

// one block: chunkSums becomes its own exclusive prefix; the total goes to *total and, where the caller keeps it behind the items, to *itemEnd (or nullptr)
template <class T>
__global__ __launch_bounds__(kBuildThreads) void scan_chunks_kernel(unsigned long long* chunkSums, uint32_t chunks, T* itemEnd, unsigned long long* total)
{
    __shared__ unsigned long long s[2][kBuildThreads];
    const uint32_t per = (chunks + kBuildThreads - 1u) / kBuildThreads, first = threadIdx.x * per;
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < per; i++) if (first + i < chunks) sum += chunkSums[first + i];
    int in = 0; s[0][threadIdx.x] = sum; __syncthreads();
    for (uint32_t off = 1u; off < kBuildThreads; off <<= 1) {
        s[1 - in][threadIdx.x] = s[in][threadIdx.x] + (threadIdx.x >= off ? s[in][threadIdx.x - off] : 0ull);
        __syncthreads(); in = 1 - in;
    }
    unsigned long long run = s[in][threadIdx.x] - sum;                                // exclusive
    for (uint32_t i = 0; i < per; i++) if (first + i < chunks) { const unsigned long long c = chunkSums[first + i]; chunkSums[first + i] = run; run += c; }
    if (threadIdx.x == kBuildThreads - 1u) { if (itemEnd) *itemEnd = (T)s[in][threadIdx.x]; *total = s[in][threadIdx.x]; }
}

template <class T>
__global__ __launch_bounds__(kBuildThreads) void scan_apply_kernel(T* item, uint32_t n, const unsigned long long* __restrict__ chunkSums)
{
    __shared__ T s[2][kBuildThreads];
    const uint32_t first = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    T v[kScanItems]; T sum = 0;
    for (uint32_t i = 0; i < kScanItems; i++) { v[i] = first + i < n ? item[first + i] : (T)0; sum += v[i]; }
    int in = 0; s[0][threadIdx.x] = sum; __syncthreads();
    for (uint32_t off = 1u; off < kBuildThreads; off <<= 1) {
        s[1 - in][threadIdx.x] = s[in][threadIdx.x] + (threadIdx.x >= off ? s[in][threadIdx.x - off] : (T)0);
        __syncthreads(); in = 1 - in;
    }
    T run = (T)chunkSums[blockIdx.x] + (s[in][threadIdx.x] - sum);
    for (uint32_t i = 0; i < kScanItems; i++) if (first + i < n) { item[first + i] = run; run += v[i]; }
}

// chunkSums: `chunks` words of scratch, chunks = scan_chunks(n) or 1 for no items (the one-block pass then writes a total of 0)
template <class T>
static hipError_t scan(T* item, uint32_t n, uint32_t chunks, unsigned long long* chunkSums, T* itemEnd, unsigned long long* total, hipStream_t stream)
{
    hipError_t e;
    hipLaunchKernelGGL(scan_sums_kernel<T>, dim3(chunks), dim3(kBuildThreads), 0, stream, item, n, chunkSums);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(scan_chunks_kernel<T>, dim3(1), dim3(kBuildThreads), 0, stream, chunkSums, chunks, itemEnd, total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3(chunks), dim3(kBuildThreads), 0, stream, item, n, chunkSums);
    return hipGetLastError();
}

} // namespace crt
#endif
