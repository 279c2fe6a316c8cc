// grid_build.hip — Grid::Build / BLASGrid::Build (infra/grid.cpp:4-50) on the device, from vertex positions that live in device memory (crt_build_grid_device).
// The build is not a recursion: bounds, resolution, a cell range per triangle, then count / prefix / fill.  The resolution lines stay on the host
// (host/grid_resolution.h, shared with the host build); everything that touches the triangles runs here, in three groups of launches with one host read between them:
//
//   grid_bounds_kernel       localBounds over the 3 * triCount vertices, and a flag for a non-finite component.  The reference folds with _mm_min_ps(acc, p) /
//                            _mm_max_ps(acc, p), which return the SECOND operand on a tie: when -0 and +0 tie for an extreme, the last one in (triangle, vertex)
//                            order wins, and the bytes of the bounds are compared.  So the reduction runs on 64-bit keys (value, position, sign of zero) with integer
//                            min / max, which is order-independent: value = the float's bits mapped to an ordered integer with -0 and +0 on one key, position =
//                            the vertex index (complemented for the minimum, so that the LAST tying vertex wins both), the low bit = the sign the winner had.
//   grid_count_kernel        one lane per triangle: its box and clamped cell range exactly as the host build's `range` lambda (true IEEE division; the float -> int
//                            conversion restated as x86's, which gives INT_MIN for NaN and for anything out of range: a NaN quotient — 0 / 0 on a flat axis — ends in
//                            cell 0 after the clamp, as on the host), then one atomicAdd per covered cell.  A triangle that covers more than 64 cells is spread over
//                            its wavefront, so one large triangle does not serialise 2 M atomics on one lane.
//   scan_*_kernel<uint32_t>  exclusive prefix over the cells + 1 counters (build_common.h: multi-block, 64-bit chunk sums): the total goes back to the host, which
//                            sizes cellRefs from it and refuses more than 2^31 - 1 references.
//   grid_fill_kernel         the same ranges again; slots are handed out by atomics, so their order inside a cell is not deterministic ...
//   grid_sort_kernel         ... and every cell's segment is then put in ascending order, which is the host build's push_back order: indices inside a cell are
//                            distinct, so out[#smaller] = e is exact.  One lane per cell of up to 32 references, the wavefront together for a longer one.
//   grid_tris_kernel         the AltTri records (v0, v1 - v0, v2 - v0) from the positions; triIdx / objIdx from the BVH's LeafTri records, which carry both.
//
// Integer atomics only; -ffp-contract=off as everywhere.
#include "launch.h"
#include "build_common.h"

namespace crt {

typedef float row4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kGridThreads = kBuildThreads;
constexpr uint32_t kWaveCells = 64u;                                              // a triangle over more cells than this is spread over the wavefront
constexpr uint32_t kLaneCellRefs = 32u;                                           // a cell with more references than this is sorted by the wavefront

struct CellRange { int mn[3]; uint32_t nx, ny, n; };                              // first cell per axis, cells along x and y, cells in all (>= 1)

// Tri::GetBounds (aabb from +-1e34, Grow(vertex0), Grow(vertex1), Grow(vertex2)) and the `range` lambda of Grid::Build
__device__ __forceinline__ CellRange tri_range(const float* v, const GridParams& g)
{
    CellRange r; uint32_t ext[3];
    for (int k = 0; k < 3; k++) {
        const float blo = lesser(lesser(lesser(1e34f, v[k]), v[3 + k]), v[6 + k]), bhi = greater(greater(greater(-1e34f, v[k]), v[3 + k]), v[6 + k]);
        const int lo = x86_int((blo - g.lo[k]) / g.cell[k]), hi = x86_int((bhi - g.lo[k]) / g.cell[k]);
        const int top = g.res[k] - 1;
        const int mn = lo < 0 ? 0 : (lo > top ? top : lo), mx = hi < 0 ? 0 : (hi > top ? top : hi);
        r.mn[k] = mn; ext[k] = mx >= mn ? (uint32_t)(mx - mn) + 1u : 0u;          // mx < mn: the host's loop over this axis runs zero times
    }
    r.nx = ext[0]; r.ny = ext[1]; r.n = ext[0] * ext[1] * ext[2];
    return r;
}

// f(cell, triangle) for every cell of every lane's range (have: the lane holds a triangle).  EVERY lane of the wavefront must call this.
template <class F>
__device__ __forceinline__ void for_each_cell(bool have, const CellRange& r, uint32_t tri, const GridParams& g, F&& f)
{
    const uint32_t rx = (uint32_t)g.res[0], rxy = rx * (uint32_t)g.res[1];
    const uint32_t n = have ? r.n : 0u;
    const bool wide = n > kWaveCells;
    if (!wide && n) {
        const uint32_t nxy = r.nx * r.ny;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t iz = i / nxy, rem = i - iz * nxy, iy = rem / r.nx, ix = rem - iy * r.nx;
            f((uint32_t)r.mn[0] + ix + ((uint32_t)r.mn[1] + iy) * rx + ((uint32_t)r.mn[2] + iz) * rxy, tri);
        }
    }
    unsigned long long m = __builtin_amdgcn_ballot_w64(wide);
    const uint32_t lane = threadIdx.x & 63u;
    while (m) {
        const int src = __builtin_ctzll(m); m &= m - 1;
        const uint32_t m0 = (uint32_t)__shfl(r.mn[0], src), m1 = (uint32_t)__shfl(r.mn[1], src), m2 = (uint32_t)__shfl(r.mn[2], src);
        const uint32_t nx = __shfl(r.nx, src), ny = __shfl(r.ny, src), nn = __shfl(r.n, src), t = __shfl(tri, src);
        const uint32_t nxy = nx * ny;
        for (uint32_t i = lane; i < nn; i += 64u) {
            const uint32_t iz = i / nxy, rem = i - iz * nxy, iy = rem / nx, ix = rem - iy * nx;
            f(m0 + ix + (m1 + iy) * rx + (m2 + iz) * rxy, t);
        }
    }
}

__global__ __launch_bounds__(kGridThreads) void grid_bounds_kernel(const float* __restrict__ pos, uint32_t nVerts, GridBuildState* st)
{
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    bool bad = false;
    for (uint32_t v = blockIdx.x * kGridThreads + threadIdx.x; v < nVerts; v += gridDim.x * kGridThreads) {
        const float* p = pos + (size_t)v * 3u;
        for (int k = 0; k < 3; k++) {
            if ((__float_as_uint(p[k]) & 0x7f800000u) == 0x7f800000u) { bad = true; continue; }
            unsigned long long kmin, kmax; bound_keys(p[k], v, &kmin, &kmax);
            mn[k] = kmin < mn[k] ? kmin : mn[k]; mx[k] = kmax > mx[k] ? kmax : mx[k];
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 3; k++) {
            const unsigned long long a = __shfl_xor(mn[k], off), b = __shfl_xor(mx[k], off);
            mn[k] = a < mn[k] ? a : mn[k]; mx[k] = b > mx[k] ? b : mx[k];
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 3; k++) { atomicMin(&st->key[k], mn[k]); atomicMax(&st->key[3 + k], mx[k]); }
    if (bad) atomicOr(&st->nonFinite, 1u);
}

__global__ __launch_bounds__(kGridThreads) void grid_count_kernel(const float* __restrict__ pos, uint32_t triCount, GridParams g, uint32_t* counts)
{
    for (uint32_t base = blockIdx.x * kGridThreads; base < triCount; base += gridDim.x * kGridThreads) {
        const uint32_t t = base + threadIdx.x; const bool have = t < triCount;
        CellRange r{}; if (have) r = tri_range(pos + (size_t)t * 9u, g);
        for_each_cell(have, r, t, g, [&](uint32_t cell, uint32_t) { atomicAdd(&counts[cell], 1u); });
    }
}

__global__ __launch_bounds__(kGridThreads) void grid_fill_kernel(const float* __restrict__ pos, uint32_t triCount, GridParams g, uint32_t* cursor, int32_t* refs, uint32_t total)
{
    for (uint32_t base = blockIdx.x * kGridThreads; base < triCount; base += gridDim.x * kGridThreads) {
        const uint32_t t = base + threadIdx.x; const bool have = t < triCount;
        CellRange r{}; if (have) r = tri_range(pos + (size_t)t * 9u, g);
        for_each_cell(have, r, t, g, [&](uint32_t cell, uint32_t tri) { const uint32_t slot = atomicAdd(&cursor[cell], 1u); if (slot < total) refs[slot] = (int32_t)tri; });
    }
}

// every cell's segment of `in` in ascending order into `out` (the same offsets)
__global__ __launch_bounds__(kGridThreads) void grid_sort_kernel(const uint32_t* __restrict__ cellStart, uint32_t cells, uint32_t total, const int32_t* __restrict__ in, int32_t* out)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * kGridThreads; base < cells; base += gridDim.x * kGridThreads) {
        const uint32_t c = base + threadIdx.x;
        uint32_t s = 0, len = 0;
        if (c < cells) { s = cellStart[c]; const uint32_t e = cellStart[c + 1]; if (s <= e && e <= total) len = e - s; }
        const bool wide = len > kLaneCellRefs;
        if (!wide)
            for (uint32_t i = 0; i < len; i++) {
                const int32_t x = in[s + i]; uint32_t r = 0;
                for (uint32_t j = 0; j < len; j++) r += in[s + j] < x ? 1u : 0u;
                out[s + r] = x;
            }
        unsigned long long m = __builtin_amdgcn_ballot_w64(wide);
        while (m) {
            const int src = __builtin_ctzll(m); m &= m - 1;
            const uint32_t sb = __shfl(s, src), lb = __shfl(len, src);
            for (uint32_t i = lane; i < lb; i += 64u) {
                const int32_t x = in[sb + i]; uint32_t r = 0;
                for (uint32_t j = 0; j < lb; j++) r += in[sb + j] < x ? 1u : 0u;
                out[sb + r] = x;
            }
        }
    }
}

// one lane per leaf slot of the BVH: slot j holds triangle shadeIdx - triBase and the object id a hit reports; the record goes to the triangle's own place
__global__ __launch_bounds__(kGridThreads) void grid_tris_kernel(const char* __restrict__ geom, uint32_t leafOff, uint32_t triBase, uint32_t triCount, const float* __restrict__ pos,
                                                                 int globalIdx, AltTri* out)
{
    const uint32_t j = blockIdx.x * kGridThreads + threadIdx.x;
    if (j >= triCount) return;
    const row4* lt = reinterpret_cast<const row4*>(geom + leafOff + (size_t)(triBase + j) * 48u);
    const uint32_t shadeIdx = __float_as_uint(lt[0].w), objIdx = __float_as_uint(lt[1].w);
    const uint32_t tri = shadeIdx - triBase;
    if (tri >= triCount) return;
    const float* v = pos + (size_t)tri * 9u;
    const float v0x = v[0], v0y = v[1], v0z = v[2];
    row4 r0, r1, r2;
    r0.x = v0x; r0.y = v0y; r0.z = v0z; r0.w = __uint_as_float(globalIdx ? shadeIdx : tri);
    r1.x = v[3] - v0x; r1.y = v[4] - v0y; r1.z = v[5] - v0z; r1.w = __uint_as_float(objIdx);
    r2.x = v[6] - v0x; r2.y = v[7] - v0y; r2.z = v[8] - v0z; r2.w = 0.0f;
    row4* o = reinterpret_cast<row4*>(out + tri);
    o[0] = r0; o[1] = r1; o[2] = r2;
}

} // namespace crt

// workgroups of 256 lanes the device holds at once for the build's kernels (occupancy of the count kernel x compute units); 0: the device could not be asked
extern "C" uint32_t crt_grid_build_blocks(int device)
{
    int perCu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, crt::grid_count_kernel, (int)crt::kGridThreads, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || perCu <= 0 || cus <= 0) { (void)hipGetLastError(); return 0u; }
    return (uint32_t)perCu * (uint32_t)cus;
}

extern "C" size_t crt_grid_scan_chunks(uint32_t cells) { return crt::scan_chunks((size_t)cells + 1u); }

extern "C" hipError_t crt_launch_grid_bounds(const float* pos, uint32_t triCount, crt::GridBuildState* state, uint32_t maxBlocks, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(state, 0, sizeof(crt::GridBuildState), stream);
    if (e == hipSuccess) e = hipMemsetAsync(state, 0xff, 3 * sizeof(unsigned long long), stream);   // the three minimum keys
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::grid_bounds_kernel, dim3(crt::blocks_for(3u * triCount, maxBlocks)), dim3(crt::kGridThreads), 0, stream, pos, 3u * triCount, state);
    return hipGetLastError();
}

// counts: cells + 1 words; comes back as cellStart.  chunkSums: crt_grid_scan_chunks(cells) 64-bit words of scratch.  state->total receives the reference count.
extern "C" hipError_t crt_launch_grid_count(const float* pos, uint32_t triCount, const crt::GridParams* g, uint32_t cells, uint32_t* counts, unsigned long long* chunkSums,
                                            crt::GridBuildState* state, uint32_t maxBlocks, hipStream_t stream)
{
    const uint32_t n = cells + 1u, chunks = (uint32_t)crt_grid_scan_chunks(cells);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * 4u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crt::grid_count_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), dim3(crt::kGridThreads), 0, stream, pos, triCount, *g, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return crt::scan(counts, n, chunks, chunkSums, (uint32_t*)nullptr, &state->total, stream);     // (the last counter is 0, so counts[cells] ends as the total too)
}

// cursor: cells words of scratch; unsorted: total words of scratch; refs: the total references of the finished grid; tris: the BVH's triCount AltTri records
extern "C" hipError_t crt_launch_grid_fill(const float* pos, uint32_t triCount, const crt::GridParams* g, uint32_t cells, const uint32_t* cellStart, uint32_t* cursor, int32_t* unsorted,
                                           int32_t* refs, uint32_t total, const char* geom, uint32_t leafOff, uint32_t triBase, int globalIdx, crt::AltTri* tris, uint32_t maxBlocks,
                                           hipStream_t stream)
{
    hipError_t e = hipSuccess;
    if (total) {
        if ((e = hipMemcpyAsync(cursor, cellStart, (size_t)cells * 4u, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(crt::grid_fill_kernel, dim3(crt::blocks_for(triCount, maxBlocks)), dim3(crt::kGridThreads), 0, stream, pos, triCount, *g, cursor, unsorted, total);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(crt::grid_sort_kernel, dim3(crt::blocks_for(cells, maxBlocks)), dim3(crt::kGridThreads), 0, stream, cellStart, cells, total, unsorted, refs);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(crt::grid_tris_kernel, dim3((triCount + crt::kGridThreads - 1u) / crt::kGridThreads), dim3(crt::kGridThreads), 0, stream, geom, leafOff, triBase, triCount, pos,
                       globalIdx, tris);
    return hipGetLastError();
}

// the AltTri records alone (crt_build_kdtree_device writes them as the grid build does)
extern "C" hipError_t crt_launch_alt_tris(const float* pos, uint32_t triCount, const char* geom, uint32_t leafOff, uint32_t triBase, int globalIdx, crt::AltTri* tris, hipStream_t stream)
{
    hipLaunchKernelGGL(crt::grid_tris_kernel, dim3((triCount + crt::kGridThreads - 1u) / crt::kGridThreads), dim3(crt::kGridThreads), 0, stream, geom, leafOff, triBase, triCount, pos,
                       globalIdx, tris);
    return hipGetLastError();
}
