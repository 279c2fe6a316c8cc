// tlas_alt.hip — scene.FindNearest / scene.IsOccluded of a TLASFileScene built with TLAS_USE_KDTree or TLAS_USE_Grid (tlas_file_scene.cpp:40-90, 201-218) for a
// buffer of rays, over the BLAS set of crt_upload_blas_accel:
//   tlas_alt_query_kernel<1|2, false>   find-nearest: light quad, floor plane, then TLASKDTree::Intersect / TLASGrid::Intersect
//   tlas_alt_query_kernel<1|2, true>    IsOccluded: the light quad bounded by the ray's t, then the walk over the whole ray (shadow.t = 1e34f), stopped at the first
//                                       successful triangle test
// Records as find_nearest_kernel's for a TLAS scene: objIdx = the BLAS's, triIdx BLAS-local, traversed = TLAS steps + every BLAS's steps, tested over the query.
// Form: the persistent waves of alt_accel.hip and find_nearest_kernel — a lane whose ray is finished takes the next one from the launch-wide cursor once a quarter
// of the wavefront is idle, and one trip of the wave's loop runs each KIND of step once for the lanes at it: TLAS step, instance entry, KD node or grid cell, one
// triangle test, return to the caller frame or DDA advance, return to the TLAS.  Per ray these are the steps of alt_common.h's tlas_alt_intersect (the render and
// Whitted kernels' walk) in the same order with the same arithmetic: the same nodes, cells and triangles (tests/tlas_alt_restate.py, compared field for field).
#include "alt_common.h"
#include "launch.h"

namespace crt {

struct RayIn { float O[3]; float D[3]; int32_t inside; };
struct HitOut { float t, u, v; int32_t objIdx, triIdx, traversed, tested; };
struct ShadowRayIn { float O[3]; float D[3]; float t; };

constexpr uint32_t kQueryRefill = 16u;                                   // idle lanes that trigger the next draw from the cursor (as alt_accel.hip)

// OCCL: exact for the reason of is_occluded_kernel (kernels.hip), and BLASKDTree's early return does not change it: until the first successful triangle test the
// shadow ray's objIdx is -1, so `ray.objIdx == objIdx && ray.t < t` never holds and every box, plane, pop and DDA decision is the full walk's.
template <int ACCEL, bool OCCL>
__global__ __launch_bounds__(64) void tlas_alt_query_kernel(const Scene sc, const TlasAltDev tl, const void* __restrict__ rays, void* __restrict__ out, uint32_t n,
                                                             uint32_t* __restrict__ cursor)
{
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const char* __restrict__ g = sc.geom;
    const KdNode* __restrict__ kdNodes = reinterpret_cast<const KdNode*>(tl.kdNodes);
    const AltTri* __restrict__ tris = reinterpret_cast<const AltTri*>(tl.tris);
    uint32_t* stkNode = lds + lane;                                       // KD: (far child, plane distance) frames, alt_common.h layout
    uint32_t* tstk = stkNode + tl.kdStack * 128u;                         // TLAS entries above them (tlas_alt_intersect's layout)
    // the ray in this lane.  mode: 0 idle, 3 at a TLAS reference (`tcur`), 5 entering instance `inst`, 1 at a KD node / grid cell, 2 in a triangle list,
    // 6 this BLAS is done (back to the TLAS), 4 finished
    uint32_t mode = 0u;
    uint32_t idx = 0; f3 O = mk3(0, 0, 0), D = O, rD = O, Oo = O, Do = O, rDo = O;   // world-space ray; the object-space ray of the BLAS being walked
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    int traversed = 0, tested = 0;
    uint32_t tcur = 0, tsp = 0, inst = 0;
    int32_t objIdx = 0;                                                   // the BLAS's objIdx (BLASKDTree's early return)
    uint32_t triBase = 0, nodeBase = 0, refBase = 0;                      // the BLAS's slices: triangles; KD nodes / grid cellStart; leaf / cell references
    uint32_t triK = 0, triEnd = 0;
    int32_t node = 0; uint32_t sp = 0;                                    // KD-tree
    int32_t res0 = 0, res1 = 0;                                           // grid (3D-DDA state, blas_grid.cpp:183-211)
    int exitc[3] = {0, 0, 0}, step[3] = {0, 0, 0}, c[3] = {0, 0, 0}; float deltaT[3] = {0, 0, 0}, next[3] = {0, 0, 0};
    bool more = true;                                                     // wave-uniform: the cursor has rays left
    for (;;) {
        // ---------------- refill: idle lanes draw the next rays ----------------
        const uint64_t mIdle = __builtin_amdgcn_ballot_w64(mode == 0u);
        const uint32_t nIdle = (uint32_t)__popcll(mIdle);
        if (more && (nIdle >= kQueryRefill)) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, nIdle);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            more = base + nIdle < n;
            const uint32_t my = base + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mIdle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mIdle, 0u));
            if (mode == 0u && my < n) {
                idx = my;
                h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1; traversed = 0; tested = 0;
                tcur = sc.rootRef; tsp = 0;
                if (OCCL) {
                    const ShadowRayIn r = reinterpret_cast<const ShadowRayIn*>(rays)[idx];
                    O = mk3(r.O[0], r.O[1], r.O[2]); D = mk3(r.D[0], r.D[1], r.D[2]);
                    if (quad_occluded(sc, O, D, r.t)) reinterpret_cast<int32_t*>(out)[idx] = 1;   // the lane stays idle
                    else { rD = mk3(1 / D.x, 1 / D.y, 1 / D.z); mode = 3u; }
                } else {
                    const RayIn r = reinterpret_cast<const RayIn*>(rays)[idx];
                    O = mk3(r.O[0], r.O[1], r.O[2]); D = mk3(r.D[0], r.D[1], r.D[2]);
                    rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);                  // Ray ctor, template/ray.h:15-24
                    hit_light_floor(sc, O, D, h);
                    mode = 3u;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(mode != 0u) == 0ull) {
            if (!more) break;                                             // nothing in flight, nothing left to draw
            continue;                                                     // (occlusion: every drawn ray was quad-occluded) draw again
        }
        // ---------------- TLAS step (tlas_bvh.cpp:83-111): a leaf names the instance to enter, an interior node orders its children ----------------
        if (mode == 3u) {
            traversed++;
            if ((tcur & kRefTlasLeaf) == kRefTlasLeaf) { inst = tcur & 0xffffu; mode = 5u; }
            else {
                const uint32_t o1 = sc.tlasOff + (tcur & 0x7fffu) * 32u, o2 = sc.tlasOff + ((tcur >> 15) & 0x7fffu) * 32u;
                const rec4 alo = ldg(g, o1), ahi = ldg(g, o1 + 16), blo = ldg(g, o2), bhi = ldg(g, o2 + 16);
                float d1 = box_exact(alo, ahi, O, rD, h.t), d2 = box_exact(blo, bhi, O, rD, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) { if (tsp == 0) mode = 4u; else tcur = tstk[(--tsp) * 64]; }
                else { tcur = r1; if (d2 != 1e30f) { tstk[tsp * 64] = r2; tsp++; } }
            }
        }
        // ---------------- instance entry: BLASKDTree::Intersect / BLASGrid::Intersect's transform (blas_kdtree.cpp:420-433, blas_grid.cpp:233-248) ----------------
        if (mode == 5u) {
            const uint32_t io = sc.instOff + inst * 128u;
            const rec4 r0 = ldg(g, io), r1 = ldg(g, io + 16), r2 = ldg(g, io + 32), ids = ldg(g, io + 48);
            to_object_space(r0, r1, r2, O, D, Oo, Do, rDo);
            objIdx = (int32_t)asu(ids.w);
            const BlasAltDesc& d = tl.desc[inst];
            triBase = d.triBase;
            mode = 1u;
            if (ACCEL == 1) { nodeBase = d.nodeBase; refBase = d.refBase; node = 0; sp = 0; }
            else {
                // BLASGrid::IntersectGrid up to its loop, blas_grid.cpp:183-211
                nodeBase = d.cellBase; refBase = d.cellRefBase; res0 = d.res[0]; res1 = d.res[1];
                float lo[3], hi[3], cell[3]; int32_t res[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) { lo[a] = d.lo[a]; hi[a] = d.hi[a]; cell[a] = d.cell[a]; res[a] = d.res[a]; }
                float tmn, tmx;
                if (!alt_box(lo, hi, Oo, rDo, h.t, tmn, tmx)) mode = 6u;    // misses the grid: back to the TLAS
                else {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float rayOrigCell = comp(Oo, a) - lo[a];
                        c[a] = clampi((int)__builtin_floorf(rayOrigCell / cell[a]), 0, res[a] - 1);
                        if (comp(Do, a) < 0) { deltaT[a] = -cell[a] * comp(rDo, a); next[a] = ((float)c[a] * cell[a] - rayOrigCell) * comp(rDo, a); exitc[a] = -1; step[a] = -1; }
                        else { deltaT[a] = cell[a] * comp(rDo, a); next[a] = ((float)(c[a] + 1) * cell[a] - rayOrigCell) * comp(rDo, a); exitc[a] = res[a]; step[a] = 1; }
                    }
                }
            }
        }
        bool leave = false;                                               // this lane's BLAS step is over: KD -> return to the caller frames, grid -> advance the DDA
        if (ACCEL == 1) {
            // ---------------- BLASKDTree::IntersectKDTree(ray, node), blas_kdtree.cpp:336-398: one node per trip ----------------
            if (mode == 1u) {
                traversed++;
                const KdNode nd = kdNodes[nodeBase + (uint32_t)node];
                float tmin, tmax;
                leave = true;
                if (alt_box(nd.lo, nd.hi, Oo, rDo, h.t, tmin, tmax)) {
                    if (nd.left < 0) {
                        if (nd.triCount) { triK = nd.firstTri; triEnd = nd.firstTri + nd.triCount; mode = 2u; leave = false; }
                    } else {
                        const int axis = nd.splitAxis;
                        const float splitPos = nd.lo[axis] + nd.splitDistance;
                        const float t = (splitPos - comp(Oo, axis)) / comp(Do, axis);
                        const bool pos = comp(Do, axis) > 0;
                        const int32_t first = pos ? nd.left : nd.right, second = pos ? nd.right : nd.left;
                        if ((double)t < (double)tmin + 0.001) node = second;                    // the plane lies before the box: only the far side
                        else if ((double)t > (double)tmax - 0.001) node = first;               // ... behind it: only the near side
                        else { stkNode[sp * 128u] = (uint32_t)second; stkNode[sp * 128u + 64u] = asu(t); sp++; node = first; }
                        leave = false;
                    }
                }
            } else if (mode == 2u) {
                // ---------------- one triangle of the leaf, blas_kdtree.cpp:344-353 ----------------
                alt_tri(tris + triBase, tl.kdRefs[refBase + triK], Oo, Do, h); tested++;
                triK++;
                if (OCCL && h.objIdx > -1) mode = 4u;                      // the first successful test ends the walk
                else if (triK == triEnd) { leave = true; mode = 1u; }
            }
            if (leave) {
                // return to the caller frames: `IntersectKDTree(first); if (ray.objIdx == objIdx && ray.t < t) return; IntersectKDTree(second);` (:377, :396)
                bool found = false;
                while (sp > 0) {
                    sp--;
                    const float t = asf(stkNode[sp * 128u + 64u]);
                    if (h.objIdx == objIdx && h.t < t) continue;
                    node = (int32_t)stkNode[sp * 128u]; found = true; break;
                }
                if (!found) mode = 6u;
            }
        } else {
            // ---------------- one cell of the 3D-DDA, blas_grid.cpp:212-231 ----------------
            if (mode == 1u) {
                traversed++;
                const uint32_t index = (uint32_t)c[0] + (uint32_t)c[1] * (uint32_t)res0 + (uint32_t)c[2] * (uint32_t)res0 * (uint32_t)res1;
                triK = tl.cellStart[nodeBase + index]; triEnd = tl.cellStart[nodeBase + index + 1];
                if (triK < triEnd) mode = 2u; else leave = true;
            } else if (mode == 2u) {
                tested++; alt_tri(tris + triBase, (uint32_t)tl.cellRefs[refBase + triK], Oo, Do, h);
                triK++;
                if (OCCL && h.objIdx > -1) mode = 4u;
                else if (triK == triEnd) { leave = true; mode = 1u; }
            }
            if (leave) {
                const uint32_t k = ((uint32_t)(next[0] < next[1]) << 2) + ((uint32_t)(next[0] < next[2]) << 1) + (uint32_t)(next[1] < next[2]);
                const int axis = (0x00221212u >> (4u * k)) & 0xfu;             // map[8] = {2, 1, 2, 1, 2, 2, 0, 0}, blas_grid.cpp:222
                const float nx = axis == 0 ? next[0] : (axis == 1 ? next[1] : next[2]);
                if (h.t < nx) mode = 6u;
                else {
                    bool outc = false;
                    if (axis == 0) { c[0] += step[0]; outc = c[0] == exitc[0]; next[0] += deltaT[0]; }
                    else if (axis == 1) { c[1] += step[1]; outc = c[1] == exitc[1]; next[1] += deltaT[1]; }
                    else { c[2] += step[2]; outc = c[2] == exitc[2]; next[2] += deltaT[2]; }
                    if (outc) mode = 6u;
                }
            }
        }
        // ---------------- return to the TLAS loop (tlas_bvh.cpp:95): its next stack entry, or the walk is over ----------------
        if (mode == 6u) { if (tsp == 0) mode = 4u; else { tcur = tstk[(--tsp) * 64]; mode = 3u; } }
        if (mode == 4u) {                                                  // finished: the result record, and the lane is free
            if (OCCL) reinterpret_cast<int32_t*>(out)[idx] = h.objIdx > -1 ? 1 : 0;
            else {
                int triIdx = h.triIdx;
                if (h.objIdx >= 2) triIdx -= (int)asu(ldg(g, sc.instOff + (uint32_t)(h.objIdx - 2) * 128u + 48u).x);   // - Instance::shadeBase: BLAS-local
                HitOut o; o.t = h.t; o.u = h.u; o.v = h.v; o.objIdx = h.objIdx; o.triIdx = triIdx; o.traversed = traversed; o.tested = tested;
                reinterpret_cast<HitOut*>(out)[idx] = o;
            }
            mode = 0u;
        }
    }
}

} // namespace crt

extern "C" hipError_t crt_launch_tlas_alt_query(int kind, bool occl, const crt::Scene* sc, const crt::TlasAltDev* tl, const void* rays, void* out, uint32_t n, uint32_t* cursor,
                                                hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (sc->kind == 0 || (kind != 1 && kind != 2)) return hipErrorInvalidValue;
    const uint32_t ldsBytes = crt::tlas_alt_stack_words(*sc, *tl) * 64u * 4u;
    if (ldsBytes > 64u * 1024u) return hipErrorInvalidValue;
    hipError_t e; if (!crt::query_launch_begin(n, cursor, stream, &e)) return e;       // no rays: nothing to do; the cursor zeroed on the stream (launch.h)
    dim3 grid(crt::query_grid(n, ldsBytes)), block(64);
    if (occl) {
        if (kind == 1) hipLaunchKernelGGL((crt::tlas_alt_query_kernel<1, true>), grid, block, ldsBytes, stream, *sc, *tl, rays, out, n, cursor);
        else hipLaunchKernelGGL((crt::tlas_alt_query_kernel<2, true>), grid, block, ldsBytes, stream, *sc, *tl, rays, out, n, cursor);
    } else {
        if (kind == 1) hipLaunchKernelGGL((crt::tlas_alt_query_kernel<1, false>), grid, block, ldsBytes, stream, *sc, *tl, rays, out, n, cursor);
        else hipLaunchKernelGGL((crt::tlas_alt_query_kernel<2, false>), grid, block, ldsBytes, stream, *sc, *tl, rays, out, n, cursor);
    }
    return hipGetLastError();
}
