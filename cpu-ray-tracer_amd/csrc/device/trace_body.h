// trace_body.h — the ONE definition of the Whitted integrator's per-ray body, Renderer::Trace(ray, depth) ("2. WhittedStyle/renderer.cpp":21-91), for every kernel
// that runs it: whitted_kernel (kernels.hip: one thread per pixel of the context's camera) and trace_query_kernel (trace_query.h: a caller's rays).
//
// Trace()'s recursion (a dielectric spawns a refracted AND a reflected ray) runs on an explicit frame stack in post-order, so every float sum and product happens
// in the reference's order:  return medium * (((0 + cA*Trace(a)) + cB*Trace(b)) + C).  The machine has two steps over a lane's TraceState + its frames:
//     trace_descend   Trace(ray, depth = sp) up to the point where it needs its children: the depth test (trace_depth_cut), FindNearest, the surface,
//                     DirectIllumination with whitted_occluded (at most one shadow walk), the child set-up.  One traversal (+ at most one shadow walk) per call.
//     trace_return    a child returned `res` to the frame below it: accumulate, start child B, or complete the frame.  No traversal.  true: the root completed.
// A kernel loops `if (t.descend) trace_descend(...); else if (trace_return(...)) break;` — how it interleaves the two among its lanes is the kernel's business.
// The traversal is dev_common.h's / alt_common.h's (find_nearest_seq, traverse_bvh_seq, hit_light_floor, alt_walk), the surface sample_body.h's.
//
// Numerics: -ffp-contract=off, IEEE + - * / sqrt only, crt_expf inside medium_of.  No MFMA.
#pragma once
#include "alt_common.h"
#include "sample_body.h"

namespace crt {

struct WFrame { f3 cA, cB, C, medium, out, bO, bD; int flags; };     // flags: 1 hasA, 2 hasB, 4 hasC, 8 b.inside, 16 waiting for B
constexpr int kWhittedMaxDepth = 7;

// a lane's tree: the ray (O, D, inside) is traced at depth `sp` (= frames in use) when `descend`, else `res` is what the child at depth `sp` returned
struct TraceState { f3 O, D; bool inside; int sp; f3 res; bool descend; };
__device__ __forceinline__ void trace_begin(TraceState& t, f3 O, f3 D, bool inside) { t.O = O; t.D = D; t.inside = inside; t.sp = 0; t.res = mk3(0, 0, 0); t.descend = true; }

// renderer.cpp:23, `if (depth > depthLimit) return 0`, checked BEFORE tracing: true when the pending descend at depth t.sp ended there (t.res = 0, a return is next)
__device__ __forceinline__ bool trace_depth_cut(const Scene& sc, TraceState& t)
{
    if (t.sp > sc.depthLimit) { t.res = mk3(0, 0, 0); t.descend = false; return true; }
    return false;
}

template <int ACCEL, class ALT>
__device__ __forceinline__ bool whitted_occluded(const Scene& sc, const ALT& alt, f3 O, f3 D, float tmax, uint32_t* stk, Cnt& cn)   // FileScene::IsOccluded, file_scene.cpp:177-187
{
    {   // Quad::IsOccluded, primitives.h:347-362
        const float* c = sc.lightInvT;
        const float Oy = c[4] * O.x + c[5] * O.y + c[6] * O.z + c[7];
        const float Dy = c[4] * D.x + c[5] * D.y + c[6] * D.z;
        const float t = Oy / -Dy;
        if (t < tmax && t > 0) {
            const float Ox = c[0] * O.x + c[1] * O.y + c[2] * O.z + c[3];
            const float Oz = c[8] * O.x + c[9] * O.y + c[10] * O.z + c[11];
            const float Dx = c[0] * D.x + c[1] * D.y + c[2] * D.z;
            const float Dz = c[8] * D.x + c[9] * D.y + c[10] * D.z;
            const float Ix = Ox + t * Dx, Iz = Oz + t * Dz;
            const float size = sc.lightSize;
            if (Ix > -size && Ix < size && Iz > -size && Iz < size) return true;
        }
    }
    // shadow.t = 1e34f; acc.Intersect(shadow): a full nearest-hit query over the whole ray (bug-compatible: not clipped at the light)
    Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
    const f3 rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);
    int traversed = 0, tested = 0;
    cn.rays++;
    if constexpr (ACCEL != 0) alt_walk<ACCEL>(sc, alt, O, D, rD, h, stk, traversed, tested);   // (stk: this lane's column, two words per KD entry)
    else if (sc.kind == 0) traverse_bvh_seq(sc, sc.rootRef, O, D, rD, h, stk, cn, traversed, tested);
    else {
        Hit hh = h; Cnt dummy = cn;
        // TLAS walk without the quad / plane tests: reuse find_nearest_seq's TLAS part through a light-less copy is not possible, so inline it
        const char* __restrict__ g = sc.geom;
        uint32_t* tstk = stk + sc.bvhStack * 64;
        uint32_t cur = sc.rootRef, sp = 0;
        for (;;) {
            cn.tlas++;
            if ((cur & kRefTlasLeaf) == kRefTlasLeaf) {
                cn.visits++;
                const uint32_t io = sc.instOff + (cur & 0xffffu) * 128u;
                const rec4 r0 = ldg(g, io), r1 = ldg(g, io + 16), r2 = ldg(g, io + 32), ids = ldg(g, io + 48);
                f3 Oo, Do, rDo; to_object_space(r0, r1, r2, O, D, Oo, Do, rDo);
                traverse_bvh_seq(sc, asu(ids.z), Oo, Do, rDo, h, stk, cn, traversed, tested);
                if (sp == 0) break;
                cur = tstk[(--sp) * 64];
            } else {
                const uint32_t o1 = sc.tlasOff + (cur & 0x7fffu) * 32u, o2 = sc.tlasOff + ((cur >> 15) & 0x7fffu) * 32u;
                const rec4 alo = ldg(g, o1), ahi = ldg(g, o1 + 16), blo = ldg(g, o2), bhi = ldg(g, o2 + 16);
                float d1 = box_exact(alo, ahi, O, rD, h.t), d2 = box_exact(blo, bhi, O, rD, h.t);
                uint32_t r1 = asu(alo.w), r2 = asu(blo.w);
                if (d1 > d2) { float td = d1; d1 = d2; d2 = td; uint32_t tr = r1; r1 = r2; r2 = tr; }
                if (d1 == 1e30f) { if (sp == 0) break; cur = tstk[(--sp) * 64]; }
                else { cur = r1; if (d2 != 1e30f) { tstk[sp * 64] = r2; sp++; } }
            }
        }
        (void)hh; (void)dummy;
    }
    return h.objIdx > -1;
}

// ---- Trace(ray, depth = t.sp) up to the point where it needs its children.  ACCEL: 0 = the scene's BVH / TLAS, 1 / 2 = the KD-tree / uniform grid for both the
// nearest-hit and the shadow queries: FileScene's (ALT = AltAccelDev) or a two-level scene's set (ALT = TlasAltDev).  COUNTS: the depth-0 ray's Ray::traversed /
// Ray::tested go to primTraversed / primTested.  On return t.descend says whether the next step is the first child's descend or a return with t.res.
template <int ACCEL, bool COUNTS, class ALT>
__device__ __forceinline__ void trace_descend(const Scene& sc, const ALT& alt, uint32_t* stk, Cnt& cn, TraceState& t, WFrame* fr, int32_t& primTraversed, int32_t& primTested)
{
    f3& O = t.O; f3& D = t.D; bool& inside = t.inside; int& sp = t.sp; f3& res = t.res;
    if (trace_depth_cut(sc, t)) return;
    bool terminal = true;
    {
        Hit h; h.t = 1e34f; h.u = 0; h.v = 0; h.objIdx = -1; h.triIdx = -1;
        const f3 rD = mk3(1 / D.x, 1 / D.y, 1 / D.z);
        int traversed = 0, tested = 0;
        if (ACCEL == 0) find_nearest_seq(sc, O, D, rD, h, stk, cn, traversed, tested);
        else {
            cn.rays++;
            hit_light_floor(sc, O, D, h);
            alt_walk<ACCEL>(sc, alt, O, D, rD, h, stk, traversed, tested);
            if (h.objIdx >= 2) cn.meshhits++;
        }
        if constexpr (COUNTS) { if (sp == 0) { primTraversed = traversed; primTested = tested; } }
        if (h.objIdx == -1) res = sky_color(sc, D);
        else if (h.objIdx == 0) res = mk3(24, 24, 22);
        else {
            const f3 I = O + h.t * D;
            SurfPoint p;
            if (h.objIdx == 1) p = floor_point(mk3(sc.floorN[0], sc.floorN[1], sc.floorN[2]), sc.floorInvto, sc.floorMat, I);
            else {
                const uint32_t so = sc.shadeOff + (uint32_t)h.triIdx * 64u;
                const rec4 s0 = ldg(sc.geom, so), s1 = ldg(sc.geom, so + 16), s2 = ldg(sc.geom, so + 32), s3 = ldg(sc.geom, so + 48);
                p = sc.kind == 0 ? mesh_point<0>(s0, s1, s2, s3, h.u, h.v, h.objIdx, sc.geom, sc.instOff, sc.mats)
                                 : mesh_point<1>(s0, s1, s2, s3, h.u, h.v, h.objIdx, sc.geom, sc.instOff, sc.mats);
            }
            const f3 N = face_ray(p.N, D);
            const f3 albedo = (p.tW > 0) ? tex_sample(sc, p.tOff, p.tW, p.tH, p.tu, p.tv) : mk3(1.0f, 1.0f, 1.0f);
            WFrame& f = fr[sp];
            f.flags = 0; f.out = mk3(0, 0, 0);
            const float refl = p.refl, refr = p.refr;
            const float diffuseness = 1 - (refl + refr);
            f3 aO = O, aD = D; bool aInside = false;
            if (refl > 0.0f) {                                               // renderer.cpp:49-54
                const f3 R = D - 2.0f * N * dot3(N, D);
                aO = I + R * CRT_EPS; aD = R; aInside = false;
                f.cA = refl * albedo; f.flags |= 1;
            } else if (refr > 0.0f) {                                        // renderer.cpp:55-72
                const f3 R = D - 2.0f * N * dot3(N, D);
                const float n1 = inside ? 1.2f : 1, n2 = inside ? 1 : 1.2f;
                const float eta = n1 / n2, cosi = dot3(-D, N);
                const float cost2 = 1.0f - eta * eta * (1 - cosi * cosi);
                float Fr = 1;
                if (cost2 > 0) {
                    const float a = n1 - n2, b = n1 + n2, R0 = (a * a) / (b * b), c = 1 - cosi;
                    Fr = R0 + (1 - R0) * (c * c * c * c * c);
                    const f3 T = eta * D + ((eta * cosi - __builtin_sqrtf(__builtin_fabsf(cost2))) * N);
                    aO = I + T * CRT_EPS; aD = T; aInside = !inside;
                    f.cA = albedo * (1 - Fr); f.flags |= 1;
                }
                f.bO = I + R * CRT_EPS; f.bD = R; f.cB = albedo * Fr; f.flags |= 2;
            }
            if (diffuseness > 0) {                                           // renderer.cpp:74-80, DirectIllumination :105-126
                f3 irr = mk3(0, 0, 0);
                f3 L = mk3(sc.lightPos[0], sc.lightPos[1], sc.lightPos[2]) - I;
                const float dist = __builtin_sqrtf(dot3(L, L));
                L = L * (1 / dist);
                const float ndotl = dot3(N, L);
                if (!(ndotl < CRT_EPS)) {
                    if (!whitted_occluded<ACCEL>(sc, alt, I + L * CRT_EPS, L, dist - 2 * CRT_EPS, stk, cn)) {
                        const float att = 1 / (dist * dist);
                        const f3 inr = mk3(24, 24, 22) * att;
                        irr = inr * dot3(N, L);
                    }
                }
                const f3 brdf = albedo * CRT_INVPI;
                f.C = diffuseness * brdf * (irr + mk3(0.3f, 0.3f, 0.3f)); f.flags |= 4;
            }
            f.medium = medium_of(inside, p.absorb, h.t);
            terminal = false;
            if (f.flags & 1) { O = aO; D = aD; inside = aInside; sp++; }                      // trace child A next
            else if (f.flags & 2) { O = f.bO; D = f.bD; inside = false; f.flags |= 16; sp++; } // (not reachable in the reference: B only exists with refr > 0)
            else { res = (f.flags & 4) ? f.out + f.C : f.out; res = f.medium * res; terminal = true; }
        }
    }
    if (terminal) t.descend = false;
}

// ---- a child returned t.res to the frame below it.  true: there is no frame below (t.res is the root's Trace); false: t.descend says what comes next
__device__ __forceinline__ bool trace_return(TraceState& t, WFrame* fr)
{
    if (t.sp == 0) return true;
    WFrame& f = fr[t.sp - 1];
    bool finalize = true;
    if (!(f.flags & 16)) {                                                   // it was child A (or the only child)
        if (f.flags & 1) f.out = f.out + f.cA * t.res;
        if (f.flags & 2) { t.O = f.bO; t.D = f.bD; t.inside = false; f.flags |= 16; t.descend = true; finalize = false; }
    } else f.out = f.out + f.cB * t.res;
    if (finalize) {
        f3 o = f.out;
        if (f.flags & 4) o = o + f.C;
        t.res = f.medium * o;
        t.sp--;
    }
    return false;
}

} // namespace crt
