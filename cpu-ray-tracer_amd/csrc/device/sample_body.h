// sample_body.h — the steps of Renderer::Sample ("3. PathTracer/renderer.cpp":50-100) that every render kernel evaluates, each defined ONCE: the surface of a floor
// or mesh hit, the medium's absorption, the bounce (mirror / dielectric / rejection-sampled diffuse) and its throughput factor, the primary ray, the recursion's
// return path, and the ordered two-child step of the traversal around it.  Plain functions on VALUES: where a kernel's operands come from (kernel-argument reads,
// Scene members, pre-loaded or freshly loaded records), when it issues its loads and how it schedules its lanes is the kernel's business and nothing here knows
// about it.  render_tiles_kernel, whitted_kernel (kernels.hip), render_pool_kernel (render_pool.hip), sample_step (seq_sample.h) and FileSurface (file_surface.h)
// call these; none of them has a copy.
//
// Numerics: as everywhere (dev_common.h) — every float expression as the reference writes it, the rnd draws in its order.
#pragma once
#include "dev_common.h"

namespace crt {

// ------------------------------------------------------------------------------------------------------------
// the surface at a hit: GetHitInfo's normal (NOT yet facing the ray: face_ray) and uv, and the Material's words
// ------------------------------------------------------------------------------------------------------------
struct SurfPoint { f3 N; float tu, tv, refl, refr; f3 absorb; uint32_t tOff; int tW, tH, mat; };   // mat: index into Scene::mats ([1] = the floor's)

// Material {reflectivity, refractivity, absorption[3], texOffset, texW, texH} as its two 16-byte halves
__device__ __forceinline__ void set_material(SurfPoint& p, rec4 m0, rec4 m1)
{
    p.refl = m0.x; p.refr = m0.y; p.absorb = mk3(m0.z, m0.w, m1.x);
    p.tOff = asu(m1.y); p.tW = (int)asu(m1.z); p.tH = (int)asu(m1.w);
}
// floor: Plane::GetNormal / GetUV (primitives.h:112-133)
__device__ __forceinline__ SurfPoint floor_point(f3 floorN, float floorInvto, rec4 m0, rec4 m1, f3 I)
{
    SurfPoint p; p.N = floorN; p.tu = 0; p.tv = 0; p.mat = 1;
    if (floorN.y == 1) {
        float u = I.x, v = I.z;
        u *= floorInvto; v *= floorInvto;
        p.tu = u - __builtin_floorf(u); p.tv = v - __builtin_floorf(v);
    }
    set_material(p, m0, m1);
    return p;
}
__device__ __forceinline__ SurfPoint floor_point(f3 floorN, float floorInvto, const Material& m, f3 I)      // (the Material as a struct: Scene::floorMat)
{
    const rec4 m0 = {m.reflectivity, m.refractivity, m.absorption[0], m.absorption[1]}, m1 = {m.absorption[2], asf(m.texOffset), asf((uint32_t)m.texW), asf((uint32_t)m.texH)};
    return floor_point(floorN, floorInvto, m0, m1, I);
}
// mesh: GetNormal / GetUV (bvh.cpp:290-305, blas_bvh.cpp:391-406) from the hit's ShadeTri (s0..s3); KIND 1: the normal goes through the instance's T.
// (The T rows are fetched with ldp<>, whose assumption — 64 bytes from the given offset lie inside the geometry buffer — holds for `io`: it is the second
// 64-byte half of a 128-byte Instance record.)
// (materialOf(mat, m0, m1): fetches the two halves of the Material record ShadeTri::mat names — from the live table, below, or from a job-local look, render_looks.h)
template <int KIND, class MaterialOf>
__device__ __forceinline__ SurfPoint mesh_point_with(rec4 s0, rec4 s1, rec4 s2, rec4 s3, float u, float v, int objIdx, const char* __restrict__ geom, uint32_t instOff, MaterialOf&& materialOf)
{
    SurfPoint p;
    const f3 n0 = mk3(s0.x, s0.y, s0.z), n1 = mk3(s0.w, s1.x, s1.y), n2 = mk3(s1.z, s1.w, s2.x);
    const float w = 1 - u - v;
    const f3 Nn = w * n0 + u * n1 + v * n2;
    p.tu = w * s2.y + u * s2.w + v * s3.y;
    p.tv = w * s2.z + u * s3.x + v * s3.z;
    p.mat = (int)asu(s3.w);
    rec4 m0, m1;
    materialOf(p.mat, m0, m1);
    set_material(p, m0, m1);
    if (KIND == 0) p.N = normalize3(Nn);
    else {
        const uint32_t io = instOff + (uint32_t)(objIdx - 2) * 128u + 64u;       // Instance::T rows
        const rec4 r0 = ldp<0>(geom, io), r1 = ldp<1>(geom, io), r2 = ldp<2>(geom, io);
        p.N = normalize3(mk3(r0.x * Nn.x + r0.y * Nn.y + r0.z * Nn.z + r0.w * 0.0f,
                             r1.x * Nn.x + r1.y * Nn.y + r1.z * Nn.z + r1.w * 0.0f,
                             r2.x * Nn.x + r2.y * Nn.y + r2.z * Nn.z + r2.w * 0.0f));
    }
    return p;
}
template <int KIND>
__device__ __forceinline__ SurfPoint mesh_point(rec4 s0, rec4 s1, rec4 s2, rec4 s3, float u, float v, int objIdx, const char* __restrict__ geom, uint32_t instOff, const Material* __restrict__ mats)
{
    return mesh_point_with<KIND>(s0, s1, s2, s3, u, v, objIdx, geom, instOff, [&](int mat, rec4& m0, rec4& m1) __attribute__((always_inline)) {
        const rec4* mp = reinterpret_cast<const rec4*>(mats + mat);
        m0 = mp[0]; m1 = mp[1];
    });
}
__device__ __forceinline__ f3 face_ray(f3 N, f3 D) { return (dot3(N, D) > 0) ? -N : N; }

// ------------------------------------------------------------------------------------------------------------
// the bounce (renderer.cpp:73-99)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f3 medium_of(bool inside, f3 absorb, float t)
{
    f3 medium = mk3(1, 1, 1);
    if (inside) {
        const f3 ab = absorb * -t;
        medium = mk3(crt_expf(ab.x), crt_expf(ab.y), crt_expf(ab.z));
    }
    return medium;
}
enum Branch : int { kMirror, kDielectric, kDiffuse };
struct Bounce { f3 v; Branch branch; bool newInside; };                          // v: the outgoing direction; a diffuse one is still to be normalised
__device__ __forceinline__ Bounce draw_bounce(uint32_t& seed, f3 D, f3 N, bool inside, float refl, float refr)
{
    Bounce b; b.newInside = false;
    const float r = rnd(seed);
    if (r < refl) {                                                              // HandleMirror, renderer.cpp:20-25
        b.v = D - 2.0f * N * dot3(N, D); b.branch = kMirror;
    } else if (r < refl + refr) {                                                // HandleDielectric, renderer.cpp:27-45
        b.v = D - 2.0f * N * dot3(N, D); b.branch = kDielectric;
        const float n1 = inside ? 1.2f : 1, n2 = inside ? 1 : 1.2f;
        const float eta = n1 / n2, cosi = dot3(-D, N);
        const float cost2 = 1.0f - eta * eta * (1 - cosi * cosi);
        if (cost2 > 0) {
            const float a = n1 - n2, b2 = n1 + n2, R0 = (a * a) / (b2 * b2), cc = 1 - cosi;
            const float Fr = R0 + (1 - R0) * (cc * cc * cc * cc * cc);
            const f3 T = eta * D + ((eta * cosi - sqrt_exact(__builtin_fabsf(cost2))) * N);
            if (rnd(seed) > Fr) { b.v = T; b.newInside = !inside; }
        }
    } else {                                                                     // diffuse, renderer.cpp:93-99; diffusereflection tmplmath.h:535-544
        f3 Rr;
        do {
            const float rz = rnd_pm1(seed);                                      // draw order pinned z, y, x
            const float ry = rnd_pm1(seed);
            const float rx = rnd_pm1(seed);
            Rr = mk3(rx, ry, rz);
        } while (dot3(Rr, Rr) > 1);
        if (dot3(Rr, N) < 0) Rr = Rr * -1.0f;
        b.v = Rr; b.branch = kDiffuse;
    }
    return b;
}
// the bounce's throughput factor: albedo c, medium, and for a diffuse bounce the cosine with the NORMALISED direction nv
__device__ __forceinline__ f3 bounce_factor(Branch branch, f3 c, f3 medium, f3 nv, f3 N)
{
    if (branch != kDiffuse) return c * medium;
    const f3 brdf = c * CRT_INVPI;
    return medium * brdf * 2.0f * CRT_PI * dot3(nv, N);
}
// the recursion's return path: the factors of the `depth` bounces (per-lane column: component j of depth k at fst[(3k + j) * 64]) multiply the radiance innermost
// first (depth <= 5); a level is read only by the lanes that deep
__device__ __forceinline__ void sample_unwind(const float* fst, int depth, f3& L)
{
#pragma unroll
    for (int k = 4; k >= 0; k--)
        if (depth > k) { const float* fd = fst + (uint32_t)(3 * k) * 64u; L = mk3(fd[0], fd[64], fd[128]) * L; }
}

// ------------------------------------------------------------------------------------------------------------
// the ray's start
// ------------------------------------------------------------------------------------------------------------
// The RNG stream of frame `frame` (of the launch; `passes` samples per pixel and frame) of tile (tx, ty) of a W-wide image starts here (renderer.cpp:120).
__device__ __forceinline__ uint32_t stream_seed(uint32_t tx, uint32_t ty, uint32_t W, uint32_t sppFirst, uint32_t frame, uint32_t passes)
{
    return init_seed(tx + ty * W + (sppFirst + frame * passes) * 1799u);
}

// ------------------------------------------------------------------------------------------------------------
// the sample slab of a launch: [64-frame window][local tile] tile blocks of 256 pixel rows of rowLen = 64 x passes samples.  Every writer (render_pool_kernel,
// render_tiles_kernel, render_sky_kernel, render_seq_kernel) and every reader (accumulate_kernel, commit_frame_kernel) takes its byte positions from here.
//   sample form  12 bytes: L.x, L.y, L.z.  Sample (frame, pass) of a pixel at [frame-in-window x passes + pass] of the pixel's row: the order they are added in.
//   texel form    4 bytes: the packed sky texel, before tex_unpack.  Only the tiles of a render_sky_kernel launch whose accumulate follows at once hold it
//                 (abi.cpp launch_frames).  Its rows lie in the same tile block, [pixel][pass][frame-in-window]: the 64 lanes of one (pixel, pass) of that kernel
//                 write 256 contiguous bytes, and the tile touches the first third of its block only.
// Positions are bytes from the slab's start, 4-byte aligned.  (__host__ too: crt_debug_slab_layout evaluates them for the layout test without a device.)
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSampleBytes = 12u, kTexelBytes = 4u;
struct Sample3 { float x, y, z; };
__host__ __device__ __forceinline__ size_t slab_tile_bytes(uint32_t passes) { return (size_t)(256u * 64u * kSampleBytes) * passes; }
__host__ __device__ __forceinline__ size_t slab_window_bytes(uint32_t tileCount, uint32_t passes) { return (size_t)tileCount * slab_tile_bytes(passes); }
// a position = the tile's block of the frame's window + the sample's place inside the block (under 2^20: 32-bit arithmetic).  A kernel whose wavefront stays with
// one (window, tile) — render_tiles_kernel, render_seq_kernel — adds the block to its slab pointer once and stores at slab_sample_offset.
__host__ __device__ __forceinline__ size_t slab_block_position(uint32_t window, uint32_t tileCount, uint32_t tl, uint32_t rowLen)
{
    return ((size_t)window * tileCount + tl) * (256u * kSampleBytes) * rowLen;
}
// (slab_row_offset: by the sample's place in its pixel row, frameInWindow x passes + pass — what a reader that walks rows has in hand)
__host__ __device__ __forceinline__ uint32_t slab_row_offset(uint32_t pix, uint32_t rowLen, uint32_t sampleInRow) { return (pix * rowLen + sampleInRow) * kSampleBytes; }
__host__ __device__ __forceinline__ uint32_t slab_sample_offset(uint32_t frameInWindow, uint32_t pix, uint32_t rowLen, uint32_t passes, uint32_t pass)
{
    return slab_row_offset(pix, rowLen, frameInWindow * passes + pass);
}
__host__ __device__ __forceinline__ uint32_t slab_texel_offset(uint32_t frameInWindow, uint32_t pix, uint32_t passes, uint32_t pass)
{
    return ((pix * passes + pass) * 64u + frameInWindow) * kTexelBytes;
}
__host__ __device__ __forceinline__ size_t slab_position(uint32_t fr, uint32_t tileCount, uint32_t tl, uint32_t pix, uint32_t rowLen, uint32_t passes, uint32_t pass)
{
    return slab_block_position(fr >> 6, tileCount, tl, rowLen) + slab_sample_offset(fr & 63u, pix, rowLen, passes, pass);
}
__host__ __device__ __forceinline__ size_t slab_texel_position(uint32_t fr, uint32_t tileCount, uint32_t tl, uint32_t pix, uint32_t rowLen, uint32_t passes, uint32_t pass)
{
    return slab_block_position(fr >> 6, tileCount, tl, rowLen) + slab_texel_offset(fr & 63u, pix, passes, pass);
}
__device__ __forceinline__ void store_sample(char* __restrict__ slab, size_t at, f3 L) { Sample3 s; s.x = L.x; s.y = L.y; s.z = L.z; *reinterpret_cast<Sample3*>(slab + at) = s; }
__device__ __forceinline__ Sample3 load_sample(const char* __restrict__ slab, size_t at) { return *reinterpret_cast<const Sample3*>(slab + at); }
__device__ __forceinline__ void store_texel(char* __restrict__ slab, size_t at, uint32_t texel) { *reinterpret_cast<uint32_t*>(slab + at) = texel; }
__device__ __forceinline__ uint32_t load_texel(const char* __restrict__ slab, size_t at) { return *reinterpret_cast<const uint32_t*>(slab + at); }
// ProcessTile + Camera::GetPrimaryRay (renderer.cpp:125-126, camera.h:23-30) for pixel `pix` of tile (tx, ty): P - camPos, still to be normalised.
// right / down = topRight - topLeft / bottomLeft - topLeft
__device__ __forceinline__ f3 primary_target(f3 camPos, f3 TL, f3 right, f3 down, float invW, float invH, uint32_t tx, uint32_t ty, uint32_t pix, uint32_t& seed)
{
    const int x = (int)(tx * 16u + (pix & 15u)), y = (int)(ty * 16u + (pix >> 4));
    const float jy = rnd(seed);                                                  // pinned: first draw is the y jitter
    const float jx = rnd(seed);
    const float u = ((float)x + jx) * invW, vv = ((float)y + jy) * invH;
    const f3 P = TL + u * right + vv * down;
    return P - camPos;
}
// hit_light_floor's operands from the kernel-argument segment (the Scene is the kernel's first argument; dev_common.h scene_floats).  PRIM: with the sums a ray from
// the camera needs (Scene::primLight / primFloor)
template <bool PRIM>
__device__ __forceinline__ LightFloor light_floor_from_kernarg()
{
    const kernarg_f lp = scene_floats(offsetof(Scene, lightInvT));               // lightInvT[12] lightNrm[3] lightSize lightPos[3] floorN[3] floorD: one block of the Scene
    const kernarg_f ax = scene_floats(offsetof(Scene, lightAxis));               // lightAxis, floorAxisY
    LightFloor lf;
#pragma unroll
    for (int i = 0; i < 12; i++) lf.lightInvT[i] = lp[i];
    lf.lightSize = lp[15]; lf.floorN[0] = lp[19]; lf.floorN[1] = lp[20]; lf.floorN[2] = lp[21]; lf.floorD = lp[22];
    lf.lightAxis = asu(ax[0]); lf.floorAxisY = asu(ax[1]);
    lf.preOy = lf.preOx = lf.preOz = lf.preNum = 0.0f;
    if constexpr (PRIM) {
        constexpr size_t pl = (offsetof(Scene, primLight) - offsetof(Scene, lightInvT)) / 4;   // primLight[3], primFloor: the same Scene block, further on
        lf.preOy = lp[pl]; lf.preOx = lp[pl + 1]; lf.preOz = lp[pl + 2]; lf.preNum = lp[pl + 3];
    }
    return lf;
}

// ------------------------------------------------------------------------------------------------------------
// ordered two-child step (infra/bvh.cpp:244-257 / tlas_bvh.cpp:96-110): d1, d2 = the slab tests of children A and B (1e30f = missed)
// ------------------------------------------------------------------------------------------------------------
struct Ordered { uint32_t nearRef, farRef; bool hitN, push; };                   // descend into nearRef if hitN; the far child is pushed if `push`
__device__ __forceinline__ Ordered ordered_step(float d1, float d2, uint32_t refA, uint32_t refB)
{
    const bool sw = d1 > d2;                                                     // near child first (strict >: ties keep child A)
    const float dn = sw ? d2 : d1, df = sw ? d1 : d2;
    Ordered o;
    o.nearRef = sw ? refB : refA; o.farRef = sw ? refA : refB;
    o.hitN = dn != 1e30f; o.push = o.hitN && df != 1e30f;
    return o;
}

} // namespace crt
