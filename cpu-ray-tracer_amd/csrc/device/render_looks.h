// render_looks.h — crt_render_looks: the frames of many cameras over many LOOKS of the live scene in one job.  render_views_kernel (render_views.h) with one
// difference: what a lane shades with is not the launch's Scene block and the live Material table but the look of the lane's view.  A look is a block of the look
// table (look_build.hip; layout.h LookDev): the light quad, the floor material and the sky words, then the look's Material records in Scene::mats' order.  The
// geometry — BVH / TLAS, triangles, ShadeTri records, the floor plane — is the live scene's for every look and stays where it is, in Scene::geom.
//
//   LookWorld<KIND>   trace:   hit_light_floor (dev_common.h) on a LightFloor filled from the lane's look, in the GENERAL quad form (lightAxis 0: the short form is
//                              bit-identical to it, tests/test_gpu_parity.py test_general_code_paths_are_bit_identical), the floor half as the live scene's;
//                              then traverse_bvh_seq / tlas_walk over Scene::geom — find_nearest_seq's order, the functions it calls;
//                     surface: FileSurface<KIND>'s steps (floor_point / mesh_point / face_ray / tex_sample) with the floor's and the mesh's Material read from the look;
//                     miss:    sky_color's lookup with the look's sky words.
//
// Addressing: as PoseWorld's (render_poses.h) — the table is one allocation of at most kMaxGeomBytes, so a lane names its look by ONE 32-bit byte offset and every
// load is scalar base + per-lane offset.  LDS: the live scene's stack depth; a look changes no tree.
//
// Numerics: seq_sample.h's (-ffp-contract=off, IEEE + - * / sqrt).  No MFMA.
#pragma once
#include "file_surface.h"
#include "render_views.h"

namespace crt {

constexpr uint32_t kLookFloorMat = 64u, kLookSky = 96u, kLookMats = 128u;        // LookDev::floorMat, ::skyOffset; the Material records behind the LookDev
static_assert(offsetof(LookDev, floorMat) == kLookFloorMat && offsetof(LookDev, skyOffset) == kLookSky && sizeof(LookDev) == kLookMats && offsetof(LookDev, lightSize) == 60, "LookDev");

template <int KIND>
struct LookWorld : FileSurface<KIND> {
    const char* table;                    // the look table (wave-uniform)
    uint32_t look;                        // this lane's look: its LookDev's offset in the table
    __device__ __host__ uint32_t stack_words(const Scene& sc) const { return sc.stackDepth; }
    __device__ __forceinline__ uint32_t trace(const Scene& sc, f3 O, f3 D, f3 rD, Hit& h, uint32_t* stk) const
    {
        Cnt cn; cn.rays = cn.primary = cn.interior = cn.leaf = cn.tri = cn.tlas = cn.visits = cn.meshhits = 0;
        int traversed = 0, tested = 0;
        {
            const rec4 r0 = ldp<0>(table, look), r1 = ldp<1>(table, look), r2 = ldp<2>(table, look), r3 = ldp<3>(table, look);   // lightInvT rows 0..2; lightNrm, lightSize
            LightFloor lf;
            lf.lightInvT[0] = r0.x; lf.lightInvT[1] = r0.y; lf.lightInvT[2] = r0.z; lf.lightInvT[3] = r0.w;
            lf.lightInvT[4] = r1.x; lf.lightInvT[5] = r1.y; lf.lightInvT[6] = r1.z; lf.lightInvT[7] = r1.w;
            lf.lightInvT[8] = r2.x; lf.lightInvT[9] = r2.y; lf.lightInvT[10] = r2.z; lf.lightInvT[11] = r2.w;
            lf.lightSize = r3.w; lf.lightAxis = 0u; lf.floorAxisY = sc.floorAxisY;
            lf.floorN[0] = sc.floorN[0]; lf.floorN[1] = sc.floorN[1]; lf.floorN[2] = sc.floorN[2]; lf.floorD = sc.floorD;
            lf.preOy = lf.preOx = lf.preOz = lf.preNum = 0.0f;
            hit_light_floor(lf, O, D, h);
        }
        if (KIND == 0) traverse_bvh_seq(sc, sc.rootRef, O, D, rD, h, stk, cn, traversed, tested);
        else {
            // TLAS entries live above the BVH part of this lane's column, as in find_nearest_seq
            tlas_walk(sc, O, D, rD, h, stk + sc.bvhStack * 64, cn, traversed, [&](uint32_t, rec4 ids, f3 Oo, f3 Do, f3 rDo) __attribute__((always_inline)) {
                traverse_bvh_seq(sc, asu(ids.z), Oo, Do, rDo, h, stk, cn, traversed, tested);
            });
        }
        return 0u;
    }
    // FileSurface<KIND>::surface_of with the two Material fetches redirected: the floor's is the look's floorMat, a triangle's is record ShadeTri::mat of the look's table
    __device__ __forceinline__ Surf surface(const Scene& sc, const Hit& h, f3 I, f3 D) const
    {
        const char* __restrict__ geom = sc.geom;
        SurfPoint p;
        if (h.objIdx == 1) p = floor_point(mk3(sc.floorN[0], sc.floorN[1], sc.floorN[2]), sc.floorInvto, ldg(table, look + kLookFloorMat), ldg(table, look + kLookFloorMat + 16u), I);
        else {
            const uint32_t so = sc.shadeOff + (uint32_t)h.triIdx * 64u;
            const rec4 s0 = ldg(geom, so), s1 = ldg(geom, so + 16u), s2 = ldg(geom, so + 32u), s3 = ldg(geom, so + 48u);
            p = mesh_point_with<KIND>(s0, s1, s2, s3, h.u, h.v, h.objIdx, geom, sc.instOff, [&](int mat, rec4& m0, rec4& m1) __attribute__((always_inline)) {
                const uint32_t mo = look + kLookMats + (uint32_t)mat * (uint32_t)sizeof(Material);
                m0 = ldg(table, mo); m1 = ldg(table, mo + 16u);
            });
        }
        Surf s; s.N = face_ray(p.N, D); s.refl = p.refl; s.refr = p.refr; s.absorb = p.absorb;
        s.c = mk3(1.0f, 1.0f, 1.0f);
        if (p.tW > 0) s.c = tex_sample(sc, p.tOff, p.tW, p.tH, p.tu, p.tv);   // Material::GetAlbedo
        return s;
    }
    // GetSkyColor (sky_color, dev_common.h) with the look's skydome
    __device__ __forceinline__ f3 miss(const Scene& sc, f3 D) const
    {
        const rec4 sky = ldg(table, look + kLookSky);
        float phi, theta;
        sky_angles(D, phi, theta);
        return tex_sample(sc, asu(sky.x), (int)asu(sky.y), (int)asu(sky.z), phi * CRT_INV2PI, theta * CRT_INVPI);
    }
};

// the look of `view`: an index the build launch has found to lie in [0, L) before this kernel is launched
template <int KIND>
__device__ __forceinline__ LookWorld<KIND> look_world(const LookTableDev& lt, uint32_t view)
{
    const uint32_t l = lt.viewLook ? (uint32_t)lt.viewLook[view] : view;
    LookWorld<KIND> w;
    w.table = lt.table; w.look = lt.looksOff + l * lt.lookStride;
    return w;
}

// render_views_kernel's launch shape, slab, seeds and camera handling (render_views.h: entry = tile rank * windows + window, lane = view-frame, the camera read again
// per pixel); the path itself is sample_step / sample_unwind over the lane's LookWorld.
template <int KIND>
__global__ __launch_bounds__(256, 4) void render_looks_kernel(const Scene sc, const LookTableDev lt, const float* __restrict__ cams, char* __restrict__ slab,
                                                             Counters* __restrict__ counters, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                             uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t jFirst, uint32_t nj, uint32_t nEntries)
{
    extern __shared__ uint32_t ldsAll[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t entry = blockIdx.x * kSeqWaves + wave;
    if (entry >= nEntries) return;
    const uint32_t windows = (nj + 63u) / 64u;
    const uint32_t tl = entry / windows, win = entry % windows;
    if (tl >= tileCount) return;
    const uint32_t jl = win * 64u + lane;                                         // view-frame of the launch
    if (jl >= nj) return;
    const uint32_t j = jFirst + jl, view = j / frames, frame = j - view * frames;
    slab += slab_block_position(win, tileCount, tl, 64u * passes);                // this tile's block of this window's region of the sample slab
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    const LookWorld<KIND> world = look_world<KIND>(lt, view);
    // this lane's LDS columns: the traversal stack, then the throughput factors
    const uint32_t stackWords = world.stack_words(sc);
    uint32_t* stk = ldsAll + wave * (stackWords + 15u) * 64u + lane;
    float* fst = reinterpret_cast<float*>(stk + stackWords * 64u);

    uint32_t nRays = 0, nPrimary = 0, nMesh = 0, steps = 0;
    const uint32_t items = 256u * passes;                                         // (pixel, pass) pairs in stream order
    uint32_t seed = stream_seed(tx, ty, (uint32_t)sc.W, sppFirst, frame, passes); // renderer.cpp:120
    const float* __restrict__ cam = cams + (size_t)view * 12u;                    // camPos, topLeft, topRight, bottomLeft
    const kernarg_f inv = scene_floats(offsetof(Scene, invW));
    const float invW = inv[0], invH = inv[1];

    for (uint32_t item = 0; item < items; item++) {
        const uint32_t pix = (passes == 1u) ? item : item / passes;
        const f3 camPos = mk3(cam[0], cam[1], cam[2]);
        const f3 TL = mk3(cam[3], cam[4], cam[5]), TR = mk3(cam[6], cam[7], cam[8]), BL = mk3(cam[9], cam[10], cam[11]);
        const f3 v = primary_target(camPos, TL, TR - TL, BL - TL, invW, invH, tx, ty, pix, seed);
        f3 O = camPos, D = v * rcp_exact(sqrt_exact(dot3(v, v)));                 // normalize()
        bool inside = false; int depth = 0;
        nPrimary++;
        f3 L = mk3(0, 0, 0);
        while (!sample_step<LookWorld<KIND>, false>(sc, world, stk, fst, O, D, inside, depth, seed, L, nRays, nMesh, steps)) {}
        sample_unwind(fst, depth, L);
        uint32_t pass = 0;
        if (passes != 1u) pass = item - pix * passes;
        store_sample(slab, slab_sample_offset(lane, pix, 64u * passes, passes, pass), L);
    }
    atomicAdd(&counters->v[0], (unsigned long long)nRays);
    atomicAdd(&counters->v[1], (unsigned long long)nPrimary);
    if (nMesh) atomicAdd(&counters->v[7], (unsigned long long)nMesh);
}

} // namespace crt
