// render_sky.hip — render_sky_kernel: the tiles of a job whose class is kTileSky (tile_class.h: no primary ray of the tile passes the light quad's, the floor
// plane's or the root pair's test), in straight-line code beside the job's render_pool_kernel launch.
//
// Every path of such a tile is Renderer::Sample's first return (renderer.cpp:52-55): two RNG draws, the primary ray, its normalisation, GetSkyColor's one texel.
// The pool carries these streams through its machinery all the same — parked in LDS, queued on the END ring, popped by a pass at 53 of 64 lanes inside a trip —
// and its sample store scatters 12 bytes into 768-byte pixel rows.  Here a lane IS a stream: lane l renders frame l of a 64-frame window and walks the tile's 256
// pixels in registers.  No LDS, no queue, no trip, 64 of 64 lanes, and the 64 lanes' texels of one (pixel, pass) are 256 contiguous bytes of the slab.
//
// Which slab position and which RNG stream belong to a (tile, frame) is the pool kernel's definition (sample_body.h stream_seed / slab_position), and every step
// of the path is the function the pool kernel's END pass calls: the accumulator cannot tell which of the two kernels rendered a tile.
#include "launch.h"
#include "sample_body.h"

namespace crt {

// block -> (sky rank, 64-frame window), rank-major; the sky tiles are the ranks [rankFirst, rankFirst + skyTiles) of the tile order (abi.cpp: its tail)
// texels (the same for the whole launch): the tiles' blocks take the texel form — the sample IS tex_unpack(texel), and the launch's accumulate unpacks it — else
// the 12-byte sample form (sample_body.h)
__global__ __launch_bounds__(64) void render_sky_kernel(const Scene sc, char* __restrict__ slab, Counters* __restrict__ counters, const uint32_t* __restrict__ tileOrder,
                                                        uint32_t rankFirst, uint32_t skyTiles, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX,
                                                        uint32_t sppFirst, uint32_t frames, uint32_t passes, uint32_t groups, uint32_t texels, unsigned long long* __restrict__ launchClk)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t r = blockIdx.x / groups, grp = blockIdx.x - r * groups;
    if (r >= skyTiles) return;
    // a measuring job (abi.cpp adopt_job_costs): ~(first wavefront's start), last wavefront's end — the launch's span on the device
    const unsigned long long clk0 = launchClk ? wall_clock64() : 0ull;
    const uint32_t tl = tileOrder[rankFirst + r];
    const uint32_t tile = tileFirst + tl * tileStride;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    const uint32_t fr = grp * 64u + lane;                                        // frame of the launch
    const uint32_t items = 256u * passes, rowLen = 64u * passes;
    uint32_t paths = 0;
    if (fr < frames) {                                                           // (lanes past `frames` in the last window do nothing)
        uint32_t seed = stream_seed(tx, ty, (uint32_t)sc.W, sppFirst, fr, passes);
        const f3 camPos = mk3(sc.camPos[0], sc.camPos[1], sc.camPos[2]), TL = mk3(sc.topLeft[0], sc.topLeft[1], sc.topLeft[2]);
        const f3 right = mk3(sc.primRight[0], sc.primRight[1], sc.primRight[2]), down = mk3(sc.primDown[0], sc.primDown[1], sc.primDown[2]);
        uint32_t pix = 0, pass = 0;
#pragma unroll 4
        for (uint32_t item = 0; item < items; item++) {                          // (pixel, pass) pairs in stream order
            const f3 v = primary_target(camPos, TL, right, down, sc.invW, sc.invH, tx, ty, pix, seed);
            const f3 D = v * rcp_exact(sqrt_exact(dot3(v, v)));                  // normalize()
            float phi, theta; sky_angles(D, phi, theta);                         // GetSkyColor (file_scene.cpp:142-154)
            const uint32_t texel = sc.texels[tex_index(sc.skyOffset, sc.skyW, sc.skyH, phi * CRT_INV2PI, theta * CRT_INVPI)];
            if (texels) store_texel(slab, slab_texel_position(fr, tileCount, tl, pix, rowLen, passes, pass), texel);
            else store_sample(slab, slab_position(fr, tileCount, tl, pix, rowLen, passes, pass), tex_unpack(texel));
            if (++pass == passes) { pass = 0; pix++; }
        }
        paths = items;
    }
    const uint32_t sum = wave_sum(paths);                                        // one ray and one primary ray per path, as the pool counts them
    if (lane == 0 && sum) { atomicAdd(&counters->v[0], (unsigned long long)sum); atomicAdd(&counters->v[1], (unsigned long long)sum); }
    if (launchClk && lane == 0) { atomicMax(&launchClk[0], ~clk0); atomicMax(&launchClk[1], wall_clock64()); }
}

} // namespace crt

extern "C" hipError_t crt_launch_render_sky(const crt::Scene* sc, void* slab, crt::Counters* counters, const uint32_t* tileOrder, uint32_t rankFirst, uint32_t skyTiles,
                                            uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint32_t tilesX, uint32_t sppFirst, uint32_t frames, uint32_t passes,
                                            int texels, unsigned long long* launchClk, hipStream_t stream)
{
    if (skyTiles == 0 || frames == 0) return hipSuccess;
    if (!tileOrder || rankFirst > tileCount || skyTiles > tileCount - rankFirst || passes == 0) return hipErrorInvalidValue;
    const uint32_t groups = (frames + 63u) / 64u;
    if ((unsigned long long)skyTiles * groups > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::render_sky_kernel, dim3(skyTiles * groups), dim3(64), 0, stream, *sc, (char*)slab, counters, tileOrder, rankFirst, skyTiles, tileFirst, tileStride,
                       tileCount, tilesX, sppFirst, frames, passes, groups, texels ? 1u : 0u, launchClk);
    return hipGetLastError();
}
