// look_build.hip — crt_render_looks' build launch: the job's L look records (crt_abi.h: crt_look_header, then materialCount crt_material records, all 4-byte words)
// become the look table the render kernel reads (layout.h LookJobHeader, LookDev): per look one light / floor-material / sky block and the look's device Material
// records, every texture index bound through the uploaded texture table as crt_upload_scene binds it.
//
//   look_build_kernel   lane t of L * (M + 1): look t / (M + 1); item t % (M + 1) = a material, or (item M) the look's header.  Lanes below K also check view_look.
//
// Every texture index is checked before it is used as an address; a lane that finds one out of range writes an untextured record and reports (look, field) with a
// 64-bit atomicMin, so the header names the lowest look and in it the first field however the lanes are scheduled.  The host reads the header back and does not run
// the job unless it is clean.  No float arithmetic but the three negations of lightNrm (Quad::GetNormal, primitives.h:363-367).
#include "dev_common.h"
#include "launch.h"

namespace crt {

// a texture index as crt_upload_scene's bindTex leaves it in a Material; t < 0: untextured
__device__ __forceinline__ void bind_tex(Material& m, const TexDesc* __restrict__ tex, int32_t t)
{
    if (t < 0) { m.texOffset = 0; m.texW = 0; m.texH = 0; }
    else { const TexDesc d = tex[t]; m.texOffset = d.offset; m.texW = d.w; m.texH = d.h; }
}

__global__ __launch_bounds__(256) void look_build_kernel(const LookBuildDev b)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    LookJobHeader* head = reinterpret_cast<LookJobHeader*>(b.table);
    if (b.viewLook && t < b.K) {
        const int32_t l = b.viewLook[t];
        if (l < 0 || (uint32_t)l >= b.L) atomicMin(&head->badView, t);
    }
    const uint32_t per = b.M + 1u;
    if (t >= b.L * per) return;
    const uint32_t look = t / per, item = t - look * per;
    const uint32_t* __restrict__ rec = b.looks + (size_t)look * (kLookHeaderWords + b.M * kLookMaterialWords);
    char* block = b.table + b.looksOff + (size_t)look * b.lookStride;
    Material* mats = reinterpret_cast<Material*>(block + sizeof(LookDev));
    auto bad = [&](uint32_t field) { atomicMin(&head->badField, ((unsigned long long)look << 32) | field); };
    if (item < b.M) {
        const uint32_t* __restrict__ m = rec + kLookHeaderWords + item * kLookMaterialWords;
        Material out;
        out.reflectivity = __uint_as_float(m[0]); out.refractivity = __uint_as_float(m[1]);
        out.absorption[0] = __uint_as_float(m[2]); out.absorption[1] = __uint_as_float(m[3]); out.absorption[2] = __uint_as_float(m[4]);
        int32_t tex = (int32_t)m[5];
        if (tex < -1 || tex >= (int32_t)b.texCount) { bad(kLookFieldMaterial + item); tex = -1; }
        bind_tex(out, b.tex, tex);
        mats[2u + item] = out;
        return;
    }
    // the look's header: lightT[16], lightInvT[16], lightSize, floorTexture, skyTexture, pad
    LookDev d;
#pragma unroll
    for (int i = 0; i < 12; i++) d.lightInvT[i] = __uint_as_float(rec[16 + i]);
    d.lightNrm[0] = -__uint_as_float(rec[1]); d.lightNrm[1] = -__uint_as_float(rec[5]); d.lightNrm[2] = -__uint_as_float(rec[9]);
    d.lightSize = __uint_as_float(rec[32]);
    int32_t floorTex = (int32_t)rec[33], skyTex = (int32_t)rec[34];
    if (floorTex < 0 || floorTex >= (int32_t)b.texCount) { bad(kLookFieldFloor); floorTex = -1; }
    if (skyTex < 0 || skyTex >= (int32_t)b.texCount) { bad(kLookFieldSky); skyTex = -1; }
    Material zero;
    zero.reflectivity = zero.refractivity = 0.0f; zero.absorption[0] = zero.absorption[1] = zero.absorption[2] = 0.0f;
    bind_tex(zero, b.tex, -1);
    d.floorMat = zero; bind_tex(d.floorMat, b.tex, floorTex);
    Material sky = zero; bind_tex(sky, b.tex, skyTex);
    d.skyOffset = sky.texOffset; d.skyW = sky.texW; d.skyH = sky.texH;
#pragma unroll
    for (int i = 0; i < 5; i++) d.pad[i] = 0u;
    *reinterpret_cast<LookDev*>(block) = d;
    mats[0] = zero;                                                               // [0] the light, [1] the floor: Scene::mats' order
    mats[1] = d.floorMat;
}

} // namespace crt

// the caller sets the LookJobHeader to all ones on the stream first (kPoseNoBadView, kLookNoBadField)
extern "C" hipError_t crt_launch_look_build(const crt::LookBuildDev* b, hipStream_t stream)
{
    const unsigned long long lanes = (unsigned long long)b->L * (b->M + 1u);
    const unsigned long long n = lanes > b->K ? lanes : b->K;
    if (n == 0) return hipSuccess;
    if (n > 0x7fffffffull || !b->tex || !b->table) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::look_build_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, *b);
    return hipGetLastError();
}
