// probe.hip — diagnostics: the fp32 building blocks of dev_common.h, one element per thread, for crt_debug_device_probe (abi.cpp; tests/test_gpu_device_probe.py).
// The render and query kernels' bit-exact parity rests on "only IEEE + - * / sqrt, so results are bit-identical with a scalar CPU evaluation of the same
// expressions" (dev_common.h); the renders check that sentence through whole paths, this unit checks each block by itself at the inputs where it can go wrong.
// It is a translation unit of its own, built with the library's flags: it compiles ITS OWN copy of the inline functions (the copies inlined into the render
// kernels are still checked by the renders), and the timed kernels' sources do not change.
//
// Straight-line code: plain loads and stores, no LDS, no traversal, no loop (the two 8-draw RNG sequences are unrolled).  Every input ends in a stored result;
// NaN, inf and zero operands are data.
//
// Record layouts (32-bit words; op numbers shared with abi.cpp's table and, for 11 .. 16, with the fp64 probe at the end of render_prim.hip):
//   op  name      in (words)                                          out (words)
//    0  EXPF      x                                              1    crt_expf(x)                                                        1
//    1  ACOSF     x                                              1    crt_acosf(x)                                                       1
//    2  ATAN2F    y, x                                           2    crt_atan2f(y, x)                                                   1
//    3  SQRTF     x                                              1    __builtin_sqrtf(x)                                                 1
//    4  DIVF      a, b                                           2    a / b                                                              1
//    5  VEC3      a.xyz, b.xyz                                   6    normalize3(a).xyz, cross3(a, b).xyz, dot3(a, b)                    7
//    6  RNG       base (u32)                                     1    init_seed(base) (u32), 8 x rnd, 8 x rnd_pm1, final state (u32)    18
//    7  TEX       u, v, w (i32), h (i32)                         4    tex_index(0, w, h, u, v) (u32)                                     1
//    8  SKY       D.xyz, w (i32), h (i32)                        5    phi, theta, tex_index(0, w, h, phi / 2pi, theta / pi) (u32)        3
//    9  BOX       lo.xyz, hi.xyz, O.xyz, rD.xyz, tray           13    box_exact, box_fast                                                2
//   10  TRI       v0.xyz, e1.xyz, e2.xyz, O.xyz, D.xyz, t_in    16    t, u, v, accepted (u32 0 / 1); a rejected record keeps t_in, 0, 0  4
//   11  ACOS64    x (double)                                     2    det_acos(x) (double)                                               2
//   12  COS64     x (double)                                     2    det_cos(x) (double)                                                2
//   13  CBRT64    x (double)                                     2    cbrt_fast(x) (double)                                              2
//   14  SQRT64    x (double)                                     2    __builtin_sqrt(x) (double)                                         2
//   15  DIV64     a, b (doubles)                                 4    a / b (double)                                                     2
//   16  F64TOF32  x (double)                                     2    (float)x                                                           1
//   17  SKYFAST   D.xyz, w (i32), h (i32)                        5    as op 8, through sky_angles: the guarded lookup as the render kernels call it  3
//
// probe_arith_kernel (crt_debug_arith_forms; tests/test_gpu_arith_forms.py): the short arithmetic forms of dev_common.h next to the forms they stand for, on the
// device, one record per thread; counted are the records whose two results differ in a bit (two NaNs count as equal), and a second launch writes the operands
// and both results of the lowest such record.  Records [0, nIn) are read from `in`; the records behind them are generated from (seed, index).
//   what  name   record (words)        old form                                         new form                                        generated records
//    0    PRED   tmin, tmax, tray  3   tmax >= tmin && tmin < tray && tmax > 0          slab_accept(tmin, tmax, tray_pred(tray)) where  any non-NaN tmin / tmax, any positive tray, three
//                                       ? tmin : 1e30f                                  tray_tame(tray) (per lane), else the old form   in four with tmax and / or tray next to tmin
//    1    DIV    a, b              2   a / b                                            div_guarded(a, b): div_short = div_by_rcp with  tame a and b: every exponent -40 .. 39, any mantissa
//                                                                                        rcp_nr(b), behind the tame-operand guard
//    2    SKY    D.xyz             3   crt_atan2f(-D.z, D.x) + pi, crt_acosf(-D.y)      sky_angles(D)                                   normalised random directions
//    3    DIV sweep:                   in = {b's sign and exponent bits, three numerators}; record i is (numerator i >> 23, b = bits | (i & 0x7fffff)), 3 * 2^23 records
#include "dev_common.h"
#include "launch.h"

namespace crt {

__global__ __launch_bounds__(256) void probe_f32_kernel(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    switch (op) {
    case 0: out[i] = asu(crt_expf(asf(in[i]))); break;
    case 1: out[i] = asu(crt_acosf(asf(in[i]))); break;
    case 2: out[i] = asu(crt_atan2f(asf(in[2 * (size_t)i]), asf(in[2 * (size_t)i + 1]))); break;
    case 3: out[i] = asu(__builtin_sqrtf(asf(in[i]))); break;
    case 4: out[i] = asu(asf(in[2 * (size_t)i]) / asf(in[2 * (size_t)i + 1])); break;
    case 5: {
        const uint32_t* p = in + 6 * (size_t)i; uint32_t* o = out + 7 * (size_t)i;
        const f3 a = mk3(asf(p[0]), asf(p[1]), asf(p[2])), b = mk3(asf(p[3]), asf(p[4]), asf(p[5]));
        const f3 nn = normalize3(a), cr = cross3(a, b);
        o[0] = asu(nn.x); o[1] = asu(nn.y); o[2] = asu(nn.z); o[3] = asu(cr.x); o[4] = asu(cr.y); o[5] = asu(cr.z); o[6] = asu(dot3(a, b));
        break;
    }
    case 6: {
        uint32_t* o = out + 18 * (size_t)i;
        uint32_t s = init_seed(in[i]);
        o[0] = s;
#pragma unroll
        for (int k = 0; k < 8; k++) o[1 + k] = asu(rnd(s));
#pragma unroll
        for (int k = 0; k < 8; k++) o[9 + k] = asu(rnd_pm1(s));
        o[17] = s;
        break;
    }
    case 7: {
        const uint32_t* p = in + 4 * (size_t)i;
        out[i] = tex_index(0u, (int)p[2], (int)p[3], asf(p[0]), asf(p[1]));
        break;
    }
    case 8: {   // sky_color's lookup (file_scene.cpp:142-154) up to the texel fetch
        const uint32_t* p = in + 5 * (size_t)i; uint32_t* o = out + 3 * (size_t)i;
        const f3 D = mk3(asf(p[0]), asf(p[1]), asf(p[2]));
        const float phi = crt_atan2f(-D.z, D.x) + CRT_PI;
        const float theta = crt_acosf(-D.y);
        o[0] = asu(phi); o[1] = asu(theta); o[2] = tex_index(0u, (int)p[3], (int)p[4], phi * CRT_INV2PI, theta * CRT_INVPI);
        break;
    }
    case 17: {  // the same lookup as the render kernels and the sky query make it: sky_angles' plain forms unless a lane of the wavefront holds a special operand
        const uint32_t* p = in + 5 * (size_t)i; uint32_t* o = out + 3 * (size_t)i;
        float phi, theta;
        sky_angles(mk3(asf(p[0]), asf(p[1]), asf(p[2])), phi, theta);
        o[0] = asu(phi); o[1] = asu(theta); o[2] = tex_index(0u, (int)p[3], (int)p[4], phi * CRT_INV2PI, theta * CRT_INVPI);
        break;
    }
    case 9: {
        const uint32_t* p = in + 13 * (size_t)i;
        rec4 lo, hi; lo.x = asf(p[0]); lo.y = asf(p[1]); lo.z = asf(p[2]); lo.w = 0.0f; hi.x = asf(p[3]); hi.y = asf(p[4]); hi.z = asf(p[5]); hi.w = 0.0f;
        const f3 O = mk3(asf(p[6]), asf(p[7]), asf(p[8])), rD = mk3(asf(p[9]), asf(p[10]), asf(p[11]));
        const float tray = asf(p[12]);
        out[2 * (size_t)i] = asu(box_exact(lo, hi, O, rD, tray)); out[2 * (size_t)i + 1] = asu(box_fast(lo, hi, O, rD, tray));
        break;
    }
    case 10: {
        const uint32_t* p = in + 16 * (size_t)i; uint32_t* o = out + 4 * (size_t)i;
        rec4 a, b, c;
        a.x = asf(p[0]); a.y = asf(p[1]); a.z = asf(p[2]); a.w = asf(7u);            // shadeIdx 7: the mark of an accepted hit
        b.x = asf(p[3]); b.y = asf(p[4]); b.z = asf(p[5]); b.w = asf(2u);
        c.x = asf(p[6]); c.y = asf(p[7]); c.z = asf(p[8]); c.w = asf(1u);
        const f3 O = mk3(asf(p[9]), asf(p[10]), asf(p[11])), D = mk3(asf(p[12]), asf(p[13]), asf(p[14]));
        Hit h; h.t = asf(p[15]); h.u = 0.0f; h.v = 0.0f; h.objIdx = -1; h.triIdx = -1;
        hit_tri(a, b, c, O, D, h);
        o[0] = asu(h.t); o[1] = asu(h.u); o[2] = asu(h.v); o[3] = (h.triIdx == 7) ? 1u : 0u;
        break;
    }
    default: break;
    }
}

__device__ __forceinline__ uint32_t probe_hash(uint32_t seed, uint32_t i, uint32_t k) { return wang_hash(wang_hash(i * 0x9e3779b9u + seed) + k * 0x85ebca6bu); }
__device__ __forceinline__ uint32_t probe_no_nan(uint32_t u) { return ((u & 0x7fffffffu) > 0x7f800000u) ? (u & 0xff800000u) : u; }     // a NaN becomes the infinity of its sign
__device__ __forceinline__ uint32_t probe_tame(uint32_t h) { return (h & 0x807fffffu) | ((87u + ((h >> 23) & 0xffu) % 80u) << 23); }     // 2^-40 <= |x| < 2^40
__device__ __forceinline__ bool probe_same(float a, float b) { return asu(a) == asu(b) || (a != a && b != b); }

__global__ __launch_bounds__(256) void probe_arith_kernel(int what, const uint32_t* __restrict__ in, uint32_t nIn, uint32_t n, uint32_t seed, uint32_t dumpAt, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = i - nIn;                                                  // index among the generated records
    uint32_t op[3] = {0u, 0u, 0u};
    float was[2] = {0.0f, 0.0f}, is[2] = {0.0f, 0.0f};
    switch (what) {
    case 0: {
        if (i < nIn) { op[0] = in[3 * (size_t)i]; op[1] = in[3 * (size_t)i + 1]; op[2] = in[3 * (size_t)i + 2]; }
        else {
            op[0] = probe_no_nan(probe_hash(seed, j, 1u)); op[1] = probe_no_nan(probe_hash(seed, j, 2u)); op[2] = probe_no_nan(probe_hash(seed, j, 3u)) & 0x7fffffffu;
            if (j & 1u) op[1] = probe_no_nan(op[0] + probe_hash(seed, j, 4u) % 5u - 2u);
            if (j & 2u) op[2] = probe_no_nan((op[0] & 0x7fffffffu) + probe_hash(seed, j, 5u) % 5u - 2u) & 0x7fffffffu;
        }
        const float tmin = asf(op[0]), tmax = asf(op[1]), tray = asf(op[2]);
        was[0] = (tmax >= tmin && tmin < tray && tmax > 0) ? tmin : 1e30f;
        is[0] = tray_tame(tray) ? slab_accept(tmin, tmax, tray_pred(tray)) : was[0];
        break;
    }
    case 1: case 3: {
        if (what == 3) { op[0] = in[1u + (i >> 23)]; op[1] = in[0] | (i & 0x7fffffu); }
        else if (i < nIn) { op[0] = in[2 * (size_t)i]; op[1] = in[2 * (size_t)i + 1]; }
        else { op[0] = probe_tame(probe_hash(seed, j, 1u)); op[1] = probe_tame(probe_hash(seed, j, 2u)); }
        const float a = asf(op[0]), b = asf(op[1]);
        was[0] = a / b;
        is[0] = div_guarded(a, b);
        break;
    }
    case 2: {
        f3 D;
        if (i < nIn) D = mk3(asf(in[3 * (size_t)i]), asf(in[3 * (size_t)i + 1]), asf(in[3 * (size_t)i + 2]));
        else {
            uint32_t s0 = probe_hash(seed, j, 1u) | 1u;
            const float x = rnd_pm1(s0), y = rnd_pm1(s0), z = rnd_pm1(s0);
            D = normalize3(mk3(x, y, z));
        }
        op[0] = asu(D.x); op[1] = asu(D.y); op[2] = asu(D.z);
        was[0] = crt_atan2f(-D.z, D.x) + CRT_PI; was[1] = crt_acosf(-D.y);
        sky_angles(D, is[0], is[1]);
        break;
    }
    default: break;
    }
    if (!probe_same(was[0], is[0]) || !probe_same(was[1], is[1])) { atomicAdd(&out[0], 1u); atomicMin(&out[1], i); }
    if (i == dumpAt) { out[2] = op[0]; out[3] = op[1]; out[4] = op[2]; out[5] = asu(was[0]); out[6] = asu(was[1]); out[7] = asu(is[0]); out[8] = asu(is[1]); }
}

} // namespace crt

// out: 9 words {differing records, the lowest of them, its operands [3], old result [2], new result [2]}; out[0] = 0 and out[1] = 0xffffffff before the first launch
extern "C" hipError_t crt_launch_probe_arith(int what, const void* in, uint32_t nIn, uint32_t n, uint32_t seed, uint32_t dumpAt, void* out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (what < 0 || what > 3 || nIn > n || (what == 3 && (n != 3u << 23 || nIn != 0u || !in)) || (nIn && !in)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::probe_arith_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, what, (const uint32_t*)in, nIn, n, seed, dumpAt, (uint32_t*)out);
    return hipGetLastError();
}

extern "C" hipError_t crt_launch_probe_f32(int op, const void* in, void* out, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if ((op < 0 || op > 10) && op != 17) return hipErrorInvalidValue;
    hipLaunchKernelGGL(crt::probe_f32_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, op, (const uint32_t*)in, (uint32_t*)out, n);
    return hipGetLastError();
}
