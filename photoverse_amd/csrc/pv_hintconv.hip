// pv_hint_conv3x3: the small-channel 3x3 convs of a ControlNet's conditioning ("hint") embedding - 3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 channels on a
// 512 x 512 control image, three of them stride 2.  pv_gemm_conv takes none of these shapes (cin % 64, N % 128 / 160); padding them would move 4 - 20 x
// the bytes.  Two kernels, both direct convs (no im2col buffer, no LDS), fp32 accumulation, fp16 rows out:
//   hint_conv_image_kernel  fp32 NCHW input with cin <= 4 (K = 9 cin <= 36: too short for a matrix instruction): one output pixel per thread, plain
//                           vector FMAs, the weights read at wave-uniform addresses;
//   hint_conv_rows_kernel   fp16 rows input, cin % 8 == 0: implicit GEMM on v_mfma_f32_16x16x32_f16 over the flat contraction k = tap * cin + c (the
//                           order of the weight rows).  Eight consecutive k lie in one tap (cin % 8 == 0), so every lane's operand is ONE 16-byte load of
//                           the input row (zero where the tap falls on the padding or k >= 9 cin - the last 32-deep step of K = 144 is half empty) and
//                           one of the weight row.  Operands are passed swapped (weights as MFMA-A, pixels as MFMA-B), so a lane ends up with four
//                           consecutive output channels of one pixel: one 8-byte store.  A wave owns 64 pixels x up to 64 channels (4 x 4 accumulator
//                           tiles: every weight fragment feeds four MFMAs, every pixel fragment four); a workgroup is four such waves.
#include "pv_common.h"

#define HC_PIX_FRAGS 4          // 16-pixel fragments per wave
#define HC_CO_FRAGS 4           // 16-channel fragments per wave
#define HC_WAVES 4

__global__ __launch_bounds__(256) void hint_conv_image_kernel(const float* __restrict__ x, const half_t* __restrict__ w, const float* __restrict__ bias,
                                                              half_t* __restrict__ out, int ldo, int batch, int cin, int cout, int h, int wd, int ho,
                                                              int wo, int stride, int act) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long M = (long long)batch * ho * wo;
    if (m >= M) return;
    const int ox = (int)(m % wo), oy = (int)((m / wo) % ho), b = (int)(m / ((long long)wo * ho));
    float in[36];                               // [tap][ci], zero on the padding
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = oy * stride + t / 3 - 1, ix = ox * stride + t % 3 - 1;
        const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < wd;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            in[t * 4 + ci] = (ok && ci < cin) ? x[(((size_t)b * cin + ci) * h + iy) * wd + ix] : 0.f;
    }
    const int K = 9 * cin;
    for (int c0 = 0; c0 < cout; c0 += 8) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bias[c0 + j];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
                if (ci < cin) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(in[t * 4 + ci], (float)w[(size_t)(c0 + j) * K + t * cin + ci], acc[j]);
                }
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(act == PV_ACT_SILU ? pv_silu(acc[j]) : acc[j]);
        *(half8_t*)(out + (size_t)m * ldo + c0) = o;
    }
}

__global__ __launch_bounds__(256) void hint_conv_rows_kernel(const half_t* __restrict__ x, int ldx, const half_t* __restrict__ w,
                                                             const float* __restrict__ bias, half_t* __restrict__ out, int ldo, int batch, int cin,
                                                             int cout, int h, int wd, int ho, int wo, int stride, int act) {
    const int lane = pv_lane_id(), wave = pv_wave_id();
    const int r16 = lane & 15, g = lane >> 4;
    const long long M = (long long)batch * ho * wo;
    const long long m0 = ((long long)blockIdx.x * HC_WAVES + wave) * (16 * HC_PIX_FRAGS);
    const int n0 = blockIdx.y * (16 * HC_CO_FRAGS);
    const int K = 9 * cin;
    if (m0 >= M) return;                         // wave-uniform

    // this lane's pixel of every pixel fragment: the row of its image (-1: past the end) and the top-left input coordinate of its 3x3 window
    int iy0[HC_PIX_FRAGS], ix0[HC_PIX_FRAGS];
    long long base[HC_PIX_FRAGS];
#pragma unroll
    for (int p = 0; p < HC_PIX_FRAGS; ++p) {
        const long long m = m0 + p * 16 + r16;
        if (m < M) {
            const int ox = (int)(m % wo), oy = (int)((m / wo) % ho);
            base[p] = (m / ((long long)wo * ho)) * h * wd;
            iy0[p] = oy * stride - 1;
            ix0[p] = ox * stride - 1;
        } else {
            base[p] = -1;
            iy0[p] = ix0[p] = 0;
        }
    }
    float4_t acc[HC_CO_FRAGS][HC_PIX_FRAGS];
#pragma unroll
    for (int f = 0; f < HC_CO_FRAGS; ++f)
#pragma unroll
        for (int p = 0; p < HC_PIX_FRAGS; ++p) acc[f][p] = (float4_t){0.f, 0.f, 0.f, 0.f};

    int tap = 0, c = 8 * g;                      // k = 32 step + 8 g as (tap, channel)
    while (c >= cin) { c -= cin; ++tap; }
    for (int k0 = 8 * g; k0 - 8 * g < K; k0 += 32) {
        const bool kin = k0 < K;
        const int ky = tap / 3, kx = tap - 3 * ky;
        half8_t wa[HC_CO_FRAGS], xb[HC_PIX_FRAGS];
#pragma unroll
        for (int f = 0; f < HC_CO_FRAGS; ++f) {
            wa[f] = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
            if (kin && n0 + f * 16 < cout) wa[f] = *(const half8_t*)(w + (size_t)(n0 + f * 16 + r16) * K + k0);
        }
#pragma unroll
        for (int p = 0; p < HC_PIX_FRAGS; ++p) {
            const int iy = iy0[p] + ky, ix = ix0[p] + kx;
            xb[p] = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
            if (kin && base[p] >= 0 && iy >= 0 && iy < h && ix >= 0 && ix < wd)
                xb[p] = *(const half8_t*)(x + (size_t)(base[p] + (long long)iy * wd + ix) * ldx + c);
        }
#pragma unroll
        for (int f = 0; f < HC_CO_FRAGS; ++f)
            if (n0 + f * 16 < cout) {            // wave-uniform
#pragma unroll
                for (int p = 0; p < HC_PIX_FRAGS; ++p) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[f], xb[p], acc[f][p], 0, 0, 0);
            }
        c += 32;
        while (c >= cin) { c -= cin; ++tap; }
    }
    // D[channel = 4 g + r][pixel = lane & 15]: four consecutive channels of one pixel per lane
#pragma unroll
    for (int f = 0; f < HC_CO_FRAGS; ++f) {
        const int co = n0 + f * 16 + 4 * g;
        if (n0 + f * 16 >= cout) continue;
        const float4_t bv = *(const float4_t*)(bias + co);
#pragma unroll
        for (int p = 0; p < HC_PIX_FRAGS; ++p) {
            const long long m = m0 + p * 16 + r16;
            if (m >= M) continue;
            half4_t o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[f][p][r] + bv[r];
                o[r] = (half_t)(act == PV_ACT_SILU ? pv_silu(v) : v);
            }
            *(half4_t*)(out + (size_t)m * ldo + co) = o;
        }
    }
}

extern "C" int32_t pv_hint_conv3x3(const void* x, int32_t x_is_image, int32_t ldx, const void* w, const float* bias, void* out, int32_t ldo, int32_t batch,
                               int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t stride, int32_t act, void* stream) {
    if (!x || !w || !bias || !out) return (int)hipErrorInvalidValue;
    if (batch < 1 || h < 1 || wd < 1 || cin < 1 || cout < 1) return (int)hipErrorInvalidValue;
    if (stride != 1 && stride != 2) return (int)hipErrorInvalidValue;
    if (act != PV_ACT_NONE && act != PV_ACT_SILU) return (int)hipErrorInvalidValue;
    if (x_is_image != 0 && x_is_image != 1) return (int)hipErrorInvalidValue;
    if (cout % 16 || cout > 256) return (int)hipErrorInvalidValue;
    if (x_is_image ? cin > 4 : (cin % 8 != 0 || cin > 256)) return (int)hipErrorInvalidValue;
    if (ldo < cout || ldo % 8 || (!x_is_image && (ldx < cin || ldx % 8))) return (int)hipErrorInvalidValue;
    if (((uintptr_t)out | (uintptr_t)w | (uintptr_t)bias | (x_is_image ? 0 : (uintptr_t)x)) & 15) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 3)) return (int)hipErrorInvalidValue;
    const int ho = (h - 1) / stride + 1, wo = (wd - 1) / stride + 1;
    const unsigned long long lim = 1ull << 31;
    // every factor is below 2^31, so no product of two of them overflows 64 bits; the running product is checked after every step
    unsigned long long in_el = (unsigned long long)batch * (unsigned long long)h;
    if (in_el >= lim) return (int)hipErrorInvalidValue;
    in_el *= (unsigned long long)wd;
    if (in_el >= lim) return (int)hipErrorInvalidValue;
    const unsigned long long in_bytes = in_el * (x_is_image ? 4ull * cin : 2ull * ldx);
    unsigned long long out_el = (unsigned long long)batch * (unsigned long long)ho;
    if (out_el >= lim) return (int)hipErrorInvalidValue;
    out_el *= (unsigned long long)wo;
    if (out_el >= lim) return (int)hipErrorInvalidValue;
    const unsigned long long out_bytes = out_el * 2ull * ldo;
    if (in_bytes >= lim || out_bytes >= lim) return (int)hipErrorInvalidValue;
    const long long M = (long long)out_el;
    hipStream_t s = (hipStream_t)stream;
    if (x_is_image) {
        hint_conv_image_kernel<<<dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s>>>((const float*)x, (const half_t*)w, bias, (half_t*)out, ldo, batch, cin,
                                                                                      cout, h, wd, ho, wo, stride, act);
    } else {
        const int per_wg = 16 * HC_PIX_FRAGS * HC_WAVES;
        hint_conv_rows_kernel<<<dim3((unsigned)((M + per_wg - 1) / per_wg), (unsigned)((cout + 16 * HC_CO_FRAGS - 1) / (16 * HC_CO_FRAGS))), dim3(256), 0, s>>>(
            (const half_t*)x, ldx, (const half_t*)w, bias, (half_t*)out, ldo, batch, cin, cout, h, wd, ho, wo, stride, act);
    }
    return PV_CHECK_LAUNCH();
}
