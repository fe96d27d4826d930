// pv_tiny_conv3x3: the 3x3 convs of AutoencoderTiny (TAESD) - 19 per direction, all at width 64 except the first (<= 4 image channels in) and the last
// (<= 4 image channels out).  pv_gemm_conv takes none of these shapes (N tiles of 128 / 160); pv_hint_conv3x3 re-reads the whole weight per wave.
//
//   tiny_conv_rows_kernel<PF, CF, IMG>   fp16 rows in (cin = 64).  Implicit GEMM on v_mfma_f32_16x16x32_f16 over k = tap * 64 + c: K = 576 = 18 steps, none
//       zero-filled.  One persistent workgroup of 8 waves per CU:
//         * the weight goes to LDS ONCE per workgroup, in fragment order - step s, channel fragment f, lane l at ((s * CF + f) * 64 + l) * 16 bytes - so a
//           wave's operand read is one lane-linear ds_read_b128 (conflict-free by construction).  CF = 4: cout = 64, 72 KiB; CF = 1: cout <= 4 (image
//           output), the rows >= cout are zero, 18 KiB;
//         * the workgroup walks output tiles (tile id = blockIdx.x, + gridDim.x, ...) of 16 x 32 pixels (PF = 4: a wave owns 2 rows x 32 columns = four
//           16-pixel fragments) or 8 x 16 (PF = 1, the stride-2 form: a wave owns one row of 16).  Per tile the INPUT patch with its halo is staged once:
//           18 x 34 pixels at stride 1, 17 x 33 at stride 2, and with `upsample` the LOW-RESOLUTION 10 x 18 patch - the upsampled tensor exists nowhere,
//           tap (iy, ix) reads patch pixel (iy >> 1, ix >> 1).  Pixels outside the image are stored as zeros, so the nine taps need no bounds test and
//           nothing outside an image's own h x wd rows is ever loaded (a tile lies in ONE image: no tap crosses into a neighbour's rows);
//         * a patch pixel is 128 bytes (64 halfs); its eight 16-byte chunks are XOR-swizzled by (pixel & 7), which makes the fragment read of 16
//           consecutive pixels x one chunk column conflict-free for ds_read_b128 (two pixels per 256-byte bank row, eight chunk slots each);
//         * operands are passed swapped (weights as MFMA-A, pixels as MFMA-B), as in pv_hintconv.hip: a lane ends with four consecutive output channels of
//           one pixel - an 8-byte store, an 8-byte residual load, a 16-byte bias load.
//       Accumulation order: steps 0 .. 17 in order, inside the MFMA the hardware's fixed order: every launch gives the same bits, and a pixel's result
//       does not depend on the tile walk (the batch equals its images one by one).
//   tiny_conv_image_kernel   fp32 NCHW in, cin <= 4 (K <= 36: too short for a matrix instruction): one output pixel per thread on vector FMAs, the input
//       read through `pre`, the padding taps 0 AFTER `pre`; eight output channels at a time, weights at wave-uniform addresses.
#include "pv_common.h"

#define TC_THREADS 512
#define TC_CIN 64
#define TC_K (9 * TC_CIN)
#define TC_STEPS (TC_K / 32)
#define TC_PATCH_PIXELS (18 * 34)                // the largest staged patch: stride 1 under a 16 x 32 tile
#define TC_PATCH_BYTES (TC_PATCH_PIXELS * 128)
#define TC_MAX_WGS 256                           // one persistent workgroup per CU

namespace {

struct tc_args {
    const half_t* x; int ldx;
    const half_t* w; const float* bias;
    const half_t* res; int ldr;
    void* out; int ldo;
    float out_scale, out_shift;
    int batch, cout, h, wd, ho, wo, stride, ups, act;
    int tiles_x, tiles_y, tiles;
};

__device__ __forceinline__ float tc_pre(float v, int pre) {
    if (pre == PV_TINY_PRE_TANH3) return 3.f * tanhf(v * (1.f / 3.f));
    if (pre == PV_TINY_PRE_UNIT) return (v + 1.f) * 0.5f;
    return v;
}

template <int PF, int CF, bool IMG>
__global__ __launch_bounds__(TC_THREADS) void tiny_conv_rows_kernel(const tc_args a) {
    constexpr int RPW = PF == 4 ? 2 : 1;         // output rows per wave
    constexpr int CPF = PF / RPW;                // 16-pixel fragments per row
    constexpr int TH = 8 * RPW, TW = 16 * CPF;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const wlds = smem;                                      // [TC_STEPS][CF][64 lanes][16 bytes]
    char* const patch = smem + TC_STEPS * CF * 1024;              // [PH * PW pixels][128 bytes], chunks swizzled
    const int tid = (int)threadIdx.x, lane = pv_lane_id(), wave = pv_wave_id();
    const int r16 = lane & 15, g = lane >> 4;

    for (int i = tid; i < TC_STEPS * CF * 64; i += TC_THREADS) {
        const int l = i & 63, f = (i >> 6) % CF, s = i / (64 * CF);
        const int co = f * 16 + (l & 15), k = s * 32 + 8 * (l >> 4);
        half8_t v = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
        if (co < a.cout) v = *(const half8_t*)(a.w + (size_t)co * TC_K + k);
        *(half8_t*)(wlds + (size_t)i * 16) = v;
    }

    const int stride = a.stride, ups = a.ups;
    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += (int)gridDim.x) {
        const int tx = tile % a.tiles_x, ty = (tile / a.tiles_x) % a.tiles_y, b = tile / (a.tiles_x * a.tiles_y);
        const int oy0 = ty * TH, ox0 = tx * TW;
        // the patch in input coordinates: [p0y, p0y + PH) x [p0x, p0x + PW) covers every tap of the whole tile (also of its pixels beyond ho / wo)
        const int p0y = (oy0 * stride - 1) >> ups, p0x = (ox0 * stride - 1) >> ups;
        const int PH = ((((oy0 + TH - 1) * stride + 1) >> ups) - p0y) + 1, PW = ((((ox0 + TW - 1) * stride + 1) >> ups) - p0x) + 1;
        const half_t* const img = a.x + (size_t)b * a.h * a.wd * a.ldx;
        __syncthreads();                         // the previous tile's reads of the patch are done (first tile: nothing to wait for)
        for (int i = tid; i < PH * PW * 8; i += TC_THREADS) {
            const int pix = i >> 3, ch = i & 7;
            const int py = pix / PW, px = pix - py * PW;
            const int sy = p0y + py, sx = p0x + px;
            half8_t v = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
            if (sy >= 0 && sy < a.h && sx >= 0 && sx < a.wd) v = *(const half8_t*)(img + ((size_t)sy * a.wd + sx) * a.ldx + ch * 8);
            *(half8_t*)(patch + pix * 128 + ((ch ^ (pix & 7)) << 4)) = v;
        }
        __syncthreads();

        // this lane's pixel of every fragment: patch row offsets of the three tap rows and patch columns of the three tap columns
        int rowoff[PF][3], col[PF][3];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int oy = oy0 + wave * RPW + p / CPF, ox = ox0 + (p % CPF) * 16 + r16;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                rowoff[p][t] = (((oy * stride + t - 1) >> ups) - p0y) * PW;
                col[p][t] = ((ox * stride + t - 1) >> ups) - p0x;
            }
        }
        float4_t acc[CF][PF];
#pragma unroll
        for (int f = 0; f < CF; ++f)
#pragma unroll
            for (int p = 0; p < PF; ++p) acc[f][p] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < TC_STEPS; ++s) {
            const int tap = s >> 1, ky = tap / 3, kx = tap - 3 * ky, ch = (s & 1) * 4 + g;
            half8_t wa[CF], xb[PF];
#pragma unroll
            for (int f = 0; f < CF; ++f) wa[f] = *(const half8_t*)(wlds + ((s * CF + f) * 64 + lane) * 16);
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int pix = rowoff[p][ky] + col[p][kx];
                xb[p] = *(const half8_t*)(patch + pix * 128 + ((ch ^ (pix & 7)) << 4));
            }
#pragma unroll
            for (int f = 0; f < CF; ++f)
#pragma unroll
                for (int p = 0; p < PF; ++p) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[f], xb[p], acc[f][p], 0, 0, 0);
        }

        // D[channel = 4 g + r][pixel = lane & 15]
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int oy = oy0 + wave * RPW + p / CPF, ox = ox0 + (p % CPF) * 16 + r16;
            if (oy >= a.ho || ox >= a.wo) continue;
            if (IMG) {
                float* const o = (float*)a.out;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = 4 * g + r;
                    if (co < a.cout) {
                        const float y = acc[0][p][r] + (a.bias ? a.bias[co] : 0.f);
                        o[(((size_t)b * a.cout + co) * a.ho + oy) * a.wo + ox] = fmaf(a.out_scale, y, a.out_shift);
                    }
                }
            } else {
                const size_t m = ((size_t)b * a.ho + oy) * a.wo + ox;
#pragma unroll
                for (int f = 0; f < CF; ++f) {
                    const int co = f * 16 + 4 * g;
                    float4_t v = acc[f][p];
                    if (a.bias) v += *(const float4_t*)(a.bias + co);
                    if (a.res) {
                        const half4_t rv = *(const half4_t*)(a.res + m * a.ldr + co);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
                    }
                    half4_t o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (half_t)(a.act == PV_ACT_RELU ? (v[r] > 0.f ? v[r] : 0.f) : v[r]);
                    *(half4_t*)((half_t*)a.out + m * a.ldo + co) = o;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void tiny_conv_image_kernel(const float* __restrict__ x, int pre, const half_t* __restrict__ w,
                                                              const float* __restrict__ bias, const half_t* __restrict__ res, int ldr,
                                                              half_t* __restrict__ out, int ldo, int batch, int cin, int cout, int h, int wd, int act) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long M = (long long)batch * h * wd;
    if (m >= M) return;
    const int ox = (int)(m % wd), oy = (int)((m / wd) % h), b = (int)(m / ((long long)wd * h));
    float in[36];                               // [tap][ci]; the padding is 0 AFTER the pre-transform
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
        const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < wd;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            in[t * 4 + ci] = (ok && ci < cin) ? tc_pre(x[(((size_t)b * cin + ci) * h + iy) * wd + ix], pre) : 0.f;
    }
    const int K = 9 * cin;
    for (int c0 = 0; c0 < cout; c0 += 8) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = bias ? bias[c0 + j] : 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
                if (ci < cin) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(in[t * 4 + ci], (float)w[(size_t)(c0 + j) * K + t * cin + ci], acc[j]);
                }
        if (res) {
            const half8_t rv = *(const half8_t*)(res + (size_t)m * ldr + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)rv[j];
        }
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(act == PV_ACT_RELU ? (acc[j] > 0.f ? acc[j] : 0.f) : acc[j]);
        *(half8_t*)(out + (size_t)m * ldo + c0) = o;
    }
}

// [lo, hi) byte ranges
bool tc_overlap(uintptr_t a, unsigned long long an, uintptr_t b, unsigned long long bn) { return a < b + bn && b < a + an; }

template <int PF, int CF, bool IMG>
int tc_launch(const tc_args& a, hipStream_t s) {
    constexpr int smem = TC_STEPS * CF * 1024 + TC_PATCH_BYTES;
    static bool attr_set_dev[64] = {};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    auto kern = tiny_conv_rows_kernel<PF, CF, IMG>;
    if (!attr_set_dev[dev_id & 63]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        attr_set_dev[dev_id & 63] = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.tiles < TC_MAX_WGS ? a.tiles : TC_MAX_WGS)), dim3(TC_THREADS), smem, s, a);
    return PV_CHECK_LAUNCH();
}

}  // namespace

extern "C" int32_t pv_tiny_conv3x3(const void* x, int32_t x_is_image, int32_t ldx, int32_t pre, const void* w, const float* bias, const void* res,
                                   int32_t ldr, void* out, int32_t out_is_image, int32_t ldo, float out_scale, float out_shift, int32_t batch, int32_t cin,
                                   int32_t cout, int32_t h, int32_t wd, int32_t stride, int32_t upsample, int32_t act, void* stream) {
    const int INVALID = (int)hipErrorInvalidValue;
    if (!x || !w || !out) return INVALID;
    if (batch < 1 || h < 1 || wd < 1) return INVALID;
    if ((x_is_image != 0 && x_is_image != 1) || (out_is_image != 0 && out_is_image != 1)) return INVALID;
    if (x_is_image && out_is_image) return INVALID;                                  // one side is always the 64-wide rows
    if (x_is_image ? (cin < 1 || cin > 4) : cin != TC_CIN) return INVALID;
    if (out_is_image ? (cout < 1 || cout > 4) : cout != 64) return INVALID;
    if (stride != 1 && stride != 2) return INVALID;
    if (upsample != 0 && upsample != 1) return INVALID;
    if (stride == 2 && upsample) return INVALID;
    if (x_is_image && (stride != 1 || upsample)) return INVALID;                      // the geometry belongs to the rows input
    if (pre != PV_TINY_PRE_NONE && pre != PV_TINY_PRE_TANH3 && pre != PV_TINY_PRE_UNIT) return INVALID;
    if (!x_is_image && pre != PV_TINY_PRE_NONE) return INVALID;
    if (act != PV_ACT_NONE && act != PV_ACT_RELU) return INVALID;
    if (out_is_image && (act != PV_ACT_NONE || res)) return INVALID;
    if (out_is_image ? !(out_scale == out_scale && out_shift == out_shift && out_scale - out_scale == 0.f && out_shift - out_shift == 0.f) : false)
        return INVALID;
    if (!x_is_image && (ldx < cin || ldx % 8)) return INVALID;
    if (!out_is_image && (ldo < cout || ldo % 8)) return INVALID;
    if (res && (ldr < cout || ldr % 8)) return INVALID;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)out) & 15) return INVALID;
    const unsigned long long lim = 1ull << 31;
    unsigned long long in_el = (unsigned long long)batch * (unsigned long long)h;
    if (in_el >= lim) return INVALID;
    in_el *= (unsigned long long)wd;
    if (in_el >= lim) return INVALID;
    const unsigned long long in_bytes = x_is_image ? in_el * 4ull * cin : ((in_el - 1) * ldx + cin) * 2ull;
    if (in_bytes >= lim) return INVALID;
    const int hv = upsample ? 2 * h : h, wv = upsample ? 2 * wd : wd;                 // h * wd * 8 <= in_bytes < 2^31: no overflow
    const int ho = (hv - 1) / stride + 1, wo = (wv - 1) / stride + 1;
    unsigned long long out_el = (unsigned long long)batch * (unsigned long long)ho;
    if (out_el >= lim) return INVALID;
    out_el *= (unsigned long long)wo;
    if (out_el >= lim) return INVALID;
    const unsigned long long out_bytes = out_is_image ? out_el * 4ull * cout : ((out_el - 1) * ldo + cout) * 2ull;
    const unsigned long long res_bytes = res ? ((out_el - 1) * ldr + cout) * 2ull : 0;
    if (out_bytes >= lim || res_bytes >= lim) return INVALID;
    if (tc_overlap((uintptr_t)out, out_bytes, (uintptr_t)x, in_bytes) || tc_overlap((uintptr_t)out, out_bytes, (uintptr_t)w, 18ull * cin * cout) ||
        (bias && tc_overlap((uintptr_t)out, out_bytes, (uintptr_t)bias, 4ull * cout)) ||
        (res && tc_overlap((uintptr_t)out, out_bytes, (uintptr_t)res, res_bytes)))
        return INVALID;

    hipStream_t s = (hipStream_t)stream;
    if (x_is_image) {
        tiny_conv_image_kernel<<<dim3((unsigned)((out_el + 255) / 256)), dim3(256), 0, s>>>((const float*)x, pre, (const half_t*)w, bias, (const half_t*)res,
                                                                                            ldr, (half_t*)out, ldo, batch, cin, cout, h, wd, act);
        return PV_CHECK_LAUNCH();
    }
    tc_args a;
    a.x = (const half_t*)x; a.ldx = ldx; a.w = (const half_t*)w; a.bias = bias; a.res = (const half_t*)res; a.ldr = ldr; a.out = out; a.ldo = ldo;
    a.out_scale = out_scale; a.out_shift = out_shift;
    a.batch = batch; a.cout = cout; a.h = h; a.wd = wd; a.ho = ho; a.wo = wo; a.stride = stride; a.ups = upsample; a.act = act;
    const int th = stride == 2 ? 8 : 16, tw = stride == 2 ? 16 : 32;
    a.tiles_x = (wo + tw - 1) / tw;
    a.tiles_y = (ho + th - 1) / th;
    const unsigned long long tiles = (unsigned long long)a.tiles_x * a.tiles_y * batch;      // <= out_el < 2^31
    a.tiles = (int)tiles;
    if (stride == 2) return out_is_image ? tc_launch<1, 1, true>(a, s) : tc_launch<1, 4, false>(a, s);
    return out_is_image ? tc_launch<4, 1, true>(a, s) : tc_launch<4, 4, false>(a, s);
}
