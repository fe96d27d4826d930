// pv_dense_conv3x3: the 3x3 convs of an RRDBNet (Real-ESRGAN's RealESRGAN_x4plus): cin in {64, 96, 128, 160, 192} -> cout in {32, 64}, LeakyReLU, up to
// two scaled residuals, optionally over the nearest-x2 upsampling of the input.  pv_gemm_conv has no N tile of 32 / 64 and no K of 96 / 160 per tap;
// pv_tiny_conv3x3 is 64 -> 64 with the whole weight resident in LDS, which the 192 -> 64 weight (216 KiB) is not.
//
//   dense_conv_kernel<CF, UPS>   implicit GEMM on v_mfma_f32_16x16x32_f16 over k = tap * cin + c, as pv_tinyconv.hip: one persistent workgroup of 8 waves
//       per CU walks 16 x 32 output tiles (tile id = blockIdx.x, + gridDim.x, ...), a wave owns 2 rows x 32 columns = four 16-pixel fragments and all
//       CF = cout / 16 channel fragments; operands swapped (weights as MFMA-A, pixels as MFMA-B), so a lane ends with four consecutive output channels of
//       one pixel: an 8-byte store, 8-byte residual loads, a 16-byte bias load.
//       K is staged in SLICES of 32 input channels (cin / 32 = 2 ... 6 slices per tile, 9 MFMA steps each - one per tap):
//         * the slice of the input patch with its halo: 18 x 34 pixels (UPS: the LOW-RESOLUTION 10 x 18 patch; tap (iy, ix) reads (iy >> 1, ix >> 1), the
//           upsampled tensor exists nowhere) x 64 bytes.  Pixels outside the image are stored as zeros: no tap needs a bounds test and nothing outside an
//           image's own h x wd rows is ever loaded.  The only global reads of x are these 16-byte chunks at columns slice * 32 + {0, 8, 16, 24} < cin:
//           nothing at or beyond column cin is read, which is what lets `out` be a column slice of x's own rows;
//         * a patch pixel is four 16-byte chunks, four pixels per 256-byte bank row; chunk c of pixel q sits in slot c ^ (3 * ((q >> 2) & 1)).  A
//           ds_read_b128 lane group holds the pixels {0-3, 12-15} of a fragment with chunk g and the pixels {4-11} with chunk g ^ 1: per residue q & 3 the
//           four pixels have q >> 2 = m ... m + 3 and the chunks (g, g^1, g^1, g), and s(m), s(m+1)^1, s(m+2)^1, s(m+3) are distinct for s = (0, 3, 0, 3)
//           at every m: the fragment read is conflict-free (UPS reads pixel pairs twice - a broadcast - and is not conflict-free everywhere);
//         * the slice of the weight in fragment order - tap t, channel fragment f, lane l at ((t * CF + f) * 64 + l) * 16 bytes, holding
//           w[f * 16 + (l & 15)][t * cin + slice * 32 + 8 * (l >> 4) ...] - so a wave's operand read is one lane-linear ds_read_b128.
//       Two stages: while the waves run the 9 steps of slice q out of one stage, slice q + 1 (of the same tile, or the first of the workgroup's next
//       tile) is in flight from global memory into registers (<= 5 + 5 16-byte loads per lane) and is written to the other stage behind the MFMAs; one
//       barrier per slice.
//       LDS per form (2 stages x (weight slice + patch slice)):
//           CF = 4            2 x (36864 + 18 * 34 * 64 = 39168) = 152064 bytes (148.5 KiB of 160)
//           CF = 2            2 x (18432 + 39168)                = 115200 bytes (112.5 KiB)
//           CF = 4, UPS       2 x (36864 + 10 * 18 * 64 = 11520) =  96768 bytes ( 94.5 KiB)
//       Accumulation order: slices 0 ... cin / 32 - 1, inside a slice the taps 0 ... 8, inside the MFMA the hardware's fixed order; fp32 throughout, one
//       rounding at the store.  Every launch gives the same bits, and a pixel's result does not depend on the tile walk (a batch equals its images one by
//       one).  No atomics, no scratch buffer.
#include "pv_common.h"

#define DC_THREADS 512
#define DC_TH 16
#define DC_TW 32
#define DC_MAX_WGS 256                           // one persistent workgroup per CU

namespace {

struct dc_args {
    const half_t* x; int ldx;
    const half_t* w; const float* bias;
    const half_t* res; int ldr;
    const half_t* res2; int ldr2;
    half_t* out; int ldo;
    float slope, alpha, beta;
    int cin, h, wd, ho, wo, act;
    int tiles_x, tiles_y, tiles;
};

template <int CF, bool UPS>
struct dc_geo {
    static constexpr int PH = UPS ? 10 : 18, PW = UPS ? 18 : 34;
    static constexpr int PCH = PH * PW * 4;                       // 16-byte chunks of a patch slice
    static constexpr int WCH = 9 * CF * 64;                       // 16-byte chunks of a weight slice
    static constexpr int PLD = (PCH + DC_THREADS - 1) / DC_THREADS, WLD = (WCH + DC_THREADS - 1) / DC_THREADS;
    static constexpr int WBYTES = WCH * 16, STAGE = WBYTES + PCH * 16;
};

template <int CF, bool UPS>
__global__ __launch_bounds__(DC_THREADS) void dense_conv_kernel(const dc_args a) {
    using G = dc_geo<CF, UPS>;
    constexpr int PW = G::PW;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][weight slice | patch slice]
    const int tid = (int)threadIdx.x, lane = pv_lane_id(), wave = pv_wave_id();
    const int r16 = lane & 15, g = lane >> 4;
    const int nsl = a.cin >> 5, cin = a.cin;
    const int my_tiles = (a.tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;        // >= 1: gridDim.x <= tiles
    const int total = my_tiles * nsl;

    // this lane's patch pixel of every fragment and tap; the same in every tile (a tile's patch starts one pixel - UPS: one low-resolution pixel -
    // above and left of it, and tile origins are even)
    int rowoff[4][3], col[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int ly = wave * 2 + (p >> 1), lx = (p & 1) * 16 + r16;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            rowoff[p][t] = (UPS ? ((ly + t - 1) >> 1) + 1 : ly + t) * PW;
            col[p][t] = UPS ? ((lx + t - 1) >> 1) + 1 : lx + t;
        }
    }

    half8_t pre_p[G::PLD], pre_w[G::WLD];
    // the load cursor: slice l_sl of tile l_tile
    int l_tile = (int)blockIdx.x, l_sl = 0;
    auto load = [&]() {
        const int tx = l_tile % a.tiles_x, ty = (l_tile / a.tiles_x) % a.tiles_y, b = l_tile / (a.tiles_x * a.tiles_y);
        const int p0y = UPS ? ty * (DC_TH / 2) - 1 : ty * DC_TH - 1, p0x = UPS ? tx * (DC_TW / 2) - 1 : tx * DC_TW - 1;
        const half_t* const img = a.x + (size_t)b * a.h * a.wd * a.ldx + l_sl * 32;
#pragma unroll
        for (int j = 0; j < G::PLD; ++j) {
            const int i = tid + j * DC_THREADS, pix = i >> 2, ch = i & 3;
            const int py = pix / PW, px = pix - py * PW;
            const int sy = p0y + py, sx = p0x + px;
            half8_t v = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
            if (i < G::PCH && sy >= 0 && sy < a.h && sx >= 0 && sx < a.wd) v = *(const half8_t*)(img + ((size_t)sy * a.wd + sx) * a.ldx + ch * 8);
            pre_p[j] = v;
        }
        const half_t* const ws = a.w + l_sl * 32;
#pragma unroll
        for (int j = 0; j < G::WLD; ++j) {
            const int i = tid + j * DC_THREADS;
            const int l = i & 63, f = (i >> 6) % CF, t = i / (64 * CF);
            half8_t v = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
            if (i < G::WCH) v = *(const half8_t*)(ws + (size_t)(f * 16 + (l & 15)) * (9 * cin) + t * cin + 8 * (l >> 4));
            pre_w[j] = v;
        }
        if (++l_sl == nsl) { l_sl = 0; l_tile += (int)gridDim.x; }
    };
    auto store = [&](char* stage) {
#pragma unroll
        for (int j = 0; j < G::WLD; ++j) {
            const int i = tid + j * DC_THREADS;
            if (i < G::WCH) *(half8_t*)(stage + i * 16) = pre_w[j];
        }
#pragma unroll
        for (int j = 0; j < G::PLD; ++j) {
            const int i = tid + j * DC_THREADS, pix = i >> 2, ch = i & 3;
            if (i < G::PCH) *(half8_t*)(stage + G::WBYTES + pix * 64 + ((ch ^ (((pix >> 2) & 1) * 3)) << 4)) = pre_p[j];
        }
    };

    load();
    store(smem);
    __syncthreads();

    float4_t acc[CF][4];
    int tile = (int)blockIdx.x, sl = 0;
    for (int q = 0; q < total; ++q) {
        if (q + 1 < total) load();                                // in flight under this slice's MFMAs
        if (sl == 0) {
#pragma unroll
            for (int f = 0; f < CF; ++f)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[f][p] = (float4_t){0.f, 0.f, 0.f, 0.f};
        }
        const char* const wlds = smem + (q & 1) * G::STAGE;
        const char* const patch = wlds + G::WBYTES;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
            half8_t wa[CF], xb[4];
#pragma unroll
            for (int f = 0; f < CF; ++f) wa[f] = *(const half8_t*)(wlds + ((t * CF + f) * 64 + lane) * 16);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int pix = rowoff[p][ky] + col[p][kx];
                xb[p] = *(const half8_t*)(patch + pix * 64 + ((g ^ (((pix >> 2) & 1) * 3)) << 4));
            }
#pragma unroll
            for (int f = 0; f < CF; ++f)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[f][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[f], xb[p], acc[f][p], 0, 0, 0);
        }

        if (sl == nsl - 1) {
            // D[channel = 4 g + r][pixel = lane & 15]
            const int tx = tile % a.tiles_x, ty = (tile / a.tiles_x) % a.tiles_y, b = tile / (a.tiles_x * a.tiles_y);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int oy = ty * DC_TH + wave * 2 + (p >> 1), ox = tx * DC_TW + (p & 1) * 16 + r16;
                if (oy >= a.ho || ox >= a.wo) continue;
                const size_t m = ((size_t)b * a.ho + oy) * a.wo + ox;
#pragma unroll
                for (int f = 0; f < CF; ++f) {
                    const int co = f * 16 + 4 * g;
                    float4_t v = acc[f][p];
                    if (a.bias) v += *(const float4_t*)(a.bias + co);
                    if (a.act == PV_ACT_LEAKY_RELU) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : a.slope * v[r];
                    }
                    if (a.res) {
                        const half4_t rv = *(const half4_t*)(a.res + m * a.ldr + co);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = fmaf(a.alpha, v[r], (float)rv[r]);
                        if (a.res2) {
                            const half4_t sv = *(const half4_t*)(a.res2 + m * a.ldr2 + co);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = fmaf(a.beta, v[r], (float)sv[r]);
                        }
                    }
                    half4_t o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (half_t)v[r];
                    *(half4_t*)(a.out + m * a.ldo + co) = o;
                }
            }
            tile += (int)gridDim.x;
            sl = 0;
        } else {
            ++sl;
        }
        if (q + 1 < total) store(smem + ((q + 1) & 1) * G::STAGE);    // the other stage: its last readers passed the barrier below one slice ago
        __syncthreads();
    }
}

bool dc_finite(float v) { return v == v && v - v == 0.f; }

// Two strided regions of fp16 rows - widths wa / wb elements, leading dimensions lda / ldb, byte extents an / bn - share no element: their byte ranges
// are apart, or they are column slices of the same rows (equal leading dimensions, the later one starting inside the earlier one's first row, behind
// its columns, and ending inside that row).
bool dc_disjoint(uintptr_t a, int lda, int wa, unsigned long long an, uintptr_t b, int ldb, int wb, unsigned long long bn) {
    if (!(a < b + bn && b < a + an)) return true;
    if (lda != ldb) return false;
    const uintptr_t lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned long long wlo = a < b ? wa : wb, whi = a < b ? wb : wa, d = hi - lo;
    return d >= 2ull * wlo && d + 2ull * whi <= 2ull * (unsigned long long)lda;
}

bool dc_overlap(uintptr_t a, unsigned long long an, uintptr_t b, unsigned long long bn) { return a < b + bn && b < a + an; }

template <int CF, bool UPS>
int dc_launch(const dc_args& a, hipStream_t s) {
    constexpr int smem = 2 * dc_geo<CF, UPS>::STAGE;
    static bool attr_set_dev[64] = {};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    auto kern = dense_conv_kernel<CF, UPS>;
    if (!attr_set_dev[dev_id & 63]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        attr_set_dev[dev_id & 63] = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.tiles < DC_MAX_WGS ? a.tiles : DC_MAX_WGS)), dim3(DC_THREADS), smem, s, a);
    return PV_CHECK_LAUNCH();
}

}  // namespace

extern "C" int32_t pv_dense_conv3x3(const void* x, int32_t ldx, const void* w, const float* bias, const void* res, int32_t ldr, const void* res2,
                                    int32_t ldr2, void* out, int32_t ldo, int32_t batch, int32_t cin, int32_t cout, int32_t h, int32_t wd,
                                    int32_t upsample, int32_t act, float slope, float alpha, float beta, void* stream) {
    const int INVALID = (int)hipErrorInvalidValue;
    if (!x || !w || !out) return INVALID;
    if (batch < 1 || h < 1 || wd < 1) return INVALID;
    if (cin != 64 && cin != 96 && cin != 128 && cin != 160 && cin != 192) return INVALID;
    if (cout != 32 && cout != 64) return INVALID;
    if (upsample != 0 && upsample != 1) return INVALID;
    if (upsample && (cin != 64 || cout != 64)) return INVALID;
    if (act != PV_ACT_NONE && act != PV_ACT_LEAKY_RELU) return INVALID;
    if (!dc_finite(slope) || !dc_finite(alpha) || !dc_finite(beta)) return INVALID;
    if (res2 && !res) return INVALID;
    if (ldx < cin || ldx % 8 || ldo < cout || ldo % 8) return INVALID;
    if (res && (ldr < cout || ldr % 8)) return INVALID;
    if (res2 && (ldr2 < cout || ldr2 % 8)) return INVALID;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)res2 | (uintptr_t)out) & 15) return INVALID;
    const unsigned long long lim = 1ull << 31;
    unsigned long long in_el = (unsigned long long)batch * (unsigned long long)h;
    if (in_el >= lim) return INVALID;
    in_el *= (unsigned long long)wd;
    if (in_el >= lim) return INVALID;
    const unsigned long long in_bytes = ((in_el - 1) * ldx + cin) * 2ull;
    if (in_bytes >= lim) return INVALID;
    const int ho = upsample ? 2 * h : h, wo = upsample ? 2 * wd : wd;                 // h * wd * 128 <= in_bytes < 2^31: no overflow
    unsigned long long out_el = (unsigned long long)batch * (unsigned long long)ho;
    if (out_el >= lim) return INVALID;
    out_el *= (unsigned long long)wo;
    if (out_el >= lim) return INVALID;
    const unsigned long long out_bytes = ((out_el - 1) * ldo + cout) * 2ull;
    const unsigned long long res_bytes = res ? ((out_el - 1) * ldr + cout) * 2ull : 0, res2_bytes = res2 ? ((out_el - 1) * ldr2 + cout) * 2ull : 0;
    if (out_bytes >= lim || res_bytes >= lim || res2_bytes >= lim) return INVALID;
    if (dc_overlap((uintptr_t)out, out_bytes, (uintptr_t)w, 18ull * cin * cout) || (bias && dc_overlap((uintptr_t)out, out_bytes, (uintptr_t)bias, 4ull * cout)))
        return INVALID;
    // out may be a column slice of x's rows at or behind column cin (the in-place dense block); the residuals are read where out is written
    if (!dc_disjoint((uintptr_t)x, ldx, cin, in_bytes, (uintptr_t)out, ldo, cout, out_bytes)) return INVALID;
    if (res && !dc_disjoint((uintptr_t)res, ldr, cout, res_bytes, (uintptr_t)out, ldo, cout, out_bytes)) return INVALID;
    if (res2 && !dc_disjoint((uintptr_t)res2, ldr2, cout, res2_bytes, (uintptr_t)out, ldo, cout, out_bytes)) return INVALID;
    if (res2 && !dc_disjoint((uintptr_t)res, ldr, cout, res_bytes, (uintptr_t)res2, ldr2, cout, res2_bytes)) return INVALID;

    dc_args a;
    a.x = (const half_t*)x; a.ldx = ldx; a.w = (const half_t*)w; a.bias = bias; a.res = (const half_t*)res; a.ldr = ldr;
    a.res2 = (const half_t*)res2; a.ldr2 = ldr2; a.out = (half_t*)out; a.ldo = ldo;
    a.slope = slope; a.alpha = alpha; a.beta = beta;
    a.cin = cin; a.h = h; a.wd = wd; a.ho = ho; a.wo = wo; a.act = act;
    a.tiles_x = (wo + DC_TW - 1) / DC_TW;
    a.tiles_y = (ho + DC_TH - 1) / DC_TH;
    a.tiles = (int)((unsigned long long)a.tiles_x * a.tiles_y * batch);               // <= out_el < 2^31
    hipStream_t s = (hipStream_t)stream;
    if (upsample) return dc_launch<4, true>(a, s);
    return cout == 64 ? dc_launch<4, false>(a, s) : dc_launch<2, false>(a, s);
}
