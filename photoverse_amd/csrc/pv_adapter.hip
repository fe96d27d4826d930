// The two launches a T2I-Adapter needs beyond the existing paths (header: pv_add_feature_rows, pv_pixel_unshuffle8).  Both are HBM-bound: 16-byte
// loads and stores, no atomics, no scratch.
#include "pv_common.h"

namespace {

// pv_add_feature_rows.  A 256-thread workgroup owns one 64-row block of one 128-column group: 16 column chunks of 8 (a lane's 16-byte load) x 16 row
// lanes, every lane 4 rows (r, r + 16, r + 32, r + 48 of the block) - a wave reads 256 contiguous bytes of each of 4 rows per load instruction, and a
// lane's 4 x loads (and 4 f loads) are issued before the first use.  The column statistics of the block are the workgroup's alone: a lane sums its 4 rows
// in row order, the 16 row lanes meet in LDS and are added in lane order by the thread that owns the (statistic, column) - the same bits on every launch,
// eager, replayed or on a side stream.  LDS: 16 x 2 x 128 fp32 = 16 KB.
constexpr int AF_BLOCK_ROWS = 64, AF_CHUNKS = 16, AF_COLS = AF_CHUNKS * 8, AF_ROW_LANES = 16, AF_ROWS_PER_LANE = 4;

// step index of the loop state block, clamped to the table length state[1] (0 = length unknown), as every per-step table read of the library
__device__ __forceinline__ int af_step_index(const int32_t* state) {
    const int i = state[0], n = state[1];
    return n > 0 ? min(i, n - 1) : i;
}

template <bool STATS>
__global__ __launch_bounds__(256) void add_feature_rows_kernel(const half_t* __restrict__ x, int ldx, const half_t* __restrict__ f, int ldf, int feat_rows,
                                                               half_t* __restrict__ out, int ldo, int rows, int cols, float scale,
                                                               const float* __restrict__ scale_tab, const int32_t* __restrict__ state,
                                                               float* __restrict__ colstats, int col_groups) {
    __shared__ __attribute__((aligned(16))) float red[STATS ? AF_ROW_LANES : 1][2][AF_COLS];
    const int tid = threadIdx.x, ch = tid & (AF_CHUNKS - 1), rl = tid / AF_CHUNKS;
    const int blk = blockIdx.x / col_groups, cg = blockIdx.x - blk * col_groups;     // column group fastest: neighbouring workgroups share rows
    const float s = scale_tab ? scale_tab[af_step_index(state)] : scale;             // the same in every lane
    const int c0 = cg * AF_COLS + ch * 8;
    const bool col_ok = c0 < cols;                                                   // cols % 8 == 0: a chunk is inside or outside as a whole
    const int r0 = blk * AF_BLOCK_ROWS + rl;
    half8_t xv[AF_ROWS_PER_LANE], fv[AF_ROWS_PER_LANE];
    bool ok[AF_ROWS_PER_LANE];
#pragma unroll
    for (int k = 0; k < AF_ROWS_PER_LANE; ++k) {
        const int r = r0 + k * AF_ROW_LANES;
        ok[k] = col_ok && r < rows;
        if (ok[k]) xv[k] = *reinterpret_cast<const half8_t*>(x + (long)r * ldx + c0);
    }
    if (s != 0.f) {
#pragma unroll
        for (int k = 0; k < AF_ROWS_PER_LANE; ++k) {
            const int r = r0 + k * AF_ROW_LANES;
            if (ok[k]) fv[k] = *reinterpret_cast<const half8_t*>(f + (long)(r % feat_rows) * ldf + c0);
        }
    }
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < AF_ROWS_PER_LANE; ++k) {
        if (!ok[k]) continue;
        half8_t o = xv[k];                                                           // s == 0: the bits of x, f never read
        if (s != 0.f) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)fmaf(s, (float)fv[k][e], (float)xv[k][e]);
        }
        *reinterpret_cast<half8_t*>(out + (long)(r0 + k * AF_ROW_LANES) * ldo + c0) = o;
        if (STATS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = (float)o[e];                                         // of the fp16-rounded output, as the GEMM epilogues'
                sum[e] += v;
                sq[e] = fmaf(v, v, sq[e]);
            }
        }
    }
    if (STATS) {
        float4_t* d0 = reinterpret_cast<float4_t*>(&red[rl][0][ch * 8]);
        float4_t* d1 = reinterpret_cast<float4_t*>(&red[rl][1][ch * 8]);
        d0[0] = float4_t{sum[0], sum[1], sum[2], sum[3]};
        d0[1] = float4_t{sum[4], sum[5], sum[6], sum[7]};
        d1[0] = float4_t{sq[0], sq[1], sq[2], sq[3]};
        d1[1] = float4_t{sq[4], sq[5], sq[6], sq[7]};
        __syncthreads();
        const int st = tid / AF_COLS, c = tid - st * AF_COLS;                        // 256 threads = 2 statistics x 128 columns
        const int col = cg * AF_COLS + c;
        if (col < cols) {
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < AF_ROW_LANES; ++i) a += red[i][st][c];              // fixed order
            colstats[((long)blk * 2 + st) * cols + col] = a;
        }
    }
}

// pv_pixel_unshuffle8.  One lane owns 8 adjacent output columns of one output row: fixed (c, i), j = 0 ... 7 - the 32 contiguous bytes
// image[b][c][8 y + i][8 x ... 8 x + 7] in (two 16-byte loads), one 16-byte store out; chunk index fastest, so a wave writes whole output rows.
__global__ __launch_bounds__(256) void pixel_unshuffle8_kernel(const float* __restrict__ img, long bstride, half_t* __restrict__ out, int ldo, int C, int H,
                                                               int W, long lanes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lanes) return;
    const int cpr = C * 8;                                    // 8-column chunks per output row
    const long pix = i / cpr;                                 // (b * hp + y) * wp + x
    const int q = (int)(i - pix * cpr);                       // c * 8 + i
    const int c = q >> 3, ii = q & 7;
    const int hp = H >> 3, wp = W >> 3;
    const long row = pix / wp;
    const int ox = (int)(pix - row * wp);
    const long b = row / hp;
    const int oy = (int)(row - b * hp);
    const float* src = img + b * bstride + ((long)c * H + (oy * 8 + ii)) * W + ox * 8;
    const float4_t lo = *reinterpret_cast<const float4_t*>(src), hi = *reinterpret_cast<const float4_t*>(src + 4);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[e] = (half_t)lo[e];
        o[e + 4] = (half_t)hi[e];
    }
    *reinterpret_cast<half8_t*>(out + pix * ldo + q * 8) = o;
}
}  // namespace

extern "C" int32_t pv_add_feature_rows(const void* x, int32_t ldx, const void* f, int32_t ldf, int32_t feat_rows, void* out, int32_t ldo, int32_t rows,
                                       int32_t cols, float scale, const float* scale_tab, const int32_t* state, float* colstats, void* stream) {
    if (!x || !f || !out || out == x || out == f) return (int)hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0 || (cols % 8) || feat_rows <= 0 || (rows % feat_rows)) return (int)hipErrorInvalidValue;
    if ((ldx % 8) || (ldf % 8) || (ldo % 8) || ldx < cols || ldf < cols || ldo < cols) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(x) % 16) || (reinterpret_cast<uintptr_t>(f) % 16) || (reinterpret_cast<uintptr_t>(out) % 16) ||
        (reinterpret_cast<uintptr_t>(colstats) % 4) || (reinterpret_cast<uintptr_t>(scale_tab) % 4) || (reinterpret_cast<uintptr_t>(state) % 4))
        return (int)hipErrorInvalidValue;
    if (scale_tab ? !state : !__builtin_isfinite(scale)) return (int)hipErrorInvalidValue;      // the table is indexed by the loop's step counter
    // rows of ld elements below 2 GiB = 2^30 halfs
    const int64_t lim = (int64_t)1 << 30;
    if ((int64_t)rows * ldx >= lim || (int64_t)rows * ldo >= lim || (int64_t)feat_rows * ldf >= lim) return (int)hipErrorInvalidValue;
    const int col_groups = (cols + AF_COLS - 1) / AF_COLS;
    const int64_t blocks = (int64_t)((rows + AF_BLOCK_ROWS - 1) / AF_BLOCK_ROWS) * col_groups;
    if (blocks >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
#define PV_AF_LAUNCH(STATS)                                                                                                                        \
    hipLaunchKernelGGL((add_feature_rows_kernel<STATS>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const half_t*>(x), \
                       ldx, reinterpret_cast<const half_t*>(f), ldf, feat_rows, reinterpret_cast<half_t*>(out), ldo, rows, cols, scale, scale_tab, state, \
                       colstats, col_groups)
    if (colstats) PV_AF_LAUNCH(true);
    else PV_AF_LAUNCH(false);
#undef PV_AF_LAUNCH
    return PV_CHECK_LAUNCH();
}

extern "C" int32_t pv_pixel_unshuffle8(const float* image, int64_t batch_stride, void* out, int32_t ldo, int32_t batch, int32_t channels, int32_t h,
                                       int32_t w, void* stream) {
    if (!image || !out || (const void*)image == out) return (int)hipErrorInvalidValue;
    if (batch <= 0 || channels < 1 || channels > 4 || h <= 0 || w <= 0 || (h % 8) || (w % 8)) return (int)hipErrorInvalidValue;
    const int cols = channels * 64;
    if ((ldo % 8) || ldo < cols) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(image) % 16) || (reinterpret_cast<uintptr_t>(out) % 16)) return (int)hipErrorInvalidValue;
    const int64_t lim = (int64_t)1 << 30;
    const int64_t plane = (int64_t)h * w;                      // < 2^62
    if (plane >= lim || plane * channels >= lim) return (int)hipErrorInvalidValue;
    if (batch_stride != 0 && (batch_stride < plane * channels || (batch_stride % 4))) return (int)hipErrorInvalidValue;   // 0: one image for every sample
    const int64_t pixels = (int64_t)batch * (plane / 64);
    if (pixels >= lim || pixels * ldo >= lim || (batch_stride != 0 && batch_stride >= lim / batch)) return (int)hipErrorInvalidValue;
    const int64_t lanes = pixels * channels * 8;
    const int64_t blocks = (lanes + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pixel_unshuffle8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, image, (long)batch_stride,
                       reinterpret_cast<half_t*>(out), ldo, channels, h, w, (long)lanes);
    return PV_CHECK_LAUNCH();
}
