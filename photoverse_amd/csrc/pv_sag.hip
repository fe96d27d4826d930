// [EXT] Self-attention guidance (Hong et al., ICCV 2023; diffusers' StableDiffusionSAGPipeline): the two launches it needs that the project did not have.
//   attn_colmass_kernel  mass[b][j] = mean_h sum_i softmax_j(q_i . k_j / sqrt d): how much attention key j receives.  pv_attention never holds the map, so
//                        this kernel forms it tile by tile on v_mfma_f32_16x16x32_f16 and keeps only its column sums.
//   sag_degrade_kernel   x_deg = x + (1/ca) m (blur(x0) - x0): threshold of the mass, nearest upsample, x0 from the step's coefficient row, the 9x9
//                        Gaussian blur with reflect padding and the blend, in one launch.
#include "pv_common.h"

#define CM_WAVES 8              // waves of a column-mass workgroup
#define CM_MAX_N 1024           // queries / keys per (batch, head)

// One workgroup per batch element.  The work items (head, 16-query tile) are dealt to the waves round-robin, item t to wave t % CM_WAVES, and a wave runs
// its items in order; each item is two sweeps over the keys in 16-key tiles, scores S = Q K^T on the MFMA (queries as A, keys as B: lane (r16, g) holds
// S[query 4 g + r][key r16], r = 0 .. 3):
//   sweep 1  per lane the online (max, sum) of its keys of every row, then one butterfly over the 16 lanes of a row: the row maximum M and l = sum exp(s - M);
//   sweep 2  the scores again, p = exp2(t - M) / l in fp32 (never rounded to fp16), summed over the tile's 16 queries (in-lane over r, two lane swaps over g)
//            and added to the wave's own LDS row col[wave][key].
// Then the rows of the waves are added in wave order and scaled by 1 / heads.  No atomics and a fixed order everywhere: a graph replay gives the bits of an
// eager launch.  K is read twice from L2; nothing is written but mass.  KS = ceil(d / 32) MFMA steps per tile; the k >= d part of the last step is zero-filled.
template <int KS>
__global__ __launch_bounds__(CM_WAVES * 64) void attn_colmass_kernel(const half_t* __restrict__ q, int ldq, const half_t* __restrict__ k, int ldk,
                                                                     float* __restrict__ mass, int heads, int nq, int nk, int d, float scale_log2) {
    __shared__ float col[CM_WAVES][CM_MAX_N];
    const int lane = pv_lane_id(), wave = pv_wave_id();
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.x;
    for (int j = lane; j < nk; j += 64) col[wave][j] = 0.f;            // a wave's row is its own until the final sum
    __syncthreads();
    const int qtiles = (nq + 15) >> 4, ktiles = (nk + 15) >> 4;
    const int items = heads * qtiles;
    const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const float NEG = -3.0e38f;                                        // finite: exp2(NEG - x) is 0, never inf - inf
    for (int it = wave; it < items; it += CM_WAVES) {                  // wave-uniform
        const int hd = it / qtiles, q0 = (it - hd * qtiles) * 16;
        half8_t qa[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int kk = s * 32 + 8 * g;
            qa[s] = zero8;
            if (q0 + r16 < nq && kk < d) qa[s] = *(const half8_t*)(q + ((size_t)b * nq + q0 + r16) * ldq + hd * d + kk);
        }
        const half_t* kh = k + (size_t)b * nk * ldk + hd * d;
        float m[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = NEG; l[r] = 0.f; }
        for (int kt = 0; kt < ktiles; ++kt) {
            const int key = kt * 16 + r16;
            float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int kk = s * 32 + 8 * g;
                half8_t kb = zero8;
                if (key < nk && kk < d) kb = *(const half8_t*)(kh + (size_t)key * ldk + kk);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[s], kb, acc, 0, 0, 0);
            }
            if (key < nk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float t = acc[r] * scale_log2;
                    const float mn = fmaxf(m[r], t);
                    l[r] = l[r] * PV_EXP2(m[r] - mn) + PV_EXP2(t - mn);
                    m[r] = mn;
                }
            }
        }
        float inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float M = m[r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
            float L = l[r] * PV_EXP2(m[r] - M);                        // a lane without a key: 0 * 0
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) L += __shfl_xor(L, o, 64);
            m[r] = M;
            inv[r] = (q0 + 4 * g + r < nq) ? 1.f / L : 0.f;            // rows past nq add nothing
        }
        for (int kt = 0; kt < ktiles; ++kt) {
            const int key = kt * 16 + r16;
            float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int kk = s * 32 + 8 * g;
                half8_t kb = zero8;
                if (key < nk && kk < d) kb = *(const half8_t*)(kh + (size_t)key * ldk + kk);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[s], kb, acc, 0, 0, 0);
            }
            float c = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) c += PV_EXP2(acc[r] * scale_log2 - m[r]) * inv[r];
            c = pv_quad_sum(c);                                        // over the four query groups g
            if (g == 0 && key < nk) col[wave][key] += c;
        }
    }
    __syncthreads();
    const float inv_heads = 1.f / (float)heads;
    for (int j = threadIdx.x; j < nk; j += CM_WAVES * 64) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < CM_WAVES; ++w) s += col[w][j];
        mass[(size_t)b * nk + j] = s * inv_heads;
    }
}

extern "C" int32_t pv_attn_colmass(const void* q, int32_t ldq, const void* k, int32_t ldk, float* mass, int32_t batch, int32_t heads, int32_t nq, int32_t nk,
                                   int32_t d, void* stream) {
    if (!q || !k || !mass) return (int)hipErrorInvalidValue;
    if (d != 40 && d != 64 && d != 80 && d != 160) return (int)hipErrorInvalidValue;
    if (batch < 1 || heads < 1 || nq < 1 || nk < 1 || nq > CM_MAX_N || nk > CM_MAX_N) return (int)hipErrorInvalidValue;
    const long long width = (long long)heads * d, lim = 1ll << 31;
    if (width >= lim || ldq < width || ldk < width || (ldq % 8) || (ldk % 8)) return (int)hipErrorInvalidValue;
    if ((((uintptr_t)q | (uintptr_t)k) & 15) || ((uintptr_t)mass & 3)) return (int)hipErrorInvalidValue;
    if ((long long)batch * nq * ldq * 2 >= lim || (long long)batch * nk * ldk * 2 >= lim) return (int)hipErrorInvalidValue;     // (each factor < 2^31, nq / nk <= 1024: no overflow of 64 bits)
    const float scale_log2 = (float)(1.4426950408889634 / sqrt((double)d));
    const dim3 grid((unsigned)batch), block(CM_WAVES * 64);
    hipStream_t s = (hipStream_t)stream;
#define PV_CM_LAUNCH(KS) \
    hipLaunchKernelGGL((attn_colmass_kernel<KS>), grid, block, 0, s, (const half_t*)q, ldq, (const half_t*)k, ldk, mass, heads, nq, nk, d, scale_log2)
    if (d <= 64) PV_CM_LAUNCH(2);
    else if (d == 80) PV_CM_LAUNCH(3);
    else PV_CM_LAUNCH(5);
#undef PV_CM_LAUNCH
    return PV_CHECK_LAUNCH();
}

#define SD_TILE 16              // output pixels per side of a workgroup's tile
#define SD_R 4                  // blur radius: 9 taps
#define SD_HALO (SD_TILE + 2 * SD_R)

// step index of the loop state block, clamped to the table length state[1] (0 = length unknown), as the solver-step kernels of pv_misc.hip read it
__device__ __forceinline__ int sd_step_index(const int32_t* state) {
    const int i = state[0], n = state[1];
    return n > 0 ? min(i, n - 1) : i;
}

struct sag_taps { float k[SD_R + 1]; };     // k[|t|], t = -4 .. 4: exp(-t^2 / 2) normalised over the nine taps

// torch's "reflect" padding: -1 -> 1, n -> n - 2 (the edge pixel is not repeated); |overshoot| <= 4 < n
__device__ __forceinline__ int sd_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// One workgroup per 16 x 16 tile of one (sample, channel) plane: x0 = ca x + cb eps on the tile and its 4-pixel halo (reflected at the plane's edge) into
// LDS, the separable blur - rows, then columns - through LDS, then per pixel
//   m = mass[b][(y mh / h) mw + (x mw / w)] > 1   (integer nearest upsample, strict comparison)
//   out = m ? x + (1/ca) (blur - x0) : x           (the bits of x where the mask is off)
// (ca, cb) = columns 0, 1 of the coefficient row the step's solver launch reads.
__global__ __launch_bounds__(SD_TILE * SD_TILE) void sag_degrade_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ mass,
                                                                        const float* __restrict__ coef, const int32_t* __restrict__ state, float* __restrict__ out,
                                                                        int channels, int h, int w, int mh, int mw, int tiles_x, int tiles_y, sag_taps taps) {
    __shared__ float x0s[SD_HALO][SD_HALO + 1];
    __shared__ float rows[SD_HALO][SD_TILE + 1];
    const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
    const int ty0 = (tile / tiles_x) * SD_TILE, tx0 = (tile % tiles_x) * SD_TILE;
    const int b = plane / channels;
    const float* c = coef + (long)sd_step_index(state) * 8;
    const float ca = c[0], cb = c[1];
    const size_t base = (size_t)plane * h * w;
    for (int i = threadIdx.x; i < SD_HALO * SD_HALO; i += SD_TILE * SD_TILE) {
        const int hy = i / SD_HALO, hx = i - hy * SD_HALO;
        // past the plane's last row / column (a partial tile) the index is clamped first: those values feed no pixel that is written
        const int y = sd_reflect(min(ty0 + hy - SD_R, h + SD_R - 1), h), xx = sd_reflect(min(tx0 + hx - SD_R, w + SD_R - 1), w);
        const size_t o = base + (size_t)y * w + xx;
        x0s[hy][hx] = ca * x[o] + cb * eps[o];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SD_HALO * SD_TILE; i += SD_TILE * SD_TILE) {
        const int hy = i / SD_TILE, px = i - hy * SD_TILE;
        float s = taps.k[0] * x0s[hy][px + SD_R];
#pragma unroll
        for (int t = 1; t <= SD_R; ++t) s += taps.k[t] * (x0s[hy][px + SD_R - t] + x0s[hy][px + SD_R + t]);
        rows[hy][px] = s;
    }
    __syncthreads();
    const int py = threadIdx.x / SD_TILE, px = threadIdx.x % SD_TILE;
    const int y = ty0 + py, xx = tx0 + px;
    if (y >= h || xx >= w) return;
    float bl = taps.k[0] * rows[py + SD_R][px];
#pragma unroll
    for (int t = 1; t <= SD_R; ++t) bl += taps.k[t] * (rows[py + SD_R - t][px] + rows[py + SD_R + t][px]);
    const size_t o = base + (size_t)y * w + xx;
    const float xv = x[o];
    const bool on = mass[(size_t)b * mh * mw + (size_t)((y * mh) / h) * mw + (xx * mw) / w] > 1.0f;
    out[o] = on ? xv + (1.f / ca) * (bl - x0s[py + SD_R][px + SD_R]) : xv;
}

extern "C" int32_t pv_sag_degrade(const float* x, const float* eps_base, const float* mass, const float* coef, const int32_t* state, float* x_deg,
                                  int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t mh, int32_t mw, void* stream) {
    if (!x || !eps_base || !mass || !coef || !state || !x_deg || x_deg == x || x_deg == eps_base) return (int)hipErrorInvalidValue;
    if (batch < 1 || channels < 1 || h < SD_R + 1 || w < SD_R + 1 || mh < 1 || mw < 1) return (int)hipErrorInvalidValue;
    const long long lim = 1ll << 31;
    if ((long long)h * w >= lim || (long long)h * mh >= lim || (long long)w * mw >= lim || (long long)mh * mw >= lim) return (int)hipErrorInvalidValue;
    if ((long long)batch * channels >= lim || (long long)batch * channels * ((long long)h * w) * 4 >= lim || (long long)batch * mh * mw * 4 >= lim)
        return (int)hipErrorInvalidValue;
    const int tiles_x = (w + SD_TILE - 1) / SD_TILE, tiles_y = (h + SD_TILE - 1) / SD_TILE;
    const long long blocks = (long long)batch * channels * tiles_x * tiles_y;
    if (blocks >= lim) return (int)hipErrorInvalidValue;
    sag_taps taps;
    double kd[SD_R + 1], sum = 0.0;
    for (int t = 0; t <= SD_R; ++t) {
        kd[t] = exp(-0.5 * t * t);
        sum += (t ? 2.0 : 1.0) * kd[t];
    }
    for (int t = 0; t <= SD_R; ++t) taps.k[t] = (float)(kd[t] / sum);
    hipLaunchKernelGGL(sag_degrade_kernel, dim3((unsigned)blocks), dim3(SD_TILE * SD_TILE), 0, (hipStream_t)stream, x, eps_base, mass, coef, state, x_deg,
                       channels, h, w, mh, mw, tiles_x, tiles_y, taps);
    return PV_CHECK_LAUNCH();
}
