// Small HBM-bound kernels around the UNet: timestep embedding, conv_in / conv_out (layout change
// fused), GEGLU gate, CFG + DPM-Solver++ update, casts, patch-token mean.
#include "pv_common.h"

extern "C" int pv_abi_version(void) { return PV_ABI_VERSION; }

extern "C" int pv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

namespace {

// step index of the loop state block, clamped to the table length state[1] (0 = length unknown): a step() past the end of the
// schedule re-reads the last row instead of reading beyond the tables (the host raises before that, pipeline.DenoiseLoop.step)
__device__ __forceinline__ int pv_step_index(const int32_t* state) {
    const int i = state[0], n = state[1];
    return n > 0 ? min(i, n - 1) : i;
}

// [EXT] diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]
__global__ void timestep_embedding_kernel(const float* timesteps, const int32_t* state, int rows, int dim, half_t* out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * dim) return;
    const int row = idx / dim, i = idx - row * dim;
    const int half = dim >> 1;
    const float t = state ? timesteps[pv_step_index(state)] : timesteps[row];
    const int k = i < half ? i : i - half;
    const float freq = expf(-9.210340371976184f * (float)k / (float)half);  // ln(10000)
    const float a = t * freq;
    out[idx] = (half_t)(i < half ? cosf(a) : sinf(a));
}

// conv_out: NHWC fp16 -> NCHW fp32, 3x3 pad 1, cout <= 8 (UNet 320 -> 4, VAE 128 -> 3).  Far too few output channels for the
// MFMA tile: VALU kernel.  8 threads per output pixel, each owning the 16-byte channel chunks {sub, sub+8, ...} of all 9
// taps (one pixel's 8 threads read 128 contiguous bytes; neighbouring pixels re-read the same rows out of L1); the whole
// filter (cout*9*cin halfs, <= 23 KB) sits in LDS and is read as broadcasts; products by v_dot2_f32_f16; the 8 partial sums
// of a pixel meet through three lane-xor steps.  (The first version - one wave per pixel, weights from global - spent
// 109 us on the UNet's 65536 x 320 -> 4 launch.)
// CPT: 16-byte channel chunks per thread (cin = 64 * CPT) - the chunk loads of a tap are issued together and the next tap's
// loads are in flight while the current tap is multiplied (45 dependent load -> use round trips per thread otherwise).
template <int COUT, int CPT>
__global__ __launch_bounds__(256, 4) void conv_out_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, int batch, int cin,
                                                       int h, int wd) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    half_t* sw = reinterpret_cast<half_t*>(smem_raw);
    const int tid = threadIdx.x;
    const int wtot = COUT * 9 * cin;
    for (int i = tid * 8; i < wtot; i += 256 * 8) *reinterpret_cast<half8_t*>(sw + i) = *reinterpret_cast<const half8_t*>(w + i);
    __syncthreads();
    const int sub = tid & 7;
    const long total = (long)batch * h * wd;
    // grid-stride over 32-pixel groups: the LDS filter fill (as many bytes as 36 pixels of input) is paid once per workgroup
    for (long grp = blockIdx.x; grp * 32 < total; grp += gridDim.x) {
    const long pix_raw = grp * 32 + (tid >> 3);
    const bool ok = pix_raw < total;
    const long pix = ok ? pix_raw : total - 1;
    const int b = (int)(pix / (h * wd));
    const int rem = (int)(pix - (long)b * h * wd);
    const int y = rem / wd, xx = rem - y * wd;
    float acc[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = 0.f;
    auto load_tap = [&](int tap, half8_t (&v)[CPT]) {
        const int iy = y + tap / 3 - 1, ix = xx + tap % 3 - 1;
        const bool in = iy >= 0 && iy < h && ix >= 0 && ix < wd;
        const half_t* xr = x + ((long)(b * h + (in ? iy : y)) * wd + (in ? ix : xx)) * cin;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            v[i] = *reinterpret_cast<const half8_t*>(xr + (sub + i * 8) * 8);
            if (!in) v[i] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    auto mac_tap = [&](int tap, const half8_t (&v)[CPT]) {
        const half_t* wr = sw + tap * cin;
#pragma unroll
        for (int i = 0; i < CPT; ++i)
#pragma unroll
            for (int c = 0; c < COUT; ++c) {
                const half8_t ww = *reinterpret_cast<const half8_t*>(wr + c * 9 * cin + (sub + i * 8) * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[c] = __builtin_amdgcn_fdot2(half2_t{v[i][2 * j], v[i][2 * j + 1]}, half2_t{ww[2 * j], ww[2 * j + 1]}, acc[c], false);
            }
    };
    half8_t va[CPT], vb[CPT];
    load_tap(0, va);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {      // rolled: fully unrolled, hipcc hoists every load / LDS read and spills (916 B scratch)
        load_tap(min(tap + 1, 8), vb);
        mac_tap(tap, va);
#pragma unroll
        for (int i = 0; i < CPT; ++i) va[i] = vb[i];
    }
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
        acc[c] += __shfl_xor(acc[c], 1, 64);
        acc[c] += __shfl_xor(acc[c], 2, 64);
        acc[c] += __shfl_xor(acc[c], 4, 64);
    }
    if (ok && sub < COUT) {
        float v = acc[0];
#pragma unroll
        for (int c = 1; c < COUT; ++c) v = (sub == c) ? acc[c] : v;
        out[(((long)b * COUT + sub) * h + y) * wd + xx] = v + (bias ? bias[sub] : 0.f);
    }
    }
}

template <int COUT>
int launch_conv_out(const half_t* x, const half_t* w, const float* bias, float* out, int batch, int cin, int h, int wd, hipStream_t stream) {
    const long pix = (long)batch * h * wd;
    const size_t smem = (size_t)COUT * 9 * cin * sizeof(half_t);
    const long groups = (pix + 31) / 32;
    const long per_cu = smem ? (long)(160 * 1024 / smem) : 8;                     // workgroups per CU that fit (LDS, <= 8 by waves)
    const long cap = 256 * (per_cu < 8 ? per_cu : 8);
    const dim3 grid((unsigned)(groups < cap ? groups : cap)), block(256);
    switch (cin / 64) {
        case 1: hipLaunchKernelGGL((conv_out_kernel<COUT, 1>), grid, block, smem, stream, x, w, bias, out, batch, cin, h, wd); break;
        case 2: hipLaunchKernelGGL((conv_out_kernel<COUT, 2>), grid, block, smem, stream, x, w, bias, out, batch, cin, h, wd); break;
        case 4: hipLaunchKernelGGL((conv_out_kernel<COUT, 4>), grid, block, smem, stream, x, w, bias, out, batch, cin, h, wd); break;
        case 5: hipLaunchKernelGGL((conv_out_kernel<COUT, 5>), grid, block, smem, stream, x, w, bias, out, batch, cin, h, wd); break;
        case 8: hipLaunchKernelGGL((conv_out_kernel<COUT, 8>), grid, block, smem, stream, x, w, bias, out, batch, cin, h, wd); break;
        default: return (int)hipErrorInvalidValue;
    }
    return PV_CHECK_LAUNCH();
}

__global__ void geglu_kernel(const half_t* x, int ldx, half_t* out, int ldo, int rows, int n) {
    const int nchunk = n >> 3;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * nchunk) return;
    const int ch = (int)(idx % nchunk);
    const long r = idx / nchunk;
    const half8_t a = *reinterpret_cast<const half8_t*>(x + r * ldx + ch * 8);
    const half8_t g = *reinterpret_cast<const half8_t*>(x + r * ldx + n + ch * 8);
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)a[j] * pv_gelu_erf((float)g[j]));
    *reinterpret_cast<half8_t*>(out + r * ldo + ch * 8) = o;
}

// coef row (8 floats): {ca, cb, cx, c0, c1, -, -, -}
//   eps = eps_u + g (eps_c - eps_u)              infer.py:116
//   x0  = ca*x + cb*eps                          epsilon -> data prediction
//   x'  = cx*x + c0*x0 + c1*x0_prev              DPM-Solver++ 1st / 2nd order (midpoint)
__global__ void cfg_dpm_step_kernel(const float* eu, const float* ec, float* lat, float* x0p, const float* coef,
                                    const int32_t* state, float g, long n) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = coef + (long)pv_step_index(state) * 8;
    const float ca = c[0], cb = c[1], cx = c[2], c0 = c[3], c1 = c[4];
    const float4_t u = *reinterpret_cast<const float4_t*>(eu + i);
    const float4_t cc = *reinterpret_cast<const float4_t*>(ec + i);
    float4_t x = *reinterpret_cast<const float4_t*>(lat + i);
    float4_t xp = *reinterpret_cast<const float4_t*>(x0p + i);
    float4_t x0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float e = u[j] + g * (cc[j] - u[j]);
        x0[j] = ca * x[j] + cb * e;
        x[j] = cx * x[j] + c0 * x0[j] + c1 * xp[j];
    }
    *reinterpret_cast<float4_t*>(lat + i) = x;
    *reinterpret_cast<float4_t*>(x0p + i) = x0;
}

// a*x + b*y with each product and the sum rounded on its own: what fp32 host arithmetic computes (hipcc contracts a*x + b*y into a multiply-add otherwise)
__device__ __forceinline__ float pv_axpby_unfused(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    return a * x + b * y;
}

// cfg_dpm_step_kernel + the 4-channel inpainting blend of the step's result with the known latents noised to the NEXT timestep:
// coef row {ca, cb, cx, c0, c1, q0, q1, -}
//   xn = cx*x + c0*x0 + c1*x0_prev               the step above, same expressions (m == 1 reproduces its bits)
//   k  = q0*known + q1*noise                     add_noise(known, noise, t_next); (q0, q1) = (1, 0) on the last row
//   x' = m*xn + (1-m)*k                          two products: m == 1 -> xn, m == 0 -> k, exactly
// k is rounded product by product (pv_axpby_unfused) so that fp32 host arithmetic reproduces the kept region bit for bit.
// mask [B][1][hw] is broadcast over the channels; hw % 4 == 0, so the four elements of a thread share one plane.  x0_prev gets the unblended x0.
__global__ void cfg_dpm_step_masked_kernel(const float* eu, const float* ec, float* lat, float* x0p, const float* coef, const int32_t* state,
                                           float g, const float* __restrict__ mask, const float* __restrict__ known,
                                           const float* __restrict__ noise, long chw, int hw, long n) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float* c = coef + (long)pv_step_index(state) * 8;
    const float ca = c[0], cb = c[1], cx = c[2], c0 = c[3], c1 = c[4], q0 = c[5], q1 = c[6];
    const long b = i / chw;
    const int px = (int)((i - b * chw) % hw);
    const float4_t u = *reinterpret_cast<const float4_t*>(eu + i);
    const float4_t cc = *reinterpret_cast<const float4_t*>(ec + i);
    const float4_t m = *reinterpret_cast<const float4_t*>(mask + b * hw + px);
    const float4_t kn = *reinterpret_cast<const float4_t*>(known + i);
    const float4_t nz = *reinterpret_cast<const float4_t*>(noise + i);
    float4_t x = *reinterpret_cast<const float4_t*>(lat + i);
    float4_t xp = *reinterpret_cast<const float4_t*>(x0p + i);
    float4_t x0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float e = u[j] + g * (cc[j] - u[j]);
        x0[j] = ca * x[j] + cb * e;
        const float xn = cx * x[j] + c0 * x0[j] + c1 * xp[j];
        const float k = pv_axpby_unfused(q0, kn[j], q1, nz[j]);
        x[j] = m[j] * xn + (1.f - m[j]) * k;
    }
    *reinterpret_cast<float4_t*>(lat + i) = x;
    *reinterpret_cast<float4_t*>(x0p + i) = x0;
}

// Philox4x32-10 (Salmon et al. 2011): counter-based - a draw is a function of (key, counter) alone, no stored stream
struct philox_block { uint32_t w[4]; };
__device__ __forceinline__ philox_block philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return philox_block{{c0, c1, c2, c3}};
}

// Four standard normals from one Philox block by Box-Muller (part of pv_cfg_dpm_step_stochastic's interface, restated in numpy by the tests):
//   u_k = ((w_k >> 9) + 0.5) * 2^-23      exact in fp32, strictly inside (0, 1): the logarithm is finite
//   z0, z1 = sqrt(-2 ln u0) * (cos, sin)(2 pi u1);   z2, z3 = sqrt(-2 ln u2) * (cos, sin)(2 pi u3)
// sincospif(2 u) reduces the argument exactly (no rounded 2 pi); logf / sqrtf are the accurate ones.
__device__ __forceinline__ float4_t pv_normal4(const philox_block& p) {
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = ((float)(p.w[k] >> 9) + 0.5f) * (1.0f / 8388608.0f);
    const float r0 = sqrtf(-2.f * logf(u[0])), r1 = sqrtf(-2.f * logf(u[2]));
    float s0, c0, s1, c1;
    sincospif(2.f * u[1], &s0, &c0);
    sincospif(2.f * u[3], &s1, &c1);
    return float4_t{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

// Sum of a and of b over the workgroup, returned to every thread: __shfl_down inside the wave, one LDS slot per wave, then every thread adds the
// slots in wave order.  No atomics and a fixed order: a graph replay gives the bits of an eager run.  slots: 2 x 16 floats no other reduction uses.
__device__ __forceinline__ void pv_block_sum2(float& a, float& b, float* slots) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        slots[wave] = a;
        slots[16 + wave] = b;
    }
    __syncthreads();
    a = 0.f;
    b = 0.f;
    for (int w = 0; w < nwaves; ++w) {
        a += slots[w];
        b += slots[16 + w];
    }
}

// The guided noise prediction: the two-term CFG of cfg_dpm_step_kernel (same expression), or with an image-only forward em = eps(uncond text, image
// tokens) the split of [EXT] InstructPix2Pix  eu + g_image (em - eu) + g_text (ec - em)
template <bool IMG>
__device__ __forceinline__ float pv_guided_eps(float u, float m, float c, float gt, float gi) {
    if (IMG) return u + gi * (m - u) + gt * (c - m);
    return u + gt * (c - u);
}

// [EXT] Perturbed-attention guidance (Ahn et al. 2024) on top of the guided prediction: ep = eps of the conditional forward whose chosen self-attention
// maps are the identity;  e = e0 + g_pag (ec - ep).  PAG = false is pv_guided_eps itself (ep is not read).
template <bool IMG, bool PAG>
__device__ __forceinline__ float pv_guided_eps_pag(float u, float m, float c, float p, float gt, float gi, float gp) {
    const float e0 = pv_guided_eps<IMG>(u, m, c, gt, gi);
    if (PAG) return e0 + gp * (c - p);
    return e0;
}

// cfg_dpm_step_kernel / cfg_dpm_step_masked_kernel with the guided prediction above and [EXT] diffusers' guidance_rescale:
//   f  = rescale * std_b(ec) / std_b(e) + (1 - rescale)      per sample b over its chw elements (f = 1 where std_b(e) == 0)
//   e  = f * e;  x0, xn, the blend: the expressions of the two kernels above (IMG = RESCALE = NOISE = false reproduces their bits)
// NOISE (pv_cfg_dpm_step_stochastic, the SDE form of the solver): xn += cn * z before the blend, cn = column 7 of the row, z the four normals of the
// Philox block keyed (rng[0], rng[1]) at counter (float4 index inside the sample, rng[2] + sample, step index, rng[3]).  Everything z depends
// on is contents of device buffers, so a captured launch serves any seed / start row / batch offset, and a replay gives the bits of an eager run.
// PAG (pv_cfg_dpm_step_pag): e is pv_guided_eps_pag - the statistics of the rescale are those of that e; everything behind e is unchanged.
// One workgroup per sample, so the statistics need no second launch and no scratch: mean first, then the squared deviations (noise
// predictions are not zero-mean), both passes over eps_* only; the last pass recomputes e and writes latents / x0_prev in place.
template <bool IMG, bool RESCALE, bool MASK, bool NOISE, bool PAG>
__global__ __launch_bounds__(1024) void cfg_dpm_step_guided_kernel(const float* eu, const float* em, const float* ec, const float* ep, float* lat,
                                                                   float* x0p, const float* coef, const int32_t* state,
                                                                   const uint32_t* __restrict__ rng, float gt, float gi, float gp, float rescale,
                                                                   const float* __restrict__ mask,
                                                                   const float* __restrict__ known, const float* __restrict__ noise, long chw,
                                                                   int hw) {
    __shared__ float red[4 * 16];
    const long base = (long)blockIdx.x * chw;
    const int nv = (int)(chw >> 2);
    float f = 1.f;
    if (RESCALE) {
        float sc = 0.f, se = 0.f;
        for (int v = threadIdx.x; v < nv; v += blockDim.x) {
            const long i = base + (long)v * 4;
            const float4_t u = *reinterpret_cast<const float4_t*>(eu + i);
            const float4_t cc = *reinterpret_cast<const float4_t*>(ec + i);
            const float4_t mm = IMG ? *reinterpret_cast<const float4_t*>(em + i) : u;
            const float4_t pp = PAG ? *reinterpret_cast<const float4_t*>(ep + i) : cc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sc += cc[j];
                se += pv_guided_eps_pag<IMG, PAG>(u[j], mm[j], cc[j], pp[j], gt, gi, gp);
            }
        }
        pv_block_sum2(sc, se, red);
        const float mc = sc / (float)chw, me = se / (float)chw;
        float qc = 0.f, qe = 0.f;
        for (int v = threadIdx.x; v < nv; v += blockDim.x) {
            const long i = base + (long)v * 4;
            const float4_t u = *reinterpret_cast<const float4_t*>(eu + i);
            const float4_t cc = *reinterpret_cast<const float4_t*>(ec + i);
            const float4_t mm = IMG ? *reinterpret_cast<const float4_t*>(em + i) : u;
            const float4_t pp = PAG ? *reinterpret_cast<const float4_t*>(ep + i) : cc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dc = cc[j] - mc, de = pv_guided_eps_pag<IMG, PAG>(u[j], mm[j], cc[j], pp[j], gt, gi, gp) - me;
                qc += dc * dc;
                qe += de * de;
            }
        }
        pv_block_sum2(qc, qe, red + 32);
        if (qe > 0.f) f = rescale * (sqrtf(qc) / sqrtf(qe)) + (1.f - rescale);
    }
    const int step = pv_step_index(state);
    const float* c = coef + (long)step * 8;
    const float ca = c[0], cb = c[1], cx = c[2], c0 = c[3], c1 = c[4], q0 = c[5], q1 = c[6];
    float cn = 0.f;
    uint32_t k0 = 0u, k1 = 0u, sample = 0u, stream = 0u;
    if (NOISE) {
        cn = c[7];
        k0 = rng[0]; k1 = rng[1]; sample = rng[2] + blockIdx.x; stream = rng[3];
    }
    for (int v = threadIdx.x; v < nv; v += blockDim.x) {
        const int o = v * 4;
        const long i = base + o;
        const float4_t u = *reinterpret_cast<const float4_t*>(eu + i);
        const float4_t cc = *reinterpret_cast<const float4_t*>(ec + i);
        const float4_t mm = IMG ? *reinterpret_cast<const float4_t*>(em + i) : u;
        const float4_t pp = PAG ? *reinterpret_cast<const float4_t*>(ep + i) : cc;
        float4_t x = *reinterpret_cast<const float4_t*>(lat + i);
        float4_t xp = *reinterpret_cast<const float4_t*>(x0p + i);
        float4_t x0;
        float4_t z = {0.f, 0.f, 0.f, 0.f};
        if (NOISE) z = pv_normal4(philox4x32_10(k0, k1, (uint32_t)v, sample, (uint32_t)step, stream));
        if (MASK) {
            const float4_t m = *reinterpret_cast<const float4_t*>(mask + (long)blockIdx.x * hw + o % hw);
            const float4_t kn = *reinterpret_cast<const float4_t*>(known + i);
            const float4_t nz = *reinterpret_cast<const float4_t*>(noise + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e = pv_guided_eps_pag<IMG, PAG>(u[j], mm[j], cc[j], pp[j], gt, gi, gp);
                if (RESCALE) e = f * e;
                x0[j] = ca * x[j] + cb * e;
                float xn = cx * x[j] + c0 * x0[j] + c1 * xp[j];
                if (NOISE) xn += cn * z[j];
                const float k = pv_axpby_unfused(q0, kn[j], q1, nz[j]);
                x[j] = m[j] * xn + (1.f - m[j]) * k;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float e = pv_guided_eps_pag<IMG, PAG>(u[j], mm[j], cc[j], pp[j], gt, gi, gp);
                if (RESCALE) e = f * e;
                x0[j] = ca * x[j] + cb * e;
                x[j] = cx * x[j] + c0 * x0[j] + c1 * xp[j];
                if (NOISE) x[j] += cn * z[j];
            }
        }
        *reinterpret_cast<float4_t*>(lat + i) = x;
        *reinterpret_cast<float4_t*>(x0p + i) = x0;
    }
}

// out = clamp(m*gen + (1-m)*orig, lo, hi) over NCHW fp32 images, mask [B][1][hw] broadcast over the channels (hw % 4 == 0); out may be gen
__global__ void composite_clamp_kernel(const float* gen, const float* __restrict__ orig, const float* __restrict__ mask, float* out, float lo, float hi,
                                       long chw, int hw, long n) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const long b = i / chw;
    const int px = (int)((i - b * chw) % hw);
    const float4_t gv = *reinterpret_cast<const float4_t*>(gen + i);
    const float4_t ov = *reinterpret_cast<const float4_t*>(orig + i);
    const float4_t m = *reinterpret_cast<const float4_t*>(mask + b * hw + px);
    float4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(m[j] * gv[j] + (1.f - m[j]) * ov[j], lo), hi);
    *reinterpret_cast<float4_t*>(out + i) = o;
}

__global__ void step_advance_kernel(int32_t* state) { state[0] += 1; }

// the draws of pv_fusion_draw: counter (c0, c1, 0, 0), first word of the block
__device__ __forceinline__ uint32_t philox_first_word(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1) {
    return philox4x32_10(k0, k1, c0, c1, 0u, 0u).w[0];
}

__global__ void fusion_draw_kernel(const int32_t* state, uint32_t* rng, const float* forced, float* out, int n, float r1, float r2,
                                   float scale, int only_last) {
    const int i = threadIdx.x;
    const uint32_t call = rng[2];
    float wt = 1.f, wi = 1.f;
    const bool on = !(only_last && state) || state[0] == state[1] - 1;
    if (i < n && on) {
        float u = (float)(philox_first_word(rng[0], rng[1], call, (uint32_t)i) >> 8) * (1.0f / 16777216.0f);   // [0, 1)
        if (forced && forced[i] >= 0.f) u = forced[i];
        if (u < r1) { wt = scale; wi = 0.f; }
        else if (u > r2) { wt = 0.f; wi = scale; }
    }
    if (i < n) { out[2 * i] = wt; out[2 * i + 1] = wi; }
    __syncthreads();
    if (i == 0) rng[2] = call + 1u;
}

__global__ void cast_f32_f16_kernel(const float* x, half_t* y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (half_t)x[i];
}
__global__ void cast_f16_f32_kernel(const half_t* x, float* y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];
}

// one workgroup = one group x 32 eight-column chunks x 8 row lanes: lane l sums rows l, l + 8, ...; the eight partial sums are added in lane
// order (fixed).  16 groups x 257 rows x 1024 columns: 78 -> ~10 us against one thread walking all rows of its chunk.
__global__ __launch_bounds__(256) void rows_mean_kernel(const half_t* x, int ldx, half_t* y, int ldy, int groups, int count, int group_rows, int cols,
                                                        int accumulate) {
    __shared__ float part[8][32][9];
    const int nchunk = cols >> 3, cpb = (nchunk + 31) / 32;
    const int g = blockIdx.x / cpb, ch = (blockIdx.x % cpb) * 32 + (threadIdx.x & 31), rl = threadIdx.x >> 5;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (ch < nchunk)
        for (int r = rl; r < count; r += 8) {
            const half8_t v = *reinterpret_cast<const half8_t*>(x + ((long)g * group_rows + r) * ldx + ch * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[rl][threadIdx.x & 31][j] = acc[j];
    __syncthreads();
    if (rl != 0 || ch >= nchunk) return;
#pragma unroll
    for (int k = 1; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += part[k][threadIdx.x & 31][j];
    half_t* yo = y + (long)g * ldy + ch * 8;
    half8_t o;
    half8_t prev = accumulate ? *reinterpret_cast<const half8_t*>(yo) : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)(acc[j] / (float)count + (float)prev[j]);
    *reinterpret_cast<half8_t*>(yo) = o;
}

// im2col of a 3x3 / pad 1 convolution over an NCHW fp32 tensor with few channels (the UNet's conv_in, cin = 4):
// rows [B*H*W][kpad] fp16, column k = ci*9 + ky*3 + kx (the flattened Conv2d weight order), zero padded to kpad.
// The conv itself then runs on the MFMA GEMM.
__global__ void im2col3x3_kernel(const float* __restrict__ x, half_t* __restrict__ out, int batch, int cin, int h, int wd, int kpad) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // one thread = 8 consecutive columns of one row
    const int nch = kpad >> 3;
    if (idx >= (long)batch * h * wd * nch) return;
    const int ch = (int)(idx % nch);
    const long pix = idx / nch;
    const int b = (int)(pix / (h * wd));
    const int rem = (int)(pix - (long)b * h * wd);
    const int y = rem / wd, xx = rem - y * wd;
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = ch * 8 + j;
        float v = 0.f;
        if (k < cin * 9) {
            const int ci = k / 9, t = k - ci * 9;
            const int iy = y + t / 3 - 1, ix = xx + t % 3 - 1;
            if (iy >= 0 && iy < h && ix >= 0 && ix < wd) v = x[(((long)b * cin + ci) * h + iy) * wd + ix];
        }
        o[j] = (half_t)v;
    }
    *reinterpret_cast<half8_t*>(out + pix * kpad + ch * 8) = o;
}

// in-place row softmax of fp16 scores: x[r][c] = softmax_c(scale * x[r][c]); one 256-thread workgroup per row, fp32 math
__global__ __launch_bounds__(256) void softmax_rows_kernel(half_t* __restrict__ x, int ld, int cols, float scale) {
    __shared__ float red[4];
    half_t* row = x + (size_t)blockIdx.x * ld;
    const int nch = cols >> 3, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float sl2 = scale * 1.4426950408889634f;
    float mx = -INFINITY;
    for (int ch = threadIdx.x; ch < nch; ch += 256) {
        const half8_t v = *reinterpret_cast<const half8_t*>(row + ch * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, (float)v[j]);
    }
    mx = pv_wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * sl2;
    __syncthreads();
    float sum = 0.f;
    for (int ch = threadIdx.x; ch < nch; ch += 256) {
        const half8_t v = *reinterpret_cast<const half8_t*>(row + ch * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += __builtin_amdgcn_exp2f(fmaf((float)v[j], sl2, -mx));
    }
    sum = pv_wave_sum(sum);
    if (lane == 0) red[wv] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int ch = threadIdx.x; ch < nch; ch += 256) {
        const half8_t v = *reinterpret_cast<const half8_t*>(row + ch * 8);
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(__builtin_amdgcn_exp2f(fmaf((float)v[j], sl2, -mx)) * inv);
        *reinterpret_cast<half8_t*>(row + ch * 8) = o;
    }
}

// 1x1 convolution over an NCHW fp32 tensor with few channels (VAE post_quant_conv, 4 -> 4)
__global__ void pointwise_nchw_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                      float* __restrict__ out, int batch, int cin, int cout, int hw) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)batch * hw) return;
    const int b = (int)(idx / hw), px = (int)(idx - (long)b * hw);
    for (int co = 0; co < cout; ++co) {
        float acc = bias ? bias[co] : 0.f;
        for (int ci = 0; ci < cin; ++ci) acc += w[co * cin + ci] * x[((long)b * cin + ci) * hw + px];
        out[((long)b * cout + co) * hw + px] = acc;
    }
}

__global__ void clamp_f32_kernel(float* x, float lo, float hi, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = fminf(fmaxf(x[i], lo), hi);
}

// CLIP ViT patchify: NCHW fp32 pixels -> fp16 rows [B*gh*gw][kpad], row = one patch flattened (c, py, px), zero padded
__global__ void patchify_kernel(const float* __restrict__ x, half_t* __restrict__ out, int batch, int ch, int img, int patch, int kpad) {
    const int g = img / patch;
    const long total = (long)batch * g * g * kpad;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % kpad);
    const long row = idx / kpad;
    float v = 0.f;
    if (k < ch * patch * patch) {
        const int c = k / (patch * patch), r = k - c * patch * patch;
        const int py = r / patch, px = r - py * patch;
        const int b = (int)(row / (g * g)), pr = (int)(row - (long)b * g * g);
        const int gy = pr / g, gx = pr - gy * g;
        v = x[(((long)b * ch + c) * img + gy * patch + py) * img + gx * patch + px];
    }
    out[idx] = (half_t)v;
}

// CLIP vision embeddings: out[b][0] = cls + pos[0]; out[b][1+i] = patch[b][i] + pos[1+i]     (fp16 rows, fp32 params)
__global__ void vision_embed_kernel(const half_t* __restrict__ patches, const float* __restrict__ cls, const float* __restrict__ pos,
                                    half_t* __restrict__ out, int batch, int ntok, int dim) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)batch * ntok * dim) return;
    const int d = (int)(idx % dim);
    const long row = idx / dim;
    const int t = (int)(row % ntok), b = (int)(row / ntok);
    const float v = t == 0 ? cls[d] : (float)patches[((long)b * (ntok - 1) + (t - 1)) * dim + d];
    out[idx] = (half_t)(v + pos[(long)t * dim + d]);
}

// CLIP text embeddings with PhotoVerse concept injection (models/clip.py:17-24,57-63), one thread per element:
//   j <  idx       : tok[ids[b][j]]
//   idx<=j<idx+E   : concept[b][j-idx]
//   j >= idx+E     : tok[ids[b][j-E+1]]          (tail shifted right by E-1, truncated)
// then + pos[j].  E == 0 (no concept) is the stock embedding.
__global__ void text_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                  const half_t* __restrict__ concept, const int64_t* __restrict__ pidx, int E, half_t* __restrict__ out,
                                  int batch, int seq, int dim) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)batch * seq * dim) return;
    const int d = (int)(i % dim);
    const long row = i / dim;
    const int j = (int)(row % seq), b = (int)(row / seq);
    float v;
    const int idx = E > 0 ? (int)pidx[b] : seq;
    if (j < idx) v = tok[ids[(long)b * seq + j] * dim + d];
    else if (j < idx + E) v = (float)concept[((long)b * E + (j - idx)) * dim + d];
    else v = tok[ids[(long)b * seq + (j - E + 1)] * dim + d];
    out[i] = (half_t)(v + pos[(long)j * dim + d]);
}

}  // namespace

extern "C" int pv_im2col3x3(const float* x, void* out, int32_t batch, int32_t cin, int32_t h, int32_t wd, int32_t kpad, void* stream) {
    if (batch <= 0 || cin <= 0 || h <= 0 || wd <= 0 || (kpad % 8) || kpad < cin * 9 || !x || !out) return (int)hipErrorInvalidValue;
    const long total = (long)batch * h * wd * (kpad / 8);
    hipLaunchKernelGGL(im2col3x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<half_t*>(out), batch, cin, h, wd, kpad);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_softmax_rows(void* x, int32_t ld, int32_t rows, int32_t cols, float scale, void* stream) {
    if (rows <= 0 || cols <= 0 || (cols % 8) || (ld % 8) || !x) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<half_t*>(x), ld, cols, scale);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_pointwise_nchw(const float* x, const float* w, const float* bias, float* out, int32_t batch, int32_t cin, int32_t cout,
                                 int32_t hw, void* stream) {
    if (batch <= 0 || cin <= 0 || cout <= 0 || hw <= 0 || !x || !w || !out) return (int)hipErrorInvalidValue;
    const long total = (long)batch * hw;
    hipLaunchKernelGGL(pointwise_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w, bias, out,
                       batch, cin, cout, hw);
    return PV_CHECK_LAUNCH();
}

namespace {
// out[b][i] = ca[b] * x[b][i] + cb[b] * y[b][i]   (per-sample coefficients; y / cb may be NULL: out = ca[b] * x)
__global__ void affine_rows_kernel(const float* x, const float* y, const float* ca, const float* cb, float* out, long per, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long b = i / per;
    float v = ca[b] * x[i];
    if (y) v += cb[b] * y[i];
    out[i] = v;
}
// one axis of F.interpolate(mode="bilinear", align_corners=False): src = max((dst + 0.5) * in / out - 0.5, 0) = max(((2 dst + 1) in - out) / (2 out), 0).
// The numerator is an exact integer in fp64 (in, out < 2^29), so the only rounding is the division's: at in == out it is dst itself and the weight exactly 0.
__device__ __forceinline__ void bilinear_taps(int dst, int in, int out, int& i0, int& i1, float& wt) {
    const double src = fmax(((2.0 * dst + 1.0) * in - out) / (2.0 * out), 0.0);
    i0 = min((int)src, in - 1);
    i1 = min(i0 + 1, in - 1);
    wt = (float)(src - (double)i0);
}
// weight 0 returns a itself (also when b is not finite, and with the sign of a zero)
__device__ __forceinline__ float bilinear_mix(float a, float b, float wt) { return wt == 0.f ? a : (1.f - wt) * a + wt * b; }

// out[b][c] = ca[b] * bilinear(x[b][c]: h x w -> oh x ow) (+ cb[b] * y[b][c]) over NCHW fp32; ca NULL = 1.  V outputs of one row per thread:
// V = 4 (ow % 4 == 0, y / out 16-byte aligned) reads y and writes out as float4; V = 1 takes every other shape.  x is gathered: 4 taps per output.
template <int V>
__global__ void resize_bilinear_affine_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ ca,
                                              const float* __restrict__ cb, float* __restrict__ out, int channels, int h, int w, int oh, int ow, int n) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i >= n) return;
    const int row = i / ow, ox = i - row * ow;          // V divides ow: the V outputs share the row
    const int plane = row / oh, oy = row - plane * oh;
    const int b = plane / channels;
    int y0, y1;
    float wy;
    bilinear_taps(oy, h, oh, y0, y1, wy);
    const float* r0 = x + ((long)plane * h + y0) * w;
    const float* r1 = x + ((long)plane * h + y1) * w;
    const float a = ca ? ca[b] : 1.f;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int x0, x1;
        float wx;
        bilinear_taps(ox + j, w, ow, x0, x1, wx);
        const float r = bilinear_mix(bilinear_mix(r0[x0], r0[x1], wx), bilinear_mix(r1[x0], r1[x1], wx), wy);
        v[j] = ca ? a * r : r;
    }
    if constexpr (V == 4) {
        float4_t o = {v[0], v[1], v[2], v[3]};
        if (y) {
            const float4_t yv = *reinterpret_cast<const float4_t*>(y + i);
            const float c = cb[b];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += c * yv[j];
        }
        *reinterpret_cast<float4_t*>(out + i) = o;
    } else {
        out[i] = y ? v[0] + cb[b] * y[i] : v[0];
    }
}
// posterior sample of the VAE encoder: out = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps; moments = [B][2c][hw] (mean | logvar)
__global__ void posterior_sample_kernel(const float* moments, const float* eps, float* out, long chw, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long b = i / chw, r = i - b * chw;
    const float mean = moments[b * 2 * chw + r];
    const float logvar = fminf(fmaxf(moments[b * 2 * chw + chw + r], -30.f), 20.f);
    out[i] = mean + __expf(0.5f * logvar) * eps[i];
}
// stage 1 of a deterministic mean: block partial sums of f(a, b); mode 0: a, 1: |a|, 2: (a - b)^2, 3: a^2.  a / b: fp32, or fp16 when f16 != 0
__global__ __launch_bounds__(256) void reduce_partial_kernel(const void* a_, const void* b_, int mode, int f16, long n, float* partial) {
    __shared__ float red[4];
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float a = f16 ? (float)reinterpret_cast<const half_t*>(a_)[i] : reinterpret_cast<const float*>(a_)[i];
        if (mode == 0) acc += a;
        else if (mode == 1) acc += fabsf(a);
        else if (mode == 3) acc += a * a;
        else {
            const float b = f16 ? (float)reinterpret_cast<const half_t*>(b_)[i] : reinterpret_cast<const float*>(b_)[i];
            acc += (a - b) * (a - b);
        }
    }
    acc = pv_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void reduce_final_kernel(const float* partial, int nb, float scale, float* out) {
    float acc = 0.f;
    for (int i = 0; i < nb; ++i) acc += partial[i];     // fixed order
    out[0] = acc * scale;
}
}  // namespace

extern "C" int pv_affine_rows_f32(const float* x, const float* y, const float* ca, const float* cb, float* out, int64_t per_sample, int32_t batch,
                                  void* stream) {
    if (!x || !ca || !out || per_sample <= 0 || batch <= 0 || (y && !cb)) return (int)hipErrorInvalidValue;
    const long n = (long)per_sample * batch;
    hipLaunchKernelGGL(affine_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, ca, cb, out, (long)per_sample, n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_resize_bilinear_affine_f32(const float* x, const float* y, const float* ca, const float* cb, float* out, int32_t batch,
                                             int32_t channels, int32_t h, int32_t w, int32_t oh, int32_t ow, void* stream) {
    if (!x || !out || batch <= 0 || channels <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || ((y != nullptr) != (cb != nullptr)))
        return (int)hipErrorInvalidValue;
    // every operand below 2 GiB = 2^29 floats (so the kernel indexes with int); checked factor by factor, the full product may not fit 64 bits
    const int64_t lim = (int64_t)1 << 29, planes = (int64_t)batch * channels;
    if (planes >= lim || planes * h >= lim || planes * h * w >= lim || planes * oh >= lim || planes * oh * ow >= lim) return (int)hipErrorInvalidValue;
    const int n = (int)(planes * oh * ow);
    const bool vec = (ow % 4) == 0 && (reinterpret_cast<uintptr_t>(out) % 16) == 0 && (reinterpret_cast<uintptr_t>(y) % 16) == 0;
    if (vec)
        hipLaunchKernelGGL(resize_bilinear_affine_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, ca, cb, out,
                           channels, h, w, oh, ow, n);
    else
        hipLaunchKernelGGL(resize_bilinear_affine_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, ca, cb, out,
                           channels, h, w, oh, ow, n);
    return PV_CHECK_LAUNCH();
}

namespace {
// FreeU on the two inputs of one decoder ResnetBlock (header: pv_freeu_rows).  256 threads = 16 channel chunks of 8 (a thread's 16-byte load; the
// 16 chunks of a row are 256 contiguous bytes) x 16 pixel lanes.
// Blocks [0, skip_blocks): one (image, 128-channel group) of the skip each.  Pass 1: every thread walks the pixels lane, lane + 16, ... of its
// chunk and accumulates the seven sums S0, sum p cos/sin(c), sum p cos/sin(a), sum p cos/sin(a + c)  (a = 2 pi y/h, c = 2 pi x/w) in fp32; the 16
// lanes' partials meet in LDS and are added in lane order.  Pass 2 reads the same pixels again (the plane is at most a few hundred KB: L2) and
// stores  p + k (S0 + Cc cos c + Sc sin c + Ca cos a + Sa sin a + Cac cos(a + c) + Sac sin(a + c)),  k = (s - 1)/(h w):  with
// X[0,-1] = Cc + i Sc, X[-1,0] = Ca + i Sa, X[-1,-1] = Cac + i Sac that is the header's sum of Re(X[u,v] exp(+2 pi i (u y/h + v x/w))).
// Every sum depends on the plane alone - not on the batch, the grid or the other half - so a plane has the same bits in every launch that holds it.
// Blocks from skip_blocks on: the backbone half, one chunk per thread.
constexpr int FREEU_CHUNKS = 16, FREEU_LANES = 16, FREEU_COLS = FREEU_CHUNKS * 8;

__device__ __forceinline__ void freeu_trig(int p, int w, float inv_h, float inv_w, float (&t)[6]) {
    const int y = p / w, x = p - y * w;
    float sa, ca, sc, cc;
    sincospif(2.f * (float)y * inv_h, &sa, &ca);          // y < h: the argument is below 2; y = h/2 gives exactly (0, -1)
    sincospif(2.f * (float)x * inv_w, &sc, &cc);
    t[0] = cc; t[1] = sc; t[2] = ca; t[3] = sa;
    t[4] = ca * cc - sa * sc;                             // cos(a + c)
    t[5] = sa * cc + ca * sc;                             // sin(a + c)
}

__global__ __launch_bounds__(256) void freeu_rows_kernel(const half_t* __restrict__ x, int ldx, int cx, half_t* __restrict__ xo, int ldxo, float b,
                                                         long x_chunks, const half_t* __restrict__ sk, int lds, int cs, half_t* __restrict__ so,
                                                         int ldso, float s, int h, int w, int groups, int skip_blocks) {
    __shared__ __attribute__((aligned(16))) float part[2][FREEU_LANES][FREEU_COLS];     // 16 KB: one sum's partials, double buffered
    __shared__ __attribute__((aligned(16))) float tot[7][FREEU_COLS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= skip_blocks) {
        const long i = (long)((int)blockIdx.x - skip_blocks) * 256 + tid;
        if (i >= x_chunks) return;
        const int cpr = cx >> 3;
        const long r = i / cpr;
        const int c0 = (int)(i - r * cpr) * 8;
        half8_t v = *reinterpret_cast<const half8_t*>(x + r * ldx + c0);
        if (c0 < (cx >> 1)) {                             // cx % 16 == 0: a chunk lies in one half
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] * b);
        }
        *reinterpret_cast<half8_t*>(xo + r * ldxo + c0) = v;
        return;
    }
    const int img = (int)blockIdx.x / groups, grp = (int)blockIdx.x - img * groups;
    const int chunk = tid & (FREEU_CHUNKS - 1), lane = tid >> 4;
    const int c0 = grp * FREEU_COLS + chunk * 8;
    const bool active = c0 < cs;                          // cs % 8 == 0: a chunk is whole or absent
    const int hw = h * w;
    const float inv_h = 1.f / (float)h, inv_w = 1.f / (float)w;
    const half_t* src = sk + (long)img * hw * lds + c0;
    float acc[7][8];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    if (active) {
        for (int p = lane; p < hw; p += FREEU_LANES) {
            const half8_t v = *reinterpret_cast<const half8_t*>(src + (long)p * lds);
            float t[6];
            freeu_trig(p, w, inv_h, inv_w, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e];
                acc[0][e] += f;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[k + 1][e] = fmaf(f, t[k], acc[k + 1][e]);
            }
        }
    }
    const float scale = (s - 1.f) / (float)hw;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        // sum k on buffer k & 1: the reads of a buffer (two sums back) lie before the barrier of the sum in between
        *reinterpret_cast<float4_t*>(&part[k & 1][lane][chunk * 8]) = float4_t{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
        *reinterpret_cast<float4_t*>(&part[k & 1][lane][chunk * 8 + 4]) = float4_t{acc[k][4], acc[k][5], acc[k][6], acc[k][7]};
        __syncthreads();
        if (tid < FREEU_COLS) {
            float sum = 0.f;
#pragma unroll
            for (int l = 0; l < FREEU_LANES; ++l) sum += part[k & 1][l][tid];      // lane order: fixed
            tot[k][tid] = sum * scale;
        }
    }
    __syncthreads();
    if (!active) return;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float4_t lo = *reinterpret_cast<const float4_t*>(&tot[k][chunk * 8]), hi = *reinterpret_cast<const float4_t*>(&tot[k][chunk * 8 + 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[k][e] = lo[e]; acc[k][e + 4] = hi[e]; }
    }
    half_t* dst = so + (long)img * hw * ldso + c0;
    for (int p = lane; p < hw; p += FREEU_LANES) {
        const half8_t v = *reinterpret_cast<const half8_t*>(src + (long)p * lds);
        float t[6];
        freeu_trig(p, w, inv_h, inv_w, t);
        half8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float d = acc[0][e];
#pragma unroll
            for (int k = 0; k < 6; ++k) d = fmaf(acc[k + 1][e], t[k], d);
            o[e] = (half_t)((float)v[e] + d);
        }
        *reinterpret_cast<half8_t*>(dst + (long)p * ldso) = o;
    }
}
}  // namespace

extern "C" int pv_freeu_rows(const void* x, int32_t ldx, int32_t cx, void* x_out, int32_t ldxo, float b, const void* skip, int32_t lds, int32_t cs,
                             void* skip_out, int32_t ldso, float s, int32_t batch, int32_t h, int32_t w, void* stream) {
    const bool do_x = x != nullptr || x_out != nullptr, do_s = skip != nullptr || skip_out != nullptr;
    if (!do_x && !do_s) return (int)hipErrorInvalidValue;
    if (batch < 1 || h < 2 || w < 2) return (int)hipErrorInvalidValue;
    // rows of ld elements below 2 GiB = 2^30 halfs, checked factor by factor (the full product may not fit 64 bits)
    const int64_t lim = (int64_t)1 << 30;
    const int64_t rows = (int64_t)batch * h;
    if (rows >= lim || rows * w >= lim) return (int)hipErrorInvalidValue;
    auto bad_half = [&](const void* in, const void* out, int32_t ldi, int32_t ldo, int32_t c, int32_t cmod, float scale) {
        return !in || !out || in == out || c <= 0 || (c % cmod) || ldi < c || ldo < c || (ldi % 8) || (ldo % 8) ||
               (reinterpret_cast<uintptr_t>(in) % 16) || (reinterpret_cast<uintptr_t>(out) % 16) || !__builtin_isfinite(scale) ||
               rows * w * ldi >= lim || rows * w * ldo >= lim;
    };
    if (do_x && bad_half(x, x_out, ldx, ldxo, cx, 16, b)) return (int)hipErrorInvalidValue;
    if (do_s && bad_half(skip, skip_out, lds, ldso, cs, 8, s)) return (int)hipErrorInvalidValue;
    const int groups = do_s ? (cs + FREEU_COLS - 1) / FREEU_COLS : 1;
    const int64_t skip_blocks = do_s ? (int64_t)batch * groups : 0;
    const int64_t x_chunks = do_x ? rows * w * (cx / 8) : 0;
    const int64_t blocks = skip_blocks + (x_chunks + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(freeu_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const half_t*>(x), ldx, cx,
                       reinterpret_cast<half_t*>(x_out), ldxo, b, (long)x_chunks, reinterpret_cast<const half_t*>(skip), lds, cs,
                       reinterpret_cast<half_t*>(skip_out), ldso, s, h, w, groups, (int)skip_blocks);
    return PV_CHECK_LAUNCH();
}

namespace {
// Token pooling of fp16 rows (header: pv_token_pool).  One lane owns 8 adjacent columns of one output pixel: chunk index fastest, so the lanes of a
// wave read whole 16-byte pieces of consecutive addresses of one input row per (dy, dx) and write one output row contiguously.  F > 0: the block
// side at compile time (the f * f loads of a lane unroll and are in flight together); F = 0: the run-time side.  AVG: fp32 sum over the in-bounds
// pixels in row-major order, one division by their count, one rounding; otherwise the bits of the top-left pixel.  No LDS, no atomics.
template <int F, bool AVG>
__global__ __launch_bounds__(256) void token_pool_kernel(const half_t* __restrict__ x, int ldx, half_t* __restrict__ out, int ldo, int cpr, int h, int w,
                                                         int hp, int wp, int f_rt, long lanes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lanes) return;
    const int f = F > 0 ? F : f_rt;
    const long pix = i / cpr;                              // (image * hp + oy) * wp + ox
    const int c0 = (int)(i - pix * cpr) * 8;
    const long row = pix / wp;                             // image * hp + oy
    const int ox = (int)(pix - row * wp);
    const long img = row / hp;
    const int oy = (int)(row - img * hp);
    const int y0 = oy * f, x0 = ox * f;
    const half_t* src = x + ((img * h + y0) * w + x0) * ldx + c0;
    half8_t o;
    if (!AVG) {
        o = *reinterpret_cast<const half8_t*>(src);
    } else {
        const int ny = min(f, h - y0), nx = min(f, w - x0);            // >= 1: y0 < h and x0 < w by hp = ceil(h / f), wp = ceil(w / f)
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (F > 0) {
            // every load unconditional (an out-of-bounds pixel reads the block's last in-bounds one and counts 0), so all F * F are issued before the first add
            half8_t v[F > 0 ? F * F : 1];
#pragma unroll
            for (int dy = 0; dy < F; ++dy)
#pragma unroll
                for (int dx = 0; dx < F; ++dx)
                    v[dy * F + dx] = *reinterpret_cast<const half8_t*>(src + ((long)min(dy, ny - 1) * w + min(dx, nx - 1)) * ldx);
#pragma unroll
            for (int dy = 0; dy < F; ++dy)
#pragma unroll
                for (int dx = 0; dx < F; ++dx) {
                    const bool in = dy < ny && dx < nx;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += in ? (float)v[dy * F + dx][e] : 0.f;
                }
        } else {
            for (int dy = 0; dy < ny; ++dy)
                for (int dx = 0; dx < nx; ++dx) {
                    const half8_t v = *reinterpret_cast<const half8_t*>(src + ((long)dy * w + dx) * ldx);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
                }
        }
        const float cnt = (float)(ny * nx);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[e] / cnt);
    }
    *reinterpret_cast<half8_t*>(out + pix * ldo + c0) = o;
}
}  // namespace

extern "C" int32_t pv_token_pool(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t cols, int32_t batch, int32_t h, int32_t w, int32_t f,
                                 int32_t mode, void* stream) {
    if (!x || !out || x == out) return (int)hipErrorInvalidValue;
    if (cols <= 0 || (cols % 8) || (ldx % 8) || (ldo % 8) || ldx < cols || ldo < cols) return (int)hipErrorInvalidValue;
    if (batch <= 0 || h <= 0 || w <= 0 || f < 2 || f > 8) return (int)hipErrorInvalidValue;
    if (mode != PV_POOL_AVG && mode != PV_POOL_NEAREST) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(x) % 16) || (reinterpret_cast<uintptr_t>(out) % 16)) return (int)hipErrorInvalidValue;
    // rows of ld elements below 2 GiB = 2^30 halfs, checked factor by factor (the full product may not fit 64 bits); the output has no more rows than the input
    const int64_t lim = (int64_t)1 << 30;
    const int64_t rows = (int64_t)batch * h;
    if (rows >= lim || rows * w >= lim || rows * w * ldx >= lim || rows * w * ldo >= lim) return (int)hipErrorInvalidValue;
    const int hp = (h + f - 1) / f, wp = (w + f - 1) / f, cpr = cols / 8;
    const int64_t lanes = (int64_t)batch * hp * wp * cpr;
    const int64_t blocks = (lanes + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    const half_t* xi = reinterpret_cast<const half_t*>(x);
    half_t* oo = reinterpret_cast<half_t*>(out);
#define PV_POOL_LAUNCH(F, AVG) \
    hipLaunchKernelGGL((token_pool_kernel<F, AVG>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xi, ldx, oo, ldo, cpr, h, w, hp, wp, f, (long)lanes)
    if (mode == PV_POOL_NEAREST) PV_POOL_LAUNCH(0, false);
    else if (f == 2) PV_POOL_LAUNCH(2, true);
    else if (f == 4) PV_POOL_LAUNCH(4, true);
    else PV_POOL_LAUNCH(0, true);
#undef PV_POOL_LAUNCH
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_posterior_sample(const float* moments, const float* eps, float* out, int32_t batch, int64_t chw, void* stream) {
    if (!moments || !eps || !out || batch <= 0 || chw <= 0) return (int)hipErrorInvalidValue;
    const long n = (long)batch * chw;
    hipLaunchKernelGGL(posterior_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, moments, eps, out, (long)chw, n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_reduce_mean(const void* a, const void* b, int32_t mode, int32_t is_f16, int64_t n, float* partial, int32_t n_partial, float* out,
                              void* stream) {
    if (!a || !partial || !out || n <= 0 || n_partial <= 0 || n_partial > 4096 || mode < 0 || mode > 2 || (mode == 2 && !b)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(reduce_partial_kernel, dim3((unsigned)n_partial), dim3(256), 0, (hipStream_t)stream, a, b, mode, is_f16, (long)n, partial);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, partial, n_partial, 1.0f / (float)n, out);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_reduce_sumsq(const float* a, int64_t n, float scale, float* partial, int32_t n_partial, float* out, void* stream) {
    if (!a || !partial || !out || n <= 0 || n_partial <= 0 || n_partial > 4096) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(reduce_partial_kernel, dim3((unsigned)n_partial), dim3(256), 0, (hipStream_t)stream, a, nullptr, 3, 0, (long)n, partial);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, partial, n_partial, scale, out);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_clamp_f32(float* x, float lo, float hi, int64_t n, void* stream) {
    if (n <= 0 || !x) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(clamp_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, lo, hi, (long)n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_patchify(const float* x, void* out, int32_t batch, int32_t ch, int32_t img, int32_t patch, int32_t kpad, void* stream) {
    if (batch <= 0 || ch <= 0 || img <= 0 || patch <= 0 || (img % patch) || kpad < ch * patch * patch || !x || !out)
        return (int)hipErrorInvalidValue;
    const long total = (long)batch * (img / patch) * (img / patch) * kpad;
    hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<half_t*>(out), batch, ch, img, patch, kpad);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_clip_vision_embed(const void* patches, const float* cls, const float* pos, void* out, int32_t batch, int32_t ntok,
                                    int32_t dim, void* stream) {
    if (batch <= 0 || ntok <= 1 || dim <= 0 || !patches || !cls || !pos || !out) return (int)hipErrorInvalidValue;
    const long total = (long)batch * ntok * dim;
    hipLaunchKernelGGL(vision_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const half_t*>(patches), cls, pos, reinterpret_cast<half_t*>(out), batch, ntok, dim);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_clip_text_embed(const int64_t* ids, const float* tok, const float* pos, const void* concept, const int64_t* placeholder_idx,
                                  int32_t n_concept, void* out, int32_t batch, int32_t seq, int32_t dim, void* stream) {
    if (batch <= 0 || seq <= 0 || dim <= 0 || n_concept < 0 || n_concept > seq || !ids || !tok || !pos || !out ||
        (n_concept > 0 && (!concept || !placeholder_idx)))
        return (int)hipErrorInvalidValue;
    const long total = (long)batch * seq * dim;
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids, tok, pos,
                       reinterpret_cast<const half_t*>(concept), placeholder_idx, n_concept, reinterpret_cast<half_t*>(out), batch, seq, dim);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_timestep_embedding(const float* timesteps, const int32_t* state, int32_t rows, int32_t dim, void* out,
                                     void* stream) {
    if (rows <= 0 || dim <= 0 || (dim & 1) || !timesteps || !out) return (int)hipErrorInvalidValue;
    const int n = rows * dim;
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, timesteps, state, rows,
                       dim, reinterpret_cast<half_t*>(out));
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_conv_out(const void* x, const void* w, const float* bias, float* out, int32_t batch, int32_t cin, int32_t h,
                           int32_t wd, int32_t cout, void* stream) {
    if (batch <= 0 || (cin % 64) || (cout != 4 && cout != 3) || !x || !w || !out) return (int)hipErrorInvalidValue;
    // cin in {64, 128, 256, 320, 512}: the filter (<= 37 KB) lives in LDS
    if (cout == 4)
        return launch_conv_out<4>(reinterpret_cast<const half_t*>(x), reinterpret_cast<const half_t*>(w), bias, out, batch, cin, h, wd, (hipStream_t)stream);
    return launch_conv_out<3>(reinterpret_cast<const half_t*>(x), reinterpret_cast<const half_t*>(w), bias, out, batch, cin, h, wd, (hipStream_t)stream);
}

extern "C" int pv_geglu(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t rows, int32_t n, void* stream) {
    if (rows <= 0 || n <= 0 || (n % 8) || !x || !out) return (int)hipErrorInvalidValue;
    const long total = (long)rows * (n / 8);
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const half_t*>(x), ldx, reinterpret_cast<half_t*>(out), ldo, rows, n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_cfg_dpm_step(const float* eps_uncond, const float* eps_cond, float* latents, float* x0_prev, const float* coef,
                               const int32_t* state, float guidance, int64_t n, void* stream) {
    if (n <= 0 || (n % 4) || !eps_uncond || !eps_cond || !latents || !x0_prev || !coef || !state) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(cfg_dpm_step_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, eps_uncond,
                       eps_cond, latents, x0_prev, coef, state, guidance, (long)n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_cfg_dpm_step_masked(const float* eps_uncond, const float* eps_cond, float* latents, float* x0_prev, const float* coef,
                                      const int32_t* state, float guidance, const float* mask, const float* known, const float* noise,
                                      int32_t channels, int32_t hw, int64_t n, void* stream) {
    if (!eps_uncond || !eps_cond || !latents || !x0_prev || !coef || !state || !mask || !known || !noise) return (int)hipErrorInvalidValue;
    if (channels <= 0 || hw <= 0 || (hw % 4) || n <= 0 || (n % ((int64_t)channels * hw))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(cfg_dpm_step_masked_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, eps_uncond,
                       eps_cond, latents, x0_prev, coef, state, guidance, mask, known, noise, (long)channels * hw, hw, (long)n);
    return PV_CHECK_LAUNCH();
}

template <bool IMG, bool RESCALE, bool NOISE, bool PAG = false>
static int launch_cfg_dpm_step_guided(const float* eu, const float* em, const float* ec, const float* ep, float* lat, float* x0p, const float* coef,
                                      const int32_t* state, const uint32_t* rng, float gt, float gi, float gp, float rescale, const float* mask,
                                      const float* known, const float* noise, int batch, long chw, int hw, hipStream_t stream) {
    const long nv = chw / 4;
    const dim3 grid((unsigned)batch), block((unsigned)(nv >= 1024 ? 1024 : (nv + 63) / 64 * 64));     // whole waves: every lane shuffles
    if (mask)
        hipLaunchKernelGGL((cfg_dpm_step_guided_kernel<IMG, RESCALE, true, NOISE, PAG>), grid, block, 0, stream, eu, em, ec, ep, lat, x0p, coef, state,
                           rng, gt, gi, gp, rescale, mask, known, noise, chw, hw);
    else
        hipLaunchKernelGGL((cfg_dpm_step_guided_kernel<IMG, RESCALE, false, NOISE, PAG>), grid, block, 0, stream, eu, em, ec, ep, lat, x0p, coef, state,
                           rng, gt, gi, gp, rescale, mask, known, noise, chw, hw);
    return PV_CHECK_LAUNCH();
}

// the body of pv_cfg_dpm_step_guided (rng == NULL) and pv_cfg_dpm_step_stochastic (rng != NULL): validation before the first HIP call
// and of pv_cfg_dpm_step_pag (either, with eps_perturbed / g_pag; the other two pass nullptr / 0 and land on the PAG = false instantiations)
template <bool NOISE>
static int cfg_dpm_step_guided_entry(const float* eps_uncond, const float* eps_image, const float* eps_cond, const float* eps_perturbed, float* latents,
                                     float* x0_prev, const float* coef, const int32_t* state, const uint32_t* rng, float g_text, float g_image,
                                     float g_pag, float rescale, const float* mask, const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw,
                                     void* stream) {
    if (!eps_uncond || !eps_cond || !latents || !x0_prev || !coef || !state || (NOISE && !rng)) return (int)hipErrorInvalidValue;
    if (batch < 1 || channels < 1 || hw < 1 || (hw % 4)) return (int)hipErrorInvalidValue;
    if ((mask != nullptr) != (known != nullptr) || (mask != nullptr) != (noise != nullptr)) return (int)hipErrorInvalidValue;
    if (!__builtin_isfinite(g_text) || !__builtin_isfinite(g_image) || !__builtin_isfinite(g_pag) || !(rescale >= 0.f && rescale <= 1.f))
        return (int)hipErrorInvalidValue;
    const int64_t chw = (int64_t)channels * hw, lim = (int64_t)1 << 31;
    if (chw >= lim || (int64_t)batch * chw >= lim) return (int)hipErrorInvalidValue;
    const hipStream_t s = (hipStream_t)stream;
    // equal scales: the eps_image terms cancel, eu + g (em - eu) + g (ec - em) == eu + g (ec - eu).  Evaluate the two-term expression: the same
    // polynomial with fewer roundings, so a three-forward step at equal scales has the bits of the two-forward step (eps_image is then not read)
    if (eps_image && g_image == g_text) eps_image = nullptr;
    // no perturbed prediction, or scale 0: the term vanishes - the instantiations (and bits) of the entry points without it; eps_perturbed is not read
    if (eps_perturbed && g_pag == 0.f) eps_perturbed = nullptr;
#define PV_GUIDED(IMG, RS, PAG) \
    launch_cfg_dpm_step_guided<IMG, RS, NOISE, PAG>(eps_uncond, eps_image, eps_cond, eps_perturbed, latents, x0_prev, coef, state, rng, g_text, g_image, \
                                                    g_pag, rescale, mask, known, noise, batch, (long)chw, hw, s)
    if (eps_perturbed) {
        if (eps_image) return rescale > 0.f ? PV_GUIDED(true, true, true) : PV_GUIDED(true, false, true);
        return rescale > 0.f ? PV_GUIDED(false, true, true) : PV_GUIDED(false, false, true);
    }
    if (eps_image) return rescale > 0.f ? PV_GUIDED(true, true, false) : PV_GUIDED(true, false, false);
    return rescale > 0.f ? PV_GUIDED(false, true, false) : PV_GUIDED(false, false, false);
#undef PV_GUIDED
}

extern "C" int pv_cfg_dpm_step_guided(const float* eps_uncond, const float* eps_image, const float* eps_cond, float* latents, float* x0_prev,
                                      const float* coef, const int32_t* state, float g_text, float g_image, float rescale, const float* mask,
                                      const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw, void* stream) {
    return cfg_dpm_step_guided_entry<false>(eps_uncond, eps_image, eps_cond, nullptr, latents, x0_prev, coef, state, nullptr, g_text, g_image, 0.f, rescale,
                                            mask, known, noise, batch, channels, hw, stream);
}

extern "C" int pv_cfg_dpm_step_stochastic(const float* eps_uncond, const float* eps_image, const float* eps_cond, float* latents, float* x0_prev,
                                          const float* coef, const int32_t* state, const uint32_t* rng, float g_text, float g_image, float rescale,
                                          const float* mask, const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw,
                                          void* stream) {
    return cfg_dpm_step_guided_entry<true>(eps_uncond, eps_image, eps_cond, nullptr, latents, x0_prev, coef, state, rng, g_text, g_image, 0.f, rescale, mask,
                                           known, noise, batch, channels, hw, stream);
}

extern "C" int pv_cfg_dpm_step_pag(const float* eps_uncond, const float* eps_image, const float* eps_cond, const float* eps_perturbed, float* latents,
                                   float* x0_prev, const float* coef, const int32_t* state, const uint32_t* rng, float g_text, float g_image, float g_pag,
                                   float rescale, const float* mask, const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw,
                                   void* stream) {
    if (rng)
        return cfg_dpm_step_guided_entry<true>(eps_uncond, eps_image, eps_cond, eps_perturbed, latents, x0_prev, coef, state, rng, g_text, g_image, g_pag,
                                               rescale, mask, known, noise, batch, channels, hw, stream);
    return cfg_dpm_step_guided_entry<false>(eps_uncond, eps_image, eps_cond, eps_perturbed, latents, x0_prev, coef, state, nullptr, g_text, g_image, g_pag,
                                            rescale, mask, known, noise, batch, channels, hw, stream);
}

extern "C" int pv_composite_clamp_f32(const float* gen, const float* orig, const float* mask, float* out, float lo, float hi, int32_t batch,
                                      int32_t channels, int32_t hw, void* stream) {
    if (!gen || !orig || !mask || !out || batch <= 0 || channels <= 0 || hw <= 0 || (hw % 4)) return (int)hipErrorInvalidValue;
    const long chw = (long)channels * hw, n = chw * batch;
    hipLaunchKernelGGL(composite_clamp_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gen, orig, mask, out, lo, hi,
                       chw, hw, n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_step_advance(int32_t* state, void* stream) {
    if (!state) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_fusion_draw(const int32_t* state, uint32_t* rng, const float* forced, float* out, int32_t n_layers, float rule1, float rule2,
                              float scale, int32_t only_last_step, void* stream) {
    if (!rng || !out || n_layers <= 0 || n_layers > 256) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fusion_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, rng, forced, out, n_layers, rule1, rule2, scale,
                       only_last_step);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
    if (n <= 0 || !x || !y) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(cast_f32_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<half_t*>(y), (long)n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream) {
    if (n <= 0 || !x || !y) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(cast_f16_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const half_t*>(x), y, (long)n);
    return PV_CHECK_LAUNCH();
}

extern "C" int pv_rows_mean(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t groups, int32_t count, int32_t group_rows,
                            int32_t cols, int32_t accumulate, void* stream) {
    if (groups <= 0 || count <= 0 || group_rows < count || cols <= 0 || (cols % 8) || !x || !y) return (int)hipErrorInvalidValue;
    const int blocks = groups * ((cols / 8 + 31) / 32);
    hipLaunchKernelGGL(rows_mean_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const half_t*>(x), ldx, reinterpret_cast<half_t*>(y), ldy, groups, count, group_rows, cols, accumulate);
    return PV_CHECK_LAUNCH();
}
