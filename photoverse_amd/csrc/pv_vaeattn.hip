// pv_vae_attention (header: the contract): single-head flash attention for the VAE mid block's wide head (d = 256 / 512) - softmax(scale q k^T) v per
// image without the [n][n] score matrix.  A translation unit of its own: pv_attn.hip's d = 40 loop is pinned against instruction-fetch alignment, so the
// helpers this kernel shares with attn_kernel<D, NQ, DMA> (fragment layouts, the transposed V read, the V row stride rule) are copied, not moved.
//
// One 256-thread workgroup owns 64 queries, a wave 16 of them: its Q fragments (d / 32 x 4 VGPRs) and its 16 x d fp32 output (d / 4 registers, the AGPR
// half) stay in registers for the whole key loop - 64 + 128 registers at d = 512, one wave per SIMD.  Keys go by in tiles of 64: the K tile and the V tile
// each have an LDS image of their own (d = 512: 65 KiB + 66 KiB), and ONE 64-register staging set carries both - V(t) is fetched while K(t).Q^T runs and
// written before the tile's second barrier, K(t + 1) is fetched under the softmax and V^T.P^T and written behind them:
//     barrier | fetch V(t) | S^T = K.Q^T | write V(t), fetch K(t+1) | barrier | softmax, O^T += V^T.P^T | write K(t+1) |
// As in attn_kernel the products are transposed (S^T = K Q^T, O^T = V^T P^T): the score tile leaves the MFMA with the query on the lane and the keys in the
// registers, which is the B operand of the second product with no lane movement, and the output fragment is four adjacent columns of one query row.
// Scores, the running maximum and the denominator are fp32; P is rounded to fp16 once, for the MFMA, and the denominator adds up those rounded values.
// No scratch, no atomics, a fixed summation order: the same bits on every launch.
#include "pv_common.h"

namespace {

// how far (log2 units) a score may exceed its row's softmax reference before the reference moves: P <= 2^8 keeps its relative precision in fp16 and the sums
// are fp32, while the rescale of the d / 4 output registers leaves the common path (attn_kernel's PV_ATTN_LAZY_UP)
#define PV_VA_LAZY_UP 8.f

template <int D>
struct VCfg {
    static constexpr int KB = 64;                  // keys per tile
    static constexpr int KSTEPS = D / 32;          // 32-deep contraction steps of K.Q^T
    static constexpr int DVF = D / 16;             // 16-wide output fragments of V^T.P^T
    static constexpr int CH = D / 8;               // 16-byte chunks per row
    static constexpr int KS = D + 8;               // K row stride in halfs: rows padded by 16 B (consecutive rows start one 16-B slot apart)
    // V row stride in halfs.  ds_read_b64_tr_b16: a 32-lane group reads 8 consecutive key rows x 32 B, so the eight rows must land on eight different
    // 32-B slots of the 256-B bank window: stride = 8 * odd dwords (mod 64) - d = 256 -> 272 halfs, d = 512 -> 528 (ACfg::vs_dwords of pv_attn.hip)
    static constexpr int vs_dwords() {
        int v = DVF * 8;
        while ((v & 63) != 8 && (v & 63) != 24 && (v & 63) != 40 && (v & 63) != 56) v += 4;
        return v;
    }
    static constexpr int VS = vs_dwords() * 2;
    static constexpr int KPT = KB * CH / 256;      // 16-byte chunks of one tile per thread
    static constexpr int SMEM = KB * (KS + VS) * 2;
};

// V^T fragment (MFMA-A) for output columns dv0..dv0+15 and the 8 keys {key0+4fq..+3, key0+16+4fq..+3} (vt_frag of pv_attn.hip)
__device__ __forceinline__ half8_t va_vt_frag(const half_t* sV, int VS, int key0, int dv0, int fr, int fq) {
    const half_t* a = sV + (key0 + fq * 4 + (fr >> 2)) * VS + dv0 + (fr & 3) * 4;
    const fp16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(a));
    const fp16x4_t t2 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(a + 16 * VS));
    half8_t r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[j] = (half_t)t1[j];
        r[j + 4] = (half_t)t2[j];
    }
    return r;
}

struct va_params {
    const half_t *q, *k, *v;
    half_t* out;
    int ldq, ldk, ldv, ldo, n;
    float scale_log2;                              // scale * log2(e): the scores are exponentiated in base 2
};

template <int D>
__global__ __launch_bounds__(256) void vae_attn_kernel(const va_params p) {
    using C = VCfg<D>;
    constexpr int KB = C::KB;
    // hipcc's scheduler may move instructions inside windows of WIN contraction steps (4 WIN K-fragment reads + MFMAs) and 2 WIN output fragments only: left
    // alone it hoists the LDS reads of a whole tile ahead of their MFMAs and the d = 512 instance spills
    constexpr int WIN = 4;
    extern __shared__ __attribute__((aligned(16))) char va_smem[];
    half_t* sK = reinterpret_cast<half_t*>(va_smem);
    half_t* sV = sK + KB * C::KS;

    const int tid = threadIdx.x, lane = tid & 63, wave = pv_wave_id();
    const int fr = lane & 15, fq = lane >> 4;
    // the query tiles of one image get consecutive remapped ids, i.e. run on one XCD and share its L2's copy of the image's K and V
    const int nqt = (p.n + 63) / 64;
    const int rid = pv_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int qt = rid % nqt, b = rid / nqt;
    const size_t row0 = (size_t)b * p.n;           // the image's first row: nothing of another image is ever addressed
    const half_t* Q = p.q + row0 * p.ldq;
    const half_t* Kg = p.k + row0 * p.ldk;
    const half_t* Vg = p.v + row0 * p.ldv;

    // Q^T fragments (MFMA-B): query fr of the wave's 16, columns 32 ks + 8 fq .. + 7.  A query row behind the image reads the image's last row (and is
    // never stored)
    const int qrow = qt * 64 + wave * 16 + fr;
    half8_t qf[C::KSTEPS];
    {
        const half_t* qp = Q + (size_t)min(qrow, p.n - 1) * p.ldq + fq * 8;
#pragma unroll
        for (int ks = 0; ks < C::KSTEPS; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(qp + ks * 32);
    }

    // the staging set: chunk tid + 256 i of the [64][CH] tile, fetched through a buffer descriptor over the IMAGE's rows.  Keys behind the image's n take an
    // out-of-range offset and read ZEROS without a branch: the row there may be another image's or hold NaN, and a masked probability of 0 times such a V
    // would still be NaN.  (Every in-range offset is below 2 GiB: the launcher checks the extents.)
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(Kg), 0, ((p.n - 1) * p.ldk + D) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(Vg), 0, ((p.n - 1) * p.ldv + D) * 2, 0x00020000);
    const int key0 = tid / C::CH, c0 = tid - key0 * C::CH;
    half8_t sreg[C::KPT];
    auto gload = [&](const __amdgpu_buffer_rsrc_t r, int ld, int t) {
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            const int gk = t * KB + i * (256 / C::CH) + key0;
            const unsigned off = gk < p.n ? (unsigned)(gk * ld * 2 + c0 * 16) : 0x80000000u;
            sreg[i] = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
        }
    };
    auto swrite = [&](half_t* s, int stride) {
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            *reinterpret_cast<half8_t*>(s + (i * (256 / C::CH) + key0) * stride + c0 * 8) = sreg[i];
        }
    };

    float4_t o[C::DVF];
#pragma unroll
    for (int f = 0; f < C::DVF; ++f) o[f] = float4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = 0.f, l_run = 0.f;                // m_run (log2 units) is set by the first tile; l_run: this lane's share of the denominator

    const int ntiles = (p.n + KB - 1) / KB;
    gload(rk, p.ldk, 0);
    swrite(sK, C::KS);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                           // K(t) is visible; every wave is done with V(t - 1)
        gload(rv, p.ldv, t);
        // S^T = K.Q^T: s[kb][r] = key 16 kb + 4 fq + r against query fr
        float4_t s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C::KSTEPS; ++ks) {
            if (ks % WIN == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const half8_t a = *reinterpret_cast<const half8_t*>(sK + (kb * 16 + fr) * C::KS + ks * 32 + fq * 8);
                s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], s[kb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        swrite(sV, C::VS);
        const bool more = t + 1 < ntiles;          // block-uniform
        if (more) gload(rk, p.ldk, t + 1);
        __syncthreads();                           // V(t) is visible; every wave is done with K(t)

        // online softmax in log2 units, relative to the row's reference m_run
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] = fmaf(s[kb][r], p.scale_log2, -m_run);
        if ((t + 1) * KB > p.n) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t * KB + kb * 16 + fq * 4 + r >= p.n) s[kb][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = pv_quad_max(mx);                      // the tile's row maximum minus m_run; finite: every tile has at least one key of the image
        const bool first = t == 0;
        if (first || __any(mx > PV_VA_LAZY_UP)) {
            // move the reference by d and rescale what the row has accumulated (nothing yet in the first tile)
            const float d = first ? mx : fmaxf(mx, 0.f);
            const float alpha = first ? 0.f : PV_EXP2(-d);
            m_run += d;
            l_run *= alpha;
#pragma unroll
            for (int f = 0; f < C::DVF; ++f) {
                if (f % WIN == 0) __builtin_amdgcn_sched_barrier(0);     // (the accumulators pass through VGPRs here: a few at a time)
                o[f] *= alpha;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[kb][r] -= d;
        }
        // P^T fragments (MFMA-B) of the two 32-key steps: element j of lane quarter fq is key 32 s2 + 4 fq + j (j < 4), 32 s2 + 16 + 4 fq + j - 4 (j >= 4) -
        // the order va_vt_frag reads V in.  The denominator adds the ROUNDED probabilities: numerator and denominator agree
        half8_t pb[2];
        float rs = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const half_t p0 = (half_t)PV_EXP2(s[2 * s2][r]), p1 = (half_t)PV_EXP2(s[2 * s2 + 1][r]);
                pb[s2][r] = p0;
                pb[s2][r + 4] = p1;
                rs += (float)p0;
                rs += (float)p1;
            }
        l_run += rs;
        // O^T += V^T.P^T: o[f][r] = output column 16 f + 4 fq + r of query fr
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int f = 0; f < C::DVF; ++f) {
                if (f % (2 * WIN) == 0) __builtin_amdgcn_sched_barrier(0);
                const half8_t a = va_vt_frag(sV, C::VS, s2 * 32, f * 16, fr, fq);
                o[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[s2], o[f], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
        if (more) swrite(sK, C::KS);               // behind the second barrier: nobody reads K(t) any more
    }

    const float inv = 1.0f / pv_quad_sum(l_run);
    if (qrow < p.n) {
        half_t* O = p.out + (row0 + qrow) * p.ldo + fq * 4;
#pragma unroll
        for (int f = 0; f < C::DVF; ++f) {
            half4_t ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = (half_t)(o[f][r] * inv);
            *reinterpret_cast<half4_t*>(O + f * 16) = ov;
        }
    }
}

template <int D>
int va_launch(const va_params& p, int batch, hipStream_t s) {
    constexpr int smem = VCfg<D>::SMEM;            // 67 KiB / 131 KiB: above the default limit of dynamic LDS
    static bool attr_set_dev[64] = {};             // per device: one process may drive several GPUs
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    if (!attr_set_dev[dev_id & 63]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vae_attn_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        attr_set_dev[dev_id & 63] = true;
    }
    const unsigned wgs = (unsigned)batch * (unsigned)((p.n + 63) / 64);
    hipLaunchKernelGGL((vae_attn_kernel<D>), dim3(wgs), dim3(256), smem, s, p);
    return PV_CHECK_LAUNCH();
}

bool va_overlap(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) { return a < b + (uintptr_t)nb && b < a + (uintptr_t)na; }

}  // namespace

extern "C" int32_t pv_vae_attention(const void* q, const void* k, const void* v, int32_t ldq, int32_t ldk, int32_t ldv, void* out, int32_t ldo, int32_t batch,
                                    int32_t n, int32_t d, float scale, void* stream) {
    if (!q || !k || !v || !out) return (int)hipErrorInvalidValue;
    if (d != 256 && d != 512) return (int)hipErrorInvalidValue;
    if (batch < 1 || n < 1 || !__builtin_isfinite(scale) || !__builtin_isfinite(scale * 1.4426950408889634f)) return (int)hipErrorInvalidValue;
    if (ldq < d || ldk < d || ldv < d || ldo < d || ((ldq | ldk | ldv | ldo) & 7)) return (int)hipErrorInvalidValue;
    const uintptr_t uq = reinterpret_cast<uintptr_t>(q), uk = reinterpret_cast<uintptr_t>(k), uv = reinterpret_cast<uintptr_t>(v),
                    uo = reinterpret_cast<uintptr_t>(out);
    if ((uq | uk | uv | uo) & 15) return (int)hipErrorInvalidValue;
    // extents in bytes: rows [batch * n] of d halfs at the leading dimension.  2^22 rows of 256 halfs are 2 GiB already, so the products below fit 64 bits
    const int64_t rows = (int64_t)batch * n;
    if (rows >= ((int64_t)1 << 22)) return (int)hipErrorInvalidValue;
    const int64_t lim = (int64_t)1 << 31;
    const int64_t eq = ((rows - 1) * ldq + d) * 2, ek = ((rows - 1) * ldk + d) * 2, ev = ((rows - 1) * ldv + d) * 2, eo = ((rows - 1) * ldo + d) * 2;
    if (eq >= lim || ek >= lim || ev >= lim || eo >= lim) return (int)hipErrorInvalidValue;
    if (va_overlap(uo, eo, uq, eq) || va_overlap(uo, eo, uk, ek) || va_overlap(uo, eo, uv, ev)) return (int)hipErrorInvalidValue;
    va_params p;
    p.q = reinterpret_cast<const half_t*>(q);
    p.k = reinterpret_cast<const half_t*>(k);
    p.v = reinterpret_cast<const half_t*>(v);
    p.out = reinterpret_cast<half_t*>(out);
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.n = n;
    p.scale_log2 = scale * 1.4426950408889634f;
    return d == 256 ? va_launch<256>(p, batch, (hipStream_t)stream) : va_launch<512>(p, batch, (hipStream_t)stream);
}
