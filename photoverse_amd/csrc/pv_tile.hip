// The one launch tiled VAE decode / encode needs beyond the existing plans (header: pv_tile_blend): the seam blend of one tile position over the whole
// batch.  HBM-bound: 16-byte loads and stores where every row start and width is a multiple of 4 floats, a scalar path otherwise; no atomics, no scratch.
#include "pv_common.h"

namespace {

// One lane owns W adjacent pixels of one tile row (W = 4 on the 16-byte path, 1 on the scalar path); the x index runs fastest, so a wave reads and writes
// whole row segments.  A lane reads and writes only its own pixels of `tile`, which is what makes the in-place update safe; `above` and `left` are the
// already blended neighbours and are only read.  The tile is written back only where a blend changed it (y < ev or x < eh).
template <int W>
__global__ __launch_bounds__(256) void tile_blend_kernel(float* __restrict__ tile, const float* __restrict__ above, const float* __restrict__ left,
                                                         float* __restrict__ out, int th, int tw, int ah, int lw, int ev, int eh, int keep_h, int keep_w,
                                                         int out_h, int out_w, int oy, int ox, long lanes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lanes) return;
    const int cpr = tw / W;                                   // lanes per tile row
    const long row = i / cpr;                                 // plane * th + y, plane = b * channels + c
    const int x = (int)(i - row * cpr) * W;
    const long plane = row / th;
    const int y = (int)(row - plane * th);
    float* tp = tile + row * tw + x;
    float v[W];
    if (W == 4) {
        const float4_t t4 = *reinterpret_cast<const float4_t*>(tp);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = t4[e];
    } else {
        v[0] = *tp;
    }
    const bool vert = y < ev, horz = x < eh;                  // W == 4: eh % 4 == 0, the four pixels are inside or outside together
    if (vert) {
        const float* ap = above + (plane * ah + (ah - ev + y)) * tw + x;
        const float wy = (float)y / (float)ev, wa = 1.0f - wy;
        if (W == 4) {
            const float4_t a4 = *reinterpret_cast<const float4_t*>(ap);
#pragma unroll
            for (int e = 0; e < W; ++e) v[e] = a4[e] * wa + v[e] * wy;
        } else {
            v[0] = ap[0] * wa + v[0] * wy;
        }
    }
    if (horz) {
        const float* lp = left + row * lw + (lw - eh + x);
        float l[W];
        if (W == 4) {
            const float4_t l4 = *reinterpret_cast<const float4_t*>(lp);
#pragma unroll
            for (int e = 0; e < W; ++e) l[e] = l4[e];
        } else {
            l[0] = lp[0];
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float wx = (float)(x + e) / (float)eh;
            v[e] = l[e] * (1.0f - wx) + v[e] * wx;
        }
    }
    const bool kept = y < keep_h && x < keep_w;               // W == 4: keep_w % 4 == 0
    float* op = out + (plane * out_h + (oy + y)) * out_w + (ox + x);
    if (W == 4) {
        const float4_t o4 = {v[0], v[1], v[2], v[3]};
        if (vert || horz) *reinterpret_cast<float4_t*>(tp) = o4;
        if (kept) *reinterpret_cast<float4_t*>(op) = o4;
    } else {
        if (vert || horz) *tp = v[0];
        if (kept) *op = v[0];
    }
}

// a * b * c * d < lim without overflow (all factors positive 32-bit values)
bool tb_fits(int64_t a, int64_t b, int64_t c, int64_t d, int64_t lim) {
    int64_t p = a * b;
    if (p >= lim) return false;
    p *= c;
    if (p >= lim) return false;
    p *= d;
    return p < lim;
}

bool tb_overlap(const float* p, int64_t np, const float* q, int64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)nq * 4 && b < a + (uintptr_t)np * 4;
}
}  // namespace

extern "C" int32_t pv_tile_blend(float* tile, const float* above, const float* left, float* out, int32_t batch, int32_t channels, int32_t th, int32_t tw,
                                 int32_t ah, int32_t lw, int32_t ev, int32_t eh, int32_t keep_h, int32_t keep_w, int32_t out_h, int32_t out_w, int32_t oy,
                                 int32_t ox, void* stream) {
    if (!tile || !out) return (int)hipErrorInvalidValue;
    if (batch <= 0 || channels <= 0 || th <= 0 || tw <= 0 || out_h <= 0 || out_w <= 0) return (int)hipErrorInvalidValue;
    // a neighbour comes with its blend extent, no neighbour with extent 0
    if (above ? (ah <= 0 || ev <= 0 || ev > ah || ev > th) : (ev != 0)) return (int)hipErrorInvalidValue;
    if (left ? (lw <= 0 || eh <= 0 || eh > lw || eh > tw) : (eh != 0)) return (int)hipErrorInvalidValue;
    if (keep_h <= 0 || keep_w <= 0 || keep_h > th || keep_w > tw || oy < 0 || ox < 0) return (int)hipErrorInvalidValue;
    if ((int64_t)oy + keep_h > out_h || (int64_t)ox + keep_w > out_w) return (int)hipErrorInvalidValue;
    const int64_t lim = (int64_t)1 << 29;                      // 2 GiB of fp32
    if (!tb_fits(batch, channels, th, tw, lim) || !tb_fits(batch, channels, out_h, out_w, lim)) return (int)hipErrorInvalidValue;
    if ((above && !tb_fits(batch, channels, ah, tw, lim)) || (left && !tb_fits(batch, channels, th, lw, lim))) return (int)hipErrorInvalidValue;
    const int64_t planes = (int64_t)batch * channels;
    const int64_t n_tile = planes * th * tw, n_out = planes * out_h * out_w, n_above = above ? planes * ah * tw : 0, n_left = left ? planes * th * lw : 0;
    const uintptr_t align = reinterpret_cast<uintptr_t>(tile) | reinterpret_cast<uintptr_t>(above) | reinterpret_cast<uintptr_t>(left) |
                            reinterpret_cast<uintptr_t>(out);
    if (align % 4) return (int)hipErrorInvalidValue;
    // the two written operands overlap nothing else (above and left are both read only and may be one buffer)
    if (tb_overlap(tile, n_tile, out, n_out) || (above && (tb_overlap(tile, n_tile, above, n_above) || tb_overlap(out, n_out, above, n_above))) ||
        (left && (tb_overlap(tile, n_tile, left, n_left) || tb_overlap(out, n_out, left, n_left))))
        return (int)hipErrorInvalidValue;
    // 16-byte path: every row of every operand starts on a 16-byte boundary and the blend / keep edges fall between 4-pixel chunks
    const bool vec = !(align % 16) && !(tw % 4) && !(out_w % 4) && !(ox % 4) && !(keep_w % 4) && (!left || (!(lw % 4) && !(eh % 4)));
    const int64_t lanes = vec ? n_tile / 4 : n_tile;           // < 2^29
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
#define PV_TB_LAUNCH(W)                                                                                                                              \
    hipLaunchKernelGGL((tile_blend_kernel<W>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, tile, above, left, out, th, tw, ah, lw, ev, eh, keep_h, \
                       keep_w, out_h, out_w, oy, ox, (long)lanes)
    if (vec) PV_TB_LAUNCH(4);
    else PV_TB_LAUNCH(1);
#undef PV_TB_LAUNCH
    return PV_CHECK_LAUNCH();
}
