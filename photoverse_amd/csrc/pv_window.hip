// The two launches of windowed denoising (MultiDiffusion; header: pv_window_gather, pv_window_blend): cut the overlapping windows out of a latent canvas,
// and set the canvas to the weighted mean of the windows.  HBM-bound: 16-byte loads and stores where every row start and width is a multiple of 4
// floats, a scalar path otherwise; every lane owns its output elements - no atomics, no LDS, no scratch.
#include "pv_common.h"

namespace {

constexpr int kMaxWin = 64;                                   // windows per axis

// The window origins travel by value in the kernel arguments (read on the host during the call: no device table to keep alive, and the launch can be
// captured).  Every index into them below is uniform over the workgroup, so they are read with scalar loads.
struct WinOrigins {
    int oy[kMaxWin];
    int ox[kMaxWin];
};

template <int W>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[W]) {
    if (W == 4) {
        const float4_t t = *reinterpret_cast<const float4_t*>(p);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = t[e];
    } else {
        v[0] = *p;
    }
}

template <int W>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[W]) {
    if (W == 4) {
        const float4_t t = {v[0], v[W > 1 ? 1 : 0], v[W > 2 ? 2 : 0], v[W > 3 ? 3 : 0]};
        *reinterpret_cast<float4_t*>(p) = t;
    } else {
        *p = v[0];
    }
}

// blockIdx.y = window k = ky * nx + kx; the lanes of blockIdx.x run over (b, c, y, x / W) of that window, x fastest: a wave reads and writes row segments.
template <int W>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ canvas, float* __restrict__ windows, WinOrigins org, int nx, int nwin,
                                                            int channels, int H, int Wd, int S, long lanes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lanes) return;
    const int k = blockIdx.y, ky = k / nx, kx = k - ky * nx;
    const int y0 = org.oy[ky], x0 = org.ox[kx];
    const int cpr = S / W;                                    // lanes per window row
    const long row = i / cpr;                                 // (b * channels + c) * S + y
    const int x = (int)(i - row * cpr) * W;
    const long plane = row / S;                               // b * channels + c
    const int y = (int)(row - plane * S);
    const long b = plane / channels;
    const long c = plane - b * channels;
    float v[W];
    load_vec<W>(canvas + (plane * H + (y0 + y)) * Wd + (x0 + x), v);
    store_vec<W>(windows + (((b * nwin + k) * channels + c) * S + y) * S + x, v);
}

// One lane owns W adjacent canvas elements of one row.  The two loops run over ALL windows of an axis, in ascending order, with a uniform index; a lane
// takes part where the window covers it (W == 4: S and every ox are multiples of 4, so its four elements are inside or outside together).
template <int W>
__global__ __launch_bounds__(256) void window_blend_kernel(const float* __restrict__ windows, const float* __restrict__ profile, float* __restrict__ canvas,
                                                           WinOrigins org, int ny, int nx, int channels, int H, int Wd, int S, long lanes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= lanes) return;
    const int cpr = Wd / W;                                   // lanes per canvas row
    const long row = i / cpr;                                 // (b * channels + c) * H + y
    const int x = (int)(i - row * cpr) * W;
    const long plane = row / H;
    const int y = (int)(row - plane * H);
    const long b = plane / channels;
    const long c = plane - b * channels;
    const int nwin = ny * nx;
    float num[W], den_x[W], den_y = 0.0f;
    bool first = true, first_x = true;
#pragma unroll
    for (int e = 0; e < W; ++e) num[e] = den_x[e] = 0.0f;
    for (int kx = 0; kx < nx; ++kx) {                         // the x normaliser: one sum per element, ascending kx
        const int dx = x - org.ox[kx];
        if (dx < 0 || dx >= S) continue;
        float px[W];
#pragma unroll
        for (int e = 0; e < W; ++e) px[e] = 1.0f;
        if (profile) load_vec<W>(profile + dx, px);
#pragma unroll
        for (int e = 0; e < W; ++e) den_x[e] = first_x ? px[e] : den_x[e] + px[e];
        first_x = false;
    }
    bool first_y = true;
    for (int ky = 0; ky < ny; ++ky) {
        const int dy = y - org.oy[ky];
        if (dy < 0 || dy >= S) continue;
        const float py = profile ? profile[dy] : 1.0f;
        den_y = first_y ? py : den_y + py;
        first_y = false;
        for (int kx = 0; kx < nx; ++kx) {
            const int dx = x - org.ox[kx];
            if (dx < 0 || dx >= S) continue;
            float px[W], w[W];
#pragma unroll
            for (int e = 0; e < W; ++e) px[e] = 1.0f;
            if (profile) load_vec<W>(profile + dx, px);
            load_vec<W>(windows + (((b * nwin + (ky * nx + kx)) * channels + c) * S + dy) * S + dx, w);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float t = (py * px[e]) * w[e];
                num[e] = first ? t : num[e] + t;              // the first term as it is: a single window keeps its bits, the sign of zero included
            }
            first = false;
        }
    }
    float out[W];
#pragma unroll
    for (int e = 0; e < W; ++e) out[e] = num[e] / (den_y * den_x[e]);
    store_vec<W>(canvas + row * Wd + x, out);
}

// the product of the factors is below lim (all factors positive 32-bit values)
bool win_fits(std::initializer_list<int64_t> f, int64_t lim) {
    int64_t p = 1;
    for (int64_t v : f) {
        p *= v;
        if (p >= lim) return false;
    }
    return true;
}

bool win_overlap(const float* p, int64_t np, const float* q, int64_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)nq * 4 && b < a + (uintptr_t)np * 4;
}

// origins of one axis: o[0] == 0, strictly increasing, at most S apart (every position covered), the last window ends on the extent
bool win_origins_ok(const int32_t* o, int32_t n, int32_t S, int32_t extent) {
    if (!o || n < 1 || n > kMaxWin || o[0] != 0) return false;
    for (int i = 1; i < n; ++i)
        if (o[i] <= o[i - 1] || (int64_t)o[i] - o[i - 1] > S) return false;
    return (int64_t)o[n - 1] + S == extent;
}

// Everything the two launchers share: the checks, the by-value origins and the choice of path.  Returns false for a call to reject.
bool win_prepare(const float* canvas, const float* windows, const float* profile, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t S,
                 const int32_t* oy, int32_t ny, const int32_t* ox, int32_t nx, WinOrigins& org, bool& vec) {
    if (!canvas || !windows) return false;
    if (batch <= 0 || channels <= 0 || H <= 0 || W <= 0 || S < 1 || S > H || S > W) return false;
    if (!win_origins_ok(oy, ny, S, H) || !win_origins_ok(ox, nx, S, W)) return false;
    const int64_t lim = (int64_t)1 << 29;                      // 2 GiB of fp32
    if (!win_fits({batch, channels, H, W}, lim) || !win_fits({batch, ny, nx, channels, S, S}, lim)) return false;
    const int64_t n_canvas = (int64_t)batch * channels * H * W, n_win = (int64_t)batch * ny * nx * channels * S * S;
    const uintptr_t align = reinterpret_cast<uintptr_t>(canvas) | reinterpret_cast<uintptr_t>(windows) | reinterpret_cast<uintptr_t>(profile);
    if (align % 4) return false;
    if (win_overlap(canvas, n_canvas, windows, n_win)) return false;
    if (profile && (win_overlap(canvas, n_canvas, profile, S) || win_overlap(windows, n_win, profile, S))) return false;
    memset(&org, 0, sizeof(org));
    bool ox4 = true;
    for (int i = 0; i < ny; ++i) org.oy[i] = oy[i];
    for (int i = 0; i < nx; ++i) {
        org.ox[i] = ox[i];
        ox4 = ox4 && !(ox[i] % 4);
    }
    // 16-byte path: every row of both tensors (and every profile read) starts on a 16-byte boundary
    vec = !(align % 16) && !(W % 4) && !(S % 4) && ox4;
    return true;
}
}  // namespace

extern "C" int32_t pv_window_gather(const float* canvas, float* windows, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t S,
                                    const int32_t* oy, int32_t ny, const int32_t* ox, int32_t nx, void* stream) {
    WinOrigins org;
    bool vec;
    if (!win_prepare(canvas, windows, nullptr, batch, channels, H, W, S, oy, ny, ox, nx, org, vec)) return (int)hipErrorInvalidValue;
    const int64_t per_window = (int64_t)batch * channels * S * S;
    const int64_t lanes = vec ? per_window / 4 : per_window;   // < 2^29
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)(ny * nx));      // ny * nx <= 4096
#define PV_WG_LAUNCH(V)                                                                                                                          \
    hipLaunchKernelGGL((window_gather_kernel<V>), grid, dim3(256), 0, (hipStream_t)stream, canvas, windows, org, nx, ny * nx, channels, H, W, S, \
                       (long)lanes)
    if (vec) PV_WG_LAUNCH(4);
    else PV_WG_LAUNCH(1);
#undef PV_WG_LAUNCH
    return PV_CHECK_LAUNCH();
}

extern "C" int32_t pv_window_blend(const float* windows, const float* profile, float* canvas, int32_t batch, int32_t channels, int32_t H, int32_t W,
                                   int32_t S, const int32_t* oy, int32_t ny, const int32_t* ox, int32_t nx, void* stream) {
    WinOrigins org;
    bool vec;
    if (!win_prepare(canvas, windows, profile, batch, channels, H, W, S, oy, ny, ox, nx, org, vec)) return (int)hipErrorInvalidValue;
    const int64_t n_canvas = (int64_t)batch * channels * H * W;
    const int64_t lanes = vec ? n_canvas / 4 : n_canvas;       // < 2^29
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
#define PV_WB_LAUNCH(V)                                                                                                                                  \
    hipLaunchKernelGGL((window_blend_kernel<V>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, windows, profile, canvas, org, ny, nx, channels, H, W, \
                       S, (long)lanes)
    if (vec) PV_WB_LAUNCH(4);
    else PV_WB_LAUNCH(1);
#undef PV_WB_LAUNCH
    return PV_CHECK_LAUNCH();
}
