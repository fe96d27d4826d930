/*
 * photoverse_hip.h - C-ABI of libphotoverse_hip.so, the MI355X (gfx950) kernels behind the
 * PhotoVerse denoising hot path.
 *
 * The reference (idonahum/photoVerse) is pure Python on top of diffusers and has no FFI of
 * its own.  Its "operators" for this path are the vendor kernels the
 * eager PyTorch graph dispatches to.  Each entry point below replaces one family of those
 * dispatches; the call site in the reference that reaches it is cited per function.  The
 * Python host layer (photoverse_amd/) binds these with ctypes and mirrors the reference's
 * Python interfaces (attention-processor protocol, UNet call, run_inference).
 *
 * Conventions
 *   - plain C, raw device pointers, caller-owned outputs and workspace;
 *   - no allocation, no host synchronisation, safe under HIP stream capture;
 *   - every launcher returns a hipError_t value as int (0 = success) and enqueues on `stream`
 *     (a hipStream_t passed as void*);
 *   - activations are NHWC / token-major fp16: a (B,C,H,W) tensor of the reference is stored
 *     as rows [B*H*W][C] with an explicit row stride `ld*` in elements;
 *   - GEMM weights are fp16 [N][K] (torch Linear layout); 3x3 conv weights are repacked to
 *     [Cout][ky][kx][Cin];  biases / norm affine parameters are fp32.
 */
#ifndef PHOTOVERSE_HIP_H
#define PHOTOVERSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_ABI_VERSION 19

enum pv_act { PV_ACT_NONE = 0, PV_ACT_SILU = 1, PV_ACT_QUICK_GELU = 2, PV_ACT_LEAKY_RELU = 3, PV_ACT_GELU = 4,
              PV_ACT_RELU = 5 /* pv_tiny_conv3x3 only: every other launcher rejects it */ };

int pv_abi_version(void);
/* number of HIP devices visible, or -1 on runtime error; never initialises a context */
int pv_device_count(void);

/* ------------------------------------------------------------------------------------------
 * pv_gemm_conv: out[M][N] = epilogue( A[M][K] * W[N][K]^T ), MFMA f16 -> f32 accumulate.
 *   taps == 1 : Linear / 1x1 conv.  Replaces nn.Linear / Conv2d(k=1) dispatches of
 *               attention_processor.py:297,304-305,392-393,423 (to_q/to_k/to_v/to_k_ip/
 *               to_v_ip/to_out), adapters.py:14-28, and the [EXT] diffusers proj_in/proj_out/
 *               GEGLU/FF/time-embedding/conv_shortcut layers reached from infer.py:103-114.
 *   taps == 9 : implicit-GEMM 3x3 conv, zero padding, stride 1|2, optional nearest x2 upsample
 *               folded into the gather (ResnetBlock2D conv1/conv2, Downsample2D, Upsample2D).
 *   A may come from two tensors concatenated along channels (skip connections): channels
 *   [0,c0) from a0 and [c0,c0+c1) from a1; c0, c1 multiples of 64.
 *   epilogue: (+bias[n]) (+rowadd[img][n]) act (+residual[m][n]) -> fp16 (or fp32) store.
 *   Requirements: N % 128 == 0 or N % 160 == 0; (c0+c1) % 64 == 0; pointers 16-byte aligned; each operand < 2 GiB.
 */
typedef struct pv_gemm_params {
    const void* a0;        /* fp16 */
    const void* a1;        /* fp16 or NULL */
    int32_t c0, c1;        /* channels taken from a0 / a1 */
    int32_t lda0, lda1;    /* row strides in elements */
    const void* w;         /* fp16 [N][taps*(c0+c1)] */
    const float* bias;     /* [N] or NULL */
    const float* rowadd;   /* fp32 [images][rowadd_ld] added per image (time embedding) or NULL */
    int32_t rowadd_ld;     /* 0 => one row shared by all images */
    const void* residual;  /* fp16 [M][ldr] or NULL */
    int32_t ldr;
    void* out;             /* fp16 [M][ldc] (fp32 when out_f32) */
    int32_t ldc;
    int32_t M, N;
    int32_t taps;          /* 1 or 9 */
    int32_t batch, hin, win, hout, wout; /* taps==9 geometry; taps==1: hout*wout = rows per image */
    int32_t stride;        /* 1 or 2 */
    int32_t upsample;      /* 1 => logical input is the x2 nearest upsample of (hin,win) */
    int32_t pad;           /* taps==9: zero padding in front (top / left): 1 = Conv2d(padding=1) (every UNet / decoder conv);
                              0 = the VAE encoder's Downsample2D, F.pad(x,(0,1,0,1)) + Conv2d(stride=2,padding=0) (stride 2
                              only).  Reads past the bottom / right edge are zeros in both cases (hout, wout say how far). */
    int32_t act;           /* enum pv_act */
    int32_t out_f32;
    int32_t geglu;         /* 1 => W rows are tile-interleaved (value|gate); out[M][N/2] = value*gelu(gate) */
    int32_t splitk;        /* > 1: split the K loop over this many workgroups per tile (small-M layers); needs splitk_ws */
    float* splitk_ws;      /* fp32 workspace [splitk][M][N] for the partial slabs, reduced in fixed order */
    float* colstats;       /* optional fp32 [ceil(M/64)][2][N]: per 64-row block and output column, the sum and the sum of
                              squares of the (fp16-rounded) outputs - GroupNorm statistics of the tensor being written,
                              consumed by pv_groupnorm_stats_from_colstats.  NULL = off.  fp16 output, no geglu (with splitk > 1 the
                              reduce launch produces them). */
    const float* ln_rowsum; /* optional (ABI 12) fp32 [N]: sum_k w[n][k] of the fp16 weights.  Non-NULL = the launch computes
                              epilogue( LayerNorm_noaffine(a0) . w^T + bias ): BasicTransformerBlock.norm1 / norm3 [EXT] folded into the Linear that
                              follows it - the GEMM runs on the RAW rows and the epilogue applies rstd * (acc - mean * ln_rowsum[n]); the caller
                              folds the affine part (gamma scales the columns of w, w . beta joins the bias).  Row statistics come from the
                              fragments the MFMAs consume.  Only the 256-row-tile Linear path takes it (taps == 1, K >= 640, c1 == 0, no split-K,
                              N % 320 == 0 or geglu with N % 256 == 0, >= 256 tiles): anything else returns hipErrorInvalidValue. */
    float ln_eps;
    int32_t big_tile_min;  /* (ABI 12) 256-row-tile path (pv_convbig.hip): minimum number of 256-row tiles (x K slices) the launch must have to take it.
                              0 = library default (256 = one workgroup per CU; env PV_CONV_BIG overrides), < 0 = never.  A caller that runs two such
                              launches side by side on two streams (the uncond / cond forwards of a CFG step) passes 128: each fills half the chip. */
    const float* a_norm;   /* (ABI 15) optional fp32 [batch][2][c0+c1]: per image and INPUT channel (a0's channels, then a1's) the scale and the shift of a
                              GroupNorm over the conv's input, from pv_groupnorm_scale_shift.  Non-NULL = the launch computes conv( act_a( a * scale + shift ) ):
                              [EXT] ResnetBlock2D.norm1 / norm2 + SiLU folded into conv1 / conv2 - the conv reads the RAW tensor(s), each input pixel is
                              normalised once, in LDS, where the LDS-resident input patch of the 256-row tile holds it (zero padding stays zero), the same
                              fp32 arithmetic and fp16 rounding as pv_groupnorm_apply: results equal the two-launch path bit for bit.  Only that path takes it
                              (taps == 9, stride 1, no upsampling, 64- or 32-pixel image rows, no split-K): anything else returns hipErrorInvalidValue. */
    int32_t a_norm_act;    /* PV_ACT_NONE or PV_ACT_SILU, applied after the affine part */
} pv_gemm_params;
int pv_gemm_conv(const pv_gemm_params* p, void* stream);
/* (ABI 17) Which kernel pv_gemm_conv would launch for this block: the symbol as rocprofv3 prints it (without the namespace and the argument
 * list, e.g. "big_tile_kernel<true, false, 8, 3, false>") and the workgroup count (split-K slices included).  Same validation and the same dispatch
 * code as pv_gemm_conv with the launchers in describe-only mode: no HIP call, no GPU needed.  The host side tags its recorded launches with it
 * (bench.py's per-symbol roofline reads the tags); nothing in the reference corresponds (measurement scaffolding of this build). */
int pv_gemm_conv_kernel_info(const pv_gemm_params* p, char* name, int32_t name_len, int64_t* workgroups);

/* ------------------------------------------------------------------------------------------
 * GroupNorm(32 groups) over NHWC fp16, optionally over a channel concat of two tensors.
 * Replaces F.group_norm (+ SiLU) dispatches of [EXT] ResnetBlock2D.norm1/norm2,
 * Transformer2DModel.norm, conv_norm_out.
 *   pv_groupnorm_stats : partial (sum, sumsq) per (image, split, group) -> partial[B][S][G][2], then reduced in a
 *                        fixed order to (mean, rstd) stored at partial[b][0][g][0..1] (deterministic, no atomics)
 *   pv_groupnorm_apply : y = act(gamma*(x-mean)*rstd+beta), contiguous fp16 [B*HW][C]; must follow _stats
 */
typedef struct pv_groupnorm_params {
    const void* x0; const void* x1;  /* fp16 sources; x1 may be NULL */
    int32_t c0, c1, ld0, ld1;
    int32_t batch, hw, groups;
    int32_t splits;                  /* S: pixel splits per image */
    float* partial;                  /* [B][S][G][2] fp32 workspace */
    const float* gamma; const float* beta;
    float eps;
    int32_t act;                     /* PV_ACT_NONE or PV_ACT_SILU */
    void* y;                         /* fp16 [B*HW][c0+c1] */
    const float* colstats0;          /* pv_gemm_params.colstats of the launches that produced x0 / x1 (ld == c), or NULL */
    const float* colstats1;
} pv_groupnorm_params;
int pv_groupnorm_stats(const pv_groupnorm_params* p, void* stream);
/* same result as pv_groupnorm_stats, from the column statistics the producing GEMM epilogues left behind (no pass over x);
 * needs hw % 64 == 0, colstats0 (and colstats1 when c1 > 0); fixed reduction order */
int pv_groupnorm_stats_from_colstats(const pv_groupnorm_params* p, void* stream);
/* (ABI 15) the same statistics turned into the per-(image, channel) affine form a consumer can apply by itself:
 * table[b][0][c] = gamma[c] * rstd(b, group(c)), table[b][1][c] = beta[c] - mean(b, group(c)) * table[b][0][c]   (fp32 [batch][2][c0+c1]),
 * so that pv_groupnorm_apply's y = act(x * table[b][0][c] + table[b][1][c]) can be folded into the conv that follows (pv_gemm_params.a_norm).
 * Needs what pv_groupnorm_stats_from_colstats needs; also leaves (mean, rstd) in partial like it.  Fixed reduction order. */
int pv_groupnorm_scale_shift(const pv_groupnorm_params* p, float* table, void* stream);
int pv_groupnorm_apply(const pv_groupnorm_params* p, void* stream);

/* LayerNorm over the last dim of fp16 rows (BasicTransformerBlock.norm1-3, CLIP layer norms,
 * adapters.py:15,18 with LeakyReLU fused).  y = act(gamma*(x-mean)*rstd+beta) */
typedef struct pv_layernorm_params {
    const void* x; int32_t ldx;
    void* y; int32_t ldy;
    const float* gamma; const float* beta;
    int32_t rows, cols;              /* cols % 8 == 0, cols <= 4096 */
    float eps;
    int32_t act;
} pv_layernorm_params;
int pv_layernorm(const pv_layernorm_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flash-style self attention (stock AttnProcessor2_0 on attn1, unet.py:20-24; CLIP encoder
 * self-attention).  q,k,v are column slices of one fp16 buffer (fused QKV GEMM output):
 * head h uses columns [h*d,(h+1)*d) of each.  softmax scale = 1/sqrt(d).  d in {40,64,80,160}.
 */
typedef struct pv_attn_params {
    const void* q; const void* k; const void* v;
    int32_t ldq, ldk, ldv;
    void* out; int32_t ldo;
    int32_t batch, heads, nq, nk, d;
    int32_t causal;
    float* lse;                      /* optional fp32 [B][heads][nq]: log-sum-exp of the scaled scores in log2 units, kept for
                                        pv_attention_backward; NULL = not written */
} pv_attn_params;
int pv_attention(const pv_attn_params* p, void* stream);
/* (ABI 17) Which kernel pv_attention would launch for this block (pv_gemm_conv_kernel_info's contract): "attn8_kernel<497>", "attn_kernel<80, 2, false>", ... */
int pv_attention_kernel_info(const pv_attn_params* p, char* name, int32_t name_len, int64_t* workgroups);

/* Backward of pv_attention (the [EXT] AttnProcessor2_0 SDPA of attn1, models/unet.py:20-24, and the CLIP text layers the gradient
 * of text_adapter crosses, train.py:498-500).  Probabilities are recomputed from lse; delta: fp32 workspace [B][heads][nq]; qs: fp16 workspace like q.
 * dq / dk / dv: fp16 rows (may be column slices of one [dq | dk | dv] buffer).  d in {40, 64, 80, 160}.  Deterministic. */
typedef struct pv_attn_bwd_params {
    const void* q; const void* k; const void* v;
    int32_t ldq, ldk, ldv;
    const void* out; int32_t ldo;    /* the forward output O */
    const void* dout; int32_t lddo;
    const float* lse;
    float* delta;
    void* qs; int32_t ldqs;          /* fp16 workspace [B*nq][heads*d]: the scaled queries, written by the call */
    void* dq; void* dk; void* dv;
    int32_t lddq, lddk, lddv;
    int32_t batch, heads, nq, nk, d;
    int32_t causal;
    void* ws; int64_t ws_bytes;      /* optional workspace: with >= 2 * batch * heads * nq * 96 bytes (d = 40; * 224 at d = 80) the unmasked launches
                                      * with nq, nk % 512 == 0 (d = 40) / % 256 == 0 (d = 80) take the 8-wave staggered kernels (pv_attnbwd.hip);
                                      * NULL = the 4-wave kernels */
} pv_attn_bwd_params;
int pv_attention_backward(const pv_attn_bwd_params* p, void* stream);

/* GroupNorm (+ SiLU) backward over NHWC fp16 ([EXT] ResnetBlock2D.norm1/2, Transformer2DModel.norm, conv_norm_out): data gradient
 * only (the affine parameters are frozen in train.py).  stats: the forward's pv_groupnorm_params.partial after the statistics launch
 * ((mean, rstd) at stats[b * stats_stride + g * 2]); partial: fp32 [B][splits][2][C]; sums: fp32 [B][groups][2].
 * dx0 / dx1 receive the gradient of x0 / x1 (+ add0 / add1 when given - gradient accumulation of a tensor with several consumers);
 * a NULL dx is skipped. */
typedef struct pv_groupnorm_bwd_params {
    const void* x0; const void* x1;
    int32_t c0, c1, ld0, ld1;
    int32_t batch, hw, groups, splits;
    const float* stats; int32_t stats_stride;
    const float* gamma; const float* beta;
    int32_t act;
    const void* dy; int32_t ld_dy;
    float* partial; float* sums;
    void* dx0; int32_t ld_dx0; const void* add0; int32_t ld_add0;
    void* dx1; int32_t ld_dx1; const void* add1; int32_t ld_add1;
} pv_groupnorm_bwd_params;
int pv_groupnorm_backward(const pv_groupnorm_bwd_params* p, void* stream);
/* GEGLU backward: h = [value | gate] fp16 [rows][2n] (pre-activation of GEGLU.proj), dy [rows][n] -> dh [rows][2n] */
int pv_geglu_backward(const void* h, int32_t ldh, const void* dy, int32_t lddy, void* dh, int32_t lddh, int32_t rows, int32_t n, void* stream);
/* dx = dy * act'(x) for a saved pre-activation x (quick-GELU of the CLIP MLP, SiLU, LeakyReLU, GELU) */
int pv_act_backward(const void* x, int32_t ldx, const void* dy, int32_t lddy, void* dx, int32_t lddx, int32_t rows, int32_t cols, int32_t act,
                    void* stream);
/* y = act(x) as its own pass (the training forward keeps the pre-activation) */
int pv_act_forward(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t rows, int32_t cols, int32_t act, void* stream);
/* Dropout on the input of a LoRA branch (peft LoRA layer: result += B(A(dropout(x))) * scaling; train.py:265-270).  Counter-based
 * (Philox4x32-10): the keep mask is a function of (rng key, site, rng[2] = iteration, copy, element), recomputed by the backward.
 * forward: out[r][k*cols + c] = x[r][c] * keep_k / (1-p), k < copies (several independently masked copies side by side);
 * backward: out[r][c] = sum_k x[r][k*cols + c] * keep_k / (1-p) (+ add).  rng: the {key lo, key hi, counter} block of pv_fusion_draw.
 * The mask: the 8-column chunk q = r * (cols / 8) + c / 8 of copy k draws ONE Philox block, key (rng[0], rng[1]), counter (q, site, rng[2], k); its
 * element j = c % 8 takes the 16-bit lane (word[j / 2] >> (16 * (j % 2))) & 0xFFFF and is kept when lane >= uint32(p * 65536) (p = 0 keeps
 * everything).  1 / (1 - p) is formed in fp32; the backward adds `add`, then the copies in k order, in fp32; one fp16 rounding at the store.
 * cols % 8 == 0, 1 <= copies <= 4, 0 <= p < 1. */
int pv_dropout_f16(const void* x, int32_t ldx, void* out, int32_t ldo, const void* add, int32_t ldadd, int32_t rows, int32_t cols, int32_t copies,
                   float p, const int32_t* rng, int32_t site, int32_t backward, void* stream);
/* ---- the ArcFace identity loss (models/loss.py, models/arcface_resnet.py; train.py:521-535) and the VAE-decoder backward under it ---- */
/* y = x * scale[c] + shift[c] over fp16 rows: an eval-mode BatchNorm in FRONT of a zero-padded conv (IRBlock.bn0, bn4, arcface_resnet.py:18,82);
 * shift == NULL: its backward */
int pv_col_affine_f16(const void* x, int32_t ldx, const float* scale, const float* shift, void* y, int32_t ldy, int32_t rows, int32_t cols, void* stream);
/* nn.PReLU() with one slope (device scalar): dy == NULL: out = prelu(x); else out = dy * prelu'(x) */
int pv_prelu_f16(const void* x, int32_t ldx, const void* dy, int32_t lddy, const float* slope, void* out, int32_t ldo, int32_t rows, int32_t cols,
                 void* stream);
/* nn.MaxPool2d(2, 2) over NHWC fp16 (B,h,w,c): dy == NULL: out (B,h/2,w/2,c); else out (B,h,w,c) = dy routed to each window's first maximum */
int pv_maxpool2x2(const void* x, const void* dy, void* out, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* FaceLoss.preprocess (loss.py:26-62): y (B,1,size,size) = bilinear(align_corners=False) of gray(x) * mul + add; x fp32 (B,3,h,w) with the given
 * image stride (elements).  _backward: dx (B,3,h,w) contiguous from dy (B,1,size,size) with its image stride; deterministic gather.
 * gray = 0.2989 r + 0.5870 g + 0.1140 b.  Taps of one axis (in -> size), evaluated in fp32 as written: src = max((o + 0.5) * (in / size) - 0.5, 0),
 * i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), weights (1 - t, t) with t = src - i0; y = (1 - ty) * row(y0) + ty * row(y1), each row
 * (1 - tx) * gray[x0] + tx * gray[x1].  The backward gives input pixel (iy, ix) the sum over the outputs whose taps include it of
 * wy(oy, iy) * wx(ox, ix) * dy[oy][ox], outputs in row-major order, times mul, times the channel's gray weight. */
int pv_gray_resize(const float* x, int64_t x_image_stride, float* y, int32_t batch, int32_t h, int32_t w, int32_t size, float mul, float add, void* stream);
int pv_gray_resize_backward(const float* dy, int64_t dy_image_stride, float* dx, int32_t batch, int32_t h, int32_t w, int32_t size, float mul, void* stream);
/* nn.CosineEmbeddingLoss (margin 0) per sample: target > 0: 1 - cos(e1, e2), else max(0, cos); e1 / e2 fp16 [batch][dim];
 * de2 (optional, fp16) = gscale / batch * d(loss_b)/d(e2_b) - the gradient of the batch MEAN times gscale.
 * cos = ab / sqrt((aa + 1e-8) * (cc + 1e-8)) with ab = e1.e2, aa = e1.e1, cc = e2.e2 (fp32: 64 lanes of ceil(dim / 64) terms each, then a tree);
 * d(cos)/d(e2) = e1 / sqrt(..) - cos * e2 / (cc + 1e-8); a cosine <= 0 with target <= 0 has loss 0 and gradient 0. */
int pv_cosine_embedding_loss(const void* e1, const void* e2, int32_t batch, int32_t dim, float target, float gscale, float* per_sample, void* de2,
                             void* stream);
/* in-place backward of pv_softmax_rows: dp <- scale * p * (dp - sum_j p_j dp_j) per row */
/* Weight gradient of a Linear layer (loss.backward() reaching a trainable weight, train.py:536): partial slabs
 * out[s][n][k] (fp32, s < nsplit) = sum over rows m in [s * rows_per_split, min(m, (s + 1) * rows_per_split)) of dy[m][n] * x[m][k] -
 * both operands fp16 row matrices as the forward / data-gradient chain leaves them (no transposed copies; the MFMA operands are read with the
 * transposing LDS load).  n, k, lddy, ldx multiples of 8; rows_per_split a multiple of 64.  Sum the slabs in s order with pv_reduce_blocks
 * (nblk = nsplit, inner = n * k): deterministic. */
int pv_wgrad_tn(const void* dy, int32_t lddy, const void* x, int32_t ldx, int32_t m, int32_t n, int32_t k, float* out, int32_t nsplit,
                int32_t rows_per_split, void* stream);
int pv_softmax_rows_backward(const void* p, int32_t ldp, void* dp, int32_t lddp, int32_t rows, int32_t cols, float scale, void* stream);
/* out = dy where lo < y < hi else 0: gradient of images.clamp(-1, 1) (infer.py:122) */
int pv_clamp_mask_f32(const float* y, const float* dy, float lo, float hi, float* out, int64_t n, void* stream);
/* out = a + b over fp16 rows (gradient accumulation) */
int pv_add_rows_f16(const void* a, int32_t lda, const void* b, int32_t ldb, void* out, int32_t ldo, int32_t rows, int32_t cols, void* stream);
/* z (B,2h,2w,c) = x (B,h,w,c) at the even positions, 0 elsewhere: input of the data gradient of a stride-2 3x3 conv (Downsample2D) */
int pv_dilate2x(const void* x, int32_t ldx, void* z, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* out (B,h,w,c) = 2x2 block sums of g (B,2h,2w,c) (+ add): gradient of the x2 nearest upsample (Upsample2D) */
int pv_pool2x_sum(const void* g, const void* add, int32_t ldadd, void* out, int32_t batch, int32_t h, int32_t w, int32_t c, void* stream);
/* out = coef * sign(x): gradient of |x|.mean() (train.py:509, coef = weight / n) */
int pv_sign_f32(const float* x, float coef, float* out, int64_t n, void* stream);
/* out[b][e][:] = scale * x[b*seq + idx[b] + e][:] (fp16 rows -> fp32): gradient of the rows _inject_concept_embeddings wrote (clip.py:17-24) */
int pv_gather_rows_f32(const void* x, int32_t ldx, const int32_t* idx, float* out, int32_t batch, int32_t seq, int32_t n_e, int32_t dim, float scale,
                       void* stream);

/* Fused dual-branch cross attention = the SDPA part of PhotoVerseAttnProcessor2_0.__call__
 * (attention_processor.py:307-322 text branch, :392-420 image-token branch and fusion):
 *   out = w_text * softmax(q Kt^T / sqrt(d)) Vt  +  w_ip * softmax(q Kip^T / sqrt(d)) Vip
 * with two INDEPENDENT softmaxes.  (w_text,w_ip) = (1,1) under no_grad (:411-412); the
 * grad-mode fusion rule (:413-420) selects (2,0), (0,2) or (1,1).
 * Also emits to_v_ip_norm[b][h][p] = ||Vip[b,p,h,:]||_2 (:397) when vnorm != NULL.
 * nt <= 77+..., nt + nip <= 96.
 */
typedef struct pv_xattn_params {
    const void* q; int32_t ldq;
    const void* kt; const void* vt; int32_t ldkt, ldvt;   /* text K/V rows [B*nt] */
    const void* kip; const void* vip; int32_t ldkip, ldvip; /* image-token K/V rows [B*nip] */
    void* out; int32_t ldo;
    float* vnorm;                                          /* [B][H][nip] or NULL */
    int32_t batch, heads, nq, nt, nip, d;
    float w_text, w_ip;
    const float* fusion;                                   /* optional DEVICE pair overriding (w_text, w_ip), see pv_fusion_draw */
} pv_xattn_params;
int pv_cross_attention(const pv_xattn_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole attn2 branch of a BasicTransformerBlock as ONE launch (heads = 8; C = heads*d = 320 / d = 40 or C = 640 / d = 80):
 *   out = hs + to_out( w_text*softmax(q Kt^T/sqrt(d)) Vt + w_ip*softmax(q Kip^T/sqrt(d)) Vip ) + bias_o,
 *   q = to_q(LayerNorm(hs))
 * = BasicTransformerBlock.norm2 [EXT diffusers] -> PhotoVerseAttnProcessor2_0.__call__
 * (attention_processor.py:297 to_q, :307-322 text SDPA, :392-420 image-token SDPA + fusion rule,
 * :423 to_out[0]) -> the block's residual add.  Replaces pv_layernorm + pv_gemm_conv +
 * pv_cross_attention + pv_gemm_conv.  nq % 128 == 0, 64 < nt <= 80, nip <= 16.
 *
 * pv_xattn_pack_kv (once per conditioning) turns the projected text / image-token K,V rows into
 * the kernel's K / V images (kimg: batch*heads*96*64 halfs at d = 40, *128 at d = 80; vimg: batch*(C/80)*96*80 halfs) and
 * emits to_v_ip_norm (:397).  wo is to_out[0].weight with its COLUMNS reordered: column slot s of
 * the packed matrix holds natural column pv_xattn_fused_wo_slot(s).
 */
typedef struct pv_xattn_fused_params {
    const void* hs; int32_t ld_hs;             /* fp16 [batch*nq][C]: block input (pre-norm2) = residual */
    int32_t ln; float ln_eps;                  /* ln != 0: q = to_q((hs - mean) * rstd) - norm2 WITHOUT its affine part, which the */
                                               /* caller folds into wq (gamma scales its columns) and q_bias (= to_q.weight . beta) */
    const void* wq;                            /* fp16 [C][C] to_q.weight (x diag(gamma) when ln) */
    const float* q_bias;                       /* fp32 [C] added to q, or NULL */
    const void* wo;                            /* fp16 [C][C] to_out[0].weight, columns in slot order */
    const float* bias_o;                       /* fp32 [C] or NULL */
    const void* kimg; const void* vimg;        /* from pv_xattn_pack_kv */
    void* out; int32_t ld_out;                 /* fp16 [batch*nq][C] */
    int32_t batch, nq, heads, d, nt, nip;
    float w_text, w_ip;                        /* branch weights: (1,1) no_grad; (2,0) / (0,2) / (1,1) grad mode */
    const float* fusion;                       /* optional DEVICE pair overriding (w_text, w_ip): graph-safe grad-mode fusion */
    int32_t rows_per_workgroup;                /* C = 640 only; 0 = the launch decides (64-row workgroups while 128-row ones would not fill the chip: */
                                               /* < 384), 64 / 128 = the caller's choice: a caller that runs two such launches side by side on two */
                                               /* streams (the uncond / cond forwards, infer.py:103-114) asks for 128.  Same results either way (ABI 13) */
} pv_xattn_fused_params;
int pv_cross_attention_fused(const pv_xattn_fused_params* p, void* stream);
int pv_xattn_pack_kv(const void* kt, const void* vt, int32_t ldkt, int32_t ldvt, const void* kip, const void* vip,
                     int32_t ldkip, int32_t ldvip, void* kimg, void* vimg, float* vnorm, int32_t batch,
                     int32_t heads, int32_t d, int32_t nt, int32_t nip, void* stream);
int pv_xattn_fused_wo_slot(int32_t slot);

/* ------------------------------------------------------------------------------------------
 * The C = 1280 / d = 160 attn2 layers (16x16 and 8x8 levels): norm2 -> to_q -> dual-branch SDPA + fusion in ONE head-parallel
 * launch (one workgroup = 128 query rows of ONE head); attn.to_out[0] + bias + the block's residual add follow as one pv_gemm_conv.
 * Replaces pv_layernorm + pv_gemm_conv (to_q, attention_processor.py:297) + pv_cross_attention (:307-322, :392-420) - two launches
 * per layer instead of four (the one-launch pv_cross_attention_fused exists for C = 320 / 640).
 *   ctx[b, m, h*d:(h+1)*d] = w_text*softmax(q Kt^T/sqrt(d)) Vt + w_ip*softmax(q Kip^T/sqrt(d)) Vip,  q = to_q(LayerNorm(hs))[:, head h]
 * norm2 is folded algebraically so that the GEMM reads the raw rows: to_q(LN(x)) = rstd * (wq . x - mean * wq_rowsum) + q_bias with
 * wq = to_q.weight x diag(gamma) (fp16), wq_rowsum[n] = sum_k wq[n][k] (of the fp16 values), q_bias = to_q.weight . beta.
 * d in {160, 80} (80: two heads per 160-feature block); C = heads*d a multiple of 320 (whole 160-feature blocks, and the to_q GEMM walks K = C in
 * 64-deep stages: anything else returns hipErrorInvalidValue); every row extent (batch*nq*ld_hs, ...) below 2 GiB; nt <= 80, nip <= 16; K / V rows as for pv_cross_attention.  (ABI 11)
 */
typedef struct pv_xattn_lnq_params {
    const void* hs; int32_t ld_hs;             /* fp16 [batch*nq][heads*d]: block input (pre-norm2) */
    int32_t ln; float ln_eps;                  /* ln != 0: LayerNorm statistics over the row, affine part folded by the caller */
    const void* wq;                            /* fp16 [C][C] */
    const float* q_bias;                       /* fp32 [C] or NULL */
    const float* wq_rowsum;                    /* fp32 [C]; required when ln */
    const void* kt; const void* vt; int32_t ldkt, ldvt;       /* text K / V rows [batch*nt] */
    const void* kip; const void* vip; int32_t ldkip, ldvip;   /* image-token K / V rows [batch*nip] */
    void* out; int32_t ldo;                    /* fp16 ctx [batch*nq][C] */
    float* vnorm;                              /* [batch][heads][nip] to_v_ip_norm (:397) or NULL */
    int32_t batch, nq, heads, d, nt, nip;
    float w_text, w_ip;
    const float* fusion;                       /* optional DEVICE pair overriding (w_text, w_ip), see pv_fusion_draw */
} pv_xattn_lnq_params;
int pv_cross_attention_lnq(const pv_xattn_lnq_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * pv_row_gemm: LayerNorm + Linear (+ GEGLU gate) for the K = 320 layers of the 64x64-level transformer blocks as ONE row-owning
 * launch: BasicTransformerBlock.norm1 -> [to_q; to_k; to_v] of attn1 (stock AttnProcessor2_0, /root/reference/models/unet.py:20-24) and
 * norm3 -> ff.net[0] (GEGLU) [EXT diffusers transformer block, driven by /root/reference/models/infer.py:103-114].
 *   out[M][N'] = epi( ((x - mean) * rstd)[M][320] . w[N][320]^T + bias ),  N' = N, or N / 2 with geglu (value * gelu_erf(gate))
 * ln != 0: rows are normalised WITHOUT the affine part - the caller folds gamma into the columns of w and w . beta into bias.
 * geglu: w / bias rows packed per 160-row chunk c as 10 fragments of 16 rows, fragment 2q = value rows of output columns
 * 80 c + 16 q .. + 15, fragment 2q + 1 = their gate rows.  N % 320 == 0; K must be 320; M arbitrary (tails through the descriptors).
 */
typedef struct pv_row_gemm_params {
    const void* x; int32_t ld_x;               /* fp16 [M][K] rows */
    int32_t M, K, N;
    const void* w;                             /* fp16 [N][K] */
    const float* bias;                         /* fp32 [N] or NULL */
    int32_t ln; float ln_eps;
    int32_t geglu;
    void* out; int32_t ld_out;                 /* fp16 [M][N or N/2] */
    const float* x_norm;                       /* (ABI 15) optional fp32 [images][2][K]: a GroupNorm of the rows as a per-(image, channel) scale / shift
                                                  (pv_groupnorm_scale_shift): the launch computes epi( (x * scale + shift) . w^T + bias ) - [EXT]
                                                  Transformer2DModel.norm folded into proj_in on the raw tensor, the normalised rows rounded to fp16 exactly as
                                                  pv_groupnorm_apply writes them.  Needs rows_per_image % 128 == 0; not together with ln */
    int32_t rows_per_image;
} pv_row_gemm_params;
int pv_row_gemm(const pv_row_gemm_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * BACKWARD of PhotoVerse's own trainable modules (the backward of the stock SD-v1.5 / CLIP blocks the gradient crosses is
 * declared further up: pv_attention_backward, pv_groupnorm_backward, ...).
 *
 * pv_cross_attention_backward: gradient of the dual-branch SDPA (attention_processor.py:317-322,
 * :392-420) given dout = dL/d(attention output before to_out):
 *   dq   fp16 [B*nq][C]         dkt, dvt  fp32 [B*nt][C]        dkip, dvip  fp32 [B*nip][C]
 * every output is multiplied by out_scale (un-scaling of a loss-scaled dout); dvip additionally gets
 * (vnorm_coef + vnorm_grad[b][h][p]) * v / ||v||_head (gradient through to_v_ip_norm, :397 / train.py:512-513)
 * before that scaling.  partial: fp32 workspace batch*heads*ceil(nq/512)*2*96*d.  MFMA (pv_train.hip).  Deterministic.
 */
typedef struct pv_xattn_bwd_params {
    const void* q; int32_t ldq;
    const void* kt; const void* vt; int32_t ldkt, ldvt;
    const void* kip; const void* vip; int32_t ldkip, ldvip;
    const void* dout; int32_t lddo;
    void* dq; int32_t lddq;
    float* partial;
    float* stats;                      /* fp32 workspace [B][heads][nq][4]: per-query (lse_text, lse_ip, delta_text, delta_ip) */
    float* dkt; float* dvt; float* dkip; float* dvip;
    int32_t ld_dt, ld_di;              /* row strides (floats) of dkt / dvt and of dkip / dvip (e.g. 2C for a [dK | dV] buffer) */
    int32_t batch, heads, nq, nt, nip, d;
    float w_text, w_ip;
    const float* fusion;               /* optional device pair overriding (w_text, w_ip) */
    float out_scale, vnorm_coef;
    const float* vnorm_grad;           /* optional dL/d(to_v_ip_norm) fp32 [B][heads][nip], added to vnorm_coef per (b, h, p) */
} pv_xattn_bwd_params;
int pv_cross_attention_backward(const pv_xattn_bwd_params* p, void* stream);
/* out[c][r] = x[r][c] (fp16), rows zero-padded to rows_pad: operand layout of dW = dY^T . X on pv_gemm_conv */
int pv_transpose_f16(const void* x, int32_t ldx, int32_t rows, int32_t cols, void* out, int32_t ldo, int32_t rows_pad, void* stream);
/* LayerNorm (+ LeakyReLU) backward (adapters.py:15-19): dx fp16; dgb_partial (optional) fp32 [ceil(rows / (4 * rows_per_wave))][2][cols] =
 * per-row-block (dgamma, dbeta) terms, to be summed with pv_reduce_blocks.  act: PV_ACT_NONE or PV_ACT_LEAKY_RELU.
 *   g = dy * dy_scale * act'(gamma * xhat + beta), dxhat = g * gamma, dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat)) (+ add);
 *   block b of dgb_partial = (sum g * xhat, sum g) over its rows (each wave its rows_per_wave rows in order, then the four waves in order).
 * Without dgb_partial, with cols % 8 == 0 and every row stride a multiple of 8, a vector form runs LPR lanes per row (4 * 64 / LPR rows per
 * workgroup), chosen by cols / 8: <= 40: 8, <= 96: 16, <= 160: 32, else 64 (six instantiations: <= 40, 80, 96, 128, 160 chunks and above);
 * otherwise one wave per row.  cols <= 2048. */
typedef struct pv_layernorm_bwd_params {
    const void* x; int32_t ldx;
    const void* dy; int32_t lddy;
    void* dx; int32_t lddx;
    const float* gamma; const float* beta;
    float* dgb_partial;
    int32_t rows, cols;
    float eps;
    int32_t act;
    int32_t dy_group, dy_skip;         /* dy_group > 1: row r reads dy row r / dy_group; the first dy_skip rows of a group get 0 */
    float dy_scale;                    /* multiplies dy (1 / count of a mean; 1.0 otherwise) */
    int32_t rows_per_wave;             /* rows each wave walks (0 = 1): dgb_partial has ceil(rows / (4 * rows_per_wave)) blocks */
    const void* add; int32_t ldadd;    /* optional fp16 [rows][cols]: dx = LayerNorm gradient + add (the gradient x already holds from its other */
                                       /* consumers - the residual stream: one launch instead of the gradient + an add pass) (ABI 14) */
} pv_layernorm_bwd_params;
int pv_layernorm_backward(const pv_layernorm_bwd_params* p, void* stream);
/* out[i] = scale * sum_b x[b][i] (x: fp32 [nblk][inner]), in a fixed order (deterministic): eight groups, group g adds the blocks g, g + 8, g + 16, ...
 * - while four of them 8 apart remain, into four accumulators (a0..a3, each taking every 32nd block), the up to three left over into a0 - and
 * closes with (a0 + a1) + (a2 + a3); the eight group sums are then added in g order and multiplied by scale. */
int pv_reduce_blocks(const float* x, int32_t nblk, int64_t inner, float scale, float* out, void* stream);
/* out[0] = scale * sum(a^2), deterministic (gradient norms of clip_grad_norm_): the reduction order of pv_reduce_mean (partial: n_partial floats) */
int pv_reduce_sumsq(const float* a, int64_t n, float scale, float* partial, int32_t n_partial, float* out, void* stream);
/* Multi-tensor forms of the three optimizer launches: ONE launch each over every parameter tensor.  entries: int64 [T][6] =
 * {param, grad, exp_avg, exp_avg_sq, gscale pointer (or 0), n}; workgroup b handles elements [blk_chunk[b] * chunk, + chunk) of tensor
 * blk_tensor[b].  pv_sumsq_multi: partial[b] = sum of grad^2 of that range; pv_clip_coef_groups: group g owns partial[group_start[g] ..
 * group_start[g+1]): out[2g] = base * min(1, max_norm / (base * sqrt(sum) + 1e-6)), out[2g+1] = base * sqrt(sum) (base = 1 / loss scale);
 * pv_adamw_multi: the AdamW update (torch.optim.AdamW, train.py:372-377, :545) of every range, reading its tensor's gscale.
 * Overflow guard (fp16 gradients under a static loss scale): when any group norm is not finite, pv_clip_coef_groups writes -1 into every
 * out[2g] and adds 1 to counters[1]; otherwise it adds 1 to counters[0] (applied steps).  pv_adamw_multi skips tensors whose gscale is
 * negative and, given counters, takes its bias-correction step from counters[0] instead of `step` - the behaviour of torch's GradScaler,
 * without a host synchronisation.  counters may be NULL (no guard bookkeeping; `step` is used).  `out` holds groups + 1 rows of two floats: the
 * extra row [groups] = {base, 0}, or {-1, 0} on overflow, is the gscale of tensors in NO clip group (skipped with the rest); with counters[0] == 0
 * (nothing applied yet) pv_adamw_multi leaves everything untouched (ABI 10). */
int pv_sumsq_multi(const int64_t* entries, const int32_t* blk_tensor, const int32_t* blk_chunk, int32_t n_blocks, int32_t chunk, float* partial, void* stream);
int pv_clip_coef_groups(const float* partial, const int32_t* group_start, int32_t groups, float max_norm, float base, float* out, int32_t* counters,
                        void* stream);
int pv_adamw_multi(const int64_t* entries, const int32_t* blk_tensor, const int32_t* blk_chunk, int32_t n_blocks, int32_t chunk, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int32_t step, const int32_t* counters, void* stream);
/* The fp16 working copies of the trainable weights, re-made from their fp32 masters after every optimizer step (the reference's autocast does
 * the same cast inside every Linear, train.py:464-470) - ONE launch over all of them.  entries: int64 [E][9] = {src (fp32), ld_src, rows, cols,
 * scale (float bits in the low word), dst (fp16), ld_dst, dstT (fp16 or 0), ld_dstT}: dst[r][c] = fp16(scale * src[r][c]) and, when given,
 * dstT[c][r] = the same value (the transposed operand of the data-gradient GEMM).  Workgroup b handles the 32 x 32 tile blk_tile[b] (row-major
 * over ceil(rows/32) x ceil(cols/32)) of entry blk_entry[b].  A destination may be a block of a larger zero-padded matrix (block-diagonal LoRA
 * factors, stacked k / v projections). */
int pv_pack_weights(const int64_t* entries, const int32_t* blk_entry, const int32_t* blk_tile, int32_t n_blocks, void* stream);
/* out[c] = sum_r x[r][c] over fp16 rows (bias gradients); partial: nblk*cols floats of workspace.  Block b adds the rows
 * [b * rpb, min(rows, (b + 1) * rpb)), rpb = ceil(rows / nblk), in row order in fp32 (a block past the last row holds 0); the nblk block sums are
 * then added in pv_reduce_blocks' order. */
int pv_colsum_f16(const void* x, int32_t ldx, int32_t rows, int32_t cols, float* partial, int32_t nblk, float* out, void* stream);

/* GEGLU gate (diffusers GEGLU, exact-erf GELU): out[m][j] = x[m][j] * gelu(x[m][n+j]) */
int pv_geglu(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t rows, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Step-state driven pieces of the denoising loop (infer.py:98-119).  `state` is a small device
 * block of int32: step index at state[0], number of table rows at state[1] (0 = unknown); the
 * tables are indexed with min(state[0], state[1]-1) so that ONE captured HIP graph can be
 * replayed for every step and a step past the end of the schedule never reads beyond them.
 */
/* sinusoidal timestep embedding (flip_sin_to_cos, shift 0) -> fp16 [rows][dim];
 * t taken from timesteps[state ? *state : 0 ... ] : rows>1 => per-row timesteps[row] */
int pv_timestep_embedding(const float* timesteps, const int32_t* state, int32_t rows, int32_t dim,
                          void* out, void* stream);
/* conv_out: NHWC fp16 (B,H,W,cin) -> NCHW fp32 (B,cout,H,W), 3x3 pad 1; w fp16 [cout][3][3][cin]; cout 4 (UNet) or 3 (VAE);
 * cin in {64, 128, 256, 320, 512} (512: the data gradient of the VAE decoder's conv_in) */
int pv_conv_out(const void* x, const void* w, const float* bias, float* out, int32_t batch, int32_t cin,
                int32_t h, int32_t wd, int32_t cout, void* stream);
/* CFG combine (infer.py:116) + DPM-Solver++(2M) update (infer.py:119) on fp32 NCHW latents.
 * coef[step][4] = {c_x, c_eps, c_x0, c_x0prev}:  x0 = inv_alpha*x - sig_over_alpha*eps ... see
 * photoverse_amd/scheduler.py; advances nothing (pv_step_advance does). */
int pv_cfg_dpm_step(const float* eps_uncond, const float* eps_cond, float* latents, float* x0_prev,
                    const float* coef, const int32_t* state, float guidance, int64_t n, void* stream);
int pv_step_advance(int32_t* state, void* stream);
/* (ABI 18) pv_cfg_dpm_step + the inpainting blend of a 4-channel UNet, in the same launch.  Nothing in the reference: replaces the
 * per-step `latents = (1 - init_mask) * init_latents_proper + init_mask * latents` of [EXT] diffusers'
 * StableDiffusionInpaintPipeline (with init_latents_proper = scheduler.add_noise(image_latents, noise, t_next), the clean
 * image latents after the last step).  Same contract as pv_cfg_dpm_step; in addition the row's coef[5], coef[6] = {q0, q1}:
 *   k = q0*known + q1*noise;   latents = m*x_next + (1-m)*k      (m == 1 -> pv_cfg_dpm_step's bits, m == 0 -> k exactly)
 * mask fp32 [B][1][hw] broadcast over `channels`; known / noise fp32 like latents, read only; x0_prev receives the unblended x0.
 * hw % 4 == 0 and n % (channels*hw) == 0. */
int pv_cfg_dpm_step_masked(const float* eps_uncond, const float* eps_cond, float* latents, float* x0_prev,
                           const float* coef, const int32_t* state, float guidance, const float* mask, const float* known,
                           const float* noise, int32_t channels, int32_t hw, int64_t n, void* stream);
/* (ABI 19, a symbol added) pv_cfg_dpm_step / _masked with separate guidance scales and a rescale of the guided prediction.  Nothing in the
 * reference: [EXT] the InstructPix2Pix split of classifier-free guidance and diffusers' guidance_rescale.  Per sample b over its
 * chw = channels*hw elements, coefficient row as above:
 *   e  = eu + g_text*(ec - eu)                          eps_image == NULL (pv_cfg_dpm_step's expression)
 *   e  = eu + g_image*(em - eu) + g_text*(ec - em)      otherwise; em = eps(uncond text, cond image tokens)
 *        (g_image == g_text: the em terms cancel and the first expression is evaluated - the bits of the two-forward step; em is not read)
 *   f  = rescale*std_b(ec)/std_b(e) + (1 - rescale)     if rescale > 0 and std_b(e) > 0, else 1;   e = f*e
 *   x0, x_next as pv_cfg_dpm_step; with mask / known / noise (all three or none) the blend of pv_cfg_dpm_step_masked.
 * std_b: two passes (mean, then squared deviations) in fp32, one workgroup per sample, no atomics: replays are bit-identical.
 * eps_image == NULL, rescale == 0 gives the bits of pv_cfg_dpm_step (no mask) / pv_cfg_dpm_step_masked (mask).  eps_* are read only.
 * hw % 4 == 0, rescale in [0, 1], finite scales, batch*chw < 2^31. */
int pv_cfg_dpm_step_guided(const float* eps_uncond, const float* eps_image, const float* eps_cond, float* latents, float* x0_prev,
                           const float* coef, const int32_t* state, float g_text, float g_image, float rescale, const float* mask,
                           const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw, void* stream);
/* (ABI 19, a symbol added) pv_cfg_dpm_step_guided as the step of the STOCHASTIC solver SDE-DPM-Solver++(2M) ([EXT] diffusers'
 * algorithm_type="sde-dpmsolver++", first-order and midpoint second-order updates): the guided step above, then
 *   xn += cn * z        cn = column 7 of the coefficient row {ca, cb, cx, c0, c1, q0, q1, cn}, z ~ N(0, I) fresh per step
 * before the inpainting blend (the kept region stays on the re-noised known latents); x0_prev gets x0 as before.  The rows of the SDE table
 * (scheduler.coefficient_table of that type), h = lambda_t - lambda_s, r0 = h_prev / h:
 *   A = alpha_t (1 - exp(-2h)),  cx = (sigma_t / sigma_s) exp(-h),  cn = sigma_t sqrt(1 - exp(-2h))
 *   first order: c0 = A, c1 = 0;   second order: c0 = A (1 + 1/(2 r0)), c1 = -A / (2 r0);   last row (sigma_t = 0): cx = 0, c0 = 1, c1 = 0, cn = 0.
 * The noise is generated in the kernel and is part of the interface.  rng = four device words {seed_lo, seed_hi, sample_offset, stream}.  The
 * thread that owns elements 4q .. 4q+3 of sample b (q = offset inside the sample's chw elements / 4) evaluates one Philox4x32-10 block with
 *   key (seed_lo, seed_hi),  counter (q, sample_offset + b, step, stream),  step = the clamped step index of `state`
 * and turns its words w0..w3 into four normals by Box-Muller:
 *   u_k = ((w_k >> 9) + 0.5) * 2^-23                      exact in fp32, strictly inside (0, 1)
 *   z0 = r0 cos(2 pi u1), z1 = r0 sin(2 pi u1), r0 = sqrt(-2 ln u0);   z2 = r1 cos(2 pi u3), z3 = r1 sin(2 pi u3), r1 = sqrt(-2 ln u2)
 * (sincospif(2 u), accurate logf).  Everything the noise depends on is contents of device buffers - the step counter and rng -, so a captured
 * launch serves any seed, start row and batch offset; no atomics: a replay gives the bits of an eager run.  Sample b at sample_offset s gets the
 * noise of sample 0 at sample_offset s + b.  rng must not be NULL; every other argument and limit as pv_cfg_dpm_step_guided. */
int pv_cfg_dpm_step_stochastic(const float* eps_uncond, const float* eps_image, const float* eps_cond, float* latents, float* x0_prev,
                               const float* coef, const int32_t* state, const uint32_t* rng, float g_text, float g_image, float rescale,
                               const float* mask, const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw,
                               void* stream);
/* (ABI 19, a symbol added) pv_cfg_dpm_step_guided / _stochastic with one more prediction: [EXT] perturbed-attention guidance (Ahn et al. 2024;
 * diffusers' pag_scale).  ep = eps of the conditional forward in which the self-attention map of the chosen layers is the identity:
 *   e0 = the guided prediction of pv_cfg_dpm_step_guided (two or three forwards; g_image == g_text drops eps_image)
 *   e  = e0 + g_pag*(ec - ep)
 *   f  = rescale*std_b(ec)/std_b(e) + (1 - rescale)     on THAT e;   e = f*e
 * then the solver update, with rng != NULL the cn*z of pv_cfg_dpm_step_stochastic (rng == NULL: the deterministic step), and the inpainting blend.
 * eps_perturbed == NULL or g_pag == 0: eps_perturbed is not read and the launch is that of pv_cfg_dpm_step_guided (rng == NULL) /
 * pv_cfg_dpm_step_stochastic (rng != NULL), bit for bit.  Every other argument and limit as pv_cfg_dpm_step_guided; g_pag finite. */
int pv_cfg_dpm_step_pag(const float* eps_uncond, const float* eps_image, const float* eps_cond, const float* eps_perturbed, float* latents,
                        float* x0_prev, const float* coef, const int32_t* state, const uint32_t* rng, float g_text, float g_image, float g_pag,
                        float rescale, const float* mask, const float* known, const float* noise, int32_t batch, int32_t channels, int32_t hw,
                        void* stream);

/* Grad-mode branch fusion of PhotoVerseAttnProcessor2_0 (attention_processor.py:413-420) WITHOUT the reference's per-layer
 * host sync (`torch.rand(1).item()`): one tiny launch draws u ~ U(0,1) per cross-attention layer on the device
 * (Philox4x32-10, key = rng[0..1], counter = {rng[2] = launch count, layer}) and writes out[layer] = (w_text, w_ip):
 * u < rule1 -> (scale, 0); u > rule2 -> (0, scale); else (1, 1).  rng[2] advances by one per launch, so a captured graph draws
 * fresh numbers on every replay.  forced (optional, [n_layers]): entries >= 0 replace the drawn u (tests).
 * only_last_step != 0 with state != NULL: the rule applies only when state[0] == state[1] - 1 (run_inference's
 * training_mode, infer.py:99: grad is enabled on the last denoising step only), otherwise every layer gets (1, 1). */
int pv_fusion_draw(const int32_t* state, uint32_t* rng, const float* forced, float* out, int32_t n_layers, float rule1,
                   float rule2, float scale, int32_t only_last_step, void* stream);

/* small helpers */
int pv_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int pv_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* mean over `count` consecutive rows: x fp16 [groups*count][cols] -> y fp16 [groups][cols]
 * (adapters.py:36 mean over the 256 patch tokens); group g starts at row g*group_rows (group_rows >= count);
 * y may be accumulated (+=) when accumulate!=0 */
int pv_rows_mean(const void* x, int32_t ldx, void* y, int32_t ldy, int32_t groups, int32_t count, int32_t group_rows,
                 int32_t cols, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pre-loop conditioning front ends (infer.py:76-96).
 */
/* ------------------------------------------------------------------------------------------
 * VAE decode helpers (infer.py:121-123; [EXT] diffusers AutoencoderKL.decode).  The decoder's convolutions, GroupNorms
 * and Linear layers run on pv_gemm_conv / pv_groupnorm_*; its single-head attention over H*W tokens (head dim 512) is
 * GEMM -> pv_softmax_rows -> GEMM.
 */
/* in place: x[r][c] = softmax_c(scale * x[r][c]) over fp16 rows (fp32 math), cols % 8 == 0 */
int pv_softmax_rows(void* x, int32_t ld, int32_t rows, int32_t cols, float scale, void* stream);
/* 1x1 conv over NCHW fp32 with few channels (post_quant_conv 4->4): w [cout][cin], bias [cout] or NULL */
int pv_pointwise_nchw(const float* x, const float* w, const float* bias, float* out, int32_t batch, int32_t cin, int32_t cout,
                      int32_t hw, void* stream);
/* in place clamp of fp32 values (images.clamp(-1, 1), infer.py:122) */
int pv_clamp_f32(float* x, float lo, float hi, int64_t n, void* stream);
/* (ABI 18) out = clamp(m*gen + (1-m)*orig, lo, hi) on fp32 NCHW images, mask fp32 [B][1][hw] at pixel resolution, broadcast over
 * `channels`; out may alias gen; hw % 4 == 0.  Nothing in the reference: replaces the paste-back of an inpainting result onto
 * the input photograph ([EXT] diffusers apply_overlay) AND the images.clamp(-1, 1) of infer.py:122, in one launch. */
int pv_composite_clamp_f32(const float* gen, const float* orig, const float* mask, float* out, float lo, float hi, int32_t batch,
                           int32_t channels, int32_t hw, void* stream);
/* out[b][i] = ca[b]*x[b][i] (+ cb[b]*y[b][i]): scheduler.add_noise (infer.py:65, train.py:484: ca = sqrt(acp[t_b]),
 * cb = sqrt(1 - acp[t_b])) and the 1/scaling_factor latent scaling (infer.py:121) */
int pv_affine_rows_f32(const float* x, const float* y, const float* ca, const float* cb, float* out, int64_t per_sample,
                       int32_t batch, void* stream);
/* (ABI 19) out[b][c] = ca[b] * bilinear(x[b][c]: h x w -> oh x ow) (+ cb[b] * y[b][c])   fp32 NCHW, contiguous
 * bilinear = F.interpolate(mode="bilinear", align_corners=False, antialias=False):
 *   src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), weight = src - i0, per axis
 * ca NULL = 1; y and cb are given together or both NULL; x, y, ca, cb are read only; out must not overlap x.
 * Any h, w, oh, ow >= 1; every operand below 2 GiB.  At oh == h, ow == w without ca / y / cb the result is x bit for bit (the weights are exactly 0).
 * Nothing in the reference: the step between the two passes of a high-resolution generation ([EXT] the "hires fix" of A1111 / diffusers' latent
 * upscale), x_start = sqrt(acp[t]) * upsample(latents) + sqrt(1 - acp[t]) * noise, in one launch. */
int pv_resize_bilinear_affine_f32(const float* x, const float* y, const float* ca, const float* cb, float* out,
                                  int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t oh, int32_t ow, void* stream);
/* (ABI 19, a symbol added) [EXT] FreeU (Si et al., CVPR 2024; diffusers' enable_freeu) on the two inputs of one decoder ResnetBlock, before their
 * (virtual) channel concat, in ONE launch.  Rows are fp16 [batch*h*w][C]; image i is the h*w consecutive rows from i*h*w, row y*w + x its pixel (y, x).
 *   backbone:  x_out[r][c] = fp16(float(x[r][c]) * (c < cx/2 ? b : 1))                                   (the upper half is copied bit for bit)
 *   skip:      per (image, channel) plane p[y][x], diffusers' fourier_filter(threshold = 1, scale = s) - fftn, fftshift, the 2 x 2 window
 *              [h/2-1 : h/2+1, w/2-1 : w/2+1] times s, ifftshift, ifftn, .real - in closed form: the window holds the frequencies (u, v) in {0, -1}^2,
 *                X[u,v]          = sum_{y,x} p[y][x] * exp(-2 pi i (u y/h + v x/w))
 *                skip_out[y][x]  = fp16(p[y][x] + (s - 1)/(h w) * sum_{u,v} Re(X[u,v] * exp(+2 pi i (u y/h + v x/w))))
 *              seven real sums per plane and a rank-4 update; fp32 accumulation in a fixed order (no atomics: the same bits on every launch).
 * Either half may be absent (x == x_out == NULL, or skip == skip_out == NULL; its widths and scale are then ignored) but not both; an input without
 * its output (or the reverse) is rejected.  Inputs are read only, outputs must not be the inputs.  cx % 16 == 0, cs % 8 == 0, every row stride a
 * multiple of 8 elements and >= its width, every pointer 16-byte aligned, h >= 2, w >= 2, batch >= 1, b and s finite, every extent
 * (batch*h*w rows of ld elements) below 2 GiB. */
int pv_freeu_rows(const void* x, int32_t ldx, int32_t cx, void* x_out, int32_t ldxo, float b, const void* skip, int32_t lds, int32_t cs,
                  void* skip_out, int32_t ldso, float s, int32_t batch, int32_t h, int32_t w, void* stream);
/* (ABI 19, a symbol added) [EXT] The small-channel 3x3 convs of a ControlNet's conditioning embedding (diffusers' ControlNetConditioningEmbedding):
 *   out[(b*ho + oy)*wo + ox][co] = fp16(act(bias[co] + sum_{ky,kx,ci} in[b][oy*stride + ky - 1][ox*stride + kx - 1][ci] * w[co][(ky*3 + kx)*cin + ci]))
 * pad 1 (taps outside the image are 0), stride 1 or 2, ho = (h - 1)/stride + 1, wo = (wd - 1)/stride + 1, fp32 accumulation; act = PV_ACT_NONE or
 * PV_ACT_SILU.  w: fp16 [cout][9*cin], tap-major; bias: fp32 [cout]; out: fp16 rows with the leading dimension ldo.  Two input forms:
 *   x_is_image = 1   x is fp32 NCHW [batch][cin][h][wd], contiguous, cin <= 4 (ldx is ignored): the first layer, on ordinary vector instructions;
 *   x_is_image = 0   x is fp16 rows [batch*h*wd][cin] with the leading dimension ldx, cin % 8 == 0, cin <= 256: v_mfma_f32_16x16x32_f16 over the flat
 *                    contraction k = tap*cin + ci, zero-filled to a multiple of 32.
 * cout % 16 == 0, cout <= 256; ldo >= cout, ldx >= cin, both multiples of 8; w, bias, out (and x as rows) 16-byte aligned; x and out below 2 GiB each.
 * Inputs are read only; out must not overlap x.  Anything else returns hipErrorInvalidValue before any HIP call.
 * (Bound through _lib.EXT_SIGNATURES: the launcher is not yet in the launch audit's catalogue, which covers every `int pv_*` declaration of this header.) */
int32_t pv_hint_conv3x3(const void* x, int32_t x_is_image, int32_t ldx, const void* w, const float* bias, void* out, int32_t ldo, int32_t batch,
                        int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t stride, int32_t act, void* stream);
/* (ABI 19, a symbol added) [EXT] Token downsampling (ToDo, Smith et al. 2024): the token grid of fp16 rows pooled by a factor f per side - the keys and
 * values of a self-attention whose queries stay at full resolution.
 *   x:    rows [batch*h*w] of cols columns with the row stride ldx (a column slice of a wider buffer: the [K | V] columns of a qkv row);
 *   out:  rows [batch*hp*wp][cols] with the row stride ldo, hp = ceil(h / f), wp = ceil(w / f); row (b*hp + oy)*wp + ox is the block
 *         y in [oy*f, min(oy*f + f, h)), x in [ox*f, min(ox*f + f, w)) of image b:
 *   PV_POOL_AVG      fp16(sum of the block's in-bounds pixels / their count): fp32 sum in row-major order, one division, one rounding
 *                    (F.avg_pool2d(ceil_mode=True, count_include_pad=False)); an edge block of a grid f does not divide averages what it has;
 *   PV_POOL_NEAREST  the bits of the block's top-left pixel (y, x) = (oy*f, ox*f)   ([::f, ::f]).
 * 2 <= f <= 8; cols % 8 == 0, ldx and ldo multiples of 8 and >= cols; both pointers 16-byte aligned; batch, h, w >= 1; x is read only and out must not be
 * x; every extent (batch*h*w rows of ld elements) below 2 GiB.  Anything else returns hipErrorInvalidValue before any HIP call.
 * (Bound through _lib.EXT_SIGNATURES, as pv_hint_conv3x3 is.) */
#define PV_POOL_AVG 0
#define PV_POOL_NEAREST 1
int32_t pv_token_pool(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t cols, int32_t batch, int32_t h, int32_t w, int32_t f, int32_t mode,
                      void* stream);
/* (ABI 19, symbols added) [EXT] The two launches self-attention guidance needs beyond a forward (SAG, Hong et al., ICCV 2023; diffusers'
 * StableDiffusionSAGPipeline), bound through _lib.EXT_SIGNATURES as pv_hint_conv3x3 is.  Nothing records them into a plan yet.
 *
 * pv_attn_colmass: the attention each key receives, from the q and k rows pv_attention reads (fp16 rows with their own leading dimensions: column slices
 * of a fused qkv buffer will do, a row offset goes through the pointers; head hd owns columns hd*d .. hd*d + d):
 *   A[b][hd][i][j] = softmax_j(q[b][i][hd] . k[b][j][hd] / sqrt(d))          i < nq, j < nk
 *   mass[b][j]     = (1 / heads) * sum_hd sum_i A[b][hd][i][j]               fp32 [batch][nk]; every row of A sums to 1, so sum_j mass[b][j] = nq
 * Scores on v_mfma_f32_16x16x32_f16 (fp32 accumulation), softmax with the row maximum, probabilities and every sum in fp32.  No atomics; heads and query
 * tiles are added in a fixed order: a graph replay gives the bits of an eager launch.  One launch, no scratch; q and k are read only.
 * d in {40, 64, 80, 160}; 1 <= nq, nk <= 1024; batch, heads >= 1; ldq, ldk >= heads*d and multiples of 8; q and k 16-byte aligned; q and k below 2 GiB
 * each.  Anything else returns hipErrorInvalidValue before any HIP call. */
int32_t pv_attn_colmass(const void* q, int32_t ldq, const void* k, int32_t ldk, float* mass, int32_t batch, int32_t heads, int32_t nq, int32_t nk, int32_t d,
                        void* stream);
/* pv_sag_degrade: the input of SAG's degraded forward.  x, eps_base, x_deg fp32 NCHW [batch][channels][h][w], contiguous; mass fp32 [batch][mh*mw] (the
 * column mass of an mh x mw token grid); (ca, cb) = columns 0, 1 of the coefficient row pv_cfg_dpm_step reads at the step index of `state`:
 *   m[b][y][x]  = mass[b][((y*mh)/h)*mw + (x*mw)/w] > 1.0      integer nearest upsample, strict comparison, one mask for all channels
 *   x0          = ca*x + cb*eps_base
 *   blur        = per plane, the 9x9 Gaussian of sigma 1 (k1d[t] = exp(-t*t/2) / sum, t = -4 .. 4; k2d = outer(k1d, k1d); evaluated rows, then columns) on x0
 *                 with reflect padding 4 (-1 -> 1, n -> n - 2)
 *   x_deg       = m ? x + (1/ca)*(blur - x0) : x               the bits of x where the mask is off
 * (== add_noise(m*blur + (1 - m)*x0, eps_base, t) of diffusers: sqrt(acp_t) = 1/ca.)  One launch; inputs and state are read only; x_deg must be neither x
 * nor eps_base.  h, w >= 5 (the padding reflects inside the plane); batch, channels, mh, mw >= 1; any h != w and map sizes that do not divide the plane;
 * every operand below 2 GiB.  Anything else returns hipErrorInvalidValue before any HIP call. */
int32_t pv_sag_degrade(const float* x, const float* eps_base, const float* mass, const float* coef, const int32_t* state, float* x_deg, int32_t batch,
                       int32_t channels, int32_t h, int32_t w, int32_t mh, int32_t mw, void* stream);
/* (ABI 19, symbols added) [EXT] The two launches a T2I-Adapter (Mou et al. 2023; diffusers' T2IAdapter / down_intrablock_additional_residuals) needs beyond
 * the existing paths, bound through _lib.EXT_SIGNATURES as pv_hint_conv3x3 is.
 *
 * pv_add_feature_rows: the per-step launch - a static feature map added at the end of a down block:
 *   out[r][c] = fp16(fmaf(s, f[r % feat_rows][c], x[r][c]))                 r < rows, c < cols; one fp32 fma, one rounding
 *   s         = scale_tab ? scale_tab[step index of `state`] : scale        scale_tab: device fp32, one entry per schedule row; state: the loop's step
 *                                                                           counter {step index, table rows, -, -}, the index clamped as everywhere
 * x, f, out: fp16 rows with the leading dimensions ldx, ldf, ldo (column slices will do).  feat_rows divides rows: a plan at batch 2B, or a sub-batch whose
 * f pointer is offset, reads the per-sample features.  With s == 0 out holds the bits of x and f is not read (it may hold NaN).
 * colstats (optional): fp32 [ceil(rows/64)][2][cols], the sum and the sum of squares of the fp16-rounded outputs per 64-row block and column - the format
 * of pv_gemm_params.colstats, for pv_groupnorm_stats_from_colstats; a partial last block sums the rows it has; with s == 0 they are x's statistics.  A
 * workgroup owns whole 64-row blocks of its columns and adds in a fixed order: no atomics, the same bits on every launch.
 * cols % 8 == 0; ldx, ldf, ldo multiples of 8 and >= cols; x, f, out 16-byte aligned; out is neither x nor f; scale_tab needs state; without scale_tab
 * scale is finite; every extent below 2 GiB.  Anything else returns hipErrorInvalidValue before any HIP call. */
int32_t pv_add_feature_rows(const void* x, int32_t ldx, const void* f, int32_t ldf, int32_t feat_rows, void* out, int32_t ldo, int32_t rows, int32_t cols,
                            float scale, const float* scale_tab, const int32_t* state, float* colstats, void* stream);
/* pv_pixel_unshuffle8: PixelUnshuffle(8) of an fp32 NCHW image [batch][channels][h][w] into fp16 rows [batch*(h/8)*(w/8)][channels*64] (leading dimension
 * ldo): row (b*(h/8) + y)*(w/8) + x, column c*64 + i*8 + j is fp16(image[b][c][8y + i][8x + j]) - exact, the rounding of the input.  batch_stride: elements
 * between two images; 0 reads one image for every sample.  channels in 1 ... 4; h % 8 == 0, w % 8 == 0; ldo % 8 == 0, ldo >= channels*64; batch_stride 0
 * or a multiple of 4 and >= channels*h*w; image and out 16-byte aligned; every extent below 2 GiB.  Anything else returns hipErrorInvalidValue before
 * any HIP call. */
int32_t pv_pixel_unshuffle8(const float* image, int64_t batch_stride, void* out, int32_t ldo, int32_t batch, int32_t channels, int32_t h, int32_t w,
                            void* stream);
/* (ABI 19, symbol added) [EXT] pv_tile_blend: the seam blend of tiled VAE decode / encode (diffusers' enable_tiling: blend_v, then blend_h, then the crop),
 * one launch per tile position over the whole batch, bound through _lib.EXT_SIGNATURES.  All operands fp32 NCHW, contiguous:
 *   tile  [batch][channels][th][tw]        read and written in place        above [batch][channels][ah][tw]   the tile one row up, already blended, or NULL
 *   out   [batch][channels][out_h][out_w]  written inside the kept region   left  [batch][channels][th][lw]   the tile one column left, likewise
 * For every pixel (y, x) of every plane, in fp32 (wy = (float)y / ev, wx = (float)x / eh):
 *   v = tile[y][x]
 *   if (y < ev)  v = above[ah - ev + y][x] * (1 - wy) + v * wy           the LAST ev rows of the neighbour, whatever its height
 *   if (x < eh)  v = left[y][lw - eh + x]  * (1 - wx) + v * wx           the LAST eh columns; the vertical blend comes first
 *   if (y < ev || x < eh)           tile[y][x] = v                       in place: the tiles below and to the right read it
 *   if (y < keep_h && x < keep_w)   out[oy + y][ox + x] = v              nothing else of out is touched
 * A lane reads and writes only its own pixels of tile; above and left are read only (they may be one buffer).  16-byte loads and stores where all four
 * pointers are 16-byte aligned and tw, lw, eh, keep_w, out_w and ox are multiples of 4; a scalar path for everything else - any channel count and extents.
 * No atomics, no scratch.
 * tile and out non-null; batch, channels, th, tw, out_h, out_w >= 1; above comes with 1 <= ev <= min(ah, th), no above with ev == 0 (ah is then
 * ignored); left with 1 <= eh <= min(lw, tw), no left with eh == 0; 1 <= keep_h <= th, 1 <= keep_w <= tw; oy, ox >= 0 and the kept region inside out;
 * pointers 4-byte aligned; tile and out overlap neither each other nor a neighbour; every operand below 2 GiB.  Anything else returns
 * hipErrorInvalidValue before any HIP call. */
int32_t pv_tile_blend(float* tile, const float* above, const float* left, float* out, int32_t batch, int32_t channels, int32_t th, int32_t tw, int32_t ah,
                      int32_t lw, int32_t ev, int32_t eh, int32_t keep_h, int32_t keep_w, int32_t out_h, int32_t out_w, int32_t oy, int32_t ox,
                      void* stream);
/* (ABI 19, symbol added) [EXT] pv_vae_attention: the VAE mid block's single-head attention (head width 256 / 512) as ONE flash launch over the whole
 * sub-batch (AutoencoderKL.enable_flash_attention; pv_vaeattn.hip), bound through _lib.EXT_SIGNATURES.  No [n][n] score matrix exists anywhere.
 *   out = softmax(scale * q k^T) v   per image: image i owns the rows i*n ... i*n + n - 1 of every operand and attends only to its own rows
 * q, k, v: fp16 rows [batch*n][d] with the leading dimensions ldq, ldk, ldv (column slices of one fused QKV buffer will do); out: fp16 [batch*n][d],
 * leading dimension ldo.  Scores, the running maximum and the denominator are fp32 (online softmax, base-2 exponent with scale * log2 e folded into the
 * fp32 score); P is rounded to fp16 once, for the P.V MFMA, and the denominator is the sum of those ROUNDED values, so numerator and denominator agree;
 * accumulation and the final division are fp32, one rounding to fp16.
 * d in {256, 512}; batch >= 1; any n >= 1.  Keys beyond an image's n contribute exactly 0 and are never loaded (the row behind an image may be another
 * image's or hold NaN: no 0 * x); query rows beyond n are not stored; nothing outside out[r][0..d), r < batch*n, is written.  No scratch buffer, no atomics,
 * a fixed summation order: every launch gives the same bits, and a batch equals its images launched one by one.  Safe under stream capture.
 * Returns hipErrorInvalidValue before any HIP call for: a null pointer; d outside the set; an ld below d or not a multiple of 8; a pointer not 16-byte
 * aligned; batch or n below 1; a non-finite scale; out overlapping an input; any operand extent ((batch*n - 1) * ld + d halfs) of 2 GiB or more. */
int32_t pv_vae_attention(const void* q, const void* k, const void* v, int32_t ldq, int32_t ldk, int32_t ldv, void* out, int32_t ldo, int32_t batch,
                         int32_t n, int32_t d, float scale, void* stream);
/* (ABI 19, symbol added) [EXT] pv_tiny_conv3x3: the 3x3 convs (pad 1) of AutoencoderTiny / TAESD (pv_tinyconv.hip), bound through _lib.EXT_SIGNATURES.
 *   y[b][oy][ox][co] = bias[co] (0 if bias == NULL)
 *                    + sum_{ky,kx,ci} X[b][iy][ix][ci] * w[co][(ky*3 + kx)*cin + ci]        w: fp16 [cout][9*cin], tap-major (as pv_hint_conv3x3)
 *                    + res[row][co]                                                         optional fp16 rows (leading dimension ldr), added in fp32
 *   out = act(y)                                                                            act = PV_ACT_NONE or PV_ACT_RELU
 * fp32 accumulation in a fixed order.  (iy, ix) = (oy*stride + ky - 1, ox*stride + kx - 1); taps outside the (virtual) input are 0.
 * Input forms:   x_is_image = 0   fp16 rows [batch*h*wd][64], leading dimension ldx; cin == 64; pre == PV_TINY_PRE_NONE.
 *                x_is_image = 1   fp32 NCHW [batch][cin][h][wd], contiguous, cin <= 4, read through pre: NONE, TANH3 (3*tanh(x/3)) or UNIT ((x + 1)/2); the
 *                                 padding taps are 0 AFTER pre.  stride 1, no upsample, ldx ignored.  Ordinary vector instructions (K <= 36).
 * Geometry (rows input): stride 1 or 2, ho = (h' - 1)/stride + 1, wo likewise; upsample 0 or 1: with 1 the conv sees the 2h x 2wd nearest-neighbour
 *                upsampling (h' = 2h) - tap (iy, ix) reads row (iy >> 1, ix >> 1), the zero padding lies outside [0, 2h) x [0, 2wd), and the upsampled tensor
 *                is never written.  stride 2 with upsample 1 is rejected.
 * Output forms:  out_is_image = 0  fp16 rows [batch*ho*wo][64], leading dimension ldo; cout == 64; ONE rounding, after residual and activation; ReLU gives
 *                                  +0 for every y <= 0 (no negative zero).
 *                out_is_image = 1  fp32 NCHW [batch][cout][ho][wo], cout <= 4, holding out_scale*y + out_shift (one fma); no fp16 rounding; act must be
 *                                  NONE and res NULL.  Image in with image out is rejected.
 * Inputs are read only; out overlaps nothing the launch reads.  No atomics, no scratch buffer; every launch gives the same bits, and a batch gives the bits
 * of its images launched one by one (no tap crosses into a neighbouring image's rows; rows behind the last image and columns beyond the width are never
 * read).  Safe under stream capture.  Pointers 16-byte aligned; ldx, ldo, ldr multiples of 8 and >= the width; every extent below 2 GiB; batch, h, wd >= 1;
 * out_scale, out_shift finite.  Anything else returns hipErrorInvalidValue before any HIP call. */
#define PV_TINY_PRE_NONE 0
#define PV_TINY_PRE_TANH3 1
#define PV_TINY_PRE_UNIT 2
int32_t pv_tiny_conv3x3(const void* x, int32_t x_is_image, int32_t ldx, int32_t pre, const void* w, const float* bias, const void* res, int32_t ldr,
                        void* out, int32_t out_is_image, int32_t ldo, float out_scale, float out_shift, int32_t batch, int32_t cin, int32_t cout, int32_t h,
                        int32_t wd, int32_t stride, int32_t upsample, int32_t act, void* stream);
/* (ABI 19, symbols added) [EXT] pv_dense_conv3x3: the 3x3 convs (pad 1, stride 1) of an RRDBNet - Real-ESRGAN's RealESRGAN_x4plus super-resolution model
 * (Wang et al. 2021; basicsr's RRDBNet; pv_denseconv.hip), bound through _lib.EXT_SIGNATURES.  x: fp16 rows [batch*h*wd][>= cin], leading dimension ldx;
 * ONLY the columns [0, cin) of a row are read.
 *   y   = bias[co] (0 if bias == NULL) + sum_{ky,kx,ci} X[b][iy][ix][ci] * w[co][(ky*3 + kx)*cin + ci]     w: fp16 [cout][9*cin], tap-major (as pv_tiny_conv3x3)
 *   a   = act(y)                      act = PV_ACT_NONE or PV_ACT_LEAKY_RELU: y > 0 ? y : slope * y (slope: a float argument, not the 0.01 of the other launchers)
 *   o   = alpha * a + res[row][co]    if res  != NULL (fp16 rows, leading dimension ldr), else a
 *   o   = beta  * o + res2[row][co]   if res2 != NULL (fp16 rows, leading dimension ldr2); res2 needs res
 *   out[row][co] = fp16(o)            ONE rounding; fp32 before it (each scaled residual is one fma), a fixed accumulation order
 * cin in {64, 96, 128, 160, 192}; cout in {32, 64}.  upsample 0 or 1: with 1 the conv sees the 2h x 2wd nearest-neighbour upsampling - tap (iy, ix) reads
 * row (iy >> 1, ix >> 1), the zero padding lies outside [0, 2h) x [0, 2wd), the upsampled tensor is never written, out has batch*2h*2wd rows - and
 * cin == cout == 64.
 * THE IN-PLACE DENSE BLOCK.  out may be a column slice of the buffer x lives in: the same rows (ldo == ldx), the columns [c_off, c_off + cout) with
 * c_off >= cin and c_off + cout <= ldx.  The launch reads nothing at or beyond column cin of any row - no 16-byte access of x reaches past column cin - and
 * writes nothing outside out[row][0 .. cout).  res and res2 overlap neither out nor each other, in elements: either may be a column slice of the rows out
 * or x lives in, e.g. x's own columns [0, 64).  So a ResidualDenseBlock needs no concatenation: one [rows][192] buffer, conv1 .. conv4 writing the columns
 * 64-95, 96-127, 128-159, 160-191 with LeakyReLU, conv5 reading all 192 and writing the next block's buffer with alpha = 0.2, res = x; the third block's
 * conv5 carries the RRDB's outer residual as beta = 0.2, res2 = the RRDB's input: two residuals, one rounding.
 * No atomics, no scratch buffer; every launch gives the same bits, and a batch gives the bits of its images launched one by one (no tap crosses into a
 * neighbouring image's rows; rows behind the last image are never read).  Safe under stream capture.  Pointers 16-byte aligned; ldx, ldo, ldr, ldr2
 * multiples of 8 and >= the width read or written; every extent below 2 GiB; batch, h, wd >= 1; slope, alpha, beta finite; out overlaps neither w nor
 * bias.  Anything else returns hipErrorInvalidValue before any HIP call. */
int32_t pv_dense_conv3x3(const void* x, int32_t ldx, const void* w, const float* bias, const void* res, int32_t ldr, const void* res2, int32_t ldr2,
                         void* out, int32_t ldo, int32_t batch, int32_t cin, int32_t cout, int32_t h, int32_t wd, int32_t upsample, int32_t act,
                         float slope, float alpha, float beta, void* stream);
/* (ABI 19, symbols added) [EXT] pv_window_gather / pv_window_blend: the two launches of windowed denoising (MultiDiffusion, Bar-Tal et al. 2023; diffusers'
 * StableDiffusionPanoramaPipeline; pv_window.hip), bound through _lib.EXT_SIGNATURES.  Both tensors fp32 NCHW, contiguous:
 *   canvas  [batch][channels][H][W]                    windows [batch*ny*nx][channels][S][S]
 * Window k = ky*nx + kx of sample b is row b*ny*nx + k of windows and covers canvas rows oy[ky] ... oy[ky]+S-1, columns ox[kx] ... ox[kx]+S-1.
 * oy[ny] and ox[nx] are HOST arrays: they are read during the call and reach the kernel by value, so nothing has to outlive the call, the launch can be
 * captured, and every check below runs before the first HIP call.
 *   pv_window_gather:  windows[b*ny*nx + k][c][y][x] = canvas[b][c][oy[ky] + y][ox[kx] + x]                       a copy, bit for bit
 *   pv_window_blend:   canvas[b][c][y][x] = num / den, in fp32, with the sums over the windows that cover (y, x), ky outer and kx inner, ascending:
 *                        num = sum_ky sum_kx (profile[y - oy[ky]] * profile[x - ox[kx]]) * windows[b*ny*nx + k][c][y - oy[ky]][x - ox[kx]]
 *                        den = (sum_ky profile[y - oy[ky]]) * (sum_kx profile[x - ox[kx]])
 *                      profile: device fp32 [S], strictly positive; NULL: all ones.  A sum starts with its first term (no 0 + ...), so an element that
 *                      one window covers, under a NULL profile, keeps that window's bits.
 * Every lane owns its output elements: no atomics, no LDS, no scratch, a fixed summation order - every launch gives the same bits.  16-byte loads and stores
 * where all pointers are 16-byte aligned and W, S and every ox are multiples of 4; a scalar path for everything else.
 * canvas, windows, oy, ox non-null; pointers 4-byte aligned; batch, channels >= 1; 1 <= ny, nx <= 64; 1 <= S <= min(H, W); per axis o[0] == 0, the origins
 * strictly increasing and at most S apart (every element is covered), o[last] + S == the extent; both tensors below 2^29 elements; windows and canvas do
 * not overlap (nor does profile overlap either).  Anything else returns hipErrorInvalidValue before any HIP call. */
int32_t pv_window_gather(const float* canvas, float* windows, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t S, const int32_t* oy,
                         int32_t ny, const int32_t* ox, int32_t nx, void* stream);
int32_t pv_window_blend(const float* windows, const float* profile, float* canvas, int32_t batch, int32_t channels, int32_t H, int32_t W, int32_t S,
                        const int32_t* oy, int32_t ny, const int32_t* ox, int32_t nx, void* stream);
/* vae.encode(x).latent_dist.sample() (infer.py:63, train.py:473): moments fp32 [B][2c][hw] (mean | logvar, NCHW),
 * out = mean + exp(0.5*clamp(logvar,-30,20)) * eps */
int pv_posterior_sample(const float* moments, const float* eps, float* out, int32_t batch, int64_t chw, void* stream);
/* deterministic mean reductions of the training losses (train.py:509-516): mode 0 mean(a), 1 mean|a| (concept_text_loss),
 * 2 mean((a-b)^2) (F.mse_loss); a / b fp32 or fp16 (is_f16); partial: workspace of n_partial floats; out[0] = result.
 * Order (fp32): n_partial workgroups of 256 threads; thread t of workgroup w adds the elements 256 w + t, + 256 n_partial, ... in order; a
 * 6-level butterfly per 64-lane wave, the four waves as (w0 + w1) + (w2 + w3) -> partial[w]; the partials are added in w order and multiplied by
 * the fp32 1 / n (pv_reduce_sumsq: by scale). */
int pv_reduce_mean(const void* a, const void* b, int32_t mode, int32_t is_f16, int64_t n, float* partial, int32_t n_partial,
                   float* out, void* stream);

/* im2col of a 3x3 / pad-1 conv over NCHW fp32 with few channels (UNet conv_in): fp16 rows [B*H*W][kpad], column
 * k = ci*9 + ky*3 + kx, zero padded (kpad % 64 == 0), so conv_in runs on pv_gemm_conv with w.reshape(cout, cin*9). */
int pv_im2col3x3(const float* x, void* out, int32_t batch, int32_t cin, int32_t h, int32_t wd, int32_t kpad, void* stream);
/* CLIP ViT patch embedding input: NCHW fp32 pixels -> fp16 rows [B*(img/patch)^2][kpad], one patch per row in
 * (channel, py, px) order = the flattened Conv2d(3,dim,patch,stride=patch) weight order, zero padded to kpad
 * (kpad % 64 == 0) so the patch embedding is a pv_gemm_conv call.  [EXT transformers CLIPVisionEmbeddings] */
int pv_patchify(const float* x, void* out, int32_t batch, int32_t ch, int32_t img, int32_t patch, int32_t kpad, void* stream);
/* out[b][0] = cls + pos[0]; out[b][1+i] = patches[b][i] + pos[1+i]  (fp16 rows [B*ntok][dim]) */
int pv_clip_vision_embed(const void* patches, const float* cls, const float* pos, void* out, int32_t batch, int32_t ntok,
                         int32_t dim, void* stream);
/* Token + position embedding of the CLIP text encoder with PhotoVerse's concept injection fused
 * (models/clip.py:17-24 _inject_concept_embeddings, :57-63): per row the placeholder position
 * placeholder_idx[b] is overwritten by n_concept concept embeddings and the tail is shifted right by
 * n_concept-1 (truncated).  n_concept == 0: stock embedding.  ids/placeholder_idx int64, tok/pos fp32, out fp16. */
int pv_clip_text_embed(const int64_t* ids, const float* tok, const float* pos, const void* concept, const int64_t* placeholder_idx,
                       int32_t n_concept, void* out, int32_t batch, int32_t seq, int32_t dim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHOTOVERSE_HIP_H */
