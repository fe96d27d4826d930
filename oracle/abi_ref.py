"""fp64 references of the C-ABI launchers, computed from a launch's own parameter block (``include/photoverse_hip.h``).

Each launcher has two functions here:

* ``LAYOUT[name](p)`` - the buffers the parameter block ``p`` addresses: field -> ``Buf(dtype, rows, cols, ld, role)``.  ``role`` is ``"in"``,
  ``"out"``, ``"inout"`` (read and written in place), ``"scratch"`` (written, contents undefined) or ``"opaque"`` (an output whose layout the
  header leaves undocumented: checked for determinism only, and through its consumer).
* ``REF[name](p, v)`` - ``v`` maps every non-NULL field to a 2-D ``[rows, cols]`` view of its buffer; the result maps each checked output
  field to an ``Expect``: the fp64 reference, a per-element error bound, and the aggregate term of its documented intermediates.

The semantics are written from the header alone.  Arithmetic is fp64 on the exact fp16 / fp32 inputs, with plain ``torch.matmul``; a 3x3
convolution is nine shifted matmuls.  Error bounds (every constant derived here, none fitted to a measurement):

* ``U16 = 2^-11``: half an fp16 ulp, the relative error of rounding a normal value to fp16; ``SUB16 = 2^-25``: half the fp16 subnormal spacing,
  its absolute error below 2^-14.  The final fp16 store is allowed ``2^-10 |ref| + 2^-24`` (twice that: the store rounds ``ref + e``, not ``ref``).
* ``U32 = 2^-24``: the same for fp32.
* ``mfma_c(K)``: fp16 products are exact in fp32 and the MFMA accumulates them as a k-ordered fp32 chain; the CDNA guide measures that chain
  against fp64 at 0.75-1.5e-7 Sum|a b| for K <= 1024 and 3.5e-7 Sum|a b| at K = 4096.  A chain's worst error grows linearly in its length, so
  ``c(K) = 3.5e-7 max(1, K / 4096)``.
* ``gamma(n) = n U32``: worst relative error of an n-term fp32 sum of same-sign values (norm statistics, softmax normalisers).
* ``DACT = 1.13``: the largest slope of SiLU / quick-GELU / GELU / LeakyReLU (GELU's is 1.129), the factor an accumulator error passes through
  an activation with.
* ``GELU_APPROX = 1.25e-5``: the documented absolute error bound of the epilogues' erf approximation, per unit |x| (``pv_common.h``).

* fp32 pointwise launchers (the solver steps, the resize, the embeds): every operation rounds within U32 of its own result; a reduction's relative
  error is its longest addition chain times U32 (``step_chain``, ``freeu_chain``: the chains of the kernels' documented reduction orders), not its
  length.  One term is measured, not derived: ``TOL_NOISE``, the error the device's ``logf`` / ``sincospif`` leave on a generated normal.

* the training tape's single launches (``TRAINING``): the pointwise fp16 launchers carry the store rounding and a few U32 of their fp32 expression
  (``__expf`` derived from the ISA's one-ulp exp2 / rcp, ``GELU_APPROX`` through the GELU forms and their derivatives); exact-select launchers compare
  bit for bit; reductions take the longest chain of their documented order (``blocks_chain``, ``mean_chain``, ``ln_bwd_chain``); ``pv_wgrad_tn`` takes
  ``mfma_c(rows_per_split)`` per slab.  Branch points - the LeakyReLU of ``pv_layernorm_backward``, the max(0, cos) of the cosine loss - widen the bound of
  the elements within their own fp32 error of the branch by the branch difference; the integer tap boundaries of the gray resizes need no widening, the
  bilinear weights being continuous across them (``gray_taps``).

Every function of the C ABI is in exactly one of ``REF`` (audited) and ``NOT_AUDITED`` (outside the audit, with the reason).  A buffer whose extent
depends on the contents of another one (the coefficient row by the step counter, the token table by the ids) is listed in ``DEPENDENT``.

Two kinds of error term.  ``det``: worst-case terms (accumulation, the erf approximation, norm statistics), added as they are.  ``sig``: the
documented fp16 roundings of intermediates (q, P, the normalised rows, the attention context).  Each is an independent rounding bounded by
+-U16 |t|, so a sum of many of them through a linear stage adds in quadrature: ``sig = sqrt(Sum (U16 t_j w_j)^2)``, a standard deviation
bounded with the largest rounding (the uniform rounding's is U16 |t| / sqrt 3).  Summing them with absolute values instead grows with
sqrt(terms) faster than the error does and would let an O(1e-2) error pass.
* Element bound: ``store + det + KAPPA sig``, ``KAPPA = 6`` (with the sqrt 3 above, more than 10 standard deviations).
* Aggregate bound: ``1.5 rel_l2(round(ref), ref) + 1e-6 + (||det|| + 2 ||sig||) / ||ref||`` (twice the expected rms of the statistical
  part), and never looser than the tolerance ``tests/test_hip_kernels.py`` asserts for the same launcher (``CAP``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import torch

F16, F32, I32, I64 = torch.float16, torch.float32, torch.int32, torch.int64
U16, SUB16, U32 = 2.0 ** -11, 2.0 ** -25, 2.0 ** -24
STORE16_REL, STORE16_ABS = 2.0 ** -10, 2.0 ** -24
STORE32_REL = 2.0 ** -23
DACT = 1.13
GELU_APPROX = 1.25e-5
LN2 = math.log(2.0)
KAPPA = 6.0

#: aggregate rel-L2 tolerances the kernel tests assert for each launcher (tests/test_hip_kernels.py): no audit bound is looser
CAP = {"gemm16": 1e-3, "gemm32": 2e-5, "attention": 2e-3, "xattn": 2e-3, "lnq": 2e-3, "fused": 1e-3, "fused_attn": 3e-3, "row_gemm": 1e-3,
       "layernorm": 1e-3, "groupnorm": 1e-3, "conv_out": 1e-5,
       # the training tape's launchers (test_elementwise_backward_pieces, test_arcface_loss_pieces, test_layernorm_backward_kernels; wgrad: ``wgrad_cap``)
       "pointwise16": 1e-3, "pointwise_bwd": 2e-3, "gray": 1e-5, "ln_bwd_dx": 1.5e-3, "ln_bwd_dgb": 1e-4}


def mfma_c(k: int) -> float:
    return 3.5e-7 * max(1.0, k / 4096.0)


def gamma(n: int) -> float:
    return n * U32


@dataclass
class Buf:
    dtype: torch.dtype
    rows: int
    cols: int
    ld: int
    role: str = "in"


@dataclass
class Expect:
    ref: torch.Tensor                 # fp64, the shape of the output view
    bound: torch.Tensor               # fp64, per element
    agg_extra: float = 0.0            # aggregate (rel-L2) allowance of documented intermediates
    store: Optional[torch.dtype] = None   # the output type: the aggregate bound rounds ``ref`` to it; None = exact (bit compare)
    after: Optional[Callable] = None  # after(got_views) -> Expect: a check that needs the kernel's own output (column statistics)
    cap: Optional[float] = None       # the aggregate bound never exceeds this (CAP)
    derive: Optional[Callable] = None  # derive(got_views) -> the tensor compared (default: the field itself)
    rounded: Optional[torch.Tensor] = None   # the exact answer as stored (default: ref rounded to ``store``), for the aggregate bound


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float64)


def store_bound(ref: torch.Tensor, dtype) -> torch.Tensor:
    if dtype == F16:
        return STORE16_REL * ref.abs() + STORE16_ABS
    return STORE32_REL * ref.abs() + 2.0 ** -140


def expect(ref, det, dtype, sig=None, cap=None):
    """Element bound = store rounding + ``det`` + KAPPA ``sig``; aggregate allowance (||det|| + 2 ||sig||) / ||ref||, capped at ``cap``."""
    den = ref.norm().item()
    tot = det.norm().item() + (0.0 if sig is None else 2 * sig.norm().item())
    bound = store_bound(ref, dtype) + det + (0.0 if sig is None else KAPPA * sig)
    return Expect(ref, bound, (tot / den) if den > 0 else 0.0, dtype, cap=cap)


def _act(x, act):
    if act == 0:
        return x
    if act == 1:
        return x * torch.sigmoid(x)
    if act == 2:
        return x * torch.sigmoid(1.702 * x)
    if act == 3:
        return torch.where(x > 0, x, 0.01 * x)
    if act == 4:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    raise ValueError(f"unknown activation {act}")


def _gelu(x):
    return _act(x, 4)


def _ptr(p, name) -> bool:
    return bool(getattr(p, name))


# ===================================================================================================================== pv_gemm_conv
def gemm_geometry(p):
    """(images, rows per image) of the epilogue's ``rowadd`` indexing and the input row count."""
    if p.taps == 9:
        return p.batch, p.hout * p.wout, p.batch * p.hin * p.win
    rpi = p.hout * p.wout
    return (p.M + rpi - 1) // rpi, rpi, p.M


def gemm_unpack_geglu(N: int):
    """Packed weight row -> (output column, is gate), from ``pack_geglu``'s documented fragment order: each 128-row tile holds, per wave
    half, alternating 16-row [value | gate] fragments of the same 16 output columns."""
    pr = torch.arange(N)
    t, wn, ni, e = pr // 128, (pr % 128) // 64, (pr % 64) // 16, pr % 16
    return t * 64 + wn * 32 + (ni // 2) * 16 + e, (ni & 1).bool()


def rowgemm_unpack_geglu(N: int):
    """``pv_row_gemm``'s order: per 160-row chunk c, fragment 2q = value rows of columns 80 c + 16 q .., fragment 2q + 1 = their gate rows."""
    pr = torch.arange(N)
    c, i, e = pr // 160, (pr % 160) // 16, pr % 16
    return 80 * c + 16 * (i // 2) + e, (i & 1).bool()


def layout_gemm(p):
    imgs, rpi, rows_in = gemm_geometry(p)
    n_out = p.N // 2 if p.geglu else p.N
    L = {"a0": Buf(F16, rows_in, p.c0, p.lda0), "w": Buf(F16, p.N, p.taps * (p.c0 + p.c1), p.taps * (p.c0 + p.c1)),
         "out": Buf(F32 if p.out_f32 else F16, p.M, n_out, p.ldc, "out")}
    if _ptr(p, "a1"):
        L["a1"] = Buf(F16, rows_in, p.c1, p.lda1)
    if _ptr(p, "bias"):
        L["bias"] = Buf(F32, 1, p.N, p.N)
    if _ptr(p, "rowadd"):
        L["rowadd"] = Buf(F32, imgs if p.rowadd_ld else 1, n_out, p.rowadd_ld or n_out)
    if _ptr(p, "residual"):
        L["residual"] = Buf(F16, p.M, n_out, p.ldr)
    if p.splitk > 1 and _ptr(p, "splitk_ws"):
        L["splitk_ws"] = Buf(F32, p.splitk * p.M, p.N, p.N, "scratch")
    if _ptr(p, "colstats"):
        L["colstats"] = Buf(F32, (p.M + 63) // 64, 2 * n_out, 2 * n_out, "out")
    if _ptr(p, "ln_rowsum"):
        L["ln_rowsum"] = Buf(F32, 1, p.N, p.N)
    if _ptr(p, "a_norm"):
        L["a_norm"] = Buf(F32, p.batch, 2 * (p.c0 + p.c1), 2 * (p.c0 + p.c1))
    return L


def conv_taps(x: torch.Tensor, batch, hin, win, hout, wout, stride, upsample, pad):
    """The nine shifted input matrices of a 3x3 conv over NHWC rows x [batch*hin*win, C]: tap t = 3 ky + kx -> [batch*hout*wout, C].
    Logical input = the x2 nearest upsample when ``upsample``; zero padding ``pad`` in front; reads past the bottom / right edge are 0."""
    C = x.shape[1]
    img = x.reshape(batch, hin, win, C)
    if upsample:
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
    hl, wl = img.shape[1], img.shape[2]
    need_h, need_w = (hout - 1) * stride + 3, (wout - 1) * stride + 3
    padded = img.new_zeros(batch, max(need_h, hl + pad), max(need_w, wl + pad), C)
    padded[:, pad:pad + hl, pad:pad + wl] = img
    out = []
    for ky in range(3):
        for kx in range(3):
            out.append(padded[:, ky:ky + (hout - 1) * stride + 1:stride, kx:kx + (wout - 1) * stride + 1:stride].reshape(-1, C))
    return out


def ref_gemm(p, v):
    imgs, rpi, rows_in = gemm_geometry(p)
    K1 = p.c0 + p.c1
    a = f64(v["a0"]) if p.c1 == 0 else torch.cat([f64(v["a0"]), f64(v["a1"])], 1)
    sig2 = None
    if "a_norm" in v:
        # GroupNorm folded into the conv: per image and input channel scale / shift, act, then the fp16 rounding pv_groupnorm_apply does
        tab = f64(v["a_norm"]).reshape(p.batch, 2, K1)
        img = torch.arange(rows_in, device=a.device) // (p.hin * p.win)
        a = _act(a * tab[img, 0] + tab[img, 1], p.a_norm_act)
        a = a.to(F16).to(torch.float64)     # the kernel rounds the same fp32 value: a rare one-ulp flip, at most U16 |a| per element
        sig2 = 0
    w = f64(v["w"])
    if p.taps == 9:
        xs = conv_taps(a, p.batch, p.hin, p.win, p.hout, p.wout, p.stride, p.upsample, p.pad)
        acc = torch.zeros(p.M, p.N, dtype=torch.float64, device=a.device)
        S = torch.zeros_like(acc)
        for t, xt in enumerate(xs):
            wt = w[:, t * K1:(t + 1) * K1]
            acc += xt @ wt.T
            S += xt.abs() @ wt.abs().T
            if sig2 is not None:
                sig2 = sig2 + (U16 * xt) ** 2 @ (wt * wt).T
    else:
        acc = a @ w.T
        S = a.abs() @ w.abs().T
        if sig2 is not None:
            sig2 = (U16 * a) ** 2 @ (w * w).T
    Kt = p.taps * K1
    err = mfma_c(Kt) * S
    sig = None if sig2 is None else torch.sqrt(sig2)
    if "ln_rowsum" in v:
        # LayerNorm folded into the GEMM: epilogue rstd * (acc - mean * rowsum[n]) over the raw rows of a0 (K = c0)
        x = f64(v["a0"])
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + float(p.ln_eps))
        rs = f64(v["ln_rowsum"]).reshape(1, -1)
        acc = rstd * (acc - mean * rs)
        # accumulation of both terms, then the row statistics' fp32 sums (relative gamma(K) on mean and variance -> on the result)
        err = rstd * (err + mfma_c(Kt) * mean.abs() * rs.abs()) + 2 * gamma(p.c0) * acc.abs() + rstd * gamma(p.c0) * x.abs().mean(1, keepdim=True) * rs.abs()
    if "bias" in v:
        acc = acc + f64(v["bias"]).reshape(1, -1)
    n_out = p.N // 2 if p.geglu else p.N
    rows = torch.arange(p.M, device=acc.device)
    if p.geglu:
        col, gate = gemm_unpack_geglu(p.N)
        col, gate = col.to(acc.device), gate.to(acc.device)
        val = torch.empty(p.M, n_out, dtype=torch.float64, device=acc.device)
        gt, ev, eg = torch.empty_like(val), torch.empty_like(val), torch.empty_like(val)
        val[:, col[~gate]] = acc[:, ~gate]
        gt[:, col[gate]] = acc[:, gate]
        ev[:, col[~gate]] = err[:, ~gate]
        eg[:, col[gate]] = err[:, gate]
        g = _gelu(gt)
        acc = val * g
        # value error x |gelu(gate)| + |value| x gelu slope x gate error + the erf approximation (GEGLU: one fp16 rounding of the fp32 product)
        err = ev * g.abs() + val.abs() * (DACT * eg + GELU_APPROX * gt.abs())
        if sig is not None:
            sv, sg = torch.empty_like(val), torch.empty_like(val)
            sv[:, col[~gate]], sg[:, col[gate]] = sig[:, ~gate], sig[:, gate]
            sig = torch.sqrt((sv * g) ** 2 + (DACT * val * sg) ** 2)
    if "rowadd" in v:
        ra = f64(v["rowadd"])
        acc = acc + (ra[rows // rpi] if p.rowadd_ld else ra.reshape(1, -1))
    if p.act:
        acc = _act(acc, p.act)
        err = DACT * err
        sig = None if sig is None else DACT * sig
    if "residual" in v:
        acc = acc + f64(v["residual"])
    dt = F32 if p.out_f32 else F16
    res = {"out": expect(acc, err, dt, sig, CAP["gemm32" if p.out_f32 else "gemm16"])}
    if "colstats" in v:
        res["colstats"] = Expect(None, None, 0.0, F32, after=lambda got, M=p.M, n=n_out: colstats_expect(got["out"], M, n))
    return res


def colstats_expect(y: torch.Tensor, M: int, N: int) -> Expect:
    """Per 64-row block and column: (sum, sum of squares) of the kernel's OWN fp16 output; fp32 accumulation of <= 64 terms: gamma(64)."""
    yy = f64(y)
    nb = (M + 63) // 64
    pad = torch.zeros(nb * 64 - M, N, dtype=torch.float64, device=yy.device)
    blk = torch.cat([yy, pad]).reshape(nb, 64, N)
    s, ss = blk.sum(1), (blk * blk).sum(1)
    sa = blk.abs().sum(1)
    ref = torch.stack([s, ss], 1).reshape(nb, 2 * N)
    bound = torch.stack([gamma(64) * sa, gamma(64) * ss], 1).reshape(nb, 2 * N) + 2.0 ** -140
    return Expect(ref, bound, 0.0, F32)


# ===================================================================================================================== attention
def sdpa(q, k, v, scale, causal=False, q_sig=None, q_det=None):
    """softmax(q k^T scale) v over [..., n, d] (leading dims batched) in fp64, with its error terms: (out, lse, det, sig).

    First-order effects of each perturbation on out_i = Sum_j p_ij v_j:
    - a score error e_ij moves out_i by Sum_j p_ij e_ij (v_j - out_i).  Per score: the fp32 accumulation of its d products (mfma_c(d) |q|.|k_j|
      scale) and the fp32 rounding of the exp2 argument (2 U32 (|s_ij| + |max_j s_ij|)); independent across (i, j): quadrature.
    - a q error dq moves out_i by scale Sum_d dq_d Cov_p(v, k_d) (the p_i-weighted covariance of v and column d of k).  q's fp16 rounding
      (the kernels fold scale log2 e into q once; lnq / fused pass their q stage as ``q_sig``), independent across d: quadrature; ``q_det``:
      worst case.
    - P rounded to fp16 for the PV product, and exp2's own ulp: (U16 + 2 U32) p_ij v_j, independent across j: quadrature.
    - the normaliser, an nk-term fp32 sum: a random walk of sqrt(nk) U32 relative, scaling out_i.
    - the PV accumulation: mfma_c(nk) Sum_j p_ij |v_j| (det)."""
    nk, d = k.shape[-2], k.shape[-1]
    s = (q @ k.transpose(-1, -2)) * scale
    qk = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    if causal:
        i = torch.arange(q.shape[-2], device=q.device)[:, None]
        j = torch.arange(nk, device=q.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = p @ v
    sf = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
    e = mfma_c(d) * qk + 2 * U32 * (sf.abs() + sf.abs().amax(-1, keepdim=True))
    A = (p * e) ** 2
    var = (A @ (v * v) - 2 * out * (A @ v) + out ** 2 * A.sum(-1, keepdim=True)).clamp_min(0)
    var = var + ((U16 + 2 * U32) * p) ** 2 @ (v * v) + (math.sqrt(nk) * U32 * out) ** 2
    vk = (v.unsqueeze(-1) * k.unsqueeze(-2)).reshape(*v.shape[:-1], v.shape[-1] * d)
    cov = (p @ vk).reshape(*out.shape, d) - out.unsqueeze(-1) * (p @ k).unsqueeze(-2)
    qs = U16 * q.abs() if q_sig is None else q_sig
    var = var + torch.einsum("...id,...icd->...ic", (scale * qs) ** 2, cov * cov)
    det = mfma_c(nk) * (p @ v.abs())
    if q_det is not None:
        det = det + torch.einsum("...id,...icd->...ic", scale * q_det, cov.abs())
    # log-sum-exp (natural units): the largest score error, the q rounding through |k|, the normaliser and the log / exp ulps
    lerr = ((mfma_c(d) + U16) * qk).amax(-1) + math.sqrt(nk) * U32 * KAPPA + 4 * U32
    return out, lse, det, torch.sqrt(var), lerr


def layout_attention(p):
    C = p.heads * p.d
    L = {"q": Buf(F16, p.batch * p.nq, C, p.ldq), "k": Buf(F16, p.batch * p.nk, C, p.ldk), "v": Buf(F16, p.batch * p.nk, C, p.ldv),
         "out": Buf(F16, p.batch * p.nq, C, p.ldo, "out")}
    if _ptr(p, "lse"):
        L["lse"] = Buf(F32, p.batch * p.heads, p.nq, p.nq, "out")
    return L


def ref_attention(p, v):
    B, H, nq, nk, d = p.batch, p.heads, p.nq, p.nk, p.d
    scale = 1.0 / math.sqrt(d)
    q, k, vv = f64(v["q"]), f64(v["k"]), f64(v["v"])
    out = torch.empty(B * nq, H * d, dtype=torch.float64, device=q.device)
    det, sig = torch.empty_like(out), torch.empty_like(out)
    lse = torch.empty(B * H, nq, dtype=torch.float64, device=q.device)
    lerr = torch.empty_like(lse)
    for b in range(B):                      # one (image, head) at a time: the score matrix of a 96 x 96 latent is 9216^2
        for h in range(H):
            r, c = slice(b * nq, (b + 1) * nq), slice(h * d, (h + 1) * d)
            kr = slice(b * nk, (b + 1) * nk)
            out[r, c], l, det[r, c], sig[r, c], le = sdpa(q[r, c], k[kr, c], vv[kr, c], scale, bool(p.causal))
            lse[b * H + h], lerr[b * H + h] = l / LN2, le / LN2 + 2 * U32 * (l / LN2).abs()
    res = {"out": expect(out, det, F16, sig, CAP["attention"])}
    if "lse" in v:
        res["lse"] = expect(lse, lerr, F32)      # its terms are worst-case ones (det): the same element bound, and ||lerr|| / ||lse|| in aggregate
    return res


# ===================================================================================================================== cross attention
def _fusion(p, v):
    if "fusion" in v:
        f = v["fusion"].reshape(-1).double().cpu()
        return float(f[0]), float(f[1])
    return float(p.w_text), float(p.w_ip)


def xattn_core(q, kt, vt, kip, vip, B, H, nq, nt, nip, d, wt, wi, q_sig=None, q_det=None):
    """Dual-branch SDPA with two independent softmaxes, one image at a time (heads batched): (out, det, sig), [B*nq, H*d]."""
    scale = 1.0 / math.sqrt(d)
    heads = lambda t, n, b: None if t is None else t[b * n:(b + 1) * n].reshape(n, H, d).permute(1, 0, 2)     # [H, n, d]
    back = lambda t: t.permute(1, 0, 2).reshape(nq, H * d)
    out = torch.zeros(B * nq, H * d, dtype=torch.float64, device=q.device)
    det, var = torch.zeros_like(out), torch.zeros_like(out)
    for b in range(B):
        r = slice(b * nq, (b + 1) * nq)
        qh = heads(q, nq, b)
        for w_, K_, V_, n in ((wt, kt, vt, nt), (wi, kip, vip, nip)):
            if n == 0 or w_ == 0.0:
                continue
            o, _, dt, sg, _ = sdpa(qh, heads(K_, n, b), heads(V_, n, b), scale, q_sig=heads(q_sig, nq, b), q_det=heads(q_det, nq, b))
            out[r] += w_ * back(o)
            det[r] += abs(w_) * back(dt)
            var[r] += (w_ * back(sg)) ** 2
    return out, det, torch.sqrt(var)


def _vnorm(vip, B, H, nip, d):
    v3 = vip.reshape(B, nip, H, d)
    n = v3.norm(dim=3).permute(0, 2, 1).reshape(B * H, nip)
    # fp32 sum of d squares, then sqrt: gamma(d) / 2 + one ulp
    return n, (gamma(d) + 2 * U32) * n + 2.0 ** -140


def layout_xattn(p):
    C = p.heads * p.d
    L = {"q": Buf(F16, p.batch * p.nq, C, p.ldq), "kt": Buf(F16, p.batch * p.nt, C, p.ldkt), "vt": Buf(F16, p.batch * p.nt, C, p.ldvt),
         "out": Buf(F16, p.batch * p.nq, C, p.ldo, "out")}
    if p.nip:
        L.update(kip=Buf(F16, p.batch * p.nip, C, p.ldkip), vip=Buf(F16, p.batch * p.nip, C, p.ldvip))
    if _ptr(p, "vnorm"):
        L["vnorm"] = Buf(F32, p.batch * p.heads, p.nip, p.nip, "out")
    if _ptr(p, "fusion"):
        L["fusion"] = Buf(F32, 1, 2, 2)
    return L


def ref_xattn(p, v):
    wt, wi = _fusion(p, v)
    kip = f64(v["kip"]) if "kip" in v else None
    vip = f64(v["vip"]) if "vip" in v else None
    out, det, sig = xattn_core(f64(v["q"]), f64(v["kt"]), f64(v["vt"]), kip, vip, p.batch, p.heads, p.nq, p.nt, p.nip, p.d, wt, wi)
    res = {"out": expect(out, det, F16, sig, CAP["xattn"])}
    if "vnorm" in v:
        n, b = _vnorm(vip, p.batch, p.heads, p.nip, p.d)
        res["vnorm"] = Expect(n, b, 0.0, F32)
    return res


def layout_xattn_lnq(p):
    C = p.heads * p.d
    L = {"hs": Buf(F16, p.batch * p.nq, C, p.ld_hs), "wq": Buf(F16, C, C, C), "kt": Buf(F16, p.batch * p.nt, C, p.ldkt),
         "vt": Buf(F16, p.batch * p.nt, C, p.ldvt), "out": Buf(F16, p.batch * p.nq, C, p.ldo, "out")}
    if _ptr(p, "q_bias"):
        L["q_bias"] = Buf(F32, 1, C, C)
    if _ptr(p, "wq_rowsum"):
        L["wq_rowsum"] = Buf(F32, 1, C, C)
    if p.nip:
        L.update(kip=Buf(F16, p.batch * p.nip, C, p.ldkip), vip=Buf(F16, p.batch * p.nip, C, p.ldvip))
    if _ptr(p, "vnorm"):
        L["vnorm"] = Buf(F32, p.batch * p.heads, p.nip, p.nip, "out")
    if _ptr(p, "fusion"):
        L["fusion"] = Buf(F32, 1, 2, 2)
    return L


def q_stage(p, v, C, round_x: bool):
    """q = to_q(LayerNorm_noaffine(hs)) + q_bias (or to_q(hs) + q_bias) and its error terms (det, sig), q's own fp16 rounding included.
    ``round_x``: the normalised rows are rounded to fp16 before the product (the fused launch's register-resident X)."""
    x = f64(v["hs"])
    wq = f64(v["wq"])
    if p.ln:
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + float(p.ln_eps))
        xn = (x - mean) * rstd
    else:
        xn = x
    q = xn @ wq.T
    if p.ln and not round_x:
        # the folded form rstd * (wq . x - mean * rowsum): accumulation over the raw rows, then the cancellation
        det = rstd * mfma_c(C) * (x.abs() @ wq.abs().T + mean.abs() * wq.abs().sum(1)[None, :])
    else:
        det = mfma_c(C) * (xn.abs() @ wq.abs().T)
    var = torch.zeros_like(q)
    if p.ln:
        det = det + 2 * gamma(C) * q.abs()             # fp32 row statistics: relative gamma(C) on mean and variance
        if round_x:
            var = var + (U16 * xn) ** 2 @ (wq * wq).T  # X normalised in registers, rounded to fp16 for the MFMA
    if "q_bias" in v:
        q = q + f64(v["q_bias"]).reshape(1, -1)
    var = var + (U16 * q) ** 2 + SUB16 ** 2           # q (pre-scaled) is an fp16 MFMA operand of the score product
    return q, det, torch.sqrt(var)


def ref_xattn_lnq(p, v):
    C = p.heads * p.d
    wt, wi = _fusion(p, v)
    q, qdet, qsig = q_stage(p, v, C, round_x=False)
    kip = f64(v["kip"]) if "kip" in v else None
    vip = f64(v["vip"]) if "vip" in v else None
    out, det, sig = xattn_core(q, f64(v["kt"]), f64(v["vt"]), kip, vip, p.batch, p.heads, p.nq, p.nt, p.nip, p.d, wt, wi, q_sig=qsig, q_det=qdet)
    res = {"out": expect(out, det, F16, sig, CAP["lnq"])}
    if "vnorm" in v:
        n, b = _vnorm(vip, p.batch, p.heads, p.nip, p.d)
        res["vnorm"] = Expect(n, b, 0.0, F32)
    return res


def layout_xattn_fused(p):
    C = p.heads * p.d
    L = {"hs": Buf(F16, p.batch * p.nq, C, p.ld_hs), "wq": Buf(F16, C, C, C), "wo": Buf(F16, C, C, C),
         "kimg": Buf(F16, 1, p.batch * p.heads * 96 * (64 if p.d == 40 else 128), 0),
         "vimg": Buf(F16, 1, p.batch * (C // 80) * 96 * 80, 0), "out": Buf(F16, p.batch * p.nq, C, p.ld_out, "out")}
    if _ptr(p, "q_bias"):
        L["q_bias"] = Buf(F32, 1, C, C)
    if _ptr(p, "bias_o"):
        L["bias_o"] = Buf(F32, 1, C, C)
    if _ptr(p, "fusion"):
        L["fusion"] = Buf(F32, 1, 2, 2)
    return L


def ref_xattn_fused(p, v, kv, wo_slot):
    """``kv``: (kt, vt, kip, vip) - the K / V rows ``pv_xattn_pack_kv`` built ``kimg`` / ``vimg`` from (their layout is not documented);
    ``wo_slot``: packed column s -> natural column (``pv_xattn_fused_wo_slot``).  Checked twice: the whole output (with its residual) at the
    kernel test's 1e-3, and the attention part (out - hs) at its 3e-3."""
    C = p.heads * p.d
    wt, wi = _fusion(p, v)
    q, qdet, qsig = q_stage(p, v, C, round_x=True)
    kt, vt, kip, vip = (None if t is None else f64(t) for t in kv)
    ctx, cdet, csig = xattn_core(q, kt, vt, kip, vip, p.batch, p.heads, p.nq, p.nt, p.nip, p.d, wt, wi, q_sig=qsig, q_det=qdet)
    wo_p = f64(v["wo"])
    wo = torch.empty_like(wo_p)
    wo[:, torch.as_tensor(wo_slot, device=wo.device)] = wo_p
    att = ctx @ wo.T
    # ctx's errors and its fp16 rounding (ctx is the MFMA operand of to_out) through wo, and to_out's accumulation
    det = cdet @ wo.abs().T + mfma_c(C) * (ctx.abs() @ wo.abs().T)
    sig = torch.sqrt((csig ** 2 + (U16 * ctx) ** 2 + SUB16 ** 2) @ (wo * wo).T)
    if "bias_o" in v:
        att = att + f64(v["bias_o"]).reshape(1, -1)
    hs = f64(v["hs"])
    out = att + hs
    e_out = expect(out, det, F16, sig, CAP["fused"])
    e_att = expect(att, det, F16, sig, CAP["fused_attn"])
    e_att.bound = e_out.bound                     # the one fp16 store is of out = hs + att
    e_att.derive = lambda got, hs=hs: got["out"].double() - hs
    e_att.rounded = out.to(F16).double() - hs
    return {"out": e_out, "out - hs": e_att}


def ref_pack_kv(a, v):
    res = {}
    if "vnorm" in v:
        n, b = _vnorm(f64(v["vip"]), a.batch, a.heads, a.nip, a.d)
        res["vnorm"] = Expect(n, b, 0.0, F32)
    return res


def layout_pack_kv(a):
    C = a.heads * a.d
    L = {"kt": Buf(F16, a.batch * a.nt, C, a.ldkt), "vt": Buf(F16, a.batch * a.nt, C, a.ldvt),
         "kimg": Buf(F16, 1, a.batch * a.heads * 96 * (64 if a.d == 40 else 128), 0, "opaque"),
         "vimg": Buf(F16, 1, a.batch * (C // 80) * 96 * 80, 0, "opaque")}
    if a.nip:
        L.update(kip=Buf(F16, a.batch * a.nip, C, a.ldkip), vip=Buf(F16, a.batch * a.nip, C, a.ldvip))
    if a.vnorm:
        L["vnorm"] = Buf(F32, a.batch * a.heads, a.nip, a.nip, "out")
    return L


# ===================================================================================================================== row GEMM / norms
def layout_row_gemm(p):
    n_out = p.N // 2 if p.geglu else p.N
    L = {"x": Buf(F16, p.M, p.K, p.ld_x), "w": Buf(F16, p.N, p.K, p.K), "out": Buf(F16, p.M, n_out, p.ld_out, "out")}
    if _ptr(p, "bias"):
        L["bias"] = Buf(F32, 1, p.N, p.N)
    if _ptr(p, "x_norm"):
        L["x_norm"] = Buf(F32, p.M // p.rows_per_image, 2 * p.K, 2 * p.K)
    return L


def ref_row_gemm(p, v):
    x = f64(v["x"])
    w = f64(v["w"])
    det_in = sig_in = None
    if p.ln:
        raw = x
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + float(p.ln_eps))
        x = (x - mean) * rstd
        # fp32 row statistics: relative gamma(K) on mean and variance -> 2 gamma(K) |x_norm|; and the mean's ABSOLUTE error gamma(K) mean|x|
        # (+ the two roundings of x * rstd - mean * rstd) times rstd, which is what remains when x - mean cancels (a constant row: x_norm = 0,
        # rstd = eps^-1/2) - the same term ref_layernorm and the LayerNorm fold of ref_gemm carry
        det_in = 2 * gamma(p.K) * x.abs() + rstd * (gamma(p.K) + 2 * U32) * raw.abs().mean(1, keepdim=True)
        sig_in = U16 * x.abs() + SUB16                                # rows normalised in registers, rounded to fp16 for the MFMA
    elif "x_norm" in v:
        tab = f64(v["x_norm"]).reshape(-1, 2, p.K)
        img = torch.arange(p.M, device=x.device) // p.rows_per_image
        x = (x * tab[img, 0] + tab[img, 1]).to(F16).to(torch.float64)   # rounded to fp16 exactly as pv_groupnorm_apply writes it
        sig_in = U16 * x.abs()                                        # the same fp32 value rounded: a rare one-ulp flip
    acc = x @ w.T
    err = mfma_c(p.K) * (x.abs() @ w.abs().T)
    if det_in is not None:
        err = err + det_in @ w.abs().T
    sig = None if sig_in is None else torch.sqrt(sig_in ** 2 @ (w * w).T)
    if "bias" in v:
        acc = acc + f64(v["bias"]).reshape(1, -1)
    if p.geglu:
        col, gate = rowgemm_unpack_geglu(p.N)
        col, gate = col.to(acc.device), gate.to(acc.device)
        n_out = p.N // 2
        val, gt = torch.empty(p.M, n_out, dtype=torch.float64, device=acc.device), torch.empty(p.M, n_out, dtype=torch.float64, device=acc.device)
        ev, eg = torch.empty_like(val), torch.empty_like(val)
        val[:, col[~gate]], gt[:, col[gate]] = acc[:, ~gate], acc[:, gate]
        ev[:, col[~gate]], eg[:, col[gate]] = err[:, ~gate], err[:, gate]
        g = _gelu(gt)
        acc = val * g
        err = ev * g.abs() + val.abs() * (DACT * eg + GELU_APPROX * gt.abs())
        if sig is not None:
            sv, sg = torch.empty_like(val), torch.empty_like(val)
            sv[:, col[~gate]], sg[:, col[gate]] = sig[:, ~gate], sig[:, gate]
            sig = torch.sqrt((sv * g) ** 2 + (DACT * val * sg) ** 2)
    return {"out": expect(acc, err, F16, sig, CAP["row_gemm"])}


def layout_layernorm(p):
    return {"x": Buf(F16, p.rows, p.cols, p.ldx), "y": Buf(F16, p.rows, p.cols, p.ldy, "out"), "gamma": Buf(F32, 1, p.cols, p.cols),
            "beta": Buf(F32, 1, p.cols, p.cols)}


def ref_layernorm(p, v):
    x = f64(v["x"])
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + float(p.eps))
    g = f64(v["gamma"]).reshape(1, -1)
    z = g * (x - mean) * rstd
    y = _act(z + f64(v["beta"]).reshape(1, -1), p.act)
    # fp32 statistics (gamma(cols) relative on mean and variance -> 2 gamma on the normalised value) and the affine ops' roundings
    err = DACT * ((2 * gamma(p.cols) + 4 * U32) * z.abs() + g.abs() * rstd * gamma(p.cols) * x.abs().mean(1, keepdim=True) + 2 * U32 * y.abs())
    return {"y": expect(y, err, F16, cap=CAP["layernorm"])}


def layout_groupnorm(p, table=False):
    B, G = p.batch, p.groups
    Ct = p.c0 + p.c1
    L = {"x0": Buf(F16, B * p.hw, p.c0, p.ld0)}
    L["partial"] = Buf(F32, B * p.splits, 2 * G, 2 * G, "scratch")
    if p.c1:
        L["x1"] = Buf(F16, B * p.hw, p.c1, p.ld1)
    return L, B, G, Ct


def group_stats(p, v):
    """(mean, rstd) per (image, group) of x0 | x1 over hw pixels x C/G channels, with their error bounds."""
    B, G = p.batch, p.groups
    x = f64(v["x0"]) if p.c1 == 0 else torch.cat([f64(v["x0"]), f64(v["x1"])], 1)
    C = x.shape[1]
    xg = x.reshape(B, p.hw, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    n = xg.shape[2]
    mean = xg.mean(2)
    var = ((xg - mean[..., None]) ** 2).mean(2)
    ex2 = (xg * xg).mean(2)
    rstd = 1.0 / torch.sqrt(var + float(p.eps))
    # fp32 sums of n terms (sum and sum of squares, or the column statistics' 64-row sums + their reduction): gamma(n) relative on each;
    # var = E[x^2] - mean^2 then carries 2 gamma(n) E[x^2] absolute; rstd = (var + eps)^-1/2 halves the relative error, + its own ulps
    e_mean = gamma(n) * xg.abs().mean(2) + 2.0 ** -140
    e_var = 2 * gamma(n) * ex2 + 2 * mean.abs() * e_mean
    e_rstd = 0.5 * rstd * e_var / (var + float(p.eps)) + 4 * U32 * rstd
    return mean, rstd, e_mean, e_rstd


def layout_gn_stats(p):
    L, B, G, Ct = layout_groupnorm(p)
    if _ptr(p, "colstats0"):
        L["colstats0"] = Buf(F32, (B * p.hw + 63) // 64, 2 * p.c0, 2 * p.c0)
    if p.c1 and _ptr(p, "colstats1"):
        L["colstats1"] = Buf(F32, (B * p.hw + 63) // 64, 2 * p.c1, 2 * p.c1)
    return L


def _stats_expect(p, v):
    mean, rstd, em, er = group_stats(p, v)
    ref = torch.stack([mean, rstd], 2)          # [B][G][2] at partial[b][0][g][0..1]
    bound = torch.stack([em + store_bound(mean, F32), er + store_bound(rstd, F32)], 2)
    return ref, bound


def ref_gn_stats(p, v):
    ref, bound = _stats_expect(p, v)
    return {"partial[:, 0]": Expect(ref.reshape(p.batch, 2 * p.groups), bound.reshape(p.batch, 2 * p.groups), 0.0, F32)}


def layout_gn_scale_shift(p):
    L = layout_gn_stats(p)
    L["table"] = Buf(F32, p.batch, 2 * (p.c0 + p.c1), 2 * (p.c0 + p.c1), "out")
    L["gamma"] = Buf(F32, 1, p.c0 + p.c1, p.c0 + p.c1)
    L["beta"] = Buf(F32, 1, p.c0 + p.c1, p.c0 + p.c1)
    return L


def ref_gn_scale_shift(p, v):
    mean, rstd, em, er = group_stats(p, v)
    Ct = p.c0 + p.c1
    grp = torch.arange(Ct, device=mean.device) // (Ct // p.groups)
    g, b = f64(v["gamma"]).reshape(1, -1), f64(v["beta"]).reshape(1, -1)
    sc = g * rstd[:, grp]
    sh = b - mean[:, grp] * sc
    esc = g.abs() * er[:, grp] + 2 * U32 * sc.abs()
    esh = mean[:, grp].abs() * esc + sc.abs() * em[:, grp] + 2 * U32 * (b.abs() + (mean[:, grp] * sc).abs())
    ref = torch.stack([sc, sh], 1).reshape(p.batch, 2 * Ct)
    bound = torch.stack([esc, esh], 1).reshape(p.batch, 2 * Ct) + store_bound(ref, F32)
    sref, sbound = _stats_expect(p, v)
    return {"table": Expect(ref, bound, 0.0, F32),
            "partial[:, 0]": Expect(sref.reshape(p.batch, 2 * p.groups), sbound.reshape(p.batch, 2 * p.groups), 0.0, F32)}


def layout_gn_apply(p):
    L, B, G, Ct = layout_groupnorm(p)
    L["partial"] = Buf(F32, B * p.splits, 2 * G, 2 * G, "in")
    L["gamma"] = Buf(F32, 1, Ct, Ct)
    L["beta"] = Buf(F32, 1, Ct, Ct)
    L["y"] = Buf(F16, B * p.hw, Ct, Ct, "out")
    return L


def ref_gn_apply(p, v):
    """y = act(gamma (x - mean) rstd + beta) with the (mean, rstd) the statistics launch left in partial[b][0][g] (an input here)."""
    B, G = p.batch, p.groups
    x = f64(v["x0"]) if p.c1 == 0 else torch.cat([f64(v["x0"]), f64(v["x1"])], 1)
    Ct = x.shape[1]
    st = f64(v["partial"]).reshape(B, p.splits, G, 2)[:, 0]
    grp = torch.arange(Ct, device=x.device) // (Ct // G)
    img = torch.arange(B * p.hw, device=x.device) // p.hw
    mean, rstd = st[img][:, grp, 0], st[img][:, grp, 1]
    g, b = f64(v["gamma"]).reshape(1, -1), f64(v["beta"]).reshape(1, -1)
    z = g * (x - mean) * rstd
    y = _act(z + b, p.act)
    err = DACT * 4 * U32 * (z.abs() + g.abs() * (x.abs() + mean.abs()) * rstd + b.abs())
    return {"y": expect(y, err, F16, cap=CAP["groupnorm"])}


# ===================================================================================================================== small launchers
def layout_im2col(a):
    return {"x": Buf(F32, 1, a.batch * a.cin * a.h * a.wd, 0), "out": Buf(F16, a.batch * a.h * a.wd, a.kpad, a.kpad, "out")}


def ref_im2col(a, v):
    x = v["x"].reshape(a.batch, a.cin, a.h, a.wd).permute(0, 2, 3, 1).reshape(-1, a.cin)
    taps = conv_taps(x.double(), a.batch, a.h, a.wd, a.h, a.wd, 1, 0, 1)        # tap t -> [pixels, cin]
    cols = torch.stack(taps, 2).reshape(-1, a.cin * 9)                         # column k = ci * 9 + t
    out = torch.zeros(a.batch * a.h * a.wd, a.kpad, dtype=torch.float64, device=x.device)
    out[:, :a.cin * 9] = cols
    return {"out": Expect(out.to(F16).double(), torch.zeros_like(out), 0.0, None)}


def layout_conv_out(a):
    return {"x": Buf(F16, a.batch * a.h * a.wd, a.cin, a.cin), "w": Buf(F16, a.cout, 9 * a.cin, 9 * a.cin), "bias": Buf(F32, 1, a.cout, a.cout),
            "out": Buf(F32, a.batch * a.cout, a.h * a.wd, a.h * a.wd, "out")}


def ref_conv_out(a, v):
    x, w = f64(v["x"]), f64(v["w"])
    acc = torch.zeros(a.batch * a.h * a.wd, a.cout, dtype=torch.float64, device=x.device)
    S = torch.zeros_like(acc)
    for t, xt in enumerate(conv_taps(x, a.batch, a.h, a.wd, a.h, a.wd, 1, 0, 1)):
        wt = w[:, t * a.cin:(t + 1) * a.cin]
        acc += xt @ wt.T
        S += xt.abs() @ wt.abs().T
    acc = acc + f64(v["bias"]).reshape(1, -1)
    ref = acc.reshape(a.batch, a.h * a.wd, a.cout).permute(0, 2, 1).reshape(a.batch * a.cout, a.h * a.wd)
    err = (mfma_c(9 * a.cin) * S).reshape(a.batch, a.h * a.wd, a.cout).permute(0, 2, 1).reshape(a.batch * a.cout, a.h * a.wd)
    return {"out": expect(ref, err, F32, cap=CAP["conv_out"])}


def step_index(state: torch.Tensor) -> int:
    s = state.reshape(-1).cpu().tolist()
    return min(s[0], s[1] - 1) if s[1] > 0 else s[0]


def layout_timestep(a):
    L = {"timesteps": Buf(F32, 1, max(a.rows, 1), 0), "out": Buf(F16, a.rows, a.dim, a.dim, "out")}
    if a.state:
        L["state"] = Buf(I32, 1, 2, 2)
        L["timesteps"] = None            # extent known once the state is read (resolved by the audit)
    return L


def ref_timestep(a, v):
    half = a.dim // 2
    if "state" in v:
        t = v["timesteps"].reshape(-1)[step_index(v["state"])].double().reshape(1, 1).expand(a.rows, 1)
    else:
        t = f64(v["timesteps"]).reshape(-1)[:a.rows, None]
    k = torch.arange(half, dtype=torch.float64, device=t.device)
    arg = t * torch.exp(-math.log(10000.0) * k / half)[None, :]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    # fp32: the exponent (9.21 k / half: 2 ulps), expf and the product t * freq (one ulp each) -> 6 U32 |arg| on the argument of cos / sin
    # (slope <= 1), + cosf / sinf's own 2 ulps
    extra = 6 * U32 * torch.cat([arg, arg], 1).abs() + 4 * U32
    return {"out": expect(ref, extra, F16)}


def layout_cfg(a):
    n = a.n
    return {"eps_uncond": Buf(F32, 1, n, 0), "eps_cond": Buf(F32, 1, n, 0), "latents": Buf(F32, 1, n, 0, "inout"),
            "x0_prev": Buf(F32, 1, n, 0, "inout"), "coef": None, "state": Buf(I32, 1, 2, 2)}


def ref_cfg(a, v):
    """coef row (8 floats) {ca, cb, cx, c0, c1, -}: e = u + g (c - u); x0 = ca x + cb e; x' = cx x + c0 x0 + c1 x0_prev.  fp32: each of
    the <= 4 chained roundings is within U32 of the running magnitude sum -> 4 U32 M (x0), and x' also carries c0 x that error: 8 U32 M."""
    c = v["coef"].reshape(-1).double().cpu().tolist()
    ca, cb, cx, c0, c1 = c[:5]
    g = float(a.guidance)
    u, cc, x, xp = (f64(v[k]) for k in ("eps_uncond", "eps_cond", "latents", "x0_prev"))
    e = u + g * (cc - u)
    x0 = ca * x + cb * e
    xn = cx * x + c0 * x0 + c1 * xp
    me = u.abs() + abs(g) * (cc.abs() + u.abs())
    mx0 = abs(ca) * x.abs() + abs(cb) * me
    mx = abs(cx) * x.abs() + abs(c0) * mx0 + abs(c1) * xp.abs()
    return {"latents": Expect(xn, 8 * U32 * mx + 2.0 ** -140, 0.0, F32), "x0_prev": Expect(x0, 4 * U32 * mx0 + 2.0 ** -140, 0.0, F32)}


def layout_cfg_masked(a):
    L = layout_cfg(a)
    L.update(mask=Buf(F32, a.n // (a.channels * a.hw), a.hw, a.hw), known=Buf(F32, 1, a.n, 0), noise=Buf(F32, 1, a.n, 0))
    return L


def ref_cfg_masked(a, v):
    """pv_cfg_dpm_step's update x', then latents = m x' + (1 - m) k with k = q0 known + q1 noise, (q0, q1) = columns 5, 6 of the coefficient
    row and m [B][1][hw] broadcast over the channels; x0_prev receives the unblended x0.  fp32 roundings: k is two products and a sum
    (2 U32 M(k), M the sum of magnitudes), which the blend scales by |1 - m|; the blend itself rounds 1 - m, both products and the sum: at
    most 3 U32 (|m| |x'| + |1 - m| M(k)); x' 's own error e(x') passes scaled by |m|."""
    res = ref_cfg(a, v)
    c = v["coef"].reshape(-1).double().cpu().tolist()
    q0, q1 = c[5], c[6]
    B = a.n // (a.channels * a.hw)
    m = f64(v["mask"]).reshape(B, 1, a.hw).expand(B, a.channels, a.hw).reshape(1, -1)
    kn, nz = f64(v["known"]), f64(v["noise"])
    k = q0 * kn + q1 * nz
    mk = abs(q0) * kn.abs() + abs(q1) * nz.abs()
    xn, ex = res["latents"].ref, res["latents"].bound
    mag = m.abs() * (xn.abs() + ex) + (1 - m).abs() * mk
    res["latents"] = Expect(m * xn + (1 - m) * k, m.abs() * ex + 2 * U32 * (1 - m).abs() * mk + 3 * U32 * mag + 2.0 ** -140, 0.0, F32)
    return res


def layout_step_advance(a):
    return {"state": Buf(I32, 1, 1, 1, "inout")}


def ref_step_advance(a, v):
    s = v["state"].reshape(-1).double()
    return {"state": Expect((s + 1).reshape(1, 1), torch.zeros(1, 1, dtype=torch.float64, device=s.device), 0.0, None)}


def layout_pointwise(a):
    return {"x": Buf(F32, a.batch * a.cin, a.hw, a.hw), "w": Buf(F32, a.cout, a.cin, a.cin), "bias": Buf(F32, 1, a.cout, a.cout),
            "out": Buf(F32, a.batch * a.cout, a.hw, a.hw, "out")}


def ref_pointwise(a, v):
    x = f64(v["x"]).reshape(a.batch, a.cin, a.hw)
    w = f64(v["w"])
    out = torch.einsum("oc,bcp->bop", w, x)
    S = torch.einsum("oc,bcp->bop", w.abs(), x.abs())
    if "bias" in v:
        b = f64(v["bias"]).reshape(1, -1, 1)
        out, S = out + b, S + b.abs()
    # a (cin + 1)-term fp32 fma chain
    return {"out": expect(out.reshape(a.batch * a.cout, a.hw), gamma(a.cin + 1) * S.reshape(a.batch * a.cout, a.hw), F32)}


def layout_softmax_rows(a):
    return {"x": Buf(F16, a.rows, a.cols, a.ld, "inout")}


def ref_softmax_rows(a, v):
    s = f64(v["x"]) * float(a.scale)
    p = torch.softmax(s, 1)
    # exp2 of an fp32 fma argument (one ulp of |s log2 e| + |max| -> ln2 x that relative) and exp2's own ulp, the cols-term normaliser,
    # the reciprocal and the product: each relative to p
    arg = (s.abs() + s.max(1, keepdim=True).values.abs()) / LN2
    rel = LN2 * 2 * U32 * arg + gamma(a.cols) + 6 * U32
    return {"x": expect(p, rel * p, F16)}


def layout_posterior(a):
    n = a.batch * a.chw
    return {"moments": Buf(F32, a.batch, 2 * a.chw, 2 * a.chw), "eps": Buf(F32, 1, n, 0), "out": Buf(F32, 1, n, 0, "out")}


def ref_posterior(a, v):
    m = f64(v["moments"]).reshape(a.batch, 2, a.chw)
    mean, logvar = m[:, 0], m[:, 1].clamp(-30.0, 20.0)
    sd = torch.exp(0.5 * logvar)
    e = f64(v["eps"]).reshape(a.batch, a.chw)
    out = mean + sd * e
    # __expf = exp2(x log2 e): the product's ulp times |x| (relative on exp), exp2's ulp, then the fma
    term = (sd * e).abs() * (2 * U32 * (0.5 * logvar).abs() / LN2 * LN2 + 4 * U32) + 2 * U32 * (mean.abs() + (sd * e).abs())
    return {"out": expect(out.reshape(1, -1), term.reshape(1, -1), F32)}


# ===================================================================================================================== guided / stochastic / PAG steps
#: measured, not derived: ``tests/test_sampler_gpu.py``'s ``TOL_NOISE`` - the largest |z_kernel - z_fp64| the device's ``logf`` / ``sincospif`` /
#: ``sqrtf`` leave on a Box-Muller normal (their error is no IEEE quantity), with that file's margin of four
TOL_NOISE = 4 * 5.477e-7


def _f32(x) -> float:
    """A host scalar as the launcher receives it: rounded to fp32."""
    return torch.tensor(float(x), dtype=F32).item()


def _opt(p, name) -> bool:
    """An optional pointer (absent from the shorter argument lists of the same family counts as NULL)."""
    return bool(getattr(p, name, 0) or 0)


def step_reads(p):
    """(eps_image is read, eps_perturbed is read): the launcher's own substitutions - equal scales cancel the eps_image terms, a zero g_pag the
    perturbed term; the pointer is then not dereferenced."""
    return (_opt(p, "eps_image") and _f32(p.g_image) != _f32(p.g_text)), (_opt(p, "eps_perturbed") and _f32(getattr(p, "g_pag", 0.0)) != 0.0)


def layout_step(p):
    n = p.batch * p.channels * p.hw
    three, pag = step_reads(p)
    L = {"eps_uncond": Buf(F32, 1, n, 0), "eps_cond": Buf(F32, 1, n, 0), "latents": Buf(F32, 1, n, 0, "inout"), "x0_prev": Buf(F32, 1, n, 0, "inout"),
         "coef": None, "state": Buf(I32, 1, 2, 2)}
    if three:
        L["eps_image"] = Buf(F32, 1, n, 0)
    if pag:
        L["eps_perturbed"] = Buf(F32, 1, n, 0)
    if _opt(p, "rng"):
        L["rng"] = Buf(I32, 1, 4, 4)
    if _opt(p, "mask"):
        L.update(mask=Buf(F32, p.batch, p.hw, p.hw), known=Buf(F32, 1, n, 0), noise=Buf(F32, 1, n, 0))
    return L


def step_chain(chw: int) -> int:
    """Longest fp32 addition chain of the per-sample reductions of ``cfg_dpm_step_guided_kernel`` over ``chw`` elements: one workgroup of
    min(1024, nv rounded up to whole waves) threads (nv = chw / 4 float4s), each adding its 4 x trips elements in order, a 6-level shuffle tree inside
    the wave, then the wave slots in wave order.  A sum of same-sign terms is within ``chain x U32`` of exact, relative."""
    nv = max(chw // 4, 1)
    threads = 1024 if nv >= 1024 else (nv + 63) // 64 * 64
    return 4 * ((nv + threads - 1) // threads) + 6 + threads // 64


def ref_step(p, v):
    """pv_cfg_dpm_step_guided / _stochastic / _pag from the header, per sample b over chw = channels * hw elements, row {ca, cb, cx, c0, c1, q0, q1, cn}:
        e = eu + g_text (ec - eu)   |   eu + g_image (em - eu) + g_text (ec - em)          (+ g_pag (ec - ep))
        f = rescale std_b(ec) / std_b(e) + 1 - rescale  (rescale > 0 and std_b(e) > 0, else 1);  e = f e
        x0 = ca x + cb e;  x' = cx x + c0 x0 + c1 x0_prev (+ cn z);  with a mask  latents = m x' + (1 - m) (q0 known + q1 noise)
    z: ``oracle.philox`` from the rng words and the step index, both read from the device buffers.

    Bounds.  Every fp32 operation rounds within U32 of its own result (a fused multiply-add only removes roundings): in e each difference, its product
    with the scale and the running sum; in x0 = ca x + cb e the two products (U32 of their magnitudes M(x0) together) and the sum (at most M(x0) again);
    in x' three products (U32 M(x') together) and two sums: 3 U32 M(x'); the noise adds a product and a sum.
    The factor f (the rescale term; L = ``step_chain(chw)`` accounts for the two reductions over chw elements): with s = sqrt(sum of squared deviations),
        E(s) = (L / 2 + 2) U32 s            the sum's chain (relative L U32 on the sum, half on its root), the squares and the root
             + KAPPA eps                    the deviations' own roundings eps = max(err(e)) + U32 max|d|: independent over the elements, so
                                            2 sum d_i eps_i is a random sum of deviation 2 eps s - on s itself eps, taken KAPPA times
             + chw delta^2 / (2 s)          the mean's error delta = L U32 mean|v| + max err(v) + U32 |mean|: first order it cancels (sum d_i = 0)
        err(f) = rescale (E(s_c) / s_e + s_c E(s_e) / s_e^2) + 4 U32 (rescale s_c / s_e + |1 - rescale|)
    and err(f e) = |f| err(e) + |e| err(f) + U32 |f e|.  A sample with s_e = 0 in fp64 has f = 1 and err(f) = 0: that is the header's contract
    when the fp32 sums are exact too (an all-zero sample; a constant sample of dyadic values, as the catalogue's).  A constant sample whose fp32
    mean rounds has an undetermined f in the kernel - 0 / 0 of rounding residue - and no finite bound; the term chw delta^2 / (2 s) says so as s -> 0.
    The noise term: |cn| TOL_NOISE - a MEASURED number (the device's logf / sincospif are not IEEE operations), tests/test_sampler_gpu.py's."""
    B, chw = p.batch, p.channels * p.hw
    c = v["coef"].reshape(-1).double().cpu().tolist()
    ca, cb, cx, c0, c1, q0, q1, cn = c[:8]
    gt, gi, gp, rs = _f32(p.g_text), _f32(p.g_image), _f32(getattr(p, "g_pag", 0.0)), _f32(p.rescale)
    three, pag = step_reads(p)
    u, cc, x, xp = (f64(v[k]).reshape(B, chw) for k in ("eps_uncond", "eps_cond", "latents", "x0_prev"))
    # err(e): every operation's rounding is within U32 of ITS result - the difference, its product with the scale (twice the product's magnitude covers
    # both), the running sum
    if three:
        m_ = f64(v["eps_image"]).reshape(B, chw)
        part = u + gi * (m_ - u)
        e = part + gt * (cc - m_)
        ee = U32 * (2 * (gi * (m_ - u)).abs() + part.abs() + 2 * (gt * (cc - m_)).abs() + e.abs())
    else:
        e = u + gt * (cc - u)
        ee = U32 * (2 * (gt * (cc - u)).abs() + e.abs())
    if pag:
        pp = f64(v["eps_perturbed"]).reshape(B, chw)
        e = e + gp * (cc - pp)
        ee = ee + U32 * (2 * (gp * (cc - pp)).abs() + e.abs())
    if rs > 0:
        L = step_chain(chw)

        def root(t, err):
            mean = t.mean(1, keepdim=True)
            d = t - mean
            s = d.pow(2).sum(1, keepdim=True).sqrt()
            eps = err.amax(1, keepdim=True) + U32 * d.abs().amax(1, keepdim=True)
            delta = L * U32 * t.abs().mean(1, keepdim=True) + err.amax(1, keepdim=True) + U32 * mean.abs()
            return s, (L / 2 + 2) * U32 * s + KAPPA * eps + chw * delta ** 2 / (2 * s.clamp_min(1e-300))
        sc, Ec = root(cc, torch.zeros_like(cc))
        se, Ee = root(e, ee)
        live = se > 0
        sden = torch.where(live, se, torch.ones_like(se))
        f = torch.where(live, rs * sc / sden + (1 - rs), torch.ones_like(se))
        ef = torch.where(live, rs * (Ec / sden + sc * Ee / sden ** 2) + 4 * U32 * (rs * sc / sden + abs(1 - rs)), torch.zeros_like(se))
        ee = f.abs() * ee + e.abs() * ef + U32 * (f * e).abs()
        e = f * e
    x0 = ca * x + cb * e
    mx0 = abs(ca) * x.abs() + abs(cb) * e.abs()
    ex0 = abs(cb) * ee + 2 * U32 * mx0
    xn = cx * x + c0 * x0 + c1 * xp
    mx = abs(cx) * x.abs() + abs(c0) * (mx0 + ex0) + abs(c1) * xp.abs()
    exn = abs(c0) * ex0 + 3 * U32 * mx
    if "rng" in v:
        from .philox import noise_from_words
        z = noise_from_words(v["rng"].reshape(-1).cpu().tolist(), B, chw, step_index(v["state"])).to(x.device)
        xn = xn + cn * z
        exn = exn + abs(cn) * TOL_NOISE + 2 * U32 * (mx + abs(cn) * z.abs())
    if "mask" in v:
        m = f64(v["mask"]).reshape(B, 1, p.hw).expand(B, p.channels, p.hw).reshape(B, chw)
        kn, nz = f64(v["known"]).reshape(B, chw), f64(v["noise"]).reshape(B, chw)
        k = q0 * kn + q1 * nz
        mk = abs(q0) * kn.abs() + abs(q1) * nz.abs()
        mag = m.abs() * (xn.abs() + exn) + (1 - m).abs() * mk
        xn, exn = m * xn + (1 - m) * k, m.abs() * exn + 2 * U32 * (1 - m).abs() * mk + 3 * U32 * mag
    return {"latents": expect(xn.reshape(1, -1), exn.reshape(1, -1), F32), "x0_prev": expect(x0.reshape(1, -1), ex0.reshape(1, -1), F32)}


def layout_fusion_draw(p):
    L = {"rng": Buf(I32, 1, 4, 4, "inout"), "out": Buf(F32, p.n_layers, 2, 2, "out")}
    if _opt(p, "state"):
        L["state"] = Buf(I32, 1, 2, 2)
    if _opt(p, "forced"):
        L["forced"] = Buf(F32, 1, p.n_layers, p.n_layers)
    return L


def ref_fusion_draw(p, v):
    """out[layer] = (w_text, w_ip): u < rule1 -> (scale, 0); u > rule2 -> (0, scale); else (1, 1), u = ``oracle.philox.fusion_uniform`` of the rng
    words (forced[layer] >= 0 replaces it); with only_last_step and a state the rule holds at state[0] == state[1] - 1 alone.  rng[2] advances by one.
    Every value is exact: u has 24 bits, the comparisons are fp32 ones, the outputs are the fp32 scale, 0 or 1."""
    from .philox import fusion_uniform
    n = p.n_layers
    words = v["rng"].reshape(-1).cpu().tolist()
    u = torch.from_numpy(fusion_uniform(words, n))
    if "forced" in v:
        fo = f64(v["forced"]).reshape(-1).cpu()
        u = torch.where(fo >= 0, fo, u)
    on = True
    if p.only_last_step and "state" in v:
        s = v["state"].reshape(-1).cpu().tolist()
        on = s[0] == s[1] - 1
    sc, r1, r2 = _f32(p.scale), _f32(p.rule1), _f32(p.rule2)
    out = torch.ones(n, 2, dtype=torch.float64)
    if on:
        out[u < r1] = torch.tensor([sc, 0.0], dtype=torch.float64)
        out[(u >= r1) & (u > r2)] = torch.tensor([0.0, sc], dtype=torch.float64)
    dev = v["out"].device
    nxt = list(words)
    nxt[2] = ((int(words[2]) & 0xFFFFFFFF) + 1) & 0xFFFFFFFF
    nxt[2] -= (1 << 32) if nxt[2] >= (1 << 31) else 0
    return {"out": Expect(out.to(dev), torch.zeros(n, 2, dtype=torch.float64, device=dev), 0.0, None),
            "rng": Expect(torch.tensor([nxt], dtype=torch.float64, device=dev), torch.zeros(1, 4, dtype=torch.float64, device=dev), 0.0, None)}


# ===================================================================================================================== FreeU, resize, pointwise fp32
def layout_freeu(p):
    rows = p.batch * p.h * p.w
    L = {}
    if _opt(p, "x"):
        L.update(x=Buf(F16, rows, p.cx, p.ldx), x_out=Buf(F16, rows, p.cx, p.ldxo, "out"))
    if _opt(p, "skip"):
        L.update(skip=Buf(F16, rows, p.cs, p.lds), skip_out=Buf(F16, rows, p.cs, p.ldso, "out"))
    return L


def freeu_chain(hw: int) -> int:
    """Longest fp32 chain of one of pv_freeu_rows' seven plane sums: 16 pixel lanes of ceil(hw / 16) terms each, then the lanes in order."""
    return (hw + 15) // 16 + 16


def ref_freeu(p, v):
    """Backbone: x_out = fp16(float(x) * b) in the first cx / 2 columns (one fp32 product), the other columns bit for bit.  Skip: per (image, channel)
    plane the frequencies (u, v) in {0, -1}^2 times s, in the header's closed form  p + (s - 1) / (h w) Sum_{u,v} Re(X[u,v] e^{+2 pi i (u y/h + v x/w)}).
    Bound of the skip, with L = ``freeu_chain(hw)`` and S = Sum|p| over the plane: each of the seven sums is an fp32 chain of L terms p x (a cosine /
    sine: sincospif's 2 ulps, the angle sum's two products and sum 4 more), so within (L + 6) U32 S; it is scaled once (1), multiplied with such a cosine /
    sine again (6 + 1) and added (1): (L + 15) U32 S per term, seven terms, times |s - 1| / (h w); then one fp32 add before the fp16 store."""
    res = {}
    B, h, w = p.batch, p.h, p.w
    if "x" in v:
        x = f64(v["x"])
        half = p.cx // 2
        b = _f32(p.b)
        ref = x.clone()
        ref[:, :half] *= b
        det = torch.zeros_like(ref)
        det[:, :half] = U32 * ref[:, :half].abs()
        res["x_out"] = expect(ref, det, F16)
        res["x_out (upper half)"] = Expect(x[:, half:], torch.zeros_like(x[:, half:]), 0.0, None, derive=lambda got, half=half: got["x_out"][:, half:])
    if "skip" in v:
        sk = f64(v["skip"])
        s = _f32(p.s)
        pl = sk.reshape(B, h, w, p.cs)
        yy = (torch.arange(h, dtype=torch.float64, device=sk.device) / h).view(1, h, 1, 1)
        xx = (torch.arange(w, dtype=torch.float64, device=sk.device) / w).view(1, 1, w, 1)
        upd = torch.zeros_like(pl)
        for fu in (0, -1):
            for fv in (0, -1):
                ph = 2 * math.pi * (fu * yy + fv * xx)
                Xr = (pl * torch.cos(ph)).sum((1, 2), keepdim=True)          # X = Sum p e^{-i ph}
                Xi = -(pl * torch.sin(ph)).sum((1, 2), keepdim=True)
                upd = upd + Xr * torch.cos(ph) - Xi * torch.sin(ph)          # Re(X e^{+i ph})
        k = (s - 1.0) / (h * w)
        ref = pl + k * upd
        sabs = pl.abs().sum((1, 2), keepdim=True)
        det = abs(k) * 7 * (freeu_chain(h * w) + 15) * U32 * sabs + U32 * ref.abs()
        res["skip_out"] = expect(ref.reshape(-1, p.cs), det.expand_as(ref).reshape(-1, p.cs), F16)
    return res


def bilinear_taps(n_in: int, n_out: int, device):
    """One axis of F.interpolate(mode="bilinear", align_corners=False): src = max((dst + 0.5) in / out - 0.5, 0) as the exact ratio
    ((2 dst + 1) in - out) / (2 out), i0 = floor(src), i1 = min(i0 + 1, in - 1), weight = src - i0."""
    dst = torch.arange(n_out, dtype=torch.float64, device=device)
    src = (((2 * dst + 1) * n_in - n_out) / (2 * n_out)).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), src - i0


def layout_resize(p):
    planes = p.batch * p.channels
    L = {"x": Buf(F32, 1, planes * p.h * p.w, 0), "out": Buf(F32, 1, planes * p.oh * p.ow, 0, "out")}
    if _opt(p, "ca"):
        L["ca"] = Buf(F32, 1, p.batch, p.batch)
    if _opt(p, "y"):
        L.update(y=Buf(F32, 1, planes * p.oh * p.ow, 0), cb=Buf(F32, 1, p.batch, p.batch))
    return L


def ref_resize(p, v):
    """out[b][c] = ca[b] bilinear(x[b][c]: h x w -> oh x ow) (+ cb[b] y[b][c]); a weight of exactly 0 returns the tap itself (no 0 x b product).
    Bound: a mix (1 - t) a + t b rounds the weight, 1 - t, two products and a sum - 5 U32 of its magnitudes; two levels of it; then the product with ca
    and the product and sum with cb y: 3 U32 of theirs."""
    B, C_ = p.batch, p.channels
    x = f64(v["x"]).reshape(B, C_, p.h, p.w)
    y0, y1, wy = bilinear_taps(p.h, p.oh, x.device)
    x0, x1, wx = bilinear_taps(p.w, p.ow, x.device)
    wy = wy.view(p.oh, 1)

    def mix(a, b, t):
        return torch.where(t == 0, a, (1 - t) * a + t * b)
    top, bot = mix(x[:, :, y0][..., x0], x[:, :, y0][..., x1], wx), mix(x[:, :, y1][..., x0], x[:, :, y1][..., x1], wx)
    r = mix(top, bot, wy)
    xa = x.abs()
    mag = mix(mix(xa[:, :, y0][..., x0], xa[:, :, y0][..., x1], wx), mix(xa[:, :, y1][..., x0], xa[:, :, y1][..., x1], wx), wy)
    det = 10 * U32 * mag
    if "ca" in v:
        ca = f64(v["ca"]).reshape(B, 1, 1, 1)
        r, mag, det = ca * r, ca.abs() * mag, ca.abs() * det
    if "y" in v:
        t = f64(v["cb"]).reshape(B, 1, 1, 1) * f64(v["y"]).reshape(B, C_, p.oh, p.ow)
        r, mag = r + t, mag + t.abs()
    if "ca" in v or "y" in v:
        det = det + 3 * U32 * mag
    return {"out": expect(r.reshape(1, -1), det.reshape(1, -1), F32)}


def layout_affine_rows(p):
    n = p.per_sample * p.batch
    L = {"x": Buf(F32, 1, n, 0), "ca": Buf(F32, 1, p.batch, p.batch), "out": Buf(F32, 1, n, 0, "out")}
    if _opt(p, "y"):
        L.update(y=Buf(F32, 1, n, 0), cb=Buf(F32, 1, p.batch, p.batch))
    return L


def ref_affine_rows(p, v):
    """out[b][i] = ca[b] x[b][i] (+ cb[b] y[b][i]): one product (the store's rounding), or two products and a sum: 2 U32 of the magnitudes."""
    B = p.batch
    r = f64(v["ca"]).reshape(B, 1) * f64(v["x"]).reshape(B, p.per_sample)
    det = torch.zeros_like(r)
    if "y" in v:
        t = f64(v["cb"]).reshape(B, 1) * f64(v["y"]).reshape(B, p.per_sample)
        det = 2 * U32 * (r.abs() + t.abs())
        r = r + t
    return {"out": expect(r.reshape(1, -1), det.reshape(1, -1), F32)}


def layout_composite(p):
    n = p.batch * p.channels * p.hw
    return {"gen": Buf(F32, 1, n, 0), "orig": Buf(F32, 1, n, 0), "mask": Buf(F32, p.batch, p.hw, p.hw), "out": Buf(F32, 1, n, 0, "out")}


def ref_composite(p, v):
    """out = clamp(m gen + (1 - m) orig, lo, hi), m [B][1][hw] over the channels; out may be gen.  1 - m, two products, a sum: 4 U32 of the magnitudes
    (the clamp only moves a value towards the reference's)."""
    B, hw = p.batch, p.hw
    m = f64(v["mask"]).reshape(B, 1, hw).expand(B, p.channels, hw).reshape(1, -1)
    g, o = f64(v["gen"]), f64(v["orig"])
    r = (m * g + (1 - m) * o).clamp(_f32(p.lo), _f32(p.hi))
    return {"out": expect(r, 4 * U32 * ((m * g).abs() + ((1 - m) * o).abs()), F32)}


def layout_clamp(p):
    return {"x": Buf(F32, 1, p.n, 0, "inout")}


def ref_clamp(p, v):
    """In place, exact."""
    r = f64(v["x"]).clamp(_f32(p.lo), _f32(p.hi))
    return {"x": Expect(r, torch.zeros_like(r), 0.0, None)}


# ===================================================================================================================== conditioning front ends
def layout_rows_mean(p):
    return {"x": Buf(F16, (p.groups - 1) * p.group_rows + p.count, p.cols, p.ldx), "y": Buf(F16, p.groups, p.cols, p.ldy, "inout" if p.accumulate else "out")}


def ref_rows_mean(p, v):
    """y[g] (+)= mean of the ``count`` rows from g * group_rows on.  fp32: eight row lanes of ceil(count / 8) terms each, then the lanes in order - a chain
    of ceil(count / 8) + 8 on Sum|x| -, the division and the sum with the previous y: 2 U32 of their magnitudes."""
    x = f64(v["x"])
    idx = (torch.arange(p.groups, device=x.device) * p.group_rows)[:, None] + torch.arange(p.count, device=x.device)[None, :]
    blk = x[idx]                                                     # [groups, count, cols]
    mean, mabs = blk.mean(1), blk.abs().mean(1)
    prev = f64(v["y"]) if p.accumulate else torch.zeros_like(mean)
    det = ((p.count + 7) // 8 + 8) * U32 * mabs + 2 * U32 * (mean.abs() + prev.abs())
    return {"y": expect(mean + prev, det, F16)}


def round_f16(x: torch.Tensor) -> torch.Tensor:
    """fp64 values rounded to the fp16 grid, to nearest, ties to even, overflow (>= 65520) to infinity - in integer steps of the value's quantum
    2^(max(e, -14) - 10), written out here and not through a library cast."""
    ax = x.abs()
    _, ex = torch.frexp(ax.clamp_min(2.0 ** -30))                    # ax = m 2^ex, m in [0.5, 1): e = ex - 1
    k = (ex - 1).clamp(-14, 16).long() - 10                          # a table of exact powers of two (a device's pow() need not be exact)
    q = torch.tensor([2.0 ** i for i in range(-24, 7)], dtype=torch.float64, device=x.device)[k + 24]
    r = torch.round(ax / q) * q                                      # torch.round: half to even; the division by a power of two is exact
    r = torch.where(r >= 65520.0, torch.full_like(r, float("inf")), r)
    r = torch.where(torch.isinf(ax), ax, r)
    return torch.copysign(r, x)


def _bits16(t):
    return t.contiguous().view(torch.int16)


def layout_cast_to_f16(p):
    return {"x": Buf(F32, 1, p.n, 0), "y": Buf(F16, 1, p.n, 0, "out")}


def ref_cast_to_f16(p, v):
    """Round to nearest even, overflow to infinity, signed zeros kept: exact (value and sign bit)."""
    r = round_f16(f64(v["x"]))
    z = torch.zeros_like(r)
    return {"y": Expect(r, z, 0.0, None), "y (sign)": Expect(torch.signbit(r).double(), z, 0.0, None, derive=lambda got: torch.signbit(got["y"]))}


def layout_cast_to_f32(p):
    return {"x": Buf(F16, 1, p.n, 0), "y": Buf(F32, 1, p.n, 0, "out")}


def ref_cast_to_f32(p, v):
    """Exact: every fp16 value (subnormals, infinities, signed zeros) is an fp32 value."""
    r = f64(v["x"])
    z = torch.zeros_like(r)
    return {"y": Expect(r, z, 0.0, None), "y (sign)": Expect(torch.signbit(r).double(), z, 0.0, None, derive=lambda got: torch.signbit(got["y"]))}


def layout_patchify(p):
    g = p.img // p.patch
    return {"x": Buf(F32, 1, p.batch * p.ch * p.img * p.img, 0), "out": Buf(F16, p.batch * g * g, p.kpad, p.kpad, "out")}


def ref_patchify(p, v):
    """Row = one patch in (channel, py, px) order, rounded to fp16, zero padded to kpad (the padding is output): exact."""
    g, P = p.img // p.patch, p.patch
    x = f64(v["x"]).reshape(p.batch, p.ch, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(p.batch * g * g, p.ch * P * P)
    out = torch.zeros(p.batch * g * g, p.kpad, dtype=torch.float64, device=x.device)
    out[:, :p.ch * P * P] = round_f16(x)
    return {"out": Expect(out, torch.zeros_like(out), 0.0, None)}


def layout_vision_embed(p):
    return {"patches": Buf(F16, p.batch * (p.ntok - 1), p.dim, p.dim), "cls": Buf(F32, 1, p.dim, p.dim), "pos": Buf(F32, p.ntok, p.dim, p.dim),
            "out": Buf(F16, p.batch * p.ntok, p.dim, p.dim, "out")}


def ref_vision_embed(p, v):
    """out[b][0] = cls + pos[0]; out[b][1 + i] = patches[b][i] + pos[1 + i]: one fp32 sum, then the fp16 store."""
    B, T, dim = p.batch, p.ntok, p.dim
    tokv = torch.cat([f64(v["cls"]).reshape(1, 1, dim).expand(B, 1, dim), f64(v["patches"]).reshape(B, T - 1, dim)], 1)
    pos = f64(v["pos"]).reshape(1, T, dim)
    return {"out": expect((tokv + pos).reshape(B * T, dim), (U32 * (tokv.abs() + pos.abs())).reshape(B * T, dim), F16)}


def layout_text_embed(p):
    L = {"ids": Buf(I64, p.batch, p.seq, p.seq), "tok": None, "pos": Buf(F32, p.seq, p.dim, p.dim), "out": Buf(F16, p.batch * p.seq, p.dim, p.dim, "out")}
    if p.n_concept > 0:
        L.update(concept=Buf(F16, p.batch * p.n_concept, p.dim, p.dim), placeholder_idx=Buf(I64, 1, p.batch, p.batch))
    return L


def ref_text_embed(p, v):
    """Row j of sample b: tok[ids[b][j]] before the placeholder position i = placeholder_idx[b], concept[b][j - i] on the n_concept positions from it,
    tok[ids[b][j - n_concept + 1]] behind (the tail shifted right by n_concept - 1, truncated); + pos[j]: one fp32 sum, then the fp16 store.
    n_concept == 0: the stock embedding (placeholder_idx and concept are not read)."""
    B, S, dim, E = p.batch, p.seq, p.dim, p.n_concept
    ids = v["ids"].reshape(B, S).long()
    tok = f64(v["tok"])
    j = torch.arange(S, device=ids.device)[None, :].expand(B, S)
    if E > 0:
        i = v["placeholder_idx"].reshape(B, 1).long()
        src = torch.where(j < i, j, (j - E + 1).clamp(0, S - 1))
        val = tok[torch.gather(ids, 1, src)]
        inside = (j >= i) & (j < i + E)
        con = f64(v["concept"]).reshape(B, E, dim)
        cj = (j - i).clamp(0, E - 1)
        val = torch.where(inside[..., None], torch.gather(con, 1, cj[..., None].expand(B, S, dim)), val)
    else:
        val = tok[ids]
    pos = f64(v["pos"]).reshape(1, S, dim)
    return {"out": expect((val + pos).reshape(B * S, dim), (U32 * (val.abs() + pos.abs())).reshape(B * S, dim), F16)}


# ===================================================================================================================== the training tape: pointwise
# Single launches of the training tape (the backward passes of the stock blocks, the ArcFace identity loss, the reductions of the losses and of the
# optimizer): the same rules - semantics from the header alone, fp64 on the exact fp16 / fp32 inputs, every constant derived.
#
# The fp32 expressions of the pointwise fp16 launchers are a handful of operations; their error sits three orders below the fp16 store (U32 / U16 =
# 2^-13).  What is used of the device, from the CDNA ISA's documented accuracy: v_exp_f32, v_rcp_f32 and v_rsq_f32 are within one ulp (2 U32); a division
# is allowed two ulps (4 U32).  ``__expf(t)`` is exp2 of the rounded product t log2 e: the product's rounding moves the exponent by U32 |t| log2 e, the
# exponential by ln 2 times that, relative: |t| U32; with exp2's own ulp: (|t| + 2) U32 - derived, so no measured term enters these bounds.
# sigmoid(t) = 1 / (1 + e), e = exp(-t): the relative error of e reaches s scaled by e / (1 + e) = 1 - s; the sum and the division add 5 U32.
ACT_NAMES = {0: "none", 1: "silu", 2: "quick-gelu", 3: "leaky-relu", 4: "gelu"}


def _sigmoid_err(t, s):
    """Relative error of the fp32 sigmoid(t) as the kernels form it (1 / (1 + __expf(-t))), in units of U32."""
    return (t.abs() + 3) * (1 - s) + 5


def _pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _cdf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _act_grad(x, act):
    """(act'(x), its absolute fp32 error bound) for the activation codes of the header."""
    if act == 0:
        return torch.ones_like(x), torch.zeros_like(x)
    if act in (1, 2):
        a = 1.0 if act == 1 else 1.702
        s = torch.sigmoid(a * x)
        g = s * (1 + a * x * (1 - s))
        # s carries R U32 relative; 1 - s then s R U32 absolute; the products and the sum round four times
        R = _sigmoid_err(a * x, s)
        return g, U32 * (R * (g.abs() + s * s * (a * x).abs()) + 4 * s * (1 + (a * x).abs() * (1 - s)))
    if act == 3:
        g = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.01))
        return g, U32 * g                                   # 0.01f is the fp32 nearest to 0.01
    if act == 4:
        pdf = _pdf(x)
        g = _cdf(x) + x * pdf
        # Phi through an erf approximation: GELU_APPROX |x| on gelu is GELU_APPROX on its derivative; phi through __expf(-x^2 / 2)
        return g, GELU_APPROX + U32 * ((0.5 * x * x + 4) * (x * pdf).abs() + 4 * g.abs())
    raise ValueError(f"unknown activation {act}")


def _act_err(x, y, act):
    """Absolute fp32 error bound of y = act(x) before the store."""
    if act == 0:
        return torch.zeros_like(x)
    if act in (1, 2):
        a = 1.0 if act == 1 else 1.702
        return U32 * (_sigmoid_err(a * x, torch.sigmoid(a * x)) + 2) * y.abs()
    if act == 3:
        return 2 * U32 * y.abs()
    return (GELU_APPROX + 8 * U32) * x.abs()


def layout_act_forward(p):
    return {"x": Buf(F16, p.rows, p.cols, p.ldx), "y": Buf(F16, p.rows, p.cols, p.ldy, "out")}


def ref_act_forward(p, v):
    x = f64(v["x"])
    y = _act(x, p.act)
    return {"y": expect(y, _act_err(x, y, p.act), F16, cap=CAP["pointwise16"])}


def layout_act_backward(p):
    return {"x": Buf(F16, p.rows, p.cols, p.ldx), "dy": Buf(F16, p.rows, p.cols, p.lddy), "dx": Buf(F16, p.rows, p.cols, p.lddx, "out")}


def ref_act_backward(p, v):
    """dx = dy act'(x): the derivative's error times |dy|, and the product's rounding."""
    x, dy = f64(v["x"]), f64(v["dy"])
    g, eg = _act_grad(x, p.act)
    return {"dx": expect(dy * g, dy.abs() * eg + U32 * (dy * g).abs(), F16, cap=CAP["pointwise_bwd"])}


def layout_geglu(p):
    return {"x": Buf(F16, p.rows, 2 * p.n, p.ldx), "out": Buf(F16, p.rows, p.n, p.ldo, "out")}


def ref_geglu(p, v):
    x = f64(v["x"])
    a, g = x[:, :p.n], x[:, p.n:]
    y = a * _gelu(g)
    return {"out": expect(y, a.abs() * (GELU_APPROX + 8 * U32) * g.abs() + U32 * y.abs(), F16, cap=CAP["pointwise16"])}


def layout_geglu_backward(p):
    return {"h": Buf(F16, p.rows, 2 * p.n, p.ldh), "dy": Buf(F16, p.rows, p.n, p.lddy), "dh": Buf(F16, p.rows, 2 * p.n, p.lddh, "out")}


def ref_geglu_backward(p, v):
    """y = a gelu(g), h = [a | g]: dh = [dy gelu(g) | dy a gelu'(g)]."""
    h, dy = f64(v["h"]), f64(v["dy"])
    a, g = h[:, :p.n], h[:, p.n:]
    gp, egp = _act_grad(g, 4)
    da, dg = dy * _gelu(g), dy * a * gp
    eda = dy.abs() * (GELU_APPROX + 8 * U32) * g.abs() + U32 * da.abs()
    edg = (dy * a).abs() * egp + 2 * U32 * dg.abs()
    return {"dh": expect(torch.cat([da, dg], 1), torch.cat([eda, edg], 1), F16, cap=CAP["pointwise_bwd"])}


def layout_col_affine(p):
    L = {"x": Buf(F16, p.rows, p.cols, p.ldx), "scale": Buf(F32, 1, p.cols, 0), "y": Buf(F16, p.rows, p.cols, p.ldy, "out")}
    if _ptr(p, "shift"):
        L["shift"] = Buf(F32, 1, p.cols, 0)
    return L


def ref_col_affine(p, v):
    t = f64(v["x"]) * f64(v["scale"])
    sh = f64(v["shift"]) if "shift" in v else torch.zeros_like(t[:1])
    return {"y": expect(t + sh, 2 * U32 * (t.abs() + sh.abs()), F16, cap=CAP["pointwise16"])}


def layout_prelu(p):
    L = {"x": Buf(F16, p.rows, p.cols, p.ldx), "slope": Buf(F32, 1, 1, 0), "out": Buf(F16, p.rows, p.cols, p.ldo, "out")}
    if _ptr(p, "dy"):
        L["dy"] = Buf(F16, p.rows, p.cols, p.lddy)
    return L


def ref_prelu(p, v):
    """dy NULL: x > 0 ? x : a x; else dy (x > 0 ? 1 : a) - x = 0 takes the slope branch.  One fp32 product."""
    x, a = f64(v["x"]), f64(v["slope"]).reshape(())
    k = torch.where(x > 0, torch.ones_like(x), a * torch.ones_like(x))
    y = (f64(v["dy"]) if "dy" in v else x) * k
    return {"out": expect(y, U32 * y.abs(), F16, cap=CAP["pointwise16"])}


def layout_add_rows(p):
    return {"a": Buf(F16, p.rows, p.cols, p.lda), "b": Buf(F16, p.rows, p.cols, p.ldb), "out": Buf(F16, p.rows, p.cols, p.ldo, "out")}


def ref_add_rows(p, v):
    """fp16(float(a) + float(b)) is the correctly rounded exact sum.  The fp32 sum is inexact only when the exponents differ by 14 or more; then
    |b| < 2^(e_a - 13), an eighth of a's fp16 ulp (a quarter of the ulp below a power of two): the fp32 result stays strictly inside the interval that
    rounds to a, as the exact sum does.  So the compare is exact, against ``round_f16`` of the fp64 sum (exact: 40 bits at most)."""
    r = round_f16(f64(v["a"]) + f64(v["b"]))
    return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}


def dropout_keep(words, rows, cols, copies, p32, site):
    """keep[k][r][c] of pv_dropout_f16 (header): chunk q = r (cols / 8) + c / 8; Philox4x32-10 block at key (rng[0], rng[1]), counter
    (q, site, rng[2], k); element j = c % 8 takes the 16-bit lane (word[j / 2] >> 16 (j % 2)) & 0xFFFF; keep = lane >= uint32(p * 65536)."""
    import numpy as np
    from .philox import philox4x32_10
    k0, k1, it = (int(w) & 0xFFFFFFFF for w in words[:3])
    thr = int(float(p32) * 65536.0)
    q = np.arange(rows * (cols // 8), dtype=np.uint64)
    keep = np.empty((copies, rows, cols), dtype=bool)
    for k in range(copies):
        w = philox4x32_10((k0, k1), (q, int(site) & 0xFFFFFFFF, it, k))
        lanes = np.stack([(w[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF) for j in range(8)], 1)      # [chunks, 8]
        keep[k] = (lanes >= thr).reshape(rows, cols)
    return torch.from_numpy(keep)


def layout_dropout(p):
    wide = p.copies * p.cols
    L = {"x": Buf(F16, p.rows, wide if p.backward else p.cols, p.ldx), "out": Buf(F16, p.rows, p.cols if p.backward else wide, p.ldo, "out"),
         "rng": Buf(I32, 1, 3, 0)}
    if p.backward and _ptr(p, "add"):
        L["add"] = Buf(F16, p.rows, p.cols, p.ldadd)
    return L


def ref_dropout(p, v):
    """inv = 1 / (1 - p) in fp32 (the difference, the reciprocal: 3 U32 with the product; p = 0: exactly 1); the backward adds ``add`` and the copies in
    order: a chain of copies + 1."""
    p32 = _f32(p.p)
    keep = dropout_keep(v["rng"].reshape(-1).cpu().tolist(), p.rows, p.cols, p.copies, p32, p.site).to(v["x"].device).double()
    inv = 1.0 / (1.0 - p32)
    x = f64(v["x"])
    if not p.backward:
        y = torch.cat([x * keep[k] * inv for k in range(p.copies)], 1)
        return {"out": expect(y, 3 * U32 * y.abs(), F16)}
    terms = [x[:, k * p.cols:(k + 1) * p.cols] * keep[k] * inv for k in range(p.copies)]
    if "add" in v:
        terms.append(f64(v["add"]))
    mag = sum(t.abs() for t in terms)
    return {"out": expect(sum(terms), (3 + p.copies + 1) * U32 * mag, F16)}


def layout_softmax_rows_backward(p):
    return {"p": Buf(F16, p.rows, p.cols, p.ldp), "dp": Buf(F16, p.rows, p.cols, p.lddp, "inout")}


def ref_softmax_rows_backward(p, v):
    """dp <- scale p (dp - Sum_j p_j dp_j).  The dot product: 256 threads of 8 ceil(cols / 2048) terms each, a 6-level tree per wave, two levels over
    the waves; then the difference and two products."""
    pm, dp = f64(v["p"]), f64(v["dp"])
    sc = _f32(p.scale)
    dot = (pm * dp).sum(1, keepdim=True)
    chain = 8 * ((p.cols // 8 + 255) // 256) + 6 + 2 + 1
    edot = chain * U32 * (pm * dp).abs().sum(1, keepdim=True)
    ref = sc * pm * (dp - dot)
    return {"dp": expect(ref, (sc * pm).abs() * (edot + 3 * U32 * (dp.abs() + dot.abs())), F16, cap=CAP["pointwise_bwd"])}


# ===================================================================================================================== the training tape: layout, exact
def layout_transpose(p):
    return {"x": Buf(F16, p.rows, p.cols, p.ldx), "out": Buf(F16, p.cols, p.rows_pad, p.ldo, "out")}


def ref_transpose(p, v):
    r = torch.zeros(p.cols, p.rows_pad, dtype=torch.float64, device=v["x"].device)
    r[:, :p.rows] = f64(v["x"]).T
    return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}


def layout_dilate(p):
    return {"x": Buf(F16, p.batch * p.h * p.w, p.c, p.ldx), "z": Buf(F16, p.batch * 4 * p.h * p.w, p.c, p.c, "out")}


def ref_dilate(p, v):
    z = torch.zeros(p.batch, 2 * p.h, 2 * p.w, p.c, dtype=torch.float64, device=v["x"].device)
    z[:, ::2, ::2] = f64(v["x"]).reshape(p.batch, p.h, p.w, p.c)
    z = z.reshape(-1, p.c)
    return {"z": Expect(z, torch.zeros_like(z), 0.0, None)}


def layout_pool2x(p):
    L = {"g": Buf(F16, p.batch * 4 * p.h * p.w, p.c, p.c), "out": Buf(F16, p.batch * p.h * p.w, p.c, p.c, "out")}
    if _ptr(p, "add"):
        L["add"] = Buf(F16, p.batch * p.h * p.w, p.c, p.ldadd)
    return L


def ref_pool2x(p, v):
    """add, then the four taps in row-major order: an fp32 chain of four."""
    g = f64(v["g"]).reshape(p.batch, p.h, 2, p.w, 2, p.c)
    s, mag = g.sum((2, 4)).reshape(-1, p.c), g.abs().sum((2, 4)).reshape(-1, p.c)
    if "add" in v:
        s, mag = s + f64(v["add"]), mag + f64(v["add"]).abs()
    return {"out": expect(s, 4 * U32 * mag, F16, cap=CAP["pointwise16"])}


def layout_maxpool(p):
    full, half = p.batch * p.h * p.w, p.batch * (p.h // 2) * (p.w // 2)
    L = {"x": Buf(F16, full, p.c, p.c), "out": Buf(F16, full if _ptr(p, "dy") else half, p.c, p.c, "out")}
    if _ptr(p, "dy"):
        L["dy"] = Buf(F16, half, p.c, p.c)
    return L


def ref_maxpool(p, v):
    """Windows in (0,0), (0,1), (1,0), (1,1) order; the backward routes dy to the FIRST maximum of that order, zero elsewhere.  Exact."""
    B, h, w, c = p.batch, p.h, p.w, p.c
    win = f64(v["x"]).reshape(B, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, h // 2, w // 2, 4, c)
    mx = win.max(3).values
    if "dy" not in v:
        r = mx.reshape(-1, c)
        return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}
    is_max = win == mx.unsqueeze(3)
    first = is_max & (is_max.cumsum(3) == 1)
    r = (first * f64(v["dy"]).reshape(B, h // 2, w // 2, 1, c)).reshape(B, h // 2, w // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, c)
    return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}


def layout_sign(p):
    return {"x": Buf(F32, 1, p.n, 0), "out": Buf(F32, 1, p.n, 0, "out")}


def ref_sign(p, v):
    r = _f32(p.coef) * torch.sign(f64(v["x"]))
    return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}


def layout_clamp_mask(p):
    return {"y": Buf(F32, 1, p.n, 0), "dy": Buf(F32, 1, p.n, 0), "out": Buf(F32, 1, p.n, 0, "out")}


def ref_clamp_mask(p, v):
    """dy where lo < y < hi (both strict), else 0.  Exact."""
    y, dy = f64(v["y"]), f64(v["dy"])
    r = torch.where((y > _f32(p.lo)) & (y < _f32(p.hi)), dy, torch.zeros_like(dy))
    return {"out": Expect(r, torch.zeros_like(r), 0.0, None)}


def layout_gather_rows(p):
    return {"x": Buf(F16, p.batch * p.seq, p.dim, p.ldx), "idx": Buf(I32, 1, p.batch, 0), "out": Buf(F32, 1, p.batch * p.n_e * p.dim, 0, "out")}


def ref_gather_rows(p, v):
    """out[b][e] = scale x[b seq + idx[b] + e] where 0 <= idx[b] + e < seq, else 0 (a row of another sample is never read): one fp32 product."""
    x = f64(v["x"]).reshape(p.batch, p.seq, p.dim)
    row = v["idx"].reshape(p.batch, 1).long() + torch.arange(p.n_e, device=x.device)[None, :]
    ok = (row >= 0) & (row < p.seq)
    r = torch.gather(x, 1, row.clamp(0, p.seq - 1)[..., None].expand(p.batch, p.n_e, p.dim)) * _f32(p.scale) * ok[..., None]
    return {"out": expect(r.reshape(1, -1), torch.zeros(1, r.numel(), dtype=torch.float64, device=x.device), F32)}


# ===================================================================================================================== the training tape: reductions
def blocks_chain(nblk: int) -> int:
    """Longest fp32 addition chain of pv_reduce_blocks (header): eight groups, group g adds blocks g, g + 8, ... into four accumulators (blocks 32 apart,
    then at most three single ones into the first), (a0 + a1) + (a2 + a3), the eight groups in order, the product with ``scale``."""
    return (nblk + 31) // 32 + 3 + 2 + 7 + 1


def mean_chain(n: int, n_partial: int) -> int:
    """pv_reduce_mean / pv_reduce_sumsq (header): n_partial workgroups of 256 threads stride over the elements (ceil(n / (256 n_partial)) terms a thread), a
    6-level tree per wave, two levels over the four waves, the partials in order, the product with the scale."""
    return (n + 256 * n_partial - 1) // (256 * n_partial) + 6 + 2 + n_partial + 1


def layout_reduce_blocks(p):
    return {"x": Buf(F32, p.nblk, p.inner, p.inner), "out": Buf(F32, 1, p.inner, 0, "out")}


def ref_reduce_blocks(p, v):
    x, sc = f64(v["x"]), _f32(p.scale)
    return {"out": expect(sc * x.sum(0, keepdim=True), blocks_chain(p.nblk) * U32 * abs(sc) * x.abs().sum(0, keepdim=True), F32)}


def layout_colsum(p):
    L = {"x": Buf(F16, p.rows, p.cols, p.ldx), "out": Buf(F32, 1, p.cols, 0, "out")}
    if _ptr(p, "partial"):                                   # the per-block sums: their order is documented, their contents are not an output
        L["partial"] = Buf(F32, p.nblk, p.cols, p.cols, "scratch")
    return L


def ref_colsum(p, v):
    """Block b sums the rows [b rpb, (b + 1) rpb) in order, rpb = ceil(rows / nblk) (a block past the last row holds 0); then pv_reduce_blocks' order."""
    x = f64(v["x"])
    chain = (p.rows + p.nblk - 1) // p.nblk + blocks_chain(p.nblk)
    return {"out": expect(x.sum(0, keepdim=True), chain * U32 * x.abs().sum(0, keepdim=True), F32)}


def _reduce_scalar(terms, eterm, chain, scale):
    """scale Sum terms with a per-term relative rounding ``eterm`` (in U32) and the fp32 rounding of the scale itself -> Expect [1, 1]."""
    mag = terms.abs().sum().reshape(1, 1)
    return expect(scale * terms.sum().reshape(1, 1), (chain + eterm + 1) * U32 * abs(scale) * mag, F32)


def layout_reduce_mean(p):
    dt = F16 if p.is_f16 else F32
    L = {"a": Buf(dt, 1, p.n, 0), "out": Buf(F32, 1, 1, 0, "out")}
    if _ptr(p, "partial"):
        L["partial"] = Buf(F32, 1, p.n_partial, 0, "scratch")
    if p.mode == 2:
        L["b"] = Buf(dt, 1, p.n, 0)
    return L


def ref_reduce_mean(p, v):
    """mode 0 mean(a), 1 mean|a|, 2 mean((a - b)^2); the scale is the fp32 1 / n (one more rounding)."""
    a = f64(v["a"])
    if p.mode == 2:
        terms, et = (a - f64(v["b"])) ** 2, 3 + 1           # the difference enters squared: twice its rounding, and the product's
    else:
        terms, et = (a.abs() if p.mode == 1 else a), 1
    return {"out": _reduce_scalar(terms, et, mean_chain(p.n, p.n_partial), 1.0 / p.n)}


def layout_reduce_sumsq(p):
    L = {"a": Buf(F32, 1, p.n, 0), "out": Buf(F32, 1, 1, 0, "out")}
    if _ptr(p, "partial"):
        L["partial"] = Buf(F32, 1, p.n_partial, 0, "scratch")
    return L


def ref_reduce_sumsq(p, v):
    return {"out": _reduce_scalar(f64(v["a"]) ** 2, 1, mean_chain(p.n, p.n_partial), _f32(p.scale))}


def wgrad_cap(m: int) -> float:
    """tests/test_hip_kernels.py::test_wgrad_tn's tolerance."""
    return 2e-6 * max(1.0, math.sqrt(m / 64.0))


def layout_wgrad(p):
    return {"dy": Buf(F16, p.m, p.n, p.lddy), "x": Buf(F16, p.m, p.k, p.ldx), "out": Buf(F32, p.nsplit, p.n * p.k, p.n * p.k, "out")}


def ref_wgrad(p, v):
    """Slab s = dy[rows]^T x[rows] over the rows [s rps, min(m, (s + 1) rps)): an MFMA chain of at most rps products per element."""
    dy, x = f64(v["dy"]), f64(v["x"])
    ref, det = [], []
    for s in range(p.nsplit):
        r = slice(s * p.rows_per_split, min(p.m, (s + 1) * p.rows_per_split))
        ref.append((dy[r].T @ x[r]).reshape(-1))
        det.append(mfma_c(p.rows_per_split) * (dy[r].abs().T @ x[r].abs()).reshape(-1))
    return {"out": expect(torch.stack(ref), torch.stack(det), F32, cap=wgrad_cap(p.m))}


# ===================================================================================================================== the identity loss
GRAY = (0.2989, 0.5870, 0.1140)


def gray_taps(n_in: int, n_out: int, device):
    """One axis of pv_gray_resize as matrices [n_out, n_in]: C, the bilinear weights of ``bilinear_taps`` (src = max((o + 0.5) in / out - 0.5, 0), i0 =
    floor, i1 = min(i0 + 1, in - 1), weights 1 - t and t - summed where i1 == i0), and E, the bound of |C' - C| for the weights C' of a kernel that
    evaluates src in fp32 as the header writes it: the ratio, the product and the difference round (3 U32 of (o + 0.5) in / out + 0.5), and every weight
    is a hat function of src with slope 1 - continuous over the integer tap boundaries, where the fp32 floor may fall on the other side: the weight that
    moves to the neighbouring tap is itself below that error.  E holds the error at the taps i0 - 1 .. i0 + 2, the only ones either side can touch."""
    i0, i1, t = bilinear_taps(n_in, n_out, device)
    o = torch.arange(n_out, device=device)
    Cm = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    Cm[o, i0] += 1 - t
    Cm[o, i1] += t
    es = U32 * (3 * (o.double() + 0.5) * n_in / n_out + 0.5) + U32             # and the weight's own rounding
    Em = torch.zeros_like(Cm)
    for d in (-1, 0, 1, 2):
        Em[o, (i0 + d).clamp(0, n_in - 1)] = es
    return Cm, Em


def layout_gray_resize(p):
    return {"x": Buf(F32, p.batch, 3 * p.h * p.w, p.x_image_stride), "y": Buf(F32, 1, p.batch * p.size * p.size, 0, "out")}


def ref_gray_resize(p, v):
    """y = mul bilinear(0.2989 r + 0.5870 g + 0.1140 b) + add.  |C'y G C'x^T - Cy G Cx^T| <= (Cy + Ey) |G| (Cx + Ex)^T - Cy |G| Cx^T for the tap
    boundaries (``gray_taps``); roundings: the gray value (three fp32 constants, three products, two sums: 8 U32), the two mixes (10), mul and add (2)."""
    x = f64(v["x"]).reshape(p.batch, 3, p.h, p.w)
    g = GRAY[0] * x[:, 0] + GRAY[1] * x[:, 1] + GRAY[2] * x[:, 2]
    ga = GRAY[0] * x[:, 0].abs() + GRAY[1] * x[:, 1].abs() + GRAY[2] * x[:, 2].abs()
    Cy, Ey = gray_taps(p.h, p.size, x.device)
    Cx, Ex = gray_taps(p.w, p.size, x.device)
    mul, add = _f32(p.mul), _f32(p.add)
    r = Cy @ g @ Cx.T
    mag = Cy @ ga @ Cx.T
    tap = (Cy + Ey) @ ga @ (Cx + Ex).T - mag
    det = abs(mul) * (tap + 18 * U32 * mag) + 2 * U32 * (abs(mul) * mag + abs(add))
    return {"y": expect((mul * r + add).reshape(1, -1), det.reshape(1, -1), F32, cap=CAP["gray"])}


def layout_gray_resize_backward(p):
    return {"dy": Buf(F32, p.batch, p.size * p.size, p.dy_image_stride), "dx": Buf(F32, 1, p.batch * 3 * p.h * p.w, 0, "out")}


def ref_gray_resize_backward(p, v):
    """dx[b][ch] = GRAY[ch] mul Cy^T dy[b] Cx: a gather per input pixel over the outputs whose taps include it - at most ny nx of them, ny / nx the
    largest number of outputs one input row / column reaches: the chain; each term two products; then mul and the channel weight."""
    dy = f64(v["dy"]).reshape(p.batch, p.size, p.size)
    Cy, Ey = gray_taps(p.h, p.size, dy.device)
    Cx, Ex = gray_taps(p.w, p.size, dy.device)
    mul = _f32(p.mul)
    acc = Cy.T @ dy @ Cx
    mag = Cy.T @ dy.abs() @ Cx
    tap = (Cy + Ey).T @ dy.abs() @ (Cx + Ex) - mag
    chain = int(((Cy + Ey) > 0).sum(0).max().item() * ((Cx + Ex) > 0).sum(0).max().item())
    det = abs(mul) * (tap + (chain + 6) * U32 * mag)
    w = torch.tensor(GRAY, dtype=torch.float64, device=dy.device).view(1, 3, 1, 1)
    return {"dx": expect((w * (mul * acc).unsqueeze(1)).reshape(1, -1), (w * det.unsqueeze(1)).reshape(1, -1), F32, cap=CAP["gray"])}


COS_EPS = 1e-8


def cosine_parts(p, v):
    """(cos, its error bound, the sums) of pv_cosine_embedding_loss: cos = ab / sqrt((aa + eps)(cc + eps)), eps = 1e-8; each sum: 64 lanes of
    ceil(dim / 64) terms, a 6-level tree."""
    a, c = f64(v["e1"]), f64(v["e2"])
    ab, aa, cc = (a * c).sum(1, keepdim=True), (a * a).sum(1, keepdim=True) + COS_EPS, (c * c).sum(1, keepdim=True) + COS_EPS
    chain = (p.dim + 63) // 64 + 6 + 1
    den = torch.sqrt(aa * cc)
    cos = ab / den
    rden = (chain + 4) * U32                              # half of each sum's relative error, the product, the root
    ecos = chain * U32 * (a * c).abs().sum(1, keepdim=True) / den + cos.abs() * (rden + 4 * U32)
    return a, c, ab, aa, cc, den, cos, ecos, chain, rden


def layout_cosine_loss(p):
    L = {"e1": Buf(F16, p.batch, p.dim, p.dim), "e2": Buf(F16, p.batch, p.dim, p.dim), "per_sample": Buf(F32, 1, p.batch, 0, "out")}
    if _ptr(p, "de2"):
        L["de2"] = Buf(F16, p.batch, p.dim, p.dim, "out")
    return L


def cosine_ambiguous(p, v):
    """Samples whose max(0, cos) branch the fp32 cosine may take on the other side (target <= 0, |cos| within its error)."""
    cos, ecos = cosine_parts(p, v)[6:8]
    return (cos.abs() <= ecos) if _f32(p.target) <= 0 else torch.zeros_like(cos, dtype=torch.bool)


def ref_cosine_loss(p, v):
    """target > 0: 1 - cos; else max(0, cos).  de2 = gscale / batch dloss/dcos (a / den - cos c / (cc + eps)).  A sample whose cosine lies within its own
    error of 0 may take either branch of the max: its bounds are widened by the branch difference (|cos|, and the whole gradient)."""
    a, c, ab, aa, cc, den, cos, ecos, chain, rden = cosine_parts(p, v)
    pos = _f32(p.target) > 0
    amb = cosine_ambiguous(p, v)
    loss = 1 - cos if pos else cos.clamp_min(0)
    eloss = ecos + U32 * (1 + cos.abs()) + amb * cos.abs()
    res = {"per_sample": expect(loss.reshape(1, -1), eloss.reshape(1, -1), F32)}
    if "de2" in v:
        k = _f32(p.gscale) / p.batch
        dcos = -torch.ones_like(cos) if pos else (cos > 0).double()
        t1, t2 = a / den, cos * c / cc
        # a / den carries den's relative error; cos c / cc the cosine's error and the sum's; four divisions / products and the difference round
        e = t1.abs() * rden + ecos * (c / cc).abs() + t2.abs() * chain * U32 + 8 * U32 * (t1.abs() + t2.abs())
        grad = k * dcos * (t1 - t2)
        wide = amb * abs(k) * (t1 - t2).abs()
        res["de2"] = expect(grad, abs(k) * dcos.abs() * e + 2 * U32 * grad.abs() + wide, F16, cap=CAP["pointwise_bwd"])
    return res


# ===================================================================================================================== LayerNorm backward
def ln_bwd_chain(cols: int) -> int:
    """Longest fp32 chain of a row sum of pv_layernorm_backward: a lane adds at most 48 of the row's elements (8 x 6 chunks of the widest vector form; 32
    in the one-wave-per-row form at 2048 columns), then a tree of at most 6 levels."""
    return min(cols, 48) + 6


def layout_layernorm_backward(p):
    grp = max(p.dy_group, 1)
    rpw = max(p.rows_per_wave, 1)
    L = {"x": Buf(F16, p.rows, p.cols, p.ldx), "dy": Buf(F16, (p.rows - 1) // grp + 1, p.cols, p.lddy), "dx": Buf(F16, p.rows, p.cols, p.lddx, "out"),
         "gamma": Buf(F32, 1, p.cols, 0), "beta": Buf(F32, 1, p.cols, 0)}
    if _ptr(p, "dgb_partial"):
        L["dgb_partial"] = Buf(F32, (p.rows + 4 * rpw - 1) // (4 * rpw), 2 * p.cols, 2 * p.cols, "out")
    if _ptr(p, "add"):
        L["add"] = Buf(F16, p.rows, p.cols, p.ldadd)
    return L


def ln_bwd_terms(p, v):
    """The fp64 quantities of the LayerNorm (+ LeakyReLU) backward and the elements whose LeakyReLU branch fp32 may decide the other way."""
    if p.act not in (0, 3):
        raise ValueError(f"pv_layernorm_backward: activation {p.act} (the header: LeakyReLU or none)")
    x = f64(v["x"])
    rows, cols = x.shape
    L = ln_bwd_chain(cols)
    grp = max(p.dy_group, 1)
    r = torch.arange(rows, device=x.device)
    dys = torch.where((r % grp < p.dy_skip) if p.dy_group > 1 else torch.zeros_like(r, dtype=torch.bool), 0.0, _f32(p.dy_scale)).double()[:, None]
    g0 = f64(v["dy"])[r // grp] * dys
    gam, bet = f64(v["gamma"]).reshape(1, -1), f64(v["beta"]).reshape(1, -1)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(p.eps))
    xh = (x - mean) * rstd
    # mean: a chain of L on Sum|x| / cols and the division; rstd: half the variance's chain and the squares' roundings, rsqrt's ulp
    em = (L + 1) * U32 * x.abs().mean(1, keepdim=True)
    r_rstd = (L / 2 + 6) * U32
    exh = rstd * (em + U32 * (x.abs() + mean.abs())) + xh.abs() * (r_rstd + U32)
    z = gam * xh + bet
    ez = gam.abs() * exh + 2 * U32 * ((gam * xh).abs() + bet.abs())
    leaky = p.act == 3
    amb = (z.abs() <= ez) if leaky else torch.zeros_like(z, dtype=torch.bool)
    g = torch.where(z < 0, 0.01 * g0, g0) if leaky else g0
    return dict(x=x, L=L, g0=g0, g=g, gam=gam, rstd=rstd, xh=xh, exh=exh, r_rstd=r_rstd, amb=amb)


def ref_layernorm_backward(p, v):
    """y = act(gamma xhat + beta), g = dy[r / dy_group] dy_scale act'(z) (0 on the first dy_skip rows of a group), dxhat = g gamma:
        dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) (+ add);   dgb_partial[block] = (Sum g xhat, Sum g) over the block's 4 rows_per_wave rows.
    An element whose pre-activation lies within its own fp32 error of 0 may take either LeakyReLU branch: its g moves by 0.99 |g0|, which reaches the
    element itself, both row means (every element of its row) and its column of the block's partial sums - all widened by exactly that."""
    t = ln_bwd_terms(p, v)
    x, L, g, gam, rstd, xh, exh, r_rstd = t["x"], t["L"], t["g"], t["gam"], t["rstd"], t["xh"], t["exh"], t["r_rstd"]
    rows, cols = x.shape
    dxh = g * gam
    edxh = 3 * U32 * dxh.abs()                               # dy dy_scale, the slope, gamma
    s1, s2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    e1 = (L + 1) * U32 * dxh.abs().mean(1, keepdim=True) + edxh.mean(1, keepdim=True)
    e2 = (L + 2) * U32 * (dxh * xh).abs().mean(1, keepdim=True) + (dxh.abs() * exh + edxh * xh.abs()).mean(1, keepdim=True)
    core = rstd * (dxh - s1 - xh * s2)
    D = 0.99 * (t["g0"] * gam).abs() * t["amb"]
    wide = rstd * (D + D.mean(1, keepdim=True) + xh.abs() * (D * xh.abs()).mean(1, keepdim=True))
    err = rstd * (edxh + e1 + exh * s2.abs() + xh.abs() * e2 + 3 * U32 * (dxh.abs() + s1.abs() + (xh * s2).abs())) + core.abs() * (r_rstd + U32) + wide
    ref = core
    if "add" in v:
        ref = core + f64(v["add"])
        err = err + U32 * (core.abs() + f64(v["add"]).abs())
    res = {"dx": expect(ref, err, F16, cap=CAP["ln_bwd_dx"])}
    if "dgb_partial" in v:
        rpw = max(p.rows_per_wave, 1)
        blk = 4 * rpw
        nb = (rows + blk - 1) // blk

        def per_block(q):
            return torch.cat([q, torch.zeros(nb * blk - rows, cols, dtype=torch.float64, device=x.device)]).reshape(nb, blk, cols).sum(1)
        Dg = 0.99 * t["g0"].abs() * t["amb"]
        dg, db = per_block(g * xh), per_block(g)
        edg = (rpw + 4 + 2) * U32 * per_block((g * xh).abs()) + per_block(g.abs() * exh + Dg * xh.abs())
        edb = (rpw + 4 + 1) * U32 * per_block(g.abs()) + per_block(Dg)
        res["dgb_partial"] = expect(torch.cat([dg, db], 1), torch.cat([edg, edb], 1), F32, cap=CAP["ln_bwd_dgb"])
    return res


# ===================================================================================================================== tables
#: positional argument names of the launchers that take no parameter struct (``_lib.SIGNATURES`` order, stream excluded)
ARGS = {
    "pv_xattn_pack_kv": ("kt", "vt", "ldkt", "ldvt", "kip", "vip", "ldkip", "ldvip", "kimg", "vimg", "vnorm", "batch", "heads", "d", "nt", "nip"),
    "pv_im2col3x3": ("x", "out", "batch", "cin", "h", "wd", "kpad"),
    "pv_conv_out": ("x", "w", "bias", "out", "batch", "cin", "h", "wd", "cout"),
    "pv_timestep_embedding": ("timesteps", "state", "rows", "dim", "out"),
    "pv_cfg_dpm_step": ("eps_uncond", "eps_cond", "latents", "x0_prev", "coef", "state", "guidance", "n"),
    "pv_cfg_dpm_step_masked": ("eps_uncond", "eps_cond", "latents", "x0_prev", "coef", "state", "guidance", "mask", "known", "noise", "channels", "hw", "n"),
    "pv_step_advance": ("state",),
    "pv_pointwise_nchw": ("x", "w", "bias", "out", "batch", "cin", "cout", "hw"),
    "pv_softmax_rows": ("x", "ld", "rows", "cols", "scale"),
    "pv_posterior_sample": ("moments", "eps", "out", "batch", "chw"),
    "pv_groupnorm_scale_shift": ("table",),       # after the struct
    "pv_cfg_dpm_step_guided": ("eps_uncond", "eps_image", "eps_cond", "latents", "x0_prev", "coef", "state", "g_text", "g_image", "rescale", "mask", "known",
                               "noise", "batch", "channels", "hw"),
    "pv_cfg_dpm_step_stochastic": ("eps_uncond", "eps_image", "eps_cond", "latents", "x0_prev", "coef", "state", "rng", "g_text", "g_image", "rescale", "mask",
                                   "known", "noise", "batch", "channels", "hw"),
    "pv_cfg_dpm_step_pag": ("eps_uncond", "eps_image", "eps_cond", "eps_perturbed", "latents", "x0_prev", "coef", "state", "rng", "g_text", "g_image", "g_pag",
                            "rescale", "mask", "known", "noise", "batch", "channels", "hw"),
    "pv_fusion_draw": ("state", "rng", "forced", "out", "n_layers", "rule1", "rule2", "scale", "only_last_step"),
    "pv_freeu_rows": ("x", "ldx", "cx", "x_out", "ldxo", "b", "skip", "lds", "cs", "skip_out", "ldso", "s", "batch", "h", "w"),
    "pv_resize_bilinear_affine_f32": ("x", "y", "ca", "cb", "out", "batch", "channels", "h", "w", "oh", "ow"),
    "pv_affine_rows_f32": ("x", "y", "ca", "cb", "out", "per_sample", "batch"),
    "pv_composite_clamp_f32": ("gen", "orig", "mask", "out", "lo", "hi", "batch", "channels", "hw"),
    "pv_clamp_f32": ("x", "lo", "hi", "n"),
    "pv_rows_mean": ("x", "ldx", "y", "ldy", "groups", "count", "group_rows", "cols", "accumulate"),
    "pv_cast_f32_to_f16": ("x", "y", "n"),
    "pv_cast_f16_to_f32": ("x", "y", "n"),
    "pv_patchify": ("x", "out", "batch", "ch", "img", "patch", "kpad"),
    "pv_clip_vision_embed": ("patches", "cls", "pos", "out", "batch", "ntok", "dim"),
    "pv_clip_text_embed": ("ids", "tok", "pos", "concept", "placeholder_idx", "n_concept", "out", "batch", "seq", "dim"),
    # the training tape
    "pv_act_forward": ("x", "ldx", "y", "ldy", "rows", "cols", "act"),
    "pv_act_backward": ("x", "ldx", "dy", "lddy", "dx", "lddx", "rows", "cols", "act"),
    "pv_geglu": ("x", "ldx", "out", "ldo", "rows", "n"),
    "pv_geglu_backward": ("h", "ldh", "dy", "lddy", "dh", "lddh", "rows", "n"),
    "pv_col_affine_f16": ("x", "ldx", "scale", "shift", "y", "ldy", "rows", "cols"),
    "pv_prelu_f16": ("x", "ldx", "dy", "lddy", "slope", "out", "ldo", "rows", "cols"),
    "pv_add_rows_f16": ("a", "lda", "b", "ldb", "out", "ldo", "rows", "cols"),
    "pv_dropout_f16": ("x", "ldx", "out", "ldo", "add", "ldadd", "rows", "cols", "copies", "p", "rng", "site", "backward"),
    "pv_softmax_rows_backward": ("p", "ldp", "dp", "lddp", "rows", "cols", "scale"),
    "pv_transpose_f16": ("x", "ldx", "rows", "cols", "out", "ldo", "rows_pad"),
    "pv_dilate2x": ("x", "ldx", "z", "batch", "h", "w", "c"),
    "pv_pool2x_sum": ("g", "add", "ldadd", "out", "batch", "h", "w", "c"),
    "pv_maxpool2x2": ("x", "dy", "out", "batch", "h", "w", "c"),
    "pv_sign_f32": ("x", "coef", "out", "n"),
    "pv_clamp_mask_f32": ("y", "dy", "lo", "hi", "out", "n"),
    "pv_gather_rows_f32": ("x", "ldx", "idx", "out", "batch", "seq", "n_e", "dim", "scale"),
    "pv_reduce_blocks": ("x", "nblk", "inner", "scale", "out"),
    "pv_colsum_f16": ("x", "ldx", "rows", "cols", "partial", "nblk", "out"),
    "pv_reduce_mean": ("a", "b", "mode", "is_f16", "n", "partial", "n_partial", "out"),
    "pv_reduce_sumsq": ("a", "n", "scale", "partial", "n_partial", "out"),
    "pv_wgrad_tn": ("dy", "lddy", "x", "ldx", "m", "n", "k", "out", "nsplit", "rows_per_split"),
    "pv_gray_resize": ("x", "x_image_stride", "y", "batch", "h", "w", "size", "mul", "add"),
    "pv_gray_resize_backward": ("dy", "dy_image_stride", "dx", "batch", "h", "w", "size", "mul"),
    "pv_cosine_embedding_loss": ("e1", "e2", "batch", "dim", "target", "gscale", "per_sample", "de2"),
}

#: the training tape's single launches (tests/test_abi_ref_cpu.py: none of them may leave ``REF`` again): launcher -> (layout, reference, helpers)
TRAINING = {
    "pv_act_forward": (layout_act_forward, ref_act_forward), "pv_act_backward": (layout_act_backward, ref_act_backward),
    "pv_geglu": (layout_geglu, ref_geglu), "pv_geglu_backward": (layout_geglu_backward, ref_geglu_backward),
    "pv_col_affine_f16": (layout_col_affine, ref_col_affine), "pv_prelu_f16": (layout_prelu, ref_prelu),
    "pv_add_rows_f16": (layout_add_rows, ref_add_rows), "pv_dropout_f16": (layout_dropout, ref_dropout),
    "pv_softmax_rows_backward": (layout_softmax_rows_backward, ref_softmax_rows_backward), "pv_transpose_f16": (layout_transpose, ref_transpose),
    "pv_dilate2x": (layout_dilate, ref_dilate), "pv_pool2x_sum": (layout_pool2x, ref_pool2x), "pv_maxpool2x2": (layout_maxpool, ref_maxpool),
    "pv_sign_f32": (layout_sign, ref_sign), "pv_clamp_mask_f32": (layout_clamp_mask, ref_clamp_mask),
    "pv_gather_rows_f32": (layout_gather_rows, ref_gather_rows), "pv_reduce_blocks": (layout_reduce_blocks, ref_reduce_blocks),
    "pv_colsum_f16": (layout_colsum, ref_colsum), "pv_reduce_mean": (layout_reduce_mean, ref_reduce_mean),
    "pv_reduce_sumsq": (layout_reduce_sumsq, ref_reduce_sumsq), "pv_wgrad_tn": (layout_wgrad, ref_wgrad),
    "pv_gray_resize": (layout_gray_resize, ref_gray_resize), "pv_gray_resize_backward": (layout_gray_resize_backward, ref_gray_resize_backward),
    "pv_cosine_embedding_loss": (layout_cosine_loss, ref_cosine_loss, cosine_parts),
    "pv_layernorm_backward": (layout_layernorm_backward, ref_layernorm_backward, ln_bwd_terms),
}

LAYOUT = {
    **{n: f[0] for n, f in TRAINING.items()},
    "pv_gemm_conv": layout_gemm, "pv_attention": layout_attention, "pv_cross_attention": layout_xattn,
    "pv_cross_attention_lnq": layout_xattn_lnq, "pv_cross_attention_fused": layout_xattn_fused, "pv_xattn_pack_kv": layout_pack_kv,
    "pv_row_gemm": layout_row_gemm, "pv_layernorm": layout_layernorm, "pv_groupnorm_stats": layout_gn_stats,
    "pv_groupnorm_stats_from_colstats": layout_gn_stats, "pv_groupnorm_scale_shift": layout_gn_scale_shift, "pv_groupnorm_apply": layout_gn_apply,
    "pv_im2col3x3": layout_im2col, "pv_conv_out": layout_conv_out, "pv_timestep_embedding": layout_timestep, "pv_cfg_dpm_step": layout_cfg,
    "pv_step_advance": layout_step_advance, "pv_pointwise_nchw": layout_pointwise, "pv_softmax_rows": layout_softmax_rows,
    "pv_posterior_sample": layout_posterior, "pv_cfg_dpm_step_masked": layout_cfg_masked,
    "pv_cfg_dpm_step_guided": layout_step, "pv_cfg_dpm_step_stochastic": layout_step, "pv_cfg_dpm_step_pag": layout_step, "pv_fusion_draw": layout_fusion_draw,
    "pv_freeu_rows": layout_freeu, "pv_resize_bilinear_affine_f32": layout_resize, "pv_affine_rows_f32": layout_affine_rows,
    "pv_composite_clamp_f32": layout_composite, "pv_clamp_f32": layout_clamp, "pv_rows_mean": layout_rows_mean, "pv_cast_f32_to_f16": layout_cast_to_f16,
    "pv_cast_f16_to_f32": layout_cast_to_f32, "pv_patchify": layout_patchify, "pv_clip_vision_embed": layout_vision_embed,
    "pv_clip_text_embed": layout_text_embed,
}

REF = {
    **{n: f[1] for n, f in TRAINING.items()},
    "pv_gemm_conv": ref_gemm, "pv_attention": ref_attention, "pv_cross_attention": ref_xattn, "pv_cross_attention_lnq": ref_xattn_lnq,
    "pv_cross_attention_fused": ref_xattn_fused, "pv_xattn_pack_kv": ref_pack_kv, "pv_row_gemm": ref_row_gemm, "pv_layernorm": ref_layernorm,
    "pv_groupnorm_stats": ref_gn_stats, "pv_groupnorm_stats_from_colstats": ref_gn_stats, "pv_groupnorm_scale_shift": ref_gn_scale_shift,
    "pv_groupnorm_apply": ref_gn_apply, "pv_im2col3x3": ref_im2col, "pv_conv_out": ref_conv_out, "pv_timestep_embedding": ref_timestep,
    "pv_cfg_dpm_step": ref_cfg, "pv_step_advance": ref_step_advance, "pv_pointwise_nchw": ref_pointwise, "pv_softmax_rows": ref_softmax_rows,
    "pv_posterior_sample": ref_posterior, "pv_cfg_dpm_step_masked": ref_cfg_masked,
    "pv_cfg_dpm_step_guided": ref_step, "pv_cfg_dpm_step_stochastic": ref_step, "pv_cfg_dpm_step_pag": ref_step, "pv_fusion_draw": ref_fusion_draw,
    "pv_freeu_rows": ref_freeu, "pv_resize_bilinear_affine_f32": ref_resize, "pv_affine_rows_f32": ref_affine_rows, "pv_composite_clamp_f32": ref_composite,
    "pv_clamp_f32": ref_clamp, "pv_rows_mean": ref_rows_mean, "pv_cast_f32_to_f16": ref_cast_to_f16, "pv_cast_f16_to_f32": ref_cast_to_f32,
    "pv_patchify": ref_patchify, "pv_clip_vision_embed": ref_vision_embed, "pv_clip_text_embed": ref_text_embed,
}


def _coef_rows(p, state):
    return Buf(F32, 1, (step_index(state) + 1) * 8, 0)


#: launchers with a buffer whose extent depends on the CONTENTS of another (device-resident) buffer: launcher -> (the buffer read first, the dependent
#: buffer, extent(p, first view) -> Buf, the width of the row the reference is handed - 0: the whole buffer).  The step launchers index the coefficient
#: table with the clamped step index of ``state``; the text embedding gathers rows of ``tok`` by ``ids`` (the vocabulary size is no argument).
DEPENDENT = {
    "pv_timestep_embedding": ("state", "timesteps", lambda p, s: Buf(F32, 1, step_index(s) + 1, 0), 0),
    **{n: ("state", "coef", _coef_rows, 8) for n in ("pv_cfg_dpm_step", "pv_cfg_dpm_step_masked", "pv_cfg_dpm_step_guided", "pv_cfg_dpm_step_stochastic",
                                                     "pv_cfg_dpm_step_pag")},
    "pv_clip_text_embed": ("ids", "tok", lambda p, ids: Buf(F32, int(ids.max().item()) + 1, p.dim, p.dim), 0),
}

_QUERY = "a host-side query: launches nothing"
_TABLE = ("its operands are reached through a device table of pointers (%s), which the Auditor cannot resolve to held tensors yet; "
          "tests/test_hip_kernels.py tests it directly (%s)")
#: every other symbol of ``photoverse_amd._lib.SIGNATURES``: deliberately outside the launch audit, and why.  A launcher is in exactly one of REF and
#: this table (tests/test_abi_ref_cpu.py); nothing a plan of ``run_inference`` / ``generate.py`` can record may be listed here.
NOT_AUDITED = {
    "pv_abi_version": _QUERY, "pv_device_count": _QUERY, "pv_xattn_fused_wo_slot": _QUERY,
    "pv_gemm_conv_kernel_info": _QUERY + " (the dispatch rule the edge catalogue asks)", "pv_attention_kernel_info": _QUERY + " (the dispatch rule the edge catalogue asks)",
    "pv_attention_backward": "a multi-kernel MFMA backward pass (the delta pass, dq, dk / dv): the bounds of its fp16 P / dS intermediates through three "
                             "products need their own derivation - the next slice of the training audit",
    "pv_cross_attention_backward": "a multi-kernel MFMA backward pass (dq, the dK / dV partials per 512-query chunk, their ordered reduce) over two "
                                   "softmaxes and the to_v_ip_norm gradient: its bounds need their own derivation - the next slice of the training audit",
    "pv_groupnorm_backward": "three kernels (partial sums, their reduce, the apply pass) whose group sums cancel: the bound of (dxhat - m1 - xhat m2) over "
                             "hw x C/G terms needs its own derivation - the next slice of the training audit",
    "pv_pack_weights": _TABLE % ("entries: int64 [E][9] with src / dst / dstT addresses", "test_pack_weights_multi"),
    "pv_sumsq_multi": _TABLE % ("entries: int64 [T][6] with the gradient addresses", "the multi-tensor optimizer tests"),
    "pv_clip_coef_groups": "reads the partial sums pv_sumsq_multi wrote for a pointer table and updates the overflow counters in place: audited with "
                           "pv_sumsq_multi once the Auditor resolves pointer tables; the multi-tensor optimizer tests cover it",
    "pv_adamw_multi": _TABLE % ("entries: int64 [T][6] with parameter, gradient and moment addresses, updated in place", "the multi-tensor optimizer tests"),
}

#: struct fields no layout / reference reads, and why.  Every other field of an audited struct is read by its layout or its reference
#: (``fields_read``); a field in neither fails ``test_abi_ref_cpu.py``'s coverage test until it is modelled or listed here.
DISPATCH_ONLY = {
    "GemmParams": {"big_tile_min": "dispatch: the minimum tile count of the 256-row-tile kernel; every kernel computes the same product",
                   "splitk_ws": "scratch: the fp32 partial slabs of a split-K launch, reduced in fixed order"},
    "XAttnFusedParams": {"rows_per_workgroup": "dispatch: 64- or 128-row workgroups, the same results (ABI 13)"},
}

#: per ctypes struct (``photoverse_amd._lib``): the functions of this module that read its fields
STRUCT_FUNCS = {
    "GemmParams": (layout_gemm, ref_gemm, gemm_geometry),
    "AttnParams": (layout_attention, ref_attention),
    "XAttnParams": (layout_xattn, ref_xattn, _fusion),
    "XAttnLnqParams": (layout_xattn_lnq, ref_xattn_lnq, q_stage, _fusion),
    "XAttnFusedParams": (layout_xattn_fused, ref_xattn_fused, q_stage, _fusion),
    "RowGemmParams": (layout_row_gemm, ref_row_gemm),
    "LayerNormParams": (layout_layernorm, ref_layernorm),
    "GroupNormParams": (layout_groupnorm, layout_gn_stats, layout_gn_scale_shift, layout_gn_apply, group_stats, ref_gn_stats, ref_gn_scale_shift,
                        ref_gn_apply),
    "LayerNormBwdParams": TRAINING["pv_layernorm_backward"],
}


#: per argument-list launcher (``ARGS``) added with the guided / conditioning audit: the functions that read its arguments
ARG_FUNCS = {
    **{n: (layout_step, ref_step, step_reads) for n in ("pv_cfg_dpm_step_guided", "pv_cfg_dpm_step_stochastic", "pv_cfg_dpm_step_pag")},
    "pv_fusion_draw": (layout_fusion_draw, ref_fusion_draw), "pv_freeu_rows": (layout_freeu, ref_freeu),
    "pv_resize_bilinear_affine_f32": (layout_resize, ref_resize), "pv_affine_rows_f32": (layout_affine_rows, ref_affine_rows),
    "pv_composite_clamp_f32": (layout_composite, ref_composite), "pv_clamp_f32": (layout_clamp, ref_clamp), "pv_rows_mean": (layout_rows_mean, ref_rows_mean),
    "pv_cast_f32_to_f16": (layout_cast_to_f16, ref_cast_to_f16), "pv_cast_f16_to_f32": (layout_cast_to_f32, ref_cast_to_f32),
    "pv_patchify": (layout_patchify, ref_patchify), "pv_clip_vision_embed": (layout_vision_embed, ref_vision_embed),
    "pv_clip_text_embed": (layout_text_embed, ref_text_embed),
    **{n: f for n, f in TRAINING.items() if n in ARGS},
}


def _names_read(fns) -> set:
    import inspect
    import re
    names = set()
    for fn in fns:
        for line in inspect.getsource(fn).splitlines():
            if '"scratch"' in line:
                continue
            names |= set(re.findall(r"\bp\.(\w+)", line)) | set(re.findall(r'"(\w+)": (?:Buf\(|None)', line)) | set(re.findall(r'L\["(\w+)"\]', line))
            names |= set(re.findall(r"(\w+)=Buf\(", line)) | set(re.findall(r'"(\w+)" in v', line)) | set(re.findall(r'v\["(\w+)"\]', line))
            names |= set(re.findall(r'(?:getattr|_opt|_ptr)\(p, "(\w+)"', line))
    return names


def args_read(launcher: str, funcs=None) -> set:
    """``fields_read`` for a launcher that takes positional arguments: the names of ``ARGS[launcher]`` its layout / reference functions mention
    (the same tripwire: an argument added to the ABI and to ``ARGS`` that nobody models is in ``ARGS`` and not here)."""
    return _names_read(ARG_FUNCS[launcher] if funcs is None else funcs) & set(ARGS[launcher])


def fields_read(struct: str) -> set:
    """Fields of ``struct`` its layout / reference functions mention: ``p.<field>``, a buffer key ``"<field>": Buf(`` / ``L["<field>"]`` /
    ``<field>=Buf(``, ``v["<field>"]`` or ``"<field>" in v`` - lines that declare a scratch buffer do not count.  A tripwire for fields added
    to the ABI, not a proof that a field's meaning is modelled: that is what the CPU tests against independent formulations check."""
    import inspect
    import re
    names = set()
    for fn in STRUCT_FUNCS[struct]:
        for line in inspect.getsource(fn).splitlines():
            if '"scratch"' in line:
                continue
            names |= set(re.findall(r"\bp\.(\w+)", line)) | set(re.findall(r'"(\w+)": Buf\(', line)) | set(re.findall(r'L\["(\w+)"\]', line))
            names |= set(re.findall(r"(\w+)=Buf\(", line)) | set(re.findall(r'"(\w+)" in v', line)) | set(re.findall(r'v\["(\w+)"\]', line))
    return names
