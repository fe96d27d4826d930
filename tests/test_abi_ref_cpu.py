"""CPU checks of ``oracle.abi_ref`` (the per-launch references of the plan audit) and of the audit's comparator: each reference against an
independent formulation (``F.conv2d`` / ``F.linear`` / ``F.scaled_dot_product_attention``), the comparator against injected defects, and the
field coverage of the ctypes parameter structs."""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import abi_ref as A            # noqa: E402
from oracle import plan_audit as PA        # noqa: E402

D = torch.float64


def close(a, b, tol=1e-9):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = ((a - b).norm() / b.norm()).item()
    assert err < tol, err


def h16(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def gemm_p(**kw):
    from photoverse_amd import _lib
    p = {n: 0 for n, _ in _lib.GemmParams._fields_}
    p.update(taps=1, batch=1, hin=1, win=1, wout=1, stride=1, pad=1, ln_eps=1e-5)
    p.update(kw)
    return SimpleNamespace(**p)


def to_nchw(rows, b, h, w):
    return rows.reshape(b, h, w, -1).permute(0, 3, 1, 2)


def from_nchw(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


# ------------------------------------------------------------------------------------------------------------------ pv_gemm_conv
GEOS = [  # (batch, hin, win, stride, upsample, pad, c0, c1)
    (2, 6, 5, 1, 0, 1, 64, 0),
    (2, 6, 6, 2, 0, 1, 64, 64),       # Downsample2D, dual source
    (1, 8, 6, 2, 0, 0, 64, 0),        # VAE encoder: F.pad(0, 1, 0, 1) + stride 2, padding 0
    (2, 3, 4, 1, 1, 1, 64, 64),       # Upsample2D, dual source
]


@pytest.mark.parametrize("geo", GEOS)
def test_conv_reference_matches_conv2d(geo):
    b, hin, win, stride, up, pad, c0, c1 = geo
    g = torch.Generator().manual_seed(hash(geo) % 1000)
    hl, wl = (hin * 2, win * 2) if up else (hin, win)
    hout, wout = (hl // 2, wl // 2) if stride == 2 else (hl, wl)
    N, M = 128, b * hout * wout
    Ct = c0 + c1
    # strided sources: a0 / a1 are column slices of wider buffers
    src0 = h16(b * hin * win, c0 + 32, g=g)
    src1 = h16(b * hin * win, c1 + 64, g=g) if c1 else None
    a0 = src0[:, 16:16 + c0]
    a1 = src1[:, :c1] if c1 else None
    wt = h16(N, Ct, 3, 3, g=g, scale=0.05)
    wk = wt.permute(0, 2, 3, 1).reshape(N, 9 * Ct).contiguous()          # [Cout][ky][kx][Cin]
    bias = torch.randn(N, generator=g)
    rowadd = torch.randn(b, N + 8, generator=g)[:, 4:4 + N]                # per image, strided
    res = h16(M, N, g=g)
    p = gemm_p(c0=c0, c1=c1, lda0=src0.shape[1], lda1=src1.shape[1] if c1 else 0, M=M, N=N, taps=9, batch=b, hin=hin, win=win, hout=hout,
               wout=wout, stride=stride, upsample=up, pad=pad, act=1, rowadd=1, rowadd_ld=rowadd.stride(0), bias=1, residual=1, ldr=N, ldc=N,
               a1=1 if c1 else 0)
    v = dict(a0=a0, w=wk, bias=bias.reshape(1, -1), rowadd=rowadd, residual=res)
    if c1:
        v["a1"] = a1
    got = A.ref_gemm(p, v)["out"].ref
    x = to_nchw(torch.cat([a0, a1], 1) if c1 else a0, b, hin, win).double()
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if pad == 0:
        x = F.pad(x, (0, 1, 0, 1))
    y = F.conv2d(x, wt.double(), bias.double(), stride=stride, padding=pad)
    y = y + rowadd.double()[:, :, None, None]
    y = F.silu(y)
    exp = from_nchw(y) + res.double()
    close(got, exp)


def test_linear_reference_geglu_and_rowadd_per_image():
    from photoverse_amd.ops import pack_geglu
    g = torch.Generator().manual_seed(3)
    M, K, n = 3 * 40, 128, 128
    x = h16(M, K, g=g)
    w = h16(2 * n, K, g=g, scale=0.1)
    b = torch.randn(2 * n, generator=g)
    wp, bp = pack_geglu(w, b)
    p = gemm_p(c0=K, lda0=K, M=M, N=2 * n, hout=40, geglu=1, ldc=n, bias=1)
    got = A.ref_gemm(p, dict(a0=x, w=wp, bias=bp.reshape(1, -1)))["out"].ref
    h = F.linear(x.double(), w.double(), b.double())
    close(got, h[:, :n] * F.gelu(h[:, n:]))
    # per-image rowadd (3 images of 40 rows) and out_f32 / quick-GELU
    ra = torch.randn(3, 2 * n, generator=g)
    p = gemm_p(c0=K, lda0=K, M=M, N=2 * n, hout=40, ldc=2 * n, rowadd=1, rowadd_ld=2 * n, act=2, out_f32=1)
    got = A.ref_gemm(p, dict(a0=x, w=w, rowadd=ra))["out"].ref
    y = F.linear(x.double(), w.double()) + ra.double().repeat_interleave(40, 0)
    close(got, y * torch.sigmoid(1.702 * y))


def test_layernorm_fold_and_groupnorm_fold():
    g = torch.Generator().manual_seed(4)
    M, K, N = 64, 640, 320
    x = h16(M, K, g=g) * 3 + 1
    w = h16(N, K, g=g, scale=0.05)
    p = gemm_p(c0=K, lda0=K, M=M, N=N, hout=M, ldc=N, ln_rowsum=1, ln_eps=1e-5)
    got = A.ref_gemm(p, dict(a0=x, w=w, ln_rowsum=w.float().sum(1).reshape(1, -1)))["out"].ref
    close(got, F.linear(F.layer_norm(x.double(), (K,), eps=1e-5), w.double()), 1e-7)      # ln_rowsum is an fp32 input
    # GroupNorm + SiLU folded into a dual-source 3x3 conv through a per-(image, channel) scale / shift table
    b, h, wd, c0, c1, N = 2, 4, 4, 64, 64, 128
    a0, a1 = h16(b * h * wd, c0, g=g), h16(b * h * wd, c1, g=g)
    gam, bet = torch.randn(c0 + c1, generator=g), torch.randn(c0 + c1, generator=g)
    xc = to_nchw(torch.cat([a0, a1], 1), b, h, wd).double()
    xg = xc.reshape(b, 32, -1)
    mean, rstd = xg.mean(2), 1 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)
    grp = torch.arange(c0 + c1) // ((c0 + c1) // 32)
    sc = gam.double()[None] * rstd[:, grp]
    sh = bet.double()[None] - mean[:, grp] * sc
    tab = torch.stack([sc, sh], 1).reshape(b, -1)
    wt = h16(N, c0 + c1, 3, 3, g=g, scale=0.05)
    p = gemm_p(c0=c0, c1=c1, lda0=c0, lda1=c1, a1=1, M=b * h * wd, N=N, taps=9, batch=b, hin=h, win=wd, hout=h, wout=wd, ldc=N,
               a_norm=1, a_norm_act=1)
    got = A.ref_gemm(p, dict(a0=a0, a1=a1, w=wt.permute(0, 2, 3, 1).reshape(N, -1).contiguous(), a_norm=tab))["out"].ref
    xn = F.silu(F.group_norm(xc, 32, gam.double(), bet.double(), eps=1e-5)).half().double()
    close(got, from_nchw(F.conv2d(xn, wt.double(), padding=1)), 1e-6)


def test_splitk_is_the_unsplit_product():
    g = torch.Generator().manual_seed(5)
    x, w = h16(200, 256, g=g), h16(128, 256, g=g)
    base = dict(c0=256, lda0=256, M=200, N=128, hout=200, ldc=128)
    r1 = A.ref_gemm(gemm_p(**base), dict(a0=x, w=w))["out"]
    r4 = A.ref_gemm(gemm_p(splitk=4, splitk_ws=1, **base), dict(a0=x, w=w))["out"]
    assert torch.equal(r1.ref, r4.ref) and torch.equal(r1.bound, r4.bound)


# ------------------------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("causal", [False, True])
def test_attention_reference_matches_sdpa(causal):
    g = torch.Generator().manual_seed(6)
    B, H, n, d = 2, 3, 48, 40
    qkv = h16(B * n, 3 * H * d + 8, g=g)
    q, k, v = qkv[:, :H * d], qkv[:, H * d:2 * H * d], qkv[:, 2 * H * d:3 * H * d]
    p = SimpleNamespace(batch=B, heads=H, nq=n, nk=n, d=d, causal=int(causal), lse=1)
    res = A.ref_attention(p, dict(q=q, k=k, v=v, lse=torch.zeros(1)))
    hd = lambda t: t.double().reshape(B, n, H, d).transpose(1, 2)
    exp = F.scaled_dot_product_attention(hd(q), hd(k), hd(v), is_causal=causal).transpose(1, 2).reshape(B * n, H * d)
    close(res["out"].ref, exp)
    s = hd(q) @ hd(k).transpose(2, 3) / math.sqrt(d)
    if causal:
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
    close(res["lse"].ref, (torch.logsumexp(s, 3) / math.log(2)).reshape(B * H, n))


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)
    from photoverse_amd import _lib
    return _lib.load()


def _xattn_case(g, B=2, H=8, d=40, nq=32, nt=77, nip=5):
    C = H * d
    return dict(hs=h16(B * nq, C, g=g), wq=h16(C, C, g=g, scale=0.05), wo=h16(C, C, g=g, scale=0.05), kt=h16(B * nt, C, g=g), vt=h16(B * nt, C, g=g),
                kip=h16(B * nip, C, g=g), vip=h16(B * nip, C, g=g), bias_o=torch.randn(C, generator=g)), (B, H, d, nq, nt, nip)


def _two_sdpa(q, t, dims, wt=1.0, wi=1.0):
    B, H, d, nq, nt, nip = dims
    hd = lambda x, n: x.double().reshape(B, n, H, d).transpose(1, 2)
    o = wt * F.scaled_dot_product_attention(hd(q, nq), hd(t["kt"], nt), hd(t["vt"], nt))
    o = o + wi * F.scaled_dot_product_attention(hd(q, nq), hd(t["kip"], nip), hd(t["vip"], nip))
    return o.transpose(1, 2).reshape(B * nq, H * d)


def test_cross_attention_references_match_two_sdpas(lib):
    g = torch.Generator().manual_seed(7)
    t, dims = _xattn_case(g)
    B, H, d, nq, nt, nip = dims
    C = H * d
    # pv_cross_attention with a device fusion pair overriding (w_text, w_ip); vnorm
    p = SimpleNamespace(batch=B, heads=H, nq=nq, nt=nt, nip=nip, d=d, w_text=1.0, w_ip=1.0)
    q = t["hs"]
    res = A.ref_xattn(p, dict(q=q, kt=t["kt"], vt=t["vt"], kip=t["kip"], vip=t["vip"], vnorm=torch.zeros(1), fusion=torch.tensor([[2.0, 0.0]])))
    close(res["out"].ref, _two_sdpa(q, t, dims, 2.0, 0.0))
    close(res["vnorm"].ref, t["vip"].double().reshape(B, nip, H, d).norm(dim=3).transpose(1, 2).reshape(B * H, nip))
    # pv_cross_attention_lnq: q = to_q(LayerNorm(hs)) with gamma / beta folded (wq' = wq diag(gamma), q_bias = wq . beta)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    wqf = (t["wq"].float() * gam[None]).half()
    qb = t["wq"].float() @ bet
    p = SimpleNamespace(batch=B, heads=H, nq=nq, nt=nt, nip=nip, d=d, w_text=1.0, w_ip=1.0, ln=1, ln_eps=1e-5)
    v = dict(hs=t["hs"], wq=wqf, q_bias=qb.reshape(1, -1), kt=t["kt"], vt=t["vt"], kip=t["kip"], vip=t["vip"])
    qn = F.linear(F.layer_norm(t["hs"].double(), (C,), eps=1e-5), wqf.double(), qb.double())
    close(A.ref_xattn_lnq(p, v)["out"].ref, _two_sdpa(qn, t, dims))
    # pv_cross_attention_fused: + to_out (wo columns in the library's slot order) + bias + residual
    slots = [lib.pv_xattn_fused_wo_slot(s) for s in range(C)]
    assert sorted(slots) == list(range(C))
    wo_packed = t["wo"][:, torch.tensor(slots)].contiguous()
    v = dict(hs=t["hs"], wq=wqf, q_bias=qb.reshape(1, -1), wo=wo_packed, bias_o=t["bias_o"].reshape(1, -1))
    got = A.ref_xattn_fused(p, v, kv=(t["kt"], t["vt"], t["kip"], t["vip"]), wo_slot=slots)["out"].ref
    exp = F.linear(_two_sdpa(qn, t, dims), t["wo"].double(), t["bias_o"].double()) + t["hs"].double()
    close(got, exp)


def test_row_gemm_reference_geglu_and_groupnorm_fold():
    from photoverse_amd.ops import pack_geglu_rows
    g = torch.Generator().manual_seed(8)
    M, K, n = 256, 320, 320
    x = h16(M, K, g=g) * 2 + 0.5
    w = h16(2 * n, K, g=g, scale=0.05)
    b = torch.randn(2 * n, generator=g)
    wp, bp = pack_geglu_rows(w, b)
    p = SimpleNamespace(M=M, K=K, N=2 * n, ln=1, ln_eps=1e-5, geglu=1, rows_per_image=0)
    got = A.ref_row_gemm(p, dict(x=x, w=wp, bias=bp.reshape(1, -1)))["out"].ref
    h = F.linear(F.layer_norm(x.double(), (K,), eps=1e-5), w.double(), b.double())
    close(got, h[:, :n] * F.gelu(h[:, n:]))
    tab = torch.randn(2, 2 * K, generator=g)
    p = SimpleNamespace(M=M, K=K, N=n, ln=0, ln_eps=1e-5, geglu=0, rows_per_image=128)
    got = A.ref_row_gemm(p, dict(x=x, w=w[:n].contiguous(), x_norm=tab))["out"].ref
    t3 = tab.double().reshape(2, 2, K).repeat_interleave(128, 0)
    close(got, F.linear((x.double() * t3[:, 0] + t3[:, 1]).half().double(), w[:n].double()))


def test_small_launcher_references():
    g = torch.Generator().manual_seed(9)
    # im2col: column k = ci * 9 + ky * 3 + kx of a 3x3 / pad 1 window
    x = torch.randn(2, 4, 5, 6, generator=g)
    a = SimpleNamespace(batch=2, cin=4, h=5, wd=6, kpad=64)
    got = A.ref_im2col(a, dict(x=x.reshape(1, -1)))["out"].ref
    exp = F.unfold(x.double(), 3, padding=1).transpose(1, 2).reshape(-1, 36)
    close(got[:, :36], exp.half().double(), 0.0 + 1e-300)
    assert not got[:, 36:].any()
    # conv_out: NHWC fp16 -> NCHW fp32
    xs = h16(2 * 5 * 6, 64, g=g)
    wt = h16(4, 64, 3, 3, g=g, scale=0.05)
    a = SimpleNamespace(batch=2, cin=64, h=5, wd=6, cout=4)
    got = A.ref_conv_out(a, dict(x=xs, w=wt.permute(0, 2, 3, 1).reshape(4, -1).contiguous(), bias=torch.ones(1, 4)))["out"].ref
    close(got, F.conv2d(to_nchw(xs, 2, 5, 6).double(), wt.double(), torch.ones(4, dtype=D), padding=1).reshape(8, 30))
    # timestep embedding [cos | sin], step index min(state[0], state[1] - 1)
    ts = torch.tensor([[999.0, 500.0, 1.0]])
    got = A.ref_timestep(SimpleNamespace(rows=2, dim=8, state=1), dict(timesteps=ts, state=torch.tensor([[7, 3]], dtype=torch.int32)))["out"].ref
    f = torch.exp(-math.log(10000) * torch.arange(4, dtype=D) / 4)
    assert torch.allclose(got[1], torch.cat([torch.cos(f), torch.sin(f)]))


def test_pointwise_softmax_posterior_references():
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2 * 4, 9, generator=g)
    w = torch.randn(4, 4, generator=g)
    got = A.ref_pointwise(SimpleNamespace(batch=2, cin=4, cout=4, hw=9), dict(x=x, w=w, bias=torch.zeros(1, 4)))["out"].ref
    close(got, torch.einsum("oc,bcp->bop", w.double(), x.double().reshape(2, 4, 9)).reshape(8, 9))
    s = h16(5, 64, g=g)
    close(A.ref_softmax_rows(SimpleNamespace(rows=5, cols=64, scale=0.3), dict(x=s))["x"].ref, torch.softmax(s.double() * 0.3, 1))
    m, e = torch.randn(2, 8, generator=g) * 40, torch.randn(1, 8, generator=g)
    got = A.ref_posterior(SimpleNamespace(batch=2, chw=4), dict(moments=m, eps=e))["out"].ref
    mm = m.double().reshape(2, 2, 4)
    close(got, (mm[:, 0] + torch.exp(0.5 * mm[:, 1].clamp(-30, 20)) * e.double().reshape(2, 4)).reshape(1, -1))


def test_masked_cfg_step_is_the_cfg_step_followed_by_the_blend():
    """pv_cfg_dpm_step_masked against an independent formulation: ``ref_cfg`` on the same arguments, then the inpainting blend in plain torch."""
    g = torch.Generator().manual_seed(15)
    B, ch, hw, steps = 2, 4, 12, 3
    n = B * ch * hw
    t = {k: torch.randn(1, n, generator=g) for k in ("eps_uncond", "eps_cond", "latents", "x0_prev", "known", "noise")}
    coef = torch.randn(steps, 8, generator=g)
    mask = torch.rand(B, hw, generator=g)
    mask[0, :4], mask[0, 4:8] = 1.0, 0.0
    state = torch.tensor([[1, steps]], dtype=torch.int32)
    a = SimpleNamespace(guidance=7.5, n=n, channels=ch, hw=hw)
    v = dict(t, coef=coef[1:2], state=state, mask=mask)
    L = A.layout_cfg_masked(a)
    assert (L["mask"].rows, L["mask"].cols) == (B, hw) and L["known"].cols == n and L["latents"].role == "inout" and L["known"].role == "in"
    base = A.ref_cfg(a, {k: v[k] for k in ("eps_uncond", "eps_cond", "latents", "x0_prev", "coef", "state")})
    got = A.ref_cfg_masked(a, v)
    assert torch.equal(got["x0_prev"].ref, base["x0_prev"].ref)                       # x0_prev receives the unblended x0
    m = mask.double()[:, None, :].expand(B, ch, hw).reshape(1, n)
    k = coef[1, 5].double() * t["known"].double() + coef[1, 6].double() * t["noise"].double()
    close(got["latents"].ref, m * base["latents"].ref + (1 - m) * k, 1e-14)
    keep, gen = (m == 0)[0], (m == 1)[0]
    assert keep.sum() == ch * 4 and gen.sum() == ch * 4
    assert torch.equal(got["latents"].ref[0, keep], k[0, keep]) and torch.equal(got["latents"].ref[0, gen], base["latents"].ref[0, gen])
    # m == 1 adds only the blend's own roundings to pv_cfg_dpm_step's bound; m == 0 leaves k's: a handful of fp32 ulps either way
    assert (got["latents"].bound[0, gen] <= base["latents"].bound[0, gen] + 4 * A.U32 * base["latents"].ref[0, gen].abs() + 1e-30).all()
    assert (got["latents"].bound[0, keep] <= 6 * A.U32 * (coef[1, 5].abs() * t["known"].abs() + coef[1, 6].abs() * t["noise"].abs())[0, keep].double() + 1e-30).all()
    # the comparator rejects a blend with the mask inverted
    assert PA.compare(got, {"latents": ((1 - m) * base["latents"].ref + m * k).float(), "x0_prev": base["x0_prev"].ref.float()})[0]
    assert not PA.compare(got, {"latents": got["latents"].ref.float(), "x0_prev": base["x0_prev"].ref.float()})[0]


# ------------------------------------------------------------------------------------------------------------------ comparator
def _gemm_expect(seed=11, M=200, K=512, N=128, store_rel=None):
    g = torch.Generator().manual_seed(seed)
    x, w = h16(M, K, g=g), h16(N, K, g=g, scale=0.05)
    e = A.ref_gemm(gemm_p(c0=K, lda0=K, M=M, N=N, hout=M, ldc=N), dict(a0=x, w=w))["out"]
    if store_rel is not None:                    # the same bound with another fp16-store term (the tightness check of the fragment defect)
        e.bound = e.bound - A.STORE16_REL * e.ref.abs() + store_rel * e.ref.abs()
    return e


def test_comparator_accepts_the_rounded_reference():
    e = _gemm_expect()
    fails, worst, agg = PA.compare({"out": e}, {"out": e.ref.half()})
    assert not fails and worst <= 0.5 and agg <= 1.0 / 1.5 + 1e-9


def _defect(kind, e):
    y = e.ref.half().double()
    if kind == "fragment":                        # one 16 x 16 fragment off by 2^-7 relative
        y[32:48, 64:80] = e.ref[32:48, 64:80] * (1 + 2.0 ** -7)
    elif kind == "m_tail":                        # the last row of the M tail wrong
        y[-1] = (e.ref[-1] * 1.01 + 0.01).half()
    elif kind == "nan":                           # an element never written
        y[7, 3] = float("nan")
    elif kind == "bound":                         # one element at 1.5x its bound
        y = e.ref.clone()
        y[5, 5] = e.ref[5, 5] + 1.5 * e.bound[5, 5]
    return y


@pytest.mark.parametrize("kind", ["fragment", "m_tail", "nan", "bound"])
def test_comparator_catches_injected_defects(kind):
    e = _gemm_expect()
    fails, _, _ = PA.compare({"out": e}, {"out": _defect(kind, e)})
    assert fails, kind
    if kind in ("fragment", "m_tail", "bound"):   # caught element by element, not only in aggregate
        assert [f for f in fails if "bound (" in f], fails


def test_fragment_defect_needs_the_fp16_store_term():
    """The 2^-7 fragment is caught because the store term is 2^-10 |ref|: with 2^-7 it would pass (the bound is not loose by design)."""
    e = _gemm_expect(store_rel=2.0 ** -7)
    y = e.ref.clone()
    y[32:48, 64:80] = e.ref[32:48, 64:80] * (1 + 2.0 ** -7)
    fails, _, _ = PA.compare({"out": e}, {"out": y})
    assert not [f for f in fails if "bound (" in f]


def test_comparator_catches_swapped_rowadd():
    g = torch.Generator().manual_seed(12)
    b, rpi, K, N = 3, 64, 128, 128
    x, w = h16(b * rpi, K, g=g), h16(N, K, g=g, scale=0.05)
    ra = torch.randn(b, N, generator=g)
    p = gemm_p(c0=K, lda0=K, M=b * rpi, N=N, hout=rpi, ldc=N, rowadd=1, rowadd_ld=N)
    e = A.ref_gemm(p, dict(a0=x, w=w, rowadd=ra))["out"]
    swapped = A.ref_gemm(p, dict(a0=x, w=w, rowadd=ra[[1, 0, 2]]))["out"].ref.half()
    assert PA.compare({"out": e}, {"out": swapped})[0]


def test_write_past_the_extent_is_caught():
    """A write one row past an output's extent (or into the row gap when ldc > N) changes bytes outside the described extent."""
    base = torch.zeros(10, 48, dtype=torch.float16)
    view = base[:8, :40]
    for bad in (lambda: base[8, :40].fill_(1), lambda: base[3, 40:].fill_(1)):
        before = PA.storage_bytes(base.untyped_storage()).clone()
        view.fill_(2)
        assert PA.changed_outside(before, base.untyped_storage(), [view]) == 0
        bad()
        assert PA.changed_outside(before, base.untyped_storage(), [view]) > 0
        base.zero_()


def test_colstats_check_uses_the_kernels_own_output():
    g = torch.Generator().manual_seed(13)
    y = h16(130, 64, g=g)
    e = A.colstats_expect(y, 130, 64)
    yy = y.double()
    assert torch.allclose(e.ref[2, :64], yy[128:].sum(0)) and torch.allclose(e.ref[0, 64:], (yy[:64] ** 2).sum(0))
    assert not PA.compare({"cs": e}, {"cs": e.ref.float()})[0]
    bad = e.ref.float().clone()
    bad[2, 5] += 1e-2
    assert PA.compare({"cs": e}, {"cs": bad})[0]


# ------------------------------------------------------------------------------------------------------------------ field coverage
@pytest.mark.parametrize("struct", sorted(A.STRUCT_FUNCS))
def test_every_abi_field_is_modelled_or_listed(struct):
    from photoverse_amd import _lib
    fields = {n for n, _ in getattr(_lib, struct)._fields_}
    read = A.fields_read(struct)
    listed = set(A.DISPATCH_ONLY.get(struct, {}))
    assert not (fields - read - listed), f"{struct}: fields neither read by the reference nor listed as dispatch-only / scratch: {fields - read - listed}"
    assert not (listed & read), f"{struct}: listed as dispatch-only but read: {listed & read}"
    assert listed <= fields


def test_every_recorded_launcher_has_a_reference():
    """The launchers the inference plans record (ops.Recorder's forward methods) all have a layout and a reference."""
    assert set(A.LAYOUT) == set(A.REF)
    for name in ("pv_gemm_conv", "pv_attention", "pv_cross_attention", "pv_cross_attention_fused", "pv_cross_attention_lnq", "pv_xattn_pack_kv",
                 "pv_row_gemm", "pv_layernorm", "pv_groupnorm_stats", "pv_groupnorm_stats_from_colstats", "pv_groupnorm_scale_shift",
                 "pv_groupnorm_apply", "pv_im2col3x3", "pv_conv_out", "pv_timestep_embedding", "pv_cfg_dpm_step", "pv_step_advance",
                 "pv_pointwise_nchw", "pv_softmax_rows", "pv_posterior_sample", "pv_cfg_dpm_step_masked"):
        assert name in A.REF, name


# ------------------------------------------------------------------------------------------------------------------ comparator on attention
def _attention_expects(lib_slots=None):
    """fp64 references of the three attention-family launchers at product-like scales (unit activations, weights ~ 1 / sqrt(C))."""
    g = torch.Generator().manual_seed(14)
    B, H, n, d = 1, 2, 1024, 40
    qkv = h16(B * n, 3 * H * d, g=g)
    C = H * d
    p = SimpleNamespace(batch=B, heads=H, nq=n, nk=n, d=d, causal=0, lse=0)
    out = {"attention": A.ref_attention(p, dict(q=qkv[:, :C], k=qkv[:, C:2 * C], v=qkv[:, 2 * C:]))}
    for name, (H, d, nq) in (("lnq", (8, 160, 128)), ("fused", (8, 40, 256))):
        C = H * d
        t, dims = _xattn_case(g, B=1, H=H, d=d, nq=nq)
        t["wq"], t["wo"] = h16(C, C, g=g, scale=C ** -0.5), h16(C, C, g=g, scale=C ** -0.5)
        pp = SimpleNamespace(batch=1, heads=H, nq=nq, nt=77, nip=5, d=d, w_text=1.0, w_ip=1.0, ln=1, ln_eps=1e-5)
        if name == "lnq":
            v = dict(hs=t["hs"], wq=t["wq"], kt=t["kt"], vt=t["vt"], kip=t["kip"], vip=t["vip"])
            out[name] = A.ref_xattn_lnq(pp, v)
        else:
            slots = list(range(C))
            v = dict(hs=t["hs"], wq=t["wq"], wo=t["wo"], bias_o=t["bias_o"].reshape(1, -1))
            out[name] = A.ref_xattn_fused(pp, v, kv=(t["kt"], t["vt"], t["kip"], t["vip"]), wo_slot=slots)
    return out


@pytest.fixture(scope="module")
def attn_expects():
    return _attention_expects()


@pytest.mark.parametrize("launcher", ["attention", "lnq", "fused"])
def test_attention_bounds_are_no_looser_than_the_kernel_tests(attn_expects, launcher):
    e = attn_expects[launcher]["out"]
    cap = {"attention": A.CAP["attention"], "lnq": A.CAP["lnq"], "fused": A.CAP["fused"]}[launcher]
    assert e.cap is not None and e.cap <= cap
    # the element bound stays below 2^-7 |ref| for most elements (a 2^-7 error is caught element by element)
    assert ((e.bound / e.ref.abs().clamp_min(1e-3)).median() < 2.0 ** -7).item()
    fails, _, agg = PA.compare({"out": e}, {"out": e.ref.half()})
    assert not fails and agg < 1.0


@pytest.mark.parametrize("launcher", ["attention", "lnq", "fused"])
@pytest.mark.parametrize("kind", ["fragment", "m_tail", "five_percent"])
def test_comparator_catches_defects_in_attention_outputs(attn_expects, launcher, kind):
    exp = attn_expects[launcher]
    e = exp["out"]
    y = e.ref.half().double()
    if kind == "fragment":                         # one 16 x 16 fragment off by 2^-7 relative
        y[32:48, 16:32] = e.ref[32:48, 16:32] * (1 + 2.0 ** -7)
    elif kind == "m_tail":                         # the last row of the M tail wrong
        y[-1] = e.ref[-1] * 1.01 + 0.01
    else:                                          # a 5 % error on one 16-row tile
        y[64:80] = e.ref[64:80] * 1.05
    fails, _, _ = PA.compare(exp, {"out": y})
    assert [f for f in fails if "bound (" in f], fails
