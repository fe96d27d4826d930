"""CPU checks of ``oracle.abi_ref`` (the per-launch references of the plan audit) and of the audit's comparator: each reference against an
independent formulation (``F.conv2d`` / ``F.linear`` / ``F.scaled_dot_product_attention``; for the launchers of the newer loop features and the
conditioning plans ``F.interpolate``, ``torch.fft``, the kernel tests' restatements, ``Tensor.half``, ``F.embedding``, at the inputs of the edge
catalogue), the comparator against injected defects, the derived bounds against the kernel tests' tolerances, the field / argument coverage of the
ABI, and the partition of its functions into audited and deliberately not audited ones.  The training tape's single launches (``abi_ref.TRAINING``)
go through the same catalogue checks - torch autograd in fp64 as the independent formulation of every backward launcher - and have their own tests at the
end of the file: the partition, the variants the catalogue must reach, the defects the comparator must catch, the caps, the conditions of the bounds."""
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


#: the launchers the audit covered before the partition existed: none of them may leave ``REF``
FIRST_AUDITED = ("pv_gemm_conv", "pv_attention", "pv_cross_attention", "pv_cross_attention_fused", "pv_cross_attention_lnq", "pv_xattn_pack_kv",
                 "pv_row_gemm", "pv_layernorm", "pv_groupnorm_stats", "pv_groupnorm_stats_from_colstats", "pv_groupnorm_scale_shift",
                 "pv_groupnorm_apply", "pv_im2col3x3", "pv_conv_out", "pv_timestep_embedding", "pv_cfg_dpm_step", "pv_step_advance",
                 "pv_pointwise_nchw", "pv_softmax_rows", "pv_posterior_sample", "pv_cfg_dpm_step_masked")
#: modules whose recorders are the plans of ``run_inference`` / ``generate.py`` (no backward pass lives in them)
INFERENCE_MODULES = ("infer", "pipeline", "unet", "clip", "vae", "scheduler")


def _inference_launchers():
    """Launchers the inference modules can record: the ``ops.Recorder`` methods they call on a recorder (``rec.<m>(`` / ``.tail.<m>(``), and the ``pv_*``
    functions those methods add - themselves or through the ``Recorder`` methods they call in turn (``solver_step`` picks one of five)."""
    import importlib
    import inspect
    import re
    from photoverse_amd.ops import Recorder
    source = {m: inspect.getsource(f) for m, f in inspect.getmembers(Recorder, inspect.isfunction)}
    adds = {m: set(re.findall(r"_add\(\s*self\.lib\.(pv_\w+)", src)) for m, src in source.items()}
    grew = True
    while grew:                                          # to the fixed point: a method adds what the methods it calls on ``self`` add
        grew = False
        for m, src in source.items():
            more = set().union(*(adds.get(c, set()) for c in re.findall(r"self\.(\w+)\(", src))) - adds[m]
            adds[m] |= more
            grew = grew or bool(more)
    found = set()
    for mod in INFERENCE_MODULES:
        src = inspect.getsource(importlib.import_module(f"photoverse_amd.{mod}"))
        for m in re.findall(r"(?:rec|tail)\.(\w+)\(", src):
            found |= adds.get(m, set())
    return found


def test_every_recorded_launcher_has_a_reference():
    """Every function of the C ABI (``_lib.SIGNATURES``) is in exactly one of ``REF`` (audited) and ``NOT_AUDITED`` (outside the audit, with its reason):
    a new ``pv_*`` function fails here until someone places it.  Nothing an inference plan can record is outside the audit."""
    from photoverse_amd import _lib
    assert set(A.LAYOUT) == set(A.REF)
    names = set(_lib.SIGNATURES)
    assert not (set(A.REF) & set(A.NOT_AUDITED)), set(A.REF) & set(A.NOT_AUDITED)
    assert not (names - set(A.REF) - set(A.NOT_AUDITED)), f"launchers neither audited nor listed as outside the audit: {names - set(A.REF) - set(A.NOT_AUDITED)}"
    assert not ((set(A.REF) | set(A.NOT_AUDITED)) - names), f"placed, but not in the ABI: {(set(A.REF) | set(A.NOT_AUDITED)) - names}"
    assert all(isinstance(r, str) and r.strip() for r in A.NOT_AUDITED.values())
    for name in FIRST_AUDITED:
        assert name in A.REF, name
    inference = _inference_launchers()
    assert {"pv_cfg_dpm_step_pag", "pv_freeu_rows", "pv_clip_text_embed", "pv_fusion_draw", "pv_composite_clamp_f32"} <= inference, inference
    assert not (inference & set(A.NOT_AUDITED)), f"recorded by an inference plan, listed as outside the audit: {inference & set(A.NOT_AUDITED)}"
    # every launcher with a state- or content-dependent extent names two of its own arguments
    for name, (first, dep, _, _) in A.DEPENDENT.items():
        assert name in A.REF and {first, dep} <= set(A.ARGS[name]), name


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


# ------------------------------------------------------------------------------------------------------------------ guided / conditioning launchers
NEW_LAUNCHERS = sorted(A.ARG_FUNCS)
NEW_CASES = ("step-", "product-", "fusion-", "freeu-", "resize-", "composite-", "clamp-", "affine-", "rows-mean", "casts-", "patchify", "clip-", "train-")
#: the training tape's single launches (the 24 argument-list launchers among them are in NEW_LAUNCHERS): none of them may leave ``REF`` again
TRAINING_AUDITED = ("pv_act_forward", "pv_geglu", "pv_transpose_f16", "pv_colsum_f16", "pv_reduce_blocks", "pv_reduce_mean", "pv_reduce_sumsq", "pv_dropout_f16",
                    "pv_geglu_backward", "pv_act_backward", "pv_add_rows_f16", "pv_dilate2x", "pv_pool2x_sum", "pv_sign_f32", "pv_gather_rows_f32",
                    "pv_col_affine_f16", "pv_prelu_f16", "pv_maxpool2x2", "pv_gray_resize", "pv_gray_resize_backward", "pv_cosine_embedding_loss",
                    "pv_softmax_rows_backward", "pv_clamp_mask_f32", "pv_layernorm_backward", "pv_wgrad_tn")
#: what stays outside the audit after the training slice: the two MFMA attention backward passes and the GroupNorm backward (the next slice), the four
#: pointer-table launchers, the five host queries
STILL_NOT_AUDITED = ("pv_attention_backward", "pv_cross_attention_backward", "pv_groupnorm_backward", "pv_pack_weights", "pv_sumsq_multi", "pv_clip_coef_groups",
                     "pv_adamw_multi", "pv_abi_version", "pv_device_count", "pv_xattn_fused_wo_slot", "pv_gemm_conv_kernel_info", "pv_attention_kernel_info")
AUDITED_LAUNCHERS = sorted(set(NEW_LAUNCHERS) | {"pv_layernorm_backward"})


@pytest.fixture(scope="module")
def catalogue(lib):
    """launcher -> [(case, call, params, views, expects)]: the references of the launchers above on the inputs of the edge catalogue, recorded dry."""
    from oracle import edge_cases as E
    out = {n: [] for n in AUDITED_LAUNCHERS}
    for c in E.CASES:
        if not c.name.startswith(NEW_CASES):
            continue
        with E.environment(c.env):
            rec = E.build(c, "cpu")
        for i, (fn, _) in enumerate(rec.calls):
            name, p, v = E.host_views(rec, i)
            out[name].append((c.name, i, p, v, A.REF[name](p, v)))
    return out


def same(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = torch.isfinite(b)
    assert torch.equal(a[~fin], b[~fin].to(a.dtype))
    err = ((a[fin] - b[fin]).abs() / (1 + b[fin].abs())).max().item() if fin.any() else 0.0
    assert err < tol, err


def _r32(x):
    return torch.tensor(float(x), dtype=torch.float32).item()


def _indep_step(p, v):
    """tests/test_pag_cpu.py's restatement (it contains those of test_guidance_cpu.py and test_sampler_cpu.py) with the noise of oracle.philox."""
    from oracle.philox import noise_ref
    from test_pag_cpu import pag_step_ref
    B, shape = p.batch, (p.batch, p.channels, p.hw)
    t = lambda k: v[k].reshape(shape) if k in v else None
    z = None
    if "rng" in v:
        w = [int(x) & 0xFFFFFFFF for x in v["rng"].reshape(-1).tolist()]
        st = v["state"].reshape(-1).tolist()
        z = noise_ref(shape, w[0] | (w[1] << 32), w[2], w[3], min(st[0], st[1] - 1))
    blend = dict(mask=v["mask"].reshape(B, 1, p.hw), known=t("known"), noise=t("noise")) if "mask" in v else {}
    xn, x0, _ = pag_step_ref(t("eps_uncond"), t("eps_image"), t("eps_cond"), t("eps_perturbed"), t("latents"), t("x0_prev"), v["coef"].reshape(-1),
                             _r32(p.g_text), _r32(p.g_image), _r32(getattr(p, "g_pag", 0.0)), _r32(p.rescale), z=z, **blend)
    return {"latents": xn.reshape(1, -1), "x0_prev": x0.reshape(1, -1)}


def _indep_fusion(p, v):
    from oracle.philox import philox4x32_10
    w = [int(x) & 0xFFFFFFFF for x in v["rng"].reshape(-1).tolist()]
    on = not (p.only_last_step and "state" in v) or v["state"][0, 0].item() == v["state"][0, 1].item() - 1
    out = torch.ones(p.n_layers, 2, dtype=D)
    for i in range(p.n_layers):
        u = (int(philox4x32_10((w[0], w[1]), (w[2], i, 0, 0))[0]) >> 8) / 2.0 ** 24
        if "forced" in v and v["forced"][0, i] >= 0:
            u = v["forced"][0, i].item()
        if on and u < _r32(p.rule1):
            out[i] = torch.tensor([_r32(p.scale), 0.0])
        elif on and u > _r32(p.rule2):
            out[i] = torch.tensor([0.0, _r32(p.scale)])
    nxt = v["rng"].reshape(-1).clone()
    nxt[2] += 1                                                     # int32: wraps like the device's uint32 word
    return {"out": out, "rng": nxt.double().reshape(1, 4)}


def _indep_freeu(p, v):
    from test_freeu_cpu import fourier_filter_ref
    res = {}
    if "x" in v:
        scale = torch.ones(p.cx, dtype=D)
        scale[:p.cx // 2] = _r32(p.b)
        res["x_out"] = v["x"].double() * scale
    if "skip" in v:
        planes = v["skip"].double().reshape(p.batch, p.h, p.w, p.cs).permute(0, 3, 1, 2)
        res["skip_out"] = fourier_filter_ref(planes, 1, _r32(p.s)).permute(0, 2, 3, 1).reshape(-1, p.cs)
    return res


def _indep_resize(p, v):
    B, C_ = p.batch, p.channels
    r = F.interpolate(v["x"].double().reshape(B, C_, p.h, p.w), size=(p.oh, p.ow), mode="bilinear", align_corners=False)
    if "ca" in v:
        r = r * v["ca"].double().reshape(B, 1, 1, 1)
    if "y" in v:
        r = r + v["cb"].double().reshape(B, 1, 1, 1) * v["y"].double().reshape(B, C_, p.oh, p.ow)
    return {"out": r.reshape(1, -1)}


def _indep_text(p, v):
    B, S, E = p.batch, p.seq, p.n_concept
    rows = []
    for b in range(B):
        emb = F.embedding(v["ids"][b].long(), v["tok"].double())                  # nn.Embedding's arithmetic
        if E:
            i = int(v["placeholder_idx"][0, b])
            emb = torch.cat([emb[:i], v["concept"].double().reshape(B, E, p.dim)[b], emb[i + 1:]])[:S]      # models/clip.py: insert, shift, truncate
        rows.append(emb + F.embedding(torch.arange(S), v["pos"].double()))
    return {"out": torch.cat(rows)}


def _indep_small(name, p, v):
    d = lambda k: v[k].double()
    if name == "pv_affine_rows_f32":
        r = torch.einsum("b,bi->bi", d("ca").reshape(-1), d("x").reshape(p.batch, -1))
        if "y" in v:
            r = torch.addcmul(r, d("cb").reshape(-1, 1), d("y").reshape(p.batch, -1))
        return {"out": r.reshape(1, -1)}
    if name == "pv_composite_clamp_f32":
        m = d("mask").reshape(p.batch, 1, p.hw)
        g, o = d("gen").reshape(p.batch, p.channels, p.hw), d("orig").reshape(p.batch, p.channels, p.hw)
        return {"out": torch.minimum(torch.maximum(o + m * (g - o), torch.tensor(_r32(p.lo), dtype=D)), torch.tensor(_r32(p.hi), dtype=D)).reshape(1, -1)}
    if name == "pv_clamp_f32":
        return {"x": torch.minimum(torch.maximum(d("x"), torch.tensor(_r32(p.lo), dtype=D)), torch.tensor(_r32(p.hi), dtype=D))}
    if name == "pv_rows_mean":
        out = torch.stack([d("x")[g * p.group_rows:g * p.group_rows + p.count].sum(0) / p.count for g in range(p.groups)])
        return {"y": out + (d("y") if p.accumulate else 0)}
    if name == "pv_cast_f32_to_f16":
        return {"y": v["x"].half().double()}
    if name == "pv_cast_f16_to_f32":
        return {"y": v["x"].float().double()}
    if name == "pv_patchify":
        g = p.img // p.patch
        cols = F.unfold(d("x").reshape(p.batch, p.ch, p.img, p.img), p.patch, stride=p.patch).transpose(1, 2).reshape(p.batch * g * g, -1)
        return {"out": F.pad(cols.half().double(), (0, p.kpad - cols.shape[1]))}
    if name == "pv_clip_vision_embed":
        tokens = torch.cat([d("cls").reshape(1, 1, p.dim).expand(p.batch, 1, p.dim), d("patches").reshape(p.batch, p.ntok - 1, p.dim)], 1)
        return {"out": (tokens + F.embedding(torch.arange(p.ntok), d("pos"))).reshape(-1, p.dim)}
    raise KeyError(name)


def _philox_scalar(key, ctr):
    """Philox4x32-10 on Python integers (one block), written out from the paper: a formulation independent of oracle.philox's numpy arrays."""
    k0, k1 = key
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _torch_act(x, act):
    return (lambda t: t, F.silu, lambda t: t * torch.sigmoid(1.702 * t), lambda t: F.leaky_relu(t, 0.01), F.gelu)[act](x)


def _grad(fn, x, dy):
    """d(fn(x) . dy) / dx by torch autograd in fp64."""
    xr = x.double().clone().requires_grad_()
    fn(xr).backward(dy.double())
    return xr.grad


def _indep_ln_bwd(p, v):
    rows, cols = p.rows, p.cols
    grp = max(p.dy_group, 1)
    dy = v["dy"].double().repeat_interleave(grp, 0)[:rows] * _r32(p.dy_scale)
    if p.dy_group > 1:
        dy = dy * (torch.arange(rows) % grp >= p.dy_skip).double()[:, None]
    x = v["x"].double().clone().requires_grad_()
    gam = v["gamma"].double().reshape(1, cols).expand(rows, cols).clone().requires_grad_()          # one copy of gamma / beta per row: their gradients are
    bet = v["beta"].double().reshape(1, cols).expand(rows, cols).clone().requires_grad_()           # the rows' own (g xhat, g) terms
    y = F.layer_norm(x, (cols,), eps=float(p.eps)) * gam + bet
    if p.act == 3:
        y = F.leaky_relu(y, 0.01)
    y.backward(dy)
    res = {"dx": x.grad + (v["add"].double() if "add" in v else 0)}
    if "dgb_partial" in v:
        blk = 4 * max(p.rows_per_wave, 1)
        res["dgb_partial"] = torch.stack([torch.cat([gam.grad[i:i + blk].sum(0), bet.grad[i:i + blk].sum(0)]) for i in range(0, rows, blk)])
    return res


def _indep_train(name, p, v):
    d = lambda k: v[k].double()
    nhwc = lambda t, b, h, w: t.reshape(b, h, w, -1).permute(0, 3, 1, 2)
    rows_of = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    if name == "pv_act_forward":
        return {"y": _torch_act(d("x"), p.act)}
    if name == "pv_act_backward":
        return {"dx": _grad(lambda t: _torch_act(t, p.act), v["x"], v["dy"])}
    if name == "pv_geglu":
        return {"out": d("x")[:, :p.n] * F.gelu(d("x")[:, p.n:])}
    if name == "pv_geglu_backward":
        return {"dh": _grad(lambda t: t[:, :p.n] * F.gelu(t[:, p.n:]), v["h"], v["dy"])}
    if name == "pv_col_affine_f16":
        return {"y": torch.addcmul(d("shift") if "shift" in v else torch.zeros(1, p.cols, dtype=D), d("x"), d("scale"))}
    if name == "pv_prelu_f16":
        a = d("slope").reshape(1)
        return {"out": _grad(lambda t: F.prelu(t, a), v["x"], v["dy"]) if "dy" in v else F.prelu(d("x"), a)}
    if name == "pv_add_rows_f16":
        return {"out": (v["a"].float() + v["b"].float()).half().double()}
    if name == "pv_dropout_f16":
        w = [int(t) & 0xFFFFFFFF for t in v["rng"].reshape(-1).tolist()]
        thr, inv = int(_r32(p.p) * 65536.0), 1.0 / (1.0 - _r32(p.p))
        x = d("x")
        out = torch.zeros(p.rows, p.cols if p.backward else p.copies * p.cols, dtype=D)
        for k in range(p.copies):
            for r in range(p.rows):
                for ch in range(p.cols // 8):
                    blk = _philox_scalar((w[0], w[1]), (r * (p.cols // 8) + ch, p.site & 0xFFFFFFFF, w[2], k))
                    for j in range(8):
                        if ((blk[j // 2] >> (16 * (j % 2))) & 0xFFFF) >= thr:
                            c = ch * 8 + j
                            if p.backward:
                                out[r, c] += x[r, k * p.cols + c] * inv
                            else:
                                out[r, k * p.cols + c] = x[r, c] * inv
        return {"out": out + (d("add") if "add" in v else 0)}
    if name == "pv_softmax_rows_backward":
        pm = d("p")
        jac = torch.diag_embed(pm) - pm.unsqueeze(2) * pm.unsqueeze(1)          # the softmax Jacobian at p, per row
        return {"dp": _r32(p.scale) * torch.einsum("rij,rj->ri", jac, d("dp"))}
    if name == "pv_transpose_f16":
        return {"out": F.pad(d("x").t(), (0, p.rows_pad - p.rows))}
    if name == "pv_dilate2x":
        x = nhwc(d("x"), p.batch, p.h, p.w)
        return {"z": rows_of(F.conv_transpose2d(x, torch.ones(p.c, 1, 1, 1, dtype=D), stride=2, output_padding=1, groups=p.c))}
    if name == "pv_pool2x_sum":
        g = _grad(lambda t: F.interpolate(t, scale_factor=2, mode="nearest"), torch.zeros(p.batch, p.c, p.h, p.w), nhwc(v["g"], p.batch, 2 * p.h, 2 * p.w))
        return {"out": rows_of(g) + (d("add") if "add" in v else 0)}
    if name == "pv_maxpool2x2":
        x = nhwc(v["x"], p.batch, p.h, p.w)
        if "dy" not in v:
            return {"out": rows_of(F.max_pool2d(x.double(), 2, 2))}
        return {"out": rows_of(_grad(lambda t: F.max_pool2d(t, 2, 2), x, nhwc(v["dy"], p.batch, p.h // 2, p.w // 2)))}
    if name == "pv_sign_f32":
        return {"out": _grad(lambda t: _r32(p.coef) * t.abs(), v["x"], torch.ones_like(v["x"]))}
    if name == "pv_clamp_mask_f32":
        return {"out": _grad(lambda t: F.hardtanh(t, _r32(p.lo), _r32(p.hi)), v["y"], v["dy"])}          # hardtanh's gradient: strictly inside
    if name == "pv_gather_rows_f32":
        out = torch.zeros(p.batch, p.n_e, p.dim, dtype=D)
        for b in range(p.batch):
            for e in range(p.n_e):
                row = int(v["idx"][0, b]) + e
                if 0 <= row < p.seq:
                    out[b, e] = _r32(p.scale) * d("x")[b * p.seq + row]
        return {"out": out.reshape(1, -1)}
    if name == "pv_reduce_blocks":
        return {"out": _r32(p.scale) * torch.einsum("bi->i", d("x")).reshape(1, -1)}
    if name == "pv_colsum_f16":
        return {"out": torch.ones(1, p.rows, dtype=D) @ d("x")}
    if name == "pv_reduce_mean":
        r = F.mse_loss(d("a"), d("b")) if p.mode == 2 else F.l1_loss(d("a"), torch.zeros_like(d("a"))) if p.mode == 1 else torch.mean(d("a"))
        return {"out": r.reshape(1, 1)}
    if name == "pv_reduce_sumsq":
        return {"out": (_r32(p.scale) * torch.linalg.vector_norm(d("a")) ** 2).reshape(1, 1)}
    if name == "pv_wgrad_tn":
        slabs = []
        for s in range(p.nsplit):
            r = slice(s * p.rows_per_split, min(p.m, (s + 1) * p.rows_per_split))
            w = torch.zeros(p.n, p.k, dtype=D, requires_grad=True)                     # the weight gradient of y = x W^T under dy, by autograd
            F.linear(d("x")[r], w).backward(d("dy")[r])
            slabs.append(w.grad.reshape(-1))
        return {"out": torch.stack(slabs)}
    if name in ("pv_gray_resize", "pv_gray_resize_backward"):
        wts = torch.tensor([0.2989, 0.5870, 0.1140], dtype=D)
        fwd = lambda t: F.interpolate(torch.tensordot(t, wts, dims=([1], [0])).unsqueeze(1), size=(p.size, p.size), mode="bilinear", align_corners=False) * _r32(p.mul)
        if name == "pv_gray_resize":
            return {"y": (fwd(d("x").reshape(p.batch, 3, p.h, p.w)) + _r32(p.add)).reshape(1, -1)}
        return {"dx": _grad(fwd, torch.zeros(p.batch, 3, p.h, p.w), v["dy"].reshape(p.batch, 1, p.size, p.size)).reshape(1, -1)}
    if name == "pv_cosine_embedding_loss":
        e2 = d("e2").clone().requires_grad_()
        loss = torch.nn.CosineEmbeddingLoss(reduction="none")(d("e1"), e2, torch.full((p.batch,), 1.0 if p.target > 0 else -1.0, dtype=D))
        res = {"per_sample": loss.detach().reshape(1, -1)}
        if "de2" in v:
            (loss.mean() * _r32(p.gscale)).backward()
            res["de2"] = e2.grad
        return res
    if name == "pv_layernorm_backward":
        return _indep_ln_bwd(p, v)
    raise KeyError(name)


def independent(name, p, v):
    if name.startswith("pv_cfg_dpm_step"):
        return _indep_step(p, v)
    if name in A.TRAINING:
        return _indep_train(name, p, v)
    return {"pv_fusion_draw": _indep_fusion, "pv_freeu_rows": _indep_freeu, "pv_resize_bilinear_affine_f32": _indep_resize,
            "pv_clip_text_embed": _indep_text}.get(name, lambda p_, v_: _indep_small(name, p_, v_))(p, v)


@pytest.mark.parametrize("launcher", AUDITED_LAUNCHERS)
def test_reference_matches_an_independent_evaluation(catalogue, launcher):
    """Each reference against another formulation of the same operation at every launch of the catalogue: F.interpolate (resize), torch.fft (FreeU),
    the kernel tests' restatements (steps), Tensor.half (casts), F.embedding / F.unfold (embeds, patchify): equal to fp64 rounding.  The training tape:
    torch autograd in fp64 for every backward launcher, F.max_pool2d, F.interpolate, nn.CosineEmbeddingLoss, F.layer_norm, F.gelu, F.prelu, F.hardtanh, a
    scalar Philox for the dropout masks, F.linear's weight gradient for wgrad."""
    entries = catalogue[launcher]
    assert entries, launcher
    for case, i, p, v, exp in entries:
        ind = independent(launcher, p, v)
        assert set(ind) <= set(exp), (case, set(ind), set(exp))
        for k, t in ind.items():
            # the FreeU closed form sums seven terms where the FFT transforms the plane: both within 1e-11 of the exact filter
            # torch's CosineEmbeddingLoss adds 1e-12 to the squared norms where the header says 1e-8: 1e-8 / |e|^2 apart
            same(exp[k].ref, t, 1e-11 if launcher == "pv_freeu_rows" else 1e-8 if launcher == "pv_cosine_embedding_loss" else 1e-12)


def _as_stored(exp, v):
    return {k: e.ref.to(v[k].dtype) for k, e in exp.items() if e.derive is None}


@pytest.mark.parametrize("launcher", AUDITED_LAUNCHERS)
def test_comparator_accepts_the_rounded_reference_and_rejects_twice_the_bound(catalogue, launcher):
    for case, i, p, v, exp in catalogue[launcher]:
        got = _as_stored(exp, v)
        fails, worst, worst_agg = PA.compare(exp, got)
        assert not fails and worst < 1.0 and worst_agg < 1.0, (case, i, fails, worst, worst_agg)
        for k, e in exp.items():
            if e.derive is not None:
                continue
            bad = {kk: t.clone() for kk, t in got.items()}
            fin = torch.isfinite(e.ref)
            j = int(torch.where(fin, -e.ref.abs(), torch.full_like(e.ref, -float("inf"))).argmax())      # the smallest finite reference: the move is not absorbed
            r, c = divmod(j, e.ref.shape[1])
            step = 1.0 if e.store is None else 2 * e.bound[r, c].item()
            bad[k][r, c] = (e.ref[r, c] + step).to(bad[k].dtype) if fin.any() else 0.0       # (a reference of infinities only: a finite value is wrong)
            assert PA.compare(exp, bad)[0], (case, i, k, "an element moved by twice its bound passes")


def test_step_bounds_are_no_looser_than_the_kernel_tests(catalogue):
    """At the catalogue's inputs every derived element bound of the three step launchers is within what tests/test_guidance_gpu.py, test_sampler_gpu.py
    and test_pag_gpu.py allow: TOL_STEP / TOL_RESCALE in (1 + |ref|) form, plus TOL_NOISE |cn| on the latents of a stochastic launch."""
    import test_guidance_gpu as G
    import test_sampler_gpu as S
    assert A.TOL_NOISE == S.TOL_NOISE and (S.TOL_STEP, S.TOL_RESCALE) == (G.TOL_STEP, G.TOL_RESCALE)
    n = 0
    for launcher in ("pv_cfg_dpm_step_guided", "pv_cfg_dpm_step_stochastic", "pv_cfg_dpm_step_pag"):
        for case, i, p, v, exp in catalogue[launcher]:
            tol = G.TOL_RESCALE if p.rescale > 0 else G.TOL_STEP
            cn = abs(v["coef"][0, 7].item()) if "rng" in v else 0.0
            for k, extra in (("latents", S.TOL_NOISE * cn), ("x0_prev", 0.0)):
                e = exp[k]
                worst = (e.bound / (tol * (1 + e.ref.abs()) + extra)).max().item()
                assert worst <= 1.0, (case, i, k, worst)
                n += 1
    assert n >= 2 * 18 * 16


def test_freeu_and_resize_bounds_are_no_looser_than_the_kernel_tests(catalogue):
    """FreeU's skip: 2^-10 |ref| + 2^-12 max|x| (1 + |s - 1|) (tests/test_freeu_gpu.py); the resize: rtol = atol = 1e-5 (tests/test_hires_gpu.py)."""
    n = 0
    for case, i, p, v, exp in catalogue["pv_freeu_rows"]:
        if "skip_out" in exp:
            e, s = exp["skip_out"], _r32(p.s)
            allowed = 2.0 ** -10 * e.ref.abs() + 2.0 ** -12 * v["skip"].double().abs().max() * (1 + abs(s - 1))
            assert (e.bound <= allowed).all(), (case, (e.bound / allowed).max().item())
            n += 1
    for case, i, p, v, exp in catalogue["pv_resize_bilinear_affine_f32"]:
        e = exp["out"]
        assert (e.bound <= 1e-5 * (1 + e.ref.abs())).all(), (case, (e.bound / (1e-5 * (1 + e.ref.abs()))).max().item())
        n += 1
    assert n >= 8 + 12


def test_the_identity_resize_and_the_zero_weight_taps_are_exact(catalogue):
    ident = [(p, v, exp) for case, i, p, v, exp in catalogue["pv_resize_bilinear_affine_f32"] if (p.h, p.w) == (p.oh, p.ow) and "ca" not in v and "y" not in v]
    assert ident
    for p, v, exp in ident:
        assert torch.equal(exp["out"].ref, v["x"].double())
    # a weight of exactly 0 returns the tap itself, whatever its neighbour holds
    x = torch.tensor([[1.0, float("inf")], [2.0, float("nan")]]).reshape(1, -1)
    p = SimpleNamespace(batch=1, channels=1, h=2, w=2, oh=2, ow=2, ca=0, y=0, cb=0)
    assert torch.equal(A.ref_resize(p, dict(x=x))["out"].ref.nan_to_num(nan=-7.0), x.double().nan_to_num(nan=-7.0))


@pytest.mark.parametrize("launcher", NEW_LAUNCHERS)
def test_every_positional_argument_is_modelled(launcher, monkeypatch):
    """Every name of ``ARGS[launcher]`` is read by its layout or its reference, and ``ARGS`` has the C signature's length (the stream excluded)."""
    from photoverse_amd import _lib
    assert len(A.ARGS[launcher]) == len(_lib.SIGNATURES[launcher][1]) - 1
    assert not (set(A.ARGS[launcher]) - A.args_read(launcher)), set(A.ARGS[launcher]) - A.args_read(launcher)
    # an argument added to the ABI that nobody models shows up as unread
    monkeypatch.setitem(A.ARGS, launcher, A.ARGS[launcher] + ("an_argument_nobody_models",))
    assert set(A.ARGS[launcher]) - A.args_read(launcher) == {"an_argument_nobody_models"}


# ------------------------------------------------------------------------------------------------------------------ the training tape's single launches
def test_training_launchers_stay_audited_and_the_rest_is_named():
    """The 25 launchers of the training slice are in ``REF`` for good; ``NOT_AUDITED`` holds exactly the twelve that remain, each with a reason of its own
    (the five host queries share theirs)."""
    assert len(TRAINING_AUDITED) == 25 and set(TRAINING_AUDITED) == set(A.TRAINING)
    for name in TRAINING_AUDITED:
        assert name in A.REF and name in A.LAYOUT and name not in A.NOT_AUDITED, name
        assert name in A.ARGS or name == "pv_layernorm_backward", name
    assert set(A.NOT_AUDITED) == set(STILL_NOT_AUDITED) and len(A.NOT_AUDITED) == 12
    reasons = [A.NOT_AUDITED[n] for n in STILL_NOT_AUDITED[:7]]
    assert len(set(reasons)) == 7 and all(len(r) > 80 and "separate piece of work" not in r for r in reasons), reasons
    assert all("launches nothing" in A.NOT_AUDITED[n] for n in STILL_NOT_AUDITED[7:])
    assert A.STRUCT_FUNCS["LayerNormBwdParams"] == A.TRAINING["pv_layernorm_backward"]


def _training_entries(catalogue):
    return [(n, e) for n in TRAINING_AUDITED for e in catalogue[n]]


def test_training_catalogue_reaches_every_variant_the_audit_names(catalogue):
    """The shapes and variants the training slice exists for are in the dry-recorded catalogue (a case that lost one would still pass its own audit)."""
    get = lambda n: [p for _, _, p, _, _ in catalogue[n]]
    for n in ("pv_act_forward", "pv_act_backward"):
        assert {(p.rows, p.cols, p.act) for p in get(n)} == {(r, c, a) for r, c in ((1, 8), (33, 40), (65, 40)) for a in range(5)}
    for n in ("pv_geglu", "pv_geglu_backward", "pv_add_rows_f16", "pv_col_affine_f16", "pv_prelu_f16", "pv_softmax_rows_backward", "pv_dropout_f16"):
        assert {(1, 8), (33, 40), (65, 40)} <= {(p.rows, getattr(p, "cols", 0) or p.n) for p in get(n)}, n
    assert {bool(p.shift) for p in get("pv_col_affine_f16")} == {False, True} and {bool(p.dy) for p in get("pv_prelu_f16")} == {False, True}
    assert {(round(p.p, 3), p.copies, p.backward, bool(p.add)) for p in get("pv_dropout_f16")} >= {(pp, k, b, a) for pp in (0.0, 0.1) for k in (1, 3)
                                                                                                     for b, a in ((0, False), (1, False), (1, True))}
    assert {(p.batch, p.h, p.w, p.c, bool(p.dy)) for p in get("pv_maxpool2x2")} == {(1, 2, 2, 8, False), (1, 2, 2, 8, True), (2, 4, 6, 16, False), (2, 4, 6, 16, True)}
    assert {(p.h, p.w, p.c) for p in get("pv_dilate2x")} == {(3, 5, 8), (3, 5, 24)} and {(p.c, bool(p.add)) for p in get("pv_pool2x_sum")} == {(8, False), (8, True), (24, False), (24, True)}
    assert any(p.n_e == 3 and p.dim % 256 for p in get("pv_gather_rows_f32"))
    idx = [v["idx"].reshape(-1).tolist() for _, _, p, v, _ in catalogue["pv_gather_rows_f32"] if p.n_e == 3][0]
    assert 6 in idx and min(idx) < 0
    for n in ("pv_gray_resize", "pv_gray_resize_backward"):
        assert {(p.h, p.w, p.size) for p in get(n)} == {(5, 5, 8), (9, 9, 4), (6, 6, 6), (7, 5, 4)}
    assert all(p.x_image_stride > 3 * p.h * p.w for p in get("pv_gray_resize")) and all(p.dy_image_stride == 3 * p.size ** 2 for p in get("pv_gray_resize_backward"))
    assert {(p.dim, p.target > 0, bool(p.de2)) for p in get("pv_cosine_embedding_loss")} == {(d_, t, g) for d_ in (8, 100, 512) for t in (False, True) for g in (False, True)}
    assert {p.n for p in get("pv_sign_f32")} == {1, 257} == {p.n for p in get("pv_clamp_mask_f32")}
    assert {(p.rows, p.cols, p.rows_pad, p.ldo > p.rows_pad) for p in get("pv_transpose_f16")} == {(33, 40, 64, False), (7, 8, 7, False), (33, 40, 33, True)}
    assert {(p.nblk, p.inner) for p in get("pv_reduce_blocks")} >= {(b, i) for b in (1, 7, 8, 9, 31, 32, 33, 57) for i in (1, 33)} and all(p.scale != 1 for p in get("pv_reduce_blocks")[:16])
    assert {(p.rows, p.cols, p.nblk) for p in get("pv_colsum_f16")} == {(130, 257, 2), (5, 8, 4)}
    assert {(p.mode, p.is_f16, p.n) for p in get("pv_reduce_mean")} == {(m, f, n) for m in range(3) for f in (0, 1) for n in (1, 255, 4097)}
    assert any(p.n > 256 * p.n_partial for p in get("pv_reduce_mean")) and {p.n for p in get("pv_reduce_sumsq")} == {1, 255, 4097}
    assert {(p.m, p.n, p.k) for p in get("pv_wgrad_tn")} == {(7, 8, 8), (65, 136, 200), (1025, 8, 136)}
    assert any(p.nsplit > 1 and p.m - (p.nsplit - 1) * p.rows_per_split == 1 for p in get("pv_wgrad_tn")) and all(p.lddy > p.n for p in get("pv_wgrad_tn"))
    ln = get("pv_layernorm_backward")
    vec = [p for p in ln if not p.dgb_partial and p.cols % 8 == 0 and p.ldx % 8 == 0]
    assert {p.cols for p in vec} >= {8, 200, 320, 328, 640, 648, 768, 776, 1024, 1032, 1280, 1288, 2048}
    from oracle import edge_cases as E
    assert all(p.rows == E.ln_bwd_full_workgroup(p.cols) + 1 for p in vec if p.dy_group <= 1)
    assert any(p.cols == 324 for p in ln) and any(p.cols == 320 and p.ldx % 8 for p in ln)
    assert {(p.rows_per_wave, p.rows, p.cols) for p in ln if p.dgb_partial} >= {(1, 9, 40), (2, 2053, 8)}
    assert {p.act for p in ln} == {0, 3} and any(p.add and p.ldadd > p.cols for p in ln)
    assert {bool(p.dgb_partial) for p in ln if (p.dy_group, p.dy_skip, p.dy_scale) == (5, 1, 0.25)} == {False, True}


def test_training_comparator_catches_a_wrong_last_chunk_a_wrong_tail_row_and_a_flipped_exact_element(catalogue):
    """On round(ref) of every launch of the training catalogue: the last 8-column chunk of the last row off by 2^-7 relative; the last row replaced by
    a rotation of itself; one element of an exact output flipped - each must fail ``compare``."""
    seen = {n: set() for n in TRAINING_AUDITED}
    for name, (case, i, p, v, exp) in _training_entries(catalogue):
        base = _as_stored(exp, v)
        for k, e in exp.items():
            rows, cols = e.ref.shape
            if e.store is None:
                bad = {kk: t.clone() for kk, t in base.items()}
                bad[k][rows - 1, cols - 1] = 1.0 if e.ref[rows - 1, cols - 1] == 0 else 0.0
                assert PA.compare(exp, bad)[0], (case, i, k, "a flipped element of an exact output passes")
                seen[name].add("flip")
                continue
            chunk = e.ref[rows - 1, max(cols - 8, 0):]
            if (chunk.abs() > 2.0 ** -10).any():          # (below that a relative 2^-7 is under the fp16 subnormal spacing: a dropout row of zeros, a skipped row)
                bad = {kk: t.clone() for kk, t in base.items()}
                bad[k][rows - 1, max(cols - 8, 0):] = (chunk * (1 + 2.0 ** -7)).to(bad[k].dtype)
                assert PA.compare(exp, bad)[0], (case, i, k, "a last chunk off by 2^-7 passes")
                seen[name].add("chunk")
            if rows > 1 and cols > 1 and e.ref[rows - 1].abs().max() > 0:
                bad = {kk: t.clone() for kk, t in base.items()}
                bad[k][rows - 1] = base[k][rows - 1].roll(1)
                if not torch.equal(bad[k][rows - 1], base[k][rows - 1]):
                    assert PA.compare(exp, bad)[0], (case, i, k, "a wrong tail row passes")
                    seen[name].add("row")
    exact = {"pv_sign_f32", "pv_clamp_mask_f32", "pv_dilate2x", "pv_transpose_f16", "pv_maxpool2x2", "pv_add_rows_f16"}
    for n in TRAINING_AUDITED:
        assert seen[n] == {"flip"} if n in exact else "chunk" in seen[n], (n, seen[n])
    assert all("row" in seen[n] for n in ("pv_act_forward", "pv_act_backward", "pv_geglu", "pv_geglu_backward", "pv_col_affine_f16", "pv_prelu_f16", "pv_dropout_f16",
                                          "pv_softmax_rows_backward", "pv_pool2x_sum", "pv_layernorm_backward", "pv_wgrad_tn", "pv_cosine_embedding_loss"))


def test_layernorm_backward_without_dy_skip_and_wgrad_without_its_last_row_fail(catalogue):
    """Two defects only these launchers have: the CLS row of each group given a gradient (dy_skip dropped), the single row of the last slab left out."""
    n = 0
    for case, i, p, v, exp in catalogue["pv_layernorm_backward"]:
        if p.dy_group > 1:
            q = SimpleNamespace(**{k: getattr(p, k) for k, _ in type(p._s)._fields_})
            q.dy_skip = 0
            wrong = A.ref_layernorm_backward(q, v)
            got = {k: wrong[k].ref.to(v[k].dtype) for k in exp}
            fails = PA.compare(exp, got)[0]
            assert any("field dx" in f for f in fails), (case, fails)
            assert "dgb_partial" not in exp or any("field dgb_partial" in f for f in fails), (case, fails)
            n += 1
    assert n == 2
    m = 0
    for case, i, p, v, exp in catalogue["pv_wgrad_tn"]:
        if p.nsplit > 1 and p.m - (p.nsplit - 1) * p.rows_per_split == 1:
            got = _as_stored(exp, v)
            assert not PA.compare(exp, got)[0]
            got["out"][p.nsplit - 1] = 0.0                  # the last slab is that one row's outer product
            assert PA.compare(exp, got)[0], case
            m += 1
    assert m == 2


def test_training_caps_are_the_kernel_tests_tolerances():
    """Every new ``CAP`` entry is a tolerance tests/test_hip_kernels.py asserts for the same launcher (none looser), read from that file's own text."""
    src = open(os.path.join(ROOT, "tests", "test_hip_kernels.py")).read()
    for key, lines in {"pointwise_bwd": ("rel_l2(dh.float().cpu(), hr.grad) < 2e-3", "rel_l2(dq_.float().cpu(), want_q) < 2e-3", "rel_l2(ds_.float().cpu(), xr.grad) < 2e-3",
                                         "rel_l2(de_p, 4.0 * e2r.grad) < 2e-3", "rel_l2(dS, 0.3 * Pf * (dPf - (Pf * dPf).sum(-1, keepdim=True))) < 2e-3"),
                       "pointwise16": ("rel_l2(ca, xf * sc + sh) < 1e-3", "rel_l2(pr, torch.where(xf > 0, xf, 0.25 * xf)) < 1e-3", "rel_l2(pl.float().cpu().view(2, 3, 5, 64), pr) < 1e-3"),
                       "gray": ("rel_l2(got, ref.detach()) < 1e-5", "rel_l2(gotb, ir.grad) < 1e-5"),
                       "ln_bwd_dx": ("rel_l2(dx.float(), xr.grad) < 1.5e-3",), "ln_bwd_dgb": ("rel_l2(dgb[0], gr.grad) < 1e-4 and rel_l2(dgb[1], br.grad) < 1e-4",)}.items():
        for line in lines:
            assert line in src, line
            assert A.CAP[key] <= float(line.rsplit("<", 1)[1]), (key, line)
    assert "(dw - ref).norm() / ref.norm() < 2e-6 * max(1.0, (m / 64) ** 0.5)" in src
    for m_ in (7, 64, 65, 1025, 65536):
        assert A.wgrad_cap(m_) == 2e-6 * max(1.0, (m_ / 64) ** 0.5)


def test_training_conditions_hold_on_the_catalogue(catalogue):
    """The conditions the bounds rest on, on the catalogue's seeded inputs: at most 0.5 % of the elements of a LayerNorm backward case sit within their own
    fp32 error of the LeakyReLU branch point (their bounds, their rows' and their blocks' are widened), no cosine lies within its error of 0, and the
    ``__expf`` terms of the SiLU / quick-GELU launches (derived in ``abi_ref``, not measured) stay below a quarter of the fp16 store bound - they cannot
    hide anything an fp16 ulp would show."""
    shares = []
    for case, i, p, v, exp in catalogue["pv_layernorm_backward"]:
        amb = A.ln_bwd_terms(p, v)["amb"]
        shares.append(amb.double().mean().item())
        assert shares[-1] <= 0.005, (case, i, shares[-1])
        assert p.act == 3 or not amb.any()
    assert len(shares) >= 20
    for case, i, p, v, exp in catalogue["pv_cosine_embedding_loss"]:
        assert not A.cosine_ambiguous(p, v).any(), (case, i)
        assert A.cosine_parts(p, v)[6].abs().min() > 0.3
    n = 0
    for name, key in (("pv_act_forward", "y"), ("pv_act_backward", "dx")):
        for case, i, p, v, exp in catalogue[name]:
            if p.act in (1, 2):
                e = exp[key]
                store = A.store_bound(e.ref, torch.float16)
                # forward: against the store bound of y itself; backward: the derivative crosses 0 (SiLU's at x = -1.28) where |dy act'| and its store
                # bound vanish and the term does not - there it is held against the store bound of dy, the output at slope 1
                room = store if name == "pv_act_forward" else torch.maximum(store, A.store_bound(v["dy"].double(), torch.float16))
                assert ((e.bound - store) <= 0.25 * room).all(), (case, i, ((e.bound - store) / room).max().item())
                n += 1
    assert n == 12
