"""GPU parity of every HIP kernel (through the C-ABI) against a plain PyTorch fp32 reference of the same op,
evaluated on the SAME fp16-rounded inputs.  Tolerances: fp16 storage of the result (2^-11 relative) plus fp32
accumulation-order noise; stated per test."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def h16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def test_recorder_holds_a_caller_owned_statistics_buffer(rec_cls):
    """A launch recorded with ``colstats_out`` writes a buffer the caller owns.  Before, the recorder's only reference to it was its
    ``colstats`` table entry, and recording the same output again without statistics drops that entry: a caller that then let the buffer go left
    the first launch writing freed memory.  The recorder now holds every buffer it records by address (in the shipped plans the loop also holds
    it), so the buffer outlives the caller's reference."""
    import gc
    import weakref
    rec = rec_cls("cuda")
    a, w = h16(128, 64, seed=1).cuda(), h16(128, 64, scale=0.1, seed=2).cuda()
    y = torch.empty(128, 128, dtype=torch.float16, device="cuda")
    cs = torch.zeros(2, 2, 128, dtype=torch.float32, device="cuda")
    rec.gemm(a, w, out=y, colstats=True, colstats_out=cs)
    rec.gemm(a, w, out=y)                          # the same output again, without statistics: the table entry goes
    assert (y.data_ptr(), 128, 128) not in rec.colstats
    ref = weakref.ref(cs)
    del cs
    gc.collect()
    held = ref()
    assert held is not None, "the recorded statistics buffer was freed while the plan still writes it"
    rec.run()
    torch.cuda.synchronize()
    yy = y.double().cpu().reshape(2, 64, 128)
    assert torch.allclose(held.double().cpu()[:, 0], yy.sum(1), rtol=1e-5, atol=1e-4)


# small, ragged (M tail) and large-M shapes; K from one K-step to 64 of them
@pytest.mark.parametrize("M,N,K", [(256, 320, 320), (1000, 640, 768), (16, 1280, 1280), (130, 128, 64), (128, 1024, 4096),
                                   (16384, 640, 640), (32700, 320, 64), (8192, 1024, 128),
                                   (65536, 320, 128), (33000, 640, 192), (32768, 512, 64)])
def test_gemm_bias_residual_act(rec_cls, M, N, K):
    from photoverse_amd import ops
    a, w, res = h16(M, K, seed=1), h16(N, K, scale=K ** -0.5, seed=2), h16(M, N, seed=3)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(4))
    for act, fn in ((ops.ACT_NONE, lambda x: x), (ops.ACT_SILU, F.silu), (ops.ACT_QUICK_GELU, lambda x: x * torch.sigmoid(1.702 * x)),
                    (ops.ACT_LEAKY_RELU, lambda x: F.leaky_relu(x, 0.01))):
        rec = rec_cls("cuda")
        out = rec.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), residual=res.cuda(), act=act)
        out32 = rec.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), out_f32=True)
        rec.run()
        torch.cuda.synchronize()
        ref = fn(a.float() @ w.float().t() + bias) + res.float()
        assert rel_l2(out, ref) < 1e-3
        assert rel_l2(out32, a.float() @ w.float().t() + bias) < 2e-5     # fp32 store: accumulation noise only


@pytest.mark.parametrize("M,N,K,S", [(300, 640, 1280, 3), (1024, 1280, 2560, 8), (64, 320, 640, None), (4096, 1280, 1280, None)])
def test_gemm_splitk(rec_cls, M, N, K, S):
    """Small-M layers split the K loop over several workgroups; partial slabs are reduced in a fixed order."""
    from photoverse_amd import ops
    a, w, res = h16(M, K, seed=41), h16(N, K, scale=K ** -0.5, seed=42), h16(M, N, seed=43)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(44))
    temb = torch.randn(2, N, generator=torch.Generator().manual_seed(45))
    rec = rec_cls("cuda")
    out = rec.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), rowadd=temb.cuda(), rowadd_ld=N, rows_per_image=M // 2, residual=res.cuda(),
                   act=ops.ACT_SILU, splitk=S)
    base = rec.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), rowadd=temb.cuda(), rowadd_ld=N, rows_per_image=M // 2, residual=res.cuda(),
                    act=ops.ACT_SILU, splitk=0)
    rec.run()
    first = out.clone()
    rec.run()
    torch.cuda.synchronize()
    ref = F.silu(a.float() @ w.float().t() + bias + temb.repeat_interleave(M // 2, 0)) + res.float()
    assert rel_l2(out, ref) < 1e-3 and rel_l2(base, ref) < 1e-3
    assert torch.equal(out, first)                       # deterministic (no atomics)


def test_gemm_dual_source_and_strided(rec_cls):
    M, c0, c1, N = 300, 320, 640, 320
    big0, big1 = h16(M, c0 + 64, seed=5).cuda(), h16(M, c1 + 128, seed=6).cuda()
    a0, a1 = big0[:, :c0], big1[:, 128:]                      # strided row views
    w = h16(N, c0 + c1, scale=0.03, seed=7)
    outbuf = torch.zeros(M, N + 160, dtype=torch.float16, device="cuda")
    rec = rec_cls("cuda")
    rec.gemm(a0, w.cuda(), a1=a1, out=outbuf[:, 160:])
    rec.run()
    torch.cuda.synchronize()
    ref = torch.cat([a0.float().cpu(), a1.float().cpu()], 1) @ w.float().t()
    assert rel_l2(outbuf[:, 160:], ref) < 1e-3
    assert outbuf[:, :160].abs().max().item() == 0.0


def test_gemm_geglu_fused_matches_unfused(rec_cls):
    from photoverse_amd.ops import pack_geglu
    M, C = 200, 320
    x, w = h16(M, C, seed=8), h16(8 * C, C, scale=C ** -0.5, seed=9)
    b = torch.randn(8 * C, generator=torch.Generator().manual_seed(10))
    wp, bp = pack_geglu(w.cuda(), b.cuda())
    rec = rec_cls("cuda")
    fused = rec.gemm(x.cuda(), wp, bias=bp, geglu=True)
    proj = rec.gemm(x.cuda(), w.cuda(), bias=b.cuda())
    unf = rec.geglu(proj)
    rec.run()
    torch.cuda.synchronize()
    h, g = (x.float() @ w.float().t() + b).chunk(2, dim=-1)
    ref = h * F.gelu(g)
    assert rel_l2(fused, ref) < 1e-3
    assert rel_l2(unf, ref) < 2e-3          # extra fp16 rounding of the projection


@pytest.mark.parametrize("cin,cout,h,stride,ups,B", [(320, 320, 16, 1, 0, 2), (640, 320, 8, 1, 0, 2), (320, 320, 16, 2, 0, 2),
                                                     (320, 640, 8, 1, 1, 2), (64, 128, 5, 1, 0, 2),
                                                     (64, 320, 64, 1, 0, 8), (128, 128, 32, 1, 1, 4),
                                                     (1280, 1280, 8, 1, 0, 4), (640, 1280, 8, 2, 0, 2),   # split-K heuristic
                                                     (64, 320, 64, 1, 0, 16), (128, 256, 64, 1, 0, 8)])   # M = 65536 / 32768
def test_conv3x3(rec_cls, cin, cout, h, stride, ups, B):
    x = h16(B, cin, h, h, seed=11)
    w = h16(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=12)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(13))
    temb = torch.randn(B, cout, generator=torch.Generator().manual_seed(14))
    ho = h * 2 if ups else (h // 2 if stride == 2 else h)
    res = h16(B * ho * ho, cout, seed=15)
    xin = x.permute(0, 2, 3, 1).reshape(B * h * h, cin).contiguous().cuda()
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda()
    rec = rec_cls("cuda")
    out = rec.gemm(xin, wp, bias=bias.cuda(), rowadd=temb.cuda(), rowadd_ld=cout, residual=res.cuda(),
                   conv=dict(batch=B, hin=h, win=h, hout=ho, wout=ho, stride=stride, upsample=ups))
    rec.run()
    torch.cuda.synchronize()
    xr = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xr, w.float(), bias, stride=stride, padding=1) + temb[:, :, None, None]
    ref = ref.permute(0, 2, 3, 1).reshape(B * ho * ho, cout) + res.float()
    assert rel_l2(out, ref) < 1e-3


@pytest.mark.parametrize("cin,cout,h,B", [(128, 128, 16, 2), (256, 256, 10, 3), (64, 320, 32, 2)])
def test_conv3x3_stride2_asymmetric_pad(rec_cls, cin, cout, h, B):
    """pad=0: the VAE encoder's Downsample2D = F.pad(x,(0,1,0,1)) + Conv2d(3x3, stride 2, padding 0)."""
    x = h16(B, cin, h, h, seed=61)
    w = h16(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=62)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(63))
    ho = h // 2
    rec = rec_cls("cuda")
    out = rec.gemm(x.permute(0, 2, 3, 1).reshape(B * h * h, cin).contiguous().cuda(), w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(),
                   bias=bias.cuda(), conv=dict(batch=B, hin=h, win=h, hout=ho, wout=ho, stride=2, pad=0))
    rec.run()
    torch.cuda.synchronize()
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), bias, stride=2, padding=0)
    assert ref.shape[-1] == ho
    assert rel_l2(out, ref.permute(0, 2, 3, 1).reshape(B * ho * ho, cout)) < 1e-3
    with pytest.raises(AssertionError):          # pad=0 exists for that one layer type only
        rec_cls("cuda").gemm(x.permute(0, 2, 3, 1).reshape(B * h * h, cin).contiguous().cuda(), w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(),
                             conv=dict(batch=B, hin=h, win=h, hout=h, wout=h, stride=1, pad=0))


def test_conv3x3_dual_source(rec_cls):
    B, c0, c1, cout, h = 2, 320, 640, 320, 8
    x0, x1 = h16(B, c0, h, h, seed=16), h16(B, c1, h, h, seed=17)
    w = h16(cout, c0 + c1, 3, 3, scale=0.01, seed=18)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * h * h, -1).contiguous().cuda()
    rec = rec_cls("cuda")
    out = rec.gemm(rows(x0), w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(), a1=rows(x1),
                   conv=dict(batch=B, hin=h, win=h, hout=h, wout=h))
    rec.run()
    torch.cuda.synchronize()
    ref = F.conv2d(torch.cat([x0, x1], 1).float(), w.float(), padding=1).permute(0, 2, 3, 1).reshape(B * h * h, cout)
    assert rel_l2(out, ref) < 1e-3


def test_conv3x3_dual_source_big_tile(rec_cls):
    B, c0, c1, cout, h = 16, 64, 128, 320, 64
    x0, x1 = h16(B, c0, h, h, seed=51), h16(B, c1, h, h, seed=52)
    w = h16(cout, c0 + c1, 3, 3, scale=0.02, seed=53)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * h * h, -1).contiguous().cuda()
    rec = rec_cls("cuda")
    out = rec.gemm(rows(x0), w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(), a1=rows(x1),
                   conv=dict(batch=B, hin=h, win=h, hout=h, wout=h))
    rec.run()
    torch.cuda.synchronize()
    ref = F.conv2d(torch.cat([x0, x1], 1).float(), w.float(), padding=1).permute(0, 2, 3, 1).reshape(B * h * h, cout)
    assert rel_l2(out, ref) < 1e-3


@pytest.mark.parametrize("M,N,K,geglu", [(65536, 320, 1280, False), (16384, 1920, 640, False), (8192 + 100, 3840, 1280, False), (16384, 5120, 640, True),
                                          (4096 + 40, 10240, 1280, True)])
def test_linear_on_the_256_row_tile_equals_the_128_row_kernel_bitwise(rec_cls, monkeypatch, M, N, K, geglu):
    """The Linear / GEGLU modes of pv_convbig.hip's staggered 256-row tile (K >= 640: ff2 of the 64 x 64 level, fused qkv and the GEGLU projections
    of the 32 x 32 / 16 x 16 levels) vs fp32 torch and, bit for bit, vs pv_gemm.hip's 128-row kernel (same MFMA, same K order); bias + residual +
    column statistics on the plain form, the value * gelu(gate) epilogue on 256-column tiles, ragged M."""
    from photoverse_amd.ops import pack_geglu
    x = h16(M, K, seed=150)
    w = h16(N, K, scale=K ** -0.5, seed=151)
    b = torch.randn(N, generator=torch.Generator().manual_seed(152))
    res = None if geglu else h16(M, N, seed=153)
    dx, dw, db = x.cuda(), w.cuda(), b.cuda()
    if geglu:
        dw, db = pack_geglu(dw, db)
    outs, stats = {}, {}
    for name, env in (("big", "1"), ("small", "0")):
        monkeypatch.setenv("PV_CONV_BIG", env)
        rec = rec_cls("cuda")
        outs[name] = rec.gemm(dx, dw, bias=db, residual=None if res is None else res.cuda(), geglu=geglu, colstats=not geglu and M % 64 == 0, splitk=0)
        assert rec.tags[-1][0].startswith("big_tile_kernel" if name == "big" else "gemm_conv_kernel"), rec.tags[-1]
        stats[name] = rec.colstats.get((outs[name].data_ptr(), M, N))
        rec.run()
        torch.cuda.synchronize()
    y = x.float() @ w.float().t() + b
    ref = y[:, :N // 2] * F.gelu(y[:, N // 2:]) if geglu else y + res.float()
    assert rel_l2(outs["big"], ref) < 1e-3
    assert torch.equal(outs["big"], outs["small"])
    if stats["small"] is not None:
        assert torch.equal(stats["big"], stats["small"])


@pytest.mark.parametrize("M,N,K,geglu", [(16384, 1920, 640, False), (8192 + 72, 3840, 1280, False), (16384, 5120, 640, True), (4096 + 40, 10240, 1280, True)])
def test_layernorm_folded_into_the_linear_behind_it(rec_cls, monkeypatch, M, N, K, geglu):
    """pv_gemm_params.ln_rowsum (ABI 12): norm1 -> fused qkv and norm3 -> GEGLU projection of the 32 x 32 / 16 x 16 transformer blocks as ONE launch on
    the 256-row tile - the GEMM runs on the raw rows, the row statistics come from the MFMA fragments, the epilogue applies
    rstd * (acc - mean * rowsum(W)) - vs fp32 torch and vs the two launches it replaces (LayerNorm, GEMM); large row means exercise the cancellation."""
    from photoverse_amd import ops
    from photoverse_amd.ops import pack_geglu
    monkeypatch.setattr(ops.Recorder, "GEMM_LN", True)          # (off by default: measured neutral-to-negative in the loop; the entry point stays tested)
    x = h16(M, K, seed=160)
    x[:, ::5] += 1.0
    x[: M // 2] += 3.0
    w = h16(N, K, scale=K ** -0.5, seed=161)
    b = torch.randn(N, generator=torch.Generator().manual_seed(162))
    gamma = 1.0 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(163))
    beta = 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(164))
    assert ops.Recorder.gemm_ln_supported(M, N, K, geglu)
    rec = rec_cls("cuda")
    dx, dw, db = x.cuda(), w.cuda(), b.cuda()
    wl, bl = ops.Recorder.fold_layernorm(dw, db, gamma, beta)
    if geglu:
        wl, bl = pack_geglu(wl, bl)
    out = rec.gemm(dx, wl, bias=bl, geglu=geglu, ln_gamma=True, splitk=0)
    assert rec.tags[-1][0].startswith("big_tile_kernel") and rec.tags[-1][0].endswith("true>"), rec.tags[-1]
    n1 = rec.layernorm(dx, gamma.cuda(), beta.cuda())
    w2, b2 = pack_geglu(dw, db) if geglu else (dw, db)
    two = rec.gemm(n1, w2, bias=b2, geglu=geglu, splitk=0)
    rec.run()
    torch.cuda.synchronize()
    y = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.float().t() + b
    ref = y[:, :N // 2] * F.gelu(y[:, N // 2:]) if geglu else y
    e1, e2 = rel_l2(out, ref), rel_l2(two, ref)
    print(f"LayerNorm folded into the Linear M={M} N={N} K={K} geglu={geglu}: vs fp32 {e1:.2e} (two launches: {e2:.2e})")
    assert torch.isfinite(out).all() and e1 < 1e-3 and e2 < 1e-3 and rel_l2(out, two) < 1e-3


@pytest.mark.parametrize("B,c0,c1,cout,hin,splitk", [(4, 64, 0, 320, 32, None), (2, 64, 64, 640, 16, None), (8, 1280, 0, 1280, 16, 4), (2, 640, 640, 320, 16, 2)])
def test_conv3x3_256x320_tile_upsample_and_splitk(rec_cls, monkeypatch, B, c0, c1, cout, hin, splitk):
    """The x2-upsampling gather of pv_convbig.hip (source pixel of tap (ky, kx) = ((y + ky - 1) >> 1, (x + kx - 1) >> 1), selected per lane from the
    output coordinate's parity) and its split-K form (fp32 slabs, pv_gemm.hip's K partition and reduce launch) vs fp32 torch and, bit for bit, vs
    the 128-row kernel."""
    ups = splitk is None
    x0 = h16(B, c0, hin, hin, seed=91)
    x1 = h16(B, c1, hin, hin, seed=92) if c1 else None
    w = h16(cout, c0 + c1, 3, 3, scale=(9 * (c0 + c1)) ** -0.5, seed=93)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(94))
    ho = hin * 2 if ups else hin
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * hin * hin, -1).contiguous().cuda()
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda()
    outs, stats = {}, {}
    for name, env in (("big", "1"), ("small", "0")):
        monkeypatch.setenv("PV_CONV_BIG", env)
        rec = rec_cls("cuda")
        outs[name] = rec.gemm(rows(x0), wp, a1=rows(x1) if c1 else None, bias=bias.cuda(), colstats=True, splitk=splitk,
                              conv=dict(batch=B, hin=hin, win=hin, hout=ho, wout=ho, upsample=int(ups)))
        assert rec.tags[-1][0].startswith("big_tile_kernel" if name == "big" else "gemm_conv_kernel"), rec.tags[-1]
        stats[name] = rec.colstats.get((outs[name].data_ptr(), B * ho * ho, cout))
        rec.run()
        torch.cuda.synchronize()
    xin = torch.cat([x0, x1], 1).float() if c1 else x0.float()
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.float(), bias, padding=1).permute(0, 2, 3, 1).reshape(B * ho * ho, cout)
    assert rel_l2(outs["big"], ref) < 1e-3
    assert torch.equal(outs["big"], outs["small"])
    assert stats["big"] is not None and torch.equal(stats["big"], stats["small"])


@pytest.mark.parametrize("B,c0,c1,cout,h,extras", [(16, 64, 0, 320, 64, True), (16, 128, 64, 320, 64, False), (8, 64, 0, 640, 64, True), (1, 64, 0, 320, 24, True)])
def test_conv3x3_256x320_tile_equals_the_128_row_kernel_bitwise(rec_cls, monkeypatch, B, c0, c1, cout, h, extras):
    """pv_convbig.hip (256 x 320 x 64 tile, one 8-wave workgroup per CU: the 3x3 convs of the 64 x 64 level) against fp32 torch AND, bit for bit,
    against the 128 x 160 kernel it replaces (same MFMA, same K order, same rounding points): single and dual source, N = 320 / 640,
    bias + time-embedding row + residual + SiLU epilogue, GroupNorm column statistics, and an M tail (one 24 x 24 image: 576 rows = 2.25 tiles, run on
    the big tile by lowering its minimum tile count)."""
    from photoverse_amd.ops import ACT_SILU
    monkeypatch.setenv("PV_CONV_PATCH", "0")                 # the GATHERED form of the tile (the LDS-resident patch has its own K order: next test)
    x0 = h16(B, c0, h, h, seed=81)
    x1 = h16(B, c1, h, h, seed=82) if c1 else None
    w = h16(cout, c0 + c1, 3, 3, scale=(9 * (c0 + c1)) ** -0.5, seed=83)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(84))
    temb = torch.randn(B, cout, generator=torch.Generator().manual_seed(85))
    res = h16(B * h * h, cout, seed=86)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * h * h, -1).contiguous().cuda()
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda()
    kw = dict(bias=bias.cuda(), conv=dict(batch=B, hin=h, win=h, hout=h, wout=h), colstats=True)
    if extras:
        kw.update(rowadd=temb.cuda(), rowadd_ld=cout, residual=res.cuda(), act=ACT_SILU)
    outs, stats = {}, {}
    for name, env in (("big", "1"), ("small", "0")):
        monkeypatch.setenv("PV_CONV_BIG", env)
        rec = rec_cls("cuda")
        outs[name] = rec.gemm(rows(x0), wp, a1=rows(x1) if c1 else None, **kw)
        stats[name] = rec.colstats.get((outs[name].data_ptr(), B * h * h, cout))
        rec.run()
        torch.cuda.synchronize()
    xin = torch.cat([x0, x1], 1).float() if c1 else x0.float()
    ref = F.conv2d(xin, w.float(), bias, padding=1)
    if extras:
        ref = F.silu(ref + temb[:, :, None, None])
    ref = ref.permute(0, 2, 3, 1).reshape(B * h * h, cout)
    if extras:
        ref = ref + res.float()
    assert rel_l2(outs["big"], ref) < 1e-3
    assert torch.equal(outs["big"], outs["small"])
    assert stats["big"] is not None and torch.equal(stats["big"], stats["small"])
    # the statistics are those of the stored (rounded) values: per 64-row block column sums
    blk = outs["big"].float().view(-1, 64, cout)
    torch.testing.assert_close(stats["big"].view(-1, 2, cout)[:, 0], blk.sum(1), rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(stats["big"].view(-1, 2, cout)[:, 1], (blk * blk).sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("B,c0,c1,cout,h,pmode", [(16, 320, 0, 320, 64, "64"), (16, 640, 320, 320, 64, "64"), (2, 128, 128, 640, 64, "64"), (16, 640, 0, 640, 32, "1"),
                                                   (1, 128, 0, 320, 64, "64")])
def test_groupnorm_silu_folded_into_the_patch_conv(rec_cls, monkeypatch, B, c0, c1, cout, h, pmode):
    """pv_gemm_params.a_norm (ABI 15): ResnetBlock2D.norm1 / norm2 + SiLU folded into conv1 / conv2 where the conv runs on the LDS-resident input patch -
    pv_groupnorm_scale_shift turns the producers' column statistics into a per-(image, channel) scale / shift table, the conv reads the RAW tensor(s) and
    normalises each staged pixel once, in LDS, with pv_groupnorm_apply's arithmetic.  Against fp32 torch (group_norm -> silu -> conv2d) and, BIT FOR BIT,
    against the two launches it replaces (GroupNorm-apply, then the same patch conv on the normalised tensor): single / dual source (the norm spans the
    concatenation), image borders (padding stays zero, not silu(shift)), W = 64 and 32, column statistics of the output."""
    from photoverse_amd.ops import ACT_SILU
    monkeypatch.setenv("PV_CONV_PATCH", pmode)
    monkeypatch.setattr(rec_cls, "GN_FOLD", True)            # (off by default: break-even alone, -0.5 % in the loop; the entry point stays tested)
    C = c0 + c1
    g = torch.Generator().manual_seed(300 + C)
    # the inputs are themselves conv outputs in the plan (that is where their column statistics come from): produce them with a 1x1 GEMM here
    src0, src1 = h16(B * h * h, 64, seed=301), h16(B * h * h, 64, seed=302)
    wp0, wp1 = h16(c0, 64, scale=0.2, seed=303), (h16(c1, 64, scale=0.3, seed=304) if c1 else None)
    b0 = torch.randn(c0, generator=g) * 0.5
    w = h16(cout, C, 3, 3, scale=(9 * C) ** -0.5, seed=305)
    bias = torch.randn(cout, generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    wpk = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda()
    geo = dict(batch=B, hin=h, win=h, hout=h, wout=h)
    rec = rec_cls("cuda")
    rec.big_min = 1
    x0 = rec.gemm(src0.cuda(), wp0.cuda(), bias=b0.cuda(), rows_per_image=h * h, colstats=True, splitk=0)
    x1 = rec.gemm(src1.cuda(), wp1.cuda(), rows_per_image=h * h, colstats=True, splitk=0) if c1 else None
    assert rec_cls.gn_conv_supported((B, h, h, h, h, 1, 0, 1), B * h * h, cout, c0, c1, rec.big_min)
    tab = rec.groupnorm_table(x0, gamma.cuda(), beta.cuda(), batch=B, hw=h * h, x1=x1)
    assert tab is not None
    fused = rec.gemm(x0, wpk, a1=x1, bias=bias.cuda(), conv=geo, colstats=True, a_norm=tab, a_norm_act=ACT_SILU, splitk=0)
    want_mode = 5 if h == 64 else 6
    assert rec.tags[-1][0] == f"big_tile_kernel<true, false, 8, {want_mode}, false>", rec.tags[-1]
    cs_f = rec.colstats[(fused.data_ptr(), B * h * h, cout)]
    hn = rec.groupnorm(x0, gamma.cuda(), beta.cuda(), batch=B, hw=h * h, x1=x1, act=ACT_SILU)
    two = rec.gemm(hn, wpk, bias=bias.cuda(), conv=geo, colstats=True, splitk=0)
    assert rec.tags[-1][0] == f"big_tile_kernel<true, false, 8, {want_mode - 2}, false>", rec.tags[-1]
    cs_t = rec.colstats[(two.data_ptr(), B * h * h, cout)]
    rec.run()
    torch.cuda.synchronize()
    xin = torch.cat([x0.float().cpu(), x1.float().cpu()], 1) if c1 else x0.float().cpu()
    xin = xin.view(B, h, h, C).permute(0, 3, 1, 2)
    ref = F.conv2d(F.silu(F.group_norm(xin, 32, gamma, beta, 1e-5)), w.float(), bias, padding=1).permute(0, 2, 3, 1).reshape(B * h * h, cout)
    e_f, e_t = rel_l2(fused, ref), rel_l2(two, ref)
    print(f"GroupNorm + SiLU folded into the patch conv ({c0}+{c1} -> {cout} @ {h}): vs fp32 {e_f:.2e} (two launches {e_t:.2e}), fused == two launches: {torch.equal(fused, two)}")
    assert e_f < 1.5e-3 and e_t < 1.5e-3
    assert torch.equal(fused, two) and torch.equal(cs_f, cs_t)


@pytest.mark.parametrize("B,c0,c1,cout,h,extras,pmode", [(16, 320, 0, 320, 64, True, "64"), (16, 640, 320, 320, 64, False, "64"), (4, 64, 64, 640, 64, True, "64"),
                                                          (16, 640, 0, 640, 32, True, "1"), (2, 64, 64, 320, 32, False, "1"), (1, 64, 0, 320, 64, True, "64")])
def test_conv3x3_lds_resident_input_patch(rec_cls, monkeypatch, B, c0, c1, cout, h, extras, pmode):
    """pv_convbig.hip MODE 3 / 4 (round 5): the tile's 256 output pixels are whole image rows, the (R + 2) x (W + 2) input pixels of a 32-channel chunk are
    staged ONCE in LDS and the nine taps read them at shifted addresses (chunk ^ 2 * ((pixel >> 2) & 1): conflict-free at any pixel alignment) instead of
    gathering 256 shifted rows per tap.  Against fp32 conv2d and against the gathered form of the same tile (same products, 32-channel-chunk-major K order:
    equal to fp32 accumulation order, not to the bit): single / dual source, N = 320 / 640, image borders, bias + time-embedding row + residual + SiLU,
    GroupNorm column statistics; W = 64 (default) and W = 32 (PV_CONV_PATCH=1); small launches are put on the tile by lowering its minimum tile count."""
    from photoverse_amd.ops import ACT_SILU
    x0 = h16(B, c0, h, h, seed=181)
    x1 = h16(B, c1, h, h, seed=182) if c1 else None
    w = h16(cout, c0 + c1, 3, 3, scale=(9 * (c0 + c1)) ** -0.5, seed=183)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(184))
    temb = torch.randn(B, cout, generator=torch.Generator().manual_seed(185))
    res = h16(B * h * h, cout, seed=186)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * h * h, -1).contiguous().cuda()
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda()
    kw = dict(bias=bias.cuda(), conv=dict(batch=B, hin=h, win=h, hout=h, wout=h), colstats=True)
    if extras:
        kw.update(rowadd=temb.cuda(), rowadd_ld=cout, residual=res.cuda(), act=ACT_SILU)
    outs, stats = {}, {}
    for name, env in (("patch", pmode), ("gathered", "0")):
        monkeypatch.setenv("PV_CONV_PATCH", env)             # read at record time (the tag) and at launch time (the kernel): set around both
        rec = rec_cls("cuda")
        rec.big_min = 1
        outs[name] = rec.gemm(rows(x0), wp, a1=rows(x1) if c1 else None, **kw)
        want_mode = (3 if h == 64 else 4) if name == "patch" else 0
        assert rec.tags[-1][0] == f"big_tile_kernel<true, false, 8, {want_mode}, false>", rec.tags[-1]
        stats[name] = rec.colstats.get((outs[name].data_ptr(), B * h * h, cout))
        rec.run()
        torch.cuda.synchronize()
    xin = torch.cat([x0, x1], 1).float() if c1 else x0.float()
    ref = F.conv2d(xin, w.float(), bias, padding=1)
    if extras:
        ref = F.silu(ref + temb[:, :, None, None])
    ref = ref.permute(0, 2, 3, 1).reshape(B * h * h, cout)
    if extras:
        ref = ref + res.float()
    assert rel_l2(outs["patch"], ref) < 1e-3 and rel_l2(outs["gathered"], ref) < 1e-3
    assert rel_l2(outs["patch"], outs["gathered"]) < 1e-4 and rel_l2(stats["patch"], stats["gathered"]) < 1e-4


@pytest.mark.parametrize("c0,c1,hw,act", [(320, 0, 64 * 64, 1), (640, 320, 16 * 16, 1), (1280, 1280, 64, 0), (2560, 0, 64, 1), (64, 0, 25, 0)])
def test_groupnorm(rec_cls, c0, c1, hw, act):
    B = 2
    C = c0 + c1
    x = h16(B, hw, C, seed=19) * 2 + 0.5
    gamma = torch.randn(C, generator=torch.Generator().manual_seed(20))
    beta = torch.randn(C, generator=torch.Generator().manual_seed(21))
    xr = x.reshape(B * hw, C).cuda()
    rec = rec_cls("cuda")
    y = rec.groupnorm(xr[:, :c0], gamma.cuda(), beta.cuda(), batch=B, hw=hw, x1=(xr[:, c0:] if c1 else None), eps=1e-5, act=act)
    rec.run()
    torch.cuda.synchronize()
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    if act:
        ref = F.silu(ref)
    assert rel_l2(y, ref.reshape(B * hw, C)) < 1e-3


@pytest.mark.parametrize("c0,c1,cout,h,B", [(320, 0, 320, 16, 2), (64, 0, 128, 8, 3), (640, 320, 320, 16, 2), (128, 0, 320, 24, 1)])
def test_groupnorm_from_gemm_column_statistics(rec_cls, c0, c1, cout, h, B):
    """The GEMM / conv epilogue leaves per-64-row-block column (sum, sumsq) behind (pv_gemm_params.colstats) and GroupNorm takes
    its statistics from them: same result as the pass over the tensor, on single- and dual-source (skip concat) inputs."""
    hw = h * h
    g = torch.Generator().manual_seed(70 + c0 + h)
    gamma, beta = torch.randn(cout + (cout if c1 else 0), generator=g), torch.randn(cout + (cout if c1 else 0), generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * hw, -1).contiguous().cuda()
    xa = h16(B, c0, h, h, seed=71)
    wa = h16(cout, c0, 3, 3, scale=(9 * c0) ** -0.5 * 3, seed=72)
    res = h16(B * hw, cout, seed=73)
    rec = rec_cls("cuda")
    ya = rec.gemm(rows(xa), wa.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(), bias=torch.ones(cout).cuda(), residual=res.cuda(),
                  conv=dict(batch=B, hin=h, win=h, hout=h, wout=h), colstats=True, splitk=0)   # (split-K launches have no statistics)
    yb = None
    if c1:   # second source: a 1x1 GEMM output (like a skip tensor written by proj_out)
        xb = h16(B * hw, c1, seed=74)
        yb = rec.gemm(xb.cuda(), h16(cout, c1, scale=c1 ** -0.5, seed=75).cuda(), rows_per_image=hw, colstats=True, splitk=0)
    out = rec.groupnorm(ya, gamma.cuda(), beta.cuda(), batch=B, hw=hw, x1=yb, eps=1e-5, act=1)
    names = [fn.__name__ for fn, _ in rec.calls]
    assert ("pv_groupnorm_stats_from_colstats" in names) == (hw % 64 == 0) and ("pv_groupnorm_stats" in names) == (hw % 64 != 0)
    rec.run()
    torch.cuda.synchronize()
    # the statistics themselves
    cs = rec.colstats[(ya.data_ptr(), B * hw, cout)].cpu()
    yf = ya.float().cpu()
    nblk = (B * hw + 63) // 64
    pad = torch.zeros(nblk * 64, cout); pad[:B * hw] = yf
    blocks = pad.view(nblk, 64, cout)
    assert torch.allclose(cs[:, 0], blocks.sum(1), rtol=1e-4, atol=1e-3)
    assert torch.allclose(cs[:, 1], (blocks * blocks).sum(1), rtol=1e-4, atol=1e-3)
    # GroupNorm of the stored tensors
    x_all = torch.cat([yf] + ([yb.float().cpu()] if c1 else []), 1).view(B, hw, -1).permute(0, 2, 1)
    ref = F.silu(F.group_norm(x_all, 32, gamma, beta, 1e-5)).permute(0, 2, 1).reshape(B * hw, -1)
    assert rel_l2(out, ref) < 1e-3
    # a buffer rewritten without statistics falls back to the pass over the tensor
    rec2 = rec_cls("cuda")
    y2 = rec2.gemm(rows(xa), wa.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(), conv=dict(batch=B, hin=h, win=h, hout=h, wout=h), colstats=True, splitk=0)
    assert rec2.colstats
    rec2.gemm(rows(xa), wa.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().cuda(), conv=dict(batch=B, hin=h, win=h, hout=h, wout=h), out=y2)
    rec2.groupnorm(y2, gamma[:cout].cuda(), beta[:cout].cuda(), batch=B, hw=hw)
    assert "pv_groupnorm_stats_from_colstats" not in [fn.__name__ for fn, _ in rec2.calls]


@pytest.mark.parametrize("cols", [320, 640, 768, 1024, 1280])
def test_layernorm(rec_cls, cols):
    rows = 77
    x = h16(rows, cols, seed=22) * 3 + 1
    gamma = torch.randn(cols, generator=torch.Generator().manual_seed(23))
    beta = torch.randn(cols, generator=torch.Generator().manual_seed(24))
    rec = rec_cls("cuda")
    y = rec.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), eps=1e-5)
    y2 = rec.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), eps=1e-5, act=3)
    rec.run()
    torch.cuda.synchronize()
    ref = F.layer_norm(x.float(), (cols,), gamma, beta, 1e-5)
    assert rel_l2(y, ref) < 1e-3
    assert rel_l2(y2, F.leaky_relu(ref, 0.01)) < 1e-3


@pytest.mark.parametrize("d,n,causal", [(40, 1024, False), (80, 256, False), (160, 64, False), (160, 256, False), (64, 257, False),
                                         (64, 77, True), (40, 100, False)])
def test_self_attention(rec_cls, d, n, causal):
    B, H = 2, 8
    C = H * d
    qkv = h16(B * n, 3 * C, seed=25)
    dev = qkv.cuda()
    rec = rec_cls("cuda")
    out = rec.attention(dev[:, :C], dev[:, C:2 * C], dev[:, 2 * C:], batch=B, heads=H, nq=n, nk=n, d=d, causal=causal)
    rec.run()
    torch.cuda.synchronize()
    q, k, v = [t.float().view(B, n, H, d).transpose(1, 2) for t in qkv.split(C, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(B * n, C)
    assert rel_l2(out, ref) < 2e-3           # P is rounded to fp16 before the second product


def test_self_attention_spiky_rows(rec_cls):
    """Forces the online-softmax rescale: one key far above the rest, late in the sequence."""
    B, H, d, n = 1, 8, 40, 512
    C = H * d
    qkv = h16(B * n, 3 * C, seed=26)
    qkv[300, C:2 * C] *= 12.0
    dev = qkv.cuda()
    rec = rec_cls("cuda")
    out = rec.attention(dev[:, :C], dev[:, C:2 * C], dev[:, 2 * C:], batch=B, heads=H, nq=n, nk=n, d=d)
    rec.run()
    torch.cuda.synchronize()
    q, k, v = [t.float().view(B, n, H, d).transpose(1, 2) for t in qkv.split(C, dim=1)]
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * n, C)
    assert torch.isfinite(out).all()
    assert rel_l2(out, ref) < 2e-3


def _attn40(rec_cls, qkv, B, H, n, lse=False):
    C = H * 40
    dev = qkv.cuda()
    rec = rec_cls("cuda")
    l = rec.empty((B, H, n), torch.float32) if lse else None
    out = rec.attention(dev[:, :C], dev[:, C:2 * C], dev[:, 2 * C:], batch=B, heads=H, nq=n, nk=n, d=40, lse=l)
    rec.run()
    torch.cuda.synchronize()
    return out.cpu(), (l.cpu() if lse else None)


@pytest.mark.parametrize("var", [1, 9, 225, 497])
@pytest.mark.parametrize("n", [1536, 1000, 100, 64])
def test_self_attention_8wave_staggered_forms(rec_cls, monkeypatch, var, n):
    """attn8_kernel (pv_attn.hip: one 512-query workgroup of eight waves, SIMD partners staggered by one barrier interval) in the forms the
    build ships: 1 = the eager online softmax (round 4's arithmetic) in the staggered structure; 9 = lazy softmax reference, decided per query fragment -
    the 4-wave kernel's arithmetic, BIT-IDENTICAL to it; 225 / 497 (default) = exponentiate-first reference check, V prefetch, 48-deep score contraction
    (497: + per-segment priorities, LDS-DMA issued behind the prefetch reads).  Ragged sizes (query and key
    tails), one- and two-tile sequences, the log-sum-exp output the training backward reads, and a late dominant key (forces the reference
    move long after the first tile: the path that goes back to the scores in 225 / 241)."""
    B, H, d = 2, 8, 40
    C = H * d
    qkv = h16(B * n, 3 * C, seed=225 + n)
    spiky = qkv.clone()
    spiky[(n * 3) // 5, C:2 * C] *= 12.0
    monkeypatch.setenv("PV_ATTN8_MIN", "1")                  # these launches are far below one workgroup per CU: take the 8-wave form anyway
    res = {}
    for v in (-1, var):
        monkeypatch.setenv("PV_ATTN8", str(v))
        res[v] = [_attn40(rec_cls, t, B, H, n, lse=True) for t in (qkv, spiky)]
    for k, t in enumerate((qkv, spiky)):
        q, kk, vv = [x.float().view(B, n, H, d).transpose(1, 2) for x in t.split(C, dim=1)]
        ref = F.scaled_dot_product_attention(q, kk, vv).transpose(1, 2).reshape(B * n, C)
        out, lse = res[var][k]
        assert torch.isfinite(out).all()
        assert rel_l2(out, ref) < 2e-3
        want_lse = torch.logsumexp((q @ kk.transpose(-1, -2)) / d ** 0.5, -1) / math.log(2.0)
        assert (lse - want_lse).abs().max() < 2e-2
        if var == 9:
            assert torch.equal(out, res[-1][k][0]) and torch.equal(lse, res[-1][k][1])
        else:
            assert rel_l2(out, res[-1][k][0]) < 1e-3


@pytest.mark.parametrize("d,n,p,wt,wi", [(40, 4096, 1, 1.0, 1.0), (80, 1024, 5, 1.0, 1.0), (160, 256, 6, 1.0, 1.0), (160, 64, 1, 2.0, 0.0),
                                          (40, 200, 5, 0.0, 2.0), (80, 64, 16, 1.0, 1.0)])
def test_cross_attention_dual_branch(rec_cls, d, n, p, wt, wi):
    B, H, NT = 2, 8, 77
    C = H * d
    q, kvt, kvip = h16(B * n, C, seed=27), h16(B * NT, 2 * C, seed=28), h16(B * p, 2 * C, seed=29)
    dq, dt, di = q.cuda(), kvt.cuda(), kvip.cuda()
    vn = torch.zeros(B, H, p, device="cuda")
    rec = rec_cls("cuda")
    out, _ = rec.cross_attention(dq, dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], batch=B, heads=H, nq=n, nt=NT, nip=p, d=d,
                                 w_text=wt, w_ip=wi, vnorm=vn)
    rec.run()
    torch.cuda.synchronize()
    hv = lambda t, m: t.float().view(B, m, H, d).transpose(1, 2)
    qq = hv(q, n)
    ot = F.scaled_dot_product_attention(qq, hv(kvt[:, :C], NT), hv(kvt[:, C:], NT))
    vip = hv(kvip[:, C:], p)
    oi = F.scaled_dot_product_attention(qq, hv(kvip[:, :C], p), vip)
    ref = (wt * ot + wi * oi).transpose(1, 2).reshape(B * n, C)
    assert rel_l2(out, ref) < 2e-3
    torch.testing.assert_close(vn.cpu(), vip.norm(dim=-1), rtol=1e-4, atol=1e-4)     # to_v_ip_norm, attention_processor.py:397


@pytest.mark.parametrize("d,n,p,wt,wi,ln,fus", [(40, 4096, 1, 1.0, 1.0, True, False), (40, 128, 5, 1.0, 1.0, True, False),
                                               (40, 256, 6, 2.0, 0.0, False, False), (40, 128, 16, 0.0, 2.0, True, True),
                                               (80, 1024, 1, 1.0, 1.0, True, False), (80, 128, 5, 1.0, 1.0, True, False),
                                               (80, 256, 6, 2.0, 0.0, False, False), (80, 128, 16, 0.0, 2.0, True, True)])
def test_cross_attention_fused_branch(rec_cls, d, n, p, wt, wi, ln, fus):
    """pv_cross_attention_fused (norm2 -> to_q -> dual-branch SDPA -> to_out + bias + residual in ONE launch; the C = 320 / d = 40 and
    C = 640 / d = 80 instantiations) vs an fp32 torch reference on the same fp16-rounded operands, and vs the four-launch path it replaces."""
    from photoverse_amd import ops
    B, H, NT = 2, 8, 77
    C = H * d
    hs = h16(B * n, C, seed=40)
    hs[:, ::7] += 1.5                                   # non-zero row means: LayerNorm has something to remove
    kvt, kvip = h16(B * NT, 2 * C, seed=41), h16(B * p, 2 * C, seed=42)
    wq, wo = h16(C, C, scale=C ** -0.5, seed=43), h16(C, C, scale=C ** -0.5, seed=44)
    bo = torch.randn(C, generator=torch.Generator().manual_seed(45))
    gamma = 1.0 + 0.2 * torch.randn(C, generator=torch.Generator().manual_seed(46))
    beta = 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(47))
    assert ops.Recorder.xattn_fused_supported(C, H, n, NT, p)
    rec = rec_cls("cuda")
    dhs, dt, di = hs.cuda(), kvt.cuda(), kvip.cuda()
    vn = torch.zeros(B, H, p, device="cuda")
    kimg, vimg = rec.xattn_pack_kv(dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], batch=B, heads=H, d=d, nt=NT, nip=p, vnorm=vn)
    fusion = torch.tensor([wt, wi], device="cuda") if fus else None
    out, _ = rec.cross_attention_fused(dhs, wq.cuda(), rec.pack_wo_for_fused(wo.cuda()), bo.cuda(), kimg, vimg, batch=B, nq=n, heads=H, d=d,
                                       nt=NT, nip=p, ln_gamma=gamma.cuda() if ln else None, ln_beta=beta.cuda() if ln else None,
                                       w_text=-7.0 if fus else wt, w_ip=-7.0 if fus else wi, fusion=fusion)
    # C = 640: the 128-row-workgroup form a plan asks for when it runs beside its CFG twin (pv_xattn_fused_params.rows_per_workgroup)
    out128 = None
    if d == 80:
        rec.big_min = 128
        out128, p128 = rec.cross_attention_fused(dhs, wq.cuda(), rec.pack_wo_for_fused(wo.cuda()), bo.cuda(), kimg, vimg, batch=B, nq=n, heads=H, d=d,
                                                 nt=NT, nip=p, ln_gamma=gamma.cuda() if ln else None, ln_beta=beta.cuda() if ln else None,
                                                 w_text=-7.0 if fus else wt, w_ip=-7.0 if fus else wi, fusion=fusion)
        assert p128.rows_per_workgroup == 128
        rec.big_min = 256
    # the four-launch path
    n2 = rec.layernorm(dhs, gamma.cuda(), beta.cuda()) if ln else dhs
    q = rec.gemm(n2, wq.cuda(), rows_per_image=n)
    xa, _ = rec.cross_attention(q, dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], batch=B, heads=H, nq=n, nt=NT, nip=p, d=d, w_text=wt, w_ip=wi)
    unf = rec.gemm(xa, wo.cuda(), bias=bo.cuda(), residual=dhs, rows_per_image=n)
    rec.run()
    torch.cuda.synchronize()
    if out128 is not None:
        assert torch.equal(out128, out)              # the row arithmetic does not depend on the workgroup's row count
    x = hs.float()
    xn = F.layer_norm(x, (C,), gamma, beta, 1e-5) if ln else x
    hv = lambda t, m: t.float().view(B, m, H, d).transpose(1, 2)
    qq = hv(xn @ wq.float().t(), n)
    ot = F.scaled_dot_product_attention(qq, hv(kvt[:, :C], NT), hv(kvt[:, C:], NT))
    vip = hv(kvip[:, C:], p)
    oi = F.scaled_dot_product_attention(qq, hv(kvip[:, :C], p), vip)
    ctx = (wt * ot + wi * oi).transpose(1, 2).reshape(B * n, C)
    ref = ctx @ wo.float().t() + bo + x
    assert torch.isfinite(out).all()
    # the branch (out - hs) is what the kernel computes; the residual only adds an exactly representable term
    assert rel_l2(out.float().cpu() - x, ref - x) < 3e-3 and rel_l2(out, ref) < 1e-3
    assert rel_l2(unf, ref) < 1e-3 and rel_l2(out, unf) < 1e-3
    torch.testing.assert_close(vn.cpu(), vip.norm(dim=-1), rtol=1e-4, atol=1e-4)     # to_v_ip_norm, attention_processor.py:397


@pytest.mark.parametrize("d,n,p,wt,wi,ln,fus", [(160, 256, 1, 1.0, 1.0, True, False), (160, 64, 5, 1.0, 1.0, True, False), (160, 200, 6, 2.0, 0.0, False, False),
                                               (160, 256, 16, 0.0, 2.0, True, True), (160, 130, 0, 1.0, 0.0, True, False),
                                               (80, 1024, 1, 1.0, 1.0, True, False), (80, 200, 5, 1.0, 1.0, True, False), (80, 128, 16, 0.0, 2.0, False, True)])
def test_cross_attention_lnq_head_parallel(rec_cls, d, n, p, wt, wi, ln, fus):
    """pv_cross_attention_lnq (C = 1280 / d = 160 and C = 640 / d = 80 - two heads per 160-feature block, the shared contraction step masked per
    head: norm2 -> to_q -> dual-branch SDPA in ONE head-parallel launch, norm2 folded algebraically into
    the GEMM on the raw rows) vs an fp32 torch reference on the same fp16-rounded operands and vs the three launches it replaces (LayerNorm,
    to_q GEMM, pv_cross_attention); ragged row counts (tails), no image tokens, device-side fusion weights, a LARGE row mean (the fold subtracts
    mean * rowsum(W) from the accumulators: cancellation is exercised)."""
    from photoverse_amd import ops
    B, H, NT = 2, 8, 77
    C = H * d
    hs = h16(B * n, C, seed=140)
    hs[:, ::7] += 1.5
    hs[: n // 2] += 3.0                                  # half of the rows: mean ~ 3 sigma
    kvt, kvip = h16(B * NT, 2 * C, seed=141), h16(B * max(p, 1), 2 * C, seed=142)
    wq = h16(C, C, scale=C ** -0.5, seed=143)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=torch.Generator().manual_seed(146))
    beta = 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(147))
    assert ops.Recorder.xattn_lnq_supported(C, H, NT, p)
    rec = rec_cls("cuda")
    dhs, dt, di = hs.cuda(), kvt.cuda(), kvip.cuda()
    vn = torch.zeros(B, H, max(p, 1), device="cuda")
    fusion = torch.tensor([wt, wi], device="cuda") if fus else None
    out, _ = rec.cross_attention_lnq(dhs, wq.cuda(), dt[:, :C], dt[:, C:], di[:, :C] if p else None, di[:, C:] if p else None, batch=B, heads=H, nq=n, nt=NT,
                                     nip=p, ln_gamma=gamma.cuda() if ln else None, ln_beta=beta.cuda() if ln else None, vnorm=vn if p else None,
                                     w_text=-7.0 if fus else wt, w_ip=-7.0 if fus else wi, fusion=fusion)
    n2 = rec.layernorm(dhs, gamma.cuda(), beta.cuda()) if ln else dhs
    q = rec.gemm(n2, wq.cuda(), rows_per_image=n)
    if p:
        unf, _ = rec.cross_attention(q, dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], batch=B, heads=H, nq=n, nt=NT, nip=p, d=d, w_text=wt, w_ip=wi)
    rec.run()
    torch.cuda.synchronize()
    x = hs.float()
    xn = F.layer_norm(x, (C,), gamma, beta, 1e-5) if ln else x
    hv = lambda t, m: t.float().view(B, m, H, d).transpose(1, 2)
    qq = hv(xn @ wq.float().t(), n)
    ref = wt * F.scaled_dot_product_attention(qq, hv(kvt[:, :C], NT), hv(kvt[:, C:], NT))
    if p:
        vip = hv(kvip[:, C:], p)
        ref = ref + wi * F.scaled_dot_product_attention(qq, hv(kvip[:, :C], p), vip)
    ref = ref.transpose(1, 2).reshape(B * n, C)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref)
    print(f"cross_attention_lnq n={n} P={p} ln={ln}: vs fp32 {err:.2e}" + (f", three-launch path vs fp32 {rel_l2(unf, ref):.2e}" if p else ""))
    assert err < 2e-3
    if p:
        assert rel_l2(unf, ref) < 2e-3 and rel_l2(out, unf) < 2e-3
        torch.testing.assert_close(vn.cpu(), vip.norm(dim=-1), rtol=1e-4, atol=1e-4)     # to_v_ip_norm, attention_processor.py:397


@pytest.mark.parametrize("shift,tol", [(30.0, 4e-3), (100.0, 2e-2)])
def test_cross_attention_lnq_one_pass_statistics_bound(rec_cls, shift, tol):
    """pv_cross_attention_lnq takes norm2's statistics in ONE pass (E[x^2] - mean^2, fp32 accumulators over the fp16 values) and
    folds the mean algebraically; the reference's F.layer_norm is two-pass.  The cancellation grows with (mean / sigma)^2.  This pins the bound on
    rows whose mean is 30 / 100 sigma, with a few outlier channels on top: 30 sigma stays within 2x the usual tolerance, 100 sigma within 2e-2
    (LayerNorm inputs of the SD-v1.5 blocks sit below 3 sigma: tests above; the three-launch path, PV_XLNQ=0, is the two-pass fallback)."""
    B, H, NT, d, n, p = 2, 8, 77, 160, 128, 1
    C = H * d
    hs = h16(B * n, C, seed=150)
    hs[:, 5::97] *= 20.0                                 # outlier channels
    hs[: n] += shift                                     # half of the rows: mean = shift sigma
    kvt, kvip = h16(B * NT, 2 * C, seed=151), h16(B * p, 2 * C, seed=152)
    wq = h16(C, C, scale=C ** -0.5, seed=153)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=torch.Generator().manual_seed(156))
    beta = 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(157))
    rec = rec_cls("cuda")
    dhs, dt, di = hs.cuda(), kvt.cuda(), kvip.cuda()
    out, _ = rec.cross_attention_lnq(dhs, wq.cuda(), dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], batch=B, heads=H, nq=n, nt=NT, nip=p,
                                     ln_gamma=gamma.cuda(), ln_beta=beta.cuda())
    rec.run()
    torch.cuda.synchronize()
    xn = F.layer_norm(hs.float(), (C,), gamma, beta, 1e-5)
    hv = lambda t, m: t.float().view(B, m, H, d).transpose(1, 2)
    qq = hv(xn @ wq.float().t(), n)
    ref = F.scaled_dot_product_attention(qq, hv(kvt[:, :C], NT), hv(kvt[:, C:], NT)) + F.scaled_dot_product_attention(qq, hv(kvip[:, :C], p), hv(kvip[:, C:], p))
    ref = ref.transpose(1, 2).reshape(B * n, C)
    err_hi, err_lo = rel_l2(out[:n], ref[:n]), rel_l2(out[n:], ref[n:])
    print(f"cross_attention_lnq, row mean = {shift:.0f} sigma: shifted rows {err_hi:.2e}, plain rows {err_lo:.2e}")
    assert torch.isfinite(out).all() and err_hi < tol and err_lo < 2e-3


@pytest.mark.parametrize("B,hw", [(16, 4096), (3, 256)])
def test_row_gemm_groupnorm_folded_into_proj_in(rec_cls, B, hw):
    """pv_row_gemm_params.x_norm (ABI 15): Transformer2DModel.norm (GroupNorm 32, eps 1e-6, no activation) folded into proj_in at K = 320 - the row-owning
    launch reads the RAW block output and normalises the rows in registers with pv_groupnorm_scale_shift's per-(image, channel) table - against fp32 torch
    and against the two launches it replaces (GroupNorm-apply, then the tiled GEMM)."""
    C = 320
    src = h16(B * hw, 64, seed=401)
    wp = h16(C, 64, scale=0.2, seed=402)
    b0 = torch.randn(C, generator=torch.Generator().manual_seed(403)) * 0.5
    w = h16(C, C, scale=C ** -0.5, seed=404)
    bias = torch.randn(C, generator=torch.Generator().manual_seed(405))
    gamma = 1.0 + 0.3 * torch.randn(C, generator=torch.Generator().manual_seed(406))
    beta = 0.2 * torch.randn(C, generator=torch.Generator().manual_seed(407))
    rec = rec_cls("cuda")
    x = rec.gemm(src.cuda(), wp.cuda(), bias=b0.cuda(), rows_per_image=hw, colstats=True, splitk=0)
    tab = rec.groupnorm_table(x, gamma.cuda(), beta.cuda(), batch=B, hw=hw, eps=1e-6)
    assert tab is not None
    fused = rec.row_gemm(x, w.cuda(), bias=bias.cuda(), x_norm=tab, rows_per_image=hw)
    g = rec.groupnorm(x, gamma.cuda(), beta.cuda(), batch=B, hw=hw, eps=1e-6)
    two = rec.gemm(g, w.cuda(), bias=bias.cuda(), rows_per_image=hw)
    rec.run()
    torch.cuda.synchronize()
    xin = x.float().cpu().view(B, hw, C).permute(0, 2, 1)
    ref = F.group_norm(xin, 32, gamma, beta, 1e-6).permute(0, 2, 1).reshape(B * hw, C) @ w.float().t() + bias
    e_f, e_t = rel_l2(fused, ref), rel_l2(two, ref)
    print(f"GroupNorm folded into proj_in (B={B}, hw={hw}): vs fp32 {e_f:.2e} (two launches {e_t:.2e}); fused vs two launches {rel_l2(fused, two):.2e}")
    assert e_f < 1e-3 and e_t < 1e-3 and rel_l2(fused, two) < 5e-4


@pytest.mark.parametrize("M,N,geglu,ln,bias", [(1000, 960, False, True, False), (256, 320, False, False, True), (4096, 2560, True, True, True),
                                              (130, 640, True, False, False)])
def test_row_gemm_layernorm_linear_geglu(rec_cls, M, N, geglu, ln, bias):
    """pv_row_gemm (LayerNorm -> K = 320 Linear -> optional GEGLU gate in ONE row-owning launch) vs an fp32 torch reference on the same
    fp16-rounded operands and vs the two-launch path it replaces; ragged M (tails through the buffer descriptors)."""
    from photoverse_amd.ops import pack_geglu, pack_geglu_rows
    K = 320
    x = h16(M, K, seed=60)
    x[:, ::5] += 1.0
    w = h16(N, K, scale=K ** -0.5, seed=61)
    b = torch.randn(N, generator=torch.Generator().manual_seed(62)) if bias else None
    gamma = 1.0 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(63))
    beta = 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(64))
    rec = rec_cls("cuda")
    dx, dw = x.cuda(), w.cuda()
    db = None if b is None else b.cuda()
    if geglu:
        wp, bp = pack_geglu_rows(dw, db)
    else:
        wp, bp = dw, db
    out = rec.row_gemm(dx, wp, bias=bp, ln_gamma=gamma.cuda() if ln else None, ln_beta=beta.cuda() if ln else None, geglu=geglu)
    n1 = rec.layernorm(dx, gamma.cuda(), beta.cuda()) if ln else dx
    if geglu:
        w2, b2 = pack_geglu(dw, db if db is not None else torch.zeros(N, device="cuda"))
        two = rec.gemm(n1, w2, bias=b2, geglu=True)
    else:
        two = rec.gemm(n1, dw, bias=db)
    rec.run()
    torch.cuda.synchronize()
    xn = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) if ln else x.float()
    y = xn @ w.float().t() + (b if b is not None else 0.0)
    ref = y[:, :N // 2] * F.gelu(y[:, N // 2:]) if geglu else y
    assert out.shape == ref.shape and torch.isfinite(out).all()
    print(f"row_gemm M={M} N={N} geglu={geglu} ln={ln}: vs fp32 {rel_l2(out, ref):.2e}, two-launch path vs fp32 {rel_l2(two, ref):.2e}")
    assert rel_l2(out, ref) < 1e-3 and rel_l2(two, ref) < 1e-3 and rel_l2(out, two) < 1e-3


@pytest.mark.parametrize("M", [1000, 4096 + 37])
def test_row_gemm_strides_guard_rows_and_replay_determinism(rec_cls, M):
    """The ABI advertises ld_x / ld_out and M tails through buffer descriptors: feed a column slice of a wider buffer (ld_x = 448 > 320), write
    into a column slice of a wider output whose padding columns and guard rows past M must stay untouched bit for bit, and replay the launch
    several times - the hand-counted vmcnt bookkeeping of the weight ring must give bitwise identical results run to run."""
    K, N = 320, 960
    xw = h16(M, 448, seed=70)
    xw[:, ::5] += 1.0
    w = h16(N, K, scale=K ** -0.5, seed=71)
    gamma = 1.0 + 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(72))
    beta = 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(73))
    rec = rec_cls("cuda")
    dxw = xw.cuda()
    x_view = dxw[:, 64:64 + K]                                  # ld_x = 448, offset 64 columns
    GUARD, PAD = 64, 32
    sentinel = 12345.0
    big = torch.full((M + GUARD, N + 2 * PAD), sentinel, dtype=torch.float16, device="cuda")
    out_view = big[:M, PAD:PAD + N]                             # ld_out = N + 64
    got = rec.row_gemm(x_view, w.cuda(), ln_gamma=gamma.cuda(), ln_beta=beta.cuda(), out=out_view)
    assert got.data_ptr() == out_view.data_ptr()
    rec.run()
    torch.cuda.synchronize()
    first = big.clone()
    xs = xw[:, 64:64 + K].float()
    ref = F.layer_norm(xs, (K,), gamma, beta, 1e-5) @ w.float().t()
    assert rel_l2(first[:M, PAD:PAD + N], ref) < 1e-3
    assert (first[M:] == sentinel).all(), "rows past M were written"
    assert (first[:, :PAD] == sentinel).all() and (first[:, PAD + N:] == sentinel).all(), "columns outside the output slice were written"
    for _ in range(5):
        rec.run()
        torch.cuda.synchronize()
        assert torch.equal(big, first), "replay differs bitwise"


def test_conv_in_out_timestep(rec_cls):
    B, h = 2, 16
    x = torch.randn(B, 4, h, h, generator=torch.Generator().manual_seed(30))
    w = torch.randn(320, 4, 3, 3, generator=torch.Generator().manual_seed(31)) * 0.2
    b = torch.randn(320, generator=torch.Generator().manual_seed(32))
    rec = rec_cls("cuda")
    # conv_in as the UNet plan runs it: im2col to K = 36 (zero padded to 64) + the MFMA GEMM
    cols = rec.im2col3x3(x.cuda(), batch=B, cin=4, h=h, wd=h, kpad=64)
    w_in = torch.zeros(320, 64, dtype=torch.float16)
    w_in[:, :36] = w.reshape(320, 36).half()
    y = rec.gemm(cols, w_in.cuda(), bias=b.cuda(), rows_per_image=h * h)
    xo = h16(B, 320, h, h, seed=33)
    wo = h16(4, 320, 3, 3, scale=0.02, seed=34)
    bo = torch.randn(4, generator=torch.Generator().manual_seed(35))
    z = rec.conv_out(xo.permute(0, 2, 3, 1).reshape(-1, 320).contiguous().cuda(), wo.permute(0, 2, 3, 1).reshape(4, -1).contiguous().cuda(),
                     bo.cuda(), batch=B, cin=320, h=h, wd=h, cout=4)
    xv = h16(3, 128, 10, 10, seed=36)                    # VAE-shaped: 128 -> 3, pixel count not a multiple of the 32-pixel block
    wv = h16(3, 128, 3, 3, scale=0.05, seed=37)
    zv = rec.conv_out(xv.permute(0, 2, 3, 1).reshape(-1, 128).contiguous().cuda(), wv.permute(0, 2, 3, 1).reshape(3, -1).contiguous().cuda(),
                      None, batch=3, cin=128, h=10, wd=10, cout=3)
    ts = torch.tensor([951.0, 20.0, 500.0])
    te = rec.timestep_embedding(ts.cuda(), None, 3, 320)
    rec.run()
    torch.cuda.synchronize()
    ref = F.conv2d(x.half().float(), w.half().float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, 320)
    assert rel_l2(y, ref) < 1e-3
    refo = F.conv2d(xo.float(), wo.float(), bo, padding=1)
    assert rel_l2(z, refo) < 1e-5
    assert rel_l2(zv, F.conv2d(xv.float(), wv.float(), None, padding=1)) < 1e-5
    half = 160
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    emb = ts[:, None] * freq[None]
    reft = torch.cat([emb.cos(), emb.sin()], -1)
    assert (te.float().cpu() - reft).abs().max().item() < 2e-3      # fp16 output of values in [-1,1]


def test_cfg_dpm_step_kernel(rec_cls):
    n = 2 * 4 * 16 * 16
    g = torch.Generator().manual_seed(36)
    eu, ec, x, xp = [torch.randn(n, generator=g) for _ in range(4)]
    coef = torch.randn(3, 8, generator=g)
    state = torch.tensor([1], dtype=torch.int32)
    dx, dxp, dstate = x.cuda(), xp.cuda(), state.cuda()
    rec = rec_cls("cuda")
    rec.cfg_dpm_step(eu.cuda(), ec.cuda(), dx, dxp, coef.cuda(), dstate, 7.5)
    rec.step_advance(dstate)
    rec.run()
    torch.cuda.synchronize()
    e = eu + 7.5 * (ec - eu)
    ca, cb, cx, c0, c1 = coef[1, :5]
    x0 = ca * x + cb * e
    torch.testing.assert_close(dxp.cpu(), x0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dx.cpu(), cx * x + c0 * x0 + c1 * xp, rtol=1e-5, atol=1e-5)
    assert dstate.item() == 2


def test_rows_mean(rec_cls):
    x = h16(3 * 256, 768, seed=37)
    rec = rec_cls("cuda")
    y = rec.rows_mean(x.cuda(), groups=3, count=256)
    rec.run()
    torch.cuda.synchronize()
    assert rel_l2(y, x.float().view(3, 256, 768).mean(1)) < 1e-3


def test_bad_arguments_fail_loudly(rec_cls):
    from photoverse_amd.ops import HipLaunchError
    rec = rec_cls("cuda")
    a, w = h16(64, 100).cuda(), h16(128, 100).cuda()     # K not a multiple of 64
    rec.gemm(a, w)
    with pytest.raises(HipLaunchError):
        rec.run()


# ------------------------------------------------------------------ backward kernels of the stock blocks (pv_train.hip)
@pytest.mark.parametrize("B,H,N,d,causal", [(2, 2, 200, 40, False), (1, 2, 130, 80, False), (2, 3, 77, 64, True), (1, 2, 64, 160, False),
                                             (1, 1, 333, 40, True)])
def test_self_attention_backward(rec_cls, B, H, N, d, causal):
    """pv_attention (lse output) + pv_attention_backward against autograd through fp32 SDPA."""
    g = torch.Generator().manual_seed(N + d)
    C = H * d
    qkv = torch.randn(B * N, 3 * C, generator=g)
    dout = torch.randn(B * N, C, generator=g)
    q32, k32, v32 = (qkv[:, i * C:(i + 1) * C].half().float().view(B, N, H, d).transpose(1, 2).clone().requires_grad_() for i in range(3))
    ref = F.scaled_dot_product_attention(q32, k32, v32, is_causal=causal)
    ref.backward(dout.half().float().view(B, N, H, d).transpose(1, 2))
    want = [t.grad.transpose(1, 2).reshape(B * N, C) for t in (q32, k32, v32)]

    rec = rec_cls("cuda")
    x = qkv.half().cuda()
    lse = rec.empty((B, H, N), torch.float32)
    o = rec.attention(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], batch=B, heads=H, nq=N, nk=N, d=d, causal=causal, lse=lse)
    dqkv = rec.empty((B * N, 3 * C))
    rec.attention_backward(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], o, dout.half().cuda(), lse, batch=B, heads=H, nq=N, nk=N, d=d, causal=causal,
                           dq=dqkv[:, :C], dk=dqkv[:, C:2 * C], dv=dqkv[:, 2 * C:])
    rec.run()
    torch.cuda.synchronize()
    assert rel_l2(o.float().cpu(), ref.detach().transpose(1, 2).reshape(B * N, C)) < 2e-3
    # lse: natural-log logsumexp of the scaled scores, in log2 units
    s = (q32.detach() @ k32.detach().transpose(-1, -2)) / d ** 0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), 1), float("-inf"))
    assert (lse.cpu() - torch.logsumexp(s, -1) / math.log(2.0)).abs().max() < 2e-2
    for i, name in enumerate("qkv"):
        assert rel_l2(dqkv[:, i * C:(i + 1) * C].float().cpu(), want[i]) < 4e-3, name


@pytest.mark.parametrize("var", [0, 1, 81])
@pytest.mark.parametrize("B,H,N,d,spiky", [(2, 2, 1024, 40, False), (1, 3, 512, 40, True), (2, 2, 768, 80, False), (1, 2, 256, 80, True)])
def test_self_attention_backward_8wave_staggered_passes(rec_cls, monkeypatch, var, B, H, N, d, spiky):
    """The d = 40 / 80 backward as 8-wave staggered dK/dV and dQ passes (pv_attnbwd.hip: -lse / -delta ride in the padding columns of the 48-deep
    contractions as fp16 (hi, lo) pairs) against autograd through fp32 SDPA, and against the 4-wave kernels of pv_train.hip on the same input.
    ``spiky``: one key row scaled by 12 - log-sum-exps of ~ +-60 log2 units, the range the (hi, lo) split has to carry.  d = 80: two fragments per wave,
    256 owned rows per workgroup, 96-deep contractions with the statistics in columns 80 / 81."""
    g = torch.Generator().manual_seed(N + var)
    C = H * d
    qkv = torch.randn(B * N, 3 * C, generator=g)
    if spiky:
        qkv[(N * 3) // 5, C:2 * C] *= 12.0
    dout = torch.randn(B * N, C, generator=g)
    q32, k32, v32 = (qkv[:, i * C:(i + 1) * C].half().float().view(B, N, H, d).transpose(1, 2).clone().requires_grad_() for i in range(3))
    ref = F.scaled_dot_product_attention(q32, k32, v32)
    ref.backward(dout.half().float().view(B, N, H, d).transpose(1, 2))
    want = [t.grad.transpose(1, 2).reshape(B * N, C) for t in (q32, k32, v32)]
    x, do = qkv.half().cuda(), dout.half().cuda()
    got = {}
    for form in (var, -1):
        monkeypatch.setenv("PV_ATTN8_BWD", str(form))
        monkeypatch.setenv("PV_ATTN8_BWD_MIN", "1")
        rec = rec_cls("cuda")
        lse = rec.empty((B, H, N), torch.float32)
        o = rec.attention(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], batch=B, heads=H, nq=N, nk=N, d=d, lse=lse)
        dqkv = rec.empty((B * N, 3 * C))
        dqkv.fill_(float("nan"))
        rec.attention_backward(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], o, do, lse, batch=B, heads=H, nq=N, nk=N, d=d,
                               dq=dqkv[:, :C], dk=dqkv[:, C:2 * C], dv=dqkv[:, 2 * C:])
        rec.run()
        torch.cuda.synchronize()
        got[form] = dqkv.float().cpu()
        assert torch.isfinite(got[form]).all()
    for i, name in enumerate("qkv"):
        sl = slice(i * C, (i + 1) * C)
        e8, e4 = rel_l2(got[var][:, sl], want[i]), rel_l2(got[-1][:, sl], want[i])
        assert e8 < 4e-3, (name, e8)
        assert e8 < 1.5 * e4 + 2e-4, (name, e8, e4)          # no worse than the 4-wave kernels' fp16 operand rounding
        assert rel_l2(got[var][:, sl], got[-1][:, sl]) < 2e-3, name


@pytest.mark.parametrize("d,NQ,NK", [(40, 512, 1024), (40, 1536, 512), (80, 256, 768), (80, 512, 256)])
def test_self_attention_backward_8wave_passes_with_unequal_query_and_key_counts(rec_cls, monkeypatch, d, NQ, NK):
    """pv_attn8_bwd_eligible accepts nq != nk (the dK/dV pass owns keys and walks the queries, the dQ pass the other way round): both passes against
    autograd through fp32 SDPA and against the 4-wave kernels at rectangular sizes; a PV_ATTN8_BWD value that names no instantiated form is not
    eligible and takes the 4-wave kernels (same bits as -1) instead of failing the launch."""
    B, H = 2, 8
    C = H * d
    g = torch.Generator().manual_seed(NQ + NK)
    q, kv, dout = torch.randn(B * NQ, C, generator=g), torch.randn(B * NK, 2 * C, generator=g), torch.randn(B * NQ, C, generator=g)
    heads = lambda t, n: t.half().float().view(B, n, H, d).transpose(1, 2).clone().requires_grad_()
    q32, k32, v32 = heads(q, NQ), heads(kv[:, :C], NK), heads(kv[:, C:], NK)
    F.scaled_dot_product_attention(q32, k32, v32).backward(dout.half().float().view(B, NQ, H, d).transpose(1, 2))
    want = [q32.grad.transpose(1, 2).reshape(B * NQ, C), k32.grad.transpose(1, 2).reshape(B * NK, C), v32.grad.transpose(1, 2).reshape(B * NK, C)]
    xq, xkv, do = q.half().cuda(), kv.half().cuda(), dout.half().cuda()
    monkeypatch.setenv("PV_ATTN8_BWD_MIN", "1")
    got = {}
    for form in (81, -1, 17):
        monkeypatch.setenv("PV_ATTN8_BWD", str(form))
        rec = rec_cls("cuda")
        lse = rec.empty((B, H, NQ), torch.float32)
        o = rec.attention(xq, xkv[:, :C], xkv[:, C:], batch=B, heads=H, nq=NQ, nk=NK, d=d, lse=lse)
        dq, dkv = rec.empty((B * NQ, C)), rec.empty((B * NK, 2 * C))
        dq.fill_(float("nan")); dkv.fill_(float("nan"))
        rec.attention_backward(xq, xkv[:, :C], xkv[:, C:], o, do, lse, batch=B, heads=H, nq=NQ, nk=NK, d=d, dq=dq, dk=dkv[:, :C], dv=dkv[:, C:])
        rec.run()
        torch.cuda.synchronize()
        got[form] = [dq.float().cpu(), dkv[:, :C].float().cpu(), dkv[:, C:].float().cpu()]
    for i, name in enumerate(("dq", "dk", "dv")):
        assert torch.isfinite(got[81][i]).all(), name
        e8, e4 = rel_l2(got[81][i], want[i]), rel_l2(got[-1][i], want[i])
        assert e8 < 4e-3 and e8 < 1.5 * e4 + 2e-4, (name, e8, e4)
        assert torch.equal(got[17][i], got[-1][i]), name            # unknown variant: the 4-wave kernels, not an error


@pytest.mark.parametrize("B,N,d", [(16, 4096, 40), (4, 4608, 40), (3, 1536, 40), (16, 1024, 80), (5, 2304, 80)])
def test_self_attention_8wave_kernels_repeat_bit_for_bit_under_load(rec_cls, B, N, d):
    """Race screen for the LDS-DMA rings and the segment schedules of attn8_kernel and attn8_bwd_kernel at the sizes that fill the chip: the kernels
    have a fixed summation order, so 40 replays of forward + backward must return the same bits every time (the one wrong schedule hipcc produced for
    these kernels returned different sums from run to run: EXPERIMENTS.md), and a sample of the rows is checked against fp32 autograd.  (d = 80: the
    backward passes only are 8-wave kernels.)"""
    H = 8
    C = H * d
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B * N, 3 * C, generator=g).half().cuda()
    do = torch.randn(B * N, C, generator=g).half().cuda()
    rec = rec_cls("cuda")
    lse = rec.empty((B, H, N), torch.float32)
    o = rec.attention(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], batch=B, heads=H, nq=N, nk=N, d=d, lse=lse)
    dqkv = rec.empty((B * N, 3 * C))
    rec.attention_backward(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], o, do, lse, batch=B, heads=H, nq=N, nk=N, d=d,
                           dq=dqkv[:, :C], dk=dqkv[:, C:2 * C], dv=dqkv[:, 2 * C:])
    rec.run()
    torch.cuda.synchronize()
    first = (o.clone(), dqkv.clone(), lse.clone())
    for _ in range(40):
        o.fill_(float("nan"))
        dqkv.fill_(float("nan"))
        rec.run()
        torch.cuda.synchronize()
        assert torch.equal(o, first[0]) and torch.equal(dqkv, first[1]) and torch.equal(lse, first[2])
    # one (sample, head) against fp32 autograd
    b, h = B - 1, H - 1
    rows = slice(b * N, (b + 1) * N)
    q32, k32, v32 = (x[rows, i * C + h * d:i * C + (h + 1) * d].float().clone().requires_grad_() for i in range(3))
    ref = F.scaled_dot_product_attention(q32[None], k32[None], v32[None])[0]
    ref.backward(do[rows, h * d:(h + 1) * d].float())
    assert rel_l2(o[rows, h * d:(h + 1) * d].float().cpu(), ref.detach().cpu()) < 2e-3
    for i, t in enumerate((q32, k32, v32)):
        assert rel_l2(dqkv[rows, i * C + h * d:i * C + (h + 1) * d].float().cpu(), t.grad.cpu()) < 4e-3, "qkv"[i]


@pytest.mark.parametrize("B,hw,c0,c1,act,with_add", [(2, 256, 320, 0, "silu", False), (1, 64, 640, 320, "silu", True), (2, 144, 320, 0, "none", True),
                                                      (1, 16, 1280, 1280, "silu", False)])
def test_groupnorm_backward(rec_cls, B, hw, c0, c1, act, with_add):
    from photoverse_amd import ops
    g = torch.Generator().manual_seed(hw + c0)
    C = c0 + c1
    x = (torch.randn(B, hw, C, generator=g) * 1.5 + 0.3).half()
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.2
    dy = torch.randn(B, hw, C, generator=g).half()
    add = torch.randn(B, hw, C, generator=g).half()
    xr = x.float().requires_grad_()
    y = F.group_norm(xr.permute(0, 2, 1), 32, gamma, beta, eps=1e-5).permute(0, 2, 1)
    if act == "silu":
        y = F.silu(y)
    y.backward(dy.float())
    want = xr.grad + (add.float() if with_add else 0)

    rec = rec_cls("cuda")
    xc = x.cuda().view(B * hw, C)
    x0 = xc[:, :c0].contiguous()
    x1 = xc[:, c0:].contiguous() if c1 else None
    a = ops.ACT_SILU if act == "silu" else ops.ACT_NONE
    yk, stats = rec.groupnorm(x0, gamma.cuda(), beta.cuda(), batch=B, hw=hw, x1=x1, eps=1e-5, act=a, return_stats=True)
    addc = add.cuda().view(B * hw, C)
    dx0, dx1 = rec.groupnorm_backward(x0, dy.cuda().view(B * hw, C), stats, gamma.cuda(), beta.cuda(), batch=B, hw=hw, x1=x1, act=a,
                                      add0=addc[:, :c0] if with_add else None, add1=(addc[:, c0:] if (with_add and c1) else None))
    rec.run()
    torch.cuda.synchronize()
    assert rel_l2(yk.float().cpu().view(B, hw, C), y.detach()) < 2e-3
    got = torch.cat([dx0] + ([dx1] if c1 else []), 1).float().cpu().view(B, hw, C)
    assert rel_l2(got, want) < 3e-3


def test_elementwise_backward_pieces(rec_cls):
    from photoverse_amd import ops
    g = torch.Generator().manual_seed(3)
    rec = rec_cls("cuda")
    # GEGLU
    h = torch.randn(100, 2 * 640, generator=g).half()
    dy = torch.randn(100, 640, generator=g).half()
    hr = h.float().requires_grad_()
    (hr[:, :640] * F.gelu(hr[:, 640:])).backward(dy.float())
    dh = rec.geglu_backward(h.cuda(), dy.cuda())
    # quick-GELU / SiLU
    x = torch.randn(77, 3072, generator=g).half()
    d2 = torch.randn(77, 3072, generator=g).half()
    xr = x.float().requires_grad_()
    (xr * torch.sigmoid(1.702 * xr)).backward(d2.float())
    want_q = xr.grad.clone()
    xr.grad = None
    F.silu(xr).backward(d2.float())
    dq_ = rec.act_backward(x.cuda(), d2.cuda(), ops.ACT_QUICK_GELU)
    ds_ = rec.act_backward(x.cuda(), d2.cuda(), ops.ACT_SILU)
    # add, dilate, pool
    a, b = torch.randn(50, 320, generator=g).half(), torch.randn(50, 320, generator=g).half()
    s_ = rec.add_rows(a.cuda(), b.cuda())
    t = torch.randn(2, 3, 5, 64, generator=g).half()
    z = rec.dilate2x(t.cuda().view(-1, 64), batch=2, h=3, w=5)
    big = torch.randn(2, 6, 10, 64, generator=g).half()
    addp = torch.randn(2, 3, 5, 64, generator=g).half()
    pl = rec.pool2x_sum(big.cuda().view(-1, 64), batch=2, h=3, w=5, add=addp.cuda().view(-1, 64))
    # sign, gather
    v = torch.randn(4, 1, 768, generator=g)
    v[0, 0, :5] = 0
    sg = rec.sign(v.cuda(), 0.25)
    rows = torch.randn(4 * 77, 768, generator=g).half()
    idx = torch.tensor([5, 1, 71, 76], dtype=torch.int32)
    gr = rec.gather_rows(rows.cuda(), idx.cuda(), batch=4, seq=77, n_e=1, scale=0.5)
    rec.run()
    torch.cuda.synchronize()
    assert rel_l2(dh.float().cpu(), hr.grad) < 2e-3
    assert rel_l2(dq_.float().cpu(), want_q) < 2e-3
    assert rel_l2(ds_.float().cpu(), xr.grad) < 2e-3
    assert torch.equal(s_.cpu(), (a.float() + b.float()).half())
    zr = torch.zeros(2, 6, 10, 64, dtype=torch.float16)
    zr[:, ::2, ::2] = t
    assert torch.equal(z.cpu().view(2, 6, 10, 64), zr)
    pr = big.float().view(2, 3, 2, 5, 2, 64).sum((2, 4)) + addp.float()
    assert rel_l2(pl.float().cpu().view(2, 3, 5, 64), pr) < 1e-3
    assert torch.equal(sg.cpu(), 0.25 * torch.sign(v))
    want_g = torch.stack([0.5 * rows.float().view(4, 77, 768)[b, idx[b]] for b in range(4)]).view(4, 1, 768)
    assert torch.equal(gr.cpu(), want_g)


def test_arcface_loss_pieces(rec_cls):
    """Per-channel affine, PReLU, 2x2 max-pool, gray + bilinear resize (each with its backward), cosine embedding loss, softmax-rows backward,
    clamp mask - against torch on the same fp16-rounded inputs."""
    g = torch.Generator().manual_seed(8)
    rec = rec_cls("cuda")
    x = torch.randn(2 * 8 * 8, 128, generator=g).half()
    dy = torch.randn(2 * 8 * 8, 128, generator=g).half()
    sc, sh = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    slope = torch.tensor([0.25])
    ca = rec.col_affine(x.cuda(), sc.cuda(), sh.cuda())
    cab = rec.col_affine(dy.cuda(), sc.cuda(), None)
    pr = rec.prelu(x.cuda(), slope.cuda())
    prb = rec.prelu(x.cuda(), slope.cuda(), dy=dy.cuda())
    mp = rec.maxpool2x2(x.cuda(), batch=2, h=8, w=8)
    dmp = torch.randn(2 * 4 * 4, 128, generator=g).half()
    mpb = rec.maxpool2x2(x.cuda(), batch=2, h=8, w=8, dy=dmp.cuda())
    imgs, outs = {}, {}
    for H, W, S in ((24, 24, 32), (64, 48, 16), (32, 32, 32), (100, 100, 128)):
        img = torch.randn(2, 3, H, W, generator=g)
        dg = torch.randn(2, 3, S, S, generator=g)               # gradient arrives as channel 0 of a 3-channel buffer (image stride 3 S^2)
        imgs[(H, W, S)] = (img, dg)
        outs[(H, W, S)] = (rec.gray_resize(img.cuda(), size=S, mul=0.5, add=-1.0), rec.gray_resize_backward(dg.cuda()[:, :1], h=H, w=W, mul=0.5))
    e1, e2 = torch.randn(3, 512, generator=g).half(), torch.randn(3, 512, generator=g).half()
    ls_p, de_p = rec.cosine_embedding_loss(e1.cuda(), e2.cuda(), target=1.0, gscale=4.0)
    ls_n, de_n = rec.cosine_embedding_loss(e1.cuda(), (e1 + 0.5 * e2).half().cuda(), target=-1.0, gscale=1.0)
    P = torch.softmax(torch.randn(16, 256, generator=g), -1).half()
    dP = torch.randn(16, 256, generator=g).half()
    dS = rec.softmax_rows_backward(P.cuda(), dP.clone().cuda(), scale=0.3)
    yv, dyv = torch.randn(1000, generator=g) * 1.5, torch.randn(1000, generator=g)
    cm = rec.clamp_mask(yv.cuda(), dyv.cuda(), -1.0, 1.0)
    rec.run()
    torch.cuda.synchronize()
    xf = x.float()
    assert rel_l2(ca, xf * sc + sh) < 1e-3 and rel_l2(cab, dy.float() * sc) < 1e-3
    assert rel_l2(pr, torch.where(xf > 0, xf, 0.25 * xf)) < 1e-3 and rel_l2(prb, dy.float() * torch.where(xf > 0, 1.0, 0.25)) < 1e-3
    xr = xf.view(2, 8, 8, 128).permute(0, 3, 1, 2).clone().requires_grad_()
    pooled = F.max_pool2d(xr, 2, 2)
    pooled.backward(dmp.float().view(2, 4, 4, 128).permute(0, 3, 1, 2))
    assert torch.equal(mp.float().cpu().view(2, 4, 4, 128), pooled.detach().permute(0, 2, 3, 1))
    assert rel_l2(mpb.float().cpu().view(2, 8, 8, 128), xr.grad.permute(0, 2, 3, 1)) < 1e-6
    wts = torch.tensor([0.2989, 0.5870, 0.1140])
    for (H, W, S), (img, dg) in imgs.items():
        ir = img.clone().requires_grad_()
        gray = torch.tensordot(ir, wts, dims=([1], [0])).unsqueeze(1)
        ref = F.interpolate(gray, size=(S, S), mode="bilinear", align_corners=False) * 0.5 - 1.0
        ref.backward(dg[:, :1])
        got, gotb = outs[(H, W, S)]
        assert rel_l2(got, ref.detach()) < 1e-5, (H, W, S)
        assert rel_l2(gotb, ir.grad) < 1e-5, (H, W, S)
    e2r = e2.float().requires_grad_()
    lp = torch.nn.CosineEmbeddingLoss()(e1.float(), e2r, torch.ones(3))
    lp.backward()
    assert ls_p.mean().item() == pytest.approx(lp.item(), rel=1e-4) and rel_l2(de_p, 4.0 * e2r.grad) < 2e-3
    e3 = (e1 + 0.5 * e2).half().float().requires_grad_()
    ln = torch.nn.CosineEmbeddingLoss()(e1.float(), e3, -torch.ones(3))
    ln.backward()
    assert ls_n.mean().item() == pytest.approx(ln.item(), rel=1e-4) and rel_l2(de_n, e3.grad) < 2e-3
    Pf, dPf = P.float(), dP.float()
    assert rel_l2(dS, 0.3 * Pf * (dPf - (Pf * dPf).sum(-1, keepdim=True))) < 2e-3
    assert torch.equal(cm.cpu(), torch.where((yv > -1) & (yv < 1), dyv, torch.zeros(())))


@pytest.mark.gpu
def test_pack_weights_multi():
    """pv_pack_weights: fp16 copies + transposed twins of several fp32 masters in one launch, blocks of larger zero-padded matrices, a scale."""
    from photoverse_amd.tape import Tape
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    a, b, c = (torch.randn(s, generator=g).to(dev) for s in ((8, 320), (77, 45), (640, 8)))
    tp = Tape(dev)
    w1, w1T = tp.trainable_blocks(256, 640, [(a, 0, 0, 1.0), (a, 128, 320, 1.0)])
    w2, w2T = tp.trainable_blocks(77, 45, [(b, 0, 0, 1.0)])
    w3, w3T = tp.trainable_blocks(700, 136, [(c, 60, 128, -0.125)])
    for it in range(2):
        tp.load_weights()
        torch.cuda.synchronize()
        e1 = torch.zeros(256, 640, device=dev)
        e1[:8, :320], e1[128:136, 320:] = a, a
        e3 = torch.zeros(700, 136, device=dev)
        e3[60:700, 128:136] = -0.125 * c
        for w, wT, e in ((w1, w1T, e1), (w2, w2T, b), (w3, w3T, e3)):
            assert torch.equal(w, e.half()) and torch.equal(wT, e.half().t())
        a.mul_(2.0); b.add_(1.0); c.sub_(0.5)                 # the masters move in place (an optimizer step): the next launch picks them up


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(1000, 136, 200), (65536, 128, 320), (80, 640, 768), (4112, 1024, 1024), (7, 8, 8)])
def test_wgrad_tn(m, n, k):
    """pv_wgrad_tn + slab sum: dW = dY^T X with both operands as row matrices (strided views included), ragged row / column tails,
    against fp32 matmul of the same fp16 inputs; two runs are bit-identical (fixed-order slab sum)."""
    from photoverse_amd.ops import Recorder
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(m + n + k)
    big = torch.randn(m, n + 16, generator=g).half().to(dev)
    dy = big[:, 8:8 + n]                                       # a column slice: ld != n
    x = torch.randn(m, k, generator=g).half().to(dev)
    rec = Recorder(dev)
    dw = rec.wgrad(dy, x)
    rec.run()
    torch.cuda.synchronize()
    first = dw.clone()
    ref = dy.float().t() @ x.float()
    assert dw.shape == (n, k)
    assert (dw - ref).norm() / ref.norm() < 2e-6 * max(1.0, (m / 64) ** 0.5)
    rec.run()
    torch.cuda.synchronize()
    assert torch.equal(dw, first)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(77, 200), (1000, 320), (4100, 640), (1232, 768), (130, 1024), (515, 1280), (37, 2048)])
@pytest.mark.parametrize("affine,act", [(False, "none"), (False, "leaky"), (True, "leaky")])
def test_layernorm_backward_kernels(rows, cols, affine, act):
    """pv_layernorm_backward against torch autograd (fp32 math on the same fp16 inputs): the data-only kernel in all its lanes-per-row
    instantiations (8 x 5, 16 x 5, 16 x 6, 32 x 4, 32 x 5, 64 x 4 chunks) with row counts that leave partial waves, and the kernel that also
    produces dgamma / dbeta."""
    from photoverse_amd.ops import ACT_LEAKY_RELU, ACT_NONE, Recorder
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x = (torch.randn(rows, cols, generator=g) * 1.5 + 0.3).half().to(dev)
    dy = torch.randn(rows, cols, generator=g).half().to(dev)
    gamma = (1.0 + 0.2 * torch.randn(cols, generator=g)).to(dev)
    beta = (0.1 * torch.randn(cols, generator=g)).to(dev)
    rec = Recorder(dev)
    dx, dgb = rec.layernorm_backward(x, dy, gamma, beta, eps=1e-5, act=ACT_LEAKY_RELU if act == "leaky" else ACT_NONE, want_affine=affine)
    # `add` (ABI 14): the gradient x already holds rides in the same launch; here a column-sliced view (ldadd > cols)
    wide = torch.randn(rows, cols + 8, generator=g).half().to(dev)
    dx_add, _ = rec.layernorm_backward(x, dy, gamma, beta, eps=1e-5, act=ACT_LEAKY_RELU if act == "leaky" else ACT_NONE, want_affine=affine, add=wide[:, :cols])
    rec.run()
    torch.cuda.synchronize()
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (cols,), gr, br, 1e-5)
    if act == "leaky":
        y = torch.nn.functional.leaky_relu(y, 0.01)
    y.backward(dy.float())
    assert rel_l2(dx.float(), xr.grad) < 1.5e-3
    assert rel_l2(dx_add.float(), xr.grad + wide[:, :cols].float()) < 1.5e-3
    if affine:
        assert rel_l2(dgb[0], gr.grad) < 1e-4 and rel_l2(dgb[1], br.grad) < 1e-4
    else:
        assert dgb is None


@pytest.mark.gpu
@pytest.mark.parametrize("d,n,p,wt,wi", [(40, 1024, 1, 1.0, 1.0), (40, 600, 5, 0.7, 1.3), (80, 256, 6, 1.0, 1.0), (160, 64, 16, 2.0, 0.0), (40, 520, 16, 0.0, 2.0)])
def test_cross_attention_backward_kernels(rec_cls, d, n, p, wt, wi):
    """pv_cross_attention_backward (dq pass, dK / dV partials per 512-query chunk, ordered reduce) against torch autograd over the fp32
    two-SDPA formula of the processor (attention_processor.py:317-322, :400-420) on the same fp16 operands, with the to_v_ip_norm
    regulariser gradient (:397) folded in; query counts that leave ragged chunks / tiles."""
    B, H, NT = 2, 8, 77
    C = H * d
    q, kvt, kvip, do = h16(B * n, C, seed=61), h16(B * NT, 2 * C, seed=62), h16(B * p, 2 * C, seed=63), h16(B * n, C, seed=64)
    coef = 0.05
    rec = rec_cls("cuda")
    dq_, dt, di, dd = q.cuda(), kvt.cuda(), kvip.cuda(), do.cuda()
    dq, dkv_t, dkv_i = rec.cross_attention_backward(dq_, dt[:, :C], dt[:, C:], di[:, :C], di[:, C:], dd, batch=B, heads=H, nq=n, nt=NT, nip=p, d=d,
                                                    w_text=wt, w_ip=wi, vnorm_coef=coef)
    rec.run()
    torch.cuda.synchronize()
    hv = lambda t, m: t.view(B, m, H, d).transpose(1, 2)
    qr, kt, vt = (x.float().requires_grad_(True) for x in (q, kvt[:, :C], kvt[:, C:]))
    ki, vi = (x.float().requires_grad_(True) for x in (kvip[:, :C], kvip[:, C:]))
    ot = F.scaled_dot_product_attention(hv(qr, n), hv(kt, NT), hv(vt, NT))
    oi = F.scaled_dot_product_attention(hv(qr, n), hv(ki, p), hv(vi, p))
    out = (wt * ot + wi * oi).transpose(1, 2).reshape(B * n, C)
    loss = (out * do.float()).sum() + coef * hv(vi, p).norm(dim=-1).sum()
    loss.backward()
    assert rel_l2(dq.float(), qr.grad) < 3e-3
    if wt != 0.0:
        assert rel_l2(dkv_t[:, :C], kt.grad) < 2e-3 and rel_l2(dkv_t[:, C:], vt.grad) < 2e-3
    else:
        assert float(dkv_t.abs().max()) == 0.0
    assert rel_l2(dkv_i[:, C:], vi.grad) < 2e-3
    if p == 1:
        assert float(dkv_i[:, :C].abs().max()) < 1e-4           # softmax over ONE key is constant: its key gets no gradient
    elif wi != 0.0:
        assert rel_l2(dkv_i[:, :C], ki.grad) < 2e-3
