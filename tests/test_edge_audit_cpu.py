"""CPU side of the edge audit (``oracle.edge_cases``; its GPU side is tests/test_edge_audit_gpu.py): the dispatch sweep that says which kernels have
to be audited, the validity of the catalogue (every block accepted by the library, every tensor a guarded view), the reference features the catalogue
uses that tests/test_abi_ref_cpu.py does not check yet, and the guards themselves against injected defects.  No GPU: the catalogue is recorded dry."""
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


@pytest.fixture(scope="module")
def E():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)
    from oracle import edge_cases
    return edge_cases


@pytest.fixture(scope="module")
def recorded(E):
    """case name -> its dry recorder (parameter blocks and tags; host pointers, never run)"""
    out = {}
    for c in E.CASES:
        with E.environment(c.env):
            out[c.name] = E.build(c, "cpu")
    return out


def close(a, b, tol=1e-9):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert ((a - b).norm() / b.norm()).item() < tol


def h16(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


# ------------------------------------------------------------------------------------------------------------------ dispatch coverage
def test_process_cached_switches_are_not_set(E):
    """The sweep describes the library as the suite runs it: none of the switches it reads once per process may be set."""
    assert not [k for k in E.PROCESS_SWITCHES if k in os.environ]


def test_every_dispatchable_kernel_is_the_tag_of_a_catalogue_launch(E, recorded):
    swept = E.swept_symbols()
    assert len(swept) >= 30 and all(s.startswith(E.DISPATCHED) for s in swept), sorted(swept)
    tags = {t[0] for rec in recorded.values() for t in rec.tags}
    missing = sorted(set(swept) - tags)
    assert not missing, f"kernels the dispatchers can choose that no catalogue case audits: {missing}"
    # and the catalogue reaches nothing the sweep does not know: the two sets are equal
    assert {t for t in tags if t.startswith(E.DISPATCHED)} == set(swept) - set(E.EXEMPT)


def test_exemptions_and_the_swept_set_are_disjoint(E):
    assert not (set(E.EXEMPT) & set(E.swept_symbols()))
    assert all(r for r in E.EXEMPT.values())


def test_sweep_reaches_every_threshold_of_the_dispatchers(E):
    """The grid crosses each dispatch threshold in both directions (a sweep that sat on one side of a rule would name too few kernels)."""
    swept = E.swept_symbols()
    for want in ("gemm_conv_kernel<5, false, false, false, false, 2>", "gemm_conv_kernel<5, false, false, false, false, 4>",
                 "gemm_conv_kernel<4, false, true, false, true, 4>", "big_tile_kernel<false, false, 8, 3, false>", "big_tile_kernel<false, false, 8, 4, false>",
                 "big_tile_kernel<true, false, 8, 6, false>", "big_tile_kernel<false, false, 8, 2, true>", "attn8_kernel<497>", "attn_kernel<40, 4, true>",
                 "attn_kernel<40, 2, true>", "attn_kernel<160, 2, false>"):
        assert want in swept, want


# ------------------------------------------------------------------------------------------------------------------ catalogue validity
def test_case_names_are_unique(E):
    names = [c.name for c in E.CASES]
    assert len(names) == len(set(names))


def test_every_block_is_accepted_and_lands_on_the_kernel_the_case_names(E, recorded):
    for c in E.CASES:
        rec = recorded[c.name]
        assert len(rec.calls) > 0, c.name
        tags = [t[0] for t in rec.tags]
        # ops.Recorder tags a block the library rejects with the launcher's own name
        assert "pv_gemm_conv" not in tags and "pv_attention" not in tags, (c.name, tags)
        for want in c.expect:
            assert want in tags, (c.name, want, tags)
        for fn, _ in rec.calls:
            assert fn.__name__ in A.REF, (c.name, fn.__name__)


def test_every_tensor_of_every_case_is_a_guarded_view(E, recorded):
    for name, rec in recorded.items():
        assert not E.unguarded(rec), (name, E.unguarded(rec))


def test_unguarded_finds_a_plain_tensor(E):
    ctx = E.Ctx("plain", "cpu")
    x = torch.zeros(65, 64, dtype=torch.float16)
    ctx.rec.layernorm(x, ctx.f(64), ctx.f(64), out=ctx.out(65, 64))
    assert E.unguarded(ctx.rec) == ["call 0 (pv_layernorm), field x"]


def test_catalogue_covers_every_inference_launcher(E, recorded):
    launchers = {fn.__name__ for rec in recorded.values() for fn, _ in rec.calls}
    assert launchers == set(A.REF) - {"pv_step_advance"}, set(A.REF) ^ launchers


# ------------------------------------------------------------------------------------------------------------------ the guards themselves
def test_a_store_into_any_margin_is_caught(E):
    """A fake kernel that writes its extent and one element more - the row in front, the row gap, the row behind, the far end of the arena."""
    arenas = []
    view = E.guarded_out(65, 160, torch.float16, 168, arenas=arenas)
    base = arenas[0][2]
    off = view.storage_offset()
    s = base.untyped_storage()
    before = PA.storage_bytes(s).clone()
    assert (before == E.OUT_FILL).all()
    view.fill_(1.0)
    assert PA.changed_outside(before, s, [view]) == 0
    for stray in (off - 1, off - 168 + 3, off + 160, off + 64 * 168 + 167, off + 65 * 168, off + 320 * 168 + 5, 0, base.numel() - 1):
        old = base[stray].item()
        base[stray] = 2.0
        assert PA.changed_outside(before, s, [view]) == 2, stray
        base.view(torch.int16)[stray] = torch.tensor(old).to(torch.float16).view(torch.int16)
    assert PA.changed_outside(before, s, [view]) == 0


def test_a_read_outside_an_input_extent_is_caught(E):
    """A fake kernel that reads one row past M (and "masks" it by multiplying with zero), one column into the row gap, one element in front."""
    g = torch.Generator().manual_seed(1)
    arenas = []
    a = E.guarded_in(h16(65, 64, g=g), 72, arenas=arenas)
    w = h16(128, 64, g=g, scale=0.125)
    p = SimpleNamespace(**{n: 0 for n in ("a1", "bias", "rowadd", "rowadd_ld", "residual", "splitk", "splitk_ws", "colstats", "ln_rowsum", "a_norm", "geglu", "act",
                                          "out_f32", "c1")}, c0=64, M=65, N=128, taps=1, hout=65, wout=1)
    exp = A.ref_gemm(p, dict(a0=a, w=w))
    good = (a.double() @ w.double().T).half()
    assert not PA.compare(exp, {"out": good})[0]
    base = arenas[0][2]
    off = a.storage_offset()
    tail = base[off:off + 66 * 72].view(66, 72)[:, :64]                       # 66 rows: one past the extent
    mask = torch.cat([torch.ones(65), torch.zeros(1)]).double()[:, None]
    masked = ((tail.double() * mask).sum(0, keepdim=True) @ w.double().T)     # 0 x NaN
    assert not torch.isfinite(masked).any()
    for over in (base[off:off + 65 * 72].view(65, 72)[:, 1:65], base[off - 72:off - 72 + 65 * 72].view(65, 72)[:, :64]):
        bad = (over.double() @ w.double().T).half()
        fails = PA.compare(exp, {"out": bad})[0]
        assert fails and "non-finite" in fails[0], fails
    idx = E.guarded_in(torch.tensor([3, 8], dtype=torch.int32))
    assert idx.tolist() == [3, 8] and E.guarded_in(torch.tensor([3, 8], dtype=torch.int32), arenas=arenas) is not None
    assert arenas[-1][2][0].item() == torch.iinfo(torch.int32).max


def test_guard_margins_hold_a_whole_stray_tile(E):
    arenas = []
    v = E.guarded_out(1, 160, torch.float16, 168, arenas=arenas)
    lo, hi, base = arenas[0]
    assert v.data_ptr() - lo >= E.TILE_ROWS * 168 * 2 and hi - (v.data_ptr() + 160 * 2) >= E.TILE_ROWS * 168 * 2
    assert v.data_ptr() % 16 == 0


# ------------------------------------------------------------------------------------------------------------------ reference checks
@pytest.mark.parametrize("geo", [(2, 5, 7, 2, 0), (2, 5, 7, 2, 1), (1, 7, 5, 2, 0), (2, 5, 7, 1, 1)])
def test_conv_reference_on_odd_sizes_matches_conv2d(geo):
    """pad = 0 is F.pad(x, (0, 1, 0, 1)) + Conv2d(stride=2, padding=0); on an odd size the padded row / column is read by no window."""
    b, hin, win, stride, pad = geo
    g = torch.Generator().manual_seed(2)
    x = h16(b * hin * win, 64, g=g)
    wt = h16(128, 64, 3, 3, g=g, scale=0.05)
    xn = x.reshape(b, hin, win, 64).permute(0, 3, 1, 2).double()
    y = F.conv2d(F.pad(xn, (0, 1, 0, 1)) if pad == 0 else xn, wt.double(), stride=stride, padding=pad)
    hout, wout = y.shape[2], y.shape[3]
    p = SimpleNamespace(**{n: 0 for n in ("a1", "bias", "rowadd", "rowadd_ld", "residual", "splitk", "splitk_ws", "colstats", "ln_rowsum", "a_norm", "geglu", "act",
                                          "out_f32", "c1", "upsample")}, c0=64, M=b * hout * wout, N=128, taps=9, batch=b, hin=hin, win=win, hout=hout, wout=wout,
                        stride=stride, pad=pad)
    got = A.ref_gemm(p, dict(a0=x, w=wt.permute(0, 2, 3, 1).reshape(128, -1).contiguous()))["out"].ref
    close(got, y.permute(0, 2, 3, 1).reshape(-1, 128))


def test_rowadd_per_image_with_a_boundary_inside_a_tile():
    g = torch.Generator().manual_seed(3)
    M, K, N, rpi = 65, 64, 128, 40                   # images of 40 rows: rows 40 .. 64 of the one 64-row tile belong to image 1
    x, w = h16(M, K, g=g), h16(N, K, g=g, scale=0.1)
    ra = torch.randn(2, N + 8, generator=g)[:, :N]
    p = SimpleNamespace(**{n: 0 for n in ("a1", "bias", "residual", "splitk", "splitk_ws", "colstats", "ln_rowsum", "a_norm", "geglu", "act", "out_f32", "c1")},
                        c0=K, M=M, N=N, taps=1, hout=rpi, wout=1, rowadd=1, rowadd_ld=N + 8, lda0=K, ldc=N)
    got = A.ref_gemm(p, dict(a0=x, w=w, rowadd=ra))["out"].ref
    exp = F.linear(x.double(), w.double())
    exp[:40] += ra[0].double()
    exp[40:] += ra[1].double()
    close(got, exp)
    assert A.layout_gemm(p)["rowadd"].rows == 2


@pytest.mark.parametrize("nq,nk", [(1, 65), (130, 63), (65, 1)])
def test_attention_reference_with_unequal_lengths_and_lse(nq, nk):
    g = torch.Generator().manual_seed(4)
    B, H, d = 2, 2, 40
    q, k, v = h16(B * nq, H * d, g=g), h16(B * nk, H * d, g=g), h16(B * nk, H * d, g=g)
    p = SimpleNamespace(batch=B, heads=H, nq=nq, nk=nk, d=d, causal=0, lse=1)
    res = A.ref_attention(p, dict(q=q, k=k, v=v, lse=torch.zeros(1)))
    hd = lambda t, n: t.double().reshape(B, n, H, d).transpose(1, 2)
    exp = F.scaled_dot_product_attention(hd(q, nq), hd(k, nk), hd(v, nk)).transpose(1, 2).reshape(B * nq, H * d)
    close(res["out"].ref, exp)
    s = hd(q, nq) @ hd(k, nk).transpose(2, 3) / math.sqrt(d)
    close(res["lse"].ref, (torch.logsumexp(s, 3) / math.log(2)).reshape(B * H, nq))
    L = A.layout_attention(SimpleNamespace(**vars(p), ldq=H * d, ldk=H * d, ldv=H * d, ldo=H * d))
    assert (L["lse"].rows, L["lse"].cols) == (B * H, nq) and (res["lse"].bound > 0).all()


def test_lnq_reference_without_image_tokens():
    g = torch.Generator().manual_seed(5)
    B, H, d, nq, nt = 1, 2, 80, 24, 80
    Cw = H * d
    hs, wq = h16(B * nq, Cw, g=g) * 2 + 0.5, h16(Cw, Cw, g=g, scale=0.05)
    kt, vt = h16(B * nt, Cw, g=g), h16(B * nt, Cw, g=g)
    p = SimpleNamespace(batch=B, heads=H, nq=nq, nt=nt, nip=0, d=d, w_text=1.0, w_ip=1.0, ln=1, ln_eps=1e-5)
    got = A.ref_xattn_lnq(p, dict(hs=hs, wq=wq, kt=kt, vt=vt))["out"].ref
    qn = F.linear(F.layer_norm(hs.double(), (Cw,), eps=1e-5), wq.double())
    hd = lambda t, n: t.double().reshape(B, n, H, d).transpose(1, 2)
    close(got, F.scaled_dot_product_attention(hd(qn, nq), hd(kt, nt), hd(vt, nt)).transpose(1, 2).reshape(B * nq, Cw))
    assert "kip" not in A.layout_xattn_lnq(SimpleNamespace(**vars(p), ld_hs=Cw, ldkt=Cw, ldvt=Cw, ldo=Cw, q_bias=0, wq_rowsum=0, vnorm=0, fusion=0))


def test_zero_variance_rows_and_groups_give_beta():
    g = torch.Generator().manual_seed(6)
    x = h16(4, 64, g=g)
    x[2] = -2.5
    gam, bet = torch.randn(1, 64, generator=g), torch.randn(1, 64, generator=g)
    y = A.ref_layernorm(SimpleNamespace(cols=64, eps=1e-5, act=0), dict(x=x, gamma=gam, beta=bet))["y"]
    assert torch.equal(y.ref[2], bet.double()[0]) and torch.isfinite(y.bound).all()
    xg = h16(2 * 9, 64, g=g)
    xg[:9, :2] = 1.25
    p = SimpleNamespace(batch=2, groups=32, hw=9, c0=64, c1=0, eps=1e-5, splits=1, act=0)
    mean, rstd, em, er = A.group_stats(p, dict(x0=xg))
    assert mean[0, 0].item() == 1.25 and abs(rstd[0, 0].item() - 1e-5 ** -0.5) < 1e-9 and torch.isfinite(er).all()
    close(torch.stack([mean, rstd], 2).reshape(2, 64)[1:], torch.stack([xg[9:].double().reshape(9, 32, 2).permute(1, 0, 2).reshape(32, -1).mean(1),
                                                                         1 / torch.sqrt(xg[9:].double().reshape(9, 32, 2).permute(1, 0, 2).reshape(32, -1).var(1, unbiased=False) + 1e-5)],
                                                                        1).reshape(1, 64))


def test_lnq_rejects_widths_its_gemm_cannot_walk(E):
    """pv_cross_attention_lnq walks K = C in 64-deep stages (nk = C / 64): C = 160 (2 heads of 80) or 480 would lose the last 32 columns of every row, so the
    launcher rejects any C that is no multiple of 320 before its first HIP call (found by the edge audit at C = 160), and the host never selects it there."""
    import ctypes as C
    from photoverse_amd import _lib
    from photoverse_amd.ops import Recorder
    lib = _lib.load()
    for heads, d in ((2, 80), (6, 80), (1, 160), (3, 160)):
        p = _lib.XAttnLnqParams()
        for k in ("hs", "wq", "q_bias", "wq_rowsum", "kt", "vt", "kip", "vip", "out"):
            setattr(p, k, 0x1000)                     # never dereferenced: the shape checks come first
        Cw = heads * d
        for k, v in dict(ld_hs=Cw, ln=1, ln_eps=1e-5, ldkt=Cw, ldvt=Cw, ldkip=Cw, ldvip=Cw, ldo=Cw, batch=2, nq=200, heads=heads, d=d, nt=77, nip=16, w_text=1.0,
                         w_ip=1.0).items():
            setattr(p, k, v)
        assert lib.pv_cross_attention_lnq(C.byref(p), None) == 1, (heads, d)
        assert not Recorder.xattn_lnq_supported(Cw, heads, 77, 16)
    assert Recorder.xattn_lnq_supported(1280, 8, 77, 1) and Recorder.xattn_lnq_supported(640, 8, 77, 6) and Recorder.xattn_lnq_supported(320, 4, 80, 0)
    for rec_case in ("lnq-d160-nip16-nt1", "lnq-d80-nip16-nt1-ln-fusion", "lnq-d80-nip0-nt80"):      # the catalogue's narrowest widths are the narrowest valid one
        with E.environment({}):
            p = E.build(E.by_name(rec_case)).calls[0][1][0]._obj
        assert p.heads * p.d == 320


# ------------------------------------------------------------------------------------------------------------------ the training tape's cases
def test_training_cases_give_every_leading_dimension_a_row_gap(E, recorded):
    """Every leading dimension a launch of a ``train-`` case passes is larger than the width of the buffer it strides (a kernel that took cols for ld,
    or wrote into the gap, would otherwise go unseen); the only contiguous ones are the two ``ldo == rows_pad`` transposes the catalogue asks for."""
    import ctypes as C
    seen = set()
    for name, rec in recorded.items():
        if not name.startswith("train-"):
            continue
        for fn, args in rec.calls:
            launcher, p, struct = E._call_params(fn, args)
            L = A.LAYOUT[launcher](p)
            names = [n for n, _ in type(struct)._fields_] if struct is not None else list(A.ARGS[launcher])
            for k in names:
                if not (k.startswith("ld") or k.endswith("_image_stride")) or not getattr(p, k):
                    continue
                val = getattr(p, k)
                strided = [b for b in L.values() if b is not None and b.ld == val]
                assert strided, (name, launcher, k)
                if launcher == "pv_transpose_f16" and k == "ldo" and p.ldo == p.rows_pad:
                    continue
                assert any(val > b.cols for b in strided), (name, launcher, k, val)      # (another buffer of the launch may share the value as its width)
                seen.add((launcher, k))
    assert {l for l, _ in seen} == {l for l in A.TRAINING if any(k.startswith("ld") or k.endswith("_image_stride") for k in A.ARGS.get(l, ("ldx",)))}


def test_training_cases_are_dry_recorded_with_flags_that_tell_their_variants_apart(E, recorded):
    """The coverage table's flags: the activation, forward / backward, the optional operands, the kernel form of pv_layernorm_backward."""
    flags = {}
    for name, rec in recorded.items():
        if name.startswith("train-"):
            for fn, args in rec.calls:
                launcher, p, _ = E._call_params(fn, args)
                flags.setdefault(launcher, set()).add(PA._flags(launcher, p))
    assert {f.split()[0] for f in flags["pv_act_backward"]} == {"act=none", "act=silu", "act=quick-gelu", "act=leaky-relu", "act=gelu"}
    assert any("vector" in f for f in flags["pv_layernorm_backward"]) and any("scalar" in f and "dgb_partial" in f for f in flags["pv_layernorm_backward"])
    assert len(flags["pv_dropout_f16"]) >= 10 and len(flags["pv_reduce_mean"]) == 6 and flags["pv_prelu_f16"] == {"", "dy"}
