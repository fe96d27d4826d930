"""GPU tests of the T2I-Adapter pieces: ``pv_pixel_unshuffle8`` bit for bit against ``F.pixel_unshuffle``; ``pv_add_feature_rows`` against fp64 with derived
bounds, its scale table, its zero rows, its column statistics and their GroupNorm consumer; the adapter plan against the fp32 reference of
``tests/test_t2i_adapter_cpu.py``."""
import pytest
import torch
import torch.nn.functional as F

from test_controlnet_cpu import control_image
from test_pag_cpu import B, S, TOL_FWD, rel_l2
from test_t2i_adapter_cpu import TINY_CHANNELS, tiny_adapter_ref

pytestmark = pytest.mark.gpu

ADD = "pv_add_feature_rows"
#: (rows, cols, feat_rows, ldx): one block of one chunk; two blocks of 2.5 column groups, the features read twice; a partial last block, columns that are
#: no multiple of 128 and feature rows that are no multiple of 64; eight blocks with x as a column slice of a three times wider buffer
ADD_CASES = ((64, 8, 64, 8), (128, 320, 64, 320), (200, 328, 100, 328), (512, 640, 256, 3 * 640))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd import _lib
    return _lib.load()


def rows_of(t):
    """(B, C, H, W) -> rows [B*H*W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def planes_of(r, batch, h, w):
    return r.reshape(batch, h, w, -1).permute(0, 3, 1, 2)


def _ptr(t):
    return None if t is None else t.data_ptr()


def add_launch(lib, x, f, out, *, scale=1.0, tab=None, state=None, cs=None):
    rc = lib.pv_add_feature_rows(x.data_ptr(), x.stride(0), f.data_ptr(), f.stride(0), f.shape[0], out.data_ptr(), out.stride(0), x.shape[0], x.shape[1],
                                 float(scale), _ptr(tab), _ptr(state), _ptr(cs), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def blocks_sum(v, rows):
    """fp64 (sum, sum of squares) of ``v`` [rows][cols] per 64-row block -> [ceil(rows / 64)][2][cols], and the same of |v| / v^2 for the bounds"""
    nb = (rows + 63) // 64
    pad = torch.zeros(nb * 64, v.shape[1], dtype=torch.float64)
    pad[:rows] = v
    blk = pad.view(nb, 64, -1)
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], 1), torch.stack([blk.abs().sum(1), (blk * blk).sum(1)], 1)


# ---------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("case", (((2, 3, 16, 24), 2, 0), ((1, 1, 8, 8), 3, 0), ((2, 4, 8, 16), 2, 8)), ids=("2x3x16x24", "1to3x1x8x8", "2x4x8x16+ld"))
def test_pixel_unshuffle8_is_torch_pixel_unshuffle_bit_for_bit(lib, case):
    """fp16(F.pixel_unshuffle(img, 8)) laid out as rows, bit for bit; a batch stride of 0 broadcasts one image over three samples; ``ldo > cols`` leaves the
    gap columns alone; the image is unchanged."""
    shape, batch, gap = case
    g = torch.Generator().manual_seed(sum(shape))
    img = torch.randn(shape, generator=g) * 3
    n, c, h, w = shape
    cols = c * 64
    d_img = img.cuda().contiguous()
    wide = torch.full((batch * (h // 8) * (w // 8), cols + gap), 7.0, dtype=torch.float16, device="cuda")
    out = wide[:, :cols]
    rc = lib.pv_pixel_unshuffle8(d_img.data_ptr(), 0 if n != batch else c * h * w, out.data_ptr(), out.stride(0), batch, c, h, w,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    exp = rows_of(F.pixel_unshuffle(img.expand(batch, c, h, w), 8)).half()
    assert torch.equal(out.cpu().view(torch.int16), exp.view(torch.int16))
    assert torch.equal(d_img.cpu(), img) and (gap == 0 or bool((wide[:, cols:] == 7.0).all()))


@pytest.mark.parametrize("case", ADD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_add_feature_rows_against_fp64(lib, case):
    """Outputs: ``|got - exact| <= (2^-11 + 2^-22) |exact| + 2^-25`` - one fp32 fma (relative 2^-24, absorbed with margin by the 2^-22 term and the absolute
    term) and one fp16 rounding (2^-11).  Statistics against fp64 sums of the launch's own outputs: ``|dsum| <= 64 * 2^-24 * sum |v|`` and
    ``|dsumsq| <= 64 * 2^-24 * sum v^2`` (at most 64 fp32 additions per column and block; v^2 of an fp16 value is exact in fp32).  Inputs unchanged; with and
    without statistics the outputs have the same bits.
    Measured on MI355X (printed with -s), in the order of ADD_CASES: worst |got - exact| / bound 0.991, 0.999, 0.999, 0.999 (the fp16 half-ulp, which the bound
    is); statistics worst |d| / bound 0.034, 0.058, 0.055, 0.062."""
    rows, cols, feat_rows, ldx = case
    g = torch.Generator().manual_seed(rows + cols)
    s = 0.7
    xw = torch.randn(rows, ldx, generator=g).half()
    f = torch.randn(feat_rows, cols, generator=g).half()
    d_xw, d_f = xw.cuda(), f.cuda()
    d_x = d_xw[:, ldx - cols:]
    x = xw[:, ldx - cols:]
    out = torch.full((rows, cols), float("nan"), dtype=torch.float16, device="cuda")
    out2 = torch.full_like(out, float("nan"))
    cs = torch.full(((rows + 63) // 64, 2, cols), float("nan"), dtype=torch.float32, device="cuda")
    add_launch(lib, d_x, d_f, out, scale=s, cs=cs)
    add_launch(lib, d_x, d_f, out2, scale=s)
    torch.cuda.synchronize()
    s32 = torch.tensor(s, dtype=torch.float32).double()
    exact = x.double() + s32 * f.double().repeat(rows // feat_rows, 1)
    got = out.cpu().double()
    bound = (2.0 ** -11 + 2.0 ** -22) * exact.abs() + 2.0 ** -25
    ratio = ((got - exact).abs() / bound).max().item()
    ref_cs, bound_cs = blocks_sum(got, rows)
    r_cs = ((cs.cpu().double() - ref_cs).abs() / (64 * 2.0 ** -24 * bound_cs).clamp_min(1e-300)).max().item()
    print(f"add_feature_rows {case}: worst |got - exact| / bound = {ratio:.3f}; statistics worst |d| / bound = {r_cs:.3f}")
    assert torch.isfinite(got).all() and ratio <= 1.0
    assert torch.isfinite(cs).all() and r_cs <= 1.0
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(d_xw.cpu(), xw) and torch.equal(d_f.cpu(), f)


def test_add_feature_rows_scale_table_zero_rows_and_graph_replay(lib):
    """The scale comes from the table at ``state[0]`` (rows 0 and 3 of a table with a different value per row), a zero row gives the bits of ``x`` - and
    ``x``'s statistics - with ``f`` full of NaN, the host ``scale`` is used when the table is NULL, and an eager launch and a graph replay give the same
    bits, statistics included."""
    rows, cols, feat_rows = 128, 320, 64
    g = torch.Generator().manual_seed(9)
    x, f = torch.randn(rows, cols, generator=g).half(), torch.randn(feat_rows, cols, generator=g).half()
    d_x, d_f = x.cuda(), f.cuda()
    tab = torch.tensor([0.5, 0.0, -1.25, 2.0], dtype=torch.float32, device="cuda")
    state = torch.tensor([0, 4, 0, 0], dtype=torch.int32, device="cuda")
    out = torch.empty((rows, cols), dtype=torch.float16, device="cuda")
    cs = torch.empty((2, 2, cols), dtype=torch.float32, device="cuda")
    frep = f.double().repeat(rows // feat_rows, 1)

    def check(s):
        exact = x.double() + float(s) * frep
        got = out.cpu().double()
        assert ((got - exact).abs() <= (2.0 ** -11 + 2.0 ** -22) * exact.abs() + 2.0 ** -25).all(), s

    for row in (0, 3, 2):
        state[0] = row
        out.fill_(float("nan"))
        add_launch(lib, d_x, d_f, out, scale=100.0, tab=tab, state=state, cs=cs)      # the host scale is ignored beside a table
        torch.cuda.synchronize()
        check(tab[row].item())
    # a zero row: the bits of x, f never read
    state[0] = 1
    nan_f = torch.full_like(d_f, float("nan"))
    out.fill_(float("nan"))
    add_launch(lib, d_x, nan_f, out, tab=tab, state=state, cs=cs)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int16), x.view(torch.int16))
    ref_cs, bound_cs = blocks_sum(x.double(), rows)
    assert ((cs.cpu().double() - ref_cs).abs() <= 64 * 2.0 ** -24 * bound_cs).all()
    out.fill_(float("nan"))
    add_launch(lib, d_x, nan_f, out, scale=0.0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int16), x.view(torch.int16))
    # a step counter past the table's end re-reads the last row
    state[0] = 9
    add_launch(lib, d_x, d_f, out, tab=tab, state=state)
    torch.cuda.synchronize()
    check(2.0)
    # the host scale
    add_launch(lib, d_x, d_f, out, scale=-0.375)
    torch.cuda.synchronize()
    check(-0.375)
    # eager == graph replay
    state[0] = 2
    add_launch(lib, d_x, d_f, out, tab=tab, state=state, cs=cs)
    torch.cuda.synchronize()
    eager, eager_cs = out.clone(), cs.clone()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        add_launch(lib, d_x, d_f, out, tab=tab, state=state, cs=cs)
    out.fill_(float("nan"))
    cs.fill_(float("nan"))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16)) and torch.equal(cs.view(torch.int32), eager_cs.view(torch.int32))


def test_groupnorm_consumes_the_statistics_of_add_feature(lib):
    """``Recorder.add_feature(colstats=True)`` followed by ``Recorder.groupnorm`` takes the ``pv_groupnorm_stats_from_colstats`` path; without the statistics
    GroupNorm runs its own pass over the same tensor.  The (mean, rstd) of the two agree within fp32 summation error - 1280 elements per (image, group):
    ``|d mean| <= 1e-4 mean|v|``, rstd to 1e-4 relative, both above the worst-case 1280 * 2^-24 = 7.6e-5 - and the normalised outputs differ by at most
    one fp16 rounding."""
    from photoverse_amd.ops import Recorder
    batch, hw, cols = 2, 128, 320
    g = torch.Generator().manual_seed(12)
    x, f = torch.randn(batch * hw, cols, generator=g).half().cuda(), torch.randn(hw, cols, generator=g).half().cuda()
    gamma, beta = (1 + 0.1 * torch.randn(cols, generator=g)).cuda(), (0.1 * torch.randn(cols, generator=g)).cuda()
    res = []
    for colstats in (True, False):
        rec = Recorder("cuda")
        y0 = rec.add_feature(x, f, scale=0.8, colstats=colstats)
        y, stats = rec.groupnorm(y0, gamma, beta, batch=batch, hw=hw, return_stats=True)
        names = [fn.__name__ for fn, _ in rec.calls]
        assert names == [ADD, "pv_groupnorm_stats_from_colstats" if colstats else "pv_groupnorm_stats", "pv_groupnorm_apply"]
        rec.run()
        torch.cuda.synchronize()
        res.append((y0.clone(), y.float().cpu(), stats[:, :64].reshape(batch, 32, 2).double().cpu()))      # (mean, rstd) at stats[b, 2 g : 2 g + 2]
    (a0, ya, sa), (b0, yb, sb) = res
    assert torch.equal(a0.view(torch.int16), b0.view(torch.int16))
    mean_abs = a0.float().abs().mean().item()
    assert ((sa[..., 0] - sb[..., 0]).abs() <= 1e-4 * mean_abs).all() and ((sa[..., 1] - sb[..., 1]).abs() <= 1e-4 * sb[..., 1].abs()).all()
    assert ((ya - yb).abs() <= 2.0 ** -10 * yb.abs() + 2.0 ** -24).all()
    exp = F.group_norm(planes_of(a0.float().cpu(), batch, 8, 16), 32, gamma.cpu(), beta.cpu(), eps=1e-5)
    assert rel_l2(planes_of(ya, batch, 8, 16), exp) <= TOL_FWD


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def tiny_models():
    """(adapter reference, HIP adapter): the tiny configuration, the HIP model loaded from the reference's state dict."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.t2i_adapter import T2IAdapter
    ad_ref = tiny_adapter_ref()
    ad = T2IAdapter(in_channels=3, channels=TINY_CHANNELS)
    ad.load_state_dict(ad_ref.state_dict(), strict=True)
    ad.to("cuda")
    return ad_ref, ad


@pytest.fixture(scope="module")
def images():
    return control_image(), control_image(seed=6)


RES = ["pv_gemm_conv", "pv_prelu_f16", "pv_gemm_conv"]
PLAN_NAMES = ["pv_pixel_unshuffle8", "pv_gemm_conv"] + RES * 2 + ["pv_token_pool", "pv_gemm_conv"] + RES * 2


@torch.no_grad()
@pytest.mark.parametrize("s", (S, 20, 5), ids=("S16", "S20", "S5"))
def test_adapter_plan_matches_the_reference(tiny_models, images, s):
    """Both features of a (2, 3, 8 s, 8 s) image against ``T2IAdapterRef``: rel-L2 <= TOL_FWD; a second image through the same recorder moves them by more
    than 100 x TOL_FWD; the launch names are as designed, ``pv_pixel_unshuffle8`` first.  s = 20 pools to 10, s = 5 to the odd 3 (edge blocks average
    what they have).  Measured on MI355X (printed with -s): rel-L2 4.648e-4 / 5.529e-4 (S = 16), 4.674e-4 / 5.721e-4 (S = 20), 4.622e-4 / 5.809e-4 (S = 5); on
    the reference the second image's features are 4.5e-1 .. 6.8e-1 from the first's."""
    from photoverse_amd.ops import Recorder
    from photoverse_amd.t2i_adapter import adapter_plan, feature_sizes
    ad_ref, ad = tiny_models
    img, img2 = (images if s == S else (control_image(size=8 * s), control_image(size=8 * s, seed=6)))
    d_img = img.cuda().contiguous()
    sizes = feature_sizes(s, s, 2)
    assert sizes == [(s, s), (-(-s // 2), -(-s // 2))]
    outs = [torch.full((B * hk * wk, c), float("nan"), dtype=torch.float16, device="cuda") for (hk, wk), c in zip(sizes, TINY_CHANNELS)]
    rec = Recorder("cuda")
    assert adapter_plan(rec, ad, d_img, outs)[0] is outs[0]
    assert [fn.__name__ for fn, _ in rec.calls] == PLAN_NAMES and rec.tags[0][0] == "pixel_unshuffle8_kernel"
    rec.run()
    torch.cuda.synchronize()
    exp = ad_ref(img)
    first = [o.float().cpu() for o in outs]
    for k, (got, e, (hk, wk)) in enumerate(zip(first, exp, sizes)):
        err = rel_l2(planes_of(got, B, hk, wk), e)
        print(f"adapter feature {k} {tuple(e.shape)}: rel-L2 vs T2IAdapterRef = {err:.3e}")
        assert torch.isfinite(got).all() and err <= TOL_FWD
    d_img.copy_(img2)
    rec.run()
    torch.cuda.synchronize()
    exp2 = ad_ref(img2)
    for k, (o, e, e1, (hk, wk)) in enumerate(zip(outs, exp2, exp, sizes)):
        assert rel_l2(planes_of(o.float().cpu(), B, hk, wk), e) <= TOL_FWD and rel_l2(o.float().cpu(), first[k]) > 100 * TOL_FWD
    if s == S:
        nchw = ad(img2)                                      # the inspection entry point: fp32 NCHW, a single image is its own batch
        assert [tuple(t.shape) for t in nchw] == [tuple(e.shape) for e in exp2] and all(rel_l2(t.cpu(), e) <= TOL_FWD for t, e in zip(nchw, exp2))
