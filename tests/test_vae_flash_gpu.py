"""GPU tests of the VAE's flash attention: ``pv_vae_attention`` alone against the fp64 reference of ``tests/_vae_flash_ref.py`` (every shape class, both
operand layouts, NaN around the operands and sentinels around the output, a moving and a far-off running maximum, determinism), and the model with
``enable_flash_attention()`` against the CPU oracle, against its own default path, and under tiling.

Measured on MI355X: see EXPERIMENTS.md, "VAE flash attention"."""
import pytest
import torch

from _vae_flash_ref import BOUND, DIMS, SHAPES, attention_ref, growing_case, peaked_case, randn_case, rel_l2
from test_vae_flash_cpu import TINY

pytestmark = pytest.mark.gpu
TOL = 5e-3                                       # the suite's standing VAE tolerance (tests/test_vae_gpu.py)
SENTINEL = 1234.0
WIDE = dict(TINY, block_out_channels=(128, 512))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _launch(q, k, v, out, *, batch, n, scale):
    from photoverse_amd.ops import Recorder
    rec = Recorder(torch.device("cuda"))
    rec.vae_attention(q, k, v, out, batch=batch, n=n, scale=scale)
    rec.run()
    torch.cuda.synchronize()


def _fused(q, k, v):
    """The three operands as column slices of one ``[rows][3d]`` buffer (the model's layout) and a compact output."""
    d = q.shape[1]
    qkv = torch.cat([q, k, v], 1).cuda().contiguous()
    return qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], torch.empty(q.shape[0], d, dtype=torch.float16, device="cuda")


def _padded(q, k, v, extra_rows=3):
    """Separate buffers with leading dimensions ``d + 8``, ``d + 16``, ``d + 24`` (``d + 40`` for the output) and ``extra_rows`` rows behind the last image: NaN
    in every input element that is not an operand element, a sentinel in every output element."""
    rows, d = q.shape
    views = []
    for t, pad in ((q, 8), (k, 16), (v, 24)):
        buf = torch.full((rows + extra_rows, d + pad), float("nan"), dtype=torch.float16, device="cuda")
        buf[:rows, :d] = t.cuda()
        views.append(buf[:rows, :d])
    out = torch.full((rows + extra_rows, d + 40), SENTINEL, dtype=torch.float16, device="cuda")
    return (*views, out)


def _run_fused(q, k, v, *, batch, n, scale):
    dq, dk, dv, out = _fused(q, k, v)
    _launch(dq, dk, dv, out, batch=batch, n=n, scale=scale)
    return out


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("batch,n", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_kernel_matches_the_fp64_reference(d, batch, n):
    """``randn`` operands (scaled scores ~N(0, 1)) in both layouts, rel-L2 <= 1e-3 against the fp64 reference.  In the padded layout the rows behind the
    last image and the columns between the operands' rows hold NaN, and the output buffer a sentinel: the result is finite, inside the bound, and
    every element outside ``out[r][0..d)``, ``r < batch * n``, still holds the sentinel."""
    _need_gpu()
    q, k, v = randn_case(d, batch, n)
    scale, rows = d ** -0.5, batch * n
    exp = attention_ref(q, k, v, batch=batch, n=n, scale=scale)
    got = _run_fused(q, k, v, batch=batch, n=n, scale=scale)
    e_fused = rel_l2(got, exp)
    dq, dk, dv, out = _padded(q, k, v)
    _launch(dq, dk, dv, out[:rows, :d], batch=batch, n=n, scale=scale)
    res = out[:rows, :d].clone()
    e_padded = rel_l2(res, exp)
    print(f"pv_vae_attention d = {d}, batch = {batch}, n = {n}: rel-L2 fused layout = {e_fused:.3e}, padded layout = {e_padded:.3e}")
    assert torch.isfinite(got).all() and torch.isfinite(res).all()
    assert e_fused <= BOUND and e_padded <= BOUND
    assert torch.equal(got, res)                                           # the layout is addressing only
    out[:rows, :d] = SENTINEL
    assert torch.equal(out, torch.full_like(out, SENTINEL))                # nothing else was written


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("d", DIMS)
def test_kernel_is_no_worse_than_the_default_recipe(d, n):
    """The shapes the default path accepts, batch 1: GEMM (fp16 scores) -> ``pv_softmax_rows`` (fp16 probabilities) -> GEMM on the same operands.  The
    flash error is inside the bound and at most 1.25 x the recipe's: both sit near the output-rounding floor, the quarter is summation-order noise."""
    _need_gpu()
    from photoverse_amd.ops import Recorder
    q, k, v = randn_case(d, 1, n)
    scale = d ** -0.5
    exp = attention_ref(q, k, v, batch=1, n=n, scale=scale)
    e_new = rel_l2(_run_fused(q, k, v, batch=1, n=n, scale=scale), exp)
    rec = Recorder(torch.device("cuda"))
    dq, dk, dvt = q.cuda(), k.cuda(), v.cuda().T.contiguous()              # V^T [d][n]: the recipe's second GEMM takes its weight as [N][K]
    scores = rec.gemm(dq, dk, splitk=0)
    rec.softmax_rows(scores, scale=scale)
    old = rec.gemm(scores, dvt, splitk=0)
    rec.run()
    torch.cuda.synchronize()
    e_old = rel_l2(old, exp)
    print(f"d = {d}, n = {n}: flash rel-L2 = {e_new:.3e}, default recipe rel-L2 = {e_old:.3e}")
    assert e_new <= BOUND and e_new <= 1.25 * e_old


@pytest.mark.parametrize("case", ["growing", "peaked"])
@pytest.mark.parametrize("d", DIMS)
def test_running_maximum(d, case):
    """Growing key norms (the row maximum rises by more than the kernel's lazy threshold at every tile: the rescale branch runs each time) and a peaked
    softmax with scaled scores to about +-60 (the CPU file checks both claims): the same bound, in the NaN-padded layout."""
    _need_gpu()
    (q, k, v), (batch, n) = (growing_case(d), (2, 200)) if case == "growing" else (peaked_case(d), (1, 129))
    scale, rows = d ** -0.5, batch * n
    exp = attention_ref(q, k, v, batch=batch, n=n, scale=scale)
    dq, dk, dv, out = _padded(q, k, v)
    _launch(dq, dk, dv, out[:rows, :d], batch=batch, n=n, scale=scale)
    got = out[:rows, :d]
    err = rel_l2(got, exp)
    print(f"pv_vae_attention d = {d}, {case} maximum: rel-L2 = {err:.3e}")
    assert torch.isfinite(got).all() and err <= BOUND


@pytest.mark.parametrize("d", DIMS)
def test_launches_are_deterministic_and_images_independent(d):
    _need_gpu()
    batch, n = 3, 200
    q, k, v = randn_case(d, batch, n)
    scale = d ** -0.5
    a = _run_fused(q, k, v, batch=batch, n=n, scale=scale)
    b = _run_fused(q, k, v, batch=batch, n=n, scale=scale)
    assert torch.equal(a, b)
    for i in range(batch):
        r = slice(i * n, (i + 1) * n)
        one = _run_fused(q[r], k[r], v[r], batch=1, n=n, scale=scale)
        assert torch.equal(one, a[r]), i


# ---------------------------------------------------------------------------------------------------------------- the model
def _pair(cfg, seed):
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.vae import AutoencoderKL
    torch.manual_seed(seed)
    ref = AutoencoderKLDecoderRef(**cfg, with_encoder=True).eval()
    hip = AutoencoderKL(**cfg)
    hip.load_state_dict(ref.state_dict())
    hip.to("cuda")
    return ref, hip


@pytest.fixture(scope="module")
def pair():
    _need_gpu()
    return _pair(TINY, 5)


@pytest.fixture(scope="module")
def wide_pair():
    _need_gpu()
    return _pair(WIDE, 6)


def _latents(B, h, w):
    return torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(100 * B + h + w))


def _pixels(B, H, W):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(100 * B + H + W)) * 2 - 1


def _flash(hip):
    class On:
        def __enter__(self):
            hip.enable_flash_attention()

        def __exit__(self, *a):
            hip.disable_flash_attention()
    return On()


@pytest.mark.parametrize("B,h,w", [(1, 16, 16), (3, 16, 16), (2, 5, 7), (1, 1, 1)])
@torch.no_grad()
def test_decode_with_flash_matches_the_oracle(pair, B, h, w):
    ref, hip = pair
    z = _latents(B, h, w)
    with _flash(hip):
        got = hip.decode(z.cuda()).sample
    err = rel_l2(got, ref.decode(z).sample)
    print(f"flash decode {B} x {h} x {w} (d = 256): rel-L2 vs oracle = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("H,W", [(128, 128), (40, 56)])
@torch.no_grad()
def test_encode_with_flash_matches_the_oracle(pair, H, W):
    from oracle.vae_ref import DiagonalGaussianRef
    ref, hip = pair
    x = _pixels(1, H, W)
    with _flash(hip):
        got = hip.encode(x.cuda()).latent_dist
    exp = DiagonalGaussianRef(ref.quant_conv(ref.encoder(x)))
    e_mean, e_logvar = rel_l2(got.mean, exp.mean), rel_l2(got.logvar, exp.logvar)
    print(f"flash encode {H} x {W} px (d = 256): mean rel-L2 = {e_mean:.3e}, logvar rel-L2 = {e_logvar:.3e}")
    assert e_mean < TOL and e_logvar < TOL


@pytest.mark.parametrize("B,h,w", [(1, 8, 8), (2, 3, 5)])
@torch.no_grad()
def test_decode_with_flash_at_width_512(wide_pair, B, h, w):
    ref, hip = wide_pair
    z = _latents(B, h, w)
    with _flash(hip):
        got = hip.decode(z.cuda()).sample
    err = rel_l2(got, ref.decode(z).sample)
    print(f"flash decode {B} x {h} x {w} (d = 512): rel-L2 vs oracle = {err:.3e}")
    assert err < TOL


@torch.no_grad()
def test_off_means_untouched():
    """A model that never enabled flash and the same weights after ``enable_flash_attention()`` / ``disable_flash_attention()``: bit-identical decode and
    encode.  The flash result in between differs from them by less than the VAE tolerance - and is not them."""
    _need_gpu()
    _, never = _pair(TINY, 5)
    _, hip = _pair(TINY, 5)
    z, x = _latents(2, 16, 16).cuda(), _pixels(2, 32, 32).cuda()
    base, base_m = never.decode(z).sample, never.encode(x).latent_dist.parameters
    assert never.use_flash_attention is False and all(key[-1] is False for key in never._plans)
    hip.enable_flash_attention()
    on, on_m = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
    hip.disable_flash_attention()
    off, off_m = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
    assert torch.equal(off, base) and torch.equal(off_m, base_m)
    assert {key[-1] for key in hip._plans} == {True, False}                 # one plan per form: neither replayed the other's
    e, e_m = rel_l2(on, base), rel_l2(on_m, base_m)
    print(f"flash on vs off: decode rel-L2 = {e:.3e}, moments rel-L2 = {e_m:.3e}")
    assert not torch.equal(on, base) and e < TOL and e_m < TOL


def test_launch_count_does_not_grow_with_the_batch(pair):
    """Four attention launches whatever the sub-batch with flash on (GroupNorm, fused QKV, ``pv_vae_attention``, ``to_out``); off, four per image."""
    _, hip = pair
    dev = torch.device("cuda")
    off1, off3 = len(hip._plan(1, 8, 8, dev).rec), len(hip._plan(3, 8, 8, dev).rec)
    with _flash(hip):
        p1, p3 = hip._plan(1, 8, 8, dev), hip._plan(3, 8, 8, dev)
        e1, e3 = hip._plan_encode(1, 16, 16, dev), hip._plan_encode(3, 16, 16, dev)
    assert len(p1.rec) == len(p3.rec) and len(e1.rec) == len(e3.rec)
    assert off3 > off1 and len(p1.rec) < off1                               # off: four launches per further image
    names = [t[0] for t in p3.rec.tags]
    assert names.count("vae_attn_kernel<256>") == 1 and not any("softmax" in nm for nm in names)


@torch.no_grad()
def test_flash_composes_with_tiling(pair):
    """``enable_tiling(16, 0.25)`` on 13 x 20 latents / 26 x 40 pixels (``tests/test_vae_tiling_gpu.py``'s geometry: tiles of 8, 7, 2 and 1 latents a side,
    token counts 64 down to 2): flash on against flash off."""
    _, hip = pair
    z, x = _latents(2, 13, 20).cuda(), _pixels(2, 26, 40).cuda()
    hip.enable_tiling(16, 0.25)
    try:
        off, off_m = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
        with _flash(hip):
            on, on_m = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
    finally:
        hip.disable_tiling()
    e, e_m = rel_l2(on, off), rel_l2(on_m, off_m)
    print(f"tiled, flash on vs off: decode rel-L2 = {e:.3e}, moments rel-L2 = {e_m:.3e}")
    assert on.shape == (2, 3, 26, 40) and e < TOL and e_m < TOL
