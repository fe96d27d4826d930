"""GPU tests of tiled VAE decode / encode: ``pv_tile_blend`` alone against the fp64 recursion of ``tests/test_vae_tiling_cpu.py``; ``tiled_decode`` /
``tiled_encode`` of the tiny VAE (``enable_tiling(16, 0.25)``: latent tile 8 at stride 6, blend 4 pixels / 2 latents) against the CPU oracle's result of
every tile blended by that recursion; the dispatch rule, sub-batch invariance, ``run_inference`` and the ``generate.py`` flags."""
import pytest
import torch

from test_vae_gpu import rel_l2
from test_vae_tiling_cpu import TINY, blend_h_ref, blend_v_ref, tiled_ref

pytestmark = pytest.mark.gpu
TOL = 5e-3                                       # the VAE tolerance of tests/test_vae_gpu.py; a blend is a convex combination and adds nothing to it
GEO_DEC = dict(tile=8, stride=6, blend=4, keep=12)
GEO_ENC = dict(tile=16, stride=12, blend=2, keep=6)
DECODE_CASES = [(1, 13, 20), (3, 13, 20), (1, 16, 16), (3, 16, 16), (1, 8, 14), (3, 8, 14)]
ENCODE_CASES = [(1, 26, 40), (2, 32, 32)]


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.vae import AutoencoderKL
    torch.manual_seed(5)
    ref = AutoencoderKLDecoderRef(**TINY, with_encoder=True).eval()
    hip = AutoencoderKL(**TINY)
    hip.load_state_dict(ref.state_dict())
    hip.to("cuda")
    hip.enable_tiling(16, 0.25)
    return ref, hip


def _latents(B, h, w):
    return torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(100 * B + h + w))


def _pixels(B, H, W):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(100 * B + H + W)) * 2 - 1


@pytest.fixture(scope="module")
def decode_refs(pair):
    """Per decode case, computed once on the CPU: the oracle's decode of every tile blended by the fp64 recursion, and the oracle's untiled decode."""
    ref, _ = pair
    with torch.no_grad():
        return {c: (tiled_ref(_latents(*c), lambda t: ref.decode(t).sample, out_h=2 * c[1], out_w=2 * c[2], **GEO_DEC), ref.decode(_latents(*c)).sample)
                for c in DECODE_CASES}


# ---------------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("neighbours", ["none", "above", "left", "both"])
@pytest.mark.parametrize("th,tw", [(16, 16), (16, 4), (2, 16), (3, 5)])
def test_tile_blend_kernel_matches_the_fp64_recursion(th, tw, neighbours):
    """``pv_tile_blend`` on random tiles: channels 3 and 8, batch 1 and 2, blend extents 4 (the 16-byte path where the widths allow it) and 6 (scalar;
    wider than the 4- and 5-wide and higher than the 2- and 3-high tiles, whose ``e`` is then the tile's own extent), neighbours of 16 and of 3 rows /
    columns (the second shorter than the extent), and two pictures: one with room around the kept region and one whose edge clips it.
    Bound ``|got - ref| <= 16 * 2^-24 * max|input|``: two successive lerps, each at most five fp32 roundings (the weight, one minus it, two products,
    the sum) of quantities bounded by the maximum, the first lerp's error carried into the second at weight <= 1."""
    from photoverse_amd.ops import tile_blend
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    g = torch.Generator().manual_seed(th * 100 + tw)
    SENTINEL, K = 12345.0, 12
    has_a, has_l = neighbours in ("above", "both"), neighbours in ("left", "both")
    for ch in (3, 8):
        for B in (1, 2):
            for E, n_ext in ((4, 16), (6, 16), (6, 3)):
                for clipped in (False, True):
                    tile = torch.randn(B, ch, th, tw, generator=g) * 3
                    above = torch.randn(B, ch, n_ext, tw, generator=g) * 3 if has_a else None
                    left = torch.randn(B, ch, th, n_ext, generator=g) * 3 if has_l else None
                    ev = min(n_ext, th, E) if has_a else 0
                    eh = min(n_ext, tw, E) if has_l else 0
                    oy, ox = (12 if has_a else 0), (12 if has_l else 0)
                    out_h, out_w = (oy + min(th, 5), ox + min(tw, 8)) if clipped else (oy + th + 3, ox + tw + 4)
                    kh, kw = min(K, th, out_h - oy), min(K, tw, out_w - ox)
                    exp = tile.double()
                    if has_a:
                        exp = blend_v_ref(above, exp, E)
                    if has_l:
                        exp = blend_h_ref(left, exp, E)
                    d_tile, d_out = tile.cuda(), torch.full((B, ch, out_h, out_w), SENTINEL, device="cuda")
                    tile_blend(d_tile, None if above is None else above.cuda(), None if left is None else left.cuda(), d_out, ev=ev, eh=eh, keep_h=kh,
                               keep_w=kw, oy=oy, ox=ox)
                    got_tile, got_out = d_tile.cpu().double(), d_out.cpu().double()
                    bound = 16 * 2.0 ** -24 * max(t.abs().max().item() for t in (tile, above, left) if t is not None)
                    what = (ch, B, E, n_ext, clipped)
                    assert (got_tile - exp).abs().max().item() <= bound, what                       # in place: what the next tiles read
                    assert torch.equal(got_tile[:, :, ev:, eh:], tile.double()[:, :, ev:, eh:]), what   # untouched outside the blends, bit for bit
                    assert (got_out[:, :, oy:oy + kh, ox:ox + kw] - exp[:, :, :kh, :kw]).abs().max().item() <= bound, what
                    assert torch.equal(got_out[:, :, oy:oy + kh, ox:ox + kw], got_tile[:, :, :kh, :kw]), what
                    got_out[:, :, oy:oy + kh, ox:ox + kw] = SENTINEL
                    assert torch.equal(got_out, torch.full_like(got_out, SENTINEL)), what           # nothing outside the kept region is written


# ---------------------------------------------------------------------------------------------------------------- decode / encode
def test_the_tiled_reference_is_a_target_of_its_own(decode_refs):
    """The precondition, on the CPU oracle alone: the blended tiles differ from the untiled decode by far more than the tolerance (random weights: the
    GroupNorm statistics and the attention of a tile are not the picture's), so a ``tiled_decode`` that decoded in one piece could not pass.  Measured:
    rel-L2 0.37 ... 0.54 over the six cases."""
    for c, (tiled, whole) in decode_refs.items():
        d = rel_l2(tiled, whole)
        print(f"oracle, latents {c}: tiled vs untiled rel-L2 = {d:.3e}")
        assert d > 10 * TOL, c


@pytest.mark.parametrize("B,h,w", DECODE_CASES)
def test_tiled_decode_matches_the_blended_oracle_tiles(pair, decode_refs, B, h, w):
    """13 x 20: rows 8 / 7 / 1, columns 8 / 8 / 8 / 2; 16 x 16: 8 / 8 / 4 both ways; 8 x 14: rows 8 / 2 (a second tile row starts at 6, as in diffusers' loop), columns 8 / 8 / 2."""
    _, hip = pair
    with torch.no_grad():
        got = hip.tiled_decode(_latents(B, h, w).cuda()).sample
    exp = decode_refs[(B, h, w)][0]
    assert got.shape == exp.shape == (B, 3, 2 * h, 2 * w) and got.dtype == torch.float32
    err = rel_l2(got, exp)
    print(f"tiled_decode {B} x {h} x {w}: rel-L2 vs blended oracle tiles = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("B,H,W", ENCODE_CASES)
def test_tiled_encode_matches_the_blended_oracle_tiles(pair, B, H, W):
    from oracle.vae_ref import DiagonalGaussianRef
    ref, hip = pair
    x = _pixels(B, H, W)
    with torch.no_grad():
        exp_m = tiled_ref(x, lambda t: ref.quant_conv(ref.encoder(t)), out_h=H // 2, out_w=W // 2, **GEO_ENC)
        whole = ref.quant_conv(ref.encoder(x))
        got = hip.tiled_encode(x.cuda()).latent_dist
    exp = DiagonalGaussianRef(exp_m)
    assert got.mean.shape == exp.mean.shape == (B, 4, H // 2, W // 2)
    e_mean, e_logvar, apart = rel_l2(got.mean, exp.mean), rel_l2(got.logvar, exp.logvar), rel_l2(exp_m, whole)
    print(f"tiled_encode {B} x {H} x {W}: mean rel-L2 = {e_mean:.3e}, logvar rel-L2 = {e_logvar:.3e}; oracle tiled vs untiled = {apart:.3e}")
    assert apart > 10 * TOL
    assert e_mean < TOL and e_logvar < TOL


def test_untiled_plans_take_token_counts_off_the_gemm_tile(pair, decode_refs):
    """What every edge tile relies on, on the untiled path where it is easiest to see: a mid-block attention over h * w = 260 tokens (neither a multiple
    of 128 nor of 320) pads its key axis to 384 and masks the padding.  B = 3: an image's padded key window runs into the next image's keys."""
    ref, hip = pair
    x = _pixels(3, 26, 40)
    hip.disable_tiling()
    try:
        with torch.no_grad():
            got = hip.decode(_latents(3, 13, 20).cuda()).sample
            got_m = hip.encode(x.cuda()).latent_dist.parameters
            exp_m = ref.quant_conv(ref.encoder(x))
    finally:
        hip.enable_tiling(16, 0.25)
    assert rel_l2(got, decode_refs[(3, 13, 20)][1]) < TOL
    assert rel_l2(got_m, exp_m) < TOL


# ---------------------------------------------------------------------------------------------------------------- host layer
def test_dispatch_by_size_and_switch(pair):
    _, hip = pair
    small, big = _latents(2, 8, 8).cuda(), _latents(2, 13, 20).cuda()
    x_small, x_big = _pixels(2, 16, 16).cuda(), _pixels(2, 26, 40).cuda()
    with torch.no_grad():
        assert hip.use_tiling
        on_small, on_big, tiled_big = hip.decode(small).sample, hip.decode(big).sample, hip.tiled_decode(big).sample
        on_xs, on_xb, tiled_xb = (f(v).latent_dist.parameters for f, v in ((hip.encode, x_small), (hip.encode, x_big), (hip.tiled_encode, x_big)))
        hip.disable_tiling()
        try:
            off_small, off_big = hip.decode(small).sample, hip.decode(big).sample
            off_xs, off_xb = hip.encode(x_small).latent_dist.parameters, hip.encode(x_big).latent_dist.parameters
        finally:
            hip.enable_tiling(16, 0.25)
        again = hip.decode(big).sample
    assert torch.equal(on_small, off_small) and torch.equal(on_xs, off_xs)          # one tile or less: the untiled path and its bits
    assert torch.equal(on_big, tiled_big) and torch.equal(on_xb, tiled_xb)
    assert not torch.equal(off_big, on_big) and rel_l2(off_big, on_big) > 10 * TOL  # disable_tiling() restores the untiled result ...
    assert not torch.equal(off_xb, on_xb)
    assert torch.equal(again, on_big)                                               # ... and enabling it again the tiled one


def test_tile_sub_batches_do_not_change_the_bits(pair):
    """13 x 20 at B = 3: a tile row holds 9 tiles of 8 x 8 and 3 of 8 x 2 - one plan run each by default.  With ``MAX_OPERAND_BYTES`` at two 8 x 8 tiles'
    worth of the widest activation (256 channels x 16 x 16 pixels x 2 bytes) the same tiles go through plans of sub-batch 2."""
    _, hip = pair
    z, x = _latents(3, 13, 20).cuda(), _pixels(3, 26, 40).cuda()
    with torch.no_grad():
        a, ea = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
        keys = set(hip._plans)
        hip.MAX_OPERAND_BYTES = 256 * 16 * 16 * 2 * 2
        try:
            b, eb = hip.decode(z).sample, hip.encode(x).latent_dist.parameters
        finally:
            del hip.MAX_OPERAND_BYTES
    assert type(hip).MAX_OPERAND_BYTES == 1 << 30
    new = set(hip._plans) - keys
    assert any(k[0] == 2 for k in new) and any(k[0] == "enc" for k in new), new     # other plans did run
    assert torch.equal(a, b) and torch.equal(ea, eb)


def test_run_inference_decodes_through_the_tiles(pair):
    """A plain single-pass ``run_inference`` at 16 x 16 latents (three tiles a side) with the tiling-enabled VAE: finite, the right shape, the same on
    a second call, and not the untiled picture."""
    from photoverse_amd.infer import run_inference
    from photoverse_amd.modeling_utils import load_models
    from oracle.unet_ref import TINY_CONFIG
    _, hip_vae = pair
    vis = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, image_size=56, patch_size=14)
    txt = dict(vocab_size=49408, hidden_size=768, num_attention_heads=12, intermediate_size=512, num_hidden_layers=1)
    tok, te, vae, unet, ie, ia, ta, sch, _ = load_models(None, 1, unet_config=TINY_CONFIG, vision_config=vis, text_config=txt, seed=3)
    for m in (unet, te, ie, ia, ta):
        m.to("cuda")
    g = torch.Generator().manual_seed(4)
    ex = {"pixel_values": torch.zeros(2, 3, 32, 32), "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=2, seed=1)
    with torch.no_grad():
        a = run_inference(ex, tok, ie, te, unet, ta, ia, hip_vae, sch, "cuda", [1], **kw)
        b = run_inference(ex, tok, ie, te, unet, ta, ia, hip_vae, sch, "cuda", [1], **kw)
        lat = run_inference(ex, tok, ie, te, unet, ta, ia, None, sch, "cuda", [1], **kw)
        exp = hip_vae.tiled_decode(lat / hip_vae.config.scaling_factor).sample.clamp(-1, 1)
        hip_vae.disable_tiling()
        try:
            c = run_inference(ex, tok, ie, te, unet, ta, ia, hip_vae, sch, "cuda", [1], **kw)
        finally:
            hip_vae.enable_tiling(16, 0.25)
    assert a.shape == (2, 3, 32, 32) and torch.isfinite(a).all() and a.min() >= -1 and a.max() <= 1
    assert torch.equal(a, b) and torch.equal(a, exp)
    assert c.shape == a.shape and not torch.allclose(a, c)


def test_generate_cli_runs_with_the_vae_tiling_flags(tmp_path):
    """generate.py --vae_tiling --vae_tile_size 64 --vae_tile_overlap 0.25 runs as a program and writes its PNGs: the --tiny VAE has four levels
    (up = 8), so the 16 x 16 latents are decoded in 8 x 8 latent tiles at stride 6 (three a side, the last 4 wide)."""
    import os
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--vae_tiling", "--vae_tile_size", "64", "--vae_tile_overlap", "0.25", "--num_timesteps", "4",
           "--num_of_samples", "2", "--seed", "3", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
