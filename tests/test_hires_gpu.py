"""GPU tests of two-pass high-resolution generation: ``pv_resize_bilinear_affine_f32`` against the fp64 evaluation of the header's formula
(``test_hires_cpu.bilinear_ref``), ``hires_start`` against ``add_noise(F.interpolate(...))`` in fp64, the second pass on the tiny UNet against the fp32
oracle (UNet + DPMSolverMultistepRef), and ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_hires_cpu import SHAPES, bilinear_ref

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_bilinear_affine_kernel(rec_cls, shape):
    """``pv_resize_bilinear_affine_f32`` with and without the ``(ca, y, cb)`` term (a different ``ca[b]``, ``cb[b]`` per sample) against the fp64
    evaluation of the header's formula on the same fp32 inputs, rtol = atol = 1e-5 (the bound of ``test_cfg_dpm_step_kernel`` and
    ``test_masked_step_kernel``; torch's own fp32 CPU bilinear is within 3.4e-6 of that formula on these shapes).  The equal-size plain form is ``x``
    bit for bit, the four inputs are unchanged after the launch and ``out=`` returns the tensor it was given.
    Measured on MI355X, max abs error plain / affine (printed with -s): 1.6e-7 / 2.2e-7, 1.8e-7 / 2.9e-7, 3.4e-7 / 2.3e-7, 2.1e-7 / 2.6e-7, 0 / 1.0e-8, 0 / 1.5e-7 for the six shapes."""
    B, C, h, w, oh, ow = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, y = torch.randn(B, C, h, w, generator=g), torch.randn(B, C, oh, ow, generator=g)
    ca, cb = torch.rand(B, generator=g) + 0.5, torch.rand(B, generator=g) - 0.5
    if B > 1:
        assert ca[0] != ca[1] and cb[0] != cb[1]
    dx, dy, dca, dcb = x.cuda(), y.cuda(), ca.cuda(), cb.cuda()
    given = torch.full((B, C, oh, ow), float("nan"), device="cuda")
    rec = rec_cls("cuda")
    plain = rec.resize_bilinear_affine(dx, (oh, ow))
    full = rec.resize_bilinear_affine(dx, (oh, ow), dca, dy, dcb)
    scaled = rec.resize_bilinear_affine(dx, (oh, ow), dca)                 # ca alone
    assert rec.resize_bilinear_affine(dx, (oh, ow), dca, dy, dcb, out=given) is given
    rec.run()
    torch.cuda.synchronize()
    assert plain.shape == full.shape == (B, C, oh, ow) and plain.dtype == torch.float32
    exp_plain, exp_full = bilinear_ref(x, oh, ow), bilinear_ref(x, oh, ow, ca, y, cb)
    e0, e1 = (plain.cpu().double() - exp_plain).abs().max().item(), (full.cpu().double() - exp_full).abs().max().item()
    print(f"resize_bilinear_affine {shape}: max abs error vs fp64 plain {e0:.3e}, affine {e1:.3e}")
    torch.testing.assert_close(plain.cpu().double(), exp_plain, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(full.cpu().double(), exp_full, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(scaled.cpu().double(), bilinear_ref(x, oh, ow, ca), rtol=1e-5, atol=1e-5)
    assert torch.equal(given, full)
    if (h, w) == (oh, ow):
        assert torch.equal(plain.cpu(), x)                                 # the weights are exactly 0
    assert torch.equal(dx.cpu(), x) and torch.equal(dy.cpu(), y) and torch.equal(dca.cpu(), ca) and torch.equal(dcb.cpu(), cb)
    if oh == ow:
        rec2 = rec_cls("cuda")
        sq = rec2.resize_bilinear_affine(dx, oh)                          # one int: both axes
        rec2.run()
        assert torch.equal(sq, plain)


def test_hires_start_is_add_noise_of_the_upscaled_latents(rec_cls):
    """16 -> 32, 6 steps, strength 0.5: ``start == 3`` and ``x_start`` within rtol = atol = 1e-5 of ``sqrt(acp[t]) * F.interpolate(latents) +
    sqrt(1 - acp[t]) * noise`` in fp64 with the scheduler's own ``alphas_cumprod``.  Measured on MI355X: max abs error 2.0e-7 (printed with -s)."""
    from photoverse_amd.infer import hires_start
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(71)
    lat, noise = torch.randn(2, 4, 16, 16, generator=g) * 0.8, torch.randn(2, 4, 32, 32, generator=g)
    sch = DPMSolverMultistepScheduler()
    x_start, start = hires_start(lat.cuda(), noise.cuda(), sch, 6, 0.5)
    torch.cuda.synchronize()
    assert start == 3 and x_start.shape == (2, 4, 32, 32) and x_start.is_cuda
    acp = float(sch.alphas_cumprod[int(sch.timesteps[start])])
    up = F.interpolate(lat.double(), size=(32, 32), mode="bilinear", align_corners=False)
    exp = (acp ** 0.5) * up + ((1 - acp) ** 0.5) * noise.double()
    print(f"hires_start 16 -> 32: max abs error vs fp64 = {(x_start.cpu().double() - exp).abs().max().item():.3e}")
    torch.testing.assert_close(x_start.cpu().double(), exp, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match="strength"):
        hires_start(lat.cuda(), noise.cuda(), sch, 6, 0.0)
    with pytest.raises(ValueError, match="hires_start"):
        hires_start(lat.cuda(), noise[:1].cuda(), sch, 6, 0.5)


# ---------------------------------------------------------------------------------------------------------------- the second pass on the tiny UNet
@pytest.fixture(scope="module")
def tiny_pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    torch.manual_seed(0)
    ref = UNet2DConditionModelRef(**TINY_CONFIG).eval()
    set_visual_cross_attention_adapter_ref(ref, (5,))
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    return ref, hip


# fp16-storage tolerance for a short denoise loop on the tiny config (latents, rel-L2 vs fp32 oracle): tests/test_unet_gpu.py's bound
TOL_LOOP = 2.5e-3
B, S1, S2, P, GUIDANCE = 2, 16, 32, 1, 7.5
STEPS, START = 6, 3


@torch.no_grad()
def test_second_pass_matches_oracle_and_graph_equals_eager(tiny_pair):
    """``hires_start`` + ``DenoiseLoop(32 x 32).reset(x_start, 3).run()`` against the fp32 oracle UNet stepped by DPMSolverMultistepRef from
    ``add_noise(F.interpolate(base, 32), noise, t_start)``: rel-L2 of the final latents below TOL_LOOP; graph replay == eager launches == the two-stream
    graph, bit for bit.  Measured on MI355X: 1.046e-3 (1.039e-3 for the same loop from the oracle's own ``x_start``, which is within 2.4e-7 of the
    launch's; printed with -s)."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    from photoverse_amd.infer import hires_start
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    ref, hip = tiny_pair
    g = torch.Generator().manual_seed(62)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    base = torch.randn(B, 4, S1, S1, generator=g) * 0.8
    noise = torch.randn(B, 4, S2, S2, generator=g)
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(STEPS)
    sch.step_index = START
    up = F.interpolate(base, size=(S2, S2), mode="bilinear", align_corners=False)
    x_ref = sch.add_noise(up, noise, sch.timesteps[START:START + 1].repeat(B))
    exp = x_ref.clone()
    for i in range(START, STEPS):
        t = sch.timesteps[i]
        eps_u = ref(exp, t, encoder_hidden_states=uncond).sample
        eps_c = ref(exp, t, encoder_hidden_states=cond).sample
        exp = sch.step(eps_u + GUIDANCE * (eps_c - eps_u), t, exp)
    x_start, start = hires_start(base.cuda(), noise.cuda(), DPMSolverMultistepScheduler(), STEPS, 0.5)
    assert start == START
    print(f"second pass: x_start max abs difference to the oracle's = {(x_start.cpu() - x_ref).abs().max().item():.3e}")
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, S2, P, STEPS, GUIDANCE, use_graph=use_graph, two_streams=two)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(x_start, START)
        outs.append(loop.run().clone().cpu())
        assert loop.state[0].item() == STEPS
    err = rel_l2(outs[2], exp)
    # the same loop from the ORACLE's x_start (no resize involved): tells the loop at this size from the new launch
    loop.reset(x_ref.cuda(), START)
    err_loop = rel_l2(loop.run().cpu(), exp)
    print(f"second pass 16 -> 32, steps {STEPS} start {START}: rel-L2 vs fp32 oracle = {err:.3e} (from the oracle's own x_start: {err_loop:.3e})")
    assert torch.equal(outs[0], outs[1])                       # graph replay == eager launches, bit for bit
    assert torch.equal(outs[0], outs[2])                       # ... == the two-stream graph
    assert err < TOL_LOOP


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_hires_end_to_end():
    """``run_inference(latent_size=16, hires_latent_size=32)`` on the tiny models and the tiny x2 VAE: shapes, determinism, both loops cached and reused,
    the composition ``first pass -> hires_start -> cached 32-latent loop`` bit for bit, ``hires_noise`` equal to the seeded second draw, the effect of
    ``hires_strength``, ``from_noised_image`` with hires, and an untouched plain call before and after."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.infer import hires_start, run_inference
    from photoverse_amd.modeling_utils import load_models
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    from photoverse_amd.vae import AutoencoderKL
    torch.manual_seed(5)
    hip_vae = AutoencoderKL(**VAE_TINY)
    hip_vae.load_state_dict(AutoencoderKLDecoderRef(**VAE_TINY, with_encoder=True).eval().state_dict())
    hip_vae.to("cuda")
    vis = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, image_size=56, patch_size=14)
    txt = dict(vocab_size=49408, hidden_size=768, num_attention_heads=12, intermediate_size=512, num_hidden_layers=1)
    tok, te, vae, unet, ie, ia, ta, sch, _ = load_models(None, 1, unet_config=TINY_CONFIG, vision_config=vis, text_config=txt, seed=3)
    for m in (unet, te, ie, ia, ta):
        m.to("cuda")
    g = torch.Generator().manual_seed(4)
    ex = {"pixel_values": torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4, seed=1)
    hi = dict(hires_latent_size=32, hires_strength=0.5)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)          # 5. a call without the hires keywords, before ...
    # 1. latents, determinism, both loops cached and reused
    a = run_inference(*args, None, sch, "cuda", [1], **kw, **hi)
    assert a.shape == (2, 4, 32, 32) and torch.isfinite(a).all()
    cache = unet.__dict__["_denoise_loops"]
    assert len(cache) == 2 and {k[1] for k in cache} == {16, 32}
    loops = {k[1]: v for k, v in cache.items()}
    graphs = {s: l.graph for s, l in loops.items()}
    assert all(gr is not None for gr in graphs.values())
    a2 = run_inference(*args, None, sch, "cuda", [1], **kw, **hi)
    assert torch.equal(a, a2)
    assert {k[1]: v for k, v in cache.items()} == loops and all(loops[s].graph is graphs[s] for s in loops)
    # 2. composition, bit for bit: first pass -> hires_start with the seeded second draw -> the cached 32-latent loop (it still holds the conditioning)
    first = run_inference(*args, None, sch, "cuda", [1], **kw)
    assert first.shape == (2, 4, 16, 16)
    gen = torch.manual_seed(1)
    torch.randn((2, 4, 16, 16), generator=gen)
    second_noise = torch.randn((2, 4, 32, 32), generator=gen)
    x_start, start = hires_start(first, second_noise.cuda(), DPMSolverMultistepScheduler.from_config(sch.config), 4, 0.5)
    assert start == 2 and loops[32] is cache[next(k for k in cache if k[1] == 32)]
    loops[32].reset(x_start, start)
    assert torch.equal(loops[32].run(), a)
    # 3. with the VAE: 64 x 64 images in [-1, 1]; hires_noise = the seeded second draw reproduces them; another hires_strength changes them
    img = run_inference(*args, hip_vae, sch, "cuda", [1], **kw, **hi)
    assert img.shape == (2, 3, 64, 64) and torch.isfinite(img).all() and img.min() >= -1 and img.max() <= 1
    img_n = run_inference(*args, hip_vae, sch, "cuda", [1], hires_noise=second_noise, **kw, **hi)
    assert torch.equal(img, img_n)
    img_s = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=1.0, **kw)
    assert img_s.shape == img.shape and torch.isfinite(img_s).all() and not torch.equal(img_s, img)
    # 4. from_noised_image together with hires
    fn = run_inference(*args, hip_vae, sch, "cuda", [1], from_noised_image=True, **kw, **hi)
    assert fn.shape == (2, 3, 64, 64) and torch.isfinite(fn).all()
    # 5. ... and after: identical bits
    after = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)
    assert before.shape == (2, 3, 32, 32) and torch.equal(before, after)


def test_generate_cli_runs_two_passes(tmp_path):
    """generate.py --hires_latent_size runs as a program and writes its PNGs at the second pass's resolution (the tiny model's VAE is x8: 256 x 256)."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--hires_latent_size", "32", "--num_timesteps", "4", "--num_of_samples", "2", "--seed", "3", "--encoder_layers_idx", "1", "2",
           "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (256, 256, 3) and a.dtype == np.uint8 and a.std() > 0
