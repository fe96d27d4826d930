"""GPU tests of masked image editing (inpainting) and ``strength``: the masked solver-step kernel and the paste-back kernel against fp64 / torch
evaluations of their formulas, the inpainting denoise loop on the tiny UNet against the fp32 oracle (UNet + DPMSolverMultistepRef + blend), and
``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch

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


def _mixed_mask(shape, g):
    """0, 1 and fractions, each present whatever the size."""
    r, f = torch.rand(shape, generator=g), torch.rand(shape, generator=g) * 0.98 + 0.01
    m = torch.where(r < 0.3, torch.zeros(shape), torch.where(r < 0.6, torch.ones(shape), f))
    flat = m.view(-1)
    flat[0], flat[1], flat[2] = 0.0, 1.0, 0.37
    return m


# one float4 per plane; a non-power-of-two plane; four workgroups, the last one partial (960 float4 = 3.75 x 256)
@pytest.mark.parametrize("B,C,hw", [(2, 4, 4), (2, 4, 12), (3, 4, 320)])
def test_masked_step_kernel(rec_cls, B, C, hw):
    """``pv_cfg_dpm_step_masked`` against an fp64 evaluation of its formulas on the same fp32 inputs (rtol = atol = 1e-5, the bound of
    ``test_cfg_dpm_step_kernel``); bit for bit: m == 1 is ``pv_cfg_dpm_step``'s result, m == 0 is ``q0*known + q1*noise`` in fp32, ``x0_prev`` is the
    unmasked kernel's, and the three read-only inputs stay as they were.  Measured on MI355X: max abs error 1.9e-7 / 4.2e-6 / 5.5e-6 for the three shapes (printed with -s)."""
    g = torch.Generator().manual_seed(40 + hw)
    eu, ec, x, xp, known, noise = [torch.randn(B, C, hw, generator=g) for _ in range(6)]
    coef = torch.randn(3, 8, generator=g)
    mask = _mixed_mask((B, 1, hw), g)
    state = torch.tensor([1, 3, 0, 0], dtype=torch.int32)
    deu, dec, dcoef, dstate = eu.cuda(), ec.cuda(), coef.cuda(), state.cuda()
    dx, dxp, dmask, dknown, dnoise = x.cuda(), xp.cuda(), mask.cuda(), known.cuda(), noise.cuda()
    px, pxp = x.cuda(), xp.cuda()
    rec = rec_cls("cuda")
    rec.cfg_dpm_step_masked(deu, dec, dx, dxp, dcoef, dstate, 7.5, dmask, dknown, dnoise)
    rec.cfg_dpm_step(deu, dec, px, pxp, dcoef, dstate, 7.5)
    rec.run()
    torch.cuda.synchronize()
    got, got_x0, plain, plain_x0 = dx.cpu(), dxp.cpu(), px.cpu(), pxp.cpu()
    d = lambda t: t.double()
    ca, cb, cx, c0, c1, q0, q1 = d(coef)[1, :7]
    e = d(eu) + 7.5 * (d(ec) - d(eu))
    x0 = ca * d(x) + cb * e
    xn = cx * d(x) + c0 * x0 + c1 * d(xp)
    k = q0 * d(known) + q1 * d(noise)
    exp = d(mask) * xn + (1 - d(mask)) * k
    print(f"masked step ({B}, {C}, {hw}): max abs error vs fp64 = {(d(got) - exp).abs().max().item():.3e}, x0 {(d(got_x0) - x0).abs().max().item():.3e}")
    torch.testing.assert_close(d(got_x0), x0, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(d(got), exp, rtol=1e-5, atol=1e-5)
    mm = mask.expand(B, C, hw)
    assert (mm == 1).any() and (mm == 0).any() and ((mm > 0) & (mm < 1)).any()
    assert torch.equal(got[mm == 1], plain[mm == 1])
    k32 = coef[1, 5] * known + coef[1, 6] * noise
    assert torch.equal(got[mm == 0], k32[mm == 0])
    assert torch.equal(got_x0, plain_x0)
    assert torch.equal(dmask.cpu(), mask) and torch.equal(dknown.cpu(), known) and torch.equal(dnoise.cpu(), noise)
    assert dstate.cpu().tolist() == [1, 3, 0, 0]


@pytest.mark.parametrize("B,C,hw", [(2, 3, 16), (1, 3, 4 * 9)])
def test_composite_clamp_kernel(rec_cls, B, C, hw):
    """``pv_composite_clamp_f32`` against torch: exact where m is 0 or 1, rtol = atol = 1e-6 elsewhere; the same with ``out`` aliasing ``gen``."""
    g = torch.Generator().manual_seed(50 + hw)
    gen, orig = torch.randn(B, C, hw, generator=g) * 1.5, torch.randn(B, C, hw, generator=g) * 1.5       # part of both saturates the clamp
    mask = _mixed_mask((B, 1, hw), g)
    dgen, dorig, dmask = gen.cuda(), orig.cuda(), mask.cuda()
    rec = rec_cls("cuda")
    out = rec.composite_clamp(dgen, dorig, dmask, -1.0, 1.0)
    rec.run()
    torch.cuda.synchronize()
    assert torch.equal(dgen.cpu(), gen) and torch.equal(dorig.cpu(), orig) and torch.equal(dmask.cpu(), mask)
    alias = gen.cuda()
    rec2 = rec_cls("cuda")
    assert rec2.composite_clamp(alias, dorig, dmask, -1.0, 1.0, out=alias) is alias
    rec2.run()
    torch.cuda.synchronize()
    mm = mask.expand(B, C, hw)
    exp = (mm.double() * gen.double() + (1 - mm.double()) * orig.double()).clamp(-1, 1)
    assert ((gen.abs() > 1) & (mm == 1)).any() and ((orig.abs() > 1) & (mm == 0)).any()
    for got in (out.cpu(), alias.cpu()):
        assert torch.equal(got[mm == 1], gen.clamp(-1, 1)[mm == 1]) and torch.equal(got[mm == 0], orig.clamp(-1, 1)[mm == 0])
        torch.testing.assert_close(got.double(), exp, rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- the loop on the tiny UNet
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
B, S, P, GUIDANCE = 2, 16, 1, 7.5


@pytest.fixture(scope="module")
def loop_inputs():
    from oracle.infer_ref import draw_noise_ref
    g = torch.Generator().manual_seed(61)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    known = torch.randn(B, 4, S, S, generator=g) * 0.8
    noise = draw_noise_ref(B, 4, S, seed=7)
    mask = torch.zeros(B, 1, S, S)
    mask[0, 0, :, :S // 2] = 1.0                     # the left half
    mask[1, 0, 5:9, 6:10] = 1.0                      # a 4 x 4 box
    mask2 = torch.zeros(B, 1, S, S)
    mask2[0, 0, 10:, :] = 1.0
    mask2[1, 0, :3, :] = 1.0
    return dict(cond=cond, uncond=uncond, known=known, noise=noise, mask=mask, mask2=mask2)


@torch.no_grad()
def _oracle_inpaint(ref, inp, mask, steps, start):
    """fp32 oracle UNet + DPMSolverMultistepRef started at ``step_index = start``; after every ``step()`` the diffusers inpainting blend with
    ``add_noise(known, noise, timesteps[i + 1])`` (the clean ``known`` after the last step).  Returns (start latents, final latents)."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(steps)
    sch.step_index = start
    known, noise = inp["known"], inp["noise"]
    x_start = sch.add_noise(known, noise, sch.timesteps[start:start + 1].repeat(B))
    latents = x_start.clone()
    for i in range(start, steps):
        t = sch.timesteps[i]
        eps_u = ref(latents, t, encoder_hidden_states=inp["uncond"]).sample
        eps_c = ref(latents, t, encoder_hidden_states=inp["cond"]).sample
        latents = sch.step(eps_u + GUIDANCE * (eps_c - eps_u), t, latents)
        kept = sch.add_noise(known, noise, sch.timesteps[i + 1:i + 2].repeat(B)) if i < steps - 1 else known
        latents = mask * latents + (1 - mask) * kept
    return x_start, latents


def _make_loop(hip, inp, steps, **kw):
    from photoverse_amd.pipeline import DenoiseLoop
    loop = DenoiseLoop(hip, B, S, P, steps, GUIDANCE, **kw)
    loop.set_conditioning(tuple(t.cuda() for t in inp["cond"]), tuple(t.cuda() for t in inp["uncond"]))
    return loop


@pytest.mark.parametrize("steps,start", [(4, 0), (6, 3)])
def test_inpaint_loop_matches_oracle_and_graph_equals_eager(tiny_pair, loop_inputs, steps, start):
    """The repainted region (m == 1 only, so that the exact kept region does not dilute the norm) against the fp32 oracle within TOL_LOOP (measured on MI355X: 1.46e-3 for 4 steps from row 0, 1.43e-3 for 6 steps from row 3; printed with -s);
    the kept region is ``known`` bit for bit; graph replay == eager launches == the two-stream graph; a second mask needs no new capture."""
    ref, hip = tiny_pair
    inp = loop_inputs
    known, noise, mask = inp["known"], inp["noise"], inp["mask"]
    x_start, exp = _oracle_inpaint(ref, inp, mask, steps, start)
    outs, loops = [], []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = _make_loop(hip, inp, steps, use_graph=use_graph, two_streams=two, inpaint=True)
        loop.set_inpaint(mask.cuda(), known.cuda(), noise.cuda())
        loop.reset(x_start, start)
        assert loop.state[0].item() == start
        outs.append(loop.run().clone().cpu())
        assert loop.state[0].item() == steps and loop.state[1].item() == steps
        loops.append(loop)
    assert torch.equal(outs[0], outs[1])                       # graph replay == eager launches, bit for bit
    assert torch.equal(outs[0], outs[2])                       # ... == the two-stream graph
    mm = mask.expand_as(exp) == 1
    err = rel_l2(outs[2][mm], exp[mm])
    print(f"inpaint loop steps {steps} start {start}: repainted region rel-L2 vs fp32 oracle = {err:.3e}")
    assert err < TOL_LOOP
    assert torch.equal(outs[2][~mm], known[~mm])               # the kept region is the known latents themselves
    assert not torch.equal(outs[2][mm], known[mm])
    with pytest.raises(RuntimeError, match="reset"):           # the schedule is exhausted after T - start steps
        loops[2].step()
    # another mask takes effect without a new capture
    eager, graph = loops[0], loops[2]
    captured = graph.graph
    assert captured is not None
    mask2 = inp["mask2"]
    res = []
    for loop in (eager, graph):
        loop.set_inpaint(mask2.cuda(), known.cuda(), noise.cuda())
        loop.reset(x_start, start)
        res.append(loop.run().clone().cpu())
    assert graph.graph is captured
    mm2 = mask2.expand_as(exp) == 1
    assert torch.equal(res[0], res[1]) and torch.equal(res[1][~mm2], known[~mm2])
    assert not torch.equal(res[1][mm2 & ~mm], known[mm2 & ~mm])


def test_inpaint_loop_with_trivial_masks_is_the_plain_loop_or_the_known_latents(tiny_pair, loop_inputs):
    _, hip = tiny_pair
    inp = loop_inputs
    steps = 4
    known, noise = inp["known"], inp["noise"]
    plain = _make_loop(hip, inp, steps)
    masked = _make_loop(hip, inp, steps, inpaint=True)
    assert masked.launches_per_step == plain.launches_per_step
    assert plain.coef[:, 5:].abs().max().item() == 0 and not hasattr(plain, "mask")
    with pytest.raises(RuntimeError, match="inpaint"):
        plain.set_inpaint(inp["mask"].cuda(), known.cuda(), noise.cuda())
    plain.reset(noise)
    exp = plain.run().clone().cpu()
    masked.set_inpaint(torch.ones(1, 1, S, S).cuda(), known.cuda(), noise.cuda())          # (1, 1, S, S) broadcasts over the batch
    masked.reset(noise)
    assert torch.equal(masked.run().cpu(), exp)                # all ones, start 0: the plain loop, bit for bit
    masked.set_inpaint(torch.zeros(B, 1, S, S).cuda(), known.cuda(), noise.cuda())
    masked.reset(noise)
    assert torch.equal(masked.run().cpu(), known)              # all zeros: the known latents
    # a plain loop started part-way: T - start steps, the start row first order (no history), and back to the whole schedule afterwards
    plain.reset(noise, 2)
    assert plain.state[0].item() == 2 and plain.coef[2, 4].item() == 0 and plain.coef[1, 4].item() == 0
    part = plain.run().clone().cpu()
    assert plain.state[0].item() == steps and torch.isfinite(part).all() and not torch.equal(part, exp)
    plain.reset(noise)
    assert plain.coef[2, 4].item() != 0 and torch.equal(plain.run().cpu(), exp)
    with pytest.raises(ValueError, match="start"):
        plain.reset(noise, steps)


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


class _RecordingVAE:
    """The HIP VAE with ``decode`` recording what it is handed: ``latents / scaling_factor`` of the call, i.e. the call with its decode skipped."""

    def __init__(self, vae):
        self.vae, self.config, self.encode, self.seen = vae, vae.config, vae.encode, None

    def decode(self, z):
        self.seen = z.clone()
        return self.vae.decode(z)


def test_run_inference_inpaint_and_strength():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.infer import run_inference
    from photoverse_amd.modeling_utils import load_models
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
    mask = torch.zeros(2, 1, 32, 32)                 # the tiny VAE has factor 2: latent 16
    mask[0, 0, 4:15, 9:20] = 1.0                     # odd edges: the latent mask is wider than the pixel mask
    mask[1, 0, :, 16:] = 0.8                         # binarised at 0.5
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4, seed=1)
    args = (ex, tok, ie, te, unet, ta, ia)
    with torch.no_grad():
        a = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw)
        a2 = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw)
        half = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, strength=0.5, **kw)
        recv = _RecordingVAE(hip_vae)
        raw = run_inference(*args, recv, sch, "cuda", [1], inpaint_mask=mask, paste_back=False, **kw)
        exp_raw = hip_vae.decode(recv.seen).sample.clamp(-1, 1)
        lat = run_inference(*args, None, sch, "cuda", [1], **kw)
        n0 = run_inference(*args, hip_vae, sch, "cuda", [1], from_noised_image=True, **kw)
        n1 = run_inference(*args, hip_vae, sch, "cuda", [1], from_noised_image=True, strength=1.0, **kw)
        n5 = run_inference(*args, hip_vae, sch, "cuda", [1], from_noised_image=True, strength=0.5, **kw)
        with pytest.raises(NotImplementedError, match="inpaint_mask needs a vae"):
            run_inference(*args, None, sch, "cuda", [1], inpaint_mask=mask, **kw)
    pm = (mask >= 0.5).expand(2, 3, 32, 32)
    pix = ex["pixel_values"]
    for out in (a, half):
        out = out.cpu()
        assert out.shape == (2, 3, 32, 32) and torch.isfinite(out).all() and out.min() >= -1 and out.max() <= 1
        assert torch.equal(out[~pm], pix[~pm])                 # outside the pixel mask: the photograph, bit for bit
        assert not torch.equal(out[pm], pix[pm])
    assert torch.equal(a, a2)                                  # same seed -> same posterior sample, noise and images
    assert not torch.equal(a, half)
    assert torch.equal(raw, exp_raw) and torch.equal(raw.cpu()[pm], a.cpu()[pm]) and not torch.equal(raw.cpu()[~pm], pix[~pm])
    assert lat.shape == (2, 4, 16, 16)                         # the plain call still returns latents without a VAE
    assert torch.equal(n0, n1)                                 # strength 1.0 is from_noised_image as it was
    assert torch.isfinite(n5).all() and not torch.equal(n5, n0)
    # plain and inpainting loops are cached side by side; neither call re-captured the other's
    keys = list(unet.__dict__["_denoise_loops"])
    assert len(keys) == 2 and {k[-1] for k in keys} == {True, False}


def test_generate_cli_inpaints_from_a_mask_file(tmp_path):
    """generate.py --mask_image_path runs as a program and writes its PNGs; with --synthetic_input the photograph is mid-grey, so paste-back shows in the
    file itself: grey outside the mask, generated pixels inside."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    marr = np.zeros((64, 64), dtype=np.uint8)
    marr[:, 32:] = 255                               # the right half, at half the working resolution: resized with nearest neighbour
    Image.fromarray(marr).save(tmp_path / "mask.png")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--num_timesteps", "4", "--latent_size", "16",
           "--num_of_samples", "2", "--seed", "3", "--guidance_scale", "2.0", "--encoder_layers_idx", "1", "2", "--mask_image_path", str(tmp_path / "mask.png"),
           "--strength", "0.75", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8
        assert (a[:, :64] == 128).all() and a[:, 64:].std() > 0
