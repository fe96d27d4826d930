"""GPU tests of the separate identity / prompt guidance scales and ``guidance_rescale``: ``pv_cfg_dpm_step_guided`` against the fp64 evaluation of the
header's formulas (``test_guidance_cpu.guided_step_ref``) and, bit for bit, against the two launchers it generalises; the three-forward ``DenoiseLoop`` on
the tiny UNet against the fp32 oracle (UNet x3 + DPMSolverMultistepRef); ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch

from test_guidance_cpu import SHAPES, guided_step_ref, make_eps

pytestmark = pytest.mark.gpu

#: rtol = atol of the forms without rescale: the project's bound for the step kernels (test_cfg_dpm_step_kernel, test_masked_step_kernel)
TOL_STEP = 1e-5
#: rtol = atol of the forms with rescale: four times the largest max |got - fp64| / (1 + |fp64|) measured on MI355X over SHAPES x rows x forms
#: (2.306e-6, see test_guided_step_kernel's docstring); the margin covers another reduction order under another compiler.  The factor f adds the error
#: of two length-chw fp32 reductions, multiplied by |cb| (15.6 on row 0) - but it also shrinks e, so the bound ends up below TOL_STEP
TOL_RESCALE = 9.2e-6
G_TEXT, G_IMAGE, RESCALE = 7.5, 3.0, 0.7
ROWS = (0, 3, 5)                 # first-order first row, a second-order middle row, the last row ((q0, q1) = (1, 0))


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


@pytest.fixture(scope="module")
def coef6():
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(6)
    return sch.coefficient_table(0, blend=True)


def mixed_mask(shape, g):
    """Zeros, ones and fractional values, every kind present."""
    r = torch.rand(shape, generator=g)
    m = torch.where(r < 0.3, torch.zeros(()), torch.where(r > 0.7, torch.ones(()), r))
    m.view(-1)[:3] = torch.tensor([0.0, 1.0, 0.5])
    return m.contiguous()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_guided_step_kernel(rec_cls, coef6, shape):
    """``pv_cfg_dpm_step_guided`` on rows 0, 3 and 5 of the real 6-step coefficient table, in the forms two-forward + rescale, three-forward,
    three-forward + rescale, each with and without a mask, against ``guided_step_ref`` (fp64 on the same fp32 inputs): rtol = atol = 1e-5 without
    rescale, TOL_RESCALE with.  Bit for bit: ``eps_image`` None + rescale 0 is ``pv_cfg_dpm_step`` (no mask) and ``pv_cfg_dpm_step_masked`` (mask);
    three-forward at ``g_image == g_text`` is ``pv_cfg_dpm_step`` too; ``x0_prev`` of a masked form is the unmasked form's ``x0``; mask 0 is ``q0*known + q1*noise`` in fp32; every read-only input is unchanged.
    The per-sample factors differ between the samples (means of +-3, standard deviations in [0.1, 2]: ``make_eps``).
    Measured on MI355X (printed with -s), largest max |got - fp64| / (1 + |fp64|) over the rows and forms of each shape, without / with rescale:
    2.4e-7 / 3.6e-7, 3.5e-7 / 9.8e-7, 4.3e-7 / 8.1e-7, 4.7e-6 / 2.1e-6, 3.1e-6 / 2.3e-6 (max |got - fp64|: 3.1e-5 ... 6.9e-5 / 1.5e-5 ... 3.4e-5, on values
    of several hundred: guidance 7.5 on means of +-3 times |cb| = 15.6).  TOL_RESCALE = 4 x 2.306e-6."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 7)
    eu, em, ec = make_eps(shape, g)
    x, xp, known, noise = (torch.randn(shape, generator=g).contiguous() for _ in range(4))
    mask = mixed_mask((B, 1, H, W), g)
    mm = mask.expand(B, C, H, W)
    d_eu, d_em, d_ec, d_coef, d_mask, d_known, d_noise = (t.cuda() for t in (eu, em, ec, coef6, mask, known, noise))
    forms = [(None, RESCALE), (em, 0.0), (em, RESCALE)]
    worst = {False: 0.0, True: 0.0}
    worst_abs = {False: 0.0, True: 0.0}
    for row in ROWS:
        state = torch.tensor([row, 6, 0, 0], dtype=torch.int32)
        d_state = state.cuda()
        rec = rec_cls("cuda")
        runs = []
        for img, rs in forms:
            for masked in (False, True):
                dx, dxp = x.cuda(), xp.cuda()
                blend = dict(mask=d_mask, known=d_known, noise=d_noise) if masked else {}
                rec.cfg_dpm_step_guided(d_eu, None if img is None else d_em, d_ec, dx, dxp, d_coef, d_state, G_TEXT, G_IMAGE, rs, **blend)
                runs.append((img, rs, masked, dx, dxp))
        # the two contracts: the launchers this one generalises, on their own copies
        c_new, c_new_p, c_old, c_old_p, m_new, m_new_p, m_old, m_old_p = (t.cuda() for t in (x, xp) * 4)
        rec.cfg_dpm_step_guided(d_eu, None, d_ec, c_new, c_new_p, d_coef, d_state, G_TEXT)
        rec.cfg_dpm_step(d_eu, d_ec, c_old, c_old_p, d_coef, d_state, G_TEXT)
        rec.cfg_dpm_step_guided(d_eu, None, d_ec, m_new, m_new_p, d_coef, d_state, G_TEXT, mask=d_mask, known=d_known, noise=d_noise)
        rec.cfg_dpm_step_masked(d_eu, d_ec, m_old, m_old_p, d_coef, d_state, G_TEXT, d_mask, d_known, d_noise)
        e_new, e_new_p = x.cuda(), xp.cuda()                                   # equal scales: the eps_image terms cancel
        rec.cfg_dpm_step_guided(d_eu, d_em, d_ec, e_new, e_new_p, d_coef, d_state, G_TEXT, G_TEXT)
        rec.run()
        torch.cuda.synchronize()
        assert torch.equal(c_new, c_old) and torch.equal(c_new_p, c_old_p), f"row {row}: not the bits of pv_cfg_dpm_step"
        assert torch.equal(m_new, m_old) and torch.equal(m_new_p, m_old_p), f"row {row}: not the bits of pv_cfg_dpm_step_masked"
        assert torch.equal(e_new, c_old) and torch.equal(e_new_p, c_old_p), f"row {row}: equal scales are not the bits of pv_cfg_dpm_step"
        k32 = coef6[row, 5] * known + coef6[row, 6] * noise
        x0_unmasked = {}
        for img, rs, masked, dx, dxp in runs:
            got, got_x0 = dx.cpu(), dxp.cpu()
            blend = dict(mask=mask, known=known, noise=noise) if masked else {}
            exp, x0, f = guided_step_ref(eu, img, ec, x, xp, coef6[row], G_TEXT, G_IMAGE, rs, **blend)
            if rs > 0 and B > 1:
                assert f.unique().numel() == B and (f.max() / f.min()) > 1.05            # a factor of another sample would show
            tol = TOL_RESCALE if rs > 0 else TOL_STEP
            err = max(((got.double() - exp).abs() / (1 + exp.abs())).max().item(), ((got_x0.double() - x0).abs() / (1 + x0.abs())).max().item())
            err_abs = max((got.double() - exp).abs().max().item(), (got_x0.double() - x0).abs().max().item())
            worst[rs > 0], worst_abs[rs > 0] = max(worst[rs > 0], err), max(worst_abs[rs > 0], err_abs)
            print(f"guided step {shape} row {row} {'three' if img is not None else 'two'}-forward rescale {rs} mask {int(masked)}: "
                  f"max |d| / (1 + |fp64|) = {err:.3e}, max |d| = {err_abs:.3e}, f = {[round(v, 4) for v in f.tolist()]}")
            torch.testing.assert_close(got_x0.double(), x0, rtol=tol, atol=tol)
            torch.testing.assert_close(got.double(), exp, rtol=tol, atol=tol)
            if masked:
                assert torch.equal(got_x0, x0_unmasked[(img is None, rs)])                # x0_prev holds the unblended x0
                assert torch.equal(got[mm == 0], k32[mm == 0])                            # the kept region, exactly
            else:
                x0_unmasked[(img is None, rs)] = got_x0
        assert d_state.cpu().tolist() == [row, 6, 0, 0]
    print(f"guided step {shape}: worst max |d| / (1 + |fp64|) without rescale {worst[False]:.3e} (abs {worst_abs[False]:.3e}), "
          f"with rescale {worst[True]:.3e} (abs {worst_abs[True]:.3e})")
    assert (mm == 1).any() and (mm == 0).any() and ((mm > 0) & (mm < 1)).any()
    for dev, host in ((d_eu, eu), (d_em, em), (d_ec, ec), (d_coef, coef6), (d_mask, mask), (d_known, known), (d_noise, noise)):
        assert torch.equal(dev.cpu(), host)


def test_guided_step_of_an_all_zero_sample_is_finite(rec_cls, coef6):
    """Sample 0 has all-zero ``eps_*``: ``std(e) == 0``, so ``f = 1`` there - no 0 / 0 - while sample 1 is rescaled as usual."""
    shape = (2, 4, 16, 16)
    g = torch.Generator().manual_seed(3)
    eu, em, ec = make_eps(shape, g)
    for t in (eu, em, ec):
        t[0].zero_()
    x, xp = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    state = torch.tensor([3, 6, 0, 0], dtype=torch.int32).cuda()
    for img in (None, em):
        dx, dxp = x.cuda(), xp.cuda()
        rec = rec_cls("cuda")
        rec.cfg_dpm_step_guided(eu.cuda(), None if img is None else em.cuda(), ec.cuda(), dx, dxp, coef6.cuda(), state, G_TEXT, G_IMAGE, RESCALE)
        rec.run()
        torch.cuda.synchronize()
        exp, x0, f = guided_step_ref(eu, img, ec, x, xp, coef6[3], G_TEXT, G_IMAGE, RESCALE)
        assert f[0] == 1 and f[1] != 1
        assert torch.isfinite(dx).all() and torch.isfinite(dxp).all()
        err = max(((dx.cpu().double() - exp).abs() / (1 + exp.abs())).max().item(), ((dxp.cpu().double() - x0).abs() / (1 + x0.abs())).max().item())
        print(f"all-zero sample, {'three' if img is not None else 'two'}-forward: max |d| / (1 + |fp64|) = {err:.3e}")
        torch.testing.assert_close(dx.cpu().double(), exp, rtol=TOL_RESCALE, atol=TOL_RESCALE)
        torch.testing.assert_close(dxp.cpu().double(), x0, rtol=TOL_RESCALE, atol=TOL_RESCALE)


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
B, S, P, STEPS = 2, 16, 1, 4


@pytest.fixture(scope="module")
def loop_inputs():
    g = torch.Generator().manual_seed(81)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)
    return cond, uncond, noise


def _run(loop, cond, uncond, noise):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    loop.reset(noise)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == STEPS
    return out


@torch.no_grad()
def test_three_forward_loop_matches_oracle_and_graph_equals_eager(tiny_pair, loop_inputs):
    """guidance 7.5, image_guidance_scale 3.0, guidance_rescale 0.7, 4 steps at B = 2, 16 x 16: the final latents against the fp32 oracle UNet run three
    times per step (uncond; uncond text + cond image tokens; cond), the header's formulas in torch and DPMSolverMultistepRef - rel-L2 below TOL_LOOP (the
    weights -2, -4.5, 7.5 sum in magnitude to the 14 of plain 7.5).  Eager launches == graph replay == the graph with two side streams, bit for bit.
    Measured on MI355X: rel-L2 9.613e-4 (printed with -s)."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(STEPS)
    exp = noise * sch.init_noise_sigma
    for t in sch.timesteps:
        eu = ref(exp, t, encoder_hidden_states=uncond).sample
        em = ref(exp, t, encoder_hidden_states=(uncond[0], cond[1])).sample
        ec = ref(exp, t, encoder_hidden_states=cond).sample
        e = eu + G_IMAGE * (em - eu) + G_TEXT * (ec - em)
        f = RESCALE * ec.flatten(1).std(dim=1) / e.flatten(1).std(dim=1) + (1 - RESCALE)
        exp = sch.step(f.view(B, 1, 1, 1) * e, t, exp)
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, use_graph=use_graph, two_streams=two, image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE)
        assert len(loop.engines_i) == 1 and not loop.merge_lowres and len(loop._sides) == (2 if two else 0)
        outs.append(_run(loop, cond, uncond, noise))
    err = rel_l2(outs[2], exp)
    print(f"three-forward loop, g_text {G_TEXT} g_image {G_IMAGE} rescale {RESCALE}, {STEPS} steps: rel-L2 vs fp32 oracle = {err:.3e}")
    assert torch.equal(outs[0], outs[1])                       # graph replay == eager launches, bit for bit
    assert torch.equal(outs[0], outs[2])                       # ... == the graph with two side streams
    assert err < TOL_LOOP


@torch.no_grad()
def test_rescale_only_loop_keeps_two_forwards_and_matches_oracle(tiny_pair, loop_inputs):
    """``guidance_rescale`` alone: the engines and the launch count of the default loop, only the tail's launcher differs; against the fp32 oracle with
    the rescaled two-term formula, below TOL_LOOP.  Measured on MI355X: rel-L2 7.516e-4 (printed with -s)."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(STEPS)
    exp = noise * sch.init_noise_sigma
    for t in sch.timesteps:
        eu = ref(exp, t, encoder_hidden_states=uncond).sample
        ec = ref(exp, t, encoder_hidden_states=cond).sample
        e = eu + G_TEXT * (ec - eu)
        f = RESCALE * ec.flatten(1).std(dim=1) / e.flatten(1).std(dim=1) + (1 - RESCALE)
        exp = sch.step(f.view(B, 1, 1, 1) * e, t, exp)
    plain = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, guidance_rescale=RESCALE)
    assert loop.launches_per_step == plain.launches_per_step and loop.merge_lowres == plain.merge_lowres and not loop.engines_i and loop.eps_m is None
    assert [fn.__name__ for fn, _ in loop.tail.calls] == ["pv_cfg_dpm_step_guided", "pv_step_advance"]
    out = _run(loop, cond, uncond, noise)
    err = rel_l2(out, exp)
    print(f"rescale-only loop, guidance {G_TEXT} rescale {RESCALE}, {STEPS} steps: rel-L2 vs fp32 oracle = {err:.3e}")
    assert err < TOL_LOOP
    assert not torch.equal(out, _run(plain, cond, uncond, noise))


@torch.no_grad()
def test_equal_scales_three_forward_loop_is_the_two_forward_loop_within_1e_4(tiny_pair, loop_inputs):
    """``image_guidance_scale == guidance_scale``, rescale 0: the three-forward loop within 1e-4 (rel-L2) of the two-forward loop on the same inputs.
    At equal scales the ``eps_m`` terms cancel and the launcher evaluates the two-term expression, so the two loops agree bit for bit (measured on
    MI355X: 0).  Evaluated as ``eu + g (em - eu) + g (ec - em)`` - one fp32 ulp of ``eps`` away - the loops were 3.7e-8 apart after one step and
    1.364e-4 after four: the fp16 UNet amplifies last-bit differences of the latents (EXPERIMENTS.md "Guidance scales and rescale")."""
    from photoverse_amd.pipeline import DenoiseLoop
    _, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    two = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    three = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, image_guidance_scale=G_TEXT)
    assert three.launches_per_step > two.launches_per_step and len(three.engines_i) == 1
    err = rel_l2(_run(three, cond, uncond, noise), _run(two, cond, uncond, noise))
    print(f"three-forward loop at equal scales against the two-forward loop: rel-L2 = {err:.3e}")
    assert err < 1e-4


@torch.no_grad()
def test_defaults_are_untouched_and_prefix_sharing_and_inpaint_keep_the_bits(tiny_pair, loop_inputs):
    """A default loop built after guided ones has the launches and the bits of one built before.  With ``share_prefix`` and with ``inpaint`` under
    a mask of ones the three-forward loop keeps its bits.  ``training_mode`` and a rescale outside [0, 1] are refused."""
    from photoverse_amd.pipeline import DenoiseLoop
    _, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert [fn.__name__ for fn, _ in before.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"] and not before.engines_i
    out_before = _run(before, cond, uncond, noise)
    kw = dict(image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE)
    base = _run(DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw), cond, uncond, noise)
    shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_prefix=True, **kw)
    assert shared.share_prefix and len(shared.engines_p) == 1
    assert torch.equal(_run(shared, cond, uncond, noise), base)
    inp = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, inpaint=True, **kw)               # the mask starts as ones, known / noise as zeros
    assert [fn.__name__ for fn, _ in inp.tail.calls] == ["pv_cfg_dpm_step_guided", "pv_step_advance"]
    assert torch.equal(_run(inp, cond, uncond, noise), base)
    with pytest.raises(ValueError, match="training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, image_guidance_scale=G_IMAGE)
    with pytest.raises(ValueError, match="guidance_rescale"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, guidance_rescale=1.5)
    after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert after.launches_per_step == before.launches_per_step and after.merge_lowres == before.merge_lowres
    assert [fn.__name__ for fn, _ in after.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"]
    assert torch.equal(_run(after, cond, uncond, noise), out_before)


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_guidance_end_to_end():
    """``run_inference(image_guidance_scale=..., guidance_rescale=...)`` on the tiny models and the tiny x2 VAE: shapes, finiteness, determinism, the
    cached loop and its graph reused, each keyword changes the result, equal scales run the two-forward loop, both keywords with ``inpaint_mask``
    (the kept region equals the input bits under ``paste_back``) and with ``hires_latent_size``, and an untouched plain call before and after."""
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
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4, seed=1)
    gd = dict(image_guidance_scale=1.5, guidance_rescale=0.7)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)          # a plain call, before ...
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(iter(cache.values()))
    # 1. latents: shape, finiteness, determinism, the cached loop and its graph reused
    a = run_inference(*args, None, sch, "cuda", [1], **kw, **gd)
    assert a.shape == (2, 4, 16, 16) and torch.isfinite(a).all()
    loop = next(reversed(cache.values()))
    assert loop is not plain_loop and len(loop.engines_i) == 1 and loop.guidance_rescale == 0.7 and loop.image_guidance == 1.5
    graph = loop.graph
    assert graph is not None
    a2 = run_inference(*args, None, sch, "cuda", [1], **kw, **gd)
    assert torch.equal(a, a2) and next(reversed(cache.values())) is loop and loop.graph is graph
    # 2. each keyword changes the result; equal scales are the ordinary formula on a two-forward loop
    plain = run_inference(*args, None, sch, "cuda", [1], **kw)
    only_img = run_inference(*args, None, sch, "cuda", [1], image_guidance_scale=1.5, **kw)
    only_rs = run_inference(*args, None, sch, "cuda", [1], guidance_rescale=0.7, **kw)
    assert torch.isfinite(only_img).all() and torch.isfinite(only_rs).all()
    assert not torch.equal(only_img, plain) and not torch.equal(only_rs, plain) and not torch.equal(only_img, a) and not torch.equal(only_rs, a)
    same = run_inference(*args, None, sch, "cuda", [1], image_guidance_scale=3.0, **kw)
    assert torch.equal(same, plain) and not next(reversed(cache.values())).engines_i
    # 3. with inpaint_mask: images in [-1, 1], the kept region is the photograph's own bits
    mask = torch.zeros(1, 1, 32, 32)
    mask[..., 8:24, 4:20] = 1
    img = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw, **gd)
    assert img.shape == (2, 3, 32, 32) and torch.isfinite(img).all() and img.min() >= -1 and img.max() <= 1
    keep = (mask == 0).expand(2, 3, 32, 32)
    assert torch.equal(img.cpu()[keep], ex["pixel_values"].clamp(-1, 1)[keep])
    img_plain = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw)
    assert not torch.equal(img, img_plain)
    # 4. with hires_latent_size: both passes use the settings
    hi = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw, **gd)
    assert hi.shape == (2, 3, 64, 64) and torch.isfinite(hi).all()
    assert {k[1] for k in cache} == {16, 32} and all(len(l.engines_i) == 1 and l.guidance_rescale == 0.7 for l in cache.values())
    hi_plain = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw)
    assert not torch.equal(hi, hi_plain)
    # 5. ... and after: identical bits
    after = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)
    assert before.shape == (2, 3, 32, 32) and torch.equal(before, after)


def test_generate_cli_runs_with_the_guidance_flags(tmp_path):
    """generate.py --image_guidance_scale 2 --guidance_rescale 0.5 runs as a program and writes its PNGs."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--image_guidance_scale", "2", "--guidance_rescale", "0.5", "--num_timesteps", "4", "--num_of_samples", "2",
           "--seed", "3", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
