"""GPU tests of the stochastic sampler: the noise ``pv_cfg_dpm_step_stochastic`` generates against the numpy Philox + fp64 Box-Muller of
``test_sampler_cpu``, the whole launcher against ``stochastic_step_ref`` (fp64), the counter layout bit for bit, the rejected arguments; the stochastic
``DenoiseLoop`` on the tiny UNet against the fp32 oracle UNet stepped by the fp64 SDE restatement under the same noise; graph behaviour; the default
loop untouched; ``run_inference`` / the CLI end to end on the tiny models."""
import os

import numpy as np
import pytest
import torch

from test_sampler_cpu import SDE, SHAPES, make_eps, noise_ref, sde_rows_ref, stochastic_step_ref

pytestmark = pytest.mark.gpu

#: rtol = atol of the full step without rescale: the step kernels' bound (test_guidance_gpu.TOL_STEP); with rescale: test_guidance_gpu.TOL_RESCALE
TOL_STEP = 1e-5
TOL_RESCALE = 9.2e-6
#: max |got / cn - z_fp64| of the generated normals: four times the largest value measured on MI355X over SHAPES x rows 0, 3 (5.477e-7, see
#: test_noise_itself's docstring); the margin covers another libm (logf / sincospif within their documented ulps) under another compiler
TOL_NOISE = 4 * 5.477e-7
G_TEXT, G_IMAGE, RESCALE = 7.5, 3.0, 0.7
ROWS = (0, 3, 5)                 # first order, second order, the noise-free last row
SEED, OFFSET, STREAM = 0x1234_5678_9abc_def1, 3, 1


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
    sch = DPMSolverMultistepScheduler(algorithm_type=SDE)
    sch.set_timesteps(6)
    return sch.coefficient_table(0, blend=True)


def rng_words(seed, sample_offset=0, stream=0):
    seed %= 1 << 64
    return torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32, sample_offset, stream], dtype=np.uint32).view(np.int32).copy())


def state_words(step, rows=6):
    return torch.tensor([step, rows, 0, 0], dtype=torch.int32)


def mixed_mask(shape, g):
    """Zeros, ones and fractional values, every kind present."""
    r = torch.rand(shape, generator=g)
    m = torch.where(r < 0.3, torch.zeros(()), torch.where(r > 0.7, torch.ones(()), r))
    m.view(-1)[:3] = torch.tensor([0.0, 1.0, 0.5])
    return m.contiguous()


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_itself(rec_cls, coef6, shape):
    """``eps_* = latents = x0_prev = 0``: the launch writes ``cn * z``.  Divided by ``cn`` it is compared with the fp64 Box-Muller of the numpy Philox
    at the same key and counter: max |got - ref| below TOL_NOISE, four times the largest value measured on MI355X.  (The same definition evaluated
    in fp32 by numpy is 1.8e-6 from fp64 at most over 4 * 2^20 draws; a value above 1e-5 means a rounded 2 pi or a fast logarithm.)  On the last
    row (cn = 0) the result is zero.  On (2, 4, 64, 64) the mean and the standard deviation are those of the reference within 1e-4.
    Measured on MI355X (printed with -s), max |got / cn - z_fp64| per shape: 5.163e-7, 5.163e-7, 5.163e-7, 5.477e-7, 5.163e-7 (the first three and
    the last meet their worst draw in the first 16 blocks of sample 0; it includes the rounding of ``cn * z``, up to 3e-7 at |z| = 5);
    TOL_NOISE = 4 x 5.477e-7 = 2.19e-6.  Moments on (2, 4, 64, 64), rows 0 / 3: reference mean -2.894e-3 / 1.852e-3, std 0.999505 / 1.006048, the
    device's equal to all printed digits."""
    z = torch.zeros(shape)
    d_z, d_coef, d_rng = z.cuda(), coef6.cuda(), rng_words(SEED, OFFSET, STREAM).cuda()
    worst = 0.0
    for row in ROWS:
        lat, x0p = z.cuda(), z.cuda()
        rec = rec_cls("cuda")
        rec.cfg_dpm_step_stochastic(d_z, None, d_z, lat, x0p, d_coef, state_words(row).cuda(), d_rng, G_TEXT)
        rec.run()
        torch.cuda.synchronize()
        assert (x0p == 0).all()
        cn = coef6[row, 7].double().item()
        if row == 5:
            assert cn == 0 and (lat == 0).all()
            continue
        ref = noise_ref(shape, SEED, OFFSET, STREAM, row)
        got = lat.cpu().double() / cn
        err = (got - ref).abs().max().item()
        worst = max(worst, err)
        print(f"noise {shape} row {row}: max |got / cn - z_fp64| = {err:.3e}, max |z| = {ref.abs().max().item():.3f}")
        assert err < 1e-5, "the noise definition was not followed (a rounded 2 pi? a fast logarithm?)"
        assert err < TOL_NOISE
        if shape == (2, 4, 64, 64):
            mean, std = ref.mean().item(), ref.std(unbiased=False).item()
            print(f"noise {shape} row {row}: reference mean {mean:.3e}, std {std:.6f}; device mean {got.mean().item():.3e}, std {got.std(unbiased=False).item():.6f}")
            assert abs(mean) < 0.02 and abs(std - 1) < 0.02                                     # not degenerate
            assert abs(got.mean().item() - mean) < 1e-4 and abs(got.std(unbiased=False).item() - std) < 1e-4
    print(f"noise {shape}: worst max |got / cn - z_fp64| = {worst:.3e}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stochastic_step_kernel(rec_cls, coef6, shape):
    """``pv_cfg_dpm_step_stochastic`` on rows 0, 3 and 5 of the real 6-step SDE table, three- and two-forward, with and without rescale, with and
    without a mixed mask, against ``stochastic_step_ref`` (fp64 on the same fp32 inputs, the noise from the numpy Philox): rtol = atol = 1e-5 without
    rescale and 9.2e-6 with - the bounds of the guided launcher's test, which this one keeps although it adds one rounded product.  ``x0_prev`` is the
    unblended ``x0``; mask 0 is ``q0*known + q1*noise`` in fp32 exactly (the noise goes in before the blend); read-only inputs are unchanged.
    Measured on MI355X (printed with -s), largest max |got - fp64| / (1 + |fp64|) over the rows and forms of each shape, without / with rescale:
    2.3e-7 / 2.1e-7, 2.8e-7 / 7.8e-7, 1.7e-6 / 9.1e-7, 4.2e-6 / 1.7e-6, 2.3e-6 / 2.8e-6 - inside both bounds, so neither was re-derived."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 11)
    eu, em, ec = make_eps(shape, g)
    x, xp, known, noise = (torch.randn(shape, generator=g).contiguous() for _ in range(4))
    mask = mixed_mask((B, 1, H, W), g)
    mm = mask.expand(B, C, H, W)
    rng = rng_words(SEED, OFFSET, STREAM)
    d_eu, d_em, d_ec, d_coef, d_mask, d_known, d_noise, d_rng = (t.cuda() for t in (eu, em, ec, coef6, mask, known, noise, rng))
    worst = {False: 0.0, True: 0.0}
    for row in ROWS:
        d_state = state_words(row).cuda()
        rec = rec_cls("cuda")
        runs = []
        for img in (em, None):
            for rs in (0.0, RESCALE):
                for masked in (False, True):
                    dx, dxp = x.cuda(), xp.cuda()
                    blend = dict(mask=d_mask, known=d_known, noise=d_noise) if masked else {}
                    rec.cfg_dpm_step_stochastic(d_eu, None if img is None else d_em, d_ec, dx, dxp, d_coef, d_state, d_rng, G_TEXT, G_IMAGE, rs, **blend)
                    runs.append((img, rs, masked, dx, dxp))
        rec.run()
        torch.cuda.synchronize()
        z = noise_ref(shape, SEED, OFFSET, STREAM, row)
        k32 = coef6[row, 5] * known + coef6[row, 6] * noise
        x0_unmasked = {}
        for img, rs, masked, dx, dxp in runs:
            got, got_x0 = dx.cpu(), dxp.cpu()
            blend = dict(mask=mask, known=known, noise=noise) if masked else {}
            exp, x0 = stochastic_step_ref(eu, img, ec, x, xp, coef6[row], z, G_TEXT, G_IMAGE, rs, **blend)
            tol = TOL_RESCALE if rs > 0 else TOL_STEP
            err = max(((got.double() - exp).abs() / (1 + exp.abs())).max().item(), ((got_x0.double() - x0).abs() / (1 + x0.abs())).max().item())
            worst[rs > 0] = max(worst[rs > 0], err)
            print(f"stochastic step {shape} row {row} {'three' if img is not None else 'two'}-forward rescale {rs} mask {int(masked)}: "
                  f"max |d| / (1 + |fp64|) = {err:.3e}")
            torch.testing.assert_close(got_x0.double(), x0, rtol=tol, atol=tol)
            torch.testing.assert_close(got.double(), exp, rtol=tol, atol=tol)
            if masked:
                assert torch.equal(got_x0, x0_unmasked[(img is None, rs)])                # x0_prev holds the unblended x0
                assert torch.equal(got[mm == 0], k32[mm == 0])                            # the kept region, exactly: no fresh noise there
            else:
                x0_unmasked[(img is None, rs)] = got_x0
        assert d_state.cpu().tolist() == [row, 6, 0, 0]
    print(f"stochastic step {shape}: worst max |d| / (1 + |fp64|) without rescale {worst[False]:.3e}, with rescale {worst[True]:.3e}")
    for dev, host in ((d_eu, eu), (d_em, em), (d_ec, ec), (d_coef, coef6), (d_mask, mask), (d_known, known), (d_noise, noise), (d_rng, rng)):
        assert torch.equal(dev.cpu(), host)


def test_counter_layout_bit_for_bit(rec_cls, coef6):
    """The same (seed, sample_offset, stream, step) twice gives the same bits; changing any one of them (either seed word) changes every sample's
    output; sample 1 of a B = 2 launch at offset 0 is the B = 1 launch at offset 1 on that sample's inputs; on the last row the seed does not matter.
    Rescale is on throughout (one workgroup per sample: the factor must not depend on the batch either).  The step only selects the noise here: the
    table is six copies of row 3."""
    shape = (2, 4, 16, 16)
    g = torch.Generator().manual_seed(21)
    eu, em, ec = make_eps(shape, g)
    x, xp = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    same_rows = coef6[3:4].repeat(6, 1).contiguous().cuda()
    real_rows = coef6.cuda()

    def launch(seed=SEED, off=0, stream=0, step=3, coef=same_rows, sl=slice(None)):
        dx, dxp = x[sl].contiguous().cuda(), xp[sl].contiguous().cuda()
        rec = rec_cls("cuda")
        rec.cfg_dpm_step_stochastic(eu[sl].contiguous().cuda(), em[sl].contiguous().cuda(), ec[sl].contiguous().cuda(), dx, dxp, coef,
                                    state_words(step).cuda(), rng_words(seed, off, stream).cuda(), G_TEXT, G_IMAGE, RESCALE)
        rec.run()
        torch.cuda.synchronize()
        return dx.cpu(), dxp.cpu()

    base, base_x0 = launch()
    again, again_x0 = launch()
    assert torch.equal(base, again) and torch.equal(base_x0, again_x0)
    for change in (dict(seed=SEED ^ 1), dict(seed=SEED ^ (1 << 32)), dict(off=1), dict(stream=1), dict(step=2)):
        other, other_x0 = launch(**change)
        assert torch.equal(other_x0, base_x0), change                                   # x0 carries no noise
        for b in range(shape[0]):
            assert (other[b] != base[b]).float().mean().item() > 0.99, (change, b)       # fresh normals everywhere
    assert torch.equal(launch(seed=SEED + (1 << 64))[0], base)                           # rng_words takes the seed modulo 2^64, as set_noise_stream does
    one, one_x0 = launch(off=1, sl=slice(1, 2))
    assert torch.equal(one[0], base[1]) and torch.equal(one_x0[0], base_x0[1])
    last_a, last_b = launch(step=5, coef=real_rows)[0], launch(seed=99, off=7, stream=3, step=5, coef=real_rows)[0]
    assert torch.equal(last_a, last_b)
    assert not torch.equal(launch(step=3, coef=real_rows)[0], launch(seed=99, step=3, coef=real_rows)[0])


def test_rejected_arguments_launch_nothing(rec_cls, coef6):
    """A NULL ``rng``, ``chw % 4 != 0`` and ``mask`` without ``known`` return hipErrorInvalidValue (1); the latents keep their bits."""
    from photoverse_amd import _lib
    lib = _lib.load()
    shape = (2, 4, 4, 4)
    g = torch.Generator().manual_seed(2)
    eu, ec, x, xp, known, noise = (torch.randn(shape, generator=g).cuda() for _ in range(6))
    mask = torch.ones(2, 1, 4, 4).cuda()
    coef, state, rng = coef6.cuda(), state_words(3).cuda(), rng_words(SEED).cuda()
    x_before, xp_before = x.clone(), xp.clone()
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()

    def call(rng_=rng, mask_=None, known_=None, noise_=None, channels=4, hw=16):
        return lib.pv_cfg_dpm_step_stochastic(p(eu), None, p(ec), p(x), p(xp), p(coef), p(state), p(rng_), G_TEXT, G_TEXT, 0.0, p(mask_), p(known_),
                                              p(noise_), 2, channels, hw, s)

    assert call(rng_=None) == 1
    assert call(channels=3, hw=2) == 1 and call(channels=2, hw=6) == 1 and call(channels=1, hw=9) == 1        # chw = 6, 12, 9: hw % 4 != 0
    assert call(mask_=mask) == 1 and call(mask_=mask, noise_=noise) == 1 and call(known_=known, noise_=noise) == 1
    torch.cuda.synchronize()
    assert torch.equal(x, x_before) and torch.equal(xp, xp_before)
    assert call(mask_=mask, known_=known, noise_=noise) == 0                             # the same pointers, complete: launched
    torch.cuda.synchronize()
    assert not torch.equal(x, x_before)


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
LOOP_SEED = 20261018


@pytest.fixture(scope="module")
def loop_inputs():
    g = torch.Generator().manual_seed(81)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)
    return cond, uncond, noise


def sde_scheduler():
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(algorithm_type=SDE)


def sde_loop(hip, **kw):
    from photoverse_amd.pipeline import DenoiseLoop
    return DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=sde_scheduler(), stochastic=True, **kw)


def _run(loop, cond, uncond, noise, start=0):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    loop.reset(noise, start)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == STEPS
    return out


@torch.no_grad()
def oracle_run(ref, cond, uncond, x, seed, start=0, image=False, rescale=0.0, inpaint=None, sample_offset=0, stream=0):
    """The fp32 oracle UNet stepped by the fp64 SDE restatement (``sde_rows_ref`` on the oracle scheduler's sigmas, ``stochastic_step_ref``) under the
    numpy noise of (seed, sample_offset, stream, absolute step).  ``inpaint`` = (mask, known, noise) or None."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(STEPS)
    rows = sde_rows_ref(sch.sigmas, start, blend=inpaint is not None)
    x, x0_prev = x.clone().float(), torch.zeros_like(x)
    blend = dict(zip(("mask", "known", "noise"), inpaint)) if inpaint is not None else {}
    for i in range(start, STEPS):
        t = sch.timesteps[i]
        eu = ref(x, t, encoder_hidden_states=uncond).sample
        em = ref(x, t, encoder_hidden_states=(uncond[0], cond[1])).sample if image else None
        ec = ref(x, t, encoder_hidden_states=cond).sample
        z = noise_ref(tuple(x.shape), seed, sample_offset, stream, i)
        xn, x0 = stochastic_step_ref(eu, em, ec, x, x0_prev, rows[i], z, G_TEXT, G_IMAGE if image else None, rescale, **blend)
        x, x0_prev = xn.float(), x0.float()
    return x


@torch.no_grad()
def test_defaults_are_untouched_and_mismatches_are_refused(tiny_pair, loop_inputs):
    """The first loop test of the module: a default loop built before any stochastic loop exists on this UNet and one built after several have run -
    the same tail, launch count and output bits.  The stochastic loop has the same launch count and another output; it keeps its bits under
    ``share_prefix``.  ``stochastic`` has to agree with the scheduler's type."""
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    _, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert [fn.__name__ for fn, _ in before.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"] and not before.stochastic
    out_before = _run(before, cond, uncond, noise)
    sde = sde_loop(hip)
    assert sde.launches_per_step == before.launches_per_step and sde.merge_lowres == before.merge_lowres and len(sde.tail) == 2
    out_sde = _run(sde, cond, uncond, noise)
    assert torch.isfinite(out_sde).all() and not torch.equal(out_sde, out_before)
    implied = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, stochastic=True)                 # no scheduler given: the loop builds the SDE one
    assert implied.scheduler.stochastic and torch.equal(_run(implied, cond, uncond, noise), out_sde)
    shared = sde_loop(hip, share_prefix=True)
    assert shared.share_prefix and torch.equal(_run(shared, cond, uncond, noise), out_sde)
    with pytest.raises(ValueError, match="stochastic"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=DPMSolverMultistepScheduler(), stochastic=True)
    with pytest.raises(ValueError, match="stochastic"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=sde_scheduler())
    with pytest.raises(ValueError, match="stochastic"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=DDIMScheduler(), stochastic=True)
    with pytest.raises(ValueError, match="training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, stochastic=True)
    with pytest.raises(RuntimeError, match="stochastic"):
        before.set_noise_stream(1)
    after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert after.launches_per_step == before.launches_per_step and after.merge_lowres == before.merge_lowres
    assert [fn.__name__ for fn, _ in after.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"]
    assert torch.equal(_run(after, cond, uncond, noise), out_before)


@torch.no_grad()
@pytest.mark.parametrize("full", [False, True], ids=["plain", "image3_rescale0.7_inpaint"])
def test_stochastic_loop_matches_oracle(tiny_pair, loop_inputs, full):
    """guidance 7.5, 4 steps at B = 2, 16 x 16, plain and with image_guidance_scale 3 + guidance_rescale 0.7 + an inpainting mask of mixed zeros and
    ones: the final latents against the fp32 oracle under the same noise, rel-L2 below TOL_LOOP = 2.5e-3 (the noise is identical on both sides and
    adds no error of its own).  Measured on MI355X (printed with -s): plain 1.542e-3, with the three settings 1.342e-3."""
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    kw, okw, inpaint = {}, {}, None
    if full:
        g = torch.Generator().manual_seed(5)
        mask = (torch.rand(B, 1, S, S, generator=g) > 0.4).float()
        assert 0 < mask.sum() < mask.numel()
        inpaint = (mask, torch.randn(B, 4, S, S, generator=g), torch.randn(B, 4, S, S, generator=g))
        kw = dict(image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE, inpaint=True)
        okw = dict(image=True, rescale=RESCALE, inpaint=inpaint)
    exp = oracle_run(ref, cond, uncond, noise, LOOP_SEED, **okw)
    loop = sde_loop(hip, **kw)
    assert [fn.__name__ for fn, _ in loop.tail.calls] == ["pv_cfg_dpm_step_stochastic", "pv_step_advance"]
    if full:
        loop.set_inpaint(*(t.cuda() for t in inpaint))
    loop.set_noise_stream(LOOP_SEED)
    out = _run(loop, cond, uncond, noise)
    err = rel_l2(out, exp)
    print(f"stochastic loop ({'image 3.0, rescale 0.7, inpaint' if full else 'plain'}), guidance {G_TEXT}, {STEPS} steps: rel-L2 vs fp32 oracle = {err:.3e}")
    assert err < TOL_LOOP


@torch.no_grad()
def test_graph_behaviour(tiny_pair, loop_inputs):
    """Eager == graph == graph with side streams, bit for bit, for the two-forward loop (one side stream, two graph branches) and for the
    three-forward loop with ``image_guidance_scale=3`` and ``guidance_rescale=0.7`` (two side streams, three graph branches).  After capture,
    ``set_noise_stream(other seed)`` + ``reset`` + ``run`` is a fresh
    eager loop built with that seed, bit for bit.  ``reset(noise, start=2)`` runs the last two steps of the oracle's schedule started there under the
    noise of the absolute steps 2 and 3 (measured on MI355X: rel-L2 1.739e-3 against the oracle, 0.35 against the oracle under another seed).  A
    never-set stream is seed 0; ``reset`` leaves ``rng`` alone."""
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    for kw, n_side in ((dict(image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE), 2), ({}, 1)):
        outs, loops = [], []
        for use_graph, two in ((False, False), (True, False), (True, True)):
            loop = sde_loop(hip, use_graph=use_graph, two_streams=two, **kw)
            assert len(loop._sides) == (n_side if two else 0) and len(loop.engines_i) == n_side - 1
            loop.set_noise_stream(LOOP_SEED)
            outs.append(_run(loop, cond, uncond, noise))
            loops.append(loop)
        assert loops[1].graph is not None and loops[2].graph is not None and loops[0].graph is None
        assert torch.equal(outs[0], outs[1]), kw                   # graph replay == eager launches, bit for bit
        assert torch.equal(outs[0], outs[2]), kw                   # ... == the graph with its side streams
    graph_loop = loops[2]
    graph = graph_loop.graph
    assert graph is not None
    # another seed through the captured graph == a fresh eager loop with that seed
    graph_loop.set_noise_stream(LOOP_SEED + 1)
    replay = _run(graph_loop, cond, uncond, noise)
    assert graph_loop.graph is graph and graph_loop.rng.cpu().tolist() == [LOOP_SEED + 1, 0, 0, 0]
    fresh = sde_loop(hip, use_graph=False, two_streams=False)
    fresh.set_noise_stream(LOOP_SEED + 1)
    assert torch.equal(replay, _run(fresh, cond, uncond, noise)) and not torch.equal(replay, outs[0])
    assert torch.equal(_run(graph_loop, cond, uncond, noise), replay)                   # reset() does not touch rng: the same stream again
    # a never-set stream is seed 0
    unset = sde_loop(hip)
    assert unset.rng.cpu().tolist() == [0, 0, 0, 0]
    zero = sde_loop(hip)
    zero.set_noise_stream(0)
    assert torch.equal(_run(unset, cond, uncond, noise), _run(zero, cond, uncond, noise))
    zero.set_noise_stream(-1, 5, 1)                                                     # modulo 2^64
    assert zero.rng.cpu().tolist() == [-1, -1, 5, 1]
    # start = 2 through the captured graph: the counter carries the absolute step
    graph_loop.set_noise_stream(LOOP_SEED)
    x2 = torch.randn(B, 4, S, S, generator=torch.Generator().manual_seed(6)) * 0.8
    got = _run(graph_loop, cond, uncond, x2, start=2)
    exp = oracle_run(ref, cond, uncond, x2, LOOP_SEED, start=2)
    err = rel_l2(got, exp)
    wrong = rel_l2(got, oracle_run(ref, cond, uncond, x2, LOOP_SEED + 1, start=2))
    print(f"stochastic loop from start = 2: rel-L2 vs fp32 oracle = {err:.3e} (against the oracle under another seed: {wrong:.3e})")
    assert err < TOL_LOOP < wrong


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_sampler_end_to_end():
    """``run_inference(sampler="sde-dpmsolver++")`` on the tiny models and the tiny x2 VAE: the same seed twice gives equal images, another seed
    different ones; ``sampler="dpmsolver++"`` is the call without the keyword, bit for bit; a hires call (16 -> 24) runs and its second pass draws
    from stream 1 (latents: the tiny x2 VAE has no decode plan at 24 x 24 latents); sample 1 of a batch of 2 and the same sample alone at
    ``sample_offset=1`` agree within TOL_LOOP (the plans may differ with the batch, so bit-equality is not asked; measured on MI355X: rel-L2 0, and 0.65
    at the wrong offset); an unseeded call leaves the start noise as it was."""
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
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4)
    args = (ex, tok, ie, te, unet, ta, ia)
    plain = run_inference(*args, hip_vae, sch, "cuda", [1], seed=1, **kw)
    named = run_inference(*args, hip_vae, sch, "cuda", [1], seed=1, sampler="dpmsolver++", **kw)
    assert torch.equal(plain, named)
    cache = unet.__dict__["_denoise_loops"]
    assert len(cache) == 1 and not next(iter(cache.values())).stochastic
    a = run_inference(*args, hip_vae, sch, "cuda", [1], seed=1, sampler=SDE, **kw)
    assert a.shape == (2, 3, 32, 32) and torch.isfinite(a).all() and not torch.equal(a, plain)
    loop = next(reversed(cache.values()))
    assert len(cache) == 2 and loop.stochastic and loop.rng.cpu().tolist() == [1, 0, 0, 0]
    a2 = run_inference(*args, hip_vae, sch, "cuda", [1], seed=1, sampler=SDE, **kw)
    assert torch.equal(a, a2) and next(reversed(cache.values())) is loop
    b = run_inference(*args, hip_vae, sch, "cuda", [1], seed=2, sampler=SDE, **kw)
    assert torch.isfinite(b).all() and not torch.equal(a, b) and next(reversed(cache.values())).rng.cpu().tolist() == [2, 0, 0, 0]      # (the seed is part of the cache key)
    # the stream alone changes the result: the same start noise under another seed
    start = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(8))
    n1 = run_inference(*args, None, sch, "cuda", [1], seed=1, noise=start, sampler=SDE, **kw)
    n2 = run_inference(*args, None, sch, "cuda", [1], seed=2, noise=start, sampler=SDE, **kw)
    assert n1.shape == (2, 4, 16, 16) and not torch.equal(n1, n2)
    # sample 1 of the batch of 2 == the same sample alone at sample_offset 1
    one = {k: v[1:2] for k, v in ex.items()}
    alone = run_inference(one, tok, ie, te, unet, ta, ia, None, sch, "cuda", [1], seed=1, noise=start[1:2], sampler=SDE, sample_offset=1, **kw)
    err = rel_l2(alone[0], n1[1])
    elsewhere = run_inference(one, tok, ie, te, unet, ta, ia, None, sch, "cuda", [1], seed=1, noise=start[1:2], sampler=SDE, sample_offset=0, **kw)
    print(f"sample 1 of a batch of 2 against the same sample alone at sample_offset 1: rel-L2 = {err:.3e} (at offset 0: {rel_l2(elsewhere[0], n1[1]):.3e})")
    assert err < TOL_LOOP < rel_l2(elsewhere[0], n1[1])
    # unseeded: one draw for the stream after the start noise, which stays what it was
    torch.manual_seed(77)
    first = torch.randn(2, 4, 16, 16)
    torch.manual_seed(77)
    run_inference(*args, None, sch, "cuda", [1], sampler=SDE, **kw)
    drawn = torch.randint(0, 1 << 62, (1,))                                            # the generator is one randn and one randint further
    torch.manual_seed(77)
    torch.randn(2, 4, 16, 16)
    seed_drawn = int(torch.randint(0, 1 << 62, (1,)).item())
    assert torch.equal(drawn, torch.randint(0, 1 << 62, (1,)))
    want = run_inference(*args, None, sch, "cuda", [1], seed=seed_drawn, noise=first, sampler=SDE, **kw)
    torch.manual_seed(77)
    assert torch.equal(run_inference(*args, None, sch, "cuda", [1], sampler=SDE, **kw), want)
    # hires 16 -> 24: the second pass's loop draws from stream 1
    hi = run_inference(*args, None, sch, "cuda", [1], seed=1, sampler=SDE, hires_latent_size=24, hires_strength=0.5, **kw)
    assert hi.shape == (2, 4, 24, 24) and torch.isfinite(hi).all()
    loop2 = next(reversed(cache.values()))
    assert loop2.S == 24 and loop2.stochastic and loop2.rng.cpu().tolist() == [1, 0, 0, 1]
    first_pass = [l for l in cache.values() if l.S == 16 and l.B == 2 and l.stochastic]
    assert len(first_pass) == 1 and first_pass[0].rng.cpu().tolist() == [1, 0, 0, 0]
    # ... and the deterministic call is what it was
    assert torch.equal(run_inference(*args, hip_vae, sch, "cuda", [1], seed=1, **kw), plain)


def test_generate_cli_runs_with_the_sampler_flag(tmp_path):
    """generate.py --sampler sde-dpmsolver++ runs as a program and writes its image."""
    import subprocess
    import sys
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--tiny", "--model_path", "random", "--synthetic_input", "--sampler", SDE, "--seed", "1",
           "--num_timesteps", "4", "--latent_size", "16", "--num_of_samples", "1", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png"]
    a = np.asarray(Image.open(out / files[0]))
    assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
