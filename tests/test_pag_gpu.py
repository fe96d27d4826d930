"""GPU tests of perturbed-attention guidance: ``pv_cfg_dpm_step_pag`` against the fp64 evaluation of the header's formulas
(``test_pag_cpu.pag_step_ref``; the SDE form under the numpy Philox of ``test_sampler_cpu``) and, bit for bit, against the two launchers it extends;
the engine's perturbed forward (``UNetEngine(perturb=...)``) against the fp32 oracle UNet with an identity processor on the chosen ``attn1``; the
``DenoiseLoop`` with ``pag_scale`` against the oracle loop, graph == eager, shared trunk == whole perturbed forward; ``run_inference`` / the CLI end to
end on the tiny models."""
import os

import pytest
import torch

from test_guidance_cpu import SHAPES, guided_step_ref
from test_pag_cpu import (B, G_IMAGE, G_PAG, G_TEXT, P, RESCALE, S, STEPS, TOL_FWD, TOL_LOOP, TOL_RESCALE, TOL_STEP, loop_inputs_81, make_eps4, oracle_loop,
                          pag_step_ref, perturbed_oracle, rel_l2, tiny_oracle)
from test_sampler_cpu import SDE, noise_ref

pytestmark = pytest.mark.gpu

ROWS = (0, 3, 5)                 # first-order first row, a second-order middle row, the last row ((q0, q1) = (1, 0), cn = 0)
SEED, OFFSET, STREAM = 0x1234_5678_9abc_def1, 3, 1
MID, UP11 = ("mid_block.attentions.0",), ("up_blocks.1.attentions.1",)
ALL = ("down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


def _table(algorithm_type):
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler(algorithm_type=algorithm_type)
    sch.set_timesteps(6)
    return sch.coefficient_table(0, blend=True)


@pytest.fixture(scope="module")
def tables():
    return {False: _table("dpmsolver++"), True: _table(SDE)}


def rng_words(seed, sample_offset=0, stream=0):
    import numpy as np
    seed %= 1 << 64
    return torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32, sample_offset, stream], dtype=np.uint32).view(np.int32).copy())


def mixed_mask(shape, g):
    """Zeros, ones and fractional values, every kind present."""
    r = torch.rand(shape, generator=g)
    m = torch.where(r < 0.3, torch.zeros(()), torch.where(r > 0.7, torch.ones(()), r))
    m.view(-1)[:3] = torch.tensor([0.0, 1.0, 0.5])
    return m.contiguous()


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("sde", (False, True), ids=("ode", "sde"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pag_step_kernel(rec_cls, tables, shape, sde):
    """``pv_cfg_dpm_step_pag`` on rows 0, 3 and 5 of the real 6-step coefficient table (``sde``: the SDE table with ``rng`` set, the noise from the numpy
    Philox), in the forms PAG alone, PAG + image, PAG + image + rescale, each with and without a mask, against ``pag_step_ref`` (fp64 on the same fp32
    inputs): rtol = atol = TOL_STEP without rescale, TOL_RESCALE with (the weights -1, -3, 7, -2 sum in magnitude to 13, below the 14 those bounds were
    set at).  Bit for bit: ``eps_perturbed`` None and ``g_pag`` 0 are ``pv_cfg_dpm_step_guided`` (``rng`` None) / ``pv_cfg_dpm_step_stochastic`` (``rng``
    set), masked and unmasked; ``x0_prev`` of a masked form is the unmasked form's ``x0``; mask 0 is ``q0*known + q1*noise`` in fp32; every read-only
    input is unchanged.
    Measured on MI355X (printed with -s), largest max |got - fp64| / (1 + |fp64|) over the rows and forms of each shape, without / with rescale (the
    ``sde`` cases gave the same figures to three digits except where noted): 4.9e-7 / 3.9e-7 (sde 2.8e-7), 1.7e-6 / 3.3e-7, 3.1e-6 / 5.0e-7 (sde 3.9e-7),
    4.9e-6 / 3.8e-6, 4.5e-6 / 1.4e-6; max |got - fp64| 3.2e-5 ... 7.5e-5 / 2.3e-5 ... 4.0e-5.  The two largest shapes are above a quarter of their bounds
    (2.5e-6, 2.3e-6), as they are in the guided launcher's own test (4.7e-6 / 2.3e-6): the prediction has means of 33 (weights 13 on means of +-3)
    and |cb| = 15.6 on row 0, so ``cb * e`` reaches several hundred, where one fp32 ulp is 3.1e-5 - 6.1e-5 - the absolute error IS one or two ulps
    of the largest term - and the relative figure peaks at the few elements where ``ca * x`` and ``cb * e`` cancel to a result near 10.  The error
    does not grow with chw beyond that (24 x 40 and 64 x 64 agree), so the bounds stay."""
    n, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 13)
    eu, em, ec, ep = make_eps4(shape, g)
    x, xp, known, noise = (torch.randn(shape, generator=g).contiguous() for _ in range(4))
    mask = mixed_mask((n, 1, H, W), g)
    mm = mask.expand(n, C, H, W)
    coef = tables[sde]
    rng = rng_words(SEED, OFFSET, STREAM)
    d_eu, d_em, d_ec, d_ep, d_coef, d_mask, d_known, d_noise, d_rng = (t.cuda() for t in (eu, em, ec, ep, coef, mask, known, noise, rng))
    rkw = dict(rng=d_rng) if sde else {}
    forms = [(None, 0.0), (em, 0.0), (em, RESCALE)]
    worst = {False: 0.0, True: 0.0}
    worst_abs = {False: 0.0, True: 0.0}
    for row in ROWS:
        d_state = torch.tensor([row, 6, 0, 0], dtype=torch.int32).cuda()
        rec = rec_cls("cuda")
        runs = []
        for img, rs in forms:
            for masked in (False, True):
                dx, dxp = x.cuda(), xp.cuda()
                blend = dict(mask=d_mask, known=d_known, noise=d_noise) if masked else {}
                rec.cfg_dpm_step_pag(d_eu, None if img is None else d_em, d_ec, d_ep, dx, dxp, d_coef, d_state, G_TEXT, G_IMAGE, G_PAG, rs, **rkw, **blend)
                runs.append((img, rs, masked, dx, dxp))
        # the contract: without a perturbed prediction, or at scale 0, the launchers this one extends - on their own copies
        pairs = []
        for masked in (False, True):
            blend = dict(mask=d_mask, known=d_known, noise=d_noise) if masked else {}
            old, old_p = x.cuda(), xp.cuda()
            if sde:
                rec.cfg_dpm_step_stochastic(d_eu, d_em, d_ec, old, old_p, d_coef, d_state, d_rng, G_TEXT, G_IMAGE, RESCALE, **blend)
            else:
                rec.cfg_dpm_step_guided(d_eu, d_em, d_ec, old, old_p, d_coef, d_state, G_TEXT, G_IMAGE, RESCALE, **blend)
            for d_p, gp in ((None, G_PAG), (d_ep, 0.0), (None, 0.0)):
                new, new_p = x.cuda(), xp.cuda()
                rec.cfg_dpm_step_pag(d_eu, d_em, d_ec, d_p, new, new_p, d_coef, d_state, G_TEXT, G_IMAGE, gp, RESCALE, **rkw, **blend)
                pairs.append((masked, d_p is None, gp, new, new_p, old, old_p))
        rec.run()
        torch.cuda.synchronize()
        for masked, no_p, gp, new, new_p, old, old_p in pairs:
            assert torch.equal(new, old) and torch.equal(new_p, old_p), \
                f"row {row} mask {int(masked)} eps_perturbed {'None' if no_p else 'given'} g_pag {gp}: not the bits of the launcher without PAG"
        z = noise_ref(shape, SEED, OFFSET, STREAM, row) if sde else None
        k32 = coef[row, 5] * known + coef[row, 6] * noise
        x0_unmasked = {}
        for img, rs, masked, dx, dxp in runs:
            got, got_x0 = dx.cpu(), dxp.cpu()
            blend = dict(mask=mask, known=known, noise=noise) if masked else {}
            exp, x0, f = pag_step_ref(eu, img, ec, ep, x, xp, coef[row], G_TEXT, G_IMAGE, G_PAG, rs, z=z, **blend)
            if rs > 0 and n > 1:
                assert f.unique().numel() == n                                            # a factor per sample
            tol = TOL_RESCALE if rs > 0 else TOL_STEP
            err = max(((got.double() - exp).abs() / (1 + exp.abs())).max().item(), ((got_x0.double() - x0).abs() / (1 + x0.abs())).max().item())
            err_abs = max((got.double() - exp).abs().max().item(), (got_x0.double() - x0).abs().max().item())
            worst[rs > 0], worst_abs[rs > 0] = max(worst[rs > 0], err), max(worst_abs[rs > 0], err_abs)
            print(f"pag step {'sde' if sde else 'ode'} {shape} row {row} {'PAG + image' if img is not None else 'PAG alone'} rescale {rs} mask {int(masked)}: "
                  f"max |d| / (1 + |fp64|) = {err:.3e}, max |d| = {err_abs:.3e}, f = {[round(v, 4) for v in f.tolist()]}")
            torch.testing.assert_close(got_x0.double(), x0, rtol=tol, atol=tol)
            torch.testing.assert_close(got.double(), exp, rtol=tol, atol=tol)
            # the perturbed prediction really entered: the step without it is elsewhere
            without, _, _ = guided_step_ref(eu, img, ec, x, xp, coef[row], G_TEXT, G_IMAGE, rs)
            if not masked and not sde:
                assert (got.double() - without).abs().max().item() > 1e-2
            if masked:
                assert torch.equal(got_x0, x0_unmasked[(img is None, rs)])                # x0_prev holds the unblended x0
                assert torch.equal(got[mm == 0], k32[mm == 0])                            # the kept region, exactly
            else:
                x0_unmasked[(img is None, rs)] = got_x0
        assert d_state.cpu().tolist() == [row, 6, 0, 0]
    print(f"pag step {'sde' if sde else 'ode'} {shape}: worst max |d| / (1 + |fp64|) without rescale {worst[False]:.3e} (abs {worst_abs[False]:.3e}), "
          f"with rescale {worst[True]:.3e} (abs {worst_abs[True]:.3e})")
    assert (mm == 1).any() and (mm == 0).any() and ((mm > 0) & (mm < 1)).any()
    for dev, host in ((d_eu, eu), (d_em, em), (d_ec, ec), (d_ep, ep), (d_coef, coef), (d_mask, mask), (d_known, known), (d_noise, noise), (d_rng, rng)):
        assert torch.equal(dev.cpu(), host)


# ---------------------------------------------------------------------------------------------------------------- the perturbed forward
@pytest.fixture(scope="module")
def tiny_pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    ref = tiny_oracle()
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    return ref, hip


@pytest.fixture(scope="module")
def loop_inputs():
    return loop_inputs_81()


def _launches(eng):
    return [fn.__name__ for fn, _ in eng.rec.calls], [t[0] for t in eng.rec.tags], [fn.__name__ for fn, _ in eng.rec_cond.calls]


@torch.no_grad()
def test_perturbed_forward_matches_the_perturbed_oracle(tiny_pair, loop_inputs):
    """``UNetEngine(perturb=...)`` at B = 2, 16 x 16, t = 500 against the fp32 oracle whose chosen ``attn1`` return ``to_out(to_v(x))``: rel-L2 below
    TOL_FWD for the mid block alone (C = 640, d = 80, 64 tokens), ``up_blocks.1.attentions.1`` alone (C = 320, d = 40, 256 tokens) and all four
    transformers - and each result more than 10 x TOL_FWD from the UNperturbed oracle, so an engine that ignored ``perturb`` could not pass.  The perturbed
    plan has no attention launch for a perturbed layer.  A ``perturb=()`` engine built afterwards has the launch list of one built before.
    Measured on MI355X (printed with -s), rel-L2 against the perturbed / the unperturbed oracle: mid block 1.243e-3 / 9.627e-2,
    ``up_blocks.1.attentions.1`` 1.275e-3 / 3.043e-1, all 1.262e-3 / 4.466e-1; 102, 103 and 99 launches against the unperturbed plan's 104."""
    ref, hip = tiny_pair
    cond, _, noise = loop_inputs
    t = torch.tensor([500.0])
    d_text, d_ip = cond[0].reshape(-1, 768).half().cuda().contiguous(), cond[1].reshape(-1, 768).half().cuda().contiguous()
    common = dict(latents_in=noise.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=t.cuda())
    before = hip.engine(B, S, S, P, 1, **common)
    plain_oracle = ref(noise, 500, encoder_hidden_states=cond).sample
    n_attn = sum(1 for nm in before.rec.tags if "attention" in nm[0] or "attn" in nm[0])
    for names in (MID, UP11, ALL):
        eng = hip.engine(B, S, S, P, 1, perturb=names, **common)
        assert len(eng.rec) < len(before.rec)
        got = eng.run().clone().float().cpu()
        torch.cuda.synchronize()
        exp = perturbed_oracle(ref, names)(noise, 500, encoder_hidden_states=cond).sample
        err, away = rel_l2(got, exp), rel_l2(got, plain_oracle)
        print(f"perturbed forward {names if len(names) < 4 else 'all'}: rel-L2 vs the perturbed oracle = {err:.3e}, vs the unperturbed oracle = {away:.3e}, "
              f"launches {len(eng.rec)} (unperturbed {len(before.rec)}, of them {n_attn} attention)")
        assert torch.isfinite(got).all() and err < TOL_FWD
        assert away > 10 * TOL_FWD
    got = before.run().clone().float().cpu()
    assert rel_l2(got, plain_oracle) < TOL_FWD
    after = hip.engine(B, S, S, P, 1, **common)
    assert _launches(after) == _launches(before) and after.perturb == ()
    assert torch.equal(after.run().float().cpu(), got)
    with pytest.raises(ValueError, match="perturb"):
        hip.engine(B, S, S, P, 1, perturb=("mid_block.attentions.7",), **common)
    with pytest.raises(ValueError, match="trunk"):
        hip.engine(B, S, S, P, 1, trunk=before, **common)


# ---------------------------------------------------------------------------------------------------------------- the loop
def _run(loop, cond, uncond, noise):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    loop.reset(noise)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == STEPS
    return out


@torch.no_grad()
def test_pag_loops_match_the_oracle_and_graph_equals_eager(tiny_pair, loop_inputs):
    """4 steps at B = 2, 16 x 16, guidance 5, against the oracle loop (``test_pag_cpu.oracle_loop``), rel-L2 below TOL_LOOP each: (a) PAG 2 alone on the
    mid block (three forwards per step); (b) PAG 2 + image guidance 2 + rescale 0.7 on all four transformers (four oracle forwards per step).  For
    both: eager launches == graph replay == the graph with side streams, bit for bit; no stream beyond the loop without PAG; the tail is
    ``pv_cfg_dpm_step_pag`` + ``pv_step_advance``.  Measured on MI355X (printed with -s): rel-L2 (a) 1.111e-3, (b) 8.600e-4."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    cases = (("a: PAG alone, mid block", MID, dict(), dict(pag_scale=G_PAG, pag_layers=("mid_block",))),
             ("b: PAG + image + rescale, all layers", ALL, dict(g_image=G_IMAGE, rescale=RESCALE),
              dict(pag_scale=G_PAG, pag_layers="all", image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE)))
    for label, names, okw, lkw in cases:
        exp = oracle_loop(ref, perturbed_oracle(ref, names), cond, uncond, noise, G_TEXT, g_pag=G_PAG, **okw)
        three = "image_guidance_scale" in lkw
        outs = []
        for use_graph, two in ((False, False), (True, False), (True, True)):
            loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, use_graph=use_graph, two_streams=two, **lkw)
            assert loop.pag_layers == names and len(loop.engines_p_attn) == 1 and not loop.merge_lowres and loop.share_trunk
            assert len(loop.engines_i) == (1 if three else 0) and len(loop._sides) == (((3 if three else 2) - 1) if two else 0)
            assert [fn.__name__ for fn, _ in loop.tail.calls] == ["pv_cfg_dpm_step_pag", "pv_step_advance"]
            assert loop.launches_per_step == sum(len(e.rec) for e in loop.all_engines) + 2 and loop.engines_p_attn[0] in loop.all_engines
            outs.append(_run(loop, cond, uncond, noise))
        err = rel_l2(outs[2], exp)
        print(f"pag loop ({label}), guidance {G_TEXT} pag {G_PAG}, {STEPS} steps: rel-L2 vs fp32 oracle = {err:.3e}")
        assert torch.equal(outs[0], outs[1])                       # graph replay == eager launches, bit for bit
        assert torch.equal(outs[0], outs[2])                       # ... == the graph with side streams
        assert err < TOL_LOOP


@torch.no_grad()
def test_shared_trunk_has_the_bits_of_the_whole_perturbed_forward_and_fewer_launches(tiny_pair, loop_inputs):
    """``share_trunk=True`` (the default with PAG) == ``share_trunk=False`` bit for bit, for the mid block (the trunk is the whole down path and the mid
    block's first ResnetBlock) and for ``up_blocks.1.attentions.1`` (the trunk reaches into the up path: the adopted skip stack is shorter than the
    one the down path left), eager and captured; the trunk loop has strictly fewer launches per step, the conditional plan the same launches.
    Measured on MI355X: bit for bit; launches per step 312 -> 281 (mid block: the perturbed plan 102 -> 71) and 313 -> 225 (103 -> 15)."""
    from photoverse_amd.pipeline import DenoiseLoop
    _, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    for layers in (("mid_block",), UP11):
        full = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=layers, share_trunk=False)
        trunk = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=layers)
        eager = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=layers, share_trunk=True, use_graph=False, two_streams=False)
        assert trunk.share_trunk and eager.share_trunk and not full.share_trunk
        assert trunk.launches_per_step < full.launches_per_step and eager.launches_per_step == trunk.launches_per_step
        assert len(trunk.engines_c[0].rec) == len(full.engines_c[0].rec) and len(trunk.engines_u[0].rec) == len(full.engines_u[0].rec)
        print(f"pag_layers {layers}: launches per step {full.launches_per_step} (whole perturbed forward) -> {trunk.launches_per_step} (shared trunk); "
              f"perturbed plan {len(full.engines_p_attn[0].rec)} -> {len(trunk.engines_p_attn[0].rec)}")
        out_full = _run(full, cond, uncond, noise)
        assert torch.equal(_run(trunk, cond, uncond, noise), out_full)
        assert torch.equal(_run(eager, cond, uncond, noise), out_full)
        assert torch.equal(_run(trunk, cond, uncond, noise), out_full)             # a second generation on the captured graph


@torch.no_grad()
def test_defaults_are_untouched_and_the_combinations_keep_their_bits(tiny_pair, loop_inputs):
    """``pag_scale`` 0 and None build the default loop: the launches and bits of a default loop, checked on loops built before and after the PAG
    loops.  With ``share_prefix`` (also where the first transformer itself is perturbed), with ``inpaint`` under a mask of ones, and ``stochastic``
    at ``pag_scale`` 0 the bits are kept.  ``training_mode``, a non-finite scale and unknown layers are refused."""
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    _, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert [fn.__name__ for fn, _ in before.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"] and not before.engines_p_attn and before.eps_p is None
    out_before = _run(before, cond, uncond, noise)
    kw = dict(pag_scale=G_PAG, image_guidance_scale=G_IMAGE, guidance_rescale=RESCALE)
    for layers in (("mid_block",), "all"):
        base = _run(DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_layers=layers, **kw), cond, uncond, noise)
        for trunk in (True, False):
            shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_prefix=True, pag_layers=layers, share_trunk=trunk, **kw)
            assert shared.share_prefix and len(shared.engines_p) == 1
            assert torch.equal(_run(shared, cond, uncond, noise), base), (layers, trunk)
        inp = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, inpaint=True, pag_layers=layers, **kw)          # the mask starts as ones, known / noise as zeros
        assert [fn.__name__ for fn, _ in inp.tail.calls] == ["pv_cfg_dpm_step_pag", "pv_step_advance"]
        assert torch.equal(_run(inp, cond, uncond, noise), base)
    # stochastic: scale 0 is the stochastic loop itself; with a scale the loop runs, is reproducible under its noise stream and differs
    sde = lambda: DPMSolverMultistepScheduler(algorithm_type=SDE)
    sto = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=sde(), stochastic=True)
    sto0 = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=sde(), stochastic=True, pag_scale=0.0)
    stop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, scheduler=sde(), stochastic=True, pag_scale=G_PAG)
    assert [fn.__name__ for fn, _ in sto0.tail.calls] == ["pv_cfg_dpm_step_stochastic", "pv_step_advance"] and not sto0.engines_p_attn
    assert [fn.__name__ for fn, _ in stop.tail.calls] == ["pv_cfg_dpm_step_pag", "pv_step_advance"]
    for lp in (sto, sto0, stop):
        lp.set_noise_stream(7, 0, 0)
    out_sto = _run(sto, cond, uncond, noise)
    assert torch.equal(_run(sto0, cond, uncond, noise), out_sto)
    out_stop = _run(stop, cond, uncond, noise)
    assert torch.isfinite(out_stop).all() and not torch.equal(out_stop, out_sto) and torch.equal(_run(stop, cond, uncond, noise), out_stop)
    with pytest.raises(ValueError, match="training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, pag_scale=G_PAG)
    for bad in (float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="pag_scale"):
            DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=bad)
    with pytest.raises(ValueError, match="pag_layers"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=("down_blocks.1",))
    for off in (dict(pag_scale=0), dict(pag_scale=None), dict(pag_scale=0.0, pag_layers=("nothing",), share_trunk=True), dict()):
        after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **off)
        assert after.launches_per_step == before.launches_per_step and after.merge_lowres == before.merge_lowres and not after.share_trunk
        assert not after.engines_p_attn and after.eps_p is None and len(after.all_engines) == len(before.all_engines)
        assert [fn.__name__ for fn, _ in after.tail.calls] == ["pv_cfg_dpm_step", "pv_step_advance"]
        assert [[fn.__name__ for fn, _ in e.rec.calls] for e in after.all_engines] == [[fn.__name__ for fn, _ in e.rec.calls] for e in before.all_engines]
        assert torch.equal(_run(after, cond, uncond, noise), out_before)


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_pag_end_to_end():
    """``run_inference(pag_scale=..., pag_layers=...)`` on the tiny models and the tiny x2 VAE: shapes, finiteness, determinism, the cached loop and its
    graph reused, the scale and the layers each change the result, with ``inpaint_mask`` the kept region is the photograph's bits, with
    ``hires_latent_size`` both cached loops carry PAG, and a plain call before and after gives identical bits."""
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
    pg = dict(pag_scale=2.0)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)          # a plain call, before ...
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(iter(cache.values()))
    # 1. latents: shape, finiteness, determinism, the cached loop and its graph reused
    a = run_inference(*args, None, sch, "cuda", [1], **kw, **pg)
    assert a.shape == (2, 4, 16, 16) and torch.isfinite(a).all()
    loop = next(reversed(cache.values()))
    assert loop is not plain_loop and len(loop.engines_p_attn) == 1 and loop.pag_scale == 2.0 and loop.pag_layers == MID and loop.share_trunk
    graph = loop.graph
    assert graph is not None
    a2 = run_inference(*args, None, sch, "cuda", [1], **kw, **pg)
    assert torch.equal(a, a2) and next(reversed(cache.values())) is loop and loop.graph is graph
    # 2. the scale and the layers each change the result; scale 0 is the plain call on the plain loop
    plain = run_inference(*args, None, sch, "cuda", [1], **kw)
    zero = run_inference(*args, None, sch, "cuda", [1], pag_scale=0, pag_layers=("up_blocks",), **kw)
    assert torch.equal(zero, plain) and next(reversed(cache.values())) is plain_loop
    other_scale = run_inference(*args, None, sch, "cuda", [1], pag_scale=1.0, **kw)
    other_layers = run_inference(*args, None, sch, "cuda", [1], pag_scale=2.0, pag_layers=("up_blocks",), **kw)
    assert next(reversed(cache.values())).pag_layers == ALL[2:]
    assert torch.isfinite(other_scale).all() and torch.isfinite(other_layers).all()
    assert not torch.equal(a, plain) and not torch.equal(other_scale, a) and not torch.equal(other_scale, plain) and not torch.equal(other_layers, a)
    with pytest.raises(ValueError, match="pag_layers"):
        run_inference(*args, None, sch, "cuda", [1], pag_scale=2.0, pag_layers=("down_blocks.1",), **kw)
    # 3. with inpaint_mask: images in [-1, 1], the kept region is the photograph's own bits
    mask = torch.zeros(1, 1, 32, 32)
    mask[..., 8:24, 4:20] = 1
    img = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw, **pg)
    assert img.shape == (2, 3, 32, 32) and torch.isfinite(img).all() and img.min() >= -1 and img.max() <= 1
    keep = (mask == 0).expand(2, 3, 32, 32)
    assert torch.equal(img.cpu()[keep], ex["pixel_values"].clamp(-1, 1)[keep])
    img_plain = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw)
    assert not torch.equal(img, img_plain)
    # 4. with hires_latent_size: both passes use the settings
    hi = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw, **pg)
    assert hi.shape == (2, 3, 64, 64) and torch.isfinite(hi).all()
    assert {k[1] for k in cache} == {16, 32} and all(len(l.engines_p_attn) == 1 and l.pag_scale == 2.0 and l.pag_layers == MID for l in cache.values())
    hi_plain = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw)
    assert not torch.equal(hi, hi_plain)
    # 5. ... and after: identical bits
    after = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)
    assert before.shape == (2, 3, 32, 32) and torch.equal(before, after)


def test_generate_cli_runs_with_the_pag_flags(tmp_path):
    """generate.py --pag_scale 2 --pag_layers mid_block up_blocks runs as a program and writes its PNGs."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--pag_scale", "2", "--pag_layers", "mid_block", "up_blocks", "--num_timesteps", "4", "--num_of_samples", "2",
           "--seed", "3", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
