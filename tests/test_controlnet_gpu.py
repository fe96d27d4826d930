"""GPU tests of ControlNet conditioning: ``pv_hint_conv3x3`` against an fp64 ``conv2d`` on the same fp16 inputs and weights; the conditioning embedding,
the control plan's features and the controlled UNet forward against the fp32 references of ``tests/test_controlnet_cpu.py``; the ``DenoiseLoop`` with a
ControlNet against the controlled oracle loop - graph == eager, off == today's loop, with PAG's shared trunk, FreeU, the shared prefix, the third
forward of ``image_guidance_scale`` and one stream; the control features at full-size widths; ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_controlnet_cpu import (ControlledRef, ControlNetRef, control_image, controlled_oracle, nonzero_init_, tiny_controlnet_ref)
from test_pag_cpu import B, G_PAG, G_TEXT, P, S, STEPS, TOL_FWD, TOL_LOOP, loop_inputs_81, oracle_loop, perturbed_oracle, rel_l2, tiny_oracle

pytestmark = pytest.mark.gpu

#: (B, Cin, Cout, H, W, stride): the image form at its smallest and at odd sizes; every channel pair of the embedding at sizes that leave fragments
#: ragged (fewer than 16 pixels, an odd size under stride 2, more than one workgroup with a ragged last wave); cout 96 = one and a half channel tiles
CONV_CASES = ((1, 3, 16, 2, 2, 1), (2, 3, 16, 5, 7, 1), (1, 16, 16, 3, 3, 1), (2, 16, 32, 6, 10, 2), (1, 32, 96, 5, 7, 2), (1, 96, 96, 4, 4, 1),
              (1, 96, 256, 8, 8, 2), (2, 32, 32, 33, 17, 1))
SLICE_CASE = (2, 16, 32, 6, 10, 2)
ACT_NONE, ACT_SILU = 0, 1


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


def conv_w(w):
    """[Cout, Cin, 3, 3] -> fp16 [Cout][9 * Cin], tap-major"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).half().contiguous()


def launch(lib, x, w, bias, out, *, batch, cin, cout, h, wd, stride, act):
    image = x.dim() == 4
    rc = lib.pv_hint_conv3x3(x.data_ptr(), int(image), 0 if image else x.stride(0), w.data_ptr(), bias.data_ptr(), out.data_ptr(), out.stride(0), batch,
                             cin, cout, h, wd, stride, act, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_hint_conv_against_the_fp64_conv2d(lib, case):
    """``|got - ref| <= 2^-10 |ref| + 2^-13 S`` with ``S = conv2d(|x|, |w|) + |b|``, with and without SiLU: the first term is the fp16 store, the second fp32
    accumulation over K <= 864 products (K 2^-24 <= 2^-14) with 2 x margin; SiLU's slope is at most 1.1.  ``ref``: fp64 ``conv2d`` (+ SiLU) on the same
    fp16 weights and fp16-representable inputs.  The inputs are unchanged.  SLICE_CASE also runs as a column slice of wider buffers (ldx = 24, ldo = 56)
    between guard rows: gap columns and guards keep their bits, the result has the bits of the dense launch.
    Measured on MI355X (printed with -s): worst |got - ref| / bound over both activations, in the order of CONV_CASES: 0.358, 0.410, 0.342, 0.342, 0.326,
    0.278, 0.280, 0.359 (max |got - ref| 8.3e-4 .. 1.9e-3: the fp16 store's rounding; the accumulation term is not what is used up)."""
    n, cin, cout, h, w, stride = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cin, h, w, generator=g).half()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half()
    bias = torch.randn(cout, generator=g)
    image = cin <= 4
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    pre = F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=1)
    bound_s = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), stride=stride, padding=1)
    assert pre.shape == (n, cout, ho, wo)
    host_x = x.float().contiguous() if image else rows_of(x)
    d_x, d_w, d_b = host_x.cuda(), conv_w(wt).cuda(), bias.cuda()
    worst = 0.0
    for act in (ACT_NONE, ACT_SILU):
        ref = F.silu(pre) if act == ACT_SILU else pre
        d_out = torch.full((n * ho * wo, cout), float("nan"), dtype=torch.float16, device="cuda")
        launch(lib, d_x, d_w, d_b, d_out, batch=n, cin=cin, cout=cout, h=h, wd=w, stride=stride, act=act)
        torch.cuda.synchronize()
        got = planes_of(d_out.cpu(), n, ho, wo).double()
        bound = 2.0 ** -10 * ref.abs() + 2.0 ** -13 * bound_s
        ratio = ((got - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        print(f"hint conv {case} act = {act}: max |got - ref| = {(got - ref).abs().max().item():.3e}, worst |got - ref| / bound = {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1.0
        assert torch.equal(d_x.cpu(), host_x) and torch.equal(d_w.cpu(), conv_w(wt)) and torch.equal(d_b.cpu(), bias)
        if case == SLICE_CASE:
            r_in, r_out = n * h * w, n * ho * wo
            wide_in = torch.randn(r_in, 24).half().cuda()
            wide_in[:, 8:24] = d_x
            wide_out = torch.randn(r_out + 4, 56).half().cuda()
            before = wide_out.clone()
            launch(lib, wide_in[:, 8:24], d_w, d_b, wide_out[2:2 + r_out, 16:48], batch=n, cin=cin, cout=cout, h=h, wd=w, stride=stride, act=act)
            torch.cuda.synchronize()
            assert torch.equal(wide_out[2:2 + r_out, 16:48].view(torch.int16), d_out.view(torch.int16))
            keep = torch.ones_like(wide_out, dtype=torch.bool)
            keep[2:2 + r_out, 16:48] = False
            assert torch.equal(wide_out.view(torch.int16)[keep], before.view(torch.int16)[keep])
    print(f"hint conv {case}: worst |got - ref| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def tiny_models():
    """(UNet oracle, ControlNet oracle, HIP UNet, HIP ControlNet): the tiny configuration, the HIP models loaded from the oracles' state dicts."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    ref, cn_ref = tiny_oracle(), tiny_controlnet_ref()
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    cn = ControlNetModel(**TINY_CONFIG)
    cn.load_state_dict(cn_ref.state_dict(), strict=True)
    cn.to("cuda")
    return ref, cn_ref, hip, cn


@pytest.fixture(scope="module")
def loop_inputs():
    return loop_inputs_81()


@pytest.fixture(scope="module")
def images():
    return control_image(), control_image(seed=6)


def _names(eng):
    return [fn.__name__ for fn, _ in eng.rec.calls]


@torch.no_grad()
def test_hint_embedding_all_eight_convs(tiny_models, images):
    """The conditioning embedding of a (2, 3, 128, 128) image - seven ``pv_hint_conv3x3`` launches and one ``pv_gemm_conv`` - against the fp32 reference:
    rel-L2 <= TOL_FWD; two images give different embeddings.  Measured on MI355X (printed with -s): rel-L2 9.006e-4."""
    from photoverse_amd.controlnet import hint_plan
    from photoverse_amd.ops import Recorder
    _, cn_ref, _, cn = tiny_models
    img, img2 = images
    d_img = img.cuda().contiguous()
    out = torch.full((B * S * S, 320), float("nan"), dtype=torch.float16, device="cuda")
    rec = Recorder("cuda")
    hint_plan(rec, cn.controlnet_cond_embedding, d_img, out)
    names = [fn.__name__ for fn, _ in rec.calls]
    assert names == ["pv_hint_conv3x3"] * 7 + ["pv_gemm_conv"] and [t[0] for t in rec.tags[:2]] == ["hint_conv_image_kernel", "hint_conv_rows_kernel"]
    rec.run()
    torch.cuda.synchronize()
    exp = cn_ref.controlnet_cond_embedding(img)
    err = rel_l2(planes_of(out.float().cpu(), B, S, S), exp)
    print(f"hint embedding (2, 3, 128, 128): rel-L2 vs the fp32 reference = {err:.3e}")
    assert torch.isfinite(out).all() and err <= TOL_FWD
    d_img.copy_(img2)
    rec.run()
    torch.cuda.synchronize()
    assert rel_l2(planes_of(out.float().cpu(), B, S, S), cn_ref.controlnet_cond_embedding(img2)) <= TOL_FWD
    assert rel_l2(cn_ref.controlnet_cond_embedding(img2), exp) > 100 * TOL_FWD


def _control_engine(cn, hip_common, img):
    from photoverse_amd.controlnet import hint_plan
    from photoverse_amd.ops import Recorder
    hint = torch.zeros((B * S * S, 320), dtype=torch.float16, device="cuda")
    rec = Recorder("cuda")
    hint_plan(rec, cn.controlnet_cond_embedding, img.cuda().contiguous(), hint)
    rec.run()
    return cn.control_engine(B, S, S, P, hint, **hip_common)


@torch.no_grad()
def test_control_features_and_residuals_at_tiny_size(tiny_models, loop_inputs, images):
    """The tiny control plan's 4 + 1 control features at B = 2, 16 x 16, t = 500, each against ``ControlNetRef.features``: rel-L2 <= TOL_FWD; and
    ``ControlNetModel.forward`` - the scaled zero-conv residuals in fp32 NCHW - against ``ControlNetRef.forward`` at scale 0.5.  The image-token buffer
    is filled with noise: the ControlNet's cross-attention is text-only.  Measured on MI355X (printed with -s): features 6.381e-4, 7.855e-4, 8.472e-4,
    1.004e-3, 1.198e-3 (mid); residuals 6.848e-4 .. 1.219e-3."""
    _, cn_ref, _, cn = tiny_models
    cond, _, noise = loop_inputs
    img = images[0]
    d_text, d_ip = cond[0].reshape(-1, 768).half().cuda().contiguous(), (7 * cond[1]).reshape(-1, 768).half().cuda().contiguous()
    eng = _control_engine(cn, dict(latents_in=noise.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=torch.tensor([500.0]).cuda()), img)
    assert eng.segment == "control" and "pv_conv_out" not in _names(eng) and len(eng.control_skips) == 4
    eng.run()
    torch.cuda.synchronize()
    skips, mid = cn_ref.features(noise, 500, cond[0], img)
    for k, (got, exp) in enumerate(zip(eng.control_skips + [eng.control_mid], list(skips) + [mid])):
        err = rel_l2(planes_of(got.float().cpu(), B, exp.shape[2], exp.shape[3]), exp)
        print(f"control feature {k} {tuple(exp.shape)}: rel-L2 vs ControlNetRef = {err:.3e}")
        assert err <= TOL_FWD
    down, mid_res = cn(noise.cuda(), 500, encoder_hidden_states=cond[0].cuda(), controlnet_cond=img.cuda(), conditioning_scale=0.5)
    exp_down, exp_mid = cn_ref(noise, 500, encoder_hidden_states=cond[0], controlnet_cond=img, conditioning_scale=0.5)
    assert all(d.dtype == torch.float32 and d.shape == e.shape for d, e in zip(down + [mid_res], exp_down + [exp_mid]))
    for k, (got, exp) in enumerate(zip(down + [mid_res], exp_down + [exp_mid])):
        err = rel_l2(got.cpu(), exp)
        print(f"residual {k}: rel-L2 vs ControlNetRef.forward = {err:.3e}")
        assert err <= TOL_FWD
    # one timestep per sample: the sample at t = 500 is what it was, the other one moves; any other count is refused
    down2, _ = cn(noise.cuda(), torch.tensor([500, 200]), encoder_hidden_states=cond[0].cuda(), controlnet_cond=img.cuda(), conditioning_scale=0.5)
    assert rel_l2(down2[3][0].cpu(), exp_down[3][0]) <= TOL_FWD and rel_l2(down2[3][1].cpu(), exp_down[3][1]) > 10 * TOL_FWD
    with pytest.raises(ValueError, match="timestep"):
        cn(noise.cuda(), torch.tensor([500, 200, 100]), encoder_hidden_states=cond[0].cuda(), controlnet_cond=img.cuda())


@torch.no_grad()
def test_controlled_forward_matches_the_controlled_oracle(tiny_models, loop_inputs, images):
    """``UNetEngine(control=..., control_scale=s)`` at B = 2, 16 x 16, t = 500 against ``controlled_oracle`` at s = 1.0 and 0.5: rel-L2 <= TOL_FWD, and more
    than 10 x TOL_FWD from the plain oracle.  The launch list grows by one ``pv_gemm_conv`` per skip pop and one behind the mid block (4 + 1) and is
    otherwise the plain plan's; a ``control=None`` engine built afterwards has the launch list and the bits of one built before.
    Measured on MI355X (printed with -s): rel-L2 vs ``controlled_oracle`` 1.244e-3 (scale 1) and 1.292e-3 (scale 0.5), vs the plain oracle 8.3e-1 and
    5.4e-1; 109 launches against the plain plan's 104."""
    ref, cn_ref, hip, cn = tiny_models
    cond, _, noise = loop_inputs
    img = images[0]
    d_text, d_ip = cond[0].reshape(-1, 768).half().cuda().contiguous(), cond[1].reshape(-1, 768).half().cuda().contiguous()
    common = dict(latents_in=noise.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=torch.tensor([500.0]).cuda())
    before = hip.engine(B, S, S, P, 1, **common)
    got_before = before.run().clone().float().cpu()
    plain = ref(noise, 500, encoder_hidden_states=cond).sample
    ctrl = _control_engine(cn, common, img)
    ctrl.run()
    for s in (1.0, 0.5):
        eng = hip.engine(B, S, S, P, 1, control=ctrl, control_scale=s, **common)
        got = eng.run().clone().float().cpu()
        torch.cuda.synchronize()
        exp = controlled_oracle(ref, cn_ref, noise, 500, cond, img, s).sample
        err, away = rel_l2(got, exp), rel_l2(got, plain)
        print(f"controlled forward, scale {s}: rel-L2 vs controlled_oracle = {err:.3e}, vs the plain oracle = {away:.3e}, launches {len(eng.rec)} (plain {len(before.rec)})")
        assert torch.isfinite(got).all() and err <= TOL_FWD and away > 10 * TOL_FWD
        assert len(eng.rec) == len(before.rec) + 5 and _names(eng).count("pv_gemm_conv") == _names(before).count("pv_gemm_conv") + 5
    assert rel_l2(got_before, plain) <= TOL_FWD
    after = hip.engine(B, S, S, P, 1, **common)
    assert after.control is None and _names(after) == _names(before) and [t[0] for t in after.rec.tags] == [t[0] for t in before.rec.tags]
    assert torch.equal(after.run().float().cpu(), got_before)
    with pytest.raises(ValueError, match="control"):
        hip.engine(B, S, S, P, 1, control=before, **common)


# ---------------------------------------------------------------------------------------------------------------- the loop
def _run(loop, cond, uncond, noise, img=None):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    if img is not None:
        loop.set_control(img.cuda())
    loop.reset(noise)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == loop.T
    return out


def _plan(loop):
    return [[fn.__name__ for fn, _ in e.rec.calls] for e in loop.all_engines], [fn.__name__ for fn, _ in loop.tail.calls], loop.launches_per_step


@torch.no_grad()
def test_loop_matches_the_controlled_oracle_loop_and_the_default_loop_is_untouched(tiny_models, loop_inputs, images):
    """4 steps at B = 2, 16 x 16, guidance 5 under the ControlNet at scale 1 against ``oracle_loop`` on ``ControlledRef``: rel-L2 <= TOL_LOOP (the oracle
    loops with and without control are 3.4e-1 apart, two control images 1.4e-1: test_controlnet_cpu).  Eager launches == graph replay == the graph
    with side streams, bit for bit; ``two_streams=False`` concatenates the lanes.  A second ``set_control`` with another image changes the result - within
    TOL_LOOP of that image's oracle loop - on the SAME captured graph, and the first image again gives the first bits.  ``controlnet=None`` and
    scale 0 build the default loop - launch names per engine, tail, ``launches_per_step``, schedule shape, bits - before and after.
    Measured on MI355X (printed with -s): rel-L2 vs the controlled oracle loop 8.492e-4, vs the loop without control 3.445e-1; the second image 8.805e-4
    vs its oracle loop, 1.383e-1 from the first image's result; 328 launches per step against the plain loop's 210."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, cn_ref, hip, cn = tiny_models
    cond, uncond, noise = loop_inputs
    img, img2 = images
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert before.controlnet is None and before.engines_ctrl_u == [] == before.engines_ctrl_c
    out_before = _run(before, cond, uncond, noise)
    exp = oracle_loop(ControlledRef(ref, cn_ref, img, 1.0), None, cond, uncond, noise, G_TEXT)
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, use_graph=use_graph, two_streams=two, controlnet=cn)
        assert loop.controlnet is cn and not loop.merge_lowres and len(loop.engines_ctrl_u) == len(loop.engines_ctrl_c) == 1
        assert all(e.control is loop.engines_ctrl_u[0] for e in loop.engines_u) and all(e.control is loop.engines_ctrl_c[0] for e in loop.engines_c)
        assert loop.launches_per_step == sum(len(e.rec) for e in loop.all_engines) + len(loop.tail) and _plan(loop)[1] == _plan(before)[1]
        # the control plans' group stands in front of the forwards' group: (ctrl_u | ctrl_c), (u | c), (tail)
        shape = [[len(lane) for lane in grp] for grp in loop.schedule]
        assert shape == ([[1, 1], [1, 1], [1]] if two else [[2], [2], [1]])
        assert loop.schedule[0][0][0] is loop.engines_ctrl_u[0].rec and loop.schedule[0][-1][-1] is loop.engines_ctrl_c[0].rec
        outs.append(_run(loop, cond, uncond, noise, img))
    err, away = rel_l2(outs[2], exp), rel_l2(outs[2], out_before)
    print(f"controlled loop, guidance {G_TEXT}, {STEPS} steps: rel-L2 vs the controlled oracle loop = {err:.3e}, vs the loop without control = {away:.3e}; "
          f"launches per step {loop.launches_per_step} (plain {before.launches_per_step})")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert err <= TOL_LOOP and away > 10 * TOL_LOOP
    graph = loop.graph
    assert graph is not None
    out2 = _run(loop, cond, uncond, noise, img2)
    err2 = rel_l2(out2, oracle_loop(ControlledRef(ref, cn_ref, img2, 1.0), None, cond, uncond, noise, G_TEXT))
    print(f"second control image on the captured graph: rel-L2 vs its oracle loop = {err2:.3e}, vs the first image's result = {rel_l2(out2, outs[2]):.3e}")
    assert loop.graph is graph and err2 <= TOL_LOOP and rel_l2(out2, outs[2]) > 10 * TOL_LOOP
    assert torch.equal(_run(loop, cond, uncond, noise, img), outs[0])
    one = _run(loop, cond, uncond, noise, img[:1])                    # a single image is broadcast over the batch
    assert torch.equal(one[0], outs[0][0]) and not torch.equal(one[1], outs[0][1])
    for kw in (dict(), dict(controlnet=None), dict(controlnet=cn, conditioning_scale=0), dict(controlnet=None, conditioning_scale=0.5)):
        after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw)
        assert after.controlnet is None and _plan(after) == _plan(before) and after.merge_lowres == before.merge_lowres
        assert [[len(lane) for lane in grp] for grp in after.schedule] == [[len(lane) for lane in grp] for grp in before.schedule]
        assert torch.equal(_run(after, cond, uncond, noise), out_before)
        with pytest.raises(RuntimeError, match="set_control"):
            after.set_control(img.cuda())
    with pytest.raises(ValueError, match="controlnet.*training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, controlnet=cn)
    with pytest.raises(ValueError, match="conditioning_scale"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, conditioning_scale=float("nan"))
    for bad in (img[:, :2], img[:, :, :64], torch.cat([img, img])):
        with pytest.raises(ValueError, match="control_image"):
            loop.set_control(bad.cuda())


@torch.no_grad()
def test_loop_at_half_scale(tiny_models, loop_inputs, images):
    """The loop at ``conditioning_scale=0.5`` against the oracle loop at that scale: rel-L2 <= TOL_LOOP (scales 1 and 0.5 are 1.7e-1 apart on the oracle).
    Measured on MI355X (printed with -s): 9.212e-4."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, cn_ref, hip, cn = tiny_models
    cond, uncond, noise = loop_inputs
    out = _run(DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, conditioning_scale=0.5), cond, uncond, noise, images[0])
    err = rel_l2(out, oracle_loop(ControlledRef(ref, cn_ref, images[0], 0.5), None, cond, uncond, noise, G_TEXT))
    print(f"controlled loop at scale 0.5: rel-L2 vs the oracle loop = {err:.3e}")
    assert err <= TOL_LOOP


@torch.no_grad()
@pytest.mark.parametrize("layer", (("mid_block.attentions.0",), ("up_blocks.1.attentions.0",)), ids=("mid", "up10"))
def test_pag_on_a_shared_trunk_under_control(tiny_models, loop_inputs, images, layer):
    """PAG with a ControlNet.  On the mid block the perturbed plan adopts the conditional plan's raw down path, records the mid block and adds the mid
    residual and every skip's residual itself (5 control GEMMs); on ``up_blocks.1.attentions.0`` the trunk starts after three pops: the adopted ``x``
    carries the conditional plan's control, one skip is left to pop (1 control GEMM).  The perturbed plan reads the CONDITIONAL control features: no
    further ControlNet run.  ``share_trunk=True`` == ``share_trunk=False`` bit for bit, within TOL_LOOP of the oracle loop whose perturbed model is
    ``ControlledRef(perturbed_oracle(...))``.  Measured on MI355X (printed with -s): rel-L2 1.018e-3 (mid block; launches per step 435 -> 404 with the
    trunk) and 9.872e-4 (up_blocks.1.attentions.0; 436 -> 360)."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, cn_ref, hip, cn = tiny_models
    cond, uncond, noise = loop_inputs
    img = images[0]
    exp = oracle_loop(ControlledRef(ref, cn_ref, img), ControlledRef(perturbed_oracle(ref, layer), cn_ref, img), cond, uncond, noise, G_TEXT, g_pag=G_PAG)
    kw = dict(pag_scale=G_PAG, pag_layers=layer, controlnet=cn)
    full = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_trunk=False, **kw)
    trunk = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw)
    assert trunk.share_trunk and len(trunk.engines_ctrl_c) == 1 and trunk.engines_p_attn[0].control is trunk.engines_ctrl_c[0]
    plain_trunk = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=layer)
    added = len(trunk.engines_p_attn[0].rec) - len(plain_trunk.engines_p_attn[0].rec)
    assert added == (5 if layer[0].startswith("mid") else 1)
    out_full, out_trunk = _run(full, cond, uncond, noise, img), _run(trunk, cond, uncond, noise, img)
    err = rel_l2(out_trunk, exp)
    print(f"control + PAG on {layer[0]}: rel-L2 vs the oracle loop = {err:.3e}; launches per step {full.launches_per_step} -> {trunk.launches_per_step}")
    assert torch.equal(out_trunk, out_full) and err <= TOL_LOOP


@torch.no_grad()
def test_freeu_shared_prefix_and_image_guidance_under_control(tiny_models, loop_inputs, images):
    """FreeU: the control is added to the popped skip BEFORE the Fourier filter (against ``ControlledRef(freeu_oracle(...))``).  ``share_prefix=True``: the
    bits of the loop without it.  ``image_guidance_scale``: the third forward (uncond text, cond image tokens) reuses the UNCOND control features - two
    control plans, three forwards - against the oracle loop whose ControlNet sees the text of each forward.  Each within TOL_LOOP.
    Measured on MI355X (printed with -s): rel-L2 9.439e-4 (FreeU) and 8.129e-4 (image_guidance_scale 2)."""
    from test_freeu_cpu import FREEU, freeu_oracle
    from photoverse_amd.pipeline import DenoiseLoop
    ref, cn_ref, hip, cn = tiny_models
    cond, uncond, noise = loop_inputs
    img = images[0]
    out = _run(DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, freeu=FREEU), cond, uncond, noise, img)
    err = rel_l2(out, oracle_loop(ControlledRef(freeu_oracle(ref, *FREEU), cn_ref, img), None, cond, uncond, noise, G_TEXT))
    print(f"control + FreeU: rel-L2 vs the oracle loop = {err:.3e}")
    assert err <= TOL_LOOP
    plain = _run(DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn), cond, uncond, noise, img)
    shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, share_prefix=True)
    assert shared.share_prefix and len(shared.engines_p) == 1 and [[len(lane) for lane in grp] for grp in shared.schedule] == [[1], [1, 1], [1, 1], [1]]
    assert torch.equal(_run(shared, cond, uncond, noise, img), plain)
    three = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, image_guidance_scale=2.0)
    assert len(three.engines_i) == 1 and three.engines_i[0].control is three.engines_ctrl_u[0] and len(three.engines_ctrl_u + three.engines_ctrl_c) == 2
    out3 = _run(three, cond, uncond, noise, img)
    err3 = rel_l2(out3, oracle_loop(ControlledRef(ref, cn_ref, img), None, cond, uncond, noise, G_TEXT, g_image=2.0))
    print(f"control + image_guidance_scale 2: rel-L2 vs the oracle loop = {err3:.3e}")
    assert err3 <= TOL_LOOP and not torch.equal(out3, plain)


# ---------------------------------------------------------------------------------------------------------------- full-size widths
@torch.no_grad()
def test_control_features_at_full_size_widths(full_weights):
    """The SD-1.5-sized ControlNet (the session's seeded UNet encoder weights, ``nonzero_init_`` on top) at B = 1, 64 x 64 latents, t = 481: the 12 + 1
    control features of the HIP plan against ``ControlNetRef`` run live on the CPU, each rel-L2 <= TOL_FWD.
    Measured on MI355X (printed with -s): 7.137e-4 at conv_in rising to 1.856e-3 at the last skip and 2.015e-3 at the mid block's output."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle import fullsize as fs
    from photoverse_amd.controlnet import ControlNetModel, hint_plan
    from photoverse_amd.ops import Recorder
    with fs.no_init():
        cn_ref = ControlNetRef().eval()
        cn = ControlNetModel()
    own = cn_ref.state_dict()
    cn_ref.load_state_dict({k: v for k, v in full_weights("unet").items() if k in own and "processor" not in k}, strict=False)
    torch.manual_seed(21)
    emb = cn_ref.controlnet_cond_embedding
    for m in [emb.conv_in, *emb.blocks, emb.conv_out, *cn_ref.controlnet_down_blocks, cn_ref.controlnet_mid_block]:
        m.reset_parameters()                       # (constructed under no_init: the default init now, then the seeded one on top)
        if m.kernel_size == (1, 1):
            torch.nn.init.zeros_(m.bias)
    nonzero_init_(cn_ref)
    cn.load_state_dict(cn_ref.state_dict(), strict=True)
    cn.to("cuda")
    case = fs.forward_case()
    img = control_image(batch=1, size=512, seed=9)
    hint = torch.zeros((64 * 64, 320), dtype=torch.float16, device="cuda")
    rec = Recorder("cuda")
    hint_plan(rec, cn.controlnet_cond_embedding, img.cuda().contiguous(), hint)
    rec.run()
    eng = cn.control_engine(1, 64, 64, 1, hint, latents_in=case["x"].cuda().contiguous(), text=case["text"].reshape(-1, 768).half().cuda().contiguous(),
                            ip=case["ip"].reshape(-1, 768).half().cuda().contiguous(), timesteps=torch.tensor([float(case["t"])]).cuda())
    eng.run()
    torch.cuda.synchronize()
    skips, mid = cn_ref.features(case["x"], case["t"], case["text"], img)
    assert len(eng.control_skips) == len(skips) == 12
    worst = 0.0
    for k, (got, exp) in enumerate(zip(eng.control_skips + [eng.control_mid], list(skips) + [mid])):
        err = rel_l2(planes_of(got.float().cpu(), 1, exp.shape[2], exp.shape[3]), exp)
        worst = max(worst, err)
        print(f"full-size control feature {k} {tuple(exp.shape)}: rel-L2 vs ControlNetRef = {err:.3e}")
        assert err <= TOL_FWD
    print(f"full-size control features: worst rel-L2 = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 128, 128, 128), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_controlnet_end_to_end(tmp_path):
    """``run_inference(controlnet=..., control_image=...)`` on the tiny models: shapes, finiteness, determinism, the cached loop and its graph reused, the
    control image and the scale change the result, scale 0 runs on the plain cached loop with the plain bits, new ControlNet weights (``repack``) build
    a new loop, it combines with ``inpaint_mask`` (the kept region is the photograph's bits), ``sampler``, ``pag_scale`` and ``freeu``, a sharded call
    (one-rank gloo group) with a batch-sized ``control_image`` gives the unsharded bits, and a plain call before and after gives identical bits."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import torch.distributed as dist
    from oracle.unet_ref import TINY_CONFIG
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.infer import run_inference
    from photoverse_amd.modeling_utils import load_models
    from photoverse_amd.pipeline import PhotoVersePipeline
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
    cn = ControlNetModel.from_unet(unet).randomize_zero_convs_(seed=4)
    nonzero_init_(cn)
    cn.repack()
    assert cn.device.type == "cuda"
    g = torch.Generator().manual_seed(4)
    ex = {"pixel_values": torch.rand(2, 3, 128, 128, generator=g) * 2 - 1, "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4, seed=1)
    img, img2 = control_image(), control_image(seed=6)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, None, sch, "cuda", [1], **kw)
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(iter(cache.values()))
    a = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, **kw)
    assert a.shape == (2, 4, 16, 16) and torch.isfinite(a).all() and not torch.equal(a, before)
    loop = next(reversed(cache.values()))
    graph = loop.graph
    assert loop is not plain_loop and loop.controlnet is cn and graph is not None
    b = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img2, **kw)
    assert next(reversed(cache.values())) is loop and loop.graph is graph and torch.isfinite(b).all() and not torch.equal(a, b)
    assert torch.equal(run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, **kw), a)
    half = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, controlnet_conditioning_scale=0.5, **kw)
    assert not torch.equal(half, a) and not torch.equal(half, before) and next(reversed(cache.values())) is not loop
    off = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, controlnet_conditioning_scale=0.0, **kw)
    assert torch.equal(off, before)
    with pytest.raises(ValueError, match="control_image"):
        run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=torch.cat([img, img[:1]]), **kw)
    # new weights: the cache key carries the ControlNet's pack version
    a_again = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, **kw)
    loop_a = next(reversed(cache.values()))
    cn.randomize_zero_convs_(seed=9)
    c = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, **kw)
    assert torch.equal(a_again, a) and next(reversed(cache.values())) is not loop_a and not torch.equal(c, a)
    # combinations
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 32:96, 16:80] = 1
    pix = run_inference(*args, hip_vae, sch, "cuda", [1], controlnet=cn, control_image=img, inpaint_mask=mask, strength=0.75, **kw)
    assert pix.shape == (2, 3, 128, 128) and torch.isfinite(pix).all()
    keep = (mask == 0).expand(2, 3, 128, 128)
    assert torch.equal(pix.cpu()[keep], ex["pixel_values"].clamp(-1, 1)[keep])
    combo = run_inference(*args, None, sch, "cuda", [1], controlnet=cn, control_image=img, sampler="sde-dpmsolver++", pag_scale=2.0, freeu=(1.5, 1.6, 0.9, 0.2),
                          image_guidance_scale=2.0, guidance_rescale=0.5, **kw)
    assert combo.shape == (2, 4, 16, 16) and torch.isfinite(combo).all()
    # sharded: a batch-sized control image goes with its samples
    pipe = PhotoVersePipeline(tok, te, None, unet, ie, ia, ta, sch)
    pipe.device = torch.device("cuda")
    whole = pipe(ex, image_encoder_layers_idx=[1], controlnet=cn, control_image=img, **kw)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        sharded = pipe(ex, image_encoder_layers_idx=[1], shard=True, controlnet=cn, control_image=img, **kw)
    finally:
        dist.destroy_process_group()
    assert torch.equal(sharded.cpu(), whole.cpu()) and torch.equal(whole, c)
    after = run_inference(*args, None, sch, "cuda", [1], **kw)
    assert torch.equal(before, after)


def test_generate_cli_runs_with_a_random_controlnet(tmp_path):
    """generate.py --controlnet_path random runs as a program (a ControlNet copied from the tiny UNet, seeded non-zero zero convs, a synthetic control
    image) and writes its PNGs."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--controlnet_path", "random", "--controlnet_conditioning_scale", "0.8", "--num_timesteps", "4", "--num_of_samples", "2",
           "--seed", "3", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
