"""GPU tests of FreeU: ``pv_freeu_rows`` against the fp64 ``fourier_filter_ref`` of ``tests/test_freeu_cpu.py`` on the same fp16 inputs and its backbone
half against ``x * b`` in fp64; the engine's forward (``UNetEngine(freeu=...)``) against ``freeu_oracle``; the ``DenoiseLoop`` with ``freeu`` against the
oracle loop on that model - graph == eager, with PAG's shared trunk starting inside the FreeU blocks, with the shared prefix, and in the merged
low-resolution plan at full-size widths; ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch

from test_freeu_cpu import FREEU, SETTINGS, fourier_filter_ref, freeu_oracle
from test_pag_cpu import B, G_PAG, G_TEXT, P, S, STEPS, TOL_FWD, TOL_LOOP, loop_inputs_81, oracle_loop, perturbed_oracle, rel_l2, tiny_oracle

pytestmark = pytest.mark.gpu

#: (batch, C, h, w) of the skip half: H = 2 (Nyquist), odd sizes, C below / not a multiple of / above the 128-channel group of a workgroup, planes from 4 to
#: 576 pixels (fewer pixels than pixel lanes, a ragged last round, many rounds), the widths and sizes of the UNet's first two up blocks
SKIP_SHAPES = ((1, 8, 2, 2), (2, 24, 5, 7), (3, 328, 3, 2), (2, 64, 2, 9), (2, 320, 8, 8), (1, 640, 12, 12), (1, 1280, 16, 16), (2, 40, 24, 24))
SCALES = (0.9, 0.2, 2.0)
UP11, UP10 = ("up_blocks.1.attentions.1",), ("up_blocks.1.attentions.0",)
CONST = 3.25


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd import _lib
    return _lib.load()


def launch(lib, x, xo, b, sk, so, s, batch, h, w):
    """One ``pv_freeu_rows`` launch on 2-D fp16 row views (None = the half is absent)."""
    ptr = lambda t: None if t is None else t.data_ptr()
    ld = lambda t: 0 if t is None else t.stride(0)
    rc = lib.pv_freeu_rows(ptr(x), ld(x), 0 if x is None else x.shape[1], ptr(xo), ld(xo), float(b), ptr(sk), ld(sk), 0 if sk is None else sk.shape[1],
                           ptr(so), ld(so), float(s), batch, h, w, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def rows_of(t):
    """(B, C, H, W) -> rows [B*H*W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def planes_of(r, batch, h, w):
    return r.reshape(batch, h, w, -1).permute(0, 3, 1, 2)


def skip_input(shape, seed):
    """fp16 (B, C, H, W): 2 randn + a per-channel offset (the DC term matters); channel 0 constant, channel 1 zero."""
    g = torch.Generator().manual_seed(seed)
    n, C, H, W = shape
    x = 2 * torch.randn(shape, generator=g) + 3 * torch.randn(1, C, 1, 1, generator=g)
    x[:, 0] = CONST
    x[:, 1] = 0
    return x.half()


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", SKIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_skip_half_against_the_fp64_fourier_filter(lib, shape):
    """``|got - ref| <= 2^-10 |ref| + 2^-12 max|x| (1 + |s - 1|)`` for s in {0.9, 0.2, 2.0}: the first term is twice the round-to-nearest error of the one
    fp16 store, the second bounds the fp32 accumulation over at most 576 pixels.  The constant channel comes out as s * c (inside the bound), the zero
    channel as exact zeros, the input is unchanged.  (2, 24, 5, 7) also runs as a column slice of wider buffers (lds = 40, ldso = 48) between guard
    rows: gap columns and guards keep their bits, the result has the bits of the dense launch.
    Measured on MI355X (printed with -s), worst |got - ref| / bound over the three scales, in the order of SKIP_SHAPES: 0.263, 0.351, 0.342, 0.336,
    0.325, 0.326, 0.334, 0.330 - the fp16 store's rounding (max |got - ref| 3.9e-3 at s = 0.9, 7.8e-3 at s = 2: half an ulp of the largest values),
    the same at 4 and at 576 pixels: the accumulation term is not what is used up."""
    n, C, H, W = shape
    x = skip_input(shape, 100 + sum(shape))
    rows = rows_of(x)
    d_in = rows.cuda()
    worst = 0.0
    for s in SCALES:
        d_out = torch.full_like(d_in, float("nan"))
        launch(lib, None, None, 1.0, d_in, d_out, s, n, H, W)
        torch.cuda.synchronize()
        got = planes_of(d_out.cpu(), n, H, W).double()
        ref = fourier_filter_ref(x.double(), 1, s)
        bound = 2.0 ** -10 * ref.abs() + 2.0 ** -12 * x.double().abs().max() * (1 + abs(s - 1))
        ratio = ((got - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        print(f"freeu skip {shape} s = {s}: max |got - ref| = {(got - ref).abs().max().item():.3e}, worst |got - ref| / bound = {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1.0
        assert torch.equal(got[:, 1], torch.zeros_like(got[:, 1]))
        assert ((got[:, 0] - s * CONST).abs() <= bound[:, 0]).all()
        assert torch.equal(d_in.cpu(), rows)
        if shape == (2, 24, 5, 7):
            r = rows.shape[0]
            wide_in = torch.randn(r, 40).half().cuda()
            wide_in[:, 8:32] = d_in
            wide_out = torch.randn(r + 4, 48).half().cuda()
            before = wide_out.clone()
            launch(lib, None, None, 1.0, wide_in[:, 8:32], wide_out[2:2 + r, 16:40], s, n, H, W)
            torch.cuda.synchronize()
            assert torch.equal(wide_out[2:2 + r, 16:40], d_out)
            keep = torch.ones_like(wide_out, dtype=torch.bool)
            keep[2:2 + r, 16:40] = False
            assert torch.equal(wide_out.view(torch.int16)[keep], before.view(torch.int16)[keep])
    print(f"freeu skip {shape}: worst |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("cx", (16, 48, 640, 1280))
def test_backbone_half_and_both_halves_in_one_launch(lib, cx):
    """``x_out = fp16(float(x) * (c < cx/2 ? b : 1))`` for b in {1.5, 0.5}: the upper half is the input bit for bit, the lower half within one fp16 ulp of
    ``x * b`` in fp64 (the fp32 product of an fp16 value and these b is exact, so it is the correctly rounded value).  Both halves in one launch give
    the bits of the two halves launched separately; the inputs are unchanged.  Measured on MI355X: max |got - x b| = 0.500 ulp for every cx and b."""
    n, H, W, cs = 2, 3, 5, 136
    g = torch.Generator().manual_seed(cx)
    x = (2 * torch.randn(n * H * W, cx, generator=g)).half()
    x[0, :4] = torch.tensor([0.0, -0.0, 6.1e-5, 2.0e-7]).half()          # zeros, the smallest normal's neighbourhood, a subnormal
    sk = rows_of(skip_input((n, cs, H, W), cx + 1))
    d_x, d_sk = x.cuda(), sk.cuda()
    for b in (1.5, 0.5):
        xo = torch.full_like(d_x, float("nan"))
        launch(lib, d_x, xo, b, None, None, 1.0, n, H, W)
        so = torch.full_like(d_sk, float("nan"))
        launch(lib, None, None, 1.0, d_sk, so, 0.2, n, H, W)
        xo2, so2 = torch.full_like(d_x, float("nan")), torch.full_like(d_sk, float("nan"))
        launch(lib, d_x, xo2, b, d_sk, so2, 0.2, n, H, W)
        torch.cuda.synchronize()
        got = xo.cpu()
        assert torch.equal(got[:, cx // 2:].view(torch.int16), x[:, cx // 2:].view(torch.int16))
        exact = x[:, :cx // 2].double() * b
        _, e = torch.frexp(exact)
        ulp = torch.maximum(torch.ldexp(torch.ones_like(exact), e - 11), torch.full_like(exact, 2.0 ** -24))
        d = (got[:, :cx // 2].double() - exact).abs()
        print(f"freeu backbone cx = {cx} b = {b}: max |got - x b| / ulp = {(d / ulp).max().item():.3f}")
        assert (d <= ulp).all()
        assert torch.equal(xo2.view(torch.int16), xo.view(torch.int16)) and torch.equal(so2.view(torch.int16), so.view(torch.int16))
        assert torch.equal(d_x.cpu().view(torch.int16), x.view(torch.int16)) and torch.equal(d_sk.cpu(), sk)


def test_recorder_freeu_skips_the_halves_at_scale_one():
    """``Recorder.freeu``: a half at scale 1 is the input object and is not launched; both at 1 record nothing; the outputs carry no column statistics."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    n, H, W = 2, 8, 8
    rec = Recorder("cuda")
    x = torch.randn(n * H * W, 64).half().cuda()
    sk = torch.randn(n * H * W, 32).half().cuda()
    a, c = rec.freeu(x, sk, batch=n, h=H, w=W, b=1, s=1.0)
    assert a is x and c is sk and len(rec) == 0
    a, c = rec.freeu(x, sk, batch=n, h=H, w=W, b=1.5, s=1)
    assert a is not x and c is sk and len(rec) == 1
    a2, c2 = rec.freeu(x, sk, batch=n, h=H, w=W, b=1, s=0.5)
    assert a2 is x and c2 is not sk and len(rec) == 2
    a3, c3 = rec.freeu(x, sk, batch=n, h=H, w=W, b=1.5, s=0.5)
    assert a3 is not x and c3 is not sk and len(rec) == 3 and [fn.__name__ for fn, _ in rec.calls] == ["pv_freeu_rows"] * 3
    rec.run()
    torch.cuda.synchronize()
    assert torch.equal(a3, a) and torch.equal(c3, c2) and torch.equal(a[:, 32:], x[:, 32:]) and not torch.equal(c2, sk)
    for t in (a, c2, a3, c3):
        assert (t.data_ptr(), t.shape[0], t.shape[1]) not in rec.colstats
    g = torch.ones(64 + 32, device="cuda")
    assert rec.groupnorm_table(a3, g, g, batch=n, hw=H * W, x1=c3) is None


# ---------------------------------------------------------------------------------------------------------------- the forward
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


def _names(eng):
    return [fn.__name__ for fn, _ in eng.rec.calls]


@torch.no_grad()
def test_forward_matches_the_freeu_oracle(tiny_pair, loop_inputs):
    """``UNetEngine(freeu=f)`` at B = 2, 16 x 16, t = 500 against ``freeu_oracle``: rel-L2 below TOL_FWD for the authors' setting and for each of the four
    numbers on its own - and each result more than 10 x TOL_FWD from the plain oracle, so an engine that ignored any one number could not pass.  The
    launch list grows by one ``pv_freeu_rows`` per ResnetBlock of an up block whose ``b`` or ``s`` is not 1 (both halves share the launch; the GroupNorm
    behind it trades its statistics-from-the-epilogue launch for a statistics pass, one for one).  A ``freeu=None`` engine built afterwards has the launch
    list and the bits of one built before.  Measured on MI355X (printed with -s), rel-L2 against ``freeu_oracle`` / the plain oracle, in the order of
    SETTINGS: 1.380e-3 / 3.266e-1, 1.280e-3 / 1.508e-1, 1.302e-3 / 2.102e-1, 1.237e-3 / 9.122e-2, 1.300e-3 / 1.796e-1; 108, 106, 106, 106, 106 launches
    against the plain plan's 104."""
    ref, hip = tiny_pair
    cond, _, noise = loop_inputs
    d_text, d_ip = cond[0].reshape(-1, 768).half().cuda().contiguous(), cond[1].reshape(-1, 768).half().cuda().contiguous()
    common = dict(latents_in=noise.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=torch.tensor([500.0]).cuda())
    before = hip.engine(B, S, S, P, 1, **common)
    assert before.freeu is None and "pv_freeu_rows" not in _names(before)
    plain_oracle = ref(noise, 500, encoder_hidden_states=cond).sample
    got_before = before.run().clone().float().cpu()
    for f in SETTINGS:
        eng = hip.engine(B, S, S, P, 1, freeu=f, **common)
        got = eng.run().clone().float().cpu()
        torch.cuda.synchronize()
        exp = freeu_oracle(ref, *f)(noise, 500, encoder_hidden_states=cond).sample
        err, away = rel_l2(got, exp), rel_l2(got, plain_oracle)
        added = sum(len(hip.up_blocks[bi].resnets) for bi in (0, 1) if f[bi] != 1 or f[2 + bi] != 1)
        print(f"freeu forward {f}: rel-L2 vs freeu_oracle = {err:.3e}, vs the plain oracle = {away:.3e}, launches {len(eng.rec)} (plain {len(before.rec)})")
        assert torch.isfinite(got).all() and err < TOL_FWD
        assert away > 10 * TOL_FWD
        assert len(eng.rec) == len(before.rec) + added and _names(eng).count("pv_freeu_rows") == added
        assert [nm for nm in _names(eng) if nm != "pv_freeu_rows" and not nm.startswith("pv_groupnorm_stats")] == \
               [nm for nm in _names(before) if not nm.startswith("pv_groupnorm_stats")]
    assert rel_l2(got_before, plain_oracle) < TOL_FWD
    for off in (None, (1, 1, 1, 1)):
        after = hip.engine(B, S, S, P, 1, freeu=off, **common)
        assert after.freeu is None and _names(after) == _names(before) and [t[0] for t in after.rec.tags] == [t[0] for t in before.rec.tags]
        assert torch.equal(after.run().float().cpu(), got_before)
    with pytest.raises(ValueError, match="freeu"):
        hip.engine(B, S, S, P, 1, freeu=(1.5, 1.6, 0.9), **common)


# ---------------------------------------------------------------------------------------------------------------- the loop
def _run(loop, cond, uncond, noise):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    loop.reset(noise)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == loop.T
    return out


def _plan(loop):
    return [[fn.__name__ for fn, _ in e.rec.calls] for e in loop.all_engines], [fn.__name__ for fn, _ in loop.tail.calls], loop.launches_per_step


@torch.no_grad()
def test_loop_matches_the_oracle_loop_and_the_default_loop_is_untouched(tiny_pair, loop_inputs):
    """4 steps at B = 2, 16 x 16, guidance 5, FreeU (1.5, 1.6, 0.9, 0.2) against ``oracle_loop`` on ``freeu_oracle`` (both forwards): rel-L2 below TOL_LOOP
    (the oracle loops with and without FreeU are 0.187 apart).  Eager launches == graph replay == the graph with side streams, bit for bit;
    ``share_prefix=True`` has the bits of the loop without it; every engine of the step carries the setting.  ``freeu=None`` and ``(1, 1, 1, 1)`` build
    the default loop - launch names per engine, tail, ``launches_per_step``, bits - on loops built before and after the FreeU loops.
    Measured on MI355X (printed with -s): rel-L2 against the oracle loop 1.016e-3, against the loop without FreeU 1.873e-1."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert before.freeu is None and not any("pv_freeu_rows" in names for names in _plan(before)[0])
    out_before = _run(before, cond, uncond, noise)
    exp = oracle_loop(freeu_oracle(ref, *FREEU), None, cond, uncond, noise, G_TEXT)
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, use_graph=use_graph, two_streams=two, freeu=FREEU)
        assert loop.freeu == FREEU and all(e.freeu == FREEU for e in loop.all_engines)
        assert _plan(loop)[1] == _plan(before)[1] and loop.launches_per_step == before.launches_per_step + 2 * 4
        outs.append(_run(loop, cond, uncond, noise))
    err, away = rel_l2(outs[2], exp), rel_l2(outs[2], out_before)
    print(f"freeu loop {FREEU}, guidance {G_TEXT}, {STEPS} steps: rel-L2 vs the fp32 oracle loop = {err:.3e}, vs the loop without FreeU = {away:.3e}")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert err < TOL_LOOP and away > 10 * TOL_LOOP
    shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_prefix=True, freeu=FREEU)
    assert shared.share_prefix and len(shared.engines_p) == 1 and all(e.freeu == FREEU for e in shared.all_engines)
    assert torch.equal(_run(shared, cond, uncond, noise), outs[0])
    assert torch.equal(_run(loop, cond, uncond, noise), outs[0])                  # a second generation on the captured graph
    for off in (None, (1, 1, 1, 1), dict(b1=1, b2=1, s1=1, s2=1)):
        after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, freeu=off)
        assert after.freeu is None and _plan(after) == _plan(before) and after.merge_lowres == before.merge_lowres
        assert torch.equal(_run(after, cond, uncond, noise), out_before)
    with pytest.raises(ValueError, match="freeu.*training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, freeu=FREEU)
    with pytest.raises(ValueError, match="freeu"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, freeu=(1.5, float("nan"), 0.9, 0.2))


@torch.no_grad()
@pytest.mark.parametrize("layer,behind", ((UP11, 0), (UP10, 1)), ids=("up11", "up10"))
def test_pag_trunk_that_starts_inside_the_freeu_blocks(tiny_pair, loop_inputs, layer, behind):
    """PAG with FreeU where the shared trunk starts inside the second FreeU block: on ``up_blocks.1.attentions.1`` the perturbed plan adopts an ``x`` that
    went through every FreeU launch of the conditional plan and records none; on ``up_blocks.1.attentions.0`` one ResnetBlock follows, whose skip the
    plan adopts RAW and filters itself (one launch).  ``share_trunk=True`` == ``share_trunk=False`` bit for bit, and the result is within TOL_LOOP of the
    oracle loop whose perturbed model is ``perturbed_oracle(freeu_oracle(...))``.  Measured on MI355X: rel-L2 1.098e-3 (attentions.1; launches per step 325 -> 233 with
    the trunk) and 1.127e-3 (attentions.0; 325 -> 250)."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    fo = freeu_oracle(ref, *FREEU)
    exp = oracle_loop(fo, perturbed_oracle(fo, layer), cond, uncond, noise, G_TEXT, g_pag=G_PAG)
    kw = dict(pag_scale=G_PAG, pag_layers=layer, freeu=FREEU)
    full = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_trunk=False, **kw)
    trunk = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw)
    assert trunk.share_trunk and not full.share_trunk and trunk.launches_per_step < full.launches_per_step
    names_full, names_trunk = _names(full.engines_p_attn[0]), _names(trunk.engines_p_attn[0])
    assert names_full.count("pv_freeu_rows") == 4 and names_trunk.count("pv_freeu_rows") == behind     # only the ResnetBlocks behind the adoption point
    out_full = _run(full, cond, uncond, noise)
    out_trunk = _run(trunk, cond, uncond, noise)
    err = rel_l2(out_trunk, exp)
    print(f"freeu + PAG on {layer[0]}: rel-L2 vs the oracle loop = {err:.3e}; launches per step {full.launches_per_step} -> {trunk.launches_per_step}")
    assert torch.equal(out_trunk, out_full)
    assert err < TOL_LOOP


@torch.no_grad()
def test_merged_lowres_plan_at_full_size_widths(full_hip_unet, monkeypatch):
    """B = 2, 64 x 64, 2 steps on the SD-1.5-sized UNet with split-K off: ``merge_lowres=True`` puts both FreeU blocks (C = 1280 at 8 x 8 and 16 x 16) into
    the ``mid`` segment at batch 2B and equals ``merge_lowres=False`` bit for bit - a plane's sums do not depend on the batch it sits in -, and the result
    differs from the same loop without FreeU (measured on MI355X: by rel-L2 1.07e-1)."""
    from photoverse_amd import ops
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    n, size, T = 2, 64, 2
    g = torch.Generator().manual_seed(78)
    cond = (torch.randn(n, 77, 768, generator=g), torch.randn(n, 1, 768, generator=g))
    uncond = (torch.randn(n, 77, 768, generator=g), torch.randn(n, 1, 768, generator=g))
    noise = torch.randn(n, 4, size, size, generator=g)
    monkeypatch.setattr(ops, "SPLITK_MAX", 1)

    def run(merge, freeu):
        loop = DenoiseLoop(hip, n, size, 1, T, 7.5, merge_lowres=merge, freeu=freeu)
        assert loop.merge_lowres == merge and len(loop.engines_m) == (1 if merge else 0)
        counts = [_names(e).count("pv_freeu_rows") for e in loop.all_engines]
        out = _run(loop, cond, uncond, noise)
        del loop
        return out, counts

    a, ca = run(True, FREEU)
    b, cb = run(False, FREEU)
    plain, cp = run(True, None)
    assert ca == [0, 0, 6] and cb == [6, 6] and cp == [0, 0, 0]          # merged: all six launches sit in the mid segment (batch 2B)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    print(f"merged low-resolution plan with FreeU {FREEU}: rel-L2 against the same loop without = {rel_l2(a, plain):.3e}")
    assert not torch.equal(a, plain)


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_freeu_end_to_end():
    """``run_inference(freeu=...)`` on the tiny models and the tiny x2 VAE: shapes, finiteness, determinism, the cached loop and its graph reused, the
    setting changes the result, ``(1, 1, 1, 1)`` runs on the plain cached loop with the plain bits, with ``inpaint_mask`` the kept region is the
    photograph's bits, with ``hires_latent_size`` both cached loops carry the setting, and a plain call before and after gives identical bits."""
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
    fu = dict(freeu=FREEU)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)          # a plain call, before ...
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(iter(cache.values()))
    # 1. latents: shape, finiteness, determinism, the cached loop and its graph reused
    a = run_inference(*args, None, sch, "cuda", [1], **kw, **fu)
    assert a.shape == (2, 4, 16, 16) and torch.isfinite(a).all()
    loop = next(reversed(cache.values()))
    assert loop is not plain_loop and loop.freeu == FREEU and all(e.freeu == FREEU for e in loop.all_engines)
    graph = loop.graph
    assert graph is not None
    a2 = run_inference(*args, None, sch, "cuda", [1], **kw, freeu=dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2))
    assert torch.equal(a, a2) and next(reversed(cache.values())) is loop and loop.graph is graph
    # 2. the setting changes the result; all ones is the plain call on the plain loop
    plain = run_inference(*args, None, sch, "cuda", [1], **kw)
    ones = run_inference(*args, None, sch, "cuda", [1], freeu=(1, 1, 1, 1), **kw)
    assert torch.equal(ones, plain) and next(reversed(cache.values())) is plain_loop
    other = run_inference(*args, None, sch, "cuda", [1], freeu=(1.2, 1.4, 0.9, 0.2), **kw)
    assert torch.isfinite(other).all() and not torch.equal(a, plain) and not torch.equal(other, a) and not torch.equal(other, plain)
    with pytest.raises(ValueError, match="freeu"):
        run_inference(*args, None, sch, "cuda", [1], freeu=(1.5, 1.6, 0.9), **kw)
    # 3. with inpaint_mask: images in [-1, 1], the kept region is the photograph's own bits
    mask = torch.zeros(1, 1, 32, 32)
    mask[..., 8:24, 4:20] = 1
    img = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw, **fu)
    assert img.shape == (2, 3, 32, 32) and torch.isfinite(img).all() and img.min() >= -1 and img.max() <= 1
    keep = (mask == 0).expand(2, 3, 32, 32)
    assert torch.equal(img.cpu()[keep], ex["pixel_values"].clamp(-1, 1)[keep])
    img_plain = run_inference(*args, hip_vae, sch, "cuda", [1], inpaint_mask=mask, **kw)
    assert not torch.equal(img, img_plain)
    # 4. with hires_latent_size: both passes use the setting
    hi = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw, **fu)
    assert hi.shape == (2, 3, 64, 64) and torch.isfinite(hi).all()
    assert {k[1] for k in cache} == {16, 32} and all(l.freeu == FREEU and all(e.freeu == FREEU for e in l.all_engines) for l in cache.values())
    hi_plain = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw)
    assert not torch.equal(hi, hi_plain)
    # 5. ... and after: identical bits
    after = run_inference(*args, hip_vae, sch, "cuda", [1], **kw)
    assert before.shape == (2, 3, 32, 32) and torch.equal(before, after)


def test_generate_cli_runs_with_the_freeu_flag(tmp_path):
    """generate.py --freeu 1.5 1.6 0.9 0.2 runs as a program and writes its PNGs."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--freeu", "1.5", "1.6", "0.9", "0.2", "--num_timesteps", "4", "--num_of_samples", "2",
           "--seed", "3", "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (128, 128, 3) and a.dtype == np.uint8 and a.std() > 0
