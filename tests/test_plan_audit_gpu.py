"""Every launch of the inference plans, one at a time, against its fp64 reference (``oracle.plan_audit`` / ``oracle.abi_ref``), at the shapes
the product gives it: pointers resolved to held tensors (use-after-free check), outputs poisoned, element-wise and aggregate bounds, the bytes
around every output, column statistics, and a bit-identical second run.  Plus every batch position of the headline plan against the B = 1
plan the oracle pins.

Besides the default loops and the VAE: the loops the newer features build (image guidance + rescale + inpainting, the same with the stochastic sampler,
PAG over a shared trunk with FreeU) on the tiny UNet, the pre-loop conditioning plans at full size (CLIP vision and text encoders, both adapters) and
the recorders ``run_inference`` builds around the loop (hires pre-pass, inpaint pre- and post-pass).

Wall time on one MI355X, this file alone: 52.3 s for its 11 tests - the three feature loops 0.6 s each (349 / 349 / 324 launches), the conditioning plans
2.2 s (367 launches), the hires / inpaint recorders below 0.1 s (5 launches); the parent commit's file on the same box, same visit: 49.8 s for 6 tests
(EXPERIMENTS.md, "Edge audit")."""
import time
import zlib

import pytest
import torch

from oracle import fullsize as fs
from oracle.plan_audit import Auditor

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def auditor():
    from photoverse_amd import _lib
    aud = Auditor(_lib.load())
    yield aud
    print("\nplan audit coverage (worst element error / bound, worst rel-L2 / aggregate bound):\n" + aud.table())


def _conditioning(B, S, P, seed):
    g = torch.Generator().manual_seed(seed)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    return cond, uncond, torch.randn(B, 4, S, S, generator=g)


def _recorders(loop):
    out = [loop.tail]
    for e in loop.all_engines:
        out += [r for r in (e.rec, e.rec_head, e.rec_tail, e.rec_cond) if r is not None]
    return out


def _audit_loop(aud, plan, loop, seed, prepare=None):
    """Conditioning, every launch of the first denoising step in a valid serial order (prefix, heads u / c, merged, tails u / c, tail - without a
    merged plan: the uncond, cond and image-only forwards, the perturbed one right behind its conditional forward, whose trunk it may share), then the
    second step's tail (the solver's second-order update).  ``prepare(loop)`` fills the static buffers of a feature loop (mask, noise stream) before
    the reset.  Returns (audited, recorded)."""
    B, S, P = loop.B, loop.S, loop.P
    cond, uncond, noise = _conditioning(B, S, P, seed)
    for (text, ip), (dt, di) in ((cond, (loop.text_c, loop.ip_c)), (uncond, (loop.text_u, loop.ip_u))):
        dt.copy_(text.reshape(dt.shape).to(dt.device))
        di.copy_(ip.reshape(di.shape).to(di.device))
    recs = _recorders(loop)
    n_aud = n_rec = 0

    def run(name, rec):
        nonlocal n_aud, n_rec
        n_rec += len(rec.calls)
        n_aud += aud.audit(f"{plan}", rec, holders=recs)

    for e in loop.all_engines:
        run("cond", e.rec_cond)
    if prepare is not None:
        prepare(loop)
    loop.reset(noise)
    step = []
    step += [e.rec for e in loop.engines_p]
    if loop.merge_lowres:
        (eu,), (ec,), (em,) = loop.engines_u, loop.engines_c, loop.engines_m
        step += [eu.rec_head, ec.rec_head, em.rec, eu.rec_tail, ec.rec_tail]
    else:
        after = {id(c): p for c, p in zip(loop.engines_c, loop.engines_p_attn)}
        for e in loop.engines_u + loop.engines_c + loop.engines_i:
            step += [e.rec] + ([after[id(e)].rec] if id(e) in after else [])
    flat = [rec for group in loop.schedule for lane in group for rec in lane]
    assert len(flat) == len(step) + 1 and all(a is b for a, b in zip(flat, step + [loop.tail])), "this order is not the loop's schedule, flattened"
    for r in step:
        run("step1", r)
    run("tail1", loop.tail)
    assert loop.state[0].item() == 1
    for r in step:                                    # second step: the UNet plans as the product runs them, then its tail audited
        r.run()
    run("tail2", loop.tail)
    assert loop.state[0].item() == 2 and torch.isfinite(loop.latents).all()
    return n_aud, n_rec


PLANS = {
    "a-headline": dict(batch=16, S=64, P=1, kw=dict(use_graph=True, two_streams=True, batch_splits=1, share_prefix=False)),
    "b-onestream": dict(batch=16, S=64, P=1, kw=dict(use_graph=True, two_streams=False, batch_splits=1, share_prefix=False)),
    "c-cfg4rank": dict(batch=4, S=96, P=6, kw={}),
    "d-bs1": dict(batch=1, S=64, P=1, kw={}),
}


def _want(doc, fn):
    fn.__doc__ = doc
    return fn


conv9 = lambda k: k[1] == "pv_gemm_conv" and "taps=9" in k[4]
#: (plan, launcher, kernel symbol, splitk, flags) rows each plan must contain
REQUIRED = {
    "a-headline": [_want("attn8_kernel<497>", lambda k: k[2] == "attn8_kernel<497>"),
                   _want("a 3x3 conv on big_tile_kernel<true, ...>", lambda k: conv9(k) and k[2].startswith("big_tile_kernel<true")),
                   _want("a 3x3 conv on big_tile_kernel<false, ...>", lambda k: conv9(k) and k[2].startswith("big_tile_kernel<false")),
                   _want("split-K 2 on the 256 x 320 tile (merged plan)", lambda k: conv9(k) and k[2].startswith("big_tile_kernel") and k[3] == 2),
                   _want("fused attn2, C = 320", lambda k: k[2].startswith("xattn_fused_kernel<320")),
                   _want("fused attn2, C = 640", lambda k: k[2].startswith("xattn_fused_kernel<640")),
                   _want("xattn_lnq_kernel", lambda k: k[2] == "xattn_lnq_kernel")],
    "c-cfg4rank": [_want(f"3x3 conv with {n} K-slices on gemm_conv_kernel<5, true", lambda k, n=n: conv9(k) and k[2].startswith("gemm_conv_kernel<5, true")
                         and k[3] == n) for n in (3, 5, 8)] +
                  [_want("attn8_kernel<497>", lambda k: k[2] == "attn8_kernel<497>"),
                   _want("fused attn2, C = 320", lambda k: k[2].startswith("xattn_fused_kernel<320")),
                   _want("fused attn2, C = 640", lambda k: k[2].startswith("xattn_fused_kernel<640")),
                   _want("xattn_lnq_kernel", lambda k: k[2] == "xattn_lnq_kernel")],
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_plan_audit_unet(plan, full_hip_unet, auditor):
    from photoverse_amd.pipeline import DenoiseLoop
    c = PLANS[plan]
    t0 = time.time()
    loop = DenoiseLoop(full_hip_unet, c["batch"], c["S"], c["P"], 50, 7.5, **c["kw"])
    n_aud, n_rec = _audit_loop(auditor, plan, loop, seed=zlib.crc32(plan.encode()) % 10000)
    print(f"\n{plan}: audited {n_aud} of {n_rec} recorded launches in {time.time() - t0:.1f} s (merge_lowres={loop.merge_lowres})")
    assert n_aud == n_rec and n_rec > 0
    # the dispatch decisions the plan is known to reach are in the audit (a dispatch change that drops one shows up here)
    rows = [k for k in auditor.rows if k[0] == plan]
    for want in REQUIRED.get(plan, ()):
        assert any(want(k) for k in rows), f"{plan}: no audited launch matches {want.__doc__}"
    del loop
    torch.cuda.empty_cache()


def test_plan_audit_vae(full_weights, auditor):
    from photoverse_amd.ops import Recorder
    from photoverse_amd.vae import AutoencoderKL
    with fs.no_init():
        vae = AutoencoderKL()
    vae.load_state_dict(full_weights("vae"))
    vae.to("cuda")
    g = torch.Generator().manual_seed(21)
    t0 = time.time()
    dec = vae._plan(1, 64, 64, torch.device("cuda"))
    dec.z.copy_(torch.randn(dec.z.shape, generator=g))
    n_dec = auditor.audit("e-vae-dec", dec.rec)
    enc = vae._plan_encode(1, 512, 512, torch.device("cuda"))
    enc.x.copy_(torch.rand(enc.x.shape, generator=g) * 2 - 1)
    n_enc = auditor.audit("e-vae-enc", enc.rec)
    mom = enc.moments.view(1, enc.h, enc.w, -1)[..., :enc.nm].permute(0, 3, 1, 2).contiguous()
    rec = Recorder(mom.device)
    rec.posterior_sample(mom, torch.randn(1, enc.nm // 2, enc.h, enc.w, generator=g).cuda())
    n_post = auditor.audit("e-vae-enc", rec)
    print(f"\nVAE: audited {n_dec} of {len(dec.rec)} decode, {n_enc} of {len(enc.rec)} encode, {n_post} of {len(rec)} posterior launches "
          f"in {time.time() - t0:.1f} s")
    assert (n_dec, n_enc, n_post) == (len(dec.rec), len(enc.rec), len(rec)) and n_dec and n_enc


def test_headline_plan_every_batch_position_matches_bs1(full_hip_unet):
    """All 16 samples of the bs = 16 headline plan (two streams, merged low-resolution plan, split-K, half-chip tiles) after 10 steps against the
    B = 1 plan - the plan the fp32 oracle pins (test_fullsize_gpu) - run on each sample's own conditioning and noise."""
    from photoverse_amd.pipeline import DenoiseLoop
    B, S = 16, 64
    cond, uncond, noise = _conditioning(B, S, 1, seed=31)
    big = DenoiseLoop(full_hip_unet, B, S, 1, 50, 7.5, use_graph=True, two_streams=True, batch_splits=1, share_prefix=False)
    big.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    big.reset(noise)
    got = big.run(10).clone().cpu()
    assert big.state[0].item() == 10
    del big
    one = DenoiseLoop(full_hip_unet, 1, S, 1, 50, 7.5)
    errs = []
    for i in range(B):
        one.set_conditioning(tuple(t[i:i + 1].cuda() for t in cond), tuple(t[i:i + 1].cuda() for t in uncond))
        one.reset(noise[i:i + 1])
        ref = one.run(10).clone().cpu()
        errs.append(rel_l2(got[i:i + 1], ref))
    print("headline plan vs B = 1 plan after 10 steps, per batch position:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs


# ------------------------------------------------------------------------------------------------------------------ feature loops on the tiny UNet
def _no_new_launch_after_a_hip_error(fn):
    """An AuditError is a finding (the test fails); anything else is a HIP error: nothing more is started on a device that has faulted."""
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        pytest.exit(f"plan audit: {type(e).__name__}: {e}", returncode=3)


@pytest.fixture(scope="module")
def tiny_hip():
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    torch.manual_seed(0)
    ref = UNet2DConditionModelRef(**TINY_CONFIG).eval()
    set_visual_cross_attention_adapter_ref(ref, (5,))
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.to("cuda")


def _inpaint_and_stream(loop):
    g = torch.Generator().manual_seed(5)
    if loop.inpaint:
        r = torch.rand(loop.B, 1, loop.S, loop.S, generator=g)
        mask = torch.where(r < 0.3, torch.zeros(()), torch.where(r > 0.7, torch.ones(()), r))            # zeros, ones and fractions
        loop.set_inpaint(mask.cuda(), torch.randn(loop.latents.shape, generator=g).cuda(), torch.randn(loop.latents.shape, generator=g).cuda())
    if loop.stochastic:
        loop.set_noise_stream(0x8000_0001_9000_0007, sample_offset=0xFFFFFFFF, stream=3)


GUIDED = dict(image_guidance_scale=3.0, guidance_rescale=0.7, inpaint=True)
FEATURE_LOOPS = {
    "h-guided": (dict(GUIDED), "pv_cfg_dpm_step_guided", ()),
    "i-stochastic": (dict(GUIDED, stochastic=True), "pv_cfg_dpm_step_stochastic", ()),
    "j-pag-freeu": (dict(pag_scale=2.0, pag_layers=("mid_block", "up_blocks.1.attentions.0"), freeu=(1.5, 1.6, 0.9, 0.2), share_trunk=True), "pv_cfg_dpm_step_pag",
                    ("freeu_rows_kernel",)),
}


@pytest.mark.parametrize("plan", list(FEATURE_LOOPS))
def test_plan_audit_feature_loops(plan, tiny_hip, auditor):
    """Every recorder of the loops the newer features build on the tiny UNet (B = 2, 16 x 16): three forwards with rescale and inpainting, the same
    as the stochastic sampler, and PAG on the mid block and an up-block layer over a shared trunk with FreeU."""
    from photoverse_amd.pipeline import DenoiseLoop
    kw, step_launcher, tags = FEATURE_LOOPS[plan]
    t0 = time.time()
    loop = DenoiseLoop(tiny_hip, 2, 16, 1, 4, 7.5, **kw)
    assert (len(loop.engines_i) == 1) == ("image_guidance_scale" in kw) and (len(loop.engines_p_attn) == 1) == ("pag_scale" in kw)
    n_aud, n_rec = _no_new_launch_after_a_hip_error(lambda: _audit_loop(auditor, plan, loop, seed=zlib.crc32(plan.encode()) % 10000, prepare=_inpaint_and_stream))
    print(f"\n{plan}: audited {n_aud} of {n_rec} recorded launches in {time.time() - t0:.1f} s")
    assert n_aud == n_rec and n_rec > 0
    rows = [k for k in auditor.rows if k[0] == plan]
    assert any(k[1] == step_launcher for k in rows), (plan, step_launcher)
    for tag in tags:
        assert any(k[2] == tag for k in rows), (plan, tag)
    del loop
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ conditioning plans, full size
def _spy_recorders(monkeypatch, *modules):
    """Recorders a function builds for itself (the adapters' forward, ``hires_start``, ``scheduler.add_noise``) are caught as they are made."""
    from photoverse_amd import ops
    made = []

    class Spy(ops.Recorder):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    for m in modules:
        monkeypatch.setattr(m, "Recorder", Spy)
    return made


def test_plan_audit_conditioning(full_weights, auditor, monkeypatch):
    """The pre-loop plans at full size, B = 1: the CLIP vision encoder (24 layers, 257 tokens), the CLIP text encoder without and with the product's one
    concept token, both adapters on the vision plan's own hidden states."""
    from photoverse_amd import adapters
    from photoverse_amd.adapters import PhotoVerseAdapter
    from photoverse_amd.clip import CLIPTextModel, CLIPVisionModel
    dev = torch.device("cuda")
    case = fs.pipeline_case()
    t0 = time.time()
    with fs.no_init():
        vis, txt = CLIPVisionModel(), CLIPTextModel()
        ads = {"image_adapter": PhotoVerseAdapter(1024, 768, 5), "text_adapter": PhotoVerseAdapter(1024, 768, 5)}
    vis.load_state_dict(full_weights("vision"))
    txt.load_state_dict(full_weights("text"))
    vis.to(dev), txt.to(dev)
    counts = {}

    def audit(plan, rec):
        counts[plan] = (_no_new_launch_after_a_hip_error(lambda: auditor.audit(plan, rec)), len(rec.calls))

    vp = vis._plan(1, dev)
    vp.pixels.copy_(case["example"]["pixel_values_clip"])
    audit("k-clip-vision", vp.rec)
    embs = [vp.hs[-1].view(1, vp.ntok, vp.dim)] + [vp.hs[i].view(1, vp.ntok, vp.dim) for i in case["layers"]]
    made = _spy_recorders(monkeypatch, adapters)
    concept = None
    for name, ad in ads.items():
        ad.load_state_dict(full_weights(name))
        ad.to(dev)
        with torch.no_grad():
            out = ad(embs, token_index=case["token_index"])
        concept = out if name == "text_adapter" else concept
        audit(f"l-{name.replace('_', '-')}", made[-1])
    for E in (0, 1):
        tp = txt._plan(1, 77, E, dev)
        tp.ids.copy_(case["example"]["text_input_ids"] if E else case["uncond_ids"])
        if E:
            assert concept.shape == (1, E, 768)
            tp.concept.copy_(concept.reshape(E, -1))
            tp.pidx.copy_(case["example"]["concept_placeholder_idx"].reshape(-1))
        audit(f"m-clip-text-e{E}", tp.rec)
    print(f"\nconditioning: " + ", ".join(f"{k} {a} of {n}" for k, (a, n) in counts.items()) + f" launches audited in {time.time() - t0:.1f} s")
    assert all(a == n and n > 0 for a, n in counts.values()), counts
    rows = list(auditor.rows)
    assert any(k[0].startswith("m-clip-text") and k[1] == "pv_attention" and "causal" in k[4] and "d=64" in k[4] for k in rows)
    for launcher in ("pv_clip_text_embed", "pv_patchify", "pv_clip_vision_embed", "pv_rows_mean"):
        assert any(k[1] == launcher for k in rows), launcher
    assert any(k[1] == "pv_clip_text_embed" and "n_concept" in k[4] for k in rows) and any(k[1] == "pv_clip_text_embed" and not k[4] for k in rows)
    assert any(k[1] == "pv_rows_mean" and "accumulate" in k[4] for k in rows)


def test_plan_audit_hires_and_inpaint_recorders(auditor, monkeypatch):
    """The recorders ``infer.run_inference`` builds around the loop, at 64 -> 96, B = 1: the hires pre-pass (``hires_start``), the inpaint pre-pass
    (``scheduler.add_noise``) and the post-pass (1 / scaling_factor, paste-back + clamp on the 768-pixel image, the plain clamp)."""
    from photoverse_amd import ops
    from photoverse_amd.infer import hires_start
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(43)
    t0 = time.time()
    made = _spy_recorders(monkeypatch, ops)
    sch = DPMSolverMultistepScheduler()
    x_start, start = hires_start(torch.randn(1, 4, 64, 64, generator=g).cuda(), torch.randn(1, 4, 96, 96, generator=g).cuda(), sch, 50, 0.5)
    assert start == 25 and tuple(x_start.shape) == (1, 4, 96, 96) and len(made) == 1
    sch.set_timesteps(50)
    sch.add_noise(torch.randn(1, 4, 96, 96, generator=g).cuda(), torch.randn(1, 4, 96, 96, generator=g).cuda(), sch.timesteps[10:11])
    assert len(made) == 2
    post = ops.Recorder(torch.device("cuda"))                       # infer.py's post-pass, launch for launch
    post.affine_rows(torch.randn(1, 4, 96, 96, generator=g).cuda(), torch.full((1,), 1.0 / 0.18215).cuda())
    images = (torch.randn(1, 3, 768, 768, generator=g) * 0.8).cuda()
    mask = (torch.rand(1, 1, 768, 768, generator=g) > 0.5).float().cuda()
    post.composite_clamp(images, (torch.rand(1, 3, 768, 768, generator=g) * 2 - 1).cuda(), mask, -1.0, 1.0, out=images)
    post.clamp_((torch.randn(1, 3, 768, 768, generator=g) * 0.8).cuda(), -1.0, 1.0)
    counts = {}
    for plan, rec in (("n-hires-pre", made[0]), ("o-inpaint-pre", made[1]), ("p-post", post)):
        counts[plan] = (_no_new_launch_after_a_hip_error(lambda: auditor.audit(plan, rec)), len(rec.calls))
    print(f"\nhires / inpaint recorders: " + ", ".join(f"{k} {a} of {n}" for k, (a, n) in counts.items()) + f" launches audited in {time.time() - t0:.1f} s")
    assert all(a == n and n > 0 for a, n in counts.values()), counts
    rows = list(auditor.rows)
    for plan, launcher in (("n-hires-pre", "pv_resize_bilinear_affine_f32"), ("o-inpaint-pre", "pv_affine_rows_f32"), ("p-post", "pv_composite_clamp_f32"),
                           ("p-post", "pv_clamp_f32"), ("p-post", "pv_affine_rows_f32")):
        assert any(k[0] == plan and k[1] == launcher for k in rows), (plan, launcher)
