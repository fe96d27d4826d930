"""GPU tests of windowed denoising (MultiDiffusion): ``pv_window_gather`` / ``pv_window_blend`` against the float64 slicing of
``tests/_multidiffusion_ref.py`` in guarded buffers, eagerly and under capture; ``WindowedDenoiseLoop`` against the windowed oracle loop (every window
with its own solver), bit for bit against plain ``DenoiseLoop``s where the windows are disjoint, with inpainting, PAG, token downsampling, a ControlNet
and the third forward; ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch

from _multidiffusion_ref import blend_ref, canvas_inputs, gather_ref, n_cover, windowed_oracle_loop
from test_kv_downsample_cpu import TOP, pooled_oracle
from test_pag_cpu import B, G_PAG, G_TEXT, P, S, STEPS, TOL_LOOP, oracle_loop, perturbed_oracle, rel_l2, tiny_oracle

pytestmark = pytest.mark.gpu

MID = ("mid_block.attentions.0",)
CANARY, GUARD = -7.25, 8           # guard floats in front of and behind every buffer: a multiple of 4, so the views keep the allocation's 16-byte alignment
EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the kernels
#: (B, C, H, W, S, stride)
KERNEL_SHAPES = ((1, 1, 2, 2, 2, 1),             # one window
                 (1, 1, 3, 5, 2, 1),             # scalar path, up to 4-fold coverage
                 (2, 4, 20, 18, 16, 8),          # clamped last origins 4 and 2: the scalar path is forced
                 (2, 4, 24, 32, 16, 8),          # the 16-byte path; the loop test's shape
                 (1, 4, 32, 32, 16, 4),          # 25 windows, 16-fold coverage
                 (1, 3, 128, 192, 128, 64))      # a control image's gather


def _guarded(shape, fill=None):
    """(flat buffer with canary guards, the contiguous view of ``shape`` inside it)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    view = flat[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return flat, view


def _guards_intact(flat):
    return bool((flat[:GUARD] == CANARY).all() and (flat[-GUARD:] == CANARY).all())


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_kernels(shape):
    """``window_gather``: the bits of the torch slices.  ``window_blend`` of RANDOM windows (not a gather: the mean has to average), with uniform (NULL),
    explicit all-ones and gaussian profiles, against ``blend_ref`` in float64 on the same fp32 profile values.  Per element
    ``|got - ref| <= (n + 6) * 2^-24 * max|windows|`` with ``n`` the largest number of covering windows: two roundings per product ``(py * px) * w``,
    ``n - 1`` additions, the two normaliser sums (their relative errors are below those of ``n`` additions of positive terms, counted as two), their
    product and one division, and ``sum w|e| / sum w <= max|e|``.  Where a single window covers an element the NULL profile keeps that window's bits.
    The inputs are unchanged, the guards around all three buffers intact, and a captured replay of both launches gives the eager bits.
    Measured on MI355X (printed with -s), worst share of the bound, uniform / gaussian, in the order of KERNEL_SHAPES: 0 / 0, 0.030 / 0.030, 0.074 / 0.176,
    0.035 / 0.145, 0.023 / 0.075 (16-fold coverage: 4.0e-7 / 1.3e-6 against 1.7e-5), 0.037 / 0.216."""
    from photoverse_amd.multidiffusion import window_origins, window_profile
    from photoverse_amd.ops import window_blend, window_gather
    Bn, C, H, W, Sw, stride = shape
    oy, ox = window_origins(H, Sw, stride), window_origins(W, Sw, stride)
    nW, n = len(oy) * len(ox), n_cover(H, W, Sw, oy, ox)
    g = torch.Generator().manual_seed(sum(shape))
    canvas = torch.randn(Bn, C, H, W, generator=g) * 3
    windows = torch.randn(Bn * nW, C, Sw, Sw, generator=g) * 3
    # gather
    f_canvas, d_canvas = _guarded(canvas.shape, canvas)
    f_win, d_win = _guarded(windows.shape)
    assert window_gather(d_canvas, Sw, oy, ox, out=d_win) is d_win
    torch.cuda.synchronize()
    got = d_win.cpu()
    assert torch.equal(got.view(torch.int32), gather_ref(canvas, Sw, oy, ox).float().view(torch.int32))
    assert torch.equal(d_canvas.cpu().view(torch.int32), canvas.view(torch.int32)) and _guards_intact(f_canvas) and _guards_intact(f_win)
    own = window_gather(d_canvas, Sw, oy, ox)
    assert own.shape == windows.shape and torch.equal(own.cpu(), got)
    # blend
    d_win.copy_(windows)
    cover_y = torch.tensor([sum(1 for o in oy if o <= y < o + Sw) for y in range(H)])
    cover_x = torch.tensor([sum(1 for o in ox if o <= x < o + Sw) for x in range(W)])
    single = (cover_y[:, None] * cover_x[None, :]) == 1
    bound = (n + 6) * EPS * windows.abs().max().item()
    results = {}
    for kind in ("null", "uniform", "gaussian"):
        profile = None if kind == "null" else window_profile(kind, Sw)
        f_prof, d_prof = (None, None) if profile is None else _guarded((Sw,), profile)
        d_canvas.fill_(CANARY)
        assert window_blend(d_win, d_canvas, Sw, oy, ox, d_prof) is d_canvas
        torch.cuda.synchronize()
        got = d_canvas.cpu()
        ref = blend_ref(windows, canvas.shape, Sw, oy, ox, profile)
        worst = (got.double() - ref).abs().max().item()
        print(f"window_blend {shape} {kind}: n = {n}, max |got - ref| = {worst:.3e} = {worst / bound:.3f} of the bound {bound:.3e}")
        assert torch.isfinite(got).all() and worst <= bound
        assert torch.equal(d_win.cpu().view(torch.int32), windows.view(torch.int32)) and _guards_intact(f_canvas) and _guards_intact(f_win)
        assert profile is None or (torch.equal(d_prof.cpu(), profile) and _guards_intact(f_prof))
        results[kind] = got
    assert single.any()                                                                            # the corners, at the least
    assert torch.equal(results["null"][..., single].double(), blend_ref(windows, canvas.shape, Sw, oy, ox, None)[..., single])     # one window: its bits
    assert torch.equal(results["null"].view(torch.int32), results["uniform"].view(torch.int32))
    # a captured replay of both launches: the eager bits
    d_prof = window_profile("gaussian", Sw).cuda()
    f_c2, d_c2 = _guarded(canvas.shape, canvas)
    f_w2, d_w2 = _guarded(windows.shape)
    f_o2, d_o2 = _guarded(canvas.shape)
    window_gather(d_c2, Sw, oy, ox, out=d_w2)
    window_blend(d_win, d_o2, Sw, oy, ox, d_prof)
    torch.cuda.synchronize()
    eager = (d_w2.cpu(), d_o2.cpu())
    d_w2.fill_(CANARY)
    d_o2.fill_(CANARY)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        window_gather(d_c2, Sw, oy, ox, out=d_w2)
        window_blend(d_win, d_o2, Sw, oy, ox, d_prof)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(d_w2.cpu().view(torch.int32), eager[0].view(torch.int32)) and torch.equal(d_o2.cpu().view(torch.int32), eager[1].view(torch.int32))
    assert torch.equal(eager[1], results["gaussian"]) and all(_guards_intact(f) for f in (f_c2, f_w2, f_o2))


def test_wrappers_reject_what_the_launchers_reject():
    from photoverse_amd.ops import HipLaunchError, window_blend, window_gather
    x = torch.zeros(1, 1, 8, 8, device="cuda")
    for oy, ox in (((0, 2), (0, 4)), ((0, 4), (4,)), ((0, 4), (0, 5))):
        with pytest.raises(HipLaunchError, match="pv_window_gather"):
            window_gather(x, 4, oy, ox)
    with pytest.raises(HipLaunchError, match="pv_window_blend"):
        window_blend(torch.zeros(4, 1, 4, 4, device="cuda"), x, 4, (0, 4), (1, 4))
    with pytest.raises(AssertionError):
        window_blend(torch.zeros(3, 1, 4, 4, device="cuda"), x, 4, (0, 4), (0, 4))


# ---------------------------------------------------------------------------------------------------------------- the loop
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


def _run(loop, cond, uncond, noise, img=None):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    if img is not None:
        loop.set_control(img.cuda())
    loop.reset(noise.cuda())
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == STEPS
    return out


@torch.no_grad()
def test_loop_matches_the_windowed_oracle_loop(tiny_pair):
    """B = 2, canvas 24 x 32, window 16, stride 8 (6 windows, an inner ``DenoiseLoop`` of batch 12), 4 steps, guidance 5, uniform and gaussian weights:
    rel-L2 against ``windowed_oracle_loop`` below TOL_LOOP - the bound every four-step tiny loop of this suite is held to; a convex combination of
    window results cannot lie farther from the combination of their references than the worst window - and more than TOL_LOOP away from the plain
    loop on that canvas (``DenoiseLoop`` takes no rectangle: the plain oracle loop stands for it) and from the other weights.  The graph run equals the eager run bit for bit;
    ``launches_per_step`` is the inner loop's plus two.
    Measured on MI355X (printed with -s): rel-L2 against the windowed oracle loop 7.730e-4 (uniform) and 9.936e-4 (gaussian), against the plain oracle loop
    1.449e-1 and 1.094e-1, gaussian against uniform 1.471e-1; 212 launches per step."""
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = canvas_inputs(24, 32)
    plain = oracle_loop(ref, None, cond, uncond, noise, G_TEXT)
    outs = {}
    for weights in ("uniform", "gaussian"):
        exp = windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, weights, STEPS)
        loop = WindowedDenoiseLoop(hip, B, (24, 32), 16, P, STEPS, G_TEXT, window_stride=8, window_weights=weights)
        assert (loop.oy, loop.ox, loop.nW) == ((0, 8), (0, 8, 16), 6) and isinstance(loop.inner, DenoiseLoop) and loop.inner.B == 12 and loop.inner.S == 16
        assert loop.launches_per_step == loop.inner.launches_per_step + 2 and loop.T == STEPS and loop.scheduler is loop.inner.scheduler
        assert tuple(loop.latents.shape) == (B, 4, 24, 32) and (loop.profile is None) == (weights == "uniform")
        out = _run(loop, cond, uncond, noise)
        eager = WindowedDenoiseLoop(hip, B, (24, 32), 16, P, STEPS, G_TEXT, window_stride=8, window_weights=weights, use_graph=False, two_streams=False)
        assert eager.inner.graph is None and torch.equal(_run(eager, cond, uncond, noise), out) and eager.inner.graph is None
        assert torch.equal(_run(loop, cond, uncond, noise), out)                       # a second generation on the captured graph
        err, away = rel_l2(out, exp), rel_l2(out, plain)
        print(f"windowed loop 24 x 32, window 16 stride 8, {weights}: rel-L2 vs the windowed oracle loop = {err:.3e}, vs the plain oracle loop = {away:.3e}; "
              f"launches per step {loop.launches_per_step}")
        assert torch.isfinite(out).all() and err < TOL_LOOP and away > TOL_LOOP
        outs[weights] = out
    between = rel_l2(outs["gaussian"], outs["uniform"])
    print(f"windowed loop: gaussian vs uniform rel-L2 = {between:.3e}")
    assert between > TOL_LOOP


@torch.no_grad()
def test_exact_plumbing_against_plain_loops(tiny_pair):
    """Where no element is covered twice the windowed loop is the plain loop, bit for bit (uniform weights: num = (1 * 1) * w, den = 1 * 1).
    ``window == canvas == 16``: the bits of ``DenoiseLoop(B = 2)``.  Canvas 32 x 32, window 16, stride 16 - four disjoint tiles: the bits of
    ``DenoiseLoop(B = 8)`` run on the tiles in window order (sample-major, ``k = ky * nx + kx``) under each sample's conditioning repeated four
    times, reassembled - which pins the ordering and the conditioning replication.  A loop handed in as ``inner`` is used as it is."""
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = canvas_inputs(16, 16)
    plain2 = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    exp = _run(plain2, cond, uncond, noise)
    one = WindowedDenoiseLoop(hip, B, 16, 16, P, STEPS, G_TEXT)
    assert (one.oy, one.ox, one.nW, one.stride) == ((0,), (0,), 1, 8)
    assert torch.equal(_run(one, cond, uncond, noise), exp)
    handed = WindowedDenoiseLoop(hip, B, (16, 16), 16, P, STEPS, G_TEXT, inner=plain2)
    assert handed.inner is plain2 and torch.equal(_run(handed, cond, uncond, noise), exp)
    with pytest.raises(ValueError, match="inner loop"):
        WindowedDenoiseLoop(hip, B, (16, 32), 16, P, STEPS, G_TEXT, inner=plain2)
    cond, uncond, noise = canvas_inputs(32, 32)
    tiles = WindowedDenoiseLoop(hip, B, 32, 16, P, STEPS, G_TEXT, window_stride=16)
    assert (tiles.oy, tiles.ox, tiles.nW) == ((0, 16), (0, 16), 4)
    out = _run(tiles, cond, uncond, noise)
    plain8 = DenoiseLoop(hip, 4 * B, S, P, STEPS, G_TEXT)
    rep = lambda pair: tuple(t.repeat_interleave(4, dim=0) for t in pair)
    res8 = _run(plain8, rep(cond), rep(uncond), gather_ref(noise, 16, (0, 16), (0, 16)).float())
    back = blend_ref(res8, noise.shape, 16, (0, 16), (0, 16)).float()                  # disjoint: a reassembly, exact
    assert torch.equal(back[1, :, 16:, :16], res8[4 + 2]) and torch.equal(out, back)
    assert not torch.equal(out[0, :, :16, :16], out[0, :, :16, 16:])


@torch.no_grad()
def test_ragged_canvas(tiny_pair):
    """Canvas 20 x 18, window 16, stride 8: the clamped origins (0, 4) and (0, 2) - the scalar path of both launches, overlaps of 12 and 14 - against
    its windowed oracle loop within TOL_LOOP.  Measured on MI355X (printed with -s): rel-L2 6.401e-4."""
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = canvas_inputs(20, 18)
    loop = WindowedDenoiseLoop(hip, B, (20, 18), 16, P, STEPS, G_TEXT)
    assert (loop.oy, loop.ox, loop.stride) == ((0, 4), (0, 2), 8)
    out = _run(loop, cond, uncond, noise)
    err = rel_l2(out, windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS))
    print(f"windowed loop 20 x 18, window 16 stride 8: rel-L2 vs the windowed oracle loop = {err:.3e}")
    assert torch.isfinite(out).all() and err < TOL_LOOP


@torch.no_grad()
def test_inpainting_keeps_the_known_latents(tiny_pair):
    """``inpaint=True`` on canvas 24 x 32: every window's last masked step leaves exactly ``known`` outside the mask, so the canvas ends there on the
    known latents within the blend's bound ``(n + 6) * 2^-24 * max|windows|`` (n = 4-fold coverage at most), and differs inside the mask.
    Measured on MI355X (printed with -s): max |canvas - known| outside the mask 0 (uniform: the mean of equal values adds exactly here) and 3.6e-7
    (gaussian) against bounds of 1.2e-5 and 1.3e-5."""
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = canvas_inputs(24, 32)
    g = torch.Generator().manual_seed(9)
    known, renoise = torch.randn(B, 4, 24, 32, generator=g), torch.randn(B, 4, 24, 32, generator=g)
    mask = torch.zeros(1, 1, 24, 32)
    mask[:, :, 5:19, 9:27] = 1.0
    for weights in ("uniform", "gaussian"):
        loop = WindowedDenoiseLoop(hip, B, (24, 32), 16, P, STEPS, G_TEXT, window_stride=8, window_weights=weights, inpaint=True)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.set_inpaint(mask, known.cuda(), renoise)                                  # operands arrive on either device
        loop.reset(noise.cuda())
        out = loop.run().clone().cpu()
        bound = (n_cover(24, 32, 16, loop.oy, loop.ox) + 6) * EPS * loop.inner.latents.abs().max().item()
        keep = (mask == 0).expand_as(out)
        worst = (out - known)[keep].abs().max().item()
        print(f"windowed inpainting, {weights}: max |canvas - known| outside the mask = {worst:.3e} (bound {bound:.3e})")
        assert torch.isfinite(out).all() and worst <= bound
        assert (out - known)[~keep].abs().mean().item() > 0.1                                      # inside the mask: generated


@torch.no_grad()
def test_pag_token_downsampling_and_the_third_forward_act_per_window(tiny_pair):
    """Canvas 16 x 24 (windows at x = 0 and 8, an inner batch of 4), each against its windowed oracle loop within TOL_LOOP: ``pag_scale=2`` on the mid
    block (``perturbed_oracle`` per window), ``kv_downsample=2`` (``pooled_oracle`` per window), and ``image_guidance_scale=2`` - the third forward,
    run eagerly on one stream only (no captured loop with three parallel branches is built here).
    Measured on MI355X (printed with -s), rel-L2 against its oracle loop / against the oracle loop without the option: PAG 1.040e-3 / 2.557e-2, token
    downsampling 8.559e-4 / 6.819e-3, image guidance 8.050e-4 / 3.076e-1."""
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = canvas_inputs(16, 24)
    pooled = pooled_oracle(ref, TOP, 2, "avg")
    cases = (("pag_scale=2", dict(pag_scale=G_PAG, pag_layers=("mid_block",)), dict(pert=perturbed_oracle(ref, MID), g_pag=G_PAG), ref),
             ("kv_downsample=2", dict(kv_downsample=2), dict(), pooled),
             ("image_guidance_scale=2", dict(image_guidance_scale=2.0, use_graph=False, two_streams=False), dict(g_image=2.0), ref))
    base = None
    for name, loop_kw, ref_kw, model in cases:
        loop = WindowedDenoiseLoop(hip, B, (16, 24), 16, P, STEPS, G_TEXT, **loop_kw)
        assert (loop.oy, loop.ox) == ((0,), (0, 8)) and loop.inner.B == 4
        out = _run(loop, cond, uncond, noise)
        err = rel_l2(out, windowed_oracle_loop(model, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS, **ref_kw))
        if base is None:
            base = windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS)
        print(f"windowed loop 16 x 24 with {name}: rel-L2 vs its oracle loop = {err:.3e}, vs the oracle loop without = {rel_l2(out, base):.3e}")
        assert torch.isfinite(out).all() and err < TOL_LOOP and rel_l2(out, base) > TOL_LOOP


@torch.no_grad()
def test_loop_under_a_controlnet():
    """Canvas 16 x 24 under the tiny ControlNet: ``set_control`` cuts the (2, 3, 128, 192) control image into the windows' 128 x 128 crops (the gather
    with origins and size times 8), and the loop matches the oracle loop with ``ControlledRef`` per window on the cropped image, within TOL_LOOP.
    Measured on MI355X (printed with -s): rel-L2 7.922e-4 against the oracle loop, 3.353e-1 against the oracle loop without control."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    from test_controlnet_cpu import ControlledRef, control_image, tiny_controlnet_ref
    ref, cn_ref = tiny_oracle(), tiny_controlnet_ref()
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    cn = ControlNetModel(**TINY_CONFIG)
    cn.load_state_dict(cn_ref.state_dict(), strict=True)
    cn.to("cuda")
    cond, uncond, noise = canvas_inputs(16, 24)
    img = control_image(batch=B, size=192)[:, :, :128, :].contiguous()
    loop = WindowedDenoiseLoop(hip, B, (16, 24), 16, P, STEPS, G_TEXT, controlnet=cn)
    out = _run(loop, cond, uncond, noise, img)
    assert torch.equal(loop.inner.control_image.cpu(), gather_ref(img, 128, (0,), (0, 64)).float())
    loop.inner.control_image.zero_()
    loop.set_control(img)                                                              # a CPU image, as run_inference's callers pass it
    assert torch.equal(loop.inner.control_image.cpu(), gather_ref(img, 128, (0,), (0, 64)).float())
    crops = {(0, kx): ControlledRef(ref, cn_ref, img[:, :, :, 64 * kx:64 * kx + 128].contiguous(), 1.0) for kx in (0, 1)}
    exp = windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS, model_for=lambda ky, kx: crops[ky, kx])
    err = rel_l2(out, exp)
    away = rel_l2(out, windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS))
    print(f"windowed loop 16 x 24 under a ControlNet: rel-L2 vs the oracle loop = {err:.3e}, vs the oracle loop without control = {away:.3e}")
    assert torch.isfinite(out).all() and err < TOL_LOOP and away > TOL_LOOP
    with pytest.raises(ValueError, match="control_image"):
        loop.set_control(control_image(batch=B, size=128).cuda())


def test_refusals(tiny_pair):
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    _, hip = tiny_pair
    for kw, match in ((dict(stochastic=True), "stochastic"), (dict(scheduler=DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")), "stochastic"),
                      (dict(training_mode=True), "training_mode")):
        with pytest.raises(ValueError, match=match):
            WindowedDenoiseLoop(hip, B, (24, 32), 16, P, STEPS, G_TEXT, **kw)


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
VAE_TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 128, 128, 128), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@torch.no_grad()
def test_run_inference_windowed_end_to_end():
    """``run_inference`` on the tiny models with the tiny x8 VAE.  ``latent_size=(16, 32), window=16``: (2, 3, 128, 256) finite images from a cached
    inner loop of batch 6 at 16 x 16; the weights change the result, an equal call repeats it.  ``hires_latent_size=32,
    hires_window=16``: (2, 3, 256, 256), the first pass on the plain cached loop.  A plain call before and after gives identical bits, and its cached
    loop is the same object."""
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
    ex = {"pixel_values": torch.rand(2, 3, 128, 128, generator=g) * 2 - 1, "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(guidance_scale=3.0, timesteps=4, seed=1)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, None, sch, "cuda", [1], latent_size=16, **kw)
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(reversed(cache.values()))
    assert plain_loop.B == 2
    # 1. a panorama canvas
    wide = run_inference(*args, hip_vae, sch, "cuda", [1], latent_size=(16, 32), window=16, **kw)
    assert wide.shape == (2, 3, 128, 256) and torch.isfinite(wide).all() and wide.std() > 0
    inner = next(reversed(cache.values()))
    assert inner is not plain_loop and (inner.B, inner.S) == (6, 16) and len(cache) == 2
    assert torch.equal(run_inference(*args, hip_vae, sch, "cuda", [1], latent_size=(16, 32), window=16, **kw), wide) and next(reversed(cache.values())) is inner
    lat = run_inference(*args, None, sch, "cuda", [1], latent_size=(16, 32), window=16, **kw)
    assert lat.shape == (2, 4, 16, 32) and next(reversed(cache.values())) is inner
    gau = run_inference(*args, None, sch, "cuda", [1], latent_size=(16, 32), window=16, window_weights="gaussian", **kw)
    assert gau.shape == lat.shape and torch.isfinite(gau).all() and not torch.equal(gau, lat) and next(reversed(cache.values())) is inner
    # a square canvas of one window: the plain call's bits on the plain loop
    assert torch.equal(run_inference(*args, None, sch, "cuda", [1], latent_size=16, window=16, **kw), before) and next(reversed(cache.values())) is plain_loop
    # 2. a windowed second pass
    hi = run_inference(*args, hip_vae, sch, "cuda", [1], latent_size=16, hires_latent_size=32, hires_window=16, **kw)
    assert hi.shape == (2, 3, 256, 256) and torch.isfinite(hi).all() and hi.std() > 0
    assert [(l.B, l.S) for l in cache.values()] == [(2, 16), (18, 16)] and next(iter(cache.values())) is plain_loop
    with pytest.raises(ValueError, match="needs window"):
        run_inference(*args, None, sch, "cuda", [1], latent_size=(16, 32), **kw)
    # 3. a plain call afterwards: the plain loop's bits
    after = run_inference(*args, None, sch, "cuda", [1], latent_size=16, **kw)
    assert torch.equal(after, before) and next(reversed(cache.values())) is plain_loop


@torch.no_grad()
def test_run_inference_windowed_with_a_controlnet_and_a_mask_from_the_cpu():
    """``run_inference(window=...)`` on a square canvas with the operands as callers pass them - control image and inpainting mask on the CPU.
    Canvas 24, window 16 (four windows, an inner batch of 8): the ControlNet changes the result, a CUDA control image gives the same bits; a canvas of
    one window has the bits of the plain ControlNet call; with ``inpaint_mask`` the pixels outside the mask are the photograph's."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.infer import run_inference
    from photoverse_amd.modeling_utils import load_models
    from photoverse_amd.vae import AutoencoderKL
    from test_controlnet_cpu import control_image, nonzero_init_
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
    g = torch.Generator().manual_seed(4)
    ex = {"pixel_values": torch.rand(2, 3, 192, 192, generator=g) * 2 - 1, "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(guidance_scale=3.0, timesteps=4, seed=1)
    args = (ex, tok, ie, te, unet, ta, ia)
    img = control_image(size=192)
    assert not img.is_cuda
    plain = run_inference(*args, None, sch, "cuda", [1], latent_size=24, window=16, **kw)
    ctrl = run_inference(*args, None, sch, "cuda", [1], latent_size=24, window=16, controlnet=cn, control_image=img, **kw)
    inner = next(reversed(unet.__dict__["_denoise_loops"].values()))
    assert (inner.B, inner.S) == (8, 16) and inner.controlnet is cn
    assert ctrl.shape == (2, 4, 24, 24) and torch.isfinite(ctrl).all() and not torch.equal(ctrl, plain)
    assert torch.equal(run_inference(*args, None, sch, "cuda", [1], latent_size=24, window=16, controlnet=cn, control_image=img.cuda(), **kw), ctrl)
    shared = run_inference(*args, None, sch, "cuda", [1], latent_size=24, window=16, controlnet=cn, control_image=img[:1], **kw)       # one image for the batch
    assert torch.isfinite(shared).all() and torch.equal(shared[0], ctrl[0]) and not torch.equal(shared[1], ctrl[1])
    # one window: the plain ControlNet call
    img16 = control_image(size=128)
    one = run_inference(*args, None, sch, "cuda", [1], latent_size=16, window=16, controlnet=cn, control_image=img16, **kw)
    assert torch.equal(one, run_inference(*args, None, sch, "cuda", [1], latent_size=16, controlnet=cn, control_image=img16, **kw))
    # inpainting: the mask arrives on the CPU
    mask = torch.zeros(1, 1, 192, 192)
    mask[..., 40:136, 24:120] = 1
    pix = run_inference(*args, hip_vae, sch, "cuda", [1], latent_size=24, window=16, inpaint_mask=mask, strength=0.75, controlnet=cn, control_image=img, **kw)
    assert pix.shape == (2, 3, 192, 192) and torch.isfinite(pix).all()
    keep = (mask == 0).expand(2, 3, 192, 192)
    assert torch.equal(pix.cpu()[keep], ex["pixel_values"].clamp(-1, 1)[keep]) and not torch.equal(pix.cpu()[~keep], ex["pixel_values"].clamp(-1, 1)[~keep])


def test_generate_cli_runs_with_the_window_flags(tmp_path):
    """generate.py runs as a program and writes its PNGs: a 16 x 32 canvas in windows of 16 (128 x 256 pixels), and a windowed second pass at 32."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
            "--guidance_scale", "5", "--num_timesteps", "4", "--num_of_samples", "2", "--seed", "3", "--encoder_layers_idx", "1", "2"]
    for name, flags, size in (("wide", ["--latent_width", "32", "--window", "16", "--window_stride", "8"], (128, 256)),
                              ("hires", ["--hires_latent_size", "32", "--hires_window", "16"], (256, 256))):
        out = tmp_path / name
        r = subprocess.run(base + flags + ["--results_dir", str(out)], capture_output=True, text=True, timeout=900, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        files = sorted(os.listdir(out))
        assert files == ["generated_image0.png", "generated_image1.png"]
        for f in files:
            a = np.asarray(Image.open(out / f))
            assert a.shape == size + (3,) and a.dtype == np.uint8 and a.std() > 0
