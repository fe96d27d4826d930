"""``run_inference`` with the reference's signature (``/root/reference/models/infer.py:7-123``).

Conditioning runs once per call on HIP kernels (CLIP ViT x2, adapters x3, text encoder x2, ``infer.py:76-96``); the
denoising loop (``:98-119``) is the graph-captured ``DenoiseLoop``; the VAE decode + clamp of ``:121-123`` runs on
``photoverse_amd.vae.AutoencoderKL`` (or any object with ``.decode`` / ``.config.scaling_factor``).  With ``vae=None`` the
function returns the final LATENTS (the value of ``latents`` after ``:119``).  ``from_noised_image`` (``:62-65``) starts from
``add_noise(vae.encode(pixel_values).latent_dist.sample() * scaling_factor, noise, t_0)``; the posterior sample is drawn on the
device generator (``torch.manual_seed(seed)`` seeds it like the reference's, the streams of two platforms never match bit for bit).

Beyond the reference ([EXT] diffusers' img2img ``strength`` and inpainting with a 4-channel UNet): ``strength`` starts the loop part-way down
the schedule from the image noised to that step, ``inpaint_mask`` regenerates only the masked region - the blend with the re-noised known
latents is part of the solver-step launch (``pv_cfg_dpm_step_masked``) - and ``paste_back`` composites the decoded result onto the input pixels.

Also beyond the reference ([EXT] the two-pass "hires fix" of A1111 / diffusers' latent upscale): with ``hires_latent_size`` the image is generated at
``latent_size`` (SD-v1.5 was trained at 64), its latents are upscaled and re-noised part-way up the schedule - ``hires_start``, one launch of
``pv_resize_bilinear_affine_f32`` - and only the last ``hires_strength`` of the schedule runs at the large size, on a second cached ``DenoiseLoop``.

And control over the guidance itself ([EXT] the InstructPix2Pix split of classifier-free guidance, diffusers' ``guidance_rescale``):
``image_guidance_scale`` gives the image-token branch (identity) a scale of its own beside ``guidance_scale`` (the prompt) at the price of a third forward
per step, ``guidance_rescale`` renormalises the guided prediction to the conditional one's per-sample standard deviation; both are part of the solver-step
launch (``pv_cfg_dpm_step_guided``).

And the sampler ([EXT] diffusers' ``algorithm_type="sde-dpmsolver++"``, the "DPM++ 2M SDE" of the front ends): ``sampler="sde-dpmsolver++"`` runs the
stochastic form of the solver, whose fresh noise per step is generated inside the solver-step launch (``pv_cfg_dpm_step_stochastic``) from a Philox
stream keyed on ``seed``, the global sample index and the device-resident step counter - the captured graph is the same for every step and seed.

And perturbed-attention guidance ([EXT] Ahn et al. 2024; diffusers' ``pag_scale`` / ``pag_applied_layers``): ``pag_scale`` adds a forward per step whose
chosen self-attention maps are the identity (``UNetEngine(perturb=...)``, started from the conditional forward's tensors at its first perturbed layer)
and one term to the solver-step launch (``pv_cfg_dpm_step_pag``).

And FreeU ([EXT] Si et al., CVPR 2024; diffusers' ``enable_freeu``): ``freeu=(b1, b2, s1, s2)`` re-weights the decoder's first two up blocks inside every
forward - the first half of the backbone's channels times ``b``, the four lowest spatial frequencies of the skip connection times ``s`` - with one
launch per ResnetBlock (``pv_freeu_rows``: the Fourier filter in closed form, no FFT) and no further forward or weights.

And spatial control ([EXT] ControlNet, Zhang et al. 2023; diffusers' ``StableDiffusionControlNetPipeline``): ``controlnet`` + ``control_image`` run a
``controlnet.ControlNetModel`` beside the UNet - its conditioning embedding once per call (``pv_hint_conv3x3``), its encoder twice per step - and add its
zero-conv residuals to the UNet's skip connections and mid block output (``UNetEngine(control=...)``).

And token downsampling ([EXT] ToDo, Smith et al. 2024): ``kv_downsample`` / ``hires_kv_downsample`` pool the keys and values of the chosen self-attention
layers by a factor per side (``pv_token_pool``, one launch behind the layer's qkv projection) while every query still attends: the N^2 part of the
high-resolution levels shrinks by the factor squared, approximately, with no weights changed.

And windowed denoising ([EXT] MultiDiffusion, Bar-Tal et al. 2023; diffusers' ``StableDiffusionPanoramaPipeline``): with ``window`` / ``hires_window`` a pass
runs through a ``multidiffusion.WindowedDenoiseLoop`` - every step denoises overlapping windows of the training size as samples of a larger batch on the
ordinary cached ``DenoiseLoop`` and sets the canvas to their weighted mean (``pv_window_gather`` / ``pv_window_blend`` around the step) - so the canvas may
have any height and width.
"""
from __future__ import annotations

import math
import numbers
from collections import OrderedDict

import torch

from .multidiffusion import WINDOW_WEIGHTS, WindowedDenoiseLoop, window_grid
from .pipeline import DenoiseLoop
from .scheduler import DPMSolverMultistepScheduler
from .unet import KV_DOWNSAMPLE_METHODS, check_kv_downsample_factor, normalize_freeu, resolve_kv_downsample_layers, resolve_pag_layers


#: captured loops kept per UNet (each holds two engines of static activations: ~4 GB at bs=16) - least recently used evicted
MAX_CACHED_LOOPS = 2


def strength_start(timesteps: int, strength: float) -> int:
    """Row of the schedule an img2img run of ``strength`` begins at ([EXT] diffusers ``get_timesteps``): the last ``int(timesteps * strength)`` steps run."""
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    n_run = min(int(timesteps * strength), timesteps)
    if n_run < 1:
        raise ValueError(f"strength {strength} leaves no step of {timesteps} to run")
    return timesteps - n_run


def _is_positive_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 1


def _is_finite_real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)


def hires_start(latents: torch.Tensor, noise: torch.Tensor, scheduler, timesteps: int, strength: float):
    """The step between the two passes of a high-resolution generation -> ``(x_start, start)``: ``start = strength_start(timesteps, strength)`` and
    ``x_start = sqrt(acp[t]) * bilinear(latents -> noise's size) + sqrt(1 - acp[t]) * noise`` with ``t = timesteps[start]`` of ``scheduler`` set to
    ``timesteps`` steps - ``scheduler.add_noise`` of the upscaled latents - in one launch (``pv_resize_bilinear_affine_f32``).  ``latents`` (B, C, h, w) and
    ``noise`` (B, C, H, W) live on the HIP device; ``DenoiseLoop.reset(x_start, start)`` takes the result."""
    from .ops import Recorder, require_cuda
    start = strength_start(timesteps, float(strength))
    if latents.dim() != 4 or noise.dim() != 4 or tuple(latents.shape[:2]) != tuple(noise.shape[:2]):
        raise ValueError(f"hires_start: latents {tuple(latents.shape)} and noise {tuple(noise.shape)} are not (B, C, h, w) and (B, C, H, W)")
    require_cuda(latents, "latents")
    scheduler.set_timesteps(timesteps)
    acp = torch.from_numpy(scheduler.alphas_cumprod)[scheduler.timesteps[start:start + 1].long()].to(torch.float64)     # as scheduler.add_noise
    batch, dev = latents.shape[0], latents.device
    ca, cb = (c.float().repeat(batch).to(dev) for c in (acp.sqrt(), (1 - acp).sqrt()))
    rec = Recorder(dev)
    x_start = rec.resize_bilinear_affine(latents.detach().float().contiguous(), tuple(noise.shape[2:]), ca, noise.detach().to(dev).float().contiguous(), cb)
    rec.run()
    return x_start, start


def latent_mask(inpaint_mask: torch.Tensor, batch: int, latent_size: int):
    """``inpaint_mask`` (B or 1, 1, H, W) in [0, 1], 1 = regenerate -> (pixel mask (B, 1, H, W), latent mask (B, 1, S, S)), both fp32 in {0, 1}: binarised
    at 0.5; a latent cell is regenerated when ANY pixel of its H / S x W / S block is (a max-pool), so no masked pixel is decoded from kept latents."""
    m = inpaint_mask
    if m.dim() != 4 or m.shape[1] != 1 or m.shape[0] not in (1, batch):
        raise ValueError(f"inpaint_mask has shape {tuple(m.shape)}, expected ({batch} or 1, 1, H, W)")
    H, W = m.shape[2:]
    if H % latent_size or W % latent_size or H < latent_size or W < latent_size:
        raise ValueError(f"inpaint_mask is {H} x {W}: not a multiple of latent_size {latent_size}")
    pix = (m.detach().float().cpu() >= 0.5).float().expand(batch, 1, H, W).contiguous()
    lat = pix.reshape(batch, 1, latent_size, H // latent_size, latent_size, W // latent_size).amax(dim=(3, 5))
    return pix, lat


SAMPLERS = ("dpmsolver++", "sde-dpmsolver++")


def _scheduler_for(scheduler, sampler) -> DPMSolverMultistepScheduler:
    """infer.py:39-40 - the sampler is rebuilt from the loaded scheduler's config on every call; ``sampler`` sets its algorithm type."""
    return DPMSolverMultistepScheduler.from_config(scheduler.config, algorithm_type=sampler)


def _loop_for(unet, batch, latent_size, n_ip, steps, guidance, scheduler, training_mode=False, fusion_seed=0, inpaint=False,
              image_guidance=None, guidance_rescale=0.0, pag_scale=None, pag_layers=(), freeu=None, controlnet=None,
              conditioning_scale=1.0, kv_downsample=None) -> DenoiseLoop:
    cache = unet.__dict__.setdefault("_denoise_loops", OrderedDict())
    stochastic = bool(getattr(scheduler, "stochastic", False))      # the sampler: part of the key through the scheduler run_inference built for it
    key = (batch, latent_size, n_ip, steps, float(guidance), bool(training_mode), int(fusion_seed),
           None if image_guidance is None else float(image_guidance), float(guidance_rescale), stochastic,
           None if pag_scale is None else float(pag_scale), tuple(pag_layers), freeu, bool(inpaint))
    if controlnet is not None:       # its identity, its weights' version and the scale; without one the key is what it was
        key += (id(controlnet), controlnet.__dict__.get("_pack_version", 0), float(conditioning_scale))
    kv_kw = {}
    if kv_downsample is not None:    # (factor, method, resolved names); without it the key is what it was
        key += ("kv_downsample",) + tuple(kv_downsample)
        kv_kw = dict(kv_downsample=kv_downsample[0], kv_downsample_method=kv_downsample[1], kv_downsample_layers=kv_downsample[2])
    loop = cache.pop(key, None)
    if loop is None or loop.unet_version != unet.__dict__.get("_pack_version", 0) or getattr(loop, "controlnet", None) is not controlnet:
        loop = DenoiseLoop(unet, batch, latent_size, n_ip, steps, guidance, scheduler=scheduler, training_mode=training_mode,
                           fusion_seed=fusion_seed, inpaint=inpaint, image_guidance_scale=image_guidance, guidance_rescale=guidance_rescale,
                           stochastic=stochastic, pag_scale=pag_scale, pag_layers=tuple(pag_layers) or ("mid_block",), freeu=freeu,
                           **({} if controlnet is None else dict(controlnet=controlnet, conditioning_scale=conditioning_scale)), **kv_kw)
        loop.unet_version = unet.__dict__.get("_pack_version", 0)
    cache[key] = loop                               # most recently used last
    while len(cache) > MAX_CACHED_LOOPS:
        cache.popitem(last=False)
    return loop


def _pass_loop(grid, weights, unet, batch, latent_size, n_ip, steps, guidance, scheduler, **kw):
    """The loop of one pass: the cached ``DenoiseLoop`` itself (``grid`` None), or a ``WindowedDenoiseLoop`` over ``grid`` (``window_grid``'s tuple) around
    the cached ``DenoiseLoop`` of batch ``batch * nW`` at the window size - the same cache, keys and eviction."""
    if grid is None:
        return _loop_for(unet, batch, latent_size, n_ip, steps, guidance, scheduler, **kw)
    H, W, S, stride, oy, ox = grid
    inner = _loop_for(unet, batch * len(oy) * len(ox), S, n_ip, steps, guidance, scheduler, **kw)
    return WindowedDenoiseLoop(unet, batch, (H, W), S, n_ip, steps, guidance, window_stride=stride, window_weights=weights, inner=inner)


def run_inference(example, tokenizer, image_encoder, text_encoder, unet, text_adapter, image_adapter, vae, scheduler,
                  device, image_encoder_layers_idx, latent_size=64, guidance_scale=1, timesteps=100, token_index=0,
                  disable_tqdm=False, seed=None, from_noised_image=False, training_mode=False, *, noise=None, strength=1.0,
                  image_guidance_scale=None, guidance_rescale=0.0, sampler="dpmsolver++", sample_offset=0, pag_scale=None, pag_layers=("mid_block",),
                  freeu=None, controlnet=None, control_image=None, controlnet_conditioning_scale=1.0, kv_downsample=None,
                  kv_downsample_method="avg", kv_downsample_layers=None, hires_kv_downsample=None, window=None, window_stride=None,
                  window_weights="uniform", hires_window=None, hires_window_stride=None, inpaint_mask=None, paste_back=True,
                  hires_latent_size=None, hires_strength=0.5, hires_timesteps=None, hires_noise=None):
    """Same 11 positional + 8 keyword arguments as the reference.  ``noise`` (keyword-only, new): a caller-drawn start noise
    ``(B, C, latent, latent)`` replacing the draw of ``infer.py:52-59`` - used by the batch-sharded pipeline, which draws the
    global batch once and hands each rank its slice.

    Keyword-only, beyond the reference: ``strength`` in (0, 1] (with ``from_noised_image`` or ``inpaint_mask``): only the last
    ``int(timesteps * strength)`` steps run, from the image noised to the first of them; 1.0 is the reference's ``from_noised_image``.
    ``inpaint_mask`` (B or 1, 1, H, W) in [0, 1] at the resolution of ``example["pixel_values"]``, 1 = regenerate: starts from the noised image
    and keeps the latents outside the mask on the image's.  ``paste_back``: outside the mask the returned pixels are ``pixel_values`` themselves.

    ``hires_latent_size`` (>= ``latent_size``; None: one pass, as ever): a second pass at that size.  The first pass runs as above; its latents go through
    ``hires_start`` with ``hires_strength`` in (0, 1] of a schedule of ``hires_timesteps`` steps (None: ``timesteps``), and the last
    ``int(hires_timesteps * hires_strength)`` steps run at the large size under the same conditioning; the result is decoded at that size.
    ``hires_noise`` (B, C, hires_latent_size, hires_latent_size): the noise of the second pass; otherwise it is drawn right after the first one from the
    same generator (``seed``) or with ``torch.randn``.  Not with ``inpaint_mask`` or ``training_mode``.

    ``image_guidance_scale`` (None: one scale, as ever): the noise prediction becomes ``eps_u + image_guidance_scale (eps_m - eps_u) + guidance_scale
    (eps_c - eps_m)`` with ``eps_m`` a third forward per step under (negative prompt, image tokens of the input image) - how strongly the result keeps
    the identity and how strongly it follows the prompt are set apart.  A value equal to ``guidance_scale`` is the ordinary formula and runs the ordinary
    two-forward loop.  ``guidance_rescale`` in [0, 1] (0: off): the guided prediction of every sample is scaled by
    ``guidance_rescale * std(eps_c) / std(eps) + 1 - guidance_rescale``, against the over-saturation of high scales.  Both hold for the second pass of
    a hires run and for ``inpaint_mask``; neither combines with ``training_mode``.

    ``sampler``: ``"dpmsolver++"`` (the reference's deterministic DPM-Solver++(2M)) or ``"sde-dpmsolver++"`` (its stochastic form: fresh noise at every
    step, drawn on the device).  The noise stream's seed is ``seed`` when given, otherwise one ``torch.randint`` draw from the default CPU generator
    taken after the start-noise draws (the start noise of an unseeded call is what it was); the first pass draws from stream 0, the second pass of a
    hires run from stream 1.  ``sample_offset`` (int >= 0): the global index of this call's first sample - sample ``b`` gets the per-step noise sample
    ``sample_offset + b`` of a whole-batch call gets (``PhotoVersePipeline(shard=True)`` passes the rank's offset).  That equivalence needs ``seed``:
    unseeded, every call - every rank of a sharded run - draws a key of its own.  The kept region of an
    ``inpaint_mask`` run keeps its one static noise.  Not with ``training_mode``.

    ``pag_scale`` (None or 0: off) / ``pag_layers``: perturbed-attention guidance.  One more forward per step - the conditional one with the
    self-attention map of the chosen transformers replaced by the identity - and the prediction is pushed away from it by
    ``pag_scale * (eps_c - eps_p)``: broken structure (eyes, teeth, asymmetry) at the low guidance scales this model is driven at is repaired without
    raising ``guidance_scale``.  ``pag_layers``: name prefixes of the UNet's transformers (``"mid_block"``, ``"up_blocks.1"``,
    ``"down_blocks.0.attentions.0"``, ...) or ``"all"``; an entry that selects nothing is a ``ValueError``.  Holds for both passes of a hires run
    and combines with every keyword above except ``training_mode``.

    ``freeu`` (None: off): FreeU as ``(b1, b2, s1, s2)`` or a mapping with exactly those keys, four finite numbers (the authors' SD-1.5 values:
    ``(1.5, 1.6, 0.9, 0.2)``).  In the first two up blocks of every forward the first half of the backbone's channels is scaled by ``b1`` / ``b2`` and the
    skip connection's four lowest spatial frequencies by ``s1`` / ``s2``: more weight on the semantics, less high-frequency detail from the skips, at no
    additional forward.  ``(1, 1, 1, 1)`` is None: the plain call on the plain cached loop.  Holds for both passes of a hires run and combines with
    every keyword above except ``training_mode``.

    ``controlnet`` / ``control_image`` / ``controlnet_conditioning_scale`` (None: off; the two come together): a ``controlnet.ControlNetModel`` and its
    control image (B or 1, 3, 8 * latent_size, 8 * latent_size) in [0, 1] - a pose, edge or depth map; a single image serves the whole batch.  The
    ControlNet runs beside the UNet in every step, under the prompt and the negative prompt, and steers the layout through residuals on the UNet's skip
    connections and mid block output, times ``controlnet_conditioning_scale`` (a finite number; 0 is the plain call on the plain cached loop).  Combines
    with ``inpaint_mask``, ``strength``, ``sampler``, ``image_guidance_scale``, ``guidance_rescale``, ``pag_*`` and ``freeu``.  Not with ``training_mode``,
    and not yet with ``hires_latent_size``: the second pass needs a second conditioning embedding at its own size (a follow-up).

    ``kv_downsample`` (None: off; an int in 2 ... 8) / ``kv_downsample_method`` / ``kv_downsample_layers`` / ``hires_kv_downsample``: token downsampling
    (ToDo, Smith et al. 2024).  In the self-attention of the chosen transformers every query still attends, but to keys and values pooled by the factor
    per side of the token grid: a quarter of that layer's attention work at 2, a sixteenth at 4, no further forward, no changed weight.  The result is
    approximate.  ``kv_downsample_method``: ``"avg"`` (block means; the default here because it aliases less - the paper's own default is, as far as we
    recall, nearest-neighbour) or ``"nearest"`` (the top-left token of every block).  ``kv_downsample_layers``: None - the transformers of the
    highest-resolution level, first down block and last up block, where the token count is largest - or name prefixes / ``"all"`` as ``pag_layers``
    takes them; an entry that selects nothing is a ``ValueError``.  ``hires_kv_downsample`` (needs ``hires_latent_size``): the factor of the second pass -
    None: the same as ``kv_downsample``; 1: off in the second pass; else an int in 2 ... 8.  The intended use is an exact first pass and a pooled second
    one, where self-attention dominates: ``kv_downsample=None, hires_kv_downsample=2``.  Combines with every keyword above except ``training_mode``.

    ``window`` (None: off) / ``window_stride`` (None: ``window // 2``) / ``window_weights`` (``"uniform"``, ``"gaussian"``): windowed denoising
    (MultiDiffusion).  The first pass runs on a canvas of ``latent_size`` - then an int or an ``(H, W)`` pair, each side at least ``window`` - whose every
    step denoises the overlapping ``window x window`` crops (origins ``multidiffusion.window_origins``) as one batch, each with its own solver state,
    and sets the canvas to their weighted mean: the UNet works at the size it was trained at whatever the picture's size and aspect.  Every guidance,
    ``freeu``, ``kv_downsample``, ``controlnet`` and ``inpaint_mask`` keyword acts per window.  A rectangular canvas does not combine with
    ``inpaint_mask``, ``from_noised_image``, ``controlnet`` or ``hires_latent_size`` yet.  ``hires_window`` / ``hires_window_stride`` (need
    ``hires_latent_size``): the same for the second pass, which uses the same ``window_weights`` - there is one weights argument for both passes.  A pair
    as ``latent_size`` does not work through ``PhotoVersePipeline(..., shard=True, seed=...)``: that call draws the global batch's noise for a square
    ``latent_size`` before this function runs, so a sharded seeded call takes an int (a square canvas, windowed or not).  Neither window combines with ``sampler="sde-dpmsolver++"`` (the windows' fresh noise would
    be averaged in the overlaps) or ``training_mode``.  With both None the call is what it was: same launches, same bits."""
    grid1 = grid2 = None                                                                    # before any model is touched
    if window_weights not in WINDOW_WEIGHTS:
        raise ValueError(f"window_weights must be one of {WINDOW_WEIGHTS}, got {window_weights!r}")
    if window is None:
        if window_stride is not None:
            raise ValueError("window_stride needs window")
        if not isinstance(latent_size, numbers.Integral):
            raise ValueError(f"latent_size {latent_size!r} needs window: without it the canvas is one square plan and latent_size an int")
    else:
        grid1 = window_grid(latent_size, window, window_stride)
        if grid1[0] == grid1[1]:
            latent_size = grid1[0]
        else:
            for name, given in (("inpaint_mask", inpaint_mask is not None), ("from_noised_image", bool(from_noised_image)),
                                ("controlnet", controlnet is not None or control_image is not None), ("hires_latent_size", hires_latent_size is not None)):
                if given:
                    raise ValueError(f"a rectangular canvas ({grid1[0]} x {grid1[1]}) does not combine with {name} yet")
    if hires_window is None:
        if hires_window_stride is not None:
            raise ValueError("hires_window_stride needs hires_window")
    else:
        if hires_latent_size is None:
            raise ValueError("hires_window needs hires_latent_size")
        if not _is_positive_int(hires_latent_size):
            raise ValueError(f"hires_latent_size must be a positive int, got {hires_latent_size!r}")
        grid2 = window_grid(hires_latent_size, hires_window, hires_window_stride)
    if grid1 is not None or grid2 is not None:
        if sampler == "sde-dpmsolver++":
            raise ValueError("window / hires_window do not combine with sampler='sde-dpmsolver++': the windows' noise would be averaged in the overlaps")
        if training_mode:
            raise ValueError("window / hires_window do not combine with training_mode=True")
    if kv_downsample is not None:                                                           # before any model is touched
        check_kv_downsample_factor(kv_downsample, "kv_downsample")
    if hires_kv_downsample is not None:
        check_kv_downsample_factor(hires_kv_downsample, "hires_kv_downsample", allow_one=True)
        if hires_latent_size is None:
            raise ValueError("hires_kv_downsample needs hires_latent_size")
    if kv_downsample_method not in KV_DOWNSAMPLE_METHODS:
        raise ValueError(f"kv_downsample_method must be one of {KV_DOWNSAMPLE_METHODS}, got {kv_downsample_method!r}")
    kv1 = None if kv_downsample is None else int(kv_downsample)
    kv2 = kv1 if hires_kv_downsample is None else (None if int(hires_kv_downsample) == 1 else int(hires_kv_downsample))
    if (kv1 is not None or kv2 is not None) and training_mode:
        raise ValueError("kv_downsample does not combine with training_mode=True")
    if kv_downsample_layers is not None and not isinstance(kv_downsample_layers, str):
        try:
            kv_downsample_layers = tuple(kv_downsample_layers)
        except TypeError:
            raise ValueError(f"kv_downsample_layers must be None, a string or a sequence of strings, got {kv_downsample_layers!r}") from None
    if (controlnet is None) != (control_image is None):                                     # before any model is touched
        raise ValueError("controlnet and control_image come together: got " + ("a controlnet without a control_image" if control_image is None else "a control_image without a controlnet"))
    if not _is_finite_real(controlnet_conditioning_scale):
        raise ValueError(f"controlnet_conditioning_scale must be a finite number, got {controlnet_conditioning_scale!r}")
    if controlnet is not None:
        if not _is_positive_int(latent_size):
            raise ValueError(f"latent_size must be a positive int, got {latent_size!r}")
        side = 8 * latent_size
        if not torch.is_tensor(control_image) or control_image.dim() != 4 or tuple(control_image.shape[1:]) != (3, side, side):
            raise ValueError(f"control_image must be a (B or 1, 3, {side}, {side}) tensor (8 x latent_size), got {tuple(getattr(control_image, 'shape', ()))}")
        if float(controlnet_conditioning_scale) == 0.0:
            controlnet = control_image = None          # off: the loop without it
        elif training_mode:
            raise ValueError("controlnet does not combine with training_mode=True")
        elif hires_latent_size is not None:
            raise ValueError("controlnet does not combine with hires_latent_size yet: the second pass needs a control embedding at its own size")
    freeu = normalize_freeu(freeu)                                                          # before any model is touched
    if freeu is not None and training_mode:
        raise ValueError("freeu does not combine with training_mode=True")
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if not (isinstance(sample_offset, numbers.Integral) and not isinstance(sample_offset, bool) and 0 <= sample_offset < (1 << 32)):
        raise ValueError(f"sample_offset must be an int in [0, 2^32), got {sample_offset!r}")
    stochastic = sampler == "sde-dpmsolver++"
    if stochastic and training_mode:
        raise ValueError("sampler='sde-dpmsolver++' does not combine with training_mode=True")
    if image_guidance_scale is not None and not _is_finite_real(image_guidance_scale):      # before any model is touched
        raise ValueError(f"image_guidance_scale must be a finite number or None, got {image_guidance_scale!r}")
    if not _is_finite_real(guidance_rescale) or not 0.0 <= guidance_rescale <= 1.0:
        raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
    if training_mode and (image_guidance_scale is not None or guidance_rescale > 0):
        raise ValueError("image_guidance_scale / guidance_rescale do not combine with training_mode=True")
    if image_guidance_scale is not None and float(image_guidance_scale) == float(guidance_scale):
        image_guidance_scale = None                    # the ordinary formula: two forwards
    if pag_scale is not None and not _is_finite_real(pag_scale):                            # still before any model is touched
        raise ValueError(f"pag_scale must be a finite number or None, got {pag_scale!r}")
    if pag_scale is not None and float(pag_scale) == 0.0:
        pag_scale = None                               # off: the loop without it
    if pag_scale is not None and training_mode:
        raise ValueError("pag_scale does not combine with training_mode=True")
    # the layers resolve against the UNet's module tree (names only; no weight, no launch): an unknown entry fails here, before any model runs
    pag_names = resolve_pag_layers(unet, pag_layers) if pag_scale is not None else ()
    guide = dict(image_guidance=image_guidance_scale, guidance_rescale=float(guidance_rescale), pag_scale=pag_scale, pag_layers=pag_names, freeu=freeu)
    # (the same for the pooled layers: names only, also when no pass pools - an unknown entry is an error whatever the factors are)
    kv_names = resolve_kv_downsample_layers(unet, kv_downsample_layers) if (kv1 is not None or kv2 is not None or kv_downsample_layers is not None) else ()
    kv_pass1 = None if kv1 is None else (kv1, kv_downsample_method, kv_names)
    kv_pass2 = None if kv2 is None else (kv2, kv_downsample_method, kv_names)
    hires = hires_latent_size is not None
    if hires:                                          # before anything else: the first pass must not run for a second one that cannot
        if not _is_positive_int(hires_latent_size):
            raise ValueError(f"hires_latent_size must be a positive int, got {hires_latent_size!r}")
        if hires_latent_size < latent_size:
            raise ValueError(f"hires_latent_size {hires_latent_size} is smaller than latent_size {latent_size}: the second pass upscales")
        if inpaint_mask is not None:
            raise ValueError("hires_latent_size does not combine with inpaint_mask: the mask and the known latents would need a second resolution")
        if training_mode:
            raise ValueError("hires_latent_size does not combine with training_mode=True")
        hires_steps = timesteps if hires_timesteps is None else hires_timesteps
        if not _is_positive_int(hires_steps):
            raise ValueError(f"hires_timesteps must be a positive int, got {hires_timesteps!r}")
        try:
            strength_start(hires_steps, float(hires_strength))
        except ValueError as e:
            raise ValueError(f"hires_{e}") from None
    elif hires_noise is not None:
        raise ValueError("hires_noise needs hires_latent_size")
    if training_mode and torch.is_grad_enabled():
        # the reference back-propagates through the last denoising step (infer.py:99).  Here that differentiated call is a static
        # forward + backward plan, not a dynamic autograd graph: train.TrainStep(face_loss=..., vae=...) replays exactly this function
        # (conditioning with gradient, T - 1 steps without, the last step + decode inside the plan).  Under torch.no_grad() the FORWARD
        # semantics of the mode are available from this entry point: the last step's forwards draw the grad-mode branch fusion of every
        # cross-attention layer (attention_processor.py:413-420), on the device, inside the captured step.
        raise NotImplementedError("run_inference(training_mode=True) with autograd enabled: use photoverse_amd.train.TrainStep(face_loss=..., vae=...) - "
                                  "the differentiated form of this call - or call under torch.no_grad() for the forward semantics of the mode")
    device = torch.device(device)
    sch = _scheduler_for(scheduler, sampler)
    batch = example["pixel_values"].shape[0] if "pixel_values" in example else example["pixel_values_clip"].shape[0]

    uncond_input_ids = example.get("negative_text_input_ids", None)                      # :43-49
    if uncond_input_ids is None:
        uncond_input_ids = tokenizer([""] * batch, padding="max_length", max_length=tokenizer.model_max_length,
                                     return_tensors="pt").input_ids

    shape = (batch, unet.config.in_channels) + ((latent_size, latent_size) if grid1 is None else grid1[:2])     # :52-59 noise on CPU, then moved
    generator = None
    if noise is not None:
        if tuple(noise.shape) != shape:
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {shape}")
        noise = noise.to(device)
    elif seed is None:
        noise = torch.randn(shape).to(device)
    else:
        generator = torch.manual_seed(seed)
        noise = torch.randn(shape, generator=generator).to(device)
    if hires:
        shape2 = (batch, unet.config.in_channels, hires_latent_size, hires_latent_size)
        if hires_noise is not None:
            if tuple(hires_noise.shape) != shape2:
                raise ValueError(f"hires_noise has shape {tuple(hires_noise.shape)}, expected {shape2}")
        elif seed is None:
            hires_noise = torch.randn(shape2)
        else:
            if generator is None:                     # a caller-given first noise stands for the first draw of the seeded generator
                generator = torch.manual_seed(seed)
                torch.randn(shape, generator=generator)
            hires_noise = torch.randn(shape2, generator=generator)      # the draw that follows the first one
    if stochastic:                                    # after the start-noise draws: those are what they were
        noise_seed = int(seed) if seed is not None else int(torch.randint(0, 1 << 62, (1,)).item())

    inpaint = inpaint_mask is not None
    start = strength_start(timesteps, float(strength))
    if start and not (from_noised_image or inpaint):
        raise ValueError("strength < 1 needs an image to start from: from_noised_image=True or an inpaint_mask")
    if controlnet is not None and control_image.shape[0] not in (1, batch):
        raise ValueError(f"control_image has batch {control_image.shape[0]}, expected {batch} or 1")
    if inpaint:
        pixel_mask, lat_mask = latent_mask(inpaint_mask, batch, latent_size)
        if tuple(pixel_mask.shape[2:]) != tuple(example["pixel_values"].shape[2:]):
            raise ValueError(f"inpaint_mask is {tuple(pixel_mask.shape[2:])}, pixel_values {tuple(example['pixel_values'].shape[2:])}")
    if from_noised_image or inpaint:                                                      # :62-65
        if vae is None or not hasattr(vae, "encode"):
            raise NotImplementedError(("inpaint_mask" if inpaint else "from_noised_image") + " needs a vae with .encode (photoverse_amd.vae.AutoencoderKL)")
        latents0 = vae.encode(example["pixel_values"].to(device)).latent_dist.sample().detach() * vae.config.scaling_factor
        sch.set_timesteps(timesteps)
        start_noise = noise
        noise = sch.add_noise(latents0, start_noise, sch.timesteps[start:start + 1].repeat(latents0.shape[0]))     # :65 (start = 0)

    placeholder_idx = example["concept_placeholder_idx"].to(device)                       # :72-73
    pixel_values_clip = example["pixel_values_clip"].to(device)

    image_features = image_encoder(pixel_values_clip, output_hidden_states=True)          # :76-78
    uncond_image_features = image_encoder(torch.zeros_like(pixel_values_clip), output_hidden_states=True)
    image_embeddings = [image_features[0]] + [image_features[2][i] for i in image_encoder_layers_idx if i < len(image_features[2])]
    uncond_image_embeddings = [uncond_image_features[0]] + [uncond_image_features[2][i] for i in image_encoder_layers_idx
                                                            if i < len(uncond_image_features[2])]

    concept_text_embeddings = text_adapter(image_embeddings, token_index=token_index)     # :89-91
    encoder_hidden_states_image = image_adapter(image_embeddings, token_index=token_index)
    uncond_encoder_hidden_states_image = image_adapter(uncond_image_embeddings, token_index=token_index)

    uncond_embeddings = text_encoder({"text_input_ids": uncond_input_ids.to(device)})[0]  # :93-96
    encoder_hidden_states = text_encoder({"text_input_ids": example["text_input_ids"].to(device),
                                          "concept_text_embeddings": concept_text_embeddings,
                                          "concept_placeholder_idx": placeholder_idx})[0]

    loop = _pass_loop(grid1, window_weights, unet, batch, latent_size, encoder_hidden_states_image.shape[1], timesteps, guidance_scale, sch,     # :98-119
                      training_mode=training_mode, fusion_seed=0 if seed is None else int(seed), inpaint=inpaint, **guide,
                      controlnet=controlnet, conditioning_scale=float(controlnet_conditioning_scale), kv_downsample=kv_pass1)
    loop.set_conditioning((encoder_hidden_states, encoder_hidden_states_image), (uncond_embeddings, uncond_encoder_hidden_states_image))
    if controlnet is not None:
        loop.set_control(control_image)
    if inpaint:
        loop.set_inpaint(lat_mask.to(device), latents0, start_noise)
    if stochastic:
        loop.set_noise_stream(noise_seed, int(sample_offset), stream=0)
    loop.reset(noise, start)
    latents = loop.run().clone()

    if hires:
        # second pass: upscale + re-noise in one launch, then the tail of a fresh schedule at the large size under the same conditioning
        sch2 = _scheduler_for(scheduler, sampler)
        x_start, start2 = hires_start(latents, hires_noise.to(device), sch2, hires_steps, hires_strength)
        loop2 = _pass_loop(grid2, window_weights, unet, batch, hires_latent_size, encoder_hidden_states_image.shape[1], hires_steps, guidance_scale, sch2,
                           fusion_seed=0 if seed is None else int(seed), **guide, kv_downsample=kv_pass2)
        loop2.set_conditioning((encoder_hidden_states, encoder_hidden_states_image), (uncond_embeddings, uncond_encoder_hidden_states_image))
        if stochastic:
            loop2.set_noise_stream(noise_seed, int(sample_offset), stream=1)
        loop2.reset(x_start, start2)
        latents = loop2.run().clone()

    if vae is None:
        return latents
    from .ops import Recorder
    rec = Recorder(latents.device)                                                        # :121: 1 / scaling_factor * latents
    inv = torch.full((latents.shape[0],), 1.0 / vae.config.scaling_factor, dtype=torch.float32, device=latents.device)
    _latents = rec.affine_rows(latents.contiguous(), inv)
    rec.run()
    images = vae.decode(_latents).sample                                                  # :122-123
    if inpaint and paste_back:
        # the photograph outside the (binarised) pixel mask, the decoded result inside, and the clamp of :122 - one launch
        orig = example["pixel_values"].to(device=images.device, dtype=torch.float32).contiguous()
        if images.shape != orig.shape:
            raise ValueError(f"paste_back: the decoded images are {tuple(images.shape)}, pixel_values {tuple(orig.shape)}")
        images = images.float().contiguous()
        rec = Recorder(images.device)
        rec.composite_clamp(images, orig, pixel_mask.to(images.device), -1.0, 1.0, out=images)
        rec.run()
        return images
    if images.is_cuda and images.dtype == torch.float32 and images.is_contiguous():
        rec = Recorder(images.device)
        rec.clamp_(images, -1.0, 1.0)
        rec.run()
        return images
    return images.clamp(-1, 1)
