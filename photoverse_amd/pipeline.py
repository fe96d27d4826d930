"""Graph-captured denoising loop (the hot loop of ``/root/reference/models/infer.py:98-119``) and its batch sharding.

One denoising step = UNet(uncond) + UNet(cond) at batch B (two sequential forwards, ``infer.py:103-114``) + CFG combine
(``:116``) + ``scheduler.step`` (``:119``).  All of it is a fixed list of allocation-free launches over static buffers,
so ONE step is captured into a HIP graph and replayed ``T`` times; the per-step scalars (timestep, solver coefficients)
are read on the device through a step counter the graph itself advances.

Multi-GPU (new - the reference has none): samples are independent, so the batch is sharded over ranks
with no communication inside the loop; final latents are collected with ONE ``all_gather`` over RCCL.
"""
from __future__ import annotations

import numbers
import os
from typing import Optional, Tuple

import numpy as np
import torch

from .ops import Recorder, require_cuda
from .scheduler import DPMSolverMultistepScheduler


#: 256-row-tile threshold of plans that run beside their CFG twin (each fills half of the chip); PV_SIDE_BIG_MIN overrides it for A/Bs
_SIDE_BIG_MIN = int(os.environ.get("PV_SIDE_BIG_MIN", "128"))


#: rows (batch 2B x pixels of the first merged level) from which the low-resolution levels of the two CFG forwards run as ONE merged plan
_MERGE_MIN_ROWS = int(os.environ.get("PV_MERGE_MIN_ROWS", "8192"))


class DenoiseLoop:
    """One denoising step as launch plans over static buffers, captured into a HIP graph and replayed ``T`` times.

    What runs beside what is data: ``self.schedule`` is a tuple of groups that run one after the other; a group is a tuple of lanes that run side by
    side; a lane is a tuple of ``Recorder``s that run in order on one stream - lane 0 on the current stream, lane k on ``self._sides[k - 1]``, forked
    after the previous group and joined before the next (a group of one lane issues no stream operation).  ``_step_eager`` walks it, eagerly or under
    capture, where the lanes become the parallel branches of the graph.  Its contents, from the engine lists:

    * one single-lane group per ``engines_p`` entry, the conditioning-independent prefix (``share_prefix``);
    * with ``merge_lowres`` ``(u.rec_head | c.rec_head)``, ``(m.rec)``, ``(u.rec_tail | c.rec_tail)``: the high-resolution levels of the two CFG forwards side
      by side around the ONE plan that runs their low-resolution levels and mid block over both forwards' samples;
    * otherwise one group with a lane per whole forward, ``engines_u + engines_c + engines_i`` (each per sub-batch with ``batch_splits``); with ``pag_scale``
      a conditional lane is ``(c.rec, p.rec)``, the perturbed forward right behind the conditional one whose trunk it may share;
    * with ``controlnet``, in front of the forwards' group, ``(ctrl_u.rec | ctrl_c.rec)``: the ControlNet's plans under the uncond and the cond text, whose
      control features the forwards read - the group join is the dependency;
    * ``(tail)``: the CFG combine + solver step and the step counter's advance.

    With ``two_streams=False`` every group's lanes are concatenated, in order, into its one lane."""

    def __init__(self, unet, batch: int, latent_size: int, n_ip: int, num_steps: int, guidance_scale: float,
                 scheduler: Optional[DPMSolverMultistepScheduler] = None, n_text: int = 77, use_graph: bool = True,
                 two_streams: bool = True, batch_splits: int = 1, training_mode: bool = False, fusion_seed: int = 0,
                 merge_lowres: Optional[bool] = None, share_prefix: Optional[bool] = None, inpaint: bool = False,
                 image_guidance_scale: Optional[float] = None, guidance_rescale: float = 0.0, stochastic: bool = False,
                 pag_scale: Optional[float] = None, pag_layers=("mid_block",), share_trunk: Optional[bool] = None, freeu=None,
                 controlnet=None, conditioning_scale: float = 1.0, kv_downsample: Optional[int] = None, kv_downsample_method: str = "avg",
                 kv_downsample_layers=None):
        """``training_mode``: the reference enables grad on the LAST denoising step only (infer.py:99), where every cross-attention
        layer of both forwards then draws its branch fusion (attention_processor.py:413-420).  Here the draw runs on the device inside
        the captured step (``pv_fusion_draw`` keyed on the step counter), so the same graph serves all steps.  This is the forward semantics
        of that mode; the differentiated last step lives in ``train.TrainStep(face_loss=...)``.

        ``merge_lowres`` (default: on from 8192 rows at the first merged level; env ``PV_MERGE_LOWRES`` forces it): the two CFG forwards (infer.py:103-114) run their two highest-resolution levels
        as two parallel graph branches, but everything below (16 x 16 and 8 x 8 levels, mid block) as ONE plan over both branches' samples:
        at M = B * 256 / B * 64 rows a single branch cannot fill the chip without split-K (fp32 slabs + a reduce launch per conv) and both
        branches stream the same 29.5 MB of weights per conv.  Samples never interact inside the UNet, so the result per sample is unchanged.

        ``share_prefix`` (default: env ``PV_SHARE_PREFIX``, off - the headline metric counts two FULL forwards per step): conv_in, the first ResnetBlock and the first
        transformer block up to its self-attention never see the conditioning, so the uncond and cond forwards of a step compute them twice on
        identical inputs.  With ``share_prefix`` they are one plan whose outputs both branches start from - bit-identical latents, 2.5 % fewer
        flops per step.  Reported by ``bench.py`` as a separately labelled number.

        ``inpaint`` (beyond the reference; [EXT] diffusers' inpainting with a 4-channel UNet): the solver step of the tail becomes
        ``pv_cfg_dpm_step_masked`` - still one launch - which keeps the latents where ``mask`` is 0 on ``known`` noised with ``noise`` to the step's
        next timestep (the clean ``known`` after the last step).  The three static buffers are filled by ``set_inpaint``; a mask of ones (the
        initial content) is the plain loop.

        ``image_guidance_scale`` / ``guidance_rescale`` (beyond the reference; [EXT] the InstructPix2Pix split of classifier-free guidance and diffusers'
        ``guidance_rescale``).  At their defaults (None, 0.0) the loop is the one described above: same engines, same tail launcher.  With
        ``guidance_rescale`` in (0, 1] alone the two forwards stay as they are and the solver step of the tail becomes ``pv_cfg_dpm_step_guided``, which
        scales the guided prediction of every sample to ``rescale * std(eps_cond) / std(eps) + 1 - rescale``.  With ``image_guidance_scale`` a third
        forward (uncond text, cond image tokens -> ``eps_m``) runs per step and the prediction is
        ``eps_u + image_guidance_scale (eps_m - eps_u) + guidance_scale (eps_c - eps_m)``: the image-token branch (identity) and the prompt get a scale
        each (at equal scales the ``eps_m`` terms cancel and the launcher evaluates the two-term expression: the bits of the two-forward loop).  The third engine reads the ``text_u`` / ``ip_c`` buffers of the other two, so ``set_conditioning`` is unchanged.  In this mode the three
        forwards are three whole plans (``merge_lowres`` is off) on the main and two side streams - three parallel branches of the captured graph;
        ``share_prefix`` still applies (all three start from the one prefix plan).  Not with ``training_mode``.  ``inpaint`` goes through the same
        launcher's mask arguments.

        ``stochastic`` (beyond the reference; [EXT] diffusers' ``algorithm_type="sde-dpmsolver++"``, the "DPM++ 2M SDE" of the front ends): the
        solver step adds ``cn * z`` with fresh ``z ~ N(0, I)`` at every step.  The flag has to agree with the scheduler, whose type decides the
        coefficient table: ``stochastic=True`` needs a ``DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")``, a scheduler of that type
        needs ``stochastic=True`` - a mismatch either way is a ``ValueError``, so neither a silent deterministic run nor a table without its noise
        can happen.  The tail is then ``pv_cfg_dpm_step_stochastic`` + ``pv_step_advance`` - still two launches, ``launches_per_step`` unchanged,
        the forwards untouched.  The noise is generated inside that launch from ``self.rng`` = {seed_lo, seed_hi, sample_offset, stream} and the
        device-resident step counter (``set_noise_stream``; seed 0 until it is called), so the one captured graph serves every step, seed, start
        row and batch offset.  Combines with ``inpaint`` (the noise is added before the blend; the kept region keeps its one static noise),
        ``image_guidance_scale``, ``guidance_rescale`` and ``share_prefix``.  Not with ``training_mode``.

        ``pag_scale`` / ``pag_layers`` (beyond the reference; [EXT] perturbed-attention guidance, Ahn et al. 2024, diffusers' ``pag_scale`` /
        ``pag_applied_layers``).  None or 0 builds the loop described above: same engines, same tail launcher, same ``launches_per_step``.  Otherwise
        one more forward runs per step - the conditional one with the self-attention map of the transformers ``resolve_pag_layers(unet, pag_layers)``
        selects replaced by the identity (``UNetEngine(perturb=...)`` -> ``eps_p``) - and the prediction gains ``pag_scale * (eps_c - eps_p)``
        before the rescale: structure is repaired without a higher guidance scale.  The perturbed engines (``engines_p_attn``, one per batch split)
        read ``text_c`` / ``ip_c``, so ``set_conditioning`` is unchanged; they run on the conditional forward's stream right after it - no additional
        stream or graph branch.  ``merge_lowres`` is off in this mode, ``share_prefix`` still applies.  The tail is ``pv_cfg_dpm_step_pag`` +
        ``pv_step_advance``.  Combines with ``image_guidance_scale`` (four forwards), ``guidance_rescale``, ``inpaint`` and ``stochastic``.  Not with
        ``training_mode``.

        ``share_trunk`` (None: on whenever PAG is on): up to its first perturbed transformer the perturbed forward IS the conditional forward, so
        its plan adopts the conditional plan's activation and skip tensors there (``UNetEngine(trunk=...)``) and records only the rest - with the
        default layer, the mid block, the whole down path.  Same kernels on the same inputs: the bits of ``share_trunk=False``, which records the
        whole perturbed forward.

        ``freeu`` (beyond the reference; [EXT] FreeU, Si et al. 2024, diffusers' ``enable_freeu``): None, ``(b1, b2, s1, s2)`` or a mapping with those
        keys (``unet.normalize_freeu``; all ones is None).  Every engine of the step is built with it (``UNetEngine(freeu=...)``) - uncond, cond,
        image-only, merged low-resolution part, prefix, perturbed: all forwards of a step see the same UNet - and records one ``pv_freeu_rows`` launch
        per ResnetBlock of the first two up blocks.  No further forward, stream or buffer; the tail is untouched.  None builds the loop described
        above, launch for launch.  Combines with every mode above except ``training_mode``.

        ``controlnet`` / ``conditioning_scale`` (beyond the reference; [EXT] ControlNet, diffusers' ``StableDiffusionControlNetPipeline``): a
        ``controlnet.ControlNetModel`` on the UNet's device.  None, or a scale of 0, builds the loop described above, launch for launch.  Otherwise two
        control plans per sub-batch (``engines_ctrl_u`` / ``engines_ctrl_c``: the ControlNet under ``text_u`` / ``text_c``) run per step in a group of
        their own in front of the forwards, and every forward is built with ``UNetEngine(control=..., control_scale=conditioning_scale)``: uncond and
        image-only forwards read the uncond control features, cond and perturbed forwards the cond ones (the ControlNet is not perturbed).  The
        conditioning embedding of the control image (``hint_emb``, static fp16 [B * S * S][c0]) is computed once per generation by ``set_control``,
        outside the captured step; it is zero until then.  ``merge_lowres`` is off in this mode, ``share_prefix`` still applies to the UNet plans.
        Combines with every mode above except ``training_mode``.

        ``kv_downsample`` / ``kv_downsample_method`` / ``kv_downsample_layers`` (beyond the reference; [EXT] token downsampling, ToDo, Smith et al. 2024):
        None builds the loop described above, launch for launch.  An int ``f`` in 2 ... 8: in the self-attention of the transformers
        ``resolve_kv_downsample_layers(unet, kv_downsample_layers)`` selects (None: those of the highest-resolution level) every query still attends, but
        the keys and values are the token grid pooled ``f`` per side (``"avg"``: block means, the default - it aliases less; ``"nearest"``: the top-left
        token) - ``f * f`` times fewer score and P.V flops there, approximate, no weights changed.  Every engine of the step is built with it
        (``UNetEngine(kv_downsample=...)``) - uncond, cond, image-only, merged low-resolution part, prefix, perturbed, both control plans: all forwards of
        a step see the same UNet.  ``launches_per_step`` rises by one ``pv_token_pool`` per selected, unperturbed transformer per plan that records its
        attn1; ``merge_lowres``, ``share_prefix`` and ``share_trunk`` keep their rules.  Combines with every mode above except ``training_mode``."""
        import math
        from .unet import KV_DOWNSAMPLE_METHODS, check_kv_downsample_factor, resolve_kv_downsample_layers
        if kv_downsample is not None:                        # host-side, before the UNet is touched
            check_kv_downsample_factor(kv_downsample)
            if training_mode:
                raise ValueError("kv_downsample does not combine with training_mode=True")
        if kv_downsample_method not in KV_DOWNSAMPLE_METHODS:
            raise ValueError(f"kv_downsample_method must be one of {KV_DOWNSAMPLE_METHODS}, got {kv_downsample_method!r}")
        #: what every engine of the step is built with: None, or (factor, method, transformer names)
        self.kv_downsample = None if kv_downsample is None else (int(kv_downsample), kv_downsample_method,
                                                                  resolve_kv_downsample_layers(unet, kv_downsample_layers))
        if not (isinstance(conditioning_scale, numbers.Real) and not isinstance(conditioning_scale, bool) and math.isfinite(conditioning_scale)):
            raise ValueError(f"conditioning_scale must be a finite number, got {conditioning_scale!r}")
        self.conditioning_scale = float(conditioning_scale)
        self.controlnet = controlnet if (controlnet is not None and self.conditioning_scale != 0.0) else None
        ctrl = self.controlnet is not None
        if ctrl and training_mode:
            raise ValueError("controlnet does not combine with training_mode=True")
        from .unet import normalize_freeu
        self.freeu = normalize_freeu(freeu)                  # host-side, before the UNet is touched
        if self.freeu is not None and training_mode:
            raise ValueError("freeu does not combine with training_mode=True")
        dev = unet.device
        if dev.type != "cuda":
            raise RuntimeError("DenoiseLoop needs the UNet on a HIP device (no CPU path)")
        self.unet, self.B, self.S, self.P, self.T = unet, batch, latent_size, n_ip, num_steps
        self.guidance = float(guidance_scale)
        self.training_mode = bool(training_mode)
        self.image_guidance = None if image_guidance_scale is None else float(image_guidance_scale)
        self.guidance_rescale = float(guidance_rescale)
        if not 0.0 <= self.guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {guidance_rescale}")
        three = self.image_guidance is not None
        if three and training_mode:
            raise ValueError("image_guidance_scale does not combine with training_mode=True")
        if pag_scale is not None and not (isinstance(pag_scale, numbers.Real) and not isinstance(pag_scale, bool) and np.isfinite(float(pag_scale))):
            raise ValueError(f"pag_scale must be a finite number or None, got {pag_scale!r}")
        self.pag_scale = 0.0 if pag_scale is None else float(pag_scale)
        pag = self.pag_scale != 0.0
        if pag and training_mode:
            raise ValueError("pag_scale does not combine with training_mode=True")
        from .unet import resolve_pag_layers
        self.pag_layers = resolve_pag_layers(unet, pag_layers) if pag else ()
        self.share_trunk = bool(pag and (share_trunk is None or share_trunk))
        self.stochastic = bool(stochastic)
        if self.stochastic and training_mode:
            raise ValueError("stochastic=True does not combine with training_mode=True")
        if scheduler is None:
            sch = DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++" if self.stochastic else "dpmsolver++")
        else:
            sch = scheduler
            if bool(getattr(sch, "stochastic", False)) != self.stochastic:
                raise ValueError(f"stochastic={self.stochastic} does not agree with the scheduler ({type(sch).__name__}, algorithm_type "
                                 f"{getattr(sch, 'config', {}).get('algorithm_type')!r}): the stochastic loop needs "
                                 "DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++'), every other scheduler stochastic=False")
        sch.set_timesteps(num_steps)
        self.scheduler = sch
        cfg = unet.config
        xdim = cfg.cross_attention_dim
        f32, f16 = torch.float32, torch.float16
        self.latents = torch.zeros((batch, cfg.in_channels, latent_size, latent_size), dtype=f32, device=dev)
        self.x0_prev = torch.zeros_like(self.latents)
        self.timesteps = sch.timesteps.to(device=dev, dtype=f32)
        self.inpaint = bool(inpaint)
        self._start = 0
        self.coef = sch.coefficient_table(0, blend=self.inpaint).to(dev)
        self.state = torch.tensor([0, num_steps, 0, 0], dtype=torch.int32, device=dev)   # {step index, table rows, -, -}
        self._state0 = self.state.clone()
        self._host_step = 0
        self.text_c = torch.zeros((batch * n_text, xdim), dtype=f16, device=dev)
        self.text_u = torch.zeros_like(self.text_c)
        self.ip_c = torch.zeros((batch * n_ip, xdim), dtype=f16, device=dev)
        self.ip_u = torch.zeros_like(self.ip_c)
        self.two_streams = two_streams
        # Engines: one per (CFG branch, sub-batch).  batch_splits > 1 cuts each forward into independent sub-batches (samples
        # never interact inside the UNet) that run as additional parallel graph branches.
        if batch % batch_splits:
            raise ValueError("batch_splits must divide the batch")
        sb = batch // batch_splits
        self.eps_u = torch.empty_like(self.latents)
        self.eps_c = torch.empty_like(self.latents)
        self.eps_m = torch.empty_like(self.latents) if three else None      # eps(uncond text, cond image tokens)
        self.eps_p = torch.empty_like(self.latents) if pag else None        # eps(cond) with perturbed self-attention
        self.engines_u, self.engines_c, self.engines_m, self.engines_p, self.engines_i, self.engines_p_attn = [], [], [], [], [], []
        self.engines_ctrl_u, self.engines_ctrl_c = [], []
        if share_prefix is None:
            share_prefix = os.environ.get("PV_SHARE_PREFIX", "0") == "1"
        first = unet.down_blocks[0]
        self.share_prefix = bool(share_prefix and not training_mode and batch_splits == 1 and getattr(first, "has_attn", False) and len(first.resnets) >= 1)
        pre_kw = {}
        if self.share_prefix:
            self.engines_p.append(unet.engine(batch, latent_size, latent_size, n_ip, 1, latents_in=self.latents, segment="prefix", timesteps=self.timesteps,
                                              state=self.state, n_text=n_text, freeu=self.freeu, kv_downsample=self.kv_downsample))
            pre_kw = dict(prefix=self.engines_p[0].prefix_out)
        n_lv = len(cfg.block_out_channels)
        split = int(os.environ.get("PV_MERGE_SPLIT", "2"))     # resolution levels that stay in the per-branch plans (A/B switch; 3 = only 8 x 8 + mid merged)
        if merge_lowres is None:
            # default: merge where the merged plan, which runs ALONE on the chip, can fill it - from 8192 rows at its first level (batch 2B) on: the headline
            # (2 x 16 x 256 rows) merges (+ round 4); configs[4]'s per-rank shape (2 x 4 x 576 = 4608 rows) is 4.8 % of a step faster with its two
            # low-resolution plans side by side on the two streams (round 6, profiles/r06_loop_ab_cfg4_env.txt).  PV_MERGE_LOWRES=1 / 0 forces it.
            env = os.environ.get("PV_MERGE_LOWRES")
            rows = 2 * batch * (latent_size >> split) ** 2
            # (... and at the launch-bound end, up to 1024 rows - bs = 1 / 2 at 64 x 64 latents - the merged plan's fewer launches win again: +1.0 % / +0.4 %)
            merge_lowres = (env != "0") if env is not None else (rows >= _MERGE_MIN_ROWS or rows <= 1024)
        self.merge_lowres = bool(merge_lowres and not training_mode and not three and not pag and not ctrl and batch_splits == 1 and n_lv > split
                                 and ((latent_size >> split) ** 2) % 64 == 0 and latent_size % (1 << (n_lv - 1)) == 0)
        if self.merge_lowres:
            # text / image-token buffers of the two branches are the halves of ONE buffer: the merged plan reads it whole
            text_all = torch.zeros((2 * batch * n_text, xdim), dtype=f16, device=dev)
            ip_all = torch.zeros((2 * batch * n_ip, xdim), dtype=f16, device=dev)
            self.text_u, self.text_c = text_all[:batch * n_text], text_all[batch * n_text:]
            self.ip_u, self.ip_c = ip_all[:batch * n_ip], ip_all[batch * n_ip:]
            boc = cfg.block_out_channels
            n_in, n_out = (latent_size >> split) ** 2, (latent_size >> (split - 1)) ** 2       # pixels per sample at the two seams
            c_in, c_out = boc[split - 1], boc[split]           # downsampler of level split-1 keeps its width; upsampler of the first merged up block
            mid_in = torch.empty((2 * batch * n_in, c_in), dtype=f16, device=dev)
            mid_in_cs = torch.zeros((2 * batch * n_in // 64, 2, c_in), dtype=f32, device=dev)
            mid_out = torch.empty((2 * batch * n_out, c_out), dtype=f16, device=dev)
            mid_out_cs = torch.zeros((2 * batch * n_out // 64, 2, c_out), dtype=f32, device=dev)
            kw = dict(timesteps=self.timesteps, state=self.state, n_text=n_text, split=split, freeu=self.freeu, kv_downsample=self.kv_downsample)
            side_by_side = dict(big_min=_SIDE_BIG_MIN) if two_streams else {}      # heads / tails of the two branches run concurrently: half the chip each
            for i, (text, ip, eps, lst) in enumerate(((self.text_u, self.ip_u, self.eps_u, self.engines_u), (self.text_c, self.ip_c, self.eps_c, self.engines_c))):
                half_in = (mid_in[i * batch * n_in:(i + 1) * batch * n_in], mid_in_cs[i * batch * n_in // 64:(i + 1) * batch * n_in // 64])
                half_out = (mid_out[i * batch * n_out:(i + 1) * batch * n_out], mid_out_cs[i * batch * n_out // 64:(i + 1) * batch * n_out // 64])
                lst.append(unet.engine(batch, latent_size, latent_size, n_ip, 1, latents_in=self.latents, text=text, ip=ip, out=eps, segment="outer",
                                       mid_in=half_in, mid_out=half_out, **kw, **side_by_side, **pre_kw))
            self.engines_m.append(unet.engine(2 * batch, latent_size, latent_size, n_ip, 1, text=text_all, ip=ip_all, segment="mid",
                                              mid_in=(mid_in, mid_in_cs), mid_out=(mid_out, mid_out_cs), **kw))

        def engine(i, text, ip, out, **kw):
            """the plan of sub-batch ``i`` of one forward: on its rows of the text and image-token buffers it reads and of the prediction it writes"""
            return unet.engine(sb, latent_size, latent_size, n_ip, 1, text=text[i * sb * n_text:(i + 1) * sb * n_text],
                               ip=ip[i * sb * n_ip:(i + 1) * sb * n_ip], out=out[i * sb:(i + 1) * sb], **kw)

        if ctrl:
            if controlnet.device != dev or tuple(controlnet.config.block_out_channels) != tuple(cfg.block_out_channels):
                raise ValueError("controlnet must live on the UNet's device and have its block_out_channels")
            from .controlnet import hint_plan
            c0 = cfg.block_out_channels[0]
            self.control_image = torch.zeros((batch, controlnet.config.conditioning_channels, 8 * latent_size, 8 * latent_size), dtype=f32, device=dev)
            self.hint_emb = torch.zeros((batch * latent_size * latent_size, c0), dtype=f16, device=dev)
            self.hint_rec = Recorder(dev)                           # once per generation (set_control), outside the captured step
            hint_plan(self.hint_rec, controlnet.controlnet_cond_embedding, self.control_image, self.hint_emb)
        for i in range(0 if self.merge_lowres else batch_splits):
            kw = dict(timesteps=self.timesteps, state=self.state, latents_in=self.latents[i * sb:(i + 1) * sb], n_text=n_text, freeu=self.freeu, kv_downsample=self.kv_downsample, **pre_kw)
            if two_streams and batch_splits == 1:
                kw.update(big_min=_SIDE_BIG_MIN)                    # the two whole forwards run side by side
            ctl_u = ctl_c = {}
            if ctrl:
                rows = latent_size * latent_size
                ckw = {k: v for k, v in kw.items() if k in ("timesteps", "state", "latents_in", "n_text", "big_min", "kv_downsample")}
                for text, lst in ((self.text_u, self.engines_ctrl_u), (self.text_c, self.engines_ctrl_c)):
                    # (the image-token buffer is only a shape here: the ControlNet's cross-attention is text-only, its image-token K / V weights are zero)
                    lst.append(controlnet.control_engine(sb, latent_size, latent_size, n_ip, self.hint_emb[i * sb * rows:(i + 1) * sb * rows],
                                                         text=text[i * sb * n_text:(i + 1) * sb * n_text], ip=self.ip_c[i * sb * n_ip:(i + 1) * sb * n_ip], **ckw))
                ctl_u = dict(control=self.engines_ctrl_u[i], control_scale=self.conditioning_scale)
                ctl_c = dict(control=self.engines_ctrl_c[i], control_scale=self.conditioning_scale)
            if training_mode:
                kw.update(device_fusion="last_step")
            fs = dict(fusion_seed=fusion_seed * 4096 + 2 * i) if training_mode else {}
            fs2 = dict(fusion_seed=fusion_seed * 4096 + 2 * i + 1) if training_mode else {}
            self.engines_u.append(engine(i, self.text_u, self.ip_u, self.eps_u, **kw, **fs, **ctl_u))
            self.engines_c.append(engine(i, self.text_c, self.ip_c, self.eps_c, **kw, **fs2, **ctl_c))
            if three:
                self.engines_i.append(engine(i, self.text_u, self.ip_c, self.eps_m, **kw, **ctl_u))     # uncond text: the uncond control features
            if pag:
                kwp = dict(kw, **ctl_c)                             # the perturbed forward reads the conditional control features
                if self.share_trunk:
                    kwp.update(trunk=self.engines_c[i])             # starts from the conditional plan's tensors (the prefix, if any, lies inside them)
                elif "down_blocks.0.attentions.0" in self.pag_layers:
                    kwp.pop("prefix", None)                         # the prefix holds that transformer's UNperturbed attn1
                self.engines_p_attn.append(engine(i, self.text_c, self.ip_c, self.eps_p, perturb=self.pag_layers, **kwp))
        self.eng_u, self.eng_c = self.engines_u[0], self.engines_c[0]
        self.tail = Recorder(dev)
        mask = known = noise = rng = None                 # static buffers only the loops of these modes have
        if self.inpaint:
            mask = self.mask = torch.ones((batch, 1, latent_size, latent_size), dtype=f32, device=dev)
            known = self.known = torch.zeros_like(self.latents)
            noise = self.noise = torch.zeros_like(self.latents)
        if self.stochastic:
            rng = self.rng = torch.zeros(4, dtype=torch.int32, device=dev)     # {seed_lo, seed_hi, sample_offset, stream} as uint32 bit patterns: set_noise_stream
        self.tail.solver_step(self.eps_u, self.eps_c, self.latents, self.x0_prev, self.coef, self.state, self.guidance, eps_i=self.eps_m, eps_p=self.eps_p,
                              g_image=self.image_guidance, g_pag=self.pag_scale, rescale=self.guidance_rescale, rng=rng, mask=mask, known=known, noise=noise)
        self.tail.step_advance(self.state)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.use_graph = use_graph
        self.two_streams = two_streams
        n_side = ((3 if three else 2) * batch_splits - 1) if two_streams else 0
        self._sides = [torch.cuda.Stream(device=dev) for _ in range(n_side)]
        self.launches_per_step = sum(len(e.rec) for e in self.all_engines) + len(self.tail)
        # the step (class docstring): groups one after the other, a group's lanes side by side, a lane's recorders in order.  Recorders only
        groups = [((e.rec,),) for e in self.engines_p]                   # the conditioning-independent prefix all forwards start from (share_prefix)
        if self.merge_lowres:
            (eu,), (ec,), (em,) = self.engines_u, self.engines_c, self.engines_m
            groups += [((eu.rec_head,), (ec.rec_head,)), ((em.rec,),), ((eu.rec_tail,), (ec.rec_tail,))]
        else:
            if ctrl:
                groups.append(tuple((e.rec,) for e in self.engines_ctrl_u + self.engines_ctrl_c))
            # a lane per whole forward; the perturbed forward runs in its conditional forward's lane, right behind it (whose trunk it may share)
            after = self._after_cond()
            groups.append(tuple((e.rec, after[id(e)].rec) if id(e) in after else (e.rec,) for e in self.engines_u + self.engines_c + self.engines_i))
        groups.append(((self.tail,),))
        if not two_streams:
            groups = [(sum(lanes, ()),) for lanes in groups]
        self.schedule = tuple(groups)

    @property
    def all_engines(self):
        """Every plan of a step (uncond / cond branches, with ``merge_lowres`` the merged low-resolution part, with ``image_guidance_scale`` the
        image-only branch, with ``pag_scale`` the perturbed branch)."""
        return self.engines_u + self.engines_c + self.engines_m + self.engines_p + self.engines_i + self.engines_p_attn + self.engines_ctrl_u + self.engines_ctrl_c

    # ------------------------------------------------------------------
    def set_conditioning(self, cond: Tuple[torch.Tensor, torch.Tensor], uncond: Tuple[torch.Tensor, torch.Tensor]):
        """cond / uncond = (text (B,77,768), ip (B,P,768)) - the tuples of ``infer.py:106,113``."""
        for (text, ip), (dt, di) in ((cond, (self.text_c, self.ip_c)), (uncond, (self.text_u, self.ip_u))):
            require_cuda(text, "text embeddings")
            dt.copy_(text.reshape(dt.shape))
            di.copy_(ip.reshape(di.shape))
        # K/V projections of the conditioning: once per generation, outside the per-step graph
        for e in self.all_engines:
            e.run_conditioning()

    def set_inpaint(self, mask: torch.Tensor, known: torch.Tensor, noise: torch.Tensor):
        """Fill the static buffers of an ``inpaint`` loop: ``mask`` (B or 1, 1, S, S), 1 = regenerate; ``known`` (B, C, S, S) the latents to keep;
        ``noise`` (B, C, S, S) the noise they are re-noised with at every step.  Contents only: the captured graph stays valid."""
        if not self.inpaint:
            raise RuntimeError("DenoiseLoop.set_inpaint(): the loop was built without inpaint=True")
        for src, dst, what in ((mask, self.mask, "mask"), (known, self.known, "known latents"), (noise, self.noise, "noise")):
            require_cuda(src, what)
            dst.copy_(src.to(torch.float32).expand(dst.shape))

    def set_control(self, control_image: torch.Tensor):
        """The control image of a ``controlnet`` loop: (B or 1, 3, 8 S, 8 S), values in [0, 1]; a single image is broadcast over the batch.  Runs the hint
        plan - seven ``pv_hint_conv3x3`` launches and one ``pv_gemm_conv`` - once, into the static ``hint_emb`` the control plans read.  Contents only: the
        captured graph stays valid."""
        if self.controlnet is None:
            raise RuntimeError("DenoiseLoop.set_control(): the loop was built without a controlnet (or with conditioning_scale=0)")
        want = tuple(self.control_image.shape)
        if not torch.is_tensor(control_image) or control_image.dim() != 4 or tuple(control_image.shape[1:]) != want[1:] or control_image.shape[0] not in (1, want[0]):
            raise ValueError(f"control_image has shape {tuple(getattr(control_image, 'shape', ()))}, expected ({want[0]} or 1, {want[1]}, {want[2]}, {want[3]})")
        self.control_image.copy_(control_image.to(device=self.control_image.device, dtype=torch.float32).expand(want))
        self.hint_rec.run()

    def set_noise_stream(self, seed: int, sample_offset: int = 0, stream: int = 0):
        """The noise of a ``stochastic`` loop: ``seed`` (taken modulo 2^64) is the Philox key, ``sample_offset`` the global index of this loop's first
        sample (sample ``b`` draws what sample 0 draws at ``sample_offset + b``: a rank's shard of a batch gets the noise of the one-GPU run),
        ``stream`` tells apart the loops of one generation (the two passes of a hires run).  Contents only: the captured graph stays valid."""
        if not self.stochastic:
            raise RuntimeError("DenoiseLoop.set_noise_stream(): the loop was built without stochastic=True")
        seed = int(seed) % (1 << 64)
        if not (0 <= int(sample_offset) < (1 << 32) and 0 <= int(stream) < (1 << 32)):
            raise ValueError(f"sample_offset and stream must be in [0, 2^32), got {sample_offset}, {stream}")
        words = np.array([seed & 0xFFFFFFFF, seed >> 32, int(sample_offset), int(stream)], dtype=np.uint32).view(np.int32)
        self.rng.copy_(torch.from_numpy(words.copy()))

    def reset(self, noise: torch.Tensor, start: int = 0):
        """latents = noise * init_noise_sigma (``infer.py:70``); step counter to ``start`` (0: the whole schedule; > 0: the last ``T - start`` steps
        of it, ``noise`` then being latents already at ``timesteps[start]``'s noise level).  The noise stream of a ``stochastic`` loop is not
        touched: its draws are keyed on the absolute step, so the same stream gives the same run again."""
        start = int(start)
        if not 0 <= start < self.T:
            raise ValueError(f"DenoiseLoop.reset(): start {start} is outside the schedule of {self.T} steps")
        if start != self._start:
            # the row the loop begins at has no history: it is the table's first-order row.  Same buffer, so a captured graph keeps reading it
            self.coef.copy_(self.scheduler.coefficient_table(start, blend=self.inpaint))
            self._start = start
        self.latents.copy_(noise.to(self.latents.device) * self.scheduler.init_noise_sigma)
        self.x0_prev.zero_()
        self.state.copy_(self._state0 if start == 0 else torch.tensor([start, self.T, 0, 0], dtype=torch.int32))
        self._host_step = start

    def _step_eager(self):
        """One step, as ``self.schedule`` spells it.  A group of several lanes forks lanes 1.. onto the side streams (parallel branches of the captured
        graph, so the small low-resolution launches of one forward overlap the others') and joins them before the next group starts."""
        main = torch.cuda.current_stream()
        for lanes in self.schedule:
            sides = self._sides[:len(lanes) - 1]
            for side, lane in zip(sides, lanes[1:]):
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    for rec in lane:
                        rec.run()
            for rec in lanes[0]:
                rec.run()
            for side in sides:
                main.wait_stream(side)

    def _after_cond(self):
        """conditional engine -> the perturbed engine that follows it in its lane (``pag_scale``; empty otherwise)"""
        return {id(c): p for c, p in zip(self.engines_c, self.engines_p_attn)}

    def capture(self):
        """Capture one step into a HIP graph.  The capture itself does not execute the step."""
        if self.graph is not None:
            return
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=self.latents.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):      # warm the kernels (lazy module load, hipFuncSetAttribute) outside capture
            keep = (self.latents.clone(), self.x0_prev.clone(), self.state.clone())
            self._step_eager()
            self.latents.copy_(keep[0]); self.x0_prev.copy_(keep[1]); self.state.copy_(keep[2])
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_eager()
        self.graph = g

    def step(self):
        # the device tables have T rows: a step past the end of the schedule is a caller bug (the kernels clamp the index, so it
        # could not read out of bounds, but the result would be meaningless)
        if self._host_step >= self.T:
            raise RuntimeError(f"DenoiseLoop.step(): all {self.T} steps of the schedule have run; call reset() first")
        self._host_step += 1
        if self.use_graph:
            if self.graph is None:
                self.capture()
            self.graph.replay()
        else:
            self._step_eager()

    def run(self, steps: Optional[int] = None) -> torch.Tensor:
        for _ in range(self.T - self._start if steps is None else steps):
            self.step()
        return self.latents


def shard_batch(total: int, rank: int, world: int) -> slice:
    """Contiguous, even split of the global batch (ranks must divide it)."""
    if total % world:
        raise ValueError(f"global batch {total} is not divisible by world size {world}")
    per = total // world
    return slice(rank * per, (rank + 1) * per)


def gather_latents(local: torch.Tensor, world: int, force: bool = False) -> torch.Tensor:
    """The single collective of the multi-GPU path: all_gather of the final latents (RCCL over xGMI on GPUs,
    gloo in the CPU tests).  Rank order == batch order, so the result equals the 1-GPU run sample for sample."""
    import torch.distributed as dist
    if world == 1 and not force:
        return local
    src = local.contiguous()
    if src.is_cuda and dist.get_backend() == "gloo":     # gloo has no device all_gather (tests on a 1-GPU box): stage through the host
        src = src.cpu()
    out = torch.empty((world * src.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    dist.all_gather_into_tensor(out, src)
    return out.to(local.device)


class PhotoVersePipeline:
    """Convenience bundle named in the task text (the reference itself has no such class): holds what
    ``load_models`` returns and calls ``run_inference`` - optionally sharding the batch over the ranks of an initialised
    ``torch.distributed`` process group and gathering the final latents with one collective."""

    def __init__(self, tokenizer, text_encoder, vae, unet, image_encoder, image_adapter, text_adapter, scheduler, lora_config=None):
        self.tokenizer, self.text_encoder, self.vae, self.unet = tokenizer, text_encoder, vae, unet
        self.image_encoder, self.image_adapter, self.text_adapter = image_encoder, image_adapter, text_adapter
        self.scheduler, self.lora_config = scheduler, lora_config
        self.device = torch.device("cpu")

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, extra_num_tokens=4, photoverse_path=None, **kw):
        from .modeling_utils import load_models
        return cls(*load_models(pretrained_model_name_or_path, extra_num_tokens, photoverse_path, **kw))

    def to(self, device):
        self.device = torch.device(device)
        for m in (self.unet, self.vae, self.text_encoder, self.image_encoder, self.image_adapter, self.text_adapter):
            if m is not None:
                m.to(self.device)
        return self

    @torch.no_grad()
    def __call__(self, example, image_encoder_layers_idx=(4, 8, 12, 16), shard: bool = False, **kw):
        from .infer import run_inference
        if shard:
            import torch.distributed as dist
            rank, world = dist.get_rank(), dist.get_world_size()
            n = example["pixel_values_clip"].shape[0]
            sl = shard_batch(n, rank, world)
            local = {k: (v[sl] if torch.is_tensor(v) and v.shape[:1] == (n,) else v) for k, v in example.items()}
            if torch.is_tensor(kw.get("inpaint_mask")) and kw["inpaint_mask"].shape[:1] == (n,):
                kw["inpaint_mask"] = kw["inpaint_mask"][sl]                      # a per-sample mask goes with its samples; a (1, ...) mask is shared
            if torch.is_tensor(kw.get("control_image")) and kw["control_image"].shape[:1] == (n,) and n != 1:
                kw["control_image"] = kw["control_image"][sl]                    # likewise a per-sample control image
            if kw.get("seed") is not None:
                # the noise of the GLOBAL batch is drawn once with the reference's generator semantics (infer.py:52-59: CPU global
                # generator) on every rank and sliced, so sample i equals sample i of the seeded 1-GPU run
                latent_size = kw.get("latent_size", 64)
                generator = torch.manual_seed(kw["seed"])
                kw["noise"] = torch.randn((n, self.unet.config.in_channels, latent_size, latent_size), generator=generator)[sl]
                if kw.get("hires_latent_size") is not None and kw.get("hires_noise") is None:
                    # the second pass's noise is the NEXT draw of that generator over the global batch, as in the seeded 1-GPU run
                    s2 = kw["hires_latent_size"]
                    kw["hires_noise"] = torch.randn((n, self.unet.config.in_channels, s2, s2), generator=generator)[sl]
            # the stochastic sampler's per-step noise is keyed on the GLOBAL sample index: with ``seed`` sample i of the sharded run gets the noise of
            # sample i of the 1-GPU run (unseeded, every rank draws a stream key of its own: the ranks' noises are unrelated, as their start noises are)
            kw["sample_offset"] = sl.start
            out = run_inference(local, self.tokenizer, self.image_encoder, self.text_encoder, self.unet, self.text_adapter,
                                self.image_adapter, self.vae, self.scheduler, self.device, list(image_encoder_layers_idx), **kw)
            return gather_latents(out, world, force=True)
        return run_inference(example, self.tokenizer, self.image_encoder, self.text_encoder, self.unet, self.text_adapter,
                             self.image_adapter, self.vae, self.scheduler, self.device, list(image_encoder_layers_idx), **kw)
