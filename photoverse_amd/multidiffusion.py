"""[EXT] Windowed denoising over a latent canvas of any height and width: MultiDiffusion (Bar-Tal et al., ICML 2023; diffusers'
``StableDiffusionPanoramaPipeline``, the "Tiled Diffusion" of the front ends).

Every step denoises overlapping ``window x window`` crops of the canvas - the size the UNet was trained at and the kernels here are tuned for - each
with its own solver state, and the canvas is then set to the weighted mean of the windows' results:

    for each step:   windows = gather(canvas)              pv_window_gather   (B * nW, C, S, S), window k = ky * nx + kx of sample b in row b * nW + k
                     windows = inner.step(windows)         an ordinary, unchanged ``DenoiseLoop`` of batch B * nW: engines + solver step, one graph replay;
                                                           its ``x0_prev`` rows are the per-window scheduler states
                     canvas  = blend(windows)              pv_window_blend    sum_k w_k windows_k / sum_k w_k per element

The UNet only ever sees windows, so nothing inside the captured step knows about the canvas: ``pipeline.py`` and ``unet.py`` are untouched, and the two
launches run eagerly around the replay.  Weights: ``"uniform"`` (MultiDiffusion, diffusers' panorama pipeline: the plain mean) or ``"gaussian"``
([EXT] the window weight of Mixture of Diffusers, Jimenez 2023, restated from the published method - parity unpinned).
"""
from __future__ import annotations

import numbers
from typing import Optional

import torch

from .ops import window_blend, window_gather
from .pipeline import DenoiseLoop

#: windows per axis the launchers take
MAX_WINDOWS_PER_AXIS = 64
WINDOW_WEIGHTS = ("uniform", "gaussian")


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def window_origins(size, window, stride) -> tuple:
    """Origins of the windows of one axis: ``range(0, size - window + 1, stride)``, plus ``size - window`` where the last of those would stop short of the
    end (a clamped last window: it overlaps its neighbour by more than the others).  ``1 <= stride <= window <= size``, ints, at most 64 origins."""
    if not (_is_int(size) and _is_int(window) and _is_int(stride)):
        raise ValueError(f"window_origins: size, window and stride must be ints, got {size!r}, {window!r}, {stride!r}")
    size, window, stride = int(size), int(window), int(stride)
    if not 1 <= stride <= window <= size:
        raise ValueError(f"window_origins needs 1 <= stride <= window <= size, got stride {stride}, window {window}, size {size}")
    if -(-(size - window) // stride) + 1 > MAX_WINDOWS_PER_AXIS:                  # ceil: the clamped last window counts
        raise ValueError(f"window_origins: more than {MAX_WINDOWS_PER_AXIS} windows along an axis of {size} (window {window}, stride {stride})")
    origins = list(range(0, size - window + 1, stride))
    if origins[-1] + window < size:
        origins.append(size - window)
    return tuple(origins)


def window_profile(kind, window) -> torch.Tensor:
    """The 1-D weight profile of a window, fp32 ``[window]`` on the CPU; a window's 2-D weight is the outer product of the profile with itself.
    ``"uniform"``: ones.  ``"gaussian"`` ([EXT] Mixture of Diffusers; parity unpinned): ``exp(-((i - (S - 1) / 2) / S)^2 / 0.02)`` evaluated in
    float64 - variance 0.01 in units of the window, strictly positive in fp32 for every window size (the smallest value is about exp(-12.5))."""
    if kind not in WINDOW_WEIGHTS:
        raise ValueError(f"window_weights must be one of {WINDOW_WEIGHTS}, got {kind!r}")
    if not (_is_int(window) and window >= 1):
        raise ValueError(f"window must be a positive int, got {window!r}")
    S = int(window)
    if kind == "uniform":
        return torch.ones(S, dtype=torch.float32)
    i = torch.arange(S, dtype=torch.float64)
    return torch.exp(-(((i - (S - 1) / 2) / S) ** 2) / 0.02).to(torch.float32)


def canvas_size(canvas) -> tuple:
    """``canvas`` as ``(H, W)``: an int is a square."""
    if _is_int(canvas):
        canvas = (canvas, canvas)
    try:
        H, W = canvas
    except (TypeError, ValueError):
        raise ValueError(f"canvas must be an int or an (H, W) pair, got {canvas!r}") from None
    if not (_is_int(H) and _is_int(W) and H >= 1 and W >= 1):
        raise ValueError(f"canvas must be an int or an (H, W) pair of positive ints, got {canvas!r}")
    return int(H), int(W)


def window_grid(canvas, window, window_stride=None):
    """``(H, W, S, stride, oy, ox)`` of a canvas: the checked geometry ``WindowedDenoiseLoop`` and ``run_inference`` share (host only)."""
    H, W = canvas_size(canvas)
    if not (_is_int(window) and window >= 1):
        raise ValueError(f"window must be a positive int, got {window!r}")
    if window_stride is None:
        window_stride = max(int(window) // 2, 1)
    if not (_is_int(window_stride) and window_stride >= 1):
        raise ValueError(f"window_stride must be a positive int or None, got {window_stride!r}")
    if window > min(H, W):
        raise ValueError(f"window {window} is larger than the canvas {H} x {W}")
    if window_stride > window:
        raise ValueError(f"window_stride {window_stride} is larger than window {window}: the windows would leave gaps")
    S, stride = int(window), int(window_stride)
    return H, W, S, stride, window_origins(H, S, stride), window_origins(W, S, stride)


class WindowedDenoiseLoop:
    """A denoising loop over a ``(B, C, H, W)`` canvas whose every step runs ``inner``, a plain ``DenoiseLoop`` of batch ``B * nW`` at ``window x window``,
    between a ``pv_window_gather`` and a ``pv_window_blend`` launch (the module docstring has the step).  It has the loop surface ``run_inference`` uses:
    ``set_conditioning``, ``set_inpaint``, ``set_control``, ``reset``, ``step``, ``run``, ``latents``, ``state``, ``T``, ``scheduler``,
    ``launches_per_step`` (the inner loop's plus two).

    ``canvas``: an int or ``(H, W)``; ``window_stride``: None is ``window // 2``; ``window_weights``: ``"uniform"`` or ``"gaussian"`` (``window_profile``).
    ``inner``: the ``DenoiseLoop`` to drive (``run_inference`` passes its cached one; it carries its own options, so ``loop_kw`` beside it is a
    ``ValueError``) - otherwise one is built from ``loop_kw``, which takes everything ``DenoiseLoop`` takes; it acts per window, as in diffusers.  Refused with ``ValueError`` before any device work: ``stochastic=True`` or a stochastic
    scheduler (the fresh noise of every window would be averaged in the overlaps, so the canvas would lose variance there) and ``training_mode=True``."""

    def __init__(self, unet, batch: int, canvas, window: int, n_ip: int, num_steps: int, guidance_scale: float, *, window_stride: Optional[int] = None,
                 window_weights: str = "uniform", inner: Optional[DenoiseLoop] = None, **loop_kw):
        self.H, self.W, self.S, self.stride, self.oy, self.ox = window_grid(canvas, window, window_stride)
        profile = window_profile(window_weights, self.S)
        if loop_kw.get("stochastic") or bool(getattr(loop_kw.get("scheduler"), "stochastic", False)) or bool(getattr(inner, "stochastic", False)):
            raise ValueError("windowed denoising does not combine with stochastic=True / sampler='sde-dpmsolver++': the windows' noise would be averaged "
                             "in the overlaps")
        if loop_kw.get("training_mode") or bool(getattr(inner, "training_mode", False)):
            raise ValueError("windowed denoising does not combine with training_mode=True")
        if not (_is_int(batch) and batch >= 1):
            raise ValueError(f"batch must be a positive int, got {batch!r}")
        self.B, self.nW = int(batch), len(self.oy) * len(self.ox)
        if inner is not None and loop_kw:
            raise ValueError(f"inner comes with its own options: {sorted(loop_kw)} would be ignored - build the inner loop with them, or pass no inner")
        if inner is None:
            inner = DenoiseLoop(unet, self.B * self.nW, self.S, n_ip, num_steps, guidance_scale, **loop_kw)
        elif tuple(inner.latents.shape[0:1] + inner.latents.shape[2:]) != (self.B * self.nW, self.S, self.S):
            raise ValueError(f"inner loop runs {tuple(inner.latents.shape)} latents, expected batch {self.B * self.nW} at {self.S} x {self.S}")
        self.inner = inner
        self.window_weights = window_weights
        dev = inner.latents.device
        #: None for uniform weights: the launcher's all-ones path
        self.profile = None if window_weights == "uniform" else profile.to(dev)
        self.latents = torch.zeros((self.B, inner.latents.shape[1], self.H, self.W), dtype=torch.float32, device=dev)
        self.launches_per_step = inner.launches_per_step + 2

    # the inner loop's schedule
    @property
    def state(self):
        return self.inner.state

    @property
    def T(self):
        return self.inner.T

    @property
    def scheduler(self):
        return self.inner.scheduler

    def _canvas_operand(self, t, what, channels, scale=1):
        """``t`` (B or 1, channels, scale * H, scale * W), on any device -> contiguous fp32 (B, ...) on the canvas's device (``DenoiseLoop.set_control``
        moves a CPU control image itself, and callers rely on it: so does this loop, for every canvas-sized operand)."""
        want = (channels, scale * self.H, scale * self.W)
        if not torch.is_tensor(t) or t.dim() != 4 or tuple(t.shape[1:]) != want or t.shape[0] not in (1, self.B):
            raise ValueError(f"{what} has shape {tuple(getattr(t, 'shape', ()))}, expected ({self.B} or 1, {want[0]}, {want[1]}, {want[2]})")
        return t.to(device=self.latents.device, dtype=torch.float32).expand(self.B, *want).contiguous()

    def _gather(self, t, scale=1, out=None):
        return window_gather(t, scale * self.S, tuple(scale * o for o in self.oy), tuple(scale * o for o in self.ox), out=out)

    def set_conditioning(self, cond, uncond):
        """cond / uncond = (text (B, 77, D), ip (B, P, D)): every sample's rows serve its ``nW`` windows (sample-major, the window tensor's order)."""
        rep = lambda pair: tuple(t.repeat_interleave(self.nW, dim=0) for t in pair)
        self.inner.set_conditioning(rep(cond), rep(uncond))

    def set_inpaint(self, mask, known, noise):
        """``mask`` (B or 1, 1, H, W), ``known`` and ``noise`` (B, C, H, W) on the canvas: each window gets its crop."""
        C = self.latents.shape[1]
        self.inner.set_inpaint(self._gather(self._canvas_operand(mask, "mask", 1)), self._gather(self._canvas_operand(known, "known latents", C)),
                               self._gather(self._canvas_operand(noise, "noise", C)))

    def set_control(self, control_image):
        """``control_image`` (B or 1, 3, 8 H, 8 W): each window gets its crop - the same kernel with the origins and the window size times 8."""
        self.inner.set_control(self._gather(self._canvas_operand(control_image, "control_image", 3, scale=8), scale=8))

    def reset(self, noise, start: int = 0):
        """The canvas becomes ``noise`` (``* init_noise_sigma``, as ``DenoiseLoop.reset``); every window starts from its crop with an empty solver state."""
        self.latents.copy_(self._canvas_operand(noise, "noise", self.latents.shape[1]))
        self.inner.reset(self._gather(self.latents), start)
        sigma = float(self.inner.scheduler.init_noise_sigma)
        if sigma != 1.0:
            self.latents.mul_(sigma)

    def step(self):
        self._gather(self.latents, out=self.inner.latents)
        self.inner.step()
        window_blend(self.inner.latents, self.latents, self.S, self.oy, self.ox, self.profile)

    def run(self, steps: Optional[int] = None) -> torch.Tensor:
        for _ in range(self.inner.T - self.inner._start if steps is None else steps):
            self.step()
        return self.latents
