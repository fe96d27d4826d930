"""References of the windowed-denoising tests (``test_multidiffusion_cpu.py`` / ``test_multidiffusion_gpu.py``): the two launches' formulas as float64
slicing, and the windowed denoising loop on the fp32 oracle UNet - per step and per window two forwards on the crop, the CFG combine and the window's
OWN ``DPMSolverMultistepRef`` step, then the canvas set to the weighted mean."""
import torch


def canvas_inputs(H, W, seed=83):
    """(cond, uncond) of ``test_pag_cpu.loop_inputs_81`` (B = 2) and a seeded start noise (2, 4, H, W)."""
    from test_pag_cpu import loop_inputs_81
    cond, uncond, _ = loop_inputs_81()
    return cond, uncond, torch.randn(2, 4, H, W, generator=torch.Generator().manual_seed(seed + 1000 * H + W))


def origins_ref(size, window, stride):
    """The window origins of one axis, by search: every multiple of ``stride`` whose window fits, plus the clamped last one."""
    out = [o for o in range(size) if o % stride == 0 and o + window <= size]
    if out[-1] + window < size:
        out.append(size - window)
    return tuple(out)


def profile_ref(kind, S):
    """The issue's profiles: ones, or ``exp(-((i - (S - 1) / 2) / S)^2 / 0.02)`` in float64, rounded to fp32 (the values the kernel reads)."""
    assert kind in ("uniform", "gaussian"), kind
    if kind == "uniform":
        return torch.ones(S, dtype=torch.float32)
    import math
    return torch.tensor([math.exp(-(((i - (S - 1) / 2) / S) ** 2) / 0.02) for i in range(S)], dtype=torch.float64).float()


def n_cover(H, W, S, oy, ox):
    """The largest number of windows that cover one canvas element."""
    cy = max(sum(1 for o in oy if o <= y < o + S) for y in range(H))
    cx = max(sum(1 for o in ox if o <= x < o + S) for x in range(W))
    return cy * cx


def gather_ref(canvas, S, oy, ox):
    """``pv_window_gather``: (B, C, H, W) -> (B * ny * nx, C, S, S), window k = ky * nx + kx of sample b in row b * ny * nx + k; float64."""
    B = canvas.shape[0]
    rows = [canvas[b:b + 1, :, y0:y0 + S, x0:x0 + S].double() for b in range(B) for y0 in oy for x0 in ox]
    return torch.cat(rows, dim=0)


def blend_ref(windows, shape, S, oy, ox, profile=None):
    """``pv_window_blend`` in float64: ``num / den`` with ``num`` the windows times ``profile[y - oy] * profile[x - ox]`` summed where they cover,
    ``den = (sum_ky profile[y - oy]) * (sum_kx profile[x - ox])``.  ``profile``: the [S] values the kernel reads (None: ones)."""
    B, C, H, W = shape
    ny, nx = len(oy), len(ox)
    p = torch.ones(S, dtype=torch.float64) if profile is None else profile.double().cpu()
    num = torch.zeros(shape, dtype=torch.float64)
    den_y, den_x = torch.zeros(H, dtype=torch.float64), torch.zeros(W, dtype=torch.float64)
    for y0 in oy:
        den_y[y0:y0 + S] += p
    for x0 in ox:
        den_x[x0:x0 + S] += p
    w2 = p[:, None] * p[None, :]
    win = windows.double().cpu().reshape(B, ny * nx, C, S, S)
    for ky, y0 in enumerate(oy):
        for kx, x0 in enumerate(ox):
            num[:, :, y0:y0 + S, x0:x0 + S] += w2 * win[:, ky * nx + kx]
    return num / (den_y[:, None] * den_x[None, :])


@torch.no_grad()
def windowed_oracle_loop(ref, cond, uncond, noise, g_text, window, stride, weights, steps, *, pert=None, g_pag=0.0, g_image=None, model_for=None):
    """The windowed loop on the fp32 oracle.  ``ref``: the oracle UNet (any callable with its signature); ``model_for(ky, kx)``: a model per window
    instead (a ControlNet sees the window's crop of the control image).  ``pert`` / ``g_pag``: perturbed-attention guidance, ``g_image``: the third
    forward of the split guidance - per window, as the plain ``oracle_loop`` has them.  Returns the fp32 canvas."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    B, C, H, W = noise.shape
    S = window
    oy, ox = origins_ref(H, S, stride), origins_ref(W, S, stride)
    profile = profile_ref(weights, S)
    schs = {}
    for ky in range(len(oy)):
        for kx in range(len(ox)):
            schs[ky, kx] = DPMSolverMultistepRef()
            schs[ky, kx].set_timesteps(steps)
    first = schs[0, 0]
    x = noise * first.init_noise_sigma
    for t in first.timesteps:
        outs = []
        for ky, y0 in enumerate(oy):
            for kx, x0 in enumerate(ox):
                model = ref if model_for is None else model_for(ky, kx)
                crop = x[:, :, y0:y0 + S, x0:x0 + S].contiguous()
                eu = model(crop, t, encoder_hidden_states=uncond).sample
                ec = model(crop, t, encoder_hidden_states=cond).sample
                if g_image is None:
                    e = eu + g_text * (ec - eu)
                else:
                    em = model(crop, t, encoder_hidden_states=(uncond[0], cond[1])).sample
                    e = eu + g_image * (em - eu) + g_text * (ec - em)
                if g_pag:
                    e = e + g_pag * (ec - pert(crop, t, encoder_hidden_states=cond).sample)
                outs.append(schs[ky, kx].step(e, t, crop))
        win = torch.stack(outs, dim=1).reshape(B * len(outs), C, S, S)             # sample-major, k = ky * nx + kx
        x = blend_ref(win, (B, C, H, W), S, oy, ox, profile).float()
    return x
