#!/usr/bin/env python3
"""Windowed (MultiDiffusion) against plain denoising on one canvas (``multidiffusion.WindowedDenoiseLoop``): ms per step, random-init
SD-v1.5 UNet, and the two window launches alone against a device copy of the same bytes.

One process.  Loops: the plain ``DenoiseLoop`` at the canvas size and the windowed loop at ``--window`` for every ``--strides`` entry are built and warmed
up (graphs captured, code objects loaded); then ``--reps`` rounds alternate between them, each round timing ``--steps`` steps by a host clock around a
device synchronise; median and range of ms per step are printed.  Kernels: per ``--kernel_shapes`` entry ``pv_window_gather`` and ``pv_window_blend``
(uniform and gaussian) are timed by device events around ``--launches`` back-to-back launches, next to ``Tensor.copy_`` of the canvas - the device-copy
rate the bytes are held against; bytes are what the algorithm has to move (gather: the window tensor read and written; blend: the window tensor read,
the canvas written).  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photoverse_amd.multidiffusion import WindowedDenoiseLoop, window_origins, window_profile  # noqa: E402
from photoverse_amd.ops import window_blend, window_gather  # noqa: E402
from photoverse_amd.pipeline import DenoiseLoop  # noqa: E402

parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
parser.add_argument("--batch", type=int, default=1)
parser.add_argument("--canvas", type=int, default=128)
parser.add_argument("--window", type=int, default=64)
parser.add_argument("--strides", nargs="+", type=int, default=[32, 64])
parser.add_argument("--steps", type=int, default=8, help="steps per timed round")
parser.add_argument("--reps", type=int, default=5)
parser.add_argument("--guidance", type=float, default=5.0)
parser.add_argument("--no_plain", action="store_true", help="skip the plain loop at the canvas size")
parser.add_argument("--kernel_shapes", nargs="+", default=["1x4x128x128x64x32", "1x4x128x128x64x64", "8x4x1024x1024x512x256"], help="BxCxHxWxSxSTRIDE")
parser.add_argument("--launches", type=int, default=200)
args = parser.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
dev = torch.device("cuda")


def median_range(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


# ---------------------------------------------------------------------------------------------------------------- the two launches alone
def event_ms(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


for spec in args.kernel_shapes:
    B, C, H, W, S, stride = (int(v) for v in spec.split("x"))
    oy, ox = window_origins(H, S, stride), window_origins(W, S, stride)
    canvas = torch.randn(B, C, H, W, device=dev)
    other = torch.empty_like(canvas)
    windows = window_gather(canvas, S, oy, ox)
    gauss = window_profile("gaussian", S).to(dev)
    n_canvas, n_win = canvas.numel() * 4, windows.numel() * 4
    row = dict(kernel_shape=spec, windows=len(oy) * len(ox), canvas_mib=round(n_canvas / 2 ** 20, 2), windows_mib=round(n_win / 2 ** 20, 2))
    cases = (("copy", lambda: other.copy_(canvas), 2 * n_canvas),
             ("gather", lambda: window_gather(canvas, S, oy, ox, out=windows), 2 * n_win),
             ("blend_uniform", lambda: window_blend(windows, other, S, oy, ox), n_win + n_canvas),
             ("blend_gaussian", lambda: window_blend(windows, other, S, oy, ox, gauss), n_win + n_canvas))
    for name, fn, nbytes in cases:
        ms = [event_ms(fn, args.launches) for _ in range(args.reps)]
        row[name] = dict(us=round(statistics.median(ms) * 1e3, 2), us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2), bytes=nbytes,
                         gb_per_s=round(nbytes / (statistics.median(ms) * 1e-3) / 1e9, 1))
    print(json.dumps(row), flush=True)
    del canvas, other, windows

# ---------------------------------------------------------------------------------------------------------------- the loops
from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter  # noqa: E402

torch.manual_seed(0)
P = 5
unet = UNet2DConditionModel()
set_visual_cross_attention_adapter(unet, (P,))
unet.to(dev)
g = torch.Generator().manual_seed(1)
mk = lambda *sh: torch.randn(*sh, generator=g).to(dev)
B, T = args.batch, max(args.steps, 3)
cond, uncond = (mk(B, 77, 768), mk(B, P, 768)), (mk(B, 77, 768), mk(B, P, 768))
noise = mk(B, 4, args.canvas, args.canvas)

loops = {}
if not args.no_plain:
    try:
        loops["plain"] = DenoiseLoop(unet, B, args.canvas, P, T, args.guidance)
    except Exception as e:       # a size a launcher rejects is a result, not a crash
        print(json.dumps(dict(loop="plain", canvas=args.canvas, rejected=f"{type(e).__name__}: {str(e)[:200]}")), flush=True)
for stride in args.strides:
    loops[f"window{args.window}_stride{stride}"] = WindowedDenoiseLoop(unet, B, args.canvas, args.window, P, T, args.guidance, window_stride=stride)


def timed(loop):
    loop.reset(noise)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(args.steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps


finite = {}
for name, loop in loops.items():                          # warm-up: capture, code objects
    loop.set_conditioning(cond, uncond)
    timed(loop)
    finite[name] = bool(torch.isfinite(loop.latents).all())
ms = {name: [] for name in loops}
for _ in range(args.reps):
    for name, loop in loops.items():
        ms[name].append(timed(loop))
for name, loop in loops.items():
    print(json.dumps(dict(loop=name, batch=B, canvas=args.canvas, windows=getattr(loop, "nW", None), steps=args.steps, ms_per_step=median_range(ms[name]),
                          launches_per_step=loop.launches_per_step, finite=finite[name])), flush=True)
