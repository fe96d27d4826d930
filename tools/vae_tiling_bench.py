#!/usr/bin/env python3
"""Tiled against untiled VAE decode (``AutoencoderKL.enable_tiling``): ms per decode and peak device memory, random-init SD-v1.5 VAE.

One process.  Per size, first the memory pass - per mode: plans dropped, allocator cache emptied, peak counter reset, one decode; the figure is
``torch.cuda.max_memory_allocated`` above what was allocated before (weights and the input), so it holds the plan's static buffers, the tile rows and
the output.  Then the timing pass: both modes warmed up (plans built, code objects loaded), then ``--reps`` rounds that alternate untiled / tiled, each
decode timed by a host clock around a device synchronise; median and range are printed.  A size whose untiled plan the GEMM launcher rejects (the score matrix past the 2 GiB
a buffer descriptor addresses; found by a host query of the library's dispatch code, the plan is never launched) is recorded as such and timed tiled
only.  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photoverse_amd.ops import HipLaunchError, Recorder  # noqa: E402
from photoverse_amd.vae import AutoencoderKL  # noqa: E402

parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
parser.add_argument("--sizes", nargs="+", default=["1x64", "1x96", "1x128", "1x192", "4x128"], help="BATCHxLATENT_SIDE")
parser.add_argument("--untiled_max", type=int, default=128, help="largest latent side the untiled path is asked to decode")
parser.add_argument("--reps", type=int, default=5)
parser.add_argument("--tile", type=int, default=512)
parser.add_argument("--overlap", type=float, default=0.25)
args = parser.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

torch.manual_seed(0)
vae = AutoencoderKL(with_encoder=False).to("cuda")


def set_mode(tiled):
    vae.enable_tiling(args.tile, args.overlap) if tiled else vae.disable_tiling()


def timed(z):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = vae.decode(z).sample
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mib(z, tiled):
    set_mode(tiled)
    vae.repack()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    vae.decode(z)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


for spec in args.sizes:
    B, side = (int(v) for v in spec.split("x"))
    z = torch.randn(B, 4, side, side, device="cuda")
    row = dict(batch=B, latent=side, pixels=8 * side, tile=args.tile, overlap=args.overlap)
    modes = [True]
    n = side * side
    # the untiled mid-block attention's P.V product reads the n x n fp16 score matrix as its A operand: asked from the library's own dispatch code (a
    # host query, nothing is launched) whether it takes that block
    pv_kernel = Recorder._probe_gemm(c0=n, lda0=n, N=512, ldc=512, M=n, taps=1, batch=1, hin=1, win=1, hout=n, wout=1, stride=1, pad=1)
    if not pv_kernel:
        row["untiled"] = f"rejected by pv_gemm_conv: the {n} x {n} fp16 score matrix is {n * n * 2 / 2 ** 30:.2f} GiB, past a buffer descriptor's 2 GiB"
    elif side > args.untiled_max:
        row["untiled"] = "not asked (--untiled_max)"
    else:
        modes.insert(0, False)
    for tiled in list(modes):
        name = "tiled" if tiled else "untiled"
        try:
            row[name + "_peak_mib"] = round(peak_mib(z, tiled), 1)
        except (HipLaunchError, torch.OutOfMemoryError) as e:
            row[name] = f"rejected: {type(e).__name__}: {str(e)[:120]}"
            modes.remove(tiled)
            vae.repack()
            torch.cuda.empty_cache()
    vae.repack()
    torch.cuda.empty_cache()
    outs = {}
    for tiled in modes:                                   # warm-up: plans, code objects
        set_mode(tiled)
        for _ in range(2):
            _, outs[tiled] = timed(z)
    ms = {tiled: [] for tiled in modes}
    for _ in range(args.reps):
        for tiled in modes:
            set_mode(tiled)
            ms[tiled].append(timed(z)[0])
    for tiled in modes:
        name = "tiled" if tiled else "untiled"
        row[name + "_ms"] = dict(median=round(statistics.median(ms[tiled]), 2), min=round(min(ms[tiled]), 2), max=round(max(ms[tiled]), 2))
        row[name + "_finite"] = bool(torch.isfinite(outs[tiled]).all())
    if len(modes) == 2:
        a, b = outs[True].double(), outs[False].double()
        row["tiled_vs_untiled_rel_l2"] = float((a - b).norm() / b.norm())          # a different function of the latents, not an error
    del outs
    print(json.dumps(row), flush=True)
