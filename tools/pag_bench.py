#!/usr/bin/env python3
"""ms per step of the denoising loop at the headline shape (bs 16, 64 x 64 latents, 1 image token, guidance 7.5) without and with
perturbed-attention guidance: ``default`` (two forwards, ``pv_cfg_dpm_step``), ``pag_full`` (pag_scale 2 on the mid block, the whole perturbed
forward recorded: ``share_trunk=False``), ``pag_trunk`` (the same with the perturbed plan started from the conditional plan's tensors at the mid
block: the default with PAG) and ``pag_all_layers`` (all sixteen transformers perturbed; the trunk then ends at the first one).

Method (bench.py's): seeded random SD-v1.5-shaped UNet, captured graph, warm-up steps, then a host clock around ``--steps`` replays that end in a
device synchronise.  The modes are built once and timed alternately for ``--rounds`` rounds, so that drift of the box hits them alike; the line per
mode gives the median, the minimum and the maximum over the rounds.  ``--modes default`` passes no keyword of this feature, so
``tools/guidance_bench.py --modes default`` of a tree from before it measures the same loop: alternate the two trees in one job for the same-box
comparison of the default path across the two commits."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bench import build_random_unet  # noqa: E402

MODES = {"default": {}, "pag_full": dict(pag_scale=2.0, share_trunk=False), "pag_trunk": dict(pag_scale=2.0),
         "pag_all_layers": dict(pag_scale=2.0, pag_layers="all")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="default,pag_full,pag_trunk,pag_all_layers")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pag_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    from photoverse_amd.pipeline import DenoiseLoop
    dev = torch.device("cuda")
    torch.manual_seed(0)
    unet = build_random_unet(1, dev)
    B, S, T = args.batch, args.latent, max(args.steps, args.warmup)
    g = torch.Generator().manual_seed(1234)
    noise = torch.randn(B, 4, S, S, generator=g)
    cond = (torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev))
    uncond = (torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev))
    loops = {}
    for name in args.modes.split(","):
        loop = DenoiseLoop(unet, B, S, 1, T, 7.5, share_prefix=False, **MODES[name])
        loop.set_conditioning(cond, uncond)
        loop.reset(noise)
        for _ in range(args.warmup):
            loop.step()
        torch.cuda.synchronize()
        loops[name] = loop
    times = {name: [] for name in loops}
    for _ in range(args.rounds):
        for name, loop in loops.items():
            loop.reset(noise)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loop.step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    for name, loop in loops.items():
        ts = times[name]
        print(json.dumps({"label": args.label, "mode": name, "batch": B, "latent": S, "steps": args.steps, "rounds": args.rounds,
                          "launches_per_step": loop.launches_per_step, "ms_per_step_median": round(statistics.median(ts), 3),
                          "ms_per_step_min": round(min(ts), 3), "ms_per_step_max": round(max(ts), 3),
                          "finite": bool(torch.isfinite(loop.latents).all().item())}), flush=True)


if __name__ == "__main__":
    main()
