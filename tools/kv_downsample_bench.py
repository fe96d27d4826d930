#!/usr/bin/env python3
"""Steps per second of the denoising loop (1 image token, guidance 7.5) without and with token downsampling: ``off`` (no keyword of this feature: the
loop of a tree from before it), ``f2`` (``kv_downsample=2``) and ``f4`` (``kv_downsample=4``), ``avg`` on the default layers - the five transformers of
the highest-resolution level - and the time of one ``pv_token_pool`` launch against its byte floor.

Method (bench.py's, as in tools/freeu_bench.py): seeded random SD-v1.5-shaped UNet, captured graph, warm-up steps, then a host clock around ``--steps``
replays that end in a device synchronise.  The modes are built once in ONE process and timed alternately for ``--rounds`` rounds, so that drift of the
box hits them alike; the line per mode gives the median, the minimum and the maximum over the rounds.  One process per shape (``--batch``, ``--latent``).
The launch time is taken with device events around ``--kernel-reps`` back-to-back replays of the pool launches of one plan alone (launch gaps included: an
upper bound of the kernel's own time; the input stays in the Infinity cache between replays, as it largely does behind the qkv launch in the loop)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bench import build_random_unet  # noqa: E402

MODES = {"off": {}, "f2": dict(kv_downsample=2), "f4": dict(kv_downsample=4), "f2_nearest": dict(kv_downsample=2, kv_downsample_method="nearest")}
HBM_COPY_TBS = 6.3          # what a copy reaches on this part (EXPERIMENTS.md): the floor the launch is held against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="off,f2,f4")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=100)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_downsample_bench.py needs a HIP device: a timing taken elsewhere says nothing")
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
    base = statistics.median(times["off"]) if "off" in times else None
    for name, loop in loops.items():
        ts = times[name]
        med = statistics.median(ts)
        attn = [t for e in loop.all_engines for t in e.rec.tags if t[0].startswith(("attn8_kernel", "attn_kernel"))]
        print(json.dumps({"label": args.label, "mode": name, "batch": B, "latent": S, "steps": args.steps, "rounds": args.rounds,
                          "launches_per_step": loop.launches_per_step, "merge_lowres": loop.merge_lowres,
                          "pool_launches_per_step": sum(t[0] == "token_pool_kernel" for e in loop.all_engines for t in e.rec.tags),
                          "self_attention_gflop_per_step": round(sum(t[1] for t in attn) / 1e9, 1),
                          "steps_per_s_median": round(1e3 / med, 3), "ms_per_step_median": round(med, 3), "ms_per_step_min": round(min(ts), 3),
                          "ms_per_step_max": round(max(ts), 3), "speedup_vs_off": None if base is None else round(base / med, 4),
                          "finite": bool(torch.isfinite(loop.latents).all().item())}), flush=True)
    for name, loop in loops.items():
        eng = loop.engines_c[0]
        sub = eng.rec.subset(lambda t: t[0] == "token_pool_kernel")
        if not len(sub):
            continue
        sub.run()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.kernel_reps):
            sub.run()
        stop.record()
        torch.cuda.synchronize()
        us = start.elapsed_time(stop) * 1e3 / (args.kernel_reps * len(sub))
        nbytes = max(t[2] for t in sub.tags)
        print(json.dumps({"label": args.label, "mode": name + "_pool_launch", "plan_batch": eng.B, "launches": len(sub), "reps": args.kernel_reps,
                          "bytes_per_launch": nbytes, "floor_us_at_6.3_TBs": round(nbytes / (HBM_COPY_TBS * 1e12) * 1e6, 2),
                          "us_per_launch_back_to_back": round(us, 2), "TBs": round(nbytes / (us * 1e-6) / 1e12, 3)}), flush=True)


if __name__ == "__main__":
    main()
