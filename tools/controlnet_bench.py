#!/usr/bin/env python3
"""Milliseconds per step of the denoising loop at the headline shape (bs 16, 64 x 64 latents, 1 image token, guidance 7.5) without and with a ControlNet:
``default`` (no keyword of this feature: the loop of a tree from before it) and ``controlnet`` (a ControlNet copied from the UNet with seeded non-zero
zero convs: two control plans per step in a group of their own, 13 control GEMMs per forward), and the time of the hint plan - the conditioning
embedding of the control images, seven ``pv_hint_conv3x3`` launches and one ``pv_gemm_conv``, run once per generation - alone.

Method (bench.py's, as in tools/freeu_bench.py): seeded random SD-v1.5-shaped UNet, captured graph, warm-up steps, then a host clock around ``--steps``
replays that end in a device synchronise.  The modes are built once and timed alternately for ``--rounds`` rounds, so that drift of the box hits them
alike; the line per mode gives the median, the minimum and the maximum over the rounds.  The hint plan is timed with device events around
``--hint-reps`` back-to-back runs (launch gaps included: an upper bound) and per launch the same way; its HBM floor is the bytes every launch must read
and write once (the recorder's tags) at ``--hbm-tbs`` TB/s."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bench import build_random_unet  # noqa: E402


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="default,controlnet")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hint-reps", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the floor is stated against, TB/s (MI355X: 8)")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.ops import Recorder
    from photoverse_amd.pipeline import DenoiseLoop
    dev = torch.device("cuda")
    torch.manual_seed(0)
    unet = build_random_unet(1, dev)
    cn = ControlNetModel.from_unet(unet).randomize_zero_convs_(seed=1)
    B, S, T = args.batch, args.latent, max(args.steps, args.warmup)
    g = torch.Generator().manual_seed(1234)
    noise = torch.randn(B, 4, S, S, generator=g)
    cond = (torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev))
    uncond = (torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 1, 768, generator=g).to(dev))
    image = torch.rand(B, 3, 8 * S, 8 * S, generator=g).to(dev)
    modes = {"default": {}, "controlnet": dict(controlnet=cn)}
    loops = {}
    for name in args.modes.split(","):
        loop = DenoiseLoop(unet, B, S, 1, T, 7.5, share_prefix=False, **modes[name])
        loop.set_conditioning(cond, uncond)
        if loop.controlnet is not None:
            loop.set_control(image)
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
    medians = {}
    for name, loop in loops.items():
        ts = times[name]
        med = medians[name] = statistics.median(ts)
        print(json.dumps({"label": args.label, "mode": name, "batch": B, "latent": S, "steps": args.steps, "rounds": args.rounds,
                          "launches_per_step": loop.launches_per_step, "merge_lowres": loop.merge_lowres,
                          "control_plan_launches": sum(len(e.rec) for e in loop.engines_ctrl_u + loop.engines_ctrl_c),
                          "steps_per_s_median": round(1e3 / med, 3), "ms_per_step_median": round(med, 3), "ms_per_step_min": round(min(ts), 3),
                          "ms_per_step_max": round(max(ts), 3), "finite": bool(torch.isfinite(loop.latents).all().item())}), flush=True)
    if "controlnet" in loops:
        rec = loops["controlnet"].hint_rec
        ms = _events(rec.run, args.hint_reps)
        floor_bytes = sum(t[2] for t in rec.tags)
        floor_ms = floor_bytes / (args.hbm_tbs * 1e12) * 1e3
        out = {"label": args.label, "mode": "hint_plan", "batch": B, "image": 8 * S, "launches": len(rec), "reps": args.hint_reps, "ms": round(ms, 4),
               "hbm_floor_bytes": int(floor_bytes), "hbm_floor_ms": round(floor_ms, 4), "achieved_tb_per_s": round(floor_bytes / (ms * 1e-3) / 1e12, 3),
               "fraction_of_hbm_floor_bandwidth": round(floor_ms / ms, 3)}
        if "default" in medians:
            out.update(ms_per_step_uncontrolled=round(medians["default"], 3), below_one_uncontrolled_step=bool(ms < medians["default"]))
        print(json.dumps(out), flush=True)
        for i in range(len(rec)):
            one = Recorder.__new__(Recorder)
            one.__dict__.update(rec.__dict__)
            one.calls, one.tags, one.roles = rec.calls[i:i + 1], rec.tags[i:i + 1], rec.roles[i:i + 1]
            us = _events(one.run, args.hint_reps) * 1e3
            name, flops, nbytes = rec.tags[i][:3]
            print(json.dumps({"label": args.label, "mode": "hint_launch", "index": i, "kernel": name, "us": round(us, 1), "gflop": round(flops / 1e9, 2),
                              "mbytes": round(nbytes / 1e6, 1), "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 3),
                              "tflop_per_s": round(flops / (us * 1e-6) / 1e12, 1)}), flush=True)


if __name__ == "__main__":
    main()
