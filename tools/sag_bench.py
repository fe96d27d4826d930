#!/usr/bin/env python3
"""us per launch of the two launches of self-attention guidance at the headline shape (bs 16, 64 x 64 latents): ``pv_attn_colmass`` on the mid block's
self-attention (64 tokens, 8 heads of 160, q / k as column slices of a ``[B N][3 C]`` buffer) and ``pv_sag_degrade`` on 16 x 4 x 64 x 64 latents with an
8 x 8 mass, each by device events around ``--reps`` back-to-back launches after a warm-up, ``--rounds`` times alternately; the line per launch gives the
median, the minimum and the maximum over the rounds, and the launch's algorithmic flops and bytes from its recorder tag.  ``--latent 128`` gives the
second pass of a hires run (256 tokens)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def time_launch(rec, reps):
    """us per run of ``rec``: device events around ``reps`` back-to-back runs"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        rec.run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=160)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sag_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    from photoverse_amd.ops import Recorder
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    dev = torch.device("cuda")
    B, S, heads, d = args.batch, args.latent, args.heads, args.head_dim
    m = S // 8                                                   # the mid block's grid of an SD-v1.5-shaped UNet
    n, C = m * m, heads * d
    g = torch.Generator().manual_seed(1234)
    qkv = torch.randn(B * n, 3 * C, generator=g).half().to(dev)
    x, eps = (torch.randn(B, 4, S, S, generator=g).to(dev) for _ in range(2))
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(50)
    coef = sch.coefficient_table(0).to(dev)
    state = torch.tensor([25, 50, 0, 0], dtype=torch.int32, device=dev)
    tap, deg = Recorder(dev), Recorder(dev)
    mass = tap.attn_colmass(qkv[:, :C], qkv[:, C:2 * C], batch=B, heads=heads, nq=n, nk=n, d=d)
    deg.sag_degrade(x, eps, mass, coef, state, mh=m, mw=m)
    recs = {"pv_attn_colmass": tap, "pv_sag_degrade": deg}
    for rec in recs.values():
        for _ in range(10):
            rec.run()
    torch.cuda.synchronize()
    times = {name: [] for name in recs}
    for _ in range(args.rounds):
        for name, rec in recs.items():
            times[name].append(time_launch(rec, args.reps))
    share = (mass > 1).float().mean().item()
    for name, rec in recs.items():
        ts = times[name]
        _, flops, nbytes = rec.tags[0][:3]
        print(json.dumps({"label": args.label, "launch": name, "batch": B, "latent": S, "tokens": n, "heads": heads, "head_dim": d, "reps": args.reps,
                          "rounds": args.rounds, "us_median": round(statistics.median(ts), 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                          "mflop": round(flops / 1e6, 1), "mbyte": round(nbytes / 1e6, 2), "mass_sum_over_tokens": round(mass.sum(-1).mean().item() / n, 6),
                          "share_above_threshold": round(share, 3)}), flush=True)


if __name__ == "__main__":
    main()
