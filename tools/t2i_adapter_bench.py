#!/usr/bin/env python3
"""Times of the T2I-Adapter pieces at the headline shape (bs 16, 512 x 512 control image, 64 x 64 latents): the adapter plan - ``pv_pixel_unshuffle8`` and the
existing conv, pool and ReLU launches, 31 at SD-1.5, run once per generation - and one ``pv_add_feature_rows`` launch per level of the UNet's down path, with
the column statistics, against its bytes.

Method: a seeded random-init SD-1.5-sized adapter; device events around ``--reps`` back-to-back runs after one warm-up run (launch gaps included: an upper
bound for the plan; for a single launch the smaller operands stay in the caches between runs, so those are lower bounds on its time inside a step).  The add
launches are stated against the bytes they must move - x read, f read, out written, statistics written - at ``--copy-tbs`` TB/s, what a device copy reaches
on this chip.  ``--merged``: the two lowest levels at batch 2B with the features of B, as a plan over both CFG forwards' samples would read them."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--copy-tbs", type=float, default=6.3, help="bandwidth the add launches are stated against, TB/s (a device copy on MI355X: 6.3)")
    ap.add_argument("--in-channels", type=int, default=3, choices=(1, 3))
    ap.add_argument("--merged", action="store_true", help="the two lowest levels at batch 2B, reading the features of B")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("t2i_adapter_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    from photoverse_amd.ops import Recorder
    from photoverse_amd.t2i_adapter import T2IAdapter, adapter_plan, feature_sizes
    dev = torch.device("cuda")
    ad = T2IAdapter(in_channels=args.in_channels).randomize_(seed=1).to(dev)
    B, S = args.batch, args.latent
    g = torch.Generator().manual_seed(1234)
    image = torch.rand(B, args.in_channels, 8 * S, 8 * S, generator=g).to(dev)
    feats = ad.feature_buffers(B, S, S)
    rec = Recorder(dev)
    adapter_plan(rec, ad, image, feats)
    ms = _events(rec.run, args.reps)
    print(json.dumps({"label": args.label, "mode": "adapter_plan", "batch": B, "image": 8 * S, "in_channels": args.in_channels, "launches": len(rec),
                      "reps": args.reps, "ms": round(ms, 4), "gflop": round(sum(t[1] for t in rec.tags) / 1e9, 1),
                      "finite": bool(all(torch.isfinite(f).all().item() for f in feats))}), flush=True)
    state = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=dev)
    tab = torch.ones(1, dtype=torch.float32, device=dev)
    for k, (f, (hk, wk)) in enumerate(zip(feats, feature_sizes(S, S, len(feats)))):
        mult = 2 if (args.merged and k >= 2) else 1
        x = torch.randn(mult * f.shape[0], f.shape[1], generator=g).half().to(dev)
        one = Recorder(dev)
        one.add_feature(x, f, scale_tab=tab, state=state, colstats=True)
        us = _events(one.run, args.reps) * 1e3
        name, _, nbytes = one.tags[0][:3]
        print(json.dumps({"label": args.label, "mode": "add_launch", "kernel": name, "level": f"{hk}x{wk}", "rows": x.shape[0], "cols": x.shape[1],
                          "feat_rows": f.shape[0], "us": round(us, 2), "mbytes": round(nbytes / 1e6, 2),
                          "floor_us_at_copy_bandwidth": round(nbytes / (args.copy_tbs * 1e12) * 1e6, 2),
                          "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 3)}), flush=True)


if __name__ == "__main__":
    main()
