#!/usr/bin/env python3
"""``AutoencoderTiny`` (TAESD) against ``AutoencoderKL``'s default path - ms per decode / encode and peak device memory above the weights
- and the 64 -> 64 ``pv_tiny_conv3x3`` launch alone against ``pv_hint_conv3x3`` on the same operands.  Random-init weights of the full-size models.

One process.  Per (batch, latent side) and direction, first the memory pass - per model: plans dropped, allocator cache emptied, peak counter reset, one call;
the figure is ``torch.cuda.max_memory_allocated`` above what was allocated before (weights and the input), so it holds the plan's static buffers and the
output.  Then the timing pass: both models warmed up (plans built, code objects loaded), then ``--reps`` rounds that alternate KL / tiny, each call timed by a
host clock around a device synchronise; median and range are printed.  The launch alone: ``--kernel_iters`` replays per round, timed the same way, act NONE
with a bias - the one form both launchers have.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photoverse_amd.ops import ACT_NONE, Recorder  # noqa: E402
from photoverse_amd.vae import AutoencoderKL  # noqa: E402
from photoverse_amd.vae_tiny import AutoencoderTiny  # noqa: E402

parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
parser.add_argument("--sizes", nargs="+", default=["1x64", "4x64", "1x128", "4x128"], help="BATCHxLATENT_SIDE")
parser.add_argument("--reps", type=int, default=5)
parser.add_argument("--kernel_iters", type=int, default=10)
parser.add_argument("--kernel_side", type=int, default=512, help="pixels a side of the launch measured alone")
args = parser.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

torch.manual_seed(0)
models = {"kl": AutoencoderKL().to("cuda"), "tiny": AutoencoderTiny().to("cuda")}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mib(model, fn):
    model.repack()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


# ---------------------------------------------------------------------------------------------------------------- the models
for spec in args.sizes:
    B, side = (int(v) for v in spec.split("x"))
    z = torch.randn(B, 4, side, side, device="cuda")
    x = torch.rand(B, 3, 8 * side, 8 * side, device="cuda") * 2 - 1
    calls = {"decode": {"kl": lambda: models["kl"].decode(z).sample, "tiny": lambda: models["tiny"].decode(z).sample},
             "encode": {"kl": lambda: models["kl"].encode(x).latent_dist.parameters, "tiny": lambda: models["tiny"].encode(x).latents}}
    for what, fns in calls.items():
        row = dict(measure=what, batch=B, latent=side, pixels=8 * side)
        with torch.no_grad():
            for name, fn in fns.items():
                row[name + "_peak_mib"] = round(peak_mib(models[name], fn), 1)
            for m in models.values():
                m.repack()
            torch.cuda.empty_cache()
            for fn in fns.values():                            # warm-up: plans, code objects
                for _ in range(2):
                    timed(fn)
            ms = {name: [] for name in fns}
            for _ in range(args.reps):
                for name, fn in fns.items():
                    ms[name].append(timed(fn)[0])
        for name in fns:
            row[name + "_ms"] = stats(ms[name])
            row[name + "_launches"] = max(len(p.rec) for p in models[name]._plans.values())
        row["kl_over_tiny"] = round(statistics.median(ms["kl"]) / statistics.median(ms["tiny"]), 2)
        print(json.dumps(row), flush=True)
    del z, x, calls
    for m in models.values():
        m.repack()
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- the 64 -> 64 launch alone
dev = torch.device("cuda")
side = args.kernel_side
xr = torch.randn(side * side, 64, device="cuda").half()
w = (torch.randn(64, 576, device="cuda") * 576 ** -0.5).half()
bias = torch.randn(64, device="cuda")
new, old = Recorder(dev), Recorder(dev)
o_new = new.tiny_conv(xr, w, bias, batch=1, h=side, wd=side, act=ACT_NONE)
o_old = old.hint_conv(xr, w, bias, batch=1, h=side, wd=side, stride=1, act=ACT_NONE)


def replay(rec):
    for _ in range(args.kernel_iters):
        rec.run()


for rec in (old, new):
    timed(lambda: replay(rec))
ms = {id(old): [], id(new): []}
for _ in range(args.reps):
    for rec in (old, new):
        ms[id(rec)].append(timed(lambda: replay(rec))[0] / args.kernel_iters)
flops = 2.0 * side * side * 64 * 576
tf = lambda v: round(flops / (statistics.median(v) * 1e-3) / 1e12, 1)
print(json.dumps(dict(measure="64 -> 64 launch alone", pixels=side, act="none", hint_ms=stats(ms[id(old)]), tiny_ms=stats(ms[id(new)]),
                      hint_tflops=tf(ms[id(old)]), tiny_tflops=tf(ms[id(new)]),
                      tiny_vs_hint_rel_l2=float((o_new.double() - o_old.double()).norm() / o_old.double().norm()),
                      same_bits=bool(torch.equal(o_new, o_old)))), flush=True)
