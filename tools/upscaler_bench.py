#!/usr/bin/env python3
"""``RRDBNet`` (Real-ESRGAN x4plus): ms per 4x upscale of ``--side`` x ``--side`` images through the HIP plan, the ``pv_dense_conv3x3``
launch alone per conv form (microseconds, achieved TFLOP/s and the share of the fp16 MFMA peak), and the yardstick: the same network with the same weights
through torch's own fp16 ``F.conv2d`` with ``torch.cat`` (the module of ``tests/_rrdb_ref.py``, ``.half()``), timed in the same process, alternating with
the plan.

Every figure comes from device events around the work; per measurement ``--warmup`` untimed calls (plans, code objects, the library's algorithm search), then
``--reps`` timed rounds; median with min and max.  The launch alone is timed over ``--kernel_iters`` back-to-back launches per round.  One JSON line per
measurement, each flushed as soon as it exists - the plan's figures come first, so they survive a baseline that cannot run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from photoverse_amd.ops import ACT_LEAKY_RELU, ACT_NONE, Recorder  # noqa: E402
from photoverse_amd.upscaler import RRDBNet  # noqa: E402

PEAK_FP16_TFLOPS = 2516.6         # 256 CUs x 4 SIMDs x 1024 FLOP/clk x 2.4 GHz: the dense fp16 / bf16 MFMA peak of the MI355X

parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
parser.add_argument("--blocks", type=int, default=23)
parser.add_argument("--side", type=int, default=512, help="input pixels a side")
parser.add_argument("--batches", nargs="+", type=int, default=[1, 4])
parser.add_argument("--warmup", type=int, default=2)
parser.add_argument("--reps", type=int, default=7)
parser.add_argument("--kernel_iters", type=int, default=20)
parser.add_argument("--no_baseline", action="store_true", help="skip torch's fp16 conv2d network")
parser.add_argument("--channels_last", action="store_true", help="run the baseline in torch.channels_last as well")
args = parser.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
dev = torch.device("cuda")


def timed(fn, iters=1):
    """ms per call of ``fn`` over ``iters`` back-to-back calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, out


def stats(v, digits=3):
    return dict(median=round(statistics.median(v), digits), min=round(min(v), digits), max=round(max(v), digits))


def emit(**row):
    print(json.dumps(row), flush=True)


def network_flops(blocks, pixels):
    """FLOP of one upscale of ``pixels`` input pixels: the RRDB body, the 64 -> 64 convs at 1x, 4x, 16x and 16x the pixels, conv_first and conv_last."""
    body = blocks * 3 * 18 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64)
    return float(pixels) * (body + 18 * 64 * 64 * (1 + 4 + 16 + 16) + 18 * 3 * 64 * (1 + 16))


# ---------------------------------------------------------------------------------------------------------------- the launch alone, per conv form
side = args.side
FORMS = [("dense 64 -> 32, LeakyReLU, in place", 64, 32, side, False, True, 0), ("dense 96 -> 32, LeakyReLU, in place", 96, 32, side, False, True, 0),
         ("dense 128 -> 32, LeakyReLU, in place", 128, 32, side, False, True, 0), ("dense 160 -> 32, LeakyReLU, in place", 160, 32, side, False, True, 0),
         ("conv5 192 -> 64, one residual", 192, 64, side, False, False, 1), ("conv5 192 -> 64, two residuals", 192, 64, side, False, False, 2),
         ("conv_body 64 -> 64, one residual", 64, 64, side, False, False, 1), ("conv_up1 64 -> 64, upsample, LeakyReLU", 64, 64, side, True, False, 0),
         ("conv_up2 64 -> 64, upsample, LeakyReLU", 64, 64, 2 * side, True, False, 0), ("conv_hr 64 -> 64, LeakyReLU", 64, 64, 4 * side, False, False, 0)]
g = torch.Generator(device="cuda").manual_seed(0)
for name, cin, cout, s, ups, inplace, nres in FORMS:
    rec = Recorder(dev)
    rows, so = s * s, (2 * s if ups else s)
    buf = torch.randn(rows, 192 if inplace or cin == 192 else cin, device="cuda", generator=g).half()
    w = (torch.randn(cout, 9 * cin, device="cuda", generator=g) * (9 * cin) ** -0.5).half()
    bias = torch.randn(cout, device="cuda", generator=g)
    res = [torch.randn(so * so, cout, device="cuda", generator=g).half() for _ in range(nres)]
    out = buf[:, cin:cin + cout] if inplace else torch.empty(so * so, cout, device="cuda", dtype=torch.float16)
    rec.dense_conv(buf, w, bias, cin=cin, batch=1, h=s, wd=s, upsample=ups, act=ACT_NONE if nres else ACT_LEAKY_RELU, out=out,
                   residual=res[0] if nres else None, alpha=0.2, residual2=res[1] if nres > 1 else None, beta=0.2)
    for _ in range(args.warmup):
        timed(rec.run, args.kernel_iters)
    ms = [timed(rec.run, args.kernel_iters)[0] for _ in range(args.reps)]
    flops = 2.0 * so * so * cout * 9 * cin
    tf = flops / (statistics.median(ms) * 1e-3) / 1e12
    emit(measure="pv_dense_conv3x3 alone", form=name, input_side=s, us=stats([v * 1e3 for v in ms], 1), gflop=round(flops / 1e9, 2), tflops=round(tf, 1),
         share_of_fp16_mfma_peak=round(tf / PEAK_FP16_TFLOPS, 3))
    del rec, buf, w, bias, res, out
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- the network
net = RRDBNet(num_block=args.blocks).randomize_(0).requires_grad_(False).to(dev)
base = None
if not args.no_baseline:
    from _rrdb_ref import RRDBNetRef
    base = RRDBNetRef(args.blocks).requires_grad_(False)
    base.load_state_dict(net.state_dict())
    base = base.half().to(dev).eval()


def baseline(x, channels_last=False):
    with torch.no_grad():
        t = ((x + 1) / 2).half()
        if channels_last:
            t = t.contiguous(memory_format=torch.channels_last)
        return (base(t).float() * 2 - 1).clamp(-1, 1)


for B in args.batches:
    x = torch.rand(B, 3, side, side, device="cuda", generator=g) * 2 - 1
    flops = network_flops(args.blocks, B * side * side)
    fns = {"plan": lambda: net.upscale(x)}
    row = dict(measure="4x upscale", blocks=args.blocks, batch=B, input_side=side, output_side=4 * side, tflop=round(flops / 1e12, 2))
    for _ in range(args.warmup):
        timed(fns["plan"])
    ms = {"plan": [timed(fns["plan"])[0] for _ in range(args.reps)]}
    row["plan_alone_ms"] = stats(ms["plan"])
    row["plan_launches"] = max(len(p.rec) for p in net._plans.values())
    row["plan_sub_batch"] = net._sub_batch(B, side, side)
    row["plan_tflops"] = round(flops / (statistics.median(ms["plan"]) * 1e-3) / 1e12, 1)
    row["plan_share_of_fp16_mfma_peak"] = round(row["plan_tflops"] / PEAK_FP16_TFLOPS, 3)
    emit(**row)
    if base is None:
        continue
    try:
        fns["torch_fp16"] = lambda: baseline(x)
        if args.channels_last:
            fns["torch_fp16_channels_last"] = lambda: baseline(x, True)
        for name in list(fns)[1:]:
            for i in range(args.warmup):
                t, _ = timed(fns[name])
                emit(measure="baseline warm-up", batch=B, which=name, call=i, ms=round(t, 1))
        ms = {name: [] for name in fns}
        outs = {}
        for _ in range(args.reps):
            for name, fn in fns.items():                         # alternating: plan, baseline, plan, baseline, ...
                t, outs[name] = timed(fn)
                ms[name].append(t)
        row = dict(measure="4x upscale, alternating with torch fp16 conv2d + cat", blocks=args.blocks, batch=B, input_side=side)
        for name in fns:
            row[name + "_ms"] = stats(ms[name])
        for name in list(fns)[1:]:
            row[name + "_over_plan"] = round(statistics.median(ms[name]) / statistics.median(ms["plan"]), 2)
            row[name + "_vs_plan_rel_l2"] = float((outs[name].double() - outs["plan"].double()).norm() / outs["plan"].double().norm())
        emit(**row)
        del outs
    except Exception as e:  # the yardstick could not run here: the plan's figures above stand alone
        emit(measure="baseline failed", batch=B, error=f"{type(e).__name__}: {str(e)[:300]}")
    del x
    torch.cuda.empty_cache()
