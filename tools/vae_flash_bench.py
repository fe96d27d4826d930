#!/usr/bin/env python3
"""Flash against default mid-block attention in the VAE (``AutoencoderKL.enable_flash_attention``): ms per decode / encode and peak device
memory, the attention launches alone, and the largest untiled decode - random-init SD-v1.5 VAE.

One process.  Per (batch, latent side) and direction, first the memory pass - per mode: plans dropped, allocator cache emptied, peak counter reset, one call;
the figure is ``torch.cuda.max_memory_allocated`` above what was allocated before (weights and the input), so it holds the plan's static buffers and the
output.  Then the timing pass: both modes warmed up (plans built, code objects loaded), then ``--reps`` rounds that alternate default / flash, each call timed
by a host clock around a device synchronise; median and range are printed.  The attention alone: one ``pv_vae_attention`` launch over the batch against the
default's four launches per image (Q.K^T, ``pv_softmax_rows``, V^T, P.V) on the same random operands, timed the same way over ``--kernel_iters`` replays per round.
Last, untiled decodes with flash on at growing latent sides up to ``--max_side``: the default plan there is rejected by the GEMM launcher (asked from the
library's dispatch code, never launched); the first size that fails ends the walk and is reported with its error.  One JSON line per measurement."""
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
parser.add_argument("--sizes", nargs="+", default=["1x64", "4x64", "1x128", "4x128"], help="BATCHxLATENT_SIDE")
parser.add_argument("--reps", type=int, default=5)
parser.add_argument("--kernel_iters", type=int, default=5)
parser.add_argument("--walk", nargs="+", type=int, default=[144, 160, 176, 192], help="latent sides of the untiled flash decodes, ascending")
args = parser.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"

torch.manual_seed(0)
vae = AutoencoderKL().to("cuda")
C = 512


def set_mode(flash):
    vae.enable_flash_attention() if flash else vae.disable_flash_attention()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mib(fn, flash):
    set_mode(flash)
    vae.repack()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def default_rejected(n):
    """Whether pv_gemm_conv refuses the default path's P.V launch (A operand: the n x n fp16 score matrix) - a host query, nothing is launched."""
    return not Recorder._probe_gemm(c0=n, lda0=n, N=C, ldc=C, M=n, taps=1, batch=1, hin=1, win=1, hout=n, wout=1, stride=1, pad=1)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------------------------------------------- the model
for spec in args.sizes:
    B, side = (int(v) for v in spec.split("x"))
    z = torch.randn(B, 4, side, side, device="cuda")
    x = torch.rand(B, 3, 8 * side, 8 * side, device="cuda") * 2 - 1
    for what, fn in (("decode", lambda: vae.decode(z).sample), ("encode", lambda: vae.encode(x).latent_dist.parameters)):
        row = dict(measure=what, batch=B, latent=side, pixels=8 * side, tokens=side * side)
        for flash in (False, True):
            row[("flash" if flash else "default") + "_peak_mib"] = round(peak_mib(fn, flash), 1)
        vae.repack()
        torch.cuda.empty_cache()
        outs = {}
        with torch.no_grad():
            for flash in (False, True):                       # warm-up: plans, code objects
                set_mode(flash)
                for _ in range(2):
                    _, outs[flash] = timed(fn)
            ms = {False: [], True: []}
            for _ in range(args.reps):
                for flash in (False, True):
                    set_mode(flash)
                    ms[flash].append(timed(fn)[0])
        row["default_ms"], row["flash_ms"] = stats(ms[False]), stats(ms[True])
        row["flash_vs_default_rel_l2"] = rel_l2(outs[True], outs[False])
        row["finite"] = bool(torch.isfinite(outs[True]).all())
        del outs
        print(json.dumps(row), flush=True)
    del z, x
    vae.repack()
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- the attention launches alone
dev = torch.device("cuda")
for spec in args.sizes:
    B, side = (int(v) for v in spec.split("x"))
    n = side * side
    g = torch.randn(B * n, C, device="cuda").half()                       # the normalised tokens
    qkv = torch.randn(B * n, 3 * C, device="cuda").half()                 # q | k | v, ~N(0, 1): scaled scores ~N(0, 1)
    wv = (torch.randn(C, C, device="cuda") * C ** -0.5).half()
    bv = torch.zeros(C, device="cuda")
    new = Recorder(dev)
    o_new = new.vae_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch=B, n=n, scale=C ** -0.5)
    old = Recorder(dev)
    q, k = qkv[:, :C].contiguous(), qkv[:, C:2 * C].contiguous()
    scores, vt, o_old = old.empty((n, n)), old.empty((C, n)), old.empty((B * n, C))
    for i in range(B):                                                    # AutoencoderKL._attn's per-image launches
        rows = slice(i * n, (i + 1) * n)
        old.gemm(q[rows], old.hold(k[rows]), out=scores, splitk=0)
        old.softmax_rows(scores, scale=C ** -0.5)
        old.gemm(wv, old.hold(g[rows]), out=vt, splitk=0)
        old.gemm(scores, vt, bias=bv, out=o_old[rows], splitk=0)

    def replay(rec):
        for _ in range(args.kernel_iters):
            rec.run()

    for rec in (old, new):
        timed(lambda: replay(rec))
    ms = {id(old): [], id(new): []}
    for _ in range(args.reps):
        for rec in (old, new):
            ms[id(rec)].append(timed(lambda: replay(rec))[0] / args.kernel_iters)
    flops = 4.0 * B * n * n * C
    row = dict(measure="attention alone", batch=B, tokens=n, d=C, default_launches=len(old), flash_launches=len(new), default_ms=stats(ms[id(old)]),
               flash_ms=stats(ms[id(new)]), flash_tflops=round(flops / (statistics.median(ms[id(new)]) * 1e-3) / 1e12, 1))
    print(json.dumps(row), flush=True)
    del new, old, scores, vt, o_old, o_new, qkv, g, q, k
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- the largest untiled decode
vae.enable_flash_attention()
largest, stopped = None, None
for side in args.walk:
    n = side * side
    row = dict(measure="untiled flash decode", batch=1, latent=side, pixels=8 * side, tokens=n, default_plan_rejected=default_rejected(n),
               score_matrix_gib=round(n * n * 2 / 2 ** 30, 2))
    z = torch.randn(1, 4, side, side, device="cuda")
    try:
        with torch.no_grad():
            row["peak_mib"] = round(peak_mib(lambda: vae.decode(z), True), 1)
            timed(lambda: vae.decode(z))
            t = [timed(lambda: vae.decode(z).sample) for _ in range(3)]
        row["ms"] = stats([a for a, _ in t])
        row["finite"] = bool(torch.isfinite(t[-1][1]).all())
        largest = side
        del t
    except (HipLaunchError, torch.OutOfMemoryError) as e:
        row["failed"] = stopped = f"{type(e).__name__}: {str(e)[:160]}"
    print(json.dumps(row), flush=True)
    vae.repack()
    torch.cuda.empty_cache()
    if stopped:
        break
print(json.dumps(dict(measure="largest untiled flash decode", latent=largest, pixels=None if largest is None else 8 * largest, stopped_by=stopped)), flush=True)
