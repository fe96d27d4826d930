#!/usr/bin/env python3
"""Launch-for-launch, bit-for-bit signatures of the inference plans (GPU box): what ``tests/test_plan_signatures_gpu.py`` compares a working tree
with.  ``signature()`` reads what every plan recorded (launcher, kernel symbol, flops, bytes, workgroups per launch) and hashes the result of a
seeded run; ``main`` writes them for ``CASES`` to ``tests/golden/plan_signatures.json``.  The file is regenerated only when a change MEANS to alter a
launch list or the bits - from a checkout of the commit that is to be the reference, never from the code under test:

    python tools/plan_signatures.py [--commit HASH] [--out FILE] [case ...]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_signatures.json")
FREEU = (1.5, 1.6, 0.9, 0.2)
TINY = dict(unet="tiny", B=2, S=16, P=1, steps=3)
FULL = dict(unet="full", B=2, S=32, P=1, steps=2)     # merging needs four levels; 32 x 32: the smallest seam with whole 64-row statistics blocks


def _half_mask(loop, g):
    mask = torch.ones(loop.B, 1, loop.S, loop.S)
    mask[:, :, :, :loop.S // 2] = 0.0
    shape = tuple(loop.latents.shape)
    loop.set_inpaint(mask.cuda(), torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda())


#: name -> shape, ``DenoiseLoop`` keywords (``engine``: ``unet.engine`` keywords of a bare plan instead) and what fills a feature's static buffers
CASES = {
    "tiny-default": dict(TINY, kw={}),
    "tiny-onestream-eager": dict(TINY, kw=dict(two_streams=False, use_graph=False)),
    "tiny-share-prefix": dict(TINY, kw=dict(share_prefix=True)),
    "tiny-batch-splits": dict(TINY, kw=dict(batch_splits=2)),
    "tiny-training-mode": dict(TINY, kw=dict(training_mode=True, fusion_seed=3)),
    "tiny-image-guidance-rescale": dict(TINY, kw=dict(image_guidance_scale=5.0, guidance_rescale=0.7)),
    "tiny-inpaint": dict(TINY, kw=dict(inpaint=True), prepare=_half_mask),
    "tiny-stochastic": dict(TINY, kw=dict(stochastic=True), prepare=lambda loop, g: loop.set_noise_stream(7)),
    "tiny-pag-mid": dict(TINY, kw=dict(pag_scale=2.0, pag_layers=("mid_block",))),
    "tiny-pag-up-prefix": dict(TINY, kw=dict(pag_scale=2.0, pag_layers=("up_blocks.1.attentions.0",), share_prefix=True)),
    "tiny-pag-first-no-trunk": dict(TINY, kw=dict(pag_scale=2.0, pag_layers=("down_blocks.0.attentions.0",), share_prefix=True, share_trunk=False)),
    "tiny-freeu-pag": dict(TINY, kw=dict(freeu=FREEU, pag_scale=2.0, pag_layers=("mid_block",))),
    "tiny-engine": dict(TINY, engine={}),
    "tiny-engine-device-fusion": dict(TINY, engine=dict(device_fusion="always", fusion_seed=3)),
    "full-merge": dict(FULL, kw=dict(merge_lowres=True)),
    "full-merge-prefix-freeu": dict(FULL, kw=dict(merge_lowres=True, share_prefix=True, freeu=FREEU)),
    "full-merge-96-p6": dict(FULL, S=96, P=6, kw=dict(merge_lowres=True)),       # 9 statistics blocks per sample at the seam
}


_RECS = ("rec", "rec_head", "rec_tail", "rec_cond")


def _launches(rec):
    return None if rec is None else [[fn.__name__, *tag] for (fn, _), tag in zip(rec.calls, rec.tags)]


def signature(obj) -> dict:
    """``obj``: a ``DenoiseLoop`` after its run, or a ``UNetEngine`` after its forward."""
    loop = obj if hasattr(obj, "all_engines") else None
    engines = loop.all_engines if loop is not None else [obj]
    result = loop.latents if loop is not None else obj.out
    sig = dict(engines=[{k: _launches(getattr(e, k)) for k in _RECS} for e in engines],
               tail=[fn.__name__ for fn, _ in loop.tail.calls] if loop is not None else [],
               launches_per_step=loop.launches_per_step if loop is not None else len(obj.rec),
               sides=len(loop._sides) if loop is not None else 0,
               flags={k: bool(getattr(loop, k, False)) for k in ("merge_lowres", "share_prefix", "share_trunk")},
               sha256=hashlib.sha256(result.detach().float().contiguous().cpu().numpy().tobytes()).hexdigest())
    return json.loads(json.dumps(sig))          # tuples as lists: what the committed file gives back


def tiny_unet():
    """The tiny UNet with the seeded weights of ``tests/test_pag_cpu.py::tiny_oracle``, on the GPU."""
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    torch.manual_seed(0)
    ref = UNet2DConditionModelRef(**TINY_CONFIG).eval()
    set_visual_cross_attention_adapter_ref(ref, (5,))
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.to("cuda")


def full_unet():
    """The SD-v1.5-sized UNet with ``oracle.fullsize``'s seeded weights, on the GPU (the tests' ``full_hip_unet``)."""
    from oracle import fullsize as fs
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    with fs.no_init():
        hip = UNet2DConditionModel()
        set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(fs.unet_state())
    return hip.to("cuda")


def run_case(name: str, unet) -> dict:
    """Build case ``name`` on ``unet`` (the tiny or the full-size one, as ``CASES[name]["unet"]`` says), run it on seeded inputs, return its signature."""
    from photoverse_amd.pipeline import DenoiseLoop
    c = CASES[name]
    B, S, P = c["B"], c["S"], c["P"]
    g = torch.Generator().manual_seed(81)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)
    if "engine" in c:
        eng = unet.engine(B, S, S, P, B if c["engine"] else 1, **c["engine"])
        eng.x_in.copy_(noise)
        eng.text.copy_(cond[0].reshape(eng.text.shape))
        eng.ip.copy_(cond[1].reshape(eng.ip.shape))
        eng.timesteps.fill_(500.0)
        eng.run()
        torch.cuda.synchronize()
        return signature(eng)
    loop = DenoiseLoop(unet, B, S, P, c["steps"], 7.5, **c["kw"])
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    if "prepare" in c:
        c["prepare"](loop, g)
    loop.reset(noise)
    loop.run()
    torch.cuda.synchronize()
    return signature(loop)


def pack(sigs: dict, commit: str) -> dict:
    """The committed form: every distinct launch once, in a table; the plans as lists of indices into it (the same launch recurs across plans and cases)."""
    table = {}
    cases = json.loads(json.dumps(sigs))
    for sig in cases.values():
        for e in sig["engines"]:
            for k in _RECS:
                if e[k] is not None:
                    e[k] = [table.setdefault(json.dumps(launch), len(table)) for launch in e[k]]
    return dict(commit=commit, launches=[json.loads(s) for s in table], cases=cases)


def unpack(doc: dict) -> dict:
    """``pack``'s inverse: name -> signature."""
    cases = json.loads(json.dumps(doc["cases"]))
    for sig in cases.values():
        for e in sig["engines"]:
            for k in _RECS:
                if e[k] is not None:
                    e[k] = [doc["launches"][i] for i in e[k]]
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("cases", nargs="*", help="default: all")
    ap.add_argument("--commit", help="the commit this checkout is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    unets, sigs = {}, {}
    for name in a.cases or list(CASES):
        kind = CASES[name]["unet"]
        if kind not in unets:
            unets[kind] = tiny_unet() if kind == "tiny" else full_unet()
        sigs[name] = run_case(name, unets[kind])
        print(f"{name}: {sigs[name]['launches_per_step']} launches per step, sha256 {sigs[name]['sha256'][:16]}", flush=True)
    with open(a.out, "w") as f:
        json.dump(pack(sigs, commit), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
