#!/usr/bin/env python3
"""Launch-for-launch, bit-for-bit signatures of the inference plans (GPU box): what ``tests/test_plan_signatures_gpu.py`` compares a working tree
with.  ``signature()`` reads what every plan recorded (launcher, kernel symbol, flops, bytes, workgroups per launch) and hashes the result of a
seeded run; ``main`` writes them for ``CASES`` to ``tests/golden/plan_signatures.json``.  The file is regenerated only when a change MEANS to alter a
launch list or the bits - from a checkout of the commit that is to be the reference, never from the code under test:

    python tools/plan_signatures.py [--commit HASH] [--out FILE] [case ...]

``--train``: the same for the training plans - every recorder of the ``TrainStep``s in ``TRAIN_CASES``, their dropout sites and fusion names, the sha256 of
loss and gradients after an eager and after a replayed step - to ``tests/golden/train_plan_signatures.json`` (``tests/test_train_plan_signatures_gpu.py``).

``--trace``: what one ``DenoiseLoop._step_eager()`` of every loop in ``TRACE_CASES`` issues, in order - recorder runs and stream waits with their streams,
logged instead of launched - and how many streams a build and a ``capture()`` construct, to ``tests/golden/step_traces.json``
(``tests/test_step_schedule_gpu.py``).  It reads only the engine lists, ``tail`` and ``_sides`` of a loop, so it records a commit that has no ``schedule``.
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


# ---------------------------------------------------------------------------------------------------------------- the step's order
TRACE_GOLDEN = os.path.join(ROOT, "tests", "golden", "step_traces.json")
#: the loops of ``CASES`` (the bare engines have no step).  Only plans are built, so the full-size loops shrink to B = 1 at 32 x 32 (their P stays)
TRACE_CASES = {name: dict(c, **(dict(B=1, S=32) if c["unet"] == "full" else {})) for name, c in CASES.items() if "kw" in c}


class _CountedStream(torch.cuda.Stream):
    """Counts the streams taken from torch's pool (``torch.cuda.current_stream()`` wraps an existing one by id: not counted)."""
    built = 0

    def __new__(cls, *a, **kw):
        _CountedStream.built += "stream_id" not in kw and "stream_ptr" not in kw
        return super().__new__(cls, *a, **kw)


class _NoGraph:
    """Stands in for ``torch.cuda.CUDAGraph`` and ``torch.cuda.graph`` while ``capture()`` is walked without capturing."""

    def __init__(self, *a, **kw):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def recorder_labels(loop) -> dict:
    """id(recorder) -> ``engines_u[0].rec`` ... / ``tail``: every recorder a step may run, named by where the loop holds it."""
    labels = {id(loop.tail): "tail"}
    for lst in ("engines_u", "engines_c", "engines_m", "engines_p", "engines_i", "engines_p_attn"):
        for i, e in enumerate(getattr(loop, lst)):
            for k in ("rec", "rec_head", "rec_tail"):
                if getattr(e, k) is not None:
                    labels[id(getattr(e, k))] = f"{lst}[{i}].{k}"
    return labels


def step_trace(loop) -> list:
    """What one ``loop._step_eager()`` issues, in order, with nothing launched: ``["run", stream, recorder label]`` and ``["wait", waiting stream,
    awaited stream]`` - stream 0 is the current stream, k is ``loop._sides[k - 1]``."""
    from unittest import mock
    from photoverse_amd.ops import Recorder
    labels = recorder_labels(loop)
    streams = [torch.cuda.current_stream().cuda_stream] + [s.cuda_stream for s in loop._sides]
    assert len(set(streams)) == len(streams), "two of the loop's streams are one stream"
    log = []
    with mock.patch.object(Recorder, "run", lambda rec, stream=None: log.append(["run", streams.index(torch.cuda.current_stream().cuda_stream), labels[id(rec)]])), \
            mock.patch.object(torch.cuda.Stream, "wait_stream", lambda s, other: log.append(["wait", streams.index(s.cuda_stream), streams.index(other.cuda_stream)])):
        loop._step_eager()
    return log


def trace_case(name: str, unet):
    """Build the loop of ``TRACE_CASES[name]`` and return (it, its trace record): ``step_trace`` and how many ``torch.cuda.Stream``s the build and a
    ``capture()`` construct (torch hands streams out of a fixed pool in turn: the count decides which later loops share one).  ``capture()`` is walked with the
    recorders, the stream waits and the graph replaced, so it launches and captures nothing; the loop is as built afterwards."""
    from unittest import mock
    from photoverse_amd.ops import Recorder
    from photoverse_amd.pipeline import DenoiseLoop
    c = TRACE_CASES[name]
    with mock.patch.object(torch.cuda, "Stream", _CountedStream):
        _CountedStream.built = 0
        loop = DenoiseLoop(unet, c["B"], c["S"], c["P"], c["steps"], 7.5, **c["kw"])
        built = _CountedStream.built
        with mock.patch.object(Recorder, "run", lambda rec, stream=None: None), mock.patch.object(torch.cuda, "CUDAGraph", _NoGraph), \
                mock.patch.object(torch.cuda, "graph", _NoGraph), mock.patch.object(torch.cuda.Stream, "wait_stream", lambda s, other: None):
            loop.capture()
        loop.graph = None
    return loop, dict(trace=step_trace(loop), streams_built=built, streams_capture=_CountedStream.built - built)


# ---------------------------------------------------------------------------------------------------------------- the training plans
TRAIN_GOLDEN = os.path.join(ROOT, "tests", "golden", "train_plan_signatures.json")
_TRAIN_TINY = dict(unet="tiny", B=2, S=16, E=3, lora_dropout=0.0, face=True, run=True)      # tests' test_training_step_is_bit_reproducible
#: name -> a ``TrainStep``: LoRA r = 4 with ``lora_dropout`` (None: no LoRA), the face-loss branch, and whether two seeded steps run (eager, then replayed)
TRAIN_CASES = {
    "train-tiny-lora-face": dict(_TRAIN_TINY),
    "train-tiny-lora-dropout-face": dict(_TRAIN_TINY, lora_dropout=0.1),       # the un-merged low-rank branches and their dropout sites
    "train-tiny-plain": dict(_TRAIN_TINY, E=1, lora_dropout=None, face=False),
    "train-full-built": dict(unet="full", B=1, S=32, E=1, lora_dropout=None, face=False, run=False),   # launch lists of the four-level walk
}
_VIS = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=3, image_size=56, patch_size=14)
_TXT = dict(vocab_size=49408, hidden_size=768, num_attention_heads=12, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=77)
_VAE = dict(block_out_channels=(128, 128, 256, 256), layers_per_block=1)


def _sha(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().float().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def train_recorders(step) -> dict:
    """Every recorder of a ``TrainStep`` by name: the main tape's two plans and, with the face loss, that branch's five."""
    recs = dict(rf=step.tape.rf, rb=step.tape.rb)
    if step.face is not None:
        f = step.face
        recs.update(face_rec_cond=f.rec_cond, face_loop_rf=f.loop_tape.rf, face_rec_stack=f.rec_stack, face_rec_last=f.rec_last, face_rb=f.tape.rb)
    return recs


def run_train_case(name: str, full=None) -> dict:
    """Build ``TRAIN_CASES[name]`` on seeded models (``full``: the SD-v1.5-sized UNet on the GPU for the case that wants one) and return its signature:
    every recorder's launch list, ``dropout_sites``, ``fusion_names`` and - where the case runs - the sha256 of (loss, face loss, every trainable
    gradient) after the first, eager step and after the second, replayed one on the same inputs."""
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.lora import LoraConfig
    from photoverse_amd.loss import FaceLoss
    from photoverse_amd.modeling_utils import load_models
    from photoverse_amd.train import TrainStep
    c = TRAIN_CASES[name]
    B, S, E, lora = c["B"], c["S"], c["E"], c["lora_dropout"] is not None
    _, text_encoder, vae, unet, _, image_adapter, text_adapter, scheduler, _ = load_models(
        None, E - 1, use_lora=lora, lora_config=LoraConfig(r=4, lora_alpha=4, lora_dropout=c["lora_dropout"]) if lora else None,
        unet_config=TINY_CONFIG, vision_config=_VIS, text_config=_TXT, vae_config=_VAE, seed=91)
    if c["unet"] == "full":
        unet = full
    for m in (unet, text_encoder, image_adapter, text_adapter, vae):
        m.to("cuda")
    torch.manual_seed(93)
    face = dict(face_loss=FaceLoss("cuda", "arcface"), vae=vae, face_samples=1, infer_steps=3, image_size=8 * S) if c["face"] else {}
    step = TrainStep(unet, text_encoder, text_adapter, image_adapter, batch=B, h=S, w=S, n_tokens=E, clip_tokens=17, clip_dim=256, grad_scale=512.0,
                     noise_scheduler=scheduler, **face)
    sig = dict(recorders={k: _launches(r) for k, r in train_recorders(step).items()}, dropout_sites=step.dropout_sites,
               fusion_names=step.fusion_names, sha256=[])
    if c["run"]:
        g = torch.Generator().manual_seed(92)
        fi = None
        if c["face"]:
            fi = dict(pixel_values=(torch.rand(1, 3, 8 * S, 8 * S, generator=g) * 2 - 1).cuda(), start_latents=torch.randn(1, 4, S, S, generator=g).cuda(),
                      image_embeddings=torch.randn(1, 17, 256, generator=g).half().cuda(),
                      uncond_image_embeddings=torch.randn(1, 17, 256, generator=g).half().cuda(),
                      text_input_ids=torch.randint(0, 1000, (1, 77), generator=g).cuda(), placeholder_idx=torch.tensor([[4]]).cuda(),
                      uncond_input_ids=torch.randint(0, 1000, (1, 77), generator=g).cuda(), forced_fusion=([0.5, 0.1, 0.9, 0.5], [0.9, 0.5, 0.5, 0.1]))
        kw = dict(noisy_latents=torch.randn(B, 4, S, S, generator=g).cuda(), noise=torch.randn(B, 4, S, S, generator=g).cuda(),
                  timesteps=torch.tensor([5, 900][:B]), text_input_ids=torch.randint(0, 1000, (B, 77), generator=g).cuda(),
                  placeholder_idx=torch.tensor([[2], [9]][:B]).cuda(), image_embeddings=[torch.randn(B, 17, 256, generator=g).half().cuda() for _ in range(E)],
                  forced_fusion=[0.1, 0.5, 0.9, 0.5], face_inputs=fi)
        params = [p for ps in step.trainable_parameters().values() for p in ps]
        for _ in range(2):                                  # the first step runs the plans eagerly, the second captures and replays them
            out = step.step(**kw)
            torch.cuda.synchronize()
            sig["sha256"].append(_sha([out["loss"]] + ([out["face_loss"]] if c["face"] else []) + [p.grad for p in params]))
        assert step.graph is not None and (step.face is None or step.face.graph is not None)
    return json.loads(json.dumps(sig))


def pack_train(sigs: dict, commit: str) -> dict:
    """``pack`` for the training signatures: one launch table, the recorders as index lists."""
    table = {}
    cases = json.loads(json.dumps(sigs))
    for sig in cases.values():
        sig["recorders"] = {k: [table.setdefault(json.dumps(launch), len(table)) for launch in v] for k, v in sig["recorders"].items()}
    return dict(commit=commit, launches=[json.loads(s) for s in table], cases=cases)


def unpack_train(doc: dict) -> dict:
    cases = json.loads(json.dumps(doc["cases"]))
    for sig in cases.values():
        sig["recorders"] = {k: [doc["launches"][i] for i in v] for k, v in sig["recorders"].items()}
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("cases", nargs="*", help="default: all")
    ap.add_argument("--commit", help="the commit this checkout is at (default: git rev-parse HEAD)")
    ap.add_argument("--out", help=f"default: {os.path.relpath(GOLDEN, ROOT)}, with --train {os.path.relpath(TRAIN_GOLDEN, ROOT)}")
    ap.add_argument("--train", action="store_true", help="the training plans (TRAIN_CASES) instead of the inference plans")
    ap.add_argument("--trace", action="store_true", help="the step traces of the loops (TRACE_CASES) instead of the plan signatures")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    unets, sigs = {}, {}
    if a.trace:
        for name in a.cases or list(TRACE_CASES):
            kind = TRACE_CASES[name]["unet"]
            if kind not in unets:
                unets[kind] = tiny_unet() if kind == "tiny" else full_unet()
            sigs[name] = trace_case(name, unets[kind])[1]
            print(f"{name}: {len(sigs[name]['trace'])} stream operations and recorder runs, streams {sigs[name]['streams_built']} + "
                  f"{sigs[name]['streams_capture']}", flush=True)
        with open(a.out or TRACE_GOLDEN, "w") as f:
            json.dump(dict(commit=commit, cases=sigs), f, indent=0, separators=(",", ":"))
            f.write("\n")
        return
    if a.train:
        for name in a.cases or list(TRAIN_CASES):
            sigs[name] = run_train_case(name, full_unet() if TRAIN_CASES[name]["unet"] == "full" else None)
            print(f"{name}: {', '.join(f'{k} {len(v)}' for k, v in sigs[name]['recorders'].items())} launches, sha256 "
                  f"{[s[:16] for s in sigs[name]['sha256']]}", flush=True)
        with open(a.out or TRAIN_GOLDEN, "w") as f:
            json.dump(pack_train(sigs, commit), f, separators=(",", ":"))
            f.write("\n")
        return
    for name in a.cases or list(CASES):
        kind = CASES[name]["unet"]
        if kind not in unets:
            unets[kind] = tiny_unet() if kind == "tiny" else full_unet()
        sigs[name] = run_case(name, unets[kind])
        print(f"{name}: {sigs[name]['launches_per_step']} launches per step, sha256 {sigs[name]['sha256'][:16]}", flush=True)
    with open(a.out or GOLDEN, "w") as f:
        json.dump(pack(sigs, commit), f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
