"""Who owns the plans: a ``DenoiseLoop`` built directly (not through the caches on the UNet) has no reference cycle - nothing reachable from an engine
refers back to the engine, the loop or the captured graph -, so ``del`` frees the loop, its engines and every recorder (with the tensors and parameter
blocks they keep alive for the graph) by reference counting, at a point the caller chooses, not at some later garbage collection."""
import gc
import weakref

import pytest
import torch

from tools import plan_signatures as ps

pytestmark = pytest.mark.gpu

#: name -> UNet, shape, ``DenoiseLoop`` keywords, what fills the static buffers, the plans it must have
LOOPS = {
    # three forwards on three streams (three branches of the captured graph), stochastic solver step with the inpainting blend and the rescale
    "three-forwards-stochastic-inpaint": dict(unet="tiny", B=2, S=16, kw=dict(image_guidance_scale=5.0, guidance_rescale=0.7, stochastic=True, inpaint=True),
                                              prepare=lambda loop, g: (ps._half_mask(loop, g), loop.set_noise_stream(7)), engines=3),
    # prefix plan + the perturbed plan on its conditional plan's trunk: an engine that refers to another engine (one way)
    "pag-prefix-trunk": dict(unet="tiny", B=2, S=16, kw=dict(pag_scale=2.0, share_prefix=True), engines=4),
    # outer plans (``rec_head`` / ``rec_tail`` and the ``Recorder.concat`` view over them as ``rec``) around the merged plan
    "full-merged": dict(unet="full", B=1, S=32, kw=dict(merge_lowres=True), engines=3),
}


def _weak_refs(loop) -> dict:
    refs = {"loop": weakref.ref(loop), "tail": weakref.ref(loop.tail)}
    for i, eng in enumerate(loop.all_engines):
        refs[f"engine {i}"] = weakref.ref(eng)
        for k in ("rec", "rec_head", "rec_tail", "rec_cond"):
            if getattr(eng, k) is not None:
                refs[f"engine {i} {k}"] = weakref.ref(getattr(eng, k))
    # the schedule's tuples take no weak reference: the recorders they hold (a loop of a commit before the schedule has none)
    for i, group in enumerate(getattr(loop, "schedule", ())):
        for j, lane in enumerate(group):
            for k, rec in enumerate(lane):
                refs[f"schedule {i}.{j}.{k}"] = weakref.ref(rec)
    return refs


@pytest.mark.parametrize("name", list(LOOPS))
def test_a_directly_built_loop_is_freed_by_reference_counting(name, request):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.pipeline import DenoiseLoop
    c = LOOPS[name]
    unet = ps.tiny_unet() if c["unet"] == "tiny" else request.getfixturevalue("full_hip_unet")
    B, S, P = c["B"], c["S"], 1
    g = torch.Generator().manual_seed(81)
    cond = tuple(t.cuda() for t in (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)))
    uncond = tuple(t.cuda() for t in (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)))
    noise = torch.randn(B, 4, S, S, generator=g)
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        loop = DenoiseLoop(unet, B, S, P, 3, 7.5, **c["kw"])
        loop.set_conditioning(cond, uncond)
        if "prepare" in c:
            c["prepare"](loop, g)
        loop.reset(noise)
        loop.run()
        torch.cuda.synchronize()
        assert loop.graph is not None and len(loop.all_engines) == c["engines"]
        assert (name != "pag-prefix-trunk" or (loop.share_prefix and loop.share_trunk)) and (name != "full-merged" or loop.merge_lowres)
        refs = _weak_refs(loop)
        del loop
        alive = [k for k, r in refs.items() if r() is not None]
        assert not alive, f"still alive after del, without a garbage collection: {alive}"
    finally:
        if was_enabled:
            gc.enable()
