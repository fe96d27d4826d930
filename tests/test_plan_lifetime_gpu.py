"""Who owns the plans: a ``DenoiseLoop`` built directly (not through the caches on the UNet) has no reference cycle - nothing reachable from an engine
refers back to the engine, the loop or the captured graph -, so ``del`` frees the loop, its engines and every recorder (with the tensors and parameter
blocks they keep alive for the graph) by reference counting, at a point the caller chooses, not at some later garbage collection."""
import gc
import weakref

import pytest
import torch

from tools import plan_signatures as ps

pytestmark = pytest.mark.gpu


def test_a_directly_built_loop_is_freed_by_reference_counting():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.pipeline import DenoiseLoop
    unet = ps.tiny_unet()
    B, S, P = 2, 16, 1
    g = torch.Generator().manual_seed(81)
    cond = tuple(t.cuda() for t in (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)))
    uncond = tuple(t.cuda() for t in (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)))
    noise = torch.randn(B, 4, S, S, generator=g)
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        # three forwards on three streams (three branches of the captured graph), stochastic solver step with the inpainting blend and the rescale
        loop = DenoiseLoop(unet, B, S, P, 3, 7.5, image_guidance_scale=5.0, guidance_rescale=0.7, stochastic=True, inpaint=True)
        loop.set_conditioning(cond, uncond)
        ps._half_mask(loop, g)
        loop.set_noise_stream(7)
        loop.reset(noise)
        loop.run()
        torch.cuda.synchronize()
        assert loop.graph is not None and len(loop.all_engines) == 3
        refs = {"loop": weakref.ref(loop)}
        for i, eng in enumerate(loop.all_engines):
            refs[f"engine {i}"] = weakref.ref(eng)
            for k in ("rec", "rec_head", "rec_tail", "rec_cond"):
                if getattr(eng, k) is not None:
                    refs[f"engine {i} {k}"] = weakref.ref(getattr(eng, k))
        del eng, loop
        alive = [k for k, r in refs.items() if r() is not None]
        assert not alive, f"still alive after del, without a garbage collection: {alive}"
    finally:
        if was_enabled:
            gc.enable()
