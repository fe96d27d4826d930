"""CPU-only tests of DeepCache-style feature reuse, as far as it is built (``photoverse_amd/deepcache.py``: the host-side plan layer): the two ranges of a
cached forward on the stage lists of SD-1.5 and of the tiny model, the stacked time projection of its resnets, the host-side choice between a full and a
cached step, the keyword checks, and the fp32 reference of the definition - ``cached_forward_ref`` / ``cached_oracle_loop``, walks over the oracle's own
modules - checked against the oracle's forward and shown to move the result by far more than the project's GPU tolerances, so that a GPU comparison
against it can tell caching from no caching."""
import math

import pytest
import torch

from test_pag_cpu import B, G_TEXT, S, TOL_FWD, TOL_LOOP, loop_inputs_81, rel_l2, tiny_oracle


# ---------------------------------------------------------------------------------------------------------------- the fp32 reference
def _walk(ref):
    """The oracle's forward as ``(name, function of (x, skip, emb, ehs), skip)`` in execution order: skip +1 - the output is pushed, -1 - the newest skip
    is popped and concatenated behind ``x``."""
    ops = [("conv_in", lambda x, sk, emb, ehs: ref.conv_in(x), +1)]

    def res(m):
        return lambda x, sk, emb, ehs: m(x if sk is None else torch.cat([x, sk], dim=1), emb)

    def att(m):
        return lambda x, sk, emb, ehs: m(x, encoder_hidden_states=ehs)

    def plain(m):
        return lambda x, sk, emb, ehs: m(x)

    for bi, blk in enumerate(ref.down_blocks):
        for i, r in enumerate(blk.resnets):
            ops.append((f"down_blocks.{bi}.resnets.{i}", res(r), 0 if blk.has_attn else +1))
            if blk.has_attn:
                ops.append((f"down_blocks.{bi}.attentions.{i}", att(blk.attentions[i]), +1))
        if blk.downsamplers is not None:
            ops.append((f"down_blocks.{bi}.downsamplers.0", plain(blk.downsamplers[0]), +1))
    mb = ref.mid_block
    ops += [("mid_block.resnets.0", res(mb.resnets[0]), 0), ("mid_block.attentions.0", att(mb.attentions[0]), 0), ("mid_block.resnets.1", res(mb.resnets[1]), 0)]
    for bi, blk in enumerate(ref.up_blocks):
        for i, r in enumerate(blk.resnets):
            ops.append((f"up_blocks.{bi}.resnets.{i}", res(r), -1))
            if blk.has_attn:
                ops.append((f"up_blocks.{bi}.attentions.{i}", att(blk.attentions[i]), 0))
        if blk.upsamplers is not None:
            ops.append((f"up_blocks.{bi}.upsamplers.0", plain(blk.upsamplers[0]), 0))
    ops.append(("conv_out", lambda x, sk, emb, ehs: ref.conv_out(ref.conv_act(ref.conv_norm_out(x))), 0))
    return ops


def max_depth_ref(ref):
    """The skip-pushing stages of the first resolution level, its downsample excluded."""
    blk = ref.down_blocks[0]
    return 1 + len(blk.resnets)


@torch.no_grad()
def cached_forward_ref(ref, x, t, ehs, cache=None, depth=None):
    """The issue's definition on the fp32 oracle's modules.  ``cache=None``: a full forward -> ``(prediction, {d: C_d})``, ``C_d`` the activation in front
    of the up-path resnet that pops the d-th pushed skip, before the concat.  Otherwise the cached forward at ``(x, t, ehs)``: time embedding, the down
    path up to the ``depth``-th push, ``cache[depth]`` unchanged, the up path from that resnet -> ``(prediction, cache)``."""
    from oracle.unet_ref import timestep_embedding_ref
    ts = t if torch.is_tensor(t) else torch.tensor([t], dtype=torch.int64)
    ts = (ts[None] if ts.ndim == 0 else ts).expand(x.shape[0])
    emb = ref.time_embedding(timestep_embedding_ref(ts, ref.config.block_out_channels[0]).to(x.dtype))
    ops, top = _walk(ref), max_depth_ref(ref)
    skips, points, h = [], {}, x
    if cache is None:
        for _, fn, skip in ops:
            sk = None
            if skip < 0:
                if len(skips) <= top:
                    points[len(skips)] = h
                sk = skips.pop()
            h = fn(h, sk, emb, ehs)
            if skip > 0:
                skips.append(h)
        assert not skips and sorted(points) == list(range(1, top + 1))
        return h, points
    assert 1 <= depth <= top
    it = iter(enumerate(ops))
    for _, (_, fn, skip) in it:                              # the down range: up to the depth-th push
        h = fn(h, None, emb, ehs)
        if skip > 0:
            skips.append(h)
            if len(skips) == depth:
                break
    held, entry = 0, None                                    # the up range starts where a full forward's skip stack holds ``depth`` entries
    for i, (_, _, skip) in enumerate(ops):
        if skip < 0:
            if held == depth:
                entry = i
                break
            held -= 1
        elif skip > 0:
            held += 1
    h = cache[depth]
    for _, fn, skip in ops[entry:]:
        h = fn(h, skips.pop() if skip < 0 else None, emb, ehs)
    assert not skips
    return h, cache


@torch.no_grad()
def cached_oracle_loop(ref, cond, uncond, noise, g_text, steps, interval=None, depth=2, start=0, g_image=None, rescale=0.0):
    """The denoising loop on the fp32 oracle with the issue's schedule: step ``i`` is full when ``(i - start) % interval == 0`` (always without
    ``interval``), cached otherwise, every branch (uncond, cond, image-only) on the cache points of its own last full forward.  ``DPMSolverMultistepRef`` started
    at row ``start`` and the formulas of ``test_pag_cpu.oracle_loop``.  ``noise``: the latents at row ``start``."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(steps)
    sch.step_index = start
    x = (noise * sch.init_noise_sigma).float()
    branches = {"u": uncond, "c": cond}
    if g_image is not None:
        branches["m"] = (uncond[0], cond[1])
    caches = {}
    for i in range(start, steps):
        t = sch.timesteps[i]
        full = interval is None or (i - start) % interval == 0
        eps = {}
        for k, ehs in branches.items():
            if full:
                eps[k], caches[k] = cached_forward_ref(ref, x, t, ehs)
            else:
                eps[k], _ = cached_forward_ref(ref, x, t, ehs, cache=caches[k], depth=depth)
        eu, ec = eps["u"], eps["c"]
        e = eu + g_text * (ec - eu) if g_image is None else eu + g_image * (eps["m"] - eu) + g_text * (ec - eps["m"])
        if rescale > 0:
            f = rescale * ec.flatten(1).std(dim=1) / e.flatten(1).std(dim=1) + (1 - rescale)
            e = f.view(-1, 1, 1, 1) * e
        x = sch.step(e, t, x)
    return x


# ---------------------------------------------------------------------------------------------------------------- the plan layer
SD15_RANGES = {1: (["conv_in"], ["up_blocks.3.resnets.2", "up_blocks.3.attentions.2", "conv_out"]),
               2: (["conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0"],
                   ["up_blocks.3.resnets.1", "up_blocks.3.attentions.1", "up_blocks.3.resnets.2", "up_blocks.3.attentions.2", "conv_out"]),
               3: (["conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "down_blocks.0.resnets.1", "down_blocks.0.attentions.1"],
                   ["up_blocks.3.resnets.0", "up_blocks.3.attentions.0", "up_blocks.3.resnets.1", "up_blocks.3.attentions.1", "up_blocks.3.resnets.2",
                    "up_blocks.3.attentions.2", "conv_out"])}
TINY_RANGES = {1: (["conv_in"], ["up_blocks.1.resnets.1", "up_blocks.1.attentions.1", "conv_out"]),
               2: (["conv_in", "down_blocks.0.resnets.0", "down_blocks.0.attentions.0"],
                   ["up_blocks.1.resnets.0", "up_blocks.1.attentions.0", "up_blocks.1.resnets.1", "up_blocks.1.attentions.1", "conv_out"])}
#: the stage in front of the up range: its output is the cache point
SD15_BEFORE = {1: "up_blocks.3.attentions.1", 2: "up_blocks.3.attentions.0", 3: "up_blocks.2.upsamplers.0"}
TINY_BEFORE = {1: "up_blocks.1.attentions.0", 2: "up_blocks.0.upsamplers.0"}


def _meta_unet(**cfg):
    from photoverse_amd.unet import UNet2DConditionModel
    with torch.device("meta"):
        return UNet2DConditionModel(**cfg)


@pytest.mark.parametrize("which", ["sd15", "tiny"])
def test_shallow_plan_ranges(which):
    """``shallow_ranges(stages, d)``: the exact stage names of both ranges for every valid ``d``, the second adopting ``"cache"``; the down range pushes
    exactly ``d`` skips and the up range pops exactly those, on the first resolution level only; ``d = 0`` and ``d = max + 1`` are ``ValueError``s."""
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.deepcache import cache_entry, max_cache_depth, shallow_ranges
    from photoverse_amd.unet import unet_stages
    unet, want, before = (_meta_unet(), SD15_RANGES, SD15_BEFORE) if which == "sd15" else (_meta_unet(**TINY_CONFIG), TINY_RANGES, TINY_BEFORE)
    stages = unet_stages(unet)
    assert max_cache_depth(stages) == len(want)
    for d, (down, up) in want.items():
        ranges = shallow_ranges(stages, d)
        assert len(ranges) == 2
        (a0, a1, adopts_a, writes_a), (b0, b1, adopts_b, writes_b) = ranges
        assert (a0, adopts_a, writes_a, adopts_b, writes_b, b1) == (0, None, None, "cache", None, len(stages) - 1)
        assert [st.name for st in stages[a0:a1 + 1]] == down and [st.name for st in stages[b0:b1 + 1]] == up
        assert sum(st.skip for st in stages[a0:a1 + 1]) == d == -sum(st.skip for st in stages[b0:b1 + 1])
        assert stages[b0].skip < 0 and stages[b0 - 1].name == before[d] and cache_entry(stages, d) == b0
        assert all(st.level == 0 for st in stages[a0:a1 + 1] + stages[b0:b1 + 1])             # never below the first resolution level
    for bad in (0, len(want) + 1, -1, None, 1.0, True, "2"):
        with pytest.raises(ValueError, match="cache_depth"):
            shallow_ranges(stages, bad)


def test_time_projection_of_a_shallow_plan_holds_only_its_resnets():
    """``shallow_time_projection``: the ``time_emb_proj`` rows of the resnets a cached forward records, in recording order, each with its first column, and
    zero padding to whole 160-column tiles."""
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.deepcache import shallow_ranges, shallow_time_projection
    from photoverse_amd.unet import UNet2DConditionModel, time_projection, time_projection_width, unet_stages
    torch.manual_seed(0)
    unet = UNet2DConditionModel(**TINY_CONFIG)
    stages = unet_stages(unet)
    full_w, _ = time_projection(stages)
    for d, n_res in ((1, 1), (2, 3)):
        (a0, a1, _, _), (b0, b1, _, _) = shallow_ranges(stages, d)
        own = [st for st in stages[a0:a1 + 1] + stages[b0:b1 + 1] if st.kind == "resnet"]
        assert len(own) == n_res
        wt, bt, toff = shallow_time_projection(stages, d)
        assert list(toff) == [st.name for st in own]
        assert wt.shape[0] == bt.shape[0] == time_projection_width(own) < full_w.shape[0] and wt.shape[0] % 160 == 0
        off = 0
        for st in own:
            assert toff[st.name] == off
            assert torch.equal(wt[off:off + st.tcols], full_w[st.toff:st.toff + st.tcols])
            assert torch.equal(bt[off:off + st.tcols], st.module.time_emb_proj.bias.detach().float())
            off += st.tcols
        assert not wt[off:].any() and not bt[off:].any()


# ---------------------------------------------------------------------------------------------------------------- full or cached
@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("interval", [2, 3])
def test_full_and_cached_steps_follow_the_schedule(start, interval):
    """T = 6: step ``i`` is full when ``(i - start) % N == 0``; the first step after a reset (validity flag cleared) is full whatever its row, and the
    schedule goes on from ``start`` behind it; ``None`` is full everywhere."""
    from photoverse_amd.deepcache import cached_step_is_full
    T = 6
    valid, kinds = False, []
    for i in range(start, T):
        full = cached_step_is_full(i, start, interval, valid)
        valid = valid or full
        kinds.append(full)
    assert kinds == [(i - start) % interval == 0 for i in range(start, T)] and kinds[0]
    assert all(cached_step_is_full(i, start, None, v) for i in range(start, T) for v in (False, True))
    # a reset() / set_conditioning() in mid-run: the next step is full, then the rows decide again
    for at in range(start + 1, T):
        valid, kinds = True, []
        for i in range(at, T):
            if i == at:
                valid = False
            full = cached_step_is_full(i, start, interval, valid)
            valid = valid or full
            kinds.append(full)
        assert kinds == [True] + [(i - start) % interval == 0 for i in range(at + 1, T)]


# ---------------------------------------------------------------------------------------------------------------- keyword checks
def test_keyword_checks():
    from photoverse_amd.deepcache import check_cache_depth, check_cache_interval
    from photoverse_amd.unet import unet_stages
    assert check_cache_interval(None) is None and check_cache_interval(1) is None and check_cache_interval(2) == 2 and check_cache_interval(50) == 50
    for bad in (0, -2, 2.0, "2", True, math.nan, [2]):
        with pytest.raises(ValueError, match="cache_interval"):
            check_cache_interval(bad)
        with pytest.raises(ValueError, match="hires_cache_interval"):
            check_cache_interval(bad, "hires_cache_interval")
    stages = unet_stages(_meta_unet())
    assert [check_cache_depth(stages, d) for d in (1, 2, 3)] == [1, 2, 3]
    for bad in (0, 4, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="cache_depth.*1 ... 3"):
            check_cache_depth(stages, bad)


# ---------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.fixture(scope="module")
def oracle():
    return tiny_oracle()


@pytest.fixture(scope="module")
def inputs():
    return loop_inputs_81()


@torch.no_grad()
def test_reference_full_walk_is_the_oracle_forward(oracle, inputs):
    """(a) ``cached_forward_ref`` without a cache equals ``ref(x, t, ...).sample`` exactly, at a step's timestep and inside a loop (two more inputs), and
    returns a cache point per valid depth with the first level's shape."""
    cond, uncond, noise = inputs
    g = torch.Generator().manual_seed(7)
    for x, t, ehs in ((noise, 500, cond), (noise * 0.5 + 0.2 * torch.randn(noise.shape, generator=g), torch.tensor(981), uncond),
                      (torch.randn(noise.shape, generator=g), torch.tensor([20]), (uncond[0], cond[1]))):
        got, points = cached_forward_ref(oracle, x, t, ehs)
        assert torch.equal(got, oracle(x, t, encoder_hidden_states=ehs).sample)
        assert sorted(points) == [1, 2] and points[1].shape == (B, 320, S, S) and points[2].shape == (B, 640, S, S)


@torch.no_grad()
def test_reference_cached_forward_from_its_own_cache_is_the_full_forward(oracle, inputs):
    """(b) at the same ``(x, t)``, from the cache points of that very forward, a cached forward equals the full one exactly for every valid depth - on the
    tiny model and on one with two layers per block (depths 1 ... 3)."""
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    cond, _, noise = inputs
    torch.manual_seed(1)
    deep = UNet2DConditionModelRef(**dict(TINY_CONFIG, layers_per_block=2)).eval()
    set_visual_cross_attention_adapter_ref(deep, (5,))
    for ref, depths in ((oracle, (1, 2)), (deep, (1, 2, 3))):
        full, points = cached_forward_ref(ref, noise, 500, cond)
        assert sorted(points) == list(depths)
        for d in depths:
            got, _ = cached_forward_ref(ref, noise, 500, cond, cache=points, depth=d)
            assert torch.equal(got, full), d


@torch.no_grad()
def test_reference_caching_moves_the_result_far_beyond_the_gpu_tolerances(oracle, inputs):
    """(c) what the GPU comparison can tell apart.  The oracle loop with caching differs from the plain oracle loop by at least ten times TOL_LOOP for
    d in {1, 2}, N in {2, 3}, 4 and 6 steps (measured: 4.5e-2 ... 1.1e-1); a cached forward at an input moved by 0.3 randn and a timestep moved by 200
    differs from the full forward there by at least ten times TOL_FWD (measured: 0.19 ... 0.29).  ``interval=None`` is the plain ``oracle_loop``."""
    from test_pag_cpu import oracle_loop
    cond, uncond, noise = inputs
    for steps in (4, 6):
        plain = cached_oracle_loop(oracle, cond, uncond, noise, G_TEXT, steps)
        assert torch.equal(plain, oracle_loop(oracle, None, cond, uncond, noise, G_TEXT, steps=steps))
        if steps == 4:                            # ... with three forwards and the rescale too
            assert torch.equal(cached_oracle_loop(oracle, cond, uncond, noise, G_TEXT, steps, g_image=2.0, rescale=0.7),
                               oracle_loop(oracle, None, cond, uncond, noise, G_TEXT, g_image=2.0, rescale=0.7, steps=steps))
        for d in (1, 2):
            for n in (2, 3):
                away = rel_l2(cached_oracle_loop(oracle, cond, uncond, noise, G_TEXT, steps, interval=n, depth=d), plain)
                print(f"oracle loop, {steps} steps, cache_interval {n}, cache_depth {d}: rel-L2 from the plain loop = {away:.3e}")
                assert away > 10 * TOL_LOOP
    g = torch.Generator().manual_seed(9)
    x2 = noise + 0.3 * torch.randn(noise.shape, generator=g)
    _, points = cached_forward_ref(oracle, noise, 700, cond)
    full2, _ = cached_forward_ref(oracle, x2, 500, cond)
    for d in (1, 2):
        got, _ = cached_forward_ref(oracle, x2, 500, cond, cache=points, depth=d)
        away = rel_l2(got, full2)
        print(f"cached forward, depth {d}, input moved by 0.3 randn, timestep 700 -> 500: rel-L2 from the full forward = {away:.3e}")
        assert away > 10 * TOL_FWD
