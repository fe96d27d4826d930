"""GPU tests of token downsampling (``kv_downsample``): ``pv_token_pool`` against the per-block-loop reference of ``tests/test_kv_downsample_cpu.py``;
``pv_attention`` with fewer keys than queries in every kernel form the feature reaches; ``UNetEngine(kv_downsample=...)`` against the fp32 oracle with
``PooledAttnProcessorRef`` on the same layers; the ``DenoiseLoop`` against the oracle loop, graph == eager, with the shared prefix, PAG on a shared
trunk and a ControlNet; ``run_inference`` / the CLI end to end on the tiny models."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_kv_downsample_cpu import ALL, METHODS, TOP, pool_rows_ref, pooled_oracle
from test_pag_cpu import B, G_PAG, G_TEXT, P, S, STEPS, TOL_FWD, TOL_LOOP, loop_inputs_81, oracle_loop, perturbed_oracle, rel_l2, tiny_oracle

pytestmark = pytest.mark.gpu

MID = ("mid_block.attentions.0",)
POOL = "pv_token_pool"


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


# ---------------------------------------------------------------------------------------------------------------- the kernel
#: (batch, h, w, cols, ldx, f)
POOL_SHAPES = ((1, 2, 2, 8, 8, 2),            # one block
               (1, 2, 3, 8, 8, 4),            # f larger than the grid: one output pixel over 6
               (1, 3, 3, 16, 16, 3),          # an exact fit at f = 3
               (1, 5, 7, 40, 48, 2),          # odd sides, h != w, padded stride
               (2, 6, 6, 640, 960, 4),        # edge blocks 2 wide; input at column offset 320 of a 960-wide buffer
               (2, 16, 16, 640, 960, 2))      # the tiny UNet's own shape
CANARY, GUARD = -7.25, 3


def _ordered(t16):
    """fp16 -> int32 that orders like the values (+-0 -> 0): neighbouring fp16 numbers differ by 1."""
    bits = t16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_token_pool_kernel(rec_cls, shape, method):
    """``Recorder.token_pool`` on a column slice (the last ``cols`` columns of an ``ldx``-wide buffer) into a column slice of a wider, canary-filled buffer
    with guard rows.  ``nearest``: the bits of ``[::f, ::f]``.  ``avg``: within one fp16 ulp of the fp64 block mean rounded to fp16 - the kernel adds at most
    64 fp16 terms in fp32 (relative error <= 63 * 2^-24 of the sum of magnitudes; the inputs here are N(0, 4^2), no catastrophic cancellation is needed
    for the claim: an fp32 error of that size moves the fp16 rounding by at most one step) and rounds once.  The input and everything outside the output
    slice are unchanged."""
    batch, h, w, cols, ldx, f = shape
    g = torch.Generator().manual_seed(sum(shape))
    buf = (torch.randn(batch * h * w, ldx, generator=g) * 4).half()
    d_buf = buf.cuda()
    x = d_buf[:, ldx - cols:]
    hp, wp = -(-h // f), -(-w // f)
    rows = batch * hp * wp
    d_out = torch.full((rows + 2 * GUARD, cols + 16), CANARY, dtype=torch.float16, device="cuda")
    out = d_out[GUARD:GUARD + rows, 8:8 + cols]
    rec = rec_cls("cuda")
    got = rec.token_pool(x, batch=batch, h=h, w=w, factor=f, method=method, out=out)
    assert got is out and len(rec) == 1 and rec.calls[0][0].__name__ == POOL and rec.tags[0][0] == "token_pool_kernel" and rec.tags[0][2] > 0
    rec.run()
    torch.cuda.synchronize()
    res = d_out.cpu()
    got = res[GUARD:GUARD + rows, 8:8 + cols].clone()
    ref = pool_rows_ref(buf[:, ldx - cols:], batch, h, w, f, method)
    assert got.shape == ref.shape == (rows, cols)
    if method == "nearest":
        assert torch.equal(got.view(torch.int16), ref.half().view(torch.int16))
    else:
        steps = (_ordered(got) - _ordered(ref.half())).abs().max().item()
        print(f"token_pool avg {shape}: largest distance from fp16(fp64 mean) = {steps} fp16 step(s), max |d| = {(got.double() - ref).abs().max().item():.3e}")
        assert torch.isfinite(got).all() and steps <= 1
    assert torch.equal(d_buf.cpu().view(torch.int16), buf.view(torch.int16))                       # the input is read only
    res[GUARD:GUARD + rows, 8:8 + cols] = CANARY
    assert (res == CANARY).all()                                                                   # guard rows and the columns beside the slice
    # a fresh output buffer of the recorder's own gives the same bits
    rec2 = rec_cls("cuda")
    own = rec2.token_pool(x, batch=batch, h=h, w=w, factor=f, method=method)
    rec2.run()
    torch.cuda.synchronize()
    assert own.shape == (rows, cols) and own.is_contiguous() and torch.equal(own.cpu().view(torch.int16), got.contiguous().view(torch.int16))
    with pytest.raises(ValueError, match="method"):
        rec2.token_pool(x, batch=batch, h=h, w=w, factor=f, method="max")


# ---------------------------------------------------------------------------------------------------------------- pv_attention at nq != nk
@pytest.mark.parametrize("case", ((40, 16, 8, 1024, 256, "attn8_kernel"), (40, 16, 8, 1156, 289, "attn8_kernel"), (40, 2, 8, 256, 64, "attn_kernel<40"),
                                  (40, 2, 8, 256, 16, "attn_kernel<40"), (80, 2, 8, 64, 16, "attn_kernel<80")), ids=lambda c: "-".join(map(str, c[:5])))
def test_self_attention_with_fewer_keys_than_queries(rec_cls, case):
    """``pv_attention`` with the queries of a ``qkv`` buffer and the keys / values of a pooled ``[K | V]`` buffer (the engine's layout) against fp32 SDPA on
    the same fp16 inputs, at the self-attention bound of ``tests/test_hip_kernels.py`` (rel-L2 < 2e-3).  d = 40 at B * H = 128: the 8-wave kernel, with
    whole key tiles (256) and a ragged last one (289 = 17 * 17); d = 40 at B * H = 16: the 4-wave kernel with one tile and with a quarter of one; d = 80.
    The key / value buffer ends with its last row: nothing lies behind it that a read past ``nk`` could mistake for data.
    Measured on MI355X (printed with -s): 3.528e-4, 3.535e-4 (attn8_kernel<497>), 3.275e-4, 3.033e-4 (attn_kernel<40, 2, true>), 3.024e-4
    (attn_kernel<80, 2, false>)."""
    d, batch, heads, nq, nk, kernel = case
    C = heads * d
    g = torch.Generator().manual_seed(nq + nk + d)
    qkv = torch.randn(batch * nq, 3 * C, generator=g).half()
    kv = torch.randn(batch * nk, 2 * C, generator=g).half()
    d_qkv, d_kv = qkv.cuda(), kv.cuda()
    rec = rec_cls("cuda")
    out = rec.attention(d_qkv[:, :C], d_kv[:, :C], d_kv[:, C:], batch=batch, heads=heads, nq=nq, nk=nk, d=d)
    assert rec.tags[0][0].startswith(kernel), rec.tags[0]
    rec.run()
    torch.cuda.synchronize()
    q = qkv[:, :C].float().view(batch, nq, heads, d).transpose(1, 2)
    k, v = (t.float().view(batch, nk, heads, d).transpose(1, 2) for t in (kv[:, :C], kv[:, C:]))
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * nq, C)
    err = rel_l2(out, ref)
    print(f"pv_attention d = {d}, B * H = {batch * heads}, nq = {nq}, nk = {nk} ({rec.tags[0][0]}): rel-L2 vs fp32 SDPA = {err:.3e}")
    assert torch.isfinite(out).all() and err < 2e-3
    assert torch.equal(d_qkv.cpu(), qkv) and torch.equal(d_kv.cpu(), kv)


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def tiny_pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    ref = tiny_oracle()
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    return ref, hip


@pytest.fixture(scope="module")
def loop_inputs():
    return loop_inputs_81()


def _names(eng):
    return [fn.__name__ for fn, _ in eng.rec.calls]


def _without_pool(names):
    return [nm for nm in names if nm != POOL]


@torch.no_grad()
def test_pooled_forward_matches_the_pooled_oracle(tiny_pair, loop_inputs):
    """``UNetEngine(kv_downsample=(f, method, names))`` at B = 2, t = 500 against the fp32 oracle with ``PooledAttnProcessorRef`` on the same layers: rel-L2
    below TOL_FWD (the bound the perturbed forward is held to) for both methods at f = 2 and 4 on the default layers, on all four transformers (the mid
    block: d = 80, 64 queries on 16 or 4 keys), at f = 3 (16 = 5 * 3 + 1: edge blocks one token wide) and on a 16 x 24 grid.  Each plan is the plain plan
    plus one ``pv_token_pool`` per named transformer, right behind its qkv launch; ``kv_downsample=None`` and an empty selection record the plain plan.
    Measured on MI355X (printed with -s), rel-L2 against the pooled / the plain oracle: default layers avg f = 2 1.218e-3 / 1.455e-2, f = 4 1.251e-3 /
    1.812e-2; nearest f = 2 1.240e-3 / 4.277e-2, f = 4 1.208e-3 / 1.122e-1; all layers avg f = 2 1.249e-3 / 1.495e-2, nearest f = 4 1.285e-3 / 1.201e-1,
    avg f = 3 1.290e-3 / 2.833e-2; 16 x 24 avg f = 2 1.236e-3 / 1.362e-2; 107 (default layers) and 108 (all) launches against the plain plan's 104."""
    ref, hip = tiny_pair
    cond, _, noise = loop_inputs
    t = torch.tensor([500.0])
    d_text, d_ip = cond[0].reshape(-1, 768).half().cuda().contiguous(), cond[1].reshape(-1, 768).half().cuda().contiguous()
    g = torch.Generator().manual_seed(82)
    wide = torch.randn(B, 4, 16, 24, generator=g)
    plain_names = {}
    for size, x in (((S, S), noise), ((16, 24), wide)):
        eng = hip.engine(B, *size, P, 1, latents_in=x.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=t.cuda())
        plain_names[size] = _names(eng)
        assert POOL not in plain_names[size] and eng.kv_downsample is None
    cases = [((S, S), f, m, TOP) for m in METHODS for f in (2, 4)] + [((S, S), 2, "avg", ALL), ((S, S), 4, "nearest", ALL), ((S, S), 3, "avg", ALL),
                                                                       ((16, 24), 2, "avg", TOP)]
    for size, f, method, names in cases:
        x = noise if size == (S, S) else wide
        eng = hip.engine(B, *size, P, 1, latents_in=x.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=t.cuda(), kv_downsample=(f, method, names))
        got_names = _names(eng)
        assert got_names.count(POOL) == len(names) and _without_pool(got_names) == plain_names[size]
        for i, nm in enumerate(got_names):
            if nm == POOL:
                assert got_names[i + 1] == "pv_attention" and got_names[i - 1] in ("pv_row_gemm", "pv_gemm_conv")
        got = eng.run().clone().float().cpu()
        torch.cuda.synchronize()
        exp = pooled_oracle(ref, names, f, method, size)(x, 500, encoder_hidden_states=cond).sample
        away = rel_l2(got, ref(x, 500, encoder_hidden_states=cond).sample)
        err = rel_l2(got, exp)
        print(f"pooled forward {size[0]} x {size[1]}, f = {f} {method} on {'the default layers' if names == TOP else 'all layers'}: rel-L2 vs the pooled "
              f"oracle = {err:.3e}, vs the plain oracle = {away:.3e}, launches {len(eng.rec)} (plain {len(plain_names[size])})")
        assert torch.isfinite(got).all() and err < TOL_FWD
        if names == TOP and size == (S, S):
            assert away > 4 * TOL_FWD          # the distance test_kv_downsample_cpu establishes on the oracle alone, for these four cases
        else:
            assert away > TOL_FWD
    common = dict(latents_in=noise.cuda().contiguous(), text=d_text, ip=d_ip, timesteps=t.cuda())
    for off in (None, (2, "avg", ())):
        assert _names(hip.engine(B, S, S, P, 1, kv_downsample=off, **common)) == plain_names[(S, S)]
    # a transformer that is also perturbed keeps its identity attention: nothing to pool there
    pert = hip.engine(B, S, S, P, 1, perturb=MID, kv_downsample=(2, "avg", ALL), **common)
    assert _names(pert).count(POOL) == 3 and _without_pool(_names(pert)) == _names(hip.engine(B, S, S, P, 1, perturb=MID, **common))
    with pytest.raises(ValueError, match="kv_downsample"):
        hip.engine(B, S, S, P, 1, kv_downsample=(2, "avg", ("mid_block.attentions.7",)), **common)
    with pytest.raises(ValueError, match="kv_downsample"):
        hip.engine(B, S, S, P, 1, kv_downsample=(9, "avg", TOP), **common)


# ---------------------------------------------------------------------------------------------------------------- the loop
def _run(loop, cond, uncond, noise, img=None):
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    if img is not None:
        loop.set_control(img.cuda())
    loop.reset(noise)
    out = loop.run().clone().cpu()
    assert loop.state[0].item() == STEPS
    return out


def _plan(loop):
    return [[fn.__name__ for fn, _ in e.rec.calls] for e in loop.all_engines], [fn.__name__ for fn, _ in loop.tail.calls], loop.launches_per_step


def _pools(loop):
    return [_names(e).count(POOL) for e in loop.all_engines]


@torch.no_grad()
def test_loop_matches_the_pooled_oracle_loop_and_the_default_loop_is_untouched(tiny_pair, loop_inputs):
    """4 steps at B = 2, 16 x 16, guidance 5 with ``kv_downsample=2`` (avg, default layers) against ``oracle_loop`` on the pooled oracle: rel-L2 below
    TOL_LOOP.  Eager launches == graph replay == the graph with side streams, bit for bit; ``share_prefix=True`` has the bits of the loop without it (the
    prefix plan holds the one pooled attn1 both forwards start from); ``nearest`` at f = 4 on all layers matches its own oracle loop.  ``launches_per_step``
    is the plain loop's plus one per selected transformer per plan that records its attn1.  ``kv_downsample=None`` builds the default loop - launch names
    per engine, tail, ``launches_per_step``, bits - before and after.  Measured on MI355X (printed with -s): rel-L2 against the pooled oracle loop
    9.396e-4, against the plain loop 7.087e-3; 216 launches per step against the plain loop's 210; f = 4 nearest on all layers 9.577e-4 against its
    oracle loop, 5.575e-2 from the f = 2 avg loop."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    before = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT)
    assert before.kv_downsample is None and sum(_pools(before)) == 0
    out_before = _run(before, cond, uncond, noise)
    exp = oracle_loop(pooled_oracle(ref, TOP, 2, "avg"), None, cond, uncond, noise, G_TEXT)
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, use_graph=use_graph, two_streams=two, kv_downsample=2)
        assert loop.kv_downsample == (2, "avg", TOP) and all(e.kv_downsample == (2, "avg", TOP) for e in loop.all_engines)
        assert loop.merge_lowres == before.merge_lowres and len(loop.all_engines) == len(before.all_engines) and _plan(loop)[1] == _plan(before)[1]
        assert _pools(loop) == [len(TOP)] * len(loop.all_engines)
        assert loop.launches_per_step == before.launches_per_step + sum(_pools(loop)) == sum(len(e.rec) for e in loop.all_engines) + len(loop.tail)
        assert [_without_pool(n) for n in _plan(loop)[0]] == _plan(before)[0]
        outs.append(_run(loop, cond, uncond, noise))
    err, away = rel_l2(outs[2], exp), rel_l2(outs[2], out_before)
    print(f"pooled loop f = 2 avg, guidance {G_TEXT}, {STEPS} steps: rel-L2 vs the pooled oracle loop = {err:.3e}, vs the plain loop = {away:.3e}; "
          f"launches per step {loop.launches_per_step} (plain {before.launches_per_step})")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert err < TOL_LOOP and away > TOL_LOOP
    shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_prefix=True, kv_downsample=2)
    assert shared.share_prefix and len(shared.engines_p) == 1
    assert [_names(e).count(POOL) for e in shared.engines_p + shared.engines_u + shared.engines_c] == [1, 2, 2]     # the prefix holds down_blocks.0's attn1
    plain_shared = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_prefix=True)
    assert shared.launches_per_step == plain_shared.launches_per_step + 5 and sum(_pools(plain_shared)) == 0
    assert torch.equal(_run(shared, cond, uncond, noise), outs[0])
    near = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, kv_downsample=4, kv_downsample_method="nearest", kv_downsample_layers="all")
    assert near.kv_downsample == (4, "nearest", ALL) and _pools(near) == [4] * len(near.all_engines)
    out_near = _run(near, cond, uncond, noise)
    err_near = rel_l2(out_near, oracle_loop(pooled_oracle(ref, ALL, 4, "nearest"), None, cond, uncond, noise, G_TEXT))
    print(f"pooled loop f = 4 nearest on all layers: rel-L2 vs its oracle loop = {err_near:.3e}, vs the f = 2 avg loop = {rel_l2(out_near, outs[0]):.3e}")
    assert err_near < TOL_LOOP and rel_l2(out_near, outs[0]) > TOL_LOOP
    for kw in (dict(), dict(kv_downsample=None), dict(kv_downsample=None, kv_downsample_method="nearest", kv_downsample_layers="all")):
        after = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw)
        assert after.kv_downsample is None and _plan(after) == _plan(before) and after.merge_lowres == before.merge_lowres
        assert torch.equal(_run(after, cond, uncond, noise), out_before)
    with pytest.raises(ValueError, match="kv_downsample.*training_mode"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, training_mode=True, kv_downsample=2)
    for bad in (1, 9, 2.0, "2", True):
        with pytest.raises(ValueError, match="kv_downsample"):
            DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, kv_downsample=bad)
    with pytest.raises(ValueError, match="kv_downsample_method"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, kv_downsample=2, kv_downsample_method="max")
    with pytest.raises(ValueError, match="kv_downsample_layers"):
        DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, kv_downsample=2, kv_downsample_layers=("down_blocks.1",))


@torch.no_grad()
def test_pag_on_a_shared_trunk_with_pooled_keys(tiny_pair, loop_inputs):
    """PAG 2 on the mid block with ``kv_downsample=2`` on all layers: the perturbed mid block keeps its identity attention, every other attn1 is pooled.
    The shared trunk has the bits of the whole perturbed forward, and the loop matches the oracle loop with both processors installed (rel-L2 below
    TOL_LOOP).  The trunk plan starts at the mid block: it records the two pooled transformers of the up path.
    Measured on MI355X (printed with -s): rel-L2 against the oracle loop 1.119e-3."""
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    cond, uncond, noise = loop_inputs
    kw = dict(pag_scale=G_PAG, pag_layers=("mid_block",), kv_downsample=2, kv_downsample_layers="all")
    trunk = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, **kw)
    full = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, share_trunk=False, **kw)
    assert trunk.share_trunk and not full.share_trunk
    assert [_names(e).count(POOL) for e in trunk.engines_u + trunk.engines_c + trunk.engines_p_attn] == [4, 4, 2]
    assert [_names(e).count(POOL) for e in full.engines_u + full.engines_c + full.engines_p_attn] == [4, 4, 3]
    plain = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, pag_scale=G_PAG, pag_layers=("mid_block",))
    assert trunk.launches_per_step == plain.launches_per_step + 10 and [_without_pool(n) for n in _plan(trunk)[0]] == _plan(plain)[0]
    out = _run(trunk, cond, uncond, noise)
    assert torch.equal(_run(full, cond, uncond, noise), out)
    pooled = pooled_oracle(ref, ALL, 2, "avg")
    exp = oracle_loop(pooled, perturbed_oracle(pooled, MID), cond, uncond, noise, G_TEXT, g_pag=G_PAG)
    err = rel_l2(out, exp)
    print(f"pooled PAG loop (mid block perturbed, f = 2 avg on all layers): rel-L2 vs the oracle loop = {err:.3e}")
    assert err < TOL_LOOP


@torch.no_grad()
def test_loop_under_a_controlnet_with_pooled_keys(loop_inputs):
    """With a ControlNet: both control plans pool their ``down_blocks.0.attentions.0`` (and ignore the decoder's names), the forwards pool the default
    layers, and the loop matches the oracle loop on the pooled UNet under the pooled ControlNet within TOL_LOOP.
    Measured on MI355X (printed with -s): rel-L2 against the oracle loop 8.725e-4, 5.927e-3 from the controlled loop without pooling."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    from test_controlnet_cpu import ControlledRef, control_image, tiny_controlnet_ref
    ref, cn_ref = tiny_oracle(), tiny_controlnet_ref()
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    cn = ControlNetModel(**TINY_CONFIG)
    cn.load_state_dict(cn_ref.state_dict(), strict=True)
    cn.to("cuda")
    cond, uncond, noise = loop_inputs
    img = control_image()
    plain = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn)
    loop = DenoiseLoop(hip, B, S, P, STEPS, G_TEXT, controlnet=cn, kv_downsample=2)
    assert [_names(e).count(POOL) for e in loop.engines_u + loop.engines_c + loop.engines_ctrl_u + loop.engines_ctrl_c] == [3, 3, 1, 1]
    assert loop.launches_per_step == plain.launches_per_step + 8 and [_without_pool(n) for n in _plan(loop)[0]] == _plan(plain)[0]
    out = _run(loop, cond, uncond, noise, img)
    exp = oracle_loop(ControlledRef(pooled_oracle(ref, TOP, 2, "avg"), pooled_oracle(cn_ref, TOP, 2, "avg"), img, 1.0), None, cond, uncond, noise, G_TEXT)
    err = rel_l2(out, exp)
    print(f"pooled loop under a ControlNet: rel-L2 vs the oracle loop = {err:.3e}, vs the controlled loop without pooling = "
          f"{rel_l2(out, _run(plain, cond, uncond, noise, img)):.3e}")
    assert torch.isfinite(out).all() and err < TOL_LOOP


# ---------------------------------------------------------------------------------------------------------------- run_inference and the CLI
@torch.no_grad()
def test_run_inference_kv_downsample_end_to_end():
    """``run_inference`` on the tiny models.  ``hires_kv_downsample=2`` alone: the first-pass loop has no ``pv_token_pool`` launch, the second-pass loop has
    them, the images are finite.  Two calls that differ only in one ``kv_downsample*`` keyword do not share a cached loop, equal calls do; a plain call
    before and after gives identical bits."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG
    from oracle.vae_ref import AutoencoderKLDecoderRef
    from photoverse_amd.infer import run_inference
    from photoverse_amd.modeling_utils import load_models
    from photoverse_amd.vae import AutoencoderKL
    from test_pag_gpu import VAE_TINY
    torch.manual_seed(5)
    hip_vae = AutoencoderKL(**VAE_TINY)
    hip_vae.load_state_dict(AutoencoderKLDecoderRef(**VAE_TINY, with_encoder=True).eval().state_dict())
    hip_vae.to("cuda")
    vis = dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, image_size=56, patch_size=14)
    txt = dict(vocab_size=49408, hidden_size=768, num_attention_heads=12, intermediate_size=512, num_hidden_layers=1)
    tok, te, vae, unet, ie, ia, ta, sch, _ = load_models(None, 1, unet_config=TINY_CONFIG, vision_config=vis, text_config=txt, seed=3)
    for m in (unet, te, ie, ia, ta):
        m.to("cuda")
    g = torch.Generator().manual_seed(4)
    ex = {"pixel_values": torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, "pixel_values_clip": torch.randn(2, 3, 56, 56, generator=g),
          "text_input_ids": torch.randint(0, 1000, (2, 77), generator=g), "concept_placeholder_idx": torch.tensor([[5], [3]])}
    kw = dict(latent_size=16, guidance_scale=3.0, timesteps=4, seed=1)
    args = (ex, tok, ie, te, unet, ta, ia)
    before = run_inference(*args, None, sch, "cuda", [1], **kw)
    cache = unet.__dict__["_denoise_loops"]
    plain_loop = next(reversed(cache.values()))
    # 1. an exact first pass and a pooled second one
    hi = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, hires_kv_downsample=2, **kw)
    assert hi.shape == (2, 3, 64, 64) and torch.isfinite(hi).all()
    by_size = {k[1]: l for k, l in cache.items()}
    assert set(by_size) == {16, 32} and by_size[16] is plain_loop
    assert sum(_pools(by_size[16])) == 0 and by_size[16].kv_downsample is None
    assert by_size[32].kv_downsample == (2, "avg", TOP) and all(n == len(TOP) for n in _pools(by_size[32]))
    hi_plain = run_inference(*args, hip_vae, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, **kw)
    assert not torch.equal(hi, hi_plain)
    # ... and the reverse: pooled first pass, hires_kv_downsample=1 switches the second one off
    run_inference(*args, None, sch, "cuda", [1], hires_latent_size=32, hires_strength=0.5, kv_downsample=2, hires_kv_downsample=1, **kw)
    by_size = {k[1]: l for k, l in cache.items()}
    assert by_size[16].kv_downsample == (2, "avg", TOP) and by_size[32].kv_downsample is None and sum(_pools(by_size[32])) == 0
    # 2. the keywords are part of the cache key
    a = run_inference(*args, None, sch, "cuda", [1], kv_downsample=2, **kw)
    loop_a = next(reversed(cache.values()))
    assert a.shape == (2, 4, 16, 16) and torch.isfinite(a).all() and not torch.equal(a, before) and loop_a.kv_downsample == (2, "avg", TOP)
    assert torch.equal(run_inference(*args, None, sch, "cuda", [1], kv_downsample=2, **kw), a) and next(reversed(cache.values())) is loop_a
    seen = [a]
    for other, setting in ((dict(kv_downsample=4), (4, "avg", TOP)), (dict(kv_downsample=2, kv_downsample_method="nearest"), (2, "nearest", TOP)),
                           (dict(kv_downsample=2, kv_downsample_layers="all"), (2, "avg", ALL))):
        o = run_inference(*args, None, sch, "cuda", [1], **other, **kw)
        lp = next(reversed(cache.values()))
        assert lp is not loop_a and lp.kv_downsample == setting and torch.isfinite(o).all() and not any(torch.equal(o, s) for s in seen)
        seen.append(o)
    with pytest.raises(ValueError, match="kv_downsample_layers"):
        run_inference(*args, None, sch, "cuda", [1], kv_downsample=2, kv_downsample_layers=("down_blocks.1",), **kw)
    # 3. a plain call afterwards: the plain loop's bits
    after = run_inference(*args, None, sch, "cuda", [1], **kw)
    assert torch.equal(after, before) and next(reversed(cache.values())).kv_downsample is None


def test_generate_cli_runs_with_the_kv_downsample_flags(tmp_path):
    """generate.py --hires_latent_size 32 --kv_downsample 2 --hires_kv_downsample 4 --kv_downsample_method nearest runs as a program and writes its PNGs."""
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--guidance_scale", "5", "--kv_downsample", "2", "--kv_downsample_method", "nearest", "--kv_downsample_layers", "down_blocks", "up_blocks",
           "--hires_latent_size", "32", "--hires_kv_downsample", "4", "--num_timesteps", "4", "--num_of_samples", "2", "--seed", "3",
           "--encoder_layers_idx", "1", "2", "--results_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["generated_image0.png", "generated_image1.png"]
    for f in files:
        a = np.asarray(Image.open(out / f))
        assert a.shape == (256, 256, 3) and a.dtype == np.uint8 and a.std() > 0
