"""CPU-only tests of perturbed-attention guidance (``pag_scale`` / ``pag_layers``): the new symbol in the header, ``_lib.SIGNATURES`` and the built
library, the C-ABI rejections of ``pv_cfg_dpm_step_pag``, the fp64 restatement of its formulas (``pag_step_ref``, the reference of
``tests/test_pag_gpu.py``), ``resolve_pag_layers``, the folded ``to_out . to_v`` weight, the keyword validation of ``run_inference`` / ``DenoiseLoop``,
the CLI flags, and - on the fp32 oracle alone - that the guidance moves the result by far more than the GPU loop test's tolerance."""
import copy
import math
import os
import re

import pytest
import torch

from test_guidance_cpu import SHAPES, _Untouchable, guided_eps_ref, make_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G_TEXT, G_IMAGE, G_PAG, RESCALE = 5.0, 2.0, 2.0, 0.7
#: the weights on (eu, em, ec, ep) are -1, -3, 7, -2: their magnitudes sum to 13, below the 14 of test_guidance_gpu, whose tolerances carry over
TOL_STEP, TOL_RESCALE, TOL_LOOP, TOL_FWD = 1e-5, 9.2e-6, 2.5e-3, 2.5e-3
B, S, P, STEPS = 2, 16, 1, 4


# ---------------------------------------------------------------------------------------------------------------- references
def pag_eps_ref(eu, em, ec, ep, g_text, g_image, g_pag, rescale):
    """The header's prediction of ``pv_cfg_dpm_step_pag`` in fp64 -> ``(f * e, f)``: ``e0`` = ``guided_eps_ref`` without rescale,
    ``e = e0 + g_pag (ec - ep)`` (``ep`` None: ``e0``), ``f = rescale std(ec) / std(e) + 1 - rescale`` on that ``e`` (population std; 1 where std(e) = 0)."""
    e, _ = guided_eps_ref(eu, em, ec, g_text, g_image, 0.0)
    if ep is not None:
        e = e + g_pag * (ec.double() - ep.double())
    n = e.shape[0]
    f = torch.ones(n, dtype=torch.float64)
    if rescale > 0:
        sc, se = ec.double().reshape(n, -1).std(dim=1, unbiased=False), e.reshape(n, -1).std(dim=1, unbiased=False)
        f = torch.where(se > 0, rescale * sc / se.clamp_min(1e-300) + (1 - rescale), f)
    return f.view(n, *([1] * (e.dim() - 1))) * e, f


def pag_step_ref(eu, em, ec, ep, x, x0_prev, row, g_text, g_image=None, g_pag=0.0, rescale=0.0, z=None, mask=None, known=None, noise=None):
    """``pv_cfg_dpm_step_pag`` in fp64 -> ``(latents', x0, f)``; ``row`` = {ca, cb, cx, c0, c1, q0, q1, cn}; ``z``: the launch's normals (the SDE
    form, ``rng`` given) or None."""
    ca, cb, cx, c0, c1, q0, q1, cn = row.double()[:8]
    e, f = pag_eps_ref(eu, em, ec, ep, g_text, g_image, g_pag, rescale)
    x0 = ca * x.double() + cb * e
    xn = cx * x.double() + c0 * x0 + c1 * x0_prev.double()
    if z is not None:
        xn = xn + cn * z.double()
    if mask is not None:
        m = mask.double()
        xn = m * xn + (1 - m) * (q0 * known.double() + q1 * noise.double())
    return xn, x0, f


def make_eps4(shape, g):
    """``make_eps``'s three predictions and a fourth, ``ep``, of the same kind (mean -+3, its own spread of standard deviations)."""
    eu, em, ec = make_eps(shape, g)
    n = shape[0]
    sign = torch.tensor([1.0 if b % 2 else -1.0 for b in range(n)])
    sd = torch.tensor([0.1 + 1.9 * (((b * 5 + 1) % 7) / 6.0) for b in range(n)])
    ep = (torch.randn(shape, generator=g) * sd.view(n, 1, 1, 1) + 3.0 * sign.view(n, 1, 1, 1)).contiguous()
    return eu, em, ec, ep


class IdentityAttnProcessorRef:
    """Self-attention with the identity attention map: every query returns its own value row."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kw):
        return attn.to_out[1](attn.to_out[0](attn.to_v(hidden_states)))


def perturbed_oracle(ref, names):
    """A deep copy of the fp32 oracle UNet whose transformers ``names`` (as ``resolve_pag_layers`` returns them) have the identity processor on attn1."""
    pert = copy.deepcopy(ref)
    procs = dict(pert.attn_processors)
    for nm in names:
        key = f"{nm}.transformer_blocks.0.attn1.processor"
        assert key in procs, key
        procs[key] = IdentityAttnProcessorRef()
    pert.set_attn_processor(procs)
    return pert


def tiny_oracle():
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    torch.manual_seed(0)
    ref = UNet2DConditionModelRef(**TINY_CONFIG).eval()
    set_visual_cross_attention_adapter_ref(ref, (5,))
    return ref


def loop_inputs_81():
    g = torch.Generator().manual_seed(81)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)
    return cond, uncond, noise


@torch.no_grad()
def oracle_loop(ref, pert, cond, uncond, noise, g_text, g_image=None, g_pag=0.0, rescale=0.0, steps=STEPS):
    """The denoising loop on the fp32 oracle: UNet x2 (+1 with ``g_image``, +1 on ``pert`` with ``g_pag``) per step, the header's formulas in torch,
    DPMSolverMultistepRef."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    sch = DPMSolverMultistepRef()
    sch.set_timesteps(steps)
    x = noise * sch.init_noise_sigma
    for t in sch.timesteps:
        eu = ref(x, t, encoder_hidden_states=uncond).sample
        ec = ref(x, t, encoder_hidden_states=cond).sample
        if g_image is None:
            e = eu + g_text * (ec - eu)
        else:
            em = ref(x, t, encoder_hidden_states=(uncond[0], cond[1])).sample
            e = eu + g_image * (em - eu) + g_text * (ec - em)
        if g_pag:
            e = e + g_pag * (ec - pert(x, t, encoder_hidden_states=cond).sample)
        if rescale > 0:
            f = rescale * ec.flatten(1).std(dim=1) / e.flatten(1).std(dim=1) + (1 - rescale)
            e = f.view(-1, 1, 1, 1) * e
        x = sch.step(e, t, x)
    return x


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    """``pv_cfg_dpm_step_pag``: the stochastic launcher's arguments plus ``eps_perturbed`` behind ``eps_cond`` and ``g_pag`` behind ``g_image`` - twenty
    parameters, with the return type the 21 types of the signature."""
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    assert re.search(r"^int\s+pv_cfg_dpm_step_pag\s*\(", header, flags=re.M)
    decl = re.search(r"^int\s+pv_cfg_dpm_step_pag\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.SIGNATURES["pv_cfg_dpm_step_pag"]
    sto = _lib.SIGNATURES["pv_cfg_dpm_step_stochastic"][1]
    assert res is _lib.c_int and args == sto[:3] + [_lib.c_void_p] + sto[3:10] + [_lib.c_float] + sto[10:]
    assert len(decl.split(",")) == len(args) == 20 and len([res] + args) == 21
    assert args[9:13] == [_lib.c_float] * 4 and args[16:19] == [_lib.c_int] * 3
    assert lib.pv_cfg_dpm_step_pag is not None
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))


def test_cabi_rejects_bad_pag_step_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed), with and without ``rng``.  No valid call
    is sent: ``eps_image`` / ``eps_perturbed`` / ``rng`` NULL and an absent mask triple are legal, so they only appear together with something illegal."""
    INVALID = 1
    EU, EM, EC, EP, LAT, X0P, COEF, STATE, RNG, MASK, KNOWN, NOISE = (0x10000 * (i + 1) for i in range(12))     # never dereferenced

    def call(eu=EU, em=EM, ec=EC, ep=EP, lat=LAT, x0p=X0P, coef=COEF, state=STATE, rng=RNG, g_text=5.0, g_image=2.0, g_pag=2.0, rescale=0.7,
             mask=MASK, known=KNOWN, noise=NOISE, batch=2, channels=4, hw=256):
        return lib.pv_cfg_dpm_step_pag(eu, em, ec, ep, lat, x0p, coef, state, rng, g_text, g_image, g_pag, rescale, mask, known, noise, batch,
                                       channels, hw, None)

    for rng in (RNG, None):
        for name in ("eu", "ec", "lat", "x0p", "coef", "state"):
            assert call(**{name: None}, rng=rng) == INVALID, name
            assert call(**{name: None}, rng=rng, em=None, ep=None, mask=None, known=None, noise=None, rescale=0.0) == INVALID, name
        for name in ("batch", "channels", "hw"):
            for v in (0, -1, -16):
                assert call(**{name: v}, rng=rng) == INVALID, (name, v)
        for hw in (1, 2, 3, 6, 255, 258):
            assert call(hw=hw, rng=rng) == INVALID, hw
        for part in (dict(mask=None), dict(known=None), dict(noise=None), dict(mask=None, known=None), dict(mask=None, noise=None),
                     dict(known=None, noise=None)):
            assert call(**part, rng=rng) == INVALID, part
        for r in (-0.1, -1e-6, 1.0001, 2.0, math.nan, math.inf, -math.inf):
            assert call(rescale=r, rng=rng) == INVALID, r
        for bad in (math.nan, math.inf, -math.inf):
            assert call(g_text=bad, rng=rng) == INVALID and call(g_image=bad, rng=rng) == INVALID and call(g_pag=bad, rng=rng) == INVALID, bad
            assert call(g_pag=bad, rng=rng, ep=None) == INVALID and call(g_pag=bad, rng=rng, em=None) == INVALID, bad      # also where ep is not read
        assert call(batch=2, channels=4, hw=1 << 28, rng=rng) == INVALID                   # exactly 2^31
        assert call(batch=1, channels=1 << 16, hw=1 << 15, rng=rng) == INVALID             # chw alone is 2^31
        m = (1 << 31) - 1
        assert call(batch=1, channels=m, hw=m - 3, rng=rng) == INVALID
        assert call(batch=m, channels=m, hw=m - 3, rng=rng) == INVALID
        assert call(batch=m, channels=1, hw=4, rng=rng) == INVALID
        assert call(batch=1 << 16, channels=1 << 16, hw=1 << 16, rng=rng) == INVALID       # 2^48


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_fp64_reference_against_a_per_element_evaluation(shape):
    """``pag_step_ref`` against the formulas written out element by element in plain Python floats (fp64): the four-term prediction, the two-pass
    population statistics of the rescale on the perturbed ``e``, the solver row, ``cn z`` and the blend.  ``ep`` None / ``g_pag`` 0 is the guided step."""
    from test_guidance_cpu import guided_step_ref
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(sum(shape) + 1)
    eu, em, ec, ep = make_eps4(shape, g)
    x, xp, known, noise, z = (torch.randn(shape, generator=g) for _ in range(5))
    n, C, H, W = shape
    mask = (torch.rand((n, 1, H, W), generator=g) * 1.4 - 0.2).clamp(0, 1)
    sch = DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    sch.set_timesteps(6)
    row = sch.coefficient_table(0, blend=True)[3]
    ca, cb, cx, c0, c1, q0, q1, cn = (float(v) for v in row.double())
    assert cn != 0 and c1 != 0
    got, got_x0, f = pag_step_ref(eu, em, ec, ep, x, xp, row, G_TEXT, G_IMAGE, G_PAG, RESCALE, z=z, mask=mask, known=known, noise=noise)
    chw = C * H * W
    for b in range(n):
        U, M, Cc, Pp = (t[b].reshape(-1).tolist() for t in (eu, em, ec, ep))
        e = [U[i] + G_IMAGE * (M[i] - U[i]) + G_TEXT * (Cc[i] - M[i]) + G_PAG * (Cc[i] - Pp[i]) for i in range(chw)]
        mc, me = math.fsum(Cc) / chw, math.fsum(e) / chw
        sc = math.sqrt(math.fsum((v - mc) ** 2 for v in Cc) / chw)
        se = math.sqrt(math.fsum((v - me) ** 2 for v in e) / chw)
        fb = RESCALE * sc / se + (1 - RESCALE)
        assert abs(f[b].item() - fb) <= 1e-12 * fb
        X, XP, K, N, Z = (t[b].reshape(-1).tolist() for t in (x, xp, known, noise, z))
        Mk = mask[b].expand(C, H, W).reshape(-1).tolist()
        for i in range(0, chw, max(1, chw // 97)):
            x0 = ca * X[i] + cb * fb * e[i]
            xn = cx * X[i] + c0 * x0 + c1 * XP[i] + cn * Z[i]
            xn = Mk[i] * xn + (1 - Mk[i]) * (q0 * K[i] + q1 * N[i])
            assert abs(got_x0[b].reshape(-1)[i].item() - x0) <= 1e-11 * (1 + abs(x0))
            assert abs(got[b].reshape(-1)[i].item() - xn) <= 1e-11 * (1 + abs(xn))
    # the weights on (eu, em, ec, ep): -1, -3, 7, -2
    one = torch.ones(shape)
    for k, wgt in enumerate((1 - G_IMAGE, G_IMAGE - G_TEXT, G_TEXT + G_PAG, -G_PAG)):
        e, _ = pag_eps_ref(*(one if j == k else 0 * one for j in range(4)), G_TEXT, G_IMAGE, G_PAG, 0.0)
        assert torch.equal(e, wgt * one.double()) and wgt == (-1, -3, 7, -2)[k]
    for kw in (dict(ep=None, g_pag=G_PAG), dict(ep=ep, g_pag=0.0)):
        a = pag_step_ref(eu, em, ec, kw["ep"], x, xp, row, G_TEXT, G_IMAGE, kw["g_pag"], RESCALE, mask=mask, known=known, noise=noise)
        b_ = guided_step_ref(eu, em, ec, x, xp, row, G_TEXT, G_IMAGE, RESCALE, mask, known, noise)
        assert all(torch.equal(p, q) for p, q in zip(a, b_))


def test_resolve_pag_layers():
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.unet import UNet2DConditionModel, resolve_pag_layers, transformer_names
    tiny = UNet2DConditionModel(**TINY_CONFIG)
    assert transformer_names(tiny) == ("down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")
    assert resolve_pag_layers(tiny) == resolve_pag_layers(tiny, ("mid_block",)) == ("mid_block.attentions.0",)
    assert resolve_pag_layers(tiny, ("up_blocks",)) == ("up_blocks.1.attentions.0", "up_blocks.1.attentions.1")
    assert resolve_pag_layers(tiny, "all") == resolve_pag_layers(tiny, ("all",)) == transformer_names(tiny) and len(transformer_names(tiny)) == 4
    assert resolve_pag_layers(tiny, ["up_blocks.1.attentions.1", "mid_block", "mid_block.attentions.0"]) == ("mid_block.attentions.0",
                                                                                                            "up_blocks.1.attentions.1")
    for bad in (("mid_blocks",), ("mid_block", "down_blocks.1"), ("up_blocks.0",), (), ("",), (3,), 3, ("mid_block.attentions.1",)):
        with pytest.raises(ValueError, match="pag_layers"):
            resolve_pag_layers(tiny, bad)
    with torch.device("meta"):
        sd15 = UNet2DConditionModel()
    assert resolve_pag_layers(sd15) == ("mid_block.attentions.0",)
    assert len(resolve_pag_layers(sd15, "all")) == 16 and len(resolve_pag_layers(sd15, ("down_blocks.1", "up_blocks.3"))) == 5
    # the names are the ones the engine's plan uses: the execution order of UNetEngine._build
    assert transformer_names(sd15)[:2] == ("down_blocks.0.attentions.0", "down_blocks.0.attentions.1") and transformer_names(sd15)[6] == "mid_block.attentions.0"


def test_folded_weight_against_the_two_step_product():
    """``fold_identity_attention``: W = to_out.weight @ to_v.weight in fp32, rounded to fp16 once.  Against the two Linears applied one after the other in
    fp32 on the fp16-rounded weights and an fp16-rounded input (what two separate launches would see, without their intermediate rounding), the folded
    Linear's rel-L2 is below 1e-3 on every transformer of the tiny UNet (fp16 has 11 bits: 2^-11 = 4.9e-4 per rounded operand, averaged down by
    the K-long sums).  Measured on the CPU (printed with -s): 3.7e-4 (mid block, C = 640), 3.4e-4 (the three C = 320 transformers)."""
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.unet import UNet2DConditionModel, fold_identity_attention, transformer_names
    torch.manual_seed(0)
    tiny = UNet2DConditionModel(**TINY_CONFIG)
    g = torch.Generator().manual_seed(2)
    for nm in transformer_names(tiny):
        a1 = tiny.get_submodule(nm).transformer_blocks[0].attn1
        w, bias = fold_identity_attention(a1)
        C = a1.to_v.weight.shape[1]
        assert w.dtype == torch.float16 and w.shape == (C, C) and bias.dtype == torch.float32 and torch.equal(bias, a1.to_out[0].bias.detach())
        assert torch.equal(w, (a1.to_out[0].weight.detach().float() @ a1.to_v.weight.detach().float()).half())
        xin = torch.randn(64, C, generator=g).half().float()
        two = (xin @ a1.to_v.weight.detach().half().float().T) @ a1.to_out[0].weight.detach().half().float().T + bias
        one = xin @ w.float().T + bias
        err = rel_l2(one - bias, two - bias)
        print(f"folded to_out . to_v of {nm} (C = {C}): rel-L2 against the two-step product = {err:.3e}")
        assert err < 1e-3


def test_keywords_are_validated_before_a_model_runs():
    import inspect
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.infer import run_inference
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.unet import UNet2DConditionModel
    sig = inspect.signature(run_inference).parameters
    for name, default in (("pag_scale", None), ("pag_layers", ("mid_block",))):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    lsig = inspect.signature(DenoiseLoop.__init__).parameters
    assert lsig["pag_scale"].default is None and lsig["pag_layers"].default == ("mid_block",) and lsig["share_trunk"].default is None
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=5.0, timesteps=4)
    for bad in (math.nan, math.inf, -math.inf, "2", True, [2.0], 1 + 2j):
        with pytest.raises(ValueError, match="pag_scale"):
            run_inference(*args, pag_scale=bad, **kw)
    with pytest.raises(ValueError, match="pag_scale.*training_mode"):
        run_inference(*args, pag_scale=2.0, training_mode=True, **kw)
    # off (None, 0): nothing about the layers is looked at; the next thing is the first touch of a model argument
    for good in (dict(), dict(pag_scale=None), dict(pag_scale=0), dict(pag_scale=0.0, pag_layers=("nothing",))):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)
    # the layers resolve against the UNet's module tree alone - every other model is still untouched when an unknown entry is refused
    tiny = UNet2DConditionModel(**TINY_CONFIG)
    margs = (u, u, u, u, tiny, u, u, u, u, "cpu", [1])
    for bad in (("nothing",), ("mid_block", "up_blocks.0"), (), 7):
        with pytest.raises(ValueError, match="pag_layers"):
            run_inference(*margs, pag_scale=2.0, pag_layers=bad, **kw)
    with pytest.raises(AssertionError, match="touched a model argument"):          # legal: got past the validation
        run_inference(*margs, pag_scale=2.0, pag_layers=("up_blocks",), **kw)
    # DenoiseLoop: the UNet must be on a HIP device first (no CPU path), so its own keyword checks are reached in test_pag_gpu; the ones that need no
    # device are the same functions


def test_cli_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_pag", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.pag_scale is None and d.pag_layers == ["mid_block"]
    a = gen.parser.parse_args(["--pag_scale", "2", "--pag_layers", "mid_block", "up_blocks"])
    assert a.pag_scale == 2.0 and a.pag_layers == ["mid_block", "up_blocks"]
    assert "--pag_scale" in open(os.path.join(ROOT, "README.md")).read()


@torch.no_grad()
def test_pag_moves_the_oracle_loop_by_far_more_than_the_loop_tolerance():
    """The precondition of the GPU loop test, on the fp32 oracle alone: tiny model under ``torch.manual_seed(0)``, inputs from generator seed 81, 4 steps
    at B = 2, 16 x 16, guidance 5.  PAG 2 on the mid block moves the final latents by rel-L2 2.83e-2 against no PAG, on all layers by 1.58e-1 (measured on
    the CPU, printed with -s): both above 10 x TOL_LOOP, so a loop that ignored ``pag_scale`` or the layers could not pass the GPU test."""
    ref = tiny_oracle()
    cond, uncond, noise = loop_inputs_81()
    plain = oracle_loop(ref, None, cond, uncond, noise, G_TEXT)
    names = ("down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")
    for layers in (names[1:2], names):
        moved = oracle_loop(ref, perturbed_oracle(ref, layers), cond, uncond, noise, G_TEXT, g_pag=G_PAG)
        d = rel_l2(moved, plain)
        print(f"oracle loop, guidance {G_TEXT}, PAG {G_PAG} on {len(layers)} layer(s): rel-L2 against no PAG = {d:.3e}")
        assert torch.isfinite(moved).all() and d > 10 * TOL_LOOP
