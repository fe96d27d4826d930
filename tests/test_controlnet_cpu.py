"""CPU-only tests of ControlNet conditioning: the fp32 reference model (``ControlNetRef``, assembled from ``oracle.unet_ref``'s blocks and plain
``nn.Conv2d``s) and the controlled UNet forward built on it (``controlled_oracle`` - the references of ``tests/test_controlnet_gpu.py``); that
zero-initialised zero convs leave the UNet's result untouched and a seeded non-zero init moves the oracle loop by far more than the GPU loop test's
tolerance; the state-dict names of ``ControlNetModel``; ``from_unet``; the new symbol ``pv_hint_conv3x3`` in the header, the binding and the built
library, and its C-ABI rejections; the keyword validation of ``run_inference`` / ``DenoiseLoop``; the CLI flags."""
import inspect
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from photoverse_amd import controlnet as pv_controlnet          # (module level: on a tree without the feature every test of this file fails at import)
from test_guidance_cpu import _Untouchable
from test_pag_cpu import B, G_TEXT, S, STEPS, TOL_LOOP, loop_inputs_81, oracle_loop, rel_l2, tiny_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: (cin, cout, stride) of ``controlnet_cond_embedding.blocks``, as the issue spells them
HINT_BLOCKS = ((16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2))
#: std of the seeded non-zero init of ``controlnet_cond_embedding.conv_out`` and of the zero convs (``nonzero_init_``).  Chosen on the CPU: with 0.05 the
#: control moves the 4-step oracle loop by rel-L2 3.4e-1 at scale 1 (test_control_moves_the_oracle_loop...), more than 100 x TOL_LOOP, while every
#: activation stays of order 1 (a 1 x 1 conv over 320 .. 640 channels at std 0.05 has gain ~ 1).
INIT_STD = 0.05
INIT_SEED = 11
#: ... and the gain of the seeded re-init of the embedding's seven SiLU convs, weights ~ N(0, (gain / sqrt(9 cin))^2): at their default init the image's
#: share of the hint is 7e-5 against conv_in(sample)'s 0.56 (two control images then give loops 3.4e-5 apart - nothing a test could see); at 1.75 the
#: hint is of the order of conv_in(sample) and follows the image.
EMB_GAIN = 1.75


# ---------------------------------------------------------------------------------------------------------------- references
class _CondEmbeddingRef(nn.Module):
    def __init__(self, c0):
        super().__init__()
        self.conv_in = nn.Conv2d(3, 16, 3, padding=1)
        self.blocks = nn.ModuleList([nn.Conv2d(ci, co, 3, padding=1, stride=s) for ci, co, s in HINT_BLOCKS])
        self.conv_out = nn.Conv2d(256, c0, 3, padding=1)
        nn.init.zeros_(self.conv_out.weight)
        nn.init.zeros_(self.conv_out.bias)

    def forward(self, image):
        h = F.silu(self.conv_in(image))
        for m in self.blocks:
            h = F.silu(m(h))
        return self.conv_out(h)


def _zero_conv(ch):
    m = nn.Conv2d(ch, ch, 1)
    nn.init.zeros_(m.weight)
    nn.init.zeros_(m.bias)
    return m


class ControlNetRef(nn.Module):
    """[EXT] diffusers' ``ControlNetModel`` for SD-1.5-shaped configurations in fp32 torch: the UNet oracle's encoder blocks, stock (text-only)
    cross-attention, the conditioning embedding and the zero convs.  ``forward`` -> (down residuals, mid residual), each times ``conditioning_scale``."""

    def __init__(self, **overrides):
        super().__init__()
        from oracle.unet_ref import SD15_CONFIG, _DownBlock, _MidBlock, _TimestepEmbedding
        cfg = dict(SD15_CONFIG)
        cfg.update(overrides)
        self.config = SimpleNamespace(**cfg)
        boc = tuple(cfg["block_out_channels"])
        heads, xdim, groups, layers = cfg["attention_head_dim"], cfg["cross_attention_dim"], cfg["norm_num_groups"], cfg["layers_per_block"]
        temb = boc[0] * 4
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        self.time_embedding = _TimestepEmbedding(boc[0], temb)
        self.controlnet_cond_embedding = _CondEmbeddingRef(boc[0])
        self.down_blocks = nn.ModuleList()
        widths, cout = [boc[0]], boc[0]
        for i, kind in enumerate(cfg["down_block_types"]):
            cin, cout = cout, boc[i]
            last = i == len(boc) - 1
            self.down_blocks.append(_DownBlock(cin, cout, temb, layers, heads, xdim, groups, kind.startswith("CrossAttn"), not last))
            widths += [cout] * (layers + (0 if last else 1))
        self.mid_block = _MidBlock(boc[-1], temb, heads, xdim, groups)
        self.controlnet_down_blocks = nn.ModuleList([_zero_conv(c) for c in widths])
        self.controlnet_mid_block = _zero_conv(boc[-1])

    def features(self, sample, timestep, text, image):
        """(the pushed skips in push order, the mid block's output): the control features, before the zero convs."""
        from oracle.unet_ref import timestep_embedding_ref
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep])
        t = t.reshape(-1).expand(sample.shape[0])
        emb = self.time_embedding(timestep_embedding_ref(t, self.config.block_out_channels[0]).to(sample.dtype))
        x = self.conv_in(sample) + self.controlnet_cond_embedding(image)
        skips = (x,)
        for blk in self.down_blocks:
            x, outs = blk(x, emb, text)
            skips += outs
        return skips, self.mid_block(x, emb, text)

    def forward(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0):
        skips, mid = self.features(sample, timestep, encoder_hidden_states, controlnet_cond)
        return [conditioning_scale * z(s) for z, s in zip(self.controlnet_down_blocks, skips)], conditioning_scale * self.controlnet_mid_block(mid)


def nonzero_init_(cn, seed=INIT_SEED, std=INIT_STD):
    """Seeded N(0, std^2) weights for the conditioning embedding's ``conv_out`` and every zero conv (biases stay 0), and N(0, (EMB_GAIN / sqrt(9 cin))^2)
    weights for the embedding's other convs: a ControlNet with an effect that depends on its control image."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        emb = cn.controlnet_cond_embedding
        for m in [emb.conv_in, *emb.blocks]:
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * EMB_GAIN / (9 * m.weight.shape[1]) ** 0.5)
        for m in [cn.controlnet_cond_embedding.conv_out, *cn.controlnet_down_blocks, cn.controlnet_mid_block]:
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * std)
    return cn


def tiny_controlnet_ref(nonzero=True):
    """The tiny ControlNet oracle with the tiny UNet oracle's encoder weights (what ``from_unet`` gives), zero convs seeded non-zero unless asked."""
    from oracle.unet_ref import TINY_CONFIG
    ref = tiny_oracle()
    torch.manual_seed(1)
    cn = ControlNetRef(**TINY_CONFIG).eval()
    own = cn.state_dict()
    cn.load_state_dict({k: v for k, v in ref.state_dict().items() if k in own and "processor" not in k}, strict=False)
    return nonzero_init_(cn) if nonzero else cn


def control_image(batch=B, size=8 * S, seed=5):
    """A control image in [0, 1] with structure: random rectangles on a smooth ramp, one image per sample."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, size), torch.linspace(0, 1, size), indexing="ij")
    img = (0.25 * (yy + xx))[None, None].repeat(batch, 3, 1, 1)
    for b in range(batch):
        for _ in range(6):
            y0, x0 = (int(v) for v in torch.randint(0, size - 8, (2,), generator=g))
            hh, ww = (int(v) for v in torch.randint(4, size // 2, (2,), generator=g))
            img[b, :, y0:y0 + hh, x0:x0 + ww] = torch.rand(3, 1, 1, generator=g)
    return img.clamp(0, 1).contiguous()


@torch.no_grad()
def controlled_oracle(ref_unet, cn_ref, sample, timestep, encoder_hidden_states, image, scale=1.0):
    """The UNet oracle's forward under a ControlNet, diffusers semantics: the ControlNet sees (sample, t, text, image); its residuals are added to
    the stored skips AFTER the down path (which continues on the raw activations) and to the mid block's output."""
    from oracle.unet_ref import timestep_embedding_ref
    ehs = encoder_hidden_states
    t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep])
    t = t.reshape(-1).expand(sample.shape[0])
    emb = ref_unet.time_embedding(timestep_embedding_ref(t, ref_unet.config.block_out_channels[0]).to(sample.dtype))
    x = ref_unet.conv_in(sample)
    skips = (x,)
    for blk in ref_unet.down_blocks:
        x, outs = blk(x, emb, ehs)
        skips += outs
    x = ref_unet.mid_block(x, emb, ehs)
    down_res, mid_res = cn_ref(sample, timestep, encoder_hidden_states=ehs[0], controlnet_cond=image, conditioning_scale=scale)
    assert len(down_res) == len(skips)
    skips = tuple(s + r for s, r in zip(skips, down_res))
    x = x + mid_res
    for blk in ref_unet.up_blocks:
        n = len(blk.resnets)
        x = blk(x, skips[-n:], emb, ehs)
        skips = skips[:-n]
    return SimpleNamespace(sample=ref_unet.conv_out(ref_unet.conv_act(ref_unet.conv_norm_out(x))))


class ControlledRef:
    """``controlled_oracle`` with the call signature of the UNet oracle (what ``oracle_loop`` calls): works on any model with the oracle's attributes
    (the plain one, ``perturbed_oracle(...)``, ``freeu_oracle(...)``)."""

    def __init__(self, ref_unet, cn_ref, image, scale=1.0):
        self.ref, self.cn, self.image, self.scale = ref_unet, cn_ref, image, scale

    def __call__(self, sample, timestep, encoder_hidden_states=None):
        return controlled_oracle(self.ref, self.cn, sample, timestep, encoder_hidden_states, self.image, self.scale)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


@torch.no_grad()
def test_zero_initialised_zero_convs_leave_the_forward_untouched():
    """With the zero convs at their zero init every residual is exactly 0, so the controlled oracle forward IS the plain one, bit for bit - whatever the
    control image and the scale.  ``conv_out`` of the conditioning embedding is zero too: the hint is exactly 0."""
    ref, cn = tiny_oracle(), tiny_controlnet_ref(nonzero=False)
    cond, _, noise = loop_inputs_81()
    img = control_image()
    assert torch.equal(cn.controlnet_cond_embedding(img), torch.zeros(B, 320, S, S))
    plain = ref(noise, 500, encoder_hidden_states=cond).sample
    for scale in (1.0, 0.5, 7.0):
        assert torch.equal(controlled_oracle(ref, cn, noise, 500, cond, img, scale).sample, plain)
    down, mid = cn(noise, 500, encoder_hidden_states=cond[0], controlnet_cond=img)
    assert [tuple(d.shape) for d in down] == [(B, 320, S, S), (B, 320, S, S), (B, 320, S // 2, S // 2), (B, 640, S // 2, S // 2)]
    assert tuple(mid.shape) == (B, 640, S // 2, S // 2) and all(not d.any() for d in down) and not mid.any()


@torch.no_grad()
def test_control_moves_the_oracle_loop_by_far_more_than_the_loop_tolerance():
    """The precondition of the GPU comparisons, on the fp32 oracle alone: tiny models, ``nonzero_init_`` at INIT_STD = 0.05 / seed 11, inputs from generator
    seed 81, 4 steps at B = 2, 16 x 16, guidance 5.  Control at scale 1 moves the final latents by more than 10 x TOL_LOOP against no control, scale 0.5
    and a second control image each by more than 10 x TOL_LOOP against scale 1 / the first image, so a loop that ignored the ControlNet, its scale or
    ``set_control`` could not pass.  Measured on the CPU (printed with -s): 3.445e-1, 1.706e-1 and 1.383e-1."""
    ref, cn = tiny_oracle(), tiny_controlnet_ref()
    cond, uncond, noise = loop_inputs_81()
    img, img2 = control_image(), control_image(seed=6)
    plain = oracle_loop(ref, None, cond, uncond, noise, G_TEXT)
    one = oracle_loop(ControlledRef(ref, cn, img, 1.0), None, cond, uncond, noise, G_TEXT)
    half = oracle_loop(ControlledRef(ref, cn, img, 0.5), None, cond, uncond, noise, G_TEXT)
    other = oracle_loop(ControlledRef(ref, cn, img2, 1.0), None, cond, uncond, noise, G_TEXT)
    d1, d2, d3 = rel_l2(one, plain), rel_l2(half, one), rel_l2(other, one)
    print(f"oracle loop, guidance {G_TEXT}: control at scale 1 vs none rel-L2 = {d1:.3e}; scale 0.5 vs 1 = {d2:.3e}; second image vs first = {d3:.3e}")
    assert all(torch.isfinite(t).all() for t in (one, half, other))
    assert d1 > 10 * TOL_LOOP and d2 > 10 * TOL_LOOP and d3 > 10 * TOL_LOOP


def test_state_dict_names_and_shapes():
    """diffusers' ``ControlNetModel`` layout: the UNet's encoder names, ``controlnet_cond_embedding.{conv_in, blocks.0-5, conv_out}``, one
    ``controlnet_down_blocks.k`` per pushed skip (tiny: 320, 320, 320, 640; SD-1.5: 320 x 4, 640 x 3, 1280 x 5) and ``controlnet_mid_block``; the HIP model
    and the oracle agree name for name and shape for shape; the zero convs and the embedding's ``conv_out`` are zero-initialised."""
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.unet import UNet2DConditionModel
    assert pv_controlnet.HINT_BLOCKS == HINT_BLOCKS
    tiny = ControlNetModel(**TINY_CONFIG)
    sd = tiny.state_dict()
    ref_sd = ControlNetRef(**TINY_CONFIG).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref_sd.items()}
    emb = [("conv_in", 3, 16)] + [(f"blocks.{i}", ci, co) for i, (ci, co, _) in enumerate(HINT_BLOCKS)] + [("conv_out", 256, 320)]
    for name, ci, co in emb:
        assert tuple(sd[f"controlnet_cond_embedding.{name}.weight"].shape) == (co, ci, 3, 3) and tuple(sd[f"controlnet_cond_embedding.{name}.bias"].shape) == (co,)
    assert [m.stride[0] for m in tiny.controlnet_cond_embedding.blocks] == [s for _, _, s in HINT_BLOCKS]
    assert [tuple(sd[f"controlnet_down_blocks.{k}.weight"].shape) for k in range(4)] == [(320, 320, 1, 1)] * 3 + [(640, 640, 1, 1)]
    assert "controlnet_down_blocks.4.weight" not in sd and tuple(sd["controlnet_mid_block.weight"].shape) == (640, 640, 1, 1)
    for k, v in sd.items():
        if k.startswith(("controlnet_down_blocks", "controlnet_mid_block", "controlnet_cond_embedding.conv_out")):
            assert not v.any(), k
    assert sd["controlnet_cond_embedding.conv_in.weight"].any()
    unet_sd = UNet2DConditionModel(**TINY_CONFIG).state_dict()
    enc = {k for k in unet_sd if k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block")}
    assert enc == {k for k in sd if not k.startswith("controlnet_")}
    assert not any(k.startswith(("up_blocks", "conv_out", "conv_norm_out")) for k in sd)
    with torch.device("meta"):
        full = ControlNetModel()
    fsd = full.state_dict()
    widths = [320] * 4 + [640] * 3 + [1280] * 5
    assert [tuple(fsd[f"controlnet_down_blocks.{k}.weight"].shape) for k in range(12)] == [(c, c, 1, 1) for c in widths]
    assert "controlnet_down_blocks.12.weight" not in fsd and tuple(fsd["controlnet_mid_block.weight"].shape) == (1280, 1280, 1, 1)
    assert tuple(fsd["controlnet_cond_embedding.conv_out.weight"].shape) == (320, 256, 3, 3)
    assert tuple(fsd["down_blocks.2.attentions.1.transformer_blocks.0.attn2.to_k.weight"].shape) == (1280, 768)


def test_from_unet_copies_the_encoder_and_unet_stages_is_what_it_was():
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.controlnet import ControlNetModel
    from photoverse_amd.unet import UNet2DConditionModel, plan_ranges, unet_stages
    torch.manual_seed(3)
    unet = UNet2DConditionModel(**TINY_CONFIG)
    cn = ControlNetModel.from_unet(unet)
    usd, csd = unet.state_dict(), cn.state_dict()
    copied = [k for k in csd if not k.startswith("controlnet_")]
    assert len(copied) > 50 and all(torch.equal(csd[k], usd[k]) for k in copied)
    assert all(not csd[k].any() for k in csd if k.startswith(("controlnet_down_blocks", "controlnet_mid_block")))
    assert cn.config.block_out_channels == unet.config.block_out_channels
    v0 = cn.__dict__.get("_pack_version", 0)
    cn.randomize_zero_convs_(seed=2)
    assert cn.controlnet_mid_block.weight.any() and cn.controlnet_cond_embedding.conv_out.weight.any() and cn.__dict__["_pack_version"] > v0
    v1 = cn.__dict__["_pack_version"]
    cn.load_state_dict(cn.state_dict())
    assert cn.__dict__["_pack_version"] > v1
    # the encoder-only walk is the head of the UNet's walk, and the control range covers all of it
    whole, enc = unet_stages(unet), unet_stages(cn, encoder_only=True)
    assert [(s.kind, s.name, s.block, s.level, s.skip, s.toff, s.tcols) for s in enc] == [(s.kind, s.name, s.block, s.level, s.skip, s.toff, s.tcols) for s in whole[:len(enc)]]
    assert enc[-1].name == "mid_block.resnets.1" and unet_stages(unet, encoder_only=True)[-1].name == "mid_block.resnets.1"
    assert plan_ranges(enc, "control") == ((0, len(enc) - 1, None, None),) == plan_ranges(whole, "control")
    assert sum(s.skip for s in enc) == len(cn.controlnet_down_blocks) == 4


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    """``pv_hint_conv3x3``: fourteen parameters and the stream, declared in the header, bound by ``_lib.load()`` and exported by the library, whose ABI
    number stays 19."""
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_hint_conv3x3\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_hint_conv3x3"]
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 15
    assert args == [_lib.c_void_p, _lib.c_int, _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p] + [_lib.c_int] * 8 + [_lib.c_void_p]
    assert lib.pv_hint_conv3x3 is not None and lib.pv_hint_conv3x3.argtypes == args
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    from photoverse_amd.build import SOURCES
    assert "pv_hintconv.hip" in SOURCES


def test_cabi_rejects_bad_hint_conv_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed): null pointers, a stride other than 1 / 2,
    an unknown activation, a leading dimension below the channel count (or not a multiple of 8), unsupported channel counts, misaligned pointers,
    non-positive sizes and buffers of 2^31 bytes or more.  The pointers are never dereferenced; no valid call is sent."""
    INVALID = 1
    X, W, BIAS, OUT = (0x10000 * (i + 1) for i in range(4))

    def call(x=X, image=0, ldx=16, w=W, bias=BIAS, out=OUT, ldo=32, batch=1, cin=16, cout=32, h=8, wd=8, stride=1, act=1):
        return lib.pv_hint_conv3x3(x, image, ldx, w, bias, out, ldo, batch, cin, cout, h, wd, stride, act, None)

    for image, cin in ((0, 16), (1, 3)):
        kw = dict(image=image, cin=cin)
        for name in ("x", "w", "bias", "out"):
            assert call(**{name: None}, **kw) == INVALID, name
        for stride in (0, 3, 4, -1, -2):
            assert call(stride=stride, **kw) == INVALID, stride
        for act in (2, 3, 4, 5, -1, 100):                               # only PV_ACT_NONE (0) and PV_ACT_SILU (1)
            assert call(act=act, **kw) == INVALID, act
        for ldo in (31, 16, 0, -32, 36):
            assert call(ldo=ldo, **kw) == INVALID, ldo
        for cout in (0, -16, 8, 24, 40, 257, 272, 512):
            assert call(cout=cout, ldo=512, **kw) == INVALID, cout
        for name in ("batch", "h", "wd"):
            for v in (0, -1):
                assert call(**{name: v}, **kw) == INVALID, (name, v)
        for name in ("w", "bias", "out"):
            assert call(**{name: 0x10008}, **kw) == INVALID, name
        assert call(image=2, cin=cin) == INVALID and call(image=-1, cin=cin) == INVALID
        # out: batch * ho * wo rows of ldo fp16 elements reach 2^31 bytes
        assert call(batch=1, h=1 << 13, wd=1 << 12, ldo=32, **kw) == INVALID                       # 2^25 rows x 64 bytes
        assert call(batch=1 << 10, h=1 << 11, wd=1 << 11, **kw) == INVALID                          # 2^32 rows
        m = (1 << 31) - 1
        assert call(batch=m, h=m, wd=m, **kw) == INVALID
    for ldx in (15, 8, 0, -16, 20):                                      # rows form: ldx >= cin, a multiple of 8
        assert call(ldx=ldx) == INVALID, ldx
    for cin in (0, -8, 3, 4, 12, 20, 260, 264, 512):                     # rows form: cin % 8 == 0, <= 256
        assert call(cin=cin, ldx=512) == INVALID, cin
    for cin in (0, -1, 5, 8, 16):                                        # image form: cin <= 4
        assert call(image=1, cin=cin) == INVALID, cin
    assert call(x=0x10008) == INVALID and call(image=1, cin=3, x=0x10002) == INVALID
    # x: rows form 2^22 pixels x ldx 256 x 2 bytes = 2^31 (the output, at stride 2 and ldo 32, stays small); image form 2^27 pixels x 4 channels x 4 bytes
    assert call(h=1 << 11, wd=1 << 11, ldx=256, stride=2) == INVALID
    assert call(image=1, cin=4, h=1 << 14, wd=1 << 13, stride=2, cout=16, ldo=16) == INVALID


def test_keywords_are_validated_before_a_model_runs():
    from photoverse_amd.infer import run_inference
    from photoverse_amd.pipeline import DenoiseLoop
    sig = inspect.signature(run_inference).parameters
    for name, default in (("controlnet", None), ("control_image", None), ("controlnet_conditioning_scale", 1.0)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    lsig = inspect.signature(DenoiseLoop.__init__).parameters
    assert lsig["controlnet"].default is None and lsig["conditioning_scale"].default == 1.0 and hasattr(DenoiseLoop, "set_control")
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=5.0, timesteps=4)
    img = torch.zeros(2, 3, 128, 128)
    with pytest.raises(ValueError, match="controlnet.*control_image|control_image.*controlnet"):
        run_inference(*args, controlnet=u, **kw)
    with pytest.raises(ValueError, match="controlnet.*control_image|control_image.*controlnet"):
        run_inference(*args, control_image=img, **kw)
    for bad in (math.nan, math.inf, -math.inf, "1", True, [1.0], 1 + 2j, None):
        with pytest.raises(ValueError, match="controlnet_conditioning_scale"):
            run_inference(*args, controlnet=u, control_image=img, controlnet_conditioning_scale=bad, **kw)
    for bad in (torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 128, 120), torch.zeros(2, 1, 128, 128), torch.zeros(3, 128, 128), "image", [[1.0]]):
        with pytest.raises(ValueError, match="control_image"):
            run_inference(*args, controlnet=u, control_image=bad, **kw)
    with pytest.raises(ValueError, match="controlnet.*training_mode"):
        run_inference(*args, controlnet=u, control_image=img, training_mode=True, **kw)
    with pytest.raises(ValueError, match="controlnet.*hires_latent_size"):
        run_inference(*args, controlnet=u, control_image=img, hires_latent_size=32, **kw)
    # legal (and off at scale 0): the next thing is the first touch of a model argument
    for good in (dict(), dict(controlnet=u, control_image=img), dict(controlnet=u, control_image=img[:1], controlnet_conditioning_scale=0.5),
                 dict(controlnet=u, control_image=img, controlnet_conditioning_scale=0)):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)
    # DenoiseLoop: the scale and the training_mode exclusion are checked before the UNet or the ControlNet is touched (the rest needs a HIP device:
    # test_controlnet_gpu)
    for bad in (math.nan, math.inf, -math.inf, "1", True, None):
        with pytest.raises(ValueError, match="conditioning_scale"):
            DenoiseLoop(u, 2, 16, 1, 4, 5.0, controlnet=u, conditioning_scale=bad)
    with pytest.raises(ValueError, match="controlnet.*training_mode"):
        DenoiseLoop(u, 2, 16, 1, 4, 5.0, controlnet=u, training_mode=True)
    for off in (dict(), dict(controlnet=None), dict(controlnet=u, conditioning_scale=0), dict(controlnet=u, conditioning_scale=0.5)):
        with pytest.raises(AssertionError, match="touched a model argument"):          # legal: got past the validation to the first touch of the UNet
            DenoiseLoop(u, 2, 16, 1, 4, 5.0, **off)
    # with the scale at 0 the control is off: its exclusions do not fire
    for kw_off in (dict(training_mode=True), dict(hires_latent_size=32)):
        with torch.no_grad(), pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, controlnet=u, control_image=img, controlnet_conditioning_scale=0, **kw_off, **kw)
    with pytest.raises(ValueError, match="latent_size"):
        run_inference(*args, controlnet=u, control_image=img, **dict(kw, latent_size=16.5))


def test_pipeline_slices_a_batch_sized_control_image_with_its_samples(monkeypatch):
    """``PhotoVersePipeline(shard=True)`` hands a rank the rows of a batch-sized ``control_image`` that belong to its samples and a single image whole;
    unsharded, the keywords arrive unchanged."""
    import torch.distributed as dist
    import photoverse_amd.infer as infer
    from photoverse_amd.pipeline import PhotoVersePipeline, shard_batch
    seen = []

    def fake(example, *a, **kw):
        seen.append(kw)
        return torch.zeros(example["pixel_values_clip"].shape[0], 4, 2, 2)

    monkeypatch.setattr(infer, "run_inference", fake)
    pipe = PhotoVersePipeline(*([None] * 8))
    ex = {"pixel_values_clip": torch.zeros(4, 3, 4, 4)}
    img = torch.arange(4.0).view(4, 1, 1, 1).expand(4, 3, 8, 8).contiguous()
    pipe(ex, controlnet="cn", control_image=img, controlnet_conditioning_scale=0.5)
    assert seen[-1]["control_image"] is img and seen[-1]["controlnet"] == "cn" and seen[-1]["controlnet_conditioning_scale"] == 0.5
    monkeypatch.setattr(dist, "get_rank", lambda: 1)                   # rank 1 of 2, without a process group: the one collective is replaced too
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    monkeypatch.setattr("photoverse_amd.pipeline.gather_latents", lambda local, world, force=False: local)
    pipe(ex, shard=True, controlnet="cn", control_image=img)
    assert torch.equal(seen[-1]["control_image"], img[shard_batch(4, 1, 2)]) and seen[-1]["control_image"][:, 0, 0, 0].tolist() == [2.0, 3.0]
    pipe(ex, shard=True, controlnet="cn", control_image=img[:1])
    assert torch.equal(seen[-1]["control_image"], img[:1])


def test_cli_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_controlnet", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.controlnet_path is None and d.control_image_path is None and d.controlnet_conditioning_scale == 1.0
    a = gen.parser.parse_args(["--controlnet_path", "random", "--control_image_path", "pose.png", "--controlnet_conditioning_scale", "0.7"])
    assert a.controlnet_path == "random" and a.control_image_path == "pose.png" and a.controlnet_conditioning_scale == 0.7
    assert "--controlnet_path" in open(os.path.join(ROOT, "README.md")).read()
