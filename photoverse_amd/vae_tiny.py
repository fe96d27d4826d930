"""[EXT] ``AutoencoderTiny`` (diffusers' name; the TAESD weights): the tiny autoencoder every Stable Diffusion front end ships beside the KL VAE - a fast final
decode and a cheap latents-to-RGB.  19 plain 3x3 convs at width 64 per direction, no GroupNorm, no attention; every conv is one ``pv_tiny_conv3x3`` launch
(``csrc/pv_tinyconv.hip``) with ReLU, the block's residual, the nearest-x2 upsample, the stride, the input transform and the output affine fused: 35 launches
per direction whatever the batch.

The architecture is written from memory of diffusers' ``AutoencoderTiny`` / ``EncoderTiny`` / ``DecoderTiny`` - nothing here can check it against diffusers;
DESIGN.md section 5 is the definition:

    block(x)  = relu(conv.4(relu(conv.2(relu(conv.0(x))))) + x)                    three 64 -> 64 convs with bias, identity skip
    decoder   = conv(4 -> 64, bias) on 3 tanh(z / 3), ReLU; per level i: num_decoder_blocks[i] blocks, then (all but the last level) Upsample x2 and a
                conv 64 -> 64 WITHOUT bias; last: conv 64 -> 3 with bias; the image is 2 y - 1
    encoder   = on (x + 1) / 2: conv(3 -> 64, bias), num_encoder_blocks[0] blocks; per further level a stride-2 conv 64 -> 64 WITHOUT bias and its blocks;
                last: conv 64 -> 4 with bias

Parameter names are diffusers' (``decoder.layers.N``, ``encoder.layers.N``, blocks ``.conv.{0,2,4}``): the indices count the parameter-free ReLU / Upsample
entries too.  ``config.scaling_factor`` is 1.0 - TAESD works on the UNet's own latents - so the object drops into ``run_inference`` as the ``vae``.

Plans: one ``Recorder`` per (direction, sub-batch, h, w, device), cached; the activations of one resolution level rotate through at most FOUR buffers (a block
needs three: its input, which is also its residual, and two temporaries - its output goes into the first temporary), whatever the block counts.
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Dict, List

import torch
import torch.nn as nn

from .ops import ACT_NONE, ACT_RELU, Recorder, require_cuda

TAESD_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=4, encoder_block_out_channels=(64, 64, 64, 64),
                    decoder_block_out_channels=(64, 64, 64, 64), num_encoder_blocks=(1, 3, 3, 3), num_decoder_blocks=(3, 3, 3, 1), act_fn="relu",
                    upsampling_scaling_factor=2, latent_magnitude=3, latent_shift=0.5, scaling_factor=1.0)
WIDTH = 64                       # the one width pv_tiny_conv3x3 has
BUFFERS_PER_LEVEL = 4


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise NotImplementedError(f"{type(self).__name__} only holds parameters")


class _Block(_Holder):
    def __init__(self):
        super().__init__()
        self.conv = nn.ModuleList([nn.Conv2d(WIDTH, WIDTH, 3, padding=1), _Holder(), nn.Conv2d(WIDTH, WIDTH, 3, padding=1), _Holder(),
                                   nn.Conv2d(WIDTH, WIDTH, 3, padding=1)])


class _Relu(_Holder):
    pass


class _Upsample(_Holder):
    pass


class _Layers(_Holder):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)


def _decoder_layers(latent, out_channels, blocks):
    layers: List[nn.Module] = [nn.Conv2d(latent, WIDTH, 3, padding=1), _Relu()]
    for i, nb in enumerate(blocks):
        last = i == len(blocks) - 1
        layers += [_Block() for _ in range(nb)]
        if not last:
            layers.append(_Upsample())
        layers.append(nn.Conv2d(WIDTH, out_channels if last else WIDTH, 3, padding=1, bias=last))
    return layers


def _encoder_layers(in_channels, latent, blocks):
    layers: List[nn.Module] = []
    for i, nb in enumerate(blocks):
        layers.append(nn.Conv2d(in_channels, WIDTH, 3, padding=1) if i == 0 else nn.Conv2d(WIDTH, WIDTH, 3, padding=1, stride=2, bias=False))
        layers += [_Block() for _ in range(nb)]
    layers.append(nn.Conv2d(WIDTH, latent, 3, padding=1))
    return layers


class _Deterministic:
    """What ``run_inference`` reads as ``latent_dist``: TAESD's encoder is deterministic, so ``sample()`` and ``mode()`` are the latents themselves."""

    def __init__(self, latents):
        self.latents = latents

    def sample(self, generator=None):
        return self.latents

    def mode(self):
        return self.latents


def _check_config(cfg):
    for name in ("encoder_block_out_channels", "decoder_block_out_channels"):
        if any(int(c) != WIDTH for c in cfg[name]) or len(cfg[name]) < 1:
            raise ValueError(f"AutoencoderTiny: {name} must be {WIDTH} at every level (the one width pv_tiny_conv3x3 has), got {tuple(cfg[name])}")
    if cfg["act_fn"] != "relu":
        raise ValueError(f"AutoencoderTiny: act_fn must be 'relu', got {cfg['act_fn']!r}")
    if cfg["upsampling_scaling_factor"] != 2:
        raise ValueError(f"AutoencoderTiny: upsampling_scaling_factor must be 2, got {cfg['upsampling_scaling_factor']!r}")
    for name, blocks in (("num_encoder_blocks", "encoder_block_out_channels"), ("num_decoder_blocks", "decoder_block_out_channels")):
        if len(cfg[name]) != len(cfg[blocks]) or any(int(n) < 0 for n in cfg[name]):
            raise ValueError(f"AutoencoderTiny: {name} must hold one non-negative count per level of {blocks}, got {tuple(cfg[name])}")
    if len(cfg["num_encoder_blocks"]) != len(cfg["num_decoder_blocks"]):
        raise ValueError(f"AutoencoderTiny: num_encoder_blocks and num_decoder_blocks must have the same number of levels, got "
                         f"{tuple(cfg['num_encoder_blocks'])} and {tuple(cfg['num_decoder_blocks'])}")
    for name in ("in_channels", "out_channels", "latent_channels"):
        if not 1 <= int(cfg[name]) <= 4:
            raise ValueError(f"AutoencoderTiny: {name} must be 1 ... 4 (the image forms of pv_tiny_conv3x3), got {cfg[name]!r}")


def _conv3_w(w):
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.float16).contiguous()


class AutoencoderTiny(nn.Module):
    """``decode(z).sample``: fp32 (B, 4, h, w) -> fp32 (B, 3, 8h, 8w), not clamped.  ``encode(x)``: fp32 (B, 3, H, W) in [-1, 1] -> ``.latents`` (B, 4,
    ceil(H / 8), ceil(W / 8)) and a ``.latent_dist`` whose ``sample()`` / ``mode()`` return the same tensor.  Any extents >= 1."""

    MAX_OPERAND_BYTES = 1 << 30     # as AutoencoderKL: every activation operand well under the 2 GiB the launcher accepts

    def __init__(self, **overrides):
        super().__init__()
        cfg = dict(TAESD_CONFIG)
        cfg.update(overrides)
        for name in ("encoder_block_out_channels", "decoder_block_out_channels", "num_encoder_blocks", "num_decoder_blocks"):
            cfg[name] = tuple(cfg[name])
        _check_config(cfg)
        self.config = SimpleNamespace(**cfg)
        self.decoder = _Layers(_decoder_layers(cfg["latent_channels"], cfg["out_channels"], cfg["num_decoder_blocks"]))
        self.encoder = _Layers(_encoder_layers(cfg["in_channels"], cfg["latent_channels"], cfg["num_encoder_blocks"]))
        self._plans: Dict[tuple, object] = {}
        self._packed: Dict[tuple, tuple] = {}

    # ---- constructors / state, as the other models ----
    @classmethod
    def from_pretrained(cls, path: str, **overrides) -> "AutoencoderTiny":
        """``<path>/config.json`` (the fields of ``TAESD_CONFIG`` it holds) and ``<path>/diffusion_pytorch_model.safetensors`` in diffusers' layout, strict:
        every parameter must come from the file."""
        from .modeling_utils import _load_safetensors_into       # imports safetensors lazily
        cfg = {}
        cfg_path = os.path.join(path, "config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as f:
                cfg = {k: v for k, v in json.load(f).items() if k in TAESD_CONFIG}
        cfg.update(overrides)
        m = cls(**cfg)
        _load_safetensors_into(m, os.path.join(path, "diffusion_pytorch_model.safetensors"), "tiny autoencoder", strict=True)
        m.repack()
        return m

    def repack(self):
        self._plans.clear()
        self._packed.clear()

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.repack()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._plans, self._packed = {}, {}
        return r

    @property
    def device(self):
        return self.decoder.layers[0].weight.device

    @property
    def _up(self) -> int:
        return 2 ** (len(self.config.num_decoder_blocks) - 1)

    def scale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """raw latents -> [0, 1] (plain torch, diffusers' helper): ``x / (2 latent_magnitude) + latent_shift``, clamped."""
        return x.div(2 * self.config.latent_magnitude).add(self.config.latent_shift).clamp(0, 1)

    def unscale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """[0, 1] -> raw latents: ``(x - latent_shift) * 2 latent_magnitude``."""
        return x.sub(self.config.latent_shift).mul(2 * self.config.latent_magnitude)

    # ---- plans ----
    def _wb(self, conv: nn.Conv2d):
        """(tap-major fp16 weight, fp32 bias or None) of one conv, packed once per ``repack``."""
        key = id(conv)
        if key not in self._packed:
            self._packed[key] = (_conv3_w(conv.weight), None if conv.bias is None else conv.bias.detach().to(torch.float32).contiguous())
        return self._packed[key]

    def _plan_key(self, kind, sb, h, w, dev):
        return (kind, sb, h, w, dev)

    def _sub_batch(self, batch, h, w):
        """``h`` x ``w``: the largest activation grid of the plan (decode: the output's; encode: the input's)."""
        return max(1, min(batch, self.MAX_OPERAND_BYTES // (WIDTH * h * w * 2)))

    @staticmethod
    def _pool(rec: Recorder, levels: dict, level: int, rows: int, live):
        """A buffer of ``level``'s pool that none of ``live`` occupies; the pool grows to BUFFERS_PER_LEVEL and no further."""
        pool = levels.setdefault(level, [])
        for t in pool:
            if all(t is not u for u in live):
                return t
        assert len(pool) < BUFFERS_PER_LEVEL, (level, len(pool))
        pool.append(rec.empty((rows, WIDTH)))
        return pool[-1]

    def _block(self, rec, levels, level, blk: _Block, x, geo):
        rows = x.shape[0]
        (w0, b0), (w2, b2), (w4, b4) = self._wb(blk.conv[0]), self._wb(blk.conv[2]), self._wb(blk.conv[4])
        t1 = rec.tiny_conv(x, w0, b0, act=ACT_RELU, out=self._pool(rec, levels, level, rows, (x,)), **geo)
        t2 = rec.tiny_conv(t1, w2, b2, act=ACT_RELU, out=self._pool(rec, levels, level, rows, (x, t1)), **geo)
        return rec.tiny_conv(t2, w4, b4, act=ACT_RELU, residual=x, out=t1, **geo)       # t1 is dead: the block's output takes its place

    def _plan_decode(self, sb, h, w, dev):
        cfg, layers = self.config, list(self.decoder.layers)
        rec, levels, level = Recorder(dev), {}, 0
        z = rec.empty((sb, cfg.latent_channels, h, w), torch.float32)
        wi, bi = self._wb(layers[0])
        x = rec.tiny_conv(z, wi, bi, batch=sb, h=h, wd=w, pre="tanh3", act=ACT_RELU, out=self._pool(rec, levels, 0, sb * h * w, ()))
        img, up_next = None, False
        for i, m in enumerate(layers[2:], 2):
            if isinstance(m, _Block):
                x = self._block(rec, levels, level, m, x, dict(batch=sb, h=h, wd=w))
            elif isinstance(m, _Upsample):
                up_next = True
            elif i == len(layers) - 1:
                wo, bo = self._wb(m)
                img = rec.tiny_conv(x, wo, bo, batch=sb, h=h, wd=w, image_out=True, out_scale=2.0, out_shift=-1.0)
            else:
                wc, bc = self._wb(m)
                ho, wo_ = (2 * h, 2 * w) if up_next else (h, w)
                nxt = level + 1 if up_next else level
                x = rec.tiny_conv(x, wc, bc, batch=sb, h=h, wd=w, upsample=up_next,
                                  out=self._pool(rec, levels, nxt, sb * ho * wo_, (x,)))
                h, w, level, up_next = ho, wo_, nxt, False
        return SimpleNamespace(rec=rec, z=z, img=img, levels=levels)

    def _plan_encode(self, sb, H, W, dev):
        cfg, layers = self.config, list(self.encoder.layers)
        rec, levels, level = Recorder(dev), {}, 0
        x_in = rec.empty((sb, cfg.in_channels, H, W), torch.float32)
        h, w = H, W
        wi, bi = self._wb(layers[0])
        x = rec.tiny_conv(x_in, wi, bi, batch=sb, h=h, wd=w, pre="unit", out=self._pool(rec, levels, 0, sb * h * w, ()))
        lat = None
        for i, m in enumerate(layers[1:], 1):
            if isinstance(m, _Block):
                x = self._block(rec, levels, level, m, x, dict(batch=sb, h=h, wd=w))
            elif i == len(layers) - 1:
                wo, bo = self._wb(m)
                lat = rec.tiny_conv(x, wo, bo, batch=sb, h=h, wd=w, image_out=True)
            else:
                wc, bc = self._wb(m)
                ho, wo_ = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                x = rec.tiny_conv(x, wc, bc, batch=sb, h=h, wd=w, stride=2, out=self._pool(rec, levels, level + 1, sb * ho * wo_, ()))
                h, w, level = ho, wo_, level + 1
        return SimpleNamespace(rec=rec, x=x_in, latents=lat, levels=levels)

    def _run(self, kind, t: torch.Tensor, sb, build, src, dst) -> torch.Tensor:
        B, _, h, w = t.shape
        key = self._plan_key(kind, sb, h, w, t.device)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = build(sb, h, w, t.device)
        outs = []
        for i in range(0, B, sb):
            chunk = t[i:i + sb].to(torch.float32)
            n = chunk.shape[0]
            getattr(plan, src)[:n].copy_(chunk)
            plan.rec.run()
            outs.append(getattr(plan, dst)[:n].clone())
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def decode(self, z: torch.Tensor, generator=None, return_dict=True):
        require_cuda(z, "latents")
        self._need_device(z)
        up = self._up
        img = self._run("dec", z, self._sub_batch(z.shape[0], z.shape[2] * up, z.shape[3] * up), self._plan_decode, "z", "img")
        return SimpleNamespace(sample=img.to(z.dtype))

    def encode(self, x: torch.Tensor, return_dict=True):
        require_cuda(x, "pixel_values")
        self._need_device(x)
        lat = self._run("enc", x, self._sub_batch(x.shape[0], x.shape[2], x.shape[3]), self._plan_encode, "x", "latents").to(x.dtype)
        return SimpleNamespace(latents=lat, latent_dist=_Deterministic(lat))

    def _need_device(self, t):
        if self.device != t.device:
            raise RuntimeError(f"AutoencoderTiny: the weights live on {self.device}, the input on {t.device}: call .to('cuda') (there is no CPU path)")
