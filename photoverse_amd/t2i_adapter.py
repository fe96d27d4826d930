"""[EXT] SD-v1.5 ``T2IAdapter(adapter_type="full_adapter")`` (Mou et al. 2023; parameter names of diffusers' ``T2IAdapter``) executed by HIP kernels (gfx950).

Nothing in the reference: spatial control (pose, depth, edges, sketch, colour, segmentation) at the price of a few pointwise launches per step.  Unlike a
ControlNet (``controlnet.py``) the adapter sees only the control image - not the noisy latents, not the timestep - so its network runs ONCE per generation:

* ``x = PixelUnshuffle(8)(image)``: ``(B, in_channels, 8 S, 8 S)`` in [0, 1] -> ``(B, 64 in_channels, S, S)``, channel ``c * 64 + i * 8 + j`` = pixel
  ``(c, 8 y + i, 8 x + j)``;
* ``x = conv_in(x)`` (3x3, pad 1, -> ``channels[0]``);
* per block ``k``: for ``k > 0`` ``AvgPool2d(2, stride=2, ceil_mode=True)`` (edge blocks average what they have); ``in_conv`` (1x1) where the width changes;
  ``num_res_blocks`` times ``x = block2(relu(block1(x))) + x`` (3x3 pad 1, then 1x1); ``feature[k] = x``.

One feature per UNet down block, at that block's resolution and width.  In diffusers the UNet adds ``s_t * feature[k]`` at the end of down block ``k``,
before that output is pushed as a skip and before the block's downsample (``down_intrablock_additional_residuals``); the launch for that sum exists
(``Recorder.add_feature`` -> ``pv_add_feature_rows``), its hook in ``UNetEngine`` and the loop's keywords do not yet (sections 5 and 7).

Like the UNet's, the module tree only HOLDS parameters; execution is a static launch plan (``adapter_plan``: ``pv_pixel_unshuffle8``, then the convs on
``pv_gemm_conv``, the pools on ``pv_token_pool``, the ReLUs on ``pv_prelu_f16`` with a zero slope).  No CPU path exists.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import List, Sequence, Tuple

import torch
import torch.nn as nn

from .ops import ACT_NONE, Recorder
from .unet import _Holder, _conv1_w, _conv3_w, _f32

#: ``channels`` of the SD-v1.5 checkpoints (= the UNet's ``block_out_channels``)
SD15_ADAPTER_CHANNELS = (320, 640, 1280, 1280)


class AdapterResnetBlock(_Holder):
    def __init__(self, ch: int):
        super().__init__()
        self.block1 = nn.Conv2d(ch, ch, 3, padding=1)
        self.block2 = nn.Conv2d(ch, ch, 1)


class AdapterBlock(_Holder):
    """``in_conv`` exists only where the width changes (diffusers writes no such key otherwise); the pool of blocks ``k > 0`` has no parameters."""

    def __init__(self, cin: int, cout: int, num_res_blocks: int, down: bool):
        super().__init__()
        self.down = bool(down)
        self.in_conv = nn.Conv2d(cin, cout, 1) if cin != cout else None
        self.resnets = nn.ModuleList([AdapterResnetBlock(cout) for _ in range(num_res_blocks)])


class FullAdapter(_Holder):
    def __init__(self, in_channels: int, channels: Sequence[int], num_res_blocks: int, downscale_factor: int):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels * downscale_factor ** 2, channels[0], 3, padding=1)
        self.body = nn.ModuleList([AdapterBlock(channels[max(k - 1, 0)], channels[k], num_res_blocks, down=k > 0) for k in range(len(channels))])


def feature_sizes(h: int, w: int, levels: int) -> List[Tuple[int, int]]:
    """(h_k, w_k) of the adapter's features for an ``h x w`` latent grid: every block after the first halves with ``ceil_mode``."""
    out = []
    for k in range(levels):
        if k > 0:
            h, w = -(-h // 2), -(-w // 2)
        out.append((h, w))
    return out


def adapter_plan(rec: Recorder, adapter: "T2IAdapter", image: torch.Tensor, outs: Sequence[torch.Tensor], batch: int = None) -> List[torch.Tensor]:
    """Record the adapter's forward of ``image`` (fp32 (B or 1, in_channels, 8 S, 8 S), static) into the caller-owned static feature buffers ``outs``
    (fp16 rows ``[B * h_k * w_k][channels[k]]``) and return them.  Launches: ``pv_pixel_unshuffle8``; ``conv_in``; per block the pool (``k > 0``), ``in_conv``
    (where the width changes) and per res block conv3x3 -> ReLU -> conv1x1 + residual, the last one writing ``outs[k]``.  ``batch``: the features' batch when
    the image has batch 1 (read for every sample)."""
    full = adapter.adapter
    B = image.shape[0] if batch is None else int(batch)
    h, w = image.shape[2] // 8, image.shape[3] // 8
    assert len(outs) == len(full.body), (len(outs), len(full.body))
    zero = rec.hold(torch.zeros(1, dtype=torch.float32, device=rec.device))       # PReLU with a zero slope is ReLU
    x = rec.pixel_unshuffle(image, batch=B)
    x = rec.gemm(x, _conv3_w(full.conv_in.weight), bias=_f32(full.conv_in.bias), conv=dict(batch=B, hin=h, win=w, hout=h, wout=w), act=ACT_NONE)
    for k, blk in enumerate(full.body):
        if blk.down:
            x = rec.token_pool(x, batch=B, h=h, w=w, factor=2, method="avg")
            h, w = -(-h // 2), -(-w // 2)
        if blk.in_conv is not None:
            x = rec.gemm(x, _conv1_w(blk.in_conv.weight), bias=_f32(blk.in_conv.bias), rows_per_image=h * w)
        assert tuple(outs[k].shape) == (B * h * w, x.shape[1]), (k, tuple(outs[k].shape), B, h, w, x.shape[1])
        for j, res in enumerate(blk.resnets):
            t = rec.gemm(x, _conv3_w(res.block1.weight), bias=_f32(res.block1.bias), conv=dict(batch=B, hin=h, win=w, hout=h, wout=w))
            t = rec.prelu(t, zero)
            x = rec.gemm(t, _conv1_w(res.block2.weight), bias=_f32(res.block2.bias), residual=x, rows_per_image=h * w,
                         out=outs[k] if j == len(blk.resnets) - 1 else None)
    return list(outs)


class T2IAdapter(nn.Module):
    """Parameter holder under diffusers' names (``adapter.conv_in.*``, ``adapter.body.K.in_conv.*``, ``adapter.body.K.resnets.J.block1.*`` / ``.block2.*``)."""

    def __init__(self, in_channels: int = 3, channels: Sequence[int] = SD15_ADAPTER_CHANNELS, num_res_blocks: int = 2, downscale_factor: int = 8,
                 adapter_type: str = "full_adapter"):
        super().__init__()
        if adapter_type != "full_adapter":
            raise ValueError(f"adapter_type {adapter_type!r}: only 'full_adapter' exists here")
        if downscale_factor != 8:
            raise ValueError("downscale_factor must be 8: the control image is 8 x the latent grid (pv_pixel_unshuffle8)")
        if in_channels not in (1, 3):
            raise ValueError(f"in_channels must be 1 or 3, got {in_channels!r}")
        channels = tuple(int(c) for c in channels)
        if not channels or num_res_blocks < 1:
            raise ValueError("channels and num_res_blocks must name at least one block of at least one res block")
        self.config = SimpleNamespace(in_channels=int(in_channels), channels=channels, num_res_blocks=int(num_res_blocks),
                                      downscale_factor=int(downscale_factor), adapter_type=adapter_type)
        self.adapter = FullAdapter(int(in_channels), channels, int(num_res_blocks), int(downscale_factor))

    @classmethod
    def from_pretrained(cls, path: str, **overrides) -> "T2IAdapter":
        """``<path>/diffusion_pytorch_model.safetensors`` in diffusers' layout, strict: every parameter must come from the file."""
        from .modeling_utils import _load_safetensors_into
        ad = cls(**overrides)
        _load_safetensors_into(ad, os.path.join(path, "diffusion_pytorch_model.safetensors"), "t2i_adapter", strict=True)
        ad.repack()
        return ad

    def randomize_(self, seed: int = 0, gain: float = 1.0) -> "T2IAdapter":
        """Seeded init with weights ~ N(0, (gain / sqrt(fan_in))^2) and zero biases: an untrained adapter whose features are of the UNet activations' order
        and follow the image - smoke runs, tests and ``tools/t2i_adapter_bench.py``."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                    m.weight.copy_((torch.randn(m.weight.shape, generator=g) * float(gain) / fan_in ** 0.5).to(m.weight.device))
                    m.bias.zero_()
        self.repack()
        return self

    # ---- cache plumbing, as the other models': cached loops are dropped when the weights change ----
    def repack(self):
        self.__dict__["_pack_version"] = self.__dict__.get("_pack_version", 0) + 1

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.repack()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.__dict__["_pack_version"] = self.__dict__.get("_pack_version", 0) + 1
        return r

    @property
    def device(self):
        return self.adapter.conv_in.weight.device

    def feature_buffers(self, batch: int, h: int, w: int, device=None) -> List[torch.Tensor]:
        """Zeroed static feature buffers for an ``h x w`` latent grid: fp16 rows ``[batch * h_k * w_k][channels[k]]``."""
        dev = self.device if device is None else device
        return [torch.zeros((batch * hk * wk, c), dtype=torch.float16, device=dev)
                for (hk, wk), c in zip(feature_sizes(h, w, len(self.config.channels)), self.config.channels)]

    def forward(self, image: torch.Tensor) -> List[torch.Tensor]:
        """The features in fp32 NCHW, as diffusers' ``T2IAdapter`` returns them.  Records a fresh plan per call; a caller that runs it more than once keeps
        an ``adapter_plan`` over static buffers of its own."""
        if self.device.type != "cuda":
            raise RuntimeError("photoverse_amd.T2IAdapter runs on a HIP device only (no CPU path): call .to('cuda')")
        cin = self.config.in_channels
        if not torch.is_tensor(image) or image.dim() != 4 or image.shape[1] != cin or image.shape[2] % 8 or image.shape[3] % 8:
            raise ValueError(f"image must be (B, {cin}, 8 h, 8 w), got {tuple(getattr(image, 'shape', ()))}")
        B, h, w = image.shape[0], image.shape[2] // 8, image.shape[3] // 8
        img = image.to(device=self.device, dtype=torch.float32).contiguous()
        outs = self.feature_buffers(B, h, w)
        rec = Recorder(self.device)
        adapter_plan(rec, self, img, outs)
        rec.run()
        return [o.view(B, hk, wk, o.shape[1]).permute(0, 3, 1, 2).float().contiguous() for o, (hk, wk) in zip(outs, feature_sizes(h, w, len(outs)))]
