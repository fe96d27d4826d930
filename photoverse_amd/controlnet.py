"""[EXT] SD-v1.5 ``ControlNetModel`` (Zhang et al. 2023; parameter names of diffusers' ``ControlNetModel``) executed by HIP kernels (gfx950).

Nothing in the reference: spatial control (pose, edges, depth) beside the identity adapter.  A ControlNet is the UNet's encoder - ``conv_in`` ...
``mid_block.resnets.1`` of ``unet.unet_stages`` - with weights of its own, plus

* ``controlnet_cond_embedding``: eight 3x3 convs (3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 -> c0, three of them stride 2, SiLU behind all but the last)
  that take the control image at 8x the latent resolution to the ``hint`` added to ``conv_in(sample)``;
* ``controlnet_down_blocks.k``: one zero-initialised 1x1 conv per skip connection the encoder pushes, and ``controlnet_mid_block`` for the mid block's output.

Forward: ``temb`` as in the UNet; ``x = conv_in(sample) + hint``; down path and mid block as in the UNet with text-only cross-attention;
``res_k = scale * zero_k(skip_k)``, ``res_mid = scale * zero_mid(x)``.  The UNet then runs with ``skip_k + res_k`` in place of its stored skips (its own
down path continues on the raw activations) and ``x + res_mid`` behind its mid block (``UNetEngine(control=...)``).

Like the UNet's, the module tree only HOLDS parameters; execution is a static launch plan (``UNetEngine(segment="control")`` over the same stage walk;
``hint_plan`` for the embedding: seven ``pv_hint_conv3x3`` launches and one ``pv_gemm_conv``).  No CPU path exists.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from . import ops
from .ops import ACT_NONE, ACT_SILU, Recorder
from .unet import SD15_CONFIG, DownBlock, MidBlock, TimestepEmbedding, UNetEngine, _Holder, _conv3_w, _f32, unet_stages

#: (cin, cout, stride) of ``controlnet_cond_embedding.blocks``
HINT_BLOCKS = ((16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2))


class ControlNetConditioningEmbedding(_Holder):
    def __init__(self, c0: int, cond_channels: int = 3):
        super().__init__()
        self.conv_in = nn.Conv2d(cond_channels, 16, 3, padding=1)
        self.blocks = nn.ModuleList([nn.Conv2d(ci, co, 3, padding=1, stride=s) for ci, co, s in HINT_BLOCKS])
        self.conv_out = nn.Conv2d(256, c0, 3, padding=1)
        nn.init.zeros_(self.conv_out.weight)
        nn.init.zeros_(self.conv_out.bias)


def _zero_conv(ch: int) -> nn.Conv2d:
    m = nn.Conv2d(ch, ch, 1)
    nn.init.zeros_(m.weight)
    nn.init.zeros_(m.bias)
    return m


def hint_plan(rec: Recorder, emb: ControlNetConditioningEmbedding, image: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Record the conditioning embedding of ``image`` (fp32 (B, 3, 8 S, 8 S), static) into ``out`` (fp16 rows [B * S * S][c0], static): seven
    ``pv_hint_conv3x3`` launches, then ``conv_out`` (256 -> c0 at the latent resolution, no activation) on ``pv_gemm_conv``."""
    B, _, h, w = image.shape
    x = rec.hint_conv(image, _conv3_w(emb.conv_in.weight), _f32(emb.conv_in.bias), batch=B, h=h, wd=w, act=ACT_SILU)
    for m in emb.blocks:
        s = m.stride[0]
        x = rec.hint_conv(x, _conv3_w(m.weight), _f32(m.bias), batch=B, h=h, wd=w, stride=s, act=ACT_SILU)
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
    assert out.shape[0] == B * h * w, (out.shape, B, h, w)
    return rec.gemm(x, _conv3_w(emb.conv_out.weight), bias=_f32(emb.conv_out.bias), conv=dict(batch=B, hin=h, win=w, hout=h, wout=w), out=out, act=ACT_NONE)


class ControlNetModel(nn.Module):
    def __init__(self, **overrides):
        super().__init__()
        cfg = dict(SD15_CONFIG)
        cfg.update(overrides)
        cfg.setdefault("conditioning_channels", 3)
        self.config = SimpleNamespace(**cfg)
        boc = tuple(cfg["block_out_channels"])
        heads, xdim, groups, layers = cfg["attention_head_dim"], cfg["cross_attention_dim"], cfg["norm_num_groups"], cfg["layers_per_block"]
        temb = boc[0] * 4
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(boc[0], cfg["conditioning_channels"])
        self.down_blocks = nn.ModuleList()
        cout = boc[0]
        for i, kind in enumerate(cfg["down_block_types"]):
            cin, cout = cout, boc[i]
            self.down_blocks.append(DownBlock(cin, cout, temb, layers, heads, xdim, groups, kind.startswith("CrossAttn"), i != len(boc) - 1))
        self.mid_block = MidBlock(boc[-1], temb, heads, xdim, groups)
        # one zero conv per skip the encoder pushes, of that skip's width; one for the mid block's output
        self.controlnet_down_blocks = nn.ModuleList([_zero_conv(boc[st.block[1]]) for st in unet_stages(self, encoder_only=True) if st.skip > 0])
        self.controlnet_mid_block = _zero_conv(boc[-1])
        self._engines: Dict[tuple, tuple] = {}

    # ---- constructors ----
    @classmethod
    def from_unet(cls, unet) -> "ControlNetModel":
        """A ControlNet on ``unet``'s configuration with its encoder weights copied (``conv_in``, ``time_embedding``, ``down_blocks``, ``mid_block``);
        the conditioning embedding keeps its default init (``conv_out`` zero) and every zero conv is zero: the controlled UNet computes what the plain
        one does until the ControlNet is trained."""
        cn = cls(**{k: v for k, v in vars(unet.config).items()})
        own = cn.state_dict()
        src = {k: v for k, v in unet.state_dict().items() if k in own and k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block")}
        cn.load_state_dict(src, strict=False)
        return cn.to(unet.conv_in.weight.device)

    @classmethod
    def from_pretrained(cls, path: str, **overrides) -> "ControlNetModel":
        """``<path>/diffusion_pytorch_model.safetensors`` in diffusers' layout, strict: every parameter must come from the file."""
        from .modeling_utils import _load_safetensors_into
        cn = cls(**overrides)
        _load_safetensors_into(cn, os.path.join(path, "diffusion_pytorch_model.safetensors"), "controlnet", strict=True)
        cn.repack()
        return cn

    def randomize_zero_convs_(self, seed: int = 0, std: float = 0.05, embedding_gain: float = 1.75) -> "ControlNetModel":
        """Seeded non-zero init of ``controlnet_cond_embedding.conv_out`` and of every zero conv (weights ~ N(0, std^2), biases 0): an untrained ControlNet
        whose control has an effect - smoke runs and tests, ``generate.py --controlnet_path random``.  ``embedding_gain`` (None: leave them): the
        embedding's seven SiLU convs are re-drawn as N(0, (gain / sqrt(9 cin))^2) - at their default init the biases carry the hint and the control
        IMAGE's share of it is four orders below ``conv_in(sample)``; at 1.75 the hint is of that order and follows the image."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            if embedding_gain is not None:
                emb = self.controlnet_cond_embedding
                for m in [emb.conv_in, *emb.blocks]:
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) * float(embedding_gain) / (9 * m.weight.shape[1]) ** 0.5)
            for m in [self.controlnet_cond_embedding.conv_out, *self.controlnet_down_blocks, self.controlnet_mid_block]:
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * std)
        self.repack()
        return self

    # ---- cache plumbing, as the UNet's: cached plans and loops are dropped when the weights change ----
    def repack(self):
        self._engines.clear()
        self.__dict__["_pack_version"] = self.__dict__.get("_pack_version", 0) + 1

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.repack()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._engines = {}
        self.__dict__["_pack_version"] = self.__dict__.get("_pack_version", 0) + 1
        return r

    @property
    def device(self):
        return self.conv_in.weight.device

    def control_engine(self, batch: int, h: int, w: int, n_ip: int, hint: torch.Tensor, t_rows: int = 1, **kw) -> UNetEngine:
        """The control plan for one shape over caller-owned static buffers (``hint`` and ``kw``: ``latents_in``, ``text``, ``ip``, ``timesteps``, ``state``, ...)."""
        if self.device.type != "cuda":
            raise RuntimeError("photoverse_amd.ControlNetModel runs on a HIP device only (no CPU path): call .to('cuda')")
        return UNetEngine(self, batch, h, w, n_ip, t_rows, self.device, segment="control", hint=hint, **kw)

    def forward(self, sample: torch.Tensor, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale: float = 1.0) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """``(down residuals, mid residual)`` in fp32 NCHW: ``conditioning_scale * zero_k(skip_k)`` per pushed skip and the same of the mid block's output
        - what diffusers' ``ControlNetModel`` returns.  ``encoder_hidden_states``: the text embeddings (B, 77, xdim); ``controlnet_cond``: the control
        image (B, 3, 8 h, 8 w); ``timestep``: one value, or one per sample.  For inspection and tests; the denoising loop reads the control features
        directly (``DenoiseLoop(controlnet=...)``).  The plans of the four most recent shapes are kept."""
        ops.require_cuda(sample, "sample")
        B, _, h, w = sample.shape
        text = encoder_hidden_states[0] if isinstance(encoder_hidden_states, tuple) else encoder_hidden_states
        if controlnet_cond is None or tuple(controlnet_cond.shape) != (B, self.config.conditioning_channels, 8 * h, 8 * w):
            raise ValueError(f"controlnet_cond must be ({B}, {self.config.conditioning_channels}, {8 * h}, {8 * w}), got "
                             f"{None if controlnet_cond is None else tuple(controlnet_cond.shape)}")
        dev, c0 = sample.device, self.config.block_out_channels[0]
        t = (timestep if torch.is_tensor(timestep) else torch.tensor([timestep])).reshape(-1)
        if t.numel() not in (1, B):
            raise ValueError(f"timestep has {t.numel()} values, expected 1 or one per sample ({B})")
        key = (B, h, w, text.shape[1], t.numel())
        if key not in self._engines:
            while len(self._engines) >= 4:
                self._engines.pop(next(iter(self._engines)))
            image = torch.zeros((B, self.config.conditioning_channels, 8 * h, 8 * w), dtype=torch.float32, device=dev)
            hint = torch.zeros((B * h * w, c0), dtype=torch.float16, device=dev)
            hrec = Recorder(dev)
            hint_plan(hrec, self.controlnet_cond_embedding, image, hint)
            ip = torch.zeros((B, self.config.cross_attention_dim), dtype=torch.float16, device=dev)
            self._engines[key] = (image, hrec, self.control_engine(B, h, w, 1, hint, t_rows=t.numel(), n_text=text.shape[1], ip=ip))
        image, hrec, eng = self._engines[key]
        image.copy_(controlnet_cond)
        eng.x_in.copy_(sample)
        eng.text.copy_(text.reshape(-1, text.shape[-1]))
        eng.timesteps.copy_(t.to(device=dev, dtype=torch.float32))
        hrec.run()
        eng.run()
        rec, outs = Recorder(dev), []
        s = float(conditioning_scale)
        for c, m in zip(eng.control_skips + [eng.control_mid], [*self.controlnet_down_blocks, self.controlnet_mid_block]):
            wz = (s * m.weight.detach().float().reshape(m.weight.shape[0], -1)).to(torch.float16).contiguous()
            outs.append(rec.gemm(c, wz, bias=(s * m.bias.detach().float()).contiguous(), out_f32=True))
        rec.run()
        nchw = [o.view(B, hh, ww, o.shape[1]).permute(0, 3, 1, 2).contiguous() for o, (hh, ww) in zip(outs, self._feature_sizes(h, w))]
        return nchw[:-1], nchw[-1]

    def _feature_sizes(self, h: int, w: int):
        sizes = [(h >> st.level, w >> st.level) if st.kind != "downsample" else (h >> (st.level + 1), w >> (st.level + 1))
                 for st in unet_stages(self, encoder_only=True) if st.skip > 0]
        return sizes + [sizes[-1]]
