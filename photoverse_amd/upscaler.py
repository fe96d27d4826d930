"""[EXT] ``RRDBNet``: Real-ESRGAN's 4x super-resolution network (Wang et al. 2021, ``RealESRGAN_x4plus``; basicsr's ``RRDBNet``) - the step every Stable
Diffusion front end offers after the VAE decode.  It runs on the tensor ``run_inference`` returns and touches nothing of the denoising loop.

    RDB(x)    x1 = lrelu(conv1(x)); x2 = lrelu(conv2([x, x1])); x3 = lrelu(conv3([x, x1, x2])); x4 = lrelu(conv4([x .. x3]));
              0.2 * conv5([x .. x4]) + x                      conv1 .. conv4: 64 + 32 (k - 1) -> 32, conv5: 192 -> 64, LeakyReLU(0.2)
    RRDB(x)   0.2 * RDB3(RDB2(RDB1(x))) + x
    net(img)  f = conv_first(img); f = f + conv_body(body(f)); f = lrelu(conv_up1(up2(f))); f = lrelu(conv_up2(up2(f))); conv_last(lrelu(conv_hr(f)))
              up2 = nearest-neighbour x2; img and the result in [0, 1]

Parameter names are basicsr's (``conv_first``, ``body.N.rdb{1,2,3}.conv{1..5}``, ``conv_body``, ``conv_up1``, ``conv_up2``, ``conv_hr``, ``conv_last``), so the
published ``.pth`` files load.  ``num_feat`` 64, ``num_grow_ch`` 32 and scale 4 are fixed; ``num_block`` is 23 for ``x4plus`` and 6 for the anime model.

The plan: ``conv_first`` and ``conv_last`` are ``pv_tiny_conv3x3`` launches (image in with ``(x + 1) / 2``, image out with ``2 y - 1``), every conv between them
is one ``pv_dense_conv3x3`` launch (``csrc/pv_denseconv.hip``).  A dense block is ONE ``[rows][192]`` buffer: conv1 .. conv4 write their 32 channels into its
columns 64-95 ... 160-191 in place - no concatenation exists - and conv5 writes the next block's buffer with ``alpha = 0.2`` and the block's input as the
residual; the third block's conv5 also carries the RRDB's outer residual (``beta = 0.2``, the RRDB's input): two residuals, one rounding.  Three such buffers
rotate (a block's input, the RRDB's input, the block's output) beside the one ``conv_first`` wrote, which ``conv_body``'s residual still needs at the end:
15 ``num_block`` + 6 conv launches and one clamp, whatever the batch.
"""
from __future__ import annotations

import math
import os
import re
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .ops import ACT_LEAKY_RELU, ACT_NONE, Recorder, require_cuda

NUM_FEAT, NUM_GROW, SCALE = 64, 32, 4
DENSE_WIDTH = NUM_FEAT + 4 * NUM_GROW          # 192: the columns of a dense block's buffer
SLOPE, RES_SCALE = 0.2, 0.2
#: bytes of the largest activation operand per INPUT pixel: the 64-channel fp16 rows at 4x the resolution
BYTES_PER_PIXEL = SCALE * SCALE * NUM_FEAT * 2


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise NotImplementedError(f"{type(self).__name__} only holds parameters")


class _RDB(_Holder):
    def __init__(self):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", nn.Conv2d(NUM_FEAT + (k - 1) * NUM_GROW, NUM_GROW, 3, padding=1))
        self.conv5 = nn.Conv2d(DENSE_WIDTH, NUM_FEAT, 3, padding=1)


class _RRDB(_Holder):
    def __init__(self):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _RDB(), _RDB(), _RDB()


def _conv3_w(w):
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.float16).contiguous()


def tile_grid(height: int, width: int, tile: int, tile_pad: int) -> List[Tuple[int, int, int, int, int, int, int, int]]:
    """Real-ESRGAN's ``tile_process`` grid, in input pixels, row-major: per tile ``(y0, y1, x0, x1, py0, py1, px0, px1)`` - the tile ``[y0, y1) x [x0, x1)``
    of a ``tile`` x ``tile`` grid (the last row / column may be smaller) and the region ``[py0, py1) x [px0, px1)`` that is run for it: the tile grown by
    ``tile_pad`` pixels of real neighbourhood where the image has one.  The output keeps the tile's own 4x pixels and drops the padding's; no blending."""
    if height < 1 or width < 1:
        raise ValueError(f"tile_grid: the image must have at least one pixel, got {height} x {width}")
    if tile < 1:
        raise ValueError(f"tile_grid: tile must be >= 1, got {tile}")
    if tile_pad < 0:
        raise ValueError(f"tile_grid: tile_pad must be >= 0, got {tile_pad}")
    cells = []
    for ty in range(math.ceil(height / tile)):
        for tx in range(math.ceil(width / tile)):
            y0, x0 = ty * tile, tx * tile
            y1, x1 = min(y0 + tile, height), min(x0 + tile, width)
            cells.append((y0, y1, x0, x1, max(y0 - tile_pad, 0), min(y1 + tile_pad, height), max(x0 - tile_pad, 0), min(x1 + tile_pad, width)))
    return cells


def default_tile(height: int, width: int, tile_pad: int, max_operand_bytes: int) -> Optional[int]:
    """``tile=None`` of ``RRDBNet.upscale``: None - the whole image in one piece - when its largest operand (``BYTES_PER_PIXEL`` per input pixel) stays within
    ``max_operand_bytes``, else the largest tile size whose padded tile does."""
    if BYTES_PER_PIXEL * height * width <= max_operand_bytes:
        return None
    side = math.isqrt(max_operand_bytes // BYTES_PER_PIXEL) - 2 * tile_pad
    if side < 1:
        raise ValueError(f"RRDBNet: no tile fits {max_operand_bytes} bytes per operand with tile_pad {tile_pad}")
    return side


class RRDBNet(nn.Module):
    """``upscale(images)``: fp32 (B, 3, H, W) in [-1, 1] - what ``run_inference`` returns - -> fp32 (B, 3, 4H, 4W) in [-1, 1], clamped.  Any extents >= 1."""

    MAX_OPERAND_BYTES = 1 << 30     # as AutoencoderTiny: every activation operand well under the 2 GiB the launchers accept

    def __init__(self, num_block: int = 23):
        super().__init__()
        if int(num_block) < 1:
            raise ValueError(f"RRDBNet: num_block must be >= 1, got {num_block!r}")
        self.num_block = int(num_block)
        self.conv_first = nn.Conv2d(3, NUM_FEAT, 3, padding=1)
        self.body = nn.ModuleList([_RRDB() for _ in range(self.num_block)])
        for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
            setattr(self, name, nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, padding=1))
        self.conv_last = nn.Conv2d(NUM_FEAT, 3, 3, padding=1)
        self._plans: Dict[tuple, object] = {}
        self._packed: Dict[int, tuple] = {}

    # ---- constructors / state, as the other models ----
    @classmethod
    def from_pretrained(cls, path: str) -> "RRDBNet":
        """A Real-ESRGAN ``.pth`` (a dict with ``params_ema`` or ``params``, or a bare state dict; read with ``weights_only=True``) or a ``.safetensors`` of the
        same names.  ``num_block`` comes from the keys; strict: every parameter must come from the file and the file holds nothing else."""
        if not os.path.exists(path):
            raise FileNotFoundError(f"RRDBNet: no weights at {path}")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
            for key in ("params_ema", "params"):
                if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
                    sd = sd[key]
                    break
        blocks = {int(m.group(1)) for m in (re.match(r"body\.(\d+)\.", k) for k in sd) if m}
        if not blocks or "conv_first.weight" not in sd:
            raise KeyError(f"RRDBNet: {path} holds no basicsr RRDBNet state dict (no conv_first / body.N keys; first keys: {list(sd)[:4]})")
        if tuple(sd["conv_first.weight"].shape) != (NUM_FEAT, 3, 3, 3):
            raise ValueError(f"RRDBNet: conv_first.weight is {tuple(sd['conv_first.weight'].shape)}, not {(NUM_FEAT, 3, 3, 3)}: only the x4 model with "
                             f"num_feat {NUM_FEAT} is built (the x2 model feeds conv_first 12 pixel-unshuffled channels)")
        m = cls(num_block=max(blocks) + 1)
        m.load_state_dict(sd, strict=True)
        return m

    def randomize_(self, seed: int = 0) -> "RRDBNet":
        """Seeded weights (``--upscaler_path random``): every conv uniform in +- 1 / sqrt(fan_in), torch's own default, drawn on the CPU from ``seed``."""
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for mod in self.modules():
                if isinstance(mod, nn.Conv2d):
                    bound = (mod.weight.shape[1] * 9) ** -0.5
                    mod.weight.copy_((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * bound)
                    mod.bias.copy_((torch.rand(mod.bias.shape, generator=g) * 2 - 1) * bound)
        self.repack()
        return self

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
        return self.conv_first.weight.device

    # ---- plans ----
    def _wb(self, conv: nn.Conv2d):
        """(tap-major fp16 weight, fp32 bias) of one conv, packed once per ``repack``."""
        key = id(conv)
        if key not in self._packed:
            self._packed[key] = (_conv3_w(conv.weight), conv.bias.detach().to(torch.float32).contiguous())
        return self._packed[key]

    def _sub_batch(self, batch, h, w):
        return max(1, min(batch, self.MAX_OPERAND_BYTES // (BYTES_PER_PIXEL * h * w)))

    def _plan(self, sb, h, w, dev):
        rec = Recorder(dev)
        rows = sb * h * w
        geo = dict(batch=sb, h=h, wd=w)
        x_in = rec.empty((sb, 3, h, w), torch.float32)
        first = rec.empty((rows, DENSE_WIDTH))                    # conv_first's output in its columns 0-63: kept for conv_body's residual
        pool = [rec.empty((rows, DENSE_WIDTH)) for _ in range(3)]
        rec.tiny_conv(x_in, *self._wb(self.conv_first), pre="unit", out=first[:, :NUM_FEAT], **geo)
        cur = first
        for rrdb in self.body:
            x0 = cur
            for j, rdb in enumerate((rrdb.rdb1, rrdb.rdb2, rrdb.rdb3)):
                for k in range(1, 5):
                    cin = NUM_FEAT + (k - 1) * NUM_GROW
                    rec.dense_conv(cur, *self._wb(getattr(rdb, f"conv{k}")), cin=cin, act=ACT_LEAKY_RELU, slope=SLOPE, out=cur[:, cin:cin + NUM_GROW], **geo)
                nxt = next(t for t in pool if t is not cur and t is not x0)
                outer = dict(residual2=x0[:, :NUM_FEAT], beta=RES_SCALE) if j == 2 else {}
                rec.dense_conv(cur, *self._wb(rdb.conv5), cin=DENSE_WIDTH, act=ACT_NONE, residual=cur[:, :NUM_FEAT], alpha=RES_SCALE, out=nxt[:, :NUM_FEAT],
                               **outer, **geo)
                cur = nxt
        feat = next(t for t in pool if t is not cur)[:, :NUM_FEAT]
        rec.dense_conv(cur, *self._wb(self.conv_body), cin=NUM_FEAT, residual=first[:, :NUM_FEAT], alpha=1.0, out=feat, **geo)
        up1 = rec.dense_conv(feat, *self._wb(self.conv_up1), upsample=True, act=ACT_LEAKY_RELU, slope=SLOPE, **geo)
        up2 = rec.dense_conv(up1, *self._wb(self.conv_up2), upsample=True, act=ACT_LEAKY_RELU, slope=SLOPE, batch=sb, h=2 * h, wd=2 * w)
        hr = rec.dense_conv(up2, *self._wb(self.conv_hr), act=ACT_LEAKY_RELU, slope=SLOPE, batch=sb, h=4 * h, wd=4 * w)
        wl, bl = self._wb(self.conv_last)
        img = rec.tiny_conv(hr, wl, bl, batch=sb, h=4 * h, wd=4 * w, image_out=True, out_scale=2.0, out_shift=-1.0)
        rec.clamp_(img, -1.0, 1.0)
        return SimpleNamespace(rec=rec, x=x_in, img=img, buffers=[first] + pool)

    def _run(self, t: torch.Tensor) -> torch.Tensor:
        B, _, h, w = t.shape
        sb = self._sub_batch(B, h, w)
        key = (sb, h, w, t.device)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._plan(sb, h, w, t.device)
        outs = []
        for i in range(0, B, sb):
            chunk = t[i:i + sb]
            n = chunk.shape[0]
            plan.x[:n].copy_(chunk)
            plan.rec.run()
            outs.append(plan.img[:n].clone())
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    @torch.no_grad()
    def upscale(self, images: torch.Tensor, tile: Optional[int] = None, tile_pad: int = 10) -> torch.Tensor:
        """``tile``: Real-ESRGAN's ``tile_process`` - the image is cut into a grid of ``tile`` x ``tile`` input tiles, each is run with ``tile_pad`` pixels of
        real neighbourhood where it exists, and the padding is cropped from the output (no blending).  None: the whole image when every operand stays under
        ``MAX_OPERAND_BYTES``, else the largest tile size that does.  The batch is cut into sub-batches by the same limit."""
        require_cuda(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or min(images.shape) < 1:
            raise ValueError(f"RRDBNet.upscale: images must be (B, 3, H, W) with B, H, W >= 1, got {tuple(images.shape)}")
        if self.device != images.device:
            raise RuntimeError(f"RRDBNet: the weights live on {self.device}, the input on {images.device}: call .to('cuda') (there is no CPU path)")
        B, _, H, W = images.shape
        x = images.to(torch.float32)
        if tile is None:
            tile = default_tile(H, W, int(tile_pad), self.MAX_OPERAND_BYTES)
            if tile is None:
                return self._run(x.contiguous())
        cells = tile_grid(H, W, int(tile), int(tile_pad))
        if any(BYTES_PER_PIXEL * (c[5] - c[4]) * (c[7] - c[6]) > self.MAX_OPERAND_BYTES for c in cells):
            raise ValueError(f"RRDBNet.upscale: a padded tile of tile={tile}, tile_pad={tile_pad} exceeds {self.MAX_OPERAND_BYTES} bytes per operand")
        out = torch.empty((B, 3, SCALE * H, SCALE * W), dtype=torch.float32, device=x.device)
        for y0, y1, x0, x1, py0, py1, px0, px1 in cells:
            o = self._run(x[:, :, py0:py1, px0:px1].contiguous())
            oy, ox = SCALE * (y0 - py0), SCALE * (x0 - px0)
            out[:, :, SCALE * y0:SCALE * y1, SCALE * x0:SCALE * x1] = o[:, :, oy:oy + SCALE * (y1 - y0), ox:ox + SCALE * (x1 - x0)]
        return out
