"""The references of the upscaler tests, plain torch on the CPU (no photoverse_amd import):

* ``RRDBNetRef`` - Real-ESRGAN's RRDBNet as ``torch.nn`` modules with basicsr's key names (``conv_first``, ``body.N.rdb{1,2,3}.conv{1..5}``, ``conv_body``,
  ``conv_up1``, ``conv_up2``, ``conv_hr``, ``conv_last``), with ``torch.cat`` dense blocks, run in fp32; ``emulate_fp16=True`` runs the same modules with
  fp16-rounded weights and every LAUNCH's output rounded to fp16 exactly where the HIP plan rounds - the two-residual conv5 of an RRDB's third block once;
* ``dense_conv_ref`` - the fp64 contract of ONE ``pv_dense_conv3x3`` launch, with the per-element sum of |terms|;
* ``tile_process_ref`` - Real-ESRGAN's ``tile_process`` around any ``fn(tile) -> 4x tile``;
* the seeded weights, operands and inputs of ``tests/test_upscaler_gpu.py``, so that ``tests/test_upscaler_cpu.py`` can check them against the bounds before
  the kernel ever sees them.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

KERNEL_BOUND = 1e-3              # rel-L2 of an fp16 output against fp64: the tree's kernel bound, 2 x 2^-11
TOL = 5e-3                       # the suite's standing VAE tolerance (tests/test_vae_gpu.py)
IMAGE_ULPS = 32 * 2.0 ** -24     # fp32 arithmetic before the one rounding: |got - exact| <= half an fp16 ulp of exact + IMAGE_ULPS * sum |terms| per element
NUM_FEAT, NUM_GROW, SCALE = 64, 32, 4
SLOPE = 0.2

#: (num_block, input shape) of the model tests
MODEL_BLOCKS = (2, 23)
MODEL_CASES = [(1, 3, 12, 20), (2, 3, 5, 7), (1, 3, 1, 1)]
#: the tiled run: 12 x 20 pixels in 8 x 8 tiles with 1 pixel of padding - six tiles of six different padded shapes.  The network's receptive field is far
#: wider than 1 pixel, so the tiled result is NOT the untiled one: the CPU suite checks that they differ by more than 10 x TOL, which is what makes the GPU
#: comparison against ``tile_process_ref`` a test of the tiling and not of the network
TILE_CASE = dict(shape=(1, 3, 12, 20), tile=8, tile_pad=1)
#: (batch, h, w) of the kernel tests
KERNEL_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 9, 17)]
#: the smallest output shape that spans two 16 x 32 pixel tiles in BOTH directions (17 x 33) and two persistent iterations: 65 images x 4 tiles = 260 tiles
#: for the 256 workgroups, so the first four take a second tile - with cin = 192 the prefetch of that tile's first K slice runs under the previous tile's
#: last one.  With ``upsample`` the OUTPUT is 18 x 34 - the same four tiles - from a 9 x 17 input.
WALK_SHAPE = (65, 17, 33)
WALK_SHAPE_UPSAMPLE = (65, 9, 17)
WALK_FORMS = ("dense192", "body_res", "upsample")
#: name -> dict(cin, cout, bias, act, res, res2, alpha, beta, upsample, inplace)
KERNEL_FORMS = {
    "dense64": dict(cin=64, cout=32, act="leaky", inplace=True),
    "dense96": dict(cin=96, cout=32, act="leaky", inplace=True),
    "dense128": dict(cin=128, cout=32, act="leaky", inplace=True),
    "dense160": dict(cin=160, cout=32, act="leaky", inplace=True),
    "dense192": dict(cin=192, cout=32, act="leaky", inplace=True),          # not a launch of the model (its buffer is 192 wide): the widest K at CF = 2
    "conv5_res": dict(cin=192, cout=64, res=True, alpha=0.2),
    "conv5_res2": dict(cin=192, cout=64, res=True, alpha=0.2, res2=True, beta=0.2),
    "upsample": dict(cin=64, cout=64, act="leaky", upsample=True),
    "body_res": dict(cin=64, cout=64, res=True, alpha=1.0),
    "nobias": dict(cin=128, cout=32, act="leaky", bias=False, inplace=True),
}


def rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def _h(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------------- the model
class RDBRef(nn.Module):
    def __init__(self):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", nn.Conv2d(NUM_FEAT + (k - 1) * NUM_GROW, NUM_GROW, 3, padding=1))
        self.conv5 = nn.Conv2d(NUM_FEAT + 4 * NUM_GROW, NUM_FEAT, 3, padding=1)

    def forward(self, x):
        x1 = F.leaky_relu(self.conv1(x), SLOPE)
        x2 = F.leaky_relu(self.conv2(torch.cat((x, x1), 1)), SLOPE)
        x3 = F.leaky_relu(self.conv3(torch.cat((x, x1, x2), 1)), SLOPE)
        x4 = F.leaky_relu(self.conv4(torch.cat((x, x1, x2, x3), 1)), SLOPE)
        return self.conv5(torch.cat((x, x1, x2, x3, x4), 1)) * 0.2 + x


class RRDBRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = RDBRef(), RDBRef(), RDBRef()

    def forward(self, x):
        return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x


class RRDBNetRef(nn.Module):
    """basicsr's ``RRDBNet(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_grow_ch=32)``; ``forward`` on [0, 1] images as there, ``upscale`` on the
    [-1, 1] images of this project: ``clamp(2 forward((x + 1) / 2) - 1, -1, 1)``."""

    def __init__(self, num_block=23):
        super().__init__()
        self.conv_first = nn.Conv2d(3, NUM_FEAT, 3, padding=1)
        self.body = nn.Sequential(*[RRDBRef() for _ in range(num_block)])
        self.conv_body = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, padding=1)
        self.conv_up1 = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, padding=1)
        self.conv_up2 = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, padding=1)
        self.conv_hr = nn.Conv2d(NUM_FEAT, NUM_FEAT, 3, padding=1)
        self.conv_last = nn.Conv2d(NUM_FEAT, 3, 3, padding=1)

    def forward(self, x):
        feat = self.conv_first(x)
        feat = feat + self.conv_body(self.body(feat))
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")), SLOPE)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")), SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), SLOPE))

    @torch.no_grad()
    def upscale(self, x, emulate_fp16=False):
        y = self._emulated((x + 1) / 2) if emulate_fp16 else self.forward((x + 1) / 2)
        return (y * 2 - 1).clamp(-1, 1)

    def _emulated(self, x):
        """``forward`` with fp16-rounded weights and one fp16 rounding per launch of the HIP plan: conv + LeakyReLU; conv5 + scaled residual; the third
        block's conv5 + both scaled residuals (ONE rounding); conv_body + residual; upsample + conv + LeakyReLU.  conv_last's fp32 image is not rounded."""
        conv = lambda m, t: F.conv2d(t, _h(m.weight), m.bias, padding=1)
        lrelu = lambda t: F.leaky_relu(t, SLOPE)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        first = _h(conv(self.conv_first, x))
        feat, self.max_activation = first, 0.0
        for rrdb in self.body:
            x0 = feat
            for j, rdb in enumerate((rrdb.rdb1, rrdb.rdb2, rrdb.rdb3)):
                cat = feat
                for k in range(1, 5):
                    cat = torch.cat((cat, _h(lrelu(conv(getattr(rdb, f"conv{k}"), cat)))), 1)
                y = 0.2 * conv(rdb.conv5, cat) + feat
                feat = _h(0.2 * y + x0) if j == 2 else _h(y)
                self.max_activation = max(self.max_activation, float(cat.abs().max()), float(feat.abs().max()))
        feat = _h(conv(self.conv_body, feat) + first)
        feat = _h(lrelu(conv(self.conv_up1, up(feat))))
        feat = _h(lrelu(conv(self.conv_up2, up(feat))))
        feat = _h(lrelu(conv(self.conv_hr, feat)))
        self.max_activation = max(self.max_activation, float(feat.abs().max()))
        return conv(self.conv_last, feat)


_REFS = {}


def seeded_ref(num_block, seed=0):
    """torch's default conv init (uniform in +- 1 / sqrt(fan_in), weights and biases) from a seeded stream, then ``conv_last`` rescaled - it is linear - so
    that the [0, 1] output of a fixed probe image has mean 0.5 and standard deviation 0.15: with the default init alone the output sits at 0.03 +- 0.02,
    ``upscale`` clamps most of it to -1, and a relative error against that constant would measure nothing.  One module per (num_block, seed), shared by the
    tests and never changed by them."""
    key = (num_block, seed)
    if key not in _REFS:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(1000 + 10 * seed + num_block)
            ref = RRDBNetRef(num_block).eval().requires_grad_(False)
        y = ref.forward(torch.rand(1, 3, 8, 8, generator=torch.Generator().manual_seed(5)))
        s = 0.15 / y.std()
        ref.conv_last.bias.copy_(ref.conv_last.bias * s + 0.5 - s * y.mean())
        ref.conv_last.weight.mul_(s)
        _REFS[key] = ref
    return _REFS[key]


def pixels_case(shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape) * 13 + shape[0])) * 2 - 1


def tile_process_ref(fn, img, tile, tile_pad, scale=SCALE):
    """Real-ESRGAN's ``RealESRGANer.tile_process`` around ``fn``: a grid of ``tile`` x ``tile`` input tiles, each run with ``tile_pad`` pixels of real
    neighbourhood where the image has one; the padding is cropped from the output, no blending."""
    B, C, H, W = img.shape
    out = img.new_zeros((B, C, H * scale, W * scale))
    for y in range(math.ceil(H / tile)):
        for x in range(math.ceil(W / tile)):
            x0, y0 = x * tile, y * tile
            x1, y1 = min(x0 + tile, W), min(y0 + tile, H)
            px0, px1, py0, py1 = max(x0 - tile_pad, 0), min(x1 + tile_pad, W), max(y0 - tile_pad, 0), min(y1 + tile_pad, H)
            o = fn(img[:, :, py0:py1, px0:px1])
            ox0, oy0 = (x0 - px0) * scale, (y0 - py0) * scale
            out[:, :, y0 * scale:y1 * scale, x0 * scale:x1 * scale] = o[:, :, oy0:oy0 + (y1 - y0) * scale, ox0:ox0 + (x1 - x0) * scale]
    return out


# ---------------------------------------------------------------------------------------------------------------- one launch
_CASES = {}


def kernel_case(form, batch, h, w, seed=0):
    """The operands of one kernel test, built once per (form, shape, seed) and shared: dict(x, w, b, r, r2, **form fields); x, r, r2 NCHW with fp16-representable
    values, r / r2 at the output's resolution."""
    key = (form, batch, h, w, seed)
    if key in _CASES:
        return _CASES[key]
    f = dict(cin=64, cout=64, bias=True, act=None, res=False, res2=False, alpha=1.0, beta=1.0, upsample=False, inplace=False)
    f.update(KERNEL_FORMS[form])
    g = torch.Generator().manual_seed(1000 * seed + 100 * batch + 10 * h + w + 7 * len(form) + f["cin"])
    K = 9 * f["cin"]
    x = _h(torch.randn(batch, f["cin"], h, w, generator=g))
    wt = _h(torch.randn(f["cout"], K, generator=g) * K ** -0.5)                        # [cout][9 cin], tap-major
    ho, wo = (2 * h, 2 * w) if f["upsample"] else (h, w)
    bias = torch.randn(f["cout"], generator=g) * 0.5 if f["bias"] else None
    res = _h(torch.randn(batch, f["cout"], ho, wo, generator=g)) if f["res"] else None
    res2 = _h(torch.randn(batch, f["cout"], ho, wo, generator=g)) if f["res2"] else None
    _CASES[key] = dict(f, form=form, x=x, w=wt, b=bias, r=res, r2=res2, ho=ho, wo=wo, batch=batch, h=h, wd=w)
    return _CASES[key]


_EXACT = {}


def dense_conv_ref(c):
    """fp64 contract of one ``pv_dense_conv3x3`` launch on the operands of ``kernel_case`` -> (out NCHW fp64, sum |terms| NCHW fp64); computed once per case."""
    key = id(c)
    if key in _EXACT:
        return _EXACT[key][1:]
    x = c["x"].double()
    if c["upsample"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    cin, cout = c["cin"], c["cout"]
    w4 = c["w"].double().view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()           # tap-major [co][ky][kx][ci] -> [co][ci][ky][kx]
    y = F.conv2d(x, w4, None, padding=1)                                                # zero padding AFTER the upsample
    mag = F.conv2d(x.abs(), w4.abs(), None, padding=1)
    if c["b"] is not None:
        y = y + c["b"].double().view(1, -1, 1, 1)
        mag = mag + c["b"].double().abs().view(1, -1, 1, 1)
    if c["act"] == "leaky":
        y = torch.where(y > 0, y, SLOPE * y)                                            # |act(y)| <= |y|: mag stands
    if c["r"] is not None:
        y = c["alpha"] * y + c["r"].double()
        mag = abs(c["alpha"]) * mag + c["r"].double().abs()
    if c["r2"] is not None:
        y = c["beta"] * y + c["r2"].double()
        mag = abs(c["beta"]) * mag + c["r2"].double().abs()
    _EXACT[key] = (c, y, mag)                                                           # holds c: its id stays its own
    return y, mag


def half_ulp_fp16(v):
    """Half the spacing of fp16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 11), 2^-25 in the subnormal range."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))) - 11)


def element_bound(exact, mag):
    return half_ulp_fp16(exact) + IMAGE_ULPS * mag


def to_rows(t):
    """NCHW -> [batch * h * w][c]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def from_rows(t, batch, h, w):
    return t.reshape(batch, h, w, -1).permute(0, 3, 1, 2).contiguous()
