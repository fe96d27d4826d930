"""The references of the AutoencoderTiny tests, plain torch on the CPU (no photoverse_amd import):

* ``AutoencoderTinyRef`` - ``torch.nn`` modules built from the definition in DESIGN.md section 5 with diffusers' key names (``decoder.layers.N``,
  ``encoder.layers.N``, blocks ``.conv.{0,2,4}``), run in fp32; ``emulate_fp16=True`` runs the same modules with fp16-rounded weights and every launch's
  output rounded to fp16 - what the HIP plan does, minus the summation order;
* ``conv_ref`` - the fp64 contract of ONE ``pv_tiny_conv3x3`` launch, with the per-element sum of |terms| for the fp32 image bound;
* the seeded weights, operands and inputs of ``tests/test_vae_tiny_gpu.py``, so that ``tests/test_vae_tiny_cpu.py`` can check them against the bounds before
  the kernel ever sees them.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

KERNEL_BOUND = 1e-3              # rel-L2 of an fp16 output against fp64: the tree's kernel bound, 2 x 2^-11
TOL = 5e-3                       # the suite's standing VAE tolerance (tests/test_vae_gpu.py)
IMAGE_ULPS = 32 * 2.0 ** -24     # fp32 image output: |got - exact| <= IMAGE_ULPS * sum |terms| per element
WIDTH = 64

DECODE_CASES = [(1, 4, 1, 1), (2, 4, 5, 7), (1, 4, 8, 8), (3, 4, 16, 16)]      # (1, 4, 8, 8) is 4 * randn: TANH3 in its curved range
ENCODE_CASES = [(1, 3, 8, 8), (1, 3, 13, 21), (2, 3, 40, 56)]
#: (batch, h, w) of the kernel tests
KERNEL_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 8, 8), (1, 9, 17), (3, 16, 16)]
#: the smallest shape that spans two pixel tiles in BOTH directions (16 x 32 tiles: 17 x 33) and two persistent iterations (256 workgroups walk
#: 65 images x 4 tiles = 260 tiles: the first four workgroups take a second tile)
WALK_SHAPE = (65, 17, 33)
#: name -> dict(x_image, cin, pre, out_image, cout, bias, res, act, stride, upsample, scale, shift)
KERNEL_FORMS = {
    "plain": dict(),
    "bias_relu": dict(bias=True, act="relu"),
    "bias_res_relu": dict(bias=True, res=True, act="relu"),
    "stride2": dict(stride=2),
    "upsample": dict(upsample=True),
    "image3_unit_in": dict(x_image=True, cin=3, pre="unit", bias=True),
    "image4_tanh3_in": dict(x_image=True, cin=4, pre="tanh3", bias=True, act="relu"),
    "image3_out": dict(out_image=True, cout=3, bias=True, scale=2.0, shift=-1.0),
    "image4_out": dict(out_image=True, cout=4, bias=True, scale=1.0, shift=0.0),
}


def rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


class BlockRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(WIDTH, WIDTH, 3, padding=1), nn.ReLU(), nn.Conv2d(WIDTH, WIDTH, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(WIDTH, WIDTH, 3, padding=1))

    def forward(self, x):
        return F.relu(self.conv(x) + x)


class DecoderRef(nn.Module):
    def __init__(self, latent=4, out_channels=3, blocks=(3, 3, 3, 1)):
        super().__init__()
        layers = [nn.Conv2d(latent, WIDTH, 3, padding=1), nn.ReLU()]
        for i, nb in enumerate(blocks):
            last = i == len(blocks) - 1
            layers += [BlockRef() for _ in range(nb)]
            if not last:
                layers.append(nn.Upsample(scale_factor=2))
            layers.append(nn.Conv2d(WIDTH, out_channels if last else WIDTH, 3, padding=1, bias=last))
        self.layers = nn.Sequential(*layers)

    def forward(self, z):
        return self.layers(torch.tanh(z / 3) * 3) * 2 - 1


class EncoderRef(nn.Module):
    def __init__(self, in_channels=3, latent=4, blocks=(1, 3, 3, 3)):
        super().__init__()
        layers = []
        for i, nb in enumerate(blocks):
            layers.append(nn.Conv2d(in_channels, WIDTH, 3, padding=1) if i == 0 else nn.Conv2d(WIDTH, WIDTH, 3, padding=1, stride=2, bias=False))
            layers += [BlockRef() for _ in range(nb)]
        layers.append(nn.Conv2d(WIDTH, latent, 3, padding=1))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers((x + 1) / 2)


def _h(t):
    return t.half().float()


class AutoencoderTinyRef(nn.Module):
    def __init__(self, num_encoder_blocks=(1, 3, 3, 3), num_decoder_blocks=(3, 3, 3, 1)):
        super().__init__()
        self.encoder = EncoderRef(blocks=num_encoder_blocks)
        self.decoder = DecoderRef(blocks=num_decoder_blocks)

    @torch.no_grad()
    def decode(self, z, emulate_fp16=False):
        return self._walk(self.decoder.layers, torch.tanh(z / 3) * 3, emulate_fp16, 2.0, -1.0)

    @torch.no_grad()
    def encode(self, x, emulate_fp16=False):
        return self._walk(self.encoder.layers, (x + 1) / 2, emulate_fp16, 1.0, 0.0)

    def _walk(self, layers, x, emu, scale, shift):
        """``layers(x) * scale + shift``; with ``emu`` the convs use fp16-rounded weights and the output of every LAUNCH of the HIP plan is rounded to fp16:
        conv + ReLU, conv + residual + ReLU, upsample + conv are one launch each; the last conv's fp32 image output is not rounded."""
        if not emu:
            return layers(x) * scale + shift
        conv = lambda m, t, **k: F.conv2d(t, _h(m.weight), m.bias, stride=m.stride, padding=1)
        mods, self.max_activation = list(layers), 0.0
        for i, m in enumerate(mods):
            if isinstance(m, BlockRef):
                t = _h(F.relu(conv(m.conv[0], x)))
                t = _h(F.relu(conv(m.conv[2], t)))
                x = _h(F.relu(conv(m.conv[4], t) + x))
            elif isinstance(m, nn.Upsample):
                x = m(x)
            elif isinstance(m, nn.ReLU):
                x = _h(F.relu(x))
            elif i == len(mods) - 1:
                return conv(m, x) * scale + shift
            else:
                x = conv(m, x)
                if not (i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)):
                    x = _h(x)
            self.max_activation = max(self.max_activation, float(x.abs().max()))
        raise AssertionError("the last layer is a conv")


def seeded_ref(seed=0, **kw):
    """Conv weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.1^2): the activations stay O(1) through the residual blocks (variance 2 / fan_in lets them grow to
    hundreds)."""
    g = torch.Generator().manual_seed(seed)
    ref = AutoencoderTinyRef(**kw).eval()
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * 9
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * fan_in ** -0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return ref


def latents_case(shape):
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape) * 7 + shape[0]))
    return 4 * z if tuple(shape) == (1, 4, 8, 8) else z


def pixels_case(shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(sum(shape) * 11 + shape[0])) * 2 - 1


# ---------------------------------------------------------------------------------------------------------------- one launch
def kernel_case(form, batch, h, w, seed=0):
    """The operands of one kernel test: dict(x, w, bias, res, **form fields); x fp32 NCHW (image input) or fp16-representable NCHW values (rows input)."""
    f = dict(x_image=False, cin=WIDTH, pre=None, out_image=False, cout=WIDTH, bias=False, res=False, act=None, stride=1, upsample=False, scale=1.0,
             shift=0.0)
    f.update(KERNEL_FORMS[form])
    g = torch.Generator().manual_seed(1000 * seed + 100 * batch + 10 * h + w + len(form))
    K = 9 * f["cin"]
    x = torch.randn(batch, f["cin"], h, w, generator=g)
    if not f["x_image"]:
        x = _h(x)
    wt = _h(torch.randn(f["cout"], K, generator=g) * K ** -0.5)                       # [cout][9 cin], tap-major
    hv, wv = (2 * h, 2 * w) if f["upsample"] else (h, w)
    ho, wo = (hv - 1) // f["stride"] + 1, (wv - 1) // f["stride"] + 1
    bias = torch.randn(f["cout"], generator=g) * 0.5 if f["bias"] else None
    res = _h(torch.randn(batch, f["cout"], ho, wo, generator=g)) if f["res"] else None
    return dict(f, x=x, w=wt, b=bias, r=res, ho=ho, wo=wo, batch=batch, h=h, wd=w)


def conv_ref(c, round_out=False):
    """fp64 contract of one launch on the operands of ``kernel_case`` -> (out NCHW fp64, sum |terms| NCHW fp64).  ``round_out``: the rows output rounded to
    fp16 once, after residual and activation, as the kernel does."""
    x = c["x"].double()
    if c["pre"] == "tanh3":
        x = 3 * torch.tanh(x / 3)
    elif c["pre"] == "unit":
        x = (x + 1) / 2
    if c["upsample"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    cin, cout = c["cin"], c["cout"]
    w4 = c["w"].double().view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()           # tap-major [co][ky][kx][ci] -> [co][ci][ky][kx]
    y = F.conv2d(x, w4, None, stride=c["stride"], padding=1)                            # zero padding AFTER pre / upsample
    mag = F.conv2d(x.abs(), w4.abs(), None, stride=c["stride"], padding=1)
    if c["b"] is not None:
        y = y + c["b"].double().view(1, -1, 1, 1)
        mag = mag + c["b"].double().abs().view(1, -1, 1, 1)
    if c["r"] is not None:
        y = y + c["r"].double()
    if c["act"] == "relu":
        y = F.relu(y)
    if c["out_image"]:
        return y * c["scale"] + c["shift"], mag * abs(c["scale"]) + abs(c["shift"])
    return (y.half().double() if round_out else y), mag


def to_rows(t):
    """NCHW -> [batch * h * w][c]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def from_rows(t, batch, h, w):
    return t.view(batch, h, w, -1).permute(0, 3, 1, 2).contiguous()
