"""CPU-only tests of FreeU (``freeu=(b1, b2, s1, s2)``): the fp64 references of ``tests/test_freeu_gpu.py`` - ``fourier_filter_ref`` (diffusers' fftn /
fftshift / 2 x 2 window / ifftn().real sequence) against the closed form the header of ``pv_freeu_rows`` states, and ``freeu_oracle`` (the fp32 oracle
UNet with both FreeU steps in front of the concat of its first two up blocks) -, the new symbol in the header, ``_lib.SIGNATURES`` and the built
library with its C-ABI rejections, the keyword validation of ``run_inference`` / ``DenoiseLoop``, the CLI flag, and - on the oracle alone - that each of
the four numbers moves the result by far more than the GPU tests' tolerances."""
import copy
import inspect
import math
import os
import re
import types

import pytest
import torch

from test_guidance_cpu import _Untouchable
from test_pag_cpu import B, G_TEXT, P, S, TOL_FWD, TOL_LOOP, loop_inputs_81, oracle_loop, rel_l2, tiny_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the FreeU authors' values for SD-1.5, and one setting per number on its own (s1 = 0.9 alone moves the tiny oracle by only 1.7e-2, hence 0.5)
FREEU = (1.5, 1.6, 0.9, 0.2)
SETTINGS = (FREEU, (1.5, 1, 1, 1), (1, 1.6, 1, 1), (1, 1, 0.5, 1), (1, 1, 1, 0.2))
MATH_SHAPES = ((2, 3, 8, 8), (1, 5, 2, 2), (2, 4, 5, 7), (1, 2, 3, 2), (2, 2, 6, 10), (1, 1, 12, 12), (1, 2, 2, 9), (1, 2, 16, 16))


# ---------------------------------------------------------------------------------------------------------------- references
def fourier_filter_ref(x, threshold=1, scale=1.0):
    """[EXT] diffusers ``fourier_filter`` on (B, C, H, W), in the dtype's complex companion (pass fp64 for the reference): fftn over (H, W), fftshift, the
    window ``[H//2 - threshold : H//2 + threshold, W//2 - threshold : W//2 + threshold]`` times ``scale``, ifftshift, ifftn, ``.real``."""
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    H, W = x.shape[-2:]
    mask = torch.ones(x.shape, dtype=x.dtype)
    mask[..., H // 2 - threshold:H // 2 + threshold, W // 2 - threshold:W // 2 + threshold] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def closed_form_ref(x, scale):
    """The header's formula in fp64: ``p + (s - 1)/(H W) sum_{(u, v) in {0, -1}^2} Re(X[u, v] exp(+2 pi i (u y/H + v x/W)))``,
    ``X[u, v] = sum p exp(-2 pi i (u y/H + v x/W))``."""
    x = x.double()
    H, W = x.shape[-2:]
    yy = torch.arange(H, dtype=torch.float64).view(H, 1) / H
    xx = torch.arange(W, dtype=torch.float64).view(1, W) / W
    upd = torch.zeros_like(x)
    for u in (0, -1):
        for v in (0, -1):
            ph = 2 * math.pi * (u * yy + v * xx)
            X = (x * torch.complex(torch.cos(ph), -torch.sin(ph))).sum(dim=(-2, -1), keepdim=True)
            upd = upd + (X * torch.complex(torch.cos(ph), torch.sin(ph))).real
    return x + (scale - 1.0) / (H * W) * upd


def freeu_oracle(ref, b1, b2, s1, s2):
    """A deep copy of the fp32 oracle UNet whose ``up_blocks[0]`` / ``up_blocks[1]`` apply FreeU before every ``torch.cat``, as diffusers' ``apply_freeu``
    does for ``resolution_idx`` 0 / 1: the first half of the backbone's channels times ``b``, ``fourier_filter_ref(skip, 1, s)``."""
    model = copy.deepcopy(ref)

    def make_forward(b, s):
        def forward(self, x, skips, temb, ehs):
            for i, res in enumerate(self.resnets):
                half = x.shape[1] // 2
                x = torch.cat([x[:, :half] * b, x[:, half:]], dim=1)
                x = torch.cat([x, fourier_filter_ref(skips[-1], 1, s)], dim=1)
                skips = skips[:-1]
                x = res(x, temb)
                if self.has_attn:
                    x = self.attentions[i](x, encoder_hidden_states=ehs)
            if self.upsamplers is not None:
                x = self.upsamplers[0](x)
            return x
        return forward

    for blk, b, s in ((model.up_blocks[0], b1, s1), (model.up_blocks[1], b2, s2)):
        blk.forward = types.MethodType(make_forward(float(b), float(s)), blk)
    return model


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("shape", MATH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fourier_filter_ref_is_the_closed_form_of_the_header(shape):
    """fftn / fftshift / window / ifftn().real == the four-frequency closed form in fp64 to 1e-12, odd sizes and H = 2 (where -1 is the Nyquist
    frequency) included; ``s`` = 1 is the identity to 1e-12.  Measured here: largest difference 1.8e-15."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 2 + torch.randn(shape[:2] + (1, 1), generator=g, dtype=torch.float64)
    for s in (0.9, 0.2, 1.0, 2.0):
        a, c = fourier_filter_ref(x, 1, s), closed_form_ref(x, s)
        d = (a - c).abs().max().item()
        print(f"fourier_filter_ref vs closed form {shape} s = {s}: max |d| = {d:.2e}")
        assert a.dtype == torch.float64 and d <= 1e-12
    assert (fourier_filter_ref(x, 1, 1.0) - x).abs().max().item() <= 1e-12 and (closed_form_ref(x, 1.0) - x).abs().max().item() <= 1e-12
    # a constant plane is its DC term: the result is s times the constant
    const = torch.full(shape, 3.25, dtype=torch.float64)
    assert (fourier_filter_ref(const, 1, 0.2) - 0.2 * const).abs().max().item() <= 1e-12


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int\s+pv_freeu_rows\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.SIGNATURES["pv_freeu_rows"]
    v, i, f = _lib.c_void_p, _lib.c_int, _lib.c_float
    assert res is i and args == [v, i, i, v, i, f, v, i, i, v, i, f, i, i, i, v]
    assert len(decl.split(",")) == len(args) == 16
    comment = header[:header.index("int pv_freeu_rows")].rsplit("/*", 1)[1]
    assert comment.startswith(" (ABI 19") and "Re(X[u,v]" in comment and "(s - 1)/(h w)" in comment and "c < cx/2 ? b : 1" in comment
    assert lib.pv_freeu_rows is not None
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))


def test_cabi_rejects_bad_freeu_blocks_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  No valid call is sent: an absent half is
    legal, so it only appears together with something illegal."""
    INVALID = 1
    X, XO, SK, SO = (0x10000 * (i + 1) for i in range(4))               # never dereferenced

    def call(x=X, ldx=640, cx=640, xo=XO, ldxo=640, b=1.5, sk=SK, lds=320, cs=320, so=SO, ldso=320, s=0.2, batch=2, h=8, w=8):
        return lib.pv_freeu_rows(x, ldx, cx, xo, ldxo, b, sk, lds, cs, so, ldso, s, batch, h, w, None)

    no_x, no_s = dict(x=None, xo=None), dict(sk=None, so=None)
    assert call(**no_x, **no_s) == INVALID                               # both halves absent
    for part in (dict(xo=None), dict(so=None), dict(x=None), dict(sk=None), dict(xo=None, **no_s), dict(so=None, **no_x)):
        assert call(**part) == INVALID, part                             # an input without its output, an output without its input
    assert call(xo=X) == INVALID and call(so=SK) == INVALID              # in place
    for other in (dict(), no_x, no_s):
        for name in ("h", "w"):
            for bad in (1, 0, -2):
                assert call(**{name: bad}, **other) == INVALID, (name, bad)
        for bad in (0, -1):
            assert call(batch=bad, **other) == INVALID, bad
    for bad in (math.nan, math.inf, -math.inf):
        assert call(b=bad) == INVALID and call(s=bad) == INVALID and call(b=bad, **no_s) == INVALID and call(s=bad, **no_x) == INVALID, bad
    for cx in (0, -16, 8, 24, 632, 648):                                 # cx % 16
        assert call(cx=cx, ldx=656, ldxo=656) == INVALID and call(cx=cx, ldx=656, ldxo=656, **no_s) == INVALID, cx
    for cs in (0, -8, 4, 12, 316, 321):                                  # cs % 8
        assert call(cs=cs, lds=328, ldso=328) == INVALID and call(cs=cs, lds=328, ldso=328, **no_x) == INVALID, cs
    for name, width in (("ldx", 640), ("ldxo", 640), ("lds", 320), ("ldso", 320)):
        for bad in (width - 8, width + 4, width + 1, 0, -width):         # narrower than the rows, or not 16 bytes
            assert call(**{name: bad}) == INVALID, (name, bad)
    for name in ("x", "xo", "sk", "so"):
        assert call(**{name: 0x10000 * 7 + 8}) == INVALID, name          # not 16-byte aligned
    # extents of 2 GiB and beyond: 2^30 halfs
    assert call(batch=1 << 14, h=256, w=256, cx=16, ldx=16, ldxo=16, **no_s) == INVALID       # exactly 2^30 elements
    assert call(batch=1 << 14, h=256, w=256, cs=8, lds=8, ldso=16, **no_x) == INVALID         # the output alone reaches it
    m = (1 << 31) - 1
    assert call(batch=m, h=m, w=m) == INVALID and call(batch=1, h=m, w=m) == INVALID and call(batch=m, h=2, w=2) == INVALID


def test_keywords_are_validated_before_a_model_runs():
    from photoverse_amd.infer import run_inference
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.unet import UNetEngine, normalize_freeu
    sig = inspect.signature(run_inference).parameters
    assert sig["freeu"].kind is inspect.Parameter.KEYWORD_ONLY and sig["freeu"].default is None
    assert inspect.signature(DenoiseLoop.__init__).parameters["freeu"].default is None
    assert inspect.signature(UNetEngine.__init__).parameters["freeu"].default is None
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=5.0, timesteps=4)
    bads = ((1.5, 1.6, 0.9), (1.5, 1.6, 0.9, 0.2, 1.0), (), (1.5, math.nan, 0.9, 0.2), (1.5, 1.6, math.inf, 0.2), (1.5, 1.6, 0.9, -math.inf),
            "abcd", "1.5 1.6 0.9 0.2", ("1.5", "1.6", "0.9", "0.2"), (1.5, 1.6, 0.9, "0.2"), (True, 1, 1, 1), 1.5, dict(b1=1.5, b2=1.6, s1=0.9),
            dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2, s3=1.0), dict(b1=1.5, b2=1.6, s1=0.9, s2=math.nan), dict(b1=1.5, b2=1.6, s1=0.9, s2="x"),
            (1.5, 1.6, 0.9, 1 + 2j))
    for bad in bads:
        with pytest.raises(ValueError, match="freeu"):
            run_inference(*args, freeu=bad, **kw)
        with pytest.raises(ValueError, match="freeu"):
            DenoiseLoop(None, 2, 16, 1, 4, 5.0, freeu=bad)
        with pytest.raises(ValueError, match="freeu"):
            normalize_freeu(bad)
    with pytest.raises(ValueError, match="freeu.*training_mode"):
        run_inference(*args, freeu=FREEU, training_mode=True, **kw)
    with pytest.raises(ValueError, match="freeu.*training_mode"):
        DenoiseLoop(None, 2, 16, 1, 4, 5.0, freeu=FREEU, training_mode=True)
    # legal values get past the validation: the next thing is the first touch of a model argument
    for good in (None, FREEU, list(FREEU), (1, 1, 1, 1), dict(b1=1.5, b2=1.6, s1=0.9, s2=0.2), dict(s2=1, s1=1.0, b2=1, b1=1)):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, freeu=good, **kw)
    # all ones is off
    assert normalize_freeu(None) is None and normalize_freeu((1, 1, 1, 1)) is None and normalize_freeu(dict(b1=1, b2=1.0, s1=1, s2=1)) is None
    assert normalize_freeu(FREEU) == FREEU == normalize_freeu(dict(s2=0.2, s1=0.9, b2=1.6, b1=1.5)) == normalize_freeu(list(FREEU))
    assert normalize_freeu((1, 1, 1, 0.5)) == (1.0, 1.0, 1.0, 0.5)


def test_a_unet_with_one_up_block_refuses_freeu():
    """FreeU acts on the first two up blocks: a UNet with fewer is a ``ValueError`` before anything is recorded (no device needed)."""
    from photoverse_amd.unet import UNet2DConditionModel, UNetEngine
    with torch.device("meta"):
        one = UNet2DConditionModel(block_out_channels=(320,), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D",),
                                   up_block_types=("CrossAttnUpBlock2D",))
    assert len(one.up_blocks) == 1
    with pytest.raises(ValueError, match="freeu"):
        UNetEngine(one, 1, 8, 8, 1, 1, "cpu", freeu=FREEU)
    with pytest.raises(ValueError, match="freeu"):
        UNetEngine(one, 1, 8, 8, 1, 1, "cpu", freeu=(1.5, 1.6))


def test_pipeline_passes_the_keyword_through(monkeypatch, tmp_path):
    """``PhotoVersePipeline.__call__`` hands ``freeu`` to ``run_inference`` unsharded and with ``shard=True`` (a one-rank gloo group)."""
    import torch.distributed as dist
    import photoverse_amd.infer as infer
    from photoverse_amd.pipeline import PhotoVersePipeline
    seen = []

    def fake(example, *a, **kw):
        seen.append(kw)
        return torch.zeros(example["pixel_values_clip"].shape[0], 4, 2, 2)

    monkeypatch.setattr(infer, "run_inference", fake)
    pipe = PhotoVersePipeline(*([None] * 8))
    ex = {"pixel_values_clip": torch.zeros(2, 3, 4, 4)}
    pipe(ex, freeu=FREEU)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        out = pipe(ex, shard=True, freeu=FREEU)
    finally:
        dist.destroy_process_group()
    assert out.shape == (2, 4, 2, 2) and [kw["freeu"] for kw in seen] == [FREEU, FREEU] and seen[1]["sample_offset"] == 0


def test_cli_lists_the_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_freeu", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.parser.parse_args([]).freeu is None
    assert gen.parser.parse_args(["--freeu", "1.5", "1.6", "0.9", "0.2"]).freeu == [1.5, 1.6, 0.9, 0.2]
    with pytest.raises(SystemExit):
        gen.parser.parse_args(["--freeu", "1.5", "1.6", "0.9"])
    text = gen.parser.format_help()
    assert "--freeu" in text and "1.5 1.6 0.9 0.2" in " ".join(text.split())
    assert "--freeu" in open(os.path.join(ROOT, "README.md")).read()


@torch.no_grad()
def test_freeu_oracle_at_ones_is_the_plain_oracle_and_every_number_moves_it():
    """``freeu_oracle(ref, 1, 1, 1, 1)`` reproduces the plain oracle to 1e-5 rel-L2 (measured 8.8e-7: the FFT round trip), and - the precondition of the
    GPU forward test - each of the five settings moves the forward at t = 500 by more than 10 x TOL_FWD.  Measured here (printed with -s): 0.327,
    0.151, 0.210, 0.091, 0.180."""
    ref = tiny_oracle()
    cond, _, noise = loop_inputs_81()
    plain = ref(noise, 500, encoder_hidden_states=cond).sample
    ones = freeu_oracle(ref, 1, 1, 1, 1)(noise, 500, encoder_hidden_states=cond).sample
    d = rel_l2(ones, plain)
    print(f"freeu_oracle(1, 1, 1, 1) vs the plain oracle: rel-L2 = {d:.3e}")
    assert d < 1e-5
    for f in SETTINGS:
        moved = freeu_oracle(ref, *f)(noise, 500, encoder_hidden_states=cond).sample
        d = rel_l2(moved, plain)
        print(f"freeu_oracle{f} vs the plain oracle: rel-L2 = {d:.3e}")
        assert torch.isfinite(moved).all() and d > 10 * TOL_FWD
    assert torch.equal(ref(noise, 500, encoder_hidden_states=cond).sample, plain)          # the oracle itself is untouched


@torch.no_grad()
def test_freeu_moves_the_oracle_loop_by_far_more_than_the_loop_tolerance():
    """The precondition of the GPU loop test on the fp32 oracle alone: 4 steps at B = 2, 16 x 16, guidance 5.  Measured here: rel-L2 0.187."""
    ref = tiny_oracle()
    cond, uncond, noise = loop_inputs_81()
    plain = oracle_loop(ref, None, cond, uncond, noise, G_TEXT)
    moved = oracle_loop(freeu_oracle(ref, *FREEU), None, cond, uncond, noise, G_TEXT)
    d = rel_l2(moved, plain)
    print(f"oracle loop, guidance {G_TEXT}, FreeU {FREEU}: rel-L2 against no FreeU = {d:.3e}")
    assert torch.isfinite(moved).all() and d > 10 * TOL_LOOP
