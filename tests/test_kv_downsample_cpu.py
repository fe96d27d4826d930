"""CPU-only tests of token downsampling (``kv_downsample``; ToDo, Smith et al. 2024): the new symbol ``pv_token_pool`` in the header, ``_lib`` and the built
library, its C-ABI rejections, the per-block-loop references of the pooling (``pool_rows_ref``: the reference of ``tests/test_kv_downsample_gpu.py``) and
of the pooled self-attention (``PooledAttnProcessorRef`` on the fp32 oracle), ``resolve_kv_downsample_layers``, the keyword validation of
``run_inference``, the CLI flags, and - on the oracle alone - that the pooling moves a forward by far more than the GPU tests' tolerance."""
import copy
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle.unet_ref import AttnProcessor2_0Ref
from test_guidance_cpu import _Untouchable
from test_pag_cpu import B, S, TOL_FWD, loop_inputs_81, rel_l2, tiny_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHODS = ("avg", "nearest")
#: the tiny UNet's transformers at its highest-resolution level (the default selection) and all of them
TOP = ("down_blocks.0.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")
ALL = ("down_blocks.0.attentions.0", "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1")


# ---------------------------------------------------------------------------------------------------------------- references
def pool_grid_ref(x, f, method):
    """``x`` (B, h, w, C), any float dtype -> (B, ceil(h / f), ceil(w / f), C) in fp64, block by block in explicit loops: ``avg`` - the mean of the block's
    in-bounds pixels; ``nearest`` - its top-left pixel."""
    b, h, w, c = x.shape
    hp, wp = -(-h // f), -(-w // f)
    out = torch.empty((b, hp, wp, c), dtype=torch.float64)
    for oy in range(hp):
        for ox in range(wp):
            blk = x[:, oy * f:min(oy * f + f, h), ox * f:min(ox * f + f, w)].double()
            out[:, oy, ox] = blk.reshape(b, -1, c).mean(dim=1) if method == "avg" else blk[:, 0, 0]
    return out


def pool_rows_ref(rows, batch, h, w, f, method):
    """``pv_token_pool`` on rows ``[batch * h * w][cols]`` -> fp64 rows ``[batch * hp * wp][cols]``."""
    cols = rows.shape[1]
    return pool_grid_ref(rows.reshape(batch, h, w, cols), f, method).reshape(-1, cols)


def grid_of(n_tokens, size):
    """(h, w) of the level of a UNet run at latent ``size = (H, W)`` whose token count is ``n_tokens``."""
    H, W = size
    for lvl in range(8):
        if (H >> lvl) * (W >> lvl) == n_tokens:
            return H >> lvl, W >> lvl
    raise AssertionError((n_tokens, size))


class PooledAttnProcessorRef(AttnProcessor2_0Ref):
    """Self-attention whose keys and values come from the pooled token grid: the stock processor, handed the pooled hidden states as
    ``encoder_hidden_states`` (``to_k`` / ``to_v`` have no bias: projecting pooled rows is pooling projected rows)."""

    def __init__(self, factor, method, size):
        self.factor, self.method, self.size = factor, method, size

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kw):
        assert encoder_hidden_states is None
        b, n, c = hidden_states.shape
        h, w = grid_of(n, self.size)
        pooled = pool_grid_ref(hidden_states.reshape(b, h, w, c), self.factor, self.method).to(hidden_states.dtype)
        return super().__call__(attn, hidden_states, encoder_hidden_states=pooled.reshape(b, -1, c))


def pooled_oracle(ref, names, factor, method, size=(S, S)):
    """A deep copy of an oracle (UNet or ControlNet) whose transformers ``names`` - those it has - carry ``PooledAttnProcessorRef`` on attn1."""
    out = copy.deepcopy(ref)
    mods = dict(out.named_modules())
    hit = 0
    for nm in names:
        a1 = mods.get(f"{nm}.transformer_blocks.0.attn1")
        if a1 is not None:
            a1.set_processor(PooledAttnProcessorRef(factor, method, size))
            hit += 1
    assert hit or not names
    return out


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    """``pv_token_pool``: ten parameters and the stream, declared in the header, bound by ``_lib.load()`` and exported by the library, whose ABI number
    stays 19; the two modes have the header's values."""
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_token_pool\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_token_pool"]
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 11
    assert args == [_lib.c_void_p, _lib.c_int, _lib.c_void_p] + [_lib.c_int] * 7 + [_lib.c_void_p]
    assert lib.pv_token_pool is not None and lib.pv_token_pool.argtypes == args
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    for name, value in _lib.POOL_MODES.items():
        assert int(re.search(rf"#define PV_POOL_{name.upper()} (\d+)", header).group(1)) == value
    assert set(_lib.POOL_MODES) == set(METHODS)


def test_cabi_rejects_bad_token_pool_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  The pointers are never dereferenced; no
    valid call is sent."""
    INVALID = 1
    X, OUT = 0x10000, 0x20000

    def call(x=X, ldx=960, out=OUT, ldo=640, cols=640, batch=2, h=16, w=16, f=2, mode=0):
        return lib.pv_token_pool(x, ldx, out, ldo, cols, batch, h, w, f, mode, None)

    for mode in (0, 1):
        for name in ("x", "out"):
            assert call(**{name: None}, mode=mode) == INVALID, name
        for cols in (0, -8, 4, 12, 636, 641):
            assert call(cols=cols, mode=mode) == INVALID, cols
        for ldx in (961, 964, 636, 632, 0, -960):                    # not a multiple of 8; below cols
            assert call(ldx=ldx, mode=mode) == INVALID, ldx
        for ldo in (641, 644, 636, 632, 0, -640):
            assert call(ldo=ldo, mode=mode) == INVALID, ldo
        for name in ("batch", "h", "w"):
            for v in (0, -1, -16):
                assert call(**{name: v}, mode=mode) == INVALID, (name, v)
        for f in (-2, -1, 0, 1, 9, 16, 1 << 20):
            assert call(f=f, mode=mode) == INVALID, f
        assert call(x=0x10008, mode=mode) == INVALID and call(out=0x20002, mode=mode) == INVALID     # 16-byte alignment
        assert call(out=X, mode=mode) == INVALID                                                         # in place
        # extents of 2^31 bytes and beyond
        assert call(batch=1, h=1 << 10, w=1 << 10, ldx=1024, mode=mode) == INVALID                       # 2^20 rows x 2^10 halfs = 2^31 bytes
        m = (1 << 31) - 1
        assert call(batch=m, h=m, w=m, mode=mode) == INVALID
        assert call(batch=1 << 16, h=1 << 16, w=1 << 16, mode=mode) == INVALID
    for mode in (-1, 2, 3, 100):
        assert call(mode=mode) == INVALID, mode


@pytest.mark.parametrize("f", (2, 3, 4, 8))
def test_block_loop_reference_is_avg_pool2d_and_the_strided_slice(f):
    """``pool_grid_ref`` - explicit loops over the blocks - equals ``F.avg_pool2d(ceil_mode=True, count_include_pad=False)`` and ``[::f, ::f]`` on grids that
    ``f`` divides, does not divide, and exceeds, ``h != w`` included."""
    g = torch.Generator().manual_seed(f)
    for b, h, w, c in ((1, 2, 2, 3), (1, 2, 3, 5), (2, 5, 7, 4), (2, 6, 6, 8), (1, 16, 24, 2), (1, 9, 1, 3)):
        x = torch.randn(b, h, w, c, generator=g, dtype=torch.float64)
        avg = F.avg_pool2d(x.permute(0, 3, 1, 2), f, ceil_mode=True, count_include_pad=False).permute(0, 2, 3, 1)
        got = pool_grid_ref(x, f, "avg")
        assert got.shape == (b, -(-h // f), -(-w // f), c) == avg.shape
        torch.testing.assert_close(got, avg, rtol=1e-13, atol=1e-13)
        assert torch.equal(pool_grid_ref(x, f, "nearest"), x[:, ::f, ::f])
        rows = x.reshape(b * h * w, c)
        assert torch.equal(pool_rows_ref(rows, b, h, w, f, "avg"), got.reshape(-1, c))


def test_pooled_processor_is_the_stock_one_on_pooled_keys():
    """``PooledAttnProcessorRef`` on a tiny attention module: the stock processor's result with the pooled grid as ``encoder_hidden_states`` - and, the
    projections having no bias, the same as pooling the projected K and V rows (what the engine does)."""
    ref = tiny_oracle()
    a1 = dict(ref.named_modules())["down_blocks.0.attentions.0.transformer_blocks.0.attn1"]
    assert a1.to_k.bias is None and a1.to_v.bias is None
    g = torch.Generator().manual_seed(3)
    b, h, w, c = 2, 6, 10, a1.to_q.weight.shape[1]
    hs = torch.randn(b, h * w, c, generator=g)
    for f, method in ((2, "avg"), (4, "avg"), (2, "nearest"), (4, "nearest")):
        got = PooledAttnProcessorRef(f, method, (h, w))(a1, hs)
        k = pool_grid_ref(a1.to_k(hs).reshape(b, h, w, c), f, method).float().reshape(b, -1, a1.heads, c // a1.heads).transpose(1, 2)
        v = pool_grid_ref(a1.to_v(hs).reshape(b, h, w, c), f, method).float().reshape(b, -1, a1.heads, c // a1.heads).transpose(1, 2)
        q = a1.to_q(hs).reshape(b, -1, a1.heads, c // a1.heads).transpose(1, 2)
        exp = a1.to_out[1](a1.to_out[0](F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, -1, c)))
        assert got.shape == hs.shape
        torch.testing.assert_close(got, exp, rtol=1e-4, atol=1e-5)


def test_resolve_kv_downsample_layers():
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.unet import UNet2DConditionModel, normalize_kv_downsample, resolve_kv_downsample_layers, resolve_pag_layers, transformer_names
    tiny = UNet2DConditionModel(**TINY_CONFIG)
    assert transformer_names(tiny) == ALL
    assert resolve_kv_downsample_layers(tiny) == resolve_kv_downsample_layers(tiny, None) == TOP
    assert resolve_kv_downsample_layers(tiny, "all") == resolve_kv_downsample_layers(tiny, ("all",)) == ALL
    assert resolve_kv_downsample_layers(tiny, ("mid_block",)) == ALL[1:2] == resolve_pag_layers(tiny, ("mid_block",))
    assert resolve_kv_downsample_layers(tiny, ["up_blocks.1.attentions.1", "down_blocks"]) == (ALL[0], ALL[3])
    for bad in (("mid_blocks",), ("mid_block", "down_blocks.1"), ("up_blocks.0",), (), ("",), (3,), 3):
        with pytest.raises(ValueError, match="kv_downsample_layers"):
            resolve_kv_downsample_layers(tiny, bad)
        if bad != ():
            with pytest.raises(ValueError, match="pag_layers"):          # one resolver, two names
                resolve_pag_layers(tiny, bad)
    with torch.device("meta"):
        sd15 = UNet2DConditionModel()
    # SD-1.5: the 64 x 64 level - two transformers of the first down block, three of the last up block
    assert resolve_kv_downsample_layers(sd15) == ("down_blocks.0.attentions.0", "down_blocks.0.attentions.1", "up_blocks.3.attentions.0",
                                                  "up_blocks.3.attentions.1", "up_blocks.3.attentions.2")
    assert len(resolve_kv_downsample_layers(sd15, "all")) == 16
    # the engine's form of the setting
    assert normalize_kv_downsample(None) is None and normalize_kv_downsample((2, "avg", ())) is None
    assert normalize_kv_downsample((4, "nearest", list(TOP))) == (4, "nearest", TOP)
    for bad in (2, (2, "avg"), (1, "avg", TOP), (9, "avg", TOP), (2.0, "avg", TOP), (True, "avg", TOP), (2, "max", TOP), (2, "avg", (3,))):
        with pytest.raises(ValueError, match="kv_downsample"):
            normalize_kv_downsample(bad)


def test_keywords_are_validated_before_a_model_runs():
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.infer import run_inference
    from photoverse_amd.pipeline import DenoiseLoop
    from photoverse_amd.unet import UNet2DConditionModel
    sig = inspect.signature(run_inference).parameters
    for name, default in (("kv_downsample", None), ("kv_downsample_method", "avg"), ("kv_downsample_layers", None), ("hires_kv_downsample", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    lsig = inspect.signature(DenoiseLoop.__init__).parameters
    assert lsig["kv_downsample"].default is None and lsig["kv_downsample_method"].default == "avg" and lsig["kv_downsample_layers"].default is None
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=5.0, timesteps=4)
    hi = dict(hires_latent_size=32)
    for bad in (0, 1, 9, -2, 2.0, "2", True, math.nan, [2]):
        with pytest.raises(ValueError, match="kv_downsample"):
            run_inference(*args, kv_downsample=bad, **kw)
    for bad in (0, 9, -2, 2.0, "2", True, math.nan, [2]):
        with pytest.raises(ValueError, match="hires_kv_downsample"):
            run_inference(*args, hires_kv_downsample=bad, **hi, **kw)
    with pytest.raises(ValueError, match="hires_kv_downsample.*hires_latent_size"):
        run_inference(*args, hires_kv_downsample=2, **kw)
    for bad in ("max", "bilinear", None, 0, ("avg",)):
        with pytest.raises(ValueError, match="kv_downsample_method"):
            run_inference(*args, kv_downsample=2, kv_downsample_method=bad, **kw)
        with pytest.raises(ValueError, match="kv_downsample_method"):          # also while the factor is off
            run_inference(*args, kv_downsample_method=bad, **kw)
    with pytest.raises(ValueError, match="kv_downsample_layers"):
        run_inference(*args, kv_downsample=2, kv_downsample_layers=7, **kw)
    with pytest.raises(ValueError, match="kv_downsample.*training_mode"):
        run_inference(*args, kv_downsample=2, training_mode=True, **kw)
    # off: the next thing is the first touch of a model argument
    for good in (dict(), dict(kv_downsample=None), dict(kv_downsample=None, kv_downsample_method="nearest"), dict(hires_kv_downsample=1, **hi)):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)
    # the layers resolve against the UNet's module tree alone - every other model is still untouched when an unknown entry is refused
    tiny = UNet2DConditionModel(**TINY_CONFIG)
    margs = (u, u, u, u, tiny, u, u, u, u, "cpu", [1])
    for bad in (("nothing",), ("mid_block", "up_blocks.0"), ()):
        with pytest.raises(ValueError, match="kv_downsample_layers"):
            run_inference(*margs, kv_downsample=2, kv_downsample_layers=bad, **kw)
        with pytest.raises(ValueError, match="kv_downsample_layers"):
            run_inference(*margs, hires_kv_downsample=4, kv_downsample_layers=bad, **hi, **kw)
    for good in (dict(kv_downsample=2), dict(kv_downsample=8, kv_downsample_method="nearest", kv_downsample_layers="all"),
                 dict(hires_kv_downsample=2, kv_downsample_layers=("up_blocks",), **hi), dict(kv_downsample=2, hires_kv_downsample=1, **hi)):
        with pytest.raises(AssertionError, match="touched a model argument"):          # legal: got past the validation
            run_inference(*margs, **good, **kw)


def test_cli_flags_parse_and_default_to_off():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_kv", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.kv_downsample is None and d.kv_downsample_method == "avg" and d.kv_downsample_layers is None and d.hires_kv_downsample is None
    a = gen.parser.parse_args(["--kv_downsample", "2", "--kv_downsample_method", "nearest", "--kv_downsample_layers", "down_blocks.0", "up_blocks",
                               "--hires_kv_downsample", "4"])
    assert a.kv_downsample == 2 and a.kv_downsample_method == "nearest" and a.kv_downsample_layers == ["down_blocks.0", "up_blocks"]
    assert a.hires_kv_downsample == 4
    with pytest.raises(SystemExit):
        gen.parser.parse_args(["--kv_downsample_method", "max"])
    for flag in ("--kv_downsample", "--kv_downsample_method", "--kv_downsample_layers", "--hires_kv_downsample"):
        assert flag in gen.__doc__, flag
    assert "--hires_kv_downsample" in open(os.path.join(ROOT, "README.md")).read()
    assert "kv_downsample" in open(os.path.join(ROOT, "DESIGN.md")).read()


@torch.no_grad()
def test_pooling_moves_the_oracle_forward_by_far_more_than_the_forward_tolerance():
    """The precondition of the GPU engine test, on the fp32 oracle alone: the tiny model under ``torch.manual_seed(0)``, inputs from generator seed 81,
    one conditional forward at B = 2, 16 x 16, t = 500.  Pooling the default layers moves it by at least 4 x TOL_FWD in rel-L2 for both methods at f = 2
    and 4, so an engine that ignored the setting - or the method - could not pass.  Measured on the CPU (printed with -s): avg 1.45e-2 (f = 2) and 1.81e-2
    (f = 4), nearest 4.28e-2 and 1.12e-1."""
    ref = tiny_oracle()
    cond, _, noise = loop_inputs_81()
    assert noise.shape == (B, 4, S, S)
    plain = ref(noise, 500, encoder_hidden_states=cond).sample
    seen = {}
    for method in METHODS:
        for f in (2, 4):
            moved = pooled_oracle(ref, TOP, f, method)(noise, 500, encoder_hidden_states=cond).sample
            d = seen[(method, f)] = rel_l2(moved, plain)
            print(f"oracle forward, kv_downsample {f} {method} on the default layers: rel-L2 against the plain forward = {d:.3e}")
            assert torch.isfinite(moved).all() and d >= 4 * TOL_FWD
    assert rel_l2(pooled_oracle(ref, TOP, 2, "avg")(noise, 500, encoder_hidden_states=cond).sample,
                  pooled_oracle(ref, TOP, 2, "nearest")(noise, 500, encoder_hidden_states=cond).sample) >= 4 * TOL_FWD
