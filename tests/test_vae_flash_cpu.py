"""CPU-only tests of the VAE's flash attention switch (``AutoencoderKL.enable_flash_attention``): the fp64 reference of
``pv_vae_attention`` (``tests/_vae_flash_ref.py``) pinned against the oracle's mid-block attention, the inputs of ``tests/test_vae_flash_gpu.py`` checked
against the bound before the kernel ever sees them, the switch and the plan-cache key, the ``generate.py`` flag, the symbol in the header / binding /
library, and the launcher's C-ABI rejections."""
import math
import os
import re

import pytest
import torch

from _vae_flash_ref import BOUND, DIMS, SHAPES, attention_ref, growing_case, peaked_case, randn_case, rel_l2
from photoverse_amd.vae import AutoencoderKL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the reference
@torch.no_grad()
def test_reference_reproduces_the_oracles_mid_block_attention():
    """The definition pin: GroupNorm -> fused [3c][c] projection with the fused bias (the V bias inside V) -> ``attention_ref`` at ``scale = c^-0.5``
    -> ``to_out`` + residual, all from the oracle's weights, is the oracle's ``_Attn.forward`` (separate projections, ``scaled_dot_product_attention``)
    to 1e-5 rel-L2 in fp32.  Two images of 5 x 7 tokens: an image's softmax runs over its own keys."""
    from oracle.vae_ref import AutoencoderKLDecoderRef
    torch.manual_seed(3)
    m = AutoencoderKLDecoderRef(**TINY, with_encoder=True).eval().decoder.mid_block.attentions[0]
    b, c, h, w = 2, 256, 5, 7
    x = torch.randn(b, c, h, w)
    exp = m(x)
    t = m.group_norm(x).view(b, c, h * w).transpose(1, 2).reshape(b * h * w, c)
    wqkv = torch.cat([m.to_q.weight, m.to_k.weight, m.to_v.weight], 0)
    bqkv = torch.cat([m.to_q.bias, m.to_k.bias, m.to_v.bias], 0)
    qkv = t @ wqkv.T + bqkv
    o = attention_ref(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], batch=b, n=h * w, scale=c ** -0.5).float()
    got = (o @ m.to_out[0].weight.T + m.to_out[0].bias).view(b, h * w, c).transpose(1, 2).reshape(b, c, h, w) + x
    err = rel_l2(got, exp)
    print(f"reference vs oracle mid-block attention: rel-L2 = {err:.3e}")
    assert err < 1e-5
    # and one image's result does not depend on the other image's rows
    alone = attention_ref(qkv[:h * w, :c], qkv[:h * w, c:2 * c], qkv[:h * w, 2 * c:], batch=1, n=h * w, scale=c ** -0.5).float()
    assert torch.equal(alone, o[:h * w])


@pytest.mark.parametrize("d", DIMS)
def test_the_gpu_tests_inputs_leave_room_under_the_bound(d):
    """Before the inputs are fixed: the fp64 reference with P and the output rounded as the kernel rounds them stays under the kernel bound on every
    input of ``tests/test_vae_flash_gpu.py`` (so the bound can be met), and the two running-maximum cases are what they claim - finite in fp64, scaled
    scores to about +-60 in the peaked case, a row maximum that rises by more than 8 binary orders per full 64-key tile (the kernel's lazy threshold) in the growing one."""
    scale = d ** -0.5
    cases = [(f"randn {s}", randn_case(d, *s), s) for s in SHAPES] + [("growing", growing_case(d), (2, 200)), ("peaked", peaked_case(d), (1, 129))]
    for name, (q, k, v), (batch, n) in cases:
        exact = attention_ref(q, k, v, batch=batch, n=n, scale=scale)
        rounded = attention_ref(q, k, v, batch=batch, n=n, scale=scale, round_p=True)
        assert torch.isfinite(exact).all() and torch.isfinite(rounded).all(), name
        err = rel_l2(rounded, exact)
        print(f"d = {d}, {name}: rounded-P reference vs exact rel-L2 = {err:.3e}")
        assert err < BOUND, name
    q, k, _ = peaked_case(d)
    s = scale * (q.double() @ k.double().T)
    assert 45 < s.abs().max().item() < 110
    q, k, _ = growing_case(d)
    s = scale * (q[:200].double() @ k[:200].double().T) * math.log2(math.e)
    tile_max = torch.stack([s[:, t:t + 64].max(dim=1).values for t in range(0, 200, 64)], 1)
    rise = tile_max[:, 1:] - tile_max[:, :-1]
    assert (rise[:, :2] > 8).all() and (rise[:, 2] > 0).all()         # the fourth tile holds 8 keys: it rises again, by less


# ---------------------------------------------------------------------------------------------------------------- the switch
def test_switch_is_off_by_default_and_checks_the_width():
    vae = AutoencoderKL(**TINY)
    assert vae.use_flash_attention is False
    vae.enable_flash_attention()
    assert vae.use_flash_attention is True
    vae.disable_flash_attention()
    assert vae.use_flash_attention is False
    with torch.device("meta"):
        AutoencoderKL().enable_flash_attention()                       # SD-1.5: 512 wide
    narrow = AutoencoderKL(**dict(TINY, block_out_channels=(128, 128)))
    with pytest.raises(ValueError, match="256 and 512"):
        narrow.enable_flash_attention()
    assert narrow.use_flash_attention is False                         # a rejected call changes nothing
    with pytest.raises(ValueError, match="256 and 512"):
        AutoencoderKL(**dict(TINY, block_out_channels=(128, 384))).enable_flash_attention()


def test_plan_cache_key_carries_the_flag():
    vae = AutoencoderKL(**TINY)
    dev = torch.device("cpu")
    off = (vae._plan_key("dec", 2, 8, 8, dev), vae._plan_key("enc", 2, 16, 16, dev))
    vae.enable_flash_attention()
    on = (vae._plan_key("dec", 2, 8, 8, dev), vae._plan_key("enc", 2, 16, 16, dev))
    vae.disable_flash_attention()
    assert off == (vae._plan_key("dec", 2, 8, 8, dev), vae._plan_key("enc", 2, 16, 16, dev))
    assert off[0] != on[0] and off[1] != on[1] and len({*off, *on}) == 4
    assert off[0][:4] == on[0][:4] == (2, 8, 8, dev) and off[1][:5] == on[1][:5] == ("enc", 2, 16, 16, dev)     # the leading fields other code reads


def test_generate_flag_reaches_the_vae():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_vae_flash", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)

    class Stub:
        calls = []

        def enable_flash_attention(self):
            self.calls.append("flash")

        def enable_tiling(self, size, overlap):
            self.calls.append(("tiling", size, overlap))

    assert gen.parser.parse_args([]).vae_flash_attention is False
    gen.configure_vae(gen.parser.parse_args([]), Stub())
    assert Stub.calls == []
    gen.configure_vae(gen.parser.parse_args(["--vae_flash_attention"]), Stub())
    assert Stub.calls == ["flash"]
    gen.configure_vae(gen.parser.parse_args(["--vae_flash_attention", "--vae_tiling", "--vae_tile_size", "256"]), Stub())
    assert Stub.calls == ["flash", ("tiling", 256, 0.25), "flash"]
    assert "--vae_flash_attention" in gen.parser.format_help()
    assert "--vae_flash_attention" in open(os.path.join(ROOT, "README.md")).read()


# ---------------------------------------------------------------------------------------------------------------- the symbol
def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    from photoverse_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_vae_attention\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_vae_attention"]
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 13
    v, i = _lib.c_void_p, _lib.c_int
    assert args == [v, v, v, i, i, i, v, i, i, i, i, _lib.c_float, v]
    assert lib.pv_vae_attention.argtypes == args and "pv_vae_attention" not in _lib.SIGNATURES
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    assert "pv_vaeattn.hip" in SOURCES


def test_cabi_rejects_bad_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  The pointers are never dereferenced; no
    valid call is sent."""
    INVALID = 1
    Q, K, V, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000        # 256 MiB apart

    def attn(q=Q, k=K, v=V, ldq=512, ldk=512, ldv=512, out=OUT, ldo=512, batch=2, n=100, d=512, scale=512 ** -0.5):
        return lib.pv_vae_attention(q, k, v, ldq, ldk, ldv, out, ldo, batch, n, d, scale, None)

    for name in ("q", "k", "v", "out"):
        assert attn(**{name: None}) == INVALID, name
        assert attn(**{name: 0x10000008}) == INVALID, name                 # 8-byte aligned only
    for d in (0, 40, 128, 255, 264, 384, 1024, -256):
        assert attn(d=d, ldq=1024, ldk=1024, ldv=1024, ldo=1024) == INVALID, d
    for name in ("ldq", "ldk", "ldv", "ldo"):
        for bad in (0, -512, 256, 504, 516, 513):                          # below d; not a multiple of 8
            assert attn(**{name: bad}) == INVALID, (name, bad)
        assert attn(d=256, **{name: 260}) == INVALID, name
    for name in ("batch", "n"):
        for bad in (0, -1):
            assert attn(**{name: bad}) == INVALID, (name, bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert attn(scale=bad) == INVALID, bad
    # out overlaps an input: the same buffer, a column slice of the same rows, its last element on an input's first
    ext = ((2 * 100 - 1) * 512 + 512) * 2
    for name in ("q", "k", "v"):
        assert attn(**{name: OUT}) == INVALID, name
        assert attn(**{name: OUT + ext - 16}) == INVALID, name
        assert attn(**{name: OUT - ext + 16}) == INVALID, name
    assert attn(q=Q, k=Q + 1024, v=Q + 2048, out=Q + 3072, ldq=2048, ldk=2048, ldv=2048, ldo=2048) == INVALID
    # an operand extent of 2 GiB or more: by rows, by a leading dimension, and without 32- or 64-bit wrap-around
    assert attn(batch=1, n=1 << 21, d=512) == INVALID                                                # 2^21 rows x 1 KiB
    assert attn(batch=1 << 11, n=1 << 11, d=256, ldq=256, ldk=256, ldv=256, ldo=256) == INVALID
    assert attn(batch=1, n=3, ldk=1 << 30) == INVALID
    assert attn(batch=1, n=2, ldo=(1 << 30) - 248) == INVALID                                        # ((n - 1) * ld + d) * 2 = 2^31 + 528
    assert attn(batch=1 << 30, n=1 << 30) == INVALID
    assert attn(batch=(1 << 31) - 1, n=(1 << 31) - 1, ldq=(1 << 31) - 8) == INVALID
