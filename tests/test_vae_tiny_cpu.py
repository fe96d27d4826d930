"""CPU-only tests of ``AutoencoderTiny``: the reference of ``tests/_taesd_ref.py`` checked by hand, the inputs of
``tests/test_vae_tiny_gpu.py`` checked against their bounds before the kernel ever sees them, the ``pv_tiny_conv3x3`` symbol in the header / binding / library
and its C-ABI rejections, the model's config errors and state dict, and the ``generate.py`` flag."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from _taesd_ref import (DECODE_CASES, ENCODE_CASES, IMAGE_ULPS, KERNEL_BOUND, KERNEL_FORMS, KERNEL_SHAPES, TOL, WALK_SHAPE, conv_ref,
                        kernel_case, latents_case, pixels_case, rel_l2, seeded_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ref():
    return seeded_ref(0)


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_reference_shapes_keys_and_parameter_count(ref):
    sd = ref.state_dict()
    convs = lambda side, idx: [k for k in sd if re.fullmatch(rf"{side}\.layers\.(\d+)\.weight", k) and int(k.split(".")[2]) in idx]
    assert len(convs("decoder", {0, 6, 11, 16, 18})) == 5 and len(convs("encoder", {0, 2, 6, 10, 14})) == 5
    for n in (6, 11, 16):
        assert f"decoder.layers.{n}.bias" not in sd                                   # the convs behind an upsample have no bias
    for n in (2, 6, 10):
        assert f"encoder.layers.{n}.bias" not in sd and ref.encoder.layers[n].stride == (2, 2)
    assert "decoder.layers.18.bias" in sd and "encoder.layers.14.bias" in sd and "encoder.layers.0.bias" in sd
    blocks = lambda side: sorted({int(k.split(".")[2]) for k in sd if k.startswith(side) and ".conv." in k})
    assert blocks("decoder") == [2, 3, 4, 7, 8, 9, 12, 13, 14, 17] and blocks("encoder") == [1, 3, 4, 5, 7, 8, 9, 11, 12, 13]
    assert {k.split(".")[4] for k in sd if ".conv." in k} == {"0", "2", "4"}
    conv64, block = 64 * 64 * 9, 3 * (64 * 64 * 9 + 64)
    dec = (4 * 64 * 9 + 64) + 10 * block + 3 * conv64 + (64 * 3 * 9 + 3)
    enc = (3 * 64 * 9 + 64) + 10 * block + 3 * conv64 + (64 * 4 * 9 + 4)
    assert sum(p.numel() for p in ref.decoder.parameters()) == dec and sum(p.numel() for p in ref.encoder.parameters()) == enc
    assert sum(p.numel() for p in ref.parameters()) == dec + enc == 2445063
    assert ref.decode(torch.zeros(2, 4, 5, 7)).shape == (2, 3, 40, 56) and ref.encode(torch.zeros(1, 3, 13, 21)).shape == (1, 4, 2, 3)
    assert ref.encode(torch.zeros(2, 3, 40, 56)).shape == (2, 4, 5, 7) and ref.decode(torch.zeros(1, 4, 1, 1)).shape == (1, 3, 8, 8)


def test_conv_reference_by_hand():
    """One conv against sums written out: the UNIT pre-transform with zero padding AFTER it (a -1 input becomes 0, the padding is 0 - not (0 + 1) / 2), stride-2
    output sizes on odd extents, and ``upsample`` = ``F.interpolate(nearest)`` then conv."""
    c = kernel_case("image3_unit_in", 1, 2, 3)
    c["x"] = -torch.ones(1, 3, 2, 3)
    c["x"][0, 1, 0, 0] = 1.0                                                          # (1 + 1) / 2 = 1 at channel 1, pixel (0, 0); everything else 0
    y, mag = conv_ref(c)
    w = c["w"].double().view(64, 3, 3, 3)                                             # [co][ky][kx][ci]
    b = c["b"].double()
    assert torch.allclose(y[0, :, 0, 0], b + w[:, 1, 1, 1]) and torch.allclose(y[0, :, 1, 1], b + w[:, 0, 0, 1])
    assert torch.allclose(y[0, :, 1, 2], b) and torch.allclose(y[0, :, 0, 1], b + w[:, 1, 0, 1])        # a padded border adds nothing
    assert torch.allclose(mag[0, :, 0, 0], b.abs() + w[:, 1, 1, 1].abs())
    for h, wd, ho, wo in ((1, 1, 1, 1), (3, 5, 2, 3), (9, 17, 5, 9), (8, 8, 4, 4)):
        c = kernel_case("stride2", 1, h, wd)
        y, _ = conv_ref(c)
        assert (c["ho"], c["wo"]) == (ho, wo) and y.shape == (1, 64, ho, wo)
        w4 = c["w"].double().view(64, 3, 3, 64)
        exp = sum(w4[:, ky, kx, :] @ c["x"].double()[0, :, ky - 1, kx - 1] for ky in (1, 2) for kx in (1, 2) if ky - 1 < h and kx - 1 < wd)
        assert torch.allclose(y[0, :, 0, 0], exp)                                     # output (0, 0) reads inputs (-1 .. 1, -1 .. 1)
    c = kernel_case("upsample", 2, 3, 5)
    y, _ = conv_ref(c)
    w4 = c["w"].double().view(64, 3, 3, 64).permute(0, 3, 1, 2)
    assert torch.allclose(y, F.conv2d(F.interpolate(c["x"].double(), scale_factor=2, mode="nearest"), w4, padding=1)) and y.shape == (2, 64, 6, 10)
    # tap (iy, ix) of the upsampled conv reads the low-resolution pixel (iy >> 1, ix >> 1); outside [0, 2h) x [0, 2w) it is 0
    x = c["x"].double()
    oy, ox = 5, 9                                                                     # the last output pixel: taps at iy = 6 and ix = 10 are padding
    exp = sum(w4[:, :, ky, kx] @ x[1, :, (oy + ky - 1) >> 1, (ox + kx - 1) >> 1] for ky in range(3) for kx in range(3) if oy + ky - 1 < 6 and ox + kx - 1 < 10)
    assert torch.allclose(y[1, :, oy, ox], exp)


def test_the_gpu_tests_inputs_leave_room_under_the_bound(ref):
    """The precondition of the GPU bounds: the reference with fp16 weights and every launch's output rounded to fp16 stays under HALF of ``TOL`` on exactly
    the model inputs of the GPU tests; one launch's fp64 result rounded to fp16 once stays under half of the kernel bound; and fp32 arithmetic on the image
    outputs stays inside half of the per-element bound."""
    for shape in DECODE_CASES:
        z = latents_case(shape)
        err = rel_l2(ref.decode(z, emulate_fp16=True), ref.decode(z))
        print(f"decode {shape}: fp16-emulated vs fp32 rel-L2 = {err:.3e}, max |activation| = {ref.max_activation:.2f}")
        assert err < TOL / 2 and ref.max_activation < 100
    assert latents_case((1, 4, 8, 8)).abs().max() > 6                                 # TANH3 in its curved range
    for shape in ENCODE_CASES:
        x = pixels_case(shape)
        err = rel_l2(ref.encode(x, emulate_fp16=True), ref.encode(x))
        print(f"encode {shape}: fp16-emulated vs fp32 rel-L2 = {err:.3e}, max |activation| = {ref.max_activation:.2f}")
        assert err < TOL / 2 and ref.max_activation < 100
    for form in KERNEL_FORMS:
        for shape in KERNEL_SHAPES + [WALK_SHAPE if form in ("plain", "stride2", "upsample", "image3_out") else (1, 1, 1)]:
            c = kernel_case(form, *shape)
            exact, mag = conv_ref(c)
            assert torch.isfinite(exact).all()
            if c["out_image"]:
                w4 = c["w"].view(c["cout"], 3, 3, 64).permute(0, 3, 1, 2).contiguous()
                got = (F.conv2d(c["x"], w4, c["b"], padding=1) * c["scale"] + c["shift"]).double()
                assert ((got - exact).abs() <= IMAGE_ULPS / 2 * mag).all(), (form, shape)
            else:
                err = rel_l2(conv_ref(c, round_out=True)[0], exact)
                assert err < KERNEL_BOUND / 2, (form, shape, err)


# ---------------------------------------------------------------------------------------------------------------- the symbol
def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib, ops
    from photoverse_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_tiny_conv3x3\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_tiny_conv3x3"]
    v, i, f = _lib.c_void_p, _lib.c_int, _lib.c_float
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 22
    assert args == [v, i, i, i, v, v, v, i, v, i, i, f, f, i, i, i, i, i, i, i, i, v]
    assert lib.pv_tiny_conv3x3.argtypes == args and "pv_tiny_conv3x3" not in _lib.SIGNATURES
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    assert "pv_tinyconv.hip" in SOURCES
    assert ops.ACT_RELU == 5 == int(re.search(r"PV_ACT_RELU = (\d+)", header).group(1))
    for name, val in (("none", 0), ("tanh3", 1), ("unit", 2)):
        assert ops.TINY_PRE[name] == val == int(re.search(rf"#define PV_TINY_PRE_{name.upper()} (\d+)", header).group(1))
    import photoverse_amd
    from photoverse_amd.vae_tiny import AutoencoderTiny
    assert photoverse_amd.AutoencoderTiny is AutoencoderTiny


def test_cabi_rejects_bad_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  The pointers are never dereferenced; no valid
    call is sent."""
    INVALID = 1
    X, W, B, R, OUT = 0x10000000, 0x20000000, 0x28000000, 0x30000000, 0x40000000
    RELU = 5

    def conv(x=X, x_is_image=0, ldx=64, pre=0, w=W, bias=B, res=None, ldr=0, out=OUT, out_is_image=0, ldo=64, scale=1.0, shift=0.0, batch=2, cin=64,
             cout=64, h=9, wd=17, stride=1, upsample=0, act=0):
        return lib.pv_tiny_conv3x3(x, x_is_image, ldx, pre, w, bias, res, ldr, out, out_is_image, ldo, scale, shift, batch, cin, cout, h, wd, stride,
                                   upsample, act, None)

    image_in = dict(x_is_image=1, cin=3, pre=2, ldx=0)
    image_out = dict(out_is_image=1, cout=3, ldo=0)
    for name in ("x", "w", "out"):
        assert conv(**{name: None}) == INVALID, name
    for name in ("x", "w", "bias", "out"):
        assert conv(**{name: 0x10000008 + 0x1000000}) == INVALID, name                # 8-byte aligned only
    assert conv(res=R + 8, ldr=64) == INVALID
    for name in ("ldx", "ldo"):
        for bad in (0, -64, 56, 63, 68, 100):                                         # below the width; not a multiple of 8
            assert conv(**{name: bad}) == INVALID, (name, bad)
    for bad in (0, 56, 68):
        assert conv(res=R, ldr=bad) == INVALID, bad
    for bad in (0, 8, 32, 63, 128, -64):                                              # rows in / rows out are 64 wide
        assert conv(cin=bad, ldx=128) == INVALID and conv(cout=bad, ldo=128) == INVALID, bad
    for bad in (0, 5, 8, 64, -1):                                                     # the image forms carry 1 ... 4 channels
        assert conv(**dict(image_in, cin=bad)) == INVALID and conv(**dict(image_out, cout=bad)) == INVALID, bad
    assert conv(**image_in, **image_out) == INVALID                                   # image in and image out
    assert conv(stride=2, upsample=1) == INVALID
    for bad in (0, 3, -1):
        assert conv(stride=bad) == INVALID, bad
    for bad in (2, -1):
        assert conv(upsample=bad) == INVALID, bad
    assert conv(**image_in, stride=2) == INVALID and conv(**image_in, upsample=1) == INVALID     # the geometry belongs to the rows input
    assert conv(**image_out, res=R, ldr=64) == INVALID and conv(**image_out, act=RELU) == INVALID
    for bad in (float("nan"), float("inf")):
        assert conv(**image_out, scale=bad) == INVALID and conv(**image_out, shift=bad) == INVALID
    for bad in (3, -1, 7):
        assert conv(**dict(image_in, pre=bad)) == INVALID, bad
    assert conv(pre=1) == INVALID                                                     # a pre-transform on the rows input
    for bad in (1, 2, 3, 4, 6, -1):                                                   # only PV_ACT_NONE (0) and PV_ACT_RELU (5)
        assert conv(act=bad) == INVALID, bad
    for name in ("batch", "h", "wd"):
        for bad in (0, -1):
            assert conv(**{name: bad}) == INVALID, (name, bad)
    # out overlaps something the launch reads: the input, the weight, the bias, the residual - the same buffer, or by one element at either end
    ext = ((2 * 9 * 17 - 1) * 64 + 64) * 2
    for kw in (dict(x=OUT), dict(x=OUT + ext - 16), dict(x=OUT - ext + 16), dict(w=OUT), dict(w=OUT + ext - 16), dict(bias=OUT), dict(bias=OUT + ext - 16),
               dict(res=OUT, ldr=64), dict(res=OUT - ext + 16, ldr=64)):
        assert conv(**kw) == INVALID, kw
    assert conv(x=X, out=X + 128, ldx=128, ldo=128) == INVALID                        # column slices of the same rows
    # extents of 2 GiB or more, without 32- or 64-bit wrap-around
    assert conv(batch=1, h=1 << 12, wd=1 << 12) == INVALID                            # 2^24 rows x 128 B
    assert conv(batch=1, h=3, wd=1, ldx=1 << 30) == INVALID
    assert conv(batch=1, h=3, wd=1, ldo=1 << 30) == INVALID
    assert conv(batch=1, h=1 << 11, wd=1 << 11, upsample=1) == INVALID                # the input fits, the upsampled output does not
    assert conv(batch=1 << 30, h=1 << 30, wd=4) == INVALID
    assert conv(batch=(1 << 31) - 1, h=(1 << 31) - 1, wd=(1 << 31) - 1) == INVALID


# ---------------------------------------------------------------------------------------------------------------- the model
def test_config_errors_name_their_field():
    from photoverse_amd.vae_tiny import TAESD_CONFIG, AutoencoderTiny
    m = AutoencoderTiny()
    for k, v in TAESD_CONFIG.items():
        assert getattr(m.config, k) == v, k
    assert m.config.scaling_factor == 1.0 and m.config.latent_magnitude == 3 and m.config.latent_shift == 0.5
    for field, bad in (("encoder_block_out_channels", (64, 128, 64, 64)), ("decoder_block_out_channels", (32, 32, 32, 32)), ("act_fn", "silu"),
                       ("upsampling_scaling_factor", 4), ("in_channels", 5), ("out_channels", 0), ("latent_channels", 16),
                       ("num_decoder_blocks", (3, 3, 1)), ("num_encoder_blocks", (1, 3))):
        with pytest.raises(ValueError, match=field):
            AutoencoderTiny(**{field: bad})
    small = AutoencoderTiny(num_encoder_blocks=(1, 0, 2, 1), num_decoder_blocks=(2, 1, 0, 1))     # block counts may vary
    assert "decoder.layers.4.conv.0.weight" not in small.state_dict() and "decoder.layers.5.weight" in small.state_dict()
    x = torch.tensor([[-3.0, 0.0, 1.5, 30.0]])
    assert torch.equal(m.scale_latents(x), torch.tensor([[0.0, 0.5, 0.75, 1.0]]))
    assert torch.equal(m.unscale_latents(torch.tensor([0.0, 0.5, 1.0])), torch.tensor([-3.0, 0.0, 3.0]))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.decode(torch.zeros(1, 4, 2, 2))


def test_load_state_dict_round_trips_the_references_state_dict(ref):
    from photoverse_amd.vae_tiny import AutoencoderTiny
    m = AutoencoderTiny()
    sd = ref.state_dict()
    assert set(m.state_dict()) == set(sd) and len(sd) == 134
    m._plans["stale"] = m._packed["stale"] = object()
    r = m.load_state_dict(sd)                                                         # strict
    assert not r.missing_keys and not r.unexpected_keys and not m._plans and not m._packed
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "decoder.layers.6.weight"})
    w, b = m._wb(m.decoder.layers[0])                                                 # tap-major fp16 [cout][(ky * 3 + kx) * cin + ci], packed once
    assert w.dtype == torch.float16 and w.shape == (64, 36) and b.dtype == torch.float32
    assert torch.equal(w.view(64, 3, 3, 4), sd["decoder.layers.0.weight"].permute(0, 2, 3, 1).half()) and m._wb(m.decoder.layers[0])[0] is w
    assert m._wb(m.decoder.layers[6])[1] is None
    m._plans["stale"] = object()
    m.float()
    assert not m._plans and not m._packed
    dev = torch.device("cpu")
    assert m._plan_key("dec", 2, 8, 8, dev) == ("dec", 2, 8, 8, dev) and m._plan_key("enc", 1, 16, 16, dev) != m._plan_key("dec", 1, 16, 16, dev)
    assert m._sub_batch(4, 512, 512) == 4 and m._sub_batch(64, 1024, 1024) == 8 and m._sub_batch(2, 1 << 14, 1 << 14) == 1


def test_generate_flag_reaches_run_inference_as_the_vae():
    import importlib.util
    from photoverse_amd.vae_tiny import AutoencoderTiny
    spec = importlib.util.spec_from_file_location("pv_generate_vae_tiny", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)

    class KL:
        calls = []

        def enable_flash_attention(self):
            self.calls.append("flash")

        def enable_tiling(self, size, overlap):
            self.calls.append("tiling")

    kl, dev = KL(), torch.device("cpu")
    assert gen.parser.parse_args([]).vae_tiny_path is None
    assert gen.select_vae(gen.parser.parse_args([]), kl, dev) is kl                   # without the flag: the loaded VAE, untouched
    assert gen.select_vae(gen.parser.parse_args(["--vae_tiling"]), kl, dev) is kl and KL.calls == ["tiling"]
    a = gen.select_vae(gen.parser.parse_args(["--vae_tiny_path", "random", "--seed", "3"]), kl, dev)
    b = gen.select_vae(gen.parser.parse_args(["--vae_tiny_path", "random", "--seed", "3"]), kl, dev)
    assert isinstance(a, AutoencoderTiny) and a.config.scaling_factor == 1.0 and KL.calls == ["tiling"]
    assert all(torch.equal(p, q) and not p.requires_grad for p, q in zip(a.parameters(), b.parameters()))      # seeded
    for flag in ("--vae_tiling", "--vae_flash_attention"):
        with pytest.raises(SystemExit, match="AutoencoderKL"):
            gen.select_vae(gen.parser.parse_args(["--vae_tiny_path", "random", flag]), kl, dev)
    src = open(os.path.join(ROOT, "generate.py")).read()
    main = src[src.index('if __name__ == "__main__":'):]
    assert "vae = select_vae(args, vae, device)" in main and main.index("select_vae(") < main.index("run_inference(")
    assert re.search(r"run_inference\(example, tokenizer, image_encoder, text_encoder, unet, text_adapter, image_adapter, vae,", main)
    assert "--vae_tiny_path" in gen.parser.format_help() and "--vae_tiny_path" in open(os.path.join(ROOT, "README.md")).read()
    with pytest.raises(FileNotFoundError):
        AutoencoderTiny.from_pretrained(os.path.join(ROOT, "no_such_dir"))


def test_from_pretrained_reads_config_and_weights(tmp_path, ref):
    """``config.json`` (unknown fields ignored, block counts honoured) + ``diffusion_pytorch_model.safetensors`` in diffusers' layout; a file that lacks a
    parameter raises."""
    import json
    from safetensors.torch import save_file
    from photoverse_amd.vae_tiny import AutoencoderTiny
    small = seeded_ref(1, num_encoder_blocks=(1, 1, 2, 1), num_decoder_blocks=(2, 1, 1, 1))
    sd = {k: v.contiguous() for k, v in small.state_dict().items()}
    (tmp_path / "config.json").write_text(json.dumps(dict(_class_name="AutoencoderTiny", num_encoder_blocks=[1, 1, 2, 1], num_decoder_blocks=[2, 1, 1, 1],
                                                          act_fn="relu", force_upcast=False, scaling_factor=1.0)))
    save_file(sd, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    m = AutoencoderTiny.from_pretrained(str(tmp_path))
    assert m.config.num_decoder_blocks == (2, 1, 1, 1) and not hasattr(m.config, "force_upcast")
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and set(m.state_dict()) == set(sd)
    save_file({k: v for k, v in sd.items() if k != "encoder.layers.0.bias"}, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    with pytest.raises(KeyError, match="tiny autoencoder"):
        AutoencoderTiny.from_pretrained(str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps(dict(act_fn="gelu")))
    with pytest.raises(ValueError, match="act_fn"):
        AutoencoderTiny.from_pretrained(str(tmp_path))
