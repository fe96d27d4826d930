"""CPU-only tests of the Real-ESRGAN upscaler: the ``pv_dense_conv3x3`` symbol in the header / binding / library and its C-ABI
rejections, ``RRDBNet``'s key names, parameter count and weight files, the tile grid, the inputs of ``tests/test_upscaler_gpu.py`` checked against their
bounds on the reference alone, and the ``generate.py`` flags."""
import os
import re

import pytest
import torch

from _rrdb_ref import (IMAGE_ULPS, KERNEL_BOUND, KERNEL_FORMS, KERNEL_SHAPES, MODEL_BLOCKS, MODEL_CASES, TILE_CASE, TOL, WALK_FORMS, WALK_SHAPE,
                       WALK_SHAPE_UPSAMPLE, RRDBNetRef, dense_conv_ref, element_bound, half_ulp_fp16, kernel_case, pixels_case, rel_l2, seeded_ref,
                       tile_process_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the symbol
def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib, ops
    from photoverse_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_dense_conv3x3\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_dense_conv3x3"]
    v, i, f = _lib.c_void_p, _lib.c_int, _lib.c_float
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 21
    assert args == [v, i, v, v, v, i, v, i, v, i, i, i, i, i, i, i, i, f, f, f, v]
    assert lib.pv_dense_conv3x3.argtypes == args and "pv_dense_conv3x3" not in _lib.SIGNATURES
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    assert "pv_denseconv.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "photoverse_amd", "csrc", "pv_denseconv.hip"))
    assert ops.ACT_LEAKY_RELU == 3 == int(re.search(r"PV_ACT_LEAKY_RELU = (\d+)", header).group(1))
    assert callable(ops.Recorder.dense_conv)
    import photoverse_amd
    from photoverse_amd.upscaler import RRDBNet
    assert photoverse_amd.RRDBNet is RRDBNet


def test_cabi_rejects_bad_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  The pointers are never dereferenced; no valid
    call is sent."""
    INVALID = 1
    X, W, B, R, R2, OUT = 0x10000000, 0x20000000, 0x28000000, 0x30000000, 0x38000000, 0x40000000
    LEAKY = 3

    def conv(x=X, ldx=192, w=W, bias=B, res=None, ldr=0, res2=None, ldr2=0, out=OUT, ldo=64, batch=2, cin=192, cout=64, h=9, wd=17, upsample=0, act=0,
             slope=0.2, alpha=1.0, beta=1.0):
        return lib.pv_dense_conv3x3(x, ldx, w, bias, res, ldr, res2, ldr2, out, ldo, batch, cin, cout, h, wd, upsample, act, slope, alpha, beta, None)

    for name in ("x", "w", "out"):
        assert conv(**{name: None}) == INVALID, name
    for name in ("x", "w", "bias", "out"):
        assert conv(**{name: 0x50000008}) == INVALID, name                            # 8-byte aligned only
    assert conv(res=R + 8, ldr=64) == INVALID and conv(res=R, ldr=64, res2=R2 + 8, ldr2=64) == INVALID
    for bad in (0, -192, 64, 184, 191, 196):                                          # below the width read; not a multiple of 8
        assert conv(ldx=bad) == INVALID, bad
    for bad in (0, -64, 32, 56, 63, 68):
        assert conv(ldo=bad) == INVALID, bad
        assert conv(res=R, ldr=bad) == INVALID, bad
        assert conv(res=R, ldr=64, res2=R2, ldr2=bad) == INVALID, bad
    for bad in (0, 32, 48, 72, 100, 224, 256, -64):
        assert conv(cin=bad, ldx=256) == INVALID, bad
    for bad in (0, 16, 48, 96, 128, -32):
        assert conv(cout=bad, ldo=128) == INVALID, bad
    for bad in (2, -1):
        assert conv(cin=64, upsample=bad) == INVALID, bad
    assert conv(cin=96, upsample=1) == INVALID and conv(cin=64, cout=32, upsample=1) == INVALID and conv(upsample=1) == INVALID   # upsample is 64 -> 64
    for bad in (1, 2, 4, 5, 6, -1):                                                   # only PV_ACT_NONE (0) and PV_ACT_LEAKY_RELU (3)
        assert conv(act=bad) == INVALID, bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert conv(act=LEAKY, slope=bad) == INVALID and conv(res=R, ldr=64, alpha=bad) == INVALID, bad
        assert conv(res=R, ldr=64, res2=R2, ldr2=64, beta=bad) == INVALID, bad
        assert conv(slope=bad) == INVALID and conv(alpha=bad) == INVALID and conv(beta=bad) == INVALID, bad       # also where the value is not used
    assert conv(res2=R2, ldr2=64) == INVALID                                          # res2 needs res
    for name in ("batch", "h", "wd"):
        for bad in (0, -1):
            assert conv(**{name: bad}) == INVALID, (name, bad)
    # out overlaps something the launch reads: the weight, the bias, a residual, the input - the same buffer, or by one element at either end
    ext = ((2 * 9 * 17 - 1) * 64 + 64) * 2
    xext = ((2 * 9 * 17 - 1) * 192 + 192) * 2
    for kw in (dict(w=OUT), dict(w=OUT + ext - 16), dict(bias=OUT), dict(bias=OUT + ext - 16), dict(res=OUT, ldr=64), dict(res=OUT - ext + 16, ldr=64),
               dict(res=R, ldr=64, res2=OUT, ldr2=64), dict(res=R, ldr=64, res2=OUT + ext - 16, ldr2=64), dict(res=R, ldr=64, res2=R, ldr2=64),
               dict(res=R, ldr=64, res2=R + ext - 16, ldr2=64), dict(x=OUT, ldx=192), dict(x=OUT + ext - 16), dict(x=OUT - xext + 16)):
        assert conv(**kw) == INVALID, kw
    # the in-place dense block: out may be a column slice of x's rows - at or behind column cin, inside the row, with x's leading dimension - and only that
    for cin, bad_off in ((64, 0), (64, 32), (64, 56), (96, 64), (160, 128), (128, 168), (64, 192), (64, 192 * 3 + 64)):
        assert conv(cin=cin, cout=32, out=X + 2 * bad_off, ldo=192) == INVALID, (cin, bad_off)
    assert conv(cin=64, cout=32, ldx=192, out=X + 128, ldo=200) == INVALID            # another leading dimension: not the same rows
    assert conv(cin=64, cout=64, ldx=192, out=X + 2 * 136, ldo=192) == INVALID        # the slice would run past the row's end
    assert conv(cin=64, res=X + 2 * 32, ldr=192, out=X + 128, ldo=192, ldx=192) == INVALID       # res may sit in x's rows, but not in out's columns
    # extents of 2 GiB or more, without 32- or 64-bit wrap-around
    assert conv(batch=1, h=1 << 12, wd=1 << 11) == INVALID                            # 2^23 rows x 384 B
    assert conv(batch=1, h=3, wd=1, ldx=1 << 30) == INVALID
    assert conv(batch=1, h=3, wd=1, ldo=1 << 30) == INVALID
    assert conv(batch=1, h=3, wd=1, res=R, ldr=1 << 30) == INVALID
    assert conv(batch=1, h=3, wd=1, res=R, ldr=64, res2=R2, ldr2=1 << 30) == INVALID
    assert conv(batch=1, h=1 << 11, wd=1 << 11, cin=64, ldx=64, upsample=1) == INVALID       # the input fits, the upsampled output does not
    assert conv(batch=1 << 30, h=1 << 30, wd=4) == INVALID
    assert conv(batch=(1 << 31) - 1, h=(1 << 31) - 1, wd=(1 << 31) - 1) == INVALID


# ---------------------------------------------------------------------------------------------------------------- the model
def _count(nb):
    rdb = (64 + 96 + 128 + 160) * 32 * 9 + 4 * 32 + 192 * 64 * 9 + 64
    return (3 * 64 * 9 + 64) + 3 * nb * rdb + 4 * (64 * 64 * 9 + 64) + (64 * 3 * 9 + 3)


@pytest.mark.parametrize("nb", [23, 6])
def test_key_names_and_parameter_count(nb):
    from photoverse_amd.upscaler import RRDBNet
    m, ref = RRDBNet(num_block=nb), RRDBNetRef(nb)
    sd = m.state_dict()
    assert list(sd) == list(ref.state_dict()) and all(sd[k].shape == v.shape for k, v in ref.state_dict().items())
    names = {"conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"}
    names |= {f"body.{n}.rdb{r}.conv{c}" for n in range(nb) for r in (1, 2, 3) for c in (1, 2, 3, 4, 5)}
    assert set(sd) == {f"{n}.{p}" for n in names for p in ("weight", "bias")}
    assert sum(p.numel() for p in m.parameters()) == _count(nb)
    assert _count(23) == 16697987
    assert sd["body.0.rdb1.conv4.weight"].shape == (32, 160, 3, 3) and sd["body.0.rdb3.conv5.weight"].shape == (64, 192, 3, 3)
    with pytest.raises(ValueError, match="num_block"):
        RRDBNet(num_block=0)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.upscale(torch.zeros(1, 3, 2, 2))


def test_weight_files_round_trip(tmp_path):
    """``.pth`` with ``params_ema`` (preferred over ``params``), with ``params``, bare; ``.safetensors``; ``num_block`` from the keys; strict both ways."""
    from safetensors.torch import save_file
    from photoverse_amd.upscaler import RRDBNet
    ref, other = seeded_ref(2), seeded_ref(2, seed=1)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    torch.save(dict(params_ema=sd, params=other.state_dict()), tmp_path / "ema.pth")
    torch.save(dict(params=sd), tmp_path / "params.pth")
    torch.save(sd, tmp_path / "bare.pth")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "net.safetensors"))
    for name in ("ema.pth", "params.pth", "bare.pth", "net.safetensors"):
        m = RRDBNet.from_pretrained(str(tmp_path / name))
        assert m.num_block == 2 and set(m.state_dict()) == set(sd), name
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()), name
    torch.save({k: v for k, v in sd.items() if k != "body.1.rdb2.conv3.bias"}, tmp_path / "missing.pth")
    torch.save(dict(sd, extra=torch.zeros(1)), tmp_path / "extra.pth")
    for name in ("missing.pth", "extra.pth"):
        with pytest.raises(RuntimeError):
            RRDBNet.from_pretrained(str(tmp_path / name))
    torch.save(dict(model=torch.zeros(1)), tmp_path / "other.pth")
    with pytest.raises(KeyError, match="RRDBNet"):
        RRDBNet.from_pretrained(str(tmp_path / "other.pth"))
    x2 = dict(sd)
    x2["conv_first.weight"] = torch.zeros(64, 12, 3, 3)                                # the x2 model's pixel-unshuffled input
    torch.save(x2, tmp_path / "x2.pth")
    with pytest.raises(ValueError, match="x4"):
        RRDBNet.from_pretrained(str(tmp_path / "x2.pth"))
    with pytest.raises(FileNotFoundError):
        RRDBNet.from_pretrained(str(tmp_path / "nothing.pth"))
    # the packed weight: tap-major fp16 [cout][(ky * 3 + kx) * cin + ci], packed once, dropped by a new state dict
    m = RRDBNet.from_pretrained(str(tmp_path / "bare.pth"))
    w, b = m._wb(m.body[1].rdb1.conv2)
    assert w.dtype == torch.float16 and w.shape == (32, 9 * 96) and b.dtype == torch.float32 and m._wb(m.body[1].rdb1.conv2)[0] is w
    assert torch.equal(w.view(32, 3, 3, 96), sd["body.1.rdb1.conv2.weight"].permute(0, 2, 3, 1).half())
    m._plans["stale"] = object()
    m.load_state_dict(other.state_dict())
    assert not m._plans and not m._packed
    a, b2 = RRDBNet(num_block=2).randomize_(3), RRDBNet(num_block=2).randomize_(3)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b2.parameters()))    # seeded
    assert not all(torch.equal(p, q) for p, q in zip(a.parameters(), RRDBNet(num_block=2).randomize_(4).parameters()))


# ---------------------------------------------------------------------------------------------------------------- the tile grid
def test_tile_grid_is_real_esrgans_tile_process():
    from photoverse_amd.upscaler import BYTES_PER_PIXEL, RRDBNet, default_tile, tile_grid
    assert tile_grid(12, 20, 8, 1) == [(0, 8, 0, 8, 0, 9, 0, 9), (0, 8, 8, 16, 0, 9, 7, 17), (0, 8, 16, 20, 0, 9, 15, 20),
                                       (8, 12, 0, 8, 7, 12, 0, 9), (8, 12, 8, 16, 7, 12, 7, 17), (8, 12, 16, 20, 7, 12, 15, 20)]
    assert tile_grid(5, 7, 8, 10) == [(0, 5, 0, 7, 0, 5, 0, 7)] == tile_grid(5, 7, 7, 0)            # tile >= image: one tile, the image itself
    assert tile_grid(1, 1, 1, 0) == [(0, 1, 0, 1, 0, 1, 0, 1)]
    for bad in (dict(tile=0), dict(tile=-4), dict(tile_pad=-1), dict(height=0)):
        with pytest.raises(ValueError):
            tile_grid(**dict(dict(height=4, width=4, tile=2, tile_pad=1), **bad))

    def through_grid(fn, img, tile, pad):                                              # what RRDBNet.upscale does with the grid
        out = torch.empty(img.shape[0], 3, 4 * img.shape[2], 4 * img.shape[3])
        for y0, y1, x0, x1, py0, py1, px0, px1 in tile_grid(img.shape[2], img.shape[3], tile, pad):
            o = fn(img[:, :, py0:py1, px0:px1])
            out[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = o[:, :, 4 * (y0 - py0):4 * (y0 - py0) + 4 * (y1 - y0), 4 * (x0 - px0):4 * (x0 - px0) + 4 * (x1 - x0)]
        return out

    ref = seeded_ref(2)
    x = pixels_case(TILE_CASE["shape"])
    whole = ref.upscale(x)
    for tile, pad in ((8, 1), (5, 2), (3, 0), (7, 10), (20, 3), (64, 10)):
        assert torch.equal(through_grid(ref.upscale, x, tile, pad), tile_process_ref(ref.upscale, x, tile, pad)), (tile, pad)
    assert torch.equal(tile_process_ref(ref.upscale, x, 20, 3), whole) and torch.equal(tile_process_ref(ref.upscale, x, 64, 10), whole)   # tile >= image
    # tile=None: the whole image while the 4x-resolution 64-channel fp16 rows stay within MAX_OPERAND_BYTES, else the largest tile that does
    assert BYTES_PER_PIXEL == 2048 and RRDBNet.MAX_OPERAND_BYTES == 1 << 30
    assert default_tile(512, 512, 10, 1 << 30) is None and default_tile(512, 1024, 10, 1 << 30) is None
    t = default_tile(1024, 1024, 10, 1 << 30)
    assert t == 704 and 2048 * (t + 20) ** 2 <= 1 << 30 < 2048 * (t + 21) ** 2
    assert default_tile(12, 20, 1, 2048 * 100) == 8 and default_tile(10, 10, 1, 2048 * 100) is None
    with pytest.raises(ValueError, match="tile_pad"):
        default_tile(12, 20, 5, 2048 * 100)
    m = RRDBNet(num_block=1)
    assert m._sub_batch(4, 512, 512) == 2 and m._sub_batch(1, 512, 512) == 1 and m._sub_batch(4, 64, 64) == 4 and m._sub_batch(3, 1024, 1024) == 1


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' preconditions
def test_the_gpu_tests_inputs_leave_room_under_the_bound():
    """On the reference alone: fp16 weights and one fp16 rounding per launch stay under HALF of ``TOL`` on exactly the model inputs of the GPU tests; the
    tiled result differs from the untiled one by more than 10 x ``TOL`` (so the tiled GPU test cannot pass by computing the untiled image); one launch's
    fp64 result rounded to fp16 once stays under half of the kernel bound and inside the per-element bound's rounding term."""
    for nb in MODEL_BLOCKS:
        ref = seeded_ref(nb)
        for shape in MODEL_CASES:
            x = pixels_case(shape)
            exact = ref.upscale(x)
            err = rel_l2(ref.upscale(x, emulate_fp16=True), exact)
            saturated = float((exact.abs() == 1).float().mean())
            print(f"RRDBNet({nb}) {shape}: fp16-emulated vs fp32 rel-L2 = {err:.3e}, max |activation| = {ref.max_activation:.2f}, clamped = {saturated:.3f}")
            assert exact.shape == (shape[0], 3, 4 * shape[2], 4 * shape[3]) and err < TOL / 2 and ref.max_activation < 1000 and saturated < 0.05
        x = pixels_case(TILE_CASE["shape"])
        diff = rel_l2(tile_process_ref(ref.upscale, x, TILE_CASE["tile"], TILE_CASE["tile_pad"]), ref.upscale(x))
        print(f"RRDBNet({nb}) tiled {TILE_CASE}: vs untiled rel-L2 = {diff:.3e}")
        assert diff >= 10 * TOL
    for form in KERNEL_FORMS:
        walk = [WALK_SHAPE_UPSAMPLE if form == "upsample" else WALK_SHAPE] if form in WALK_FORMS else []
        for shape in KERNEL_SHAPES + walk:
            c = kernel_case(form, *shape)
            exact, mag = dense_conv_ref(c)
            rounded = exact.half().double()
            assert torch.isfinite(exact).all() and (mag >= exact.abs() - 1e-9).all()
            assert rel_l2(rounded, exact) < KERNEL_BOUND / 2, (form, shape)
            # torch rounds fp64 -> fp16 through fp32: a value within 2^-24 |v| of a tie may go the other way, as any fp32 result may
            assert ((rounded - exact).abs() <= half_ulp_fp16(exact) + 2.0 ** -24 * exact.abs()).all(), (form, shape)
            assert (element_bound(exact, mag) >= half_ulp_fp16(exact) + IMAGE_ULPS * exact.abs()).all(), (form, shape)
    assert IMAGE_ULPS == 32 * 2.0 ** -24
    assert torch.equal(half_ulp_fp16(torch.tensor([1.0, 1.5, 2.0, 0.75, 1e-7, 0.0], dtype=torch.float64)),
                       torch.tensor([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25], dtype=torch.float64))


def test_dense_conv_reference_by_hand():
    """One launch against sums written out: tap-major weights, LeakyReLU with the slope 0.2, both scaled residuals, and ``upsample`` = nearest x2 then conv
    with the zero padding outside the UPSAMPLED image."""
    c = kernel_case("conv5_res2", 2, 3, 5)
    y, mag = dense_conv_ref(c)
    x, w4, b = c["x"].double(), c["w"].double().view(64, 3, 3, 192), c["b"].double()
    for (n, oy, ox) in ((0, 0, 0), (1, 2, 4), (1, 1, 2)):
        s = b.clone()
        for ky in range(3):
            for kx in range(3):
                iy, ix = oy + ky - 1, ox + kx - 1
                if 0 <= iy < 3 and 0 <= ix < 5:
                    s += w4[:, ky, kx, :] @ x[n, :, iy, ix]
        exp = 0.2 * (0.2 * s + c["r"].double()[n, :, oy, ox]) + c["r2"].double()[n, :, oy, ox]
        assert torch.allclose(y[n, :, oy, ox], exp, rtol=1e-12, atol=1e-12)
    c = kernel_case("dense96", 1, 1, 1)
    y, _ = dense_conv_ref(c)
    s = c["b"].double() + c["w"].double().view(32, 3, 3, 96)[:, 1, 1, :] @ c["x"].double()[0, :, 0, 0]
    assert torch.allclose(y[0, :, 0, 0], torch.where(s > 0, s, 0.2 * s)) and (s < 0).any() and (s > 0).any()
    c = kernel_case("upsample", 2, 3, 5)
    y, _ = dense_conv_ref(c)
    assert y.shape == (2, 64, 6, 10) and (c["ho"], c["wo"]) == (6, 10)
    x, w4, oy, ox = c["x"].double(), c["w"].double().view(64, 3, 3, 64), 5, 9         # the last output pixel: taps at iy = 6 and ix = 10 are padding
    s = c["b"].double() + sum(w4[:, ky, kx, :] @ x[1, :, (oy + ky - 1) >> 1, (ox + kx - 1) >> 1] for ky in range(3) for kx in range(3)
                              if oy + ky - 1 < 6 and ox + kx - 1 < 10)
    assert torch.allclose(y[1, :, oy, ox], torch.where(s > 0, s, 0.2 * s))


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_generate_flags():
    import importlib.util
    from photoverse_amd.upscaler import RRDBNet
    spec = importlib.util.spec_from_file_location("pv_generate_upscaler", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    parse = gen.parser.parse_args
    d = parse([])
    assert d.upscaler_path is None and d.upscaler_blocks is None and d.upscale_tile is None and d.upscale_tile_pad == 10
    gen.check_upscaler_args(d)
    x = torch.zeros(1, 3, 2, 2)
    assert gen.prepare_upscaler(d, torch.device("cpu")) is None and gen.upscale_images(d, None, x) is x          # without the flag: untouched
    for argv, msg in ((["--upscaler_blocks", "2"], "needs --upscaler_path"), (["--upscale_tile", "64"], "needs --upscaler_path"),
                      (["--upscaler_path", "random", "--upscaler_blocks", "0"], "upscaler_blocks"),
                      (["--upscaler_path", "random", "--upscale_tile", "0"], "upscale_tile"),
                      (["--upscaler_path", "random", "--upscale_tile_pad", "-1"], "upscale_tile_pad"),
                      (["--upscaler_path", os.path.join(ROOT, "no_such_file.pth")], "no file"),
                      (["--upscaler_path", os.path.join(ROOT, "README.md"), "--upscaler_blocks", "6"], "random")):
        with pytest.raises(SystemExit, match=msg):
            gen.check_upscaler_args(parse(argv))
    a = gen.prepare_upscaler(parse(["--upscaler_path", "random", "--upscaler_blocks", "2", "--seed", "3"]), torch.device("cpu"))
    b = gen.prepare_upscaler(parse(["--upscaler_path", "random", "--upscaler_blocks", "2", "--seed", "3"]), torch.device("cpu"))
    assert isinstance(a, RRDBNet) and a.num_block == 2 and all(torch.equal(p, q) and not p.requires_grad for p, q in zip(a.parameters(), b.parameters()))
    assert gen.prepare_upscaler(parse(["--upscaler_path", "random", "--upscaler_blocks", "1"]), torch.device("cpu")).num_block == 1

    class Net:
        def upscale(self, images, tile, tile_pad):
            return ("upscaled", images.dtype, tile, tile_pad)

    assert gen.upscale_images(parse(["--upscaler_path", "random", "--upscale_tile", "64", "--upscale_tile_pad", "4"]), Net(), x.half()) == \
        ("upscaled", torch.float32, 64, 4)
    src = open(os.path.join(ROOT, "generate.py")).read()
    main = src[src.index('if __name__ == "__main__":'):]
    assert main.index("check_upscaler_args(args)") < main.index("load_models(")                                 # bad values exit before any model is loaded
    assert main.index("run_inference(") < main.index("upscale_images(") < main.index("denormalize(")
    for flag in ("--upscaler_path", "--upscaler_blocks", "--upscale_tile", "--upscale_tile_pad"):
        assert flag in gen.parser.format_help(), flag
    assert "--upscaler_path" in open(os.path.join(ROOT, "README.md")).read()
