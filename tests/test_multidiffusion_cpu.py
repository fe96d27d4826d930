"""CPU-only tests of windowed denoising (MultiDiffusion; ``window`` / ``hires_window``): the two new symbols in the header, ``_lib.EXT_SIGNATURES`` and the
built library, the C-ABI rejections of ``pv_window_gather`` / ``pv_window_blend``, the window geometry and profiles, the float64 references of
``tests/_multidiffusion_ref.py``, the keyword validation of ``run_inference`` / ``WindowedDenoiseLoop``, the CLI flags, and - on the fp32 oracle alone -
that windowing and the weights move the result by far more than the GPU loop test's tolerance."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from _multidiffusion_ref import blend_ref, canvas_inputs, gather_ref, n_cover, origins_ref, profile_ref, windowed_oracle_loop
from test_guidance_cpu import _Untouchable
from test_pag_cpu import G_TEXT, STEPS, TOL_LOOP, oracle_loop, rel_l2, tiny_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- symbols and ABI
def test_symbols_are_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    from photoverse_amd.build import EXTRA_FLAGS, SOURCES
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    v, i, pi = _lib.c_void_p, _lib.c_int, ctypes.POINTER(ctypes.c_int)
    for name, n_ptr in (("pv_window_gather", 2), ("pv_window_blend", 3)):
        decl = re.search(r"^int32_t\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M | re.S).group(1)
        res, args = _lib.EXT_SIGNATURES[name]
        assert res is i and len(decl.split(",")) == len(args) == n_ptr + 10
        assert args == [v] * n_ptr + [i] * 5 + [pi, i, pi, i, v]
        assert getattr(lib, name).argtypes == args and name not in _lib.SIGNATURES
        assert not re.search(r"^int\s+%s\s*\(" % name, header, flags=re.M)
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    assert "pv_window.hip" in SOURCES and "pv_window.hip" not in EXTRA_FLAGS


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def test_cabi_rejects_bad_arguments_before_touching_the_device(lib):
    """Both launchers validate before their first HIP call and return hipErrorInvalidValue = 1 (no GPU needed).  The device pointers are never
    dereferenced - only the host origin arrays are read; no valid call is sent."""
    INVALID = 1
    CANVAS, WINDOWS, PROFILE = 0x1000000, 0x2000000, 0x3000000             # 16 MiB apart

    def calls(canvas=CANVAS, windows=WINDOWS, profile=PROFILE, batch=2, ch=4, H=24, W=32, S=16, oy=(0, 8), ox=(0, 8, 16), ny=None, nx=None):
        a_oy, a_ox = (None if o is None else _ints(o) for o in (oy, ox))
        ny = (0 if oy is None else len(oy)) if ny is None else ny
        nx = (0 if ox is None else len(ox)) if nx is None else nx
        return (lib.pv_window_gather(canvas, windows, batch, ch, H, W, S, a_oy, ny, a_ox, nx, None),
                lib.pv_window_blend(windows, profile, canvas, batch, ch, H, W, S, a_oy, ny, a_ox, nx, None),
                lib.pv_window_blend(windows, None, canvas, batch, ch, H, W, S, a_oy, ny, a_ox, nx, None))

    def bad(**kw):
        return calls(**kw) == (INVALID, INVALID, INVALID)

    assert bad(canvas=None) and bad(windows=None) and bad(oy=None, ny=2) and bad(ox=None, nx=3)
    assert bad(canvas=CANVAS + 2) and bad(windows=WINDOWS + 1)                                     # not 4-byte aligned
    assert calls(profile=PROFILE + 2)[1] == INVALID
    for name in ("batch", "ch", "H", "W", "S"):
        for v in (0, -1):
            assert bad(**{name: v}), (name, v)
    # origins: o[0] == 0, strictly increasing, at most S apart, the last window ends on the extent
    assert bad(oy=(0, 0)) and bad(oy=(8, 0)) and bad(ox=(0, 16, 8)) and bad(ox=(0, 8, 8))          # not increasing
    assert bad(H=40, oy=(0, 24)) and bad(W=49, ox=(0, 16, 33)) and bad(ox=(0, 17), W=33)           # a gap larger than S
    assert bad(oy=(1, 8)) and bad(ox=(4, 8, 16)) and bad(oy=(-8, 8))                               # o[0] != 0
    assert bad(oy=(0, 4)) and bad(ox=(0, 8)) and bad(oy=(0, 8, 16)) and bad(H=25) and bad(W=31)    # the last window short of / beyond the extent
    assert bad(oy=(0,), H=24) and bad(ny=0) and bad(nx=0) and bad(ny=-1)
    # at most 64 windows per axis
    o65 = tuple(range(65))
    assert bad(H=80, oy=o65, ny=65) and bad(W=80, ox=o65, nx=65)
    assert bad(S=33, W=32, ox=(0,), H=40, oy=(0, 7)) and bad(S=25, H=24, oy=(0,), W=32, ox=(0, 7))  # S > W, S > H
    # aliasing: windows (2 * 6 * 4 * 256 floats) and canvas (2 * 4 * 24 * 32) overlap
    assert bad(windows=CANVAS) and bad(windows=CANVAS + 4 * (2 * 4 * 24 * 32 - 1)) and bad(canvas=WINDOWS + 4 * (2 * 6 * 4 * 256 - 1))
    assert calls(profile=CANVAS + 16)[1] == INVALID and calls(profile=WINDOWS + 16)[1] == INVALID
    # 2^29 elements or more, without 64-bit wrap-around
    assert bad(batch=1 << 10, ch=1 << 10, H=32, W=16, S=16, oy=(0, 16), ox=(0,))                   # the canvas
    assert bad(batch=1 << 8, ch=1 << 5, H=1009, W=64, S=64, oy=tuple(range(0, 946, 15)), ox=(0,))   # canvas 2^13 * 1009 * 64 < 2^29 < windows 2^13 * 64 * 4096
    m = (1 << 31) - 1
    assert bad(batch=m, ch=m) and bad(batch=1 << 16, ch=1 << 16, H=1 << 16, W=1 << 16, S=16)


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_window_origins_against_brute_force_and_coverage():
    from photoverse_amd import window_origins as exported
    from photoverse_amd.multidiffusion import window_origins
    assert exported is window_origins
    assert window_origins(20, 16, 8) == (0, 4) and window_origins(18, 16, 8) == (0, 2) and window_origins(16, 16, 8) == (0,)
    assert window_origins(24, 16, 8) == (0, 8) and window_origins(32, 16, 8) == (0, 8, 16) and window_origins(128, 64, 32) == (0, 32, 64)
    for size in range(1, 23):
        for window in range(1, size + 1):
            for stride in range(1, window + 1):
                o = window_origins(size, window, stride)
                assert o == origins_ref(size, window, stride), (size, window, stride)
                assert o[0] == 0 and o[-1] + window == size and all(0 < b - a <= window for a, b in zip(o, o[1:]))
                assert all(any(a <= p < a + window for a in o) for p in range(size))               # every position is covered
    assert len(window_origins(64, 1, 1)) == 64 and len(window_origins(130, 4, 2)) == 64
    for bad in ((65, 1, 1), (131, 4, 2), (16, 17, 8), (16, 8, 9), (16, 8, 0), (0, 0, 0), (16, 8, -1), (16.0, 8, 4), (16, "8", 4), (16, 8, True)):
        with pytest.raises(ValueError, match="window_origins"):
            window_origins(*bad)


def test_window_profile_is_positive_and_symmetric():
    from photoverse_amd.multidiffusion import window_profile
    for S in (1, 2, 3, 16, 17, 64, 128):
        u, g = window_profile("uniform", S), window_profile("gaussian", S)
        assert u.dtype == g.dtype == torch.float32 and u.shape == g.shape == (S,)
        assert torch.equal(u, torch.ones(S)) and (g > 0).all() and torch.isfinite(g).all() and torch.equal(g, g.flip(0))
        i = torch.arange(S, dtype=torch.float64)
        assert torch.equal(g, torch.exp(-(((i - (S - 1) / 2) / S) ** 2) / 0.02).float())
        assert (g - profile_ref("gaussian", S)).abs().max() <= 2.0 ** -24 and torch.equal(u, profile_ref("uniform", S))     # the loop reference's own profile
        if S > 2:
            assert g[S // 2] == g.max() and g[0] == g.min() and g[0] < g[S // 2]
    assert 1e-6 < window_profile("gaussian", 64)[0].item() < 1e-5                                  # exp(-(31.5 / 64)^2 / 0.02) = 5.5e-6
    with pytest.raises(ValueError, match="window_weights"):
        window_profile("linear", 16)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="window"):
            window_profile("uniform", bad)


# ---------------------------------------------------------------------------------------------------------------- reference properties
def test_blend_of_a_gather_is_the_canvas_and_one_window_is_a_copy():
    from photoverse_amd.multidiffusion import window_origins, window_profile
    g = torch.Generator().manual_seed(7)
    for B, C, H, W, S, stride in ((1, 1, 2, 2, 2, 1), (1, 1, 3, 5, 2, 1), (2, 4, 20, 18, 16, 8), (2, 4, 24, 32, 16, 8), (1, 4, 32, 32, 16, 4)):
        oy, ox = window_origins(H, S, stride), window_origins(W, S, stride)
        x = torch.randn(B, C, H, W, generator=g)
        win = gather_ref(x, S, oy, ox)
        assert win.shape == (B * len(oy) * len(ox), C, S, S)
        k = len(ox) * (len(oy) - 1) + len(ox) - 1                                                   # the last window of the last sample
        assert torch.equal(win[(B - 1) * len(oy) * len(ox) + k], x[B - 1, :, oy[-1]:, ox[-1]:].double())
        for kind in ("uniform", "gaussian"):
            back = blend_ref(win, x.shape, S, oy, ox, window_profile(kind, S))
            assert (back - x.double()).abs().max().item() <= 1e-14 * x.abs().max().item() * n_cover(H, W, S, oy, ox)
        assert torch.equal(blend_ref(win, x.shape, S, oy, ox, None), blend_ref(win, x.shape, S, oy, ox, window_profile("uniform", S)))
    assert n_cover(3, 5, 2, (0, 1), (0, 1, 2, 3)) == 4 and n_cover(32, 32, 16, window_origins(32, 16, 4), window_origins(32, 16, 4)) == 16
    x = torch.randn(2, 3, 8, 8, generator=g)
    one = gather_ref(x, 8, (0,), (0,))
    assert torch.equal(one, x.double())
    for prof in (None, window_profile("gaussian", 8)):
        assert (blend_ref(one, x.shape, 8, (0,), (0,), prof) - x.double()).abs().max().item() <= 1e-15 * x.abs().max().item()
    assert torch.equal(blend_ref(one, x.shape, 8, (0,), (0,), None), x.double())
    # disjoint tiles: a reassembly
    tiles = gather_ref(x, 4, (0, 4), (0, 4))
    assert torch.equal(tiles[5], x[1, :, 0:4, 4:8].double()) and torch.equal(blend_ref(tiles, x.shape, 4, (0, 4), (0, 4)), x.double())


# ---------------------------------------------------------------------------------------------------------------- validation
def test_run_inference_keywords_are_validated_before_a_model_runs():
    from photoverse_amd.infer import run_inference
    sig = inspect.signature(run_inference).parameters
    for name, default in (("window", None), ("window_stride", None), ("window_weights", "uniform"), ("hires_window", None), ("hires_window_stride", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(guidance_scale=5.0, timesteps=4)
    mask, img = torch.ones(1, 1, 128, 256), torch.zeros(1, 3, 128, 256)
    for bad, match in ((dict(latent_size=(16, 32)), "needs window"), (dict(latent_size=16, window_stride=8), "window_stride needs window"),
                       (dict(latent_size=16, hires_window_stride=8), "hires_window_stride needs hires_window"),
                       (dict(latent_size=16, hires_window=16), "hires_window needs hires_latent_size"),
                       (dict(latent_size=16, window=16, window_weights="linear"), "window_weights"),
                       (dict(latent_size=16, window_weights="linear"), "window_weights"),
                       (dict(latent_size=(16, 32), window=17), "larger than the canvas"), (dict(latent_size=(16, 32), window=0), "window"),
                       (dict(latent_size=(16, 32), window=16.0), "window"), (dict(latent_size=(16, 32), window=16, window_stride=17), "window_stride"),
                       (dict(latent_size=(16, 32), window=16, window_stride=0), "window_stride"), (dict(latent_size=(16, 32, 4), window=16), "canvas"),
                       (dict(latent_size=(16.0, 32), window=16), "canvas"), (dict(latent_size=(128, 32), window=2, window_stride=1), "more than 64"),
                       (dict(latent_size=(16, 32), window=16, inpaint_mask=mask), "rectangular.*inpaint_mask"),
                       (dict(latent_size=(16, 32), window=16, from_noised_image=True), "rectangular.*from_noised_image"),
                       (dict(latent_size=(16, 32), window=16, controlnet=u, control_image=img), "rectangular.*controlnet"),
                       (dict(latent_size=(16, 32), window=16, hires_latent_size=64), "rectangular.*hires_latent_size"),
                       (dict(latent_size=16, hires_latent_size=32, hires_window=33), "larger than the canvas"),
                       (dict(latent_size=16, hires_latent_size=32.0, hires_window=16), "hires_latent_size"),
                       (dict(latent_size=16, window=16, sampler="sde-dpmsolver++"), "sde-dpmsolver"),
                       (dict(latent_size=16, hires_latent_size=32, hires_window=16, sampler="sde-dpmsolver++"), "sde-dpmsolver"),
                       (dict(latent_size=16, window=16, training_mode=True), "training_mode"),
                       (dict(latent_size=16, hires_latent_size=32, hires_window=16, training_mode=True), "training_mode")):
        with pytest.raises(ValueError, match=match):
            run_inference(*args, **bad, **kw)
    # legal: past the validation, the next thing is the first touch of a model argument
    for good in (dict(latent_size=16), dict(latent_size=(16, 32), window=16), dict(latent_size=(32, 32), window=16, window_stride=16),
                 dict(latent_size=24, window=16, window_weights="gaussian"), dict(latent_size=16, hires_latent_size=32, hires_window=16),
                 dict(latent_size=(16, 16), window=16, hires_latent_size=32, hires_window=16, hires_window_stride=4)):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)


def test_windowed_loop_refuses_before_any_device_work():
    """``WindowedDenoiseLoop`` validates its geometry, the weights and the two refused modes before the UNet is looked at (an untouchable stand-in)."""
    from photoverse_amd import WindowedDenoiseLoop as exported
    from photoverse_amd.multidiffusion import WindowedDenoiseLoop, window_grid
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    assert exported is WindowedDenoiseLoop
    sig = inspect.signature(WindowedDenoiseLoop.__init__).parameters
    assert list(sig)[1:8] == ["unet", "batch", "canvas", "window", "n_ip", "num_steps", "guidance_scale"]
    for name, default in (("window_stride", None), ("window_weights", "uniform"), ("inner", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    u = _Untouchable()
    for kw, match in ((dict(stochastic=True), "stochastic"), (dict(scheduler=DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")), "stochastic"),
                      (dict(training_mode=True), "training_mode"), (dict(window_weights="linear"), "window_weights"), (dict(window_stride=17), "window_stride")):
        with pytest.raises(ValueError, match=match):
            WindowedDenoiseLoop(u, 2, (24, 32), 16, 1, 4, 5.0, **kw)
    for canvas, window in (((24, 8), 16), (15, 16), ((24, 32, 1), 16), ("24", 16), ((24, 32), 0)):
        with pytest.raises(ValueError):
            WindowedDenoiseLoop(u, 2, canvas, window, 1, 4, 5.0)
    import types
    stand_in = types.SimpleNamespace(stochastic=False, training_mode=False)
    with pytest.raises(ValueError, match="inner comes with its own options.*freeu"):       # options beside a ready inner loop would be ignored
        WindowedDenoiseLoop(u, 2, (24, 32), 16, 1, 4, 5.0, inner=stand_in, freeu=(1.5, 1.6, 0.9, 0.2))
    with pytest.raises(ValueError, match="stochastic"):
        WindowedDenoiseLoop(u, 2, (24, 32), 16, 1, 4, 5.0, inner=types.SimpleNamespace(stochastic=True, training_mode=False))
    with pytest.raises(AssertionError, match="touched a model argument"):      # legal: the inner DenoiseLoop is the first to look at the UNet
        WindowedDenoiseLoop(u, 2, (24, 32), 16, 1, 4, 5.0, window_weights="gaussian")
    assert window_grid((24, 32), 16) == (24, 32, 16, 8, (0, 8), (0, 8, 16)) and window_grid(20, 16, 8)[4:] == ((0, 4), (0, 4))
    assert window_grid(3, 1) == (3, 3, 1, 1, (0, 1, 2), (0, 1, 2))                                 # window // 2 == 0 -> stride 1


def test_ops_wrappers_have_no_cpu_path():
    from photoverse_amd.ops import window_blend, window_gather
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        window_gather(x, 2, (0, 2), (0, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        window_blend(torch.zeros(4, 1, 2, 2), x, 2, (0, 2), (0, 2))


def test_cli_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_window", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert (d.window, d.window_stride, d.window_weights, d.hires_window, d.hires_window_stride, d.latent_height, d.latent_width) == (None, None, "uniform",
                                                                                                                                 None, None, None, None)
    assert gen.canvas_size(d) == 64
    a = gen.parser.parse_args(["--latent_size", "16", "--latent_width", "32", "--window", "16", "--window_stride", "8", "--window_weights", "gaussian",
                               "--hires_window", "16", "--hires_window_stride", "4"])
    assert (a.window, a.window_stride, a.window_weights, a.hires_window, a.hires_window_stride) == (16, 8, "gaussian", 16, 4)
    assert gen.canvas_size(a) == (16, 32)
    assert gen.canvas_size(gen.parser.parse_args(["--latent_size", "16", "--latent_height", "24", "--window", "16"])) == (24, 16)
    with pytest.raises(SystemExit, match="need --window"):
        gen.canvas_size(gen.parser.parse_args(["--latent_width", "32"]))
    with pytest.raises(SystemExit):
        gen.parser.parse_args(["--window_weights", "linear"])
    assert "--window" in open(os.path.join(ROOT, "README.md")).read()


# ---------------------------------------------------------------------------------------------------------------- the precondition, on the oracle alone
@torch.no_grad()
def test_windowing_and_weights_move_the_oracle_loop_by_far_more_than_the_loop_tolerance():
    """The precondition of the GPU loop test, on the fp32 oracle alone: tiny model under ``torch.manual_seed(0)``, conditioning of generator seed 81,
    B = 2, canvas 24 x 32, window 16, stride 8, 4 steps, guidance 5.  The windowed loop differs from the plain loop on the same canvas, and gaussian
    weights from uniform ones, by more than 4 x TOL_LOOP each - so a loop that ignored the windows or the weights could not pass the GPU test.
    Measured on the CPU (printed with -s): windowed against plain 1.449e-1, gaussian against uniform 1.470e-1."""
    ref = tiny_oracle()
    cond, uncond, noise = canvas_inputs(24, 32)
    plain = oracle_loop(ref, None, cond, uncond, noise, G_TEXT)
    uni = windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "uniform", STEPS)
    gau = windowed_oracle_loop(ref, cond, uncond, noise, G_TEXT, 16, 8, "gaussian", STEPS)
    d_plain, d_gauss = rel_l2(uni, plain), rel_l2(gau, uni)
    print(f"oracle loops on 24 x 32, window 16 stride 8: windowed vs plain rel-L2 = {d_plain:.3e}, gaussian vs uniform = {d_gauss:.3e}")
    assert torch.isfinite(uni).all() and torch.isfinite(gau).all() and uni.shape == noise.shape
    assert d_plain > 4 * TOL_LOOP and d_gauss > 4 * TOL_LOOP
