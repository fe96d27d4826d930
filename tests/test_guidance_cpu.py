"""CPU-only tests of the separate identity / prompt guidance scales and ``guidance_rescale``: the new symbol in the header, ``_lib.SIGNATURES`` and the
built library, the C-ABI rejections of ``pv_cfg_dpm_step_guided``, the validation of the two keywords of ``run_inference``, the loader's answer to a
library that lacks a symbol, the CLI flags, and the fp64 restatement of the launcher's formulas (the reference of ``tests/test_guidance_gpu.py``)."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: (B, C, H, W) of the kernel test: fewer float4s than one wave; ragged (36 float4s) with an odd batch; the tiny loop's shape; rectangular; several
#: grid-stride trips of a 1024-thread workgroup
SHAPES = [(1, 4, 4, 4), (3, 4, 6, 6), (2, 4, 16, 16), (5, 4, 24, 40), (2, 4, 64, 64)]


def guided_eps_ref(eu, em, ec, g_text, g_image, rescale):
    """The header's guided prediction in fp64 on the given (fp32) values -> ``(e, f)``: ``e`` already multiplied by the per-sample factor ``f`` (B,).
    ``em`` None: the two-term formula.  The standard deviation is the population one (the divisor cancels in the ratio)."""
    eu, ec = eu.double(), ec.double()
    if em is None:
        e = eu + g_text * (ec - eu)
    else:
        e = eu + g_image * (em.double() - eu) + g_text * (ec - em.double())
    B = e.shape[0]
    f = torch.ones(B, dtype=torch.float64)
    if rescale > 0:
        sc, se = ec.reshape(B, -1).std(dim=1, unbiased=False), e.reshape(B, -1).std(dim=1, unbiased=False)
        f = torch.where(se > 0, rescale * sc / se.clamp_min(1e-300) + (1 - rescale), f)
    return f.view(B, *([1] * (e.dim() - 1))) * e, f


def guided_step_ref(eu, em, ec, x, x0_prev, row, g_text, g_image=None, rescale=0.0, mask=None, known=None, noise=None):
    """``pv_cfg_dpm_step_guided`` in fp64 -> ``(latents', x0, f)``; ``row`` = the coefficient row {ca, cb, cx, c0, c1, q0, q1, -}."""
    ca, cb, cx, c0, c1, q0, q1 = row.double()[:7]
    e, f = guided_eps_ref(eu, em, ec, g_text, g_image, rescale)
    x0 = ca * x.double() + cb * e
    xn = cx * x.double() + c0 * x0 + c1 * x0_prev.double()
    if mask is not None:
        m = mask.double()
        xn = m * xn + (1 - m) * (q0 * known.double() + q1 * noise.double())
    return xn, x0, f


def make_eps(shape, g):
    """``(eu, em, ec)`` fp32 with per-sample means of +-3 (signs alternate over the samples and differ between the three) and per-sample standard
    deviations spread over [0.1, 2]: a one-pass variance (E[x^2] - E[x]^2 in fp32 at mean^2 / var up to 900) or a factor taken from the wrong sample shows."""
    B = shape[0]
    out = []
    for k in range(3):
        sign = torch.tensor([1.0 if (b + k) % 2 == 0 else -1.0 for b in range(B)])
        sd = torch.tensor([0.1 + 1.9 * (((b * 3 + k * 2) % 7) / 6.0) for b in range(B)])
        t = torch.randn(shape, generator=g) * sd.view(B, 1, 1, 1) + 3.0 * sign.view(B, 1, 1, 1)
        out.append(t.contiguous())
    return out


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    assert re.search(r"^int\s+pv_cfg_dpm_step_guided\s*\(", header, flags=re.M)
    assert "pv_cfg_dpm_step_guided" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pv_cfg_dpm_step_guided"]
    assert len(args) == 17 and args[7:10] == [_lib.c_float] * 3 and args[13:16] == [_lib.c_int] * 3
    assert lib.pv_cfg_dpm_step_guided is not None
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))


def test_cabi_rejects_bad_guided_step_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  No valid call is sent: ``eps_image`` NULL
    and an absent mask triple are legal, so they only appear together with something illegal."""
    INVALID = 1
    EU, EM, EC, LAT, X0P, COEF, STATE, MASK, KNOWN, NOISE = (0x10000 * (i + 1) for i in range(10))     # never dereferenced: the checks come first

    def call(eu=EU, em=EM, ec=EC, lat=LAT, x0p=X0P, coef=COEF, state=STATE, g_text=7.5, g_image=3.0, rescale=0.7, mask=MASK, known=KNOWN, noise=NOISE,
             batch=2, channels=4, hw=256):
        return lib.pv_cfg_dpm_step_guided(eu, em, ec, lat, x0p, coef, state, g_text, g_image, rescale, mask, known, noise, batch, channels, hw, None)

    for name in ("eu", "ec", "lat", "x0p", "coef", "state"):
        assert call(**{name: None}) == INVALID, name
        assert call(**{name: None}, em=None, mask=None, known=None, noise=None, rescale=0.0) == INVALID, name
    for name in ("batch", "channels", "hw"):
        for v in (0, -1, -16):
            assert call(**{name: v}) == INVALID, (name, v)
    for hw in (1, 2, 3, 6, 255, 258):
        assert call(hw=hw) == INVALID, hw
    for part in (dict(mask=None), dict(known=None), dict(noise=None), dict(mask=None, known=None), dict(mask=None, noise=None),
                 dict(known=None, noise=None)):
        assert call(**part) == INVALID, part
    for r in (-0.1, -1e-6, 1.0001, 2.0, math.nan, math.inf, -math.inf):
        assert call(rescale=r) == INVALID, r
    for bad in (math.nan, math.inf, -math.inf):
        assert call(g_text=bad) == INVALID and call(g_image=bad) == INVALID, bad
        assert call(g_text=bad, em=None) == INVALID and call(g_image=bad, em=None) == INVALID, bad
    # 2 Gi elements or more, also where the product overflows 32 or 64 bits
    assert call(batch=2, channels=4, hw=1 << 28) == INVALID                   # exactly 2^31
    assert call(batch=1, channels=1 << 16, hw=1 << 15) == INVALID             # chw alone is 2^31
    m = (1 << 31) - 1
    assert call(batch=1, channels=m, hw=m - 3) == INVALID
    assert call(batch=m, channels=m, hw=m - 3) == INVALID
    assert call(batch=m, channels=1, hw=4) == INVALID
    assert call(batch=1 << 16, channels=1 << 16, hw=1 << 16) == INVALID       # 2^48


class _Untouchable:
    """Stands for a model: any attribute access, call or item access is the failure the test looks for."""

    def __getattr__(self, name):
        raise AssertionError(f"run_inference touched a model argument (.{name}) before validating its keywords")

    def __call__(self, *a, **kw):
        raise AssertionError("run_inference called a model argument before validating its keywords")

    def __getitem__(self, k):
        raise AssertionError("run_inference indexed a model argument before validating its keywords")

    def __contains__(self, k):
        raise AssertionError("run_inference searched a model argument before validating its keywords")


def test_run_inference_validates_the_guidance_keywords_before_touching_a_model():
    import inspect
    from photoverse_amd.infer import run_inference
    sig = inspect.signature(run_inference).parameters
    for name, default in (("image_guidance_scale", None), ("guidance_rescale", 0.0)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=7.5, timesteps=4)
    for bad in (math.nan, math.inf, -math.inf, "3", True, [3.0], 1 + 2j):
        with pytest.raises(ValueError, match="image_guidance_scale"):
            run_inference(*args, image_guidance_scale=bad, **kw)
    for bad in (-0.1, 1.5, math.nan, math.inf, "0.5", None, True):
        with pytest.raises(ValueError, match="guidance_rescale"):
            run_inference(*args, guidance_rescale=bad, **kw)
    with pytest.raises(ValueError, match="image_guidance_scale.*training_mode"):
        run_inference(*args, image_guidance_scale=3.0, training_mode=True, **kw)
    with pytest.raises(ValueError, match="guidance_rescale.*training_mode"):
        run_inference(*args, guidance_rescale=0.5, training_mode=True, **kw)
    with pytest.raises(ValueError, match="training_mode"):                   # also when the scale equals guidance_scale
        run_inference(*args, image_guidance_scale=7.5, training_mode=True, **kw)
    # legal values get past the validation: the next thing is the first touch of a model argument
    for good in (dict(image_guidance_scale=3.0, guidance_rescale=0.7), dict(image_guidance_scale=-1, guidance_rescale=1), dict(guidance_rescale=0)):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)


def test_a_library_without_a_declared_symbol_is_refused_by_name(lib, monkeypatch):
    """``PV_ABI_VERSION`` stayed 19 when the symbol was added, so a library built before it passes the version check: the binding loop must say which
    symbol is missing and that the library has to be rebuilt, as ``HipExtensionMissing`` - not ``AttributeError``."""
    from photoverse_amd import _lib
    sigs = dict(_lib.SIGNATURES)
    sigs["pv_symbol_of_a_newer_package"] = (_lib.c_int, [_lib.c_void_p])
    monkeypatch.setattr(_lib, "SIGNATURES", sigs)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.HipExtensionMissing, match="pv_symbol_of_a_newer_package") as ei:
        _lib.load()
    assert "rebuild" in str(ei.value)
    assert _lib._lib is None                          # nothing half-bound is kept
    monkeypatch.undo()
    assert _lib.load() is lib


def test_cli_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_guidance", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.image_guidance_scale is None and d.guidance_rescale == 0.0
    a = gen.parser.parse_args(["--guidance_scale", "7.5", "--image_guidance_scale", "2", "--guidance_rescale", "0.5"])
    assert (a.guidance_scale, a.image_guidance_scale, a.guidance_rescale) == (7.5, 2.0, 0.5)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_reduces_to_plain_cfg_and_to_factor_one(shape):
    """``guided_step_ref``: equal scales are the two-term formula (1e-12: the same polynomial, summed in another order in fp64), ``rescale == 0`` is
    ``f == 1`` exactly, ``rescale == 1`` gives every sample the standard deviation of its ``eps_cond``, and an all-zero sample keeps ``f == 1``."""
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(sum(shape))
    eu, em, ec = make_eps(shape, g)
    x, xp, known, noise = (torch.randn(shape, generator=g) for _ in range(4))
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(6)
    coef = sch.coefficient_table(0, blend=True)
    B = shape[0]
    for r in (0, 3, 5):
        row = coef[r]
        plain, plain_x0, f0 = guided_step_ref(eu, None, ec, x, xp, row, 7.5)
        same, same_x0, f1 = guided_step_ref(eu, em, ec, x, xp, row, 7.5, 7.5)
        assert torch.equal(f0, torch.ones(B, dtype=torch.float64)) and torch.equal(f1, f0)
        e = eu.double() + 7.5 * (ec.double() - eu.double())
        x0 = row[0].double() * x.double() + row[1].double() * e
        exp = row[2].double() * x.double() + row[3].double() * x0 + row[4].double() * xp.double()
        assert torch.equal(plain, exp) and torch.equal(plain_x0, x0)
        torch.testing.assert_close(same, plain, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(same_x0, plain_x0, rtol=1e-12, atol=1e-12)
    e1, f = guided_eps_ref(eu, em, ec, 7.5, 3.0, 1.0)
    torch.testing.assert_close(e1.reshape(B, -1).std(dim=1, unbiased=False), ec.double().reshape(B, -1).std(dim=1, unbiased=False), rtol=1e-12, atol=0)
    if B > 1:
        assert f.unique().numel() == B                 # a factor per sample
    z = torch.zeros(shape)
    _, fz = guided_eps_ref(z, z, z, 7.5, 3.0, 0.7)
    assert torch.equal(fz, torch.ones(B, dtype=torch.float64))
    m = torch.zeros(B, 1, *shape[2:])
    kept, _, _ = guided_step_ref(eu, em, ec, x, xp, coef[3], 7.5, 3.0, 0.7, m, known, noise)
    assert torch.equal(kept, coef[3, 5].double() * known.double() + coef[3, 6].double() * noise.double())
