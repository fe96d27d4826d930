"""CPU-only tests of the stochastic sampler (SDE-DPM-Solver++(2M), ``sampler="sde-dpmsolver++"``): a numpy Philox4x32-10 against known answers, the
SDE rows of ``scheduler.coefficient_table`` against an independent fp64 evaluation and against an exact linear-Gaussian model, the fp64 restatement of
``pv_cfg_dpm_step_stochastic`` (the reference of ``tests/test_sampler_gpu.py``) against a per-element evaluation in plain Python, the host-side
validation, the new symbol, and the ``sample_offset`` the sharded pipeline hands to each rank."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle.philox import box_muller, noise_ref, philox4x32_10  # noqa: F401  (the numpy restatement of the noise; re-exported to the GPU tests)
from test_guidance_cpu import SHAPES, guided_eps_ref, make_eps  # noqa: F401  (SHAPES / make_eps: re-exported to test_sampler_gpu)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDE = "sde-dpmsolver++"


# ---------------------------------------------------------------------------------------------------------------- the SDE rows and the step in fp64
def sde_rows_ref(sigmas, start=0, blend=False):
    """The SDE coefficient rows {ca, cb, cx, c0, c1, q0, q1, cn} in fp64 from the schedule's sigmas (``scheduler.sigmas``: sigma / alpha of the
    variance-preserving form, n + 1 values ending in 0), written from the published update alone:
        x0 = (x - sigma_s eps) / alpha_s;   x' = (sigma_t / sigma_s) e^-h x + alpha_t (1 - e^-2h) (D0 [+ D1 / 2]) + sigma_t sqrt(1 - e^-2h) z
    with D0 = x0, D1 = (x0 - x0_prev) / r0, r0 = h_prev / h, h = lambda_t - lambda_s, lambda = ln(alpha / sigma)."""
    k = np.asarray(sigmas, dtype=np.float64)
    n = len(k) - 1
    alpha = (1.0 + k * k) ** -0.5
    sigma = k * alpha
    rows = np.zeros((n, 8))
    for i in range(n):
        last = i == n - 1
        e_h = 0.0 if last else (sigma[i + 1] / alpha[i + 1]) / (sigma[i] / alpha[i])         # exp(-h) = exp(lambda_s - lambda_t)
        A = alpha[i + 1] * (1.0 - e_h * e_h)
        rows[i, 0], rows[i, 1] = 1.0 / alpha[i], -sigma[i] / alpha[i]
        rows[i, 2] = sigma[i + 1] / sigma[i] * e_h
        rows[i, 7] = sigma[i + 1] * math.sqrt(1.0 - e_h * e_h)
        if i <= start or last:
            rows[i, 3], rows[i, 4] = A, 0.0
        else:
            h = -math.log(e_h)
            h_prev = math.log(alpha[i] / sigma[i]) - math.log(alpha[i - 1] / sigma[i - 1])
            r0 = h_prev / h
            rows[i, 3], rows[i, 4] = A + 0.5 * A / r0, -0.5 * A / r0
        if blend:
            rows[i, 5], rows[i, 6] = alpha[i + 1], sigma[i + 1]
    return torch.from_numpy(rows)


def stochastic_step_ref(eu, em, ec, x, x0_prev, row, z, g_text, g_image=None, rescale=0.0, mask=None, known=None, noise=None):
    """``pv_cfg_dpm_step_stochastic`` in fp64 -> ``(latents', x0)``: the guided prediction (``test_guidance_cpu.guided_eps_ref``), the step, ``cn * z``,
    then the blend.  ``row`` = {ca, cb, cx, c0, c1, q0, q1, cn}; ``z`` = ``noise_ref`` of the launch."""
    ca, cb, cx, c0, c1, q0, q1, cn = row.double()[:8]
    e, _ = guided_eps_ref(eu, em, ec, g_text, g_image, rescale)
    x0 = ca * x.double() + cb * e
    xn = cx * x.double() + c0 * x0 + c1 * x0_prev.double() + cn * z.double()
    if mask is not None:
        m = mask.double()
        xn = m * xn + (1 - m) * (q0 * known.double() + q1 * noise.double())
    return xn, x0


def sde_table(n, start=0, blend=False, algorithm_type=SDE):
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler(algorithm_type=algorithm_type)
    sch.set_timesteps(n)
    return sch, sch.coefficient_table(start, blend=blend)


# ---------------------------------------------------------------------------------------------------------------- tests
def test_numpy_philox_known_answers():
    """Random123's known-answer vectors of philox4x32_10."""
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 2, (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, out in kat:
        assert tuple(int(w) for w in philox4x32_10(key, ctr)) == out, (key, ctr)
    # over arrays: every lane is its own block
    w = philox4x32_10((0xa4093822, 0x299f31d0), (np.array([0x243f6a88, 0, 7]), 0x85a308d3, 0x13198a2e, 0x03707344))
    assert tuple(int(x[0]) for x in w) == kat[2][2] and len({int(w[0][i]) for i in range(3)}) == 3


def test_box_muller_uniforms_are_exact_and_open_and_the_normals_are_normal():
    lo, hi = np.uint32(0), np.uint32(0xFFFFFFFF)
    for w, u in ((lo, 2.0 ** -24), (hi, 1 - 2.0 ** -24)):
        for dt in (np.float32, np.float64):
            got = ((np.array([w]) >> np.uint32(9)).astype(dt) + dt(0.5)) * dt(2.0 ** -23)
            assert got.dtype == dt and float(got[0]) == u and 0.0 < u < 1.0            # exact in fp32: 24 significant bits at most
    z = noise_ref((2, 4, 64, 64), 1234, 0, 0, 3)
    assert torch.isfinite(z).all() and abs(z.mean().item()) < 0.02 and abs(z.std().item() - 1) < 0.02
    z32 = noise_ref((2, 4, 64, 64), 1234, 0, 0, 3, dtype=np.float32)
    assert (z - z32).abs().max().item() < 5e-6                                          # the definition evaluated in fp32


@pytest.mark.parametrize("n", [6, 25])
@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("blend", [False, True])
def test_sde_table_matches_the_formulas_in_fp64(n, start, blend):
    """Every row within two fp32 ulps of the independent fp64 evaluation (both sides compute in fp64; the table is then rounded to fp32)."""
    sch, tab = sde_table(n, start, blend)
    assert tab.dtype == torch.float32 and tab.shape == (n, 8)
    exp = sde_rows_ref(sch.sigmas, start, blend)
    torch.testing.assert_close(tab.double(), exp, rtol=2.4e-7, atol=1e-12)
    assert tab[n - 1, [2, 3, 4, 7]].tolist() == [0.0, 1.0, 0.0, 0.0]                     # the last row: x0, free of noise
    assert (tab[:n - 1, 7] > 0).all() and (tab[:, 4] <= 0).all() and tab[start, 4] == 0 and (tab[start + 1:n - 1, 4] < 0).all()
    # ca, cb, q0, q1 are the deterministic type's
    _, det = sde_table(n, start, blend, "dpmsolver++")
    assert torch.equal(tab[:, [0, 1, 5, 6]], det[:, [0, 1, 5, 6]])
    if not blend:
        assert (tab[:, 5:7] == 0).all()


def _deterministic_table_as_it_was(sch, start, blend):
    """``coefficient_table`` of the deterministic type as it stood before the SDE type was added, statement by statement."""
    n = sch.num_inference_steps
    sig = sch.sigmas.astype(np.float64)
    alpha = 1.0 / np.sqrt(sig * sig + 1.0)
    sigma = sig * alpha
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)
    tab = np.zeros((n, 8), dtype=np.float64)
    for i in range(n):
        a_s, s_s, a_t, s_t = alpha[i], sigma[i], alpha[i + 1], sigma[i + 1]
        h = lam[i + 1] - lam[i]
        c = a_t * (np.exp(-h) - 1.0)
        tab[i, 0], tab[i, 1], tab[i, 2] = 1.0 / a_s, -s_s / a_s, s_t / s_s
        if i <= start or i == n - 1:
            tab[i, 3], tab[i, 4] = -c, 0.0
        else:
            r0 = (lam[i] - lam[i - 1]) / h
            tab[i, 3], tab[i, 4] = -c * (1.0 + 0.5 / r0), 0.5 * c / r0
        if blend:
            tab[i, 5], tab[i, 6] = a_t, s_t
    return torch.from_numpy(tab.astype(np.float32))


@pytest.mark.parametrize("n", [6, 25])
def test_default_type_keeps_its_table_and_a_zero_spare_column(n):
    from photoverse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    for start in (0, 2):
        for blend in (False, True):
            plain = DPMSolverMultistepScheduler()
            plain.set_timesteps(n)
            named = DPMSolverMultistepScheduler(algorithm_type="dpmsolver++")
            named.set_timesteps(n)
            cfg = DPMSolverMultistepScheduler.from_config(plain.config)
            cfg.set_timesteps(n)
            t = plain.coefficient_table(start, blend=blend)
            assert torch.equal(t, named.coefficient_table(start, blend=blend)) and torch.equal(t, cfg.coefficient_table(start, blend=blend))
            assert (t[:, 7] == 0).all() and not plain.stochastic
            assert torch.equal(t, _deterministic_table_as_it_was(plain, start, blend))
    assert DPMSolverMultistepScheduler.from_config({**plain.config, "algorithm_type": SDE}).stochastic
    assert DPMSolverMultistepScheduler(algorithm_type=SDE).config["algorithm_type"] == SDE
    # from_config: a type this scheduler does not implement gives the default, as before the key was read; the keyword overrides the config
    for other in ("dpmsolver", "sde-dpmsolver", None, 3):
        assert not DPMSolverMultistepScheduler.from_config({**plain.config, "algorithm_type": other}).stochastic
    assert not DPMSolverMultistepScheduler.from_config({**plain.config, "algorithm_type": SDE}, algorithm_type="dpmsolver++").stochastic
    assert DPMSolverMultistepScheduler.from_config(plain.config, algorithm_type=SDE).stochastic
    with pytest.raises(ValueError, match="algorithm_type"):
        DPMSolverMultistepScheduler.from_config(plain.config, algorithm_type="dpmsolver")
    with pytest.raises(ValueError, match="algorithm_type"):
        DPMSolverMultistepScheduler(algorithm_type="dpmsolver")
    with pytest.raises(ValueError, match="DDIM"):
        DDIMScheduler(algorithm_type=SDE)
    with pytest.raises(ValueError, match="DDIM"):
        DDIMScheduler.from_config({"algorithm_type": SDE})
    assert not DDIMScheduler().stochastic


def final_std_ratio(rows, sigmas, c):
    """Data ~ N(0, c^2), so the exact eps(x) at noise level (alpha, sigma) is ``sigma x / (alpha^2 c^2 + sigma^2)`` and the solver is a linear map of
    the start noise (unit variance: ``init_noise_sigma``) and the step noises: the latents are carried as their coefficients on those n + 1
    independent unit normals, and the final standard deviation is the norm of the coefficient vector.  -> std / c."""
    k = np.asarray(sigmas, dtype=np.float64)
    alpha = (1.0 + k * k) ** -0.5
    sigma = k * alpha
    rows = np.asarray(rows, dtype=np.float64)
    n = len(rows)
    x = np.zeros(n + 1)
    x[0] = 1.0
    x0_prev = np.zeros(n + 1)
    for i in range(n):
        eps = sigma[i] * x / (alpha[i] ** 2 * c * c + sigma[i] ** 2)
        x0 = rows[i, 0] * x + rows[i, 1] * eps
        x = rows[i, 2] * x + rows[i, 3] * x0 + rows[i, 4] * x0_prev
        x[i + 1] += rows[i, 7]
        x0_prev = x0
    return float(np.linalg.norm(x)) / c


#: std(final) / c of the SDE rows on the project's schedule, from the exact linear-Gaussian computation (five decimals)
RATIOS = {0.5: {10: 0.82603, 25: 0.94302, 50: 0.97638, 100: 0.98861, 200: 0.99303},
          1.0: {10: 0.96345, 25: 0.99533, 50: 0.99784, 100: 0.99823, 200: 0.99847}}
RATIOS_ODE = {10: 0.84000, 25: 0.93745, 50: 0.97026, 100: 0.98826, 200: 1.00439}          # the deterministic rows at c = 0.5


def test_sde_table_is_consistent_on_a_linear_gaussian_model():
    """With more steps the stochastic sampler's samples of N(0, c^2) data approach the data's standard deviation.  The bounds are conditions on an exact
    computation (twice the computed gaps 0.0114 and 0.00216), not measurements; the five-decimal values are the computation itself, rounded."""
    got = {c: {} for c in RATIOS}
    for c, per_n in RATIOS.items():
        for n, want in per_n.items():
            sch, tab = sde_table(n)
            got[c][n] = final_std_ratio(tab.double().numpy(), sch.sigmas, c)
            assert got[c][n] == pytest.approx(final_std_ratio(sde_rows_ref(sch.sigmas).numpy(), sch.sigmas, c), abs=2e-6)      # fp32 table vs fp64 rows
            assert got[c][n] == pytest.approx(want, abs=6e-6), (c, n)
    for n, want in RATIOS_ODE.items():                      # the harness itself: the deterministic table's known values
        sch, tab = sde_table(n, algorithm_type="dpmsolver++")
        assert final_std_ratio(tab.double().numpy(), sch.sigmas, 0.5) == pytest.approx(want, abs=6e-6), n
    r = got[0.5]
    assert r[25] < r[50] < r[100] < r[200]
    assert abs(1 - got[0.5][100]) < 0.023
    assert abs(1 - got[1.0][50]) < 0.0044


def _philox_scalar(k0, k1, c):
    """One block in Python integers, written separately from the array version."""
    c = list(c)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def test_fp64_reference_of_the_launcher_against_a_per_element_evaluation():
    """``stochastic_step_ref`` + ``noise_ref`` on (1, 4, 4, 4), three-forward with rescale and a mixed mask, on a second-order row, against the header's
    formulas evaluated element by element in Python floats and integers (1e-12: fp64 summed in another order)."""
    shape = (1, 4, 4, 4)
    g = torch.Generator().manual_seed(9)
    eu, em, ec = make_eps(shape, g)
    x, xp, known, noise = (torch.randn(shape, generator=g) for _ in range(4))
    mask = torch.tensor([0.0, 1.0, 0.5, 1.0] * 4).view(1, 1, 4, 4)
    _, tab = sde_table(6, 0, True)
    seed, off, stream, step, gt, gi, rs = (0xfeedfacecafe << 16) + 5, 7, 1, 3, 7.5, 3.0, 0.7
    row = tab[step]
    z = noise_ref(shape, seed, off, stream, step)
    got, got_x0 = stochastic_step_ref(eu, em, ec, x, xp, row, z, gt, gi, rs, mask, known, noise)
    ca, cb, cx, c0, c1, q0, q1, cn = (float(v) for v in row)
    f = lambda t: [float(v) for v in t.flatten()]
    U, M, C, X, XP, KN, NZ = map(f, (eu, em, ec, x, xp, known, noise))
    E = [U[i] + gi * (M[i] - U[i]) + gt * (C[i] - M[i]) for i in range(64)]
    mean = lambda v: sum(v) / len(v)
    std = lambda v: math.sqrt(mean([(a - mean(v)) ** 2 for a in v]))
    fac = rs * std(C) / std(E) + (1 - rs)
    for i in range(64):
        q, j = divmod(i, 4)
        w = _philox_scalar(seed & 0xFFFFFFFF, seed >> 32, (q, off + 0, step, stream))
        u = [((wk >> 9) + 0.5) / 8388608.0 for wk in w]
        r, a = math.sqrt(-2 * math.log(u[j & 2])), 2 * math.pi * u[(j & 2) + 1]
        zz = r * (math.cos(a) if j % 2 == 0 else math.sin(a))
        assert zz == pytest.approx(float(z.flatten()[i]), abs=1e-12)
        x0 = ca * X[i] + cb * fac * E[i]
        xn = cx * X[i] + c0 * x0 + c1 * XP[i] + cn * zz
        m = float(mask.flatten()[i % 16])
        want = m * xn + (1 - m) * (q0 * KN[i] + q1 * NZ[i])
        assert float(got_x0.flatten()[i]) == pytest.approx(x0, rel=1e-12, abs=1e-12)
        assert float(got.flatten()[i]) == pytest.approx(want, rel=1e-12, abs=1e-12)
    # no noise on the last row, whatever z is
    last, _ = stochastic_step_ref(eu, None, ec, x, xp, tab[5], z, gt)
    other, _ = stochastic_step_ref(eu, None, ec, x, xp, tab[5], noise_ref(shape, 1, 0, 0, 5), gt)
    assert torch.equal(last, other)


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


def test_run_inference_validates_sampler_and_sample_offset_before_touching_a_model():
    from photoverse_amd.infer import run_inference
    sig = inspect.signature(run_inference).parameters
    for name, default in (("sampler", "dpmsolver++"), ("sample_offset", 0)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    u = _Untouchable()
    args = (u,) * 9 + ("cpu", [1])
    kw = dict(latent_size=16, guidance_scale=7.5, timesteps=4)
    for bad in ("ddim", "sde", "SDE-DPMSOLVER++", "", None, 1, ["sde-dpmsolver++"]):
        with pytest.raises(ValueError, match="sampler"):
            run_inference(*args, sampler=bad, **kw)
    for bad in (-1, -100, 1.0, 0.5, "1", None, True, [0], 1 << 32):
        for sampler in ("dpmsolver++", SDE):
            with pytest.raises(ValueError, match="sample_offset"):
                run_inference(*args, sampler=sampler, sample_offset=bad, **kw)
    with pytest.raises(ValueError, match="sde-dpmsolver.*training_mode"):
        run_inference(*args, sampler=SDE, training_mode=True, **kw)
    for good in (dict(sampler=SDE), dict(sampler=SDE, sample_offset=3), dict(sampler="dpmsolver++", sample_offset=np.int64(2)), dict()):
        with pytest.raises(AssertionError, match="touched a model argument"):
            run_inference(*args, **good, **kw)


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    assert re.search(r"^int\s+pv_cfg_dpm_step_stochastic\s*\(", header, flags=re.M)
    res, args = _lib.SIGNATURES["pv_cfg_dpm_step_stochastic"]
    guided = _lib.SIGNATURES["pv_cfg_dpm_step_guided"][1]
    assert res is _lib.c_int and args == guided[:7] + [_lib.c_void_p] + guided[7:]          # the guided launcher's arguments plus rng after state
    assert lib.pv_cfg_dpm_step_stochastic is not None
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    from photoverse_amd.ops import Recorder
    assert list(inspect.signature(Recorder.cfg_dpm_step_stochastic).parameters)[1:] == [
        "eps_u", "eps_i", "eps_c", "latents", "x0_prev", "coef", "state", "rng", "g_text", "g_image", "rescale", "mask", "known", "noise"]


def test_cabi_rejects_bad_stochastic_step_arguments_before_touching_the_device(lib):
    """Validation comes before the first HIP call: hipErrorInvalidValue = 1 with pointers that are never dereferenced (no GPU needed)."""
    INVALID = 1
    EU, EM, EC, LAT, X0P, COEF, STATE, RNG, MASK, KNOWN, NOISE = (0x10000 * (i + 1) for i in range(11))

    def call(eu=EU, em=EM, ec=EC, lat=LAT, x0p=X0P, coef=COEF, state=STATE, rng=RNG, g_text=7.5, g_image=3.0, rescale=0.7, mask=MASK, known=KNOWN,
             noise=NOISE, batch=2, channels=4, hw=256):
        return lib.pv_cfg_dpm_step_stochastic(eu, em, ec, lat, x0p, coef, state, rng, g_text, g_image, rescale, mask, known, noise, batch, channels, hw,
                                              None)

    for name in ("rng", "eu", "ec", "lat", "x0p", "coef", "state"):
        assert call(**{name: None}) == INVALID, name
        assert call(**{name: None}, em=None, mask=None, known=None, noise=None, rescale=0.0) == INVALID, name
    for hw, ch in ((1, 4), (2, 4), (3, 4), (6, 2), (255, 4), (258, 4), (5, 1), (3, 3)):               # hw % 4 != 0, chw % 4 == 0 or not
        assert call(hw=hw, channels=ch) == INVALID, (hw, ch)
    for part in (dict(known=None), dict(mask=None), dict(noise=None), dict(mask=None, known=None), dict(known=None, noise=None)):
        assert call(**part) == INVALID, part
    for name in ("batch", "channels", "hw"):
        assert call(**{name: 0}) == INVALID and call(**{name: -4}) == INVALID, name
    for r in (-0.1, 1.0001, math.nan, math.inf):
        assert call(rescale=r) == INVALID, r
    assert call(g_text=math.nan) == INVALID and call(g_image=math.inf) == INVALID
    assert call(batch=2, channels=4, hw=1 << 28) == INVALID                                           # 2^31 elements


def _gloo_offset_worker(rank, world, port, q):
    """PhotoVersePipeline(shard=True) under gloo with ``run_inference`` replaced by a recorder of what it is handed."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import photoverse_amd.infer as infer_mod
    from photoverse_amd.pipeline import PhotoVersePipeline
    from types import SimpleNamespace
    seen = {}

    def fake_run_inference(example, *a, **kw):
        seen.update(kw, n_local=example["pixel_values_clip"].shape[0])
        return kw["noise"] * 2.0

    infer_mod.run_inference = fake_run_inference
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))
    pipe = PhotoVersePipeline(None, None, None, unet, None, None, None, None)
    example = {"pixel_values_clip": torch.randn(6, 3, 8, 8, generator=torch.Generator().manual_seed(11)), "text": ["x"] * 6}
    pipe(example, shard=True, seed=123, latent_size=16, sampler=SDE)
    per_rank = 6 // world
    ok = seen["n_local"] == per_rank and seen["sample_offset"] == rank * per_rank and seen["sampler"] == SDE and seen["seed"] == 123
    seen.clear()
    pipe(example, shard=True, seed=123, latent_size=16)                      # the deterministic sampler is handed the same offset (and ignores it)
    ok = ok and seen["sample_offset"] == rank * per_rank and "sampler" not in seen
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_sharded_pipeline_hands_each_rank_its_sample_offset_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_offset_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == [(0, True), (1, True)]


def test_cli_flag_parses():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pv_generate_sampler", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.parser.parse_args([]).sampler == "dpmsolver++"
    assert gen.parser.parse_args(["--sampler", SDE]).sampler == SDE
    with pytest.raises(SystemExit):
        gen.parser.parse_args(["--sampler", "euler"])
