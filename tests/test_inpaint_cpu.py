"""CPU-only tests of masked image editing (inpainting) and ``strength``: the blend / start-row columns of the scheduler tables against the oracle's
blended stepping, the C-ABI rejections of the two launchers, mask preprocessing and the latent max-pool, the ``strength`` arithmetic and the CLI flags."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def _start(steps, strength):
    return steps - min(int(steps * strength), steps)


@pytest.mark.parametrize("steps,strength", [(2, 1.0), (7, 0.5), (25, 0.3), (50, 0.75), (4, 0.25)])
def test_blend_table_reproduces_oracle_blended_stepping(steps, strength):
    """``coefficient_table(start, blend=True)`` against DPMSolverMultistepRef started at ``step_index = start`` and blended after each ``step()`` with
    ``add_noise(known, noise, timesteps[i + 1])`` (the clean ``known`` after the last step): relative 1e-6 at every step, the bound of
    ``test_scheduler_table_reproduces_oracle_stepping``; the kept region ends on ``known`` bit for bit."""
    from oracle.scheduler_ref import DPMSolverMultistepRef
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    start = _start(steps, strength)
    s = DPMSolverMultistepScheduler.from_config(DPMSolverMultistepScheduler().config)
    s.set_timesteps(steps)
    assert torch.equal(s.coefficient_table(), s.coefficient_table(0, False))
    tab = s.coefficient_table(start, blend=True).double()
    assert tab.shape == (steps, 8) and torch.equal(tab[:, :5].float(), s.coefficient_table(start)[:, :5]) and tab[:, 7].abs().max() == 0
    assert s.coefficient_table(start)[:, 5:].abs().max() == 0 and tab[-1, 5] == 1 and tab[-1, 6] == 0
    r = DPMSolverMultistepRef()
    r.set_timesteps(steps)
    r.step_index = start
    g = torch.Generator().manual_seed(steps)
    n = 256
    known, noise = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(2))
    m = (torch.rand(n, generator=g) < 0.5).double()
    x = r.add_noise(known, noise, r.timesteps[start:start + 1])
    xr, xp = x.clone(), torch.zeros_like(x)
    for i in range(start, steps):
        eps = torch.randn(n, generator=g, dtype=torch.float64)
        xr = r.step(eps, r.timesteps[i], xr)
        kr = r.add_noise(known, noise, r.timesteps[i + 1:i + 2]) if i < steps - 1 else known
        xr = m * xr + (1 - m) * kr
        ca, cb, cx, c0, c1, q0, q1 = tab[i, :7]
        x0 = ca * x + cb * eps
        xn = cx * x + c0 * x0 + c1 * xp
        x, xp = m * xn + (1 - m) * (q0 * known + q1 * noise), x0
        assert ((x - xr).norm() / xr.norm()).item() < 1e-6, i
    assert torch.equal(x[m == 0], known[m == 0])


@pytest.mark.parametrize("steps,strength", [(10, 1.0), (50, 0.5)])
def test_ddim_blend_table_reproduces_stepwise_ddim_with_the_blend(steps, strength):
    from oracle.scheduler_ref import DDIMRef
    from photoverse_amd.scheduler import DDIMScheduler
    start = _start(steps, strength)
    s = DDIMScheduler()
    s.set_timesteps(steps)
    assert torch.equal(s.coefficient_table(), s.coefficient_table(0, False))
    tab = s.coefficient_table(start, blend=True).double()
    assert torch.equal(tab[:, :5].float(), s.coefficient_table()[:, :5]) and tab[-1, 5] == 1 and tab[-1, 6] == 0
    r = DDIMRef()
    r.set_timesteps(steps)
    g = torch.Generator().manual_seed(steps)
    known, noise = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(2))
    m = (torch.rand(64, generator=g) < 0.5).double()
    a0 = r.alphas_cumprod[int(r.timesteps[start])]
    x = a0.sqrt() * known + (1 - a0).sqrt() * noise
    xr = x.clone()
    for i in range(start, steps):
        eps = torch.randn(64, generator=g, dtype=torch.float64)
        xr = r.step(eps, r.timesteps[i], xr)
        if i < steps - 1:
            a = r.alphas_cumprod[int(r.timesteps[i + 1])]            # add_noise(known, noise, t_next)
            kr = a.sqrt() * known + (1 - a).sqrt() * noise
        else:
            kr = known
        xr = m * xr + (1 - m) * kr
        ca, cb, cx, c0, _, q0, q1 = tab[i, :7]
        xn = cx * x + c0 * (ca * x + cb * eps)
        x = m * xn + (1 - m) * (q0 * known + q1 * noise)
        assert ((x - xr).norm() / xr.norm()).item() < 1e-6, i
    assert torch.equal(x[m == 0], known[m == 0])


def test_cabi_rejects_bad_masked_step_and_composite_arguments_before_touching_the_device(lib):
    """Both launchers validate before their first HIP call and return hipErrorInvalidValue = 1 (no GPU needed): null pointers, channels <= 0,
    hw <= 0, hw % 4 != 0 (a float4 must not straddle a channel plane), n not a multiple of channels * hw."""
    INVALID, FAKE = 1, 0x1000                        # never dereferenced: the checks come first

    def step(ptrs=(FAKE,) * 9, channels=4, hw=16, n=2 * 4 * 16):
        eu, ec, lat, x0p, coef, state, mask, known, noise = ptrs
        return lib.pv_cfg_dpm_step_masked(eu, ec, lat, x0p, coef, state, 7.5, mask, known, noise, channels, hw, n, None)

    for k in range(9):
        assert step(ptrs=tuple(None if j == k else FAKE for j in range(9))) == INVALID, k
    for bad in (dict(channels=0), dict(channels=-4), dict(hw=0), dict(hw=-16), dict(hw=6, n=2 * 4 * 6), dict(hw=18, n=2 * 4 * 18), dict(n=2 * 4 * 16 + 4),
                dict(n=4 * 16 + 16), dict(n=0), dict(n=-128)):
        assert step(**bad) == INVALID, bad

    def comp(ptrs=(FAKE,) * 4, batch=2, channels=3, hw=16):
        gen, orig, mask, out = ptrs
        return lib.pv_composite_clamp_f32(gen, orig, mask, out, -1.0, 1.0, batch, channels, hw, None)

    for k in range(4):
        assert comp(ptrs=tuple(None if j == k else FAKE for j in range(4))) == INVALID, k
    for bad in (dict(batch=0), dict(channels=0), dict(channels=-3), dict(hw=0), dict(hw=-4), dict(hw=6), dict(hw=9)):
        assert comp(**bad) == INVALID, bad


def test_preprocess_mask_and_latent_max_pool():
    import numpy as np
    from PIL import Image
    from photoverse_amd.image_utils import preprocess_mask
    from photoverse_amd.infer import latent_mask
    # a greyscale file: white = regenerate, nearest-neighbour to the working resolution, binary
    arr = np.zeros((64, 64), dtype=np.uint8)
    arr[:32, 48:] = 255
    arr[40, 0] = 200
    arr[41, 0] = 100
    pm = preprocess_mask(Image.fromarray(arr), size=32)
    assert pm.shape == (1, 32, 32) and pm.dtype == torch.float32 and set(pm.unique().tolist()) == {0.0, 1.0}
    assert pm[0, :16, 24:].min() == 1 and pm[0, 16:, 1:].max() == 0 and pm[0, :, :24].sum() <= 1
    same = preprocess_mask(Image.fromarray(arr).convert("RGB"), size=64)          # an RGB file is read as greyscale; no resize: the pixels themselves
    assert torch.equal(same[0], torch.from_numpy(arr >= 128).float())
    wide = np.zeros((32, 64), dtype=np.uint8)                                       # centre crop like preprocess_image: the left quarter is cropped away
    wide[:, :16] = 255
    assert preprocess_mask(Image.fromarray(wide), size=32).sum() == 0
    # one pixel marks exactly one latent cell (factor 4 from the shapes: 32 / 8)
    m = torch.zeros(2, 1, 32, 32)
    m[0, 0, 13, 22] = 1.0
    m[1, 0, 3:5, 7:9] = 1.0                          # rows 3-4 and columns 7-8 straddle block boundaries: four cells
    m[1, 0, 20, 20] = 0.49                           # below the threshold: nothing
    pix, lat = latent_mask(m, 2, 8)
    assert pix.shape == (2, 1, 32, 32) and lat.shape == (2, 1, 8, 8) and pix.dtype == lat.dtype == torch.float32
    assert lat[0].sum() == 1 and lat[0, 0, 3, 5] == 1
    assert lat[1].sum() == 4 and lat[1, 0, 0:2, 1:3].min() == 1
    assert pix[1].sum() == 4 and pix[1, 0, 20, 20] == 0
    # a mask on a boundary in one direction only marks both cells
    m2 = torch.zeros(1, 1, 16, 16)
    m2[0, 0, 5, 7:9] = 0.5                           # 0.5 itself counts as masked
    pix2, lat2 = latent_mask(m2, 3, 4)              # (1, 1, H, W) broadcasts over the batch
    assert pix2.shape == (3, 1, 16, 16) and lat2.shape == (3, 1, 4, 4)
    assert all(lat2[b].sum() == 2 and lat2[b, 0, 1, 1] == 1 and lat2[b, 0, 1, 2] == 1 for b in range(3))
    # the tiny VAE's factor 2
    _, lat3 = latent_mask(torch.ones(1, 1, 32, 32), 1, 16)
    assert lat3.shape == (1, 1, 16, 16) and lat3.min() == 1
    for bad in (torch.zeros(1, 1, 30, 32), torch.zeros(1, 1, 32, 36), torch.zeros(1, 1, 4, 4)):
        with pytest.raises(ValueError, match="latent_size"):
            latent_mask(bad, 1, 8)
    for bad in (torch.zeros(3, 1, 32, 32), torch.zeros(2, 3, 32, 32), torch.zeros(32, 32)):
        with pytest.raises(ValueError, match="shape"):
            latent_mask(bad, 2, 8)


def test_strength_arithmetic_and_cli_flags(tmp_path):
    import argparse
    import importlib.util
    from photoverse_amd.infer import run_inference, strength_start
    from photoverse_amd.tokenizer import SyntheticCLIPTokenizer
    assert strength_start(10, 1.0) == 0 and strength_start(10, 0.55) == 5 and strength_start(3, 0.34) == 2
    for bad in (0.0, 1.5, -0.1, 0.05):               # outside (0, 1]; 0.05 of 10 steps leaves none to run
        with pytest.raises(ValueError):
            strength_start(10, bad)
    # run_inference validates before it touches a device or a model
    ex = {"pixel_values": torch.zeros(1, 3, 32, 32), "pixel_values_clip": torch.zeros(1, 3, 56, 56)}
    sch = argparse.Namespace(config={})
    unet = argparse.Namespace(config=argparse.Namespace(in_channels=4))
    tok = SyntheticCLIPTokenizer()
    for s in (0.0, 1.5):
        with pytest.raises(ValueError, match="strength"):
            run_inference(ex, tok, None, None, unet, None, None, None, sch, "cpu", [1], latent_size=16, timesteps=10, from_noised_image=True, strength=s)
    with pytest.raises(ValueError, match="strength"):            # nothing to start from
        run_inference(ex, tok, None, None, unet, None, None, None, sch, "cpu", [1], latent_size=16, timesteps=10, strength=0.5)
    with pytest.raises(NotImplementedError, match=r"inpaint_mask needs a vae with \.encode"):
        run_inference(ex, tok, None, None, unet, None, None, None, sch, "cpu", [1], latent_size=16, timesteps=10, inpaint_mask=torch.ones(1, 1, 32, 32))
    with pytest.raises(ValueError, match="latent_size"):
        run_inference(ex, tok, None, None, unet, None, None, None, sch, "cpu", [1], latent_size=16, timesteps=10, inpaint_mask=torch.ones(1, 1, 40, 40))
    # the CLI: new flags parse; their defaults leave the example as it was and pass the neutral arguments on
    spec = importlib.util.spec_from_file_location("pv_generate_inpaint", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.mask_image_path is None and d.target_image_path is None and d.strength == 1.0 and d.no_paste_back is False
    assert gen.prepare_mask(d) is None
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    face, photo, mask = tmp_path / "face.png", tmp_path / "photo.png", tmp_path / "mask.png"
    Image.fromarray(rng.integers(0, 256, (80, 64, 3), dtype=np.uint8)).save(face)
    Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(photo)
    marr = np.zeros((128, 128), dtype=np.uint8)
    marr[:, 64:] = 255
    Image.fromarray(marr).save(mask)
    base = ["--input_image_path", str(face), "--latent_size", "8", "--num_of_samples", "2"]
    old = argparse.Namespace(num_of_samples=2, text="a photo of a {}", negative_prompt=None, synthetic_input=False, input_image_path=str(face), seed=None,
                             latent_size=8)              # a namespace without the new attributes: what callers of prepare_example pass today
    ex0, ex1 = gen.prepare_example(old, tok), gen.prepare_example(gen.parser.parse_args(base), tok)
    assert ex0.keys() == ex1.keys() and all(torch.equal(ex0[k], ex1[k]) if torch.is_tensor(ex0[k]) else ex0[k] == ex1[k] for k in ex0)
    a = gen.parser.parse_args(base + ["--mask_image_path", str(mask), "--target_image_path", str(photo), "--strength", "0.6", "--no_paste_back"])
    assert a.strength == 0.6 and a.no_paste_back is True
    ex2 = gen.prepare_example(a, tok)
    assert torch.equal(ex2["pixel_values_clip"], ex1["pixel_values_clip"])            # the identity image
    assert ex2["pixel_values"].shape == (2, 3, 64, 64) and not torch.equal(ex2["pixel_values"], ex1["pixel_values"])     # the photograph
    pm = gen.prepare_mask(a)
    assert pm.shape == (1, 1, 64, 64) and pm[..., 32:].min() == 1 and pm[..., :32].max() == 0
