"""CPU-only tests of two-pass high-resolution generation: the C-ABI rejections of ``pv_resize_bilinear_affine_f32``, the validation of the ``hires_*``
keywords of ``run_inference``, the CLI flags, the two consecutive global noise draws of the sharded pipeline under gloo, and the torch restatement of the
kernel's formula (the reference of ``tests/test_hires_gpu.py``) against ``F.interpolate``."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: (B, C, h, w, oh, ow) of the kernel test: ratio 1.5 with ow % 4 != 0; x2; 6400 outputs (several workgroups, the last one partial); rectangular, up on
#: one axis and down on the other; a one-pixel source (both neighbours clamp); equal size
SHAPES = [(2, 4, 4, 4, 6, 6), (2, 4, 16, 16, 32, 32), (1, 4, 16, 16, 40, 40), (2, 3, 3, 5, 7, 4), (1, 1, 1, 1, 4, 4), (2, 4, 8, 8, 8, 8)]


def bilinear_ref(x, oh, ow, ca=None, y=None, cb=None):
    """The header's formula of ``pv_resize_bilinear_affine_f32`` in fp64 on the given (fp32) values: per axis src = max((dst + 0.5) * (in / out) - 0.5, 0),
    i0 = floor(src), i1 = min(i0 + 1, in - 1), weight = src - i0; out = ca[b] * bilinear(x) (+ cb[b] * y)."""
    x = x.double()
    B, C, h, w = x.shape

    def taps(n_in, n_out):
        src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
        i0 = src.floor().long().clamp_max(n_in - 1)
        return i0, (i0 + 1).clamp_max(n_in - 1), src - i0

    y0, y1, wy = taps(h, oh)
    x0, x1, wx = taps(w, ow)
    wy = wy.view(oh, 1)
    top = (1 - wx) * x[:, :, y0][..., x0] + wx * x[:, :, y0][..., x1]
    bot = (1 - wx) * x[:, :, y1][..., x0] + wx * x[:, :, y1][..., x1]
    out = (1 - wy) * top + wy * bot
    if ca is not None:
        out = ca.double().view(B, 1, 1, 1) * out
    if y is not None:
        out = out + cb.double().view(B, 1, 1, 1) * y.double()
    return out


@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_cabi_rejects_bad_resize_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed): NULL x / out, a zero or negative dimension,
    y without cb, cb without y, an operand of 2 GiB or more.  No valid call is sent."""
    from photoverse_amd import _lib
    assert _lib.ABI_VERSION == 19 == lib.pv_abi_version() and "pv_resize_bilinear_affine_f32" in _lib.SIGNATURES
    INVALID = 1
    X, Y, CA, CB, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000          # never dereferenced: the checks come first

    def call(x=X, y=Y, ca=CA, cb=CB, out=OUT, batch=2, channels=4, h=16, w=16, oh=32, ow=32):
        return lib.pv_resize_bilinear_affine_f32(x, y, ca, cb, out, batch, channels, h, w, oh, ow, None)

    assert call(x=None) == INVALID and call(out=None) == INVALID
    assert call(x=None, y=None, cb=None) == INVALID and call(out=None, y=None, cb=None, ca=None) == INVALID
    for name in ("batch", "channels", "h", "w", "oh", "ow"):
        for v in (0, -1, -16):
            assert call(**{name: v}) == INVALID, (name, v)
    assert call(cb=None) == INVALID                  # y without cb
    assert call(y=None) == INVALID                   # cb without y
    assert call(cb=None, ca=None) == INVALID and call(y=None, ca=None) == INVALID
    # 2 GiB = 2^29 floats: the output (and y), the input, and products that overflow 64 bits when multiplied out
    assert call(batch=1, channels=1, h=1, w=1, oh=1 << 15, ow=1 << 14) == INVALID            # out is exactly 2 GiB
    assert call(batch=1, channels=1, h=1 << 14, w=1 << 15, oh=1, ow=1) == INVALID            # x is exactly 2 GiB
    assert call(batch=2, channels=4, h=1, w=1, oh=8192, ow=8192) == INVALID
    m = (1 << 31) - 1
    assert call(batch=m, channels=m, h=m, w=m, oh=m, ow=m) == INVALID
    assert call(batch=1, channels=1, h=m, w=m, oh=1, ow=1) == INVALID and call(batch=1, channels=1, h=1, w=1, oh=m, ow=m) == INVALID


def _stub_args():
    """The stub arguments of ``test_inpaint_cpu.py::test_strength_arithmetic_and_cli_flags``: nothing here could run a model."""
    import argparse
    from photoverse_amd.tokenizer import SyntheticCLIPTokenizer
    ex = {"pixel_values": torch.zeros(1, 3, 32, 32), "pixel_values_clip": torch.zeros(1, 3, 56, 56)}
    sch = argparse.Namespace(config={})
    unet = argparse.Namespace(config=argparse.Namespace(in_channels=4))
    return (ex, SyntheticCLIPTokenizer(), None, None, unet, None, None, None, sch, "cpu", [1])


def test_run_inference_validates_the_hires_keywords_before_touching_a_model():
    import inspect
    from photoverse_amd.infer import run_inference
    sig = inspect.signature(run_inference).parameters
    names = list(sig)
    assert names[names.index("paste_back") + 1:] == ["hires_latent_size", "hires_strength", "hires_timesteps", "hires_noise"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[-4:])
    assert [sig[k].default for k in names[-4:]] == [None, 0.5, None, None]
    args = _stub_args()
    kw = dict(latent_size=16, timesteps=10)
    with pytest.raises(ValueError, match="hires_latent_size"):             # smaller than the first pass
        run_inference(*args, hires_latent_size=8, **kw)
    for bad in (0, -32, 32.0, "32", True):
        with pytest.raises(ValueError, match="hires_latent_size"):
            run_inference(*args, hires_latent_size=bad, **kw)
    for s in (0.0, 1.5):
        with pytest.raises(ValueError, match="hires_strength"):
            run_inference(*args, hires_latent_size=32, hires_strength=s, **kw)
    with pytest.raises(ValueError, match="hires_strength"):                # int(10 * 0.05) = 0 steps
        run_inference(*args, hires_latent_size=32, hires_strength=0.05, hires_timesteps=10, **kw)
    with pytest.raises(ValueError, match="hires_timesteps"):
        run_inference(*args, hires_latent_size=32, hires_timesteps=0, **kw)
    with pytest.raises(ValueError, match="hires_latent_size.*inpaint_mask"):
        run_inference(*args, hires_latent_size=32, inpaint_mask=torch.ones(1, 1, 32, 32), **kw)
    with pytest.raises(ValueError, match="hires_latent_size.*training_mode"):
        run_inference(*args, hires_latent_size=32, training_mode=True, **kw)
    for bad in (torch.zeros(1, 4, 16, 16), torch.zeros(2, 4, 32, 32), torch.zeros(1, 4, 32, 31), torch.zeros(4, 32, 32)):
        with pytest.raises(ValueError, match="hires_noise"):
            run_inference(*args, hires_latent_size=32, hires_noise=bad, **kw)
    with pytest.raises(ValueError, match="hires_noise"):                   # a second noise without a second pass
        run_inference(*args, hires_noise=torch.zeros(1, 4, 32, 32), **kw)
    # without the keywords the old errors come in the old order
    with pytest.raises(ValueError, match="strength"):
        run_inference(*args, strength=0.5, **kw)


def test_cli_flags_parse_and_old_namespaces_keep_working():
    import argparse
    import importlib.util
    from photoverse_amd.tokenizer import SyntheticCLIPTokenizer
    spec = importlib.util.spec_from_file_location("pv_generate_hires", os.path.join(ROOT, "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    d = gen.parser.parse_args([])
    assert d.hires_latent_size is None and d.hires_strength == 0.5 and d.hires_timesteps is None
    a = gen.parser.parse_args(["--hires_latent_size", "96", "--hires_strength", "0.4", "--hires_timesteps", "30"])
    assert (a.hires_latent_size, a.hires_strength, a.hires_timesteps) == (96, 0.4, 30)
    tok = SyntheticCLIPTokenizer()
    old = argparse.Namespace(num_of_samples=2, text="a photo of a {}", negative_prompt=None, synthetic_input=True, input_image_path=None, seed=3,
                             latent_size=8)              # a namespace without the new (or the inpainting) attributes
    new = gen.parser.parse_args(["--synthetic_input", "--latent_size", "8", "--num_of_samples", "2", "--seed", "3", "--hires_latent_size", "16"])
    ex0, ex1 = gen.prepare_example(old, tok), gen.prepare_example(new, tok)
    assert ex0.keys() == ex1.keys() and all(torch.equal(ex0[k], ex1[k]) if torch.is_tensor(ex0[k]) else ex0[k] == ex1[k] for k in ex0)
    assert ex1["pixel_values"].shape == (2, 3, 64, 64)          # the first pass's resolution
    assert gen.prepare_mask(old) is None and gen.prepare_mask(new) is None


def _gloo_hires_worker(rank, world, port, q):
    """PhotoVersePipeline(shard=True, seed=..., hires_latent_size=...) under gloo with ``run_inference`` replaced by a recorder of what it is handed."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import photoverse_amd.infer as infer_mod
    from photoverse_amd.pipeline import PhotoVersePipeline, shard_batch
    from types import SimpleNamespace
    seen = {}

    def fake_run_inference(example, *a, **kw):
        seen.update(kw, n_local=example["pixel_values_clip"].shape[0])
        return kw["noise"] * 2.0

    infer_mod.run_inference = fake_run_inference
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))
    pipe = PhotoVersePipeline(None, None, None, unet, None, None, None, None)
    example = {"pixel_values_clip": torch.randn(6, 3, 8, 8, generator=torch.Generator().manual_seed(11)), "text": ["x"] * 6}
    out = pipe(example, shard=True, seed=123, latent_size=16, hires_latent_size=32, hires_strength=0.4)
    g = torch.manual_seed(123)                                   # the two consecutive draws of the seeded one-rank run
    n1 = torch.randn((6, 4, 16, 16), generator=g)
    n2 = torch.randn((6, 4, 32, 32), generator=g)
    sl = shard_batch(6, rank, world)
    ok = (seen["n_local"] == 3 and torch.equal(seen["noise"], n1[sl]) and torch.equal(seen["hires_noise"], n2[sl]) and seen["hires_latent_size"] == 32
          and seen["hires_strength"] == 0.4 and seen["seed"] == 123 and torch.equal(out, n1 * 2.0))
    # without hires nothing new is handed over, and a caller's own hires_noise is left alone
    seen.clear()
    pipe(example, shard=True, seed=123, latent_size=16)
    ok = ok and "hires_noise" not in seen and torch.equal(seen["noise"], n1[sl])
    seen.clear()
    own = torch.zeros(3, 4, 32, 32)
    pipe(example, shard=True, seed=123, latent_size=16, hires_latent_size=32, hires_noise=own)
    ok = ok and seen["hires_noise"] is own
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_sharded_pipeline_hands_each_rank_its_slices_of_both_global_draws_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_hires_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == [(0, True), (1, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_formula_restatement_agrees_with_torch_bilinear(shape):
    """``bilinear_ref`` (the header's formula in fp64) against ``F.interpolate(mode="bilinear", align_corners=False)``: 1e-12 against torch in fp64 -
    the same formula - and rtol = atol = 1e-5 against torch in fp32, the bound of the GPU test (torch's fp32 rounds its source coordinate: at most 3.4e-6
    on these shapes).  The affine part is checked against the plain expression; equal size is the identity."""
    B, C, h, w, oh, ow = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, y = torch.randn(B, C, h, w, generator=g), torch.randn(B, C, oh, ow, generator=g)
    ca, cb = torch.rand(B, generator=g) + 0.5, torch.rand(B, generator=g) - 0.5
    got = bilinear_ref(x, oh, ow)
    t64 = F.interpolate(x.double(), size=(oh, ow), mode="bilinear", align_corners=False)
    t32 = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
    torch.testing.assert_close(got, t64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got, t32.double(), rtol=1e-5, atol=1e-5)
    full = bilinear_ref(x, oh, ow, ca, y, cb)
    torch.testing.assert_close(full, ca.double().view(B, 1, 1, 1) * t64 + cb.double().view(B, 1, 1, 1) * y.double(), rtol=1e-12, atol=1e-12)
    if (h, w) == (oh, ow):
        assert torch.equal(got, x.double())
