"""GPU tests of ``AutoencoderTiny``: ``pv_tiny_conv3x3`` alone against the fp64 contract of ``tests/_taesd_ref.py`` (every form the model uses crossed with
ragged shapes, NaN around the operands and sentinels around the output, bit checks), the model against the fp32 reference, its plans, and one end-to-end
``generate.py`` run in a fresh process.

Measured on MI355X: see EXPERIMENTS.md, "AutoencoderTiny"."""
import os
import subprocess
import sys

import pytest
import torch

from _taesd_ref import (DECODE_CASES, ENCODE_CASES, IMAGE_ULPS, KERNEL_BOUND, KERNEL_FORMS, KERNEL_SHAPES, TOL, WALK_SHAPE, conv_ref, from_rows, kernel_case,
                        latents_case, pixels_case, rel_l2, seeded_ref, to_rows)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1234.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _padded_rows(t_nchw, pad, extra_rows=3):
    """fp16 rows of an NCHW tensor in a buffer with the leading dimension ``64 + pad`` and ``extra_rows`` rows behind the last image: NaN everywhere else."""
    rows = to_rows(t_nchw)
    buf = torch.full((rows.shape[0] + extra_rows, rows.shape[1] + pad), float("nan"), dtype=torch.float16, device="cuda")
    buf[:rows.shape[0], :rows.shape[1]] = rows.cuda().half()
    return buf[:rows.shape[0], :rows.shape[1]]


def _launch(c, padded=True):
    """One launch on the operands of ``kernel_case`` -> (result NCHW on the CPU, the whole output buffer, the view the launch wrote)."""
    from photoverse_amd.ops import ACT_NONE, ACT_RELU, Recorder
    rec = Recorder(torch.device("cuda"))
    B, ho, wo, cout = c["batch"], c["ho"], c["wo"], c["cout"]
    if c["x_image"]:
        xb = torch.full((B + 1, *c["x"].shape[1:]), float("nan"), dtype=torch.float32, device="cuda")      # NaN behind the last image
        xb[:B] = c["x"].cuda()
        x = xb[:B]
    else:
        x = _padded_rows(c["x"], 8 if padded else 0, 3 if padded else 0)
    res = None if c["r"] is None else _padded_rows(c["r"], 24 if padded else 0, 3 if padded else 0)
    w, bias = c["w"].cuda().half().contiguous(), None if c["b"] is None else c["b"].cuda().contiguous()
    if c["out_image"]:
        buf = torch.full((B + 1, cout, ho, wo), SENTINEL, dtype=torch.float32, device="cuda")
        view = buf[:B]
    else:
        buf = torch.full((B * ho * wo + (3 if padded else 0), cout + (40 if padded else 0)), SENTINEL, dtype=torch.float16, device="cuda")
        view = buf[:B * ho * wo, :cout]
    rec.tiny_conv(x, w, bias, batch=B, h=c["h"], wd=c["wd"], stride=c["stride"], upsample=c["upsample"], act=ACT_RELU if c["act"] == "relu" else ACT_NONE,
                  residual=res, pre=c["pre"], image_out=c["out_image"], out_scale=c["scale"], out_shift=c["shift"], out=view)
    rec.run()
    torch.cuda.synchronize()
    got = view.clone().cpu() if c["out_image"] else from_rows(view.clone().cpu(), B, ho, wo)
    return got, buf, view


def _check(form, shape):
    c = kernel_case(form, *shape)
    exact, mag = conv_ref(c)
    got, buf, view = _launch(c)
    assert torch.isfinite(got).all(), (form, shape)
    if c["out_image"]:
        excess = ((got.double() - exact).abs() / (IMAGE_ULPS * mag)).max().item()
        print(f"pv_tiny_conv3x3 {form} {shape}: worst |error| / (32 * 2^-24 * sum |terms|) = {excess:.3f}")
        assert excess <= 1.0
    else:
        err = rel_l2(got, exact)
        print(f"pv_tiny_conv3x3 {form} {shape}: rel-L2 vs fp64 = {err:.3e}")
        assert err <= KERNEL_BOUND
    view.fill_(SENTINEL)
    assert torch.equal(buf, torch.full_like(buf, SENTINEL))                       # nothing outside the output was written
    return c, got


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(KERNEL_FORMS))
def test_kernel_matches_the_fp64_contract(form, shape):
    """``randn`` inputs, weights N(0, 1 / K), in buffers with padded leading dimensions: NaN in every input element that is not an operand element and behind
    the last image, a sentinel around the output.  fp16 outputs: rel-L2 <= 1e-3; fp32 image outputs: every element inside 32 * 2^-24 * sum |terms|."""
    _need_gpu()
    _check(form, shape)


@pytest.mark.parametrize("form", ["plain", "bias_res_relu", "stride2", "upsample", "image3_out"])
def test_kernel_over_two_tiles_and_two_persistent_iterations(form):
    """17 x 33 pixels are two tiles in each direction (three with ``upsample``, two 8 x 16 tiles after stride 2), and 65 images make more tiles than the 256
    persistent workgroups: some walk a second tile."""
    _need_gpu()
    _check(form, WALK_SHAPE)


@pytest.mark.parametrize("form", ["bias_res_relu", "stride2", "upsample", "image4_tanh3_in", "image3_out"])
def test_launches_are_deterministic_and_images_independent(form):
    _need_gpu()
    B, h, w = 3, 9, 17
    c = kernel_case(form, B, h, w)
    a, b = _launch(c)[0], _launch(c, padded=False)[0]
    assert torch.equal(a, b)                                                      # the same bits again, and the layout is addressing only
    for i in range(B):
        one = dict(c, batch=1, x=c["x"][i:i + 1], r=None if c["r"] is None else c["r"][i:i + 1])
        assert torch.equal(_launch(one)[0], a[i:i + 1]), i


def test_relu_output_has_no_negative_zero_and_no_nan():
    """A NaN-free input with plenty of negative pre-activations, eight channels whose conv and bias are exactly zero under a residual of -0.0 / -1, so that
    the activation sees zeros of either sign and negatives: every output is +0 or positive."""
    _need_gpu()
    c = kernel_case("bias_res_relu", 2, 9, 17)
    c["w"][:8] = 0.0
    c["b"][:8] = 0.0
    c["r"][:, :8] = -0.0
    c["r"][:, 4:8] = -1.0
    got = _launch(c)[0]
    assert torch.isfinite(got).all() and (got >= 0).all()
    assert not torch.signbit(got).any()                                           # no negative zero
    assert (got[:, :8] == 0).all() and (got > 0).any()


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def pair():
    _need_gpu()
    from photoverse_amd.vae_tiny import AutoencoderTiny
    ref = seeded_ref(0)
    hip = AutoencoderTiny()
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to("cuda")


@pytest.mark.parametrize("shape", DECODE_CASES, ids=lambda s: "x".join(map(str, s)))
@torch.no_grad()
def test_decode_matches_the_reference(pair, shape):
    ref, hip = pair
    z = latents_case(shape)
    got = hip.decode(z.cuda()).sample
    B, _, h, w = shape
    assert got.shape == (B, 3, 8 * h, 8 * w) and got.dtype == torch.float32
    err = rel_l2(got, ref.decode(z))
    print(f"AutoencoderTiny decode {shape}: rel-L2 vs fp32 reference = {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("shape", ENCODE_CASES, ids=lambda s: "x".join(map(str, s)))
@torch.no_grad()
def test_encode_matches_the_reference(pair, shape):
    ref, hip = pair
    x = pixels_case(shape)
    out = hip.encode(x.cuda())
    exp = ref.encode(x)
    assert out.latents.shape == exp.shape and out.latents.dtype == torch.float32
    err = rel_l2(out.latents, exp)
    print(f"AutoencoderTiny encode {shape}: rel-L2 vs fp32 reference = {err:.3e}")
    assert err < TOL
    assert torch.equal(out.latent_dist.sample(), out.latents) and torch.equal(out.latent_dist.mode(), out.latents)
    assert torch.equal(out.latent_dist.sample(generator=torch.Generator().manual_seed(1)), out.latents)


@torch.no_grad()
def test_sub_batched_run_gives_the_bits_of_the_whole_batch(pair):
    _, hip = pair
    z, x = latents_case((3, 4, 5, 7)).cuda(), pixels_case((3, 3, 13, 21)).cuda()
    whole, whole_l = hip.decode(z).sample, hip.encode(x).latents
    assert hip._sub_batch(3, 40, 56) == 3 and ("dec", 3, 5, 7, z.device) in hip._plans and ("enc", 3, 13, 21, x.device) in hip._plans
    old = type(hip).MAX_OPERAND_BYTES
    try:
        hip.MAX_OPERAND_BYTES = 2 * 64 * 40 * 56 * 2                              # two images of the decoder's largest activation
        assert hip._sub_batch(3, 40, 56) == 2
        part = hip.decode(z).sample                                                # sub-batches of 2 and 1 through the plan of 2
        hip.MAX_OPERAND_BYTES = 64 * 13 * 21 * 2
        part_l = hip.encode(x).latents                                             # one image at a time
    finally:
        hip.MAX_OPERAND_BYTES = old
    assert ("dec", 2, 5, 7, z.device) in hip._plans and ("enc", 1, 13, 21, x.device) in hip._plans
    assert torch.equal(part, whole) and torch.equal(part_l, whole_l)


def test_launch_count_and_activation_buffers(pair):
    """35 launches per direction whatever the batch, every one of them ``pv_tiny_conv3x3``; at most four distinct activation buffers per resolution level,
    also with more blocks per level."""
    from photoverse_amd.vae_tiny import AutoencoderTiny
    _, hip = pair
    dev = torch.device("cuda")
    for build, args in ((hip._plan_decode, (8, 8)), (hip._plan_encode, (40, 56))):
        p1, p3 = build(1, *args, dev), build(3, *args, dev)
        assert len(p1.rec) == len(p3.rec) == 35
        assert all(fn.__name__ == "pv_tiny_conv3x3" for fn, _ in p3.rec.calls)
        assert len(p3.levels) == 4 and all(1 <= len(bufs) <= 4 for bufs in p3.levels.values())
        ptrs = [t.data_ptr() for bufs in p3.levels.values() for t in bufs]
        assert len(set(ptrs)) == len(ptrs)
    deep = AutoencoderTiny(num_encoder_blocks=(2, 6, 6, 5), num_decoder_blocks=(6, 5, 6, 2)).to("cuda")
    for plan in (deep._plan_decode(2, 4, 4, dev), deep._plan_encode(2, 16, 24, dev)):
        assert len(plan.rec) == 3 * 19 + 5
        assert all(len(bufs) <= 4 for bufs in plan.levels.values())
        n_act = sum(len(bufs) for bufs in plan.levels.values())
        held = [t for t in plan.rec.keep if torch.is_tensor(t) and t.dtype == torch.float16 and t.dim() == 2 and t.shape[1] == 64 and t.shape[0] > 64]
        assert len({t.data_ptr() for t in held}) <= n_act <= 16                   # the recorder holds no activation beside the pools


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_generate_cli_runs_with_the_tiny_autoencoder(tmp_path):
    """``generate.py --vae_tiny_path random`` in a fresh process: the tiny autoencoder is the ``vae`` of ``run_inference`` and the PNGs are 128 px."""
    _need_gpu()
    from PIL import Image
    cmd = [sys.executable, os.path.join(ROOT, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
           "--num_timesteps", "2", "--vae_tiny_path", "random", "--results_dir", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pngs = sorted(p for p in os.listdir(tmp_path) if p.endswith(".png"))
    assert pngs, r.stdout
    for p in pngs:
        assert Image.open(os.path.join(tmp_path, p)).size == (128, 128)
