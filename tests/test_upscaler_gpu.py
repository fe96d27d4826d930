"""GPU tests of the Real-ESRGAN upscaler: ``pv_dense_conv3x3`` alone against the fp64 contract of ``tests/_rrdb_ref.py`` (every form the model uses crossed
with ragged shapes, in place in a column slice of the input's own buffer, NaN around the operands and sentinels around the output, bit checks, one captured
replay), ``RRDBNet`` against the fp32 reference - whole, tiled, sub-batched, on its cached plan - and one end-to-end ``generate.py`` run in a fresh process.

Measured on MI355X: see EXPERIMENTS.md, "Real-ESRGAN upscaler"."""
import os
import subprocess
import sys

import pytest
import torch

from _rrdb_ref import (KERNEL_BOUND, KERNEL_FORMS, KERNEL_SHAPES, MODEL_BLOCKS, MODEL_CASES, TILE_CASE, TOL, WALK_FORMS, WALK_SHAPE, WALK_SHAPE_UPSAMPLE,
                       dense_conv_ref, element_bound, from_rows, kernel_case, pixels_case, rel_l2, seeded_ref, tile_process_ref, to_rows)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1234.0
IN_PLACE_FORMS = [f for f, d in KERNEL_FORMS.items() if d.get("inplace")]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _nan_rows(t_nchw, ld, extra_rows=3):
    """fp16 rows of an NCHW tensor in a NaN-filled buffer with the leading dimension ``ld`` and ``extra_rows`` rows behind the last image -> (buffer, view)."""
    rows = to_rows(t_nchw)
    buf = torch.full((rows.shape[0] + extra_rows, ld), float("nan"), dtype=torch.float16, device="cuda")
    buf[:rows.shape[0], :rows.shape[1]] = rows.cuda().half()
    return buf, buf[:rows.shape[0], :rows.shape[1]]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(c, in_place=False, padded=True, rec=None):
    """One launch on the operands of ``kernel_case`` -> (result NCHW on the CPU, the view the launch wrote, a check that nothing else was written).
    ``in_place``: the output is the column slice [cin, cin + cout) of the buffer the input lives in; every other column at or beyond cin holds NaN."""
    from photoverse_amd.ops import ACT_LEAKY_RELU, ACT_NONE, Recorder
    rec = Recorder(torch.device("cuda")) if rec is None else rec
    B, ho, wo, cin, cout = c["batch"], c["ho"], c["wo"], c["cin"], c["cout"]
    pad, extra = (8, 3) if padded else (0, 0)
    rows = B * ho * wo
    if in_place:
        assert not c["upsample"]
        xbuf, x = _nan_rows(c["x"], cin + cout + pad, extra)
        view = xbuf[:rows, cin:cin + cout]
        view.fill_(SENTINEL)
        buf = xbuf
    else:
        xbuf, x = _nan_rows(c["x"], cin + pad, extra)
        buf = torch.full((rows + extra, cout + 5 * pad), SENTINEL, dtype=torch.float16, device="cuda")
        view = buf[:rows, :cout]
    res = None if c["r"] is None else _nan_rows(c["r"], cout + 3 * pad, extra)[1]
    res2 = None if c["r2"] is None else _nan_rows(c["r2"], cout + pad, extra)[1]
    w, bias = c["w"].cuda().half().contiguous(), None if c["b"] is None else c["b"].cuda().contiguous()
    before = _bits(buf).clone()
    rec.dense_conv(x, w, bias, batch=B, h=c["h"], wd=c["wd"], upsample=c["upsample"], act=ACT_LEAKY_RELU if c["act"] == "leaky" else ACT_NONE, slope=0.2,
                   residual=res, alpha=c["alpha"], residual2=res2, beta=c["beta"], out=view)
    rec.run()
    torch.cuda.synchronize()
    got = from_rows(view.clone().cpu(), B, ho, wo)

    def untouched():
        after = buf.clone()
        after[:rows, (cin if in_place else 0):(cin if in_place else 0) + cout] = 0
        ref = before.view(torch.float16).view(buf.shape).clone()
        ref[:rows, (cin if in_place else 0):(cin if in_place else 0) + cout] = 0
        return torch.equal(_bits(after), _bits(ref))

    return got, view, untouched


def _check(form, shape):
    c = kernel_case(form, *shape)
    exact, mag = dense_conv_ref(c)
    got, _, untouched = _launch(c, in_place=c["inplace"])
    assert torch.isfinite(got).all(), (form, shape)
    err = rel_l2(got, exact)
    excess = ((got.double() - exact).abs() / element_bound(exact, mag)).max().item()
    print(f"pv_dense_conv3x3 {form} {shape}: rel-L2 vs fp64 = {err:.3e}; worst |error| / (half ulp + 32 * 2^-24 * sum |terms|) = {excess:.3f}")
    assert err <= KERNEL_BOUND
    assert excess <= 1.0
    assert untouched()                                                            # every byte outside the written slice is what it was
    return c, got


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(KERNEL_FORMS))
def test_kernel_matches_the_fp64_contract(form, shape):
    """``randn`` inputs, weights N(0, 1 / K), in buffers with padded leading dimensions: NaN in every column of x at or beyond cin that the launch does not
    write and in the rows behind the last image, a sentinel around the output; the dense forms write IN PLACE into the column slice behind their input.
    rel-L2 <= 1e-3, and every element inside half an fp16 ulp + 32 * 2^-24 * sum |terms|."""
    _need_gpu()
    _check(form, shape)


@pytest.mark.parametrize("form", WALK_FORMS)
def test_kernel_over_two_tiles_and_two_persistent_iterations(form):
    """17 x 33 output pixels are two 16 x 32 tiles in each direction, and 65 images make 260 tiles for the 256 persistent workgroups: four of them walk a
    second tile, whose first K slice is prefetched under the first tile's last (six slices at cin = 192)."""
    _need_gpu()
    _check(form, WALK_SHAPE_UPSAMPLE if form == "upsample" else WALK_SHAPE)


@pytest.mark.parametrize("form", ["dense160", "conv5_res2", "upsample", "body_res"])
def test_launches_are_deterministic_and_images_independent(form):
    _need_gpu()
    B, h, w = 3, 9, 17
    c = kernel_case(form, B, h, w)
    a, b = _launch(c, in_place=c["inplace"])[0], _launch(c, padded=False)[0]
    assert torch.equal(_bits(a), _bits(b))                                        # the same bits again, and the layout is addressing only
    for i in range(B):
        one = dict(c, batch=1, x=c["x"][i:i + 1], r=None if c["r"] is None else c["r"][i:i + 1], r2=None if c["r2"] is None else c["r2"][i:i + 1])
        assert torch.equal(_bits(_launch(one, in_place=c["inplace"])[0]), _bits(a[i:i + 1])), i


@pytest.mark.parametrize("form", IN_PLACE_FORMS)
def test_in_place_equals_out_of_place(form):
    """The column slice of the input's own buffer gets the bits a separate output buffer gets."""
    _need_gpu()
    for shape in ((2, 3, 5), (1, 17, 33)):
        c = kernel_case(form, *shape)
        here, _, untouched = _launch(c, in_place=True)
        apart, _, untouched_apart = _launch(c, in_place=False)
        assert torch.equal(_bits(here), _bits(apart)) and untouched() and untouched_apart(), (form, shape)


def test_a_whole_dense_block_in_one_buffer():
    """Five launches on one ``[rows][192]`` buffer - conv1 .. conv4 in place, conv5 with ``alpha = 0.2`` and the buffer's own columns 0-63 as the residual
    (and a second residual) - against the fp64 walk with one fp16 rounding per launch."""
    _need_gpu()
    from photoverse_amd.ops import ACT_LEAKY_RELU, Recorder
    import torch.nn.functional as F
    B, h, w = 2, 5, 7
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 64, h, w, generator=g).half()
    x0 = torch.randn(B, 64, h, w, generator=g).half()
    ws = [(torch.randn(32 if k < 4 else 64, 9 * (64 + 32 * k), generator=g) * (9 * (64 + 32 * k)) ** -0.5).half() for k in range(5)]
    bs = [torch.randn(32 if k < 4 else 64, generator=g) * 0.5 for k in range(5)]
    rec = Recorder(torch.device("cuda"))
    rows = B * h * w
    buf = torch.full((rows + 3, 192), float("nan"), dtype=torch.float16, device="cuda")
    buf[:rows, :64] = to_rows(x).cuda()
    outer = _nan_rows(x0, 72)[1]
    nxt = torch.full((rows + 3, 192), SENTINEL, dtype=torch.float16, device="cuda")
    blk = buf[:rows]
    for k in range(4):
        cin = 64 + 32 * k
        rec.dense_conv(blk, ws[k].cuda(), bs[k].cuda(), cin=cin, batch=B, h=h, wd=w, act=ACT_LEAKY_RELU, out=blk[:, cin:cin + 32])
    rec.dense_conv(blk, ws[4].cuda(), bs[4].cuda(), cin=192, batch=B, h=h, wd=w, residual=blk[:, :64], alpha=0.2, residual2=outer, beta=0.2, out=nxt[:rows, :64])
    rec.run()
    torch.cuda.synchronize()
    conv = lambda t, k: F.conv2d(t, ws[k].double().view(-1, 3, 3, t.shape[1]).permute(0, 3, 1, 2), bs[k].double(), padding=1)
    cat = x.double()
    for k in range(4):
        cat = torch.cat((cat, F.leaky_relu(conv(cat, k), 0.2).half().double()), 1)
    exp = (0.2 * (0.2 * conv(cat, 4) + x.double()) + x0.double())
    got = from_rows(nxt[:rows, :64].cpu(), B, h, w)
    err, err_cat = rel_l2(got, exp), rel_l2(from_rows(buf[:rows].cpu(), B, h, w), cat)
    print(f"dense block in one buffer: rel-L2 vs fp64 = {err:.3e} (output), {err_cat:.3e} (the 192 columns)")
    assert err <= KERNEL_BOUND and err_cat <= KERNEL_BOUND
    assert torch.isnan(buf[rows:]).all() and (nxt[rows:] == SENTINEL).all() and (nxt[:, 64:] == SENTINEL).all()
    assert torch.equal(_bits(buf[:rows, :64].cpu()), _bits(to_rows(x)))           # the block's input is still what it was


def test_graph_replay_equals_eager():
    """One captured ``pv_dense_conv3x3`` launch replays to the eager bits (nothing else is captured in this file)."""
    _need_gpu()
    from photoverse_amd.ops import Recorder
    c = kernel_case("conv5_res2", 2, 9, 17)
    rec = Recorder(torch.device("cuda"))
    eager, view, _ = _launch(c, rec=rec)
    view.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec.run()
    graph.replay()
    torch.cuda.synchronize()
    replayed = from_rows(view.clone().cpu(), c["batch"], c["ho"], c["wo"])
    del graph
    assert torch.equal(_bits(replayed), _bits(eager))


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module", params=MODEL_BLOCKS, ids=lambda n: f"blocks{n}")
def pair(request):
    _need_gpu()
    from photoverse_amd.upscaler import RRDBNet
    ref = seeded_ref(request.param)
    hip = RRDBNet(num_block=request.param)
    hip.load_state_dict(ref.state_dict())
    return ref, hip.to("cuda")


@pytest.mark.parametrize("shape", MODEL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_upscale_matches_the_reference(pair, shape):
    ref, hip = pair
    x = pixels_case(shape)
    got = hip.upscale(x.cuda())
    B, _, h, w = shape
    assert got.shape == (B, 3, 4 * h, 4 * w) and got.dtype == torch.float32 and got.abs().max() <= 1
    err = rel_l2(got, ref.upscale(x))
    print(f"RRDBNet({hip.num_block}) upscale {shape}: rel-L2 vs fp32 reference = {err:.3e}")
    assert err <= TOL
    plan = hip._plans[(B, h, w, got.device)]
    assert len(plan.rec) == 15 * hip.num_block + 7                                # 15 per RRDB, conv_first, conv_body, up1, up2, hr, conv_last, the clamp
    names = [fn.__name__ for fn, _ in plan.rec.calls]
    assert names.count("pv_dense_conv3x3") == 15 * hip.num_block + 4 and names.count("pv_tiny_conv3x3") == 2 and names[-1] == "pv_clamp_f32"
    n_plans = len(hip._plans)
    again = hip.upscale(x.cuda())                                                 # the cached plan: no new plan, the same bits
    assert len(hip._plans) == n_plans and hip._plans[(B, h, w, got.device)] is plan and torch.equal(again, got)


def test_tiled_upscale_matches_tile_process(pair):
    """``tile`` / ``tile_pad`` against Real-ESRGAN's ``tile_process`` around the fp32 reference (which the CPU suite shows to differ from the untiled image by
    more than 10 x TOL); a tile no smaller than the image is the untiled run, bit for bit; ``tile=None`` picks the tile from ``MAX_OPERAND_BYTES``."""
    ref, hip = pair
    x = pixels_case(TILE_CASE["shape"])
    tile, pad = TILE_CASE["tile"], TILE_CASE["tile_pad"]
    got = hip.upscale(x.cuda(), tile=tile, tile_pad=pad)
    err = rel_l2(got, tile_process_ref(ref.upscale, x, tile, pad))
    print(f"RRDBNet({hip.num_block}) tiled upscale {TILE_CASE}: rel-L2 vs tile_process on the fp32 reference = {err:.3e}")
    assert got.shape == (1, 3, 48, 80) and err <= TOL
    whole = hip.upscale(x.cuda())
    assert torch.equal(hip.upscale(x.cuda(), tile=32, tile_pad=pad), whole) and not torch.equal(got, whole)
    old = type(hip).MAX_OPERAND_BYTES
    try:
        hip.MAX_OPERAND_BYTES = 2048 * 100                                        # 12 x 20 does not fit, a 10 x 10 padded tile does: tile = 10 - 2 * pad
        auto = hip.upscale(x.cuda(), tile_pad=pad)
        with pytest.raises(ValueError, match="exceeds"):
            hip.upscale(x.cuda(), tile=16, tile_pad=pad)
    finally:
        hip.MAX_OPERAND_BYTES = old
    assert torch.equal(auto, got)


def test_sub_batched_run_gives_the_bits_of_the_whole_batch(pair):
    _, hip = pair
    x = pixels_case((3, 3, 5, 7)).cuda()
    whole = hip.upscale(x)
    assert hip._sub_batch(3, 5, 7) == 3 and (3, 5, 7, x.device) in hip._plans
    old = type(hip).MAX_OPERAND_BYTES
    try:
        hip.MAX_OPERAND_BYTES = 2 * 2048 * 5 * 7                                  # two images of the largest activation
        assert hip._sub_batch(3, 5, 7) == 2
        part = hip.upscale(x)                                                     # sub-batches of 2 and 1 through the plan of 2
    finally:
        hip.MAX_OPERAND_BYTES = old
    assert (2, 5, 7, x.device) in hip._plans and torch.equal(part, whole)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_generate_cli_upscales_the_saved_images(tmp_path):
    """``generate.py --upscaler_path random --upscaler_blocks 2`` in a fresh process: the PNGs are 4x the size of the run without the flag."""
    _need_gpu()
    from PIL import Image
    sizes = {}
    for name, extra in (("plain", []), ("upscaled", ["--upscaler_path", "random", "--upscaler_blocks", "2"])):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "generate.py"), "--model_path", "random", "--tiny", "--synthetic_input", "--latent_size", "16",
               "--num_timesteps", "2", "--results_dir", str(out)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        pngs = sorted(p for p in os.listdir(out) if p.endswith(".png"))
        assert pngs, r.stdout
        sizes[name] = [Image.open(os.path.join(out, p)).size for p in pngs]
    assert sizes["plain"] == [(128, 128)] * len(sizes["plain"]) and sizes["upscaled"] == [(512, 512)] * len(sizes["plain"])
