"""CPU-only tests of tiled VAE decode / encode (``AutoencoderKL.enable_tiling``): the tile grid and its integers for a hand-worked
case, the kept regions covering the output exactly once, every ``ValueError``, the new symbol in the header, the binding and the built library, and its
C-ABI rejections.  The fp64 torch reference of the blend recursion lives here (``blend_v_ref`` / ``blend_h_ref`` / ``tiled_ref``: diffusers' ``blend_v``,
``blend_h`` and tile loops spelled out, with their own loop bounds - nothing shared with the code under test); ``tests/test_vae_tiling_gpu.py`` compares
against it."""
import os
import re

import pytest
import torch

from photoverse_amd.vae import AutoencoderKL, tile_grid, tiling_geometry     # (module level: on a tree without the feature every test of this file fails at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32, scaling_factor=0.18215)


# ---------------------------------------------------------------------------------------------------------------- reference
def blend_v_ref(a, b, extent):
    """diffusers' ``blend_v`` in fp64: the first ``e`` rows of ``b`` against the LAST ``e`` rows of ``a``, ``e = min(rows(a), rows(b), extent)``."""
    b = b.double().clone()
    e = min(a.shape[2], b.shape[2], extent)
    for y in range(e):
        b[:, :, y, :] = a[:, :, -e + y, :].double() * (1 - y / e) + b[:, :, y, :] * (y / e)
    return b


def blend_h_ref(a, b, extent):
    b = b.double().clone()
    e = min(a.shape[3], b.shape[3], extent)
    for x in range(e):
        b[:, :, :, x] = a[:, :, :, -e + x].double() * (1 - x / e) + b[:, :, :, x] * (x / e)
    return b


def blend_rows_ref(rows, blend, keep, out_h, out_w):
    """The recursion over the results ``rows[i][j]`` (B, C, th, tw) of all tiles, in raster order: vertical blend against the already blended tile above,
    then horizontal against the already blended tile to the left, then the top-left ``keep x keep`` corner (clipped to the tile and to the image) into
    the output at ``(i * keep, j * keep)``.  fp64.  Also returns the blended tiles."""
    done = []
    b, c = rows[0][0].shape[:2]
    out = torch.full((b, c, out_h, out_w), float("nan"), dtype=torch.float64)
    for i, row in enumerate(rows):
        done.append([])
        for j, d in enumerate(row):
            d = d.double()
            if i > 0:
                d = blend_v_ref(done[i - 1][j], d, blend)
            if j > 0:
                d = blend_h_ref(done[i][j - 1], d, blend)
            done[i].append(d)
            kept = d[:, :, :keep, :keep][:, :, :out_h - i * keep, :out_w - j * keep]
            out[:, :, i * keep:i * keep + kept.shape[2], j * keep:j * keep + kept.shape[3]] = kept
    return out, done


def tiled_ref(x, fn, *, tile, stride, blend, keep, out_h, out_w):
    """diffusers' ``tiled_decode`` / ``tiled_encode``: ``fn`` on every ``tile x tile`` window of ``x`` at ``stride`` (clipped at the border), then
    ``blend_rows_ref``."""
    rows = [[fn(x[:, :, i:i + tile, j:j + tile]) for j in range(0, x.shape[3], stride)] for i in range(0, x.shape[2], stride)]
    return blend_rows_ref(rows, blend, keep, out_h, out_w)[0]


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def lib():
    from photoverse_amd.build import build_lib
    build_lib(verbose=False)              # hipcc cross-compiles gfx950 without a GPU
    from photoverse_amd import _lib
    return _lib.load()


def test_tile_grid_of_the_hand_worked_case():
    """T = 16, f = 0.25, up = 2: latent tile 8 at stride int(8 * 0.75) = 6, blend int(16 * 0.25) = 4 pixels, keep 12 = 6 * 2 pixels.  13 x 20 latents:
    row tiles start at 0 / 6 / 12 with heights 8 / 7 / 1 (13 - 6 = 7: clipped at the border), column tiles at 0 / 6 / 12 / 18 with widths 8 / 8 / 8 / 2.
    Kept pixels: rows 12 + 12 + 2 = 26, columns 12 + 12 + 12 + 4 = 40.  The encode direction of the same parameters: pixel tile 16 at stride 12, blend
    int(8 * 0.25) = 2 and keep 6 latents; a 26 x 40 image has row tiles 16 / 14 / 2 and column tiles 16 / 16 / 16 / 4 pixels."""
    g = tiling_geometry(16, 0.25, 2)
    d, e = g.decode, g.encode
    assert (d.tile, d.stride, d.blend, d.keep) == (8, 6, 4, 12) and (e.tile, e.stride, e.blend, e.keep) == (16, 12, 2, 6)
    assert tile_grid(13, d.tile, d.stride) == [(0, 8), (6, 7), (12, 1)]
    assert tile_grid(20, d.tile, d.stride) == [(0, 8), (6, 8), (12, 8), (18, 2)]
    assert [min(d.keep, n * 2) for _, n in tile_grid(13, 8, 6)] == [12, 12, 2] and [min(d.keep, n * 2) for _, n in tile_grid(20, 8, 6)] == [12, 12, 12, 4]
    assert tile_grid(26, e.tile, e.stride) == [(0, 16), (12, 14), (24, 2)] and tile_grid(40, e.tile, e.stride) == [(0, 16), (12, 16), (24, 16), (36, 4)]
    assert tile_grid(16, 8, 6) == [(0, 8), (6, 8), (12, 4)] and tile_grid(8, 8, 6) == [(0, 8), (6, 2)] and tile_grid(6, 8, 6) == [(0, 6)]
    # the defaults on SD-1.5 (up = 8): 48 * 8 = 384 = 512 - 128
    g = tiling_geometry(512, 0.25, 8)
    assert (g.decode.tile, g.decode.stride, g.decode.blend, g.decode.keep) == (64, 48, 128, 384)
    assert (g.encode.tile, g.encode.stride, g.encode.blend, g.encode.keep) == (512, 384, 16, 48)
    assert tile_grid(128, 64, 48) == [(0, 64), (48, 64), (96, 32)] and tile_grid(192, 64, 48) == [(0, 64), (48, 64), (96, 64), (144, 48)]
    # no overlap: the tiles abut and nothing is blended
    g = tiling_geometry(16, 0.0, 2)
    assert (g.decode.tile, g.decode.stride, g.decode.blend, g.decode.keep) == (8, 8, 0, 16)


@pytest.mark.parametrize("T,f,up", [(16, 0.25, 2), (16, 0.5, 2), (16, 0.75, 2), (16, 0.0, 2), (512, 0.25, 8), (64, 0.125, 8)])
def test_kept_regions_cover_the_output_exactly_once(T, f, up):
    g = tiling_geometry(T, f, up)
    for geo, sizes in ((g.decode, (1, 5, g.decode.tile, g.decode.tile + 1, 13, 20, 2 * g.decode.tile + 3)),
                       (g.encode, tuple(up * n for n in (1, 5, g.decode.tile, g.decode.tile + 1, 13, 20, 2 * g.decode.tile + 3)))):
        for size in sizes:
            out_size = size * geo.num // geo.den
            hits = torch.zeros(out_size, dtype=torch.int64)
            for i, (start, extent) in enumerate(tile_grid(size, geo.tile, geo.stride)):
                assert start == i * geo.stride and 1 <= extent <= geo.tile and start + extent <= size
                assert i * geo.keep == start * geo.num // geo.den                      # the kept region starts where the tile's own result starts
                kept = min(geo.keep, extent * geo.num // geo.den)
                hits[i * geo.keep:i * geo.keep + kept] += 1
                assert i * geo.keep + kept <= out_size
            assert torch.equal(hits, torch.ones_like(hits)), (T, f, up, size)


def test_reference_recursion_on_constants_and_on_a_hand_computed_ramp():
    # constant tiles: every blend is a convex combination of the constant
    rows = [[torch.full((2, 3, th, tw), 0.75) for tw in (16, 16, 16, 4)] for th in (16, 14, 2)]
    out, _ = blend_rows_ref(rows, 4, 12, 26, 40)
    assert out.shape == (2, 3, 26, 40) and torch.equal(out, torch.full_like(out, 0.75))
    # two tiles side by side, 0 on the left and 1 on the right, blend 4, keep 12: columns 12 ... 15 of the picture are the ramp 0, 1/4, 2/4, 3/4
    rows = [[torch.zeros(1, 1, 2, 16), torch.ones(1, 1, 2, 16)]]
    out, done = blend_rows_ref(rows, 4, 12, 2, 24)
    exp = torch.tensor([0.0] * 12 + [0.0, 0.25, 0.5, 0.75] + [1.0] * 8, dtype=torch.float64)
    assert torch.equal(out[0, 0, 0], exp) and torch.equal(out[0, 0, 1], exp)
    assert torch.equal(done[0][1][0, 0, 0], torch.tensor([0.0, 0.25, 0.5, 0.75] + [1.0] * 12, dtype=torch.float64))
    # one above the other, 2 above and 4 below; the lower tile is only 3 rows high: e = min(16, 3, 4) = 3, weights 0, 1/3, 2/3
    rows = [[torch.full((1, 1, 16, 2), 2.0)], [torch.full((1, 1, 3, 2), 4.0)]]
    out, _ = blend_rows_ref(rows, 4, 12, 15, 2)
    assert torch.allclose(out[0, 0, :, 0], torch.tensor([2.0] * 12 + [2.0, 2.0 + 2.0 / 3, 2.0 + 4.0 / 3], dtype=torch.float64), rtol=0, atol=1e-15)
    # an edge tile narrower than the blend extent reads the LAST e columns of its neighbour: a left tile whose columns are 0 ... 15, a right tile of
    # width 2 holding 100: e = 2, it blends against columns 14 and 15 -> 14 * 1 + 100 * 0, 15 * 1/2 + 100 * 1/2
    left = torch.arange(16.0).view(1, 1, 1, 16)
    got = blend_h_ref(left, torch.full((1, 1, 1, 2), 100.0), 4)
    assert torch.equal(got[0, 0, 0], torch.tensor([14.0, 57.5], dtype=torch.float64))
    # vertical first, then horizontal against the already blended left tile: the corner pixel (0, 0) of tile (1, 1) has weight 0 twice and ends as the
    # blended left tile's pixel, which is itself the last blended row of tile (0, 0)
    rows = [[torch.full((1, 1, 16, 16), 1.0), torch.full((1, 1, 16, 16), 2.0)], [torch.full((1, 1, 16, 16), 3.0), torch.full((1, 1, 16, 16), 4.0)]]
    out, done = blend_rows_ref(rows, 4, 12, 24, 24)
    assert done[1][1][0, 0, 0, 0] == 1.0 and done[1][1][0, 0, 0, 4] == 2.0 and done[1][1][0, 0, 4, 0] == 3.0 and done[1][1][0, 0, 4, 4] == 4.0
    # (2, 2): its own value is blended with tile (0, 1)'s blended pixel (1 * 0.5 + 2 * 0.5), then with tile (1, 0)'s blended pixel (1 * 0.5 + 3 * 0.5)
    assert done[1][1][0, 0, 2, 2] == (1.0 * 0.5 + 3.0 * 0.5) * 0.5 + ((1.0 * 0.5 + 2.0 * 0.5) * 0.5 + 4.0 * 0.5) * 0.5 == 2.375
    assert not torch.isnan(out).any()
    # tiled_ref on the identity with up = 1 geometry reproduces its input wherever nothing is blended, and constants everywhere
    x = torch.full((1, 2, 13, 20), -0.5)
    assert torch.equal(tiled_ref(x, lambda t: t, tile=8, stride=6, blend=2, keep=6, out_h=13, out_w=20), x.double())


def test_every_value_error_names_its_parameter():
    vae = AutoencoderKL(**TINY)                                        # up = 2
    assert vae.use_tiling is False
    for bad in (0, -16, 15, 16.0, "16", None, True):
        with pytest.raises(ValueError, match="tile_sample_min_size"):
            vae.enable_tiling(bad, 0.25)
    for bad in (-0.1, 1.0, 1.5, "0.25", None, float("nan")):
        with pytest.raises(ValueError, match="tile_overlap_factor"):
            vae.enable_tiling(16, bad)
    with pytest.raises(ValueError, match="tile_overlap_factor.*stride"):
        vae.enable_tiling(16, 0.9)                                     # int(8 * 0.1) = 0 latents between tiles
    with pytest.raises(ValueError, match="tile_sample_min_size.*tile_overlap_factor"):
        vae.enable_tiling(16, 0.3)                                     # stride int(5.6) = 5 latents = 10 pixels, keep 16 - int(4.8) = 12
    assert vae.use_tiling is False and (vae.tile_sample_min_size, vae.tile_overlap_factor) == (512, 0.25)      # a rejected call changes nothing
    with pytest.raises(ValueError, match="tile_sample_min_size.*tile_overlap_factor"):
        tiling_geometry(512, 0.3, 8)                                   # SD-1.5: K = 512 - 153 = 359, s * up = 44 * 8 = 352
    with pytest.raises(ValueError, match="tile_sample_min_size"):
        tiling_geometry(508, 0.25, 8)
    vae.enable_tiling(16, 0.25)
    assert vae.use_tiling is True and (vae.tile_sample_min_size, vae.tile_overlap_factor) == (16, 0.25)
    vae.disable_tiling()
    assert vae.use_tiling is False
    vae.enable_tiling()                                                # the defaults fit every power-of-two scale
    assert vae.use_tiling is True and (vae.tile_sample_min_size, vae.tile_overlap_factor) == (512, 0.25)
    with torch.device("meta"):
        AutoencoderKL().enable_tiling()                                # SD-1.5
    with pytest.raises(RuntimeError, match="HIP device"):
        vae.tiled_decode(torch.zeros(1, 4, 13, 20))                    # no CPU path, tiled or not


def test_symbol_is_declared_bound_and_exported_at_abi_19(lib):
    from photoverse_amd import _lib
    from photoverse_amd.build import SOURCES
    header = open(os.path.join(ROOT, "include", "photoverse_hip.h")).read()
    decl = re.search(r"^int32_t\s+pv_tile_blend\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    res, args = _lib.EXT_SIGNATURES["pv_tile_blend"]
    assert res is _lib.c_int and len(decl.split(",")) == len(args) == 19
    v, i = _lib.c_void_p, _lib.c_int
    assert args == [v, v, v, v, i, i, i, i, i, i, i, i, i, i, i, i, i, i, v]
    assert lib.pv_tile_blend.argtypes == args and "pv_tile_blend" not in _lib.SIGNATURES
    assert lib.pv_abi_version() == _lib.ABI_VERSION == 19 == int(re.search(r"#define PV_ABI_VERSION (\d+)", header).group(1))
    assert "pv_tile.hip" in SOURCES


def test_cabi_rejects_bad_arguments_before_touching_the_device(lib):
    """The launcher validates before its first HIP call and returns hipErrorInvalidValue = 1 (no GPU needed).  The pointers are never dereferenced; no
    valid call is sent."""
    INVALID = 1
    TILE, ABOVE, LEFT, OUT = 0x1000000, 0x2000000, 0x3000000, 0x4000000      # 16 MiB apart

    def blend(tile=TILE, above=ABOVE, left=LEFT, out=OUT, batch=2, ch=3, th=16, tw=16, ah=16, lw=16, ev=4, eh=4, kh=12, kw=12, oh=32, ow=32, oy=12, ox=12):
        return lib.pv_tile_blend(tile, above, left, out, batch, ch, th, tw, ah, lw, ev, eh, kh, kw, oh, ow, oy, ox, None)

    assert blend(tile=None) == INVALID and blend(out=None) == INVALID
    for name in ("tile", "above", "left", "out"):
        assert blend(**{name: 0x1000002}) == INVALID, name                 # not 4-byte aligned
    for name in ("batch", "ch", "th", "tw", "oh", "ow", "kh", "kw"):
        for bad in (0, -1):
            assert blend(**{name: bad}) == INVALID, (name, bad)
    # a neighbour comes with 1 <= e <= min(its extent, the tile's); no neighbour with e = 0
    for ev, ah, th in ((0, 16, 16), (-1, 16, 16), (5, 4, 16), (3, 16, 2), (17, 16, 16), (4, 0, 16), (4, -3, 16)):
        assert blend(ev=ev, ah=ah, th=th, kh=min(12, th)) == INVALID, (ev, ah, th)
    for eh, lw, tw in ((0, 16, 16), (-1, 16, 16), (5, 4, 16), (3, 16, 2), (17, 16, 16), (4, 0, 16), (4, -3, 16)):
        assert blend(eh=eh, lw=lw, tw=tw, kw=min(12, tw)) == INVALID, (eh, lw, tw)
    assert blend(above=None, ev=4) == INVALID and blend(left=None, eh=4) == INVALID
    # the kept region: inside the tile and inside out
    assert blend(kh=17) == INVALID and blend(kw=17) == INVALID
    assert blend(oy=-1) == INVALID and blend(ox=-4) == INVALID
    assert blend(oy=21) == INVALID and blend(ox=21) == INVALID and blend(oh=23) == INVALID and blend(ow=23) == INVALID
    assert blend(oy=2 ** 31 - 1) == INVALID and blend(ox=2 ** 31 - 1) == INVALID                   # no wrap-around in oy + keep_h
    # aliasing: the two written operands overlap nothing
    assert blend(out=TILE) == INVALID and blend(above=TILE) == INVALID and blend(left=TILE) == INVALID
    assert blend(above=OUT) == INVALID and blend(left=OUT) == INVALID
    assert blend(out=TILE + 4 * (2 * 3 * 16 * 16 - 1)) == INVALID                                    # the last element of tile
    assert blend(above=TILE - 4 * (2 * 3 * 16 * 16 - 1)) == INVALID                                  # its last element is tile's first
    assert blend(left=OUT + 4 * (2 * 3 * 32 * 32 - 1)) == INVALID
    # an operand of 2 GiB or more: 2^29 floats
    assert blend(batch=1, ch=1, th=1 << 15, tw=1 << 14, kh=12, kw=12, above=None, ev=0, left=None, eh=0) == INVALID
    assert blend(batch=1 << 10, ch=1 << 10, oh=32, ow=16, ox=0) == INVALID                           # out (and tile)
    assert blend(batch=8, ch=8, ah=1 << 20, th=16, tw=16) == INVALID                                  # above alone
    assert blend(batch=8, ch=8, lw=1 << 20) == INVALID                                                # left alone
    assert blend(batch=1 << 16, ch=1 << 16, th=1 << 16, tw=1 << 16, kh=1, kw=1) == INVALID           # no 64-bit wrap-around in the product
