"""GPU tier: the integer convolution kernel (csrc/integer_conv.hip) against the loop definition of integer_conv_ref.py.
Every comparison is exact equality of every element.  These tests are also the check of the i8 MFMA's lane map."""
import numpy as np
import pytest
import torch

from integer_conv_ref import integer_conv2d_loops, rounding_cases, rounding_operands

pytestmark = pytest.mark.gpu

SUPPORTS = [(1, 1), (3, 3), (5, 5), (5, 3)]


def _constants():
    from compression_amd.ops import integer_ops
    return integer_ops.IC_CONSTANTS


def _kernel(x, w, b, c, stride, up, out_max=255):
    from compression_amd.ops import integer_conv2d
    dev = torch.device("cuda")
    y = integer_conv2d(torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev),
                       torch.from_numpy(c).to(dev), stride, bool(up), out_max)
    assert y.dtype == torch.uint8
    return y.cpu().numpy()


def _data(rng, batch, extent, cin, cout, support, unsigned):
    """Asymmetric random operands: every axis has its own extent and the values no symmetry a swapped index keeps."""
    shape = (batch,) + tuple(extent) + (cin,)
    x = rng.integers(0, 256, shape).astype(np.uint8) if unsigned else rng.integers(-128, 128, shape).astype(np.int8)
    w = rng.integers(-128, 128, tuple(support) + (cin, cout)).astype(np.int8)
    b = rng.integers(-(1 << 16), 1 << 16, cout).astype(np.int32)
    # divisors around the typical |v| so that the outputs spread over 0 ... 255 instead of saturating
    c = rng.integers(1 << 8, 1 << 12, cout).astype(np.int32)
    return x, w, b, c


def _check(x, w, b, c, stride, up, out_max=255):
    want = integer_conv2d_loops(x, w, b, c, stride, up, out_max)
    got = _kernel(x, w, b, c, stride, up, out_max)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} of {want.size} differ, first at {bad[0]}: "
                           f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
    return want


# (Cin, Cout, batch, extent): every Cin and Cout of the list, batch 1 and 3, extents 1x1 and 3x2
SHAPES = [(32, 1, 1, (1, 1)), (64, 17, 3, (3, 2)), (96, 16, 1, (3, 2)), (192, 64, 1, (1, 1)), (32, 192, 3, (3, 2))]


@pytest.mark.parametrize("unsigned", [0, 1])
@pytest.mark.parametrize("support", SUPPORTS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("up", [0, 1])
def test_random_data_matches_the_definition(up, stride, support, unsigned):
    rng = np.random.default_rng(1000 * up + 100 * stride + 10 * support[0] + 2 * support[1] + unsigned)
    spread = 0
    for cin, cout, batch, extent in SHAPES:
        x, w, b, c = _data(rng, batch, extent, cin, cout, support, unsigned)
        want = _check(x, w, b, c, stride, up)
        spread += int(((want > 0) & (want < 255)).sum())
    assert spread > 0          # the cases do not all saturate


def _edge_pixel_counts():
    k = _constants()
    counts = set()
    for name in ("IC_TILE_PIXELS", "IC_WAVE_PIXELS", "IC_BLOCK_PIXELS"):
        counts |= {k[name] - 1, k[name], k[name] + 1}
    return sorted(counts)


@pytest.mark.parametrize("unsigned", [0, 1])
@pytest.mark.parametrize("up,stride", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_extents_around_every_pixel_tile(up, stride, unsigned):
    """One below, at and one above every pixel-tile constant, as the pixels one workgroup grid axis walks (the output
    pixels going down, the pixels of one phase going up)."""
    rng = np.random.default_rng(7 + 2 * up + stride + 10 * unsigned)
    for pixels in _edge_pixel_counts():
        # `pixels` = 1 x width grid pixels; going down with stride 2 the input is twice as wide, less one
        width = pixels * stride - 1 if (not up and stride == 2) else pixels
        x, w, b, c = _data(rng, 1, (1, width), 32, 16, (3, 3), unsigned)
        _check(x, w, b, c, stride, up)
    # and as rows x columns across two images, so that a tile straddles a row and an image
    x, w, b, c = _data(rng, 2, (5, 13), 32, 20, (3, 5), unsigned)
    _check(x, w, b, c, stride, up)


@pytest.mark.parametrize("unsigned", [0, 1])
@pytest.mark.parametrize("up,stride", [(0, 1), (0, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("extent", [(3, 3), (2, 5)])
def test_saturated_operands_and_padding(extent, up, stride, unsigned):
    """All activations at their extreme with all weights 127, then -128, 5x5 support: every output pixel sees another
    count of in-image taps, so a wrong padding correction of the a - 128 representation cannot hide.  Bias at +-2^29,
    divisor at 1 and 2^24."""
    cin, cout = 64, 8
    for xval in ((255,) if unsigned else (-128, 127)):
        x = np.full((1,) + extent + (cin,), xval, np.uint8 if unsigned else np.int8)
        for wval in (127, -128):
            w = np.full((5, 5, cin, cout), wval, np.int8)
            for bias in (0, 1 << 29, -(1 << 29)):
                b = np.full(cout, bias, np.int32)
                b[1::2] = 0
                for div in (1, 1 << 10, 1 << 24):
                    c = np.full(cout, div, np.int32)
                    c[::4] = 1 << 14
                    _check(x, w, b, c, stride, up)
    # the largest reduction the layer takes (9 x 9 x 384 = 31104 <= 32768), saturated: the sum nears 2^30
    cin = 384
    x = np.full((1,) + extent + (cin,), 255 if unsigned else -128, np.uint8 if unsigned else np.int8)
    w = np.full((9, 9, cin, 4), 127 if unsigned else -128, np.int8)
    want = _check(x, w, np.full(4, 1 << 29, np.int32), np.full(4, 1 << 24, np.int32), stride, up)
    assert want.max() > 0


@pytest.mark.parametrize("unsigned", [0, 1])
def test_rounding_division(unsigned):
    cases = rounding_cases()
    x, w, b, c = rounding_operands(cases, unsigned)
    for out_max in (1, 63, 255):
        got = _check(x, w, b, c, 1, 0, out_max)[0, 0, 0]
        for o, (v, div, om, expected) in enumerate(cases):
            if om == out_max:
                assert got[o] == min(expected, out_max), (v, div, out_max)


@pytest.mark.parametrize("up,stride", [(0, 2), (1, 2)])
def test_batch_of_three_equals_each_image_alone_and_runs_repeat(up, stride):
    rng = np.random.default_rng(99 + up)
    x, w, b, c = _data(rng, 3, (7, 5), 64, 48, (5, 5), 1)
    whole = _kernel(x, w, b, c, stride, up)
    for i in range(3):
        assert np.array_equal(_kernel(x[i:i + 1], w, b, c, stride, up)[0], whole[i])
    again = _kernel(x, w, b, c, stride, up)
    assert again.tobytes() == whole.tobytes()
    assert np.array_equal(whole, integer_conv2d_loops(x, w, b, c, stride, up, 255))
