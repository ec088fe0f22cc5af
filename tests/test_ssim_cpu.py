"""CPU tier of SSIM / multiscale SSIM: the float64 oracle (tests/ssim_ref.py) against properties that do not depend on
it, the op-by-op torch composition against the oracle, and argument validation without a device."""
import numpy as np
import pytest
import torch

import ssim_ref
from compression_amd import _lib
from compression_amd.ops import image_ops


def pair(seed, shape, degradation="noise8"):
    return ssim_ref.image_pair(seed, shape, degradation)


def test_oracle_identical_images_give_exactly_one():
    x, _ = pair(0, (161, 161, 3))
    assert ssim_ref.ssim_multiscale(x, x, 255) == 1.0
    assert ssim_ref.ssim(x, x, 255) == 1.0


def test_oracle_is_symmetric():
    x, y = pair(1, (2, 177, 203, 3))
    assert np.array_equal(ssim_ref.ssim_multiscale(x, y, 255), ssim_ref.ssim_multiscale(y, x, 255))
    assert np.array_equal(ssim_ref.ssim(x, y, 255), ssim_ref.ssim(y, x, 255))


def test_oracle_scale_invariance():
    """Images and max_val scaled together by 1/255 (what TensorFlow does to uint8 inputs) change nothing."""
    x, y = pair(2, (200, 180, 3), "blur")
    a = ssim_ref.ssim_multiscale(x, y, 255)
    b = ssim_ref.ssim_multiscale(x / 255.0, y / 255.0, 1.0)
    assert abs(a - b) < 1e-12
    assert abs(ssim_ref.ssim(x, y, 255) - ssim_ref.ssim(x / 255.0, y / 255.0, 1.0)) < 1e-12


def test_oracle_smallest_image():
    x, y = pair(3, (161, 161, 1))
    assert 0.0 < ssim_ref.ssim_multiscale(x, y, 255) < 1.0
    with pytest.raises(ValueError, match="161"):
        ssim_ref.ssim_multiscale(x[:160], y[:160], 255)


def test_oracle_odd_sizes():
    x, y = pair(4, (177, 203, 3))
    value, raw, sizes = ssim_ref.ssim_multiscale_parts(x, y, 255)
    assert sizes == [(177, 203), (89, 102), (45, 51), (23, 26), (12, 13)]
    assert raw.shape == (3, 5) and 0.0 < value < 1.0


def test_oracle_halving_repeats_the_last_row_and_column():
    a = np.arange(15, dtype=np.float64).reshape(3, 5)
    want = np.array([[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4, (4 + 4 + 9 + 9) / 4],
                     [(10 + 11) / 2, (12 + 13) / 2, 14.0]])
    assert np.array_equal(ssim_ref.halve(a), want)


@pytest.mark.parametrize("shape,degradation", [((161, 161, 1), "noise8"), ((2, 177, 203, 3), "blur"),
                                               ((256, 256, 4), "quant"), ((2, 2, 170, 190, 2), "noise20")])
def test_reference_float64_matches_the_oracle(shape, degradation):
    """Two independent compositions of one definition (convolutions / NumPy slices) pin each other."""
    x, y = pair(5, shape, degradation)
    tx, ty = torch.from_numpy(x).double(), torch.from_numpy(y).double()
    got = image_ops.ssim_multiscale_reference(tx, ty, 255)
    want = ssim_ref.ssim_multiscale(x, y, 255)
    assert got.dtype == torch.float64 and tuple(got.shape) == shape[:-3]
    assert np.abs(got.numpy() - want).max() <= 1e-10
    got1 = image_ops.ssim_reference(tx, ty, 255, filter_size=8, filter_sigma=1.0)
    assert np.abs(got1.numpy() - ssim_ref.ssim(x, y, 255, filter_size=8, filter_sigma=1.0)).max() <= 1e-10


def test_reference_float32_is_close():
    x, y = pair(6, (200, 200, 3))
    got = image_ops.ssim_multiscale_reference(torch.from_numpy(x), torch.from_numpy(y), 255)
    assert got.dtype == torch.float32
    assert abs(got.item() - ssim_ref.ssim_multiscale(x, y, 255)) < 1e-4


@pytest.mark.parametrize("fn", [image_ops.ssim_multiscale, image_ops.ssim_multiscale_reference])
def test_small_images_are_refused_on_the_host(fn):
    with pytest.raises(ValueError, match="smallest accepted side is 161"):
        fn(torch.zeros(160, 161, 3), torch.zeros(160, 161, 3), 255)
    with pytest.raises(ValueError, match="smallest accepted side is 97"):
        fn(torch.zeros(96, 200, 3), torch.zeros(96, 200, 3), 255, filter_size=7)


@pytest.mark.parametrize("fn", [image_ops.ssim, image_ops.ssim_multiscale, image_ops.ssim_reference,
                                image_ops.ssim_multiscale_reference])
def test_arguments_are_checked_on_the_host(fn):
    a = torch.zeros(200, 200, 3)
    with pytest.raises(ValueError, match="same shape"):
        fn(a, torch.zeros(200, 201, 3), 255)
    with pytest.raises(ValueError, match="filter_size"):
        fn(a, a, 255, filter_size=0)
    with pytest.raises(ValueError, match=r"\[\.\.\., H, W, C\]"):
        fn(torch.zeros(200, 200), torch.zeros(200, 200), 255)


@pytest.mark.parametrize("fn", [image_ops.ssim, image_ops.ssim_multiscale])
def test_filter_size_above_31_is_refused(fn):
    a = torch.zeros(600, 600, 3)
    with pytest.raises(ValueError, match="between 1 and 31"):
        fn(a, a, 255, filter_size=32)


def test_single_scale_minimum_is_the_window():
    with pytest.raises(ValueError, match="smallest accepted side is 11"):
        image_ops.ssim(torch.zeros(10, 40, 3), torch.zeros(10, 40, 3), 255)


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_entries_validate_on_the_host(entry):
    """Bad arguments are refused before any launch (null tensors, no device needed), with a text in tfc_last_error."""
    import ctypes as C
    lib = _lib.lib()
    taps = (C.c_float * 31)(*([1.0 / 31] * 31))

    def call(dtype=0, batch=1, height=64, width=64, channels=3, filter_size=11, c2=58.5, taps=taps):
        if entry == "forward":
            return lib.tfc_ssim_scale_forward(None, None, dtype, batch, height, width, channels, taps, filter_size,
                                              6.5, c2, None, None, None, None)
        return lib.tfc_ssim_scale_backward(None, None, dtype, batch, height, width, channels, taps, filter_size, 6.5,
                                           c2, None, None, None, None, None, None)
    for kw, word in ((dict(dtype=4), "dtype"), (dict(filter_size=0), "filter_size"), (dict(filter_size=32), "filter_size"),
                     (dict(taps=None), "taps"), (dict(batch=0), "batch"), (dict(channels=0), "channels"),
                     (dict(height=10), "smaller than the window"), (dict(width=10), "smaller than the window"),
                     (dict(c2=0.0), "c2"), (dict(c2=float("nan")), "c2"), (dict(), "null")):
        assert call(**kw) != 0
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.tfc_abi_version() == 2
