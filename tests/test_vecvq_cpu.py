"""CPU tier: `ecvq_assign_reference` against the float64 definition of tests/vecvq_ref.py, the host-side argument
checks of tfc_vecvq_assign / tfc_vecvq_backward, and the Python-side dtype and shape checks of `ecvq_assign`."""
import numpy as np
import pytest
import torch

import vecvq_ref
import compression_amd as tfc
from compression_amd import _lib
from compression_amd.ops import vq_ops

CHUNK = vq_ops.REFERENCE_CHUNK_ROWS
# (N, K, D): single row / codeword / dimension, odd sizes, and more rows than one chunk of the reference
SHAPES = [(1, 1, 1), (7, 5, 3), (33, 17, 2), (CHUNK + 1, 9, 4), (2 * CHUNK + 37, 6, 1)]


def make(n, k, d, dtype, seed=0):
    gen = torch.Generator().manual_seed(1000 * n + 10 * k + d + seed)
    x = torch.randn(n, d, generator=gen, dtype=torch.float32)
    codebook = x[torch.randint(n, (k,), generator=gen)] + 0.05 * torch.randn(k, d, generator=gen)
    logits = torch.randn(k, generator=gen)
    rates = (torch.logsumexp(logits, 0) - logits) / np.log(2.0)
    return x.to(dtype), codebook.to(dtype), rates.to(dtype), gen


@pytest.mark.parametrize("distortion", ["sse", "mse"])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_matches_the_float64_definition(shape, distortion):
    n, k, d = shape
    x, c, r, gen = make(n, k, d, torch.float64)
    c.requires_grad_(True); r.requires_grad_(True); x.requires_grad_(True)
    lmbda = 3.5
    index, rate, dist = tfc.ecvq_assign_reference(x, c, r, lmbda, distortion)
    assert index.dtype == torch.int32 and rate.dtype == torch.float64 and dist.dtype == torch.float64
    want_index, want_rate, want_dist = vecvq_ref.assign(x, c, r, lmbda, distortion)
    assert np.array_equal(index.numpy(), want_index)
    np.testing.assert_allclose(rate.detach().numpy(), want_rate, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dist.detach().numpy(), want_dist, rtol=1e-10, atol=1e-300)
    w_r = torch.randn(n, generator=gen, dtype=torch.float64)
    w_d = torch.randn(n, generator=gen, dtype=torch.float64)
    (w_r * rate + w_d * dist).sum().backward()
    d_r, d_c, d_x = vecvq_ref.gradients(x, c, want_index, w_r, w_d, distortion)
    for got, want in ((r.grad, d_r), (c.grad, d_c), (x.grad, d_x)):
        assert np.abs(got.numpy() - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_reference_ties_go_to_the_lowest_index_and_float32_stays_float32():
    x = torch.tensor([[0.0, 0.0], [2.0, 0.0]])
    c = torch.tensor([[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0], [3.0, 0.0]])
    r = torch.tensor([0.5, 0.5, 0.5, 0.5])
    index, rate, dist = tfc.ecvq_assign(x, c, r, 2.0)              # CPU tensors take the reference
    assert index.tolist() == [0, 0] and rate.dtype == torch.float32 and dist.tolist() == [1.0, 1.0]
    assert tfc.ecvq_counts(x, c, r, 2.0).tolist() == [2, 0, 0, 0]
    index, _, _ = tfc.ecvq_assign_reference(x.reshape(2, 1, 2), c, r, 2.0)
    assert tuple(index.shape) == (2, 1)
    forced, rate, _ = tfc.ecvq_assign_reference(x, c, r, 2.0, indexes=torch.tensor([3, 1]))
    assert forced.tolist() == [3, 1]


def test_entry_points_validate_on_the_host():
    """Bad scalar arguments are rejected before anything is launched (null tensors, no device needed)."""
    lib = _lib.lib()
    nan = float("nan")

    def assign(n, k, d, lmbda, kind):
        return lib.tfc_vecvq_assign(None, None, None, n, k, d, lmbda, kind, None, None, None, None, None)

    def backward(n, k, d, kind):
        return lib.tfc_vecvq_backward(None, None, None, None, None, n, k, d, kind, None, None, None, None)

    cases = [(lambda: assign(0, 0, 3, 1.0, 0), "K must be"), (lambda: assign(0, 4, 0, 1.0, 0), "D must be"),
             (lambda: assign(-1, 4, 3, 1.0, 0), "N must be"), (lambda: assign(0, 4, 3, nan, 0), "lmbda must be finite"),
             (lambda: assign(0, 4, 3, float("inf"), 0), "lmbda must be finite"),
             (lambda: assign(0, 4, 3, 1.0, 2), "distortion must be"), (lambda: backward(0, 0, 3, 0), "K must be"),
             (lambda: backward(0, 4, 0, 0), "D must be"), (lambda: backward(0, 4, 3, -1), "distortion must be")]
    for call, word in cases:
        assert call() != 0 and word in _lib.last_error(), (word, _lib.last_error())
    # N = 0 with good arguments: nothing to do, nothing launched
    assert assign(0, 4, 3, 1.0, 1) == 0 and backward(0, 4, 3, 1) == 0


def test_ecvq_assign_checks_dtype_and_shape_before_any_launch():
    """The dtype is looked at first (TypeError), the shapes next (ValueError); neither needs a device.  float64 is a
    TypeError wherever it would have to run on the float32 kernels' arguments: mixed with float32 here."""
    x = torch.zeros(4, 3)
    c = torch.zeros(5, 3)
    r = torch.zeros(5)
    with pytest.raises(TypeError):
        tfc.ecvq_assign(x.to(torch.bfloat16), c.to(torch.bfloat16), r.to(torch.bfloat16), 1.0)
    with pytest.raises(TypeError):
        tfc.ecvq_assign(x, c.double(), r, 1.0)
    with pytest.raises(TypeError):
        vq_ops._device_args(x.double(), c.double(), r.double(), 1.0, "sse")     # what a device tensor goes through
    with pytest.raises(TypeError):
        tfc.ecvq_assign(x.to(torch.bfloat16), torch.zeros(5, 2), r, 1.0)         # dtype before shape
    with pytest.raises(ValueError):
        tfc.ecvq_assign(x, torch.zeros(5, 2), r, 1.0)
    with pytest.raises(ValueError):
        tfc.ecvq_assign(x, c, torch.zeros(4), 1.0)
    with pytest.raises(ValueError):
        tfc.ecvq_assign(x, c, r, 1.0, distortion="l1")
    with pytest.raises(ValueError):
        tfc.ecvq_assign(x, c, r, float("nan"))


def test_kernel_constants_are_read_from_the_header():
    c = vq_ops.VQ_CONSTANTS
    for name in ("VQ_WAVE", "VQ_ROWS", "VQ_NARROW_MAX_D", "VQ_NARROW_CHUNK", "VQ_WIDE_KB", "VQ_WIDE_DT", "VQ_BWD_KT",
                 "VQ_BWD_DT", "VQ_BWD_SPLIT_ROWS"):
        assert c[name] >= 1, name
    assert c["VQ_WAVE"] == 64 and c["VQ_BWD_SPLIT_ROWS"] % (c["VQ_BWD_WAVES"] * c["VQ_WAVE"]) == 0
