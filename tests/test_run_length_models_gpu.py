"""PowerLawEntropyModel and LaplaceEntropyModel on the GPU: the cases of the reference's power_law_test.py and
laplace_test.py, restated in torch, plus byte equality of compress() with the restatement."""
import numpy as np
import pytest
import torch

import run_length_ref as ref

pytestmark = pytest.mark.gpu


def _models():
    import compression_amd as tfc
    return [("power_law", lambda **k: tfc.PowerLawEntropyModel(**k), (-1, -1, False)),
            ("laplace", lambda **k: tfc.LaplaceEntropyModel(**k), (-1, 0, False)),
            ("laplace_rice", lambda **k: tfc.LaplaceEntropyModel(run_length_code=2, magnitude_code=1,
                                                                 use_run_length_for_non_zeros=True, **k),
             (2, 1, True))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_quantizes_to_integers_with_straight_through_gradient(which):
    _, make, _ = _models()[which]
    em = make(coding_rank=1)
    x = torch.linspace(-20.0, 20.0, 100, device="cuda", requires_grad=True)
    y = em.quantize(x)
    assert torch.equal(y, torch.round(x.detach()))
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("rank,shape", [(0, (7, 5)), (1, (3, 100)), (2, (2, 4, 50)), (3, (2, 3, 4, 40))])
def test_compress_decompress_round_trip(which, rank, shape):
    _, make, codes = _models()[which]
    em = make(coding_rank=rank)
    g = torch.Generator().manual_seed(rank)
    x = (torch.randn(shape, generator=g) * 3).cuda()
    strings = em.compress(x)
    assert strings.shape == shape[:len(shape) - rank]
    units = torch.round(x).int().cpu().numpy().reshape((-1,) + shape[len(shape) - rank:])
    assert [bytes(s) for s in strings.reshape(-1)] == [ref.encode_np(u, *codes) for u in units]
    y = em.decompress(strings, shape[len(shape) - rank:])
    assert y.dtype == torch.get_default_dtype() and torch.equal(y, em.quantize(x))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_penalty_correlates_with_code_length(which):
    _, make, _ = _models()[which]
    em = make(coding_rank=1)
    g = torch.Generator().manual_seed(which)
    x = torch.randn(100, 100, generator=g) * torch.linspace(0.1, 20.0, 100)[:, None]
    x = x.cuda()
    strings = em.compress(x)
    lengths = np.array([8 * len(s) for s in strings], np.float64)
    penalty = em.penalty(em.quantize(x)).cpu().numpy().astype(np.float64)
    assert np.corrcoef(lengths, penalty)[0, 1] > .96


@pytest.mark.parametrize("which", [0, 1, 2])
def test_penalty_non_negative_and_gradient_sign(which):
    _, make, _ = _models()[which]
    em = make(coding_rank=1)
    x = torch.linspace(-20.0, 20.0, 100, device="cuda", requires_grad=True)
    p = em.penalty(x)
    assert float(p.detach()) >= 0
    p.backward()
    assert torch.equal(torch.sign(x.grad), torch.sign(x.detach()))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_dtypes(which, dtype):
    _, make, _ = _models()[which]
    em = make(coding_rank=1, bottleneck_dtype=dtype)
    assert em.bottleneck_dtype == dtype
    x = (torch.randn(4, 300) * 5).cuda()
    q, p = em(x)
    assert q.dtype == dtype and p.dtype == dtype and p.shape == (4,)
    y = em.decompress(em.compress(x), [300])
    assert y.dtype == dtype and torch.equal(y, torch.round(x.to(dtype)))


def test_power_law_bmshj2018_latent():
    import compression_amd as tfc
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(16, 48, 32, 192, generator=g) * 2).cuda()
    em = tfc.PowerLawEntropyModel(coding_rank=3)
    strings = em.compress(x)
    assert strings.shape == (16,)
    units = torch.round(x).int().cpu().numpy().reshape(16, -1)
    assert [bytes(s) for s in strings] == [ref.encode_np(u) for u in units]
    assert torch.equal(em.decompress(strings, [48, 32, 192]), torch.round(x))
