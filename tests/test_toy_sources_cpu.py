"""CPU tier: the toy-source family (compression_amd/models/toy_sources): the sources' closed forms, and the VECVQ and NTC
models on CPU tensors (where `ecvq_assign` is its tensor-op reference)."""
import math

import numpy as np
import pytest
import torch

import compression_amd as tfc
from compression_amd.models import toy_sources as ts

POINTS = torch.linspace(0.0, 1.0, 9)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("stationary", [True, False])
def test_sawbridge_closed_form(order, stationary):
    phase, drop = 0.3, 0.45
    source = ts.Sawbridge(POINTS, phase=phase, drop=drop, stationary=stationary, order=order)
    got = source.sample(4)
    t = torch.remainder(POINTS + torch.tensor(phase), 1.0) if stationary else POINTS
    want = (t - order * (drop < t).float()) * order ** -0.5
    assert tuple(got.shape) == (4, 9) and got.dtype == torch.float32
    assert torch.equal(got, want.expand(4, -1))
    assert tuple(source.event_shape) == (9,) and tuple(source.batch_shape) == ()


def test_sinusoid_and_ramp_closed_forms():
    phase = 0.2
    got = ts.Sinusoid(POINTS, phase=phase).sample(3)
    want = torch.sin((2 * math.pi) * (POINTS + torch.full((3, 1), phase)))
    assert torch.equal(got, want) and tuple(ts.Sinusoid(POINTS).event_shape) == (9,)
    got = ts.Ramp(POINTS, phase=phase).sample(3)
    want = torch.remainder(POINTS + torch.full((3, 1), phase), 1.0) - 0.5
    assert torch.equal(got, want) and tuple(ts.Ramp(POINTS).event_shape) == (9,)
    assert float(got.min()) >= -0.5 and float(got.max()) < 0.5


def test_sphere_samples_have_unit_norm():
    for order in (1, 2, 5):
        source = ts.Sphere(order=order)
        x = source.sample(1000, generator=torch.Generator().manual_seed(order))
        assert tuple(x.shape) == (1000, order) and tuple(source.event_shape) == (order,)
        assert float((x.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    band = ts.Sphere(order=3, width=0.2).sample(1000, generator=torch.Generator().manual_seed(0)).norm(dim=-1)
    assert float(band.min()) >= 1 / 1.1 - 1e-6 and float(band.max()) <= 1 / 0.9 + 1e-6 and float(band.std()) > 0.01


@pytest.mark.parametrize("make", [lambda: ts.Sawbridge(POINTS, order=2), lambda: ts.Sinusoid(POINTS),
                                  lambda: ts.Ramp(POINTS), lambda: ts.Sphere(order=3, width=0.1)],
                         ids=["sawbridge", "sinusoid", "ramp", "sphere"])
def test_a_fixed_generator_reproduces_the_samples(make):
    source = make()
    a = source.sample(17, generator=torch.Generator().manual_seed(3))
    b = source.sample(17, generator=torch.Generator().manual_seed(3))
    c = source.sample(17, generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape[0] == 17
    assert len(torch.unique(a, dim=0)) == 17                # the rows are separate draws


def vecvq(initialize="sample", distortion="sse", k=11):
    return ts.VECVQModel(k, initialize=initialize, source=ts.Sphere(order=3), lmbda=2.5, distortion_loss=distortion,
                         generator=torch.Generator().manual_seed(1))


@pytest.mark.parametrize("initialize", ["sample", "sample-0.1", "uniform-2.0"])
def test_vecvq_initialisers(initialize):
    model = vecvq(initialize)
    assert tuple(model.codebook.shape) == (11, 3) and tuple(model._logits.shape) == (11,)
    assert model.ndim_source == 3 and [n for n, _ in model.named_parameters()] == ["codebook", "_logits"]
    norms = model.codebook.detach().norm(dim=-1)
    if initialize == "sample":
        assert float((norms - 1).abs().max()) <= 1e-6
    if initialize == "sample-0.1":
        assert 1e-3 < float((norms - 1).abs().max()) < 1.0
    if initialize == "uniform-2.0":
        assert float(model.codebook.detach().abs().max()) <= 1.0
    with pytest.raises(ValueError):
        vecvq("grid")


@pytest.mark.parametrize("distortion", ["sse", "mse"])
def test_vecvq_losses_equal_the_explicit_path(distortion):
    model = vecvq(distortion=distortion)
    x = model.source.sample(3000, generator=torch.Generator().manual_seed(2)).reshape(30, 100, 3)
    rates, distortions = model.all_rd(x)
    assert tuple(rates.shape) == (11,) and tuple(distortions.shape) == (30, 100, 11)
    want = torch.argmin(rates + model.lmbda * distortions, dim=-1)
    codebook, got_rates, indexes = model.quantize(x)
    assert codebook is model.codebook and torch.equal(got_rates, rates)
    assert indexes.dtype == torch.int32 and torch.equal(indexes.long(), want)
    rate, dist = model.test_losses(x)
    assert torch.equal(rate, rates[want])
    torch.testing.assert_close(dist, torch.gather(distortions, -1, want[..., None])[..., 0], rtol=1e-6, atol=1e-7)
    assert model.train_losses(x)[0].requires_grad
    assert torch.equal(model.usage(x).long(), torch.bincount(want.reshape(-1), minlength=11))
    assert set(model.test_step(x)) == {"loss", "rate", "distortion"}


def ntc(prior_type, **kwargs):
    torch.manual_seed(0)
    kwargs.setdefault("dither", (1, 1, 0, 0))
    kwargs.setdefault("soft_round", (1, 0))
    return ts.NTCModel(torch.nn.Linear(3, 2), torch.nn.Linear(2, 3), prior_type=prior_type, source=ts.Sphere(order=3),
                       lmbda=4.0, distortion_loss="mse", generator=torch.Generator().manual_seed(1), **kwargs)


@pytest.mark.parametrize("prior_type", ["deep", "gmm-3"])
def test_ntc_shapes_and_equivalent_quantiser(prior_type):
    model = ntc(prior_type)
    assert model.ndim_latent == 2 and model.ndim_source == 3                 # found with a probe call of `analysis`
    assert ntc(prior_type, ndim_latent=2).ndim_latent == 2
    x = 3 * model.source.sample(200, generator=torch.Generator().manual_seed(2)).reshape(4, 50, 3)
    for losses in (model.train_losses, model.test_losses):
        rate, dist = losses(x)
        assert tuple(rate.shape) == (4, 50) and tuple(dist.shape) == (4, 50) and bool(torch.isfinite(rate).all())
        assert float(rate.detach().min()) > 0
    # dither off, soft rounding off: the codebook and indexes reproduce x_hat row for row
    y_hat, x_hat, rates = model.encode_decode(x, False, False, False)
    assert torch.equal(y_hat, torch.round(y_hat)) and tuple(y_hat.shape) == (4, 50, 2)
    codebook, code_rates, indexes = model.quantize(x)
    assert indexes.dtype == torch.int32 and tuple(indexes.shape) == (4, 50) and codebook.shape[1] == 3
    assert codebook.shape[0] == len(torch.unique(y_hat.reshape(-1, 2), dim=0)) > 1
    assert torch.equal(codebook[indexes.long()], x_hat) and torch.equal(code_rates[indexes.long()], rates)
    with pytest.raises(ValueError):
        model.analysis(torch.zeros(5, 4))


def test_ntc_priors_and_alpha():
    assert [n for n, _ in ntc("gsm-2").named_parameters() if n in ("logits", "log_scale", "loc")] == ["logits", "log_scale"]
    assert tuple(ntc("lmm-4").loc.shape) == (2, 4)
    with pytest.raises(ValueError):
        ntc("cauchy")
    model = ntc("deep")
    assert abs(float(model.alpha.detach()) - 4 / (1 + math.exp(3.0))) < 1e-6
    for value in (0.5, 2.0, 3.75):
        model.alpha = value
        assert abs(float(model.alpha) - value) < 1e-6
    model.force_alpha = None                                 # "not forced": train_step's assignment changes nothing
    assert float(model.force_alpha) == -1.0
    model.alpha = model.force_alpha
    assert abs(float(model.alpha) - 3.75) < 1e-6
    model.force_alpha = 1.25
    model.alpha = model.force_alpha
    assert abs(float(model.alpha) - 1.25) < 1e-6


@pytest.mark.parametrize("make", [lambda: vecvq(), lambda: ntc("deep"), lambda: ntc("lsm-2")],
                         ids=["vecvq", "ntc-deep", "ntc-lsm"])
def test_train_step_returns_the_metrics_and_moves_the_parameters(make):
    model = make()
    if hasattr(model, "alpha"):
        model.force_alpha = 2.0
    before = [p.detach().clone() for p in model.parameters()]
    optimizer = torch.optim.SGD(model.parameters(), lr=0.1)
    x = model.source.sample(256, generator=torch.Generator().manual_seed(3))
    metrics = model.train_step(x, optimizer)
    assert set(metrics) == {"loss", "rate", "distortion", "gradient RMS"}
    assert all(np.isfinite(float(v)) for v in metrics.values()) and float(metrics["gradient RMS"]) > 0
    assert abs(float(metrics["loss"]) - float(metrics["rate"]) - model.lmbda * float(metrics["distortion"])) < 1e-4
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    if hasattr(model, "alpha"):
        assert abs(float(model.alpha) - 2.0) < 0.05          # forced before the step, then moved by it


def test_exports():
    assert tfc.models.toy_sources.VECVQModel is ts.VECVQModel and tfc.models.NTCModel is ts.NTCModel
    assert callable(tfc.ecvq_assign) and callable(tfc.ecvq_counts) and callable(tfc.ecvq_assign_reference)
