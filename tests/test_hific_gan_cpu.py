"""CPU tier: the parts of HiFiC's GAN training that need no device — configuration constants, schedules, the
rate-target switch, the discriminator's shapes, the nearest-resize index arithmetic, and the host-side argument checks
of the new entry points (csrc/hific_gan.hip)."""
import pytest
import torch

from compression_amd import _lib
from compression_amd.layers import gan_functional
from compression_amd.models import hific, hific_train


def test_configuration_constants():
    """models/hific/configs.py:20-77, value by value."""
    for name, cp, steps_disc in (("hific", 0.1 * 1.5 ** 1, 1), ("mselpips", None, None)):
        cfg = hific_train.CONFIGS[name]
        assert cfg.lr == 1e-4 and cfg.num_steps_disc == steps_disc
        assert tuple(cfg.lambda_schedule.vals) == (2., 1.) and tuple(cfg.lambda_schedule.steps) == (50000,)
        assert tuple(cfg.lr_schedule.vals) == (1., 0.1) and tuple(cfg.lr_schedule.steps) == (500000,)
        lc = cfg.loss_config
        assert lc.CP == cp and lc.C == 0.1 * 2. ** -5 and lc.CD == 0.75 and lc.target == 0.14
        assert lc.lpips_weight == 1. and lc.lmbda_a == 0.1 * 2. ** -6 and lc.lmbda_b == 0.1 * 2. ** 1
        assert tuple(lc.target_schedule.vals) == (0.20 / 0.14, 1.) and tuple(lc.target_schedule.steps) == (50000,)
    assert set(hific_train.CONFIGS) == {"hific", "mselpips"}


def test_scheduled_value():
    """model.py:875-897: the first i with step < steps[i]; the last value beyond all steps."""
    cfg = hific_train.CONFIGS["hific"]
    lam, lr = cfg.lambda_schedule, cfg.lr_schedule
    assert hific_train.scheduled_value(3.0, lam, 0) == 6.0
    assert hific_train.scheduled_value(3.0, lam, 49999) == 6.0
    assert hific_train.scheduled_value(3.0, lam, 50000) == 3.0
    assert hific_train.scheduled_value(3.0, lam, 500000) == 3.0
    assert hific_train.scheduled_value(1e-4, lr, 49999) == 1e-4
    assert hific_train.scheduled_value(1e-4, lr, 499999) == 1e-4
    assert hific_train.scheduled_value(1e-4, lr, 500000) == 1e-4 * 0.1
    assert hific_train.scheduled_value(1e-4, lr, 10 ** 9) == 1e-4 * 0.1
    three = hific_train.Schedule(vals=(4., 2., 1.), steps=(10, 20))
    assert [hific_train.scheduled_value(1., three, s) for s in (9, 10, 19, 20, 21)] == [4., 2., 2., 1., 1.]
    with pytest.raises(ValueError, match="one more value than steps"):
        hific_train.scheduled_value(1., hific_train.Schedule(vals=(1.,), steps=(5,)), 0)


def test_rd_loss_switches_lambda_exactly_at_the_target():
    """model.py:79-102: lambda_a where total_qbpp > target, lambda_b otherwise — equality takes lambda_b."""
    cfg = hific_train.CONFIGS["hific"]
    lc = cfg.loss_config
    target = torch.tensor(lc.target, dtype=torch.float32)
    above = torch.nextafter(target, torch.tensor(1.0))
    below = torch.nextafter(target, torch.tensor(0.0))
    nbpp, distortion = torch.tensor(0.3), torch.tensor(40.0)
    for qbpp, lmbda in ((above, lc.lmbda_a), (target, lc.lmbda_b), (below, lc.lmbda_b)):
        loss, rate, dist, inv = hific_train.rd_loss(distortion, hific.BppPair(nbpp, qbpp), cfg, ignore_schedules=True)
        assert float(inv) == pytest.approx(1 / lmbda, rel=1e-6)
        assert float(rate) == pytest.approx(lc.C / lmbda * 0.3, rel=1e-6)
        assert float(dist) == pytest.approx(lc.C * lc.CD * 40.0, rel=1e-6)
        assert float(loss) == pytest.approx(float(rate) + float(dist), rel=1e-6)
    # with the schedules, step 0: lambdas doubled, target times 0.20 / 0.14
    _, _, _, inv = hific_train.rd_loss(distortion, hific.BppPair(nbpp, torch.tensor(0.19)), cfg, step=0)
    assert float(inv) == pytest.approx(1 / (2 * lc.lmbda_b), rel=1e-6)
    _, _, _, inv = hific_train.rd_loss(distortion, hific.BppPair(nbpp, torch.tensor(0.21)), cfg, step=0)
    assert float(inv) == pytest.approx(1 / (2 * lc.lmbda_a), rel=1e-6)
    _, _, _, inv = hific_train.rd_loss(distortion, hific.BppPair(nbpp, torch.tensor(0.19)), cfg, step=50000)
    assert float(inv) == pytest.approx(1 / lc.lmbda_a, rel=1e-6)


def test_rd_loss_rejects_lambda_a_not_below_lambda_b():
    cfg = hific_train.CONFIGS["hific"]
    pair = hific.BppPair(torch.tensor(0.3), torch.tensor(0.3))
    for a, b in ((0.2, 0.2), (0.3, 0.2)):
        bad = cfg._replace(loss_config=cfg.loss_config._replace(lmbda_a=a, lmbda_b=b))
        with pytest.raises(ValueError, match="Expected lmbda_a < lmbda_b"):
            hific_train.rd_loss(torch.tensor(1.0), pair, bad)


@pytest.mark.parametrize("size", [(64, 64), (50, 37), (256, 256)])
def test_discriminator_output_shapes(size):
    """archs.py:349-369: three stride-2 `SAME` convolutions (ceil(n / 2) each), two of stride 1; the latents come at
    latent_size (model.py:117-126)."""
    disc = hific.Discriminator()
    h, w = size
    want = (-(-(-(-(-(-h // 2)) // 2)) // 2), -(-(-(-(-(-w // 2)) // 2)) // 2))
    assert disc.output_size(h, w) == want
    assert [tuple(c.kernel.shape) for c in disc.convs] == [(4, 4, 15, 64), (4, 4, 64, 128), (4, 4, 128, 256),
                                                           (4, 4, 256, 512)]
    assert tuple(disc.latent_conv.kernel.shape) == (3, 3, 220, 12) and tuple(disc.conv_out.kernel.shape) == (4, 4, 512, 1)
    assert [c.strides for c in disc.convs] == [2, 2, 2, 1]
    assert tuple(disc.latent_conv.u.shape) == (1980, 1) and "latent_conv.u" in disc.state_dict()
    lh, lw = hific.latent_size(h, w)
    assert (lh, lw) == (-(-h // 16), -(-w // 16))
    assert float(disc.convs[0].bias.detach().abs().sum()) == 0.0
    assert 0.015 < float(disc.convs[3].kernel.detach().std()) < 0.025


def test_nearest_resize_indexes_against_brute_force():
    """src = min(floor((2 dst + 1) in / (2 out)), in - 1) is the nearest source of the destination's pixel centre
    ((dst + 1/2) in / out), found here by exact rational search; an integer factor f gives dst // f; and the closed form
    the backward kernel uses for the first replica of a source agrees with a scan."""
    from fractions import Fraction
    for size_in in range(1, 9):
        for size_out in range(1, 41):
            src = [gan_functional.nearest_source(d, size_in, size_out) for d in range(size_out)]
            for d, s in enumerate(src):
                centre = Fraction(2 * d + 1, 2) * size_in / size_out           # in source pixel units
                brute = max(k for k in range(size_in) if k <= centre)
                assert s == brute, (size_in, size_out, d)
            if size_out % size_in == 0:
                assert src == [d // (size_out // size_in) for d in range(size_out)]
            for s in range(size_in + 1):
                first = next((d for d in range(size_out) if src[d] >= s), size_out)
                assert gan_functional.nearest_first(s, size_in, size_out) == first, (size_in, size_out, s)


def test_new_entry_points_validate_on_the_host():
    """Bad scalar arguments are rejected before anything is launched (null tensors, no device needed)."""
    lib = _lib.lib()
    one = 1
    assert lib.tfc_spectral_norm_forward(None, None, 0, 4, None, None, None, None, None) != 0
    assert "rows must be in" in _lib.last_error()
    assert lib.tfc_spectral_norm_forward(None, None, 8, 0, None, None, None, None, None) != 0
    assert "cols must be in" in _lib.last_error()
    assert lib.tfc_spectral_norm_forward(None, None, 8, 4, None, None, None, None, None) != 0
    assert "null tensor" in _lib.last_error()
    assert lib.tfc_spectral_norm_backward(None, None, None, None, None, 8, 1 << 20, None, None) != 0
    assert "cols must be in" in _lib.last_error()
    assert lib.tfc_disc_front_forward(None, None, None, 2, one, 8, 8, 2, 2, 3, 12, 16, None) != 0
    assert "dtype" in _lib.last_error()
    assert lib.tfc_disc_front_forward(None, None, None, 0, one, 8, 8, 2, 2, 3, 14, 32, None) != 0
    assert "at most 16 together" in _lib.last_error()
    assert lib.tfc_disc_front_forward(None, None, None, 0, one, 8, 8, 2, 2, 3, 12, 14, None) != 0
    assert "multiple of 4" in _lib.last_error()
    assert lib.tfc_disc_front_backward(None, None, None, None, 0, one, 8, 0, 2, 2, 3, 12, 16, None) != 0
    assert "sizes must be positive" in _lib.last_error()
    assert lib.tfc_disc_front_backward(None, None, None, None, 0, one, 8, 8, 2, 2, 3, 12, 16, None) != 0
    assert "null tensor" in _lib.last_error()
    assert lib.tfc_lrelu_forward(None, 3, 16, None) != 0 and "dtype" in _lib.last_error()
    assert lib.tfc_lrelu_forward(None, 0, -1, None) != 0 and "non-negative" in _lib.last_error()
    assert lib.tfc_lrelu_bias_backward(None, None, None, None, 0, 16, 0, 1, None) != 0
    assert "channels must be in" in _lib.last_error()
    assert lib.tfc_gan_loss_forward(None, 0, 0, None, None) != 0 and "at least one real" in _lib.last_error()
    assert lib.tfc_gan_loss_backward(None, None, 0, 4, 2, None, None) != 0 and "mode must be" in _lib.last_error()


def test_new_ops_fail_loudly_without_device():
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    w, u = torch.randn(3, 3, 4, 5), torch.randn(36)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gan_functional.spectral_norm_forward(w, u)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gan_functional.disc_front_forward(torch.rand(1, 8, 8, 3), torch.randn(1, 2, 2, 12), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gan_functional.lrelu_(torch.randn(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gan_functional.gan_losses(torch.randn(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hific.Discriminator(num_filters_base=16, in_channels_latent=32)(torch.rand(1, 16, 16, 3),
                                                                       torch.randn(1, 1, 1, 32))
