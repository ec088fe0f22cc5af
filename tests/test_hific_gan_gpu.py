"""GPU tier: HiFiC's discriminator, GAN loss and training step (csrc/hific_gan.hip, layers/spectral_norm.py,
models/hific.py, models/hific_train.py).  compare_gan is not part of the reference tree, so every comparison is against
the float64 torch restatement below of the definitions include/tfc_hip.h states, taken on the inputs as the kernels see
them (bfloat16-rounded for bfloat16)."""
import functools

import numpy as np
import pytest
import torch

from compression_amd.layers import SpectralNormConv2D, gan_functional
from compression_amd.models import hific, hific_train
from test_keras_conv_cpu import want_conv

pytestmark = pytest.mark.gpu

SLOPE, EPS = 0.2, 1e-12
# [R, C] of the reference discriminator's six kernels (archs.py:340-367 at base 64, 220 latent channels), one ragged
SN_SHAPES = [(1980, 12), (240, 64), (1024, 128), (2048, 256), (4096, 512), (8192, 1), (37, 5)]
# (cin, cout, support, stride) of the same six layers
LAYERS = [(220, 12, 3, 1), (15, 64, 4, 2), (64, 128, 4, 2), (128, 256, 4, 2), (256, 512, 4, 1), (512, 1, 4, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (any float dtype, any device)

def l2n(a):
    return a * torch.rsqrt(torch.clamp((a * a).sum(), min=EPS))


def sn_restated(w, u):
    """W [R, C], u [R] -> (W / sigma, u', v, sigma); u' and v are constants of sigma."""
    v = l2n(w.t() @ u).detach()
    u_new = l2n(w @ v).detach()
    sigma = u_new @ (w @ v)
    return w / sigma, u_new, v, sigma


def lrelu_restated(a):
    return torch.maximum(a, SLOPE * a)


def nearest_restated(t, H, W):
    h, w = t.shape[1:3]
    iy = torch.tensor([min((2 * d + 1) * h // (2 * H), h - 1) for d in range(H)], device=t.device)
    ix = torch.tensor([min((2 * d + 1) * w // (2 * W), w - 1) for d in range(W)], device=t.device)
    return t[:, iy[:, None], ix[None, :]]


def sce(x, z):
    return torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-x.abs()))


def gan_restated(logits):
    real, fake = logits.reshape(-1).chunk(2)
    return (sce(real, 1.0).mean() + sce(fake, 0.0).mean(), sce(fake, 1.0).mean(), torch.sigmoid(real).mean(),
            torch.sigmoid(fake).mean())


def conv_same(x, kernel, bias, stride):
    """TF `SAME` cross-correlation in the dtype of x (want_conv computes in float64)."""
    k = kernel.shape[0]
    pads = []
    for length in (x.shape[2], x.shape[1]):
        out = -(-length // stride)
        total = max((out - 1) * stride + k - length, 0)
        pads += [total // 2, total - total // 2]
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), pads)
    return torch.nn.functional.conv2d(xp, kernel.permute(3, 2, 0, 1).contiguous(), bias, stride=stride).permute(0, 2, 3, 1)


class RestatedDiscriminator:
    """archs.py:300-372 as tensor ops on copies of a Discriminator's parameters, in `dtype` on `device`."""

    def __init__(self, disc, dtype, device="cpu", act_dtype=None):
        """`act_dtype`: activations (and each normalised kernel and bias at its convolution) in another dtype than the
        parameters and their normalisation, as the kernels run bfloat16."""
        self.act_dtype = act_dtype or dtype
        layers = [disc.latent_conv] + list(disc.convs) + [disc.conv_out]
        self.strides = [m.strides for m in layers]
        self.kernels = [m.kernel.detach().to(device, dtype).clone().requires_grad_() for m in layers]
        self.biases = [m.bias.detach().to(device, dtype).clone().requires_grad_() for m in layers]
        self.us = [m.u.detach().to(device, dtype).reshape(-1).clone() for m in layers]
        self.training = True

    def parameters(self):
        return self.kernels + self.biases

    def conv(self, i, t):
        w = self.kernels[i]
        w_sn, u_new, _, _ = sn_restated(w.reshape(-1, w.shape[-1]), self.us[i])
        if self.training:
            self.us[i] = u_new
        return conv_same(t, w_sn.reshape(w.shape).to(self.act_dtype), self.biases[i].to(self.act_dtype), self.strides[i])

    def __call__(self, x, latent):
        t = nearest_restated(lrelu_restated(self.conv(0, latent)), x.shape[1], x.shape[2])
        t = torch.cat([x, t], dim=-1)
        for i in range(1, len(self.kernels) - 1):
            t = lrelu_restated(self.conv(i, t))
        logits = self.conv(len(self.kernels) - 1, t).reshape(-1, 1)
        return torch.sigmoid(logits), logits


def small_disc(seed=0):
    torch.manual_seed(seed)
    return hific.Discriminator(num_filters_base=16, in_channels_latent=32).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 3: spectral norm

def sn_inputs(R, C, seed=0):
    g = torch.Generator().manual_seed(seed + R + C)
    return (torch.randn(R, C, generator=g) * 0.02).cuda(), torch.randn(R, generator=g).cuda()


@pytest.mark.parametrize("R,C", SN_SHAPES)
def test_spectral_norm_forward(R, C):
    """W / sigma, u', v: 1e-5 relative to max(1, |want|) (the bar of test_gdn_gpu / test_channel_norm_gpu); sigma: 1e-5
    relative.  Where torch's float32 evaluation of the same formula itself misses a bar, the rule of
    test_forward_f32_shifted_mean applies: at most twice torch-float32's error plus the bar."""
    w, u = sn_inputs(R, C)
    got = gan_functional.spectral_norm_forward(w, u)
    want = sn_restated(w.double(), u.double())
    own = sn_restated(w, u)
    for name, g, t, ref in zip(("w_sn", "u'", "v", "sigma"), got, own, want):
        ref = ref.reshape(g.shape)
        scale = ref.abs() if name == "sigma" else torch.clamp(ref.abs(), min=1.0)
        e_kernel = ((g.double() - ref).abs() / scale).max().item()
        e_torch = ((t.reshape(g.shape).double() - ref).abs() / scale).max().item()
        bar = 1e-5 if e_torch <= 1e-5 else 2 * e_torch + 1e-5
        print(f"spectral norm {R}x{C} {name}: kernel err = {e_kernel:.3e}, torch float32 err = {e_torch:.3e}, bar = {bar:.3e}")
        assert e_kernel <= bar, name
    assert tuple(got[0].shape) == (R, C) and bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("R,C", SN_SHAPES)
def test_spectral_norm_backward(R, C):
    """dW against float64 autograd of the restatement (u', v detached): 1e-5 relative to the sum of the absolute terms
    of each element's reduction, |G / sigma| + sum |G W| / sigma^2 |u' v^T| (the dgamma / dbeta bar of
    test_channel_norm_gpu.py)."""
    w, u = sn_inputs(R, C, seed=1)
    grad = torch.randn(R, C, generator=torch.Generator().manual_seed(R)).cuda()
    w_sn, u_new, v, sigma = gan_functional.spectral_norm_forward(w, u)
    got = gan_functional.spectral_norm_backward(grad, w, u_new, v, sigma)
    wd = w.double().requires_grad_()
    want_sn, ud, vd, sd = sn_restated(wd, u.double())
    (want_sn * grad.double()).sum().backward()
    terms = (grad.double() / sd).abs() + (grad.double() * wd.detach()).abs().sum() / sd ** 2 * torch.outer(ud, vd).abs()
    err = ((got.double() - wd.grad).abs() / terms.detach()).max().item()
    print(f"spectral norm backward {R}x{C}: max err / sum |terms| = {err:.3e}")
    assert err <= 1e-5
    # and through the autograd wrapper
    wp = w.clone().requires_grad_()
    out, _ = gan_functional.spectral_norm(wp, u)
    (out * grad).sum().backward()
    assert torch.equal(wp.grad, got)


def test_spectral_norm_is_deterministic_and_u_follows_the_mode():
    for R, C in ((4096, 512), (37, 5)):
        w, u = sn_inputs(R, C, seed=2)
        a, b = gan_functional.spectral_norm_forward(w, u), gan_functional.spectral_norm_forward(w, u)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        grad = torch.randn(R, C, device="cuda")
        assert torch.equal(gan_functional.spectral_norm_backward(grad, w, *a[1:]),
                           gan_functional.spectral_norm_backward(grad, w, *a[1:]))
    torch.manual_seed(3)
    layer = SpectralNormConv2D(8, 3, in_channels=5).cuda()
    assert tuple(layer.u.shape) == (45, 1) and "u" in layer.state_dict() and "u" not in dict(layer.named_parameters())
    x = torch.randn(1, 6, 5, 5, device="cuda")
    u0 = layer.u.clone()
    layer.train()
    y_train = layer(x)
    u1 = layer.u.clone()
    assert not torch.equal(u0, u1)
    want_u = sn_restated(layer.kernel.detach().double().reshape(45, 8), u0.double().reshape(-1))[1]
    assert (u1.double().reshape(-1) - want_u).abs().max() <= 1e-5
    layer.eval()
    y_eval = layer(x)
    assert torch.equal(layer.u, u1) and torch.equal(layer(x), y_eval)
    assert not torch.equal(y_eval, y_train)              # the stored u has moved on by one iteration
    other = SpectralNormConv2D(8, 3, in_channels=5).cuda()
    other.load_state_dict(layer.state_dict())
    other.eval()
    assert torch.equal(other.u, u1) and torch.equal(other(x), y_eval)


# ---------------------------------------------------------------------------------------------------------------------
# 4: the layer

@pytest.mark.parametrize("cin,cout,k,s", LAYERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size", [(8, 6), (9, 7)])
def test_spectral_norm_conv_against_float64(cin, cout, k, s, dtype, size):
    """The bars of test_keras_conv_gpu.py: float32 2e-5 max(1, max |want|), bfloat16 2**-7 max(1, max |want|); the
    reference convolution uses the float64-normalised kernel (rounded to bfloat16 for bfloat16, as the kernels see it)."""
    torch.manual_seed(k + s + cin)
    layer = SpectralNormConv2D(cout, k, strides=s, in_channels=cin).cuda().eval()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout))
    x = torch.randn((2,) + size + (cin,), device="cuda").to(dtype)
    with torch.no_grad():
        y = layer(x)
    w = layer.kernel.detach().double()
    w_sn = sn_restated(w.reshape(-1, cout), layer.u.double().reshape(-1))[0].reshape(w.shape)
    want = want_conv(x.float().cpu(), w_sn.to(dtype).double().cpu(), layer.bias.detach().cpu(), k, s)
    assert tuple(y.shape) == tuple(want.shape) and y.dtype == dtype
    err = (y.double().cpu() - want).abs().max().item()
    bound = (2e-5 if dtype == torch.float32 else 2 ** -7) * max(1.0, want.abs().max().item())
    print(f"sn conv k={k} s={s} {cin}->{cout} {dtype} {size}: max err = {err:.3e}, bar = {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("cin,cout,k,s", LAYERS)
@pytest.mark.parametrize("lrelu", [False, True])
def test_spectral_norm_conv_gradients_against_float64(cin, cout, k, s, lrelu):
    """dx, dw, db through normalisation, convolution, bias (and leaky ReLU): 1e-4 max(1, max |ref|), the gradient bar of
    test_keras_conv_gpu.py."""
    torch.manual_seed(cin + cout)
    layer = SpectralNormConv2D(cout, k, strides=s, in_channels=cin).cuda().eval()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout) * 0.1)
    x = torch.randn(2, 9, 7, cin, device="cuda", requires_grad=True)
    y = layer(x, lrelu=lrelu)
    weight = torch.randn_like(y)
    (y * weight).sum().backward()
    xd = x.detach().cpu().double().requires_grad_()
    kd = layer.kernel.detach().cpu().double().requires_grad_()
    bd = layer.bias.detach().cpu().double().requires_grad_()
    w_sn = sn_restated(kd.reshape(-1, cout), layer.u.double().cpu().reshape(-1))[0].reshape(kd.shape)
    want = conv_same(xd, w_sn, bd, s)          # (want_conv's permuted kernel view has no CPU gradient at cout = 1)
    if lrelu:
        want = lrelu_restated(want)
    assert (y.detach().double().cpu() - want.detach()).abs().max() <= 2e-5 * max(1.0, want.abs().max().item())
    (want * weight.cpu().double()).sum().backward()
    for got, ref, name in ((x.grad, xd.grad, "dx"), (layer.kernel.grad, kd.grad, "dw"), (layer.bias.grad, bd.grad, "db")):
        err = (got.cpu().double() - ref).abs().max().item()
        bar = 1e-4 * max(1.0, ref.abs().max().item())
        print(f"sn conv grad k={k} s={s} {cin}->{cout} lrelu={lrelu} {name}: err = {err:.3e}, bar = {bar:.3e}")
        assert err <= bar, name


# ---------------------------------------------------------------------------------------------------------------------
# 5: front end

def front_composite(x, lat, P):
    """max(v, 0.2f v) in float32, rounded once; gather; concat; zero channels."""
    act = torch.maximum(lat.float(), torch.tensor(SLOPE, dtype=torch.float32, device=lat.device) * lat.float())
    out = torch.cat([x, nearest_restated(act.to(lat.dtype), x.shape[1], x.shape[2])], dim=-1)
    return torch.nn.functional.pad(out, (0, P - out.shape[-1]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,size,lsize", [(2, (64, 48), (4, 3)), (3, (50, 37), (4, 3)), (1, (5, 3), (7, 2))])
def test_front_end_forward_and_backward(dtype, n, size, lsize):
    """Forward: equal bits to the composite, zero padding channels.  Backward: dx equal bits; the latent gradient at 1e-5
    relative to the sum of the absolute terms (plus, for bfloat16, the rounding of the stored value, at most 2**-8 of
    it); two
    runs equal bits.  (64, 48) <- (4, 3) is an exact x 16; (50, 37) <- (4, 3) is ragged; (5, 3) <- (7, 2) shrinks one
    axis, so some sources have no replica."""
    g = torch.Generator().manual_seed(size[0] * 7 + lsize[0])
    x = torch.rand((n,) + size + (3,), generator=g).cuda().to(dtype)
    lat = torch.randn((n,) + lsize + (12,), generator=g).cuda().to(dtype)
    for P in (16, 32):
        out = gan_functional.disc_front_forward(x, lat, P)
        assert torch.equal(out, front_composite(x, lat, P)) and out.dtype == dtype
        assert torch.equal(out, gan_functional.disc_front_composite(x, lat, P))
        assert float(out[..., 15:].abs().max()) == 0.0
        grad = torch.randn(out.shape, generator=g).cuda().to(dtype)
        dx, dlat = gan_functional.disc_front_backward(grad, lat, 3)
        dx2, dlat2 = gan_functional.disc_front_backward(grad, lat, 3)
        assert torch.equal(dx, dx2) and torch.equal(dlat, dlat2)
        assert torch.equal(dx, grad[..., :3])
        # float64: scatter the replicas' gradients back onto their sources
        latd = lat.double().requires_grad_()
        nearest_restated(lrelu_restated(latd), *size).backward(grad[..., 3:15].double())
        mag = lat.double().requires_grad_()
        nearest_restated(mag * torch.where(lat > 0, 1.0, SLOPE).double(), *size).backward(grad[..., 3:15].double().abs())
        terms = mag.grad
        bar = 1e-5 * terms + (2 ** -8 * latd.grad.abs() if dtype == torch.bfloat16 else 0)
        excess = ((dlat.double() - latd.grad).abs() - bar).max().item()
        print(f"front end {dtype} {size} <- {lsize} P={P}: max |err| - bar = {excess:.3e}")
        assert excess <= 0
    # through autograd
    xg, lg = x.clone().requires_grad_(), lat.clone().requires_grad_()
    (gan_functional.disc_front(xg, lg, 32) * grad).sum().backward()
    assert torch.equal(xg.grad, dx) and torch.equal(lg.grad, dlat)


# ---------------------------------------------------------------------------------------------------------------------
# 6: leaky ReLU

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pixels,C", [(315, 61), (4099, 64), (33, 512), (7, 1)])
def test_leaky_relu_forward_and_backward(dtype, pixels, C):
    """Forward and the masked gradient: equal bits to max(v, 0.2f v) / gy (y > 0 ? 1 : 0.2f) in float32 rounded once.
    Bias sums: 1e-5 relative to the sum of the absolute terms; two runs equal bits.  315 x 61 has an odd pixel count
    and a ragged channel count, 4099 x 64 more than one workgroup with a ragged last one."""
    g = torch.Generator().manual_seed(pixels + C)
    y0 = torch.randn(pixels, C, generator=g).cuda().to(dtype)
    slope = torch.tensor(SLOPE, dtype=torch.float32, device="cuda")
    y = gan_functional.lrelu_(y0.clone())
    assert torch.equal(y, torch.maximum(y0.float(), slope * y0.float()).to(dtype))
    gy = torch.randn(pixels, C, generator=g).cuda().to(dtype)
    gm, db = gan_functional.lrelu_bias_backward(gy, y)
    gm2, db2 = gan_functional.lrelu_bias_backward(gy, y)
    assert torch.equal(gm, gm2) and torch.equal(db, db2)
    want32 = gy.float() * torch.where(y0 > 0, torch.ones_like(slope), slope)
    assert torch.equal(gm, want32.to(dtype))
    want = (gy.double() * torch.where(y0 > 0, 1.0, SLOPE).double())
    err = ((db.double() - want.sum(0)).abs() / want.abs().sum(0)).max().item()
    print(f"lrelu backward {dtype} {pixels}x{C}: bias err / sum |terms| = {err:.3e}")
    assert err <= 1e-5 and db.dtype == torch.float32
    # no activation: only the sums of gy
    same, plain = gan_functional.lrelu_bias_backward(gy, None)
    assert same is gy or torch.equal(same, gy)
    assert ((plain.double() - gy.double().sum(0)).abs() / gy.double().abs().sum(0)).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 7: GAN loss

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 333, 8192])
def test_gan_loss(dtype, M):
    """Logits N(0, 3^2) with +-50 and +-100 among them: the four scalars at 1e-5 relative to max(1, |want|), the
    gradients' errors times the element count at most 1e-5 (plus, for bfloat16, the rounding of the stored value, at most
    2**-8 of it), all
    finite."""
    g = torch.Generator().manual_seed(M)
    logits = torch.randn(2 * M, generator=g) * 3
    special = torch.tensor([50.0, -50.0, 100.0, -100.0])
    if M >= 4:
        logits[:4], logits[M:M + 4] = special, special
    else:
        logits = torch.tensor([100.0, -100.0])
    logits = logits.cuda().to(dtype)
    got = gan_functional.gan_loss_forward(logits)
    ld = logits.double().requires_grad_()
    want = gan_restated(ld)
    assert bool(torch.isfinite(got).all())
    for name, a, b in zip(("d_loss", "g_loss", "d_real", "d_fake"), got, want):
        err = abs(a.item() - b.item()) / max(1.0, abs(b.item()))
        print(f"gan loss {dtype} M={M} {name}: got {a.item():.6f}, want {b.item():.6f}, err = {err:.3e}")
        assert err <= 1e-5
    for mode, k in (("d_loss", 0), ("g_loss", 1)):
        ref, = torch.autograd.grad(want[k], ld, retain_graph=True)
        scale = torch.tensor(1.0, device="cuda")
        grad = gan_functional.gan_loss_backward(logits, scale, mode)
        assert bool(torch.isfinite(grad).all()) and grad.dtype == dtype and grad.shape == logits.shape
        slack = 2 ** -8 * ref.abs() * M if dtype == torch.bfloat16 else 0
        excess = ((grad.double() - ref).abs() * M - slack - 1e-5).max().item()
        print(f"gan loss {dtype} M={M} {mode} gradient: max (err * count - bar) = {excess:.3e}")
        assert excess <= 0
    # autograd: both losses from one forward
    lg = logits.clone().requires_grad_()
    d_loss, g_loss, d_real, d_fake = gan_functional.gan_losses(lg)
    (2.0 * d_loss + 3.0 * g_loss).backward()
    two, three = torch.tensor(2.0, device="cuda"), torch.tensor(3.0, device="cuda")
    want_grad = gan_functional.gan_loss_backward(logits, two, "d_loss") + gan_functional.gan_loss_backward(logits, three, "g_loss")
    assert torch.equal(lg.grad, want_grad) and not d_real.requires_grad


# ---------------------------------------------------------------------------------------------------------------------
# 8: fused against unfused

def disc_inputs(dtype, n=2, size=(64, 64), channels=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n,) + size + (3,), generator=g).cuda().to(dtype)
    latent = torch.round(torch.randn((n,) + hific.latent_size(*size) + (channels,), generator=g)).cuda().to(dtype)
    return x, latent


def run_disc(disc, fused, x, latent, weight=None):
    disc.fused = fused
    disc.eval()                                  # the same u in both runs
    for p in disc.parameters():
        p.grad = None
    xg = x.clone().requires_grad_()
    probs, logits = disc(xg, latent)
    if weight is None:
        weight = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).cuda().to(logits.dtype)
    (logits * weight).sum().backward()
    grads = {n: p.grad.clone() for n, p in disc.named_parameters()}
    grads["x"] = xg.grad.clone()
    return probs.detach(), logits.detach(), grads


def test_fused_discriminator_equals_the_unfused_one_f32():
    """float32: EQUAL BITS for the outputs and every gradient (the image's, every kernel's and bias's, the latent
    branch's included).  The fused pieces are elementwise (leaky ReLU and its mask) or pure data movement (concat,
    padding), and the bias sums go through the same kernel in the same order in both paths.  The one exception is the
    nearest resize, whose backward is a sum over each source pixel's replicas: the composite writes that sum as tensor
    ops in the order the kernel adds (gan_functional._NearestResizeFunction), so this also pins the kernel's order."""
    disc = small_disc()
    x, latent = disc_inputs(torch.float32)
    pa, la, ga = run_disc(disc, True, x, latent)
    pb, lb, gb = run_disc(disc, False, x, latent)
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert set(ga) == set(gb) and len(ga) == 2 * 6 + 1
    differ = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not differ, differ
    # the ragged front end too: 50 x 37 from 4 x 3
    xr = torch.rand(3, 50, 37, 3, device="cuda")
    lr = torch.randn(3, 4, 3, 12, device="cuda")
    weight = torch.randn(3, 50, 37, 32, device="cuda")
    grads = []
    for front in (gan_functional.disc_front, gan_functional.disc_front_composite):
        xg, lg = xr.clone().requires_grad_(), lr.clone().requires_grad_()
        (front(xg, lg, 32) * weight).sum().backward()
        grads.append((xg.grad, lg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_fused_layer_equals_the_unfused_one_bf16():
    """bfloat16, on the first body layer and on the front end (as test_fused_generator_equals_the_unfused_one compares on
    one block).  The fused leaky ReLU runs in place on the convolution's stored (rounded) output, so y, the masked
    gradient and with it dx and dw have EQUAL BITS.  db differs: fused adds the float32 products gy * slope, unfused their
    bfloat16 roundings; a bfloat16 rounding (8 significant bits) moves a value by at most 2**-8 of it, so the sums differ
    by at most 2**-8 sum |gm|, plus 1e-5 sum |gm| for two float32 summations.  Front end: forward and dx equal bits; the
    latent gradient is fused a = bf16(k S) against unfused b = bf16(k bf16(S)) with S the float32 sum of the replicas'
    gradients (the same order in both) and k the slope: one rounding separates a from k S, two separate b from k S, each
    at most 2**-8 / (1 - 2**-8) of the rounded value:  |a - b| <= 1.01 * 2**-8 (|a| + 2 |b|)."""
    torch.manual_seed(0)
    layer = SpectralNormConv2D(64, 4, strides=2, in_channels=15).cuda().eval()
    x = torch.randn(2, 16, 12, 32, device="cuda").to(torch.bfloat16)
    x[..., 15:] = 0
    outs = []
    for fused in (True, False):
        layer.zero_grad()
        xg = x.clone().requires_grad_()
        y = layer(xg, lrelu=True) if fused else torch.nn.functional.leaky_relu(layer(xg), SLOPE)
        weight = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).cuda().to(y.dtype)
        (y * weight).sum().backward()
        outs.append((y.detach(), xg.grad, layer.kernel.grad.clone(), layer.bias.grad.clone(), weight))
    (ya, dxa, dwa, dba, weight), (yb, dxb, dwb, dbb, _) = outs
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb) and torch.equal(dwa, dwb)
    gm = (weight.float() * torch.where(ya > 0, 1.0, SLOPE)).abs().sum(dim=(0, 1, 2))
    excess = ((dba - dbb).abs() - (2 ** -8 + 1e-5) * gm).max().item()
    print(f"fused vs unfused bf16 db: max |a - b| = {(dba - dbb).abs().max().item():.3e}, max excess = {excess:.3e}")
    assert excess <= 0
    xi, lat = disc_inputs(torch.bfloat16, channels=12)
    lat = lat * 0.37
    grads = []
    for front in (gan_functional.disc_front, gan_functional.disc_front_composite):
        xg, lg = xi.clone().requires_grad_(), lat.clone().requires_grad_()
        out = front(xg, lg, 32)
        weight = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).cuda().to(out.dtype)
        (out * weight).sum().backward()
        grads.append((out.detach(), xg.grad, lg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    a, b = grads[0][2].float(), grads[1][2].float()
    excess = ((a - b).abs() - 1.01 * 2 ** -8 * (a.abs() + 2 * b.abs())).max().item()
    print(f"fused vs unfused bf16 latent gradient: max |a - b| = {(a - b).abs().max().item():.3e}, max excess = {excess:.3e}")
    assert excess <= 0


# ---------------------------------------------------------------------------------------------------------------------
# 9: the whole discriminator

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_discriminator_against_the_float64_restatement(dtype):
    """Base 16, 32 latent channels, 64 x 64.  The bar is measured: twice the error of the SAME restatement evaluated by
    torch in the kernels' dtype (float32; for bfloat16, bfloat16 activations with float32 parameters cast per layer as
    the kernels do), plus one rounding of the output: 2e-5 max(1, max |want|) for float32 (the float32 bar of
    test_keras_conv_gpu.py), 2**-7 max(1, max |want|) for bfloat16."""
    disc = small_disc(seed=4).eval()
    with torch.no_grad():
        for m in [disc.latent_conv, disc.conv_out] + list(disc.convs):
            m.bias.normal_(0, 0.1)
    x, latent = disc_inputs(dtype, n=2)
    with torch.no_grad():
        probs, logits = disc(x, latent)
    assert tuple(logits.shape) == (2 * 8 * 8, 1) == tuple(probs.shape) and logits.dtype == dtype
    ref = RestatedDiscriminator(disc, torch.float64)
    ref.training = False
    own = RestatedDiscriminator(disc, torch.float32, act_dtype=dtype)
    own.training = False
    with torch.no_grad():
        want_p, want = ref(x.cpu().double(), latent.cpu().double())
        own_p, own_l = own(x.cpu(), latent.cpu())
    for name, got, t, w in (("logits", logits, own_l, want), ("probabilities", probs, own_p, want_p)):
        e_kernel = (got.double().cpu() - w).abs().max().item()
        e_torch = (t.double() - w).abs().max().item()
        bar = 2 * e_torch + (2e-5 if dtype == torch.float32 else 2 ** -7) * max(1.0, w.abs().max().item())
        print(f"discriminator {dtype} {name}: kernel err = {e_kernel:.3e}, torch {own_l.dtype} err = {e_torch:.3e}, bar = {bar:.3e}")
        assert e_kernel <= bar


# ---------------------------------------------------------------------------------------------------------------------
# 10: D learns

def learning_inputs():
    torch.manual_seed(0)
    x = torch.rand(4, 64, 64, 3)
    fake = torch.clamp(x + 0.2 * torch.randn(4, 64, 64, 3), 0, 1)
    latent = torch.round(torch.randn(4, 4, 4, 32))
    return x, fake, latent


def mean_drop(losses):
    return np.mean(losses[:5]) - np.mean(losses[-5:])


@functools.lru_cache(maxsize=None)
def restated_learning_curve():
    """60 Adam steps at 1e-3 on d_loss, the float32 restatement on the CPU (computed once)."""
    x, fake, latent = learning_inputs()
    ref = RestatedDiscriminator(small_disc(seed=0), torch.float32)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        _, logits = ref(torch.cat([x, fake]), torch.cat([latent, latent]))
        d_loss = gan_restated(logits)[0]
        d_loss.backward()
        opt.step()
        losses.append(float(d_loss.detach()))
    return tuple(losses)


def test_discriminator_learns():
    """mean(last 5) <= mean(first 5) - 0.3 for the restatement (else the inputs are unsuitable: an error, not a pass)
    and for the kernel path.  The restatement starts at 1.388 = 2 ln 2 and ends near 0.61; 0.3 leaves more than half of
    that 0.78 drop as room for a different float trajectory."""
    ref_losses = restated_learning_curve()
    print("restated d_loss:", " ".join(f"{v:.3f}" for v in ref_losses[::5]), f"drop {mean_drop(ref_losses):.3f}")
    if not mean_drop(ref_losses) >= 0.3:
        raise RuntimeError(f"inputs unsuitable: the restatement's d_loss drops by {mean_drop(ref_losses):.3f} only")
    x, fake, latent = (t.cuda() for t in learning_inputs())
    disc = small_disc(seed=0).train()
    opt = torch.optim.Adam(disc.parameters(), lr=1e-3)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        _, logits = disc(torch.cat([x, fake]), torch.cat([latent, latent]))
        d_loss = gan_functional.gan_losses(logits)[0]
        d_loss.backward()
        opt.step()
        losses.append(float(d_loss.detach()))
    print("kernel d_loss:  ", " ".join(f"{v:.3f}" for v in losses[::5]), f"drop {mean_drop(losses):.3f}")
    assert np.isfinite(losses).all() and mean_drop(losses) >= 0.3


# ---------------------------------------------------------------------------------------------------------------------
# 11: the trainer

def small_model(seed=0, **kw):
    from test_hific_gpu import small
    return small(seed=seed, **kw)


def batches(n, count=4, size=(64, 64), seed=3):
    from compression_amd import synthetic
    return [torch.from_numpy(synthetic.lowpass_images(count, size[0], size[1], seed=seed + i)).cuda().float()
            for i in range(n)]


def snapshot(module):
    return {n: p.detach().clone() for n, p in module.named_parameters()}


def changed(module, snap):
    return [n for n, p in module.named_parameters() if not torch.equal(p.detach(), snap[n])]


def bad_gradients(module):
    return [n for n, p in module.named_parameters()
            if p.grad is None or not bool(torch.isfinite(p.grad).all()) or not bool(p.grad.abs().sum() > 0)]


def test_trainer_phases():
    model, disc = small_model(seed=1), small_disc(seed=2)
    cfg = hific_train.CONFIGS["hific"]
    calls = []

    def perceptual(a, b):
        value = (a - b).abs().mean()
        calls.append(value.detach())
        return value
    trainer = hific_train.HiFiCTrainer(model, disc, cfg, perceptual_loss=perceptual, ignore_schedules=True)
    assert set(trainer.optimizers) == {"transform", "entropy", "disc"} and trainer.num_sub_batches == 2
    xd, xg = batches(2)
    # D phase
    model_before, disc_before = snapshot(model), snapshot(disc)
    model.zero_grad()
    d_out = trainer.discriminator_step(xd)
    assert not bad_gradients(disc), bad_gradients(disc)
    assert changed(model, model_before) == [] and len(changed(disc, disc_before)) > 0
    assert all(p.grad is None for p in model.parameters())
    assert not trainer.last_disc_latents.requires_grad and trainer.last_disc_latents.grad_fn is None
    assert set(d_out) == {"d_loss", "d_real", "d_fake"}
    # G phase
    disc_before = snapshot(disc)
    disc.zero_grad()
    g_out = trainer.generator_step(xg)
    assert not bad_gradients(model), bad_gradients(model)
    assert changed(disc, disc_before) == [] and all(p.grad is None for p in disc.parameters())
    assert all(p.requires_grad for p in disc.parameters())
    assert not trainer.last_disc_latents.requires_grad and trainer.last_disc_latents.grad_fn is None
    assert len(changed(model, model_before)) == len(model_before)
    lc = cfg.loss_config
    want_inv = 1 / lc.lmbda_a if float(g_out["total_qbpp"]) > lc.target else 1 / lc.lmbda_b
    assert float(g_out["lmbda_inv"]) == pytest.approx(want_inv, rel=1e-6)
    assert float(g_out["weighted_lpips"]) == pytest.approx(lc.lpips_weight * float(calls[-1]), rel=1e-6)
    assert float(g_out["rd_loss"]) == pytest.approx(float(g_out["weighted_R"]) + float(g_out["weighted_D"]), rel=1e-5)
    for name, value in {**d_out, **g_out}.items():
        assert bool(torch.isfinite(value).all()), name


def test_trainer_step_scalars_and_the_baseline_without_a_discriminator():
    model, disc = small_model(seed=3), small_disc(seed=4)
    trainer = hific_train.HiFiCTrainer(model, disc, hific_train.CONFIGS["hific"], ignore_schedules=True,
                                       perceptual_loss=lambda a, b: (a - b).abs().mean())
    out = trainer.train_step(batches(2))
    want = {"d_loss", "g_loss", "rd_loss", "weighted_R", "weighted_D", "lmbda_inv", "total_nbpp", "total_qbpp", "d_real",
            "d_fake", "weighted_lpips"}
    assert want <= set(out)
    for name in want:
        assert bool(torch.isfinite(out[name]).all()), name
    assert trainer.step == 1 and trainer.step_disc == 1
    with pytest.raises(ValueError, match="sub-batches"):
        trainer.train_step(batches(1))
    base = hific_train.HiFiCTrainer(small_model(seed=5), None, hific_train.CONFIGS["mselpips"], ignore_schedules=True)
    assert set(base.optimizers) == {"transform", "entropy"}
    out = base.train_step(batches(1))
    assert "g_loss" not in out and "d_loss" not in out and "weighted_lpips" not in out
    assert bool(torch.isfinite(out["rd_loss"]))
    with pytest.raises(ValueError, match="needs a discriminator"):
        hific_train.HiFiCTrainer(model, None, hific_train.CONFIGS["hific"])


def test_trainer_lowers_the_rd_loss():
    """Ten steps on one fixed batch: mean(last 3) < mean(first 3), as the existing HiFiC training test."""
    model, disc = small_model(seed=1), small_disc(seed=2)
    cfg = hific_train.CONFIGS["hific"]
    cfg = cfg._replace(lr=1e-3)
    trainer = hific_train.HiFiCTrainer(model, disc, cfg, ignore_schedules=True)
    fixed = batches(1)[0]
    losses = [float(trainer.train_step([fixed, fixed])["rd_loss"]) for _ in range(10)]
    print("trainer rd_loss:", " ".join(f"{v:.4f}" for v in losses))
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 12: the reference's sizes

@pytest.mark.slow
def test_reference_sizes_train_step_bf16():
    """One train_step in bfloat16, batch 8 of 256 x 256 per sub-batch, the reference's widths: the discriminator sees
    16 x 256 x 256 x 15 and 16 x 16 x 16 x 220.  Shapes and finiteness."""
    from compression_amd import synthetic
    torch.manual_seed(0)
    model = hific.HiFiCModel(compute_dtype=torch.bfloat16).cuda()
    disc = hific.Discriminator().cuda()
    trainer = hific_train.HiFiCTrainer(model, disc, hific_train.CONFIGS["hific"], ignore_schedules=True)
    xs = [torch.from_numpy(synthetic.lowpass_images(8, 256, 256, seed=s)).cuda().float() for s in (1, 2)]
    seen = []
    handle = disc.register_forward_hook(lambda m, args, out: seen.append((tuple(args[0].shape), tuple(args[1].shape),
                                                                           tuple(out[1].shape), out[1].dtype)))
    out = trainer.train_step(xs)
    handle.remove()
    assert seen == [((16, 256, 256, 3), (16, 16, 16, 220), (16 * 32 * 32, 1), torch.bfloat16)] * 2
    for name, value in out.items():
        assert value.numel() == 1 and bool(torch.isfinite(value).all()), name
