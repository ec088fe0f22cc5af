"""GPU tier: the fused ChannelNorm kernels (csrc/channel_norm.hip) against a float64 evaluation of
models/hific/archs.py:255-273."""
import numpy as np
import pytest
import torch

from compression_amd.layers import ChannelNorm, functional
from test_channel_norm_cpu import numpy_channel_norm

pytestmark = pytest.mark.gpu

CHANNELS = [2, 3, 60, 61, 120, 220, 240, 480, 960, 1024]
FORMS = ["plain", "relu", "residual", "no_gamma", "no_beta"]


def inputs(C, seed, shape=(5, 7, 9)):
    """Standard normal with per-channel scales in [0.5, 2]; 315 pixels: no multiple of any tile."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape + (C,)) * rng.uniform(0.5, 2, C)).astype(np.float32)
    r = rng.standard_normal(x.shape).astype(np.float32)
    gamma = rng.uniform(0.5, 2, C).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    return x, r, gamma, beta


def run(form, x, r, gamma, beta, dtype):
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    g = None if form == "no_gamma" else gamma
    b = None if form == "no_beta" else beta
    res = r if form == "residual" else None
    xt = torch.from_numpy(x).cuda().to(dtype)
    rt = None if res is None else torch.from_numpy(res).cuda().to(dtype)
    y = functional.channel_norm(xt, dev(g), dev(b), 1e-3, form == "relu", rt)
    want = numpy_channel_norm(xt.float().cpu().numpy(), g, b, 1e-3, form == "relu",
                              None if rt is None else rt.float().cpu().numpy())
    return y, want


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("form", FORMS)
def test_forward_f32(C, form):
    """The project's GDN bar (tests/test_gdn_gpu.py:41-50): 1e-5 per element, relative to the element where it exceeds 1."""
    y, want = run(form, *inputs(C, C), torch.float32)
    err = np.abs(y.cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
    print(f"cnorm_f32 C={C} {form}: max err = {err.max():.3e} (max |want| = {np.abs(want).max():.3f})")
    assert y.dtype == torch.float32 and err.max() <= 1e-5


def test_forward_f32_shifted_mean():
    """Rows with mean 100 and unit spread.  The input's own float32 spacing (7.6e-6) sits at the bar, so the kernel is
    measured against torch's float32 evaluation of the same two-pass formula: at most twice its error (the reduction
    orders differ) plus 1e-5.  A one-pass E[x^2] - E[x]^2 kernel misses this by orders of magnitude."""
    for C in (60, 960):
        rng = np.random.default_rng(7)
        x = (100 + rng.standard_normal((315, C))).astype(np.float32)
        gamma = rng.uniform(0.5, 2, C).astype(np.float32)
        beta = rng.standard_normal(C).astype(np.float32)
        xt, gt, bt = (torch.from_numpy(a).cuda() for a in (x, gamma, beta))
        want = numpy_channel_norm(x, gamma, beta)
        got = functional.channel_norm(xt, gt, bt).cpu().numpy()
        own = functional.channel_norm_reference(xt, gt, bt).cpu().numpy()
        e_kernel, e_torch = np.abs(got - want).max(), np.abs(own - want).max()
        print(f"cnorm_f32 shifted mean C={C}: kernel max err = {e_kernel:.3e}, torch float32 two-pass = {e_torch:.3e}")
        assert e_kernel <= 2 * e_torch + 1e-5


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("form", FORMS)
def test_forward_bf16(C, form):
    """Against float64 on the bfloat16-rounded inputs: one bfloat16 ulp on the output (the bar of test_gdn_bf16); with
    a residual the bar applies to the sum."""
    y, want = run(form, *inputs(C, C + 1), torch.bfloat16)
    err = np.abs(y.float().cpu().numpy() - want) / (np.abs(want) + 1e-3)
    print(f"cnorm_bf16 C={C} {form}: max rel err = {err.max():.3e}")
    assert y.dtype == torch.bfloat16 and err.max() <= 2 ** -7


@pytest.mark.parametrize("C", [960, 60])
def test_bf16_stores_on_both_sides_of_the_non_temporal_line(C):
    """y leaves non-temporal where x + y exceed 128 MiB (csrc/channel_norm.hip): a tensor on each side of that line,
    ragged (odd) in pixels, gives the float64 values on a sample of its rows, and every row is written."""
    rng = np.random.default_rng(5)
    gamma = rng.uniform(0.5, 2, C).astype(np.float32)
    beta = (1 + rng.standard_normal(C)).astype(np.float32)
    gen = torch.Generator().manual_seed(11)
    big = (140 << 20) // (4 * C)                     # 140 MiB of x + y
    for pixels in (1000 + 7, big | 1):
        x = torch.randn(pixels, C, generator=gen).bfloat16()
        y = functional.channel_norm(x.cuda(), torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()).float().cpu()
        rows = torch.tensor([0, 1, 2, 7, 8, 9, pixels // 2, pixels - 10, pixels - 9, pixels - 3, pixels - 2, pixels - 1])
        want = numpy_channel_norm(x[rows].float().numpy(), gamma, beta)
        assert np.max(np.abs(y[rows].numpy() - want) / (np.abs(want) + 1e-3)) <= 2 ** -7, pixels
        assert torch.isfinite(y).all() and (y.abs().sum(dim=1) > 0).all()


def _float64_grads(x, g, gamma, beta, relu, eps=1e-3):
    x = x.double().requires_grad_()
    gamma, beta = gamma.double().requires_grad_(), beta.double().requires_grad_()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean.detach()) ** 2).sum(-1, keepdim=True) / (x.shape[-1] - 1)
    xhat = (x - mean) * torch.rsqrt(var + eps)
    pre = xhat * gamma + beta
    y = torch.relu(pre) if relu else pre
    dx, dgamma, dbeta = torch.autograd.grad(y, (x, gamma, beta), g.double())
    gp = g.double() * (pre > 0) if relu else g.double()
    return dx, dgamma, dbeta, (gp * xhat).abs().sum(0).detach(), gp.abs().sum(0)


@pytest.mark.parametrize("C", [60, 220, 960])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward(C, relu, dtype):
    """dx, dgamma, dbeta against float64 autograd.  float32 dx: the forward bar.  dgamma / dbeta are sums over P
    pixels: relative 1e-5 of sum_p |g' xhat| (resp. sum_p |g'|) per channel.  bfloat16 dx: 2**-7 as forward; the
    parameter gradients are float32 sums of float32 products of the bfloat16-rounded inputs: the same bar.  Two calls on
    the same inputs give identical bits."""
    xn, rn, gamma, beta = inputs(C, 3 * C + relu, shape=(3, 7, 15))
    x = torch.from_numpy(xn).cuda().to(dtype).reshape(-1, C)
    g = torch.from_numpy(rn).cuda().to(dtype).reshape(-1, C)
    gamma, beta = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    got = functional.channel_norm_backward(x, g, gamma, beta, 1e-3, relu)
    again = functional.channel_norm_backward(x, g, gamma, beta, 1e-3, relu)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    dx, dgamma, dbeta, scale_g, scale_b = _float64_grads(x.float(), g.float(), gamma, beta, relu)
    if dtype == torch.float32:
        e_dx = ((got[0].double() - dx).abs() / dx.abs().clamp(min=1)).max().item()
        bar = 1e-5
    else:
        e_dx = ((got[0].double() - dx).abs() / (dx.abs() + 1e-3)).max().item()
        bar = 2 ** -7
    e_g = ((got[1].double() - dgamma).abs() / scale_g.clamp(min=1e-30)).max().item()
    e_b = ((got[2].double() - dbeta).abs() / scale_b.clamp(min=1e-30)).max().item()
    print(f"cnorm backward {dtype} C={C} relu={relu}: dx err = {e_dx:.3e} (bar {bar:.1e}), dgamma rel = {e_g:.3e}, "
          f"dbeta rel = {e_b:.3e} (bar 1e-5)")
    assert e_dx <= bar and e_g <= 1e-5 and e_b <= 1e-5


@pytest.mark.parametrize("C,dtype", [(60, torch.bfloat16), (60, torch.float32), (120, torch.bfloat16),
                                     (220, torch.bfloat16), (960, torch.bfloat16), (61, torch.float32)])
def test_backward_with_epsilon_zero_on_a_ragged_pixel_count(C, dtype):
    """epsilon = 0 is a value the entries accept.  With 315 rows the last wave step of every layout with fewer than 64
    lanes per unit has lane groups past the last row; they hold zeros, whose rsqrt(0 + 0) = inf must not reach the
    parameter sums.  Against float64 autograd with epsilon = 0, bars as test_backward."""
    xn, rn, gamma, beta = inputs(C, 5 * C + 1)
    x = torch.from_numpy(xn).cuda().to(dtype).reshape(-1, C)
    g = torch.from_numpy(rn).cuda().to(dtype).reshape(-1, C)
    gamma, beta = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    for relu in (False, True):
        got = functional.channel_norm_backward(x, g, gamma, beta, 0.0, relu)
        assert all(bool(torch.isfinite(t).all()) for t in got), [bool(torch.isfinite(t).all()) for t in got]
        dx, dgamma, dbeta, scale_g, scale_b = _float64_grads(x.float(), g.float(), gamma, beta, relu, eps=0.0)
        if dtype == torch.float32:
            assert ((got[0].double() - dx).abs() / dx.abs().clamp(min=1)).max().item() <= 1e-5
        else:
            assert ((got[0].double() - dx).abs() / (dx.abs() + 1e-3)).max().item() <= 2 ** -7
        assert ((got[1].double() - dgamma).abs() / scale_g.clamp(min=1e-30)).max().item() <= 1e-5
        assert ((got[2].double() - dbeta).abs() / scale_b.clamp(min=1e-30)).max().item() <= 1e-5
    y = functional.channel_norm_forward(x, gamma, beta, 0.0)
    want = numpy_channel_norm(x.float().cpu().numpy(), gamma.cpu().numpy(), beta.cpu().numpy(), 0.0)
    bar = 1e-5 if dtype == torch.float32 else 2 ** -7
    scale = np.maximum(1.0, np.abs(want)) if dtype == torch.float32 else np.abs(want) + 1e-3
    assert (np.abs(y.float().cpu().numpy() - want) / scale).max() <= bar


@pytest.mark.parametrize("C", [3, 61, 60])
def test_backward_of_the_other_paths(C):
    """The wave-per-row kernel (C = 3, 61) and, with C = 60 in bfloat16, row pairs with an odd row left over (315 rows:
    157 pairs on the vector kernel, the last row and its partial sums on the wave-per-row kernel).  Bars as above."""
    for dtype in (torch.float32, torch.bfloat16):
        xn, rn, gamma, beta = inputs(C, C + 40)
        x = torch.from_numpy(xn).cuda().to(dtype).reshape(-1, C)
        g = torch.from_numpy(rn).cuda().to(dtype).reshape(-1, C)
        gamma_t, beta_t = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        got = functional.channel_norm_backward(x, g, gamma_t, beta_t, 1e-3, True)
        dx, dgamma, dbeta, scale_g, scale_b = _float64_grads(x.float(), g.float(), gamma_t, beta_t, True)
        if dtype == torch.float32:
            assert ((got[0].double() - dx).abs() / dx.abs().clamp(min=1)).max().item() <= 1e-5
        else:
            assert ((got[0].double() - dx).abs() / (dx.abs() + 1e-3)).max().item() <= 2 ** -7
        assert ((got[1].double() - dgamma).abs() / scale_g.clamp(min=1e-30)).max().item() <= 1e-5
        assert ((got[2].double() - dbeta).abs() / scale_b.clamp(min=1e-30)).max().item() <= 1e-5


def test_layer_trains_through_the_kernels():
    torch.manual_seed(0)
    layer = ChannelNorm().cuda()
    x = torch.randn(2, 6, 5, 120, device="cuda", requires_grad=True)
    r = torch.randn(2, 6, 5, 120, device="cuda", requires_grad=True)
    y = layer(x, residual=r)
    w = torch.randn_like(y)
    (y * w).sum().backward()
    assert torch.equal(r.grad, w)
    ref = ChannelNorm(num_channels=120)
    xc = x.detach().cpu().requires_grad_()
    (ref(xc, residual=r.detach().cpu()) * w.cpu()).sum().backward()
    assert (x.grad.cpu() - xc.grad).abs().max() <= 1e-4
    assert (layer.gamma.grad.cpu() - ref.gamma.grad).abs().max() <= 1e-3
    assert (layer.beta.grad.cpu() - ref.beta.grad).abs().max() <= 1e-3
    # non-contiguous input, rank 2, channels only
    xt = torch.randn(120, 33, device="cuda").t()
    assert torch.equal(layer(xt), layer(xt.contiguous()))
