"""GPU tier: the LPIPS kernels (csrc/lpips.hip) and the LPIPS module on them against the float64 definition of
tests/lpips_ref.py.

Bars.  Distance forward: relative error 1e-5, the project's float32 bar (torch float32 on the CPU sits near 2e-7 on these
inputs); 1e-4 on close inputs, which separates the difference form (3e-6) from the expanded one (2.4e-2).  Gradients and
the whole network have no number chosen in advance: each case also evaluates the same-dtype tensor-op composition on the
CPU and requires
    err_kernel <= 2 * err_composition + slack
(2: other reduction orders, and the float32 convolutions here run as six bfloat16 planes; slack 1e-6 in float32, and one
bfloat16 ulp, 2^-7, where the result itself is bfloat16 or went through bfloat16 features).  Both errors are printed."""
import functools

import pytest
import torch

import lpips_ref
import compression_amd as tfc
from compression_amd import _lib
from compression_amd.layers import functional

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
CHANNELS = [3, 64, 61, 192, 256, 384, 512]
BF16_ULP = 2.0 ** -7


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


@functools.lru_cache(maxsize=None)
def features(C, pixels, dtype, close=False, seed=0):
    """(f0, f1, w, g) on the CPU, f0 / f1 already rounded to `dtype`: ReLU'd normal features [3, pixels..., C].  With
    one pixel of three channels the two rows can be parallel (both (0, 0, x)): the distance is then 0 up to eps and a
    relative error of it measures nothing, so such a draw is taken again."""
    for attempt in range(100):
        gen = torch.Generator().manual_seed(100 * C + sum(pixels) + seed + 1000 * attempt)
        f0 = torch.relu(torch.randn((3,) + pixels + (C,), generator=gen))
        if close:
            f1 = torch.relu(f0 * (1 + 1e-3 * torch.randn(f0.shape, generator=gen)))
        else:
            f1 = torch.relu(torch.randn(f0.shape, generator=gen))
        w = torch.rand(C, generator=gen) / C
        g = torch.randn(3, generator=gen)
        f0, f1 = f0.to(dtype), f1.to(dtype)
        if close or float(lpips_ref.distance(f0, f1, w).min()) > 1e-3:
            return f0, f1, w, g
    raise AssertionError("no usable draw")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("pixels", [(5, 7), (1,)], ids=["P35", "P1"])
@pytest.mark.parametrize("C", CHANNELS)
def test_distance_forward(C, pixels, dtype):
    f0, f1, w, _ = features(C, pixels, dtype)
    want = lpips_ref.distance(f0, f1, w)
    got = functional.lpips_distance(f0.cuda(), f1.cuda(), w.cuda()).cpu()
    own = functional.lpips_distance_reference(f0, f1, w)
    err, err_torch = ((got - want).abs() / want.abs()).max(), ((own - want).abs() / want.abs()).max()
    print(f"lpips distance C={C} P={pixels} {dtype}: kernel rel err = {err:.3e}, torch float32 = {err_torch:.3e}")
    assert got.dtype == torch.float32 and got.shape == (3,) and err <= 1e-5


@pytest.mark.parametrize("C", [64, 384])
def test_distance_forward_close_inputs(C):
    """f1 = relu(f0 (1 + 1e-3 noise)): where a codec trains.  The expanded form a^2 S00 - 2 a b S01 + b^2 S11 cancels here."""
    f0, f1, w, _ = features(C, (5, 7), torch.float32, close=True)
    want = lpips_ref.distance(f0, f1, w)
    got = functional.lpips_distance(f0.cuda(), f1.cuda(), w.cuda()).cpu()
    err = ((got - want).abs() / want.abs()).max()
    print(f"lpips distance close inputs C={C}: kernel rel err = {err:.3e} (values {want.tolist()})")
    assert err <= 1e-4


def distance_grads(f0, f1, w, g, fn, device):
    # (copies: the inputs are shared between tests and must stay leaves without a gradient)
    a, b = (t.detach().clone().to(device).requires_grad_(True) for t in (f0, f1))
    fn(a, b, w.to(device)).backward(g.to(device))
    return a.grad.cpu(), b.grad.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("zero_pixel", [False, True], ids=["plain", "zero_pixel"])
@pytest.mark.parametrize("C", CHANNELS)
def test_distance_backward(C, zero_pixel, dtype):
    """df0 and df1 against the explicit-form float64 gradient, in relative L2: at most twice the error of the float32
    tensor-op reference on the same inputs plus 1e-6.  bfloat16 gradients are the reference's rounded to bfloat16 (the
    format's own error, about 2^-9 per element, is then on both sides).  zero_pixel: one all-zero row in f0 and one in
    f1, where sqrt's own derivative is inf * 0."""
    f0, f1, w, g = features(C, (5, 7), dtype, seed=1)
    if zero_pixel:
        f0, f1 = f0.clone(), f1.clone()
        f0[1, 2, 3] = 0
        f1[2, 4, 6] = 0
    _, want0, want1 = lpips_ref.distance_with_grads(f0, f1, w, g)
    got0, got1 = distance_grads(f0, f1, w, g, functional.lpips_distance, "cuda")
    own0, own1 = distance_grads(f0.float(), f1.float(), w, g, functional.lpips_distance_reference, "cpu")
    assert got0.dtype == dtype and got0.shape == f0.shape and got1.shape == f1.shape
    assert bool(torch.isfinite(got0).all()) and bool(torch.isfinite(got1).all())
    # the zero rows apart from the rest: the gradient at an all-zero pixel is e / eps, ten orders above the others
    zero0, zero1 = torch.zeros(f0.shape[:-1], dtype=torch.bool), torch.zeros(f0.shape[:-1], dtype=torch.bool)
    if zero_pixel:
        zero0[1, 2, 3] = zero1[2, 4, 6] = True
    for name, got, own, want, zero in (("df0", got0, own0, want0, zero0), ("df1", got1, own1, want1, zero1)):
        want, own = want.reshape(got.shape), own.reshape(got.shape).to(dtype)
        for rows in ([~zero, zero] if zero_pixel else [~zero]):
            e_kernel, e_torch = rel_l2(got[rows], want[rows]), rel_l2(own[rows], want[rows])
            print(f"lpips distance backward C={C} {dtype} zero_pixel={zero_pixel} {name} ({int(rows.sum())} rows): "
                  f"kernel = {e_kernel:.3e}, torch float32 = {e_torch:.3e}")
            assert e_kernel <= 2 * e_torch + 1e-6


@pytest.mark.parametrize("C", [64, 61])
def test_distance_backward_mask_and_determinism(C):
    f0, f1, w, g = (t.cuda() for t in features(C, (5, 7), torch.float32, seed=2))
    lib, n, p = _lib.lib(), 3, 35
    both = [torch.empty_like(f0), torch.empty_like(f1)]
    _lib.check(lib.tfc_lpips_distance_backward(g.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(),
                                               both[0].data_ptr(), both[1].data_ptr(), 0, n, p, C, 1e-10, 3,
                                               _lib.stream_ptr()))
    for mask in (1, 2):
        out = [torch.full_like(f0, 7.0), torch.full_like(f1, 7.0)]
        _lib.check(lib.tfc_lpips_distance_backward(g.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(),
                                                   out[0].data_ptr(), out[1].data_ptr(), 0, n, p, C, 1e-10, mask,
                                                   _lib.stream_ptr()))
        kept, written = (1, 0) if mask == 1 else (0, 1)
        assert torch.equal(out[kept], torch.full_like(f0, 7.0)) and torch.equal(out[written], both[written])
    # through autograd: f1 without a gradient gets none, and two calls give the same bits
    results = []
    for _ in range(2):
        a = f0.clone().requires_grad_(True)
        d = functional.lpips_distance(a, f1, w)
        d.backward(g)
        results.append((d.detach().clone(), a.grad.clone()))
        assert f1.grad is None and torch.equal(a.grad, both[0])
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_distance_validates_on_the_host():
    f = torch.zeros(2, 4, 8, device="cuda")
    with pytest.raises(ValueError, match="weight shape"):
        functional.lpips_distance(f, f, torch.zeros(7, device="cuda"))
    with pytest.raises(ValueError, match="must match"):
        functional.lpips_distance(f, f[:, :2], torch.zeros(8, device="cuda"))
    with pytest.raises(TypeError, match="float32 and bfloat16"):
        functional.lpips_distance(f.half(), f.half(), torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        _lib.check(_lib.lib().tfc_lpips_distance_backward(f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(),
                                                          None, None, 0, 2, 4, 8, 1e-10, 4, _lib.stream_ptr()))


# ---------------------------------------------------------------------------------------------------------------------

POOL_SIZES = [(3, 3), (7, 7), (8, 9), (15, 14)]
POOL_CHANNELS = [3, 64, 61, 192]


@functools.lru_cache(maxsize=None)
def pool_inputs(size, C, k, s):
    """x: a few bfloat16-exact positive levels, so that windows tie; g: normal."""
    gen = torch.Generator().manual_seed(size[0] * 100 + size[1] + C + k)
    x = torch.randint(1, 7, (2,) + size + (C,), generator=gen).float() / 4
    oh, ow = (size[0] - k) // s + 1, (size[1] - k) // s + 1
    g = torch.randn(2, oh, ow, C, generator=gen).bfloat16().float()
    return x, g, lpips_ref.max_pool_first_backward(x, g, k, s), lpips_ref.tied_windows(x, k, s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
@pytest.mark.parametrize("C", POOL_CHANNELS)
@pytest.mark.parametrize("size", POOL_SIZES)
def test_max_pool(size, C, k, s, dtype):
    """Forward: the bits of torch's max_pool2d on the CPU.  Backward: the bits of the first-maximum reference, float32
    sums of the windows in row-major order (bfloat16: that sum rounded once)."""
    gen = torch.Generator().manual_seed(size[0] + C)
    z = torch.randn((2,) + size + (C,), generator=gen).to(dtype)
    want = torch.nn.functional.max_pool2d(z.float().permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1).to(dtype)
    got = functional.max_pool2d(z.cuda(), k, s).cpu()
    assert got.dtype == dtype and torch.equal(got, want)

    x, g, want_dx, ties = pool_inputs(size, C, k, s)
    assert ties >= 1
    xd = x.to(dtype).cuda().requires_grad_(True)
    y = functional.max_pool2d(xd, k, s)
    y.backward(g.to(dtype).cuda())
    assert torch.equal(y.detach().cpu(), lpips_ref.max_pool_first(x, k, s)[0].to(dtype))
    assert xd.grad.dtype == dtype and torch.equal(xd.grad.cpu(), want_dx.to(dtype))


# ---------------------------------------------------------------------------------------------------------------------

NET_SIZES = [(31, 31), (35, 32), (64, 48)]


@functools.lru_cache(maxsize=None)
def net():
    return tfc.LPIPS.with_random_weights(0).cuda()


@functools.lru_cache(maxsize=None)
def cpu_weights():
    return {k: v.cpu() for k, v in net().state_dict().items()}


@functools.lru_cache(maxsize=None)
def image_pair(size, pair, dtype):
    """(fake, real) on the CPU, rounded to `dtype`, with the float64 value and gradient of the rounded images."""
    gen = torch.Generator().manual_seed(size[0] * 64 + size[1])
    real = torch.rand((2,) + size + (3,), generator=gen)
    if pair == "close":
        fake = (real + 0.02 * torch.randn(real.shape, generator=gen)).clamp(0, 1)
    else:
        fake = torch.rand(real.shape, generator=gen)
    fake, real = fake.to(dtype), real.to(dtype)
    return (fake, real) + lpips_ref.lpips_with_grad(cpu_weights(), fake, real)


def run_net(fake, real, real_grad=False):
    fake = fake.cuda().requires_grad_(True)
    real = real.cuda().requires_grad_(real_grad)
    value = net()(fake, real)
    value.mean().backward()
    return value.detach(), fake.grad, real.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("pair", ["close", "unrelated"])
@pytest.mark.parametrize("size", NET_SIZES)
def test_network_value_and_gradient(size, pair, dtype):
    """Value (relative error) and d mean / d fake (relative L2) against float64 on the same rounded images: at most
    twice the error of the same-dtype composition (torch conv2d / max_pool2d in `dtype` on the CPU, the distance head in
    float32 as the kernel evaluates it) plus 1e-6 (float32) or one bfloat16 ulp (bfloat16)."""
    fake, real, want, want_grad = image_pair(size, pair, dtype)
    own, own_grad = lpips_ref.lpips_with_grad(cpu_weights(), fake, real, dtype, torch.float32)
    got, got_grad, real_grad = run_net(fake, real)
    assert got.dtype == torch.float32 and got.shape == (2,) and got_grad.dtype == dtype and real_grad is None
    slack = 1e-6 if dtype == torch.float32 else BF16_ULP
    e_kernel, e_torch = float(((got.cpu() - want).abs() / want).max()), float(((own - want).abs() / want).max())
    g_kernel, g_torch = rel_l2(got_grad.cpu(), want_grad), rel_l2(own_grad, want_grad)
    print(f"lpips {size} {pair} {dtype}: value {want.tolist()} rel err kernel = {e_kernel:.3e}, composition = "
          f"{e_torch:.3e}; gradient rel L2 kernel = {g_kernel:.3e}, composition = {g_torch:.3e}")
    assert e_kernel <= 2 * e_torch + slack
    assert g_kernel <= 2 * g_torch + slack


def test_network_determinism_layouts_and_both_gradients():
    fake, real, _, _ = image_pair((35, 32), "close", torch.float32)
    first, second = run_net(fake, real), run_net(fake, real)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    # NHWC views of NCHW storage
    value = net()(fake.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1),
                  real.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1))
    assert torch.equal(value, first[0])
    # real with a gradient: d(fake, real) is symmetric, so swapping the arguments swaps the gradients
    _, gf, gr = run_net(fake, real, real_grad=True)
    _, sf, sr = run_net(real, fake, real_grad=True)
    assert gr is not None and rel_l2(gr, sf) <= 1e-5 and rel_l2(gf, sr) <= 1e-5
    # under no_grad the convolutions keep their packed weights (weights_key): the same values to the float32 bar, on
    # the unrelated pair, whose value is not a small difference of features
    fake, real, _, _ = image_pair((35, 32), "unrelated", torch.float32)
    with torch.no_grad():
        quiet = [net()(fake.cuda(), real.cuda()) for _ in range(2)]
    assert torch.equal(quiet[0], quiet[1]) and rel_l2(quiet[0], run_net(fake, real)[0]) <= 1e-5


def test_trainer_mselpips_step():
    from compression_amd import synthetic
    from compression_amd.models import hific_train
    from test_hific_gpu import small
    lpips = tfc.LPIPS.with_random_weights(0).cuda()
    before = {k: v.clone() for k, v in lpips.state_dict().items()}
    model = small(seed=1)
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    trainer = hific_train.HiFiCTrainer(model, None, hific_train.CONFIGS["mselpips"], ignore_schedules=True,
                                       perceptual_loss=tfc.LPIPSLoss(lpips))
    x = torch.from_numpy(synthetic.lowpass_images(2, 64, 64, seed=3)).cuda().float()
    out = trainer.train_step([x])
    assert out["weighted_lpips"].numel() == 1 and bool(torch.isfinite(out["weighted_lpips"])) and float(out["weighted_lpips"]) > 0
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    entropy = {id(p) for p in model.hyperprior.side_prior.parameters()}
    moved = [n for n, p in model.named_parameters() if id(p) not in entropy and not torch.equal(p.detach(), params[n])]
    assert len(moved) > 0 and not any(p.grad is None or not bool(torch.isfinite(p.grad).all())
                                      for p in model.parameters() if id(p) not in entropy)
    assert all(torch.equal(v, before[k]) for k, v in lpips.state_dict().items()) and list(lpips.parameters()) == []
    plain = hific_train.HiFiCTrainer(small(seed=1), None, hific_train.CONFIGS["mselpips"], ignore_schedules=True)
    keys = set(plain.train_step([x]))
    assert keys == {"rd_loss", "weighted_R", "weighted_D", "lmbda_inv", "total_nbpp", "total_qbpp", "loss_enc_dec_entropy"}
    assert set(out) == keys | {"weighted_lpips"}
