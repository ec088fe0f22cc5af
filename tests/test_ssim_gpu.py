"""GPU tier: the fused SSIM / multiscale SSIM kernels (csrc/ssim.hip) against the float64 oracle of tests/ssim_ref.py.

The accuracy bar is not a number chosen in advance: every case also evaluates the op-by-op torch composition
(`ssim_multiscale_reference` / `ssim_reference`) in float32 on the GPU and requires
    err_kernel <= 2 * err_torch_f32 + 1e-6
(2: a different summation order; 1e-6: about sixteen float32 spacings of a result near 1, so that the bar does not
collapse where torch happens to be exact).  Both errors are printed per case.

Test images are image-like (ssim_ref.image_pair: a smooth random field with a few edges, 8-bit, degraded by a blur, by
noise of sigma 2 ... 20, by coarse quantisation or by all three), so that MS-SSIM spans about 0.5 ... 0.999; every
cs_plane of every case is positive in the oracle (asserted), so the relu and the powers are differentiable where
gradients are compared."""
import functools

import numpy as np
import pytest
import torch

import ssim_ref
from compression_amd import models, synthetic
from compression_amd.ops import image_ops

pytestmark = pytest.mark.gpu

SIZES = [(161, 161), (177, 203), (256, 256), (512, 768)]
BATCHES = [(), (4,), (2, 3)]
CHANNELS = [1, 3, 4, 6]
CASES = [(size, batch, c) for size in SIZES for batch in BATCHES for c in CHANNELS]


def degradation_of(size, batch, c):
    """Cycles through the degradations over the case list."""
    return ssim_ref.DEGRADATIONS[CASES.index((size, batch, c)) % len(ssim_ref.DEGRADATIONS)]


@functools.lru_cache(maxsize=2)
def images(size, batch, c):
    return ssim_ref.image_pair(1000 + CASES.index((size, batch, c)), batch + size + (c,), degradation_of(size, batch, c))


def bar(err_torch):
    return 2.0 * err_torch + 1e-6


def errors(got, ref32, want):
    got, ref32 = got.double().cpu().numpy(), ref32.double().cpu().numpy()
    return float(np.abs(got - want).max()), float(np.abs(ref32 - want).max())


def cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


CASE_IDS = ["%dx%d-batch%s-c%d" % (s[0], s[1], "x".join(map(str, b)) or "none", c) for s, b, c in CASES]


@pytest.mark.parametrize("size,batch,c", CASES, ids=CASE_IDS)
def test_forward(size, batch, c):
    """ssim_multiscale and ssim, float32 and uint8 inputs, against the oracle; the bar comes from torch in float32."""
    x, y = images(size, batch, c)
    want_ms, raw, _ = ssim_ref.ssim_multiscale_parts(x, y, 255)
    want_ss = ssim_ref.ssim(x, y, 255)
    assert raw.min() > 0.0, "the oracle itself has a non-positive scale value: replace the case"
    failures = []
    for dtype in (torch.float32, torch.uint8):
        tx, ty = cuda(x, dtype), cuda(y, dtype)
        for name, fn, ref, want in (("ms", image_ops.ssim_multiscale, image_ops.ssim_multiscale_reference, want_ms),
                                    ("ssim", image_ops.ssim, image_ops.ssim_reference, want_ss)):
            got = fn(tx, ty, 255)
            assert got.dtype == torch.float32 and tuple(got.shape) == batch
            err, err_torch = errors(got, ref(tx, ty, 255), want)
            print(f"ssim_fwd {name} {size} {batch} C={c} {degradation_of(size, batch, c)} {str(dtype)[6:]}: "
                  f"value {np.mean(want):.4f} err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
            if not err <= bar(err_torch):
                failures.append((name, dtype, err, err_torch))
    assert not failures, failures


def test_cases_span_the_range():
    """The case list is not all near 1 (or near 0): MS-SSIM from below 0.75 to above 0.99 on the 161 x 161 cases."""
    values = []
    for batch in BATCHES:
        for c in CHANNELS:
            x, y = images((161, 161), batch, c)
            values.append(float(np.min(ssim_ref.ssim_multiscale(x, y, 255))))
            values.append(float(np.max(ssim_ref.ssim_multiscale(x, y, 255))))
    print("ms-ssim of the 161 x 161 cases:", " ".join(f"{v:.4f}" for v in values))
    assert min(values) < 0.75 and max(values) > 0.99


@pytest.mark.parametrize("shape", [(256, 256, 3), (2, 177, 203, 1)])
def test_shifted_mean(shape):
    """Flat, bright, nearly identical float32 images (200 + noise of sigma 0.5): the uncentred float32 formula loses its
    digits in S - mu1^2 - mu2^2.  The yardstick is the float32 reference on the CENTRED inputs x - 200, y - 200, which
    have the same variances and covariance; the quantity is the cs-only one (k1 = 1e4 makes l = 1 to float32 precision),
    for kernel, yardstick and oracle alike."""
    rng = np.random.default_rng(77)
    x = (200.0 + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    y = (200.0 + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    want = ssim_ref.ssim_multiscale(x, y, 255, k1=1e4)
    tx, ty = cuda(x), cuda(y)
    got = image_ops.ssim_multiscale(tx, ty, 255, k1=1e4)
    centred = image_ops.ssim_multiscale_reference(tx - 200.0, ty - 200.0, 255, k1=1e4)
    plain = image_ops.ssim_multiscale_reference(tx, ty, 255, k1=1e4)
    err, err_centred = errors(got, centred, want)
    _, err_plain = errors(got, plain, want)
    print(f"ssim_shifted {shape}: value {np.mean(want):.6f} err_kernel {err:.3e} err_torch_f32_centred {err_centred:.3e} "
          f"err_torch_f32_uncentred {err_plain:.3e} (expected, not required, to miss the bar {bar(err_centred):.3e})")
    assert err <= bar(err_centred)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(256, 256, 3), (4, 177, 203, 3)])
def test_half_precision_inputs(dtype, shape):
    """bfloat16 / float16 images are read directly; the oracle sees the rounded inputs, the bar is the float32 one."""
    x8, y8 = ssim_ref.image_pair(31, shape, "noise8")
    rng = np.random.default_rng(32)
    x = x8 + rng.uniform(-0.5, 0.5, shape)                # not 8-bit integers: the rounding to 16 bits matters
    y = y8 + rng.uniform(-0.5, 0.5, shape)
    tx, ty = cuda(x, dtype), cuda(y, dtype)
    xr, yr = tx.double().cpu().numpy(), ty.double().cpu().numpy()
    assert not np.array_equal(xr, x)
    want, raw, _ = ssim_ref.ssim_multiscale_parts(xr, yr, 255)
    assert raw.min() > 0.0
    got = image_ops.ssim_multiscale(tx, ty, 255)
    err, err_torch = errors(got, image_ops.ssim_multiscale_reference(tx.float(), ty.float(), 255), want)
    print(f"ssim_half {shape} {str(dtype)[6:]}: value {np.mean(want):.4f} err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
    assert got.dtype == torch.float32 and err <= bar(err_torch)


@pytest.mark.parametrize("filter_size,filter_sigma", [(7, 1.5), (8, 1.5), (11, 1.0), (8, 1.0)])
@pytest.mark.parametrize("size,batch,c", [((177, 203), (4,), 3), ((256, 256), (2, 3), 4)])
def test_other_windows(filter_size, filter_sigma, size, batch, c):
    x, y = images(size, batch, c)
    kw = dict(filter_size=filter_size, filter_sigma=filter_sigma)
    tx, ty = cuda(x, torch.float32), cuda(y, torch.float32)
    for name, fn, ref, oracle in (("ms", image_ops.ssim_multiscale, image_ops.ssim_multiscale_reference, ssim_ref.ssim_multiscale),
                                  ("ssim", image_ops.ssim, image_ops.ssim_reference, ssim_ref.ssim)):
        want = oracle(x, y, 255, **kw)
        err, err_torch = errors(fn(tx, ty, 255, **kw), ref(tx, ty, 255, **kw), want)
        print(f"ssim_window {name} n={filter_size} sigma={filter_sigma} {size} {batch} C={c}: value {np.mean(want):.4f} "
              f"err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
        assert err <= bar(err_torch)


def test_largest_window():
    """filter_size 31 (the 16 x 16 tile, the largest LDS footprint), single scale, value and gradient."""
    x, y = ssim_ref.image_pair(41, (2, 100, 131, 3), "noise8")
    tx, ty = cuda(x, torch.float32), cuda(y, torch.float32)
    kw = dict(filter_size=31, filter_sigma=5.0)
    err, err_torch = errors(image_ops.ssim(tx, ty, 255, **kw), image_ops.ssim_reference(tx, ty, 255, **kw),
                            ssim_ref.ssim(x, y, 255, **kw))
    print(f"ssim_window n=31: err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
    assert err <= bar(err_torch)
    tx.requires_grad_(True)
    image_ops.ssim(tx, ty, 255, **kw).sum().backward()
    t64 = torch.from_numpy(x).double().requires_grad_(True)
    image_ops.ssim_reference(t64, torch.from_numpy(y).double(), 255, **kw).sum().backward()
    t32 = cuda(x, torch.float32).requires_grad_(True)
    image_ops.ssim_reference(t32, ty, 255, **kw).sum().backward()
    scale = t64.grad.abs().max().item()
    rel = (tx.grad.double().cpu() - t64.grad).abs().max().item() / scale
    rel_torch = (t32.grad.double().cpu() - t64.grad).abs().max().item() / scale
    print(f"ssim_window n=31 gradient: err_kernel {rel:.3e} err_torch_f32 {rel_torch:.3e}")
    assert rel <= 2.0 * rel_torch + 1e-5


def grads(fn, x, y, device, dtype):
    tx = torch.from_numpy(x).to(device, dtype).requires_grad_(True)
    ty = torch.from_numpy(y).to(device, dtype).requires_grad_(True)
    fn(tx, ty, 255).sum().backward()
    return tx.grad.double().cpu().numpy(), ty.grad.double().cpu().numpy()


@pytest.mark.parametrize("size", [(161, 161), (177, 203), (256, 256)])
def test_gradients(size):
    """d ssim_multiscale / d image for both images against float64 autograd of the reference composition; error
    max|g - g64| / max|g64|, bar 2 * (the same error of float32 autograd of the reference) + 1e-5 (the project's float32
    bar for transform outputs, tests/test_gdn_gpu.py).  And the metric has its maximum at y = x: the gradient there is
    below 1e-5 of the gradient scale of the noisy case."""
    x, y = images(size, (4,), 3)
    _, raw, _ = ssim_ref.ssim_multiscale_parts(x, y, 255)
    assert raw.min() > 0.0
    g64 = grads(image_ops.ssim_multiscale_reference, x, y, "cpu", torch.float64)
    g32 = grads(image_ops.ssim_multiscale_reference, x, y, "cuda", torch.float32)
    got = grads(image_ops.ssim_multiscale, x, y, "cuda", torch.float32)
    failures = []
    for which, g, r, w in zip(("img1", "img2"), got, g32, g64):
        scale = np.abs(w).max()
        err, err_torch = np.abs(g - w).max() / scale, np.abs(r - w).max() / scale
        print(f"ssim_grad {size} {which}: max|g64| {scale:.3e} err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
        if not (np.isfinite(g).all() and err <= 2.0 * err_torch + 1e-5):
            failures.append((which, err, err_torch))
    assert not failures, failures
    _, at_max = grads(image_ops.ssim_multiscale, x, x.copy(), "cuda", torch.float32)
    ratio = np.abs(at_max).max() / np.abs(g64[1]).max()
    print(f"ssim_grad {size} at y = x: max|g| / max|g64 of the noisy case| = {ratio:.3e}")
    assert ratio < 1e-5


def test_gradient_flows_to_one_image_only():
    x, y = images((177, 203), (4,), 3)
    tx, ty = cuda(x, torch.float32), cuda(y, torch.float32).requires_grad_(True)
    image_ops.ssim_multiscale(tx, ty, 255).sum().backward()
    both = grads(image_ops.ssim_multiscale, x, y, "cuda", torch.float32)
    assert tx.grad is None and np.array_equal(ty.grad.cpu().numpy(), both[1])
    tu = cuda(x)                                            # a uint8 original beside a float reconstruction
    ty2 = cuda(y, torch.float32).requires_grad_(True)
    image_ops.ssim_multiscale(tu, ty2, 255).sum().backward()
    assert np.array_equal(ty2.grad.cpu().numpy(), both[1])


def test_determinism():
    x, y = images((177, 203), (2, 3), 3)
    runs = []
    for _ in range(2):
        tx, ty = cuda(x, torch.float32).requires_grad_(True), cuda(y, torch.float32).requires_grad_(True)
        value = image_ops.ssim_multiscale(tx, ty, 255)
        value.sum().backward()
        runs.append((value.detach().clone(), tx.grad.clone(), ty.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_non_contiguous_inputs():
    """A crop view of a larger image, as the models produce, gives the bits of its contiguous copy."""
    x, y = ssim_ref.image_pair(51, (2, 200, 230, 3), "noise8")
    bx, by = cuda(x, torch.float32), cuda(y, torch.float32)
    vx, vy = bx[:, 5:182, 3:206, :], by[:, 5:182, 3:206, :]
    assert not vx.is_contiguous()
    out = []
    for a, b in ((vx, vy), (vx.contiguous(), vy.contiguous())):
        a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        value = image_ops.ssim_multiscale(a, b, 255)
        value.sum().backward()
        out.append((value.detach(), a.grad, b.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def small_bls2017(seed, grey=False, **kw):
    """`grey`: an untrained synthesis transform writes values near 0, where the luminance term can turn negative and the
    relu of the last scale cuts the gradient; a bias of 0.5 on the last layer puts the reconstruction at mid-grey."""
    torch.manual_seed(seed)
    model = models.BLS2017Model(num_filters=64, **kw).cuda()
    if grey:
        with torch.no_grad():
            model.synthesis_transform.layer_2.bias.fill_(0.5)
    return model


def test_bls2017_ms_ssim_loss():
    x = torch.from_numpy(synthetic.lowpass_images(2, 256, 256, seed=3)).cuda().float()
    model = small_bls2017(0, grey=True, distortion="ms-ssim")
    seen = []
    hook = model.synthesis_transform.register_forward_hook(lambda mod, args, out: seen.append(out.detach()))
    loss, bpp, dist = model(x)
    hook.remove()
    assert torch.isfinite(loss) and torch.equal(loss, bpp + model.lmbda * dist)
    x_hat = seen[0]
    want = 1.0 - ssim_ref.ssim_multiscale(x.cpu().numpy(), x_hat.float().cpu().numpy(), 255).mean()
    ref = (1.0 - image_ops.ssim_multiscale_reference(x, x_hat.float(), 255)).mean()
    err, err_torch = abs(dist.item() - want), abs(ref.item() - want)
    print(f"bls2017 ms-ssim: distortion {want:.6f} err_kernel {err:.3e} err_torch_f32 {err_torch:.3e}")
    assert err <= bar(err_torch)
    loss.backward()
    kernels = [p for n, p in model.synthesis_transform.layer_2.named_parameters() if n.startswith("kernel")]
    assert kernels
    for p in kernels:
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0


def test_bls2017_mse_is_unchanged():
    x = torch.from_numpy(synthetic.lowpass_images(2, 256, 256, seed=3)).cuda().float()
    outs = []
    for kw in ({}, {"distortion": "mse"}):
        model = small_bls2017(5, **kw)
        torch.manual_seed(9)
        outs.append(model(x))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="distortion"):
        models.BLS2017Model(distortion="psnr")
    with pytest.raises(ValueError, match="distortion"):
        models.BMSHJ2018Model(distortion="psnr")


def test_bmshj2018_ms_ssim_loss():
    torch.manual_seed(1)
    model = models.BMSHJ2018Model(num_filters=64, distortion="ms-ssim").cuda()
    with torch.no_grad():
        model.synthesis_transform.layer_3.bias.fill_(0.5)
    x = torch.from_numpy(synthetic.lowpass_images(2, 256, 256, seed=4)).cuda().float()
    loss, bpp, dist = model(x)
    assert torch.isfinite(loss) and 0.0 < dist.item() <= 1.0 and torch.equal(loss, bpp + model.lmbda * dist)
    loss.backward()
    grads_ = [p.grad for n, p in model.synthesis_transform.layer_3.named_parameters() if n.startswith("kernel")]
    assert grads_ and all(g is not None and torch.isfinite(g).all() and g.abs().max() > 0 for g in grads_)


def test_compress_file_prints_ms_ssim(tmp_path, capsys):
    model = small_bls2017(2, grey=True).init_compression()
    img = torch.from_numpy(synthetic.lowpass_images(1, 192, 256, seed=5)[0])
    models.write_png(tmp_path / "in.png", img)
    models.compress_file(model, tmp_path / "in.png", tmp_path / "out.tfci", verbose=True)
    lines = capsys.readouterr().out.strip().splitlines()
    heads = [ln.split(":")[0] for ln in lines]
    assert heads == ["Mean squared error", "PSNR (dB)", "Multiscale SSIM", "Multiscale SSIM (dB)", "Bits per pixel"]
    x_hat = models.decompress_file(model, tmp_path / "out.tfci").cpu().numpy()
    want = float(ssim_ref.ssim_multiscale(img.numpy(), x_hat, 255))
    printed = float(lines[2].split(":")[1])
    with capsys.disabled():
        print(f"compress_file: printed {lines[2]!r}, oracle {want:.6f}")
    assert len(lines[2].split(":")[1].strip()) == 6 and abs(printed - want) <= 0.5e-4 + 1e-6
    assert abs(float(lines[3].split(":")[1]) - (-10.0 * np.log10(1.0 - want))) <= 0.02

    small = torch.from_numpy(synthetic.lowpass_images(1, 64, 64, seed=6)[0])
    models.write_png(tmp_path / "small.png", small)
    models.compress_file(model, tmp_path / "small.png", tmp_path / "small.tfci", verbose=True)
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[2] == "Multiscale SSIM: n/a (image side below 161)" and len(lines) == 4
    assert lines[3].startswith("Bits per pixel")
