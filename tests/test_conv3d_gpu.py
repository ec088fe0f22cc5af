"""GPU tier: the rank-3 kernels (tfc_conv3d_down / up / wgrad) against torch-CPU float64: F.conv3d on the explicitly
padded input and F.conv_transpose3d cropped; gradients of the autograd wrapper against torch autograd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2 ** -7}
GTOL = {torch.float32: 5e-5, torch.bfloat16: 2 ** -6}


def ref_down(x, w, b, s, relu):
    k = w.shape[:3]
    out = [-(-x.shape[1 + a] // s[a]) for a in range(3)]
    pad = []
    for a in (2, 1, 0):
        pad += [k[a] // 2, k[a] + s[a]]
    xp = F.pad(x.permute(0, 4, 1, 2, 3).double(), pad)
    y = F.conv3d(xp, w.permute(4, 3, 0, 1, 2).double(), stride=s)[:, :, :out[0], :out[1], :out[2]].permute(0, 2, 3, 4, 1)
    y = y + b.double() if b is not None else y
    return torch.relu(y) if relu else y


def ref_up(x, w, b, s, relu):
    k = w.shape[:3]
    f = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3).double(), w.permute(3, 4, 0, 1, 2).double(), stride=s)
    f = F.pad(f, (0, s[2] + k[2], 0, s[1] + k[1], 0, s[0] + k[0]))
    y = f[:, :, k[0] // 2:k[0] // 2 + x.shape[1] * s[0], k[1] // 2:k[1] // 2 + x.shape[2] * s[1],
          k[2] // 2:k[2] // 2 + x.shape[3] * s[2]].permute(0, 2, 3, 4, 1)
    y = y + b.double() if b is not None else y
    return torch.relu(y) if relu else y


def run(up, x, w, b, s, relu):
    from compression_amd.layers import functional
    fn = functional.conv3d_up if up else functional.conv3d_down
    with torch.no_grad():
        return fn(x.cuda(), w.cuda(), None if b is None else b.cuda(), s, "relu" if relu else None)


def close(got, want, tol):
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got.double().cpu() - want).abs().max()) if want.numel() else 0.0
    assert err <= tol * scale, (err, tol * scale)


CASES = [  # (n, in extents, cin, cout, support, strides)
    (2, (5, 7, 9), 16, 32, (3, 3, 3), (1, 1, 1)),
    (1, (6, 9, 11), 48, 3, (3, 5, 5), (2, 2, 2)),
    (2, (4, 10, 13), 16, 96, (3, 5, 5), (1, 2, 2)),
    (1, (5, 6, 14), 128, 1, (2, 2, 2), (2, 1, 3)),
    (3, (1, 1, 67), 16, 32, (1, 1, 5), (1, 1, 4)),
    (2, (3, 5, 37), 192, 192, (1, 1, 1), (1, 2, 2)),
    (1, (3, 4, 70), 16, 96, (5, 5, 5), (1, 1, 1)),
    (2, (2, 3, 5), 32, 40, (3, 3, 3), (2, 1, 3)),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_against_torch(case, up, dtype):
    n, ext, cin, cout, k, s = case
    g = torch.Generator().manual_seed(hash((case, up)) % 1000)
    x = torch.randn((n,) + ext + (cin,), generator=g).to(dtype)
    w = (torch.randn(k + (cin, cout), generator=g) / (np.prod(k) * cin) ** 0.5)
    if dtype == torch.bfloat16:
        w = w.bfloat16().float()            # (the kernel rounds the weights to bfloat16: compare on the same values)
    b = torch.randn(cout, generator=g)
    for bias, relu in ((None, False), (b, True)):
        got = run(up, x, w, bias, s, relu)
        want = (ref_up if up else ref_down)(x.double(), w.double(), bias, s, relu)
        assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape)
        close(got, want, TOL[dtype])


@pytest.mark.parametrize("up", [False, True])
def test_one_sample_equals_its_batch(up):
    torch.manual_seed(3)
    x = torch.randn(3, 4, 9, 21, 32).bfloat16()
    w = torch.randn(3, 3, 5, 32, 48) * 0.05
    y = run(up, x, w, None, (1, 2, 2), False)
    y1 = run(up, x[1:2], w, None, (1, 2, 2), False)
    assert torch.equal(y[1:2], y1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("case", [(2, (3, 6, 7), 16, 3, (3, 3, 3), (1, 2, 2)),
                                  (1, (4, 5, 9), 32, 48, (2, 3, 5), (2, 1, 3)),
                                  (2, (1, 1, 40), 48, 16, (1, 1, 9), (1, 1, 4))], ids=str)
def test_gradients_against_autograd(case, up, dtype):
    from compression_amd.layers import functional
    n, ext, cin, cout, k, s = case
    torch.manual_seed(4)
    x = torch.randn((n,) + ext + (cin,)).to(dtype)
    w = torch.randn(k + (cin, cout)) / (np.prod(k) * cin) ** 0.5
    if dtype == torch.bfloat16:
        w = w.bfloat16().float()
    b = torch.randn(cout)
    xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    fn = functional.conv3d_up if up else functional.conv3d_down
    y = fn(xg, wg, bg, s, "relu")
    gy = torch.randn(y.shape).to(dtype)
    y.backward(gy.cuda())
    xd, wd, bd = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    want = (ref_up if up else ref_down)(xd, wd, bd, s, False)
    mask = (y.detach().cpu().double() > 0)
    (want * mask * gy.double()).sum().backward()
    close(xg.grad, xd.grad, GTOL[dtype])
    close(wg.grad, wd.grad, GTOL[dtype])
    close(bg.grad, bd.grad, GTOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wgrad_is_deterministic(dtype):
    from compression_amd.layers import functional
    torch.manual_seed(5)
    a = torch.randn(2, 6, 20, 24, 64).to(dtype).cuda()
    b = torch.randn(2, 6, 10, 12, 48).to(dtype).cuda()
    d1 = functional.conv3d_wgrad(a, b, (3, 5, 5), (1, 2, 2), False)
    d2 = functional.conv3d_wgrad(a, b, (3, 5, 5), (1, 2, 2), False)
    assert torch.equal(d1, d2)
    want = torch.zeros(3, 5, 5, 64, 48, dtype=torch.float64)
    ad, bd = a.double().cpu(), b.double().cpu()
    for t in np.ndindex(3, 5, 5):
        sl = []
        for ax, (k, s, la, lb) in enumerate(zip((3, 5, 5), (1, 2, 2), ad.shape[1:4], bd.shape[1:4])):
            q = torch.arange(lb)
            p = q * s + t[ax] - k // 2
            sl.append((q[(p >= 0) & (p < la)], p[(p >= 0) & (p < la)]))
        aa = ad[:, sl[0][1]][:, :, sl[1][1]][:, :, :, sl[2][1]]
        bb = bd[:, sl[0][0]][:, :, sl[1][0]][:, :, :, sl[2][0]]
        want[t] = torch.einsum("ndhwa,ndhwb->ab", aa, bb)
    close(d1, want, GTOL[dtype])


def test_argument_errors_are_textual_and_empty_tensors_return():
    from compression_amd import _lib
    lib = _lib.lib()
    st = _lib.stream_ptr()
    rc = lib.tfc_conv3d_down(None, None, None, None, 1, 1, 1, 1, 4, 24, 8, 1, 1, 3, 1, 1, 1, 0, st)
    assert rc != 0 and "tfc_conv3d_down: input channels must be a multiple of 16" in _lib.last_error()
    rc = lib.tfc_conv3d_up(None, None, None, None, 2, 1, 1, 1, 4, 16, 8, 1, 1, 3, 1, 1, 1, 0, st)
    assert rc != 0 and "tfc_conv3d_up: dtype must be" in _lib.last_error()
    rc = lib.tfc_conv3d_up(None, None, None, None, 1, 1, 1, 1, 4, 16, 8, 1, 1, 3, 1, 0, 1, 0, st)
    assert rc != 0 and "tfc_conv3d_up: strides must be >= 1" in _lib.last_error()
    rc = lib.tfc_conv3d_down(None, None, None, None, 1, 1, 1, 1, 4, 16, 8, 1, 1, 3, 1, 1, 1, 2, st)
    assert rc != 0 and "activation" in _lib.last_error()
    rc = lib.tfc_conv3d_wgrad(None, None, None, 1, 1, 1, 1, 4, 24, 1, 1, 4, 16, 1, 1, 3, 1, 1, 1, 0, st)
    assert rc != 0 and "tfc_conv3d_wgrad: channel counts must be multiples of 16" in _lib.last_error()
    rc = lib.tfc_conv3d_down(None, None, None, None, 1, 0, 1, 1, 4, 16, 8, 1, 1, 3, 1, 1, 1, 0, st)
    assert rc == 0
    from compression_amd.layers import functional
    x = torch.zeros(0, 2, 3, 4, 16, device="cuda")
    y = functional.conv3d_down(x, torch.zeros(1, 1, 3, 16, 8), None, 1)
    assert tuple(y.shape) == (0, 2, 3, 4, 8)
    dw = functional.conv3d_wgrad(x, torch.zeros(0, 2, 3, 4, 16, device="cuda"), (1, 1, 3), (1, 1, 1), False)
    assert tuple(dw.shape) == (1, 1, 3, 16, 16) and not dw.any()
