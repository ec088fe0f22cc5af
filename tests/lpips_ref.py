"""The float64 definition of LPIPS (AlexNet trunk) that the LPIPS tests check against, written with torch-CPU ops and
nothing of compression_amd, plus the first-maximum max-pool in explicit loops.

Inputs `fake`, `real` [N, H, W, 3] in [0, 1]; `weights`: conv{1..5}_kernel (HWIO), conv{1..5}_bias, lin{0..4}, shift,
scale.
  x = ((2 img - 1) - shift) / scale
  conv1 11x11 stride 4 pad 2, ReLU | max-pool 3x3 stride 2 | conv2 5x5 pad 2, ReLU | max-pool 3x3 stride 2 |
  conv3, conv4, conv5 3x3 pad 1, ReLU; the taps are the five ReLU outputs
  n = sqrt(sum_c f^2), u = f0 / (n0 + eps), v = f1 / (n1 + eps), eps = 1e-10
  d_l[image] = mean over pixels of sum_c w_l[c] (u_c - v_c)^2;   lpips[image] = sum_l d_l
The gradient of the normalisation is the explicit form g / (n + eps) - f (f . g) / (n (n + eps)^2), the second term 0
where n = 0 (autograd's sqrt gives inf * 0 = NaN at an all-zero pixel)."""
import torch

EPS = 1e-10
# (name, stride, pad, pooled behind)
LAYERS = (("conv1", 4, 2, True), ("conv2", 1, 2, True), ("conv3", 1, 1, False), ("conv4", 1, 1, False),
          ("conv5", 1, 1, False))


class UnitNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, eps):
        n = torch.sqrt(torch.sum(f * f, dim=-1, keepdim=True))
        ctx.save_for_backward(f, n)
        ctx.eps = eps
        return f / (n + eps)

    @staticmethod
    def backward(ctx, g):
        f, n = ctx.saved_tensors
        dot = torch.sum(f * g, dim=-1, keepdim=True)
        safe = torch.where(n > 0, n, torch.ones_like(n))
        second = torch.where(n > 0, dot / (safe * (n + ctx.eps) ** 2), torch.zeros_like(n))
        return g / (n + ctx.eps) - f * second, None


def distance(f0, f1, w, eps=EPS, dtype=torch.float64):
    """[N, ..., C] features -> [N], differentiable, evaluated in `dtype`."""
    n, c = f0.shape[0], f0.shape[-1]
    u = UnitNormalize.apply(f0.to(dtype).reshape(n, -1, c), eps)
    v = UnitNormalize.apply(f1.to(dtype).reshape(n, -1, c), eps)
    return torch.sum(w.to(dtype) * (u - v) ** 2, dim=-1).mean(dim=-1)


def distance_with_grads(f0, f1, w, g, eps=EPS, dtype=torch.float64):
    """-> (d [N], df0, df1) for the incoming gradient g [N], in `dtype`."""
    a = f0.detach().to(dtype).requires_grad_(True)
    b = f1.detach().to(dtype).requires_grad_(True)
    d = distance(a, b, w, eps, dtype)
    d.backward(g.to(dtype))
    return d.detach(), a.grad, b.grad


def taps(weights, images, dtype=torch.float64):
    """The five ReLU outputs, NHWC, evaluated in `dtype` (weights and images converted to it)."""
    x = 2 * images.to(dtype) - 1
    x = (x - weights["shift"].to(dtype)) / weights["scale"].to(dtype)
    x = x.permute(0, 3, 1, 2)
    out = []
    for name, stride, pad, pooled in LAYERS:
        kernel = weights[f"{name}_kernel"].to(dtype).permute(3, 2, 0, 1)
        x = torch.relu(torch.nn.functional.conv2d(x, kernel, weights[f"{name}_bias"].to(dtype), stride=stride,
                                                  padding=pad))
        out.append(x.permute(0, 2, 3, 1))
        if pooled:
            x = torch.nn.functional.max_pool2d(x, 3, 2)
    return out


def lpips(weights, fake, real, dtype=torch.float64, distance_dtype=None):
    """-> [N].  dtype: what the trunk is evaluated in; distance_dtype: what the distance head is evaluated in (the
    trunk's by default; the same-dtype composition of a bfloat16 trunk takes float32, as the kernel does)."""
    n = fake.shape[0]
    feats = taps(weights, torch.cat([fake.to(dtype), real.to(dtype)], 0), dtype)
    total = 0
    for i, t in enumerate(feats):
        total = total + distance(t[:n], t[n:], weights[f"lin{i}"], EPS, distance_dtype or dtype)
    return total


def lpips_with_grad(weights, fake, real, dtype=torch.float64, distance_dtype=None):
    """-> (lpips [N], d mean(lpips) / d fake), both as float64."""
    fake = fake.detach().to(dtype).requires_grad_(True)
    value = lpips(weights, fake, real.detach(), dtype, distance_dtype)
    value.double().mean().backward()
    return value.detach().double(), fake.grad.double()


def max_pool_first(x, k, s):
    """NHWC max-pool, no padding, floor -> (y, winner) where winner [N, OH, OW, C] is the row-major index in the window
    of its FIRST maximum."""
    n, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    xf = x.float()
    y = torch.empty(n, oh, ow, c)
    winner = torch.zeros(n, oh, ow, c, dtype=torch.long)
    for i in range(oh):
        for j in range(ow):
            best = xf[:, i * s, j * s].clone()
            win = torch.zeros(n, c, dtype=torch.long)
            for t in range(1, k * k):
                v = xf[:, i * s + t // k, j * s + t % k]
                take = v > best
                best = torch.where(take, v, best)
                win = torch.where(take, torch.full_like(win, t), win)
            y[:, i, j], winner[:, i, j] = best, win
    return y.to(x.dtype), winner


def max_pool_first_backward(x, g, k, s):
    """dx in float32: every window's gradient added to its first maximum, the windows in row-major order."""
    n, h, w, c = x.shape
    _, winner = max_pool_first(x, k, s)
    dx = torch.zeros(n, h, w, c)
    gf = g.float()
    for i in range(winner.shape[1]):
        for j in range(winner.shape[2]):
            for t in range(k * k):
                hit = winner[:, i, j] == t
                dx[:, i * s + t // k, j * s + t % k] += torch.where(hit, gf[:, i, j], torch.zeros(()))
    return dx


def tied_windows(x, k, s):
    """How many windows hold their maximum more than once."""
    n, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    xf = x.float()
    count = 0
    for i in range(oh):
        for j in range(ow):
            win = xf[:, i * s:i * s + k, j * s:j * s + k].reshape(n, k * k, c)
            count += int(((win == win.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
    return count
