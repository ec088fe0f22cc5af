"""The case lists, inputs and float64 results the two SSIM scale-pass test files share (tests/test_ssim_scale_cpu.py
checks on the CPU that every forward case can tell a right kernel from a wrong one; tests/test_ssim_scale_gpu.py runs
them).  Shapes come from the tile constants of csrc/ssim_params.h through image_ops.SSIM_CONSTANTS.  Not a test module.

A ROUTE is a tap count, or "11rt": 11 taps with TFC_SSIM_RUNTIME_TAPS=1, which sends the window of the models to the
kernels with run-time taps.  With T the tile side of the route's tap count n:
  forward   positions per axis from {1, 2, T-1, T, T+1, 2T+1} (H = positions + n - 1), channels {1, 3, 4}, batch
            {1, 2}, pool on / off: a greedy cover of every pair of values of two axes;
  backward  pixels per axis from {n, n+1, T-1, T, T+1, 2T+1} that are >= n (n+1 is there so that the 31-tap window, whose
            other sizes are all odd, has an even one), channels {1, 3}, batch {1, 2}, the pooled pair's gradient
            present / absent, and dx only, dy only or both: the same cover.
Inputs are 8-bit valued, x = clip(round(128 + 40 N)), y = clip(round(x + 20 N)), every plane with data of its own, so
uint8, bfloat16, float16 and float32 see the same numbers and share one float64 result."""
import functools
import itertools
import zlib

import numpy as np
import torch

import ssim_ref
from compression_amd.ops import image_ops

K = image_ops.SSIM_CONSTANTS
MAX_TAPS = K["SSIM_MAX_TAPS"]
FIXED = K["SSIM_FIXED_TAPS"]
SMALL_MAX = K["SSIM_TILE_SMALL_N_MAX"]

ROUTES = (1, 2, 7, 8, FIXED, "%drt" % FIXED, SMALL_MAX + 1, MAX_TAPS)
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16, "uint8": torch.uint8}
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
NOISE = 20.0                          # sigma of y - x: at 2 many cases cannot tell a mutant from rounding (see the CPU file)
# (kind, case) -> seed, for a case that had to be redrawn because a wrong definition stayed within 4 bars of the right one
REDRAWN = {
    # "columns one short" moved one plane's means by 3.4 bars (the dropped column's mean happened to be the plane's)
    ("fwd", 12, 27, 28, 1, 1): 1,
    # the same mutant, 2.6 bars on one of six planes; seeds 1, 2 and 3 gave 5.0, 3.5 and 20.9, and 3 has the margin
    ("fwd", 8, 39, 72, 3, 2): 3,
}


def taps_of(route):
    return int(str(route).replace("rt", ""))


def runtime_taps(route):
    return str(route).endswith("rt")


def tile_of(n):
    """ssim_tile() of csrc/ssim.hip, restated from the constants."""
    return K["SSIM_TILE_SMALL_N"] if n <= SMALL_MAX else K["SSIM_TILE_LARGE_N"]


def sigma_of(n):
    return 1.5 if n <= 11 else n / 6.0


def window(route):
    """The taps as Python floats, as image_ops passes them."""
    n = taps_of(route)
    return tuple(float(v) for v in ssim_ref.window(n, sigma_of(n)))


POSITION_KINDS = ("1", "2", "T-1", "T", "T+1", "2T+1")
PIXEL_KINDS = ("n", "n+1", "T-1", "T", "T+1", "2T+1")


def extent(kind, n):
    t = tile_of(n)
    return {"1": 1, "2": 2, "n": n, "n+1": n + 1, "T-1": t - 1, "T": t, "T+1": t + 1, "2T+1": 2 * t + 1}[kind]


def pairwise_cover(axes, valid=lambda t: True):
    """A greedy cover of every pair of values of two different axes that occurs in a valid tuple; deterministic."""
    tuples = [t for t in itertools.product(*axes) if valid(t)]
    pairs = [frozenset((i, j, t[i], t[j]) for i in range(len(t)) for j in range(i + 1, len(t))) for t in tuples]
    missing = set().union(*pairs)
    chosen = []
    while missing:
        best = max(range(len(tuples)), key=lambda k: len(pairs[k] & missing))
        chosen.append(tuples[best])
        missing -= pairs[best]
    return chosen


def _forward_cases(routes, oh_kinds, ow_kinds, channels, dtypes=(None,)):
    found = []
    for dt, route, ohk, owk, c, batch, pool in pairwise_cover(
            [dtypes, routes, oh_kinds, ow_kinds, channels, (1, 2), (True, False)]):
        n = taps_of(route)
        case = (route, extent(ohk, n) + n - 1, extent(owk, n) + n - 1, c, batch, pool)
        found.append(case if dt is None else (dt,) + case)
    if dtypes == (None,):
        # a pairwise cover holds no triple: every route also gets one tile down and three across, and the reverse
        for route in routes:
            n, t = taps_of(route), tile_of(taps_of(route))
            found.append((route, t + n - 1, 2 * t + 1 + n - 1, 3, 2, True))
            found.append((route, 2 * t + 1 + n - 1, t - 1 + n - 1, 3, 2, True))
    return list(dict.fromkeys(found))


def _backward_cases(routes, h_kinds, w_kinds, channels, dtypes=(None,)):
    found = []
    fits = lambda t: extent(t[2], taps_of(t[1])) >= taps_of(t[1]) and extent(t[3], taps_of(t[1])) >= taps_of(t[1])    # noqa: E731
    for dt, route, hk, wk, c, batch, pooled, which in pairwise_cover(
            [dtypes, routes, h_kinds, w_kinds, channels, (1, 2), (True, False), ("dx", "dy", "both")], fits):
        n = taps_of(route)
        case = (route, extent(hk, n), extent(wk, n), c, batch, pooled, which)
        found.append(case if dt is None else (dt,) + case)
    if dtypes == (None,):
        # and every route a grid with fewer tiles down than across, and the reverse
        for route in routes:
            n, t = taps_of(route), tile_of(taps_of(route))
            found.append((route, max(n, t), 2 * t + 1, 3, 2, True, "both"))
            found.append((route, 2 * t + 1, max(n, t - 1), 3, 2, True, "both"))
    return list(dict.fromkeys(found))


# (route, H, W, C, batch, pool) and (route, H, W, C, batch, grad_pooled, which); float32
FORWARD = _forward_cases(ROUTES, POSITION_KINDS, POSITION_KINDS, (1, 3, 4))
BACKWARD = _backward_cases(ROUTES, PIXEL_KINDS, PIXEL_KINDS, (1, 3))
# the smaller cover of the other input types: (dtype name,) + a case as above
_OTHER = tuple(d for d in DTYPES if d != "float32")
FORWARD_TYPES = _forward_cases(ROUTES, ("1", "T-1", "2T+1"), ("2", "T", "T+1"), (1, 3), _OTHER)
BACKWARD_TYPES = _backward_cases(ROUTES, ("n", "T+1", "2T+1"), ("n+1", "T-1", "2T+1"), (1, 3), _OTHER)
ALL_FORWARD = FORWARD + [c[1:] for c in FORWARD_TYPES]


def forward_id(case):
    return "n%s-%dx%d-c%d-b%d-%s" % (case[:5] + ("pool" if case[5] else "nopool",))


def backward_id(case):
    return "n%s-%dx%d-c%d-b%d-%s-%s" % (case[:5] + ("gp" if case[5] else "nogp", case[6]))


def _seed(kind, case):
    key = (kind,) + tuple(case)
    if key in REDRAWN:
        return REDRAWN[key]
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def images(kind, route, h, w, c, batch):
    """(x, y) uint8 [batch, H, W, C]; `kind` ("fwd" / "bwd") only separates the random streams."""
    rng = np.random.default_rng(_seed(kind, (route, h, w, c, batch)))
    shape = (batch, h, w, c)
    x = np.clip(np.round(128.0 + 40.0 * rng.standard_normal(shape)), 0, 255)
    y = np.clip(np.round(x + NOISE * rng.standard_normal(shape)), 0, 255)
    x, y = x.astype(np.uint8), y.astype(np.uint8)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def tensor(a):
    """A torch tensor with a copy of `a` (the cached inputs are read-only)."""
    return torch.from_numpy(np.array(a, order="C"))


def planes(img):
    """[B, H, W, C] -> float64 [B * C, H, W]."""
    a = np.moveaxis(np.asarray(img, dtype=np.float64), -1, 1)
    return a.reshape((-1,) + a.shape[2:])


def unplanes(a, batch, c):
    """[B * C, H, W] -> [B, H, W, C]."""
    return np.moveaxis(a.reshape((batch, c) + a.shape[1:]), 1, -1)


@functools.lru_cache(maxsize=None)
def forward_truth(route, h, w, c, batch):
    """(means [B * C, 2], halved x, halved y [B * C, H2, W2]) in float64."""
    x, y = images("fwd", route, h, w, c, batch)
    return ssim_ref.scale_pass(planes(x), planes(y), window(route), C1, C2)


@functools.lru_cache(maxsize=None)
def forward_twin(route, h, w, c, batch):
    """The means of image_ops.scale_reference in float32 on the CPU, as float64 [B * C, 2]."""
    x, y = images("fwd", route, h, w, c, batch)
    means, _, _ = image_ops.scale_reference(tensor(x).float(), tensor(y).float(), window(route),
                                            C1, C2, False)
    return means.double().numpy()


def forward_bar(route, h, w, c, batch):
    """2 |twin - f64| + 1e-6 per plane and component (2: another summation order; 1e-6: the project's float32 slack)."""
    return 2.0 * np.abs(forward_twin(route, h, w, c, batch) - forward_truth(route, h, w, c, batch)[0]) + 1e-6


@functools.lru_cache(maxsize=None)
def backward_inputs(route, h, w, c, batch, pooled):
    """(x, y, g_means [B * C, 2], g_px, g_py [B * C, H2, W2] or None): g_means random with both signs; the pooled pair's
    gradient scaled so that a quarter of it is about the size of the largest moment term."""
    x, y = images("bwd", route, h, w, c, batch)
    rng = np.random.default_rng(_seed("bwd-g", (route, h, w, c, batch)))
    g_means = rng.standard_normal((batch * c, 2)).astype(np.float32)
    g_means[0] = (1.3, -0.7)
    g_px = g_py = None
    if pooled:
        mx, my = ssim_ref.scale_pass_gradients(planes(x), planes(y), window(route), C1, C2, g_means)
        shape = (batch * c, (h + 1) // 2, (w + 1) // 2)
        g_px = (2.0 * np.abs(mx).max() * rng.standard_normal(shape)).astype(np.float32)
        g_py = (2.0 * np.abs(my).max() * rng.standard_normal(shape)).astype(np.float32)
    return x, y, g_means, g_px, g_py


@functools.lru_cache(maxsize=None)
def backward_truth(route, h, w, c, batch, pooled):
    """(dx, dy) float64 [B, H, W, C]."""
    x, y, g_means, g_px, g_py = backward_inputs(route, h, w, c, batch, pooled)
    dx, dy = ssim_ref.scale_pass_gradients(planes(x), planes(y), window(route), C1, C2, g_means, g_px, g_py)
    return unplanes(dx, batch, c), unplanes(dy, batch, c)


def reference_gradients(x, y, taps, c1, c2, g_means, g_px, g_py, dtype):
    """(dx, dy) [B, H, W, C] as float64 arrays: torch autograd through image_ops.scale_reference in `dtype` on the CPU."""
    tx = tensor(x).to(dtype).requires_grad_(True)
    ty = tensor(y).to(dtype).requires_grad_(True)
    means, px, py = image_ops.scale_reference(tx, ty, taps, c1, c2, g_px is not None or g_py is not None)
    value = (means * tensor(g_means).to(dtype)).sum()
    if g_px is not None:
        value = value + (px[..., 0] * tensor(g_px).to(dtype)).sum()
    if g_py is not None:
        value = value + (py[..., 0] * tensor(g_py).to(dtype)).sum()
    value.backward()
    return tx.grad.double().numpy(), ty.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def backward_twin(route, h, w, c, batch, pooled):
    x, y, g_means, g_px, g_py = backward_inputs(route, h, w, c, batch, pooled)
    return reference_gradients(x, y, window(route), C1, C2, g_means, g_px, g_py, torch.float32)


def relative_error(g, g64):
    """max|g - g64| / max|g64|, the gradient error of tests/test_ssim_gpu.py."""
    return float(np.abs(g - g64).max() / np.abs(g64).max())
