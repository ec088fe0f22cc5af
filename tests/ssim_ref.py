"""Float64 NumPy oracle of SSIM and multiscale SSIM, written from the definition in DESIGN.md (TensorFlow's
`tf.image.ssim` / `tf.image.ssim_multiscale`, restated there) and from nothing in the package, one scale pass of it with
its closed-form gradient (`scale_pass`, `scale_pass_gradients`: what one kernel launch computes), plus the image-like
test inputs the SSIM tests share.  Not a test module."""
import numpy as np

POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(filter_size=11, filter_sigma=1.5):
    i = np.arange(filter_size, dtype=np.float64)
    g = np.exp(-(i - (filter_size - 1) / 2.0) ** 2 / (2.0 * filter_sigma ** 2))
    return g / g.sum()


def valid_filter(a, g):
    """The 2-D window g g^T over the last two axes of `a`, VALID."""
    n = len(g)
    h, w = a.shape[-2:]
    rows = sum(g[k] * a[..., k:k + h - n + 1, :] for k in range(n))
    return sum(g[k] * rows[..., :, k:k + w - n + 1] for k in range(n))


def position_maps(x, y, g, c1, c2):
    """x, y [..., H, W] float64 -> (l cs, cs) at the valid positions, each [..., H - n + 1, W - n + 1]."""
    mu1, mu2 = valid_filter(x, g), valid_filter(y, g)
    s, p = valid_filter(x * x + y * y, g), valid_filter(x * y, g)
    lum = (2 * mu1 * mu2 + c1) / (mu1 ** 2 + mu2 ** 2 + c1)
    cs = (2 * p - 2 * mu1 * mu2 + c2) / (s - (mu1 ** 2 + mu2 ** 2) + c2)        # symmetric in x, y to the bit
    return lum * cs, cs


def scale_maps(x, y, max_val, g, k1=0.01, k2=0.03):
    """x, y [..., H, W] float64 -> (ssim_plane, cs_plane), each [...]."""
    lcs, cs = position_maps(x, y, g, (k1 * max_val) ** 2, (k2 * max_val) ** 2)
    return lcs.mean(axis=(-2, -1)), cs.mean(axis=(-2, -1))


def halve(a):
    """Mean of each 2x2 block; an odd side first repeats its last row / column."""
    h, w = a.shape[-2:]
    if h % 2:
        a = np.concatenate([a, a[..., -1:, :]], axis=-2)
    if w % 2:
        a = np.concatenate([a, a[..., :, -1:]], axis=-1)
    return 0.25 * (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2])


def scale_pass(x, y, taps, c1, c2):
    """One scale of DESIGN.md §13 on planes x, y [planes, H, W]: -> (means [planes, 2] = (ssim_plane, cs_plane), halved x,
    halved y [planes, ceil(H / 2), ceil(W / 2)]).  The arithmetic of `scale_maps`, with C1 and C2 given."""
    x, y, g = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(taps, np.float64)
    lcs, cs = position_maps(x, y, g, c1, c2)
    return np.stack([lcs.mean(axis=(-2, -1)), cs.mean(axis=(-2, -1))], axis=-1), halve(x), halve(y)


def full_correlation(a, g):
    """The adjoint of `valid_filter`: a [..., OH, OW] -> [..., OH + n - 1, OW + n - 1], out[i, j] = sum g[k] g[l] a[i - k, j - l]."""
    n = len(g)
    oh, ow = a.shape[-2:]
    rows = np.zeros(a.shape[:-2] + (oh + n - 1, ow))
    for k in range(n):
        rows[..., k:k + oh, :] += g[k] * a
    out = np.zeros(a.shape[:-2] + (oh + n - 1, ow + n - 1))
    for k in range(n):
        out[..., :, k:k + ow] += g[k] * rows
    return out


def halve_adjoint(gp, h, w):
    """The adjoint of `halve` for an H x W plane: a quarter of gp[i // 2, j // 2], twice that on the last row / column of
    an odd side (the repeated one folds back onto it)."""
    up = np.repeat(np.repeat(np.asarray(gp, np.float64), 2, axis=-2), 2, axis=-1)[..., :h, :w] * 0.25
    if h % 2:
        up[..., -1, :] *= 2.0
    if w % 2:
        up[..., :, -1] *= 2.0
    return up


def scale_pass_gradients(x, y, taps, c1, c2, g_means, g_px=None, g_py=None):
    """(dx, dy) of  sum(g_means * means) + sum(g_px * halved x) + sum(g_py * halved y)  for `scale_pass`, in closed form:
    with V = (g0 l cs + g1 cs) / positions at every position, a1 = dV/dmu1, a2 = dV/dmu2, b = dV/dS, c = dV/dP and F' the
    full correlation with the window,
        dx = F'(a1) + 2 x F'(b) + y F'(c),   dy = F'(a2) + 2 y F'(b) + x F'(c),
    plus the adjoint of the pool where g_px / g_py is given."""
    x, y, g = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(taps, np.float64)
    g_means = np.asarray(g_means, np.float64)
    h, w = x.shape[-2:]
    mu1, mu2 = valid_filter(x, g), valid_filter(y, g)
    s, p = valid_filter(x * x + y * y, g), valid_filter(x * y, g)
    count = mu1.shape[-2] * mu1.shape[-1]
    ld = mu1 ** 2 + mu2 ** 2 + c1
    lum = (2 * mu1 * mu2 + c1) / ld
    cd = s - (mu1 ** 2 + mu2 ** 2) + c2
    cs = (2 * p - 2 * mu1 * mu2 + c2) / cd
    wa, wb = g_means[..., 0, None, None] / count, g_means[..., 1, None, None] / count
    v_l, v_cs = wa * cs, wa * lum + wb                                           # dV/dl, dV/dcs
    a1 = v_l * (2 * mu2 - 2 * mu1 * lum) / ld + v_cs * (2 * mu1 * cs - 2 * mu2) / cd
    a2 = v_l * (2 * mu1 - 2 * mu2 * lum) / ld + v_cs * (2 * mu2 * cs - 2 * mu1) / cd
    b = -v_cs * cs / cd
    c = 2 * v_cs / cd
    fb, fc = full_correlation(b, g), full_correlation(c, g)
    dx = full_correlation(a1, g) + 2 * x * fb + y * fc
    dy = full_correlation(a2, g) + 2 * y * fb + x * fc
    if g_px is not None:
        dx = dx + halve_adjoint(g_px, h, w)
    if g_py is not None:
        dy = dy + halve_adjoint(g_py, h, w)
    return dx, dy


def _planes(img):
    """[..., H, W, C] -> float64 [..., C, H, W]."""
    return np.moveaxis(np.asarray(img, dtype=np.float64), -1, -3)


def _check(img1, img2, filter_size, scales):
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if img1.shape != img2.shape:
        raise ValueError("shapes differ")
    need = (filter_size - 1) * 2 ** (scales - 1) + 1
    if img1.shape[-3] < need or img1.shape[-2] < need:
        raise ValueError(f"smallest accepted side is {need}")


def ssim(img1, img2, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    _check(img1, img2, filter_size, 1)
    value, _ = scale_maps(_planes(img1), _planes(img2), float(max_val), window(filter_size, filter_sigma), k1, k2)
    return value.mean(axis=-1)


def ssim_multiscale_parts(img1, img2, max_val, power_factors=POWER_FACTORS, filter_size=11, filter_sigma=1.5, k1=0.01,
                          k2=0.03):
    """-> (result [...], per-scale values before the relu [..., C, scales], [(H, W) of every scale])."""
    _check(img1, img2, filter_size, len(power_factors))
    g = window(filter_size, filter_sigma)
    x, y = _planes(img1), _planes(img2)
    values, sizes = [], []
    for j in range(len(power_factors)):
        if j:
            x, y = halve(x), halve(y)
        sizes.append(x.shape[-2:])
        value, cs = scale_maps(x, y, float(max_val), g, k1, k2)
        values.append(value if j == len(power_factors) - 1 else cs)
    raw = np.stack(values, axis=-1)
    result = np.prod(np.maximum(raw, 0.0) ** np.asarray(power_factors, dtype=np.float64), axis=-1).mean(axis=-1)
    return result, raw, sizes


def ssim_multiscale(img1, img2, max_val, **kw):
    return ssim_multiscale_parts(img1, img2, max_val, **kw)[0]


# ---------------------------------------------------------------------------------------------------------------------
# image-like inputs
# ---------------------------------------------------------------------------------------------------------------------

def _blur(a, g):
    """SAME-size separable blur over axes -3, -2 of [..., H, W, C] (edge replicated)."""
    r = len(g) // 2
    pad = [(0, 0)] * a.ndim
    pad[-3] = pad[-2] = (r, r)
    p = np.pad(a, pad, mode="edge")
    h, w = a.shape[-3], a.shape[-2]
    rows = sum(g[k] * p[..., k:k + h, :, :] for k in range(len(g)))
    return sum(g[k] * rows[..., :, k:k + w, :] for k in range(len(g)))


def smooth_image(rng, shape):
    """A smooth random field (low-passed noise) plus a few edges, in [0, 255], float64 [..., H, W, C]."""
    h, w = shape[-3], shape[-2]
    field = rng.standard_normal(shape)
    for sigma in (6.0, 6.0):
        field = _blur(field, window(int(6 * sigma) | 1, sigma))
    field = field / (np.abs(field).max() + 1e-12)
    img = 128.0 + 90.0 * field
    for _ in range(4):                                       # edges: rectangles of another level
        r0, r1 = sorted(rng.integers(0, h, 2))
        c0, c1 = sorted(rng.integers(0, w, 2))
        img[..., r0:r1 + 1, c0:c1 + 1, :] += rng.uniform(-50, 50)
    return np.clip(img, 0, 255)


DEGRADATIONS = ("blur", "noise2", "noise8", "noise20", "quant", "all")


def image_pair(seed, shape, degradation):
    """(original, degraded), both 8-bit valued uint8 [..., H, W, C]."""
    rng = np.random.default_rng(seed)
    x = np.round(smooth_image(rng, shape))
    if degradation == "blur":
        y = _blur(x, window(7, 1.2))
    elif degradation.startswith("noise"):
        y = x + float(degradation[5:]) * rng.standard_normal(shape)
    elif degradation == "quant":
        y = np.floor(x / 24.0) * 24.0 + 12.0
    elif degradation == "all":
        y = _blur(x, window(7, 1.2)) + 20.0 * rng.standard_normal(shape)
        y = np.floor(y / 24.0) * 24.0 + 12.0
    else:
        raise ValueError(degradation)
    return x.astype(np.uint8), np.clip(np.round(y), 0, 255).astype(np.uint8)
