"""Shared by the Gaussian-mixture tests: the adversarial parameter cases of the quantised CDF, the float64 definition of
the training likelihood and its gradients, and the host round trip through the CPU checker."""
import math

import numpy as np
import torch

WINDOWS = (1, 2, 64, 65, 4096)          # L; the last one is ops.mixture_ops.MAX_WINDOW
STREAM_LENGTHS = (1, 63, 64, 65, 129)


def adversarial_parameters(k, L, lo, seed=0):
    """float32 (logits, loc, scale) [N, K]: every scale of {1e-3, 0.11, 256} with means inside the window, 10 L below it
    and 10 L above it, once with plain logits and once with one logit at +40 and at -40."""
    rng = np.random.RandomState(seed + 7 * k + L)
    rows = []
    for sigma in (1e-3, 0.11, 256.0):
        for centre in (lo + 0.5 * (L - 1), lo - 10.0 * L, lo + L - 1 + 10.0 * L, lo + 0.25, lo + L - 1.0):
            for spike in (0.0, 40.0, -40.0):
                logits = rng.uniform(-1.0, 1.0, size=k)
                logits[rng.randint(k)] += spike
                loc = centre + rng.uniform(-0.5, 0.5, size=k) * min(L, 8)
                scale = sigma * rng.uniform(1.0, 1.5, size=k)
                rows.append((logits, loc, scale))
    logits, loc, scale = (torch.tensor(np.stack([r[i] for r in rows]), dtype=torch.float32) for i in range(3))
    return logits, loc, scale


def random_parameters(shape, k, lo, L, seed=0, sigma=(0.3, 4.0)):
    """float32 (logits, loc, scale) of shape + [K] with the means inside the window."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(*shape, k, generator=g)
    loc = lo + torch.rand(*shape, k, generator=g) * max(L - 1, 1)
    scale = sigma[0] + torch.rand(*shape, k, generator=g) * (sigma[1] - sigma[0])
    return logits, loc, scale


def check_cdf_invariants(cdf, L):
    cdf = np.asarray(cdf, dtype=np.int64)
    assert cdf.shape[-1] == L + 1
    assert (cdf[..., 0] == 0).all()
    assert (cdf[..., L] == 65536).all()
    assert (np.diff(cdf, axis=-1) >= 1).all()


def port_round_trip(port, symbols, table, lo):
    """symbols [n] (absolute) through the CPU checker on `table` [n, L + 1] -> (string, decoded absolute symbols)."""
    # debug_level 0: the checker's argument check asks for three CDF entries, a window of one symbol has two
    data = (np.asarray(symbols, dtype=np.int64) - lo).astype(np.int16)
    string = port.range_encode(data, table, 16, debug_level=0)
    back = port.range_decode(string, data.shape, table, 16, debug_level=0).astype(np.int64) + lo
    return string, back


def mixture_log_prob64(y_hat, logits, loc, scale):
    """log p of the noisy mixture in float64, differentiable: log sum_k softmax(logits)_k (Phi(zu_k) - Phi(zl_k)), the
    difference taken through log_ndtr on the side of the median where it does not cancel."""
    y = y_hat.to(torch.float64)[..., None]
    logits, loc, scale = (t.to(torch.float64) for t in (logits, loc, scale))
    zu, zl = (y + 0.5 - loc) / scale, (y - 0.5 - loc) / scale
    right = zu > 0
    log_ndtr = torch.special.log_ndtr
    big = torch.where(right, log_ndtr(-zl), log_ndtr(zu))
    small = torch.where(right, log_ndtr(-zu), log_ndtr(zl))
    lp = big + torch.log1p(-torch.exp(small - big))
    return torch.logsumexp(torch.log_softmax(logits, dim=-1) + lp, dim=-1)


def mixture_bits64(y_hat, logits, loc, scale, coding_rank):
    axes = tuple(range(y_hat.dim() - coding_rank, y_hat.dim()))
    return mixture_log_prob64(y_hat, logits, loc, scale).sum(dim=axes) / -math.log(2.0)


EPS32 = 2.0 ** -24
BF16_ULP = 2.0 ** -8
LN2 = math.log(2.0)


def mixture_terms64(y_hat, logits, loc, scale, gbits):
    """Everything the likelihood tests compare, in float64 and in closed form, with the error scale of each output.

    y_hat [U, E], parameters [U, E, K], gbits [U] = dL/dbits.  Returns a dict of log p [U, E], the gradients dy [U, E]
    and dlogits, dloc, dscale [U, E, K] of L = sum_u gbits_u bits_u, and for each a `n_*` tensor of the same shape: the
    size of a float32 evaluation's error in units of 2^-24, from the operations the formula takes.

    One term lp_k = log(Phi(zu) - Phi(zl)) is formed as big + log1p(-exp(small - big)): an error d in either log_ndtr
    moves it by d / (1 - exp(small - big)), and log_ndtr of a z that carries a relative rounding error moves by about
    z^2 times that, so bracket_k = (1 + zu^2 + zl^2) / (1 - exp(small - big)), as tests/test_bits_kernels_gpu.py holds
    the single Gaussian.  log p = logsumexp_k(logits_k + lp_k) - logsumexp(logits): logsumexp moves by no more than its
    largest argument moves, and each of its exp / log / add steps adds a rounding of the magnitudes it handles, so
      n_lp = max_k bracket_k + (1 + |max_k a_k| + |max_k logits_k| + |log p|).
    A gradient is a product of factors exp(.) whose arguments carry absolute errors: r_k (argument a_k - amax, error
    that of lp_k), phi(z) / P (argument z^2 / 2 + lp_k), softmax(logits)_k; its error scale is the gross size of the
    products before the sum over k cancels anything, times (1 + z^2 / 2 + bracket_k).
    `u_*`: what float32 underflow may take on top, as an absolute amount: a responsibility or a weight below the smallest
    normal float32, 2^-126, is flushed to zero or keeps fewer bits, so each product may be off by 2^-126 times its other
    factors (and a result by 2^-126 itself)."""
    y = y_hat.to(torch.float64)[..., None]
    logits, loc, scale = (t.to(torch.float64) for t in (logits, loc, scale))
    inv = 1.0 / scale
    zu, zl = (y + 0.5 - loc) * inv, (y - 0.5 - loc) * inv
    right = zu > 0
    log_ndtr = torch.special.log_ndtr
    big = torch.where(right, log_ndtr(-zl), log_ndtr(zu))
    small = torch.where(right, log_ndtr(-zu), log_ndtr(zl))
    lp = big + torch.log1p(-torch.exp(small - big))
    bracket = (1 + zu ** 2 + zl ** 2) / -torch.expm1(small - big)
    a = logits + lp
    log_w = torch.log_softmax(logits, dim=-1)
    log_p = torch.logsumexp(log_w + lp, dim=-1)
    n_lp = bracket.amax(dim=-1) + 1 + a.amax(dim=-1).abs() + logits.amax(dim=-1).abs() + log_p.abs()
    r = torch.softmax(a, dim=-1)
    w = torch.exp(log_w)
    c = 0.5 * math.log(2 * math.pi)
    gu = torch.exp(-0.5 * zu ** 2 - c - lp)
    gl = -torch.exp(-0.5 * zl ** 2 - c - lp)
    g = (gbits.to(torch.float64) / -LN2)[:, None, None]
    cond = 2 + 0.5 * zu ** 2 + 0.5 * zl ** 2 + bracket + lp.abs()
    dz = r * (gu + gl) * inv
    n_dz = r * (gu.abs() + gl.abs()) * inv * cond
    tiny = 2.0 ** -126
    u_dz = tiny * (g.abs() * (gu.abs() + gl.abs()) * inv + 1)
    out = {
        "u_dy": u_dz.sum(-1), "u_dloc": u_dz, "u_dlogits": tiny * (2 * g.abs() + 1) * torch.ones_like(r),
        "u_dscale": tiny * (g.abs() * (gu.abs() * zu.abs() + gl.abs() * zl.abs()) * inv + 1),
        "lp": log_p, "n_lp": n_lp,
        "dy": (g * dz).sum(-1), "n_dy": (g.abs() * n_dz).sum(-1),
        "dloc": -g * dz, "n_dloc": g.abs() * n_dz,
        "dscale": -g * r * (gu * zu + gl * zl) * inv,
        "n_dscale": g.abs() * r * (gu.abs() * zu.abs() + gl.abs() * zl.abs()) * inv * cond,
        "dlogits": g * (r - w), "n_dlogits": g.abs() * (r * cond + w * (2 + logits.abs())),
    }
    return out


# Roundings per output, counted on csrc/mixture_bits.hip: a term lp_k takes 2 subtractions, 2 additions, 3 products
# and a reciprocal (8), two log_ndtr (erfc or erfcx and a log: 4 ulp each), exp, log1p and the last add (3); the
# hardware exp and log behind __expf / __logf are 1-2 ulp where the library's are below 1.  24 covers one term; the
# logsumexp and the products of a gradient add K + 6 more of size 1.
OPS = 32
