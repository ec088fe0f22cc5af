"""The definition of entropy-constrained vector quantisation (include/tfc_hip.h, tfc_vecvq_assign / _backward) in
float64 NumPy.  Inputs are taken as the float32 values they are.  Not a test module."""
import numpy as np


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def scale_of(distortion, d):
    assert distortion in ("sse", "mse")
    return 1.0 / d if distortion == "mse" else 1.0


def costs(x, codebook, rates, lmbda, distortion="sse"):
    """-> (cost [N, K], dist [N, K]) in float64."""
    x, c, r = _f64(x), _f64(codebook), _f64(rates)
    dist = np.empty((x.shape[0], c.shape[0]))
    for at in range(0, x.shape[0], 256):
        diff = x[at:at + 256, None, :] - c[None, :, :]
        dist[at:at + 256] = (diff * diff).sum(-1)
    dist *= scale_of(distortion, x.shape[1])
    return r[None, :] + float(lmbda) * dist, dist


def assign(x, codebook, rates, lmbda, distortion="sse"):
    """-> (index [N] (lowest k among equal costs: np.argmin's rule), rate [N], distortion [N])."""
    cost, dist = costs(x, codebook, rates, lmbda, distortion)
    index = np.argmin(cost, axis=1)
    rows = np.arange(cost.shape[0])
    return index.astype(np.int64), _f64(rates)[index], dist[rows, index]


def gradients(x, codebook, index, g_rate, g_dist, distortion="sse"):
    """The written-out formulas -> (d_rates [K], d_codebook [K, D], d_x [N, D]) in float64; a None gradient is zero."""
    x, c = _f64(x), _f64(codebook)
    index = np.asarray(index.detach().cpu().numpy() if hasattr(index, "detach") else index, dtype=np.int64)
    n, d = x.shape
    k = c.shape[0]
    g_rate = np.zeros(n) if g_rate is None else _f64(g_rate)
    g_dist = np.zeros(n) if g_dist is None else _f64(g_dist)
    two_s = 2.0 * scale_of(distortion, d)
    d_rates = np.zeros(k)
    np.add.at(d_rates, index, g_rate)
    d_codebook = np.zeros((k, d))
    np.add.at(d_codebook, index, g_dist[:, None] * (c[index] - x))
    d_codebook *= two_s
    d_x = two_s * g_dist[:, None] * (x - c[index])
    return d_rates, d_codebook, d_x
