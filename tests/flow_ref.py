"""The float64 definition of the scale-space warp (include/tfc_hip.h, ops/flow_ops.py) in numpy: the volume, its
adjoint, the warp and its three gradients by their formulas.  No autograd."""
import math

import numpy as np


def radii(num_levels, sigma0):
    return [int(math.ceil(3.0 * sigma0 * 2.0 ** p)) for p in range(num_levels)]


def blur_matrix(n, sigma, normalise=True):
    """[n, n] float64: entry (i, k) is w_{k - i} for |k - i| <= ceil(3 sigma), divided by the row's sum."""
    radius = int(math.ceil(3.0 * sigma))
    d = np.abs(np.arange(n)[None, :] - np.arange(n)[:, None])
    w = np.where(d <= radius, np.exp(-(d.astype(np.float64) ** 2) / (2.0 * sigma * sigma)), 0.0)
    return w / w.sum(axis=1, keepdims=True) if normalise else w


def volume(x, num_levels=5, sigma0=1.5):
    """x [N, H, W, C] -> [N, num_levels + 1, H, W, C]."""
    x = np.asarray(x, np.float64)
    planes = [x]
    for p in range(num_levels):
        sigma = sigma0 * 2.0 ** p
        rows = np.einsum("jk,nikc->nijc", blur_matrix(x.shape[2], sigma), x)
        planes.append(np.einsum("ik,nkjc->nijc", blur_matrix(x.shape[1], sigma), rows))
    return np.stack(planes, axis=1)


def volume_adjoint(g, sigma0=1.5):
    """g [N, M + 1, H, W, C] -> [N, H, W, C]: plane 0 plus, per plane, the zero-padded symmetric correlation of
    g / norm, norm[i, j] = norm_row[j] norm_col[i]."""
    g = np.asarray(g, np.float64)
    out = g[:, 0].copy()
    h, w = g.shape[2], g.shape[3]
    for p in range(g.shape[1] - 1):
        sigma = sigma0 * 2.0 ** p
        taps_w, taps_h = blur_matrix(w, sigma, False), blur_matrix(h, sigma, False)
        norm = taps_h.sum(axis=1)[:, None] * taps_w.sum(axis=1)[None, :]
        scaled = g[:, p + 1] / norm[None, :, :, None]
        cols = np.einsum("ik,nkjc->nijc", taps_h, scaled)          # the taps are symmetric: corr == its transpose
        out += np.einsum("jk,nikc->nijc", taps_w, cols)
    return out


def coordinates(flow, num_planes):
    """The raw float64 sampling coordinates (x, y, z) of flow [N, H, W, 3], each [N, H, W]."""
    flow = np.asarray(flow, np.float64)
    _, h, w, _ = flow.shape
    return (np.arange(w, dtype=np.float64)[None, None, :] + flow[..., 0],
            np.arange(h, dtype=np.float64)[None, :, None] + flow[..., 1], flow[..., 2] + 0.0)


def axis(raw, last):
    """-> (cell 0, cell 1, weight of cell 1, inside): fmin(fmax(raw, 0), last), a NaN going to 0."""
    p = np.fmin(np.fmax(raw, 0.0), float(last))
    a0 = np.minimum(np.floor(p).astype(np.int64), max(last - 1, 0))
    a1 = np.minimum(a0 + 1, last)
    with np.errstate(invalid="ignore"):
        inside = (raw > 0.0) & (raw < last)
    return a0, a1, p - a0, inside


def _cells(vol_shape, flow):
    n, planes, h, w, _ = vol_shape
    rx, ry, rz = coordinates(flow, planes)
    return axis(rx, w - 1), axis(ry, h - 1), axis(rz, planes - 1)


def warp(vol, flow):
    """vol [N, M + 1, H, W, C], flow [N, H, W, 3] -> [N, H, W, C]."""
    vol = np.asarray(vol, np.float64)
    (x0, x1, wx, _), (y0, y1, wy, _), (z0, z1, wz, _) = _cells(vol.shape, flow)
    nn = np.arange(vol.shape[0])[:, None, None]
    out = 0.0
    for z, az in ((z0, 1.0 - wz), (z1, wz)):
        for y, ay in ((y0, 1.0 - wy), (y1, wy)):
            for x, ax in ((x0, 1.0 - wx), (x1, wx)):
                out = out + (az * ay * ax)[..., None] * vol[nn, z, y, x]
    return out


def warp_gradients(vol, flow, g):
    """-> (g_volume [N, M + 1, H, W, C], g_flow [N, H, W, 3]) for g [N, H, W, C]."""
    vol, g = np.asarray(vol, np.float64), np.asarray(g, np.float64)
    (x0, x1, wx, ix), (y0, y1, wy, iy), (z0, z1, wz, iz) = _cells(vol.shape, flow)
    nn = np.broadcast_to(np.arange(vol.shape[0])[:, None, None], x0.shape)
    g_vol = np.zeros_like(vol)
    for z, az in ((z0, 1.0 - wz), (z1, wz)):
        for y, ay in ((y0, 1.0 - wy), (y1, wy)):
            for x, ax in ((x0, 1.0 - wx), (x1, wx)):
                np.add.at(g_vol, (nn, z, y, x), (az * ay * ax)[..., None] * g)
    v = lambda z, y, x: vol[nn, z, y, x]
    ddx = sum(az * ay * (v(z, y, x1) - v(z, y, x0))[..., :].transpose(3, 0, 1, 2)
              for z, az in ((z0, 1.0 - wz), (z1, wz)) for y, ay in ((y0, 1.0 - wy), (y1, wy)))
    ddy = sum(az * ax * (v(z, y1, x) - v(z, y0, x)).transpose(3, 0, 1, 2)
              for z, az in ((z0, 1.0 - wz), (z1, wz)) for x, ax in ((x0, 1.0 - wx), (x1, wx)))
    ddz = sum(ay * ax * (v(z1, y, x) - v(z0, y, x)).transpose(3, 0, 1, 2)
              for y, ay in ((y0, 1.0 - wy), (y1, wy)) for x, ax in ((x0, 1.0 - wx), (x1, wx)))
    gt = g.transpose(3, 0, 1, 2)
    g_flow = np.stack([np.where(ix, (gt * ddx).sum(0), 0.0), np.where(iy, (gt * ddy).sum(0), 0.0),
                       np.where(iz, (gt * ddz).sum(0), 0.0)], axis=-1)
    return g_vol, g_flow


def predict(x, flow, num_levels=5, sigma0=1.5):
    return warp(volume(x, num_levels, sigma0), flow)


def predict_gradients(x, flow, g, num_levels=5, sigma0=1.5):
    """-> (g_x, g_flow)."""
    g_vol, g_flow = warp_gradients(volume(x, num_levels, sigma0), flow, g)
    return volume_adjoint(g_vol, sigma0), g_flow


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = math.sqrt(float(np.sum(want * want)))
    err = math.sqrt(float(np.sum((got - want) ** 2)))
    return err / scale if scale > 0 else err


def make_case(shape, seed):
    """The test inputs of a shape (N, H, W, C, M, sigma0): an image uniform in 0...255, dx and dy odd sixteenths in +-12,
    s an odd sixteenth in [-1, M + 1], and an output gradient; float32 arrays."""
    n, h, w, c, m, _ = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 255.0, (n, h, w, c)).astype(np.float32)
    odd = lambda lo, hi, size: (2 * rng.integers(lo * 8, hi * 8, size) + 1).astype(np.float32) / 16.0
    flow = np.stack([odd(-12, 12, (n, h, w)), odd(-12, 12, (n, h, w)), odd(-1, m + 1, (n, h, w))], axis=-1)
    g = rng.standard_normal((n, h, w, c)).astype(np.float32)
    return x, np.ascontiguousarray(flow), g
