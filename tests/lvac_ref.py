"""A float64 numpy definition of LVAC's two operations and their gradients, written from the formulas and importing
nothing of the package: what the kernels AND their tensor-op twins are held to.

Inverse RAHT.  A level is (child_count [parents] of 1s and 2s, coeff [two-child parents]); the children of a node are
adjacent and in order.  With ac [two-child parents, C]:
    child[c] = parent[p(c)] + w(c) ac[k(c)],   w = coeff_k for the left child, 1 for the right, no term for an only child
    dparent[i] = sum over the node's children of dchild;   dac[k] = coeff_k dchild[left_k] + dchild[left_k + 1]

Point decoder.  x[n] = [pos[n]; z[idx[n]]], pre = x W1 + b1, y = relu(pre) W2 + b2, r = y A^T + o (clipped to [0, 255]
on request), loss = sum (r - T)^2 / (3 N)."""
import numpy as np

IDENTITY = (np.eye(3), np.zeros(3))
RGB_TO_YUV = (np.array([[0.212600, 0.715200, 0.072200], [-0.114572, -0.385428, 0.5], [0.5, -0.454153, -0.045847]]),
              np.array([0.0, 128.0, 128.0]))
_M = np.array([[1.0, 0.0, 1.57480], [1.0, -0.18733, -0.46813], [1.0, 1.85563, 0.0]])
YUV_TO_RGB = (_M, _M @ np.array([0.0, -128.0, -128.0]))
AFFINE = {"identity": IDENTITY, "rgb_to_yuv": RGB_TO_YUV, "yuv_to_rgb": YUV_TO_RGB}


def level_tables(child_count, coeff):
    child_count = np.asarray(child_count, np.int64)
    coeff = np.asarray(coeff, np.float64).ravel()
    first = np.cumsum(child_count) - child_count
    left = first[child_count == 2]
    assert len(left) == len(coeff)
    return first, left, coeff


def raht_forward(dc, acs, levels):
    cur = np.asarray(dc, np.float64)
    for ac, (child_count, coeff) in zip(acs, levels):
        first, left, coeff = level_tables(child_count, coeff)
        out = np.repeat(cur, child_count, axis=0)
        ac = np.asarray(ac, np.float64)
        out[left] += coeff[:, None] * ac
        out[left + 1] += ac
        cur = out
    return cur


def raht_backward(g, levels):
    """-> (d_dc, [d_ac per level]) for g = dL/d(output)."""
    g = np.asarray(g, np.float64)
    d_acs = []
    for child_count, coeff in reversed(levels):
        first, left, coeff = level_tables(child_count, coeff)
        d_acs.append(coeff[:, None] * g[left] + g[left + 1])
        parent = np.repeat(np.arange(len(child_count)), child_count)
        up = np.zeros((len(child_count), g.shape[1]))
        np.add.at(up, parent, g)
        g = up
    return g, d_acs[::-1]


def point_mlp(z, idx, pos, w1, b1, w2, b2, target, affine=IDENTITY, clip=False, g=1.0):
    """-> dict(loss, recon, pre, d_w1, d_b1, d_w2, d_b2, d_z) for the upstream gradient g of the loss."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    z, pos, w1, b1, w2, b2, target = map(f, (z, pos, w1, b1, w2, b2, target))
    a, o = np.asarray(affine[0], np.float64).reshape(3, 3), np.asarray(affine[1], np.float64)
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    x = z[idx] if pos is None else np.concatenate([pos, z[idx]], axis=1)
    pre = x @ w1 + b1
    h = np.maximum(pre, 0.0)
    y = h @ w2 + b2
    raw = y @ a.T + o
    recon = np.clip(raw, 0.0, 255.0) if clip else raw
    err = recon - target
    loss = np.sum(err ** 2) / (3 * n)
    d_r = 2.0 * g * err / (3 * n)
    if clip:
        d_r = np.where((raw >= 0.0) & (raw <= 255.0), d_r, 0.0)
    d_y = d_r @ a
    d_h = (d_y @ w2.T) * (pre > 0.0)
    d_x = d_h @ w1.T
    d_z = np.zeros_like(z)
    np.add.at(d_z, idx, d_x[:, x.shape[1] - z.shape[1]:])
    return {"loss": loss, "recon": recon, "pre": pre, "d_w1": x.T @ d_h, "d_b1": d_h.sum(0), "d_w2": h.T @ d_y,
            "d_b2": d_y.sum(0), "d_z": d_z}


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.sqrt(np.sum(want ** 2))
    num = np.sqrt(np.sum((got - want) ** 2))
    return num / den if den > 0 else num
