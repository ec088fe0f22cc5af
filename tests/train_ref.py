"""The yardsticks of the training ops (numpy): what `ops.train_ops` and csrc/train.hip are held to.

crop: out[b] = image_b[top : top + P, left : left + P, :], where image_b is the [H, W, 3] array that starts at byte
`offset` of the pool; only its width is needed to find the rows.

Keras Adam (tf.keras.optimizers.Adam, Keras 2.14 `update_step`), one step in float64 from float32 inputs:
    m' = m + (g - m) (1 - beta_1)
    v' = v + (g g - v) (1 - beta_2)
    p' = p - m' alpha / (sqrt(v') + epsilon),   alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t),   t = 1, 2, ...
The float32 form rounds (g - m), the product, the sum; g g, the difference, the product, the sum; m' alpha, the root,
the sum with epsilon, the quotient, the difference.  The bounds below count those roundings, half a unit in the last
place (2^-24 relative) each, against the magnitudes they occur at."""
import numpy as np

U = 2.0 ** -24       # half a unit in the last place of float32, relative


def crop(pool, table, patchsize):
    """pool: uint8 [n]; table: int [B, 4] of (offset, width, top, left) -> uint8 [B, P, P, 3], by slicing."""
    P = patchsize
    out = np.zeros((len(table), P, P, 3), np.uint8)
    for b, (off, w, top, left) in enumerate(np.asarray(table).tolist()):
        rows = np.stack([pool[off + ((top + r) * w + left) * 3: off + ((top + r) * w + left + P) * 3] for r in range(P)])
        out[b] = rows.reshape(P, P, 3)
    return out


def adam_alpha(lr, beta_1, beta_2, step):
    return lr * np.sqrt(1.0 - beta_2 ** step) / (1.0 - beta_1 ** step)


def adam_moments(g, m, v, beta_1, beta_2):
    """-> (m', v') in float64."""
    g, m, v = (np.asarray(a, np.float64) for a in (g, m, v))
    return m + (g - m) * (1.0 - beta_1), v + (g * g - v) * (1.0 - beta_2)


def adam_update(m1, v1, lr, beta_1, beta_2, epsilon, step):
    """The update u = m' alpha / (sqrt(v') + epsilon) in float64, from given m', v'."""
    m1, v1 = np.asarray(m1, np.float64), np.asarray(v1, np.float64)
    return m1 * adam_alpha(lr, beta_1, beta_2, step) / (np.sqrt(v1) + epsilon)


def adam_bounds(p, g, m, v, m1_twin, v1_twin, lr, beta_1, beta_2, epsilon, step):
    """-> ((m' float64, bound), (v' float64, bound), (p' float64 from the twin's own m', v', bound))."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m1, v1 = adam_moments(g, m, v, beta_1, beta_2)
    u = adam_update(m1_twin, v1_twin, lr, beta_1, beta_2, epsilon, step)
    p1 = p - u
    return ((m1, 4 * U * (np.abs(g) + np.abs(m))), (v1, 5 * U * (g * g + np.abs(v))),
            (p1, 8 * U * (np.abs(p1) + np.abs(u))))
