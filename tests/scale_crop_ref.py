"""The definition of `scale_crop_patches` (include/tfc_hip.h) in numpy: the float32 coordinates exactly as written, the
three interpolations in float64.  What the tensor-op twin is held to; the kernel is held to the twin, bit for bit."""
import numpy as np

F = np.float32


def scale_crop(pool, table, P):
    """pool: uint8 [n]; table: int64 [B, 7] (offset, W, H, OW, OH, top, left) -> float64 [B, P, P, 3]."""
    pool = np.asarray(pool, np.uint8)
    out = np.zeros((len(table), P, P, 3), np.float64)
    for b, (off, W, H, OW, OH, top, left) in enumerate(np.asarray(table, np.int64).tolist()):
        image = pool[off:off + 3 * W * H].reshape(H, W, 3).astype(np.float64)
        sy, sx = F(H) / F(OH), F(W) / F(OW)
        py = (top + np.arange(P)).astype(F) * sy
        px = (left + np.arange(P)).astype(F) * sx
        assert py.dtype == F and px.dtype == F
        y0 = np.minimum(np.floor(py).astype(np.int64), H - 1)
        x0 = np.minimum(np.floor(px).astype(np.int64), W - 1)
        y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
        wy = (py - y0.astype(F)).astype(np.float64)[:, None, None]
        wx = (px - x0.astype(F)).astype(np.float64)[None, :, None]
        tl, tr = image[y0][:, x0], image[y0][:, x1]
        bl, br = image[y1][:, x0], image[y1][:, x1]
        t = tl + (tr - tl) * wx
        bo = bl + (br - bl) * wx
        out[b] = t + (bo - t) * wy
    return out


def random_pool(shapes, seed, lead=0):
    """Images of random bytes back to back behind `lead` filler bytes -> (uint8 pool, [(offset, H, W)])."""
    rng = np.random.default_rng(seed)
    parts, where, at = [np.full(lead, 7, np.uint8)], [], lead
    for h, w in shapes:
        parts.append(rng.integers(0, 256, 3 * h * w, dtype=np.uint8))
        where.append((at, h, w))
        at += 3 * h * w
    return np.concatenate(parts), where
