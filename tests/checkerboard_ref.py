"""The checkerboard context model of ops/checkerboard_ops.py as a float64 definition in numpy, position by position,
and the shapes the checkerboard tests share.  Inputs and weights are `context_ref.make_case`'s (the weights travel as
that tuple; the checkerboard mask is applied here, whatever the other taps hold).

Checked on the CPU with these weights and num_scales = 64: every shape of GPU_SHAPES uses at least 11 distinct
tables, holds at least one +-300 element on a table of index <= 45 (a proxy for taking the escape: the tables
themselves need the device) and keeps y_hat finite."""
import numpy as np

from context_ref import index_prepare, make_case, network  # noqa: F401

CHECKER_TAPS = tuple((di, dj) for di in range(-2, 3) for dj in range(-2, 3) if (di + dj) % 2)

# positions of one workgroup of csrc/space_channel.hip (CKB_TILE)
KERNEL_TILE = 32

# (B, Hl, Wl, M, H1, H2); P = 2M
GPU_SHAPES = [
    (1, 1, 2, 8, 26, 21),           # one position per pass
    (1, 2, 1, 8, 26, 21),           # single column
    (2, 3, 2, 8, 26, 21),           # small batch
    (3, 4, 7, 16, 53, 42),          # odd width; K not a multiple of 4
    (2, 5, 6, 8, 26, 21),           # even width, odd height
    (1, 20, 52, 8, 26, 21),         # many tiles
    (1, 3, 7, 192, 640, 512),       # the model's widths
    (2, 9, 8, 192, 640, 512),       # model widths over more than one tile: 36 positions per pass
    (2, 9, 15, 8, 26, 21),          # 68 and 67 positions per pass: more than two tiles of 32, no multiple of 32
]


def is_anchor(i, j):
    return (i + j) % 2 == 0


def pass_positions(hl, wl, pass_):
    """The positions of a pass in compact (raster) order."""
    return [(i, j) for i in range(hl) for j in range(wl) if is_anchor(i, j) == (pass_ == 0)]


def slot(i, j, wl):
    """The closed form of a position's place in its pass."""
    return (i * wl + j) >> 1 if wl % 2 else i * (wl // 2) + (j >> 1)


def context_at(y_hat, i, j, weights):
    """ctx[:, i, j]: the bias for an anchor, the bias and the 12 taps over y_hat [B, Hl, Wl, M] otherwise."""
    kernel, bias = weights[0], weights[1]
    hl, wl = y_hat.shape[1:3]
    ctx = np.broadcast_to(bias, (y_hat.shape[0], bias.shape[0])).copy()
    if is_anchor(i, j):
        return ctx
    for di, dj in CHECKER_TAPS:
        ii, jj = i + di, j + dj
        if 0 <= ii < hl and 0 <= jj < wl:
            ctx = ctx + y_hat[:, ii, jj] @ kernel[di + 2, dj + 2]
    return ctx


def checkerboard_scan(y, psi, weights, num_scales, dtype=np.float64):
    """-> dict(sym, idx, mu, y_hat, index_float) in the full layout: pass 0, then pass 1."""
    weights = tuple(np.asarray(w, dtype) for w in weights)
    y, psi = np.asarray(y, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y.shape
    y_hat, mu, index_float = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    sym = np.zeros(y.shape, np.int32)
    for pass_ in (0, 1):
        decoded = y_hat.copy()                        # a pass sees what the passes before it decoded
        for i, j in pass_positions(hl, wl, pass_):
            out = network(context_at(decoded, i, j, weights), psi[:, i, j], weights)
            mu[:, i, j], index_float[:, i, j] = out[:, :m], out[:, m:]
            r = np.rint(y[:, i, j] - out[:, :m])
            sym[:, i, j] = r.astype(np.int32)
            y_hat[:, i, j] = r + out[:, :m]
    return dict(sym=sym, idx=index_prepare(index_float, num_scales), mu=mu, y_hat=y_hat, index_float=index_float)


def checkerboard_parameters(y_hat, psi, weights, dtype=np.float64):
    """The teacher-forced definition -> (mu, index_float) in the full layout."""
    weights = tuple(np.asarray(w, dtype) for w in weights)
    y_hat, psi = np.asarray(y_hat, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y_hat.shape
    mu, index_float = np.zeros_like(y_hat), np.zeros_like(y_hat)
    for i in range(hl):
        for j in range(wl):
            out = network(context_at(y_hat, i, j, weights), psi[:, i, j], weights)
            mu[:, i, j], index_float[:, i, j] = out[:, :m], out[:, m:]
    return mu, index_float


def split(t):
    """[B, Hl, Wl, C] -> (pass 0, pass 1), compact, by the list of positions."""
    hl, wl = t.shape[1:3]
    return tuple(np.stack([t[:, i, j] for i, j in pass_positions(hl, wl, p)], axis=1) if pass_positions(hl, wl, p)
                 else np.zeros((t.shape[0], 0, t.shape[3]), t.dtype) for p in (0, 1))
