"""The space-channel context model of ops/scctx_ops.py as a float64 definition in numpy, position by position and step
by step, its teacher-forced form, the stream slicing by list, and the shapes and inputs the scctx tests share.

Weights travel as a list with one tuple per group: (kernel_ch [5, 5, c_g, 2 M_g] or None, kernel_sp [5, 5, M_g, 2 M_g],
kernel_bias, w1 [2 M_g + P, H1], b1, w2, b2, w3, b3); the checkerboard mask is applied to kernel_sp here, whatever the
other taps hold.  The hidden widths are the model's rule (H1 = out + 2 (in - out) // 3, H2 = out + (in - out) // 3).

Checked on the CPU with these weights and num_scales = 64 (`describe_shapes`, test_scctx_cpu.py asserts it): every
shape of GPU_SHAPES uses at least 15 distinct tables (15 on the first shape with its 16 elements, 45 on the second, 63
or 64 on all others), holds a +-300 element in every group, in every group one on a table of index <= 45 (a proxy for
taking the escape: the tables themselves need the device), and keeps y_hat finite."""
import numpy as np

from context_ref import ESCAPE_VALUE, SEED, index_prepare, network  # noqa: F401
from checkerboard_ref import CHECKER_TAPS, is_anchor, pass_positions

ALL_TAPS = tuple((di, dj) for di in range(-2, 3) for dj in range(-2, 3))

# (B, Hl, Wl, groups, stream_positions); P = 2 M
GPU_SHAPES = [
    (1, 1, 2, (4, 4), 64),                      # one position per pass, two groups
    (2, 3, 2, (3, 5), 1),                       # c_1 = 3 is no multiple of the K padding; one position per stream
    (3, 4, 7, (4, 4, 8), 5),                    # odd width; ragged last stream in both passes
    (2, 5, 6, (8,), 64),                        # one group: must equal the checkerboard kernel
    (1, 2, 5, (70, 10), 64),                    # earlier-group range longer than one staged chunk of 64 rows
    (1, 20, 52, (4, 4, 8), 64),                 # many tiles, many streams
    (2, 9, 15, (4, 12), 32),                    # 68 / 67 positions: more than two tiles, no multiple of 32; stream = tile
    (1, 3, 7, (16, 16, 32, 64, 64), 64),        # the model's widths
    (2, 9, 8, (16, 16, 32, 64, 64), 16),        # the model's widths over two tiles
]


def hidden_widths(m_g, p):
    out = 2 * m_g
    return out + 2 * p // 3, out + p // 3


def offsets(groups):
    return [sum(groups[:g]) for g in range(len(groups))]


def context_at(y_hat, i, j, group, c_g, pass_):
    """ctx_g[:, i, j] of a step: the bias, all 25 taps over the channels below c_g, and in pass 1 the 12 checkerboard
    taps over the group's own channels of y_hat [B, Hl, Wl, M]."""
    kernel_ch, kernel_sp, bias = group[0], group[1], group[2]
    m_g = kernel_sp.shape[2]
    hl, wl = y_hat.shape[1:3]
    ctx = np.broadcast_to(bias, (y_hat.shape[0], bias.shape[0])).copy()
    if c_g:
        for di, dj in ALL_TAPS:
            ii, jj = i + di, j + dj
            if 0 <= ii < hl and 0 <= jj < wl:
                ctx = ctx + y_hat[:, ii, jj, :c_g] @ kernel_ch[di + 2, dj + 2]
    if pass_ == 1:
        for di, dj in CHECKER_TAPS:
            ii, jj = i + di, j + dj
            if 0 <= ii < hl and 0 <= jj < wl:
                ctx = ctx + y_hat[:, ii, jj, c_g:c_g + m_g] @ kernel_sp[di + 2, dj + 2]
    return ctx


def _cast(weights, dtype):
    return [tuple(None if w is None else np.asarray(w, dtype) for w in group) for group in weights]


def scctx_scan(y, psi, weights, num_scales, dtype=np.float64):
    """-> dict(sym, idx, mu, y_hat, index_float) in the full layout: group 0 pass 0, group 0 pass 1, group 1 pass 0..."""
    weights = _cast(weights, dtype)
    y, psi = np.asarray(y, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y.shape
    y_hat, mu, index_float = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    sym = np.zeros(y.shape, np.int32)
    c_g = 0
    for group in weights:
        m_g = group[1].shape[2]
        ch = slice(c_g, c_g + m_g)
        for pass_ in (0, 1):
            decoded = y_hat.copy()                    # a step sees what the steps before it decoded
            for i, j in pass_positions(hl, wl, pass_):
                out = network(context_at(decoded, i, j, group, c_g, pass_), psi[:, i, j], group[1:])
                mu[:, i, j, ch], index_float[:, i, j, ch] = out[:, :m_g], out[:, m_g:]
                r = np.rint(y[:, i, j, ch] - out[:, :m_g])
                sym[:, i, j, ch] = r.astype(np.int32)
                y_hat[:, i, j, ch] = r + out[:, :m_g]
        c_g += m_g
    return dict(sym=sym, idx=index_prepare(index_float, num_scales), mu=mu, y_hat=y_hat, index_float=index_float)


def scctx_parameters(y_hat, psi, weights, dtype=np.float64):
    """The teacher-forced definition -> (mu, index_float) in the full layout."""
    weights = _cast(weights, dtype)
    y_hat, psi = np.asarray(y_hat, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y_hat.shape
    mu, index_float = np.zeros_like(y_hat), np.zeros_like(y_hat)
    c_g = 0
    for group in weights:
        m_g = group[1].shape[2]
        for i in range(hl):
            for j in range(wl):
                pass_ = 0 if is_anchor(i, j) else 1
                out = network(context_at(y_hat, i, j, group, c_g, pass_), psi[:, i, j], group[1:])
                mu[:, i, j, c_g:c_g + m_g], index_float[:, i, j, c_g:c_g + m_g] = out[:, :m_g], out[:, m_g:]
        c_g += m_g
    return mu, index_float


def streams(t, stream_positions):
    """A compact array [B, N, C] -> the list of its streams [B, n_s, C], by the list of slots."""
    n = t.shape[1]
    return [t[:, list(range(s, min(s + stream_positions, n)))] for s in range(0, n, stream_positions)]


def stream_total(hl, wl, groups, stream_positions):
    """T: the strings of one image."""
    return len(groups) * sum(-(-len(pass_positions(hl, wl, p)) // stream_positions) for p in (0, 1))


def make_case(shape, num_scales=64, seed=SEED):
    """-> (y, psi float32 arrays, weights: list of float32 tuples), seeded the way `context_ref.make_case` is.  Every
    17th element of every group of y, sign alternating, is +-ESCAPE_VALUE.  The last layer of every group is scaled so that,
    teacher-forced on rint(y), its index half spreads over all tables (mean (num_scales - 1) / 2, standard deviation
    num_scales / 3) and its means have unit scale."""
    b, hl, wl, groups, _ = shape
    m = sum(groups)
    p = 2 * m
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * m + 10 * hl + wl + 100000 * len(groups)))
    y = rng.normal(0.0, 3.0, (b, hl, wl, m))
    for c_g, m_g in zip(offsets(groups), groups):     # counted inside every group, so that each group holds some
        flat = y[..., c_g:c_g + m_g].reshape(-1)
        hot = np.arange(1, flat.size, 17)
        flat[hot] = ESCAPE_VALUE * np.where(np.arange(hot.size) % 2 == 0, 1.0, -1.0)
        y[..., c_g:c_g + m_g] = flat.reshape(b, hl, wl, m_g)
    psi = rng.normal(0.0, 1.0, (b, hl, wl, p))

    def dense(k, n):
        return rng.normal(0.0, 1.0 / np.sqrt(k), (k, n))

    weights, c_g = [], 0
    for m_g in groups:
        h1, h2 = hidden_widths(m_g, p)
        # the +-300 elements of the earlier groups reach ctx through kernel_ch: keep its sum of order one
        kernel_ch = rng.normal(0.0, 1.0 / (30.0 * np.sqrt(25 * c_g)), (5, 5, c_g, 2 * m_g)) if c_g else None
        kernel_sp = rng.normal(0.0, 1.0 / (30.0 * np.sqrt(12 * m_g)), (5, 5, m_g, 2 * m_g))
        group = [kernel_ch, kernel_sp, rng.normal(0, 0.1, 2 * m_g), dense(2 * m_g + p, h1), rng.normal(0, 0.1, h1),
                 dense(h1, h2), rng.normal(0, 0.1, h2), dense(h2, 2 * m_g), np.zeros(2 * m_g)]
        weights.append(group)
        c_g += m_g
    mu, index = scctx_parameters(np.rint(y), psi, weights)
    c_g = 0
    for group, m_g in zip(weights, groups):
        mu_g, index_g = mu[..., c_g:c_g + m_g], index[..., c_g:c_g + m_g]
        spread = (num_scales / 3.0) / max(index_g.std(), 1e-6)
        group[7][:, :m_g] /= max(mu_g.std(), 1e-6)
        group[7][:, m_g:] *= spread
        group[8][m_g:] = (num_scales - 1) / 2.0 - index_g.mean() * spread
        c_g += m_g
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    return f32(y), f32(psi), [tuple(f32(w) for w in group) for group in weights]


def describe_shapes(num_scales=64):
    """Per shape of GPU_SHAPES: (distinct tables, per group whether a +-300 element sits on a table of index <= 45, y_hat
    finite), from the float64 definition."""
    out = []
    for shape in GPU_SHAPES:
        y, psi, weights = make_case(shape, num_scales)
        scan = scctx_scan(y, psi, weights, num_scales)
        hot = np.abs(y) == ESCAPE_VALUE
        per_group = [bool((hot[..., c:c + m_g] & (scan["idx"][..., c:c + m_g] <= 45)).any())
                     for c, m_g in zip(offsets(shape[3]), shape[3])]
        out.append((int(np.unique(scan["idx"]).size), per_group, bool(np.isfinite(scan["y_hat"]).all())))
    return out
