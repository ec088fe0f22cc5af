"""The context model of ops/context_ops.py as a float64 definition in numpy, a CPU restatement of the decode loop
(network and range decoder alternating position by position), and the inputs the context tests share.

Weights travel as a tuple of arrays (kernel [5, 5, M, 2M], kernel_bias, w1 [2M + P, H1], b1, w2, b2, w3, b3); the
mask is applied here, whatever the non-causal taps hold."""
import numpy as np

CAUSAL_TAPS = tuple((di, dj) for di in range(-2, 1) for dj in range(-2, 3) if di < 0 or dj < 0)
M32 = 0xFFFFFFFF


def wavefront_order(hl, wl):
    """Positions sorted by step t = j + 3 i, rows ascending inside a step."""
    return sorted(((i, j) for i in range(hl) for j in range(wl)), key=lambda ij: (ij[1] + 3 * ij[0], ij[0]))


def raster_order(hl, wl):
    return [(i, j) for i in range(hl) for j in range(wl)]


def _lrelu(v):
    return np.where(v > 0, v, 0.2 * v)


def network(ctx, psi, weights):
    _, _, w1, b1, w2, b2, w3, b3 = weights
    h = _lrelu(np.concatenate([ctx, psi], axis=-1) @ w1 + b1)
    h = _lrelu(h @ w2 + b2)
    return h @ w3 + b3


def context_at(y_hat, i, j, weights):
    """ctx[:, i, j] from the causal neighbourhood of y_hat [B, Hl, Wl, M]."""
    kernel, bias = weights[0], weights[1]
    wl = y_hat.shape[2]
    ctx = np.broadcast_to(bias, (y_hat.shape[0], bias.shape[0])).copy()
    for di, dj in CAUSAL_TAPS:
        ii, jj = i + di, j + dj
        if ii >= 0 and 0 <= jj < wl:
            ctx = ctx + y_hat[:, ii, jj] @ kernel[di + 2, dj + 2]
    return ctx


def index_prepare(index_float, num_scales):
    return np.clip(np.nan_to_num(index_float, nan=0.0), 0, num_scales - 1).astype(np.int32)     # toward zero: >= 0


def context_scan(y, psi, weights, num_scales, order=None, dtype=np.float64):
    """-> dict(sym, idx, mu, y_hat, index_float).  `order`: a list of positions (default raster)."""
    weights = tuple(np.asarray(w, dtype) for w in weights)
    y, psi = np.asarray(y, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y.shape
    y_hat, mu, index_float = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    sym = np.zeros(y.shape, np.int32)
    for i, j in (order or raster_order(hl, wl)):
        out = network(context_at(y_hat, i, j, weights), psi[:, i, j], weights)
        mu[:, i, j], index_float[:, i, j] = out[:, :m], out[:, m:]
        r = np.rint(y[:, i, j] - out[:, :m])
        sym[:, i, j] = r.astype(np.int32)
        y_hat[:, i, j] = r + out[:, :m]
    return dict(sym=sym, idx=index_prepare(index_float, num_scales), mu=mu, y_hat=y_hat, index_float=index_float)


def context_parameters(y_hat, psi, weights, dtype=np.float64):
    """The teacher-forced definition -> (mu, index_float)."""
    weights = tuple(np.asarray(w, dtype) for w in weights)
    y_hat, psi = np.asarray(y_hat, dtype), np.asarray(psi, dtype)
    b, hl, wl, m = y_hat.shape
    padded = np.pad(y_hat, ((0, 0), (2, 0), (2, 2), (0, 0)))
    ctx = np.broadcast_to(weights[1], (b, hl, wl, 2 * m)).copy()
    for di, dj in CAUSAL_TAPS:
        ctx = ctx + padded[:, 2 + di:2 + di + hl, 2 + dj:2 + dj + wl] @ weights[0][di + 2, dj + 2]
    out = network(ctx, psi, weights)
    return out[..., :m], out[..., m:]


class RowDecoder:
    """The range decoder of one string as the device runs it (csrc/range_wave.h: DecoderState, dec_symbol, dec_bit,
    dec_escape; RangeDecoder of cc/lib/range_coder.h): 16-bit digits, zeros past the end."""

    def __init__(self, data):
        self.data = bytes(data)
        self.base, self.span_m1, self.pulls = 0, M32, 0
        self.window = (self._digit() << 16) | self._digit()

    def _digit(self):
        at = 2 * self.pulls
        self.pulls += 1
        hi = self.data[at] if at < len(self.data) else 0
        lo = self.data[at + 1] if at + 1 < len(self.data) else 0
        return (hi << 8) | lo

    def _narrow(self, lo, hi, prec):
        span = self.span_m1 + 1
        a = (span * lo) >> prec
        b = ((span * hi) >> prec) - 1
        self.base = (self.base + a) & M32
        self.span_m1 = (b - a) & M32
        if self.span_m1 >> 16 == 0:
            self.base = (self.base << 16) & M32
            self.span_m1 = ((self.span_m1 << 16) | 0xFFFF) & M32
            self.window = ((self.window << 16) | self._digit()) & M32

    def symbol(self, cdf, prec):
        span = self.span_m1 + 1
        target = (((self.window - self.base) & M32) + 1) << prec
        sym = len(cdf) - 2                                        # damaged input: the last symbol
        for k in range(len(cdf) - 1):
            if target <= span * int(cdf[k + 1]):
                sym = k
                break
        self._narrow(int(cdf[sym]), int(cdf[sym + 1]), prec)
        return sym

    def bit(self):
        return self.symbol((0, 1, 2), 1)

    def value(self, sp, cdf):
        """One element of a row with header `sp` (negative: the last symbol is the escape)."""
        sym = self.symbol(cdf, abs(sp))
        if sp < 0 and sym == len(cdf) - 2:
            nb = 0
            while nb < 31 and self.bit() == 0:                    # bounded, as on the device
                nb += 1
            v = 1 << nb
            while nb > 0:
                nb -= 1
                v |= self.bit() << nb
            sym = -v if self.bit() else v + (len(cdf) - 2) - 1
        return sym

    def ok(self):
        """RangeDecoder::Finalize (range_coder.h:144-169)."""
        if 2 * self.pulls < len(self.data):
            return False
        top = (self.base + self.span_m1) & M32
        if self.base == 0 or top < self.base:
            return self.window == 0
        sh = 24 if ((self.base - 1) >> 24) < (top >> 24) else 16
        r = ((self.base - 1) >> sh) + 1
        return ((r << sh) & M32) == self.window


def context_decode(strings, psi, weights, num_scales, rows, cdf_offset, order=None, dtype=np.float64):
    """The decode loop: strings [B][Hl] of bytes, `rows` = [(precision header, cdf)] per table -> (y_hat, ok [B, Hl]).
    Network and range decoder alternate position by position in `order` (default: wavefront)."""
    weights = tuple(np.asarray(w, dtype) for w in weights)
    psi = np.asarray(psi, dtype)
    b, hl, wl, _ = psi.shape
    m = weights[0].shape[2]
    decoders = [[RowDecoder(strings[n][i]) for i in range(hl)] for n in range(b)]
    y_hat = np.zeros((b, hl, wl, m), dtype)
    for i, j in (order or wavefront_order(hl, wl)):
        out = network(context_at(y_hat, i, j, weights), psi[:, i, j], weights)
        idx = index_prepare(out[:, m:], num_scales)
        for n in range(b):
            for c in range(m):
                sp, cdf = rows[idx[n, c]]
                value = decoders[n][i].value(sp, cdf) + int(cdf_offset[idx[n, c]])
                y_hat[n, i, j, c] = dtype(value) + out[n, c]
    ok = np.array([[d.ok() for d in per_image] for per_image in decoders])
    return y_hat, ok


# -------------------------------------------------------------------------------------------------------------------
# shared inputs

# (B, Hl, Wl, M, H1, H2); P = 2M
GPU_SHAPES = [(1, 1, 1, 8, 26, 21), (1, 1, 4, 8, 26, 21), (2, 3, 2, 8, 26, 21), (3, 4, 7, 16, 53, 42),
              (1, 20, 52, 8, 26, 21), (1, 3, 7, 192, 640, 512)]
SEED = 2018
ESCAPE_VALUE = 300.0


def make_case(shape, num_scales=64, seed=SEED):
    """-> (y, psi float32 arrays, weights float32 tuple).  Weights come from a fixed seed; the last layer is scaled so
    that, teacher-forced on rint(y), the index half spreads over all tables (mean (num_scales - 1) / 2, standard
    deviation num_scales / 3) and the means have unit scale.  Every 17th element of y, sign alternating, is
    +-ESCAPE_VALUE: beyond every table but the widest ones, so the escape code is taken."""
    b, hl, wl, m, h1, h2 = shape
    p = 2 * m
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * m + 10 * hl + wl))
    y = rng.normal(0.0, 3.0, (b, hl, wl, m))
    flat = y.reshape(-1)
    hot = np.arange(1, flat.size, 17)
    flat[hot] = ESCAPE_VALUE * np.where(np.arange(hot.size) % 2 == 0, 1.0, -1.0)
    psi = rng.normal(0.0, 1.0, (b, hl, wl, p))

    def dense(k, n):
        return rng.normal(0.0, 1.0 / np.sqrt(k), (k, n))

    kernel = rng.normal(0.0, 1.0 / np.sqrt(12 * m), (5, 5, m, 2 * m))
    weights = [kernel, rng.normal(0, 0.1, 2 * m), dense(2 * m + p, h1), rng.normal(0, 0.1, h1), dense(h1, h2),
               rng.normal(0, 0.1, h2), dense(h2, 2 * m), np.zeros(2 * m)]
    mu, index = context_parameters(np.rint(y), psi, weights)
    weights[6][:, :m] /= max(mu.std(), 1e-6)
    weights[6][:, m:] *= (num_scales / 3.0) / max(index.std(), 1e-6)
    weights[7][m:] = (num_scales - 1) / 2.0 - index.mean() * (num_scales / 3.0) / max(index.std(), 1e-6)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return f32(y), f32(psi), tuple(f32(w) for w in weights)
