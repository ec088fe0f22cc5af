"""Adaptive run-length Golomb-Rice coding of integer vectors (models/lvac/lvac.ipynb, "RLGR"): the code LVAC reports a
rate with when `use_rlgr` is set, one stream per channel.  Host code, as in the notebook: a bit-serial adaptive code
with a data-dependent state per symbol, run once per evaluation on a few thousand to a few million integers.

The stream is a sequence of bits, least significant first, in 32-bit little-endian words; the last word is cut to the
bytes it uses, after an end marker bit 1."""
from __future__ import annotations

import numpy as np

__all__ = ["rlgr", "irlgr"]

L = 4                   # fixed-point scale of the adaptive parameters
U0 = 3                  # k_P up after a zero in no-run mode
D0 = 1                  # k_P down after anything else
U1 = 2                  # k_P up after a complete run
QUOTIENT_MAX = 24       # a unary part this long announces a 31-bit literal
LITERAL_BITS = 31
MAX_ABS = (1 << 30) - 1
_FLUSH_BITS = 1 << 13


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.bits = 0

    def write(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.bits
        self.bits += n
        if self.bits >= _FLUSH_BITS:
            whole = self.bits // 8
            self.out += (self.acc & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
            self.acc >>= 8 * whole
            self.bits -= 8 * whole

    def write_unary(self, n):
        self.write(1 << n, n + 1)          # n zeros, then a one

    def finish(self):
        self.write(1, 1)
        n = (self.bits + 7) // 8
        self.out += self.acc.to_bytes(n, "little")
        return bytes(self.out)


class _BitReader:
    def __init__(self, source):
        self.source = bytes(source)
        self.at = 0
        self.acc = 0
        self.bits = 0

    def _fill(self, n):
        while self.bits < n:
            if self.at >= len(self.source):
                raise ValueError("irlgr: the stream ends before the requested number of symbols")
            chunk = self.source[self.at:self.at + 8]
            self.acc |= int.from_bytes(chunk, "little") << self.bits
            self.bits += 8 * len(chunk)
            self.at += len(chunk)

    def read(self, n):
        if n == 0:
            return 0
        self._fill(n)
        value = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.bits -= n
        return value

    def read_unary(self):
        zeros = 0
        while True:
            if self.acc == 0:
                zeros += self.bits
                self.bits = 0
                self._fill(1)
                continue
            low = (self.acc & -self.acc).bit_length() - 1
            self.acc >>= low + 1
            self.bits -= low + 1
            return zeros + low


def _adapt(k_p, k_rp, k, u, quotient):
    if quotient == 0:
        k_rp = max(0, k_rp - 2)
    elif quotient > 1:
        k_rp += quotient + 1
    if k == 0 and u == 0:
        k_p += U0
    else:
        k_p = max(0, k_p - D0)
    return k_p, k_rp


def rlgr(x):
    """x: integers with |x| <= 2^30 - 1 (any shape, read in C order) -> bytes."""
    x = np.ravel(np.asarray(x))
    if not np.issubdtype(x.dtype, np.integer):
        raise ValueError(f"rlgr codes integers, got {x.dtype}")
    x = x.astype(np.int64)
    if x.size and (x.max() > MAX_ABS or x.min() < -MAX_ABS):
        raise ValueError(f"rlgr: values must lie in [-(2^30 - 1), 2^30 - 1], got [{x.min()}, {x.max()}]")
    z = np.where(x < 0, -2 * x - 1, 2 * x)            # signed -> unsigned, 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...
    count = len(z)
    # next_nonzero[n]: the first index >= n with z != 0 (count if there is none)
    idx = np.where(z != 0, np.arange(count), count)
    next_nonzero = np.minimum.accumulate(idx[::-1])[::-1].tolist() + [count]
    z = z.tolist()

    sink = _BitWriter()
    k_p, k_rp = 0, 10 * L
    n = 0
    while n < count:
        k = k_p // L
        k_rp = min(k_rp, 31 * L)
        k_r = k_rp // L
        u = z[n]
        if k:
            span = min(1 << k, count - n)
            zeros = min(next_nonzero[n] - n, span)
            n += zeros
            if zeros == span:                        # a complete run (the last one may be cut by the end)
                sink.write(0, 1)
                k_p += U1
                continue
            sink.write(1, 1)
            sink.write(zeros, k)
            u = z[n] - 1
        quotient = u >> k_r
        if quotient < QUOTIENT_MAX:
            sink.write_unary(quotient)
            sink.write(u, k_r)
        else:
            sink.write_unary(QUOTIENT_MAX)
            sink.write(u, LITERAL_BITS)
        k_p, k_rp = _adapt(k_p, k_rp, k, u, quotient)
        n += 1
    return sink.finish()


def irlgr(source, n):
    """The first n integers of an `rlgr` stream -> int32 [n]."""
    count = int(n)
    if count < 0:
        raise ValueError(f"irlgr: n must not be negative, got {n}")
    reader = _BitReader(source)
    out = np.zeros(count, np.int64)
    k_p, k_rp = 0, 10 * L
    at = 0
    while at < count:
        k = k_p // L
        k_rp = min(k_rp, 31 * L)
        k_r = k_rp // L
        if k:
            if reader.read(1) == 0:
                at += 1 << k
                k_p += U1
                continue
            at += reader.read(k)
            if at >= count:
                raise ValueError("irlgr: a run passes the requested number of symbols")
        quotient = reader.read_unary()
        if quotient < QUOTIENT_MAX:
            u = (quotient << k_r) + reader.read(k_r)
        else:
            u = reader.read(LITERAL_BITS)
            quotient = u >> k_r
        k_p, k_rp = _adapt(k_p, k_rp, k, u, quotient)
        out[at] = u if k == 0 else u + 1
        at += 1
    negative = out % 2 == 1
    return (((out + 1) // 2) * np.where(negative, -1, 1)).astype(np.int32)
