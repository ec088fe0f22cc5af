"""Two independent CPU restatements of the run-length gamma / Rice format of tensorflow/compression
(cc/lib/bit_coder.cc, cc/kernels/run_length_kernels.cc, cc/kernels/run_length_gamma_kernels.cc), the checkers of
the GPU codec:

- BitWriter / BitReader and encode / decode: plain bit-by-bit code, the reference's loops and error order.
- encode_np: vectorised NumPy (per-symbol costs, cumsum, np.packbits(bitorder="little")), for long strings.
"""
import numpy as np

INT32_MIN = -(1 << 31)
OUT_OF_BITS = "Out of bits to read."
GAMMA_WIDTH = "Exceeded maximum gamma bit width."
PAST_END = "Decoded past end of tensor."


class BitWriter:
    def __init__(self):
        self.bits = []

    def write_bits(self, count, value):
        for k in range(count):
            self.bits.append((value >> k) & 1)

    def write_one_bit(self, bit):
        self.bits.append(1 if bit else 0)

    def write_gamma(self, value):
        assert value > 0
        w = int(value).bit_length()
        self.write_bits(w - 1, 0)
        self.write_bits(1, 1)
        self.write_bits(w - 1, value)

    def write_rice(self, value, parameter):
        assert value >= 0 and parameter >= 0
        self.write_bits(value >> parameter, 0)
        self.write_bits(1, 1)
        self.write_bits(parameter, value)

    def data(self):
        out = bytearray((len(self.bits) + 7) // 8)
        for i, b in enumerate(self.bits):
            out[i >> 3] |= b << (i & 7)
        return bytes(out)


class BitReader:
    def __init__(self, data):
        self.data = bytes(data)
        self.pos = 0
        self.end = 8 * len(self.data)

    def read_bits(self, count):
        if self.end - self.pos < count:
            raise ValueError(OUT_OF_BITS)
        v = 0
        for k in range(count):
            p = self.pos + k
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << k
        self.pos += count
        return v

    def _zeros(self):
        z = 0
        while not self.read_bits(1):
            z += 1
        return z

    def read_gamma(self):
        z = self._zeros()
        if z + 1 > 31:
            raise ValueError(GAMMA_WIDTH)
        return (1 << z) | self.read_bits(z)

    def read_rice(self, parameter):
        z = self._zeros()
        v = (z << parameter) | self.read_bits(parameter)
        if v > 0x7fffffff:      # the one deviation: the reference's int32 arithmetic is undefined here
            raise ValueError("Rice code value overflows int32")
        return v


def encode(data, run_length_code=-1, magnitude_code=-1, use_run_length_for_non_zeros=False):
    """RunLengthEncodeOp::Compute, statement by statement."""
    x = [int(v) for v in np.asarray(data, np.int64).reshape(-1)]
    enc = BitWriter()

    def write_rl(r):
        if run_length_code >= 0:
            enc.write_rice(r, run_length_code)
        else:
            enc.write_gamma(r + 1)

    def write_nz(s):
        sign = s > 0
        enc.write_one_bit(sign)
        if magnitude_code >= 0:
            enc.write_rice(s - 1 if sign else -(s + 1), magnitude_code)
        else:
            enc.write_gamma(0x7fffffff if s == INT32_MIN else abs(s))

    p, end, offset = 0, len(x), 0
    while p < end:
        q = p
        while q < end and x[q] == 0:
            q += 1
        write_rl(q - p - offset)
        p = q
        if p >= end:
            break
        if use_run_length_for_non_zeros:
            while q < end and x[q] != 0:
                q += 1
            write_rl(q - p - 1)
            while p < q:
                write_nz(x[p])
                p += 1
            offset = 1
        else:
            write_nz(x[p])
            p += 1
    return enc.data()


def gamma_encode(data):
    """RunLengthGammaEncodeOp::Compute (its own loop, not RunLengthEncode's)."""
    enc = BitWriter()
    zero_ct = 1
    for s in (int(v) for v in np.asarray(data, np.int64).reshape(-1)):
        if s == 0:
            zero_ct += 1
        else:
            enc.write_gamma(zero_ct)
            enc.write_one_bit(s > 0)
            if s == INT32_MIN:
                s += 1
            enc.write_gamma(abs(s))
            zero_ct = 1
    if zero_ct > 1:
        enc.write_gamma(zero_ct)
    return enc.data()


def decode(code, n, run_length_code=-1, magnitude_code=-1, use_run_length_for_non_zeros=False):
    """RunLengthDecodeOp::Compute; raises ValueError with the reference's text."""
    dec = BitReader(code)
    out = np.zeros(n, np.int64)

    def read_rl():
        if run_length_code >= 0:
            return dec.read_rice(run_length_code)
        return dec.read_gamma() - 1

    def read_nz():
        positive = dec.read_bits(1)
        if magnitude_code >= 0:
            r = dec.read_rice(magnitude_code)
            if positive and r == 0x7fffffff:
                raise ValueError("Rice code value overflows int32")
            return r + 1 if positive else -r - 1
        g = dec.read_gamma()
        return g if positive else -g

    p, offset = 0, 0
    while p < n:
        p += read_rl() + offset
        if p >= n:
            if p != n:
                raise ValueError(PAST_END)
            break
        if use_run_length_for_non_zeros:
            nxt = p + read_rl() + 1
            if nxt > n:
                raise ValueError(PAST_END)
            while p < nxt:
                out[p] = read_nz()
                p += 1
            offset = 1
        else:
            out[p] = read_nz()
            p += 1
    return out.astype(np.int32)


# ------------------------------------------------------------------------------------------------ vectorised


def _bw(v):
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for k in range(32):
        out += (v >> k) > 0
    return out


def _pieces(v, rice_k):
    """-> (zeros before the terminating 1, low-bit count) of each value's Rice / gamma code."""
    v = np.asarray(v, np.int64)
    if rice_k >= 0:
        return v >> rice_k, np.full(v.shape, rice_k, np.int64), v
    w = _bw(v)
    return w - 1, w - 1, v


def encode_np(data, run_length_code=-1, magnitude_code=-1, use_run_length_for_non_zeros=False):
    """Same bytes as encode(), from per-code lengths and one cumsum; scales to millions of symbols."""
    x = np.asarray(data, np.int64).reshape(-1)
    n = x.size
    if n == 0:
        return b""
    nzpos = np.flatnonzero(x)
    codes = []   # (order key, kind, value): kind 0 run-length code value, 1 sign bit, 2 magnitude value

    def rl_value(r):
        return r if run_length_code >= 0 else r + 1

    mag_k = magnitude_code
    if magnitude_code >= 0:
        magv = np.where(x[nzpos] > 0, x[nzpos] - 1, -(x[nzpos] + 1))
    else:
        magv = np.where(x[nzpos] == INT32_MIN, 0x7fffffff, np.abs(x[nzpos]))
    signs = (x[nzpos] > 0).astype(np.int64)
    prev = np.concatenate([[-1], nzpos[:-1]])
    keys, kinds, vals = [], [], []
    if not use_run_length_for_non_zeros:
        runs = nzpos - prev - 1
        for slot, kind, v in ((0, 0, rl_value(runs)), (1, 1, signs), (2, 2, magv)):
            keys.append(nzpos * 4 + slot)
            kinds.append(np.full(nzpos.size, kind))
            vals.append(v)
        trailing = n - 1 - (nzpos[-1] if nzpos.size else -1)
        tail_off = 0
    else:
        starts = nzpos[(prev != nzpos - 1) | (np.arange(nzpos.size) == 0)] if nzpos.size else nzpos
        is_start = np.isin(nzpos, starts)
        sidx = np.flatnonzero(is_start)
        ends = np.concatenate([sidx[1:], [nzpos.size]])
        lengths = ends - sidx
        zr = prev[sidx]
        zero_runs = starts - zr - 1 - np.where(np.arange(starts.size) == 0, 0, 1)
        for slot, v in ((0, rl_value(zero_runs)), (1, rl_value(lengths - 1))):
            keys.append(starts * 4 + slot)
            kinds.append(np.zeros(starts.size, np.int64))
            vals.append(v)
        keys += [nzpos * 4 + 2, nzpos * 4 + 3]
        kinds += [np.ones(nzpos.size, np.int64), np.full(nzpos.size, 2)]
        vals += [signs, magv]
        trailing = n - 1 - (nzpos[-1] if nzpos.size else -1)
        tail_off = 1 if nzpos.size else 0
    if trailing > 0:
        keys.append(np.array([4 * n]))
        kinds.append(np.array([0]))
        vals.append(np.array([rl_value(trailing - tail_off)]))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    kinds = np.concatenate(kinds)[order]
    vals = np.concatenate(vals)[order].astype(np.int64)
    zeros = np.zeros(vals.size, np.int64)
    lows = np.zeros(vals.size, np.int64)
    for kind, k in ((0, run_length_code), (2, mag_k)):
        m = kinds == kind
        z, lw, _ = _pieces(vals[m], k)
        zeros[m], lows[m] = z, lw
    sign = kinds == 1
    lengths = np.where(sign, 1, zeros + 1 + lows)
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total = int(lengths.sum())
    bits = np.zeros(total, np.uint8)
    bits[start[sign][vals[sign] == 1]] = 1
    code = ~sign
    one_at = start[code] + zeros[code]
    bits[one_at] = 1
    lw, v = lows[code], vals[code]
    for k in range(int(lw.max()) if lw.size else 0):
        m = (lw > k) & (((v >> k) & 1) == 1)
        bits[one_at[m] + 1 + k] = 1
    return np.packbits(bits, bitorder="little").tobytes()
