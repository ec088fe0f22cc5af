"""Interleaved rANS over the range coder's lookup tables: a second, opt-in stream format in which `lanes` coder states
code `lanes` consecutive elements of one stream in a step (csrc/ans_core.h, csrc/ans_coder.hip).
The bytes are this project's own, not the reference's; `lanes` is part of the format and the caller keeps it.

`ans_encode_reference` / `ans_decode_reference` are the definition in exact Python integers on the host; the kernels,
the serial host coder of csrc/ans_core.h and the recorded vectors of tests/golden/ans_vectors.npz are held to them.

The format.  A state x is a uint32 in [2^16, 2^32), renormalised in 16-bit words; a call is (start, freq, P):

    encode:  if x >= freq << (32 - P): emit x & 0xFFFF, x >>= 16;   then x = ((x // freq) << P) + x % freq + start
    decode:  slot = x & (2^P - 1), the symbol is the s with cdf[s] <= slot < cdf[s + 1];
             x = freq (x >> P) + slot - start;   if x < 2^16: x = x << 16 | next word

Element i (a table row and a value with the row's offset subtracted, as `entropy_encode_index` takes it) becomes one
call for its table symbol and, where it escapes (a row with a negative header, value < 0 or >= max_value), up to three
raw chunks (chunk, 1, bits): 6 bits `k | sign << 5` with k = bit_length(gamma) - 1, then the low min(k, 16) bits of
gamma - 2^k, then its high k - 16 bits.  Element i belongs to lane i mod W and round i div W; the decoder runs rounds
ascending, sub-steps 0..3, and inside a sub-step all lanes' calls, then the lanes that fell below 2^16 take the next
words in ascending lane order.  The encoder runs the exact reverse from x = 2^16 in every lane.  The string: the
min(N, W) final states (little-endian uint32, lane 0 first), then the words in reverse emission order."""
from __future__ import annotations

import bisect
import collections

import numpy as np
import torch

from .. import _lib

__all__ = ["AnsStrings", "ans_encode", "ans_decode", "strings_from_blob", "ans_encode_reference",
           "ans_decode_reference", "ans_ideal_bits", "ANS_CONSTANTS", "MAX_LANES"]

ANS_CONSTANTS = _lib.kernel_constants("ans_core.h", ("ANS",))
MAX_LANES = ANS_CONSTANTS["ANS_MAX_LANES"]
_LOW = ANS_CONSTANTS["ANS_STATE_LOW"]
STATUS_VALUE = ANS_CONSTANTS["ANS_STATUS_VALUE"]
STATUS_INDEX = ANS_CONSTANTS["ANS_STATUS_INDEX"]

# What `ans_encode` returns: string s is blob[offsets[s]:offsets[s + 1]]; `overflow` (one int32 on the device) is 0
# unless a stream outgrew its slab (an internal error); `status` (int32 [streams] on the device) is 0 for a good stream,
# bit 0: a value outside a row without escape, bit 1: an index outside the lookup.
AnsStrings = collections.namedtuple("AnsStrings", ["blob", "offsets", "overflow", "status"])


def _check_lanes(lanes):
    lanes = int(lanes)
    if not 1 <= lanes <= MAX_LANES or lanes & (lanes - 1):
        raise ValueError(f"lanes must be a power of two in [1, {MAX_LANES}], got {lanes}")
    return lanes


# ---------------------------------------------------------------------------------------------------------- definition
def _rows_of(lookup):
    """The rows of a lookup as the coder indexes them (range_coder_kernels.cc:106-164) -> list of int lists
    [header, cdf[0], ..., cdf[n] = 2^P]."""
    lookup = np.asarray(torch.as_tensor(lookup).cpu() if torch.is_tensor(lookup) else lookup)
    if lookup.ndim not in (1, 2):
        raise ValueError(f"`lookup` must be rank 1 or 2: {tuple(lookup.shape)}")
    rows = []
    for chunk in ([lookup] if lookup.ndim == 1 else list(lookup)):
        flat = [int(v) for v in chunk]
        p, end = 0, len(flat)
        while p != end:
            if end < p + 3:
                raise ValueError("CDF ended prematurely.")
            head = p
            prec = abs(flat[head])
            if not 1 <= prec < 17:
                raise ValueError(f"precision={prec} not in range [1, 17)")
            last = 1 << prec
            p += 1
            if flat[p] != 0:
                raise ValueError("CDF must start with 0.")
            while True:
                p += 1
                if p == end:
                    raise ValueError("CDF must end with 1 << precision.")
                if flat[p] < flat[p - 1]:
                    raise ValueError("CDF must be monotonically increasing.")
                if flat[p] == last:
                    break
            p += 1
            rows.append(flat[head:p])
            while p != end and flat[p] == last:
                p += 1
            if lookup.ndim == 2 and p != end:
                raise ValueError("CDF must end with 1 << precision.")
    return rows


def _calls_of(row, v):
    """Element -> list of (start, freq, P); ValueError for a value the row cannot code."""
    h = row[0]
    prec = abs(h)
    nsym = len(row) - 2
    max_value = nsym - 1
    calls = []
    sym = v
    if h < 0 and (v < 0 or v >= max_value):
        sign = int(v < 0)
        gamma = (-v if sign else v - max_value + 1) & 0xFFFFFFFF
        k = gamma.bit_length() - 1
        m = gamma - (1 << k)
        sym = max_value
        calls.append((k | sign << 5, 1, 6))
        if k > 0:
            calls.append((m & ((1 << min(k, 16)) - 1), 1, min(k, 16)))
        if k > 16:
            calls.append((m >> 16, 1, k - 16))
    elif not 0 <= v < nsym:
        raise ValueError(f"value={v} not in range [0, {nsym})")
    start, freq = row[1 + sym], row[2 + sym] - row[1 + sym]
    if freq <= 0:
        raise ValueError(f"value={v} has no width in its row")
    return [(start, freq, prec)] + calls


def _as_streams(a, name):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2:
        raise ValueError(f"`{name}` must be [streams, elems], received shape {tuple(a.shape)}")
    return a


def _element_rows(rows, index, s, n):
    if index is None:
        if n and not rows:
            raise ValueError("the lookup has no row")
        return [rows[i % len(rows)] for i in range(n)]
    out = []
    for i in index[s]:
        if not 0 <= int(i) < len(rows):
            raise ValueError(f"index={int(i)} not in range [0, {len(rows)})")
        out.append(rows[int(i)])
    return out


def ans_encode_reference(lookup, value, index=None, lanes=64):
    """The definition of the encoder, on the host.  value int [streams, elems] (or [elems]: one stream), offsets
    subtracted; index the same shape, or None for channel mode (element j takes row j mod rows) -> list of bytes."""
    lanes = _check_lanes(lanes)
    rows = _rows_of(lookup)
    value = _as_streams(value, "value")
    if index is not None:
        index = _as_streams(index, "index")
        if index.shape != value.shape:
            raise ValueError("`index` must have the shape of `value`")
    out = []
    for s in range(value.shape[0]):
        n = value.shape[1]
        erows = _element_rows(rows, index, s, n)
        calls = [_calls_of(erows[i], int(value[s, i])) for i in range(n)]
        used = min(n, lanes)
        x = [_LOW] * used
        words = []
        for r in range(-(-n // lanes) - 1, -1, -1):
            for t in range(3, -1, -1):
                for lane in range(min(lanes, n - r * lanes) - 1, -1, -1):
                    c = calls[r * lanes + lane]
                    if len(c) <= t:
                        continue
                    start, freq, prec = c[t]
                    xl = x[lane]
                    if xl >= freq << (32 - prec):
                        words.append(xl & 0xFFFF)
                        xl >>= 16
                    x[lane] = ((xl // freq) << prec) + xl % freq + start
        data = np.array(x, dtype="<u4").tobytes() + np.array(words[::-1], dtype="<u2").tobytes()
        out.append(data)
    return out


def ans_decode_reference(strings, lookup, shape, index=None, lanes=64):
    """The definition of the decoder, on the host.  strings: one bytes per stream; shape (streams, elems)
    -> (symbols int32 numpy [streams, elems], ok bool numpy [streams])."""
    lanes = _check_lanes(lanes)
    rows = _rows_of(lookup)
    streams, n = (int(s) for s in shape)
    strings = [bytes(s) for s in strings]
    if len(strings) != streams:
        raise ValueError(f"{streams} strings are needed, received {len(strings)}")
    if index is not None:
        index = _as_streams(index, "index")
        if index.shape != (streams, n):
            raise ValueError("`index` must have the shape (streams, elems)")
    out = np.zeros((streams, n), dtype=np.int32)
    oks = np.zeros(streams, dtype=bool)
    for s, data in enumerate(strings):
        if n == 0:
            oks[s] = len(data) == 0
            continue
        erows = _element_rows(rows, index, s, n)
        used = min(n, lanes)
        ok = len(data) >= 4 * used and (len(data) - 4 * used) % 2 == 0
        head = data[:4 * used].ljust(4 * used, b"\0")
        x = [int(v) for v in np.frombuffer(head, dtype="<u4")]
        rest = data[4 * used:]
        words = [int(v) for v in np.frombuffer(rest[:len(rest) // 2 * 2], dtype="<u2")]
        pos = 0
        missing = False

        def refill(lanes_now):
            nonlocal pos, missing
            for lane in lanes_now:
                if x[lane] < _LOW:
                    w = 0
                    if pos < len(words):
                        w = words[pos]
                    else:
                        missing = True
                    pos += 1
                    x[lane] = x[lane] << 16 | w

        def raw(lane, bits):
            slot = x[lane] & ((1 << bits) - 1)
            x[lane] >>= bits
            return slot

        for r in range(-(-n // lanes)):
            cnt = min(lanes, n - r * lanes)
            esc = []
            for lane in range(cnt):
                row = erows[r * lanes + lane]
                prec, nsym = abs(row[0]), len(row) - 2
                slot = x[lane] & ((1 << prec) - 1)
                sym = bisect.bisect_right(row, slot, 1) - 2     # the last s with cdf[s] <= slot
                start, freq = row[1 + sym], row[2 + sym] - row[1 + sym]
                x[lane] = freq * (x[lane] >> prec) + slot - start
                out[s, r * lanes + lane] = sym
                if row[0] < 0 and sym == nsym - 1:
                    esc.append(lane)
            refill(range(cnt))
            if not esc:
                continue
            heads = {lane: raw(lane, 6) for lane in esc}
            refill(esc)
            k = {lane: heads[lane] & 31 for lane in esc}
            m = {lane: 0 for lane in esc}
            low = [lane for lane in esc if k[lane] > 0]
            for lane in low:
                m[lane] = raw(lane, min(k[lane], 16))
            refill(low)
            high = [lane for lane in esc if k[lane] > 16]
            for lane in high:
                m[lane] |= raw(lane, k[lane] - 16) << 16
            refill(high)
            for lane in esc:
                gamma = (1 << k[lane]) + m[lane]
                max_value = len(erows[r * lanes + lane]) - 3
                v = -gamma if heads[lane] >> 5 else gamma + max_value - 1
                out[s, r * lanes + lane] = ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        oks[s] = ok and not missing and pos == len(words) and all(v == _LOW for v in x)
    return out, oks


def ans_ideal_bits(lookup, value, index=None):
    """sum of -log2(freq / 2^P) over all calls of each stream (float64 numpy [streams]): what the tables say the values
    cost, the length an ANS string is compared with."""
    rows = _rows_of(lookup)
    value = _as_streams(value, "value")
    if index is not None:
        index = _as_streams(index, "index")
    bits = np.zeros(value.shape[0])
    for s in range(value.shape[0]):
        erows = _element_rows(rows, index, s, value.shape[1])
        for i, row in enumerate(erows):
            for _, freq, prec in _calls_of(row, int(value[s, i])):
                bits[s] += prec - np.log2(freq)
    return bits


# -------------------------------------------------------------------------------------------------------------- device
def _tables(lookup):
    from . import gen_ops
    return gen_ops._tables_for(lookup)


def _index_on(index, shape, device):
    if index is None:
        return None
    index = torch.as_tensor(index)
    if tuple(index.shape) != tuple(shape):
        raise ValueError(f"`index` must have the shape {tuple(shape)}, received {tuple(index.shape)}")
    return index.to(device, torch.int32).contiguous()


def ans_encode(lookup, value, index=None, lanes=64):
    """value int32 [streams, elems] (the rows' offsets subtracted), index the same shape or None (channel mode: element
    j of a stream takes row j mod rows) -> AnsStrings(blob uint8 device, offsets int64 device [streams + 1], overflow,
    status).  One wave per stream; nothing is read back (`strings_from_blob` does that)."""
    device = _lib.require_device()
    lanes = _check_lanes(lanes)
    value = torch.as_tensor(value)
    if value.dim() != 2:
        raise ValueError(f"`value` must be [streams, elems], received shape {tuple(value.shape)}")
    streams, elems = (int(s) for s in value.shape)
    value = value.to(device, torch.int32).contiguous()
    index = _index_on(index, value.shape, device)
    tables = _tables(lookup)
    cap = _lib.lib().tfc_ans_blob_capacity(streams, elems, lanes)
    if cap < 0:
        raise ValueError(_lib.last_error())
    blob = torch.empty(max(int(cap), 1), dtype=torch.uint8, device=device)
    offsets = torch.empty(streams + 1, dtype=torch.int64, device=device)
    overflow = torch.empty(1, dtype=torch.int32, device=device)
    status = torch.zeros(max(streams, 1), dtype=torch.int32, device=device)[:streams]
    _lib.check(_lib.lib().tfc_ans_encode(
        tables.ptr, _lib.ptr(index), value.data_ptr(), streams, elems, lanes, blob.data_ptr(), offsets.data_ptr(),
        overflow.data_ptr(), status.data_ptr(), _lib.stream_ptr()))
    return AnsStrings(blob, offsets, overflow, status)


def strings_from_blob(encoded, check=True):
    """What `ans_encode` returned -> list of bytes (one host synchronisation).  With `check`, a stream whose status is
    not 0 raises ValueError, as the range path does for such a value or index."""
    off = encoded.offsets.cpu().numpy()
    data = encoded.blob[:int(off[-1])].cpu().numpy().tobytes()
    if int(encoded.overflow.item()):
        raise RuntimeError("internal error: an ANS stream outgrew its slab")
    if check:
        status = encoded.status.cpu().numpy()
        bad = np.flatnonzero(status)
        if bad.size:
            what = "index" if int(status[bad[0]]) & STATUS_INDEX else "value"
            raise ValueError(f"{what} not in range of its table (stream {int(bad[0])})")
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def ans_decode(strings, lookup, shape, index=None, lanes=64, stream_index=None):
    """The inverse of `ans_encode`: `strings` is a sequence of bytes or what `ans_encode` returned; `shape` = (streams,
    elems); `lanes` the encoder's.  `stream_index` (one int per string, no stream twice) names the stream each string
    is; None: all of them in order.  -> (symbols int32 device [streams, elems], ok uint8 device [strings]).  Whatever the
    bytes are the call returns and writes nothing but its outputs; `ok` is 1 only for a string that has its states, whose
    words were all consumed with none missing, and whose every state ended at 2^16."""
    device = _lib.require_device()
    lanes = _check_lanes(lanes)
    streams, elems = (int(s) for s in shape)
    index = _index_on(index, (streams, elems), device)
    tables = _tables(lookup)
    if isinstance(strings, AnsStrings) or (isinstance(strings, tuple) and len(strings) >= 2
                                           and isinstance(strings[0], torch.Tensor)):
        blob, offsets = strings[0].to(device).contiguous(), strings[1].to(device, torch.int64).contiguous()
        count = offsets.numel() - 1
    else:
        strings = [bytes(s) for s in strings]
        count = len(strings)
        off_h = np.zeros(count + 1, dtype=np.int64)
        np.cumsum([len(s) for s in strings], out=off_h[1:])
        blob_h = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
        blob = torch.from_numpy(blob_h).to(device)
        offsets = torch.from_numpy(off_h).to(device)
    if blob.numel() == 0:
        blob = torch.zeros(1, dtype=torch.uint8, device=device)
    index_d = None
    if stream_index is not None:
        index_d = torch.as_tensor(stream_index, dtype=torch.int64).reshape(-1)
        if index_d.numel() != count:
            raise ValueError(f"stream_index names {index_d.numel()} streams for {count} strings")
        if torch.unique(index_d).numel() != count:
            raise ValueError("stream_index names a stream more than once")
        index_d = index_d.to(device, torch.int32).contiguous()
    elif count != streams:
        raise ValueError(f"{streams} strings are needed, received {count}")
    out = torch.zeros(streams, elems, dtype=torch.int32, device=device)
    ok = torch.zeros(max(count, 1), dtype=torch.uint8, device=device)[:count]
    _lib.check(_lib.lib().tfc_ans_decode(
        tables.ptr, blob.data_ptr(), offsets.data_ptr(), _lib.ptr(index_d), count, _lib.ptr(index), streams, elems,
        lanes, out.data_ptr(), ok.data_ptr(), _lib.stream_ptr()))
    return out, ok
