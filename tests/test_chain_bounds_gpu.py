"""GPU tier: the interval bounds of the hand-scheduled coder steps (csrc/range_pipe.h TFC_PENC_ROW / TFC_PENC_STEP_H /
TFC_PDEC_STEP / TFC_PDEC_STEP_H, csrc/range_lanes.h TFC_LENC_B / TFC_LDEC_STEP).  A step takes both bounds
(c (S + 1)) >> 16 as the upper dword of ONE 64-bit multiply-add whose operand and addend are c << 16 — the call word's
halves shifted / masked into place, cdf entries loaded into the upper half of a register whose lower half is zero, SDWA
selects into WORD_1.  What can go wrong there is aimed at here, at the smallest shapes that reach each kernel:
 * entries with bit 15 and low bits set (precision 15 on the 16-bit scale), the bottom symbol (lower bound 0) and the top
   symbol (upper bound 2^16, an entry stored as 0) in every stream's first call (S = 0xFFFFFFFF) and in long runs;
 * two-symbol rows of masses 2^-p and 1 - 2^-p (the unlikely symbol takes the span to the bottom of [2^16, 2^32), runs
   of the likely one keep it near the top), a row of 300 symbols, a row with an escape symbol and a few escape codes;
 * 33 symbols per stream (a block, a second block, the tail's single step); 64 streams (enc_chain_direct_kernel) and
   4096 streams = 64 groups (enc_chain_kernel beside the expansion); the decoder on the full and on the compact image,
   channel and index mode; the lane-per-stream kernels alone (TFC_PIPE=0, read once: a process of its own).
A hand-scheduled ENCODER block gives up, for its whole wave, as soon as one lane holds a digit 0xFFFF, and the block is then
repeated on the generic C++ path — which no counter shows.  So the inputs come in two kinds (bounds_values): `blocks`, on
which a CPU model of the coder's state (encoder_model, checked against the oracle's strings) says that no stream ever holds
such a digit, so that every block of every wave keeps its hand-scheduled result; and `runs`, with streams of nothing but top
symbols, which is the decoder's case.
Bytes must equal the oracle's (cc/kernels/range_coder_kernels.cc:191-322, cc/lib/range_coder.cc:37-307), the oracle's
bytes must decode to the input (range_coder_kernels.cc:360-471) with Finalize true — and the pipelined kernels must have
done it: tfc_pipe_counters shows a launch per call and no workgroup of the fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from compression_amd import synthetic
from test_pipe_compact_gpu import decode_oracle_strings, pipe_format
from test_pipe_fuzz_gpu import counters, dev

pytestmark = pytest.mark.gpu

ELEMS = 33


@pytest.fixture(scope="module")
def tfc():
    import compression_amd
    compression_amd.set_default_mode("throughput")
    yield compression_amd
    compression_amd.set_default_mode("auto")


def bounds_lookup(port, precision):
    """Four rows: (2^-p, 1 - 2^-p), (1 - 2^-p, 2^-p), 300 symbols of random masses, twenty symbols and an escape symbol."""
    top = 1 << precision
    rng = np.random.default_rng(precision)
    wide = (rng.random(300) + 1e-3).astype(np.float32)
    wide = np.asarray(port.pmf_to_quantized_cdf(wide / wide.sum(), precision), np.int32)
    esc = np.concatenate([0.8 ** np.arange(20), [0.02]]).astype(np.float32)
    esc = np.asarray(port.pmf_to_quantized_cdf(esc / esc.sum(), precision), np.int32)
    assert len(wide) == 301 and len(esc) == 22
    rows = [(precision, [0, 1, top]), (precision, [0, top - 1, top]), (precision, wide), (-precision, esc)]
    return np.concatenate([np.concatenate([[sp], cdf]).astype(np.int32) for sp, cdf in rows])


def coder_calls(lookup, value, index):
    """The coder calls of every stream, in order, on the 16-bit scale the kernels use: (lo, hi, act), each
    [streams, calls] with `act` false behind a stream's last call.  A plain symbol is one call on its row's interval; a
    value outside an escape row's range is the escape symbol's call, then the Elias-gamma code of its excess — floor(log2 g)
    zeros, the bits of g — and the sign, each a call on one half of the unit interval (range_coder_kernels.cc:304-321)."""
    rows = synthetic.lookup_rows(lookup)
    streams, elems = value.shape
    tab = np.broadcast_to(np.arange(elems) % len(rows), value.shape) if index is None else index
    lo = np.zeros(value.shape, np.int64)
    hi = np.zeros(value.shape, np.int64)
    plain = np.zeros(value.shape, bool)
    for t, (sp, cdf) in enumerate(rows):
        c16 = np.asarray(cdf, np.int64) << (16 - abs(sp))
        limit = len(cdf) - 2 if sp < 0 else len(cdf) - 1
        m = tab == t
        ok = m & (value >= 0) & (value < limit)
        assert sp < 0 or (ok == m).all(), "a value outside a row without an escape symbol"
        sym = np.where(ok, value, limit)[m]
        lo[m], hi[m], plain[m] = c16[sym], c16[sym + 1], ok[m]
    extra = {}
    for s, e in zip(*np.nonzero(~plain)):
        sp, cdf = rows[tab[s, e]]
        v, limit = int(value[s, e]), len(cdf) - 2
        g = -v if v < 0 else v - limit + 1
        n = g.bit_length() - 1
        extra[(s, e)] = [(g >> k) & 1 for k in range(2 * n, -1, -1)] + [1 if v < 0 else 0]
    width = elems + max([0] + [sum(len(b) for (s2, _), b in extra.items() if s2 == s) for s in {k[0] for k in extra}])
    LO, HI, ACT = (np.zeros((streams, width), np.int64), np.zeros((streams, width), np.int64), np.zeros((streams, width), bool))
    LO[:, :elems], HI[:, :elems], ACT[:, :elems] = lo, hi, True
    for s in sorted({k[0] for k in extra}):
        calls = []
        for e in range(elems):
            calls.append((lo[s, e], hi[s, e]))
            calls += [(b << 15, (b + 1) << 15) for b in extra.get((s, e), [])]
        LO[s, :len(calls)], HI[s, :len(calls)], ACT[s, :len(calls)] = [c[0] for c in calls], [c[1] for c in calls], True
    return LO, HI, ACT


def encoder_model(lo, hi, act):
    """The encoder's state, call by call, with the carry kept in the held digit (range_pipe.h TFC_PENC_STEP_H; the same
    digits in the same order as the reference's, cc/lib/range_coder.cc:37-264) -> (tripped, digits, count).
    `tripped[s]`: at some call stream s holds a digit 0xFFFF or more — a new digit 0xFFFF, or 0xFFFE with a carry.  That is
    when a hand-scheduled encoder block gives up: the WHOLE WAVE's block is then repeated call by call on the generic C++
    path (enc_chain_kernel `hd >= 0xFFFF`, enc_chain_direct_kernel and enc_lanes_kernel FLAG), which the fallback counter
    does not show.  `digits[s, :count[s]]`: the 16-bit digits stream s has emitted by its last call (until it trips)."""
    streams, width = lo.shape
    base, span = np.zeros(streams, np.int64), np.full(streams, 0xFFFFFFFF, np.int64)
    held, had, tripped = np.zeros(streams, np.int64), np.zeros(streams, bool), np.zeros(streams, bool)
    digits, count = np.zeros((streams, width), np.int64), np.zeros(streams, np.int64)
    for k in range(width):
        on = act[:, k] & ~tripped
        a = ((span + 1) * lo[:, k]) >> 16
        b = (((span + 1) * hi[:, k]) >> 16) - 1
        bs = base + a
        carry = on & (bs >> 32 != 0)
        bs &= 0xFFFFFFFF
        t1 = b - a
        ren = on & (t1 < 0x10000)
        assert not (carry & ~had).any()
        held = held + carry
        tripped |= (ren & (bs >> 16 == 0xFFFF)) | (on & had & (held >= 0xFFFF))
        out = np.flatnonzero(ren & had & ~tripped)
        digits[out, count[out]] = held[out]
        count[out] += 1
        held = np.where(ren, bs >> 16, held)
        had |= ren
        base = np.where(on, np.where(ren, (bs << 16) & 0xFFFFFFFF, bs), base)
        span = np.where(on, np.where(ren, ((t1 << 16) | 0xFFFF) & 0xFFFFFFFF, t1), span)
    return tripped, digits, count


def bounds_values(lookup, streams, indexed, seed, escapes=None, runs=False):
    """-> (value, index or None).  Every stream's first symbol is of a row without an escape symbol: the bottom one on even
    streams, the top one on odd streams.  Behind it, stream s by s % 4:
      `runs`      all bottom symbols / all top symbols / alternating / seeded random (drawn through the row's cdf).  A
                  stream of top symbols keeps base + span at 0xFFFFFFFF: every digit it shifts out is 0xFFFF, and every
                  encoder block of its wave is repeated on the generic path (encoder_model) — the decoder's case;
      otherwise   all bottom symbols / top symbols at every third element, random ones between / alternating / random —
                  and a stream that would ever hold a digit 0xFFFF is drawn again behind its first symbol until none
                  does: no wave leaves the hand-scheduled encoder blocks.
    The random streams have, where `escapes[s]`, up to three values outside the escape row's range (magnitudes below 64:
    far fewer coder calls than a launch plans rows for)."""
    rows = synthetic.lookup_rows(lookup)
    rng = np.random.default_rng(seed)
    if indexed:
        index = rng.integers(0, len(rows), (streams, ELEMS)).astype(np.int32)
        index[:, 0] = np.arange(streams) // 2 % 3
        tab = index
    else:
        index = None
        tab = np.broadcast_to(np.arange(ELEMS) % len(rows), (streams, ELEMS))
    if escapes is None:
        escapes = np.ones(streams, bool)
    nplain = np.array([len(c) - 2 if sp < 0 else len(c) - 1 for sp, c in rows])
    last = nplain[tab] - 1                                   # the top PLAIN symbol of every element's row
    kind = (np.arange(streams) % 4)[:, None]
    place = np.arange(ELEMS)[None, :]

    def draw():
        drawn = np.zeros((streams, ELEMS), np.int64)
        for t, (sp, cdf) in enumerate(rows):
            m = tab == t
            u = rng.integers(0, 1 << abs(sp), size=int(m.sum()))
            drawn[m] = np.minimum(np.searchsorted(np.asarray(cdf), u, side="right") - 1, nplain[t] - 1)
        return drawn

    first = np.where(np.arange(streams) % 2 == 0, 0, last[:, 0])

    def with_escapes(value, which):
        for s in which:
            if s % 4 != 3 or not escapes[s]:
                continue
            at = np.flatnonzero(tab[s] == 3)
            at = at[at > 0]
            for e in rng.permutation(at)[:3]:
                mag = int(rng.integers(1, 64))
                value[s, e] = nplain[3] + mag - 1 if rng.random() < 0.5 else -mag
        value[:, 0] = first
        return value

    drawn = draw()
    tops = last if runs else np.where(place % 3 == 0, last, drawn)
    value = np.where(kind == 0, 0, np.where(kind == 1, tops, np.where(kind == 2, place % 2 * last, drawn)))
    value = with_escapes(value, range(streams))
    again = np.arange(0 if runs else streams)
    for attempt in range(32):
        if again.size == 0:
            break
        sub = None if index is None else index[again]
        again = again[encoder_model(*coder_calls(lookup, value[again], sub))[0]]
        if attempt >= 8:
            first[again] = 0          # (a top symbol of small mass in front: most continuations shift 0xFFFF out)
        value[again] = draw()[again]
        value = with_escapes(value, again)
    assert again.size == 0
    return value.astype(np.int32), index


def strings_array(strings):
    arr = np.empty(len(strings), dtype=object)
    for i, x in enumerate(strings):
        arr[i] = x
    return arr


_REFERENCE = {}


def emitted(digits, count, s):
    return b"".join(int(d).to_bytes(2, "big") for d in digits[s, :count[s]])


def case(port, precision, streams, indexed, runs):
    """Lookup, input, the oracle's strings and the streams that trip an encoder block (encoder_model) of a case: computed
    once, shared, not written to."""
    key = (precision, streams, indexed, runs)
    if key not in _REFERENCE:
        lookup = bounds_lookup(port, precision)
        value, index = bounds_values(lookup, streams, indexed, seed=1000 * precision + streams + int(indexed), runs=runs)
        strings = port.encode(lookup, value, index=index, threads=4)[0]
        tripped, digits, count = encoder_model(*coder_calls(lookup, value, index))
        # the model is the reference's coder: what it has emitted by a stream's last call is how the oracle's string begins,
        # and Finalize adds at most the held digit and two more
        for s in np.flatnonzero(~tripped):
            head = emitted(digits, count, s)
            assert strings[s][:len(head)] == head and len(strings[s]) - len(head) <= 6, s
        for a in (lookup, value, tripped) + (() if index is None else (index,)):
            a.setflags(write=False)
        _REFERENCE[key] = (lookup, value, index, strings, tripped)
    return _REFERENCE[key]


@pytest.mark.parametrize("symbols", ["blocks", "runs"])
@pytest.mark.parametrize("indexed", [False, True], ids=["channel", "index"])
@pytest.mark.parametrize("streams", [64, 4096])
@pytest.mark.parametrize("precision", [12, 15])
def test_pipelined_chains_against_the_oracle(tfc, port, precision, streams, indexed, symbols):
    """`blocks`: no stream ever holds a digit 0xFFFF, so every encoder block of every wave keeps its hand-scheduled result —
    the first call, the steps behind it and the tail are held to the oracle through TFC_PENC_STEP / TFC_PENC_STEP_H.
    `runs`: streams of nothing but top symbols among the others — spans and offsets at the top of their range for the
    decoder's steps; the encoder repeats those waves' blocks on its generic path, its bytes are compared all the same."""
    lookup, value, index, want, tripped = case(port, precision, streams, indexed, symbols == "runs")
    lt = torch.from_numpy(lookup.copy())
    # the inputs are what the docstrings say they are
    rows = synthetic.lookup_rows(lookup)
    tab = np.broadcast_to(np.arange(ELEMS) % len(rows), value.shape) if index is None else index
    top = np.array([len(c) - 2 if sp < 0 else len(c) - 1 for sp, c in rows])[tab] - 1
    assert (tab[:, 0] < 3).all() and set(np.unique(value[0::2, 0])) == {0}
    assert (value[1::2, 0] == top[1::2, 0]).sum() >= streams // 4
    plain = np.ones(streams, bool)
    plain[3::4] = False
    assert not ((value[plain] < 0) | (value[plain] >= 300)).any() and (value[~plain] < 0).any()
    if symbols == "runs":
        assert all(tripped[w:w + 64].any() for w in range(0, streams, 64)) and (value[1::4] == top[1::4]).all()
    else:
        assert not tripped.any()
        assert ((value == top) & (tab < 3))[:, 1:].sum() >= 4 * streams and (value[:, 1:] == 0).sum() >= 4 * streams
    l0, f0 = counters()
    h = tfc.create_range_encoder([streams], lt)
    d_value, d_index = dev(value.copy()), None if index is None else dev(index.copy())      # (the shared arrays are read-only)
    h = tfc.entropy_encode_channel(h, d_value) if index is None else tfc.entropy_encode_index(h, d_index, d_value)
    got = [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)]
    l1, f1 = counters()
    bad = [s for s in range(streams) if got[s] != want[s]]
    assert not bad, (len(bad), bad[:8], got[bad[0]].hex(), want[bad[0]].hex())
    assert l1 - l0 >= 1 and f1 == f0, "the encode call did not run on the pipelined kernels alone"
    for fmt in (1, 2):
        l0, f0 = counters()
        with pipe_format(fmt):
            out, ok = decode_oracle_strings(tfc, lookup.copy(), want, ELEMS, None if index is None else index.copy())
        l1, f1 = counters()
        wrong = np.argwhere(out != value)
        assert wrong.size == 0, (fmt, len(wrong), wrong[:4], out[tuple(wrong[0])], value[tuple(wrong[0])])
        assert ok, fmt
        assert l1 - l0 >= 1 and f1 == f0, ("the decode call did not run on dec_chain_kernel alone", fmt)


# The lane-per-stream kernels alone: TFC_PIPE=0 is read once per process.  128 streams: the first wave's streams carry no
# escape codes and never hold a digit 0xFFFF (encoder_model) — every lane of it stays on the plain hand-scheduled blocks
# (TFC_LENC_BLOCK in channel mode; in index mode the lane encoder has no such block and only the decoder's TFC_LDEC_STEP is
# under test) — the second wave's streams have escape codes (the freezing blocks).  One case more with streams of nothing but
# top symbols, for the decoder.
_LANES_ALONE = """
import sys
import numpy as np
import torch
import compression_amd as tfc
sys.path.insert(0, sys.argv[2])
from test_pipe_fuzz_gpu import counters, dev
z = np.load(sys.argv[1], allow_pickle=True)
tfc.set_default_mode("throughput")
l0, f0 = counters()
for key in z["keys"]:
    lookup, value, strings = z[key + "_lookup"], z[key + "_value"], z[key + "_strings"]
    index = z[key + "_index"] if key + "_index" in z.files else None
    lt = torch.from_numpy(lookup)
    h = tfc.create_range_encoder([len(value)], lt)
    h = tfc.entropy_encode_channel(h, dev(value)) if index is None else tfc.entropy_encode_index(h, dev(index), dev(value))
    got = [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)]
    assert got == [bytes(x) for x in strings], key + ": bytes differ"
    hd = tfc.create_range_decoder(strings, lt)
    if index is None:
        hd, out = tfc.entropy_decode_channel(hd, [value.shape[1]], torch.int32)
    else:
        hd, out = tfc.entropy_decode_index(hd, dev(index), [value.shape[1]], torch.int32)
    assert np.array_equal(out.cpu().numpy().reshape(value.shape), value), key + ": symbols differ"
    assert bool(tfc.entropy_decode_finalize(hd).all()), key
l1, f1 = counters()
assert l1 == l0, "a pipelined kernel was launched"
print("LANES", len(z["keys"]))
"""


def test_lane_per_stream_kernels_against_the_oracle(port, tmp_path):
    arrays, keys = {}, []
    for precision, indexed, runs in [(12, False, False), (12, True, False), (15, False, False), (15, True, False),
                                    (15, False, True)]:
        lookup = bounds_lookup(port, precision)
        value, index = bounds_values(lookup, 128, indexed, seed=7 * precision + int(indexed),
                                     escapes=np.arange(128) >= 64, runs=runs)
        assert not ((value[:64] < 0) | (value[:64] > 300)).any() and (value[64:] < 0).any()
        assert encoder_model(*coder_calls(lookup, value, index))[0].any() == runs
        key = "p%d_%s%s" % (precision, "index" if indexed else "channel", "_runs" if runs else "")
        keys.append(key)
        arrays[key + "_lookup"], arrays[key + "_value"] = lookup, value
        arrays[key + "_strings"] = strings_array(port.encode(lookup, value, index=index)[0])
        if indexed:
            arrays[key + "_index"] = index
    np.savez(tmp_path / "cases.npz", keys=np.array(keys), **arrays)
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, TFC_PIPE="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _LANES_ALONE, str(tmp_path / "cases.npz"), here], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split()[-2:] == ["LANES", "5"]
