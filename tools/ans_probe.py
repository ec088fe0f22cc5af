#!/usr/bin/env python
"""Kernel times of the interleaved rANS coder (csrc/ans_coder.hip) next to the range coder in latency mode (one wave per
stream), on the same tables and the same symbols, in one process:

    C2x1     one stream of 49 152 symbols, BASELINE config 2's 192 tables, channel mode, with their escapes
    C2x512   512 such streams
    IDXx1    one stream of 147 456 symbols in index mode over 64 scale tables (0.11 ... 256)

Every figure is the time between two HIP events the library records around the named kernel (tfc_profile_enable /
tfc_profile_query), one figure per repetition after a warm-up; the table gives the median and the spread (min ... max)
of the repetitions, taken alternately (range, ANS, range, ...).  Cycles per symbol are at the nominal 2.4 GHz.

    python tools/ans_probe.py [--reps 9] [--out notes.md]        (on a GPU machine)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compression_amd as tfc  # noqa: E402
from compression_amd import _lib, synthetic  # noqa: E402
from compression_amd.ops import ans_ops  # noqa: E402

GHZ = 2.4
RANGE_ENC = ("enc_kernel", "enc_expand", "enc_chain")
RANGE_DEC = ("dec_kernel", "dec_chain", "dec_parse", "dec_parse_next")


def query(names):
    total = 0.0
    for name in names:
        ms, n = C.c_double(), C.c_int64()
        _lib.lib().tfc_profile_query(name.encode(), C.byref(ms), C.byref(n))
        total += ms.value
    return total


def tables(device, num_tables, sigma0, octave, precision=12):
    pmfs, _ = synthetic.gaussian_pmfs(num_tables=num_tables, sigma0=sigma0, octave=octave)
    cdfs = [tfc.pmf_to_quantized_cdf(torch.from_numpy(p).to(device), precision).cpu().numpy() for p in pmfs]
    return synthetic.assemble_lookup(cdfs, precision, overflow=True)


def indexed_symbols(lookup, elems, seed):
    """(index, value) int32 [1, elems]: a table per element, the value drawn through that table's CDF (its escape
    interval kept: such a draw becomes the first value behind the table)."""
    rows = synthetic.lookup_rows(lookup)
    rng = np.random.Generator(np.random.PCG64(seed))
    index = rng.integers(0, len(rows), size=elems).astype(np.int32)
    value = np.zeros(elems, np.int32)
    for c, (sp, cdf) in enumerate(rows):
        at = np.flatnonzero(index == c)
        u = rng.integers(0, 1 << abs(sp), size=at.size, dtype=np.int64)
        value[at] = np.searchsorted(cdf, u, side="right") - 1
    return index[None], value[None]


def range_step(lookup_t, value_t, index_t):
    streams, elems = value_t.shape
    h = tfc.create_range_encoder([streams], lookup_t, mode="latency")
    h = tfc.entropy_encode_channel(h, value_t) if index_t is None else tfc.entropy_encode_index(h, index_t, value_t)
    blob, offs = tfc.gen_ops._finalize_device(h)
    d = tfc.create_range_decoder((blob, offs, (streams,)), lookup_t, mode="latency")
    if index_t is None:
        d, out = tfc.entropy_decode_channel(d, [elems], torch.int32)
    else:
        d, out = tfc.entropy_decode_index(d, index_t, [elems], torch.int32)
    ok = tfc.entropy_decode_finalize(d)
    return out, bool(ok.all()), int(offs[-1])


def ans_step(lookup_t, value_t, index_t, lanes):
    encoded = ans_ops.ans_encode(lookup_t, value_t, index_t, lanes)
    out, ok = ans_ops.ans_decode(encoded, lookup_t, tuple(value_t.shape), index_t, lanes)
    return out, bool(ok.all()) and not int(encoded.status.abs().sum()), int(encoded.offsets[-1])


def measure(label, lookup, value, index, reps, lanes=64):
    device = torch.device("cuda")
    lookup_t = torch.from_numpy(lookup)
    value_t = torch.from_numpy(value).to(device)
    index_t = None if index is None else torch.from_numpy(index).to(device)
    symbols = value.size
    per_stream = value.shape[1]
    times = {k: [] for k in ("range_enc", "range_dec", "ans_enc", "ans_dec")}
    size = {}
    for rep in range(reps + 1):                              # repetition 0 warms up
        _lib.lib().tfc_profile_enable(1)
        out, ok, size["range"] = range_step(lookup_t, value_t, index_t)
        torch.cuda.synchronize()
        assert ok and torch.equal(out, value_t)
        r_enc, r_dec = query(RANGE_ENC), query(RANGE_DEC)
        _lib.lib().tfc_profile_enable(1)
        out, ok, size["ans"] = ans_step(lookup_t, value_t, index_t, lanes)
        torch.cuda.synchronize()
        assert ok and torch.equal(out, value_t)
        a_enc, a_dec = query(("ans_encode",)), query(("ans_decode",))
        _lib.lib().tfc_profile_enable(0)
        if rep:
            for k, v in zip(times, (r_enc, r_dec, a_enc, a_dec)):
                times[k].append(v)
    rows = []
    for k, v in times.items():
        v = np.array(v)
        med = float(np.median(v))
        rows.append((k, med, float(v.min()), float(v.max()), med * 1e-3 * GHZ * 1e9 / per_stream))
    lines = [f"### {label}: {value.shape[0]} stream(s) x {per_stream} symbols, "
             f"{'index' if index is not None else 'channel'} mode, {reps} repetitions",
             "",
             f"bytes: range {size['range']}, ANS ({lanes} lanes) {size['ans']} "
             f"({8 * size['range'] / symbols:.3f} / {8 * size['ans'] / symbols:.3f} bits per symbol)",
             "",
             "| kernel | median ms | min ... max ms | cycles per symbol of a stream (2.4 GHz) |",
             "|---|---|---|---|"]
    for k, med, lo, hi, cyc in rows:
        lines.append(f"| {k} | {med:.4f} | {lo:.4f} ... {hi:.4f} | {cyc:.1f} |")
    lines.append("")
    print("\n".join(lines), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_device()
    device = torch.device("cuda")
    c2 = tables(device, 192, 0.25, 24.0)
    # the tables' own escapes: 2^-8 of the mass per row is its escape interval (about 0.4 % of the symbols)
    value = synthetic.sample_symbols(c2, 512, 49152, seed=0, escape_fraction=2.0 ** -8)
    scales = tables(device, 64, 0.11, 63.0 / np.log2(256.0 / 0.11))
    index, ivalue = indexed_symbols(scales, 147456, seed=1)
    out = []
    out += measure("C2x1", c2, value[:1].copy(), None, args.reps)
    out += measure("C2x512", c2, value, None, max(3, args.reps // 3))
    out += measure("IDXx1", scales, ivalue, index, args.reps)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
