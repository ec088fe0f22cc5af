#!/usr/bin/env python
"""Times the run-length codec (PowerLawEntropyModel's RunLengthGammaEncode/Decode) on three workloads from a fixed
seed, with device events: A = [128, 48, 32, 192] at coding_rank 3 (128 strings of 294 912 symbols), B = the same
tensor at coding_rank 1 (196 608 strings of 192 symbols), C = coding_rank 0 on 4 M symbols.  The symbols are a
symmetric discrete Laplace with about 70 % zeros.  Prints one JSON line per workload (ms per call, bits per symbol,
bytes moved over 8 TB/s) and the decoder families on A.
Usage: python tools/run_length_probe.py [--iters N] [--json out.json]
Profile: rocprofv3 --kernel-trace --stats -d DIR -- python tools/run_length_probe.py --iters 3"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import compression_amd as tfc  # noqa: E402
from compression_amd.ops import gen_ops  # noqa: E402

HBM = 8e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (128, 48, 32, 192)
    u = (torch.rand(shape, generator=g, device="cuda") - 0.5).clamp(-0.4999, 0.4999)   # no log(0)
    lap = -torch.sign(u) * torch.log1p(-2 * u.abs()) * 0.415        # Laplace, scale 0.415 -> ~70 % round to 0
    x = torch.round(lap).int()
    n = x.numel()
    work = {"A": (x.reshape(128, -1), [48 * 32 * 192]), "B": (x.reshape(-1, 192), [192]),
            "C": (x.reshape(-1)[:1 << 22].reshape(-1, 1), [1])}
    rows = []
    for name, (units, ushape) in work.items():
        sym = units.numel()
        enc_ms, res = timed(lambda: gen_ops.run_length_encode_batched(units, device_result=True), args.iters)
        blob, offsets, sh = res
        code_bytes = blob.numel()
        dec_ms, dec = timed(lambda: gen_ops.run_length_decode_batched((blob, offsets, sh), ushape), args.iters)
        assert torch.equal(dec.reshape(units.shape), units), name
        row = {"workload": name, "strings": units.shape[0], "symbols": sym, "encode_ms": round(enc_ms, 4),
               "decode_ms": round(dec_ms, 4), "bits_per_symbol": round(8 * code_bytes / sym, 4),
               "zeros": round(float((units == 0).float().mean()), 4),
               "encode_hbm_ms": round((sym * 4 * 2 + code_bytes) / HBM * 1e3, 4),
               "decode_hbm_ms": round((sym * 4 + code_bytes) / HBM * 1e3, 4)}
        if name == "A":
            fam = {}
            for f in ("lane", "chunk"):
                os.environ["TFC_RL_DECODER"] = f
                fam[f], _ = timed(lambda: gen_ops.run_length_decode_batched((blob, offsets, sh), ushape), args.iters)
            os.environ.pop("TFC_RL_DECODER")
            row["decode_lane_ms"] = round(fam["lane"], 4)
            row["decode_chunk_ms"] = round(fam["chunk"], 4)
            row["chunk_speedup"] = round(fam["lane"] / fam["chunk"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    del n


if __name__ == "__main__":
    main()
