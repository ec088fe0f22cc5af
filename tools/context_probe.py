"""Times the context model of ops/context_ops.py on the device: `context_scan`, `context_decode` and, as the yardstick,
`context_scan_reference` on device tensors (the host-driven loop: a handful of launches per latent position), on 1 and
16 images with a 32 x 48 x 192 latent (a 768 x 512 image).

    python tools/context_probe.py [--images 1 16] [--repeats 7] [--reference-repeats 1] [--json out.json]

Every shape is warmed up; a figure is the median of `--repeats` calls, each timed by a host clock around a call that
ends in a device synchronise.  The per-step split: a scan step is the network alone (its coding part is one rounding per
element), so the coder's share of a decode step is (decode - scan) / steps; cycles are at --clock-mhz.
Needs a GPU: there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def probe_inputs(latent, num_scales=64):
    """What the probes of both context models share: (normal, weights, model): the seeded float32 normal sampler
    `normal(scale, *shape)`, the eight weight tensors of a model with latent [Hl, Wl, M] drawn from it, and the
    coding_rank 2 entropy model of the y strings."""
    m = latent[2]
    h1, h2, p = 10 * m // 3, 8 * m // 3, 2 * m
    rng = np.random.Generator(np.random.PCG64(0))

    def normal(scale, *shape):
        return torch.from_numpy(rng.normal(0.0, scale, shape).astype(np.float32))

    w3 = normal(1 / math.sqrt(h2), h2, 2 * m)
    w3[:, m:] *= 8.0                                              # indexes that spread over the tables
    b3 = torch.cat([torch.zeros(m), torch.full((m,), 20.0)])
    weights = (normal(1 / math.sqrt(12 * m), 5, 5, m, 2 * m), normal(0.1, 2 * m),
               normal(1 / math.sqrt(2 * m + p), 2 * m + p, h1), normal(0.1, h1), normal(1 / math.sqrt(h1), h1, h2),
               normal(0.1, h2), w3, b3)
    return normal, weights, scale_model(num_scales, 2)


def scale_model(num_scales, coding_rank):
    from compression_amd import distributions, entropy_models
    offset = math.log(0.11)
    factor = (math.log(256.0) - offset) / (num_scales - 1.0)
    return entropy_models.LocationScaleIndexedEntropyModel(
        distributions.NoisyNormal, num_scales, lambda i: torch.exp(offset + factor * i), coding_rank=coding_rank,
        compression=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--latent", type=int, nargs=3, default=[32, 48, 192], metavar=("HL", "WL", "M"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--reference-repeats", type=int, default=1)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock that turns times into cycles "
                    "(the MI355X's peak; the runtime does not report the clock a kernel ran at)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("context_probe needs a GPU")

    from compression_amd.ops import context_ops, gen_ops

    hl, wl, m = args.latent
    p, num_scales = 2 * m, 64
    normal, weights, model = probe_inputs(args.latent, num_scales)
    params = context_ops.ContextParams(*weights, num_scales)
    per_image = scale_model(num_scales, 3)
    steps = (wl - 1) + 3 * (hl - 1) + 1
    clock_hz = args.clock_mhz * 1e6
    results = []
    for images in args.images:
        y = normal(3.0, images, hl, wl, m).cuda()
        psi = normal(1.0, images, hl, wl, p).cuda()
        scan = context_ops.context_scan(y, psi, params)
        host = model.compress((y - scan.mu).contiguous(), scan.index_float.contiguous())
        blob, offsets, shape = gen_ops.blob_from_strings(host)
        strings = (torch.from_numpy(blob).cuda(), torch.from_numpy(offsets).cuda(), shape)     # in HBM, as a codec keeps them
        y_hat, ok = context_ops.context_decode(strings, psi, params, model.cdf, model.cdf_offset)
        if not (bool(ok.all()) and torch.equal(y_hat, scan.y_hat)):
            raise SystemExit("context_decode does not invert the strings: nothing is timed")
        scan_ms = _median_ms(lambda: context_ops.context_scan(y, psi, params), args.repeats)
        decode_ms = _median_ms(lambda: context_ops.context_decode(strings, psi, params, model.cdf, model.cdf_offset),
                               args.repeats)
        loop_ms = _median_ms(lambda: context_ops.context_scan_reference(y, psi, params), args.reference_repeats,
                             warmup=1)
        network_us = scan_ms[0] * 1e3 / steps
        coder_us = (decode_ms[0] - scan_ms[0]) * 1e3 / steps
        bytes_total = int(offsets[-1])
        # the price of one stream per row: against the same symbols coded as one stream per image
        one = per_image.compress((y - scan.mu).contiguous(), scan.index_float.contiguous())
        row_overhead = (bytes_total - sum(len(s) for s in one.reshape(-1))) / (images * hl)
        row = dict(images=images, latent=[hl, wl, m], steps=steps, scan_ms=scan_ms[0], scan_ms_range=scan_ms[1:],
                   decode_ms=decode_ms[0], decode_ms_range=decode_ms[1:], host_loop_ms=loop_ms[0],
                   step_network_us=network_us, step_coder_us=coder_us,
                   step_network_cycles=network_us * 1e-6 * clock_hz, step_coder_cycles=coder_us * 1e-6 * clock_hz,
                   clock_mhz=clock_hz / 1e6, string_bytes=bytes_total,
                   row_overhead_bytes=row_overhead)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
