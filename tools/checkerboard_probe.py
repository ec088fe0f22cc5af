"""Times the checkerboard context model of ops/checkerboard_ops.py on the device beside the raster-order context model
of ops/context_ops.py: `checkerboard_scan` and `checkerboard_decode` next to `context_scan` and `context_decode`, on 1
and 16 images with a 32 x 48 x 192 latent (a 768 x 512 image), same weights' shapes, same inputs.

    python tools/checkerboard_probe.py [--images 1 16] [--repeats 7] [--json out.json]

Every shape is warmed up; a figure is the median of `--repeats` calls, each timed by a host clock around a call that
ends in a device synchronise.  `checkerboard_decode` includes the entropy model's two `decompress` calls per batch
(strings on the host, as a codec hands them over); `params_ms` is one launch of the parameter kernel for pass 1 alone
and `tflops` its float32 rate (2 flops per multiply-add of the definition).  Needs a GPU: there is no fallback."""
import argparse
import json
import sys

import numpy as np
import torch

from context_probe import _median_ms, probe_inputs          # (puts the repository on sys.path as well)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--latent", type=int, nargs=3, default=[32, 48, 192], metavar=("HL", "WL", "M"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-context", action="store_true", help="leave the raster-order model's two figures out")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("checkerboard_probe needs a GPU")

    from compression_amd.ops import checkerboard_ops, context_ops, gen_ops

    hl, wl, m = args.latent
    h1, h2, p, num_scales = 10 * m // 3, 8 * m // 3, 2 * m, 64
    normal, weights, model = probe_inputs(args.latent, num_scales)
    checker = checkerboard_ops.CheckerboardParams(*weights, num_scales)
    causal = context_ops.ContextParams(*weights, num_scales)
    macs = 2 * m * (12 * m) + (2 * m + p) * h1 + h1 * h2 + h2 * 2 * m            # per pass-1 position
    results = []
    for images in args.images:
        y = normal(3.0, images, hl, wl, m).cuda()
        psi = normal(1.0, images, hl, wl, p).cuda()
        scan = checkerboard_ops.checkerboard_scan(y, psi, checker)
        residual = checkerboard_ops.checkerboard_split((y - scan.mu).contiguous())
        index = checkerboard_ops.checkerboard_split(scan.index_float)
        strings = np.stack([np.asarray(model.compress(r, i), dtype=object).reshape(-1)
                            for r, i in zip(residual, index)], axis=1)
        y_hat = checkerboard_ops.checkerboard_decode(strings, psi, checker, model)
        if not torch.equal(y_hat, scan.y_hat):
            raise SystemExit("checkerboard_decode does not invert the strings: nothing is timed")
        scan_ms = _median_ms(lambda: checkerboard_ops.checkerboard_scan(y, psi, checker), args.repeats)
        decode_ms = _median_ms(lambda: checkerboard_ops.checkerboard_decode(strings, psi, checker, model), args.repeats)
        params_ms = _median_ms(lambda: checkerboard_ops.checkerboard_parameters(scan.y_hat, psi, checker, 1), args.repeats)
        n1 = checkerboard_ops.pass_positions(hl, wl, 1)
        row = dict(images=images, latent=[hl, wl, m], checkerboard_scan_ms=scan_ms[0], checkerboard_scan_ms_range=scan_ms[1:],
                   checkerboard_decode_ms=decode_ms[0], checkerboard_decode_ms_range=decode_ms[1:],
                   params_pass1_ms=params_ms[0], params_pass1_ms_range=params_ms[1:],
                   params_pass1_tflops=2.0 * macs * n1 * images / (params_ms[0] * 1e-3) / 1e12,
                   string_bytes=int(sum(len(s) for s in strings.reshape(-1))))
        if not args.skip_context:
            cscan = context_ops.context_scan(y, psi, causal)
            rows = model.compress((y - cscan.mu).contiguous(), cscan.index_float.contiguous())
            blob, offsets, shape = gen_ops.blob_from_strings(rows)
            held = (torch.from_numpy(blob).cuda(), torch.from_numpy(offsets).cuda(), shape)
            c_hat, ok = context_ops.context_decode(held, psi, causal, model.cdf, model.cdf_offset)
            if not (bool(ok.all()) and torch.equal(c_hat, cscan.y_hat)):
                raise SystemExit("context_decode does not invert the strings: nothing is timed")
            cs = _median_ms(lambda: context_ops.context_scan(y, psi, causal), args.repeats)
            cd = _median_ms(lambda: context_ops.context_decode(held, psi, causal, model.cdf, model.cdf_offset),
                            args.repeats)
            row.update(context_scan_ms=cs[0], context_scan_ms_range=cs[1:], context_decode_ms=cd[0],
                       context_decode_ms_range=cd[1:], context_string_bytes=int(offsets[-1]))
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
