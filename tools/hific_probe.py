"""Per-layer times of one HiFiC compress + decompress at 1 x 768 x 512, bfloat16, reference sizes, random weights
(DESIGN.md §12): device events around every convolution, ChannelNorm and hyperprior layer (forward hooks), the second of
two runs.  Events between layers serialise nothing the model does not already serialise (one stream), but the sum of the
layers leaves out the entropy coder and the tensor ops between layers: the whole-call times are given next to it.
Writes profiles/hific_probe.md (or --out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hific_probe.md"))
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--width", type=int, default=512)
    args = ap.parse_args()
    import compression_amd as tfc
    from compression_amd import synthetic
    from compression_amd.models import hific
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    model = hific.HiFiCModel(compute_dtype=torch.bfloat16).cuda().init_compression()
    x = torch.from_numpy(synthetic.lowpass_images(1, args.height, args.width, seed=7)).cuda()
    kinds = (tfc.KerasConv2D, tfc.KerasConv2DTranspose, tfc.ChannelNorm, tfc.SignalConv2D)
    records = []

    def pre(mod, inp):
        mod._probe_start = torch.cuda.Event(enable_timing=True)
        mod._probe_start.record()

    def post(mod, inp, out):
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        records.append((mod._probe_name, type(mod).__name__, tuple(inp[0].shape), tuple(out.shape), mod._probe_start, end))
    for name, mod in model.named_modules():
        if isinstance(mod, kinds):
            mod._probe_name = name
            mod.register_forward_pre_hook(pre)
            mod.register_forward_hook(post)
    whole = {}
    for run in range(2):
        records.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.compress(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        split = len(records)
        x_hat = model.decompress(*out)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        whole = {"compress": (t1 - t0) * 1e3, "decompress": (t2 - t1) * 1e3}
    assert x_hat.shape == x.shape
    rows, norm_ms, conv_ms = [], 0.0, 0.0
    for i, (name, kind, si, so, a, b) in enumerate(records):
        ms = a.elapsed_time(b)
        if kind == "ChannelNorm":
            norm_ms += ms
        else:
            conv_ms += ms
        rows.append(f"| {'compress' if i < split else 'decompress'} | {name} | {kind} | {'x'.join(map(str, si))} | "
                    f"{'x'.join(map(str, so))} | {ms:.3f} |")
    nbytes = sum(len(s) for s in out[0]) + sum(len(s) for s in out[1])
    text = [f"# HiFiC probe (tools/hific_probe.py): 1 x {args.height} x {args.width}, bfloat16, random weights", "",
            f"compress {whole['compress']:.2f} ms, decompress {whole['decompress']:.2f} ms (host clock around a "
            f"synchronised call, second run); {nbytes} bytes of strings (random weights: no meaning as a rate).", "",
            f"Sum over the hooked layers: convolutions {conv_ms:.2f} ms, ChannelNorm {norm_ms:.2f} ms "
            f"({100 * norm_ms / max(conv_ms + norm_ms, 1e-9):.1f} % of the layers' time, "
            f"{sum(1 for r in records if r[1] == 'ChannelNorm')} launches).", "",
            "| call | layer | kind | input | output | ms |", "|---|---|---|---|---|---|"] + rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text[:5]))


if __name__ == "__main__":
    main()
