"""The integer hyper-synthesis transform of bjm2019 next to the float one of bmshj2018, at bmshj2018's benchmark shapes:
z 8 x 12 (a 768 x 512 image), batch 128, 192 filters; layers 5x5 up 2, 5x5 up 2, 3x3 up 1.

What is measured, in ONE process, the three candidates alternating over --rounds rounds:
  (a) the three integer layers (csrc/integer_conv.hip), int8 z in, uint8 indexes out, and each layer alone;
  (b) bmshj2018's `HyperSynthesisTransform` in float32 and (c) in bfloat16, under no_grad as decompress() runs it.

What the figures are.  Every call takes the next of a ring of input sets, so a call does not find its own input of the
call before in a cache (the sets are small beside the 256 MB Infinity Cache: they are L2-cold, not HBM-cold; the
weights, under 1 MB a layer, stay resident in every candidate, as they do in a model).  "us" is device events around
`reps` back-to-back calls (reps sized so that a window is about --window-ms), i.e. call time: kernels plus launch
gaps, warmed up first.  "TMAC/s" is the layer's multiply-adds (output pixels x Cout x Cin x kh kw / stride^2: the
structural zeros of the transposed direction are not counted) over that time.  Random data: int8 uniform over the whole
range, weights uniform; the float transform gets the same z as floats.
Before anything is timed, one image of the batch goes through `integer_conv2d_reference` and must give the same bytes.
Writes a markdown table to --out (default profiles/integer_probe.md) and prints it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH, ZH, ZW, FILTERS, NUM_SCALES = 128, 8, 12, 192, 64
RING = 4


def timed(fn, window_ms):
    """Device us per call."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(3, min(500, int(window_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integer_probe.md"))
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from compression_amd.models import bjm2019, bmshj2018
    from compression_amd.ops import integer_conv2d_reference
    torch.manual_seed(0)
    batch = args.batch
    integer = bjm2019.IntegerHyperSynthesisTransform(FILTERS, NUM_SCALES).cuda()
    with torch.no_grad():       # activations and indexes spread over their ranges instead of sitting at 0
        integer.layer_0.bias.uniform_(0.0, 1500.0)
        integer.layer_1.bias.uniform_(0.0, 1500.0)
        integer.layer_2.bias.uniform_(0.0, 300.0)
    integer.freeze()
    layers = (integer.layer_0, integer.layer_1, integer.layer_2)
    # float32 parameters either way: the compute dtype is the activations' (as the models run it)
    float_transform = bmshj2018.HyperSynthesisTransform(FILTERS).cuda()
    floats = {dtype: float_transform for dtype in (torch.float32, torch.bfloat16)}

    gen = torch.Generator(device="cuda").manual_seed(1)
    z_sets = [torch.randint(-128, 128, (batch, ZH, ZW, FILTERS), device="cuda", generator=gen).to(torch.int8)
              for _ in range(RING)]
    z_float = {dtype: [z.to(dtype) for z in z_sets] for dtype in floats}
    # each layer's own input, as the layer before produces it
    with torch.no_grad():
        in_1 = [integer.layer_0(z) for z in z_sets]
        in_2 = [integer.layer_1(u) for u in in_1]
        out = integer.layer_2(in_2[0])
    layer_inputs = (z_sets, in_1, in_2)

    # the kernel's bytes are the definition's, on one image of this very data
    x = z_sets[0][:1].cpu()
    for layer in layers:
        k, _, b, c = layer._packed_kernel(torch.device("cpu"))
        x = integer_conv2d_reference(x, k, b, c, layer.stride, layer.up, layer.out_max)
    assert torch.equal(x, out[:1].cpu()), "the kernel disagrees with the reference"
    spread = out.float()
    print(f"indexes: min {int(spread.min())} max {int(spread.max())} mean {float(spread.mean()):.1f}", flush=True)

    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % RING
        return turn[0]

    def run_integer():
        with torch.no_grad():
            return integer.layer_2(integer.layer_1(integer.layer_0(z_sets[nxt()])))

    def run_layer(i):
        def run():
            with torch.no_grad():
                return layers[i](layer_inputs[i][nxt()])
        return run

    def run_float(dtype):
        def run():
            with torch.no_grad():
                return floats[dtype](z_float[dtype][nxt()])
        return run

    candidates = [("integer, three layers", run_integer), ("integer layer_0 (5x5 up 2)", run_layer(0)),
                  ("integer layer_1 (5x5 up 2)", run_layer(1)), ("integer layer_2 (3x3 up 1)", run_layer(2)),
                  ("float32 HyperSynthesisTransform", run_float(torch.float32)),
                  ("bfloat16 HyperSynthesisTransform", run_float(torch.bfloat16))]
    pixels = [batch * ZH * ZW * 4, batch * ZH * ZW * 16, batch * ZH * ZW * 16]
    macs = [pixels[0] * FILTERS * FILTERS * 25 / 4, pixels[1] * FILTERS * FILTERS * 25 / 4,
            pixels[2] * FILTERS * FILTERS * 9]
    work = {"integer, three layers": sum(macs), "integer layer_0 (5x5 up 2)": macs[0],
            "integer layer_1 (5x5 up 2)": macs[1], "integer layer_2 (3x3 up 1)": macs[2],
            "float32 HyperSynthesisTransform": sum(macs), "bfloat16 HyperSynthesisTransform": sum(macs)}
    times = {name: [] for name, _ in candidates}
    for _ in range(args.rounds):
        for name, fn in candidates:
            times[name].append(timed(fn, args.window_ms))
    lines = [f"z {batch} x {ZH} x {ZW} x {FILTERS}, {args.rounds} alternating rounds, window {args.window_ms:.0f} ms", "",
             "| candidate | us per call, each round | median us | GMAC | TMAC/s (median) |", "|---|---|---|---|---|"]
    for name, _ in candidates:
        med = statistics.median(times[name])
        lines.append(f"| {name} | {', '.join(f'{t:.0f}' for t in times[name])} | {med:.0f} | {work[name] / 1e9:.1f} | "
                     f"{work[name] / med / 1e6:.1f} |")
    med = {name: statistics.median(t) for name, t in times.items()}
    lines += ["", f"integer / float32 = {med['integer, three layers'] / med['float32 HyperSynthesisTransform']:.2f}, "
                  f"integer / bfloat16 = {med['integer, three layers'] / med['bfloat16 HyperSynthesisTransform']:.2f} "
                  "(below 1: the integer transform is faster)"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
