"""Rank-3 convolution kernels on the shapes of DESIGN.md §11 (P1-P4): bf16 forward of each, P1 in float32, and P1's
backward (dx, dw).  Kernel times come from the library's per-kernel events (tfc_profile_enable, "conv3d"); torch's
F.conv3d / F.conv1d on the same tensors are timed as context.  Writes profiles/conv3d_probe.md (or --out)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK = 2.5e15       # bf16 dense, MI355X

SHAPES = {  # name: (input [n, d, h, w, c], cout, support, strides, up)
    "P1": ((4, 8, 128, 128, 128), 128, (3, 5, 5), (1, 2, 2), False),
    "P2": ((4, 8, 64, 64, 128), 128, (3, 5, 5), (1, 2, 2), True),
    "P3": ((2, 16, 64, 64, 192), 192, (3, 3, 3), (2, 2, 2), False),
    "P4": ((32, 1, 1, 65536, 128), 128, (1, 1, 9), (1, 1, 4), False),
}


def useful_flop(shape, cout, k, s, up):
    n, d, h, w, c = shape
    pix = n * d * h * w if up else n * -(-d // s[0]) * -(-h // s[1]) * -(-w // s[2])
    return 2 * pix * c * cout * k[0] * k[1] * k[2]


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3d_probe.md"))
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from compression_amd.layers import functional
    torch.manual_seed(0)
    rows = []

    def run(name, dtype, shape, cout, k, s, up, backward=False):
        x = torch.randn(shape, device="cuda").to(dtype)
        w = torch.randn(k + (shape[-1], cout), device="cuda") / (k[0] * k[1] * k[2] * shape[-1]) ** 0.5
        fn = functional.conv3d_up if up else functional.conv3d_down
        flop = useful_flop(shape, cout, k, s, up)
        if not backward:
            ms = timed(lambda: fn(x, w, None, s), args.reps)
            what = "forward"
        else:
            y = fn(x, w, None, s)
            gy = torch.randn_like(y)
            ms_dx = timed(lambda: functional.conv3d_up(gy, w.transpose(3, 4), None, s), args.reps)
            ms_dw = timed(lambda: functional.conv3d_wgrad(x, gy, k, s, False), args.reps)
            rows.append((name, "dx", str(dtype).split(".")[-1], ms_dx, flop))
            ms, what = ms_dw, "dw"
        rows.append((name, what, str(dtype).split(".")[-1], ms, flop))
        if not args.no_torch and not backward and not up:
            xt = x.permute(0, 4, 1, 2, 3).contiguous()
            wt = w.to(dtype).permute(4, 3, 0, 1, 2).contiguous()
            pad = tuple(kk // 2 for kk in k)
            if shape[1] == 1 and shape[2] == 1:
                x1, w1 = xt[:, :, 0, 0], wt[:, :, 0, 0]
                ms_t = timed(lambda: F.conv1d(x1, w1, stride=s[2], padding=pad[2]), args.reps)
                rows.append((name, "torch F.conv1d (NCW)", str(dtype).split(".")[-1], ms_t, flop))
            else:
                ms_t = timed(lambda: F.conv3d(xt, wt, stride=s, padding=pad), args.reps)
                rows.append((name, "torch F.conv3d (NCDHW)", str(dtype).split(".")[-1], ms_t, flop))
        del x, w
        torch.cuda.empty_cache()

    for name, (shape, cout, k, s, up) in SHAPES.items():
        run(name, torch.bfloat16, shape, cout, k, s, up)
    shape, cout, k, s, up = SHAPES["P1"]
    run("P1", torch.float32, shape, cout, k, s, up)
    run("P1", torch.bfloat16, shape, cout, k, s, up, backward=True)
    lines = ["# conv3d probe (tools/conv3d_probe.py)", "",
             f"Device: {torch.cuda.get_device_name()}; {args.reps} timed calls after 2 warm-up calls, device events "
             "around the whole call (weight packing and, for float32, the plane split included).", "",
             "| shape | pass | dtype | ms | useful TFLOP/s | of 2.5 PF bf16 |", "|---|---|---|---|---|---|"]
    for name, what, dt, ms, flop in rows:
        tf = flop / (ms * 1e-3) / 1e12
        lines.append(f"| {name} | {what} | {dt} | {ms:.3f} | {tf:.1f} | {100 * tf * 1e12 / PEAK:.1f} % |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
