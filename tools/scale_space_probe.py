"""`scale_space_predict` next to its tensor-op twin on the same device: forward, and forward + backward,
at the training size 8 x 256 x 256 x 3, and forward only at one padded 1080p frame 1 x 1088 x 1920 x 3.

What the figures are.  The two paths alternate (kernel, twin, kernel, twin ...), each figure is device events around
back-to-back calls sized so that a window holds at least --window-s seconds of work, after a warm-up, and the best of
the rounds is kept with the spread beside it.  "GB/s" is the ALGORITHMIC bytes over the time, computed from the shapes:

    forward    4 NHW (C read + 3 flow + C written) + 2 x 4 N (M + 1) HWC      (the volume is written once, read once)
    backward   4 NHW (C g + 3 flow + 3 gflow + C gx) + 4 x 8 NHWC corner reads + 8 x 8 NHWC bytes of 64-bit atomic adds
               + 3 x 8 N (M + 1) HWC                                           (integer planes zeroed, summed, read once)

The blur passes' halo re-reads and the row-blurred temporaries are not counted: the figure says how far the whole call
is from moving its own inputs and outputs once.  Per-kernel times come from a separate trace of this script:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/scale_space_probe.py --paths kernel --cases train
    python tools/rocprof_summary.py DIR out.md "title"
Writes profiles/scale_space_probe.md (or --out)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = [("train 8x256x256x3", (8, 256, 256, 3), True), ("1080p 1x1088x1920x3", (1, 1088, 1920, 3), False)]
M, SIGMA0 = 5, 1.5


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3            # us per call


def algorithmic_bytes(shape, backward):
    n, h, w, c = shape
    nhw = n * h * w
    fwd = 4 * nhw * (2 * c + 3) + 2 * 4 * nhw * (M + 1) * c
    if not backward:
        return fwd
    return fwd + 4 * nhw * (2 * c + 6) + 4 * 8 * nhw * c + 8 * 8 * nhw * c + 3 * 8 * nhw * (M + 1) * c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_space_probe.md"))
    ap.add_argument("--window-s", type=float, default=0.5, help="device seconds per timed window, at least")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--paths", default="kernel,twin")
    ap.add_argument("--cases", default="train,1080p", help="which sizes, by the first word of their labels")
    args = ap.parse_args()
    from compression_amd.ops import flow_ops
    assert torch.cuda.is_available(), "needs the GPU"
    paths = {"kernel": flow_ops.scale_space_predict, "twin": flow_ops.scale_space_predict_reference}
    wanted = [p.strip() for p in args.paths.split(",")]
    gen = torch.Generator().manual_seed(0)
    lines = ["| size | direction | path | us (best) | us (worst round) | reps | algorithmic MB | GB/s |",
             "|---|---|---|---|---|---|---|---|"]
    for label, shape, with_backward in CASES:
        if label.split()[0] not in args.cases.split(","):
            continue
        n, h, w, c = shape
        x = (torch.rand(shape, generator=gen) * 255.0).cuda().requires_grad_(True)
        flow = torch.cat([torch.rand((n, h, w, 2), generator=gen) * 24.0 - 12.0,
                          torch.rand((n, h, w, 1), generator=gen) * (M + 2.0) - 1.0], dim=-1).cuda().requires_grad_(True)
        g = torch.randn(shape, generator=gen).cuda()
        for direction in (["forward", "forward + backward"] if with_backward else ["forward"]):
            def call(fn, direction=direction):
                if direction == "forward":
                    with torch.no_grad():
                        fn(x, flow, M, SIGMA0)
                else:
                    torch.autograd.grad(fn(x, flow, M, SIGMA0), [x, flow], g)
            reps, results = {}, {p: [] for p in wanted}
            for p in wanted:                                  # warm-up, and the window's size
                for _ in range(3):
                    call(paths[p])
                torch.cuda.synchronize()
                rough = timed(lambda: call(paths[p]), 3)
                reps[p] = max(3, int(args.window_s * 1e6 / rough) + 1)
            for _ in range(args.rounds):                      # alternating
                for p in wanted:
                    results[p].append(timed(lambda: call(paths[p]), reps[p]))
            nbytes = algorithmic_bytes(shape, direction != "forward")
            for p in wanted:
                best, worst = min(results[p]), max(results[p])
                lines.append(f"| {label} | {direction} | {p} | {best:.1f} | {worst:.1f} | {reps[p]} | {nbytes / 1e6:.1f} | "
                             f"{nbytes / best / 1e3:.1f} |")
                print(lines[-1], flush=True)
        del x, flow, g
        torch.cuda.empty_cache()
    text = ("# scale_space_predict probe (tools/scale_space_probe.py)\n\n"
            f"num_levels = {M}, sigma0 = {SIGMA0}; windows of at least {args.window_s} s, {args.rounds} alternating rounds.\n\n"
            + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
