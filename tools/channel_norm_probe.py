"""ChannelNorm kernels at HiFiC's two extreme shapes, bfloat16: [8*48*32, 960] (generator trunk for 8
images of 768x512) and [8*768*512, 60] (encoder head / decoder tail).  Forward plain / relu / residual and backward,
next to a device copy of the same tensor and the torch expression of the same formula.

What the figures are.  Every call takes the next of a ring of buffer sets (x, second input, output) that is larger than
the 256 MB Infinity Cache, so inputs AND outputs are cold.  The kernels are called through the C ABI with pointers
prepared in advance (no allocation, no tensor conversion per call); the copy is `Tensor.copy_` into the ring's output.
"us" is device events around `reps` back-to-back calls (reps sized so that the window is about 20 ms), so it is the CALL
time: kernel plus launch gap.  "host us" is the host clock over the same loop without a synchronise: where it is below
"us" the device, not the host's enqueue rate, set the pace.  TB/s is the algorithmic bytes (forward 2 tensors, 3 with a
residual; backward 3; copy 2) over "us".  A kernel's own time comes from a trace of this script:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/channel_norm_probe.py --shape 0 --calls copy,forward
    python tools/rocprof_summary.py DIR out.md "title"
Writes profiles/channel_norm_probe.md (or --out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(8 * 48 * 32, 960), (8 * 768 * 512, 60)]
CALLS = ["copy", "forward", "forward relu", "forward residual", "backward", "torch expression", "torch expression relu"]


def timed(fn, reps):
    """(device us per call, host us per call spent enqueuing)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / reps * 1e6
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_norm_probe.md"))
    ap.add_argument("--window-ms", type=float, default=20.0, help="timed window per figure")
    ap.add_argument("--shape", type=int, default=-1, help="index into the shapes; -1: both")
    ap.add_argument("--calls", default=",".join(CALLS))
    args = ap.parse_args()
    from compression_amd import _lib
    from compression_amd.layers import functional
    assert torch.cuda.is_available(), "needs the GPU"
    lib, stream = _lib.lib(), _lib.stream_ptr()
    wanted = [c.strip() for c in args.calls.split(",")]
    lines = ["| shape (bf16) | call | us | host us | reps | bytes | TB/s | x copy |", "|---|---|---|---|---|---|---|---|"]
    for index, (pixels, C) in enumerate(SHAPES):
        if args.shape not in (-1, index):
            continue
        one = pixels * C * 2
        sets = max(3, -(-(768 << 20) // (3 * one)))
        ring = [[torch.randn(pixels, C, device="cuda").bfloat16() for _ in range(2)] +
                [torch.empty(pixels, C, device="cuda", dtype=torch.bfloat16)] for _ in range(sets)]
        gamma = (0.5 + torch.rand(C)).cuda()
        beta = torch.randn(C).cuda()
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        gp, bp, dgp, dbp = (t.data_ptr() for t in (gamma, beta, dgamma, dbeta))
        ptrs = [tuple(t.data_ptr() for t in s) for s in ring]
        k = [0]

        def nxt(what=ptrs):
            k[0] += 1
            return what[k[0] % sets]

        def forward(relu, residual):
            x, r, y = nxt()
            _lib.check(lib.tfc_channel_norm_forward(x, gp, bp, r if residual else None, y, 1, pixels, C, 1e-3, relu, stream))

        def backward():
            x, g, dx = nxt()
            _lib.check(lib.tfc_channel_norm_backward(x, g, gp, bp, dx, dgp, dbp, 1, pixels, C, 1e-3, 1, stream))

        def copy():
            s = nxt(ring)
            s[2].copy_(s[0])
        calls = {
            "copy": (copy, 2),
            "forward": (lambda: forward(0, False), 2),
            "forward relu": (lambda: forward(1, False), 2),
            "forward residual": (lambda: forward(0, True), 3),
            "backward": (backward, 3),
            "torch expression": (lambda: functional.channel_norm_reference(nxt(ring)[0], gamma, beta), 2),
            "torch expression relu": (lambda: functional.channel_norm_reference(nxt(ring)[0], gamma, beta, relu=True), 2),
        }
        copy_us = None
        for name in CALLS:
            if name not in wanted:
                continue
            fn, tensors = calls[name]
            rough, _ = timed(fn, 10)
            reps = int(min(4000, max(10, args.window_ms * 1e3 / rough)))
            us, host = timed(fn, reps)
            if name == "copy":
                copy_us = us
            rel = f"{us / copy_us:.2f}" if copy_us else ""
            lines.append(f"| [{pixels}, {C}] | {name} | {us:.1f} | {host:.1f} | {reps} | {tensors * one / 1e6:.1f} MB | "
                         f"{tensors * one / us / 1e6:.2f} | {rel} |")
            print(lines[-1], flush=True)
        del ring, ptrs
        torch.cuda.empty_cache()
    text = "# ChannelNorm probe (tools/channel_norm_probe.py)\n\n" + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
