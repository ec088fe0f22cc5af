"""ECVQ on the device: `ecvq_assign` forward and forward + backward at evaluation size, N = 2^20 rows with
(D, K) in {(1, 256), (2, 1024), (16, 4096), (1024, 4096)}, and at a training batch, N = 4096, next to
`ecvq_assign_reference` (the chunked tensor-op composition) on the same device.

Every figure is device events around `reps` back-to-back calls after a warm-up of the same calls, reps sized for a
window of about `--window-ms`: the CALL time, kernel plus launch gap.  The forward's rate is 3 N K D flops per call
(subtract, multiply, add per element of the distance) against the FP32 vector peak of 157.3 TFLOP/s.  The reference is
timed on at most `--reference-rows` rows and scaled to N (it is linear in N by construction).
Writes the table to profiles/vecvq_table.md (or --out); profiles/vecvq_notes.md quotes it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FP32_TFLOPS = 157.3
SHAPES = [(1, 256), (2, 1024), (16, 4096), (1024, 4096)]


def timed(fn, window_ms):
    """Device ms per call."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(2, min(500, int(window_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--reference-rows", type=int, default=1 << 14)
    ap.add_argument("--rows", type=int, nargs="*", default=[1 << 20, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecvq_table.md"))
    args = ap.parse_args()
    import compression_amd as tfc

    lines = ["| N | D | K | forward ms | TFLOP/s | of FP32 peak | fwd+bwd ms | reference fwd ms | reference fwd+bwd ms |",
             "|---|---|---|---|---|---|---|---|---|"]
    gen = torch.Generator().manual_seed(0)
    for n in args.rows:
        for d, k in SHAPES:
            x = torch.randn(n, d, generator=gen).cuda()
            c = (x[torch.randint(n, (k,), generator=gen).cuda()] + 0.05 * torch.randn(k, d, generator=gen).cuda())
            c.requires_grad_(True)
            logits = torch.randn(k, generator=gen).cuda().requires_grad_(True)

            def step(fn, rows, backward):
                rates = torch.logsumexp(logits, 0) - logits
                _, rate, dist = fn(rows, c if backward else c.detach(), rates if backward else rates.detach(), 3.0)
                if backward:
                    c.grad = logits.grad = None
                    (rate + 3.0 * dist).mean().backward()

            fwd = timed(lambda: step(tfc.ecvq_assign, x, False), args.window_ms)
            both = timed(lambda: step(tfc.ecvq_assign, x, True), args.window_ms)
            m = min(n, args.reference_rows)
            ref_fwd = timed(lambda: step(tfc.ecvq_assign_reference, x[:m], False), args.window_ms) * n / m
            ref_both = timed(lambda: step(tfc.ecvq_assign_reference, x[:m], True), args.window_ms) * n / m
            tflops = 3.0 * n * k * d / (fwd * 1e-3) / 1e12
            lines.append(f"| {n} | {d} | {k} | {fwd:.3f} | {tflops:.1f} | {100 * tflops / PEAK_FP32_TFLOPS:.0f} % | "
                         f"{both:.3f} | {ref_fwd:.2f} | {ref_both:.2f} |")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
