#!/usr/bin/env python
"""Multiscale SSIM on the fused scale-pass kernels (csrc/ssim.hip) next to the op-by-op torch composition
(`ssim_multiscale_reference`, torch autograd) on the same tensors in the same process, the two alternated:

  * [16, 256, 256, 3] float32 — the tensor of the bls2017 training step of DESIGN.md §9;
  * [24, 512, 768, 3] uint8 — a Kodak-sized batch (forward), and the same batch in float32 (forward + backward).

"us" is device events around `reps` back-to-back calls (a window of about --window-ms), so it is the CALL time: every
launch of a call, the small torch ops on the [planes, 5] tensor and the gaps between them.  Each figure is taken
--rounds times, the calls alternated inside a round; the table gives the median and the minimum.  "kernels us" is the
library's own per-kernel events (tfc_profile_enable) summed over the launches of one call, taken in a separate loop.
"copy" is Tensor.copy_ of the two inputs.  Then one bls2017 training step (forward + backward + Adam) with
distortion="mse" and "ms-ssim".  Writes profiles/ssim_probe.md (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernel_us(fn, names, n=10):
    from compression_amd import _lib
    torch.cuda.synchronize()
    _lib.lib().tfc_profile_enable(1)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in names:
        ms, cnt = C.c_double(), C.c_int64()
        _lib.lib().tfc_profile_query(name.encode(), C.byref(ms), C.byref(cnt))
        out[name] = (ms.value * 1e3 / n, cnt.value // n)
    _lib.lib().tfc_profile_enable(0)
    return out


def scale_bytes(shape, itemsize):
    """(bytes of the two inputs, bytes of the four halved float32 pairs a fused forward writes and reads back once)."""
    b, h, w, c = shape
    read = 2 * b * h * w * c * itemsize
    written = 0
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        written += 2 * b * h * w * c * 4
    return read, written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_probe.md"))
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    from compression_amd import models, synthetic
    from compression_amd.ops import image_ops
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["| tensor | call | us median | us min | reps | kernels us (launches) | x copy |", "|---|---|---|---|---|---|---|"]
    notes = []

    def pair(batch, h, w, dtype):
        x = torch.from_numpy(synthetic.lowpass_images(8, h, w, seed=3)).repeat((batch + 7) // 8, 1, 1, 1)[:batch].cuda()
        y = (x.float() + 8.0 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1)))
        y = y.round().clamp(0, 255)
        return x.to(dtype).contiguous(), y.to(dtype).contiguous()

    for label, shape, dtype, backward in (("[16, 256, 256, 3] float32", (16, 256, 256), torch.float32, True),
                                          ("[24, 512, 768, 3] uint8", (24, 512, 768), torch.uint8, False),
                                          ("[24, 512, 768, 3] float32", (24, 512, 768), torch.float32, True)):
        x, y = pair(*shape, dtype)
        bx, by = torch.empty_like(x), torch.empty_like(y)
        yg = y.clone().requires_grad_(True) if backward else None

        def copy():
            bx.copy_(x)
            by.copy_(y)

        def fwd(fn):
            with torch.no_grad():
                return fn(x, y, 255)

        def fwd_bwd(fn):
            yg.grad = None
            (1.0 - fn(x, yg, 255)).mean().backward()

        def general(fn):
            """The same call on the kernels that read the tap count at run time (what any filter_size but 11 takes)."""
            def run():
                os.environ["TFC_SSIM_RUNTIME_TAPS"] = "1"
                try:
                    fn()
                finally:
                    os.environ["TFC_SSIM_RUNTIME_TAPS"] = "0"
            return run

        both = ("ssim_scale_forward", "ssim_scale_backward")
        calls = [("copy of both inputs", copy, None),
                 ("fused forward", lambda: fwd(image_ops.ssim_multiscale), both[:1]),
                 ("fused forward, run-time taps", general(lambda: fwd(image_ops.ssim_multiscale)), both[:1]),
                 ("op-by-op forward", lambda: fwd(image_ops.ssim_multiscale_reference), None)]
        if backward:
            calls += [("fused forward + backward", lambda: fwd_bwd(image_ops.ssim_multiscale), both),
                      ("fused forward + backward, run-time taps", general(lambda: fwd_bwd(image_ops.ssim_multiscale)), both),
                      ("op-by-op forward + backward", lambda: fwd_bwd(image_ops.ssim_multiscale_reference), None)]
        a = image_ops.ssim_multiscale(x, y, 255)
        b = image_ops.ssim_multiscale_reference(x, y, 255)
        notes.append(f"{label}: MS-SSIM {a.mean().item():.6f} fused, {b.mean().item():.6f} op-by-op "
                     f"(max difference {(a - b).abs().max().item():.2e})")
        reps = {}
        for name, fn, _ in calls:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[name] = int(min(2000, max(5, args.window_ms * 1e3 / timed(fn, 5))))
        samples = {name: [] for name, _, _ in calls}
        for _ in range(args.rounds):
            for name, fn, _ in calls:
                samples[name].append(timed(fn, reps[name]))
        copy_us = statistics.median(samples["copy of both inputs"])
        for name, fn, kernels in calls:
            ks = ""
            if kernels:
                got = kernel_us(fn, kernels)
                ks = " + ".join(f"{got[k][0]:.1f} ({got[k][1]})" for k in kernels)
            med, low = statistics.median(samples[name]), min(samples[name])
            lines.append(f"| {label} | {name} | {med:.1f} | {low:.1f} | {reps[name]} | {ks} | {med / copy_us:.2f} |")
            print(lines[-1], flush=True)
        read, written = scale_bytes(x.shape, x.element_size())
        notes.append(f"{label}: the fused forward reads {read / 1e6:.1f} MB of input, writes {written / 1e6:.1f} MB of "
                     f"halved pairs and reads them back once: {(read + 2 * written) / 1e6:.1f} MB per call; the copy "
                     f"moves {2 * read / 1e6:.1f} MB")
        del x, y, bx, by, yg
        torch.cuda.empty_cache()

    train = []
    if not args.no_train:
        for dtype in (torch.float32, torch.bfloat16):
            xs = torch.from_numpy(synthetic.lowpass_images(8, 256, 256, seed=3)).cuda().repeat(2, 1, 1, 1)
            steps = {}
            for distortion in ("mse", "ms-ssim"):
                torch.manual_seed(0)
                model = models.BLS2017Model(lmbda=0.01, num_filters=192, compute_dtype=dtype, distortion=distortion).cuda()
                with torch.no_grad():
                    model.synthesis_transform.layer_2.bias.fill_(0.5)       # mid-grey: every scale value positive
                model(xs)
                opt = torch.optim.Adam(model.parameters(), lr=1e-4)

                def step(model=model, opt=opt):
                    opt.zero_grad()
                    loss, _, _ = model(xs, training=True)
                    loss.backward()
                    opt.step()
                steps[distortion] = step
                for _ in range(3):
                    step()
            torch.cuda.synchronize()
            samples = {d: [] for d in steps}
            for _ in range(args.rounds):
                for d, step in steps.items():
                    t0 = time.perf_counter()
                    for _ in range(10):
                        step()
                    torch.cuda.synchronize()
                    samples[d].append((time.perf_counter() - t0) / 10 * 1e3)
            ks = kernel_us(steps["ms-ssim"], ("ssim_scale_forward", "ssim_scale_backward"), n=5)
            train.append(f"| bls2017 step 16 x 256 x 256, {str(dtype)[6:]} | " +
                         " | ".join(f"{statistics.median(samples[d]):.2f} ({min(samples[d]):.2f})" for d in steps) +
                         f" | {ks['ssim_scale_forward'][0] / 1e3:.3f} + {ks['ssim_scale_backward'][0] / 1e3:.3f} |")
            print(train[-1], flush=True)

    text = "# SSIM probe (tools/ssim_probe.py)\n\n" + "\n".join(lines) + "\n\n" + "\n".join(f"* {n}" for n in notes) + "\n"
    if train:
        text += ("\n## bls2017 training step (forward + backward + Adam), wall ms: median (min)\n\n"
                 "| step | mse | ms-ssim | SSIM kernels ms (forward + backward) |\n|---|---|---|---|\n" + "\n".join(train) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
