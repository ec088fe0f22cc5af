"""LPIPS on the device at the sizes HiFiC trains with: a sub-batch of 16 images of 256 x 256 (8 fake and 8
real through the trunk gives 16 trunk images; here the head is timed for 16 PAIRS, as `--batch` says).

  1. The distance head, forward and backward, at the five tap shapes, bfloat16 and float32, next to a device copy that
     moves the same bytes (forward: f0 + f1 read, so one tensor copied; backward: f0 + f1 read and df0 + df1 written,
     so both copied).
  2. The two max-pools, forward and backward, next to a copy of the input (forward) / of input and output (backward).
  3. `LPIPSLoss` forward + backward (gradient to `fake` only) next to the tensor-op composition on the same device:
     torch conv2d / max_pool2d on NCHW-shaped channels-last tensors and `lpips_distance_reference`.
Every figure is device events around `reps` back-to-back calls after a warm-up of the same calls, reps sized for a
window of about `--window-ms`: the CALL time, kernel plus launch gap.  The tap tensors of this size (0.5 - 8 MB) stay in
the 256 MB Infinity Cache between calls, for the copy as for the kernels.

`--profile-step [--no-lpips]`: warm up and run three `mselpips` generator steps (batch 8, 256 x 256, bfloat16), for
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lpips_probe.py --profile-step
`--share DIR_WITH DIR_WITHOUT`: the summed kernel time of the two traces and LPIPS's share, appended to --out.
Writes profiles/lpips_notes.md (or --out)."""
import argparse
import glob
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, window_ms):
    """Device us per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(5, min(2000, int(window_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def tap_shapes(size):
    o1 = (size - 7) // 4 + 1
    o2 = (o1 - 3) // 2 + 1
    o3 = (o2 - 3) // 2 + 1
    return [(o1, 64), (o2, 192), (o3, 384), (o3, 256), (o3, 256)], [(o1, 64), (o2, 192)]


def composition(weights, fake, real, functional):
    """LPIPS as torch's own convolution and pooling on the device, and the tensor-op distance."""
    n = fake.shape[0]
    x = torch.cat([fake, real], 0)
    x = ((2 * x.float() - 1 - weights["shift"]) / weights["scale"]).to(fake.dtype).permute(0, 3, 1, 2)
    total = 0
    for i, (name, stride, pad) in enumerate((("conv1", 4, 2), ("conv2", 1, 2), ("conv3", 1, 1), ("conv4", 1, 1),
                                             ("conv5", 1, 1))):
        x = torch.relu(torch.nn.functional.conv2d(x, weights[f"{name}_oihw"], weights[f"{name}_bias"].to(x.dtype),
                                                  stride=stride, padding=pad))
        t = x.permute(0, 2, 3, 1)
        total = total + functional.lpips_distance_reference(t[:n], t[n:].detach(), weights[f"lin{i}"])
        if i < 2:
            x = torch.nn.functional.max_pool2d(x, 3, 2)
    return total.mean()


def stats_total(directory):
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True))
    assert dbs, f"no *_results.db under {directory}"
    rows = list(sqlite3.connect(dbs[-1]).cursor().execute("select name, total_calls, total_duration from top_kernels"))
    return sum(float(r[2]) for r in rows), rows


def share(args):
    with_total, rows = stats_total(args.share[0])
    without_total, _ = stats_total(args.share[1])
    own = [(n, c, float(t)) for n, c, t in rows if "lpips" in n or "maxpool" in n]
    lines = ["", "## LPIPS's share of a `mselpips` generator step (rocprofv3 --kernel-trace --stats, three steps after warm-up"
             " and the warm-up itself, batch 8, 256 x 256, bfloat16)", "",
             f"* summed kernel time with `LPIPSLoss`: {with_total / 1e3:.2f} ms; without: {without_total / 1e3:.2f} ms; "
             f"LPIPS: {(with_total - without_total) / 1e3:.2f} ms = {100 * (with_total - without_total) / with_total:.1f} % "
             "of the kernel time of the run with it", "",
             "| LPIPS's own kernels | calls | total (us) |", "|---|---:|---:|"]
    lines += [f"| `{n[:100]}` | {c} | {t:.1f} |" for n, c, t in sorted(own, key=lambda r: -r[2])]
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def profile_step(args):
    import compression_amd as tfc
    from compression_amd import synthetic
    from compression_amd.models import hific, hific_train
    torch.manual_seed(0)
    model = hific.HiFiCModel(compute_dtype=torch.bfloat16).cuda()
    loss = None if args.no_lpips else tfc.LPIPSLoss(tfc.LPIPS.with_random_weights(0).cuda())
    trainer = hific_train.HiFiCTrainer(model, None, hific_train.CONFIGS["mselpips"], ignore_schedules=True,
                                       perceptual_loss=loss)
    x = torch.from_numpy(synthetic.lowpass_images(8, 256, 256, seed=1)).cuda().float()
    for _ in range(5):
        out = trainer.train_step([x])
    torch.cuda.synchronize()
    print({k: float(v) for k, v in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_notes.md"))
    ap.add_argument("--batch", type=int, default=16, help="image pairs")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--profile-step", action="store_true")
    ap.add_argument("--no-lpips", action="store_true")
    ap.add_argument("--share", nargs=2, metavar="DIR")
    args = ap.parse_args()
    if args.share:
        return share(args)
    assert torch.cuda.is_available(), "needs the GPU"
    if args.profile_step:
        return profile_step(args)
    import compression_amd as tfc
    from compression_amd import _lib
    from compression_amd.layers import functional
    lib, stream = _lib.lib(), _lib.stream_ptr()
    n, size = args.batch, args.size
    taps, pools = tap_shapes(size)
    lines = [f"# LPIPS on the device: {n} pairs of {size} x {size} (tools/lpips_probe.py)", "",
             "Call times (device events over back-to-back calls, kernel plus launch gap), us.", "",
             "## Distance head", "",
             "| tap [N, P, C] | dtype | forward | copy of f0 | forward / copy | backward (both) | backward (df0) | copy of f0, f1 | backward / copy |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|"]
    for side, c in taps:
        p = side * side
        for dtype, code in ((torch.bfloat16, 1), (torch.float32, 0)):
            f0 = torch.relu(torch.randn(n, p, c, device="cuda")).to(dtype)
            f1 = torch.relu(f0.float() * (1 + 0.1 * torch.randn(n, p, c, device="cuda"))).to(dtype)
            w = (torch.rand(c, device="cuda") / c).contiguous()
            d, g = torch.empty(n, device="cuda"), torch.randn(n, device="cuda")
            df0, df1 = torch.empty_like(f0), torch.empty_like(f1)

            def fwd():
                _lib.check(lib.tfc_lpips_distance_forward(f0.data_ptr(), f1.data_ptr(), w.data_ptr(), d.data_ptr(), code,
                                                          n, p, c, 1e-10, stream))

            def bwd(mask=3):
                _lib.check(lib.tfc_lpips_distance_backward(g.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(),
                                                           df0.data_ptr(), df1.data_ptr(), code, n, p, c, 1e-10, mask,
                                                           stream))

            def copy1():
                df0.copy_(f0)

            def copy2():
                df0.copy_(f0)
                df1.copy_(f1)
            t_f, t_c1 = timed(fwd, args.window_ms), timed(copy1, args.window_ms)
            t_b, t_b1, t_c2 = timed(bwd, args.window_ms), timed(lambda: bwd(1), args.window_ms), timed(copy2, args.window_ms)
            lines.append(f"| [{n}, {p}, {c}] | {str(dtype)[6:]} | {t_f:.1f} | {t_c1:.1f} | {t_f / t_c1:.2f} | {t_b:.1f} | "
                         f"{t_b1:.1f} | {t_c2:.1f} | {t_b / t_c2:.2f} |")
    lines += ["", "## Max-pool 3 x 3 stride 2 (the trunk's batch is 2 N)", "",
              "| x [N, H, W, C] | dtype | forward | copy of x | backward | copy of x and dy | torch max_pool2d fwd | torch fwd + bwd |",
              "|---|---|---:|---:|---:|---:|---:|---:|"]
    for side, c in pools:
        for dtype in (torch.bfloat16, torch.float32):
            x = torch.relu(torch.randn(2 * n, side, side, c, device="cuda")).to(dtype)
            y = functional.max_pool2d(x, 3, 2)
            gy, dx, y2 = torch.randn_like(y), torch.empty_like(x), torch.empty_like(y)
            code = 1 if dtype == torch.bfloat16 else 0
            args_f = (x.data_ptr(), y.data_ptr(), code, 2 * n, side, side, c, 3, 2, stream)
            args_b = (x.data_ptr(), gy.data_ptr(), dx.data_ptr(), code, 2 * n, side, side, c, 3, 2, stream)
            xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)      # channels-last NCHW view
            gt = gy.permute(0, 3, 1, 2)

            def torch_both():
                xt.grad = None
                torch.nn.functional.max_pool2d(xt, 3, 2).backward(gt)

            def copy2():
                dx.copy_(x)
                y2.copy_(gy)
            row = [timed(lambda: _lib.check(lib.tfc_maxpool2d_forward(*args_f)), args.window_ms),
                   timed(lambda: dx.copy_(x), args.window_ms),
                   timed(lambda: _lib.check(lib.tfc_maxpool2d_backward(*args_b)), args.window_ms),
                   timed(copy2, args.window_ms),
                   timed(lambda: torch.nn.functional.max_pool2d(xt.detach(), 3, 2), args.window_ms),
                   timed(torch_both, args.window_ms)]
            lines.append(f"| [{2 * n}, {side}, {side}, {c}] | {str(dtype)[6:]} | " + " | ".join(f"{v:.1f}" for v in row) + " |")
    lines += ["", "## `LPIPSLoss` forward + backward (gradient to `fake`), ms", "",
              "| dtype | this library | torch conv2d / max_pool2d + tensor-op distance | ratio |", "|---|---:|---:|---:|"]
    net = tfc.LPIPS.with_random_weights(0).cuda()
    loss = tfc.LPIPSLoss(net)
    weights = {k: v for k, v in net.state_dict().items()}
    for dtype in (torch.bfloat16, torch.float32):
        for name in ("conv1", "conv2", "conv3", "conv4", "conv5"):
            weights[f"{name}_oihw"] = weights[f"{name}_kernel"].permute(3, 2, 0, 1).to(dtype).contiguous(
                memory_format=torch.channels_last)
        real = torch.rand(n, size, size, 3, device="cuda").to(dtype)
        fake = (real.float() + 0.02 * torch.randn(real.shape, device="cuda")).clamp(0, 1).to(dtype)

        def ours():
            f = fake.detach().requires_grad_(True)
            loss(f, real).backward()

        def theirs():
            f = fake.detach().requires_grad_(True)
            composition(weights, f, real, functional).backward()
        t_o, t_t = timed(ours, 10 * args.window_ms), timed(theirs, 10 * args.window_ms)
        lines.append(f"| {str(dtype)[6:]} | {t_o / 1e3:.3f} | {t_t / 1e3:.3f} | {t_o / t_t:.2f} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
