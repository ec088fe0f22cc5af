"""HiFiC's discriminator pass and training step at the reference's sizes ("Discriminator and training
step"): bfloat16, sub-batches of 8 x 256 x 256, so the discriminator sees 16 x 256 x 256 x 15 and 16 x 16 x 16 x 220.

In one call, after warm-up, device events around synchronised work, the two variants alternating:
  D forward + backward (d_loss) with fused = True,
  D forward + backward with fused = False (the tensor-op composite around the same convolution kernels),
then the whole train_step, then the library's own per-kernel events (tfc_profile_enable) over one fused D pass and,
for the two elementwise kernels, a device copy of the same byte count timed in the same run.
Writes profiles/hific_gan_step.md (or --out).  `--profile-step`: only warm up and run two train_steps (what
`rocprofv3 --kernel-trace --stats -- python tools/hific_gan_step.py --profile-step` looks at)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

KERNELS = ["spectral_norm_forward", "spectral_norm_backward", "disc_front_forward", "disc_front_backward",
           "lrelu_forward", "lrelu_bias_backward", "gan_loss_forward", "gan_loss_backward", "conv2d", "conv2d_wgrad"]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hific_gan_step.md"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile-step", action="store_true")
    args = ap.parse_args()
    from compression_amd import _lib, synthetic
    from compression_amd.layers import gan_functional
    from compression_amd.models import hific, hific_train
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    dtype = torch.bfloat16
    model = hific.HiFiCModel(compute_dtype=dtype).cuda()
    disc = hific.Discriminator().cuda()
    trainer = hific_train.HiFiCTrainer(model, disc, hific_train.CONFIGS["hific"], ignore_schedules=True)
    xs = [torch.from_numpy(synthetic.lowpass_images(args.batch, args.size, args.size, seed=s)).cuda().float()
          for s in (1, 2)]
    for _ in range(2):
        trainer.train_step(xs)
    if args.profile_step:
        for _ in range(2):
            trainer.train_step(xs)
        torch.cuda.synchronize()
        return
    n = 2 * args.batch
    x = torch.rand(n, args.size, args.size, 3, device="cuda").to(dtype)
    latent = torch.round(torch.randn((n,) + hific.latent_size(args.size, args.size) + (220,), device="cuda")).to(dtype)

    def d_pass(fused):
        disc.fused = fused
        disc.zero_grad(set_to_none=True)
        _, logits = disc(x, latent)
        gan_functional.gan_losses(logits)[0].backward()
    for fused in (True, False, True, False):
        d_pass(fused)
    fused_ms, plain_ms = [], []
    for _ in range(args.reps):                                  # alternating
        fused_ms += timed(lambda: d_pass(True), 1)
        plain_ms += timed(lambda: d_pass(False), 1)
    disc.fused = True
    step_ms = timed(lambda: trainer.train_step(xs), args.reps)

    # the library's per-kernel events over one fused D pass
    lib = _lib.lib()
    lib.tfc_profile_enable(1)
    d_pass(True)
    torch.cuda.synchronize()
    kern = {}
    for name in KERNELS:
        ms, count = C.c_double(0), C.c_int64(0)
        lib.tfc_profile_query(name.encode(), C.byref(ms), C.byref(count))
        kern[name] = (ms.value, count.value)
    lib.tfc_profile_enable(0)

    # the front end and the first layer's leaky ReLU alone, next to a device copy of the same bytes
    P = disc.convs[0].padded_in_channels()
    lat12 = torch.randn(n, latent.shape[1], latent.shape[2], 12, device="cuda").to(dtype)
    act = torch.randn(n, args.size // 2, args.size // 2, 64, device="cuda").to(dtype)
    gy = torch.randn_like(act)
    front_out = gan_functional.disc_front_forward(x, lat12, P)
    cases = [
        ("disc_front_forward", lambda: gan_functional.disc_front_forward(x, lat12, P),
         x.numel() * 2 + lat12.numel() * 2 + front_out.numel() * 2),
        ("disc_front_backward", lambda: gan_functional.disc_front_backward(front_out, lat12, 3),
         n * args.size * args.size * 16 * 2 + x.numel() * 2 + 2 * lat12.numel() * 2),
        ("lrelu_forward", lambda: gan_functional.lrelu_(act), 2 * act.numel() * 2),
        ("lrelu_bias_backward", lambda: gan_functional.lrelu_bias_backward(gy, act), 3 * act.numel() * 2),
    ]
    rows = []
    for name, fn, nbytes in cases:
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for _ in range(3):
            fn()
            dst.copy_(src)
        k_ms = statistics.median(timed(fn, args.reps))
        c_ms = statistics.median(timed(lambda: dst.copy_(src), args.reps))
        rows.append((name, nbytes, k_ms, nbytes / k_ms / 1e6, c_ms, nbytes / c_ms / 1e6))

    med = statistics.median
    conv_ms = kern["conv2d"][0] + kern["conv2d_wgrad"][0]
    ours = sum(v[0] for k, v in kern.items() if not k.startswith("conv2d"))
    lines = [
        "# HiFiC discriminator pass and training step (`python tools/hific_gan_step.py`)", "",
        f"bfloat16, sub-batches of {args.batch} x {args.size} x {args.size}; D sees {n} x {args.size} x {args.size} x 15 and "
        f"{n} x {latent.shape[1]} x {latent.shape[2]} x 220.  Device events around synchronised work, {args.reps} repetitions, "
        "the two D variants alternating; median (min - max) ms.", "",
        "| what | ms |", "|---|---|",
        f"| D forward + backward, fused | {med(fused_ms):.3f} ({min(fused_ms):.3f} - {max(fused_ms):.3f}) |",
        f"| D forward + backward, tensor-op composite | {med(plain_ms):.3f} ({min(plain_ms):.3f} - {max(plain_ms):.3f}) |",
        f"| train_step (1 D step + 1 G step) | {med(step_ms):.3f} ({min(step_ms):.3f} - {max(step_ms):.3f}) |", "",
        "Per-kernel events of the library over one fused D pass (sum of the launches under each name):", "",
        "| entry | launches | ms |", "|---|---|---|"]
    lines += [f"| {name} | {count} | {ms:.3f} |" for name, (ms, count) in kern.items()]
    lines += ["", f"Convolution launches {conv_ms:.3f} ms, the new kernels {ours:.3f} ms: "
              f"{100 * ours / max(conv_ms + ours, 1e-9):.1f} % of the kernel time of the D pass is outside the convolutions "
              "(tensor ops between the launches — channel padding, crops, sigmoid, Adam — are in neither figure).", "",
              "The memory-bound kernels alone, with a device copy (read + write) of the same byte count from the same run:", "",
              "| kernel | bytes moved | ms | GB/s | copy ms | copy GB/s |", "|---|---|---|---|---|---|"]
    lines += [f"| {name} | {nbytes} | {k:.4f} | {kb:.0f} | {c:.4f} | {cb:.0f} |" for name, nbytes, k, kb, c, cb in rows]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
