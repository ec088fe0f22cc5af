"""The training step of bench.py's `training_figures` (bls2017, 192 filters, 16 x 256x256, bfloat16) with
`torch.optim.Adam(model.parameters(), lr=1e-4)`, as bench.py constructs it, and with `KerasAdam`, in one process, the
two alternating; then the input pipeline: `PatchDataset(device=...)` against a host-side crop and upload of the same
plan.

What the figures are.  "step" is the host clock around `--steps` whole steps (zero_grad, forward, backward, optimiser)
that end in a device synchronise, per step; "optimiser" is the same around `--optimiser-steps` calls of `optimizer.step()` alone
on the gradients of one backward pass.  Each figure is the median of `--groups` such groups, taken in turns (torch,
Keras, torch, ...) after a warm-up of both; min and max are the spread.  "bytes" for the optimiser is 28 per
parameter (p, g, m, v read; p, m, v written).  The dataset figures are batches per second of 16 x 256x256 bfloat16
patches out of `--images` PNGs of 512 x 768, host clock around `--batches` batches and a final synchronise, best of three;
"host" crops the decoded uint8 images on the host per the same plan, stacks, uploads and casts.
Writes profiles/train_step_probe.md (or --out)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def group_ms(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count * 1e3


def figure(samples):
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_probe.md"))
    ap.add_argument("--steps", type=int, default=20, help="steps of one timed group")
    ap.add_argument("--optimiser-steps", type=int, default=1000, help="optimiser calls of one timed group")
    ap.add_argument("--groups", type=int, default=7, help="timed groups per optimiser")
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--num_filters", type=int, default=192)
    args = ap.parse_args()
    from compression_amd import KerasAdam, PatchDataset, models, synthetic
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda")
    x = torch.from_numpy(synthetic.lowpass_images(8, 256, 256, seed=3)).to(device).repeat(2, 1, 1, 1)
    runs = {}
    for name in ("torch", "keras"):
        torch.manual_seed(0)
        model = models.BLS2017Model(lmbda=0.01, num_filters=args.num_filters, compute_dtype=torch.bfloat16).to(device)
        model(x)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4) if name == "torch" else \
            KerasAdam(model.parameters(), lr=1e-4)

        def step(model=model, opt=opt):
            opt.zero_grad()
            loss, _, _ = model(x, training=True)
            loss.backward()
            opt.step()
            return loss
        runs[name] = (model, opt, step)
    for _, _, step in runs.values():
        for _ in range(3):
            step()
    whole = {name: [] for name in runs}
    alone = {name: [] for name in runs}
    for _ in range(args.groups):
        for name, (_, _, step) in runs.items():
            whole[name].append(group_ms(step, args.steps))
    for _ in range(args.groups):
        for name, (_, opt, _) in runs.items():
            alone[name].append(group_ms(opt.step, args.optimiser_steps))
    params = sum(p.numel() for p in runs["keras"][0].parameters())
    tensors = len(list(runs["keras"][0].parameters()))
    lines = ["# Training step probe (`tools/train_step_probe.py`)", "",
             f"bls2017, {args.num_filters} filters, 16 x 256x256, bfloat16; {params} parameters in {tensors} tensors; "
             f"median (min - max) of {args.groups} groups of {args.steps} steps ({args.optimiser_steps} optimiser calls), the "
             f"optimisers taking turns.", "",
             "| optimiser | step ms | optimiser alone ms | optimiser GB/s at 28 B / parameter |", "|---|---|---|---|"]
    for name, label in (("torch", "`torch.optim.Adam`"), ("keras", "`KerasAdam`")):
        w, a = figure(whole[name]), figure(alone[name])
        lines.append(f"| {label} | {w[0]:.3f} ({w[1]:.3f} - {w[2]:.3f}) | {a[0]:.4f} ({a[1]:.4f} - {a[2]:.4f}) | "
                     f"{28 * params / a[0] / 1e6:.1f} |")
    del runs
    # the input pipeline
    P, B = 256, 16
    base = synthetic.lowpass_images(1, 512, 768, seed=5)[0]
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(args.images):
            models.write_png(os.path.join(tmp, f"{k:03d}.png"), np.roll(base, (17 * k, 29 * k), axis=(0, 1)))
        t0 = time.perf_counter()
        data = PatchDataset(os.path.join(tmp, "*.png"), P, B, repeat=True, seed=0, device=device, dtype=torch.bfloat16)
        next(data)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        host_images = [models.read_png(f) for f in data.files]

        def device_batches():
            for _ in range(args.batches):
                out = next(data)
            return out

        def host_batches(plan):
            for triples in plan:
                out = torch.stack([host_images[i][t:t + P, l:l + P] for i, t, l in triples]).to(device).to(torch.bfloat16)
            return out

        rates = {"device": [], "host": []}
        for _ in range(3):
            plan = data.plan(args.batches)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = device_batches()
            torch.cuda.synchronize()
            rates["device"].append(args.batches / (time.perf_counter() - t0))
            t0 = time.perf_counter()
            want = host_batches(plan)
            torch.cuda.synchronize()
            rates["host"].append(args.batches / (time.perf_counter() - t0))
            assert torch.equal(got, want), "the two paths deliver different batches"
    lines += ["", f"Input pipeline: batches of {B} x {P}x{P} bfloat16 out of {args.images} PNGs of 512 x 768 "
              f"(decode, upload and first batch: {first:.2f} s), best of three of {args.batches} batches.", "",
              "| path | batches/s | Mpixel/s |", "|---|---|---|"]
    for name, label in (("device", "`PatchDataset(device=)`: table upload + `crop_patches`"),
                        ("host", "host crop of decoded images, stack, upload, cast")):
        r = max(rates[name])
        lines.append(f"| {label} | {r:.0f} | {r * B * P * P / 1e6:.0f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
