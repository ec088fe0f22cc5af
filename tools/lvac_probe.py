"""An LVAC training step (models/lvac) on the fused kernels of csrc/lvac.hip and on their tensor-op twins, on the same
device, in one process.

The cloud is synthetic: `--points` random voxels of the surface of a 2^`--bits` cube, with smooth colours, in Morton
order.  The model is the notebook's default (C = 32, H = 256, "mlp", local positions) at `--target_level` (default
3 bits - 6, blocks of 4 x 4 x 4 voxels as target_level 24 gives on a 10-bit cloud).

What the figures are.  "step" is the host clock around `--steps` whole `Model.train_step()` calls that end in a device
synchronise, per step; each figure is the median of `--groups` such groups, taken in turns (fused, twins, fused, ...)
after a warm-up of both; min and max are the spread.  "decoder" is the same around the point decoder alone
(`point_mlp_loss` forward + backward on the step's own latents), "raht" around `raht_synthesize` forward + backward.
"peak" is torch's peak allocation plus the library's cached bytes over one step, above what was resident before it.
Writes profiles/lvac_probe.md (or --out)."""
import argparse
import os
import statistics
import sys
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


def synthetic_cloud(bits, points, seed):
    """Random voxels of a cube's surface, unique, in ascending Morton order, with smooth colours."""
    from compression_amd.models import lvac
    rng = np.random.default_rng(seed)
    side = 1 << bits
    p = rng.integers(0, side, (2 * points, 3))
    axis = rng.integers(0, 3, 2 * points)
    p[np.arange(2 * points), axis] = rng.integers(0, 2, 2 * points) * (side - 1)
    p = np.unique(p, axis=0)
    p = p[rng.permutation(len(p))[:points]]
    p = p[np.argsort(lvac.morton_from_position(p))]
    t = p / side * 2 * np.pi
    colours = 127.5 + 100 * np.stack([np.sin(t[:, 0] + t[:, 1]), np.cos(t[:, 1] * 2), np.sin(t[:, 2] - t[:, 0])], -1)
    return p.astype(np.float32), np.clip(colours, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lvac_probe.md"))
    ap.add_argument("--bits", type=int, default=9)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--target_level", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5, help="steps of one timed group")
    ap.add_argument("--groups", type=int, default=5, help="timed groups per route")
    args = ap.parse_args()
    from compression_amd import pipeline
    from compression_amd.models import lvac
    from compression_amd.ops import lvac_ops
    assert torch.cuda.is_available(), "needs the GPU"
    level = args.target_level if args.target_level is not None else 3 * args.bits - 6
    position, colours = synthetic_cloud(args.bits, args.points, seed=1)
    config = lvac.Config(target_level=level)
    runs = {}
    for name in ("fused", "twins"):
        torch.manual_seed(0)
        model = lvac.Model(config, position, colours).cuda()
        model.force_reference = name == "twins"
        runs[name] = model
    n = runs["fused"].count
    blocks = runs["fused"].blocks.n_blocks
    active = sum(1 for r in runs["fused"].tree.ac_rows if r)
    head = sum(1 for lv in runs["fused"].tree.levels
               if lv["n_ac"] and lv["n_child"] * config.num_channels <= lvac_ops.LVAC_CONSTANTS["RAHT_HEAD_ITEMS"])
    for model in runs.values():
        for _ in range(2):
            model.train_step()

    def peak(model):
        torch.cuda.synchronize()
        pipeline.empty_cache()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated() + pipeline.cached_bytes()
        model.train_step()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() + pipeline.cached_bytes() - before) / 2 ** 20

    peaks = {name: peak(model) for name, model in runs.items()}

    def parts(model):
        with torch.no_grad():
            _, latent, _ = model.entropy_coding(training=True)
        latent = [t.detach().requires_grad_(True) for t in latent]

        def raht():
            model.synthesize(latent).sum().backward()

        z = model.synthesize(latent).detach().requires_grad_(True)

        def decoder():
            fn = lvac_ops.point_mlp_loss_reference if model.force_reference else lvac_ops.point_mlp_loss
            loss = fn(z, model.blocks, model.position, model.mlp[0].kernel, model.mlp[0].bias, model.mlp[1].kernel,
                      model.mlp[1].bias, model.colors)[0]
            loss.backward()
        return raht, decoder

    samples = {name: {"step": [], "raht": [], "decoder": []} for name in runs}
    pieces = {name: parts(model) for name, model in runs.items()}
    for _ in range(args.groups):
        for name, model in runs.items():
            samples[name]["step"].append(group_ms(model.train_step, args.steps))
            samples[name]["raht"].append(group_ms(pieces[name][0], args.steps))
            samples[name]["decoder"].append(group_ms(pieces[name][1], args.steps))

    k = config.num_channels + 3
    flops = 2.0 * n * k * config.hidden_dim                    # one evaluation of the first layer
    lines = ["# LVAC training step: fused kernels against their tensor-op twins", "",
             f"`python tools/lvac_probe.py --bits {args.bits} --points {args.points}`: {n} points on the surface of a "
             f"2^{args.bits} cube, target_level {level} ({blocks} blocks, {active} levels with AC rows of which {head} in "
             f"the head launch), C = {config.num_channels}, H = {config.hidden_dim}, local positions, {torch.cuda.get_device_name(0)}.",
             f"Median (min .. max) of {args.groups} groups of {args.steps}, each ending in a synchronise, the two routes in turns.", "",
             "| what | fused, ms | twins, ms | twins / fused |", "|---|---|---|---|"]
    for what in ("step", "raht", "decoder"):
        f, t = figure(samples["fused"][what]), figure(samples["twins"][what])
        lines.append(f"| {what} | {f[0]:.3f} ({f[1]:.3f} .. {f[2]:.3f}) | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {t[0] / f[0]:.2f} |")
    dec = figure(samples["fused"]["decoder"])[0]
    lines += ["", f"Peak device memory of one step above what is resident: fused {peaks['fused']:.1f} MiB, twins "
              f"{peaks['twins']:.1f} MiB (the hidden tensor alone is {n * config.hidden_dim * 4 / 2 ** 20:.1f} MiB).", "",
              f"The fused decoder evaluates the first layer 3 times and its two transposed products once each: "
              f"{5 * flops / 1e9:.2f} GFLOP a step, {5 * flops / dec / 1e9:.2f} TFLOP/s of float32 on the vector unit.", "",
              "Not measured: a real voxelised scan (about 1 M points at 10 bits), per-kernel times, an MFMA variant of the "
              "contractions.  The step outside the two operations (one entropy model per level and two optimiser steps) is "
              "made of small launches and is not broken down here.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
