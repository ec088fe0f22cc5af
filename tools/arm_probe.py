"""`arm_bits` forward plus backward (csrc/arm_bits.hip) against its float32 tensor-op twin on the same device, and
against a device copy of y plus bits as the floor (the ARM section).

Two workloads at C = `--context`, L = `--layers`: one 512 x 768 grid, and the seven-level latent pyramid of a 768 x 512
image (512 x 768 down to 8 x 12, one call per level).  Gradients go to y and all four parameters.

What the figures are.  "events" is the time between two device events around `--calls` forward + backward passes, per
pass: it holds the kernels, the gaps between them and autograd's own small kernels.  "kernels" is the library's own
per-launch-scope events (tfc_profile_enable) summed over the forward and the backward entry, per pass: the kernels
alone.  Each figure is the median (min .. max) of `--groups` groups taken in turns after a warm-up of every route.
Writes profiles/arm_notes.md (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


SCOPES = ("arm_bits_forward", "arm_bits_backward")


def scope_ms(names):
    from compression_amd import _lib
    total = 0.0
    for name in names:
        ms, n = C.c_double(), C.c_int64()
        _lib.lib().tfc_profile_query(name.encode(), C.byref(ms), C.byref(n))
        total += ms.value
    return total


def group(fn, calls, scoped=False):
    """ms per pass between two device events; with `scoped`, of the library's launch scopes instead (their events cost
    host time, so the two are taken in groups of their own)."""
    from compression_amd import _lib
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _lib.lib().tfc_profile_enable(int(scoped))                   # enabling clears the scopes' totals
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    _lib.lib().tfc_profile_enable(0)
    return (scope_ms(SCOPES) if scoped else start.elapsed_time(stop)) / calls


def figure(samples):
    return f"{statistics.median(samples):.3f} ({min(samples):.3f} .. {max(samples):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arm_notes.md"))
    ap.add_argument("--context", type=int, default=24)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--calls", type=int, default=1000, help="passes of one timed group of the fused route and the copy; "
                    "the twin, ten times slower, takes a tenth")
    ap.add_argument("--groups", type=int, default=7, help="timed groups per route")
    args = ap.parse_args()
    from compression_amd.ops.arm_ops import arm_bits, arm_bits_reference
    assert torch.cuda.is_available(), "needs the GPU"
    gen = torch.Generator().manual_seed(0)
    c, layers = args.context, args.layers
    params = [(torch.randn(shape, generator=gen) * 0.3 * c ** -0.5).cuda().requires_grad_(True)
              for shape in ((layers, c, c), (layers, c), (c, 2), (2,))]
    workloads = {"512 x 768": [(512, 768)], "pyramid of 768 x 512": [(512 >> k, 768 >> k) for k in range(7)]}
    lines = ["# arm_bits: the fused kernels against the tensor-op twin", "",
             f"`python tools/arm_probe.py --context {c} --layers {layers}` on {torch.cuda.get_device_name(0)}: forward plus "
             "backward (gradients to y and the four parameters), ms per pass.",
             f"Median (min .. max) of {args.groups} groups of {args.calls} passes (the twin: a tenth), the routes in turns; \"events\" is "
             "device time between two events around a group, \"kernels\" the library's own launch scopes.", "",
             "| workload | fused, events | fused, kernels | twin, events | copy of y and bits, events | twin / fused |",
             "|---|---|---|---|---|---|"]
    scopes, pixels = {}, {}
    for label, shapes in workloads.items():
        grids = [torch.randint(-4, 5, (1,) + s, generator=gen).float().cuda().requires_grad_(True) for s in shapes]

        def passes(fn):
            def run():
                for y in grids:
                    torch.autograd.grad(fn(y, *params).sum(), [y] + params)
            return run

        def floor():
            for y in grids:
                y.detach().clone()
                torch.empty(1, device="cuda").clone()

        routes = {"fused": passes(arm_bits), "twin": passes(arm_bits_reference), "floor": floor}
        samples, kernels = {name: [] for name in routes}, []
        for fn in routes.values():
            for _ in range(3):
                fn()
        for _ in range(args.groups):
            for name, fn in routes.items():
                samples[name].append(group(fn, max(args.calls // 10, 1) if name == "twin" else args.calls))
            kernels.append(group(routes["fused"], args.calls, scoped=True))
        scopes[label] = statistics.median(kernels)
        pixels[label] = sum(h * w for h, w in shapes)
        lines.append(f"| {label} | {figure(samples['fused'])} | {figure(kernels)} | {figure(samples['twin'])} | "
                     f"{figure(samples['floor'])} | "
                     f"{statistics.median(samples['twin']) / statistics.median(samples['fused']):.1f} |")
    one, pyramid = list(workloads)
    lines += ["", f"The pyramid holds {pixels[pyramid] / pixels[one]:.2f} times the pixels of the single grid and takes "
              f"{scopes[pyramid] / scopes[one]:.2f} times its launch scopes: five launches a level, and on the small levels "
              "the device waits for the host between them.", "",
              "Not measured: per-kernel times inside a launch scope, several levels in one launch, other context sizes and "
              "depths, B > 1.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
