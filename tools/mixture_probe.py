"""The Gaussian-mixture coder and likelihood next to what they stand beside, at the mbt2018 shape: a latent of
32 x 48 x 192 (a 512 x 768 image), one image and sixteen, K = 3.

What is measured, in ONE process, the candidates alternating over --rounds rounds:
  (a) `mixture_encode` / `mixture_decode` (csrc/mixture_coder.hip: every CDF evaluated where it is coded), in streams of
      1024 symbols (the model's default) and of 9216 (a latent row, the table path's layout), against
  (b) `LocationScaleIndexedEntropyModel.compress` / `decompress` with coding_rank 2 (a stream per latent row, as mbt2018
      codes) on the same integer symbols: the table path, 64 Gaussian tables read from memory.  Both sides leave their
      strings on the device (no read-back in the timed region);
  (c) `mixture_bits` forward + backward (csrc/mixture_bits.hip) against the `NoisyNormalMixture` tensor-op composition
      (`mixture_bits_reference`) forward + backward, float32.

"ms" is the host clock around `reps` back-to-back calls that end in a device synchronise, warmed up first; the table
gives every round and the median.  Symbols: round(mean of a drawn component + its scale x normal noise); scales
log-uniform in 0.11 ... 16.  Writes a markdown table to --out (default profiles/mixture_probe.md) and prints it;
profiles/mixture_notes.md is that table with what the figures mean written in front of it by hand."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HL, WL, M, K, NUM_SCALES = 32, 48, 192, 3, 64


def timed(fn, window_ms):
    """Host ms per call, device work included."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = (time.perf_counter() - t0) * 1e3
    reps = max(3, min(200, int(window_ms / max(once, 1e-3))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_probe.md"))
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    import compression_amd as tfc
    from compression_amd.ops import mixture_ops

    lines = [f"latent {HL} x {WL} x {M}, K = {K}, {args.rounds} alternating rounds, window {args.window_ms:.0f} ms", ""]
    for batch in (1, 16):
        gen = torch.Generator(device="cuda").manual_seed(batch)
        shape = (batch, HL, WL, M)
        logits = torch.randn(*shape, K, device="cuda", generator=gen)
        loc = torch.randn(*shape, K, device="cuda", generator=gen) * 6.0
        scale = torch.exp(torch.rand(*shape, K, device="cuda", generator=gen) * math.log(16 / 0.11) + math.log(0.11))
        pick = torch.multinomial(torch.softmax(logits.reshape(-1, K), -1), 1, generator=gen).reshape(*shape, 1)
        y = loc.gather(-1, pick)[..., 0] + scale.gather(-1, pick)[..., 0] * torch.randn(*shape, device="cuda", generator=gen)
        sym = torch.round(y)
        lo, hi = int(sym.min()), int(sym.max())
        length = hi - lo + 1
        assert length <= mixture_ops.MAX_WINDOW
        flat = sym.reshape(batch, -1).to(torch.int32)
        params = tuple(t.reshape(batch, -1, K) for t in (logits, loc, scale))

        # the table path on the same symbols: a scale index per element, the location left at 0
        offset = math.log(0.11)
        factor = (math.log(256.0) - offset) / (NUM_SCALES - 1.0)
        em = tfc.LocationScaleIndexedEntropyModel(tfc.NoisyNormal, NUM_SCALES, lambda i: torch.exp(offset + factor * i),
                                                  coding_rank=2, compression=True, bottleneck_dtype=torch.float32)
        indexes = torch.rand(*shape, device="cuda", generator=gen) * (NUM_SCALES - 1)
        centred = (sym - loc.gather(-1, pick)[..., 0].round()).contiguous()          # small values, as y - mu is

        state = {}

        def mix_encode(ss):
            def run():
                state[ss] = mixture_ops.mixture_encode(flat, *params, lo, length, ss)
            return run

        def mix_decode(ss):
            def run():
                state["out"] = mixture_ops.mixture_decode(state[ss], *params, lo, length, ss)
            return run

        def table_encode():
            state["handle"] = em.compress(centred, indexes, device_result=True)

        def table_decode():
            state["table_out"] = em.decompress(state["handle"], indexes, defer_sanity=True)

        leaves = [t.clone().requires_grad_(True) for t in (logits, loc, scale)]
        y_leaf = y.clone().requires_grad_(True)
        noise = torch.rand(*shape, device="cuda", generator=gen) - 0.5

        def bits(fn):
            def run():
                for t in leaves + [y_leaf]:
                    t.grad = None
                _, b = fn(y_leaf, *leaves, 3, noise=noise)
                b.sum().backward()
            return run

        # the kernels give back what went in before anything is timed
        for ss in (1024, WL * M):
            mix_encode(ss)()
            mix_decode(ss)()
            got, ok = state["out"]
            assert torch.equal(got, flat) and bool(ok.all()), "the mixture coder does not round-trip"
        table_encode()
        table_decode()
        values, ok = state["table_out"]
        # (the values themselves come back on the table model's own quantisation grid, not as these integers)
        table_note = f"table path: {int((~ok.bool()).sum())} of {ok.numel()} streams refused after the round trip"
        bytes_mix = int(state[1024].offsets[-1])

        candidates = [("mixture_encode, streams of 1024", mix_encode(1024)),
                      ("mixture_decode, streams of 1024", mix_decode(1024)),
                      (f"mixture_encode, streams of {WL * M}", mix_encode(WL * M)),
                      (f"mixture_decode, streams of {WL * M}", mix_decode(WL * M)),
                      (f"table compress, streams of {WL * M}", table_encode),
                      (f"table decompress, streams of {WL * M}", table_decode),
                      ("mixture_bits forward + backward", bits(mixture_ops.mixture_bits)),
                      ("NoisyNormalMixture composition forward + backward", bits(mixture_ops.mixture_bits_reference))]
        times = {name: [] for name, _ in candidates}
        for _ in range(args.rounds):
            for name, fn in candidates:
                times[name].append(timed(fn, args.window_ms))
        med = {name: statistics.median(t) for name, t in times.items()}
        symbols = flat.numel()
        lines += [f"### batch {batch}: {symbols} symbols, window [{lo}, {hi}] (L = {length}), "
                  f"{8 * bytes_mix / symbols:.3f} bits per symbol coded", "",
                  "| candidate | ms per call, each round | median ms | ns per symbol |", "|---|---|---|---|"]
        for name, _ in candidates:
            lines.append(f"| {name} | {', '.join(f'{t:.3f}' for t in times[name])} | {med[name]:.3f} | "
                         f"{med[name] * 1e6 / symbols:.2f} |")
        row = WL * M
        lines += ["",
                  f"decode, mixture / table at the same stream layout: "
                  f"{med[f'mixture_decode, streams of {row}'] / med[f'table decompress, streams of {row}']:.2f}; "
                  f"encode: {med[f'mixture_encode, streams of {row}'] / med[f'table compress, streams of {row}']:.2f}; "
                  f"at the model's 1024-symbol streams: decode "
                  f"{med['mixture_decode, streams of 1024'] / med[f'table decompress, streams of {row}']:.2f}, encode "
                  f"{med['mixture_encode, streams of 1024'] / med[f'table compress, streams of {row}']:.2f}",
                  f"bits, fused / composition: "
                  f"{med['mixture_bits forward + backward'] / med['NoisyNormalMixture composition forward + backward']:.3f} "
                  "(below 1: the fused kernels are faster)", table_note, ""]
        del em, state
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
