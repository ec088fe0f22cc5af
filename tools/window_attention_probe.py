"""The window-attention kernels at the four stage shapes of the default SwinT-ChARM analysis transform for a 768x512
image, batch 8 (tokens 384x256 / 192x128 / 96x64 / 48x32, C = 128 / 192 / 256 / 320, head dimension 32, window 8,
shift 4), forward and backward, next to two baselines:
  (a) `window_attention_reference` (pad, roll, partition, two batched matmuls, softmax, and back) on the device;
  (b) a device copy of the same number of bytes: forward qkv + out, backward qkv + dout + dqkv.

What the figures are.  Every call takes the next of a ring of buffer sets that together exceed the 256 MB Infinity
Cache, so inputs are cold.  "us" is device events around `reps` back-to-back calls (reps sized so that the window is
about --window-ms), i.e. call time: kernel plus launch gap; warmed up first.  The kernels are called through the
autograd function's two halves (no allocation of inputs per call; the outputs are allocated by the caching allocator).
The reference's backward is `torch.autograd.grad` on a graph kept from one forward.  "of copy" is copy time over kernel
time: the achieved fraction of (b).  Random normal data (zeros would flatter the softmax).
Writes a markdown table to --out (default profiles/swin_probe.md) and prints it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STAGES = [(384, 256, 128), (192, 128, 192), (96, 64, 256), (48, 32, 320)]
BATCH, HEAD_DIM, WINDOW, SHIFT = 8, 32, 8, 4
CACHE_BYTES = 256 << 20


def timed(fn, window_ms):
    """Device us per call."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(3, min(200, int(window_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_probe.md"))
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--stages", default="0,1,2,3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from compression_amd.ops import attention_ops as A
    lines = ["| stage (tokens, C) | dtype | pass | kernel us | reference us | copy us | bytes | kernel TB/s | of copy | "
             "reference / kernel |", "|---|---|---|---|---|---|---|---|---|---|"]
    for index in (int(s) for s in args.stages.split(",")):
        h, w, c = STAGES[index]
        heads = c // HEAD_DIM
        for dtype in (getattr(torch, n) for n in args.dtypes.split(",")):
            es = torch.empty(0, dtype=dtype).element_size()
            tokens = BATCH * h * w
            fwd_bytes, bwd_bytes = tokens * 4 * c * es, tokens * 7 * c * es
            ring = max(2, min(8, -(-2 * CACHE_BYTES // fwd_bytes)))
            gen = torch.Generator(device="cuda").manual_seed(index)
            sets = []
            for _ in range(ring):
                qkv = torch.randn(BATCH, h, w, 3 * c, device="cuda", generator=gen).to(dtype)
                dout = torch.randn(BATCH, h, w, c, device="cuda", generator=gen).to(dtype)
                sets.append((qkv, dout))
            table = torch.randn(heads, (2 * WINDOW - 1) ** 2, device="cuda", generator=gen)
            turn = [0]

            def nxt():
                turn[0] = (turn[0] + 1) % ring
                return sets[turn[0]]

            class Ctx:      # the two halves of the autograd function, called directly
                needs_input_grad = (True, True)

                def save_for_backward(self, *t):
                    self.saved_tensors = t

            fn = A._WindowAttentionFunction

            def kernel_fwd():
                return fn.forward(Ctx(), nxt()[0], table, heads, WINDOW, SHIFT)

            def kernel_bwd():
                qkv, dout = nxt()
                ctx = Ctx()
                ctx.save_for_backward(qkv, table)
                ctx.cfg = (heads, WINDOW, SHIFT, torch.float32)
                return fn.backward(ctx, dout)

            def ref_fwd():
                with torch.no_grad():
                    return A.window_attention_reference(nxt()[0], table, heads, WINDOW, SHIFT)

            graph = {}

            def ref_bwd():
                return torch.autograd.grad(graph["out"], (graph["qkv"], graph["table"]), graph["dout"], retain_graph=True)

            def copier(nbytes):
                n = nbytes // 2 // 4
                src = [torch.empty(n, dtype=torch.float32, device="cuda").normal_() for _ in range(ring)]
                dst = torch.empty(n, dtype=torch.float32, device="cuda")
                state = [0]

                def run():
                    state[0] = (state[0] + 1) % ring
                    dst.copy_(src[state[0]])
                return run

            # the kernel and the reference agree at this shape before either is timed
            got, want = kernel_fwd(), A.window_attention_reference(sets[turn[0]][0], table, heads, WINDOW, SHIFT)
            err = (got.float() - want.float()).abs().max().item()
            assert err < (1e-4 if dtype == torch.float32 else 0.1), err
            del got, want

            t_k, _ = timed(kernel_fwd, args.window_ms)
            t_r, _ = timed(ref_fwd, args.window_ms)
            t_c, _ = timed(copier(fwd_bytes), args.window_ms)
            lines.append(f"| {index + 1} ({BATCH}x{h}x{w}, {c}) | {str(dtype)[6:]} | forward | {t_k:.0f} | {t_r:.0f} | "
                         f"{t_c:.0f} | {fwd_bytes / 1e6:.0f} MB | {fwd_bytes / t_k / 1e6:.2f} | {t_c / t_k:.2f} | "
                         f"{t_r / t_k:.1f} |")
            print(lines[-1], flush=True)
            t_k, _ = timed(kernel_bwd, args.window_ms)
            q = sets[0][0].clone().requires_grad_(True)
            tb = table.clone().requires_grad_(True)
            graph.update(qkv=q, table=tb, dout=sets[0][1], out=A.window_attention_reference(q, tb, heads, WINDOW, SHIFT))
            t_r, _ = timed(ref_bwd, args.window_ms)
            graph.clear()
            t_c, _ = timed(copier(bwd_bytes), args.window_ms)
            lines.append(f"| {index + 1} ({BATCH}x{h}x{w}, {c}) | {str(dtype)[6:]} | backward | {t_k:.0f} | {t_r:.0f} | "
                         f"{t_c:.0f} | {bwd_bytes / 1e6:.0f} MB | {bwd_bytes / t_k / 1e6:.2f} | {t_c / t_k:.2f} | "
                         f"{t_r / t_k:.1f} |")
            print(lines[-1], flush=True)
            del sets, q, tb
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
