"""The Y4M kernels at 16 frames of 1920 x 1080 4:2:0, all in one run: `unpack_frames`, `pack_frames`,
`ycbcr_to_rgb` (uint8 and bfloat16 outputs, both upsamplings) and `rgb_to_ycbcr`, each next to the torch-op expression of
the same definition (the op's `*_reference` twin on the device) and to a device copy that moves the same number of
bytes; then `Y4MDataset(device=...)` frames per second from a file in the page cache.

What the figures are.  Every call takes the next of a ring of input sets that is larger than the 256 MB Infinity Cache,
so inputs are cold; outputs come from torch's allocator as in any user's call.  "us" is device events around `reps`
back-to-back calls (reps sized so that the window is about --window-ms), so it is the CALL time: kernel plus launch gap
and allocation.  "bytes" is what the algorithm has to move (read + written; per pixel: unpack and pack 3, to RGB 4.5
for uint8 and 7.5 for bfloat16, from RGB uint8 4.5); the copy of a row moves the same total (half of it read, half
written) and is the yardstick for "fraction of achievable bandwidth" ("x copy" = us / copy us).  "fill us" is the time
to zero as many bytes as the op writes (per pixel: unpack, pack and from RGB 1.5, to RGB 3 and 6): a conversion to RGB
writes two to four times what it reads, a copy as much as it reads.
Writes profiles/y4m_probe.md (or --out)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FRAMES, WIDTH, HEIGHT = 16, 1920, 1080


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "y4m_probe.md"))
    ap.add_argument("--window-ms", type=float, default=200.0, help="timed window per figure")
    ap.add_argument("--file-frames", type=int, default=64, help="frames of the file the dataset is timed on")
    args = ap.parse_args()
    from compression_amd.datasets import Y4MDataset, Y4MWriter
    from compression_amd.ops import video_ops as v
    assert torch.cuda.is_available(), "needs the GPU"
    size = v.frame_bytes(WIDTH, HEIGHT, "420")
    stride, pixels = 6 + size, FRAMES * WIDTH * HEIGHT
    sets = 6                 # 6 x (50 + 50 + 100 + 199 MB) of inputs: far beyond the Infinity Cache
    ring = []
    for _ in range(sets):
        raw = torch.randint(0, 256, (6 + FRAMES * stride,), dtype=torch.uint8, device="cuda")
        y, cbcr = v.unpack_frames(raw, FRAMES, WIDTH, HEIGHT, "420", frame_stride=stride, first_offset=6)
        rgb8 = v.ycbcr_to_rgb(y, cbcr)
        ring.append(dict(raw=raw, y=y, cbcr=cbcr, rgb8=rgb8, rgb16=rgb8.to(torch.bfloat16),
                         out=torch.empty_like(raw)))
    k = [0]

    def nxt():
        k[0] += 1
        return ring[k[0] % sets]

    def unpack(fn):
        return lambda: fn(nxt()["raw"], FRAMES, WIDTH, HEIGHT, "420", frame_stride=stride, first_offset=6)

    def pack(fn):
        def call():
            s = nxt()
            fn(s["y"], s["cbcr"], out=s["out"], frame_stride=stride, first_offset=6)
        return call

    def to_rgb(fn, dtype, upsample):
        def call():
            s = nxt()
            fn(s["y"], s["cbcr"], upsample=upsample, dtype=dtype)
        return call

    def from_rgb(fn, key):
        return lambda: fn(nxt()[key], "420")

    rows = [("unpack_frames", 3.0, 1.5, unpack(v.unpack_frames), unpack(v.unpack_frames_reference)),
            ("pack_frames", 3.0, 1.5, pack(v.pack_frames), pack(v.pack_frames_reference))]
    for dtype, per in ((torch.uint8, 4.5), (torch.bfloat16, 7.5)):
        for upsample in ("bilinear", "nearest"):
            rows.append((f"ycbcr_to_rgb {str(dtype)[6:]} {upsample}", per, per - 1.5,
                         to_rgb(v.ycbcr_to_rgb, dtype, upsample),
                         to_rgb(v.ycbcr_to_rgb_reference, dtype, upsample)))
    rows.append(("rgb_to_ycbcr uint8", 4.5, 1.5, from_rgb(v.rgb_to_ycbcr, "rgb8"),
                 from_rgb(v.rgb_to_ycbcr_reference, "rgb8")))
    rows.append(("rgb_to_ycbcr bfloat16", 7.5, 1.5, from_rgb(v.rgb_to_ycbcr, "rgb16"),
                 from_rgb(v.rgb_to_ycbcr_reference, "rgb16")))

    # copies of every byte count in use, from and to buffers as cold as the ops' inputs
    copy_src = [torch.empty(int(6 * pixels), dtype=torch.uint8, device="cuda") for _ in range(sets)]
    copy_dst = [torch.empty_like(t) for t in copy_src]

    def copy(nbytes):
        def call():
            k[0] += 1
            copy_dst[k[0] % sets][:nbytes].copy_(copy_src[k[0] % sets][:nbytes])
        return call

    def fill(nbytes):
        def call():
            k[0] += 1
            copy_dst[k[0] % sets][:nbytes].zero_()
        return call

    lines = [f"{FRAMES} frames of {WIDTH} x {HEIGHT} 4:2:0; device {torch.cuda.get_device_name(0)}", "",
             "| op | bytes | kernel us | TB/s | copy us | x copy | fill us | torch ops us | x torch |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, per, written, op, twin in rows:
        nbytes = int(per * pixels)
        figures = []
        for fn in (op, copy(nbytes // 2), twin, fill(int(written * pixels))):
            rough = timed(fn, 3)
            figures.append(timed(fn, int(min(2000, max(5, args.window_ms * 1e3 / rough)))))
        us, copy_us, twin_us, fill_us = figures
        lines.append(f"| {name} | {nbytes / 1e6:.1f} MB | {us:.1f} | {nbytes / us / 1e6:.2f} | {copy_us:.1f} | "
                     f"{us / copy_us:.2f} | {fill_us:.1f} | {twin_us:.1f} | {twin_us / us:.1f} |")
        print(lines[-1], flush=True)

    # the dataset: a file in the page cache (written just now, read once before the clock starts)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe.y4m")
        with Y4MWriter(path, WIDTH, HEIGHT) as writer:
            for at in range(0, args.file_frames, FRAMES):
                s = nxt()
                writer.write(s["y"][:args.file_frames - at], s["cbcr"][:args.file_frames - at])
        file_bytes = os.path.getsize(path)
        lines += ["", f"`Y4MDataset` on a {file_bytes / 1e6:.0f} MB file of {args.file_frames} frames in the page cache "
                      "(host clock around the loop and a final synchronise, best of 3):", "",
                  "| mode | frames/s | file GB/s |", "|---|---|---|"]

        def run(device, convert, fpr=FRAMES):
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                count = 0
                for y, cbcr in Y4MDataset(path, device=device, frames_per_read=fpr).batches(fpr):
                    if convert:
                        v.ycbcr_to_rgb(y, cbcr)
                    count += y.shape[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            assert count == args.file_frames
            return best

        run(None, False)
        for label, device, convert, fpr in (("device=None (numpy)", None, False, FRAMES),
                                            ("device, batches(16)", "cuda", False, FRAMES),
                                            ("device, batches(16) + ycbcr_to_rgb", "cuda", True, FRAMES),
                                            ("device, batches(4)", "cuda", False, 4)):
            dt = run(device, convert, fpr)
            lines.append(f"| {label} | {args.file_frames / dt:.0f} | {file_bytes / dt / 1e9:.2f} |")
            print(lines[-1], flush=True)
    text = "# Y4M probe (tools/y4m_probe.py)\n\n" + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
