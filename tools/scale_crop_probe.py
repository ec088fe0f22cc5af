"""`scale_crop_patches` at HiFiC's training shape: 16 patches of 256 x 256 out of a pool of 2000 x 1300
images, float32 and bfloat16, next to two baselines on the same device:

    crop_patches              the plain crop kernel at the same output shape and type: bounded by the same writes
    interpolate + crop        the path this replaces, stated on the device: torch.nn.functional.interpolate of every
                              WHOLE image (bilinear, align_corners=False; to float first), then the crop and the cast

What the figures are.  Every call takes the next of a ring of pools and of a ring of outputs, each ring larger than the
256 MB Infinity Cache, so source reads and output writes are cold.  The two kernels are called through the C ABI with
tables uploaded in advance (no allocation, no upload, no tensor conversion per call).  "us" is device events around
`reps` back-to-back calls (reps sized so that the window is about --window-ms), so it is the CALL time: kernel plus launch
gap.  "host us" is the host clock over the same loop without a synchronise.  GB/s is the output bytes over "us" (the
source bytes are below 4 % of them for the kernels).  A kernel's own time comes from a trace of this script:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/scale_crop_probe.py --calls scale_crop,crop
    python tools/rocprof_summary.py DIR out.md "title"
Writes profiles/scale_crop_probe.md (or --out)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, P, B = 1300, 2000, 256, 16
IMAGES_PER_POOL = 16
CALLS = ["crop", "scale_crop", "interpolate + crop"]


def timed(fn, reps):
    """(device us per call, host us per call spent enqueuing)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / reps * 1e6
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_crop_probe.md"))
    ap.add_argument("--window-ms", type=float, default=20.0, help="timed window per figure")
    ap.add_argument("--calls", default=",".join(CALLS))
    args = ap.parse_args()
    from compression_amd import _lib
    from compression_amd.ops.video_ops import DTYPE_CODE
    assert torch.cuda.is_available(), "needs the GPU"
    lib, stream = _lib.lib(), _lib.stream_ptr()
    wanted = [c.strip() for c in args.calls.split(",")]
    image_bytes = 3 * H * W
    pools = max(3, -(-(512 << 20) // (IMAGES_PER_POOL * image_bytes)))
    gen = torch.Generator().manual_seed(0)
    ring = [torch.randint(0, 256, (IMAGES_PER_POOL * image_bytes,), dtype=torch.uint8, generator=gen).cuda()
            for _ in range(pools)]
    # one patch per image, scales over HiFiC's range [0.75, 0.95), corners anywhere
    rows, plain = [], []
    for k in range(B):
        scale = 0.75 + 0.2 * k / B
        oh, ow = math.ceil(scale * H), math.ceil(scale * W)
        top = int(torch.randint(0, oh - P + 1, (1,), generator=gen))
        left = int(torch.randint(0, ow - P + 1, (1,), generator=gen))
        rows.append([k * image_bytes, W, H, ow, oh, top, left])
        plain.append([k * image_bytes, W, min(top, H - P), min(left, W - P)])
    scaled_table, plain_table = torch.tensor(rows).cuda(), torch.tensor(plain).cuda()
    lines = ["| output | call | us | host us | reps | output bytes | GB/s | x crop |", "|---|---|---|---|---|---|---|---|"]
    for dtype in (torch.bfloat16, torch.float32):
        one = B * P * P * 3 * torch.empty((), dtype=dtype).element_size()
        outs = [torch.empty((B, P, P, 3), dtype=dtype, device="cuda") for _ in range(max(3, -(-(320 << 20) // one)))]
        k = [0]

        def nxt():
            k[0] += 1
            return ring[k[0] % len(ring)], outs[k[0] % len(outs)]

        def crop():
            pool, out = nxt()
            _lib.check(lib.tfc_crop_patches(pool.data_ptr(), pool.numel(), plain_table.data_ptr(), B, P,
                                            DTYPE_CODE[dtype], out.data_ptr(), stream))

        def scale_crop():
            pool, out = nxt()
            _lib.check(lib.tfc_scale_crop_patches(pool.data_ptr(), pool.numel(), scaled_table.data_ptr(), B, P,
                                                  DTYPE_CODE[dtype], out.data_ptr(), stream))

        def interpolate():
            pool, out = nxt()
            for b, (off, _, _, ow, oh, top, left) in enumerate(rows):
                image = pool[off:off + image_bytes].view(1, H, W, 3).permute(0, 3, 1, 2).float()
                whole = torch.nn.functional.interpolate(image, size=(oh, ow), mode="bilinear", align_corners=False)
                out[b].copy_(whole[0, :, top:top + P, left:left + P].permute(1, 2, 0))
        calls = {"crop": crop, "scale_crop": scale_crop, "interpolate + crop": interpolate}
        crop_us = None
        for name in CALLS:
            if name not in wanted:
                continue
            rough, _ = timed(calls[name], 5)
            reps = int(min(4000, max(5, args.window_ms * 1e3 / rough)))
            us, host = timed(calls[name], reps)
            if name == "crop":
                crop_us = us
            rel = f"{us / crop_us:.2f}" if crop_us else ""
            lines.append(f"| [{B}, {P}, {P}, 3] {str(dtype).replace('torch.', '')} | {name} | {us:.1f} | {host:.1f} | {reps} | "
                         f"{one / 1e6:.1f} MB | {one / us / 1e3:.1f} | {rel} |")
            print(lines[-1], flush=True)
        del outs
        torch.cuda.empty_cache()
    text = ("# scale_crop_patches probe (tools/scale_crop_probe.py)\n\n"
            f"{B} patches of {P} x {P} out of pools of {IMAGES_PER_POOL} images of {W} x {H}; {pools} pools in rotation.\n\n"
            + "\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
