"""Random patches of randomly resized PNG images, HiFiC's training input (`_get_dataset` / `_preprocess`,
models/hific/model.py:283-363): files -> read_png -> resize by a random factor -> random crop -> batch(drop_remainder)
-> repeat -> shuffle.  The reference resizes every whole image with `tf.image.resize_images` on a host thread and keeps
one crop_size x crop_size patch of it; here the decoded images stay in `PatchDataset`'s device pool and a batch is one
`scale_crop_patches` kernel, which computes the patches' pixels only: the resized images never exist.

Scale.  Per item, all in float32 (model.py:331-348), for an H x W image and patch size P:

    min_fac = max(0.75, P / min(H, W))        above 1 for an image with a side below P: it is upscaled to fit
    max_fac = max(min_fac, 0.95)
    scale   = min_fac + u (max_fac - min_fac)                     u uniform in [0, 1)
    OH      = max(ceil(scale H), P),  OW = max(ceil(scale W), P)

The outer `max` guards the float32 rounding of P / side * side, which may land just below P.

Order.  One CPU `torch.Generator` (seeded with `seed`) decides everything.  Each pass draws, in this order: a
permutation of the files; one float32 `u` per file (`torch.rand`); one pair of integers per file.  For the files in
the permuted order, item k takes the k-th `u` for its scale and the k-th pair for `top` in [0, OH - P] and `left` in
[0, OW - P], both in the RESIZED image.  The items of the passes form one stream, cut into batches as in
`PatchDataset`; what a batch holds depends on the generator alone, never on the pool limit.

Against the reference: a fresh permutation per pass stands in for `shuffle(buffer_size)` behind `repeat()`, as in
`PatchDataset`, and TensorFlow's random stream (`tf.random_uniform(seed=42)`, `tf.image.random_crop`) cannot be
reproduced here: the distribution of scales and corners is the reference's, the draws are not."""
from __future__ import annotations

import torch

from ..ops import train_ops
from .patch_dataset import PatchDataset

__all__ = ["ScaledPatchDataset"]

SMALLEST_FAC, BIGGEST_FAC = 0.75, 0.95          # model.py:298-299


class ScaledPatchDataset(PatchDataset):
    """`ScaledPatchDataset(files_or_glob, patchsize, batchsize, *, repeat, seed=0, device=None, dtype=torch.float32,
    pool_limit_bytes=2 ** 32, preprocess_threads=16)` iterates batches [B, P, P, 3] of float32 or bfloat16 `dtype` in
    [0, 255].  Images of any size are taken.  `plan()` items are (file index, OH, OW, top, left).  `device=None`:
    everything on the CPU, through `scale_crop_patches_reference`."""

    def __init__(self, files_or_glob, patchsize, batchsize, *, repeat, seed=0, device=None, dtype=torch.float32,
                 pool_limit_bytes=2 ** 32, preprocess_threads=16):
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"dtype must be torch.float32 or bfloat16 (the values are not integers), got {dtype}")
        super().__init__(files_or_glob, patchsize, batchsize, repeat=repeat, seed=seed, device=device, dtype=dtype,
                         pool_limit_bytes=pool_limit_bytes, preprocess_threads=preprocess_threads)

    def _check_image_size(self, name, h, w):
        if h > 2 ** 24 or w > 2 ** 24:
            raise ValueError(f"{name} is {h} x {w}: a side may not exceed 2^24")

    def scale_range(self, index):
        """(min_fac, max_fac) of file `index`, as float32 tensors of no dimension."""
        return tuple(v[0] for v in self._scale_range(torch.tensor([index])))

    def _scale_range(self, files):
        f32 = torch.float32
        side = torch.minimum(self._height[files], self._width[files]).to(f32)
        min_fac = torch.clamp(torch.tensor(float(self.patchsize), dtype=f32) / side, min=SMALLEST_FAC)
        return min_fac, torch.clamp(min_fac, min=BIGGEST_FAC)

    def _draw_pass(self):
        state = self._gen.get_state()
        n, P, f32 = len(self.files), self.patchsize, torch.float32
        perm = torch.randperm(n, generator=self._gen)
        u = torch.rand(n, dtype=f32, generator=self._gen)
        r = torch.randint(0, 2 ** 62, (n, 2), generator=self._gen)
        min_fac, max_fac = self._scale_range(perm)
        scale = min_fac + u * (max_fac - min_fac)
        new_height = torch.ceil(scale * self._height[perm].to(f32)).to(torch.int64).clamp(min=P)
        new_width = torch.ceil(scale * self._width[perm].to(f32)).to(torch.int64).clamp(min=P)
        top = r[:, 0] % (new_height - P + 1)
        left = r[:, 1] % (new_width - P + 1)
        self._passes.append((state, list(zip(perm.tolist(), new_height.tolist(), new_width.tolist(), top.tolist(),
                                             left.tolist()))))

    def _cut(self, piece, items):
        table = torch.tensor([[piece.where[i], int(self._width[i]), int(self._height[i]), ow, oh, top, left]
                              for i, oh, ow, top, left in items], dtype=torch.int64)
        return train_ops.scale_crop_patches(piece.pool, table, self.patchsize, self.dtype)
