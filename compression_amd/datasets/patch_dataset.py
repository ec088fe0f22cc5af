"""Random patches of PNG images, the training input of the model scripts (`get_custom_dataset` / `crop_image`,
models/bls2017.py:198-232): files -> shuffle(len(files), reshuffle_each_iteration) -> [repeat] -> read_png -> random
crop -> cast -> batch(drop_remainder).  The reference decodes every image anew for every patch on `preprocess_threads`
host threads; here the decoded images stay in one flat pool on the device and a batch is one `crop_patches` kernel.

Order.  One CPU `torch.Generator` (seeded with `seed`) decides everything: each pass draws a permutation of the files
and then, for the files in that order, `top` in [0, H - P] and `left` in [0, W - P].  The items of the passes form one
stream; a batch is the next `batchsize` items of it.  With `repeat=True` the stream has no end (a batch may hold the
end of one pass and the start of the next, as `repeat()` in front of `batch()` gives); with `repeat=False` an
iteration is one pass without its remainder, and the next iteration is the next pass.

Pool.  If all images fit `pool_limit_bytes` they are decoded once and stay.  Otherwise the pool holds the images of a
run of consecutive batches of the stream (as many as fit, at least one batch), and the next run is decoded on a
background thread while this one is consumed.  What a batch holds depends on the generator alone, never on the pool
limit."""
from __future__ import annotations

import glob as _glob
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import torch

from ..ops import train_ops

__all__ = ["PatchDataset"]


def _image_size(filename):
    from PIL import Image
    with Image.open(filename) as im:
        return im.size          # (W, H)


class _Slice:
    """The decoded images of `count` consecutive items of the stream, back to back in one pool."""

    def __init__(self, count, host_pool, where):
        self.count = count
        self.host_pool = host_pool      # pinned where a device will take it
        self.pool = None                # on the device (or the host pool itself) once current
        self.where = where              # file index -> byte offset


class PatchDataset:
    """`PatchDataset(files_or_glob, patchsize, batchsize, *, repeat, seed=0, device=None, dtype=torch.float32,
    pool_limit_bytes=2 ** 32, preprocess_threads=16)` iterates batches [B, P, P, 3] of `dtype` holding the integers
    0...255.  `device=None`: everything on the CPU, through `crop_patches_reference`."""

    def __init__(self, files_or_glob, patchsize, batchsize, *, repeat, seed=0, device=None, dtype=torch.float32,
                 pool_limit_bytes=2 ** 32, preprocess_threads=16):
        if isinstance(files_or_glob, (str, os.PathLike)):
            files = sorted(_glob.glob(os.fspath(files_or_glob)))
            if not files:
                raise RuntimeError(f"No training images found with glob '{os.fspath(files_or_glob)}'.")
        else:
            files = [os.fspath(f) for f in files_or_glob]
            if not files:
                raise RuntimeError("No training images found: the list of files is empty.")
        self.files = files
        self.patchsize, self.batchsize = int(patchsize), int(batchsize)
        if self.patchsize < 1 or self.batchsize < 1:
            raise ValueError(f"patchsize and batchsize must be positive, got {patchsize} and {batchsize}")
        if dtype not in train_ops.DTYPE_CODE:
            raise TypeError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
        self.repeat = bool(repeat)
        self.seed = int(seed)
        self.device = None if device is None else torch.device(device)
        self.dtype = dtype
        self.pool_limit_bytes = int(pool_limit_bytes)
        self.threads = max(1, min(16, int(preprocess_threads)))
        with ThreadPoolExecutor(self.threads) as pool:
            sizes = list(pool.map(_image_size, files))
        for name, (w, h) in zip(files, sizes):
            self._check_image_size(name, h, w)
        self._width = torch.tensor([w for w, _ in sizes], dtype=torch.int64)
        self._height = torch.tensor([h for _, h in sizes], dtype=torch.int64)
        self._bytes = 3 * self._width * self._height
        self._fits = int(self._bytes.sum()) <= self.pool_limit_bytes
        self._gen = torch.Generator(device="cpu").manual_seed(self.seed)
        # the stream: drawn passes not yet used up, (generator state in front of the pass, its items)
        self._passes = deque()
        self._pass_no = 0           # passes used up so far
        self._offset = 0            # items of the first pass in `_passes` already delivered
        self._open = True           # repeat=False: the current iteration has not ended
        self._slice = None
        self._slice_left = 0
        self._next = None           # (future of the next slice, its first item as (pass_no, offset))
        self._worker = None

    # ---------------------------------------------------------------------------------------------------------------
    # what a subclass with another kind of patch replaces (ScaledPatchDataset): which images it takes, what an item of
    # the stream is beyond its file index (`_draw_pass`), and how a batch is cut from the pool

    def _check_image_size(self, name, h, w):
        if h < self.patchsize or w < self.patchsize:
            raise ValueError(f"{name} is {h} x {w}, smaller than the {self.patchsize} x {self.patchsize} patch")

    def _cut(self, piece, items):
        table = torch.tensor([[piece.where[i], int(self._width[i]), top, left] for i, top, left in items],
                             dtype=torch.int64)
        return train_ops.crop_patches(piece.pool, table, self.patchsize, self.dtype)

    # ---------------------------------------------------------------------------------------------------------------
    # the stream

    def _draw_pass(self):
        state = self._gen.get_state()
        n = len(self.files)
        perm = torch.randperm(n, generator=self._gen)
        r = torch.randint(0, 2 ** 62, (n, 2), generator=self._gen)
        top = r[:, 0] % (self._height[perm] - self.patchsize + 1)
        left = r[:, 1] % (self._width[perm] - self.patchsize + 1)
        self._passes.append((state, list(zip(perm.tolist(), top.tolist(), left.tolist()))))

    def _peek(self, count):
        """The next `count` items, fewer where a pass without repeat ends; nothing is consumed."""
        items, at, k = [], self._offset, 0
        while len(items) < count:
            if k == len(self._passes):
                if not self.repeat and k > 0:
                    break
                self._draw_pass()
            take = self._passes[k][1][at:at + count - len(items)]
            items.extend(take)
            at, k = 0, k + 1
        return items

    def _advance(self, count):
        self._offset += count
        # without repeat the pass stays until its iteration ends (__next__ drops it with its remainder)
        while self.repeat and self._passes and self._offset >= len(self._passes[0][1]):
            self._offset -= len(self._passes[0][1])
            self._passes.popleft()
            self._pass_no += 1

    def _batches_left(self, num_batches):
        if not self.repeat:
            num_batches = min(num_batches, (len(self.files) - self._offset) // self.batchsize)
        return num_batches

    def plan(self, num_batches):
        """The (file index, top, left) triples of the next `num_batches` batches (fewer where the pass of a dataset
        without repeat ends first; after its end, those of the next iteration), one list per batch.  Consumes nothing."""
        n = self._batches_left(int(num_batches))
        items = self._peek(n * self.batchsize)
        return [items[k * self.batchsize:(k + 1) * self.batchsize] for k in range(n)]

    # ---------------------------------------------------------------------------------------------------------------
    # the pool

    def _decode(self, indices):
        from ..models.codec_io import read_png
        with ThreadPoolExecutor(min(self.threads, max(1, len(indices)))) as pool:
            return list(pool.map(lambda i: read_png(self.files[i]), indices))

    def _build(self, indices, count):
        where, at = {}, 0
        for i in indices:
            where[i] = at
            at += int(self._bytes[i])
        host = torch.empty(at, dtype=torch.uint8, pin_memory=self.device is not None and self.device.type == "cuda")
        for i, image in zip(indices, self._decode(indices)):
            if image.shape != (int(self._height[i]), int(self._width[i]), 3):
                raise ValueError(f"{self.files[i]} decodes to {tuple(image.shape)}, its header says "
                                 f"{int(self._height[i])} x {int(self._width[i])}")
            host[where[i]:where[i] + image.numel()] = image.reshape(-1)
        return _Slice(count, host, where)

    def _slice_items(self, items):
        """How many whole batches from the head of `items` one pool takes (at least one), and their distinct files."""
        seen, size, count = [], 0, 0
        known = set()
        for k in range(0, len(items) - self.batchsize + 1, self.batchsize):
            fresh = [i for i in dict.fromkeys(it[0] for it in items[k:k + self.batchsize]) if i not in known]
            more = sum(int(self._bytes[i]) for i in fresh)
            if count and size + more > self.pool_limit_bytes:
                break
            seen.extend(fresh)
            known.update(fresh)
            size += more
            count += self.batchsize
        return count, seen

    def _plan_slice(self, skip):
        """The slice that starts `skip` items ahead: (count, files)."""
        # look ahead one pass worth of whole batches; a slice never needs more than every file
        horizon = (len(self.files) // self.batchsize + 1) * self.batchsize
        if not self.repeat:
            horizon = min(horizon, (len(self.files) - self._offset - skip) // self.batchsize * self.batchsize)
        if horizon <= 0:
            return 0, []
        return self._slice_items(self._peek(skip + horizon)[skip:])

    def _current_slice(self):
        if self._fits:
            if self._slice is None:
                self._slice = self._build(list(range(len(self.files))), 0)
                self._upload(self._slice)
            return self._slice
        if self._slice is None or self._slice_left == 0:
            here = (self._pass_no, self._offset)
            if self._next is not None and self._next[1] == here:
                self._slice = self._next[0].result()
            else:
                count, files = self._plan_slice(0)
                self._slice = self._build(files, count)
            self._next = None
            self._upload(self._slice)
            self._slice_left = self._slice.count
            # the run behind this one, decoded while this one is consumed
            count, files = self._plan_slice(self._slice.count)
            if count:
                if self._worker is None:
                    self._worker = ThreadPoolExecutor(1)
                k, at = self._pass_no, self._offset + self._slice.count
                for _, items in self._passes:
                    if at < len(items):
                        break
                    at, k = at - len(items), k + 1
                self._next = (self._worker.submit(self._build, files, count), (k, at))
        return self._slice

    def _upload(self, piece):
        if self.device is None:
            piece.pool = piece.host_pool
        else:
            piece.pool = piece.host_pool.to(self.device, non_blocking=True)
            if self._fits:
                piece.host_pool = None

    # ---------------------------------------------------------------------------------------------------------------
    # iteration

    def __iter__(self):
        if not self.repeat and not self._open:
            self._open = True           # the next pass
        return self

    def __next__(self):
        if not self._open:
            raise StopIteration         # until the next iter()
        if self._batches_left(1) == 0:
            if not self.repeat:
                # one pass is over: drop its remainder
                self._open = False
                if self._passes:
                    self._passes.popleft()
                    self._pass_no += 1
                self._offset = 0
                self._slice_left = 0
                self._next = None
            raise StopIteration
        items = self._peek(self.batchsize)
        piece = self._current_slice()
        batch = self._cut(piece, items)
        self._advance(self.batchsize)
        if not self._fits:
            self._slice_left -= self.batchsize
        return batch

    def close(self):
        """Ends the background decoding thread (started only when the images exceed the pool limit)."""
        self._next = None
        if self._worker is not None:
            self._worker.shutdown(wait=True)
            self._worker = None

    def __del__(self):
        if getattr(self, "_worker", None) is not None:
            self._worker.shutdown(wait=False)

    # ---------------------------------------------------------------------------------------------------------------
    # state

    def state_dict(self):
        """The generator state in front of the current pass and the position within it."""
        state = self._passes[0][0] if self._passes else self._gen.get_state()
        return {"generator": state.clone(), "pass_no": self._pass_no, "offset": self._offset, "open": self._open,
                "seed": self.seed, "num_files": len(self.files), "patchsize": self.patchsize,
                "batchsize": self.batchsize}

    def load_state_dict(self, state):
        for key in ("num_files", "patchsize", "batchsize"):
            mine = len(self.files) if key == "num_files" else getattr(self, key)
            if state[key] != mine:
                raise ValueError(f"the state was saved with {key} = {state[key]}, this dataset has {mine}")
        self._gen.set_state(state["generator"].clone())
        self._passes.clear()
        self._pass_no, self._offset, self._open = int(state["pass_no"]), int(state["offset"]), bool(state["open"])
        self._next = None
        if not self._fits:
            self._slice, self._slice_left = None, 0
