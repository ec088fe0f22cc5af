"""Random clips of '.y4m' files, the training input of the video model (models/ssf2020.py): `clip_length` consecutive
frames of one file, one random crop per clip (the same window in every frame), batched.

The frames come through `Y4MDataset` and `ycbcr_to_rgb` once per file and stay resident (uint8 RGB, on `device` when
one is given); a batch is cut from them with plain tensor ops.  One CPU `torch.Generator` (seeded with `seed`) decides
everything: each item draws its file, its first frame, `top` and `left`, in that order.  The stream has no end."""
from __future__ import annotations

import glob as _glob
import os

import torch

from ..ops import video_ops
from .y4m_dataset import Y4MDataset

__all__ = ["ClipDataset"]


class ClipDataset:
    """`ClipDataset(filenames, clip_length=3, patchsize=256, batch_size=8, device=None, seed=0)` iterates batches
    [batch_size, clip_length, patchsize, patchsize, 3] float32 holding the integers 0...255.  `filenames`: a glob or a
    sequence of paths.  `device=None`: everything on the CPU, through the conversion's tensor-op twin."""

    def __init__(self, filenames, clip_length=3, patchsize=256, batch_size=8, device=None, seed=0):
        if isinstance(filenames, (str, os.PathLike)):
            files = sorted(_glob.glob(os.fspath(filenames)))
            if not files:
                raise RuntimeError(f"No training clips found with glob '{os.fspath(filenames)}'.")
        else:
            files = [os.fspath(f) for f in filenames]
            if not files:
                raise RuntimeError("No training clips found: the list of files is empty.")
        self.files = files
        self.clip_length, self.patchsize, self.batch_size = int(clip_length), int(patchsize), int(batch_size)
        if self.clip_length < 1 or self.patchsize < 1 or self.batch_size < 1:
            raise ValueError(f"clip_length, patchsize and batch_size must be positive, got {clip_length}, {patchsize} "
                             f"and {batch_size}")
        self.device = None if device is None else torch.device(device)
        self.seed = int(seed)
        self._frames = [self._read(name) for name in files]
        for name, frames in zip(files, self._frames):
            t, h, w, _ = frames.shape
            if t < self.clip_length:
                raise ValueError(f"{name} holds {t} frames, fewer than the {self.clip_length} of a clip")
            if h < self.patchsize or w < self.patchsize:
                raise ValueError(f"{name} is {h} x {w}, smaller than the {self.patchsize} x {self.patchsize} patch")
        self._gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self._delivered = 0

    def _read(self, name):
        on_device = self.device is not None and self.device.type == "cuda"
        parts = [video_ops.ycbcr_to_rgb(y, cbcr)
                 for y, cbcr in Y4MDataset(name, device=self.device if on_device else None).batches(8)]
        if not parts:
            raise ValueError(f"Input file '{name}' holds no frame")
        return torch.cat(parts)

    def _draw(self):
        """The next item: (file index, first frame, top, left)."""
        r = torch.randint(0, 2 ** 62, (4,), generator=self._gen).tolist()
        f = r[0] % len(self.files)
        t, h, w, _ = self._frames[f].shape
        return f, r[1] % (t - self.clip_length + 1), r[2] % (h - self.patchsize + 1), r[3] % (w - self.patchsize + 1)

    def plan(self, num_batches):
        """The (file index, first frame, top, left) items of the next `num_batches` batches; consumes nothing."""
        state = self._gen.get_state()
        out = [[self._draw() for _ in range(self.batch_size)] for _ in range(int(num_batches))]
        self._gen.set_state(state)
        return out

    def __iter__(self):
        return self

    def __next__(self):
        p, clips = self.patchsize, []
        for f, first, top, left in (self._draw() for _ in range(self.batch_size)):
            clips.append(self._frames[f][first:first + self.clip_length, top:top + p, left:left + p])
        self._delivered += 1
        return torch.stack(clips).to(torch.float32)

    def state_dict(self):
        return {"generator": self._gen.get_state().clone(), "delivered": self._delivered, "seed": self.seed,
                "num_files": len(self.files), "clip_length": self.clip_length, "patchsize": self.patchsize,
                "batch_size": self.batch_size}

    def load_state_dict(self, state):
        for key in ("num_files", "clip_length", "patchsize", "batch_size"):
            mine = len(self.files) if key == "num_files" else getattr(self, key)
            if state[key] != mine:
                raise ValueError(f"the state was saved with {key} = {state[key]}, this dataset has {mine}")
        self._gen.set_state(state["generator"].clone())
        self._delivered = int(state["delivered"])
