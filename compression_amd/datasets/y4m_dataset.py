"""Y'CbCr video frames from and to '.y4m' (YUV4MPEG2) files.

`Y4MDataset` mirrors python/datasets/y4m_dataset.py and restates the semantics of its op
(cc/kernels/y4m_dataset_kernels.cc:125-406): the header is read in 256-byte chunks up to the first newline, its
parameters may come in any order, `C420jpeg`, `C420` and `C444` progressive material is accepted and everything else
refused with the reference's messages (as ValueError), every frame starts with exactly `FRAME\\n`, a clean end of file
moves on to the next file, and the iterator's state is (file_index, file_pos) with file_pos = -1 for "no file open".

What differs is the shape of the work.  The reference is a CPU source that reads one frame per call and de-interleaves
it one byte at a time.  Here a read covers up to `frames_per_read` whole frames, markers included, and
  * with device=None the planes are split with numpy (the definition the kernel is tested against);
  * with a HIP device the read goes into one of two pinned buffers, one asynchronous copy takes it to the device and
    `ops.video_ops.unpack_frames` (one kernel) splits it there.  A pinned buffer is refilled only after the event
    recorded behind its copy has completed.
`Y4MWriter` is the inverse (the reference has none), so that reconstructions can be written back."""
from __future__ import annotations

import os

import numpy as np
import torch

from ..ops import video_ops

__all__ = ["Y4MDataset", "Y4MWriter"]

FRAME_MARKER = b"FRAME\n"
HEADER_CHUNK = 256
_DIGITS = b"0123456789"


def _fail(name, rest):
    return ValueError(f"Input file '{name}' {rest}")


def read_header(f, name):
    """The bytes up to and including the first newline, read in chunks of HEADER_CHUNK."""
    header = b""
    while True:
        f.seek(len(header))
        chunk = f.read(HEADER_CHUNK)
        pos = chunk.find(b"\n")
        if pos >= 0:
            return header + chunk[:pos + 1]
        if len(chunk) < HEADER_CHUNK:
            raise _fail(name, "does not contain a complete Y4M header.")
        header += chunk


def _leading_number(rest):
    end = 0
    while end < len(rest) and rest[end] in _DIGITS:
        end += 1
    text = rest[:end]
    value = int(text) if text and int(text) < 2 ** 63 else 0
    return text.decode("latin-1"), value, rest[end:]


def parse_header(header, name):
    """-> (width, height, chroma) with chroma "420" or "444"; `header` ends with its newline."""
    rest = header[:-1]
    if not rest.startswith(b"YUV4MPEG2"):
        raise _fail(name, "does not have a YUV4MPEG2 marker.")
    rest = rest[len(b"YUV4MPEG2"):]
    width = height = 0
    chroma = None
    while rest:
        if len(rest) < 2 or rest[:1] != b" ":
            raise _fail(name, f"has an invalid Y4M header. Remaining header: '{rest.decode('latin-1')}'.")
        key, rest = rest[1:2], rest[2:]
        if key == b"W":
            text, width, rest = _leading_number(rest)
            if width <= 0:
                raise _fail(name, f"has an invalid width specifier '{text}'.")
        elif key == b"H":
            text, height, rest = _leading_number(rest)
            if height <= 0:
                raise _fail(name, f"has an invalid height specifier '{text}'.")
        elif key == b"C":
            for prefix, found in ((b"420jpeg", "420"), (b"420", "420"), (b"444", "444")):
                if rest.startswith(prefix):
                    chroma, rest = found, rest[len(prefix):]
                    break
            else:
                text = rest.split(b" ", 1)[0].decode("latin-1")
                raise _fail(name, f"has an unsupported chroma format '{text}'.")
        elif key == b"I":
            if not rest.startswith(b"p"):
                raise _fail(name, "is not in progressive format.")
            rest = rest[1:]
        else:
            pos = rest.find(b" ")
            rest = b"" if pos < 0 else rest[pos:]
    if not width:
        raise _fail(name, "has no width specifier.")
    if not height:
        raise _fail(name, "has no height specifier.")
    if chroma is None:
        raise _fail(name, "has no chroma format specifier.")
    if chroma == "420" and (width & 1 or height & 1):
        raise _fail(name, "has 4:2:0 chroma format, but odd width or height.")
    return width, height, chroma


def _as_filenames(filenames):
    if isinstance(filenames, (str, bytes, os.PathLike)):
        return [os.fspath(filenames)]
    if isinstance(filenames, np.ndarray):
        if filenames.ndim > 1:
            raise ValueError("`filenames` must be a scalar or a vector.")
        filenames = filenames.reshape(-1).tolist()
    try:
        names = list(filenames)
    except TypeError:
        raise ValueError("`filenames` must be a scalar or a vector.") from None
    if not all(isinstance(n, (str, bytes, os.PathLike)) for n in names):
        raise ValueError("`filenames` must be a scalar or a vector.")
    return [os.fspath(n) for n in names]


class Y4MIterator:
    """Frames of the dataset's files in order.  `state_dict()` is what `Y4MDataset.iterator(state)` resumes from."""

    def __init__(self, dataset, state=None):
        self._ds = dataset
        self._file = None
        self._file_index = 0
        self._file_pos = -1             # where the next read starts
        self._group = None              # (y, cbcr) of the last read
        self._group_at = 0              # frames of it already yielded
        self._pinned = [None, None]
        self._events = [None, None]
        self._turn = 0
        self._host = None
        if state is not None:
            self._file_index = int(state["file_index"])
            pos = int(state["file_pos"])
            if pos >= 0:
                self._open()
                self._file_pos = pos

    def __iter__(self):
        return self

    def __del__(self):
        self._close()

    def _close(self):
        if self._file is not None:
            self._file.close()
            self._file = None

    def _name(self):
        return self._ds.filenames[self._file_index]

    def _open(self):
        name = self._name()
        self._file = open(name, "rb", buffering=0)
        try:
            header = read_header(self._file, name)
            self._width, self._height, self._chroma = parse_header(header, name)
        except ValueError:
            self._close()
            raise
        self._frame_bytes = video_ops.frame_bytes(self._width, self._height, self._chroma)
        self._stride = len(FRAME_MARKER) + self._frame_bytes
        self._file_pos = len(header)

    def state_dict(self):
        if self._file is None:
            return {"file_index": self._file_index, "file_pos": -1}
        pos = self._file_pos
        if self._group is not None:      # frames read ahead count as unread
            pos -= (self._group[0].shape[0] - self._group_at) * self._stride
        return {"file_index": self._file_index, "file_pos": pos}

    # ---- one read ----

    def _buffer(self, nbytes):
        """-> (uint8 numpy view of nbytes to read into, the tensor behind it or None)."""
        if self._ds.device is None:
            if self._host is None or self._host.size < nbytes:
                self._host = np.empty(nbytes, np.uint8)
            return self._host[:nbytes], None
        turn = self._turn
        self._turn ^= 1
        if self._events[turn] is not None:
            self._events[turn].synchronize()     # the copy out of this buffer has completed
            self._events[turn] = None
        if self._pinned[turn] is None or self._pinned[turn].numel() < nbytes:
            self._pinned[turn] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._pinned[turn].numpy()[:nbytes], (turn, self._pinned[turn])

    def _read_frames(self, limit):
        """Up to `limit` frames of the open file in one read -> (y [k, H, W, 1], cbcr [k, h, w, 2]) with k >= 1, or
        None at a clean end of the file."""
        name, stride, pos = self._name(), self._stride, self._file_pos
        view, pinned = self._buffer(limit * stride)
        self._file.seek(pos)
        got = 0
        while got < view.size:              # a raw file may return less than asked for
            more = self._file.readinto(memoryview(view)[got:])
            if not more:
                break
            got += more
        k = got // stride
        if k == 0:
            if got == 0:
                return None
            raise _fail(name, f"has an incomplete or unsupported frame at byte {pos}. Expected to read {stride} "
                              f"bytes, only {got} were available.")
        frames = view[:k * stride].reshape(k, stride)
        good = (frames[:, :len(FRAME_MARKER)] == np.frombuffer(FRAME_MARKER, np.uint8)).all(axis=1)
        if not good.all():
            k = int(np.argmin(good))        # the frames in front of the first bad marker are still delivered
            if k == 0:
                raise _fail(name, f"has a FRAME marker at byte {pos} which is either invalid or has unsupported "
                                  "frame parameters.")
            frames = frames[:k]
        self._file_pos = pos + k * stride
        width, height, chroma = self._width, self._height, self._chroma
        if pinned is None:
            ys = width * height
            cs = (self._frame_bytes - ys) // 2
            body = frames[:, len(FRAME_MARKER):]
            y = body[:, :ys].reshape(k, height, width, 1).copy()
            cbcr = np.stack([body[:, ys:ys + cs], body[:, ys + cs:]], axis=-1)
            cbcr = cbcr.reshape(k, (height // 2 if chroma == "420" else height), -1, 2)
            return torch.from_numpy(y), torch.from_numpy(np.ascontiguousarray(cbcr))
        turn, buf = pinned
        with torch.cuda.device(self._ds.device):
            raw = torch.empty(k * stride, dtype=torch.uint8, device=self._ds.device)
            raw.copy_(buf[:k * stride], non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            self._events[turn] = event
            return video_ops.unpack_frames(raw, k, width, height, chroma, frame_stride=stride,
                                           first_offset=len(FRAME_MARKER))

    def next_group(self, limit):
        """The next up to `limit` frames, all of one file -> (y, cbcr, file_index); raises StopIteration at the end."""
        if self._group is not None:
            y, cbcr = self._group
            at, end = self._group_at, min(self._group_at + limit, self._group[0].shape[0])
            self._group_at = end
            if end == y.shape[0]:
                self._group = None
            return y[at:end], cbcr[at:end], self._file_index
        while True:
            if self._file is not None:
                group = self._read_frames(limit)
                if group is not None:
                    return group[0], group[1], self._file_index
                self._close()
                self._file_index += 1
            if self._file_index >= len(self._ds.filenames):
                raise StopIteration
            self._open()

    def __next__(self):
        if self._group is None:
            y, cbcr, _ = self.next_group(self._ds.frames_per_read)
            self._group, self._group_at = (y, cbcr), 0
        y, cbcr = self._group
        at = self._group_at
        self._group_at += 1
        if self._group_at == y.shape[0]:
            self._group = None
        return y[at], cbcr[at]


class Y4MDataset:
    """Frames of '.y4m' files as (y, cbcr) uint8 tensors: y [H, W, 1], cbcr [H/2, W/2, 2] for 4:2:0 (`C420jpeg`,
    `C420`) or [H, W, 2] for 4:4:4 (`C444`); all files in order as one sequence.  Other chroma formats and interlaced
    material are refused; other header parameters are ignored.

    filenames: a path or a sequence of paths.  device: None for CPU tensors, or a HIP device, where `frames_per_read`
    frames go to the device in one copy and are split by one kernel (the frames yielded are views of that batch)."""

    def __init__(self, filenames, device=None, frames_per_read=8):
        self.filenames = _as_filenames(filenames)
        if int(frames_per_read) < 1:
            raise ValueError(f"frames_per_read must be positive, got {frames_per_read}")
        self.frames_per_read = int(frames_per_read)
        self.device = None
        if device is not None:
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError(f"device must be None or a HIP device, got {device}")
            if not torch.cuda.is_available():
                raise RuntimeError("Y4MDataset(device=...) needs a HIP device: torch.cuda.is_available() is False")
            self.device = device

    def __iter__(self):
        return self.iterator()

    def iterator(self, state=None):
        """A fresh iterator, or one that resumes where `state` (an iterator's `state_dict()`) was taken: the header of
        file `file_index` is read again and frames continue at byte `file_pos`."""
        return Y4MIterator(self, state)

    def batches(self, n, drop_remainder=False):
        """Yields (y [k, H, W, 1], cbcr [k, h, w, 2]) with k <= n (k == n with drop_remainder).  A batch never spans
        two files: their frame sizes may differ.  Each batch is one read (and one copy and one kernel)."""
        if int(n) < 1:
            raise ValueError(f"the batch size must be positive, got {n}")
        it = self.iterator()
        while True:
            try:
                y, cbcr, _ = it.next_group(int(n))
            except StopIteration:
                return
            if drop_remainder and y.shape[0] < n:
                continue
            yield y, cbcr


class Y4MWriter:
    """Writes frames as a '.y4m' file that `Y4MDataset` reads back identically:

        with Y4MWriter("out.y4m", width, height, chroma="420jpeg") as w:
            w.write(*rgb_to_ycbcr(reconstruction))

    `write` takes one frame (y [H, W, 1], cbcr [h, w, 2]) or a batch, uint8, on the CPU or on a device; device
    frames are laid out by `ops.video_ops.pack_frames` and leave the device in one copy per call."""

    def __init__(self, filename, width, height, chroma="420jpeg", frame_rate=(30, 1)):
        if chroma not in ("420jpeg", "444"):
            raise ValueError(f"chroma must be '420jpeg' or '444', got {chroma!r}")
        self.width, self.height, self.chroma = int(width), int(height), chroma
        self._frame_bytes = video_ops.frame_bytes(self.width, self.height, chroma)
        num, den = (int(v) for v in frame_rate)
        if num < 1 or den < 1:
            raise ValueError(f"frame_rate must be a pair of positive integers, got {frame_rate!r}")
        self._file = open(filename, "wb")
        self._file.write(f"YUV4MPEG2 W{self.width} H{self.height} F{num}:{den} Ip C{chroma}\n".encode())

    def write(self, y, cbcr):
        if self._file is None:
            raise ValueError("write to a closed Y4MWriter")
        y, cbcr, n, height, width, code, _ = video_ops.check_planes(y, cbcr, "Y4MWriter.write")
        if (width, height) != (self.width, self.height) or code != (444 if self.chroma == "444" else 420):
            raise ValueError(f"frames of y {tuple(y.shape)} and cbcr {tuple(cbcr.shape)} do not fit a {self.width} x "
                             f"{self.height} file of {self.chroma} chroma")
        if n == 0:
            return
        mark = len(FRAME_MARKER)
        stride = mark + self._frame_bytes
        packed = video_ops.pack_frames(y, cbcr, frame_stride=stride, first_offset=mark)
        host = packed.cpu().numpy()
        frames = host[:n * stride].reshape(n, stride)
        # pack_frames put frame k's planes behind byte mark + k stride: its marker goes in front of them
        frames[:, :mark] = np.frombuffer(FRAME_MARKER, np.uint8)
        self._file.write(frames.tobytes())

    def close(self):
        if self._file is not None:
            self._file.close()
            self._file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
