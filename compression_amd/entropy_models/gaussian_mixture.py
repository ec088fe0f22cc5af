"""Entropy model of a discretized Gaussian mixture (Cheng, Sun, Takeuchi, Katto, CVPR 2020): every element has K weights,
K means and K scales, so no table set spans the likelihood and the coder evaluates each element's CDF where it codes it
(ops/mixture_ops.py, csrc/mixture_coder.hip).  The definition is this project's own."""
from __future__ import annotations

import numpy as np
import torch

from ..ops import mixture_ops

__all__ = ["GaussianMixtureEntropyModel"]


class GaussianMixtureEntropyModel:
    """`coding_rank` trailing dimensions of the bottleneck form one coding unit; the parameters `logits`, `loc` and
    `scale` have the bottleneck's shape plus a last dimension of `num_components`.

    Symbols are round(y) (half to even): no mean is subtracted, so the symbol does not depend on the parameters.  A unit
    is cut into streams of `stream_symbols` symbols (one wave of the device codes one stream); its symbols are coded
    inside a window [lo, lo + L - 1] that `compress` returns next to the strings and `decompress` takes back: the
    smallest window holding the unit's symbols where that has at most MAX_WINDOW = 4096 values, else the 4096 values
    starting at max(smallest symbol, -2048).  A value outside the window is coded as the window's nearest end and
    `quantize(y, window)` returns it clamped the same way, so `compress` never fails on a latent.

    Strings decode on the build and device kind that encoded them: the CDF is float32 arithmetic on the device.

    `decode_sanity_check`: `decompress` raises "Sanity check failed." when the decoder's verdict on a stream is bad.
    The verdict is the stream format's own weak check (the reference calls `RangeDecoder::Finalize` one) and one rule
    more: it refuses a string that does not end the way the encoder ends one for the symbols that came out, and an
    empty string wherever the symbols cost a digit.  It cannot refuse a damaged string that happens to be the code of
    other symbols, and most strings that merely lost their last byte are exactly that: the flag
    guards against mismatched parameters or containers, it is no checksum."""

    def __init__(self, num_components, coding_rank, stream_symbols=1024, compression=False,
                 bottleneck_dtype=torch.float32, decode_sanity_check=True):
        if not 1 <= int(num_components) <= mixture_ops.MAX_COMPONENTS:
            raise ValueError(f"num_components must be in [1, {mixture_ops.MAX_COMPONENTS}], got {num_components}")
        if int(coding_rank) < 1:
            raise ValueError(f"coding_rank must be positive, got {coding_rank}")
        if int(stream_symbols) < 1:
            raise ValueError(f"stream_symbols must be positive, got {stream_symbols}")
        self.num_components, self.coding_rank = int(num_components), int(coding_rank)
        self.stream_symbols, self.compression = int(stream_symbols), bool(compression)
        self.bottleneck_dtype, self.decode_sanity_check = bottleneck_dtype, bool(decode_sanity_check)

    # ------------------------------------------------------------------------------------------------------------------
    def _check(self, shape, logits, loc, scale):
        if len(shape) < self.coding_rank:
            raise ValueError(f"the bottleneck must have at least coding_rank = {self.coding_rank} dimensions")
        want = tuple(shape) + (self.num_components,)
        for name, t in (("logits", logits), ("loc", loc), ("scale", scale)):
            if tuple(t.shape) != want:
                raise ValueError(f"{name} must be {list(want)}, received {list(t.shape)}")

    def _unit_shape(self, shape):
        lead = tuple(shape[:len(shape) - self.coding_rank])
        units = int(np.prod(lead, dtype=np.int64)) if lead else 1
        elems = int(np.prod(shape[len(lead):], dtype=np.int64))
        return lead, units, elems

    def streams_per_unit(self, elems):
        return -(-int(elems) // self.stream_symbols)

    def __call__(self, y, logits, loc, scale, training=True, noise=None):
        """(y_hat, bits): training: y_hat = y + uniform noise (`noise` where given); else y_hat = round(y).  bits has
        the shape of the leading dimensions.  The fused kernel on a HIP device, the `NoisyNormalMixture` composition
        elsewhere."""
        self._check(y.shape, logits, loc, scale)
        if training:
            if noise is None:
                noise = torch.rand_like(y) - 0.5
        else:
            y, noise = self.quantize(y), None
        fused = y.is_cuda and y.dtype in (torch.float32, torch.bfloat16) and y.numel() > 0
        fn = mixture_ops.mixture_bits if fused else mixture_ops.mixture_bits_reference
        return fn(y, logits, loc, scale, self.coding_rank, noise=noise)

    @staticmethod
    def quantize(y, window=None):
        """round(y), half to even; with `window` (int [units, 2]: lo, L per unit, as `compress` returns it) clamped to
        each unit's window: the value `decompress` gives back."""
        y_hat = torch.round(y)
        if window is None:
            return y_hat
        window = torch.as_tensor(np.asarray(window, dtype=np.int64)).reshape(-1, 2).to(y.device)
        flat = y_hat.reshape(window.shape[0], -1)
        lo = window[:, :1].to(flat.dtype)
        hi = (window[:, :1] + window[:, 1:] - 1).to(flat.dtype)
        return torch.minimum(torch.maximum(flat, lo), hi).reshape(y.shape)

    @staticmethod
    def choose_window(smallest, largest):
        """(lo, L) for a unit whose symbols span [smallest, largest]."""
        limit, bound = mixture_ops.MAX_WINDOW, mixture_ops.MAX_ABS_LO
        smallest, largest = int(smallest), int(largest)
        if largest - smallest + 1 <= limit:
            lo = smallest
        else:
            lo = max(smallest, -(limit // 2))
        lo = min(max(lo, -bound), bound)
        return lo, min(max(largest - lo + 1, 1), limit)

    def compress(self, y, logits, loc, scale):
        """-> (strings: numpy object array [units * streams_per_unit] of bytes, unit after unit; window: int32 numpy
        [units, 2] holding (lo, L) of every unit)."""
        if not self.compression:
            raise RuntimeError("compress needs compression=True")
        self._check(y.shape, logits, loc, scale)
        _, units, elems = self._unit_shape(y.shape)
        sym = torch.round(y.detach().float()).reshape(units, elems)
        if elems == 0 or units == 0:
            return np.empty(0, dtype=object), np.zeros((units, 2), dtype=np.int32)
        ends = torch.stack([sym.amin(dim=1), sym.amax(dim=1)], dim=1).clamp(-2.0 ** 30, 2.0 ** 30).cpu().numpy()
        window = np.array([self.choose_window(a, b) for a, b in ends], dtype=np.int32).reshape(units, 2)
        sym = sym.clamp(-2.0 ** 30, 2.0 ** 30).to(torch.int32)
        k = self.num_components
        encoded = mixture_ops.mixture_encode(
            sym, logits.reshape(units, elems, k), loc.reshape(units, elems, k), scale.reshape(units, elems, k),
            window[:, 0], window[:, 1], self.stream_symbols)
        strings = np.empty(encoded.offsets.numel() - 1, dtype=object)
        strings[:] = mixture_ops.strings_from_blob(encoded)
        return strings, window

    def decompress(self, strings, window, logits, loc, scale):
        """The strings and the window of `compress` and the same parameters -> y_hat of the parameters' shape without
        its last dimension, `bottleneck_dtype`."""
        if not self.compression:
            raise RuntimeError("decompress needs compression=True")
        shape = tuple(logits.shape[:-1])
        self._check(shape, logits, loc, scale)
        lead, units, elems = self._unit_shape(shape)
        window = np.asarray(window, dtype=np.int64).reshape(-1)
        if window.size != 2 * units:
            raise ValueError(f"the window must hold (lo, L) of {units} unit(s), received {window.size} value(s)")
        window = window.reshape(units, 2)
        strings = np.asarray(strings, dtype=object).reshape(-1)
        want = units * self.streams_per_unit(elems)
        if strings.shape[0] != want:
            raise ValueError(f"{want} strings are needed for {units} unit(s) of {self.streams_per_unit(elems)} "
                             f"stream(s), received {strings.shape[0]}")
        if want == 0:
            return torch.zeros(shape, dtype=self.bottleneck_dtype, device=logits.device)
        k = self.num_components
        sym, ok = mixture_ops.mixture_decode(
            list(strings), logits.reshape(units, elems, k), loc.reshape(units, elems, k),
            scale.reshape(units, elems, k), window[:, 0], window[:, 1], self.stream_symbols)
        if self.decode_sanity_check and not bool(ok.all()):
            raise RuntimeError("Sanity check failed.")
        return sym.reshape(shape).to(self.bottleneck_dtype)
