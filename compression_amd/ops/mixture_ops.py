"""The discretized Gaussian mixture of Cheng, Sun, Takeuchi and Katto (CVPR 2020) as device calls: a fused training
likelihood (csrc/mixture_bits.hip) and a range coder that evaluates every element's CDF where it codes it
(csrc/mixture_coder.hip).  The definition is this project's own.

Every element has K weights (given as logits), K means and K scales; `logits`, `loc` and `scale` carry K as their
last dimension, the batch-shape convention of `distributions.NoisyNormalMixture`.  The kernels read float32 planes
[K, N]; the functions here make them.

The quantised CDF, at precision 16, of a window [lo, lo + L - 1] with 1 <= L <= MAX_WINDOW:

    c_0 = 0     c_L = 65536     c_b = RESERVE b + floor(F(lo + b - 1/2) (65536 - RESERVE L))     for 0 < b < L
    F(t) = sum_k softmax(logits)_k Phi((t - loc_k) / scale_k)

`mixture_cdf_reference` is that definition in float64 on the host; `mixture_cdf` is the table the coder uses, dumped.
Symbols are round(y), half to even; one outside the window is coded as the window's nearest end."""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from .. import _lib

__all__ = ["MixtureStrings", "strings_from_blob", "mixture_bits", "mixture_bits_reference", "mixture_cdf",
           "mixture_cdf_reference", "mixture_encode", "mixture_decode", "mixture_planes", "MIXTURE_CONSTANTS",
           "PRECISION", "RESERVE", "MAX_WINDOW", "MAX_COMPONENTS", "MAX_ABS_LO"]

# the named constants of csrc/mixture_cdf.h
MIXTURE_CONSTANTS = _lib.kernel_constants("mixture_cdf.h", ("MIX",))
PRECISION = MIXTURE_CONSTANTS["MIX_PRECISION"]
RESERVE = MIXTURE_CONSTANTS["MIX_RESERVE"]
MAX_WINDOW = MIXTURE_CONSTANTS["MIX_MAX_WINDOW"]
MAX_COMPONENTS = MIXTURE_CONSTANTS["MIX_MAX_COMPONENTS"]
MAX_ABS_LO = MIXTURE_CONSTANTS["MIX_MAX_ABS_LO"]


# What `mixture_encode` returns: string s is blob[offsets[s]:offsets[s + 1]]; `overflow` (one int32 on the device) is 0
# unless a stream outgrew its slab, an internal error that `strings_from_blob` raises for.
MixtureStrings = collections.namedtuple("MixtureStrings", ["blob", "offsets", "overflow"])


def _check_window(lo, length):
    if not 1 <= int(length) <= MAX_WINDOW:
        raise ValueError(f"L must be in [1, {MAX_WINDOW}], got {length}")
    if abs(int(lo)) > MAX_ABS_LO:
        raise ValueError(f"lo must be in [-{MAX_ABS_LO}, {MAX_ABS_LO}], got {lo}")


def _check_parameters(logits, loc, scale, shape=None):
    if not (logits.shape == loc.shape == scale.shape) or logits.dim() < 1:
        raise ValueError(f"logits, loc and scale must share one shape [..., K], received {tuple(logits.shape)}, "
                         f"{tuple(loc.shape)} and {tuple(scale.shape)}")
    k = int(logits.shape[-1])
    if not 1 <= k <= MAX_COMPONENTS:
        raise ValueError(f"the number of components K must be in [1, {MAX_COMPONENTS}], got {k}")
    if shape is not None and tuple(logits.shape[:-1]) != tuple(shape):
        raise ValueError(f"the parameters must be {list(shape)} + [K], received {list(logits.shape)}")
    return k


def mixture_cdf_reference(logits, loc, scale, lo, L):
    """The quantised CDF in float64 on the host -> int32 numpy [N, L + 1] for parameters [N, K] (any leading shape is
    flattened).  The parameters are taken at the values given (float32 inputs are widened, not re-derived)."""
    _check_window(lo, L)
    logits, loc, scale = (torch.as_tensor(t).detach().cpu().to(torch.float64) for t in (logits, loc, scale))
    k = _check_parameters(logits, loc, scale)
    logits, loc, scale = (t.reshape(-1, k) for t in (logits, loc, scale))
    lo, L = int(lo), int(L)
    w = torch.softmax(logits, dim=-1)
    t = torch.arange(L + 1, dtype=torch.float64) + (lo - 0.5)                     # [L + 1]
    z = (t[None, :, None] - loc[:, None, :]) / scale[:, None, :]                  # [N, L + 1, K]
    big_f = (w[:, None, :] * (0.5 * torch.erfc(-z * math.sqrt(0.5)))).sum(-1).clamp(0.0, 1.0)
    b = torch.arange(L + 1, dtype=torch.int64)
    c = RESERVE * b[None] + torch.floor(big_f * float((1 << PRECISION) - RESERVE * L)).to(torch.int64)
    c[:, 0] = 0
    c[:, L] = 1 << PRECISION
    return c.to(torch.int32).numpy()


def mixture_planes(t):
    """[..., K] -> float32 planes [K, N], contiguous: what the kernels read."""
    return t.detach().to(torch.float32).reshape(-1, t.shape[-1]).t().contiguous()


def mixture_cdf(logits, loc, scale, lo, L):
    """The table the coder uses for parameters [..., K] on the device -> int32 device tensor [N, L + 1]."""
    device = _lib.require_device()
    _check_window(lo, L)
    k = _check_parameters(logits, loc, scale)
    pl, pm, ps = (mixture_planes(t.to(device)) for t in (logits, loc, scale))
    n = pl.shape[1]
    out = torch.empty(n, int(L) + 1, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().tfc_mixture_cdf(pl.data_ptr(), pm.data_ptr(), ps.data_ptr(), k, n, int(lo), int(L),
                                          out.data_ptr(), _lib.stream_ptr()))
    return out


def _windows(lo, L, batch, device):
    lo = torch.as_tensor(lo, dtype=torch.int64).reshape(-1).expand(batch) if np.ndim(lo) == 0 else \
        torch.as_tensor(lo, dtype=torch.int64).reshape(-1)
    L = torch.as_tensor(L, dtype=torch.int64).reshape(-1).expand(batch) if np.ndim(L) == 0 else \
        torch.as_tensor(L, dtype=torch.int64).reshape(-1)
    if lo.numel() != batch or L.numel() != batch:
        raise ValueError(f"lo and L must be scalars or hold one value per batch entry ({batch})")
    for a, b in zip(lo.tolist(), L.tolist()):
        _check_window(a, b)
    return lo.to(device, torch.int32).contiguous(), L.to(device, torch.int32).contiguous()


def _stream_layout(batch, elems, stream_symbols):
    stream_symbols = int(stream_symbols)
    if stream_symbols < 1:
        raise ValueError(f"stream_symbols must be positive, got {stream_symbols}")
    return stream_symbols, -(-elems // stream_symbols) if elems else 0


def mixture_encode(symbols, logits, loc, scale, lo, L, stream_symbols):
    """symbols int [B, E] (absolute values), parameters [B, E, K], lo and L scalars or one per batch entry.  Each batch
    entry is cut into ceil(E / stream_symbols) streams, the last one shorter where it has to be.
    -> MixtureStrings(blob uint8 device, offsets int64 device [streams + 1], overflow): string s is
    blob[offsets[s]:offsets[s + 1]], streams in the order (batch entry, stream).  One launch for the coding, no host
    synchronisation."""
    device = _lib.require_device()
    if symbols.dim() != 2:
        raise ValueError(f"symbols must be [B, E], received shape {tuple(symbols.shape)}")
    batch, elems = (int(s) for s in symbols.shape)
    k = _check_parameters(logits, loc, scale, symbols.shape)
    stream_symbols, per_entry = _stream_layout(batch, elems, stream_symbols)
    lo_d, len_d = _windows(lo, L, batch, device)
    sym = symbols.to(device, torch.int32).contiguous()
    pl, pm, ps = (mixture_planes(t.to(device)) for t in (logits, loc, scale))
    cap = _lib.lib().tfc_mixture_blob_capacity(batch, elems, stream_symbols)
    if cap < 0:
        raise ValueError(_lib.last_error())
    blob = torch.empty(max(int(cap), 1), dtype=torch.uint8, device=device)
    offsets = torch.empty(batch * per_entry + 1, dtype=torch.int64, device=device)
    overflow = torch.empty(1, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().tfc_mixture_encode(
        sym.data_ptr(), pl.data_ptr(), pm.data_ptr(), ps.data_ptr(), k, batch, elems, stream_symbols,
        lo_d.data_ptr(), len_d.data_ptr(), blob.data_ptr(), offsets.data_ptr(), overflow.data_ptr(),
        _lib.stream_ptr()))
    return MixtureStrings(blob, offsets, overflow)


def strings_from_blob(encoded):
    """What `mixture_encode` returned -> list of bytes (one host synchronisation)."""
    off = encoded.offsets.cpu().numpy()
    data = encoded.blob[:int(off[-1])].cpu().numpy().tobytes()
    if int(encoded.overflow.item()):
        raise RuntimeError("internal error: a mixture stream outgrew its slab")
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def mixture_decode(strings, logits, loc, scale, lo, L, stream_symbols, stream_index=None):
    """The inverse of `mixture_encode`: `strings` is a sequence of bytes, what `mixture_encode` returned or a (device
    blob, device offsets) pair; parameters [B, E, K].  `stream_index` (one int per string, no stream twice) names the
    stream each string is, in the order of `mixture_encode`; None: all of them in order.
    -> (symbols int32 device [B, E], ok uint8 device [strings]); the
    elements of streams that were not decoded are 0.  Whatever the bytes are, a decoded symbol is inside its window and
    the call returns; `ok` is 0 for a string that does not end the way the encoder ends one."""
    device = _lib.require_device()
    k = _check_parameters(logits, loc, scale)
    if logits.dim() != 3:
        raise ValueError(f"the parameters must be [B, E, K], received shape {tuple(logits.shape)}")
    batch, elems = int(logits.shape[0]), int(logits.shape[1])
    stream_symbols, per_entry = _stream_layout(batch, elems, stream_symbols)
    lo_d, len_d = _windows(lo, L, batch, device)
    if isinstance(strings, tuple) and len(strings) in (2, 3) and isinstance(strings[0], torch.Tensor):
        blob, offsets = strings[0].to(device).contiguous(), strings[1].to(device, torch.int64).contiguous()
        count = offsets.numel() - 1
    else:
        strings = [bytes(s) for s in strings]
        count = len(strings)
        off_h = np.zeros(count + 1, dtype=np.int64)
        np.cumsum([len(s) for s in strings], out=off_h[1:])
        blob_h = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
        blob = torch.from_numpy(blob_h).to(device)
        offsets = torch.from_numpy(off_h).to(device)
    if blob.numel() == 0:
        blob = torch.zeros(1, dtype=torch.uint8, device=device)
    index_d = None
    if stream_index is not None:
        index_d = torch.as_tensor(stream_index, dtype=torch.int64).reshape(-1)
        if index_d.numel() != count:
            raise ValueError(f"stream_index names {index_d.numel()} streams for {count} strings")
        if count and (int(index_d.min()) < 0 or int(index_d.max()) >= batch * per_entry):
            raise ValueError(f"stream_index must be in [0, {batch * per_entry})")
        if torch.unique(index_d).numel() != count:
            # two waves would write the same elements of the output, whichever came last
            raise ValueError("stream_index names a stream more than once")
        index_d = index_d.to(device, torch.int32).contiguous()
    elif count != batch * per_entry:
        raise ValueError(f"{batch * per_entry} strings are needed for {batch} batch entries of {per_entry} streams, "
                         f"received {count}")
    pl, pm, ps = (mixture_planes(t.to(device)) for t in (logits, loc, scale))
    out = torch.zeros(batch, elems, dtype=torch.int32, device=device)
    ok = torch.zeros(count, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().tfc_mixture_decode(
        blob.data_ptr(), offsets.data_ptr(), _lib.ptr(index_d), count, pl.data_ptr(), pm.data_ptr(), ps.data_ptr(), k,
        batch, elems, stream_symbols, lo_d.data_ptr(), len_d.data_ptr(), out.data_ptr(), ok.data_ptr(),
        _lib.stream_ptr()))
    return out, ok


class _MixtureBits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, noise, logits, loc, scale, units, elems):
        _lib.require_device()
        y = y.contiguous()
        k = int(logits.shape[-1])
        planes = tuple(mixture_planes(t) for t in (logits, loc, scale))
        y_hat = torch.empty_like(y)
        bits = torch.empty(units, dtype=torch.float32, device=y.device)
        _lib.check(_lib.lib().tfc_mixture_bits_forward(
            y.data_ptr(), _lib.ptr(noise), planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), k,
            y_hat.data_ptr(), _lib.DTYPE_CODE[y.dtype], units, elems, bits.data_ptr(), _lib.stream_ptr()))
        ctx.save_for_backward(y_hat, *planes)
        ctx.meta = (units, elems, k, tuple(logits.shape), (logits.dtype, loc.dtype, scale.dtype))
        return y_hat, bits

    @staticmethod
    def backward(ctx, g_yhat, g_bits):
        y_hat, pl, pm, ps = ctx.saved_tensors
        units, elems, k, shape, dtypes = ctx.meta
        dy = torch.empty_like(y_hat)
        grads = [torch.empty_like(pl) for _ in range(3)]
        gb = (g_bits if g_bits is not None else torch.zeros(units, device=y_hat.device)).to(torch.float32).contiguous()
        _lib.check(_lib.lib().tfc_mixture_bits_backward(
            y_hat.data_ptr(), pl.data_ptr(), pm.data_ptr(), ps.data_ptr(), k, _lib.DTYPE_CODE[y_hat.dtype], units,
            elems, gb.data_ptr(), dy.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(),
            _lib.stream_ptr()))
        if g_yhat is not None:
            dy = dy + g_yhat
        dl, dm, ds = (g.t().reshape(shape).to(d) for g, d in zip(grads, dtypes))
        return dy, None, dl, dm, ds, None, None


def mixture_bits(y, logits, loc, scale, coding_rank, noise=None):
    """(y_hat, bits) of the noisy Gaussian mixture, fused (csrc/mixture_bits.hip): y_hat = y + noise (noise None: y
    itself), bits summed over the last `coding_rank` dimensions of y in a fixed order, shape = the leading dimensions.
    y float32 or bfloat16 on the device; logits, loc, scale [*y.shape, K], differentiable."""
    if y.dtype not in _lib.DTYPE_CODE:
        raise TypeError(f"y must be float32 or bfloat16, got {y.dtype}")
    _check_parameters(logits, loc, scale, y.shape)
    if not 1 <= coding_rank <= y.dim():
        raise ValueError(f"coding_rank must be in [1, {y.dim()}], got {coding_rank}")
    lead = y.shape[:y.dim() - coding_rank]
    units = 1
    for s in lead:
        units *= int(s)
    elems = y.numel() // max(units, 1)
    if noise is not None:
        noise = noise.to(y.dtype).contiguous()
    y_hat, bits = _MixtureBits.apply(y, noise, logits, loc, scale, units, elems)
    return y_hat, bits.reshape(lead)


def mixture_bits_reference(y, logits, loc, scale, coding_rank, noise=None):
    """The same through `distributions.NoisyNormalMixture` (tensor ops, any device): the path a CPU tensor takes."""
    from ..distributions import uniform_noise
    y_hat = y if noise is None else y + noise.to(y.dtype)
    prior = uniform_noise.NoisyNormalMixture(loc=loc, scale=scale, weight=torch.softmax(logits, dim=-1))
    log_prob = prior.log_prob(y_hat.to(loc.dtype))
    axes = tuple(range(y.dim() - coding_rank, y.dim()))
    return y_hat, log_prob.sum(dim=axes) / -math.log(2.0)
