"""Entropy-constrained vector quantisation: the one operation the toy-source VECVQ model spends its time in
(models/toy_sources/vecvq.py:53-71 with the distortion of compression_model.py:88-95).

    dist[n, k]    = s sum_d (x[n, d] - c[k, d])^2,   s = 1 ("sse") or 1 / D ("mse")
    index[n]      = argmin_k (rates[k] + lmbda dist[n, k]),  ties to the lowest k
    rate[n]       = rates[index[n]]
    distortion[n] = dist[n, index[n]]

`ecvq_assign` runs tfc_vecvq_assign / tfc_vecvq_backward (csrc/vecvq.hip): the [N, K] cost matrix is never written, and
the gradients for codebook, rates and x are a gather in a fixed order (bit-identical from call to call).
`ecvq_assign_reference` is the same definition as tensor ops, chunked over N; CPU tensors take it."""
from __future__ import annotations

import math

import torch

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["ecvq_assign", "ecvq_counts", "ecvq_assign_reference", "VQ_CONSTANTS"]

DISTORTION_CODE = {"sse": 0, "mse": 1}
REFERENCE_CHUNK_ROWS = 1024     # rows of the cost matrix `ecvq_assign_reference` holds at a time, at most
REFERENCE_CHUNK_ELEMENTS = 1 << 24   # and elements of the [rows, K, D] difference it is summed from, at most


# the named constants of csrc/vecvq_params.h (tile sizes, the narrow / wide boundary)
VQ_CONSTANTS = _lib.kernel_constants("vecvq_params.h", ("VQ",))


def _check_args(x, codebook, rates, lmbda, distortion, dtypes):
    if distortion not in DISTORTION_CODE:
        raise ValueError(f"distortion must be 'sse' or 'mse', got {distortion!r}")
    for name, t in (("x", x), ("codebook", codebook), ("rates", rates)):
        if t.dtype not in dtypes:
            raise TypeError(f"ecvq_assign supports {' and '.join(str(d) for d in dtypes)}, got {name} of {t.dtype}")
        if t.dtype != x.dtype:
            raise TypeError(f"x, codebook and rates must share a dtype, got x of {x.dtype} and {name} of {t.dtype}")
    if codebook.dim() != 2 or codebook.shape[0] < 1 or codebook.shape[1] < 1:
        raise ValueError(f"codebook must be [K, D] with K, D >= 1, received shape {tuple(codebook.shape)}")
    if x.dim() < 1 or x.shape[-1] != codebook.shape[1]:
        raise ValueError(f"x must be [..., {codebook.shape[1]}] to match the codebook, received shape {tuple(x.shape)}")
    if tuple(rates.shape) != (codebook.shape[0],):
        raise ValueError(f"rates must be [{codebook.shape[0]}], received shape {tuple(rates.shape)}")
    if not math.isfinite(float(lmbda)):
        raise ValueError(f"lmbda must be finite, got {lmbda}")


def ecvq_assign_reference(x, codebook, rates, lmbda, distortion="sse", indexes=None):
    """The definition as differentiable tensor ops in float32 (a float64 input stays float64), over at most
    `REFERENCE_CHUNK_ROWS` rows of the cost matrix (and `REFERENCE_CHUNK_ELEMENTS` of the differences) at a time
    -> (indexes int32, rate, distortion), shaped as x without its last axis.  With `indexes` given the arg-min is
    skipped and those codewords are used (what a checker needs to compare gradients under one assignment)."""
    _check_args(x, codebook, rates, lmbda, distortion, (torch.float32, torch.float64))
    ft = torch.float64 if x.dtype == torch.float64 else torch.float32
    k, d = codebook.shape
    scale = 1.0 / d if distortion == "mse" else 1.0
    batch = x.shape[:-1]
    xf, c, r = x.reshape(-1, d).to(ft), codebook.to(ft), rates.to(ft)
    if indexes is None:
        found = []
        with torch.no_grad():
            step = max(1, min(REFERENCE_CHUNK_ROWS, REFERENCE_CHUNK_ELEMENTS // (k * d)))
            for at in range(0, xf.shape[0], step):
                rows = xf[at:at + step]
                cost = r + float(lmbda) * scale * ((rows[:, None, :] - c[None, :, :]) ** 2).sum(dim=-1)
                # torch.argmin does not promise the first of equal minima: take the lowest index among them
                low = cost.min(dim=-1, keepdim=True).values
                ids = torch.arange(k, device=cost.device).expand_as(cost)
                found.append(torch.where(cost == low, ids, k).min(dim=-1).values.clamp(max=k - 1))
        idx = torch.cat(found) if found else torch.zeros(0, dtype=torch.int64, device=xf.device)
    else:
        idx = indexes.reshape(-1).to(xf.device, torch.int64)
        if idx.shape[0] != xf.shape[0]:
            raise ValueError("indexes must have the shape of x without its last axis")
    rate = r[idx]
    dist = scale * ((xf - c[idx]) ** 2).sum(dim=-1)
    return idx.to(torch.int32).reshape(batch), rate.reshape(batch), dist.reshape(batch)


def _launch_assign(x, codebook, rates, lmbda, code, with_counts):
    n, d = x.shape
    k = codebook.shape[0]
    index = torch.empty(n, dtype=torch.int32, device=x.device)
    rate = torch.empty(n, dtype=torch.float32, device=x.device)
    dist = torch.empty(n, dtype=torch.float32, device=x.device)
    counts = torch.empty(k, dtype=torch.int32, device=x.device) if with_counts else None
    _lib.check(_lib.lib().tfc_vecvq_assign(
        x.data_ptr(), codebook.data_ptr(), rates.data_ptr(), n, k, d, lmbda, code, index.data_ptr(), rate.data_ptr(),
        dist.data_ptr(), _ptr(counts), _lib.stream_ptr()))
    return index, rate, dist, counts


class _EcvqAssignFunction(torch.autograd.Function):
    """tfc_vecvq_assign / tfc_vecvq_backward (include/tfc_hip.h).  A gradient nobody needs is not computed."""

    @staticmethod
    def forward(ctx, x, codebook, rates, lmbda, code):
        x, codebook, rates = x.contiguous(), codebook.contiguous(), rates.contiguous()
        index, rate, dist, _ = _launch_assign(x, codebook, rates, lmbda, code, False)
        ctx.save_for_backward(x, codebook, index)
        ctx.code = code
        ctx.mark_non_differentiable(index)
        return index, rate, dist

    @staticmethod
    def backward(ctx, _g_index, g_rate, g_dist):
        x, codebook, index = ctx.saved_tensors
        n, d = x.shape
        k = codebook.shape[0]
        need_x, need_c, need_r = ctx.needs_input_grad[:3]
        g_rate = g_rate.to(torch.float32).contiguous() if g_rate is not None and need_r else None
        g_dist = g_dist.to(torch.float32).contiguous() if g_dist is not None and (need_x or need_c) else None
        d_x = torch.empty_like(x) if need_x else None
        d_c = torch.empty_like(codebook) if need_c else None
        d_r = torch.empty(k, dtype=torch.float32, device=x.device) if need_r else None
        if need_x or need_c or need_r:
            _lib.check(_lib.lib().tfc_vecvq_backward(
                x.data_ptr(), codebook.data_ptr(), index.data_ptr(), _ptr(g_rate), _ptr(g_dist), n, k, d, ctx.code,
                _ptr(d_r), _ptr(d_c), _ptr(d_x), _lib.stream_ptr()))
        return d_x, d_c, d_r, None, None


def _device_args(x, codebook, rates, lmbda, distortion):
    _check_args(x, codebook, rates, lmbda, distortion, (torch.float32,))
    if not (codebook.is_cuda and rates.is_cuda) or codebook.device != x.device or rates.device != x.device:
        raise ValueError("x, codebook and rates must be on the same device")
    return x.reshape(-1, x.shape[-1]), float(lmbda), DISTORTION_CODE[distortion]


def ecvq_assign(x, codebook, rates, lmbda, distortion="sse"):
    """x [..., D], codebook [K, D], rates [K], float32 -> (indexes int32 [...], rate [...], distortion [...]): the
    codeword of least rates[k] + lmbda dist(x, c_k) per row (ties to the lowest k), its rate and its distortion, on the
    HIP kernels; differentiable in codebook, rates and x.  CPU tensors take `ecvq_assign_reference`."""
    if not x.is_cuda:
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"ecvq_assign supports float32 (and float64 on the CPU), got {x.dtype}")
        return ecvq_assign_reference(x, codebook, rates, lmbda, distortion)
    xf, lmbda, code = _device_args(x, codebook, rates, lmbda, distortion)
    index, rate, dist = _EcvqAssignFunction.apply(xf, codebook, rates, lmbda, code)
    batch = x.shape[:-1]
    return index.reshape(batch), rate.reshape(batch), dist.reshape(batch)


def ecvq_counts(x, codebook, rates, lmbda, distortion="sse"):
    """The usage histogram of `ecvq_assign`: int32 [K], the number of rows of x assigned to each codeword."""
    k = codebook.shape[0]
    if not x.is_cuda:
        idx, _, _ = ecvq_assign_reference(x.detach(), codebook.detach(), rates.detach(), lmbda, distortion)
        return torch.bincount(idx.reshape(-1).to(torch.int64), minlength=k).to(torch.int32)
    xf, lmbda, code = _device_args(x, codebook, rates, lmbda, distortion)
    return _launch_assign(xf.detach().contiguous(), codebook.detach().contiguous(), rates.detach().contiguous(),
                          lmbda, code, True)[3]

