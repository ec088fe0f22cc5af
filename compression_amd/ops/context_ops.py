"""The spatial context model of Minnen, Ballé and Toderici 2018 as two device calls (csrc/context_model.hip).

Definition, with y [B, Hl, Wl, M] the latent, psi [B, Hl, Wl, P] the hyper-synthesis output and y_hat zero outside the
latent:

    ctx[i, j]  = bc + sum over the 12 causal taps of y_hat[i + di, j + dj] @ Wc[di + 2, dj + 2]      M -> 2M
                 (a tap is causal when di < 0, or di == 0 and dj < 0)
    out        = b3 + lrelu(b2 + lrelu(b1 + [ctx, psi] @ W1) @ W2) @ W3                               slope 0.2
    mu, index  = out[:M], out[M:]
    idx        = int32(min(max(index, 0), num_scales - 1))           (layers.functional.index_prepare)
    sym        = rint(y - mu)  (half to even)        y_hat = float32(sym) + mu

`context_scan` runs it for a whole batch in one launch, `context_decode` runs the same network with the range decoder
in the loop: one code stream per latent row, the row in raster order, channels innermost — the strings of
`LocationScaleIndexedEntropyModel(..., coding_rank=2).compress(y - mu, index)`.  `context_scan_reference` is the
definition as tensor ops, position by position, for any float dtype and for CPU tensors;
`context_parameters_reference` is its parallel (teacher-forced) form."""
from __future__ import annotations

import collections

import torch

from .. import _lib

__all__ = ["ContextParams", "ContextScan", "context_scan", "context_decode", "context_scan_reference",
           "context_parameters_reference", "causal_mask", "CONTEXT_CONSTANTS", "wavefront_steps"]

ContextScan = collections.namedtuple("ContextScan", ["sym", "idx", "mu", "y_hat", "index_float"])

# (di, dj) of the causal taps in the kernels' order: row-major over the 5x5 window
CAUSAL_TAPS = tuple((di, dj) for di in range(-2, 1) for dj in range(-2, 3) if di < 0 or dj < 0)


# the named constants of csrc/context_params.h
CONTEXT_CONSTANTS = _lib.kernel_constants("context_params.h", ("CTX",))
assert CONTEXT_CONSTANTS["CTX_TAPS"] == len(CAUSAL_TAPS)


def tap_mask(taps, dtype=torch.float32, device=None):
    """[5, 5, 1, 1]: 1 on the taps (di, dj) of the list, 0 elsewhere."""
    mask = torch.zeros(5, 5, 1, 1, dtype=dtype, device=device)
    for di, dj in taps:
        mask[di + 2, dj + 2] = 1
    return mask


def causal_mask(dtype=torch.float32, device=None):
    """[5, 5, 1, 1]: 1 on the 12 causal taps, 0 on the centre and everything after it in raster order."""
    return tap_mask(CAUSAL_TAPS, dtype, device)


def tap_sum(start, y_hat, kernel, taps):
    """start + the sum over `taps`, in the list's order, of y_hat [B, Hl, Wl, M] moved by the tap @ kernel[tap], with
    y_hat zero outside the latent.  Rows below the latent are padded only when a tap reads them."""
    hl, wl = y_hat.shape[1:3]
    padded = torch.nn.functional.pad(y_hat, (0, 0, 2, 2, 2, max(di for di, _ in taps)))
    for di, dj in taps:
        start = start + padded[:, 2 + di:2 + di + hl, 2 + dj:2 + dj + wl] @ kernel[di + 2, dj + 2]
    return start


def wavefront_steps(hl, wl):
    """The positions of every wavefront step t = j + 3 i, in step order: [[(i, j), ...], ...]."""
    steps = []
    for t in range((wl - 1) + 3 * (hl - 1) + 1):
        lo = -(-(t - (wl - 1)) // 3) if t > wl - 1 else 0
        steps.append([(i, t - 3 * i) for i in range(lo, min(t // 3, hl - 1) + 1)])
    return steps


def _pad(v):
    k = CONTEXT_CONSTANTS["CTX_KPAD"]
    return -(-v // k) * k


def _layout(m, p, h1, h2):
    """ctx_layout of csrc/context_params.h: {section: (offset, rows, padded rows, columns)} and the total floats."""
    c2 = 2 * m
    sections = [("wc", CONTEXT_CONSTANTS["CTX_TAPS"] * m, CONTEXT_CONSTANTS["CTX_TAPS"] * _pad(m), c2), ("bc", 1, 1, c2),
                ("w1c", c2, _pad(c2), h1), ("w1p", p, _pad(p), h1), ("b1", 1, 1, h1),
                ("w2", h1, _pad(h1), h2), ("b2", 1, 1, h2), ("w3", h2, _pad(h2), c2), ("b3", 1, 1, c2)]
    out, at = {}, 0
    for name, rows, padded, cols in sections:
        out[name] = (at, rows, padded, cols)
        at += _pad(padded * cols)
    return out, at


class ContextParams:
    """The weights of the context model, checked and packed once.

    kernel [5, 5, M, 2M] (HWIO, as `MaskedConv2D.kernel`; the causal mask is applied here whatever the non-causal
    taps hold), kernel_bias [2M], w1 [2M + P, H1], b1 [H1], w2 [H1, H2], b2 [H2], w3 [H2, 2M], b3 [2M]: rows are
    inputs, as a 1x1 `SignalConv2D` kernel [1, 1, in, out] reshaped.  Holds detached copies.

    `TAPS` is the tap list, in the order of the packed rows; a subclass with another list of CTX_TAPS taps
    (ops/checkerboard_ops.py) gets the same checks, cache and packed layout with its own mask."""

    TAPS = CAUSAL_TAPS

    @classmethod
    def mask(cls, dtype=torch.float32, device=None):
        """[5, 5, 1, 1]: 1 on `TAPS`, 0 elsewhere."""
        return tap_mask(cls.TAPS, dtype, device)

    def __init__(self, kernel, kernel_bias, w1, b1, w2, b2, w3, b3, num_scales):
        t = [torch.as_tensor(v).detach() for v in (kernel, kernel_bias, w1, b1, w2, b2, w3, b3)]
        kernel, kernel_bias, w1, b1, w2, b2, w3, b3 = t
        if kernel.dim() != 4 or tuple(kernel.shape[:2]) != (5, 5) or kernel.shape[3] != 2 * kernel.shape[2]:
            raise ValueError(f"kernel must be [5, 5, M, 2M], received shape {tuple(kernel.shape)}")
        m = int(kernel.shape[2])
        if m < 1:
            raise ValueError("kernel must have at least one input channel")
        if w1.dim() != 2 or w1.shape[0] <= 2 * m:
            raise ValueError(f"w1 must be [2M + P, H1] with P >= 1 (M = {m}), received shape {tuple(w1.shape)}")
        p, h1 = int(w1.shape[0]) - 2 * m, int(w1.shape[1])
        if w2.dim() != 2 or w2.shape[0] != h1:
            raise ValueError(f"w2 must be [{h1}, H2], received shape {tuple(w2.shape)}")
        h2 = int(w2.shape[1])
        if tuple(w3.shape) != (h2, 2 * m):
            raise ValueError(f"w3 must be [{h2}, {2 * m}], received shape {tuple(w3.shape)}")
        for name, b, n in (("kernel_bias", kernel_bias, 2 * m), ("b1", b1, h1), ("b2", b2, h2), ("b3", b3, 2 * m)):
            if tuple(b.shape) != (n,):
                raise ValueError(f"{name} must be [{n}], received shape {tuple(b.shape)}")
        if min(h1, h2) < 1:
            raise ValueError("H1 and H2 must be at least 1")
        if any(not v.dtype.is_floating_point for v in t):
            raise TypeError("the weights must be floating point")
        if int(num_scales) < 1:
            raise ValueError(f"num_scales must be positive, got {num_scales}")
        limit = CONTEXT_CONSTANTS["CTX_MAX_DIM"]
        if max(m, p, h1, h2) > limit:
            raise ValueError(f"M, P, H1 and H2 must be at most {limit}")
        self.m, self.p, self.h1, self.h2, self.num_scales = m, p, h1, h2, int(num_scales)
        self.kernel = kernel * self.mask(kernel.dtype, kernel.device)
        self.kernel_bias, self.w1, self.b1, self.w2, self.b2, self.w3, self.b3 = kernel_bias, w1, b1, w2, b2, w3, b3
        self._cache = {}

    @classmethod
    def from_layers(cls, context_conv, layers, num_scales):
        """From a `MaskedConv2D` and the three 1x1 `SignalConv2D` layers of the entropy-parameter network."""
        w = [layer.kernel.reshape(layer.kernel.shape[-2], layer.kernel.shape[-1]) for layer in layers]
        b = [layer._bias_value() for layer in layers]
        return cls(context_conv.kernel, context_conv._bias_value(), w[0], b[0], w[1], b[1], w[2], b[2], num_scales)

    def tensors(self, dtype, device):
        """(kernel masked, kernel_bias, w1, b1, w2, b2, w3, b3) in `dtype` on `device`."""
        key = ("tensors", dtype, str(device))
        if key not in self._cache:
            self._cache[key] = tuple(v.to(device=device, dtype=dtype) for v in (
                self.kernel, self.kernel_bias, self.w1, self.b1, self.w2, self.b2, self.w3, self.b3))
        return self._cache[key]

    def _ab_rows(self):
        """Floats per position of the kernels' two activation buffers: A holds ctx then h2, B holds h1 then the output."""
        return max(_pad(2 * self.m), _pad(self.h2)) + max(_pad(self.h1), _pad(2 * self.m))

    def fits_kernel(self):
        """Whether one position's activations fit the kernels' LDS (csrc/context_params.h, ctx_layout)."""
        return max(self._ab_rows(), _pad(self.p)) <= CONTEXT_CONSTANTS["CTX_LDS_FLOATS"]

    def packed(self, device):
        """The float32 buffer the kernels read (layout: csrc/context_params.h)."""
        key = ("packed", str(device))
        if key not in self._cache:
            kernel, bc, w1, b1, w2, b2, w3, b3 = self.tensors(torch.float32, "cpu")
            m = self.m
            sections, total = _layout(self.m, self.p, self.h1, self.h2)
            buf = torch.zeros(total, dtype=torch.float32)

            def put(name, value):
                at, rows, padded, cols = sections[name]
                assert tuple(value.shape) == (rows, cols), (name, tuple(value.shape), rows, cols)
                buf[at:at + rows * cols] = value.reshape(-1)

            taps = torch.zeros(len(self.TAPS), _pad(m), 2 * m)
            for k, (di, dj) in enumerate(self.TAPS):
                taps[k, :m] = kernel[di + 2, dj + 2]
            at = sections["wc"][0]
            buf[at:at + taps.numel()] = taps.reshape(-1)
            for name, value in (("bc", bc[None]), ("w1c", w1[:2 * m]), ("w1p", w1[2 * m:]), ("b1", b1[None]),
                                ("w2", w2), ("b2", b2[None]), ("w3", w3), ("b3", b3[None])):
                put(name, value)
            self._cache[key] = buf.to(device)
        return self._cache[key]


def _check_inputs(y, psi, params, what="y", kind=None):
    kind = kind or ContextParams
    if not isinstance(params, kind) or params.TAPS != kind.TAPS:
        raise TypeError(f"params must be a {kind.__name__}")
    if psi.dim() != 4 or psi.shape[-1] != params.p:
        raise ValueError(f"psi must be [B, Hl, Wl, {params.p}], received shape {tuple(psi.shape)}")
    if y is not None:
        if y.dim() != 4 or y.shape[-1] != params.m:
            raise ValueError(f"{what} must be [B, Hl, Wl, {params.m}], received shape {tuple(y.shape)}")
        if tuple(y.shape[:3]) != tuple(psi.shape[:3]):
            raise ValueError(f"{what} and psi must share [B, Hl, Wl], received {tuple(y.shape)} and {tuple(psi.shape)}")
        if y.device != psi.device or y.dtype != psi.dtype:
            raise ValueError(f"{what} and psi must share dtype and device")
    if psi.shape[1] < 1 or psi.shape[2] < 1:
        raise ValueError(f"Hl and Wl must be at least 1, received shape {tuple(psi.shape)}")
    if not psi.dtype.is_floating_point:
        raise TypeError("y and psi must be floating point")


def _network(ctx, psi, w):
    _, _, w1, b1, w2, b2, w3, b3 = w
    lrelu = torch.nn.functional.leaky_relu
    h = lrelu(torch.cat([ctx, psi], dim=-1) @ w1 + b1, 0.2)
    h = lrelu(h @ w2 + b2, 0.2)
    return h @ w3 + b3


def _index_prepare(index_float, num_scales):
    # NaN goes to 0, as fmaxf(NaN, 0) does on the device
    clamped = torch.nan_to_num(index_float, nan=0.0).clamp(0, num_scales - 1)
    return clamped.to(torch.int32)


def context_parameters_reference(y_hat, psi, params):
    """The parallel (teacher-forced) definition -> (mu, index_float), each [B, Hl, Wl, M]: the parameters every position
    gets when its causal neighbourhood holds `y_hat`."""
    _check_inputs(y_hat, psi, params, "y_hat")
    w = params.tensors(y_hat.dtype, y_hat.device)
    b, hl, wl, m = y_hat.shape
    out = _network(tap_sum(w[1].expand(b, hl, wl, 2 * m), y_hat, w[0], CAUSAL_TAPS), psi, w)
    return out[..., :m], out[..., m:]


def context_scan_reference(y, psi, params, order="raster"):
    """The definition, one position after the other -> ContextScan(sym int32, idx int32, mu, y_hat, index_float).
    `order`: "raster" or "wavefront" (t = j + 3 i ascending); the results are the same.  Any float dtype, any
    device."""
    _check_inputs(y, psi, params)
    if order not in ("raster", "wavefront"):
        raise ValueError(f'order must be "raster" or "wavefront", got {order!r}')
    w = params.tensors(y.dtype, y.device)
    b, hl, wl, m = y.shape
    if order == "raster":
        positions = [(i, j) for i in range(hl) for j in range(wl)]
    else:
        positions = [pos for step in wavefront_steps(hl, wl) for pos in step]
    y_hat = torch.zeros_like(y)
    mu, index_float = torch.zeros_like(y), torch.zeros_like(y)
    sym = torch.zeros(y.shape, dtype=torch.int32, device=y.device)
    for i, j in positions:
        ctx = w[1].expand(b, 2 * m)
        for di, dj in CAUSAL_TAPS:
            ii, jj = i + di, j + dj
            if ii >= 0 and 0 <= jj < wl:
                ctx = ctx + y_hat[:, ii, jj] @ w[0][di + 2, dj + 2]
        out = _network(ctx, psi[:, i, j], w)
        mu[:, i, j], index_float[:, i, j] = out[:, :m], out[:, m:]
        r = torch.round(y[:, i, j] - out[:, :m])
        sym[:, i, j] = r.to(torch.int32)
        y_hat[:, i, j] = r + out[:, :m]
    return ContextScan(sym, _index_prepare(index_float, params.num_scales), mu, y_hat, index_float)


def _workspace(params, b, hl, wl, device):
    n = _lib.lib().tfc_context_workspace(b, hl, wl, params.m, params.p, params.h1, params.h2)
    if n < 0:
        raise ValueError(_lib.last_error())
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=device)


def context_scan(y, psi, params):
    """y [B, Hl, Wl, M], psi [B, Hl, Wl, P] -> ContextScan(sym int32, idx int32, mu, y_hat, index_float): float32 device
    tensors run tfc_context_scan, one launch for the batch; CPU tensors and other float dtypes take
    `context_scan_reference`."""
    _check_inputs(y, psi, params)
    if not y.is_cuda or y.dtype != torch.float32:
        return context_scan_reference(y, psi, params)
    y, psi = y.detach().contiguous(), psi.detach().contiguous()
    b, hl, wl, m = y.shape
    packed = params.packed(y.device)
    work = _workspace(params, b, hl, wl, y.device)
    sym = torch.empty(y.shape, dtype=torch.int32, device=y.device)
    idx = torch.empty_like(sym)
    mu, index_float, y_hat = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
    _lib.check(_lib.lib().tfc_context_scan(
        y.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(), b, hl, wl, m, params.p, params.h1, params.h2,
        params.num_scales, work.data_ptr(), sym.data_ptr(), idx.data_ptr(), mu.data_ptr(), index_float.data_ptr(),
        y_hat.data_ptr(), _lib.stream_ptr()))
    return ContextScan(sym, idx, mu, y_hat, index_float)


def context_decode(strings, psi, params, lookup, cdf_offset):
    """The row strings [B, Hl] (a container of bytes, a (device blob, device offsets, shape) triple or a finalized
    encoder handle, as `create_range_decoder` takes them), psi [B, Hl, Wl, P] float32 on the device, the entropy
    model's `cdf` (lookup) and `cdf_offset` -> (y_hat [B, Hl, Wl, M], ok uint8 [B, Hl]).  One launch."""
    from . import gen_ops
    _check_inputs(None, psi, params)
    if not psi.is_cuda or psi.dtype != torch.float32:
        raise ValueError("context_decode needs float32 psi on the device")
    psi = psi.detach().contiguous()
    b, hl, wl, _ = psi.shape
    device = psi.device
    if isinstance(strings, gen_ops.EncoderHandle):
        blob, offsets = gen_ops.device_strings(strings)
        shape = tuple(strings.shape)
    elif isinstance(strings, tuple) and len(strings) == 3 and isinstance(strings[0], torch.Tensor):
        blob, offsets, shape = strings[0].to(device), strings[1].to(device, torch.int64), tuple(strings[2])
    else:
        blob_h, off_h, shape = gen_ops.blob_from_strings(strings)
        blob, offsets = torch.from_numpy(blob_h).to(device), torch.from_numpy(off_h).to(device)
    if tuple(int(s) for s in shape) != (b, hl):
        raise ValueError(f"strings must have shape [{b}, {hl}] (one per latent row), received {list(shape)}")
    blob, offsets = blob.contiguous(), offsets.contiguous()
    if blob.numel() == 0:
        blob = torch.zeros(1, dtype=torch.uint8, device=device)
    tables = gen_ops._tables_for(lookup)
    if tables.count != params.num_scales:
        raise ValueError(f"the tables hold {tables.count} rows, num_scales is {params.num_scales}")
    cdf_offset = torch.as_tensor(cdf_offset).to(device, torch.int32).contiguous()
    if cdf_offset.numel() != params.num_scales:
        raise ValueError(f"cdf_offset must have {params.num_scales} entries, received {cdf_offset.numel()}")
    packed = params.packed(device)
    work = _workspace(params, b, hl, wl, device)
    y_hat = torch.empty(b, hl, wl, params.m, dtype=torch.float32, device=device)
    ok = torch.empty(b, hl, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().tfc_context_decode(
        tables.ptr, blob.data_ptr(), offsets.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(),
        cdf_offset.data_ptr(), b, hl, wl, params.m, params.p, params.h1, params.h2, params.num_scales,
        work.data_ptr(), y_hat.data_ptr(), ok.data_ptr(), _lib.stream_ptr()))
    y_hat._tfc_keep = (blob, offsets, tables, cdf_offset, packed, work, strings)
    return y_hat, ok
