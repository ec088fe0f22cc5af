"""Thin torch-tensor front-ends of the transform kernels in libtfc_hip.so."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import ptr as _ptr

_DTYPE_CODE = _lib.DTYPE_CODE


class GDNPrepared:
    """The forward kernels' LDS image of one (beta, gamma) pair, built once (include/tfc_hip.h
    tfc_gdn_params_create): the per-call preparation launch drops out of inference calls."""

    def __init__(self, beta: torch.Tensor, gamma: torch.Tensor, dtype: torch.dtype):
        device = _lib.require_device()
        if dtype not in _DTYPE_CODE:
            raise TypeError(f"GDN kernel supports float32 and bfloat16, got {dtype}")
        beta = beta.detach().to(device, torch.float32).contiguous()
        gamma = gamma.detach().to(device, torch.float32).contiguous()
        C = beta.shape[0]
        if gamma.shape != (C, C):
            raise ValueError(f"beta/gamma shapes {tuple(beta.shape)}/{tuple(gamma.shape)} do not match")
        import ctypes
        out = ctypes.c_void_p()
        _lib.check(_lib.lib().tfc_gdn_params_create(beta.data_ptr(), gamma.data_ptr(), C, _DTYPE_CODE[dtype],
                                                    _lib.stream_ptr(), ctypes.byref(out)))
        self.ptr, self.channels, self.dtype = out, C, dtype
        self._keep = (beta, gamma)        # read by the preparation kernel in stream order

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _lib.lib().tfc_gdn_params_destroy(self.ptr)
        except Exception:
            pass


def gdn_forward(x: torch.Tensor, beta: torch.Tensor, gamma: torch.Tensor, inverse: bool = False,
                rectify: bool = False, alpha: float = 1, epsilon: float = 1, prepared: GDNPrepared = None) -> torch.Tensor:
    """Fused GDN/IGDN forward, channels-last: x [..., C], beta [C], gamma [C(in), C(out)]
    (the layout of `GDN.gamma`, python/layers/gdn.py:394-398).  `prepared` (GDNPrepared of the same beta /
    gamma / dtype): skips the per-call parameter preparation (fixed alpha in {1, 2}, epsilon in {1, .5})."""
    _lib.require_device()
    if x.dtype not in _DTYPE_CODE:
        raise TypeError(f"GDN kernel supports float32 and bfloat16, got {x.dtype}")
    alpha, epsilon = float(alpha), float(epsilon)
    x = x.contiguous()
    C = x.shape[-1]
    if prepared is not None and alpha in (1, 2) and epsilon in (1, 0.5):
        if prepared.channels != C or prepared.dtype != x.dtype:
            raise ValueError("prepared GDN parameters do not match the input")
        y = torch.empty_like(x)
        _lib.check(_lib.lib().tfc_gdn_forward_prepared(
            prepared.ptr, x.data_ptr(), y.data_ptr(), x.numel() // C, int(bool(inverse)), int(bool(rectify)),
            int(alpha), 1 if epsilon == 0.5 else 0, _lib.stream_ptr()))
        return y
    beta = beta.detach().to(x.device, torch.float32).contiguous()
    gamma = gamma.detach().to(x.device, torch.float32).contiguous()
    if beta.shape != (C,) or gamma.shape != (C, C):
        raise ValueError(f"beta/gamma shapes {tuple(beta.shape)}/{tuple(gamma.shape)} do not match C={C}")
    y = torch.empty_like(x)
    if alpha not in (1, 2) or epsilon not in (1, 0.5):
        # general exponents (gdn.py:386-387, :411-412: tf.pow), the kernels' GEN variant
        _lib.check(_lib.lib().tfc_gdn_forward_general(
            x.data_ptr(), y.data_ptr(), _DTYPE_CODE[x.dtype], x.numel() // C, C, beta.data_ptr(),
            gamma.data_ptr(), int(bool(inverse)), int(bool(rectify)), alpha, epsilon, _lib.stream_ptr()))
        return y
    _lib.check(_lib.lib().tfc_gdn_forward(
        x.data_ptr(), y.data_ptr(), _DTYPE_CODE[x.dtype], x.numel() // C, C, beta.data_ptr(),
        gamma.data_ptr(), int(bool(inverse)), int(bool(rectify)), int(alpha),
        1 if epsilon == 0.5 else 0, _lib.stream_ptr()))
    return y


def channel_norm_reference(x, gamma, beta, epsilon=1e-3, relu=False, residual=None):
    """The formula of `channel_norm` as differentiable tensor ops in float32 (archs.py:255-273, the variance through
    `mean.detach()` as the reference's tf.stop_gradient; a float64 input stays float64): what ChannelNorm evaluates for
    a CPU tensor."""
    ft = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(ft)
    C = xf.shape[-1]
    mean = xf.mean(dim=-1, keepdim=True)
    var = ((xf - mean.detach()) ** 2).sum(dim=-1, keepdim=True) / (C - 1)
    y = (xf - mean) * torch.rsqrt(var + epsilon)
    if gamma is not None:
        y = y * gamma.to(ft)
    if beta is not None:
        y = y + beta.to(ft)
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + residual.to(ft)
    return y.to(x.dtype)


def _channel_norm_args(x, gamma, beta, epsilon):
    _lib.require_device()
    if x.dtype not in _DTYPE_CODE:
        raise TypeError(f"ChannelNorm kernel supports float32 and bfloat16, got {x.dtype}")
    if x.dim() < 2:
        raise ValueError(f"Input tensor must have at least rank 2, received shape {tuple(x.shape)}.")
    C = x.shape[-1]
    if C < 2:
        raise ValueError(f"ChannelNorm divides by channels - 1: at least 2 channels, got {C}")
    params = []
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            t = t.detach().to(x.device, torch.float32).contiguous()
            if t.shape != (C,):
                raise ValueError(f"{name} shape {tuple(t.shape)} does not match C={C}")
        params.append(t)
    return x.contiguous(), params[0], params[1], C, float(epsilon)


def channel_norm_forward(x, gamma, beta, epsilon=1e-3, relu=False, residual=None):
    """tfc_channel_norm_forward (include/tfc_hip.h): one launch, no gradient."""
    x, gamma, beta, C, epsilon = _channel_norm_args(x, gamma, beta, epsilon)
    if residual is not None:
        if residual.shape != x.shape:
            raise ValueError(f"residual shape {tuple(residual.shape)} does not match the input's {tuple(x.shape)}")
        residual = residual.detach().to(x.dtype).contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().tfc_channel_norm_forward(
        x.data_ptr(), _ptr(gamma), _ptr(beta), _ptr(residual), y.data_ptr(), _DTYPE_CODE[x.dtype], x.numel() // C, C,
        epsilon, int(bool(relu)), _lib.stream_ptr()))
    return y


def channel_norm_backward(x, grad, gamma, beta, epsilon=1e-3, relu=False):
    """tfc_channel_norm_backward: -> (dx, dgamma, dbeta), float32 [C] parameter gradients (None for a missing one)."""
    x, gamma, beta, C, epsilon = _channel_norm_args(x, gamma, beta, epsilon)
    grad = grad.to(x.dtype).contiguous()
    dx = torch.empty_like(x)
    dgamma = None if gamma is None else torch.empty(C, dtype=torch.float32, device=x.device)
    dbeta = None if beta is None else torch.empty(C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tfc_channel_norm_backward(
        x.data_ptr(), grad.data_ptr(), _ptr(gamma), _ptr(beta), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta),
        _DTYPE_CODE[x.dtype], x.numel() // C, C, epsilon, int(bool(relu)), _lib.stream_ptr()))
    return dx, dgamma, dbeta


class _ChannelNormFunction(torch.autograd.Function):
    """Differentiable wrapper of the two ChannelNorm entries (the reference differentiates archs.py:255-273 with TF
    autodiff).  The residual's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, epsilon, relu):
        ctx.save_for_backward(x, gamma, beta)
        ctx.cfg = (epsilon, relu, residual is not None)
        return channel_norm_forward(x, gamma, beta, epsilon, relu, residual)

    @staticmethod
    def backward(ctx, grad):
        x, gamma, beta = ctx.saved_tensors
        epsilon, relu, has_residual = ctx.cfg
        dx, dgamma, dbeta = channel_norm_backward(x, grad, gamma, beta, epsilon, relu)
        if gamma is not None:
            dgamma = dgamma.to(gamma.dtype)
        if beta is not None:
            dbeta = dbeta.to(beta.dtype)
        return dx, dgamma, dbeta, (grad if has_residual else None), None, None


def channel_norm(x, gamma, beta, epsilon=1e-3, relu=False, residual=None):
    """ChannelNorm of HiFiC (archs.py:214-297) over the last axis of x [..., C] on the fused kernel: unbiased variance,
    gamma / beta [C] or None, then ReLU if `relu`, then `+ residual` if given.  Differentiable in x, gamma, beta and
    residual."""
    needs = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, gamma, beta, residual))
    if needs:
        return _ChannelNormFunction.apply(x, gamma, beta, residual, float(epsilon), bool(relu))
    return channel_norm_forward(x, gamma, beta, epsilon, relu, residual)


def _ntuple(v, n):
    return (int(v),) * n if isinstance(v, int) else tuple(int(s) for s in v)


def pad_channels(t, multiple=16, dim=-1):
    """Zero channels up to a multiple of 16 along `dim` (what the convolution kernels take; zero channels change nothing)."""
    extra = -t.shape[dim] % multiple
    if not extra:
        return t
    pad = [0, 0] * (t.dim() - 1 - (dim % t.dim())) + [0, extra]
    return torch.nn.functional.pad(t, pad)


def _conv_args(x, kernel, bias, rank):
    """The convolution launchers' checks -> (kernel, bias) as float32 on x's device."""
    _lib.require_device()
    if x.dtype not in _DTYPE_CODE:
        raise TypeError(f"conv kernel supports float32 and bfloat16, got {x.dtype}")
    if x.dim() != rank + 2:
        raise ValueError(f"Input tensor must have rank {rank + 2}, received shape {tuple(x.shape)}.")
    if kernel.shape[-2] != x.shape[-1]:
        raise ValueError(f"kernel expects {kernel.shape[-2]} input channels, input has {x.shape[-1]}")
    kernel = kernel.detach().to(x.device, torch.float32)
    if bias is not None:
        bias = bias.detach().to(x.device, torch.float32).contiguous()
    return kernel, bias


def _conv_output(x, strides, up, cout):
    """The output tensor: in * s per axis (up) or ceil(in / s) (down)."""
    spatial = tuple(n * s if up else -(-n // s) for n, s in zip(x.shape[1:-1], strides))
    return torch.empty((x.shape[0],) + spatial + (cout,), dtype=x.dtype, device=x.device)


def _conv(x, kernel, bias, stride, activation, up, weights_key=0):
    kernel, bias = _conv_args(x, kernel, bias, 2)
    x, kernel = x.contiguous(), kernel.contiguous()
    n, h, w, cin = x.shape
    kh, kw, _, cout = kernel.shape
    y = _conv_output(x, (stride, stride), up, cout)
    act = {None: 0, "relu": 1}[activation]
    if weights_key:
        _lib.lib().tfc_conv2d_weights_key(weights_key)      # this thread's next conv call: fragments packed once per value
    fn = _lib.lib().tfc_conv2d_up if up else _lib.lib().tfc_conv2d_down
    _lib.check(fn(
        x.data_ptr(), kernel.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
        _DTYPE_CODE[x.dtype], n, h, w, cin, cout, kh, kw, int(stride), act, _lib.stream_ptr()))
    return y


def conv2d_gdn(x, kernel, bias, stride, up, prepared: GDNPrepared, inverse: bool, weights_key=0):
    """SignalConv2D with GDN / IGDN as its activation (inference, bfloat16): -> (y, fused).  fused: the convolution
    kernel applied the activation itself (include/tfc_hip.h, tfc_conv2d_gdn); else y is the convolution's output and
    the caller applies the GDN kernel."""
    import ctypes
    kernel, bias = _conv_args(x, kernel, bias, 2)
    x, kernel = x.contiguous(), kernel.contiguous()
    n, h, w, cin = x.shape
    kh, kw, _, cout = kernel.shape
    y = _conv_output(x, (stride, stride), up, cout)
    fused = ctypes.c_int(0)
    if weights_key:
        _lib.lib().tfc_conv2d_weights_key(weights_key)
    _lib.check(_lib.lib().tfc_conv2d_gdn(
        x.data_ptr(), kernel.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
        _DTYPE_CODE[x.dtype], n, h, w, cin, cout, kh, kw, int(stride), int(bool(up)), prepared.ptr, int(bool(inverse)),
        ctypes.byref(fused), _lib.stream_ptr()))
    return y, bool(fused.value)


def _wgrad_width(c):
    """The channel count the weight gradient kernel runs a side of `c` channels at: 1 ... 4, or a multiple of 32."""
    return c if c <= 4 else c + -c % 32


def conv2d_wgrad(a, b, kernel_support, stride, transpose):
    """Weight gradient kernel: G[t][ca][cb] = sum A[n, q*s + t - k/2, ca] B[n, q, cb] as a float32
    [kh, kw, Cin, Cout] tensor (transpose=True: A carries Cout, B carries Cin).  A side of more than 4 channels that is
    no multiple of 32 gets zero channels up to the next one, sliced off the result."""
    _lib.require_device()
    ca, cb = a.shape[-1], b.shape[-1]
    if (_wgrad_width(ca), _wgrad_width(cb)) != (ca, cb):
        dw = conv2d_wgrad(pad_channels(a, _wgrad_width(ca)), pad_channels(b.to(a.dtype), _wgrad_width(cb)),
                          kernel_support, stride, transpose)
        return dw[..., :cb, :ca] if transpose else dw[..., :ca, :cb]
    built = (256, 192, 128, 64, 32)
    if any(c > 4 and c not in built for c in (ca, cb)):
        # the kernel is built for 32, 64, 128, 192 or 256 channels on either side; the gradient of a channel
        # block pair only needs those channels, so other widths (ms2020: 224, 320 .. 512) go in blocks
        def blocks(c):
            if c <= 4 or c in built:
                return [(0, c)]
            out, i = [], 0
            while i < c:
                w = next(w for w in built if w <= c - i)
                out.append((i, i + w))
                i += w
            return out
        rows = []
        for a0, a1 in blocks(ca):
            cols = [conv2d_wgrad(a[..., a0:a1], b[..., b0:b1], kernel_support, stride, transpose)
                    for b0, b1 in blocks(cb)]
            rows.append(torch.cat(cols, dim=2 if transpose else 3))
        return torch.cat(rows, dim=3 if transpose else 2)
    return _conv2d_wgrad_launch(a, b, kernel_support, stride, transpose)


def _conv2d_wgrad_launch(a, b, kernel_support, stride, transpose):
    """tfc_conv2d_wgrad (include/tfc_hip.h) on channel counts it is built for."""
    kh, kw = kernel_support
    a, b = a.contiguous(), b.contiguous()
    n, ha, wa, ca = a.shape
    _, hb, wb, cb = b.shape
    shape = (kh, kw, cb, ca) if transpose else (kh, kw, ca, cb)
    dw = torch.zeros(shape, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().tfc_conv2d_wgrad(
        a.data_ptr(), b.data_ptr(), dw.data_ptr(), _DTYPE_CODE[a.dtype], n, ha, wa, ca, hb, wb, cb,
        kh, kw, int(stride), int(bool(transpose)), _lib.stream_ptr()))
    return dw


CONV2D_WGRAD_PLAN_FIELDS = ("tiles_ca", "tiles_cb", "chunks", "chunk_steps", "pixels_in_last_stage", "tr", "lds_bytes")


def conv2d_wgrad_plan(n, b_extent, ca, cb, kernel_support, dtype, cus):
    """What the host of tfc_conv2d_wgrad chooses over B's grid [n, *b_extent] for tensors of `dtype` on a device of `cus`
    compute units, as a dict over CONV2D_WGRAD_PLAN_FIELDS (include/tfc_hip.h, tfc_conv2d_wgrad_plan).  Host only: needs
    no device and launches nothing."""
    import ctypes
    out = (ctypes.c_int32 * len(CONV2D_WGRAD_PLAN_FIELDS))()
    _lib.check(_lib.lib().tfc_conv2d_wgrad_plan(_DTYPE_CODE[dtype], n, *b_extent, ca, cb, *kernel_support, int(cus), out))
    return dict(zip(CONV2D_WGRAD_PLAN_FIELDS, out))


def _conv3d(x, kernel, bias, strides, activation, up):
    kernel, bias = _conv_args(x, kernel, bias, 3)
    x, kernel = pad_channels(x).contiguous(), pad_channels(kernel, dim=-2).contiguous()
    n, d, h, w, cin = x.shape
    kd, kh, kw, _, cout = kernel.shape
    sd, sh, sw = strides
    y = _conv_output(x, strides, up, cout)
    act = {None: 0, "relu": 1}[activation]
    fn = _lib.lib().tfc_conv3d_up if up else _lib.lib().tfc_conv3d_down
    _lib.check(fn(
        x.data_ptr(), kernel.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
        _DTYPE_CODE[x.dtype], n, d, h, w, cin, cout, kd, kh, kw, sd, sh, sw, act, _lib.stream_ptr()))
    return y


def conv3d_wgrad(a, b, kernel_support, strides, transpose):
    """Weight gradient kernel (include/tfc_hip.h, tfc_conv3d_wgrad): G[t][ca][cb] = sum A[n, q*s + t - k/2, ca] B[n, q, cb]
    as a float32 [kd, kh, kw, Cin, Cout] tensor (transpose=True: A carries Cout, B carries Cin).  Channel counts that
    are not multiples of 16 are padded with zeros and sliced off."""
    _lib.require_device()
    kd, kh, kw = kernel_support
    sd, sh, sw = strides
    ca, cb = a.shape[-1], b.shape[-1]
    a, b = pad_channels(a).contiguous(), pad_channels(b.to(a.dtype)).contiguous()
    n, da, ha, wa, cap = a.shape
    _, db, hb, wb, cbp = b.shape
    shape = (kd, kh, kw, cbp, cap) if transpose else (kd, kh, kw, cap, cbp)
    dw = torch.empty(shape, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().tfc_conv3d_wgrad(
        a.data_ptr(), b.data_ptr(), dw.data_ptr(), _DTYPE_CODE[a.dtype], n, da, ha, wa, cap, db, hb, wb, cbp,
        kd, kh, kw, sd, sh, sw, int(bool(transpose)), _lib.stream_ptr()))
    return dw[..., :cb, :ca] if transpose else dw[..., :ca, :cb]


CONV3D_PLAN_FIELDS = ("TW", "TH", "NT", "nblk", "tiles_w", "tiles_h", "phases", "lds_bytes")
CONV3D_WGRAD_PLAN_FIELDS = ("tiles_ca", "tiles_cb", "chunks", "chunk_steps", "pixels_in_last_chunk")


def conv3d_plan(up, extent, cin_k, cout, kernel_support, strides):
    """What the host of tfc_conv3d_down / tfc_conv3d_up chooses for an input of `extent` (d, h, w) with cin_k channels as
    the kernel sees them (Cin for bfloat16, 6 Cin for float32), as a dict over CONV3D_PLAN_FIELDS (include/tfc_hip.h,
    tfc_conv3d_plan).  Host only: needs no device and launches nothing."""
    import ctypes
    out = (ctypes.c_int32 * len(CONV3D_PLAN_FIELDS))()
    _lib.check(_lib.lib().tfc_conv3d_plan(int(bool(up)), *extent, cin_k, cout, *kernel_support, *strides, out))
    return dict(zip(CONV3D_PLAN_FIELDS, out))


def conv3d_wgrad_plan(n, b_extent, ca, cb, kernel_support):
    """What the host of tfc_conv3d_wgrad chooses over B's grid [n, *b_extent], as a dict over CONV3D_WGRAD_PLAN_FIELDS
    (include/tfc_hip.h, tfc_conv3d_wgrad_plan).  Host only."""
    import ctypes
    out = (ctypes.c_int32 * len(CONV3D_WGRAD_PLAN_FIELDS))()
    _lib.check(_lib.lib().tfc_conv3d_wgrad_plan(n, *b_extent, ca, cb, *kernel_support, out))
    return dict(zip(CONV3D_WGRAD_PLAN_FIELDS, out))


# per number of spatial axes: (forward launcher, weight gradient); rank 2 takes one stride, rank 3 one per axis
_CONV_KERNELS = {2: (_conv, conv2d_wgrad), 3: (_conv3d, conv3d_wgrad)}


class _ConvFunction(torch.autograd.Function):
    """Differentiable wrapper of a rank's conv entry points (the reference differentiates
    signal_conv.py:663-690 / 778-847 with TF autodiff):
      dx  = the OTHER direction's forward kernel on dy with the kernel's channel axes swapped (cropped after up),
      dw  = the rank's weight gradient kernel,   dbias = sum of dy over pixels."""

    @staticmethod
    def forward(ctx, x, kernel, bias, strides, activation, up, rank):
        y = _CONV_KERNELS[rank][0](x, kernel, bias, strides, activation, up)
        ctx.save_for_backward(x, kernel, y if activation == "relu" else None)
        ctx.meta = (strides, activation, up, bias is not None, rank)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, kernel, y = ctx.saved_tensors
        strides, activation, up, has_bias, rank = ctx.meta
        launch, wgrad = _CONV_KERNELS[rank]
        gy = gy.to(x.dtype).contiguous()
        if activation == "relu":
            gy = gy * (y > 0)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            g, kt = gy, kernel.transpose(-1, -2)
            if rank == 2 and g.shape[-1] > 4:
                # the rank-2 kernels take 1 ... 4 or a multiple of 16 input channels: here the layer's `filters`
                g, kt = pad_channels(g), pad_channels(kt, dim=-2)
            if up:
                dx = launch(g, kt, None, strides, None, False)
            else:
                dx = launch(g, kt, None, strides, None, True)[(slice(None),) + tuple(slice(n) for n in x.shape[1:-1])]
        if ctx.needs_input_grad[1]:
            support = tuple(kernel.shape[:rank])
            dw = wgrad(gy, x, support, strides, True) if up else wgrad(x, gy, support, strides, False)
            dw = dw.to(kernel.dtype)
        if has_bias and ctx.needs_input_grad[2]:
            db = gy.float().sum(dim=tuple(range(rank + 1)))
        return dx, dw, db, None, None, None, None


def _conv_dispatch(rank, x, kernel, bias, strides, activation, up, **launch_args):
    needs = torch.is_grad_enabled() and (x.requires_grad or kernel.requires_grad
                                         or (bias is not None and bias.requires_grad))
    if needs:
        return _ConvFunction.apply(x, kernel, bias, strides, activation, up, rank)
    return _CONV_KERNELS[rank][0](x, kernel, bias, strides, activation, up, **launch_args)


def conv2d_down(x, kernel, bias=None, stride=1, activation=None, weights_key=0):
    """Analysis correlation (signal_conv.py:663-690): NHWC x, HWIO kernel, `same_zeros`.  weights_key: a number that
    names this VALUE of `kernel` (include/tfc_hip.h, tfc_conv2d_weights_key): its packed fragments are kept between
    calls; 0: packed per call."""
    return _conv_dispatch(2, x, kernel, bias, stride, activation, False, weights_key=weights_key)


def conv2d_up(x, kernel, bias=None, stride=1, activation=None, weights_key=0):
    """Synthesis transposed convolution (signal_conv.py:778-847, extra_pad_end=True)."""
    return _conv_dispatch(2, x, kernel, bias, stride, activation, True, weights_key=weights_key)


def conv3d_down(x, kernel, bias=None, strides=1, activation=None):
    """Analysis correlation of rank 3 (signal_conv.py:663-690): NDHWC x, DHWIO kernel, `same_zeros`, one stride per
    axis; out = ceil(in / s).  Rank 1 is d = h = 1."""
    return _conv_dispatch(3, x, kernel, bias, _ntuple(strides, 3), activation, False)


def conv3d_up(x, kernel, bias=None, strides=1, activation=None):
    """Synthesis transposed convolution of rank 3 (signal_conv.py:778-847, extra_pad_end=True); out = in * s."""
    return _conv_dispatch(3, x, kernel, bias, _ntuple(strides, 3), activation, True)


def pad3d(x, pads, reflect=False):
    """Padding of an NDHWC tensor, ((front, back), (top, bottom), (left, right)), as two pad2d calls: depth on the
    [n, d, 1, h*w*c] view, then H and W on the [n*d, h, w, c] view."""
    (f, k), ph, pw = pads
    n, d, h, w, c = x.shape
    if f or k:
        x = pad2d(x.reshape(n, d, 1, h * w * c), (f, k), (0, 0), reflect=reflect).reshape(n, d + f + k, h, w, c)
        d = d + f + k
    if any(ph) or any(pw):
        x = pad2d(x.reshape(n * d, h, w, c), ph, pw, reflect=reflect)
        x = x.reshape(n, d, x.shape[1], x.shape[2], c)
    return x


def gdn_backward(x, grad, beta, gamma, inverse=False, rectify=False, alpha=1, epsilon=1):
    """Gradients of gdn_forward w.r.t. (x, beta, gamma) on the HIP kernel (alpha in {1, 2}, epsilon in {1, .5};
    the general exponents go through `gdn_general_composite`)."""
    _lib.require_device()
    if alpha not in (1, 2) or epsilon not in (1, 0.5):
        raise NotImplementedError("tfc_gdn_backward implements alpha in {1, 2} and epsilon in {1, .5}")
    x = x.contiguous()
    grad = grad.contiguous()
    C = x.shape[-1]
    beta = beta.detach().to(x.device, torch.float32).contiguous()
    gamma = gamma.detach().to(x.device, torch.float32).contiguous()
    dx = torch.empty_like(x)
    dbeta = torch.zeros(C, dtype=torch.float32, device=x.device)
    dgamma = torch.zeros(C, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tfc_gdn_backward(
        x.data_ptr(), grad.data_ptr(), dx.data_ptr(), _DTYPE_CODE[x.dtype], x.numel() // C, C,
        beta.data_ptr(), gamma.data_ptr(), int(bool(inverse)), int(bool(rectify)), int(alpha),
        1 if epsilon == 0.5 else 0, dbeta.data_ptr(), dgamma.data_ptr(), _lib.stream_ptr()))
    return dx, dbeta, dgamma


def gdn_general_composite(x, beta, gamma, alpha, epsilon, inverse=False, rectify=False):
    """The layer with general exponents as differentiable device tensor ops (float32 arithmetic): the
    training path of learned alpha / epsilon, whose gradients d/dalpha and d/depsilon the fused backward
    kernel does not produce.  Same formula and op order as gdn.py:377-416; the forward-only (inference)
    path of the same configuration is `gdn_forward` on the HIP kernel."""
    _lib.require_device()
    xf = x.float()
    if rectify:
        xf = torch.relu(xf)
    norm = torch.pow(xf, alpha) @ gamma.to(xf.device, torch.float32) + beta.to(xf.device, torch.float32)
    norm = torch.pow(norm, epsilon)
    y = xf * norm if inverse else xf / norm
    return y.to(x.dtype)


def image_to_unit(x, dtype):
    """uint8 image tensor -> dtype(x) / 255 in one pass (the input scaling of the models' analysis transforms:
    bls2017.py:164-170, bmshj2018.py:219-224).  Other inputs take the torch expression."""
    if x.dtype != torch.uint8 or dtype not in _DTYPE_CODE or not x.is_cuda or not x.is_contiguous():
        return x.to(dtype) / 255.0
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(_lib.lib().tfc_image_to_unit(x.data_ptr(), y.data_ptr(), _DTYPE_CODE[dtype], x.numel(), _lib.stream_ptr()))
    return y


def unit_to_image(x):
    """saturate_cast(round(x * 255), uint8) with the product rounded to x's dtype, in one pass (the output of the
    models' synthesis transforms: bls2017.py:186-190, bmshj2018.py:262-264)."""
    if x.dtype not in _DTYPE_CODE or not x.is_cuda or not x.is_contiguous():
        return torch.clamp(torch.round((x * 255.0).float()), 0, 255).to(torch.uint8)
    y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().tfc_unit_to_image(x.data_ptr(), _DTYPE_CODE[x.dtype], y.data_ptr(), x.numel(), _lib.stream_ptr()))
    return y


def index_prepare(indexes, num_tables):
    """int32(min(max(indexes, 0), num_tables - 1)) in one pass, or None where the torch ops have to do it (integer or
    non-contiguous indexes, gradients wanted)."""
    if (indexes.dtype not in _DTYPE_CODE or not indexes.is_cuda or not indexes.is_contiguous()
            or (torch.is_grad_enabled() and indexes.requires_grad)):
        return None
    out = torch.empty(indexes.shape, dtype=torch.int32, device=indexes.device)
    _lib.check(_lib.lib().tfc_index_prepare(indexes.data_ptr(), _DTYPE_CODE[indexes.dtype], out.data_ptr(),
                                            indexes.numel(), int(num_tables), _lib.stream_ptr()))
    return out


def pad2d(x, pad_h, pad_w, reflect=False):
    """Spatial padding of an NHWC tensor: zeros (tf.pad CONSTANT) or mirror without the edge sample (tf.pad REFLECT) —
    SignalConv2D's pre-pad (signal_conv.py:880-893).  One HBM-bound kernel (tfc_pad2d) where no gradient is wanted and
    the tensor is on the device; differentiable tensor ops (zero pad / index gathers) otherwise."""
    (t, b), (l, r) = (int(pad_h[0]), int(pad_h[1])), (int(pad_w[0]), int(pad_w[1]))
    if t == b == l == r == 0:
        return x
    n, h, w, c = x.shape
    if reflect and (max(t, b) >= h or max(l, r) >= w):
        raise ValueError(f"reflect padding {(t, b), (l, r)} must be smaller than the input's {(h, w)}")
    needs = torch.is_grad_enabled() and x.requires_grad
    if x.is_cuda and not needs and x.element_size() in (2, 4):
        x = x.contiguous()
        y = torch.empty((n, h + t + b, w + l + r, c), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().tfc_pad2d(x.data_ptr(), y.data_ptr(), x.element_size(), n, h, w, c, t, b, l, r,
                                        int(bool(reflect)), _lib.stream_ptr()))
        return y
    if not reflect:
        return torch.nn.functional.pad(x, (0, 0, l, r, t, b))

    def mirror(length, before, after):
        i = torch.arange(-before, length + after, device=x.device).abs()
        return torch.where(i >= length, 2 * (length - 1) - i, i)
    return x.index_select(1, mirror(h, t, b)).index_select(2, mirror(w, l, r))


def _pool_windows(x, k, s):
    """The k * k shifted views of an NHWC tensor whose element [n, i, j] is that of window (i, j), in the window's
    row-major order -> [N, OH, OW, k * k, C]."""
    n, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    return torch.stack([x[:, i:i + s * (oh - 1) + 1:s, j:j + s * (ow - 1) + 1:s]
                        for i in range(k) for j in range(k)], dim=3)


def _pool_args(x, kernel_size, stride):
    k, s = int(kernel_size), int(stride)
    if x.dim() != 4:
        raise ValueError(f"Input tensor must have rank 4, received shape {tuple(x.shape)}.")
    if k < 1 or s < 1 or x.shape[1] < k or x.shape[2] < k:
        raise ValueError(f"a {x.shape[1]} x {x.shape[2]} image holds no {k} x {k} window (stride {s})")
    return k, s


def max_pool2d_reference(x, kernel_size=3, stride=2):
    """The definition of `max_pool2d` as differentiable tensor ops: NHWC, no padding, out = (in - k) // s + 1.  The
    gradient of a window goes to its FIRST maximum in row-major order (torch.argmax returns the first): what
    `max_pool2d` evaluates for a CPU tensor."""
    k, s = _pool_args(x, kernel_size, stride)
    win = _pool_windows(x, k, s)
    first = win.detach().float().argmax(dim=3, keepdim=True) if win.dtype == torch.bfloat16 else \
        win.detach().argmax(dim=3, keepdim=True)
    return win.gather(3, first).squeeze(3)


class _MaxPoolFunction(torch.autograd.Function):
    """tfc_maxpool2d_forward / _backward (include/tfc_hip.h): the forward keeps x, the backward finds the winners again."""

    @staticmethod
    def forward(ctx, x, k, s):
        x = x.contiguous()
        n, h, w, c = x.shape
        y = torch.empty((n, (h - k) // s + 1, (w - k) // s + 1, c), dtype=x.dtype, device=x.device)
        _lib.check(_lib.lib().tfc_maxpool2d_forward(x.data_ptr(), y.data_ptr(), _DTYPE_CODE[x.dtype], n, h, w, c, k, s,
                                                    _lib.stream_ptr()))
        ctx.save_for_backward(x)
        ctx.cfg = (k, s)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        k, s = ctx.cfg
        n, h, w, c = x.shape
        gy = gy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().tfc_maxpool2d_backward(x.data_ptr(), gy.data_ptr(), dx.data_ptr(), _DTYPE_CODE[x.dtype],
                                                     n, h, w, c, k, s, _lib.stream_ptr()))
        return dx, None, None


def max_pool2d(x, kernel_size=3, stride=2):
    """Max-pool of an NHWC tensor, window `kernel_size`, no padding, out = (in - k) // s + 1, on the HIP kernels
    (float32 / bfloat16); differentiable in x, ties to the first element of a window.  CPU tensors take
    `max_pool2d_reference`."""
    k, s = _pool_args(x, kernel_size, stride)
    if not x.is_cuda:
        return max_pool2d_reference(x, k, s)
    if x.dtype not in _DTYPE_CODE:
        raise TypeError(f"max-pool kernel supports float32 and bfloat16, got {x.dtype}")
    return _MaxPoolFunction.apply(x, k, s)


class _UnitNormalize(torch.autograd.Function):
    """f / (|f| + eps) over the last axis with its derivative written out, g / (n + eps) - f (f . g) / (n (n + eps)^2)
    and the second term 0 where n = 0: autograd's own sqrt gives inf * 0 at an all-zero pixel."""

    @staticmethod
    def forward(ctx, f, eps):
        n = f.pow(2).sum(dim=-1, keepdim=True).sqrt()
        ctx.save_for_backward(f, n)
        ctx.eps = eps
        return f / (n + eps)

    @staticmethod
    def backward(ctx, g):
        f, n = ctx.saved_tensors
        dot = (f * g).sum(dim=-1, keepdim=True)
        second = torch.where(n > 0, dot / (n * (n + ctx.eps) ** 2), torch.zeros_like(n))
        return g / (n + ctx.eps) - f * second, None


def _distance_args(f0, f1, w):
    if f0.shape != f1.shape or f0.dim() < 3:
        raise ValueError(f"feature shapes {tuple(f0.shape)} / {tuple(f1.shape)} must match and be [N, ..., C]")
    c = f0.shape[-1]
    if w.shape != (c,):
        raise ValueError(f"weight shape {tuple(w.shape)} does not match C={c}")
    n = f0.shape[0]
    p = f0.numel() // (n * c) if n else 1
    if p < 1:
        raise ValueError(f"features {tuple(f0.shape)} hold no pixel")
    return n, p, c


def lpips_distance_reference(f0, f1, w, epsilon=1e-10):
    """The definition of `lpips_distance` as differentiable tensor ops in float32 (a float64 input stays float64), the
    normalisation's gradient in the explicit form: what `lpips_distance` evaluates for CPU tensors."""
    n, p, c = _distance_args(f0, f1, w)
    ft = torch.float64 if f0.dtype == torch.float64 else torch.float32
    u = _UnitNormalize.apply(f0.to(ft).reshape(n, p, c), float(epsilon))
    v = _UnitNormalize.apply(f1.to(ft).reshape(n, p, c), float(epsilon))
    return ((u - v) ** 2 * w.to(ft)).sum(dim=-1).mean(dim=-1)


class _LpipsDistanceFunction(torch.autograd.Function):
    """tfc_lpips_distance_forward / _backward (include/tfc_hip.h).  A gradient nobody needs is not written."""

    @staticmethod
    def forward(ctx, f0, f1, w, epsilon):
        n, p, c = _distance_args(f0, f1, w)
        f0, f1 = f0.contiguous(), f1.to(f0.dtype).contiguous()
        d = torch.empty(n, dtype=torch.float32, device=f0.device)
        _lib.check(_lib.lib().tfc_lpips_distance_forward(
            f0.data_ptr(), f1.data_ptr(), w.data_ptr(), d.data_ptr(), _DTYPE_CODE[f0.dtype], n, p, c, epsilon,
            _lib.stream_ptr()))
        ctx.save_for_backward(f0, f1, w)
        ctx.cfg = (n, p, c, epsilon)
        return d

    @staticmethod
    def backward(ctx, g):
        f0, f1, w = ctx.saved_tensors
        n, p, c, epsilon = ctx.cfg
        g = g.to(torch.float32).contiguous()
        df0 = torch.empty_like(f0) if ctx.needs_input_grad[0] else None
        df1 = torch.empty_like(f1) if ctx.needs_input_grad[1] else None
        mask = (1 if df0 is not None else 0) | (2 if df1 is not None else 0)
        _lib.check(_lib.lib().tfc_lpips_distance_backward(
            g.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(), _ptr(df0), _ptr(df1), _DTYPE_CODE[f0.dtype],
            n, p, c, epsilon, mask, _lib.stream_ptr()))
        return df0, df1, None, None


def lpips_distance(f0, f1, w, epsilon=1e-10):
    """One tap of LPIPS: features f0, f1 [N, ..., C] (float32 / bfloat16), w [C] -> float32 [N],
    mean over pixels of sum_c w[c] (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2, in one pass on the HIP kernel;
    differentiable in f0 and f1 (w is frozen).  CPU tensors take `lpips_distance_reference`."""
    if not f0.is_cuda:
        return lpips_distance_reference(f0, f1, w, epsilon)
    if f0.dtype not in _DTYPE_CODE:
        raise TypeError(f"LPIPS distance kernel supports float32 and bfloat16, got {f0.dtype}")
    if w.requires_grad:
        raise ValueError("the LPIPS layer weights are frozen: lpips_distance gives no gradient for w")
    w = w.detach().to(f0.device, torch.float32).contiguous()
    return _LpipsDistanceFunction.apply(f0, f1, w, float(epsilon))
