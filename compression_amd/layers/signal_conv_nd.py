"""`SignalConv1D` and `SignalConv3D` (python/layers/signal_conv.py:1031-1047, `_conv_class_factory`) on the rank-3
kernels (include/tfc_hip.h, tfc_conv3d_*).  A rank-1 layer runs as the rank-3 case d = h = 1.  The models'
configuration (`same_zeros`, explicit padding, extra_pad_end, strides on one side only) is one kernel launch; every
other configuration of the reference (`valid`, `same_reflect`, extra_pad_end=False, up + down strides, unequal strides,
even supports, rank-1 channel_separable) is a pad and a crop around the same two kernels, as in SignalConv2D."""
from __future__ import annotations

import math

import torch

from . import functional

__all__ = ["SignalConv1D", "SignalConv3D"]


def _tuple(v, rank):
    return (int(v),) * rank if isinstance(v, int) else tuple(int(s) for s in v)


def _rdft_from_kernel(kernel, rank):
    """[*support, I, O] kernel -> (real, imag) of its normalised RDFT over the support (parameters.py:85-127), [I, O, ...]."""
    spec = torch.fft.rfftn(kernel.movedim((-2, -1), (0, 1)).float(), dim=tuple(range(2, 2 + rank)))
    spec = spec / math.sqrt(math.prod(kernel.shape[:rank]))
    return spec.real.contiguous(), spec.imag.contiguous()


def _kernel_from_rdft(real, imag, support):
    spec = torch.complex(real.float(), imag.float()) * math.sqrt(math.prod(support))
    kernel = torch.fft.irfftn(spec, s=support, dim=tuple(range(2, 2 + len(support))))
    return kernel.movedim((0, 1), (-2, -1))


class _SignalConvND(torch.nn.Module):
    """Same constructor arguments as the reference (signal_conv.py:279-296).  Weights: `kernel_real` / `kernel_imag`
    (kernel_parameter="rdft") or `kernel` (kernel_parameter="variable"), and `bias`."""

    _rank = None

    def __init__(self, filters, kernel_support, corr=False, strides_down=1, strides_up=1,
                 padding="valid", extra_pad_end=None, channel_separable=False,
                 data_format="channels_last", activation=None, use_bias=False, use_explicit=True,
                 kernel_parameter="rdft", bias_parameter="variable", kernel_initializer=None,
                 bias_initializer=None, in_channels=None):
        super().__init__()
        r = self._rank
        self.filters = int(filters)
        self.kernel_support = _tuple(kernel_support, r)
        self.corr = bool(corr)
        self.strides_down, self.strides_up = _tuple(strides_down, r), _tuple(strides_up, r)
        if not len(self.kernel_support) == len(self.strides_down) == len(self.strides_up) == r:
            raise ValueError(f"kernel_support and strides must have {r} elements")
        self.padding = str(padding).lower()
        if self.padding not in ("valid", "same_zeros", "same_reflect"):
            raise ValueError(f"Unsupported padding mode: '{padding}'.")
        # signal_conv.py:416-419: None means padding.startswith("same_")
        self.extra_pad_end = self.padding.startswith("same_") if extra_pad_end is None else bool(extra_pad_end)
        self.channel_separable = bool(channel_separable)
        if data_format not in ("channels_last", "channels_first"):
            raise ValueError(f"Unknown data format: '{data_format}'.")
        self.data_format = data_format
        self.activation = activation
        self.use_bias = bool(use_bias)
        self.use_explicit = bool(use_explicit)
        if isinstance(kernel_parameter, str) and kernel_parameter not in ("rdft", "variable"):
            raise ValueError("kernel_parameter must be a tensor, a callable, 'rdft' or 'variable'")
        if isinstance(bias_parameter, str) and bias_parameter != "variable":
            raise ValueError("bias_parameter must be a tensor, a callable or 'variable'")
        self.kernel_parameter = kernel_parameter if isinstance(kernel_parameter, str) else "given"
        self._kernel_given = None if isinstance(kernel_parameter, str) else kernel_parameter
        self._bias_given = None if isinstance(bias_parameter, str) else bias_parameter
        self._kernel_init, self._bias_init = kernel_initializer, bias_initializer
        self.kernel_real = self.kernel_imag = self.kernel_variable = self.bias = None
        self._check_implemented()
        if in_channels is not None:
            self.build(int(in_channels))

    def _raise_notimplemented(self):
        # (signal_conv.py:577-586, the same text)
        raise NotImplementedError(
            f"The provided combination of {type(self).__name__} arguments is not currently "
            f"implemented (filters={self.filters}, kernel_support={self.kernel_support}, "
            f"corr={self.corr}, strides_down={self.strides_down}, strides_up={self.strides_up}, "
            f"channel_separable={self.channel_separable}, data_format={self.data_format}, "
            f"padding={self.padding}). Try using odd-length kernels or turning off separability?")

    def _check_implemented(self):
        """signal_conv_test.py:317-349 `is_implemented`: anything else raises NotImplementedError, as there."""
        odd = all(s % 2 == 1 for s in self.kernel_support)
        can_use_transpose = not self.corr or odd
        must_use_transpose = any(s != 1 for s in self.strides_up) or (not self.corr and not odd)
        if must_use_transpose and not can_use_transpose:
            self._raise_notimplemented()
        if self.channel_separable and (self._rank > 2 or any(s != self.strides_up[0] for s in self.strides_up)
                                       or (must_use_transpose and self.filters != 1)):
            self._raise_notimplemented()

    def build(self, cin, device=None):
        if self.kernel_real is not None or self.kernel_variable is not None:
            return
        if self.use_bias and self._bias_given is None and self.bias is None:
            b = self._bias_init((self.filters,)) if self._bias_init else torch.zeros(self.filters)
            self.bias = torch.nn.Parameter(b.float().to(device))
        if self._kernel_given is not None:
            return
        shape = self.kernel_support + (cin, self.filters)
        if self._kernel_init is not None:
            k = self._kernel_init(shape)
        else:
            # Keras VarianceScaling(scale=1, fan_in, truncated normal): fan_in = prod(support) * Cin
            std = math.sqrt(1.0 / (math.prod(self.kernel_support) * cin)) / 0.87962566103423978
            k = torch.empty(shape)
            torch.nn.init.trunc_normal_(k, std=std, a=-2 * std, b=2 * std)
        k = torch.as_tensor(k).float()
        if self.kernel_parameter == "rdft":
            real, imag = _rdft_from_kernel(k, self._rank)
            self.kernel_real = torch.nn.Parameter(real.to(device))
            self.kernel_imag = torch.nn.Parameter(imag.to(device))
        else:
            self.kernel_variable = torch.nn.Parameter(k.to(device))

    def _bias_value(self):
        if not self.use_bias:
            return None
        if self._bias_given is not None:
            return torch.as_tensor(self._bias_given() if callable(self._bias_given) else self._bias_given)
        return self.bias

    @property
    def kernel(self):
        if self._kernel_given is not None:
            return torch.as_tensor(self._kernel_given() if callable(self._kernel_given) else self._kernel_given)
        if self.kernel_variable is not None:
            return self.kernel_variable
        if self.kernel_real is None:
            raise RuntimeError("Kernel is not initialized yet. Call build().")
        return _kernel_from_rdft(self.kernel_real, self.kernel_imag, self.kernel_support)

    def _is_model_configuration(self):
        """`same_zeros`, explicit padding, extra_pad_end, strides on one side only: one kernel launch."""
        return (self.padding == "same_zeros" and not self.channel_separable and self.use_explicit
                and self.extra_pad_end
                and (all(s == 1 for s in self.strides_down) or all(s == 1 for s in self.strides_up)))

    # The reference's configurations as a pad and a crop around the two kernels, SignalConv2D._forward_general per axis.
    # With one stride per axis in the kernels, no zero upsampling is needed: every axis takes its own stride.
    def _forward_general(self, x, kernel):
        from ..ops.padding_ops import same_padding_for_kernel
        corr = self.corr
        ks, su, sd = self.kernel_support3, self.strides_up3, self.strides_down3
        odd = all(s % 2 == 1 for s in ks)
        # the reference's kernel flips (signal_conv.py:861-880)
        if not corr and all(s == 1 for s in su) and odd:
            corr, kernel = True, kernel.flip(0, 1, 2)
        elif corr and any(s != 1 for s in su) and odd:
            corr, kernel = False, kernel.flip(0, 1, 2)
        if self.channel_separable:
            # out[..., c * F + f] = in[..., c] * kernel[..., c, f]: a dense kernel that is zero off its diagonal blocks
            cin, f = kernel.shape[-2:]
            dense = kernel.new_zeros(kernel.shape[:3] + (cin, cin * f))
            for ch in range(cin):
                dense[..., ch, ch * f:(ch + 1) * f] = kernel[..., ch, :]
            kernel = dense
        if self.padding == "valid":
            prepad = ((0, 0),) * 3
        else:
            prepad = tuple(same_padding_for_kernel(ks, corr, su))
            x = functional.pad3d(x, prepad, reflect=self.padding == "same_reflect")
        if corr and all(s == 1 for s in su):
            lens = [x.shape[1 + d] for d in range(3)]
            if any(lens[d] < ks[d] for d in range(3)):
                return x.new_zeros((x.shape[0], 0, 0, 0, kernel.shape[-1]))
            e = [(-(ks[d] // 2)) % sd[d] for d in range(3)]
            xs = functional.pad3d(x, tuple((e[d], 0) for d in range(3)))
            y = functional.conv3d_down(xs, kernel, None, sd)
            sl = []
            for d in range(3):
                a = (ks[d] // 2 + e[d]) // sd[d]
                sl.append(slice(a, a + (lens[d] - ks[d]) // sd[d] + 1))
            return y[:, sl[0], sl[1], sl[2]]
        if corr:
            self._raise_notimplemented()
        pads, sl = [], []
        for d in range(3):
            k, length, s = ks[d], x.shape[1 + d], su[d]
            lup = length * s
            lfull = lup + (k - 1) - (0 if self.extra_pad_end else s - 1)
            if self.padding == "valid":
                start = stop = k - 1
            else:
                start, stop = prepad[d][0] * s + k // 2, prepad[d][1] * s + (k - 1) // 2
            end = lfull - stop
            a = max(0, -(-(k // 2 - start) // s))
            b = max(0, -(-(end - k // 2 - lup) // s))
            pads.append((a, b))
            lo = start - k // 2 + a * s
            sl.append(slice(lo, max(lo, end - k // 2 + a * s), sd[d]))
        y = functional.conv3d_up(functional.pad3d(x, tuple(pads)), kernel, None, su)
        return y[:, sl[0], sl[1], sl[2]]

    # rank-3 views of the layer's geometry (rank 1: d = h = 1)
    @property
    def kernel_support3(self):
        return (1, 1) * (self._rank == 1) + self.kernel_support

    @property
    def strides_up3(self):
        return (1, 1) * (self._rank == 1) + self.strides_up

    @property
    def strides_down3(self):
        return (1, 1) * (self._rank == 1) + self.strides_down

    def forward(self, inputs):
        if inputs.dim() != self._rank + 2:
            raise ValueError(f"Input tensor must have rank {self._rank + 2}, received shape {tuple(inputs.shape)}.")
        x = inputs.movedim(1, -1) if self.data_format == "channels_first" else inputs
        self.build(x.shape[-1], x.device)
        kernel = self.kernel.to(x.device)
        if self._rank == 1:
            x = x[:, None, None]
            kernel = kernel[None, None]
        cin = x.shape[-1]
        if cin % 16 and not self.channel_separable:
            # (the kernels take a multiple of 16 input channels: zero channels change nothing)
            extra = 16 - cin % 16
            x = torch.nn.functional.pad(x, (0, extra))
            kernel = torch.nn.functional.pad(kernel, (0, 0, 0, extra))
        act = self.activation
        if not self._is_model_configuration():
            y = self._forward_general(x, kernel)
            bias = self._bias_value()
            if bias is not None:
                y = y + bias.to(y.device, y.dtype)
            if act is not None:
                y = torch.relu(y) if act == "relu" else act(y)
        else:
            fused = "relu" if act in (torch.relu, torch.nn.functional.relu, "relu") or isinstance(
                act, torch.nn.ReLU) else None
            bias = self._bias_value()
            if bias is not None:
                bias = bias.to(x.device)
            corr, su, sd = self.corr, self.strides_up3, self.strides_down3
            if corr and any(s != 1 for s in su):
                corr, kernel = False, kernel.flip(0, 1, 2)           # signal_conv.py:875-880
            if corr:
                y = functional.conv3d_down(x, kernel, bias, sd, fused)
            else:
                y = functional.conv3d_up(x, kernel, bias, su, fused)
                if any(s != 1 for s in sd):
                    y = y[:, ::sd[0], ::sd[1], ::sd[2]]
            if act is not None and fused is None:
                y = act(y)
        if self._rank == 1:
            y = y[:, 0, 0]
        return y.movedim(-1, 1) if self.data_format == "channels_first" else y


class SignalConv1D(_SignalConvND):
    """1-D signal convolution layer (signal_conv.py:1031-1035)."""
    _rank = 1


class SignalConv3D(_SignalConvND):
    """3-D signal convolution layer (signal_conv.py:1043-1047)."""
    _rank = 3
