"""`SignalConv1D`, `SignalConv2D` and `SignalConv3D` (python/layers/signal_conv.py:61-1047), every configuration the
reference implements: the models' (`same_zeros`, explicit padding, extra_pad_end, strides on one side only) straight on
the fused kernels, the others (`valid`, `same_reflect`, extra_pad_end=False, up + down strides, unequal strides, even
supports, channel_separable) as a pad and a crop around the same kernels.  One rank-generic class holds the layer; a
rank class supplies the kernels it runs on (rank 2: tfc_conv2d_*; rank 3: tfc_conv3d_*; rank 1: rank 3 with d = h = 1),
as the reference's `_conv_class_factory` does."""
from __future__ import annotations

import math
import os

import torch

from . import cached, functional, parameters
from .functional import _ntuple
from .gdn import GDN

__all__ = ["SignalConv1D", "SignalConv2D", "SignalConv3D"]


# ---------------------------------------------------------------------------------------------------------------------
# Every configuration but the models' (`valid` — the reference's default —, `same_reflect`, pre-padded `same_zeros`,
# extra_pad_end=False, up- AND downsampling, unequal strides, even kernel supports, channel_separable), as a pad and a
# crop around the same two kernels.  With u the zero-upsampled (pre-padded) input, the reference computes
# (signal_conv.py:692-847)
#   correlation:  c[i] = sum_t u[i + t] w[t]           ("valid"), kept at i = 0, sd, 2 sd, ...
#   convolution:  f[m] = sum_j w[j] u[m - j]           ("full"),  kept at m = start, start + sd, ... < L_full - stop
# and the kernels compute  corr_down_s(x)[i] = sum_t x[i s + t - k // 2] w[t]  (zeros outside x) and
# conv_up_s(x)[n] = f[n + k // 2] over n in [0, len(x) s): a few zero samples in front / behind the input move the
# kernels' windows onto the positions wanted, per axis.  The kernel runs an axis at stride `ks`, which is the stride the
# layer wants or 1 (what the rank's kernels take); the rest is a step of the output slice (down) or zeros between the
# input's samples (up, done by the caller: `length` is the input's either way).
# ---------------------------------------------------------------------------------------------------------------------
def _corr_window(k, length, ks, sd):
    """Correlation along one axis -> (zeros in front of the input, slice of corr_down_ks's output)."""
    e = (-(k // 2)) % ks
    a = (k // 2 + e) // ks
    return e, slice(a, a + (length - k) // ks + 1, sd // ks)


def _transposed_window(k, length, ks, su, sd, prepad, extra_pad_end):
    """Convolution of the input upsampled by su along one axis -> ((zeros in front, behind) of conv_up_ks's input, slice
    of its output).  prepad: the (front, back) `same_*` padding the input carries already, None for `valid`."""
    lup = length * su
    lfull = lup + (k - 1) - (0 if extra_pad_end else su - 1)
    if prepad is None:
        start = stop = k - 1
    else:
        start, stop = prepad[0] * su + k // 2, prepad[1] * su + (k - 1) // 2
    end = lfull - stop
    a = max(0, -(-(k // 2 - start) // ks))
    b = max(0, -(-(end - k // 2 - lup) // ks))
    lo = start - k // 2 + a * ks
    return (a, b), slice(lo, max(lo, end - k // 2 + a * ks), sd)


def _spatial(y, slices):
    """y[:, *slices]: one slice per spatial axis."""
    return y[(slice(None),) + tuple(slices)]


def _fused_relu(act):
    return "relu" if act in (torch.relu, torch.nn.functional.relu, "relu") or isinstance(act, torch.nn.ReLU) else None


class SignalConv(torch.nn.Module):
    """Same constructor arguments as the reference (signal_conv.py:279-296).  Weights: `kernel_real` / `kernel_imag`
    (kernel_parameter="rdft") or `kernel_variable` (kernel_parameter="variable"), and `bias`
    (signal_conv_test.py:38-40).  A rank class sets `_rank`, the device calls `_down`, `_up`, `_pad` and what its
    kernels take (`_kernel_strides`, `_narrow_channels`, `_pads_channels_in_forward`, `_unit_axes`)."""

    _rank = None
    # the kernels' rank is _unit_axes + _rank: forward() runs on the view with that many axes of length 1 in front of
    # the spatial ones (kernel support and strides 1 there)
    _unit_axes = 0
    # signal_conv.py:416-419: None means padding.startswith("same_")
    _extra_pad_end_default = None
    # the kernels take 1 ... _narrow_channels or a multiple of 16 input channels; zero channels are added in forward()
    # for every configuration, or by the two paths themselves (rank 2, whose separable kernel is padded once dense)
    _narrow_channels = 0
    _pads_channels_in_forward = True

    def __init__(self, filters, kernel_support, corr=False, strides_down=1, strides_up=1,
                 padding="valid", extra_pad_end=None, channel_separable=False,
                 data_format="channels_last", activation=None, use_bias=False, use_explicit=True,
                 kernel_parameter="rdft", bias_parameter="variable", kernel_initializer=None,
                 bias_initializer=None, in_channels=None):
        super().__init__()
        r = self._rank
        self.filters = int(filters)
        self.kernel_support = _ntuple(kernel_support, r)
        self.corr = bool(corr)
        self.strides_down, self.strides_up = _ntuple(strides_down, r), _ntuple(strides_up, r)
        if not len(self.kernel_support) == len(self.strides_down) == len(self.strides_up) == r:
            raise ValueError(f"kernel_support and strides must have {r} elements")
        self.padding = str(padding).lower()
        if self.padding not in ("valid", "same_zeros", "same_reflect"):
            raise ValueError(f"Unsupported padding mode: '{padding}'.")
        if extra_pad_end is None:
            extra_pad_end = self._extra_pad_end_default
        self.extra_pad_end = self.padding.startswith("same_") if extra_pad_end is None else bool(extra_pad_end)
        self.channel_separable = bool(channel_separable)
        if data_format not in ("channels_last", "channels_first"):
            raise ValueError(f"Unknown data format: '{data_format}'.")
        self.data_format = data_format
        self.activation = activation
        self.use_bias = bool(use_bias)
        self.use_explicit = bool(use_explicit)
        # a tensor, a callable (e.g. a `parameters.Parameter`) or one of the strings (signal_conv.py:222-236)
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
        # (signal_conv.py:577-586: same text, so that callers' `assertRaisesRegex(NotImplementedError, "SignalConv")` hold)
        raise NotImplementedError(
            f"The provided combination of {type(self).__name__} arguments is not currently "
            f"implemented (filters={self.filters}, kernel_support={self.kernel_support}, "
            f"corr={self.corr}, strides_down={self.strides_down}, strides_up={self.strides_up}, "
            f"channel_separable={self.channel_separable}, data_format={self.data_format}, "
            f"padding={self.padding}). Try using odd-length kernels or turning off separability?")

    def _check_implemented(self):
        """The combinations the reference implements (signal_conv_test.py:317-349 `is_implemented`): anything else
        raises NotImplementedError, as there."""
        odd = all(s % 2 == 1 for s in self.kernel_support)
        can_use_transpose = not self.corr or odd
        must_use_transpose = any(s != 1 for s in self.strides_up) or (not self.corr and not odd)
        if must_use_transpose and not can_use_transpose:
            self._raise_notimplemented()
        if self.channel_separable and (self._rank > 2 or any(s != self.strides_up[0] for s in self.strides_up)
                                       or (must_use_transpose and self.filters != 1)):
            self._raise_notimplemented()

    def _is_model_configuration(self):
        """The configuration the models use and the kernels serve directly, in one launch: `same_zeros`, explicit
        padding, extra_pad_end, strides the kernels take, on one side only."""
        su, sd = self.strides_up, self.strides_down
        return (self.padding == "same_zeros" and not self.channel_separable and self.use_explicit
                and self.extra_pad_end and self._kernel_strides(su) == su and self._kernel_strides(sd) == sd
                and (all(s == 1 for s in sd) or all(s == 1 for s in su)))

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
            # Keras VarianceScaling(scale=1, fan_in, truncated normal) — signal_conv.py default: fan_in = prod(support) * Cin
            std = math.sqrt(1.0 / (math.prod(self.kernel_support) * cin)) / 0.87962566103423978
            k = torch.empty(shape)
            torch.nn.init.trunc_normal_(k, std=std, a=-2 * std, b=2 * std)
        k = torch.as_tensor(k).float()
        if self.kernel_parameter == "rdft":
            real, imag = parameters.rdft_from_kernel(k)
            self.kernel_real = torch.nn.Parameter(real.to(device))
            self.kernel_imag = torch.nn.Parameter(imag.to(device))
        else:
            self.kernel_variable = torch.nn.Parameter(k.to(device))

    def _bias_value(self):
        """The bias in use: the layer's own variable `bias`, or the tensor / callable given as `bias_parameter`."""
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
        return parameters.kernel_from_rdft(self.kernel_real, self.kernel_imag, self.kernel_support)

    # --- what a rank class supplies -----------------------------------------------------------------------------------
    def _kernel_strides(self, strides):
        """The strides, one per axis, at which the kernels can run a layer that wants `strides`."""
        return strides

    def _down(self, x, kernel, bias, strides, activation=None):
        raise NotImplementedError

    def _up(self, x, kernel, bias, strides, activation=None):
        raise NotImplementedError

    def _pad(self, x, pads, reflect=False):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------------------------------
    def _geometry(self):
        """(kernel support, strides_up, strides_down) as the kernels see them."""
        unit = (1,) * self._unit_axes
        return unit + self.kernel_support, unit + self.strides_up, unit + self.strides_down

    @staticmethod
    def _flipped(kernel):
        return kernel.flip(*range(kernel.dim() - 2))

    def _pad_channels(self, x, kernel):
        if x.shape[-1] > self._narrow_channels:
            x, kernel = functional.pad_channels(x), functional.pad_channels(kernel, dim=-2)
        return x, kernel

    def _forward_general(self, x, kernel):
        from ..ops.padding_ops import same_padding_for_kernel
        corr = self.corr
        k, su, sd = self._geometry()
        rank = len(k)
        odd = all(s % 2 == 1 for s in k)
        # the reference's kernel flips (signal_conv.py:861-880)
        if not corr and all(s == 1 for s in su) and odd:
            corr, kernel = True, self._flipped(kernel)
        elif corr and any(s != 1 for s in su) and odd:
            corr, kernel = False, self._flipped(kernel)
        if self.channel_separable:
            # out[..., c * F + f] = in[..., c] * kernel[..., c, f]: as a dense kernel that is zero off its diagonal blocks
            cin, f = kernel.shape[-2:]
            dense = kernel.new_zeros(kernel.shape[:-2] + (cin, cin * f))
            for ch in range(cin):
                dense[..., ch, ch * f:(ch + 1) * f] = kernel[..., ch, :]
            kernel = dense
        if not self._pads_channels_in_forward:
            x, kernel = self._pad_channels(x, kernel)
        if self.padding == "valid":
            prepad = (None,) * rank
        else:
            prepad = tuple(same_padding_for_kernel(k, corr, su))
            x = self._pad(x, prepad, reflect=self.padding == "same_reflect")
        lens = x.shape[1:1 + rank]
        if corr and all(s == 1 for s in su):
            if any(lens[d] < k[d] for d in range(rank)):
                return x.new_zeros((x.shape[0],) + (0,) * rank + (kernel.shape[-1],))
            ks = self._kernel_strides(sd)
            front, sl = zip(*(_corr_window(k[d], lens[d], ks[d], sd[d]) for d in range(rank)))
            return _spatial(self._down(self._pad(x, tuple((e, 0) for e in front)), kernel, None, ks), sl)
        if corr:
            self._raise_notimplemented()
        ks = self._kernel_strides(su)
        if ks != su:
            # what the kernels do not upsample: zeros behind every sample (and behind the last: the windows below
            # count from the input's length)
            step = tuple(su[d] // ks[d] for d in range(rank))
            up = x.new_zeros((x.shape[0],) + tuple(lens[d] * step[d] for d in range(rank)) + (x.shape[-1],))
            _spatial(up, (slice(None, None, s) for s in step))[...] = x
            x = up
        pads, sl = zip(*(_transposed_window(k[d], lens[d], ks[d], su[d], sd[d], prepad[d], self.extra_pad_end)
                         for d in range(rank)))
        return _spatial(self._up(self._pad(x, pads), kernel, None, ks), sl)

    def _forward_model(self, x, kernel, bias):
        act = self.activation
        fused = _fused_relu(act)
        if bias is not None:
            bias = bias.to(x.device)
        corr = self.corr
        _, su, sd = self._geometry()
        if corr and any(s != 1 for s in su):
            corr, kernel = False, self._flipped(kernel)              # signal_conv.py:875-880
        if corr:
            y = self._down(x, kernel, bias, sd, fused)
        else:
            y = self._up(x, kernel, bias, su, fused)
            if any(s != 1 for s in sd):
                y = _spatial(y, (slice(None, None, s) for s in sd))
        return y if act is None or fused else act(y)

    def forward(self, inputs):
        return self._forward(inputs)

    def _forward(self, inputs, with_bias=True):
        """`forward`, or with `with_bias=False` the same computation without the bias term."""
        if inputs.dim() != self._rank + 2:
            raise ValueError(f"Input tensor must have rank {self._rank + 2}, received shape {tuple(inputs.shape)}.")
        x = inputs.movedim(1, -1) if self.data_format == "channels_first" else inputs
        self.build(x.shape[-1], x.device)
        kernel = self.kernel.to(x.device)
        unit = self._unit_axes
        if unit:
            x, kernel = x[(slice(None),) + (None,) * unit], kernel[(None,) * unit]
        if self._pads_channels_in_forward and not self.channel_separable:
            x, kernel = self._pad_channels(x, kernel)
        bias = self._bias_value() if with_bias else None
        if self._is_model_configuration():
            y = self._forward_model(x, kernel, bias)
        else:
            y = self._forward_general(x, kernel)
            if bias is not None:
                y = y + bias.to(y.device, y.dtype)
            if self.activation is not None:
                y = torch.relu(y) if self.activation == "relu" else self.activation(y)
        if unit:
            y = y[(slice(None),) + (0,) * unit]
        return y.movedim(-1, 1) if self.data_format == "channels_first" else y


class SignalConv3D(SignalConv):
    """3-D signal convolution layer (signal_conv.py:1043-1047) on tfc_conv3d_*: one stride per axis."""
    _rank = 3

    def _down(self, x, kernel, bias, strides, activation=None):
        return functional.conv3d_down(x, kernel, bias, strides, activation)

    def _up(self, x, kernel, bias, strides, activation=None):
        return functional.conv3d_up(x, kernel, bias, strides, activation)

    def _pad(self, x, pads, reflect=False):
        return functional.pad3d(x, pads, reflect=reflect)


class SignalConv1D(SignalConv3D):
    """1-D signal convolution layer (signal_conv.py:1031-1035): the rank-3 kernels on the [n, 1, 1, w, c] view."""
    _rank = 1
    _unit_axes = 2


class SignalConv2D(cached.CachedValues, SignalConv):
    """2-D signal convolution layer (signal_conv.py:1037-1041) on tfc_conv2d_*: one stride for both axes (unequal
    strides run at stride 1), 1 ... 4 or a multiple of 16 input channels (other counts get zero channels up to the next
    multiple, in the forward pass and in both gradients).  Under no_grad it keeps the kernel of its
    RDFT parameters and names the value of its weights to the library (`keyed_weights`), and it takes a GDN layer as
    its activation into the convolution kernel."""
    _rank = 2
    # NOT the reference's default (signal_conv.py:284 there: None, as ranks 1 and 3 here)
    _extra_pad_end_default = True
    _narrow_channels = 4
    _pads_channels_in_forward = False
    _cache_attrs = ("_kernel_cache", "_wkey_cache")

    def _kernel_strides(self, strides):
        return strides if strides[0] == strides[1] else (1, 1)

    def _down(self, x, kernel, bias, strides, activation=None):
        return functional.conv2d_down(x, kernel, bias, strides[0], activation)

    def _up(self, x, kernel, bias, strides, activation=None):
        return functional.conv2d_up(x, kernel, bias, strides[0], activation)

    def _pad(self, x, pads, reflect=False):
        return functional.pad2d(x, pads[0], pads[1], reflect=reflect)

    @property
    def kernel(self):
        if self._kernel_given is not None or self.kernel_real is None or torch.is_grad_enabled():
            return super().kernel
        # inference (compress / decompress run under no_grad): the inverse RDFT once per parameter version
        # instead of once per call — 11 small FFTs per bmshj2018 step, and an FFT plan shared by host
        # threads that code batch slices on different streams is not safe to execute concurrently
        key = (self.kernel_real.data_ptr(), cached.version_of(self.kernel_real), self.kernel_imag.data_ptr(),
               cached.version_of(self.kernel_imag), str(self.kernel_real.device))
        hit = self.__dict__.get("_kernel_cache")
        if key[1] is None or key[3] is None:
            hit = None                                        # inference tensors carry no version counter: recompute
        if hit is None or hit[0] != key:
            k = super().kernel.contiguous()
            if k.is_cuda:
                torch.cuda.current_stream().synchronize()      # complete before another stream reads it
            self.__dict__["_kernel_cache"] = hit = (key, k)
        return hit[1]

    # Keyed (kept) packed weights under no_grad (cached.KEYED_WEIGHTS): per layer / per class off by assigning
    # `keyed_weights = False` (every call then packs its fragments from the tensor it is given, as training does).
    # WHAT THE KEY SEES: the parameters' storage address, their autograd version counter and the layer's
    # `weights_generation`.  An in-place write through `.data` (`p.data.copy_(ema)`, manual weight loading) advances
    # neither address nor version — after such a write call `weights_changed()` (bumps the generation; the old
    # fragments are released in stream order) or `invalidate_kernel_cache()`.  load_state_dict, .to() / .cuda() /
    # .half(), train() / eval() do it themselves; optimizer steps and every other autograd-visible in-place op advance
    # the version counter.
    keyed_weights = cached.KEYED_WEIGHTS
    weights_generation = 0

    def weights_changed(self):
        """Tell the layer its weights were written behind autograd's back (`.data` writes): the kept inference kernel
        and the library's packed fragments of the old value are dropped."""
        self.weights_generation = self.weights_generation + 1
        self.invalidate_kernel_cache()

    def _inference_weights_key(self):
        """The key of the kernel's current value, or 0: gradients enabled (the weights are about to change), a kernel
        given as a tensor / callable (computed per call), parameters without version counters, or `keyed_weights` off."""
        if torch.is_grad_enabled() or self._kernel_given is not None or not self.keyed_weights:
            return 0
        src = (self.kernel_variable,) if self.kernel_variable is not None else (self.kernel_real, self.kernel_imag)
        if any(t is None or not t.is_cuda for t in src):
            return 0
        ident = tuple((t.data_ptr(), cached.version_of(t)) for t in src) + (str(src[0].device),)
        if any(v is None for _, v in ident[:-1]):
            return 0
        ident = ident + (self.weights_generation,)
        hit = self.__dict__.get("_wkey_cache")
        if hit is None or hit[0] != ident:
            if hit is not None:
                cached.drop_weights_key(hit[1])
            self.__dict__["_wkey_cache"] = hit = (ident, cached.new_weights_key())
        return hit[1]

    def invalidate_kernel_cache(self):
        """Drops the kept inference kernel and the library's packed fragments of the weights."""
        self.__dict__.pop("_kernel_cache", None)
        hit = self.__dict__.pop("_wkey_cache", None)
        if hit is not None:
            cached.drop_weights_key(hit[1])

    def _forward_model(self, x, kernel, bias):
        act = self.activation
        fused = _fused_relu(act)
        corr, up, down = self.corr, self.strides_up[0], self.strides_down[0]
        x, kernel = self._pad_channels(x, kernel)              # (the models' counts fit and pass through as they are)
        wkey = self._inference_weights_key() if x.is_cuda else 0
        if corr and up != 1:
            corr, kernel = False, self._flipped(kernel)        # signal_conv.py:875-880
            wkey = wkey | cached.FLIPPED if wkey else 0
        gdn = self._fusable_gdn(act, x, kernel, corr, up, down)
        if gdn is not None:
            # GDN / IGDN as the activation (signal_conv.py:948-950 applying gdn.py:371-421): one kernel where the
            # convolution kernel that takes the layer can (functional.conv2d_gdn), else the GDN kernel on its output
            prepared = act._prepared_params(gdn[0], gdn[1], x.dtype)
            y, done = functional.conv2d_gdn(x, kernel, bias, down if corr else up, not corr, prepared,
                                            act.inverse, weights_key=wkey)
            if not done:
                y = functional.gdn_forward(y, gdn[0], gdn[1], act.inverse, False, 1.0, 1.0, prepared=prepared)
            return y
        if corr:
            y = functional.conv2d_down(x, kernel, bias, down, fused, weights_key=wkey)
        else:
            y = functional.conv2d_up(x, kernel, bias, up, fused, weights_key=wkey)
            if down != 1:
                y = y[:, ::down, ::down]
        return y if act is None or fused else act(y)

    # GDN / IGDN as the activation inside the convolution kernel (functional.conv2d_gdn): True / False, or None = by the
    # size of the layer's output (TFC_CONV_GDN=1 / 0 in the environment set it; unset = None).  Measured with steps in
    # flight (profiles/r04_notes.md): on bls2017 at 512 x 256x256 (outputs of 0.2 - 0.8 GB) the fused layers take
    # 9.5 -> 8.4 ms per step on one box, 8.78 -> 8.63 on another; on bmshj2018 at 128 x 768x512, whose 1.2 and 4.8 GB
    # maps are HBM-bound GDN launches of 0.55 and 2.2 ms, the step is level whether none, the small or all layers fuse
    # (four same-box comparisons), and a lone step wins 0.6 ms.  Default: no limit (TFC_CONV_GDN_MAX_MB = 0) — a model
    # step then has no GDN launches behind third-generation convolutions; a limit in MB restores the by-size rule.
    fuse_gdn_activation = {"": None, "0": False}.get(os.environ.get("TFC_CONV_GDN", ""), True)
    fuse_gdn_max_bytes = int(os.environ.get("TFC_CONV_GDN_MAX_MB", "0")) << 20
    # The image-side layer (three input channels) is different: its time is its output's HBM traffic, not the matrix
    # cores, and conv_image_gdn_kernel writes the normalised activations without the round trip (bmshj2018's first
    # layer at 128 x 768x512: 1.83 + 2.2 ms as two kernels).  On unless TFC_CONV_GDN_IMAGE=0.
    fuse_gdn_image = os.environ.get("TFC_CONV_GDN_IMAGE", "1") not in ("", "0")

    def _fusable_gdn(self, act, x, kernel, corr, up, down):
        """(beta, gamma) when `act` is a GDN layer in the configuration the fused entry point covers — inference on the
        layer's own variables, bfloat16, alpha = epsilon = 1, no rectification, channels-last inside — else None."""
        image_side = self.fuse_gdn_image and corr and kernel.shape[-2] <= 4 and not getattr(act, "inverse", True)
        wanted = self.fuse_gdn_activation
        if wanted is None:
            scale = (1.0 / down if corr else float(up)) ** 2
            wanted = self.fuse_gdn_max_bytes <= 0 or \
                x.shape[0] * x.shape[1] * x.shape[2] * scale * kernel.shape[-1] * 2 <= self.fuse_gdn_max_bytes
        if not (wanted or image_side) or not isinstance(act, GDN) or torch.is_grad_enabled() \
                or not x.is_cuda or x.dtype != torch.bfloat16:
            return None
        if (not corr and down != 1) or act.rectify or act._beta_fixed is not None or act._gamma_fixed is not None:
            return None
        if act.data_format != "channels_last":          # (the activation is applied to the channels-last tensor inside)
            return None
        alpha, epsilon = act.alpha, act.epsilon
        if torch.is_tensor(alpha) or torch.is_tensor(epsilon) or float(alpha) != 1.0 or float(epsilon) != 1.0:
            return None
        cout = kernel.shape[-1]
        act.build(cout, x.device)
        beta, gamma = act.beta.to(x.device), act.gamma.to(x.device)
        if beta.shape != (cout,) or cout % 32 or cout > 256:
            return None
        return beta, gamma
