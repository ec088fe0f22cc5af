"""Torch-CPU float64 statements of what the two rank-2 convolution kernels compute (include/tfc_hip.h; pinned to
torch on the GPU by tests/test_signal_conv_gpu.py), per axis:
    down_s(x)[i] = sum_t x[i s + t - k // 2] w[t]                i < ceil(len / s), zeros outside x
    up_s(x)[n]   = f[n + k // 2],  f[m] = sum_i x[i] w[m - i s]    n < len s
so that the Keras layers' and the HiFiC model's host logic can be checked without a device (the pattern of
tests/test_signal_conv_nd_cpu.py)."""
import torch


def _epilogue(y, bias, activation):
    if bias is not None:
        y = y + bias.double()
    return torch.relu(y) if activation == "relu" else y


def emu_down(x, kernel, bias=None, stride=1, activation=None, weights_key=0):
    kh, kw = kernel.shape[:2]
    out = [-(-x.shape[1 + a] // stride) for a in range(2)]
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2).double(), (kw // 2, kw + stride, kh // 2, kh + stride))
    y = torch.nn.functional.conv2d(xp, kernel.permute(3, 2, 0, 1).double(), stride=stride)[:, :, :out[0], :out[1]]
    return _epilogue(y.permute(0, 2, 3, 1), bias, activation).to(x.dtype).contiguous()


def emu_up(x, kernel, bias=None, stride=1, activation=None, weights_key=0):
    kh, kw = kernel.shape[:2]
    f = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2).double(), kernel.permute(2, 3, 0, 1).double(),
                                             stride=stride)
    f = torch.nn.functional.pad(f, (0, stride + kw, 0, stride + kh))
    y = f[:, :, kh // 2:kh // 2 + x.shape[1] * stride, kw // 2:kw // 2 + x.shape[2] * stride]
    return _epilogue(y.permute(0, 2, 3, 1), bias, activation).to(x.dtype).contiguous()


def install(monkeypatch):
    from compression_amd.layers import functional
    monkeypatch.setattr(functional, "conv2d_down", emu_down)
    monkeypatch.setattr(functional, "conv2d_up", emu_up)
