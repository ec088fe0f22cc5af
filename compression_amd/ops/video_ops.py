"""Video frames: the planes of YUV4MPEG2 frame bytes <-> the (y, cbcr) tensors of `Y4MDataset`, and YCbCr <-> RGB.

    unpack_frames   raw bytes -> y [N, H, W, 1], cbcr [N, h, w, 2]      (cc/kernels/y4m_dataset_kernels.cc:165-178)
    pack_frames     the inverse, for `Y4MWriter`
    ycbcr_to_rgb    (y, cbcr) -> [N, H, W, 3] on the 0...255 scale, what `model.compress` and `model.forward` take
    rgb_to_ycbcr    the inverse, so that reconstructions can be written back

Each runs one kernel of csrc/y4m.hip (tfc_y4m_unpack, tfc_y4m_pack, tfc_ycbcr_to_rgb, tfc_rgb_to_ycbcr) on device
tensors and has a `*_reference` twin of plain tensor ops, which CPU tensors take.  The definition of the conversions
(include/tfc_hip.h states it in full; tests/y4m_ref.py is the float64 form): (Kr, Kb) = (0.299, 0.114) for "bt601",
(0.2126, 0.0722) for "bt709", Kg = 1 - Kr - Kb; full range Y' = y, C' = c - 128, limited range Y' = (y - 16) 255 / 219,
C' = (c - 128) 255 / 224; R = Y' + 2 (1 - Kr) Cr', B = Y' + 2 (1 - Kb) Cb', G = Y' - (2 Kr (1 - Kr) / Kg) Cr'
- (2 Kb (1 - Kb) / Kg) Cb'.  4:2:0 chroma is upsampled "nearest" (c[i // 2, j // 2]) or "bilinear" with centre siting
(weights 0.75 / 0.25 towards the nearer neighbour, clamped at the edges), and subsampled as the mean of 2 x 2 blocks."""
from __future__ import annotations

import torch

from .. import _lib

__all__ = ["unpack_frames", "pack_frames", "ycbcr_to_rgb", "rgb_to_ycbcr", "unpack_frames_reference",
           "pack_frames_reference", "ycbcr_to_rgb_reference", "rgb_to_ycbcr_reference", "frame_bytes"]

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}      # (Kr, Kb)
MATRIX_CODE = {"bt601": 0, "bt709": 1}
UPSAMPLE_CODE = {"nearest": 0, "bilinear": 1}
DTYPE_CODE = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}
CHROMA_CODE = {"420": 420, "420jpeg": 420, "444": 444}


def _chroma_code(chroma):
    code = CHROMA_CODE.get(str(chroma))
    if code is None:
        raise ValueError(f"chroma must be '420' (or '420jpeg') or '444', got {chroma!r}")
    return code


def _chroma_shape(width, height, code):
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be positive, got {width} x {height}")
    if code == 420:
        if width % 2 or height % 2:
            raise ValueError(f"4:2:0 chroma format, but odd width or height ({width} x {height})")
        return height // 2, width // 2
    return height, width


def frame_bytes(width, height, chroma):
    """The bytes of one frame's planes (without the FRAME marker)."""
    h, w = _chroma_shape(width, height, _chroma_code(chroma))
    return width * height + 2 * h * w


def _check_raw(raw, num_frames, width, height, chroma, frame_stride, first_offset):
    if raw.dtype != torch.uint8:
        raise TypeError(f"raw must be uint8, got {raw.dtype}")
    if raw.dim() != 1 or not raw.is_contiguous():
        raise ValueError(f"raw must be a flat contiguous tensor, received shape {tuple(raw.shape)}")
    code = _chroma_code(chroma)
    h, w = _chroma_shape(width, height, code)
    size = width * height + 2 * h * w
    stride = size if frame_stride is None else int(frame_stride)
    if num_frames < 0:
        raise ValueError(f"num_frames must not be negative, got {num_frames}")
    if stride < size:
        raise ValueError(f"frame_stride {stride} is less than the {size} bytes of a frame")
    if first_offset < 0:
        raise ValueError(f"first_offset must not be negative, got {first_offset}")
    if num_frames and raw.numel() < first_offset + (num_frames - 1) * stride + size:
        raise ValueError(f"{num_frames} frames of stride {stride} from byte {first_offset} need "
                         f"{first_offset + (num_frames - 1) * stride + size} bytes, raw has {raw.numel()}")
    return code, h, w, size, stride


def check_planes(y, cbcr, what):
    """-> (y, cbcr, N, H, W, chroma code, squeeze): 4-D views of a batch or of one frame."""
    for name, t in (("y", y), ("cbcr", cbcr)):
        if t.dtype != torch.uint8:
            raise TypeError(f"{what}: {name} must be uint8, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
    if y.device != cbcr.device:
        raise ValueError(f"{what}: y and cbcr must be on the same device")
    squeeze = y.dim() == 3 and cbcr.dim() == 3
    if squeeze:
        y, cbcr = y[None], cbcr[None]
    if y.dim() != 4 or y.shape[3] != 1 or cbcr.dim() != 4 or cbcr.shape[3] != 2 or y.shape[0] != cbcr.shape[0]:
        raise ValueError(f"{what}: y must be [N, H, W, 1] and cbcr [N, h, w, 2], received {tuple(y.shape)} and "
                         f"{tuple(cbcr.shape)}")
    n, height, width = y.shape[:3]
    if width < 1 or height < 1:
        raise ValueError(f"{what}: width and height must be positive, got {width} x {height}")
    if tuple(cbcr.shape[1:3]) == (height, width):
        code = 444
    elif height % 2 == 0 and width % 2 == 0 and tuple(cbcr.shape[1:3]) == (height // 2, width // 2):
        code = 420
    else:
        raise ValueError(f"{what}: cbcr of shape {tuple(cbcr.shape)} is neither 4:4:4 nor 4:2:0 for y of shape "
                         f"{tuple(y.shape)}")
    return y, cbcr, n, height, width, code, squeeze


# -------------------------------------------------------------------------------------------------------------------
# planes


def unpack_frames_reference(raw, num_frames, width, height, chroma, frame_stride=None, first_offset=0):
    """`unpack_frames` as tensor ops (a gather of the frame bytes, a stack of U and V)."""
    _, h, w, size, stride = _check_raw(raw, num_frames, width, height, chroma, frame_stride, first_offset)
    at = (first_offset + stride * torch.arange(num_frames, device=raw.device))[:, None] + \
        torch.arange(size, device=raw.device)[None, :]
    frames = raw[at]
    ys, cs = width * height, h * w
    y = frames[:, :ys].reshape(num_frames, height, width, 1)
    cbcr = torch.stack([frames[:, ys:ys + cs], frames[:, ys + cs:]], dim=-1).reshape(num_frames, h, w, 2)
    return y.contiguous(), cbcr.contiguous()


def unpack_frames(raw, num_frames, width, height, chroma, frame_stride=None, first_offset=0):
    """raw: flat uint8; frame n's planes Y, U, V lie back to back from byte first_offset + n frame_stride (frame_stride
    defaults to the bytes of a frame) -> (y [N, H, W, 1], cbcr [N, h, w, 2]) uint8, contiguous; h, w = H / 2, W / 2 for
    chroma "420", H, W for "444".  One kernel on a device tensor, bit-exact with `unpack_frames_reference`."""
    if not raw.is_cuda:
        return unpack_frames_reference(raw, num_frames, width, height, chroma, frame_stride, first_offset)
    code, h, w, _, stride = _check_raw(raw, num_frames, width, height, chroma, frame_stride, first_offset)
    y = torch.empty((num_frames, height, width, 1), dtype=torch.uint8, device=raw.device)
    cbcr = torch.empty((num_frames, h, w, 2), dtype=torch.uint8, device=raw.device)
    _lib.check(_lib.lib().tfc_y4m_unpack(raw.data_ptr(), raw.numel(), num_frames, width, height, code, stride,
                                         first_offset, y.data_ptr(), cbcr.data_ptr(), _lib.stream_ptr()))
    return y, cbcr


def _pack_out(y, n, size, stride, first_offset, out):
    need = first_offset + (n - 1) * stride + size if n else 0
    if out is None:
        return torch.zeros(first_offset + n * stride, dtype=torch.uint8, device=y.device)
    if out.dtype != torch.uint8:
        raise TypeError(f"pack_frames: out must be uint8, got {out.dtype}")
    if out.dim() != 1 or not out.is_contiguous() or out.device != y.device:
        raise ValueError("pack_frames: out must be a flat contiguous tensor on the device of y")
    if out.numel() < need:
        raise ValueError(f"pack_frames: out has {out.numel()} bytes, {need} are needed")
    return out


def _pack_args(y, cbcr, out, frame_stride, first_offset):
    y, cbcr, n, height, width, code, _ = check_planes(y, cbcr, "pack_frames")
    size = width * height + 2 * cbcr.shape[1] * cbcr.shape[2]
    stride = size if frame_stride is None else int(frame_stride)
    if stride < size:
        raise ValueError(f"pack_frames: frame_stride {stride} is less than the {size} bytes of a frame")
    if first_offset < 0:
        raise ValueError(f"pack_frames: first_offset must not be negative, got {first_offset}")
    return y, cbcr, n, height, width, code, size, stride, _pack_out(y, n, size, stride, first_offset, out)


def pack_frames_reference(y, cbcr, out=None, frame_stride=None, first_offset=0):
    """`pack_frames` as tensor ops."""
    y, cbcr, n, _, _, _, size, stride, out = _pack_args(y, cbcr, out, frame_stride, first_offset)
    frames = torch.cat([y.reshape(n, -1), cbcr[..., 0].reshape(n, -1), cbcr[..., 1].reshape(n, -1)], dim=1)
    at = (first_offset + stride * torch.arange(n, device=y.device))[:, None] + \
        torch.arange(size, device=y.device)[None, :]
    out[at.reshape(-1)] = frames.reshape(-1)
    return out


def pack_frames(y, cbcr, out=None, frame_stride=None, first_offset=0):
    """The inverse of `unpack_frames`: writes the planes of every frame into `out` (flat uint8; by default a new zeroed
    tensor of first_offset + N frame_stride bytes) and returns it.  Only plane bytes are written."""
    if not y.is_cuda:
        return pack_frames_reference(y, cbcr, out, frame_stride, first_offset)
    y, cbcr, n, height, width, code, _, stride, out = _pack_args(y, cbcr, out, frame_stride, first_offset)
    _lib.check(_lib.lib().tfc_y4m_pack(y.data_ptr(), cbcr.data_ptr(), out.data_ptr(), out.numel(), n, width, height,
                                       code, stride, first_offset, _lib.stream_ptr()))
    return out


# -------------------------------------------------------------------------------------------------------------------
# colour


def _matrix(matrix):
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', got {matrix!r}")
    kr, kb = MATRICES[matrix]
    return kr, 1.0 - kr - kb, kb


def _upsample_bilinear(c):
    """[N, h, w, 2] float -> [N, 2h, 2w, 2]: centre siting, separable, edges clamped."""
    n, h, w, _ = c.shape
    m = torch.arange(h, device=c.device)
    even = 0.75 * c + 0.25 * c[:, (m - 1).clamp(min=0)]
    odd = 0.75 * c + 0.25 * c[:, (m + 1).clamp(max=h - 1)]
    c = torch.stack([even, odd], dim=2).reshape(n, 2 * h, w, 2)
    m = torch.arange(w, device=c.device)
    even = 0.75 * c + 0.25 * c[:, :, (m - 1).clamp(min=0)]
    odd = 0.75 * c + 0.25 * c[:, :, (m + 1).clamp(max=w - 1)]
    return torch.stack([even, odd], dim=3).reshape(n, 2 * h, 2 * w, 2)


def _to_rgb_args(y, cbcr, matrix, upsample, dtype):
    if upsample not in UPSAMPLE_CODE:
        raise ValueError(f"upsample must be 'bilinear' or 'nearest', got {upsample!r}")
    if dtype not in DTYPE_CODE:
        raise TypeError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
    return check_planes(y, cbcr, "ycbcr_to_rgb") + (_matrix(matrix),)


def ycbcr_to_rgb_reference(y, cbcr, matrix="bt601", full_range=True, upsample="bilinear", dtype=torch.uint8,
                           clip=True):
    """`ycbcr_to_rgb` as float32 tensor ops."""
    y, cbcr, _, _, _, code, squeeze, (kr, kg, kb) = _to_rgb_args(y, cbcr, matrix, upsample, dtype)
    yl, c = y.to(torch.float32), cbcr.to(torch.float32)
    if code == 420:
        if upsample == "nearest":
            c = c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        else:
            c = _upsample_bilinear(c)
    if full_range:
        c = c - 128.0
    else:
        yl = (yl - 16.0) * (255.0 / 219.0)
        c = (c - 128.0) * (255.0 / 224.0)
    cb, cr = c[..., 0:1], c[..., 1:2]
    r = yl + (2.0 * (1.0 - kr)) * cr
    g = yl - (2.0 * kr * (1.0 - kr) / kg) * cr - (2.0 * kb * (1.0 - kb) / kg) * cb
    b = yl + (2.0 * (1.0 - kb)) * cb
    rgb = torch.cat([r, g, b], dim=-1)
    if clip or dtype == torch.uint8:
        rgb = rgb.clamp(0.0, 255.0)
    if dtype == torch.uint8:
        rgb = rgb.round()
    rgb = rgb.to(dtype)
    return rgb[0] if squeeze else rgb


def ycbcr_to_rgb(y, cbcr, matrix="bt601", full_range=True, upsample="bilinear", dtype=torch.uint8, clip=True):
    """y [N, H, W, 1], cbcr [N, h, w, 2] uint8 (4:2:0 or 4:4:4 by their shapes; one frame without N is taken too) ->
    [N, H, W, 3] of `dtype` on the 0...255 scale.  uint8 is always clamped and rounds half to even; float32 and bfloat16
    are clamped to [0, 255] with `clip`.  One kernel, no intermediate tensor."""
    if not y.is_cuda:
        return ycbcr_to_rgb_reference(y, cbcr, matrix, full_range, upsample, dtype, clip)
    y, cbcr, n, height, width, code, squeeze, _ = _to_rgb_args(y, cbcr, matrix, upsample, dtype)
    rgb = torch.empty((n, height, width, 3), dtype=dtype, device=y.device)
    _lib.check(_lib.lib().tfc_ycbcr_to_rgb(
        y.data_ptr(), cbcr.data_ptr(), rgb.data_ptr(), n, width, height, code, MATRIX_CODE[matrix],
        int(bool(full_range)), UPSAMPLE_CODE[upsample], DTYPE_CODE[dtype], int(bool(clip)), _lib.stream_ptr()))
    return rgb[0] if squeeze else rgb


def _from_rgb_args(rgb, chroma, matrix):
    if rgb.dtype not in DTYPE_CODE:
        raise TypeError(f"rgb_to_ycbcr supports uint8, float32 and bfloat16, got {rgb.dtype}")
    if not rgb.is_contiguous():
        raise ValueError("rgb_to_ycbcr: rgb must be contiguous")
    squeeze = rgb.dim() == 3
    if squeeze:
        rgb = rgb[None]
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError(f"rgb_to_ycbcr: rgb must be [N, H, W, 3], received shape {tuple(rgb.shape)}")
    code = _chroma_code(chroma)
    n, height, width = rgb.shape[:3]
    h, w = _chroma_shape(width, height, code)
    return rgb, n, height, width, code, h, w, squeeze, _matrix(matrix)


def rgb_to_ycbcr_reference(rgb, chroma="420", matrix="bt601", full_range=True):
    """`rgb_to_ycbcr` as float32 tensor ops."""
    rgb, n, _, _, code, h, w, squeeze, (kr, kg, kb) = _from_rgb_args(rgb, chroma, matrix)
    v = rgb.to(torch.float32)
    r, g, b = v[..., 0:1], v[..., 1:2], v[..., 2:3]
    yl = kr * r + kg * g + kb * b
    c = torch.cat([(b - yl) * (1.0 / (2.0 * (1.0 - kb))), (r - yl) * (1.0 / (2.0 * (1.0 - kr)))], dim=-1)
    if code == 420:
        c = c.reshape(n, h, 2, w, 2, 2).mean(dim=(2, 4))
    if full_range:
        c = c + 128.0
    else:
        yl = yl * (219.0 / 255.0) + 16.0
        c = c * (224.0 / 255.0) + 128.0
    y = yl.clamp(0.0, 255.0).round().to(torch.uint8)
    cbcr = c.clamp(0.0, 255.0).round().to(torch.uint8)
    return (y[0], cbcr[0]) if squeeze else (y, cbcr)


def rgb_to_ycbcr(rgb, chroma="420", matrix="bt601", full_range=True):
    """rgb [N, H, W, 3] uint8, float32 or bfloat16 on the 0...255 scale -> (y [N, H, W, 1], cbcr [N, h, w, 2]) uint8,
    what `pack_frames` and `Y4MWriter` take.  One kernel."""
    if not rgb.is_cuda:
        return rgb_to_ycbcr_reference(rgb, chroma, matrix, full_range)
    rgb, n, height, width, code, h, w, squeeze, _ = _from_rgb_args(rgb, chroma, matrix)
    y = torch.empty((n, height, width, 1), dtype=torch.uint8, device=rgb.device)
    cbcr = torch.empty((n, h, w, 2), dtype=torch.uint8, device=rgb.device)
    _lib.check(_lib.lib().tfc_rgb_to_ycbcr(
        rgb.data_ptr(), DTYPE_CODE[rgb.dtype], y.data_ptr(), cbcr.data_ptr(), n, width, height, code,
        MATRIX_CODE[matrix], int(bool(full_range)), _lib.stream_ptr()))
    return (y[0], cbcr[0]) if squeeze else (y, cbcr)
