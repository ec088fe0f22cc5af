"""The float64 definition of the Y4M ops (numpy): what `ops.video_ops` and csrc/y4m.hip are held to.

Planes: frame n's Y, U, V lie back to back from byte first_offset + n frame_stride; cbcr[..., 0] = U, cbcr[..., 1] = V.
Colour: (Kr, Kb) = (0.299, 0.114) for bt601, (0.2126, 0.0722) for bt709, Kg = 1 - Kr - Kb;
  full range Y' = y, C' = c - 128; limited range Y' = (y - 16) 255 / 219, C' = (c - 128) 255 / 224;
  R = Y' + 2(1-Kr) Cr',  B = Y' + 2(1-Kb) Cb',  G = Y' - (2Kr(1-Kr)/Kg) Cr' - (2Kb(1-Kb)/Kg) Cb';
  Y' = Kr R + Kg G + Kb B,  Cb' = (B - Y') / (2(1-Kb)),  Cr' = (R - Y') / (2(1-Kr)).
4:2:0 chroma is upsampled "nearest" (c[i // 2, j // 2]) or "bilinear" with centre siting (separable; row 2m takes
0.75 c[m] + 0.25 c[max(m-1, 0)], row 2m+1 takes 0.75 c[m] + 0.25 c[min(m+1, h-1)]), and subsampled as the mean of each
2 x 2 block.  The functions return the unrounded float64 values; `to_uint8` is the clamp and the half-to-even rounding."""
import numpy as np

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
TIE_WINDOW = 5e-4                   # a value this close to k + 0.5 may round either way in float32
FLOAT_BOUND = 16 * 2.0 ** -15       # at most 16 roundings of float32 intermediates below 1024 (ulp 2^-14, half of it each)


def chroma_shape(width, height, chroma):
    return (height // 2, width // 2) if chroma == "420" else (height, width)


def frame_bytes(width, height, chroma):
    h, w = chroma_shape(width, height, chroma)
    return width * height + 2 * h * w


def unpack(raw, num_frames, width, height, chroma, frame_stride=None, first_offset=0):
    h, w = chroma_shape(width, height, chroma)
    ys, cs = width * height, h * w
    stride = ys + 2 * cs if frame_stride is None else frame_stride
    y = np.empty((num_frames, height, width, 1), np.uint8)
    cbcr = np.empty((num_frames, h, w, 2), np.uint8)
    for n in range(num_frames):
        at = first_offset + n * stride
        y[n, ..., 0] = raw[at:at + ys].reshape(height, width)
        cbcr[n, ..., 0] = raw[at + ys:at + ys + cs].reshape(h, w)
        cbcr[n, ..., 1] = raw[at + ys + cs:at + ys + 2 * cs].reshape(h, w)
    return y, cbcr


def pack(y, cbcr, out, frame_stride=None, first_offset=0):
    n = y.shape[0]
    ys, cs = y[0].size, cbcr[0, ..., 0].size
    stride = ys + 2 * cs if frame_stride is None else frame_stride
    for k in range(n):
        at = first_offset + k * stride
        out[at:at + ys] = y[k].reshape(-1)
        out[at + ys:at + ys + cs] = cbcr[k, ..., 0].reshape(-1)
        out[at + ys + cs:at + ys + 2 * cs] = cbcr[k, ..., 1].reshape(-1)
    return out


def upsample(c, how):
    """[N, h, w, 2] -> [N, 2h, 2w, 2] float64."""
    c = c.astype(np.float64)
    n, h, w, _ = c.shape
    if how == "nearest":
        return c.repeat(2, axis=1).repeat(2, axis=2)
    m = np.arange(h)
    rows = np.empty((n, 2 * h, w, 2))
    rows[:, 0::2] = 0.75 * c + 0.25 * c[:, np.maximum(m - 1, 0)]
    rows[:, 1::2] = 0.75 * c + 0.25 * c[:, np.minimum(m + 1, h - 1)]
    m = np.arange(w)
    out = np.empty((n, 2 * h, 2 * w, 2))
    out[:, :, 0::2] = 0.75 * rows + 0.25 * rows[:, :, np.maximum(m - 1, 0)]
    out[:, :, 1::2] = 0.75 * rows + 0.25 * rows[:, :, np.minimum(m + 1, w - 1)]
    return out


def ycbcr_to_rgb(y, cbcr, matrix="bt601", full_range=True, how="bilinear", clip=True):
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    yl = y.astype(np.float64)
    c = upsample(cbcr, how) if cbcr.shape[1:3] != y.shape[1:3] else cbcr.astype(np.float64)
    if full_range:
        c = c - 128.0
    else:
        yl = (yl - 16.0) * 255.0 / 219.0
        c = (c - 128.0) * 255.0 / 224.0
    cb, cr = c[..., 0:1], c[..., 1:2]
    r = yl + 2.0 * (1.0 - kr) * cr
    b = yl + 2.0 * (1.0 - kb) * cb
    g = yl - (2.0 * kr * (1.0 - kr) / kg) * cr - (2.0 * kb * (1.0 - kb) / kg) * cb
    rgb = np.concatenate([r, g, b], axis=-1)
    return np.clip(rgb, 0.0, 255.0) if clip else rgb


def rgb_to_ycbcr(rgb, chroma="420", matrix="bt601", full_range=True):
    """-> (y, cbcr) float64, range scaling undone, neither clamped nor rounded."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    v = rgb.astype(np.float64)
    r, g, b = v[..., 0:1], v[..., 1:2], v[..., 2:3]
    yl = kr * r + kg * g + kb * b
    c = np.concatenate([(b - yl) / (2.0 * (1.0 - kb)), (r - yl) / (2.0 * (1.0 - kr))], axis=-1)
    if chroma == "420":
        n, height, width, _ = c.shape
        c = c.reshape(n, height // 2, 2, width // 2, 2, 2).mean(axis=(2, 4))
    if full_range:
        return yl, c + 128.0
    return yl * 219.0 / 255.0 + 16.0, c * 224.0 / 255.0 + 128.0


def to_uint8(v):
    return np.rint(np.clip(v, 0.0, 255.0)).astype(np.uint8)      # np.rint rounds half to even


def near_tie(v):
    """Where the clamped value lies within TIE_WINDOW of a half-integer."""
    v = np.clip(v, 0.0, 255.0)
    return np.abs(v - np.floor(v) - 0.5) <= TIE_WINDOW


class TieCount:
    """Near-tie samples over the sizes of one case of the grid.  The 1 % cap is a statement about a case's inputs, so
    it is taken over all of the case's outputs: at 2 x 2 a single tie among 24 outputs is already 4 %."""

    def __init__(self):
        self.ties = self.total = 0

    def check_share(self, what=""):
        print(f"{what}: near-tie share {self.ties / max(self.total, 1):.5f} of {self.total}")
        assert self.ties <= 0.01 * self.total, (what, self.ties, self.total)


def check_uint8(got, want64, count, what=""):
    """`got` (uint8) equals the rounded definition away from near-ties and is within 1 at them; the near-ties are
    added to `count` (a TieCount), whose share the caller asserts."""
    got = np.asarray(got).astype(np.int64)
    want = to_uint8(want64).astype(np.int64)
    tie = near_tie(want64)
    diff = np.abs(got - want)
    print(f"{what}: near-ties {int(tie.sum())} of {tie.size}, mismatches {int((diff != 0).sum())}, worst {int(diff.max())}")
    count.ties += int(tie.sum())
    count.total += tie.size
    assert (diff[~tie] == 0).all(), (what, int((diff[~tie] != 0).sum()), int(diff.max()))
    assert (diff[tie] <= 1).all(), (what, int(diff.max()))
