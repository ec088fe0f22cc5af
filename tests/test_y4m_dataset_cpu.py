"""CPU tier: Y4MDataset / Y4MWriter against the reference's test (python/datasets/y4m_dataset_test.py:30-61) and the
semantics of its op (cc/kernels/y4m_dataset_kernels.cc:125-406), and the tensor-op twins of ops/video_ops.py against the
float64 definition of tests/y4m_ref.py."""
import itertools
import os

import numpy as np
import pytest
import torch

import y4m_ref
from compression_amd.datasets import Y4MDataset, Y4MWriter
from compression_amd.ops import video_ops

FILE_1 = b"YUV4MPEG2 W4 H2 F30:1 Ip A0:0 C420jpeg\nFRAME\nABCDEFGHIJKL"
FILE_2 = b"YUV4MPEG2 C444 W1 H1\nFRAME\nabcFRAME\ndef"


def _write(tmp_path, name, content):
    path = os.path.join(str(tmp_path), name)
    with open(path, "wb") as f:
        f.write(content)
    return path


def _u8(string, shape):
    return torch.tensor(list(string), dtype=torch.uint8).reshape(shape)


@pytest.fixture
def two_files(tmp_path):
    return [_write(tmp_path, "one.y4m", FILE_1), _write(tmp_path, "two.y4m", FILE_2)]


def _all_frames(ds_or_it):
    return [(y.clone(), c.clone()) for y, c in ds_or_it]


def _same(a, b):
    assert len(a) == len(b)
    for (y0, c0), (y1, c1) in zip(a, b):
        assert y0.shape == y1.shape and c0.shape == c1.shape
        assert torch.equal(y0, y1) and torch.equal(c0, c1)


def test_dataset_yields_the_sequence_of_the_reference_test(two_files):
    ds = Y4MDataset(two_files)
    it = iter(ds)
    y, cbcr = next(it)
    assert y.dtype == torch.uint8 and cbcr.dtype == torch.uint8
    assert torch.equal(y, _u8(b"ABCDEFGH", (2, 4, 1)))
    assert torch.equal(cbcr[..., 0], _u8(b"IJ", (1, 2))) and torch.equal(cbcr[..., 1], _u8(b"KL", (1, 2)))
    y, cbcr = next(it)
    assert y.dtype == torch.uint8 and cbcr.dtype == torch.uint8
    assert torch.equal(y, _u8(b"a", (1, 1, 1))) and torch.equal(cbcr, _u8(b"bc", (1, 1, 2)))
    y, cbcr = next(it)
    assert torch.equal(y, _u8(b"d", (1, 1, 1))) and torch.equal(cbcr, _u8(b"ef", (1, 1, 2)))
    with pytest.raises(StopIteration):
        next(it)
    # every iter() restarts from the first file; a single path is a dataset of one file
    assert len(_all_frames(ds)) == 3 and len(_all_frames(ds)) == 3
    assert len(_all_frames(Y4MDataset(two_files[1]))) == 2
    for fpr in (1, 2, 3):
        _same(_all_frames(Y4MDataset(two_files, frames_per_read=fpr)), _all_frames(ds))


def test_flat_namespace_exports_the_dataset():
    import compression_amd as tfc
    assert tfc.Y4MDataset is Y4MDataset and tfc.Y4MWriter is Y4MWriter
    assert tfc.datasets.__all__ == ["Y4MDataset", "Y4MWriter"]
    for name in ("unpack_frames", "pack_frames", "ycbcr_to_rgb", "rgb_to_ycbcr"):
        assert getattr(tfc, name) is getattr(video_ops, name)
        assert getattr(tfc, name + "_reference") is getattr(video_ops, name + "_reference")


def test_filenames_must_be_a_scalar_or_a_vector(two_files):
    for nested in ([two_files], [[two_files[0]], [two_files[1]]], np.array([two_files]), [3]):
        with pytest.raises(ValueError, match="`filenames` must be a scalar or a vector"):
            Y4MDataset(nested)
    assert list(Y4MDataset([])) == []
    assert list(Y4MDataset([]).batches(2)) == []
    assert len(_all_frames(Y4MDataset(tuple(two_files)))) == 3
    assert len(_all_frames(Y4MDataset(np.array(two_files)))) == 3


ERRORS = [
    ("C420mpeg2", b"YUV4MPEG2 W4 H2 C420mpeg2\nFRAME\nABCDEFGHIJKL", "has an invalid Y4M header. Remaining header: 'mpeg2'."),
    ("C422", b"YUV4MPEG2 W4 H2 C422 Ip\nFRAME\nABCDEFGHIJKLMNOP", "has an unsupported chroma format '422'."),
    ("Ii", b"YUV4MPEG2 W4 H2 Ii C420jpeg\nFRAME\nABCDEFGHIJKL", "is not in progressive format."),
    ("W0", b"YUV4MPEG2 W0 H2 C420jpeg\n", "has an invalid width specifier '0'."),
    ("W_no_digits", b"YUV4MPEG2 W H2 C420jpeg\n", "has an invalid width specifier ''."),
    ("H0", b"YUV4MPEG2 W4 H0 C420jpeg\n", "has an invalid height specifier '0'."),
    ("H_no_digits", b"YUV4MPEG2 W4 Hx C420jpeg\n", "has an invalid height specifier ''."),
    ("no_C", b"YUV4MPEG2 W4 H2 Ip\nFRAME\nABCDEFGHIJKL", "has no chroma format specifier."),
    ("no_W", b"YUV4MPEG2 H2 C444\n", "has no width specifier."),
    ("no_H", b"YUV4MPEG2 W2 C444\n", "has no height specifier."),
    ("odd_420", b"YUV4MPEG2 W3 H2 C420jpeg\n", "has 4:2:0 chroma format, but odd width or height."),
    ("odd_420_h", b"YUV4MPEG2 W4 H3 C420\n", "has 4:2:0 chroma format, but odd width or height."),
    ("no_marker", b"YUV4MPEG W4 H2 C444\n", "does not have a YUV4MPEG2 marker."),
    ("no_newline", b"YUV4MPEG2 W4 H2 C444", "does not contain a complete Y4M header."),
    ("empty", b"", "does not contain a complete Y4M header."),
    ("no_newline_long", b"YUV4MPEG2 W4 H2 C444 X" + b"x" * 600, "does not contain a complete Y4M header."),
    ("trailing_space", b"YUV4MPEG2 W4 H2 C444 \n", "has an invalid Y4M header. Remaining header: ' '."),
]


@pytest.mark.parametrize("device_free_fpr", [1, 8])
@pytest.mark.parametrize("case", ERRORS, ids=[e[0] for e in ERRORS])
def test_header_errors_carry_the_reference_wording(tmp_path, case, device_free_fpr):
    name, content, wording = case
    path = _write(tmp_path, name + ".y4m", content)
    with pytest.raises(ValueError) as err:
        list(Y4MDataset(path, frames_per_read=device_free_fpr))
    assert wording in str(err.value) and f"Input file '{path}'" in str(err.value)


@pytest.mark.parametrize("fpr", [1, 2, 8])
def test_frame_errors_carry_the_reference_wording(tmp_path, fpr):
    header = b"YUV4MPEG2 W1 H1 C444\n"
    # a frame with parameters: the frame in front of it is still delivered
    path = _write(tmp_path, "params.y4m", header + b"FRAME\nabcFRAME Ip\ndef")
    it = iter(Y4MDataset(path, frames_per_read=fpr))
    y, cbcr = next(it)
    assert torch.equal(y, _u8(b"a", (1, 1, 1))) and torch.equal(cbcr, _u8(b"bc", (1, 1, 2)))
    with pytest.raises(ValueError) as err:
        next(it)
    at = len(header) + 9
    assert f"Input file '{path}' has a FRAME marker at byte {at} which is either invalid or has unsupported frame " \
           "parameters." in str(err.value)
    path = _write(tmp_path, "params_first.y4m", header + b"FRAME Ip\nabc")
    with pytest.raises(ValueError, match=f"has a FRAME marker at byte {len(header)} which is either invalid"):
        list(Y4MDataset(path, frames_per_read=fpr))
    # a truncated last frame: both byte counts
    path = _write(tmp_path, "short.y4m", header + b"FRAME\nabcFRAME\nde")
    it = iter(Y4MDataset(path, frames_per_read=fpr))
    next(it)
    with pytest.raises(ValueError) as err:
        next(it)
    assert f"Input file '{path}' has an incomplete or unsupported frame at byte {at}. Expected to read 9 bytes, only 8 " \
           "were available." in str(err.value)
    path = _write(tmp_path, "short420.y4m", FILE_1[:-5])
    with pytest.raises(ValueError, match="Expected to read 18 bytes, only 13 were available."):
        list(Y4MDataset(path, frames_per_read=fpr))


def test_a_missing_file_is_an_oserror(tmp_path, two_files):
    it = iter(Y4MDataset([two_files[0], os.path.join(str(tmp_path), "absent.y4m")]))
    next(it)
    with pytest.raises(OSError):
        next(it)


def test_long_headers_and_any_parameter_order(tmp_path):
    long_header = b"YUV4MPEG2 W4 H2 X" + b"c" * 270 + b" C420jpeg Ip\n"
    assert len(long_header) >= 300
    path = _write(tmp_path, "long.y4m", long_header + b"FRAME\nABCDEFGHIJKL")
    (y, cbcr), = _all_frames(Y4MDataset(path))
    assert torch.equal(y, _u8(b"ABCDEFGH", (2, 4, 1))) and torch.equal(cbcr[..., 1], _u8(b"KL", (1, 2)))
    # exactly 256 and 257 bytes: the newline is the last byte of a chunk, or the first of the next
    for size in (256, 257, 512):
        pad = size - len(b"YUV4MPEG2 W1 H1 C444 X\n")
        header = b"YUV4MPEG2 W1 H1 C444 X" + b"p" * pad + b"\n"
        assert len(header) == size
        path = _write(tmp_path, f"h{size}.y4m", header + b"FRAME\nabc")
        (y, cbcr), = _all_frames(Y4MDataset(path))
        assert torch.equal(y, _u8(b"a", (1, 1, 1))) and torch.equal(cbcr, _u8(b"bc", (1, 1, 2)))
    for params in itertools.permutations([b"W4", b"H2", b"C420", b"Ip", b"F25:1", b"XYSCSS=420JPEG"]):
        path = _write(tmp_path, "order.y4m", b"YUV4MPEG2 " + b" ".join(params) + b"\nFRAME\nABCDEFGHIJKL")
        (y, cbcr), = _all_frames(Y4MDataset(path))
        assert torch.equal(y, _u8(b"ABCDEFGH", (2, 4, 1))) and torch.equal(cbcr[..., 0], _u8(b"IJ", (1, 2)))


def test_a_header_only_file_yields_nothing_and_the_next_file_follows(tmp_path, two_files):
    empty = _write(tmp_path, "header_only.y4m", b"YUV4MPEG2 W640 H480 C420jpeg\n")
    assert list(Y4MDataset(empty)) == []
    frames = _all_frames(Y4MDataset([empty, two_files[0], empty, two_files[1], empty]))
    _same(frames, _all_frames(Y4MDataset(two_files)))


@pytest.mark.parametrize("fpr", [1, 2, 8])
def test_state_resumes_at_each_of_the_five_positions(two_files, fpr):
    ds = Y4MDataset(two_files, frames_per_read=fpr)
    frames = _all_frames(ds)
    it = iter(ds)
    header_1, header_2 = FILE_1.index(b"\n") + 1, FILE_2.index(b"\n") + 1
    want_states = [{"file_index": 0, "file_pos": -1}, {"file_index": 0, "file_pos": len(FILE_1)},
                   {"file_index": 1, "file_pos": header_2 + 9}, {"file_index": 1, "file_pos": len(FILE_2)},
                   {"file_index": 2, "file_pos": -1}]
    assert header_1 + 18 == len(FILE_1)
    for taken in range(5):
        state = it.state_dict()
        assert state == want_states[taken], (taken, state)
        resumed = ds.iterator(dict(state))
        _same(_all_frames(resumed), frames[taken:])
        assert resumed.state_dict() == want_states[4]
        if taken < 3:
            next(it)
        elif taken == 3:
            with pytest.raises(StopIteration):
                next(it)
    with pytest.raises(StopIteration):
        next(it)


def test_batches_never_mix_files(tmp_path, two_files):
    ds = Y4MDataset(two_files)
    got = [(y.clone(), c.clone()) for y, c in ds.batches(2)]
    assert [tuple(y.shape) for y, _ in got] == [(1, 2, 4, 1), (2, 1, 1, 1)]
    assert [tuple(c.shape) for _, c in got] == [(1, 1, 2, 2), (2, 1, 1, 2)]
    assert torch.equal(got[1][0].reshape(-1), _u8(b"ad", (2,))) and torch.equal(got[1][1].reshape(-1), _u8(b"bcef", (4,)))
    assert [tuple(y.shape) for y, _ in ds.batches(2, drop_remainder=True)] == [(2, 1, 1, 1)]
    assert [y.shape[0] for y, _ in ds.batches(1)] == [1, 1, 1]
    five = _write(tmp_path, "five.y4m", b"YUV4MPEG2 W1 H1 C444\n" + b"".join(b"FRAME\n" + bytes([k, k + 1, k + 2])
                                                                            for k in range(0, 15, 3)))
    assert [y.shape[0] for y, _ in Y4MDataset([five, two_files[1]]).batches(2)] == [2, 2, 1, 2]
    assert [y.shape[0] for y, _ in Y4MDataset([five, two_files[1]]).batches(2, drop_remainder=True)] == [2, 2, 2]
    ys = torch.cat([y for y, _ in Y4MDataset(five).batches(3)]).reshape(-1)
    assert ys.tolist() == [0, 3, 6, 9, 12]


@pytest.mark.parametrize("chroma,width,height", [("420jpeg", 6, 2), ("420jpeg", 34, 66), ("444", 1, 1), ("444", 17, 3)])
def test_writer_round_trip(tmp_path, chroma, width, height):
    gen = torch.Generator().manual_seed(5)
    h, w = y4m_ref.chroma_shape(width, height, chroma[:3])
    y = torch.randint(0, 256, (3, height, width, 1), dtype=torch.uint8, generator=gen)
    cbcr = torch.randint(0, 256, (3, h, w, 2), dtype=torch.uint8, generator=gen)
    path = os.path.join(str(tmp_path), "out.y4m")
    with Y4MWriter(path, width, height, chroma=chroma, frame_rate=(25, 1)) as writer:
        writer.write(y[0], cbcr[0])             # one frame
        writer.write(y[1:], cbcr[1:])           # a batch
    with open(path, "rb") as f:
        content = f.read()
    header = f"YUV4MPEG2 W{width} H{height} F25:1 Ip C{chroma}\n".encode()
    size = y4m_ref.frame_bytes(width, height, chroma[:3])
    assert content.startswith(header) and len(content) == len(header) + 3 * (6 + size)
    assert content[len(header):len(header) + 6] == b"FRAME\n"
    frames = _all_frames(Y4MDataset(path))
    _same(frames, [(y[k], cbcr[k]) for k in range(3)])
    with pytest.raises(ValueError):
        Y4MWriter(os.path.join(str(tmp_path), "bad.y4m"), 3, 2, chroma="420jpeg")
    with Y4MWriter(os.path.join(str(tmp_path), "other.y4m"), width + 2, height, chroma=chroma) as writer:
        with pytest.raises(ValueError):
            writer.write(y, cbcr)
    with pytest.raises(ValueError):
        writer.write(y, cbcr)                   # closed


# ---------------------------------------------------------------------------------------------------------------
# the tensor-op twins against the float64 definition

SIZES_420 = [(2, 2), (6, 2), (34, 66)]
SIZES_444 = SIZES_420 + [(17, 3), (1, 1)]


def _planes(width, height, chroma, n=2, seed=0):
    rng = np.random.default_rng(seed)
    h, w = y4m_ref.chroma_shape(width, height, chroma)
    return (rng.integers(0, 256, (n, height, width, 1), dtype=np.uint8),
            rng.integers(0, 256, (n, h, w, 2), dtype=np.uint8))


@pytest.mark.parametrize("first,gap", [(0, 0), (6, 6), (1, 7)])
@pytest.mark.parametrize("chroma,width,height", [("444", 1, 1), ("444", 3, 5), ("420", 6, 2), ("420", 34, 66)])
def test_plane_twins_match_the_definition(chroma, width, height, first, gap):
    size = y4m_ref.frame_bytes(width, height, chroma)
    stride = size + gap
    raw = np.random.default_rng(1).integers(0, 256, first + 3 * stride, dtype=np.uint8)
    want_y, want_c = y4m_ref.unpack(raw, 3, width, height, chroma, stride, first)
    y, cbcr = video_ops.unpack_frames(torch.from_numpy(raw), 3, width, height, chroma, stride, first)
    assert y.is_contiguous() and cbcr.is_contiguous()
    assert np.array_equal(y.numpy(), want_y) and np.array_equal(cbcr.numpy(), want_c)
    out = torch.full((first + 3 * stride,), 0xA5, dtype=torch.uint8)
    assert video_ops.pack_frames(y, cbcr, out=out, frame_stride=stride, first_offset=first) is out
    want = y4m_ref.pack(want_y, want_c, np.full(first + 3 * stride, 0xA5, np.uint8), stride, first)
    assert np.array_equal(out.numpy(), want)
    fresh = video_ops.pack_frames(y, cbcr, frame_stride=stride, first_offset=first)
    again = video_ops.unpack_frames(fresh, 3, width, height, chroma, stride, first)
    assert torch.equal(again[0], y) and torch.equal(again[1], cbcr)


@pytest.mark.parametrize("full_range", [True, False])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_colour_twins_match_the_definition(matrix, full_range):
    for chroma, sizes, how in (("420", SIZES_420, "bilinear"), ("420", SIZES_420, "nearest"),
                               ("444", SIZES_444, "bilinear")):
        count = y4m_ref.TieCount()
        for width, height in sizes:
            y, cbcr = _planes(width, height, chroma)
            ty, tc = torch.from_numpy(y), torch.from_numpy(cbcr)
            what = f"{chroma} {width}x{height} {how}"
            want = y4m_ref.ycbcr_to_rgb(y, cbcr, matrix, full_range, how, clip=False)
            got = video_ops.ycbcr_to_rgb(ty, tc, matrix, full_range, how, dtype=torch.float32, clip=False)
            assert got.shape == want.shape and got.dtype == torch.float32
            assert np.abs(got.numpy() - want).max() <= y4m_ref.FLOAT_BOUND, what
            want = y4m_ref.ycbcr_to_rgb(y, cbcr, matrix, full_range, how, clip=True)
            got = video_ops.ycbcr_to_rgb(ty, tc, matrix, full_range, how, dtype=torch.bfloat16)
            err = np.abs(got.to(torch.float32).numpy() - want)
            assert (err <= 2.0 ** -8 * np.abs(want) + y4m_ref.FLOAT_BOUND).all(), what
            got = video_ops.ycbcr_to_rgb(ty, tc, matrix, full_range, how)
            assert got.dtype == torch.uint8
            y4m_ref.check_uint8(got.numpy(), want, count, what)
        count.check_share(f"to rgb {chroma} {how}")
    for chroma, sizes in (("420", SIZES_420), ("444", SIZES_444)):
        count = y4m_ref.TieCount()
        for width, height in sizes:
            rgb = np.random.default_rng(2).uniform(0.0, 255.0, (2, height, width, 3)).astype(np.float32)
            for values in (rgb, np.rint(rgb).astype(np.uint8),
                           torch.from_numpy(rgb).to(torch.bfloat16)):
                t = values if isinstance(values, torch.Tensor) else torch.from_numpy(values)
                want_y, want_c = y4m_ref.rgb_to_ycbcr(t.to(torch.float32).numpy(), chroma, matrix, full_range)
                got_y, got_c = video_ops.rgb_to_ycbcr(t, chroma, matrix, full_range)
                assert got_y.dtype == torch.uint8 and got_c.dtype == torch.uint8
                assert got_y.shape == want_y.shape and got_c.shape == want_c.shape
                both = np.concatenate([want_y.reshape(-1), want_c.reshape(-1)])
                got = np.concatenate([got_y.numpy().reshape(-1), got_c.numpy().reshape(-1)])
                y4m_ref.check_uint8(got, both, count, f"from rgb {chroma} {width}x{height} {t.dtype}")
        count.check_share(f"from rgb {chroma}")


def test_single_frames_and_argument_checks():
    y, cbcr = (torch.from_numpy(a) for a in _planes(6, 2, "420"))
    one = video_ops.ycbcr_to_rgb(y[0], cbcr[0])
    assert one.shape == (2, 6, 3) and torch.equal(one, video_ops.ycbcr_to_rgb(y, cbcr)[0])
    y1, c1 = video_ops.rgb_to_ycbcr(one)
    assert y1.shape == (2, 6, 1) and c1.shape == (1, 3, 2)
    with pytest.raises(TypeError):
        video_ops.ycbcr_to_rgb(y.to(torch.float32), cbcr)
    with pytest.raises(TypeError):
        video_ops.ycbcr_to_rgb(y, cbcr, dtype=torch.float16)
    with pytest.raises(TypeError):
        video_ops.rgb_to_ycbcr(torch.zeros(1, 2, 2, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        video_ops.ycbcr_to_rgb(y.transpose(1, 2), cbcr)
    with pytest.raises(ValueError):
        video_ops.ycbcr_to_rgb(y, cbcr[:, :, :2])
    with pytest.raises(ValueError):
        video_ops.ycbcr_to_rgb(y, cbcr, matrix="bt2020")
    with pytest.raises(ValueError):
        video_ops.ycbcr_to_rgb(y, cbcr, upsample="bicubic")
    with pytest.raises(ValueError):
        video_ops.rgb_to_ycbcr(torch.zeros(1, 3, 2, 3), chroma="420")
    with pytest.raises(ValueError):
        video_ops.rgb_to_ycbcr(torch.zeros(1, 2, 2, 3), chroma="422")
    with pytest.raises(ValueError):
        video_ops.unpack_frames(torch.zeros(11, dtype=torch.uint8), 1, 4, 2, "420")
    with pytest.raises(ValueError):
        video_ops.unpack_frames(torch.zeros(64, dtype=torch.uint8), 2, 4, 2, "420", frame_stride=11)
    with pytest.raises(TypeError):
        video_ops.unpack_frames(torch.zeros(12, dtype=torch.int8), 1, 4, 2, "420")


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null tensors, no device needed: the checks run on the host and the errors are textual."""
    from compression_amd import _lib
    lib = _lib.lib()

    def rejected(rc, text):
        assert rc != 0 and text in _lib.last_error(), _lib.last_error()

    rejected(lib.tfc_y4m_unpack(None, 0, 1, 0, 2, 420, 12, 0, None, None, None), "width and height")
    rejected(lib.tfc_y4m_unpack(None, 0, -1, 4, 2, 420, 12, 0, None, None, None), "num_frames")
    rejected(lib.tfc_y4m_unpack(None, 0, 1, 3, 2, 420, 12, 0, None, None, None), "odd width or height")
    rejected(lib.tfc_y4m_pack(None, None, None, 0, 1, 4, 3, 420, 12, 0, None), "odd width or height")
    rejected(lib.tfc_y4m_unpack(None, 100, 1, 4, 2, 420, 11, 0, None, None, None), "frame_stride")
    rejected(lib.tfc_y4m_pack(None, None, None, 100, 1, 4, 2, 444, 23, 0, None), "frame_stride")
    rejected(lib.tfc_y4m_unpack(None, 100, 1, 4, 2, 422, 16, 0, None, None, None), "chroma")
    rejected(lib.tfc_y4m_unpack(None, 17, 1, 4, 2, 420, 12, 6, None, None, None), "the buffer has 17")
    rejected(lib.tfc_y4m_unpack(None, 18, 1, 4, 2, 420, 12, 6, None, None, None), "must not be null")
    rejected(lib.tfc_ycbcr_to_rgb(None, None, None, 1, 4, 2, 420, 2, 1, 1, 0, 1, None), "matrix")
    rejected(lib.tfc_ycbcr_to_rgb(None, None, None, 1, 4, 2, 420, 0, 1, 2, 0, 1, None), "upsample")
    rejected(lib.tfc_ycbcr_to_rgb(None, None, None, 1, 4, 2, 420, 0, 1, 1, 3, 1, None), "dtype")
    rejected(lib.tfc_ycbcr_to_rgb(None, None, None, 1, 5, 2, 420, 0, 1, 1, 0, 1, None), "odd width or height")
    rejected(lib.tfc_ycbcr_to_rgb(None, None, None, 1, 4, -2, 444, 0, 1, 1, 0, 1, None), "width and height")
    rejected(lib.tfc_rgb_to_ycbcr(None, 5, None, None, 1, 4, 2, 420, 0, 1, None), "dtype")
    rejected(lib.tfc_rgb_to_ycbcr(None, 0, None, None, 1, 4, 2, 420, 7, 1, None), "matrix")
    rejected(lib.tfc_rgb_to_ycbcr(None, 0, None, None, 1, 4, 2, 420, 0, 1, None), "must not be null")
    assert lib.tfc_rgb_to_ycbcr(None, 0, None, None, 0, 4, 2, 420, 0, 1, None) == 0      # no frames: nothing to do
    assert lib.tfc_y4m_unpack(None, 0, 0, 4, 2, 420, 12, 0, None, None, None) == 0
