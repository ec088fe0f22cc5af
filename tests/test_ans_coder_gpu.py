"""GPU tier of csrc/ans_coder.hip: `ans_encode`'s strings against the definition (`ans_encode_reference`) byte for byte,
`ans_decode` on them, on damaged strings and on random bytes (against `ans_decode_reference`: the kernel follows the
definition on any bytes), at the sizes where the kernel can go wrong.

The decoder keeps a window of four blocks of 64 words (kWindowBlocks in ans_coder.hip) and moves it on by a block when
its read position enters the next one: the 4097-element cases (about 900 words a stream) and the all-escape rounds (up
to 64 words in one sub-step, 256 in a round) move it many times; the 63 ... 129-element cases stay inside the first
window.
The op takes streams of one length per call, so unequal lengths are separate calls here; empty streams are elems = 0."""
import numpy as np
import pytest
import torch

import ans_cases
from compression_amd import _lib
from compression_amd.ops import ans_ops, gen_ops

pytestmark = pytest.mark.gpu


def big_rows():
    """A table set too large for LDS (more than 144 KiB of raw tables): the decoder reads its rows through L2."""
    rows = ans_cases.mixed_rows() + [ans_cases.gaussian_row(16, 2000, True, sigma=40.0 + 9 * j) for j in range(19)]
    assert 4 * sum(len(r) for r in rows) > 144 * 1024
    return rows


TABLES = {"mixed": ans_cases.mixed_rows, "big": big_rows}

# (streams, elems, lanes, index mode, tables)
CASES = [
    (1, 0, 64, True, "mixed"), (3, 0, 1, False, "mixed"),
    (3, 1, 64, True, "mixed"), (1500, 1, 1, False, "mixed"),
    (1, 63, 64, False, "mixed"), (3, 64, 32, True, "mixed"), (1, 65, 1, True, "mixed"), (3, 65, 64, True, "mixed"),
    (3, 129, 64, False, "mixed"), (1, 129, 32, True, "mixed"),
    (1, 4097, 64, True, "mixed"), (3, 4097, 32, False, "mixed"), (1, 4097, 1, True, "mixed"),
    (1500, 65, 64, True, "mixed"),
    (3, 129, 64, True, "big"), (1, 4097, 32, False, "big"), (1, 4097, 64, True, "big"),
]


def draw_streams(rows, streams, elems, indexed, seed):
    index = np.zeros((streams, elems), np.int32)
    value = np.zeros((streams, elems), np.int32)
    for s in range(streams):
        given = None if indexed else np.arange(elems) % len(rows)
        index[s], value[s] = ans_cases.draw(rows, elems, seed + s, index=given)
    return index, value


def round_trip(lookup, value, index, lanes):
    """Encodes and decodes on the device and holds both to the definition -> the strings."""
    streams, elems = value.shape
    want = ans_ops.ans_encode_reference(lookup, value, index, lanes)
    table = torch.from_numpy(lookup)
    encoded = ans_ops.ans_encode(table, torch.from_numpy(value), None if index is None else torch.from_numpy(index), lanes)
    got = ans_ops.strings_from_blob(encoded)
    assert int(encoded.status.abs().sum()) == 0
    assert len(got) == streams
    for s in range(streams):
        assert got[s] == want[s], f"stream {s}: {len(got[s])} bytes, the definition has {len(want[s])}"
    for strings in (got, encoded):                          # host strings, and the device blob as it is
        symbols, ok = ans_ops.ans_decode(strings, table, (streams, elems),
                                         None if index is None else torch.from_numpy(index), lanes)
        assert bool(ok.all()) and ok.numel() == streams
        assert np.array_equal(symbols.cpu().numpy(), value)
    return got


# the cases in three tests (the suite's test count stays small); a failure names its case
GROUPS = {"short": [c for c in CASES if c[4] == "mixed" and c[1] < 4097],
          "long": [c for c in CASES if c[4] == "mixed" and c[1] == 4097],
          "global": [c for c in CASES if c[4] == "big"]}
assert sum(len(g) for g in GROUPS.values()) == len(CASES)


@pytest.mark.parametrize("group", list(GROUPS))
def test_strings_are_the_definitions_and_decode(group):
    for case in GROUPS[group]:
        try:
            strings_are_the_definitions_and_decode(*case)
        except AssertionError as e:
            raise AssertionError(f"case {case}: {e}") from e


def strings_are_the_definitions_and_decode(streams, elems, lanes, indexed, tables):
    rows = TABLES[tables]()
    index, value = draw_streams(rows, streams, elems, indexed, seed=7 * streams + elems + lanes)
    got = round_trip(ans_cases.lookup_of(rows), value, index if indexed else None, lanes)
    if elems == 4097:
        words = (len(got[0]) - 4 * min(elems, lanes)) // 2
        assert words > 2 * 4 * 64, "this case is here to move the decoder's word window"


def test_escape_rounds():
    """A round in which all 64 lanes escape with four calls each, one in which exactly one lane does, and an escape in
    the last, partial round."""
    rows = ans_cases.mixed_rows()
    lookup = ans_cases.lookup_of(rows)
    n = 3 * 64 + 2
    index = np.full((1, n), 2, np.int32)                    # P = 12, 33 symbols, the last one the escape
    value = np.random.default_rng(0).integers(0, 32, (1, n)).astype(np.int32)
    value[0, 64:128] = [(-1) ** j * (2 ** 30 + 12345 * j) for j in range(64)]     # k = 30: head, 16 low bits, 14 high bits
    value[0, 128 + 17] = -70000                             # the only escape of round 2 (k = 16: no high bits)
    value[0, n - 1] = -2 ** 31                              # the last element, in a round of two
    index[0, 5] = 0                                         # and one P = 1 row, whose every value but 0 escapes
    value[0, 5] = 1
    round_trip(lookup, value, index, 64)
    round_trip(lookup, value, index, 32)


def test_rows_narrower_and_wider_than_64_symbols_share_a_round():
    rows = ans_cases.mixed_rows()                           # 2, 5, 33, 301, 17 symbols and the one-symbol row
    n = 128
    index = (np.arange(n) % len(rows)).astype(np.int32)[None]
    _, value = ans_cases.draw(rows, n, 3, index=index[0])
    round_trip(ans_cases.lookup_of(rows), value[None], index, 64)


def decode_guarded(lookup, strings, streams, elems, index, lanes, stream_index=None):
    """tfc_ans_decode into the middle of sentinel-filled buffers -> (symbols, ok), the guards checked."""
    device = torch.device("cuda")
    tables = gen_ops._tables_for(torch.from_numpy(lookup))
    blob = torch.from_numpy(np.frombuffer(b"".join(strings) + b"\0", np.uint8).copy()).to(device)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)).to(device)
    guard = 64
    out = torch.full((2 * guard + streams * elems,), -7777, dtype=torch.int32, device=device)
    ok = torch.full((2 * guard + len(strings),), 99, dtype=torch.uint8, device=device)
    index_d = None if index is None else torch.from_numpy(index).to(device).contiguous()
    sidx = None if stream_index is None else torch.tensor(stream_index, dtype=torch.int32, device=device)
    rc = _lib.lib().tfc_ans_decode(tables.ptr, blob.data_ptr(), offsets.data_ptr(), _lib.ptr(sidx), len(strings),
                                   _lib.ptr(index_d), streams, elems, lanes, out[guard:].data_ptr(),
                                   ok[guard:].data_ptr(), _lib.stream_ptr())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    out, ok = out.cpu().numpy(), ok.cpu().numpy()
    assert (out[:guard] == -7777).all() and (out[-guard:] == -7777).all()
    assert (ok[:guard] == 99).all() and (ok[-guard:] == 99).all()
    return out[guard:-guard].reshape(streams, elems), ok[guard:-guard]


def test_random_bytes_decode_as_the_definition_says():
    for tables in ("mixed", "big"):
        random_bytes_decode_as_the_definition_says(tables)


def random_bytes_decode_as_the_definition_says(tables):
    rows = TABLES[tables]()
    lookup = ans_cases.lookup_of(rows)
    rng = np.random.default_rng(5)
    streams, elems, lanes = 9, 300, 64
    index = rng.integers(0, len(rows), (streams, elems)).astype(np.int32)
    sizes = [0, 1, 3, 255, 256, 257, 258, 600, 4000]
    strings = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for size in sizes]
    want, want_ok = ans_ops.ans_decode_reference(strings, lookup, (streams, elems), index, lanes)
    got, ok = decode_guarded(lookup, strings, streams, elems, index, lanes)
    assert np.array_equal(ok.astype(bool), want_ok)
    assert np.array_equal(got, want)


def test_damaged_strings_are_refused():
    rows = ans_cases.mixed_rows()
    lookup = ans_cases.lookup_of(rows)
    streams, elems, lanes = 4, 1000, 64
    index, value = draw_streams(rows, streams, elems, True, seed=21)
    good = ans_ops.ans_encode_reference(lookup, value, index, lanes)
    strings = [good[0][:-2], good[1] + b"\0\0", good[2] + b"\0", good[3]]
    want, want_ok = ans_ops.ans_decode_reference(strings, lookup, (streams, elems), index, lanes)
    assert list(want_ok) == [False, False, False, True]
    got, ok = decode_guarded(lookup, strings, streams, elems, index, lanes)
    assert list(ok) == [0, 0, 0, 1]
    assert np.array_equal(got, want)


def test_a_stream_index_outside_the_layout_writes_its_verdict_only():
    rows = ans_cases.mixed_rows()
    lookup = ans_cases.lookup_of(rows)
    streams, elems, lanes = 3, 200, 32
    index, value = draw_streams(rows, streams, elems, True, seed=33)
    good = ans_ops.ans_encode_reference(lookup, value, index, lanes)
    got, ok = decode_guarded(lookup, [good[2], good[0], good[0], good[0]], streams, elems, index, lanes,
                             stream_index=[2, 3, -1, 0])
    assert list(ok) == [1, 0, 0, 1]
    assert np.array_equal(got[0], value[0]) and np.array_equal(got[2], value[2])
    assert (got[1] == -7777).all()


def test_a_value_outside_a_row_without_escape_sets_its_streams_status():
    rows = [ans_cases.gaussian_row(12, 17, False), ans_cases.gaussian_row(12, 9, False)]
    lookup = ans_cases.lookup_of(rows)
    streams, elems, lanes = 4, 150, 64
    index, value = draw_streams(rows, streams, elems, True, seed=40)
    want = ans_ops.ans_encode_reference(lookup, value, index, lanes)
    value[1, 77] = 17 if index[1, 77] == 0 else -1
    index[3, 5] = 2
    encoded = ans_ops.ans_encode(torch.from_numpy(lookup), torch.from_numpy(value), torch.from_numpy(index), lanes)
    assert encoded.status.cpu().tolist() == [0, ans_ops.STATUS_VALUE, 0, ans_ops.STATUS_INDEX]
    with pytest.raises(ValueError, match="not in range"):
        ans_ops.strings_from_blob(encoded)
    got = ans_ops.strings_from_blob(encoded, check=False)
    assert got[0] == want[0] and got[2] == want[2]


def test_bad_arguments_are_refused_before_a_launch():
    table = torch.from_numpy(ans_cases.lookup_of(ans_cases.mixed_rows()))
    with pytest.raises(ValueError, match="lanes"):
        ans_ops.ans_encode(table, torch.zeros(1, 4, dtype=torch.int32), lanes=3)
    with pytest.raises(ValueError, match="strings are needed"):
        ans_ops.ans_decode([b""], table, (2, 4))
    with pytest.raises(ValueError, match="shape"):
        ans_ops.ans_encode(table, torch.zeros(1, 4, dtype=torch.int32), index=torch.zeros(1, 5, dtype=torch.int32))
