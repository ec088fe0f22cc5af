"""CPU tier: the interleaved rANS stream format as `ans_encode_reference` / `ans_decode_reference`
define it in exact integers — round trip, verdict, size against the tables' ideal, recorded vectors — and the serial
host coder of compression_amd/csrc/ans_core.h, compiled with the host compiler, held to the definition's bytes and its
quotient/remainder helper to Python's divmod."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import ans_cases
from compression_amd.ops import ans_ops

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = list(itertools.product(ans_cases.LANES, ans_cases.SIZES))


@pytest.fixture(scope="module")
def coded():
    """(lanes, n) -> (lookup, index, value, the definition's string), coded once for the module."""
    out = {}
    for lanes, n in GRID:
        rows, index, value = ans_cases.grid_case(lanes, n)
        lookup = ans_cases.lookup_of(rows)
        data, = ans_ops.ans_encode_reference(lookup, value, index, lanes)
        out[lanes, n] = (rows, lookup, index, value, data)
    return out


def each_case(check):
    """Runs `check(lanes, n)` over the whole grid in one test (the suite's test count stays small); a failure names
    its case."""
    for lanes, n in GRID:
        try:
            check(lanes, n)
        except AssertionError as e:
            raise AssertionError(f"lanes={lanes} n={n}: {e}") from e


def test_round_trip_verdict_and_size(coded):
    each_case(lambda lanes, n: _round_trip_verdict_and_size(coded, lanes, n))


def _round_trip_verdict_and_size(coded, lanes, n):
    rows, lookup, index, value, data = coded[lanes, n]
    got, ok = ans_ops.ans_decode_reference([data], lookup, (1, n), index, lanes)
    assert np.array_equal(got[0], value)
    assert bool(ok[0])
    # the tables' ideal over all calls, the reference's own 0.5 % allowance for its coder
    # (continuous_batched_test.py:143-145), and the format's states
    ideal = float(ans_ops.ans_ideal_bits(lookup, value, index)[0])
    print(f"lanes={lanes} n={n}: {8 * len(data)} bits, ideal {ideal:.1f}, states {32 * min(n, lanes)}")
    assert 8 * len(data) <= 1.005 * ideal + 32 * min(n, lanes) + 16
    if n == 0:
        assert data == b""


def test_damaged_strings_are_refused(coded):
    each_case(lambda lanes, n: _damaged_strings_are_refused(coded, lanes, n))


def _damaged_strings_are_refused(coded, lanes, n):
    rows, lookup, index, value, data = coded[lanes, n]

    def verdict(s):
        return bool(ans_ops.ans_decode_reference([s], lookup, (1, n), index, lanes)[1][0])

    if len(data) > 4 * min(n, lanes):
        assert not verdict(data[:-2]), "a string cut by one word"
    assert not verdict(data + b"\0\0"), "a string extended by a zero word"
    assert not verdict(data + b"\0"), "a string with an odd remainder"
    if n:
        assert not verdict(data[:4 * min(n, lanes) - 1]), "a string that lacks a state"


def test_every_int32_value_is_codable_on_an_escape_row():
    row = ans_cases.gaussian_row(12, 5, True)
    value = np.array(ans_cases.special_values(4) + [0, 3, 4, 5, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
    for lanes in (1, 8, 64):
        data, = ans_ops.ans_encode_reference(np.array(row, np.int32), value, None, lanes)
        got, ok = ans_ops.ans_decode_reference([data], np.array(row, np.int32), (1, value.size), None, lanes)
        assert np.array_equal(got[0], value) and bool(ok[0])


def test_a_value_outside_a_row_without_escape_is_the_callers_error():
    lookup = np.array(ans_cases.gaussian_row(12, 17, False), np.int32)
    for bad in (-1, 17, 2 ** 30):
        with pytest.raises(ValueError, match="not in range"):
            ans_ops.ans_encode_reference(lookup, np.array([3, bad], np.int32))
    with pytest.raises(ValueError, match="index"):
        ans_ops.ans_encode_reference(lookup, np.array([3], np.int32), np.array([1], np.int32))
    with pytest.raises(ValueError, match="lanes"):
        ans_ops.ans_encode_reference(lookup, np.array([3], np.int32), lanes=48)


def test_the_one_symbol_row_costs_nothing():
    lookup = np.array([16, 0, 65536], np.int32)
    data, = ans_ops.ans_encode_reference(lookup, np.zeros(1000, np.int32), lanes=64)
    assert data == np.full(64, 65536, "<u4").tobytes()


def test_recorded_vectors():
    """The format cannot drift silently: inputs and bytes recorded from the definition."""
    gold = np.load(ans_cases.GOLDEN)
    assert np.array_equal(gold["lookup"], ans_cases.lookup_of(ans_cases.mixed_rows()))
    assert len(gold["cases"]) >= 12
    for k, (lanes, n) in enumerate(gold["cases"]):
        index, value, want = gold[f"index{k}"], gold[f"value{k}"], gold[f"bytes{k}"].tobytes()
        data, = ans_ops.ans_encode_reference(gold["lookup"], value, index, int(lanes))
        assert data == want, (lanes, n)
        got, ok = ans_ops.ans_decode_reference([want], gold["lookup"], (1, int(n)), index, int(lanes))
        assert np.array_equal(got[0], value) and bool(ok[0])


# ---------------------------------------------------------------------------------------------- csrc/ans_core.h, hosted
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ans_core") / "ans_core_check.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(HERE, "native", "ans_core_check.cc")], check=True)
    lib = C.CDLL(so)
    lib.ans_check_encode.restype = C.c_longlong
    lib.ans_check_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                     C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_int)]
    lib.ans_check_decode.restype = C.c_int
    lib.ans_check_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong,
                                     C.c_longlong, C.c_int, C.c_void_p]
    lib.ans_check_divmod.restype = None
    lib.ans_check_divmod.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    return lib


def _native_encode(lib, rows, index, value, lanes):
    lookup, directory = ans_cases.lookup_of(rows), ans_cases.rows_directory(rows)
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    value = np.ascontiguousarray(value, np.int32)
    out = np.zeros(8 * value.size + 4 * lanes + 8, np.uint8)
    status = C.c_int(-1)
    n = lib.ans_check_encode(lookup.ctypes.data, directory.ctypes.data, len(rows),
                             None if index is None else index.ctypes.data, value.ctypes.data, value.size, lanes,
                             out.ctypes.data, out.size, C.byref(status))
    assert 0 <= n <= out.size
    return out[:n].tobytes(), status.value


def _native_decode(lib, rows, index, data, n, lanes):
    lookup, directory = ans_cases.lookup_of(rows), ans_cases.rows_directory(rows)
    index = None if index is None else np.ascontiguousarray(index, np.int32)
    buf = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    out = np.full(n + 2, -77, np.int32)
    ok = lib.ans_check_decode(lookup.ctypes.data, directory.ctypes.data, len(rows),
                              None if index is None else index.ctypes.data, buf.ctypes.data, len(data), n, lanes,
                              out[1:].ctypes.data)
    assert out[0] == -77 and out[-1] == -77
    return out[1:-1], bool(ok)


def test_host_coder_matches_the_definition(native, coded):
    each_case(lambda lanes, n: _host_coder_matches_the_definition(native, coded, lanes, n))


def _host_coder_matches_the_definition(native, coded, lanes, n):
    rows, lookup, index, value, data = coded[lanes, n]
    got, status = _native_encode(native, rows, index, value, lanes)
    assert status == 0 and got == data
    back, ok = _native_decode(native, rows, index, data, n, lanes)
    assert ok and np.array_equal(back, value)
    # the verdicts agree on damaged strings too, and so do the values decoded from them
    for damaged in (data[:-2], data + b"\0\0", data + b"\0", data[:3]):
        want_values, want_ok = ans_ops.ans_decode_reference([damaged], lookup, (1, n), index, lanes)
        back, ok = _native_decode(native, rows, index, damaged, n, lanes)
        assert ok == bool(want_ok[0]) and np.array_equal(back, want_values[0])


def test_host_coder_channel_mode_and_status(native):
    rows = ans_cases.mixed_rows()
    n = 333
    index, value = ans_cases.draw(rows, n, seed=5, index=np.arange(n) % len(rows))
    want, = ans_ops.ans_encode_reference(ans_cases.lookup_of(rows), value, None, 32)
    got, status = _native_encode(native, rows, None, value, 32)
    assert status == 0 and got == want
    value[4] = 99                                           # row 4 has no escape and 17 symbols
    assert _native_encode(native, rows, None, value, 32)[1] == ans_ops.STATUS_VALUE
    assert _native_encode(native, rows, np.full(n, 6, np.int32), value, 32)[1] & ans_ops.STATUS_INDEX


def test_host_coder_on_random_bytes(native):
    rows = ans_cases.mixed_rows()
    lookup = ans_cases.lookup_of(rows)
    rng = np.random.default_rng(11)
    for lanes, n in ((1, 40), (4, 130), (64, 300)):
        index = rng.integers(0, len(rows), n).astype(np.int32)
        for size in (0, 3, 4 * min(n, lanes), 4 * min(n, lanes) + 50, 2000):
            data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            want_values, want_ok = ans_ops.ans_decode_reference([data], lookup, (1, n), index, lanes)
            back, ok = _native_decode(native, rows, index, data, n, lanes)
            assert ok == bool(want_ok[0]) and np.array_equal(back, want_values[0])


def test_quotient_and_remainder_are_exact(native):
    freqs = [1, 2, 3, 255, 4095, 4096, 65535, 65536]
    xs, ds = [], []
    for d in freqs:
        top = (2 ** 32 - 1) // d
        for x in [2 ** 16, 2 ** 16 + 1, 2 ** 32 - 1] + [d * q + e for q in (1, 2, (2 ** 16) // d + 1, top - 1, top)
                                                        for e in (-1, 0, 1)]:
            if 0 <= x < 2 ** 32:
                xs.append(x)
                ds.append(d)
    rng = np.random.default_rng(3)
    xs = np.concatenate([np.array(xs, np.uint32), rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    ds = np.concatenate([np.array(ds, np.uint32), rng.integers(1, 65537, 100000).astype(np.uint32)])
    q, r = np.zeros_like(xs), np.zeros_like(xs)
    native.ans_check_divmod(xs.ctypes.data, ds.ctypes.data, xs.size, q.ctypes.data, r.ctypes.data)
    want_q, want_r = np.divmod(xs.astype(np.uint64), ds.astype(np.uint64))
    assert np.array_equal(q, want_q) and np.array_equal(r, want_r)


def test_core_header_is_plain_cxx(tmp_path):
    """g++ compiles ans_core.h with nothing else on the include path, and it names no HIP type."""
    header = os.path.join(os.path.dirname(HERE), "compression_amd", "csrc", "ans_core.h")
    src = tmp_path / "alone.cc"
    src.write_text('#include "%s"\nint main() { return tfc::ans::valid_lanes(64) ? 0 : 1; }\n' % header)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "alone"), str(src)],
                   check=True)
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    text = open(header).read()
    assert "hip/" not in text and "hipStream" not in text and "int2" not in text
