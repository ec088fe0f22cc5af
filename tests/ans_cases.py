"""Tables, values and recorded vectors the ANS tests share (test_ans_format_cpu.py, test_ans_coder_gpu.py).

`python tests/ans_cases.py` writes tests/golden/ans_vectors.npz from the definition (`ans_encode_reference`): run it
only when the format is changed on purpose."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ans_vectors.npz")

LANES = (1, 4, 64)
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 5000)


def gaussian_row(precision, width, escape, sigma=None):
    """[+-precision, cdf...]: a Gaussian-shaped row of `width` symbols (the last one the escape where `escape`), every
    symbol at least one count wide."""
    total = 1 << precision
    k = np.arange(width) - (width - 1) / 2.0
    pmf = np.exp(-0.5 * (k / (sigma or max(width / 6.0, 0.7))) ** 2)
    freq = np.maximum(1, np.floor(pmf / pmf.sum() * (total - width)).astype(np.int64))
    freq[np.argmax(freq)] += total - freq.sum()
    assert freq.min() >= 1 and freq.sum() == total
    return [-precision if escape else precision] + [0] + list(np.cumsum(freq))


def mixed_rows():
    """The rows of the format grid: P = 1 with escape, P = 12 with escape (5 and 33 symbols), P = 16 with escape (301),
    P = 12 without escape, and the one-symbol row."""
    return [[-1, 0, 1, 2], gaussian_row(12, 5, True), gaussian_row(12, 33, True), gaussian_row(16, 301, True),
            gaussian_row(12, 17, False), [16, 0, 65536]]


def lookup_of(rows):
    return np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])


def rows_directory(rows):
    """(start of header, size) per row of lookup_of(rows), int32 [rows, 2]."""
    starts = np.cumsum([0] + [len(r) for r in rows[:-1]])
    return np.array([[s, len(r)] for s, r in zip(starts, rows)], dtype=np.int32)


def special_values(max_value):
    return [-1, -2, -70000, max_value, max_value + 1, max_value + 65536, -(2 ** 31 - 1), 2 ** 30, -2 ** 31]


def draw(rows, n, seed, index=None, escape_fraction=0.03):
    """(index, value) int32 [n]: rows drawn per element (or given), values from the row's own distribution, and
    `escape_fraction` of the elements on rows with escape from special_values."""
    rng = np.random.default_rng(seed)
    if index is None:
        index = rng.integers(0, len(rows), size=n)
    index = np.asarray(index, dtype=np.int32)
    value = np.zeros(n, dtype=np.int64)
    for i in range(n):
        row = rows[index[i]]
        cdf = np.asarray(row[1:], dtype=np.int64)
        nsym = len(cdf) - 1
        plain = nsym - 1 if row[0] < 0 else nsym            # symbols that are values of their own
        if row[0] < 0 and (plain == 0 or rng.random() < escape_fraction):
            value[i] = special_values(nsym - 1)[rng.integers(0, 9)]
            continue
        while True:
            s = int(np.searchsorted(cdf, rng.integers(0, cdf[-1]), side="right")) - 1
            if s < plain:
                value[i] = s
                break
    return index, value.astype(np.int32)


def grid_case(lanes, n):
    rows = mixed_rows()
    index, value = draw(rows, n, seed=1000 * lanes + n)
    return rows, index, value


GOLDEN_CASES = [(1, 1), (1, 65), (4, 2), (4, 63), (4, 129), (64, 1), (64, 63), (64, 64), (64, 65), (64, 129),
                (64, 1000), (4, 1000)]


def write_golden():
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from compression_amd.ops import ans_ops
    out = {"lookup": lookup_of(mixed_rows()), "cases": np.array(GOLDEN_CASES, dtype=np.int32)}
    for k, (lanes, n) in enumerate(GOLDEN_CASES):
        rows, index, value = grid_case(lanes, n)
        data, = ans_ops.ans_encode_reference(lookup_of(rows), value, index, lanes)
        out[f"index{k}"], out[f"value{k}"] = index, value
        out[f"bytes{k}"] = np.frombuffer(data, dtype=np.uint8)
    np.savez_compressed(GOLDEN, **out)


if __name__ == "__main__":
    write_golden()
