"""GPU tier: the pipelined decoder's chain writes a block record only where the parse reads one (csrc/range_pipe.h,
kPipeRecordEvery: the first block of every parse tile of 128 rows, and the chain's last row), and its steady-state loop
holds a block's staged raw rows in registers from the block to the next memory phase.  The cases put the chain's last row
on and off a tile edge — whole last tile, one block, a partial block — with and without escape codes (dense codes: some
lane's code straddles every tile edge, the record's "+ (M != 0)" term), in launches whose parse runs behind the chain,
and one large launch whose parse runs beside it on released rows.  Every case, in channel and in index mode, on the
full and the compact image with one and two chain waves per workgroup: bytes equal the oracle's
(cc/kernels/range_coder_kernels.cc:191-322), the oracle's bytes decode to the input (range_coder_kernels.cc:360-471)
with Finalize true, and the pipelined kernels took every call (tfc_pipe_counters: no fallback)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = 16                   # rows of a block (kPipeBlock)
TILE = 128                   # rows of a parse tile (kParseRows): a block record every TILE / BLOCK blocks
RELEASE = 64 * BLOCK         # rows between two releases of the chain (kPipeRelease blocks)
MARGIN = 96                  # rows behind a tile the parse beside the chain waits for (kParseMargin)
NTAB = 16                    # (channel mode: the steady-state loop wants a block inside one turn of the directory)

STREAMS = (64, 65, 130)      # one full group, a group with one live lane, three waves
# the chain's last row on a tile edge (128, 256), a row short of it, one and fifteen rows (one block) behind it, one row
# behind two tiles, a partial block in the fourth tile
ELEMS = (127, 128, 129, 143, 256, 257, 391)
FORMATS = ((1, 1), (1, 2), (2, 1), (2, 2))       # (image: 1 full, 2 compact; chain waves per workgroup)


@pytest.fixture(scope="module")
def tfc():
    import compression_amd
    compression_amd.set_default_mode("throughput")
    yield compression_amd
    compression_amd.set_default_mode("auto")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).cuda()


def counters():
    from compression_amd import _lib
    a, b = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().tfc_pipe_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


class pipe_format:
    def __init__(self, fmt, waves):
        self.fmt, self.waves = fmt, waves

    def __enter__(self):
        from compression_amd import _lib
        self.prev = _lib.lib().tfc_set_pipe_format(self.fmt, self.waves)
        assert self.prev >= 0

    def __exit__(self, *exc):
        from compression_amd import _lib
        _lib.lib().tfc_set_pipe_format(self.prev, 0)


# ---- tables at precision 12: geometric masses, without and with an escape symbol (tail mass 2 %) --------------------
def nplain():
    return np.asarray([3 + 2 * t for t in range(NTAB)])


def plain_rows(port):
    rows = []
    for n in nplain():
        p = 0.8 ** np.arange(n)
        cdf = np.asarray(port.pmf_to_quantized_cdf((p / p.sum()).astype(np.float32), 12), np.int32)
        rows.append(np.concatenate([[12], cdf]).astype(np.int32))
    return np.concatenate(rows)


def escape_rows(port):
    rows = []
    for n in nplain():
        p = 0.8 ** np.arange(n)
        p = np.concatenate([p, [0.02 * p.sum()]])
        cdf = np.asarray(port.pmf_to_quantized_cdf((p / p.sum()).astype(np.float32), 12), np.int32)
        rows.append(np.concatenate([[-12], cdf]).astype(np.int32))
    return np.concatenate(rows)


def plain_values(rng, tab):
    return np.minimum(rng.geometric(0.2, size=tab.shape) - 1, nplain()[tab] - 1).astype(np.int32)


def escape_values(rng, tab, share):
    """`share` of the elements are escape codes.  Nineteen in twenty have magnitude 1 (2 rows behind the escape symbol),
    one in five hundred a magnitude up to 2^20 (up to 42 rows): the launch plans a quarter more rows than elements."""
    n = nplain()[tab]
    sym = np.minimum(rng.geometric(0.2, size=tab.shape) - 1, n - 1)
    u = rng.random(tab.shape)
    bits = np.where(u < 0.95, 0, np.where(u < 0.998, rng.integers(1, 5, size=tab.shape), rng.integers(5, 21, size=tab.shape)))
    mag = (1 << bits) + rng.integers(0, 1 << 30, size=tab.shape) % (1 << bits)
    mag = np.minimum(mag, 1 << 20)
    esc = np.where(rng.random(tab.shape) < 0.5, n + mag - 1, -mag)
    return np.where(rng.random(tab.shape) < share, esc, sym).astype(np.int32)


def coder_calls(value, tab):
    """Calls of the reference's coder per stream (OverflowEncode, range_coder_kernels.cc:290-322): one per element, and
    behind an escape symbol the Elias-gamma code of g — n - 1 zeros, n bits — and the sign, n the bit length of g."""
    n = nplain()[tab].astype(np.int64)
    v = value.astype(np.int64)
    g = np.where(v < 0, -v, np.where(v >= n, v - n + 1, 0))
    length = np.frexp(g.astype(np.float64))[1]       # g = m 2^e with 1/2 <= m < 1: e is the bit length (0 for g = 0)
    return (1 + np.where(g > 0, 2 * length, 0)).sum(axis=1)


# ---- one case: encode against the oracle once, decode under every format -------------------------------------------
def run_case(tfc, port, lookup, value, index, threads=1):
    streams, elems = value.shape
    lt = torch.from_numpy(lookup)
    want = port.encode(lookup, value, index=index, threads=threads)[0]
    h = tfc.create_range_encoder([streams], lt)
    h = tfc.entropy_encode_channel(h, dev(value)) if index is None else tfc.entropy_encode_index(h, dev(index), dev(value))
    got = [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)]
    assert got == want
    arr = np.empty(len(want), dtype=object)
    for i, x in enumerate(want):
        arr[i] = x
    dindex = None if index is None else dev(index)
    for fmt, waves in FORMATS:
        with pipe_format(fmt, waves):
            l0, f0 = counters()
            hd = tfc.create_range_decoder(arr, lt)
            if index is None:
                hd, out = tfc.entropy_decode_channel(hd, [elems], torch.int32)
            else:
                hd, out = tfc.entropy_decode_index(hd, dindex, [elems], torch.int32)
            out = out.cpu().numpy().reshape(streams, elems)
            bad = np.argwhere(out != value)
            assert bad.size == 0, (fmt, waves, len(bad), bad[:4], out[tuple(bad[0])], value[tuple(bad[0])])
            assert bool(tfc.entropy_decode_finalize(hd).all()), (fmt, waves)
            l1, f1 = counters()
            assert l1 - l0 >= 1 and f1 - f0 == 0, ("decode", fmt, waves, l1 - l0, f1 - f0)


def both_modes(tfc, port, lookup, rng, streams, elems, values, threads=1):
    """`values(rng, tab)`: the elements for the tables `tab`.  Channel mode (table = element % NTAB), then index mode."""
    tab = np.broadcast_to(np.arange(elems)[None, :] % NTAB, (streams, elems))
    run_case(tfc, port, lookup, values(rng, tab), None, threads)
    index = rng.integers(0, NTAB, (streams, elems)).astype(np.int32)
    run_case(tfc, port, lookup, values(rng, index), index, threads)


def escape_dense(rng, tab):
    v = escape_values(rng, tab, 0.2)
    assert (v < 0).any() and (v >= nplain()[tab]).any()
    return v


# (law: tables, values, seed).  Without escape rows a row per element: the chain's last row is the element count rounded up
# to a block.  Dense codes, about one in five elements: with 64 lanes some lane is inside a code at every tile edge.
LAWS = {"no_escape_rows": (plain_rows, plain_values, 1), "dense_escape_codes": (escape_rows, escape_dense, 2)}


def test_tile_and_block_edges(tfc, port):
    """Every law x STREAMS x ELEMS, in one test: the cases are 0.05 s each, and the one that fails is named."""
    for law, (rows, values, seed) in LAWS.items():
        lookup = rows(port)
        for streams in STREAMS:
            for elems in ELEMS:
                rng = np.random.default_rng([streams, elems, seed])
                try:
                    both_modes(tfc, port, lookup, rng, streams, elems, values)
                except AssertionError as e:
                    raise AssertionError("case %s, %d streams, %d elements" % (law, streams, elems)) from e


def test_parse_beside_the_chain(tfc, port):
    """4096 streams are 64 groups, a large launch: the chain runs on a stream of its own and releases its rows every
    RELEASE rows, the parse beside it takes a tile once the rows behind it (MARGIN) are released.  With more than
    RELEASE + TILE + MARGIN rows a release comes before the chain's end, and the released tiles' records are those of
    blocks inside the stream, not the final one."""
    streams, elems, share = 4096, 1280, 0.05
    assert streams // 64 >= 64 and elems > RELEASE + TILE + MARGIN
    rng = np.random.default_rng([streams, elems, 3])

    def values(rng, tab):
        v = escape_values(rng, tab, share)
        assert (v < 0).any() and (v >= nplain()[tab]).any()
        # Planned capacity of a stream: elems + elems / 4 + 64 rows, and 24 blocks for what the WAVE adds to its slowest
        # lane (blocks lanes sit out or spend finishing a code, the tail pass).  Every stream's calls stay inside the
        # first part — before the GPU is used.
        calls = coder_calls(v, tab)
        assert int(calls.min()) >= elems and int(calls.max()) <= elems + elems // 4 + 64, (calls.min(), calls.max())
        return v
    both_modes(tfc, port, escape_rows(port), rng, streams, elems, values, threads=8)
