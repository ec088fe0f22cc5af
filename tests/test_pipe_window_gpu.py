"""GPU tier: the pipelined decoder's code window is refilled only when a lane of the wave runs low (csrc/range_pipe.h,
dec_chain_kernel: "refilled only when a lane runs low").  One parked window of W bytes per lane; a memory phase skips
its request when every lane has its own block (32 bytes) and the next block's reads (34) inside the window, o + 66 <= W.
The cases drive the rule to its edges — no lane ever runs low, every lane always does, one lane decides for the wave, a
skip followed by maximal consumption, escape codes through the generic and sit-out paths, streams that end inside a
window, the index window — on the full and the compact image, with one and two chain waves per workgroup.  Bytes must
equal the oracle's (cc/kernels/range_coder_kernels.cc:191-322), the oracle's bytes must decode to the input
(range_coder_kernels.cc:360-471) with Finalize true, the pipelined kernels must have taken every call
(tfc_pipe_counters), and the chain's own counts (tfc_debug_pipe_window: memory phases and refills of the first chain
wave, streams 0 ... 63) must be what the byte counts of the oracle's strings allow."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = 96                       # bytes of a lane's window (PipeDecLds::kWords * 8)
BLOCK = 16                   # rows of a block (kPipeBlock): at most one 16-bit digit and one element per row
LOW = (W - (4 * BLOCK + 2)) + 1      # a lane this far into its window makes the wave request: o + 66 > W
PRECISION = 15
NTAB = 16                    # (channel mode: the steady-state loop wants a block inside one turn of the directory)

STREAMS = (64, 65, 130)      # one full group, a group with one live lane, three waves
ELEMS = (16 * 24, 16 * 24 + 1, 16 * 24 + 15)
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


def window_counts():
    from compression_amd import _lib
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().tfc_debug_pipe_window(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


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


# ---- tables -------------------------------------------------------------------------------------------------
# Two-rate rows at precision 15: row t has k(t) symbols of frequency 1 (15 bits each: sixteen of them are 30 bytes, a
# block's worst case but two) and one symbol with the rest of the mass (~1e-4 bits).
def rate_rows():
    ks = [1 + (t % 5) for t in range(NTAB)]
    rows = [np.concatenate([[PRECISION], np.arange(k + 1), [1 << PRECISION]]) for k in ks]
    return np.concatenate(rows).astype(np.int32), np.asarray(ks)


def rate_values(rng, tab, high):
    """`high`: which elements take a frequency-1 symbol; the others take their row's heavy one."""
    _, ks = rate_rows()
    k = ks[tab]
    return np.where(high, rng.integers(0, 1 << 30, size=tab.shape) % k, k).astype(np.int32)


def blocks_to_elems(per_block, elems):
    return np.repeat(per_block, BLOCK, axis=1)[:, :elems]


def case_lowest(s, e):
    return np.zeros((s, e), bool)


def case_highest(s, e):
    return np.ones((s, e), bool)


def case_fast_lane(s, e):
    h = np.zeros((s, e), bool)
    h[[5, s - 1]] = True
    return h


def case_slow_lane(s, e):
    return ~case_fast_lane(s, e)


def case_bursts(s, e):
    """Per lane: runs of one to three low-rate blocks, then two blocks at the highest rate, phase-shifted per lane — a
    skipped request followed by maximal consumption."""
    nb = -(-e // BLOCK)
    per_block = np.zeros((s, nb), bool)
    for lane in range(s):
        b, run = lane % 5, lane % 3
        while b < nb:
            b += 1 + run % 3
            per_block[lane, b:b + 2] = True
            b += 2
            run += 1
    return blocks_to_elems(per_block, e)


def case_short(s, e):
    """Streams that end inside a window: nothing but the heavy symbol (a few bytes in all); the same with the last one to
    six elements at the highest rate (the stream ends a few bytes after a run of skipped phases); one block at the highest
    rate somewhere (~34 bytes); every twelfth element (~60 bytes)."""
    h = np.zeros((s, e), bool)
    for lane in range(s):
        kind = lane % 4
        if kind == 1:
            h[lane, e - 1 - lane % 6:] = True
        elif kind == 2:
            b = (lane // 4) % (e // BLOCK)
            h[lane, BLOCK * b:BLOCK * (b + 1)] = True
        elif kind == 3:
            h[lane, lane % 12::12] = True
    return h


RATE_CASES = {"lowest": case_lowest, "highest": case_highest, "fast_lane": case_fast_lane, "slow_lane": case_slow_lane,
              "bursts": case_bursts, "short": case_short}


# Rows with an escape symbol at precision 12 (geometric masses, tail mass 2 %) for the dense escape codes.
def escape_rows(port):
    rows = []
    for t in range(NTAB):
        n = 3 + 2 * t
        p = 0.8 ** np.arange(n)
        p = np.concatenate([p, [0.02 * p.sum()]])
        cdf = np.asarray(port.pmf_to_quantized_cdf((p / p.sum()).astype(np.float32), 12), np.int32)
        rows.append(np.concatenate([[-12], cdf]).astype(np.int32))
    return np.concatenate(rows), np.asarray([3 + 2 * t for t in range(NTAB)])


def escape_values(rng, tab, nplain):
    """One element in five is an escape code.  Magnitudes up to 2^20, most of them short: the launch plans a quarter more
    rows than elements (and 448) for the codes' bits, the blocks a lane sits out and the wave's tail pass, and a stream that
    outgrows them is the fallback kernel's, which is not what this net is for — nineteen in twenty codes have magnitude 1 (2
    rows), one in five hundred a magnitude up to 2^20 (up to 42 rows)."""
    n = nplain[tab]
    sym = np.minimum(rng.geometric(0.2, size=tab.shape) - 1, n - 1)
    u = rng.random(tab.shape)
    bits = np.where(u < 0.95, 0, np.where(u < 0.998, rng.integers(1, 5, size=tab.shape), rng.integers(5, 21, size=tab.shape)))
    mag = (1 << bits) + rng.integers(0, 1 << 30, size=tab.shape) % (1 << bits)
    mag = np.minimum(mag, 1 << 20)
    esc = np.where(rng.random(tab.shape) < 0.5, n + mag - 1, -mag)
    return np.where(rng.random(tab.shape) < 0.2, esc, sym).astype(np.int32)


# ---- one case: encode against the oracle once, decode under every format -------------------------------------------
def run_case(tfc, port, lookup, value, index, check):
    streams, elems = value.shape
    lt = torch.from_numpy(lookup)
    want = port.encode(lookup, value, index=index)[0]
    h = tfc.create_range_encoder([streams], lt)
    h = tfc.entropy_encode_channel(h, dev(value)) if index is None else tfc.entropy_encode_index(h, dev(index), dev(value))
    got = [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)]
    assert got == want
    arr = np.empty(len(want), dtype=object)
    for i, x in enumerate(want):
        arr[i] = x
    lens = np.asarray([len(x) for x in want[:64]])
    for fmt, waves in FORMATS:
        with pipe_format(fmt, waves):
            l0, f0 = counters()
            hd = tfc.create_range_decoder(arr, lt)
            if index is None:
                hd, out = tfc.entropy_decode_channel(hd, [elems], torch.int32)
            else:
                hd, out = tfc.entropy_decode_index(hd, dev(index), [elems], torch.int32)
            phases, refills, index_refills = window_counts()
            out = out.cpu().numpy().reshape(streams, elems)
            bad = np.argwhere(out != value)
            assert bad.size == 0, (fmt, waves, bad[:4], out[tuple(bad[0])], value[tuple(bad[0])])
            assert bool(tfc.entropy_decode_finalize(hd).all()), (fmt, waves)
            l1, f1 = counters()
            assert l1 - l0 >= 1 and f1 - f0 == 0, ("decode", fmt, waves, l1 - l0, f1 - f0)
        print("format %d waves %d: %d phases, %d refills, %d index refills" % (fmt, waves, phases, refills, index_refills))
        # What holds for every input.  The first phase requests nothing (the window in front of the loop is whole).  A
        # request needs a lane that consumed LOW bytes since the last window was parked, those stretches of one lane do
        # not overlap, and a lane consumes no more digits than its string holds (+ 2: the digit a step reads ahead).
        assert phases >= -(-elems // BLOCK), (fmt, waves, phases)
        assert refills <= phases - 1, (fmt, waves, phases, refills)
        assert refills <= int(((lens + 2) // LOW).sum()), (fmt, waves, refills, lens)
        check(phases, refills, index_refills, lens)


@pytest.mark.parametrize("elems", ELEMS)
@pytest.mark.parametrize("streams", STREAMS)
@pytest.mark.parametrize("name", list(RATE_CASES))
def test_two_rate_streams(tfc, port, name, streams, elems):
    rng = np.random.default_rng([streams, elems, len(name)])
    lookup, _ = rate_rows()
    tab = np.broadcast_to(np.arange(elems)[None, :] % NTAB, (streams, elems))
    high = RATE_CASES[name](streams, elems)
    value = rate_values(rng, tab, high)

    def check(phases, refills, index_refills, lens):
        # no escape codes: a row per element, a phase per block of sixteen
        assert phases == -(-elems // BLOCK), (name, phases)
        if name == "lowest":
            # no lane's whole string reaches LOW bytes: the bound above is 0, far below the phase count
            assert int(lens.max()) + 2 < LOW and refills == 0, (refills, lens.max())
        if name in ("highest", "fast_lane", "slow_lane"):
            # 16 x 15 bits are 30 bytes of one lane in every block — 28 at the least: a digit is two bytes, and what a
            # block leaves in the coder's state the next one finds there.  One lane is enough, one slow lane changes nothing.
            # A window of 80 bytes (LOW = 15) is requested at every phase but the first.  At 96 bytes (LOW = 31) a lane that
            # took 28 or 30 bytes since its window was parked lets the wave skip ONE phase — after the next block it is 56
            # bytes in — so at least every other phase requests.
            if LOW <= 28:
                assert refills == phases - 1, (name, phases, refills)
            else:
                assert 28 + 28 >= LOW
                assert (phases - 1) // 2 <= refills <= phases - 1, (name, phases, refills)
        if name == "short":
            assert int(lens.min()) < 8 and int(lens.max()) < W, lens
    run_case(tfc, port, lookup, value, None, check)


@pytest.mark.parametrize("elems", ELEMS)
@pytest.mark.parametrize("streams", STREAMS)
def test_dense_escape_codes(tfc, port, streams, elems):
    rng = np.random.default_rng([streams, elems, 7])
    lookup, nplain = escape_rows(port)
    tab = np.broadcast_to(np.arange(elems)[None, :] % NTAB, (streams, elems))
    value = escape_values(rng, tab, nplain)
    assert (value < 0).any() and (np.abs(value) >= 1 << 12).any()

    def check(phases, refills, index_refills, lens):
        assert phases > -(-elems // BLOCK)          # the codes' bit rows
    run_case(tfc, port, lookup, value, None, check)


@pytest.mark.parametrize("elems", ELEMS)
@pytest.mark.parametrize("streams", STREAMS)
@pytest.mark.parametrize("name", ["bursts", "highest", "lowest"])
def test_index_mode(tfc, port, name, streams, elems):
    rng = np.random.default_rng([streams, elems, 11, len(name)])
    lookup, _ = rate_rows()
    index = rng.integers(0, NTAB, (streams, elems)).astype(np.int32)
    value = rate_values(rng, index, RATE_CASES[name](streams, elems))

    def check(phases, refills, index_refills, lens):
        assert phases == -(-elems // BLOCK)
        # the window of row addresses, same rule: a block of sixteen elements takes 32 of its bytes, 32 + 66 > W — every
        # phase but the first requests it
        assert index_refills == (phases - 1 if BLOCK * 2 >= LOW else 0), (phases, index_refills)
        if name == "highest":
            assert (phases - 1 if LOW <= 28 else (phases - 1) // 2) <= refills <= phases - 1
        if name == "lowest":
            assert refills == 0
    run_case(tfc, port, lookup, value, index, check)


def test_an_empty_value_tensor(tfc, port):
    lookup, _ = rate_rows()
    lt = torch.from_numpy(lookup)
    value = np.zeros((65, 0), np.int32)
    want = port.encode(lookup, value)[0]
    h = tfc.create_range_encoder([65], lt)
    h = tfc.entropy_encode_channel(h, dev(value))
    assert [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)] == want
    arr = np.empty(len(want), dtype=object)
    for i, x in enumerate(want):
        arr[i] = x
    hd = tfc.create_range_decoder(arr, lt)
    hd, out = tfc.entropy_decode_channel(hd, [0], torch.int32)
    assert tuple(out.shape) == (65, 0)
    assert bool(tfc.entropy_decode_finalize(hd).all())
