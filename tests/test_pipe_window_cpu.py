"""CPU tier: a model of the pipelined decoder's window rule (csrc/range_pipe.h, dec_chain_kernel: "refilled only when a
lane runs low").  Per lane one parked window of W bytes from `base`; at a memory phase the wave skips its request when
every lane has o + 66 <= W (o = position - base), else every lane requests from its position; the requested window is
parked behind the phase's block, so that block still reads the old one.  A block consumes at most 32 bytes of a lane
and reads at most 2 bytes ahead.  No read may reach base + W."""
import numpy as np
import pytest

BLOCK_BYTES = 32
AHEAD = 2
NEED = 2 * BLOCK_BYTES + AHEAD       # 66


def run(window, consumption):
    """consumption[block][lane] bytes; returns (phases, refills), asserts every read inside the parked window."""
    lanes = consumption.shape[1]
    pos = np.zeros(lanes, np.int64)
    base = np.zeros(lanes, np.int64)
    refills = 0
    for c in consumption:
        request = not np.all(pos - base + NEED <= window)
        requested_at = pos.copy()
        # the block: reads up to `AHEAD` bytes past what it consumes, from the window parked BEFORE this phase
        assert np.all(pos + c + AHEAD <= base + window), (window, int((pos + c + AHEAD - base).max()))
        pos = pos + c
        if request:
            base = requested_at
            refills += 1
    return len(consumption), refills


@pytest.mark.parametrize("window", [80, 96, 104])
def test_no_read_reaches_the_end_of_the_window(window):
    rng = np.random.default_rng(window)
    for lanes in (1, 2, 64):
        for kind in range(4):
            blocks = 400
            if kind == 0:
                c = rng.integers(0, BLOCK_BYTES + 1, (blocks, lanes))
            elif kind == 1:      # even digits only, as the coder consumes them
                c = 2 * rng.integers(0, BLOCK_BYTES // 2 + 1, (blocks, lanes))
            elif kind == 2:      # bursts: a lane is idle or at the maximum
                c = BLOCK_BYTES * (rng.random((blocks, lanes)) < 0.4)
            else:                # the largest skip, then the maximum
                c = np.tile(np.array([[window - NEED], [BLOCK_BYTES], [BLOCK_BYTES]]), (blocks // 3, lanes))
            phases, refills = run(window, np.asarray(c, np.int64))
            assert refills < phases


@pytest.mark.parametrize("window", [80, 96, 104])
def test_the_rule_is_tight(window):
    """One byte less of margin and the worst case — the largest offset that still skips, then two maximal blocks —
    reads past the window: 66 is not a round number."""
    o = window - NEED + 1      # would skip under o + 65 <= W
    assert o + BLOCK_BYTES + BLOCK_BYTES + AHEAD > window
    assert (window - NEED) + BLOCK_BYTES + BLOCK_BYTES + AHEAD <= window


def test_refills_per_phase_at_a_steady_rate():
    """Every lane at ~9 bytes per block (the headline's 4.07 bits per symbol): a window of 80 bytes is requested every
    other phase, wider ones less often."""
    c = np.full((400, 64), 9, np.int64)
    got = {w: run(w, c)[1] / 400 for w in (80, 96, 104)}
    assert got[80] == pytest.approx(0.5, abs=0.01) and got[96] == pytest.approx(0.25, abs=0.01) and got[104] == pytest.approx(0.2, abs=0.01)
