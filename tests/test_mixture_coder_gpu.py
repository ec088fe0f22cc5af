"""GPU tier of csrc/mixture_coder.hip: the dumped table against the float64 definition, the encoder's strings against the
CPU checker coding the same symbols on the dumped table (byte for byte, stream by stream: that ties the coder to the
reference coder's arithmetic), the decoder on all streams, on a subset and in another order, and on damaged strings.

The table bound: with K <= 4 the float32 F is within 1e-6 of the float64 one, times 65536 that is
below 0.07, so floor() moves by one count at the most."""
import numpy as np
import pytest
import torch

import mixture_ref
from compression_amd.ops import mixture_ops

pytestmark = pytest.mark.gpu


def _lo(L):
    return -2000 if L > 1000 else -7


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("L", mixture_ref.WINDOWS)
def test_dumped_table_against_the_definition(L, k):
    assert mixture_ref.WINDOWS[-1] == mixture_ops.MAX_WINDOW
    lo = _lo(L)
    params = mixture_ref.adversarial_parameters(k, L, lo)
    got = mixture_ops.mixture_cdf(*params, lo, L).cpu().numpy()
    want = mixture_ops.mixture_cdf_reference(*params, lo, L)
    mixture_ref.check_cdf_invariants(got, L)
    worst = int(np.abs(got.astype(np.int64) - want).max())
    print(f"\nMIXTURE_CDF L={L} K={k} worst difference {worst} count(s)")
    assert worst <= 1


# (stream_symbols, batch entries, elements per entry, L, K): streams of 1, 63, 64, 65 and 129 symbols; 1, 3 and 65
# streams; every window size at which the decoder's search changes shape (one round up to 64, two above); a last stream
# shorter than the rest in three of them
CASES = [
    (1, 1, 1, 64, 1),            # one stream of one symbol
    (1, 1, 3, 1, 2),             # three streams, a window of one value: empty strings
    (63, 3, 63, 2, 3),           # three batch entries of one stream
    (64, 1, 64 * 65, 65, 4),     # 65 streams
    (65, 1, 65 * 2 + 17, 64, 2),  # three streams, the last one of 17 symbols
    (129, 3, 129 + 40, 65, 3),   # two streams per entry, the second one of 40 symbols
    (129, 1, 129 * 2 + 5, 4096, 3),
    (64, 1, 64, 4096, 1),
    (63, 1, 63 * 65 - 9, 2, 4),  # 65 streams, the last one shorter
    (65, 2, 65, 1, 1),
]


def _case(case, seed=0):
    ss, batch, elems, L, k = case
    lo = _lo(L)
    rng = np.random.RandomState(seed + ss + 3 * L)
    logits, loc, scale = mixture_ref.random_parameters((batch, elems), k, lo, L, seed=seed + L + k)
    # draw around the means so that the symbols are likely ones and rare ones alike, and put both window ends into
    # every stream that has room for them
    pick = rng.randint(k, size=(batch, elems))
    centre = np.take_along_axis(loc.numpy(), pick[..., None], axis=-1)[..., 0]
    sym = np.rint(centre + rng.standard_normal((batch, elems)) * 3.0).astype(np.int64)
    sym = np.clip(sym, lo, lo + L - 1)
    for first in range(0, elems, ss):
        sym[:, first] = lo
        sym[:, min(first + ss, elems) - 1] = lo + L - 1 if min(ss, elems - first) > 1 else sym[:, first]
    return lo, L, torch.from_numpy(sym), (logits, loc, scale)


@pytest.fixture(scope="module")
def coded():
    """Every case encoded once: case -> (lo, L, symbols, parameters, strings)."""
    out = {}
    for case in CASES:
        lo, L, sym, params = _case(case)
        encoded = mixture_ops.mixture_encode(sym, *params, lo, L, case[0])
        out[case] = (lo, L, sym, params, mixture_ops.strings_from_blob(encoded))
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "ss%d-b%d-e%d-L%d-K%d" % c)
def test_strings_equal_the_checker_on_the_dumped_table(coded, port, case):
    ss, batch, elems, _, k = case
    lo, L, sym, params, strings = coded[case]
    per_entry = -(-elems // ss)
    assert len(strings) == batch * per_entry
    table = mixture_ops.mixture_cdf(*(p.reshape(-1, k) for p in params), lo, L).cpu().numpy().reshape(batch, elems, L + 1)
    mixture_ref.check_cdf_invariants(table, L)
    sym = sym.numpy()
    for b in range(batch):
        for s in range(per_entry):
            cut = slice(s * ss, min((s + 1) * ss, elems))
            want, back = mixture_ref.port_round_trip(port, sym[b, cut], table[b, cut], lo)
            assert (back == sym[b, cut]).all()
            assert strings[b * per_entry + s] == want, (b, s, len(want), len(strings[b * per_entry + s]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "ss%d-b%d-e%d-L%d-K%d" % c)
def test_decode_all_a_subset_and_another_order(coded, case):
    ss = case[0]
    lo, L, sym, params, strings = coded[case]
    got, ok = mixture_ops.mixture_decode(strings, *params, lo, L, ss)
    assert torch.equal(got.cpu().long(), sym) and bool(ok.all())
    n = len(strings)
    order = list(reversed(range(n)))[::2]                  # every other stream, last first
    got2, ok2 = mixture_ops.mixture_decode([strings[i] for i in order], *params, lo, L, ss, stream_index=order)
    assert bool(ok2.all()) and ok2.numel() == len(order)
    per_entry = -(-case[2] // ss)
    decoded = torch.zeros_like(sym, dtype=torch.bool)
    for i in order:
        b, s = divmod(i, per_entry)
        decoded[b, s * ss:(s + 1) * ss] = True
    assert torch.equal(got2.cpu().long()[decoded], sym[decoded])
    assert bool((got2.cpu()[~decoded] == 0).all())
    if n > 1:
        with pytest.raises(ValueError, match="more than once"):
            mixture_ops.mixture_decode([strings[0]] * 2, *params, lo, L, ss, stream_index=[0, 0])


def test_damaged_strings_stay_inside_the_window(coded):
    case = CASES[5]
    ss = case[0]
    lo, L, sym, params, strings = coded[case]
    assert all(len(s) > 8 for s in strings)
    damaged = list(strings)
    damaged[0] = b""
    damaged[2] = b"\xff" * len(strings[2])
    got, ok = mixture_ops.mixture_decode(damaged, *params, lo, L, ss)
    got, ok = got.cpu().long(), ok.cpu()
    assert int(got.min()) >= lo and int(got.max()) <= lo + L - 1
    # the empty string is refused (the symbols cost digits it does not hold); a string of 0xFF bytes may well be the
    # code of some symbols, so only its symbols are looked at
    assert ok[0] == 0 and ok[1] == 1 and bool(ok[3:].all())
    per_entry = -(-case[2] // ss)
    intact = torch.ones_like(sym, dtype=torch.bool)
    for i in (0, 2):
        b, s = divmod(i, per_entry)
        intact[b, s * ss:(s + 1) * ss] = False
    assert torch.equal(got[intact], sym[intact])


@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=lambda c: "ss%d-b%d-e%d-L%d-K%d" % c)
def test_strings_one_byte_short(coded, port, case):
    """Every string with its last byte taken off: the call returns, the symbols are inside the window, and `ok` is 0
    unless the shortened string is itself the code of the symbols that came out.  That is the rule of this stream format
    (DESIGN section 27): most shortened strings ARE what the encoder writes for some other symbols, so no decoder can
    tell them from damage, and the verdict has to be 1 exactly for those."""
    ss, batch, elems, _, k = case
    lo, L, sym, params, strings = coded[case]
    short = [s[:-1] for s in strings]
    got, ok = mixture_ops.mixture_decode(short, *params, lo, L, ss)
    got, ok = got.cpu().numpy().astype(np.int64), ok.cpu().numpy()
    assert got.min() >= lo and got.max() <= lo + L - 1
    table = mixture_ops.mixture_cdf(*(p.reshape(-1, k) for p in params), lo, L).cpu().numpy().reshape(batch, elems, L + 1)
    per_entry = -(-elems // ss)
    valid = []
    for i, string in enumerate(short):
        b, s = divmod(i, per_entry)
        cut = slice(s * ss, min((s + 1) * ss, elems))
        code = port.range_encode((got[b, cut] - lo).astype(np.int16), table[b, cut], 16, debug_level=0)
        # zero bytes at the end carry nothing: the decoder reads zeros behind a string anyway
        valid.append(code.rstrip(b"\0") == string.rstrip(b"\0"))
        if bool(ok[i]) != valid[-1]:
            print(f"\nMIXTURE_SHORT stream {i}: ok {ok[i]}, string {string.hex()}, code of its symbols {code.hex()}")
    print(f"\nMIXTURE_SHORT {len(short)} strings, {sum(valid)} of them the code of other symbols, "
          f"{int((ok == 0).sum())} refused")
    assert ok.tolist() == [int(v) for v in valid]
    assert not (got == sym.numpy()).all()
