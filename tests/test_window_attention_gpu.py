"""GPU tier: the window-attention kernels (csrc/window_attention.hip) through `attention_ops.window_attention` against
the float64 definition of tests/window_attention_ref.py.

Cases: a greedy pairwise cover of window size, head dimension, heads, batch, shift (0 or ws / 2) and six (H, W) kinds
(one token, one window, a row of windows, a grid, ragged on both axes, ragged with a short last window), then window
counts one below, at and one above every windows-per-workgroup constant of csrc/window_attention_params.h (read
through attention_ops.WA_CONSTANTS) and window-group counts one below, at and one above the dtable partial count.
Every case runs in float32 and in bfloat16; the inputs are bfloat16-representable, so both share one float64 result.

Bars.  No number is chosen in advance beyond the stated slack; relative L2 against float64, for out, the q, k and v
parts of dqkv, and dtable:
    float32:  err_kernel <= 2 * err(window_attention_reference in float32 on the CPU) + 1e-6
              (2: other summation orders; 1e-6: the project's float32 slack)
    bfloat16: err_kernel <= 2 * err(the bfloat16 composition) + 2^-9      (2^-9: one output rounding)
Both errors are printed.  A float64 quantity that is identically zero (one token: dS = 0) must come out as zeros.

Exact probes, compared with `==`: window means (partition, roll, channel layout), 1e30 on excluded keys (weight exactly
0), a window as its own image and an image out of its batch (a window depends on its own tokens only), and two backward
calls (no atomics)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import window_attention_ref as ref
from compression_amd.ops import attention_ops as A

pytestmark = pytest.mark.gpu

K = A.WA_CONSTANTS
FWD = {8: K["WA_FWD_WINDOWS_WS8"], 4: K["WA_FWD_WINDOWS_WS4"]}
MFMA = {8: K["WA_MFMA_WINDOWS_WS8"], 4: K["WA_MFMA_WINDOWS_WS4"]}      # the bfloat16 forward
BWD = {8: K["WA_BWD_WINDOWS_WS8"], 4: K["WA_BWD_WINDOWS_WS4"]}
PARTS = K["WA_DTABLE_PARTIALS"]

HW_KINDS = {
    "token": lambda ws: (1, 1),
    "window": lambda ws: (ws, ws),
    "row": lambda ws: (ws, 2 * ws),
    "grid": lambda ws: (2 * ws, 3 * ws),
    "ragged": lambda ws: (ws + 1, 2 * ws - 1),
    "short": lambda ws: (3 * ws - 3, ws + 2),
}


def pairwise_cover(*axes):
    """A greedy cover of every pair of values of two different axes; deterministic."""
    tuples = list(itertools.product(*axes))
    pairs = lambda t: {(i, j, t[i], t[j]) for i in range(len(t)) for j in range(i + 1, len(t))}     # noqa: E731
    missing = set().union(*(pairs(t) for t in tuples))
    chosen = []
    while missing:
        best = max(tuples, key=lambda t: len(pairs(t) & missing))
        chosen.append(best)
        missing -= pairs(best)
    return chosen


def _cases():
    """(ws, d, heads, batch, shift, H, W) tuples."""
    found = []
    for ws, d, heads, batch, shifted, kind in pairwise_cover([4, 8], [16, 32], [1, 3], [1, 2], [False, True],
                                                             list(HW_KINDS)):
        found.append((ws, d, heads, batch, ws // 2 if shifted else 0) + HW_KINDS[kind](ws))
    # window counts around the windows-per-workgroup constants (a row of windows, the last one short)
    for ws in (4, 8):
        counts = sorted({n + e for n in (FWD[ws], MFMA[ws], BWD[ws]) for e in (-1, 0, 1)} - {0})
        for n in counts:
            found.append((ws, 16, 1, 1, ws // 2, ws, n * ws - 1))
    # window groups of the backward around the dtable partial count
    for ws in (4, 8):
        for groups in (PARTS - 1, PARTS, PARTS + 1):
            windows = groups * BWD[ws] if groups <= PARTS else PARTS * BWD[ws] + 1
            found.append((ws, 16, 1, 1, 0 if ws == 4 else 4, ws, windows * ws))
    return list(dict.fromkeys(found))


CASES = _cases()
DTYPES = [torch.float32, torch.bfloat16]


def case_id(c):
    return "ws%d-d%d-h%d-b%d-s%d-%dx%d" % c


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(qkv, table, dout) on the CPU in float32, qkv and dout bfloat16-representable."""
    ws, d, heads, batch, shift, h, w = case
    gen = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    qkv = torch.randn(batch, h, w, 3 * heads * d, generator=gen).bfloat16().float()
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen)
    dout = torch.randn(batch, h, w, heads * d, generator=gen).bfloat16().float()
    return qkv, table, dout


def split(dqkv):
    c = dqkv.shape[-1] // 3
    return dqkv[..., :c], dqkv[..., c:2 * c], dqkv[..., 2 * c:]


@functools.lru_cache(maxsize=None)
def truth(case):
    """out, dq, dk, dv, dtable in float64."""
    ws, d, heads, batch, shift, h, w = case
    qkv, table, dout = inputs(case)
    out = ref.forward(qkv, table, heads, ws, shift)
    dqkv, dtable = ref.backward(qkv, table, dout, heads, ws, shift)
    return (out,) + split(dqkv) + (dtable,)


def evaluate(fn, case, dtype, device):
    """out, dq, dk, dv, dtable of `fn` as float64 arrays."""
    ws, d, heads, batch, shift, h, w = case
    qkv, table, dout = inputs(case)
    qkv = qkv.to(device, dtype).requires_grad_(True)
    table = table.to(device).requires_grad_(True)
    out = fn(qkv, table, heads, ws, shift)
    dqkv, dtable = torch.autograd.grad(out, (qkv, table), dout.to(device, dtype))
    got = (out.detach(),) + split(dqkv) + (dtable,)
    return tuple(t.double().cpu().numpy() for t in got)


@functools.lru_cache(maxsize=None)
def composition(case, dtype):
    return evaluate(A.window_attention_reference, case, dtype, "cpu")


def rel_l2(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den else float(np.linalg.norm(a - b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_float64(case, dtype):
    want = truth(case)
    base = composition(case, dtype)
    got = evaluate(A.window_attention, case, dtype, "cuda")
    slack = 1e-6 if dtype == torch.float32 else 2.0 ** -9
    bad = []
    for name, g, b, t in zip(("out", "dq", "dk", "dv", "dtable"), got, base, want):
        assert g.shape == t.shape and np.isfinite(g).all(), name
        e_kernel, e_base = rel_l2(g, t), rel_l2(b, t)
        print(f"{name}: kernel {e_kernel:.3e}  composition {e_base:.3e}")
        if not np.any(t):
            if np.any(g):
                bad.append((name, "not zero"))
        elif not e_kernel <= 2 * e_base + slack:
            bad.append((name, e_kernel, e_base))
    assert not bad, bad


def test_cases_cover_the_constants():
    for ws in (4, 8):
        windows = {-(-c[5] // ws) * -(-c[6] // ws) * c[3] for c in CASES if c[0] == ws}
        for n in (FWD[ws], MFMA[ws], BWD[ws]):
            assert {n, n + 1} <= windows and (n == 1 or n - 1 in windows)
        groups = {-(-n // BWD[ws]) for n in windows}
        assert {PARTS - 1, PARTS, PARTS + 1} <= groups
    kinds = {(c[0], c[4] != 0) for c in CASES}
    assert kinds == {(4, False), (4, True), (8, False), (8, True)}


def run(qkv, table, heads, ws, shift):
    out = A.window_attention(qkv.cuda(), table.cuda(), heads, ws, shift)
    torch.cuda.synchronize()
    return out.cpu()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ws,d,heads", [(4, 16, 3), (8, 32, 2), (8, 16, 1), (4, 32, 1)])
def test_window_means_are_exact(ws, d, heads, dtype):
    """q = 0 and table = 0: every key that takes part weighs the same, the sum of small integers is exact and the one
    division is correctly rounded, so out is the mean of v over the query's class of its window: this pins the
    partition, the roll, the wrap classes and the channel layout."""
    gen = torch.Generator().manual_seed(ws * 100 + d)
    batch, h, w, c = 2, 2 * ws, 3 * ws, heads * d
    qkv = torch.randn(batch, h, w, 3 * c, generator=gen)
    qkv[..., :c] = 0
    qkv[..., 2 * c:] = torch.randint(-8, 9, (batch, h, w, c), generator=gen).float()
    table = torch.zeros(heads, (2 * ws - 1) ** 2)
    v = qkv[..., 2 * c:]
    for shift in (0, ws // 2):
        want = torch.full((batch, h, w, c), float("nan"))
        for tokens, _ in ref.windows(h, w, ws, shift):
            for fy, fx in itertools.product((False, True), repeat=2):
                members = [(tk[0], tk[1]) for tk in tokens if tk[2] and tk[3] == fy and tk[4] == fx]
                if members:
                    ys, xs = zip(*members)
                    mean = v[:, ys, xs].sum(dim=1) / torch.tensor(float(len(members)))      # float32: one rounding
                    for y, x in members:
                        want[:, y, x] = mean
        got = run(qkv.to(dtype), table, heads, ws, shift)
        assert torch.equal(bits(got), bits(want.to(dtype))), (shift, (got.float() - want).abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ws,d,heads,h,w", [(4, 16, 2, 9, 6), (8, 32, 1, 19, 12), (8, 16, 3, 16, 16)])
def test_excluded_keys_weigh_exactly_zero(ws, d, heads, h, w, dtype):
    """v = 1e30 on all tokens of one wrap class: the outputs of every other class are the bits of the run with those v
    zeroed (an excluded key is skipped, not given a large negative score)."""
    gen = torch.Generator().manual_seed(h * 100 + w)
    shift, c = ws // 2, heads * d
    qkv = torch.randn(2, h, w, 3 * c, generator=gen)
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen)
    seen = 0
    for fy, fx in itertools.product((False, True), repeat=2):
        inside = torch.zeros(h, w, dtype=torch.bool)
        for tokens, _ in ref.windows(h, w, ws, shift):
            for tk in tokens:
                if tk[2] and tk[3] == fy and tk[4] == fx:
                    inside[tk[0], tk[1]] = True
        if not inside.any() or inside.all():
            continue
        seen += 1
        huge, zero = qkv.clone(), qkv.clone()
        huge[:, inside, 2 * c:] = 1e30
        zero[:, inside, 2 * c:] = 0
        a, b = run(huge.to(dtype), table, heads, ws, shift), run(zero.to(dtype), table, heads, ws, shift)
        assert torch.isfinite(a[:, ~inside].float()).all()
        assert torch.equal(bits(a[:, ~inside]), bits(b[:, ~inside])), (fy, fx)
    assert seen >= 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ws,d,heads", [(4, 32, 2), (8, 16, 3)])
def test_a_window_depends_on_its_own_tokens_only(ws, d, heads, dtype):
    """A window cut out as its own ws x ws image, and image 1 of a batch run alone, give bit-identical outputs."""
    gen = torch.Generator().manual_seed(ws + d)
    nwy, nwx = 3, FWD[ws] + 1
    qkv = torch.randn(3, nwy * ws, nwx * ws - 1, 3 * heads * d, generator=gen).to(dtype)
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen)
    for shift in (0, ws // 2):
        whole = run(qkv, table, heads, ws, shift)
        alone = run(qkv[1:2], table, heads, ws, shift)
        assert torch.equal(bits(whole[1:2]), bits(alone)), shift
    whole = run(qkv, table, heads, ws, 0)
    for wy, wx in ((0, 0), (1, 1), (2, nwx - 2)):
        cut = qkv[2:3, wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws].contiguous()
        got = run(cut, table, heads, ws, 0)
        assert torch.equal(bits(got), bits(whole[2:3, wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws])), (wy, wx)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ws,d,heads,h,w", [(4, 16, 2, 4, 4 * (4 * 256 + 3)), (8, 32, 3, 21, 30)])
def test_backward_is_deterministic(ws, d, heads, h, w, dtype):
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn(2, h, w, 3 * heads * d, generator=gen).to(dtype).cuda()
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen).cuda()
    dout = torch.randn(2, h, w, heads * d, generator=gen).to(dtype).cuda()
    results = []
    for _ in range(2):
        q, t = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
        results.append(torch.autograd.grad(A.window_attention(q, t, heads, ws, ws // 2), (q, t), dout))
    assert torch.equal(bits(results[0][0]), bits(results[1][0]))
    assert torch.equal(bits(results[0][1]), bits(results[1][1]))


def test_a_gradient_nobody_needs_is_not_computed():
    """dtable alone and dqkv alone equal their parts of the joint call, bit for bit."""
    gen = torch.Generator().manual_seed(11)
    ws, d, heads = 8, 16, 2
    qkv = torch.randn(1, 13, 17, 3 * heads * d, generator=gen).cuda()
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen).cuda()
    dout = torch.randn(1, 13, 17, heads * d, generator=gen).cuda()
    q, t = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    both = torch.autograd.grad(A.window_attention(q, t, heads, ws, 4), (q, t), dout)
    q = qkv.clone().requires_grad_(True)
    only_q, = torch.autograd.grad(A.window_attention(q, table, heads, ws, 4), (q,), dout)
    t = table.clone().requires_grad_(True)
    only_t, = torch.autograd.grad(A.window_attention(qkv, t, heads, ws, 4), (t,), dout)
    assert torch.equal(bits(both[0]), bits(only_q)) and torch.equal(bits(both[1]), bits(only_t))
