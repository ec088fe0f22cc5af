"""CPU tier of the checkerboard context model: the torch twin of ops/checkerboard_ops.py against the float64 numpy
definition of tests/checkerboard_ref.py, teacher forcing, the compact order, the mask, CheckerboardConv2D, the packed
layout of both parameter classes, and the argument checks."""
import numpy as np
import pytest
import torch

import checkerboard_ref
import context_ref
from compression_amd.layers import CheckerboardConv2D
from compression_amd.ops import checkerboard_ops, context_ops

NUM_SCALES = 16
SHAPES = [(1, 1, 1, 3, 7, 5), (1, 1, 2, 3, 7, 5), (2, 3, 2, 4, 9, 6), (2, 4, 7, 5, 11, 9), (2, 5, 6, 4, 9, 6)]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _params(weights, dtype=torch.float64):
    return checkerboard_ops.CheckerboardParams(*[torch.from_numpy(np.asarray(w)).to(dtype) for w in weights], NUM_SCALES)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    y, psi, weights = context_ref.make_case(request.param, NUM_SCALES)
    want = checkerboard_ref.checkerboard_scan(y, psi, weights, NUM_SCALES)
    return y, psi, weights, want


def test_scan_reference_equals_the_numpy_definition(case):
    y, psi, weights, want = case
    yt, pt = torch.from_numpy(y).double(), torch.from_numpy(psi).double()
    got = checkerboard_ops.checkerboard_scan_reference(yt, pt, _params(weights))
    for name in ("mu", "y_hat", "index_float"):
        assert rel_l2(getattr(got, name).numpy(), want[name]) <= 1e-12, name
    assert np.array_equal(got.sym.numpy(), want["sym"])
    assert np.array_equal(got.idx.numpy(), want["idx"])
    assert got.sym.dtype == torch.int32 and got.idx.dtype == torch.int32
    # the public entries take CPU tensors through the same code
    pub = checkerboard_ops.checkerboard_scan(yt, pt, _params(weights))
    assert torch.equal(pub.y_hat, got.y_hat)
    for pass_ in (0, 1):
        mu, index = checkerboard_ops.checkerboard_parameters(got.y_hat, pt, _params(weights), pass_)
        assert torch.equal(mu, checkerboard_ops.checkerboard_split(got.mu)[pass_])
        assert torch.equal(index, checkerboard_ops.checkerboard_split(got.index_float)[pass_])


def test_teacher_forcing_returns_the_scans_parameters(case):
    y, psi, weights, want = case
    params = _params(weights)
    pt = torch.from_numpy(psi).double()
    got = checkerboard_ops.checkerboard_scan_reference(torch.from_numpy(y).double(), pt, params)
    mu, index = checkerboard_ops.checkerboard_parameters_reference(got.y_hat, pt, params)
    assert rel_l2(mu.numpy(), got.mu.numpy()) <= 1e-12
    assert rel_l2(index.numpy(), got.index_float.numpy()) <= 1e-12
    mu_np, index_np = checkerboard_ref.checkerboard_parameters(want["y_hat"], psi, weights)
    assert rel_l2(mu.numpy(), mu_np) <= 1e-12 and rel_l2(index.numpy(), index_np) <= 1e-12
    # the non-anchor positions do not matter to anyone: a pass-1 position sees anchors only
    noisy = got.y_hat.clone()
    others = ~checkerboard_ops.anchor_mask(*y.shape[1:3])
    noisy[:, others] += 1.0
    mu2, index2 = checkerboard_ops.checkerboard_parameters_reference(noisy, pt, params)
    assert torch.equal(mu2, mu) and torch.equal(index2, index)


@pytest.mark.parametrize("hl,wl", [(1, 1), (1, 2), (2, 1), (3, 2), (4, 7), (5, 6), (9, 8), (3, 7), (9, 15)])
def test_split_and_merge_are_inverses_in_the_closed_form_order(hl, wl):
    t = torch.arange(2 * hl * wl * 3, dtype=torch.float64).reshape(2, hl, wl, 3)
    a, b = checkerboard_ops.checkerboard_split(t)
    n0, n1 = -(-hl * wl // 2), hl * wl // 2
    assert tuple(a.shape) == (2, n0, 3) and tuple(b.shape) == (2, n1, 3)
    assert checkerboard_ops.pass_positions(hl, wl, 0) == n0 and checkerboard_ops.pass_positions(hl, wl, 1) == n1
    assert torch.equal(checkerboard_ops.checkerboard_merge(a, b, hl, wl), t)
    anchors = checkerboard_ops.anchor_mask(hl, wl)
    for i in range(hl):
        for j in range(wl):
            assert bool(anchors[i, j]) == ((i + j) % 2 == 0)
            s = (i * wl + j) >> 1 if wl % 2 else i * (wl // 2) + (j >> 1)
            assert s == checkerboard_ref.slot(i, j, wl)
            assert torch.equal((a if (i + j) % 2 == 0 else b)[:, s], t[:, i, j]), (i, j)
    ref = checkerboard_ref.split(t.numpy())
    assert np.array_equal(a.numpy(), ref[0]) and np.array_equal(b.numpy(), ref[1])
    with pytest.raises(ValueError, match="positions per pass"):
        checkerboard_ops.checkerboard_merge(a, a, hl, wl + 2)


def test_mask_has_twelve_ones_and_none_on_the_centre():
    mask = checkerboard_ops.checkerboard_mask(torch.float64)
    assert tuple(mask.shape) == (5, 5, 1, 1) and int(mask.sum()) == 12 and mask[2, 2] == 0
    assert len(checkerboard_ops.CHECKER_TAPS) == 12 and checkerboard_ops.CHECKER_TAPS == checkerboard_ref.CHECKER_TAPS
    for di in range(-2, 3):
        for dj in range(-2, 3):
            assert mask[di + 2, dj + 2, 0, 0] == ((di + dj) % 2)
    assert list(checkerboard_ops.CHECKER_TAPS) == sorted(checkerboard_ops.CHECKER_TAPS)          # row-major
    # every tap of a pass-1 position lands on an anchor
    assert all((1 + di + 2 + dj) % 2 == 0 for di, dj in checkerboard_ops.CHECKER_TAPS)


def test_checkerboard_conv_sees_anchors_from_non_anchors_only():
    torch.manual_seed(0)
    layer = CheckerboardConv2D(6, 3).double()
    with torch.no_grad():
        layer.kernel_variable.normal_()                     # the masked taps hold values too
        layer.bias.normal_()
    mask = checkerboard_ops.checkerboard_mask(torch.float64)
    assert torch.equal(layer.kernel, layer.kernel_variable * mask)
    hl, wl = 6, 7
    anchors = checkerboard_ops.anchor_mask(hl, wl)
    x = torch.randn(2, hl, wl, 3, dtype=torch.float64)
    base = layer(x)
    # an anchor output ignores every input: it is the bias
    assert torch.equal(base[:, anchors], layer.bias.detach().expand(2, int(anchors.sum()), 6))
    other_input = layer(torch.randn(2, hl, wl, 3, dtype=torch.float64))
    assert torch.equal(other_input[:, anchors], base[:, anchors])
    assert not torch.equal(other_input[:, ~anchors], base[:, ~anchors])
    # a non-anchor output ignores every non-anchor input
    changed = x.clone()
    changed[:, ~anchors] += torch.randn(2, int((~anchors).sum()), 3, dtype=torch.float64)
    assert torch.equal(layer(changed), base)
    # the layer is the definition's context term
    w = (layer.kernel_variable.detach().numpy(), layer.bias.detach().numpy())
    for (a, b) in ((0, 0), (0, 1), (3, 4), (5, 6), (5, 0), (2, 3)):
        assert rel_l2(base[:, a, b].detach().numpy(), checkerboard_ref.context_at(x.numpy(), a, b, w)) <= 1e-12, (a, b)
    layer(x).square().sum().backward()
    grad = layer.kernel_variable.grad
    assert torch.all(grad[mask.expand_as(grad) == 0] == 0)
    assert torch.all(grad[mask.expand_as(grad) == 1] != 0)
    assert torch.all(layer.bias.grad != 0)


def _tap_rows(buf, sections, m, taps, weights):
    at, _, _, cols = sections["wc"]
    mp = -(-m // 4) * 4
    rows = buf[at:at + 12 * mp * cols].reshape(12, mp, cols)
    for k, (di, dj) in enumerate(taps):
        assert np.array_equal(rows[k, :m], weights[0][di + 2, dj + 2]), (k, di, dj)
        assert not rows[k, m:].any()


def test_checkerboard_params_packs_each_tap_where_the_header_says():
    _, _, weights = context_ref.make_case((1, 1, 1, 3, 7, 5), NUM_SCALES)
    params = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    assert (params.m, params.p, params.h1, params.h2) == (3, 6, 7, 5) and params.fits_kernel()
    buf = params.packed("cpu").numpy()
    sections, total = context_ops._layout(3, 6, 7, 5)
    assert buf.size == total
    # csrc/context_params.h: packed tap k is element 2 k + 1 of the 5x5 window, row-major
    taps = [((2 * k + 1) // 5 - 2, (2 * k + 1) % 5 - 2) for k in range(12)]
    assert tuple(taps) == checkerboard_ops.CHECKER_TAPS
    _tap_rows(buf, sections, 3, taps, weights)
    # every other section is what ContextParams packs
    plain = context_ops.ContextParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES).packed("cpu").numpy()
    after = sections["bc"][0]
    assert np.array_equal(buf[after:], plain[after:]) and not np.array_equal(buf[:after], plain[:after])
    # the masked kernel: the other 13 taps are gone whatever they held
    kernel = params.tensors(torch.float32, "cpu")[0].numpy()
    for di in range(-2, 3):
        for dj in range(-2, 3):
            want = weights[0][di + 2, dj + 2] if (di + dj) % 2 else np.zeros_like(weights[0][0, 0])
            assert np.array_equal(kernel[di + 2, dj + 2], want)


def test_context_params_packs_what_it_packed_before():
    """Computed from the causal tap list, section by section: nothing but these values, zeros elsewhere."""
    _, _, weights = context_ref.make_case((1, 1, 1, 3, 7, 5), NUM_SCALES)
    params = context_ops.ContextParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    assert params.TAPS == context_ref.CAUSAL_TAPS
    buf = params.packed("cpu").numpy()
    m, p, h1, h2 = 3, 6, 7, 5
    pad = lambda v: -(-v // 4) * 4
    want, at = [], 0

    def take(values, rows, padded, cols):
        nonlocal at
        block = np.zeros(pad(padded * cols), np.float32)
        block[:rows * cols] = np.asarray(values, np.float32).reshape(-1)
        want.append(block)
        at += block.size

    taps = np.zeros((12, pad(m), 2 * m), np.float32)
    causal = [(di, dj) for di in range(-2, 1) for dj in range(-2, 3) if di < 0 or dj < 0]
    for k, (di, dj) in enumerate(causal):
        taps[k, :m] = weights[0][di + 2, dj + 2]
    take(taps, 12 * pad(m), 12 * pad(m), 2 * m)
    take(weights[1], 1, 1, 2 * m)
    take(weights[2][:2 * m], 2 * m, pad(2 * m), h1)
    take(weights[2][2 * m:], p, pad(p), h1)
    take(weights[3], 1, 1, h1)
    take(weights[4], h1, pad(h1), h2)
    take(weights[5], 1, 1, h2)
    take(weights[6], h2, pad(h2), 2 * m)
    take(weights[7], 1, 1, 2 * m)
    assert np.array_equal(buf, np.concatenate(want))
    assert torch.equal(context_ops.ContextParams.mask(), context_ops.causal_mask())


def test_argument_errors_are_text():
    y, psi, weights = context_ref.make_case((1, 2, 3, 4, 9, 6), NUM_SCALES)
    t = [torch.from_numpy(w) for w in weights]
    params = checkerboard_ops.CheckerboardParams(*t, NUM_SCALES)
    with pytest.raises(ValueError, match=r"kernel must be \[5, 5, M, 2M\]"):
        checkerboard_ops.CheckerboardParams(t[0][:3], *t[1:], NUM_SCALES)
    with pytest.raises(ValueError, match="num_scales"):
        checkerboard_ops.CheckerboardParams(*t, 0)
    yt, pt = torch.from_numpy(y), torch.from_numpy(psi)
    with pytest.raises(ValueError, match="psi must be"):
        checkerboard_ops.checkerboard_scan(yt, pt[..., :-1], params)
    with pytest.raises(ValueError, match="y must be"):
        checkerboard_ops.checkerboard_scan(yt[..., :-1], pt, params)
    with pytest.raises(ValueError, match="share"):
        checkerboard_ops.checkerboard_scan(yt[:, :1], pt, params)
    with pytest.raises(ValueError, match="pass_ must be 0 or 1"):
        checkerboard_ops.checkerboard_parameters(yt, pt, params, 2)
    # the two parameter classes are not interchangeable: their packed taps mean different neighbours
    causal = context_ops.ContextParams(*t, NUM_SCALES)
    with pytest.raises(TypeError, match="CheckerboardParams"):
        checkerboard_ops.checkerboard_scan(yt, pt, causal)
    with pytest.raises(TypeError, match="ContextParams"):
        context_ops.context_scan(yt, pt, params)
    with pytest.raises(ValueError, match="needs float32 psi on the device"):
        checkerboard_ops.checkerboard_decode([[b"", b""]], pt, params, None)
    with pytest.raises(ValueError, match="sym and mu must be"):
        checkerboard_ops.checkerboard_place(torch.zeros(1, 2, 4), torch.zeros(1, 3, 4), torch.zeros(1, 2, 3, 4), 0)
    # place on CPU tensors is the definition's store
    y_hat = torch.zeros(1, 2, 3, 4)
    sym, mu = torch.full((1, 3, 4), 2.0), torch.full((1, 3, 4), 0.25)
    checkerboard_ops.checkerboard_place(sym, mu, y_hat, 1)
    anchors = checkerboard_ops.anchor_mask(2, 3)
    assert bool((y_hat[:, ~anchors] == 2.25).all()) and bool((y_hat[:, anchors] == 0).all())


def test_c_abi_argument_errors_need_no_device():
    """tfc_checkerboard_params / _place check their arguments on the host before any launch."""
    from compression_amd import _lib
    lib = _lib.lib()
    _, _, weights = context_ref.make_case((1, 1, 2, 3, 7, 5), NUM_SCALES)
    packed = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES).packed("cpu")
    n = packed.numel()
    args = lambda **kw: [kw.get("pass_", 0), None, None, None, None, kw.get("n", n), kw.get("batch", 1), kw.get("hl", 1),
                         kw.get("wl", 2), kw.get("m", 3), 6, kw.get("h1", 7), 5, NUM_SCALES, None, None, None, None, None]
    assert lib.tfc_checkerboard_params(*args(n=3)) != 0 and "packed weights" in _lib.last_error()
    assert lib.tfc_checkerboard_params(*args(pass_=2)) != 0 and "pass must be 0 or 1" in _lib.last_error()
    assert lib.tfc_checkerboard_params(*args(m=0)) != 0 and "at least 1" in _lib.last_error()
    assert lib.tfc_checkerboard_params(*args()) != 0 and "must not be null" in _lib.last_error()
    assert lib.tfc_checkerboard_params(*args(batch=0)) == 0                      # nothing to do
    assert lib.tfc_checkerboard_params(*args(pass_=1, wl=1)) == 0                # a 1x1 latent has no second pass
    wide = context_ops._layout(192, 384, 1200, 512)[1]
    rc = lib.tfc_checkerboard_params(0, None, None, None, None, wide, 1, 1, 2, 192, 384, 1200, 512, NUM_SCALES, None, None,
                                     None, None, None)
    assert rc != 0 and "160 KiB" in _lib.last_error()
    assert lib.tfc_checkerboard_place(3, None, None, None, 1, 1, 2, 3, None) != 0 and "pass must be" in _lib.last_error()
    assert lib.tfc_checkerboard_place(0, None, None, None, 1, 1, 2, 3, None) != 0 and "must not be null" in _lib.last_error()
    assert lib.tfc_checkerboard_place(0, None, None, None, 0, 1, 2, 3, None) == 0
