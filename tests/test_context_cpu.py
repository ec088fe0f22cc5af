"""CPU tier of the context model: the torch twin of ops/context_ops.py against the float64 numpy definition of
tests/context_ref.py, the order independence the wavefront rests on, the mask of MaskedConv2D, the decode loop on the
CPU against strings of the oracle's coder, and the argument checks."""
import numpy as np
import pytest
import torch

import context_ref
from compression_amd import synthetic
from compression_amd.layers import MaskedConv2D
from compression_amd.ops import context_ops
from oracle import oracle

NUM_SCALES = 16
SHAPES = [(1, 1, 1, 3, 7, 5), (2, 3, 2, 4, 9, 6), (2, 4, 7, 5, 11, 9)]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _params(weights, dtype=torch.float64):
    return context_ops.ContextParams(*[torch.from_numpy(np.asarray(w)).to(dtype) for w in weights], NUM_SCALES)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    y, psi, weights = context_ref.make_case(request.param, NUM_SCALES)
    want = context_ref.context_scan(y, psi, weights, NUM_SCALES)
    return y, psi, weights, want


def test_scan_reference_equals_the_numpy_definition(case):
    y, psi, weights, want = case
    got = context_ops.context_scan_reference(torch.from_numpy(y).double(), torch.from_numpy(psi).double(),
                                             _params(weights))
    for name in ("mu", "y_hat", "index_float"):
        assert rel_l2(getattr(got, name).numpy(), want[name]) <= 1e-12, name
    assert np.array_equal(got.sym.numpy(), want["sym"])
    assert np.array_equal(got.idx.numpy(), want["idx"])
    assert got.sym.dtype == torch.int32 and got.idx.dtype == torch.int32
    # the public entry takes CPU tensors through the same code
    pub = context_ops.context_scan(torch.from_numpy(y).double(), torch.from_numpy(psi).double(), _params(weights))
    assert torch.equal(pub.y_hat, got.y_hat)


def test_teacher_forcing_returns_the_scans_parameters(case):
    y, psi, weights, want = case
    params = _params(weights)
    got = context_ops.context_scan_reference(torch.from_numpy(y).double(), torch.from_numpy(psi).double(), params)
    mu, index = context_ops.context_parameters_reference(got.y_hat, torch.from_numpy(psi).double(), params)
    assert rel_l2(mu.numpy(), got.mu.numpy()) <= 1e-12
    assert rel_l2(index.numpy(), got.index_float.numpy()) <= 1e-12
    mu_np, index_np = context_ref.context_parameters(want["y_hat"], psi, weights)
    assert rel_l2(mu.numpy(), mu_np) <= 1e-12 and rel_l2(index.numpy(), index_np) <= 1e-12


def test_raster_and_wavefront_order_agree(case):
    y, psi, weights, want = case
    params = _params(weights)
    yt, pt = torch.from_numpy(y).double(), torch.from_numpy(psi).double()
    raster = context_ops.context_scan_reference(yt, pt, params, order="raster")
    wave = context_ops.context_scan_reference(yt, pt, params, order="wavefront")
    for a, b in zip(raster, wave):
        assert torch.equal(a, b)
    hl, wl = y.shape[1:3]
    other = context_ref.context_scan(y, psi, weights, NUM_SCALES, order=context_ref.wavefront_order(hl, wl))
    for name in want:
        assert np.array_equal(other[name], want[name]), name
    # the steps of ops.context_ops are that order, and every causal neighbour of a step's position is of an earlier step
    steps = context_ops.wavefront_steps(hl, wl)
    assert [p for s in steps for p in s] == context_ref.wavefront_order(hl, wl)
    step_of = {p: t for t, s in enumerate(steps) for p in s}
    for (i, j), t in step_of.items():
        for di, dj in context_ref.CAUSAL_TAPS:
            if (i + di, j + dj) in step_of:
                assert step_of[(i + di, j + dj)] < t


def test_wavefront_step_counts():
    assert len(context_ops.wavefront_steps(32, 48)) == 141
    assert max(len(s) for s in context_ops.wavefront_steps(32, 48)) == 16
    assert sum(len(s) for s in context_ops.wavefront_steps(5, 1)) == 5      # steps without a position exist: t = 1, 2


def test_masked_conv_is_causal_and_masked_taps_get_no_gradient():
    torch.manual_seed(0)
    layer = MaskedConv2D(6, 3).double()
    with torch.no_grad():
        layer.kernel_variable.normal_()                     # the non-causal taps hold values too
        layer.bias.normal_()
    mask = context_ops.causal_mask(torch.float64)
    assert torch.equal(layer.kernel, layer.kernel_variable * mask)
    assert int(mask.sum()) == 12 and mask[2, 2] == 0 and mask[2, 1] == 1 and mask[3:].sum() == 0
    x = torch.randn(2, 6, 7, 3, dtype=torch.float64)
    base = layer(x)
    i, j = 3, 4
    changed = x.clone()
    changed[:, i, j:] += torch.randn(2, 7 - j, 3, dtype=torch.float64)              # (i, j) itself and to the right
    changed[:, i + 1:] += torch.randn(2, 6 - i - 1, 7, 3, dtype=torch.float64)      # everything below
    again = layer(changed)
    assert torch.equal(again[:, i, j], base[:, i, j])
    assert torch.equal(again[:, :i], base[:, :i]) and torch.equal(again[:, i, :j + 1], base[:, i, :j + 1])
    assert not torch.equal(again[:, i, j + 1], base[:, i, j + 1])
    # the layer is the definition's context term
    w = (layer.kernel.detach().numpy(), layer.bias.detach().numpy())
    for (a, b) in ((0, 0), (3, 4), (5, 6)):
        assert rel_l2(base[:, a, b].detach().numpy(), context_ref.context_at(x.numpy(), a, b, w)) <= 1e-12
    layer(x).square().sum().backward()
    grad = layer.kernel_variable.grad
    assert torch.all(grad[mask.expand_as(grad) == 0] == 0)
    assert torch.all(grad[mask.expand_as(grad) == 1] != 0)


def _tables():
    port = oracle.port()
    pmfs, minima = synthetic.gaussian_pmfs(num_tables=NUM_SCALES, octave=2.0)
    cdfs = [port.pmf_to_quantized_cdf(p, 12) for p in pmfs]
    lookup = synthetic.assemble_lookup(cdfs, 12, overflow=True)
    return port, lookup, synthetic.lookup_rows(lookup), minima


def test_decode_loop_on_the_cpu_inverts_the_oracles_strings(case):
    y, psi, weights, want = case
    port, lookup, rows, cdf_offset = _tables()
    b, hl, wl, m = y.shape
    idx = want["idx"].reshape(b * hl, wl * m)
    value = want["sym"].reshape(b * hl, wl * m) - cdf_offset[idx]
    lengths = np.array([len(rows[t][1]) - 1 for t in range(NUM_SCALES)])
    assert np.any((value < 0) | (value >= lengths[idx] - 1)), "the inputs must take the escape"
    strings, _, _ = port.encode(lookup, value.astype(np.int32), index=idx.astype(np.int32))
    nested = [strings[n * hl:(n + 1) * hl] for n in range(b)]
    y_hat, ok = context_ref.context_decode(nested, psi, weights, NUM_SCALES, rows, cdf_offset)
    assert np.array_equal(y_hat, want["y_hat"])
    assert ok.all()
    # the order does not matter to the decoder either
    y_hat_r, _ = context_ref.context_decode(nested, psi, weights, NUM_SCALES, rows, cdf_offset,
                                            order=context_ref.raster_order(hl, wl))
    assert np.array_equal(y_hat_r, y_hat)
    # Damaged strings end the loop like intact ones.  `ok` is EntropyDecodeFinalize's weak check (range_coder.h:144-169),
    # which the oracle's decoder gives the same verdicts for: it fails when bytes are left over, but a string cut
    # short decodes zeros until base and window are both 0, which passes (measured on these inputs: cuts of 1 byte,
    # 2 bytes and half the string all pass, in the oracle too).  So a truncated string is asserted to end the loop
    # with a wrong y_hat, and a string with surplus bytes to end it with ok == False.
    cut = [list(per) for per in nested]
    cut[0][0] = cut[0][0][:len(cut[0][0]) // 2]
    y_hat_cut, ok_cut = context_ref.context_decode(cut, psi, weights, NUM_SCALES, rows, cdf_offset)
    # (the rows below the damaged one get wrong parameters, so their verdicts are not asserted; other images are)
    assert not np.array_equal(y_hat_cut[0, 0], want["y_hat"][0, 0]) and ok_cut[1:].all()
    assert np.array_equal(y_hat_cut[1:], want["y_hat"][1:])
    _, verdict = port.decode(lookup, [cut[0][0]], wl * m, index=idx[:1].astype(np.int32))
    print("truncated string: ok =", bool(ok_cut[0, 0]), "oracle's decoder on the same bytes:", bool(verdict[0]))
    longer = [list(per) for per in nested]
    longer[0][0] = longer[0][0] + b"\x12\x34\x56\x78"
    y_hat_long, ok_long = context_ref.context_decode(longer, psi, weights, NUM_SCALES, rows, cdf_offset)
    assert not ok_long[0, 0] and ok_long.reshape(-1)[1:].all()


def test_argument_errors_are_raised_on_the_host():
    y, psi, weights = context_ref.make_case((1, 2, 3, 4, 9, 6), NUM_SCALES)
    t = [torch.from_numpy(w) for w in weights]
    params = context_ops.ContextParams(*t, NUM_SCALES)
    assert (params.m, params.p, params.h1, params.h2) == (4, 8, 9, 6) and params.fits_kernel()
    with pytest.raises(ValueError, match=r"kernel must be \[5, 5, M, 2M\]"):
        context_ops.ContextParams(t[0][:3], *t[1:], NUM_SCALES)
    with pytest.raises(ValueError, match="w2 must be"):
        context_ops.ContextParams(t[0], t[1], t[2], t[3], t[4][:-1], *t[5:], NUM_SCALES)
    with pytest.raises(ValueError, match="b3 must be"):
        context_ops.ContextParams(*t[:7], t[7][:-1], NUM_SCALES)
    with pytest.raises(ValueError, match="num_scales"):
        context_ops.ContextParams(*t, 0)
    yt, pt = torch.from_numpy(y), torch.from_numpy(psi)
    with pytest.raises(ValueError, match="psi must be"):
        context_ops.context_scan(yt, pt[..., :-1], params)
    with pytest.raises(ValueError, match="y must be"):
        context_ops.context_scan(yt[..., :-1], pt, params)
    with pytest.raises(ValueError, match="share"):
        context_ops.context_scan(yt[:, :1], pt, params)
    with pytest.raises(ValueError, match="order"):
        context_ops.context_scan_reference(yt, pt, params, order="zigzag")
    with pytest.raises(TypeError, match="ContextParams"):
        context_ops.context_scan(yt, pt, weights)
    with pytest.raises(ValueError, match="needs float32 psi on the device"):
        context_ops.context_decode([[b""] * 2], pt, params, None, None)


def test_packed_layout_matches_the_header():
    """The packed buffer holds every weight where csrc/context_params.h says, zero elsewhere."""
    _, _, weights = context_ref.make_case((1, 1, 1, 3, 7, 5), NUM_SCALES)
    params = context_ops.ContextParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    buf = params.packed("cpu").numpy()
    sections, total = context_ops._layout(3, 6, 7, 5)
    assert buf.size == total and total % 4 == 0 and all(v[0] % 4 == 0 for v in sections.values())
    at, _, _, cols = sections["wc"]
    taps = buf[at:at + 12 * 4 * 6].reshape(12, 4, 6)
    for k, (di, dj) in enumerate(context_ref.CAUSAL_TAPS):
        assert np.array_equal(taps[k, :3], weights[0][di + 2, dj + 2]) and not taps[k, 3].any()
    at, rows, padded, cols = sections["w1p"]
    w1p = buf[at:at + padded * cols].reshape(padded, cols)
    assert np.array_equal(w1p[:rows], weights[2][6:]) and not w1p[rows:].any()
    at, rows, padded, cols = sections["w3"]
    assert np.array_equal(buf[at:at + rows * cols].reshape(rows, cols), weights[6])
    used = sum(v[1] * v[3] for v in sections.values())
    assert np.count_nonzero(buf) <= used
