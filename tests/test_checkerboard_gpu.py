"""GPU tier of the checkerboard context model (the one-group case of csrc/space_channel.hip): checkerboard_scan against itself (exact, and
image by image against the batched call), against the float64 definition teacher-forced on its own y_hat, and
checkerboard_decode against the strings the indexed entropy model writes from the scan's outputs (bit-identical y_hat,
also for one image taken out of a batched encode).

The kernel's tile is 32 positions (CKB_TILE, checkerboard_ref.KERNEL_TILE): (2, 9, 15, ...) has 68 and 67 positions per
pass, more than two tiles and no multiple of one; (2, 9, 8, ...) has 36 at the model's widths.

The teacher-forced bound.  FLOAT32_DEVIATION_MU / _INDEX are the largest deviations of the float32 torch evaluation of
`checkerboard_parameters_reference` from its float64 evaluation, measured on the CPU on these inputs (all SHAPES; y_hat
of the float64 scan, rounded to float32); the kernel gets 4x that, the project's margin for a different summation
order and FMA contraction.  `float32_deviation` below is the measurement."""
import math

import numpy as np
import pytest
import torch

import checkerboard_ref
import context_ref
from compression_amd.ops import checkerboard_ops

pytestmark = pytest.mark.gpu

NUM_SCALES = 64
SHAPES = checkerboard_ref.GPU_SHAPES
# max |float32 - float64| over all SHAPES, measured on the CPU with `float32_deviation` (per shape, (mu, index_float):
# 3.4e-07 8.8e-06 | 8.0e-07 1.5e-05 | 7.8e-07 1.0e-05 | 1.2e-06 2.4e-05 | 8.1e-07 1.6e-05 | 1.8e-06 3.5e-05 |
# 2.5e-06 5.1e-05 | 4.2e-06 6.1e-05 | 1.3e-06 2.6e-05; the means are of order 1, the indexes of order 64).  The
# kernel's bounds are 4x: 1.66e-05 for mu, 2.45e-04 for the indexes.
FLOAT32_DEVIATION_MU = 4.153e-06
FLOAT32_DEVIATION_INDEX = 6.116e-05
KERNEL_FACTOR = 4.0


def float32_deviation(shape):
    """(max |mu32 - mu64|, max |index32 - index64|) of the torch definition on the CPU."""
    y, psi, weights = context_ref.make_case(shape, NUM_SCALES)
    y_hat = checkerboard_ref.checkerboard_scan(y, psi, weights, NUM_SCALES)["y_hat"].astype(np.float32)
    out = {}
    for dtype in (torch.float32, torch.float64):
        params = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w).to(dtype) for w in weights], NUM_SCALES)
        out[dtype] = checkerboard_ops.checkerboard_parameters_reference(torch.from_numpy(y_hat).to(dtype),
                                                                        torch.from_numpy(psi).to(dtype), params)
    return tuple(float((a.double() - b).abs().max()) for a, b in zip(out[torch.float32], out[torch.float64]))


@pytest.fixture(scope="module")
def entropy_model():
    from compression_amd import distributions, entropy_models
    offset = math.log(0.11)
    factor = (math.log(256.0) - math.log(0.11)) / (NUM_SCALES - 1.0)
    return entropy_models.LocationScaleIndexedEntropyModel(
        distributions.NoisyNormal, NUM_SCALES, lambda i: torch.exp(offset + factor * i), coding_rank=2,
        compression=True)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    shape = request.param
    y, psi, weights = context_ref.make_case(shape, NUM_SCALES)
    params = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    scan = checkerboard_ops.checkerboard_scan(yd, pd, params)
    torch.cuda.synchronize()
    return dict(shape=shape, y=yd, psi=pd, weights=weights, params=params, scan=scan)


def test_scan_is_self_consistent_and_repeatable(case):
    scan, y = case["scan"], case["y"]
    assert scan.sym.dtype == torch.int32 and scan.idx.dtype == torch.int32
    assert all(t.shape == y.shape for t in scan)
    assert bool(torch.isfinite(scan.mu).all()) and bool(torch.isfinite(scan.index_float).all())
    rounded = torch.round(y - scan.mu)
    assert torch.equal(scan.sym, rounded.to(torch.int32))
    assert torch.equal(scan.y_hat, scan.sym.to(torch.float32) + scan.mu)
    from compression_amd.layers import functional
    assert torch.equal(scan.idx, functional.index_prepare(scan.index_float.contiguous(), NUM_SCALES))
    again = checkerboard_ops.checkerboard_scan(case["y"], case["psi"], case["params"])
    for a, b in zip(scan, again):
        assert torch.equal(a, b)


def test_compact_and_full_outputs_agree(case):
    """checkerboard_parameters (compact, no y) on the scan's y_hat returns the scan's parameters, pass by pass."""
    scan = case["scan"]
    b, hl, wl, m = case["y"].shape
    for pass_ in (0, 1):
        mu, index = checkerboard_ops.checkerboard_parameters(scan.y_hat, case["psi"], case["params"], pass_)
        n = checkerboard_ops.pass_positions(hl, wl, pass_)
        assert tuple(mu.shape) == (b, n, m) and tuple(index.shape) == (b, n, m)
        assert torch.equal(mu, checkerboard_ops.checkerboard_split(scan.mu)[pass_])
        assert torch.equal(index, checkerboard_ops.checkerboard_split(scan.index_float)[pass_])
    # pass 0 reads no y_hat at all
    mu0, _ = checkerboard_ops.checkerboard_parameters(torch.full_like(scan.y_hat, 7.0), case["psi"], case["params"], 0)
    assert torch.equal(mu0, checkerboard_ops.checkerboard_split(scan.mu)[0])
    # place is the scan's store
    y_hat = torch.zeros_like(scan.y_hat)
    for pass_ in (0, 1):
        sym = checkerboard_ops.checkerboard_split(scan.sym)[pass_].to(torch.float32)
        checkerboard_ops.checkerboard_place(sym, checkerboard_ops.checkerboard_split(scan.mu)[pass_], y_hat, pass_)
    assert torch.equal(y_hat, scan.y_hat)


def test_an_image_alone_equals_its_slice_of_the_batch(case):
    scan = case["scan"]
    for k in range(case["shape"][0]):
        alone = checkerboard_ops.checkerboard_scan(case["y"][k:k + 1], case["psi"][k:k + 1], case["params"])
        for a, b in zip(alone, scan):
            assert torch.equal(a[0], b[k]), k


def test_scan_matches_the_float64_definition_teacher_forced(case):
    shape, scan = case["shape"], case["scan"]
    p64 = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w).double() for w in case["weights"]], NUM_SCALES)
    mu, index = checkerboard_ops.checkerboard_parameters_reference(scan.y_hat.cpu().double(), case["psi"].cpu().double(),
                                                                   p64)
    dev_mu = float((scan.mu.cpu().double() - mu).abs().max())
    dev_index = float((scan.index_float.cpu().double() - index).abs().max())
    print(f"shape {shape}: |mu - mu64| {dev_mu:.3e} (bound {KERNEL_FACTOR * FLOAT32_DEVIATION_MU:.3e}), "
          f"|index - index64| {dev_index:.3e} (bound {KERNEL_FACTOR * FLOAT32_DEVIATION_INDEX:.3e})")
    assert dev_mu <= KERNEL_FACTOR * FLOAT32_DEVIATION_MU
    assert dev_index <= KERNEL_FACTOR * FLOAT32_DEVIATION_INDEX


def _escapes(sym, idx, model):
    from compression_amd import synthetic
    rows = synthetic.lookup_rows(model.cdf.numpy())
    escape_at = np.array([len(cdf) - 2 for _, cdf in rows])
    value = sym.cpu().numpy() - model.cdf_offset.numpy()[idx.cpu().numpy()]
    return int(np.count_nonzero((value < 0) | (value >= escape_at[idx.cpu().numpy()])))


def test_inputs_take_the_escape_and_many_tables(case, entropy_model):
    scan = case["scan"]
    assert _escapes(scan.sym, scan.idx, entropy_model) >= 1
    assert int(torch.unique(scan.idx).numel()) >= 8


def _strings(model, y, scan):
    """[B, 2]: pass 0 and pass 1 of every image."""
    residual = checkerboard_ops.checkerboard_split((y - scan.mu).contiguous())
    index = checkerboard_ops.checkerboard_split(scan.index_float)
    return np.stack([np.asarray(model.compress(r, i), dtype=object).reshape(-1) for r, i in zip(residual, index)], axis=1)


def test_decode_inverts_the_entropy_models_strings(case, entropy_model):
    scan, shape = case["scan"], case["shape"]
    strings = _strings(entropy_model, case["y"], scan)
    assert strings.shape == (shape[0], 2)
    y_hat = checkerboard_ops.checkerboard_decode(strings, case["psi"], case["params"], entropy_model)
    assert torch.equal(y_hat, scan.y_hat)
    # the strings of one image taken out of the batched encode decode alone
    for k in range(shape[0]):
        alone = checkerboard_ops.checkerboard_decode(strings[k:k + 1], case["psi"][k:k + 1], case["params"], entropy_model)
        assert torch.equal(alone[0], scan.y_hat[k]), k
    with pytest.raises(ValueError, match="pass 0 and pass 1 of every image"):
        checkerboard_ops.checkerboard_decode(strings[:, :1], case["psi"], case["params"], entropy_model)


def test_decode_really_decodes(case, entropy_model):
    """Strings of another y (same psi, same weights) decode to that y's y_hat."""
    rng = np.random.Generator(np.random.PCG64(7))
    other = torch.from_numpy(rng.normal(0.0, 4.0, tuple(case["y"].shape)).astype(np.float32)).cuda()
    scan = checkerboard_ops.checkerboard_scan(other, case["psi"], case["params"])
    assert not torch.equal(scan.y_hat, case["scan"].y_hat)
    y_hat = checkerboard_ops.checkerboard_decode(_strings(entropy_model, other, scan), case["psi"], case["params"],
                                                 entropy_model)
    assert torch.equal(y_hat, scan.y_hat)


def test_a_single_position_has_no_second_pass():
    """The ops accept Hl Wl = 1 and launch nothing for the empty pass."""
    y, psi, weights = context_ref.make_case((2, 1, 1, 8, 26, 21), NUM_SCALES)
    params = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    scan = checkerboard_ops.checkerboard_scan(yd, pd, params)
    want = checkerboard_ops.checkerboard_scan_reference(yd.cpu().double(), pd.cpu().double(),
                                                        checkerboard_ops.CheckerboardParams(
                                                            *[torch.from_numpy(w).double() for w in weights], NUM_SCALES))
    assert float((scan.mu.cpu().double() - want.mu).abs().max()) <= KERNEL_FACTOR * FLOAT32_DEVIATION_MU
    mu1, index1 = checkerboard_ops.checkerboard_parameters(scan.y_hat, pd, params, 1)
    assert tuple(mu1.shape) == (2, 0, 8) and tuple(index1.shape) == (2, 0, 8)


def test_argument_errors_come_from_the_host_as_text(case):
    from compression_amd import _lib
    params, psi, y = case["params"], case["psi"], case["y"]
    b, hl, wl, m = y.shape
    lib = _lib.lib()
    packed = params.packed(psi.device)
    out = torch.empty(b, checkerboard_ops.pass_positions(hl, wl, 0), m, device=psi.device)
    common = (b, hl, wl, m, params.p, params.h1, params.h2, NUM_SCALES)
    rc = lib.tfc_checkerboard_params(0, None, y.data_ptr(), psi.data_ptr(), packed.data_ptr(), 3, *common,
                                     out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "packed weights" in _lib.last_error()
    rc = lib.tfc_checkerboard_params(2, None, y.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(), *common,
                                     out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "pass must be 0 or 1" in _lib.last_error()
    rc = lib.tfc_checkerboard_params(0, None, None, psi.data_ptr(), packed.data_ptr(), packed.numel(), *common,
                                     out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "must not be null" in _lib.last_error()
    rc = lib.tfc_checkerboard_params(0, y.data_ptr(), y.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(),
                                     *common, out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "sym must not be null" in _lib.last_error()
    rc = lib.tfc_checkerboard_params(0, None, None, None, None, packed.numel(), 0, hl, wl, m, params.p, params.h1,
                                     params.h2, NUM_SCALES, None, None, None, None, None)
    assert rc == 0                                                              # batch == 0 is a no-op
    rc = lib.tfc_checkerboard_place(0, None, out.data_ptr(), y.data_ptr(), b, hl, wl, m, None)
    assert rc != 0 and "must not be null" in _lib.last_error()
    with pytest.raises(ValueError, match="strings must have shape"):
        checkerboard_ops.checkerboard_decode([b"ab"], psi, params, None)
