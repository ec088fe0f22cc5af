"""GPU tier of the context model (csrc/context_model.hip): context_scan against itself (exact), against the float64
definition teacher-forced on its own y_hat (one step's rounding), and context_decode against the strings the indexed
entropy model writes from the scan's outputs (bit-identical y_hat).

The teacher-forced bound.  FLOAT32_DEVIATION_MU / _INDEX are the largest deviations of the float32 torch evaluation of
`context_parameters_reference` from its float64 evaluation, measured on the CPU on these inputs (all SHAPES; y_hat of
the float64 scan, rounded to float32); the kernel gets 4x that, for its different summation order and
FMA contraction.  `float32_deviation` below is the measurement."""
import math

import numpy as np
import pytest
import torch

import context_ref
from compression_amd.ops import context_ops

pytestmark = pytest.mark.gpu

NUM_SCALES = 64
SHAPES = context_ref.GPU_SHAPES
# max |float32 - float64| over all SHAPES, measured on the CPU with `float32_deviation` (per shape, (mu, index_float):
# 2.0e-07 5.2e-06 | 4.1e-07 1.7e-05 | 1.2e-06 1.5e-05 | 9.3e-07 2.9e-05 | 1.2e-06 2.9e-05 | 2.9e-06 7.3e-05; the means
# are of order 1, the indexes of order 64).  The kernel's bounds are 4x: 1.16e-05 for mu, 2.93e-04 for the indexes.
FLOAT32_DEVIATION_MU = 2.891e-06
FLOAT32_DEVIATION_INDEX = 7.312e-05
KERNEL_FACTOR = 4.0


def float32_deviation(shape):
    """(max |mu32 - mu64|, max |index32 - index64|) of the torch definition on the CPU."""
    y, psi, weights = context_ref.make_case(shape, NUM_SCALES)
    y_hat = context_ref.context_scan(y, psi, weights, NUM_SCALES)["y_hat"].astype(np.float32)
    out = {}
    for dtype in (torch.float32, torch.float64):
        params = context_ops.ContextParams(*[torch.from_numpy(w).to(dtype) for w in weights], NUM_SCALES)
        out[dtype] = context_ops.context_parameters_reference(torch.from_numpy(y_hat).to(dtype),
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
    params = context_ops.ContextParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    scan = context_ops.context_scan(yd, pd, params)
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
    again = context_ops.context_scan(case["y"], case["psi"], case["params"])
    for a, b in zip(scan, again):
        assert torch.equal(a, b)


def test_scan_matches_the_float64_definition_teacher_forced(case):
    shape, scan = case["shape"], case["scan"]
    p64 = context_ops.ContextParams(*[torch.from_numpy(w).double() for w in case["weights"]], NUM_SCALES)
    mu, index = context_ops.context_parameters_reference(scan.y_hat.cpu().double(), case["psi"].cpu().double(), p64)
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
    return model.compress((y - scan.mu).contiguous(), scan.index_float.contiguous())


def test_decode_inverts_the_entropy_models_strings(case, entropy_model):
    scan, shape = case["scan"], case["shape"]
    strings = _strings(entropy_model, case["y"], scan)
    assert strings.shape == shape[:2]
    y_hat, ok = context_ops.context_decode(strings, case["psi"], case["params"], entropy_model.cdf,
                                           entropy_model.cdf_offset)
    assert ok.shape == shape[:2] and bool(ok.all())
    assert torch.equal(y_hat, scan.y_hat)
    # the strings are what the model's own decoder inverts with the scan's parameters, too
    plain = entropy_model.decompress(strings, scan.index_float.contiguous())
    assert torch.equal(plain + scan.mu, scan.y_hat)


def test_decode_really_decodes(case, entropy_model):
    """Strings of another y (same psi, same weights) decode to that y's y_hat."""
    rng = np.random.Generator(np.random.PCG64(7))
    other = torch.from_numpy(rng.normal(0.0, 4.0, tuple(case["y"].shape)).astype(np.float32)).cuda()
    scan = context_ops.context_scan(other, case["psi"], case["params"])
    assert not torch.equal(scan.y_hat, case["scan"].y_hat)
    y_hat, ok = context_ops.context_decode(_strings(entropy_model, other, scan), case["psi"], case["params"],
                                           entropy_model.cdf, entropy_model.cdf_offset)
    assert bool(ok.all()) and torch.equal(y_hat, scan.y_hat)


def test_argument_errors_come_from_the_host_as_text(case, entropy_model):
    from compression_amd import _lib
    params, psi = case["params"], case["psi"]
    b, hl, wl, m = case["y"].shape
    lib = _lib.lib()
    assert lib.tfc_context_workspace(b, hl, wl, m, params.p, params.h1, params.h2) >= 16 * b * hl
    assert lib.tfc_context_workspace(b, hl, wl, 0, params.p, params.h1, params.h2) == -1
    assert "at least 1" in _lib.last_error()
    assert lib.tfc_context_workspace(b, hl, wl, m, params.p, 40000, params.h2) == -1
    assert "do not fit" in _lib.last_error()
    with pytest.raises(ValueError, match="one per latent row"):
        context_ops.context_decode([b"ab"], psi, params, entropy_model.cdf, entropy_model.cdf_offset)
    rc = lib.tfc_context_scan(None, psi.data_ptr(), params.packed(psi.device).data_ptr(), 3, b, hl, wl, m, params.p,
                              params.h1, params.h2, NUM_SCALES, None, None, None, None, None, None, None)
    assert rc != 0 and "packed weights" in _lib.last_error()
