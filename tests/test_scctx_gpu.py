"""GPU tier of the space-channel context model (csrc/space_channel.hip): scctx_scan against itself (exact, step by step
against the compact entry, image by image against the batched call), the single group against the checkerboard model's
ops and hand-written two-string format (bit for bit; both run these kernels, and test_context_digests_gpu.py pins them
to the former checkerboard kernel), the raw checkerboard entries against the raw one-group entries, against the float64
definition teacher-forced on its own y_hat, causality on the device, and scctx_decode against the strings the indexed
entropy model writes from the scan's outputs (bit-identical y_hat, also for one image taken out of a batched encode).

The teacher-forced bound.  FLOAT32_DEVIATION_MU / _INDEX are the largest deviations of the float32 torch evaluation of
`scctx_parameters_reference` from its float64 evaluation, measured on the CPU on these inputs (all SHAPES; y_hat of the
float64 scan, rounded to float32); the kernel gets 4x that, the project's margin for a different summation order and
FMA contraction.  `float32_deviation` below is the measurement."""
import math

import numpy as np
import pytest
import torch

import scctx_ref
from compression_amd.ops import checkerboard_ops, scctx_ops

pytestmark = pytest.mark.gpu

NUM_SCALES = 64
SHAPES = scctx_ref.GPU_SHAPES
# max |float32 - float64| over all SHAPES, measured on the CPU with `float32_deviation` (per shape, (mu, index_float):
# 4.1e-07 1.1e-05 | 9.9e-07 2.1e-05 | 1.2e-06 2.2e-05 | 8.1e-07 1.8e-05 | 2.1e-06 4.2e-05 | 1.6e-06 3.6e-05 |
# 1.7e-06 3.4e-05 | 2.8e-06 5.1e-05 | 3.3e-06 7.4e-05; the means are of order 1, the indexes of order 64).  The
# kernel's bounds are 4x: 1.34e-05 for mu, 2.95e-04 for the indexes.
FLOAT32_DEVIATION_MU = 3.342e-06
FLOAT32_DEVIATION_INDEX = 7.378e-05
KERNEL_FACTOR = 4.0


def params_of(weights, dtype=torch.float32, stream_positions=64):
    groups = [tuple(None if w is None else torch.from_numpy(np.asarray(w)).to(dtype) for w in group) for group in weights]
    return scctx_ops.SpaceChannelParams(groups, NUM_SCALES, stream_positions)


def float32_deviation(shape):
    """(max |mu32 - mu64|, max |index32 - index64|) of the torch definition on the CPU."""
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    y_hat = scctx_ref.scctx_scan(y, psi, weights, NUM_SCALES)["y_hat"].astype(np.float32)
    out = {}
    for dtype in (torch.float32, torch.float64):
        out[dtype] = scctx_ops.scctx_parameters_reference(torch.from_numpy(y_hat).to(dtype),
                                                          torch.from_numpy(psi).to(dtype), params_of(weights, dtype))
    return tuple(float((a.double() - b).abs().max()) for a, b in zip(out[torch.float32], out[torch.float64]))


@pytest.fixture(scope="module")
def entropy_model():
    from compression_amd import distributions, entropy_models
    offset = math.log(0.11)
    factor = (math.log(256.0) - math.log(0.11)) / (NUM_SCALES - 1.0)
    return entropy_models.LocationScaleIndexedEntropyModel(
        distributions.NoisyNormal, NUM_SCALES, lambda i: torch.exp(offset + factor * i), coding_rank=2,
        compression=True)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + "-" + "_".join(map(str, s[3])))
def case(request):
    shape = request.param
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    params = params_of(weights, stream_positions=shape[4])
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    scan = scctx_ops.scctx_scan(yd, pd, params)
    torch.cuda.synchronize()
    return dict(shape=shape, y=yd, psi=pd, weights=weights, params=params, scan=scan)


def test_scan_is_self_consistent_and_repeatable(case):
    scan, y = case["scan"], case["y"]
    assert scan.sym.dtype == torch.int32 and scan.idx.dtype == torch.int32
    assert all(t.shape == y.shape for t in scan)
    assert bool(torch.isfinite(scan.mu).all()) and bool(torch.isfinite(scan.index_float).all())
    assert torch.equal(scan.sym, torch.round(y - scan.mu).to(torch.int32))
    assert torch.equal(scan.y_hat, scan.sym.to(torch.float32) + scan.mu)
    from compression_amd.layers import functional
    assert torch.equal(scan.idx, functional.index_prepare(scan.index_float.contiguous(), NUM_SCALES))
    again = scctx_ops.scctx_scan(case["y"], case["psi"], case["params"])
    for a, b in zip(scan, again):
        assert torch.equal(a, b)


def test_compact_steps_and_full_outputs_agree(case):
    """scctx_parameters (compact, no y) on the scan's y_hat returns the scan's parameters, step by step."""
    scan, params = case["scan"], case["params"]
    b, hl, wl, m = case["y"].shape
    split = checkerboard_ops.checkerboard_split
    y_hat = torch.zeros_like(scan.y_hat)
    for g, (c, mg) in enumerate(zip(params.offsets, params.groups)):
        for pass_ in (0, 1):
            mu, index = scctx_ops.scctx_parameters(scan.y_hat, case["psi"], params, g, pass_)
            n = checkerboard_ops.pass_positions(hl, wl, pass_)
            assert tuple(mu.shape) == (b, n, mg) and tuple(index.shape) == (b, n, mg)
            assert torch.equal(mu, split(scan.mu[..., c:c + mg])[pass_])
            assert torch.equal(index, split(scan.index_float[..., c:c + mg])[pass_])
            # place is the scan's store
            scctx_ops.scctx_place(split(scan.sym[..., c:c + mg])[pass_].to(torch.float32), mu, y_hat, c, pass_)
    assert torch.equal(y_hat, scan.y_hat)


def test_an_image_alone_equals_its_slice_of_the_batch(case):
    scan = case["scan"]
    for k in range(case["shape"][0]):
        alone = scctx_ops.scctx_scan(case["y"][k:k + 1], case["psi"][k:k + 1], case["params"])
        for a, b in zip(alone, scan):
            assert torch.equal(a[0], b[k]), k


def _checker_strings(model, y, scan):
    """[B, 2]: pass 0 and pass 1 of every image, the checkerboard model's format."""
    residual = checkerboard_ops.checkerboard_split((y - scan.mu).contiguous())
    index = checkerboard_ops.checkerboard_split(scan.index_float)
    return np.stack([np.asarray(model.compress(r, i), dtype=object).reshape(-1) for r, i in zip(residual, index)], axis=1)


@pytest.fixture(scope="module")
def single(request):
    """The case of the one shape that has a single group."""
    (shape,) = [s for s in SHAPES if len(s[3]) == 1]
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    params = params_of(weights, stream_positions=shape[4])
    yd, pd = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    return dict(shape=shape, y=yd, psi=pd, weights=weights, params=params, scan=scctx_ops.scctx_scan(yd, pd, params))


def test_one_group_is_the_checkerboard_kernel_bit_for_bit(single, entropy_model):
    case = single
    checker = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in case["weights"][0][1:]], NUM_SCALES)
    want = checkerboard_ops.checkerboard_scan(case["y"], case["psi"], checker)
    for name, a, b in zip(want._fields, case["scan"], want):
        assert torch.equal(a, b), name
    b, hl, wl, _ = case["y"].shape
    assert case["params"].stream_positions >= checkerboard_ops.pass_positions(hl, wl, 0)
    strings = scctx_ops.scctx_encode(case["y"], case["scan"], case["params"], entropy_model)
    want_strings = _checker_strings(entropy_model, case["y"], want)
    assert strings.shape == want_strings.shape == (b, 2)
    assert [bytes(s) for s in strings.reshape(-1)] == [bytes(s) for s in want_strings.reshape(-1)]


@pytest.mark.parametrize("shape", [(1, 1, 2, 8, 26, 21), (2, 9, 15, 8, 26, 21)], ids=lambda s: "x".join(map(str, s[:4])))
def test_the_checkerboard_entries_are_the_one_group_entries(shape):
    """Raw tfc_checkerboard_params / _place against raw tfc_scctx_params / _place with c_g = 0 and M_g = M on the same
    buffers: both passes, with and without y, every output."""
    import context_ref
    from compression_amd import _lib
    lib = _lib.lib()
    y, psi, weights = context_ref.make_case(shape, NUM_SCALES)
    own = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
    y, psi = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
    b, hl, wl, m = y.shape
    packed = own.packed(y.device)
    sizes = (own.p, own.h1, own.h2, NUM_SCALES)

    def run(entry, group, pass_, y_in, y_hat):
        n = checkerboard_ops.pass_positions(hl, wl, pass_)
        mu, index = torch.zeros(b, n, m, device=y.device), torch.zeros(b, n, m, device=y.device)
        idx = torch.zeros(b, n, m, dtype=torch.int32, device=y.device)
        sym = torch.zeros_like(idx)
        _lib.check(entry(pass_, None if y_in is None else y_in.data_ptr(), y_hat.data_ptr(), psi.data_ptr(),
                         packed.data_ptr(), packed.numel(), b, hl, wl, m, *group, *sizes, mu.data_ptr(), index.data_ptr(),
                         idx.data_ptr(), None if y_in is None else sym.data_ptr(), None))
        return mu, index, idx, sym

    def chain(params_entry, place_entry, group):
        """The encoder's two passes, then the decoder's: parameters without y and the store, pass after pass."""
        out, y_hat = [], torch.zeros_like(y)
        for pass_ in (0, 1):
            out += run(params_entry, group, pass_, y, y_hat)
        decoded = torch.zeros_like(y)
        for pass_ in (0, 1):
            mu, index, idx, _ = run(params_entry, group, pass_, None, decoded)
            sym = out[4 * pass_ + 3].to(torch.float32)
            _lib.check(place_entry(pass_, sym.data_ptr(), mu.data_ptr(), decoded.data_ptr(), b, hl, wl, m, *group, None))
            out += [mu, index, idx, decoded.clone()]
        torch.cuda.synchronize()
        return out + [y_hat]

    checker = chain(lib.tfc_checkerboard_params, lib.tfc_checkerboard_place, ())
    group = chain(lib.tfc_scctx_params, lib.tfc_scctx_place, (0, m))
    assert len(checker) == len(group) == 17
    for k, (a, g) in enumerate(zip(checker, group)):
        assert torch.equal(a, g), k
    assert torch.equal(checker[-1], checker[-2])                # the decoder's y_hat is the encoder's
    assert bool(checker[-1].abs().sum() > 0)


def test_scan_matches_the_float64_definition_teacher_forced(case):
    shape, scan = case["shape"], case["scan"]
    mu, index = scctx_ops.scctx_parameters_reference(scan.y_hat.cpu().double(), case["psi"].cpu().double(),
                                                     params_of(case["weights"], torch.float64))
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


def test_decode_inverts_the_entropy_models_strings(case, entropy_model):
    scan, shape, params = case["scan"], case["shape"], case["params"]
    b, hl, wl, groups, sp = shape
    strings = scctx_ops.scctx_encode(case["y"], scan, params, entropy_model)
    total = scctx_ref.stream_total(hl, wl, groups, sp)
    assert strings.shape == (b, total) and total == len(groups) * sum(scctx_ops.stream_counts(hl, wl, sp))
    y_hat = scctx_ops.scctx_decode(strings, case["psi"], params, entropy_model)
    assert torch.equal(y_hat, scan.y_hat)
    # the strings of one image taken out of the batched encode decode alone
    for k in range(b):
        alone = scctx_ops.scctx_decode(strings[k:k + 1], case["psi"][k:k + 1], params, entropy_model)
        assert torch.equal(alone[0], scan.y_hat[k]), k
    with pytest.raises(ValueError, match=rf"strings must have shape \[{b}, {total}\]"):
        scctx_ops.scctx_decode(strings[:, :-1], case["psi"], params, entropy_model)


def test_a_stream_is_what_the_entropy_model_writes_for_its_block(case, entropy_model):
    """The first and the last string of the last step, compressed on their own."""
    scan, params = case["scan"], case["params"]
    b, hl, wl, groups, sp = case["shape"]
    strings = scctx_ops.scctx_encode(case["y"], scan, params, entropy_model)
    c, mg = params.offsets[-1], params.groups[-1]
    residual = checkerboard_ops.checkerboard_split((case["y"] - scan.mu)[..., c:c + mg].contiguous())[1]
    index = checkerboard_ops.checkerboard_split(scan.index_float[..., c:c + mg].contiguous())[1]
    s1 = scctx_ops.stream_counts(hl, wl, sp)[1]
    for s in {0, s1 - 1}:
        block = slice(s * sp, min((s + 1) * sp, residual.shape[1]))
        alone = entropy_model.compress(residual[:, block].contiguous(), index[:, block].contiguous())
        got = strings[:, strings.shape[1] - s1 + s]
        assert [bytes(v) for v in np.asarray(alone, dtype=object).reshape(-1)] == [bytes(v) for v in got], s


def test_decode_really_decodes(case, entropy_model):
    """Strings of another y (same psi, same weights) decode to that y's y_hat."""
    rng = np.random.Generator(np.random.PCG64(7))
    other = torch.from_numpy(rng.normal(0.0, 4.0, tuple(case["y"].shape)).astype(np.float32)).cuda()
    scan = scctx_ops.scctx_scan(other, case["psi"], case["params"])
    assert not torch.equal(scan.y_hat, case["scan"].y_hat)
    strings = scctx_ops.scctx_encode(other, scan, case["params"], entropy_model)
    assert torch.equal(scctx_ops.scctx_decode(strings, case["psi"], case["params"], entropy_model), scan.y_hat)


def test_later_steps_do_not_reach_earlier_ones_on_the_device(case):
    scan, params, y, psi = case["scan"], case["params"], case["y"], case["psi"]
    hl, wl = y.shape[1:3]
    anchors = checkerboard_ops.anchor_mask(hl, wl, device=y.device)
    for g, (c, mg) in enumerate(zip(params.offsets, params.groups)):
        changed = y.clone()
        changed[..., c:] += 3.0
        other = scctx_ops.scctx_scan(changed, psi, params)
        for name in ("mu", "index_float"):
            a, b = getattr(other, name), getattr(scan, name)
            assert torch.equal(a[..., :c], b[..., :c]), (g, name)
            assert torch.equal(a[:, anchors, c:c + mg], b[:, anchors, c:c + mg]), (g, name)
        changed = y.clone()
        changed[:, ~anchors, c:c + mg] += 3.0
        other = scctx_ops.scctx_scan(changed, psi, params)
        for name in ("mu", "index_float"):
            a, b = getattr(other, name), getattr(scan, name)
            assert torch.equal(a[..., :c + mg], b[..., :c + mg]), (g, name)


def test_argument_errors_come_from_the_host_as_text(case):
    from compression_amd import _lib
    params, psi, y = case["params"], case["psi"], case["y"]
    b, hl, wl, m = y.shape
    g = len(params) - 1
    own, c = params.own[g], params.offsets[g]
    lib = _lib.lib()
    packed = params.packed(g, psi.device)
    out = torch.empty(b, checkerboard_ops.pass_positions(hl, wl, 0), own.m, device=psi.device)
    common = (b, hl, wl, m, c, own.m, own.p, own.h1, own.h2, NUM_SCALES)
    rc = lib.tfc_scctx_params(0, None, y.data_ptr(), psi.data_ptr(), packed.data_ptr(), 3, *common, out.data_ptr(),
                              out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "packed weights" in _lib.last_error()
    rc = lib.tfc_scctx_params(2, None, y.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(), *common,
                              out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "pass must be 0 or 1" in _lib.last_error()
    rc = lib.tfc_scctx_params(0, None, None, psi.data_ptr(), packed.data_ptr(), packed.numel(), *common, out.data_ptr(),
                              out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "must not be null" in _lib.last_error()
    rc = lib.tfc_scctx_params(0, y.data_ptr(), y.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(), *common,
                              out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert rc != 0 and "sym must not be null" in _lib.last_error()
    rc = lib.tfc_scctx_params(0, None, None, None, None, packed.numel(), 0, *common[1:], None, None, None, None, None)
    assert rc == 0                                                              # batch == 0 is a no-op
    rc = lib.tfc_scctx_place(0, None, out.data_ptr(), y.data_ptr(), b, hl, wl, m, c, own.m, None)
    assert rc != 0 and "must not be null" in _lib.last_error()
    with pytest.raises(ValueError, match="strings must have shape"):
        scctx_ops.scctx_decode([b"ab"], psi, params, None)
