"""GPU tier: csrc/factorized_bits.hip and csrc/noisy_normal_bits.hip against the float64 definition of
tests/bits_ref.py, element by element.  No mask: every element of every output is compared and must be finite.

Tolerance.  |error_i| <= A 2^-24 norm_i, where norm_i follows the conditioning of the formula
(forward, factorized: (1 + |up| + |lo|) / (1 - exp(-|up - lo|)) + |log p|; normal: 1 + zu^2 + zl^2 over
1 - exp(-|big - small|); gradients: the same bracket times the gross size of the terms before they cancel,
bits_ref._eval).  A is not fixed in advance: A_ref is the smallest A at which the float32 HOST evaluation of
bits_ref's own functions passes on the same inputs, and the kernel must pass with 4 A_ref (hardware exp / log /
rcp are 1-2 ulp where libm is below 1, and the MLP's fma order differs).  A wrong term, a missing gate or the
wrong side of the median moves log p by orders of magnitude more.  bfloat16: y_hat is the bf16 rounding of the
float32 sum, the definition is evaluated at that y_hat, and dy gets one bf16 ulp on top.  Unit sums: within the
sum of the elements' tolerances.  Every gradient (dy, dscale, each raw-parameter tensor) is held to 4 x its OWN
A_ref; the one exception, a scalar scale (a single number summed over every element), is explained where it is
made, bits_ref.reference.  Each case prints A_ref and the kernel's own smallest passing A
(profiles/bits_numerics.md is that table)."""
import pytest
import torch

import bits_ref
import compression_amd as tfc
from compression_amd import _lib
from compression_amd.ops import bottleneck_ops

pytestmark = pytest.mark.gpu
_CODE = {torch.float32: 0, torch.bfloat16: 1}


def _base(case, inp):
    base = tfc.DeepFactorized(batch_shape=(case.C,), num_filters=case.num_filters, init_scale=case.init_scale).cuda()
    raw = [t for g in inp["params"] for t in g]
    with torch.no_grad():
        for dst, src in zip(list(base.matrices) + list(base.biases) + list(base.factors), raw):
            dst.copy_(src)
    return base


def _leaves(base):
    return list(base.matrices) + list(base.biases) + list(base.factors)


def _factorized_log_prob(case, inp, base):
    """The per-element log_prob output of the C entry (the Python wrapper never asks for it)."""
    params = bottleneck_ops.pack_factorized_params(base).detach()
    y = inp["y"].cuda().contiguous()
    noise = inp["noise"].cuda().contiguous() if inp["noise"] is not None else None
    units = int(torch.Size(case.lead).numel())
    elems = y.numel() // units
    y_hat = torch.empty_like(y)
    lp = torch.full(case.shape, float("nan"), device="cuda")
    bits = torch.full((units,), float("nan"), device="cuda")
    head = (y.data_ptr(), noise.data_ptr() if noise is not None else None, y_hat.data_ptr(), _CODE[y.dtype], units,
            elems, case.C, params.data_ptr(), len(case.num_filters) + 1, case.num_filters[0])
    if case.tail_mass:
        _lib.check(_lib.lib().tfc_factorized_bits_forward_tail(*head, case.tail_mass, lp.data_ptr(), bits.data_ptr(),
                                                               _lib.stream_ptr()))
    else:
        _lib.check(_lib.lib().tfc_factorized_bits_forward(*head, lp.data_ptr(), bits.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return y_hat, lp, bits


def _normal_log_prob(case, inp):
    """One coding unit per element: bits of the unit IS the element's log p."""
    v = inp["v"].cuda().reshape(-1, 1)
    s = torch.broadcast_to(inp["scale"], case.shape).cuda().reshape(-1, 1)
    _, bits = bottleneck_ops.noisy_normal_bits(v, s, 1, None, laplace_tail_mass=case.tail_mass)
    return (bits.double() * -bits_ref.LN2).reshape(case.shape)


def _check(case):
    ref = bits_ref.reference(case)
    inp, want, a_ref = ref["inputs"], ref["f64"], ref["A_ref"]
    margin = bits_ref.MARGIN
    y = inp["y"].cuda()
    if case.strided:
        y = y.transpose(1, 2).contiguous().transpose(1, 2)
        assert not y.is_contiguous()
    y.requires_grad_(True)
    noise = inp["noise"].cuda() if inp["noise"] is not None else None
    if case.prior == "factorized":
        base = _base(case, inp)
        leaves = _leaves(base)
        y_hat, bits = bottleneck_ops.factorized_bits(y, base, case.coding_rank, noise, expected_grads=case.expected,
                                                     laplace_tail_mass=case.tail_mass)
    else:
        leaves = [inp["scale"].cuda().requires_grad_(True)]
        y_hat, bits = bottleneck_ops.noisy_normal_bits(y, leaves[0], case.coding_rank, noise,
                                                       expected_grads=case.expected, laplace_tail_mass=case.tail_mass)
    loss = 0
    if case.loss in ("both", "bits"):
        loss = loss + (bits * inp["w"].cuda()).sum()
    if case.loss in ("both", "y_hat"):
        loss = loss + 1e-3 * (y_hat.float() ** 2).sum()
    loss.backward()
    torch.cuda.synchronize()

    # the perturbed tensor: the dtype's rounding of the float32 sum, exactly
    assert y_hat.dtype == case.torch_dtype and torch.equal(y_hat.detach().cpu(), inp["v"])

    # per-element log p
    if case.prior == "factorized":
        y_hat2, lp, bits2 = _factorized_log_prob(case, inp, base)
        assert torch.equal(y_hat2.cpu(), inp["v"]) and torch.equal(bits2, bits.detach().reshape(-1))
    else:
        lp = _normal_log_prob(case, inp)
    assert bool(torch.isfinite(lp).all())
    a_lp = bits_ref.smallest_a(lp, want["lp"], want["bracket"])

    # unit sums
    tol = (margin * a_ref["lp"] * bits_ref.EPS32 / bits_ref.LN2) * want["bracket"].sum(
        dim=tuple(range(-case.coding_rank, 0)))
    err_bits = (bits.detach().double().cpu() - want["bits"]).abs()
    assert bool(torch.isfinite(bits).all())

    # gradients
    dy = y.grad
    assert dy is not None and dy.dtype == case.torch_dtype and bool(torch.isfinite(dy.float()).all())
    extra = bits_ref.BF16_ULP * want["dy"].abs() if case.dtype == "bf16" else None
    a_dy = bits_ref.smallest_a(dy, want["dy"], want["n_dy"], extra)
    a_leaves = []
    for leaf, w64, n64 in zip(leaves, want["dleaves"], want["n_dleaves"]):
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert bool(torch.isfinite(g).all())
        a_leaves.append(bits_ref.smallest_a(g, w64, n64))

    worst_leaf = max(range(len(a_leaves)), key=lambda j: a_leaves[j] / max(a_ref["dleaves"][j], 1e-30))
    print("\nBITS_LEAVES", case.name, " ".join(f"{o:.3g}/{r:.3g}/{k:.3g}" for o, r, k in zip(a_ref["dleaves_own"], a_ref["dleaves"], a_leaves)))
    print(f"BITS_NUMERICS | {case.name} | {a_ref['lp']:.3g} | {a_lp:.3g} | {a_ref['dy']:.3g} | {a_dy:.3g} | "
          f"{a_ref['dleaves'][worst_leaf]:.3g} | {a_leaves[worst_leaf]:.3g} | "
          f"{float((err_bits / tol.clamp(min=1e-300)).max()) if tol.numel() else 0:.3g} |")
    assert a_lp <= margin * a_ref["lp"], ("log p", a_lp, a_ref["lp"], bits_ref.worst_element(lp, want["lp"], want["bracket"]))
    assert bool((err_bits <= tol).all()), ("bits", err_bits.max(), tol.min())
    assert a_dy <= margin * a_ref["dy"], ("dy", a_dy, a_ref["dy"], bits_ref.worst_element(dy, want["dy"], want["n_dy"], extra))
    for j, (got, env) in enumerate(zip(a_leaves, a_ref["dleaves"])):
        assert got <= margin * env, ("parameter gradient", j, got, env,
                                     bits_ref.worst_element(leaves[j].grad, want["dleaves"][j], want["n_dleaves"][j]))


@pytest.mark.parametrize("case", bits_ref.factorized_matrix_cases(), ids=lambda c: c.name)
def test_factorized_build_by_mode(case):
    """3 builds x 2 dtypes x 4 modes at C = 48, near and far inputs.  The far plain / expected cases are the ones
    whose logits pass +-90: sigmoid(u) sigmoid(-u) / P in probability space is 0 * inf there."""
    _check(case)


@pytest.mark.parametrize("case", bits_ref.factorized_plan_cases(), ids=lambda c: c.name)
def test_factorized_block_plan(case):
    """C in {1, 3, 65, 128, 150, 192, 220, 257, 320, 512}: blocks of 256, 255, 195, 256, 300, 192, 220, 257, 320, 512
    threads; above 256 the MAXT = 512 build (up to 112 KiB of dynamic LDS with (5, 5))."""
    _check(case)


@pytest.mark.parametrize("case", bits_ref.geometry_cases(), ids=lambda c: c.name)
def test_unit_geometry(case):
    _check(case)


@pytest.mark.parametrize("case", bits_ref.call_shape_cases(), ids=lambda c: c.name)
def test_call_shapes(case):
    """noise=None, a non-contiguous bottleneck, and losses that use only bits, only y_hat, or both."""
    _check(case)


@pytest.mark.parametrize("case", bits_ref.normal_matrix_cases(), ids=lambda c: c.name)
def test_noisy_normal_matrix(case):
    _check(case)


# ------------------------------------------------------------------------------------------------ empty units
def _nan(n):
    return torch.full((max(n, 1),), float("nan"), device="cuda")


def test_empty_coding_units_cost_zero_bits_c_entries():
    """units > 0, elems == 0: bits == 0 (the definition sums an empty unit to 0); the buffer starts as NaN."""
    lib = _lib.lib()
    base = tfc.DeepFactorized(batch_shape=(48,)).cuda()
    params = bottleneck_ops.pack_factorized_params(base).detach()
    one = torch.zeros(1, device="cuda")
    for dtype in (torch.float32, torch.bfloat16):
        buf = one.to(dtype)
        for tail in (0.0, 1e-3):
            bits = _nan(5)
            head = (buf.data_ptr(), None, buf.data_ptr(), _CODE[dtype], 5, 0, 48, params.data_ptr(), 3, 3)
            if tail:
                _lib.check(lib.tfc_factorized_bits_forward_tail(*head, tail, None, bits.data_ptr(), _lib.stream_ptr()))
            else:
                _lib.check(lib.tfc_factorized_bits_forward(*head, None, bits.data_ptr(), _lib.stream_ptr()))
            assert torch.equal(bits.cpu(), torch.zeros(5)), (dtype, tail)
            bits = _nan(5)
            head = (buf.data_ptr(), None, one.data_ptr(), buf.data_ptr(), _CODE[dtype], 5, 0)
            if tail:
                _lib.check(lib.tfc_noisy_normal_bits_forward_tail(*head, tail, bits.data_ptr(), _lib.stream_ptr()))
            else:
                _lib.check(lib.tfc_noisy_normal_bits_forward(*head, bits.data_ptr(), _lib.stream_ptr()))
            assert torch.equal(bits.cpu().abs(), torch.zeros(5)), (dtype, tail)
    # units == 0: returns, touches nothing
    bits = _nan(1)
    _lib.check(lib.tfc_factorized_bits_forward(one.data_ptr(), None, one.data_ptr(), 0, 0, 48, 48, params.data_ptr(), 3, 3,
                                               None, bits.data_ptr(), _lib.stream_ptr()))
    _lib.check(lib.tfc_noisy_normal_bits_forward(one.data_ptr(), None, one.data_ptr(), one.data_ptr(), 0, 0, 48,
                                                 bits.data_ptr(), _lib.stream_ptr()))
    assert bool(torch.isnan(bits.cpu()).all())


@pytest.mark.parametrize("shape,rank", [((3, 0, 48), 2), ((0, 5, 48), 2), ((2, 3, 0, 48), 3)])
@pytest.mark.parametrize("tail", [0, 1e-3])
def test_empty_bottleneck_through_the_entropy_model(shape, rank, tail):
    prior = tfc.NoisyDeepFactorized(batch_shape=(48,)).cuda()
    em = tfc.ContinuousBatchedEntropyModel(prior, coding_rank=rank, compression=False, laplace_tail_mass=tail)
    y = torch.zeros(shape, device="cuda", requires_grad=True)
    y_hat, bits = em(y, training=True)
    assert y_hat.shape == y.shape and bits.shape == shape[:-rank]
    assert torch.equal(bits.detach().cpu(), torch.zeros(shape[:-rank]))
    (bits.sum() + y_hat.sum()).backward()
    assert y.grad.shape == y.shape
    assert all(p.grad is None or (bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) == 0)
               for p in prior.parameters())


def test_empty_bottleneck_noisy_normal():
    y = torch.zeros(3, 0, 8, device="cuda", requires_grad=True)
    scale = torch.ones(8, device="cuda", requires_grad=True)
    y_hat, bits = bottleneck_ops.noisy_normal_bits(y, scale, 2, torch.zeros_like(y))
    assert torch.equal(bits.detach().cpu().abs(), torch.zeros(3))
    (bits.sum() + y_hat.sum()).backward()
    assert float(scale.grad.abs().max()) == 0 and y.grad.shape == y.shape
