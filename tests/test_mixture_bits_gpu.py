"""GPU tier of csrc/mixture_bits.hip against the float64 definition of tests/mixture_ref.py, element by element.

Tolerance.  |error_i| <= OPS 2^-24 n_i: n_i is the error scale of the formula at element i (mixture_ref.mixture_terms64
says how it follows from the operations), OPS = 32 the number of roundings one output collects (counted in
mixture_ref).  A wrong term, a wrong sign or the wrong side of the median moves a value by orders of magnitude more.
bfloat16: y_hat is the bf16 rounding of the float32 sum, the definition is evaluated at exactly that y_hat with the same
tolerance, and dy, itself stored as bf16, gets one bf16 ulp on top.  A unit's bits: within the sum of its elements'
tolerances.  The gradients get float32's underflow on top (mixture_ref: `u_*`): a component that is 2^-126 times less
likely than the element's best one has no responsibility left in float32.  Each case prints the smallest factor in place of OPS at which it would still pass."""
import pytest
import torch

import mixture_ref
from compression_amd.ops import bottleneck_ops, mixture_ops

pytestmark = pytest.mark.gpu

UNITS = 2
ELEMS = (1, 255, 256, 257, 773)          # the block-loop edges at 256 threads


def _inputs(elems, k, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + elems + 7 * k)
    lo, L = -6, 13
    logits, loc, scale = mixture_ref.random_parameters((UNITS, elems), k, lo, L, seed=seed + elems, sigma=(0.11, 5.0))
    y = (torch.randn(UNITS, elems, generator=g) * 6.0).to(dtype)
    noise = (torch.rand(UNITS, elems, generator=g) - 0.5).to(dtype)
    gbits = torch.tensor([0.75, -1.5])
    return y, noise, logits, loc, scale, gbits


def _smallest_factor(got, want, scale, extra=None):
    err = (got.detach().double().cpu() - want).abs()
    if extra is not None:
        err = (err - extra).clamp(min=0)
    return float((err / (mixture_ref.EPS32 * scale).clamp(min=1e-300)).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("elems", ELEMS)
def test_forward_and_backward_against_float64(elems, k, dtype):
    y, noise, logits, loc, scale, gbits = _inputs(elems, k, dtype)
    leaves = [t.cuda().requires_grad_(True) for t in (logits, loc, scale)]
    y_dev = y.cuda().requires_grad_(True)
    y_hat, bits = mixture_ops.mixture_bits(y_dev, *leaves, 1, noise=noise.cuda())
    (bits * gbits.cuda()).sum().backward()
    torch.cuda.synchronize()

    # the perturbed tensor: the dtype's rounding of the float32 sum, exactly
    v = (y.float() + noise.float()).to(dtype)
    assert y_hat.dtype == dtype and torch.equal(y_hat.detach().cpu(), v)
    want = mixture_ref.mixture_terms64(v, logits, loc, scale, gbits)

    # per-element log p: one coding unit per element
    _, each = mixture_ops.mixture_bits(v.cuda().reshape(-1, 1), *(t.detach().reshape(-1, 1, k) for t in leaves), 1)
    lp = (each.double().cpu() * -mixture_ref.LN2).reshape(UNITS, elems)
    assert bool(torch.isfinite(lp).all())
    factors = {"lp": _smallest_factor(lp, want["lp"], want["n_lp"])}

    tol_bits = mixture_ref.OPS * mixture_ref.EPS32 / mixture_ref.LN2 * want["n_lp"].sum(dim=1)
    err_bits = (bits.detach().double().cpu() - want["lp"].sum(dim=1) / -mixture_ref.LN2).abs()
    assert bits.shape == (UNITS,) and bool(torch.isfinite(bits).all())

    assert y_dev.grad.dtype == dtype
    extra = want["u_dy"] + (mixture_ref.BF16_ULP * want["dy"].abs() if dtype == torch.bfloat16 else 0)
    factors["dy"] = _smallest_factor(y_dev.grad, want["dy"], want["n_dy"], extra)
    for name, leaf in zip(("dlogits", "dloc", "dscale"), leaves):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()), name
        factors[name] = _smallest_factor(leaf.grad, want[name], want["n_" + name], want["u_" + name])
    print(f"\nMIXTURE_BITS elems={elems} K={k} {dtype}: " + " ".join(f"{n}={f:.3g}" for n, f in factors.items())
          + f" bits={float((err_bits / tol_bits).max()):.3g} (of {mixture_ref.OPS})")
    for name, f in factors.items():
        assert f <= mixture_ref.OPS, (name, f)
    assert bool((err_bits <= tol_bits).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_same_call_twice_is_bit_identical(dtype):
    y, noise, logits, loc, scale, gbits = _inputs(773, 3, dtype)
    runs = []
    for _ in range(2):
        leaves = [t.cuda().requires_grad_(True) for t in (logits, loc, scale)]
        y_dev = y.cuda().requires_grad_(True)
        y_hat, bits = mixture_ops.mixture_bits(y_dev, *leaves, 1, noise=noise.cuda())
        (bits * gbits.cuda()).sum().backward()
        runs.append([y_hat.detach(), bits.detach(), y_dev.grad] + [t.grad for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_component_is_the_single_gaussian_kernel():
    y, noise, logits, loc, scale, _ = _inputs(773, 1, torch.float32)
    y_hat, bits = mixture_ops.mixture_bits(y.cuda(), logits.cuda(), loc.cuda(), scale.cuda(), 1, noise=noise.cuda())
    # the single-Gaussian kernel takes the location subtracted: (y + u) - mu and (y - mu) + u differ by roundings of
    # |y| + |mu|, which move log p by |d log p / dy| times as much
    shifted = (y + noise).cuda() - loc.cuda()[..., 0]
    _, bits1 = bottleneck_ops.noisy_normal_bits(shifted, scale.cuda()[..., 0], 1)
    want = mixture_ref.mixture_terms64(y + noise, logits, loc, scale, torch.ones(UNITS))
    slack = (want["n_dy"] * mixture_ref.LN2 * (y.abs() + loc[..., 0].abs() + 1).double()).sum(dim=1)
    tol = (mixture_ref.OPS * mixture_ref.EPS32 / mixture_ref.LN2) * (2 * want["n_lp"].sum(dim=1) + slack)
    err = (bits.double().cpu() - bits1.double().cpu()).abs()
    print(f"\nMIXTURE_K1 difference {err.tolist()} of {tol.tolist()}")
    assert bool((err <= tol).all())
    assert torch.equal(y_hat.cpu(), y + noise)
