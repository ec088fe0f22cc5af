"""CPU tier: pins tests/gdn_ref.py, the definition the GDN kernels are held to in tests/test_gdn_loops_gpu.py.

* The hand-written float64 gradients are float64 autograd of the forward formula (1e-12 relative), every variant.
* The exact family's input sets really are exact: every value the definition produces on them is representable in
  float32 (in bfloat16 where the bfloat16 kernels store bfloat16 on the way to dbeta / dGamma), and every sum stays,
  in units of its smallest step, below 2^24 even if all its terms had the largest magnitude and one sign — so no
  summation order, in the kernels or in BLAS, can round.
* The twins' own errors against float64 are printed per variant (the GPU tier allows the kernels twice that)."""
import numpy as np
import pytest
import torch

import gdn_ref

PAIRS = [(False, 1), (False, 0.5), (True, 1), (True, 0.5)]
VARIANTS = [(inverse, rectify, alpha, eps) for inverse, eps in PAIRS for alpha in (1, 2) for rectify in (False, True)]
CUS = 256          # the MI355X; the GPU tier takes the count from the device and repeats the 2^24 bound for its size


def autograd64(x, g, beta, gamma, inverse, rectify, alpha, eps):
    x = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    gamma = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    xe = torch.relu(x) if rectify else x
    u = xe.abs() if alpha == 1 else xe * xe
    n = u @ gamma + beta
    y = xe * n ** eps if inverse else xe / n ** eps
    y.backward(torch.tensor(g, dtype=torch.float64))
    return y.detach().numpy(), x.grad.numpy(), beta.grad.numpy(), gamma.grad.numpy()


@pytest.mark.parametrize("inverse,rectify,alpha,eps", VARIANTS)
def test_float64_gradients_are_autograd_of_the_forward_formula(inverse, rectify, alpha, eps):
    C, pixels = 48, 131
    x, g = (t.double().numpy() for t in gdn_ref.random_inputs(pixels, C, 1, False))
    assert (x == 0).sum() > pixels * C // 32          # exact zeros: the subgradient and the closed rectifier
    beta, gamma = (t.double().numpy() for t in gdn_ref.params(C, 2))
    want = autograd64(x, g, beta, gamma, inverse, rectify, alpha, eps)
    got = gdn_ref.grads(x, g, beta, gamma, inverse, rectify, alpha, eps)
    assert np.array_equal(got["y"], gdn_ref.forward(x, beta, gamma, inverse, rectify, alpha, eps))
    for name, w in zip(("y", "dx", "dbeta", "dgamma"), want):
        err = np.max(np.abs(got[name] - w)) / np.max(np.abs(w))
        assert err <= 1e-12, (name, err)
    zero = (x <= 0) if rectify else np.zeros_like(x, bool)
    assert not got["dx"][zero].any()


def representable(a, dtype):
    t = torch.as_tensor(np.asarray(a, np.float64))
    return bool(torch.equal(t.to(dtype).double(), t))


def check_exact_set(pixels, C, seed, bf16):
    x, g, beta, gamma = gdn_ref.exact_inputs(pixels, C, seed)
    store = torch.bfloat16 if bf16 else torch.float32
    for t in (x, g, gamma):
        assert representable(t, store)
    vals = set(x.unique().tolist())
    assert vals <= {0.0, 1.0, -1.0, 2.0, -2.0} and set(g.unique().tolist()) <= {1.0, -1.0, 2.0, -2.0}
    if pixels * C >= 4096:
        assert 1 / 12 < float((x == 0).float().mean()) < 1 / 6 and bool((torch.signbit(x) & (x == 0)).any())
    for rectify, alpha in gdn_ref.EXACT_VARIANTS:
        r = gdn_ref.grads(x.numpy(), g.numpy(), beta.numpy(), gamma.numpy(), True, rectify, alpha, 1)
        assert representable(r["u"], store) and representable(r["T"], store)        # the matrix cores' operands
        assert representable(r["n"], torch.float32)
        assert representable(r["dbeta"], torch.float32) and representable(r["dgamma"], torch.float32)
        if not bf16:              # (bfloat16 rounds R = g n, y and dx when it stores them: not part of that family)
            for name in ("y", "R", "dx"):
                assert representable(r[name], torch.float32), name
        # Every sum, worst case, in units of its smallest step (u, T, g, x are integers; Gamma counts 2^-6):
        umax, tmax, gmax = np.abs(r["u"]).max(), np.abs(r["T"]).max(), float(gamma.max())
        assert pixels * umax * tmax < 2 ** 24                       # dGamma = U^T T   (step 1)
        assert pixels * tmax < 2 ** 24                              # dbeta = sum T    (step 1)
        assert (1 + C * umax * gmax) * 64 < 2 ** 24                 # n = 1 + U Gamma  (step 2^-6)
        assert C * tmax * gmax * 64 < 2 ** 24                       # T Gamma^T        (step 2^-6)
        assert np.abs(r["dx"]).max() * 64 < 2 ** 24 and np.abs(r["y"]).max() * 64 < 2 ** 24


@pytest.mark.parametrize("C", gdn_ref.EXACT_SMALL_CHANNELS)
@pytest.mark.parametrize("bf16", [False, True])
def test_exact_family_is_exact_at_the_small_sizes(C, bf16):
    for pixels in gdn_ref.EXACT_SMALL_PIXELS:
        check_exact_set(pixels, C, pixels, bf16)


@pytest.mark.parametrize("dtype,C", [(d, c) for d, cs in gdn_ref.EXACT_LOOP_CHANNELS.items() for c in cs])
def test_exact_family_is_exact_at_the_loop_size(dtype, C):
    check_exact_set(gdn_ref.p_loop(CUS), C, C, dtype == "bfloat16")


def test_loop_size_is_past_every_threshold():
    for cus in (64, 104, 256, 304):
        assert all(gdn_ref.p_loop(cus) > t for t in gdn_ref.loop_thresholds(cus).values())
        assert gdn_ref.p_loop(cus) % 32 and gdn_ref.p_loop(cus) % 64


@pytest.mark.parametrize("bf16", [False, True])
def test_twins_follow_the_definition(bf16):
    """The twins against float64, printed per variant; they are the same formulas, so float32 stays within 1e-5 and
    bfloat16 within a few bfloat16 steps (2^-8 each) in relative L2 — a gross bar: the figures are what matters."""
    C, pixels = 96, 2000
    x, g = gdn_ref.random_inputs(pixels, C, 3, bf16)
    beta, gamma = gdn_ref.params(C, 4)
    gam = gamma.bfloat16().float() if bf16 else gamma
    for inverse, rectify, alpha, eps in VARIANTS:
        want = gdn_ref.grads(x.numpy(), g.numpy(), beta.numpy(), gam.numpy(), inverse, rectify, alpha, eps)
        got = gdn_ref.twin(x, g, beta, gamma, inverse, rectify, alpha, eps, bf16=bf16)
        errs = {k: gdn_ref.rel_l2(got[k], want[k]) for k in ("y", "dx", "dbeta", "dgamma")}
        print(f"twin {'bf16' if bf16 else 'f32'} inverse={inverse} rectify={rectify} alpha={alpha} eps={eps}: "
              + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert all(v <= (2 ** -6 if bf16 else 1e-5) for v in errs.values()), errs
