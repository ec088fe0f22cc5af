"""CPU tier: tests/bits_ref.py, the float64 definition the fused likelihood kernels are held to, pinned on its
own: against 60-digit arithmetic, against the package's float64 classes (written independently: two evaluations
that agree pin each other), by the PMF property, and, for every input set of tests/test_bits_kernels_gpu.py, that
the definition is finite everywhere and that each regime the GPU test claims to cover is really populated."""
import math

import mpmath
import pytest
import torch

import bits_ref
import compression_amd as tfc

mpmath.mp.dps = 60
CASES = bits_ref.all_cases()


# ------------------------------------------------------------------------------------------------ mpmath
def _mp_logits(x, params, c):
    mats, bias, fact = params
    h = [mpmath.mpf(x)]
    for i, (m, b) in enumerate(zip(mats, bias)):
        nxt = []
        for o in range(m.shape[1]):
            s = mpmath.mpf(float(b[c, o, 0]))
            for j in range(m.shape[2]):
                s += mpmath.log(1 + mpmath.exp(mpmath.mpf(float(m[c, o, j])))) * h[j]
            if i < len(fact):
                s += mpmath.tanh(mpmath.mpf(float(fact[i][c, o, 0]))) * mpmath.tanh(s)
            nxt.append(s)
        h = nxt
    return h[0]


def _mp_interval(cdf_up, cdf_lo, sf_up, sf_lo):
    # the same number either way; each difference keeps its digits on one side of the median only
    return sf_lo - sf_up if sf_up < cdf_up else cdf_up - cdf_lo


def _mp_sigmoid(t):
    return 1 / (1 + mpmath.exp(-t))


def _mp_laplace_cdf(t):
    return mpmath.exp(t) / 2 if t < 0 else 1 - mpmath.exp(-t) / 2


def _mp_tail(p, v, m):
    with mpmath.workdps(400):                      # the plain difference of two cumulatives, to any |v| used here
        q = +(_mp_laplace_cdf(mpmath.mpf(v) + 0.5) - _mp_laplace_cdf(mpmath.mpf(v) - 0.5))
    probs = (1 - mpmath.mpf(m)) * p + mpmath.mpf(m) * q
    return mpmath.log(m) + mpmath.log(q) if probs < mpmath.mpf("1e-10") else mpmath.log(probs)


def _rel(a, b):
    # relative; absolute below |log p| = 1e-6 (a box of scale 1e-3 has log p = -1e-54300 at its centre)
    return abs(a - b) / max(abs(b), mpmath.mpf(1e-6))


@pytest.mark.parametrize("num_filters,init_scale", [((3, 3), 10.0), ((3, 3, 3), 1.0), ((5, 5), 0.3)])
def test_factorized_definition_against_mpmath(num_filters, init_scale):
    C = 3
    params = bits_ref.factorized_raw_params(C, num_filters, init_scale, seed=3)
    p64 = [[t.double() for t in g] for g in params]
    xs = [0.0, 0.3, -0.7, 2.5, -4.0, 11.0, -23.0, 60.0, -150.0, 400.0, -700.0, 1500.0, -2e4]
    v = torch.tensor([[x * init_scale for _ in range(C)] for x in xs], dtype=torch.float64)
    lp, up, lo = bits_ref.factorized_parts(v, *p64)
    assert float(up.abs().max()) > 700 and float(lp.min()) < -1e4
    worst = 0
    for i in range(len(xs)):
        for c in range(C):
            x = float(v[i, c])
            u, l = _mp_logits(x + 0.5, params, c), _mp_logits(x - 0.5, params, c)
            assert _rel(mpmath.mpf(float(up[i, c])), u) < 1e-12
            p = _mp_interval(_mp_sigmoid(u), _mp_sigmoid(l), _mp_sigmoid(-u), _mp_sigmoid(-l))
            worst = max(worst, _rel(mpmath.mpf(float(lp[i, c])), mpmath.log(p)))
            for m in (1e-3,):
                got = bits_ref.laplace_tail(lp[i, c], v[i, c], m)
                worst = max(worst, _rel(mpmath.mpf(float(got)), _mp_tail(p, x, m)))
    print("factorized vs mpmath: worst relative", mpmath.nstr(worst, 3))
    assert worst < 1e-10


def test_normal_definition_against_mpmath():
    scales = [1e-3, 0.03, 0.7, 1.0, 9.0, 1e3]
    zs = [0.0, 0.2, -0.9, 1.0, -3.0, 7.5, -20.0, 38.0, -150.0, 300.0, -550.0]
    v = torch.tensor([[z * s for s in scales] for z in zs], dtype=torch.float64)
    v[3] = torch.round(v[3])                                 # integers
    s = torch.tensor(scales, dtype=torch.float64)
    lp = bits_ref.normal_log_prob(v, s)
    assert float(lp.min()) < -1e4
    worst = 0
    for i in range(len(zs)):
        for j in range(len(scales)):
            x, sc = mpmath.mpf(float(v[i, j])), mpmath.mpf(float(s[j]))
            zu, zl = (x + 0.5) / sc, (x - 0.5) / sc
            p = _mp_interval(mpmath.ncdf(zu), mpmath.ncdf(zl), mpmath.ncdf(-zu), mpmath.ncdf(-zl))
            worst = max(worst, _rel(mpmath.mpf(float(lp[i, j])), mpmath.log(p)))
            if abs(x) < 300:
                got = bits_ref.laplace_tail(lp[i, j], v[i, j], 1e-3)
                worst = max(worst, _rel(mpmath.mpf(float(got)), _mp_tail(p, x, 1e-3)))
    print("normal vs mpmath: worst relative", mpmath.nstr(worst, 3))
    assert worst < 1e-10


# ------------------------------------------------------------------------------------------------ the package
def _package_prior(case, inp):
    prior = tfc.NoisyDeepFactorized(batch_shape=(case.C,), num_filters=case.num_filters,
                                    init_scale=case.init_scale, dtype=torch.float64)
    with torch.no_grad():
        for dst, src in zip(list(prior.base.matrices) + list(prior.base.biases) + list(prior.base.factors),
                            [t for g in inp["params"] for t in g]):
            dst.copy_(src.double())
    return prior


@pytest.mark.parametrize("case", [c for c in bits_ref.factorized_matrix_cases() if c.dtype == "f32" and not c.expected],
                         ids=lambda c: c.name)
def test_factorized_definition_against_package_float64(case):
    """NoisyDeepFactorized(dtype=float64).log_prob and ContinuousBatchedEntropyModel._log_prob, over all three
    num_filters, near and far, with and without the tail."""
    inp = bits_ref.make_inputs(case)
    prior = _package_prior(case, inp)
    v = inp["v"].double()
    p64 = [[t.double() for t in g] for g in inp["params"]]
    mine = bits_ref.factorized_log_prob(v, *p64)
    with torch.no_grad():
        theirs = prior.log_prob(v)
        assert float((mine - theirs).abs().max()) < 1e-11
        if case.tail_mass:
            em = tfc.ContinuousBatchedEntropyModel(prior, coding_rank=case.coding_rank, laplace_tail_mass=case.tail_mass)
            theirs = em._log_prob(prior, v)
            m = case.tail_mass
            probs = (1 - m) * torch.exp(mine) + m * torch.exp(bits_ref.laplace_unit_log_mass(v))
            mine = bits_ref.laplace_tail(mine, v, m)
            # Their mixture adds two DIFFERENCES of float64 probabilities.  Compare where both still have 11
            # digits: the prior's difference (or the prior is negligible), and the Laplace cumulative, which
            # cancels left of about -8 (its survival function, used on the right, does not).  The 1e-10
            # branch is in log space on both sides and is compared everywhere.  The points left out are held
            # by the 60-digit comparison above.
            ok = (prior.prob(v) > 1e-4 * torch.exp(mine)) | ((1 - m) * prior.prob(v) < 1e-13 * torch.exp(mine))
            ok &= v > -8
            ok |= probs < bits_ref.TAIL_SWITCH
            assert int(ok.sum()) > 0.9 * ok.numel()
            assert float((mine - theirs)[ok].abs().max()) < 1e-11


@pytest.mark.parametrize("tail", [0.0, 1e-3])
def test_normal_definition_against_package_float64(tail):
    g = torch.Generator().manual_seed(5)
    scale = 10.0 ** (-2 + 4 * torch.rand(4000, generator=g, dtype=torch.float64))
    v = scale * torch.randn(4000, generator=g, dtype=torch.float64) * 3
    v[::9] *= 6
    mine = bits_ref.normal_log_prob(v, scale)
    prior = tfc.NoisyNormal(loc=torch.zeros((), dtype=torch.float64), scale=scale, dtype=torch.float64)
    if not tail:
        theirs = prior.log_prob(v)
    else:
        em = tfc.ContinuousBatchedEntropyModel(prior, coding_rank=1, laplace_tail_mass=tail)
        theirs = em._log_prob(prior, v)
        probs = (1 - tail) * torch.exp(mine) + tail * torch.exp(bits_ref.laplace_unit_log_mass(v))
        mine = bits_ref.laplace_tail(mine, v, tail)
        # Their mixture adds two differences of float64 probabilities: the Laplace cumulative cancels left of
        # about -8, and torch's float64 ndtr is 1 + erf in the lower tail (absolute, not relative, accuracy:
        # 8.6e-9 relative at z = -5.8), so the mixture branch has 11 digits only where the mixture is above
        # ~1e-4.  The 1e-10 branch is in log space on both sides; the rest is held by the 60-digit comparison.
        ok = ((v > -8) & (probs > 1e-4)) | (probs < bits_ref.TAIL_SWITCH)
        assert int(ok.sum()) > 0.5 * ok.numel() and int((probs < bits_ref.TAIL_SWITCH).sum()) > 100
        mine, theirs = mine[ok], theirs[ok]
    # relative to 1 + |log p|: log p reaches -1e4 here and float64 carries 16 digits of it
    assert float(((mine - theirs).abs() / (1 + theirs.abs())).max()) < 1e-11


def test_perturb_and_apply_against_package():
    from compression_amd.ops import math_ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(50, dtype=torch.float64, generator=g).requires_grad_(True)
    s = (1 + torch.rand(50, dtype=torch.float64, generator=g)).requires_grad_(True)
    u = torch.rand(50, dtype=torch.float64, generator=g) - 0.5
    f = lambda t: bits_ref.normal_log_prob(t, s)
    for expected in (False, True):
        a = bits_ref.perturb_and_apply(f, x, x + u, expected)
        b, _ = math_ops.perturb_and_apply(f, x, u=u, expected_grads=expected)
        ga, gb = torch.autograd.grad(a.sum(), [x, s]), torch.autograd.grad(b.sum(), [x, s])
        assert torch.equal(a, b) and all(torch.allclose(p, q, rtol=0, atol=1e-14) for p, q in zip(ga, gb))
    # the expected gradient IS the average of d f / d x over the noise
    us = torch.linspace(-0.5, 0.5, 20001, dtype=torch.float64)[:, None]
    xd = x.detach()[:5].clone().requires_grad_(True)
    mean = torch.autograd.grad(bits_ref.normal_log_prob(xd + us, s.detach()[:5]).sum(), xd)[0] / 20001
    want = torch.autograd.grad(bits_ref.perturb_and_apply(lambda t: bits_ref.normal_log_prob(t, s.detach()[:5]), xd,
                                                          xd + 0.1, True).sum(), xd)[0]
    assert torch.allclose(mean, want, rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("tail", [0.0, 1e-3])
def test_noisy_densities_sum_to_one_on_an_integer_grid(tail):
    grid = 0.3 + torch.arange(-4000, 4000, dtype=torch.float64)
    for nf, sc in (((3, 3), 10.0), ((3, 3, 3), 1.0), ((5, 5), 0.3)):
        params = [[t.double() for t in g] for g in bits_ref.factorized_raw_params(4, nf, sc, seed=7)]
        lp = bits_ref.factorized_log_prob(grid[:, None].expand(-1, 4), *params)
        if tail:
            lp = bits_ref.laplace_tail(lp, grid[:, None].expand(-1, 4), tail)
        assert float((torch.exp(lp).sum(0) - 1).abs().max()) < (1e-12 if not tail else 1e-7)   # 1e-10 clamp per point
    for sc in (1e-3, 0.3, 1.0, 40.0):
        lp = bits_ref.normal_log_prob(grid - 0.05, torch.tensor(sc, dtype=torch.float64))
        if tail:
            lp = bits_ref.laplace_tail(lp, grid - 0.05, tail)
        assert abs(float(torch.exp(lp).sum()) - 1) < (1e-12 if not tail else 1e-7)


def test_block_plan_table():
    """The block sizes the plan cases are meant to hit (plan_blocks of csrc/factorized_bits.hip, restated)."""
    for C, want in bits_ref.PLAN_THREADS.items():
        t = (512 // C) * C
        while t > 256 and t - C >= 192:
            t -= C
        assert t == want, (C, t)


# ------------------------------------------------------------------------------------------------ GPU input sets
def test_case_names_are_unique():
    assert len({c.name for c in CASES}) == len(CASES) and len({c for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_input_set(case):
    """Definition finite at every element, gradients included (so the GPU test compares EVERY element, no
    mask); the float32 envelope finite as well; every claimed regime holds at least 32 elements."""
    ref = bits_ref.reference(case)
    for r in (ref["f64"], ref["f32"]):
        for t in [r["lp"], r["bits"], r["dy"]] + list(r["dleaves"]):
            assert bool(torch.isfinite(t).all())
    for t in [ref["f64"]["bracket"], ref["f64"]["n_dy"]] + list(ref["f64"]["n_dleaves"]):
        assert bool(torch.isfinite(t).all()) and bool((t >= 0).all())
    a = ref["A_ref"]
    assert all(math.isfinite(x) for x in [a["lp"], a["dy"]] + a["dleaves"]), a
    counts = bits_ref.regime_counts(case)
    print(case.name, "A_ref", a, counts)
    for regime in case.regimes:
        if regime == "lp_0.1":
            assert counts["min_abs_lp"] >= 0.1, counts
            # an element dropped or counted twice cannot hide: the unit's tolerance in the GPU test is below
            # the smallest |log p| in that unit
            dims = tuple(range(-case.coding_rank, 0))
            tol = bits_ref.MARGIN * a["lp"] * bits_ref.EPS32 * ref["f64"]["bracket"].sum(dim=dims)
            assert bool((tol < ref["f64"]["lp"].abs().amin(dim=dims)).all()), (tol.max(), counts)
        else:
            assert counts[regime] >= 32, (regime, counts)
    if case.tail_mass:
        assert counts["tail_switch_margin"] > 1e-3, counts      # no element within float32 reach of the 1e-10 switch
    assert ref["inputs"]["y"].numel() <= 3_200_000
