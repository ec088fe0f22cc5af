"""CPU tier: tests/tails_ref.py, the float64 definition csrc/deep_factorized_tails.hip is held to, pinned on its own:
its logits and their derivative against the package's float64 class and autograd, its iteration against
helpers.estimate_tails on the float64 prior, and, for every case and target of tests/test_tails_gpu.py, the
preconditions that make that file's exact assertions fair: definition and float32 twin stop after the same number of
steps, the channel that stops the loop crosses its root at a distance no float32 rounding can bridge, and both give the
same table supports."""
import numpy as np
import pytest
import torch

import tails_ref
from tails_ref import CASES, EPS32, EPS64, TARGETS

INDICES = range(len(CASES))
IDS = [f"{c}x{'-'.join(map(str, nf))}" for c, nf in CASES]


def _double_prior(case):
    return case.prior().double()


def _estimate_tails(prior64, target):
    """helpers.estimate_tails on the float64 prior -> (best iterates, number of steps: one call of the function each)."""
    from compression_amd.distributions import helpers
    calls = []

    def func(x):
        calls.append(1)
        return prior64._logits_cumulative(x)
    got = helpers.estimate_tails(func, target, prior64.batch_shape, torch.float64)
    return got.numpy(), len(calls)


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_logits_and_derivative_equal_the_float64_class_and_autograd(index):
    """Relative to magnitude (of the logits: at least 1, they pass through 0; of the derivative: its own), at the level
    of float64 rounding: the two sum the same products in another order, and autograd's reverse sweep multiplies the
    layers' factors from the other end.  Measured here over the six cases: at most 2.1 eps for the logits, 2.9 eps for
    the derivative; the bar is 100 times that, 5e-14 and 6e-14."""
    case = tails_ref.case(index)
    prior = _double_prior(case)
    points = [np.full(case.channels, v) for v in (-40.0, -6.0, -0.7, 0.0, 0.3, 2.5, 11.0, 60.0)]
    points += [r.best_x for r in case.definition]
    worst_f = worst_d = 0.0
    for x in points:
        f, df = tails_ref.logits(case.params, x)
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        ft = prior._logits_cumulative(xt)
        dt, = torch.autograd.grad(ft.sum(), xt)
        ft, dt = ft.detach().numpy(), dt.numpy()
        assert np.all(df > 0)
        worst_f = max(worst_f, float((np.abs(f - ft) / np.maximum(np.abs(ft), 1.0)).max()))
        worst_d = max(worst_d, float((np.abs(df - dt) / np.abs(dt)).max()))
    print(f"{IDS[index]}: logits {worst_f / EPS64:.1f} eps, derivative {worst_d / EPS64:.1f} eps relative")
    assert worst_f <= 100 * 2.1 * EPS64
    assert worst_d <= 100 * 2.9 * EPS64


def test_float32_twin_keeps_its_dtype():
    case = tails_ref.case(3)
    f, df = tails_ref.logits(case.params, 0.25, np.float32)
    assert f.dtype == df.dtype == np.float32
    f64, df64 = tails_ref.logits(case.params, 0.25)
    # float32 products and sums of O(1) terms through 4 layers: a few float32 ulps of the magnitude
    assert np.all(np.abs(f - f64) <= 64 * EPS32 * np.maximum(np.abs(f64), 1.0))
    assert np.all(np.abs(df - df64) <= 64 * EPS32 * np.abs(df64))
    assert all(r.best_x.dtype == np.float32 for r in case.twin)


def test_root_is_where_the_logits_cross_the_target():
    case = tails_ref.case(4)
    for target in TARGETS:
        x = tails_ref.root(case.params, target)
        below, _ = tails_ref.logits(case.params, np.nextafter(x, -np.inf))
        above, _ = tails_ref.logits(case.params, np.nextafter(x, np.inf))
        assert np.all(below <= target) and np.all(above >= target) and np.all(below < above)


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_iteration_reproduces_estimate_tails_in_float64(index):
    """The same loop, autograd's derivative there and the analytic one here: the same number of steps, and iterates
    apart by no more than 100 float64 epsilons per step at the scale of the largest |x|."""
    case = tails_ref.case(index)
    prior = _double_prior(case)
    for t, target in enumerate(TARGETS):
        want, steps = _estimate_tails(prior, target)
        got = case.definition[t]
        scale = float(np.abs(want).max())
        diff = float(np.abs(got.best_x - want).max())
        print(f"{IDS[index]} target {target:+.3f}: {got.iterations} steps (estimate_tails {steps}), max |x| {scale:.3f}, "
              f"largest |x - estimate_tails| {diff:.3g}")
        assert got.iterations == steps
        assert diff <= 100 * EPS64 * steps * scale


# ------------------------------------------------------------------------------------------------ preconditions of the GPU tests
@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_definition_and_twin_stop_after_the_same_number_of_steps(index):
    """(a): what makes `iterations(kernel) == iterations(definition)` a fair assertion."""
    case = tails_ref.case(index)
    for t, target in enumerate(TARGETS):
        d, w = case.definition[t], case.twin[t]
        print(f"{IDS[index]} target {target:+.3f}: {d.iterations} steps in float64, {w.iterations} in float32; "
              f"stopped by channel {d.stopping_channel} / {w.stopping_channel}")
        assert d.iterations == w.iterations
        assert d.stopping_channel == w.stopping_channel
        # the loop ended by the counts, 99 steps after the last channel's first sign flip, not by a loss below 1e-8
        assert np.all(d.first_flip > 0) and d.iterations == d.first_flip.max() + 99


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_the_stopping_channel_crosses_its_root_with_a_margin(index):
    """(b): the channel whose first sign flip comes last decides the number of steps.  Its last iterate before and its
    first one past the root are both at least 1000 float32 ulps of |x| away from the root (float64 bisection): a few
    hundred steps whose rounding differs by a few ulps each cannot move the crossing to another step."""
    case = tails_ref.case(index)
    for t, target in enumerate(TARGETS):
        d = case.definition[t]
        s = d.stopping_channel
        x = tails_ref.root(case.params, target)[s]
        before, after = float(d.before[s]), float(d.after[s])
        assert (before - x) * (after - x) < 0
        margins = [abs(v - x) / float(np.spacing(np.float32(abs(v)))) for v in (before, after)]
        print(f"{IDS[index]} target {target:+.3f}: channel {s} crosses {x:.6f} from {before:.6f} to {after:.6f}: "
              f"{margins[0]:.0f} and {margins[1]:.0f} float32 ulps away")
        assert min(margins) >= 1000


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_definition_and_twin_give_the_same_supports(index):
    """(c): floor(lower - offset) and ceil(upper - offset) agree on at least 99 % of the channels; the GPU test leaves
    out the others."""
    case = tails_ref.case(index)
    (lo64, hi64), (lo32, hi32) = case.support("definition"), case.support("twin")
    differ = int(((lo64 != lo32) | (hi64 != hi32)).sum())
    print(f"{IDS[index]}: supports differ on {differ} of {case.channels} channels; lengths "
          f"{int((hi64 - lo64 + 1).min())} .. {int((hi64 - lo64 + 1).max())}")
    assert np.all(hi64 > lo64)
    assert differ <= 0.01 * case.channels


def test_stopping_channels_fall_in_the_first_wave_and_in_later_ones():
    waves = {tails_ref.case(i).definition[t].stopping_channel // 64 for i in INDICES for t in range(len(TARGETS))}
    assert 0 in waves and max(waves) > 0


def test_residuals_of_definition_and_twin():
    """The figures the GPU test's value bound is made of (printed, and finite)."""
    for i in INDICES:
        for t, target in enumerate(TARGETS):
            twin, definition = tails_ref.case(i).worst_residual(t)
            print(f"{IDS[i]} target {target:+.3f}: max residual twin {twin:.3g}, definition {definition:.3g}")
            assert np.isfinite(twin) and np.isfinite(definition)


# ------------------------------------------------------------------------------------------------ NaN and the cap
@pytest.mark.parametrize("channel", [64, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_loss_ends_the_loop_with_the_best_so_far(channel, dtype):
    """One channel's first bias is NaN: its loss is NaN after the first step, `NaN > 1e-8` is false, and every
    channel's best iterate then is the start."""
    case = tails_ref.case(3)
    params = tails_ref.with_nan_bias(case.params, channel)
    for target in TARGETS:
        best, iterations, first_flip = tails_ref.iterate(params, target, dtype)
        assert iterations == 1 and np.all(first_flip == -1)
        assert best.dtype == dtype and np.array_equal(best, np.zeros(case.channels, dtype))
    if dtype is np.float64:
        prior = _double_prior(case)
        with torch.no_grad():
            prior.biases[0][channel, 0, 0] = float("nan")
        want, steps = _estimate_tails(prior, TARGETS[1])
        assert steps == 1 and np.array_equal(want, np.zeros(case.channels))


def test_the_capped_input_stops_at_the_cap():
    """f(x) = 1e-6 x, target 1: the gradient never changes, the step tends to 0.1 from below (|m| / sqrt(v) < 1, and v
    forgets its start of 1 against g^2 = 2^-40 within some 50 halvings), the loss falls all the way, so the best iterate
    is the last one evaluated: the sum of cap - 1 steps.  Float32 rounds each sum by at most half an ulp of x < 2^14."""
    cap = tails_ref.CAP_ITERATIONS
    definition, twin = tails_ref.capped(np.float64), tails_ref.capped(np.float32)
    print(f"capped input: definition {definition.best_x[0]:.6f}, twin {twin.best_x[0]:.6f} after {definition.iterations} steps")
    assert definition.iterations == twin.iterations == cap
    assert definition.first_flip[0] == twin.first_flip[0] == -1
    assert 0.1 * (cap - 1 - 100) < definition.best_x[0] < 0.1 * (cap - 1)
    assert twin.best_x.dtype == np.float32 and np.isfinite(twin.best_x[0])
    assert abs(float(twin.best_x[0]) - definition.best_x[0]) <= cap * 2.0 ** 13 * EPS32
