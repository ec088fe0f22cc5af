"""GPU tier: csrc/deep_factorized_tails.hip against tests/tails_ref.py, the float64 definition of the iteration from the
prior's raw parameters (pinned on its own, with the preconditions of the exact assertions below, by
tests/test_tails_ref_cpu.py).  The C entry is called directly, so that the `iterations` output can be read; the Python
route (`_solve_device`, `_tail`, the entropy model's tables) is taken where it is the subject."""
import functools
import time

import numpy as np
import pytest
import torch

import tails_ref
from tails_ref import CASES, EPS32, TARGETS

pytestmark = pytest.mark.gpu

INDICES = range(len(CASES))
IDS = [f"{c}x{'-'.join(map(str, nf))}" for c, nf in CASES]
SENTINEL = -12345


def _packed(prior):
    from compression_amd.ops.bottleneck_ops import pack_factorized_params
    return pack_factorized_params(prior).detach()


def _call(packed, channels, params_per_channel, layers, width, targets, out, iters):
    """tfc_deep_factorized_tails as it is -> its return code."""
    from compression_amd import _lib
    t = torch.tensor([float(v) for v in targets] or [0.0], dtype=torch.float32, device="cuda")
    rc = _lib.lib().tfc_deep_factorized_tails(packed.data_ptr(), channels, params_per_channel, layers, width, t.data_ptr(),
                                              len(targets), out.data_ptr(), iters.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _launch(packed, layers, width, targets):
    """One launch, one workgroup per target -> (out [targets, channels] float32, iterations [targets])."""
    from compression_amd import _lib
    channels = packed.shape[0]
    out = torch.full((len(targets), channels), float("nan"), dtype=torch.float32, device="cuda")
    iters = torch.full((len(targets),), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(_call(packed, channels, packed.shape[1], layers, width, targets, out, iters))
    return out.cpu().numpy(), iters.cpu().numpy()


def _launch_prior(prior, targets):
    return _launch(_packed(prior), len(prior.num_filters) + 1, prior.num_filters[0], targets)


@functools.lru_cache(maxsize=None)
def _kernel(index):
    """The kernel's three results and step counts for CASES[index]: one launch with the three targets."""
    out, iters = _launch_prior(tails_ref.case(index).prior().cuda(), TARGETS)
    out.setflags(write=False)
    iters.setflags(write=False)
    return out, iters


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_iteration_count_equals_the_definitions(index):
    """The kernel makes exactly as many steps as the float64 definition (fair: the float32 twin does, and the channel
    that decides crosses its root 1000 float32 ulps away, tests/test_tails_ref_cpu.py).  The count is the result of the
    workgroup's reduction: a wrong minimum or maximum across waves, a dead lane leaking into either, or a stopping rule
    off by one step changes it.  It also holds the derivative, but only in part: a wrong df changes the ratio m / sqrt(v)
    along the approach, and with it the step at which the slowest channel crosses; a df wrong by a common factor, or
    wrong only where no channel decides, would pass here (the value test does not see df at all)."""
    case = tails_ref.case(index)
    _, iters = _kernel(index)
    for t, target in enumerate(TARGETS):
        d = case.definition[t]
        s = d.stopping_channel
        print(f"{IDS[index]} target {target:+.3f}: iterations kernel {int(iters[t])} / definition {d.iterations}; "
              f"stopped by channel {s} (wave {s // 64})")
    assert [int(i) for i in iters] == [d.iterations for d in case.definition]


def test_stopping_channels_fall_in_the_first_wave_and_in_later_ones():
    waves = {tails_ref.case(i).definition[t].stopping_channel // 64 for i in INDICES for t in range(len(TARGETS))}
    print("waves of the channels that stop a loop:", sorted(waves))
    assert 0 in waves and max(waves) > 0


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_residual_is_within_twice_the_references(index):
    """r = |logits64(x) - target| per channel, in float64 from the raw parameters.  The kernel's worst channel is within
    twice the worse of the twin's and the definition's worst channel (another summation order, FMA contraction; the
    best iterate is a minimum over a trajectory, and twin and definition are themselves up to 1.7 times apart), plus the
    rounding of the target to float32.  One channel's best iterate is a single draw, so the one-channel case takes the
    right-hand side over all cases."""
    case = tails_ref.case(index)
    out, _ = _kernel(index)
    for t, target in enumerate(TARGETS):
        got = float(tails_ref.residual(case.params, out[t], target).max())
        pool = INDICES if case.channels == 1 else [index]
        twin, definition = (max(v) for v in zip(*(tails_ref.case(i).worst_residual(t) for i in pool)))
        bound = 2 * max(twin, definition) + EPS32 * abs(target)
        print(f"{IDS[index]} target {target:+.3f}: max residual kernel {got:.3g} / twin {twin:.3g} / definition "
              f"{definition:.3g}; bound {bound:.3g}")
        assert np.all(np.isfinite(out[t]))
        assert got <= bound


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_supports_equal_the_definitions(index):
    """floor(lower - offset) and ceil(upper - offset) from the kernel's three results, in float32 as
    continuous_base._build_tables forms them, equal the definition's on every channel where the twin's do; those left
    out are at most 1 %."""
    case = tails_ref.case(index)
    out, _ = _kernel(index)
    assert out.dtype == np.float32
    lo, hi = tails_ref.supports(out[0], out[1], out[2])
    (lo64, hi64), (lo32, hi32) = case.support("definition"), case.support("twin")
    fair = (lo64 == lo32) & (hi64 == hi32)
    skipped = int((~fair).sum())
    print(f"{IDS[index]}: {skipped} of {case.channels} channels skipped in the support check")
    assert skipped <= 0.01 * case.channels
    assert np.array_equal(lo[fair], lo64[fair]) and np.array_equal(hi[fair], hi64[fair])


def test_entropy_model_tables_have_these_supports():
    """ContinuousBatchedEntropyModel over a NoisyDeepFactorized with the 96-channel case's parameters: cdf_offset and the
    table lengths are exactly the supports of the kernel's results, and those are the definition's."""
    import compression_amd as tfc
    from compression_amd import synthetic
    index = 4
    case = tails_ref.case(index)
    assert (case.channels, case.num_filters) == (96, (5, 5))
    prior = tfc.distributions.NoisyDeepFactorized(batch_shape=(case.channels,), num_filters=case.num_filters)
    prior.base.load_state_dict(case.prior().state_dict())
    prior = prior.cuda()
    em = tfc.entropy_models.ContinuousBatchedEntropyModel(prior, coding_rank=1, compression=True)
    assert em.tail_mass == 2.0 ** -8
    out, _ = _kernel(index)
    lo, hi = tails_ref.supports(out[0], out[1], out[2])
    rows = synthetic.lookup_rows(em.cdf.cpu().numpy())
    lengths = np.array([len(c) - 2 for _, c in rows])            # masses per row (the cdf has the overflow's + 1 more)
    assert np.array_equal(em.cdf_offset.cpu().numpy(), lo)
    assert np.array_equal(lengths, hi - lo + 1)
    lo64, hi64 = case.support("definition")
    twin = case.support("twin")
    assert np.array_equal(twin[0], lo64) and np.array_equal(twin[1], hi64)
    assert np.array_equal(lo, lo64) and np.array_equal(hi, hi64)


@pytest.mark.parametrize("index", INDICES, ids=IDS)
def test_targets_together_equal_targets_alone(index):
    """One launch with the three targets is byte-identical to three launches with one target each and to a second
    launch of the same, in `out` and in `iterations`; `_solve_device` returns the same bytes."""
    prior = tails_ref.case(index).prior().cuda()
    out, iters = _kernel(index)
    again, iters_again = _launch_prior(prior, TARGETS)
    assert out.tobytes() == again.tobytes() and iters.tobytes() == iters_again.tobytes()
    for t, target in enumerate(TARGETS):
        alone, iters_alone = _launch_prior(prior, [target])
        assert alone[0].tobytes() == out[t].tobytes() and int(iters_alone[0]) == int(iters[t])
    solved = prior._solve_device(TARGETS)
    assert solved is not None and solved.cpu().numpy().tobytes() == out.tobytes()
    assert prior._tail(TARGETS[1]).cpu().numpy().tobytes() == out[1].tobytes()


@pytest.mark.parametrize("channel", [64, 0])
def test_a_nan_loss_ends_the_loop_with_the_best_so_far(channel):
    """The 65-channel case with one channel's first bias NaN: channel 64 is alone in the second wave with 63 dead lanes,
    so its flag has to cross waves; channel 0 sits in the wave that decides.  The reference's loop ends at once on a NaN
    loss and returns every channel's best iterate so far: what tails_ref.iterate gives for the same inputs."""
    case = tails_ref.case(3)
    assert case.channels == 65
    prior = case.prior()
    with torch.no_grad():
        prior.biases[0][channel, 0, 0] = float("nan")
    params = tails_ref.raw_params(prior)
    assert np.isnan(params[1][0][channel, 0, 0]) and int(np.isnan(params[1][0]).sum()) == 1
    out, iters = _launch_prior(prior.cuda(), TARGETS)
    for t, target in enumerate(TARGETS):
        for dtype in (np.float64, np.float32):
            best, iterations, _ = tails_ref.iterate(params, target, dtype)
            assert int(iters[t]) == iterations
            assert np.array_equal(out[t], best.astype(np.float32))
    print(f"NaN in channel {channel}: iterations {[int(i) for i in iters]}, results all {float(out.max())}")


def test_iteration_cap_bounds_a_channel_that_never_arrives():
    """f(x) = 1e-6 x with target 1, hand-packed (K = 2, W = 1, one channel): the root is at 1e6 and steps of 0.1 do not
    reach it, so the launch ends at kTailMaxIters with the last iterate evaluated, where the definition stands after as
    many steps, to within twice the float32 twin's own distance from it."""
    packed = torch.tensor([tails_ref.CAP_PACKED], dtype=torch.float32, device="cuda")
    assert float(packed[0, 0]) == tails_ref.CAP_SLOPE
    big = tails_ref.case(5).prior().cuda()
    _launch_prior(big, TARGETS)
    t0 = time.perf_counter()
    _launch_prior(big, TARGETS)
    t_big = time.perf_counter() - t0
    t0 = time.perf_counter()
    out, iters = _launch(packed, 2, 1, [tails_ref.CAP_TARGET])
    t_cap = time.perf_counter() - t0
    print(f"capped launch {1e3 * t_cap:.1f} ms; the 1024-channel case's launch {1e3 * t_big:.1f} ms")
    definition, twin = tails_ref.capped(np.float64), tails_ref.capped(np.float32)
    x, want, near = float(out[0, 0]), float(definition.best_x[0]), float(twin.best_x[0])
    print(f"at the cap: kernel {x:.6f}, twin {near:.6f}, definition {want:.6f}")
    from compression_amd.distributions import deep_factorized
    assert int(iters[0]) == definition.iterations == deep_factorized._DEVICE_TAIL_ITERATION_CAP == 100000
    assert np.isfinite(x)
    assert abs(x - want) <= 2 * abs(near - want) + EPS32 * abs(x)


@pytest.mark.parametrize("channels,num_filters,dtype", [
    (4, (), torch.float32), (4, (3, 5), torch.float32), (4, (9, 9), torch.float32), (1025, (3, 3), torch.float32),
    (4, (3, 3), torch.float64)], ids=["no-hidden-layer", "unequal-widths", "width-9", "1025-channels", "float64"])
def test_where_the_kernel_does_not_apply_the_tensor_ops_decide(channels, num_filters, dtype):
    from compression_amd import distributions
    from compression_amd.distributions import helpers
    torch.manual_seed(11)
    prior = distributions.DeepFactorized(batch_shape=(channels,), num_filters=num_filters, dtype=dtype).cuda()
    assert prior._solve_device([0.0]) is None and prior._solve_device(TARGETS) is None
    got = prior._lower_tail(2.0 ** -8)
    want = helpers.estimate_tails(prior._logits_cumulative, TARGETS[1], prior.batch_shape, dtype, "cuda")
    assert got.dtype == dtype and got.shape == (channels,) and torch.equal(got, want)
    with torch.no_grad():
        miss = (prior._logits_cumulative(got) - TARGETS[1]).abs()
        start = (prior._logits_cumulative(torch.zeros_like(got)) - TARGETS[1]).abs()
    assert bool((miss < start).all())          # a solution, not the start


@pytest.mark.parametrize("channels,ppc,layers,width,words", [
    (0, 28, 3, 3, "1 ... 1024 channels (one workgroup iterates them together), got 0"),
    (1025, 28, 3, 3, "1 ... 1024 channels (one workgroup iterates them together), got 1025"),
    (4, 28, 1, 3, "layers >= 2 and hidden width 1 ... 8 (got 1, 3)"),
    (4, 28, 3, 0, "layers >= 2 and hidden width 1 ... 8 (got 3, 0)"),
    (4, 28, 3, 9, "layers >= 2 and hidden width 1 ... 8 (got 3, 9)"),
    (4, 27, 3, 3, "27 parameters per channel, the layout has 28"),
    (4, 28, 2, 3, "28 parameters per channel, the layout has 13")],
    ids=["channels-0", "channels-1025", "layers-1", "width-0", "width-9", "short-parameters", "parameters-of-3-layers"])
def test_c_entry_refuses_in_words_and_launches_nothing(channels, ppc, layers, width, words):
    """3 W + (K - 2) (W^2 + 2 W) + W + 1 parameters per channel: 28 for K = 3, W = 3 and 13 for K = 2."""
    from compression_amd import _lib
    packed = torch.zeros((1025, 28), dtype=torch.float32, device="cuda")
    out = torch.full((3, 1025), float(SENTINEL), dtype=torch.float32, device="cuda")
    iters = torch.full((3,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = _call(packed, channels, ppc, layers, width, TARGETS, out, iters)
    assert rc != 0
    message = _lib.last_error()
    assert "tfc_deep_factorized_tails" in message and words in message, message
    assert bool((out == SENTINEL).all()) and bool((iters == SENTINEL).all())


def test_no_targets_is_no_work():
    packed = _packed(tails_ref.case(0).prior().cuda())
    out = torch.full((3, 1), float(SENTINEL), dtype=torch.float32, device="cuda")
    iters = torch.full((3,), SENTINEL, dtype=torch.int32, device="cuda")
    assert _call(packed, 1, packed.shape[1], 3, 3, [], out, iters) == 0
    assert bool((out == SENTINEL).all()) and bool((iters == SENTINEL).all())
