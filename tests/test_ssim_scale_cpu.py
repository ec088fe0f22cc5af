"""CPU tier of the SSIM scale pass (csrc/ssim.hip, one launch of `image_ops.scale_forward` / `scale_backward`): the float64
definition of one scale in tests/ssim_ref.py (`scale_pass`, `scale_pass_gradients`) against derivations that do not
share its code, the constants the GPU file builds its shapes from, and a check that every forward case of
tests/test_ssim_scale_gpu.py can tell a right kernel from a wrong one.

The last one: for every forward case the float64 means are also taken under deliberately wrong definitions, the valid
range one position short in an axis (where that axis has more than one position) and both images shifted by one pixel
along an axis (for more than one tap: with one tap the mean over all pixels does not change).  Each must move every plane's
means by at least 4 bars of that case (the bar of the GPU file, 2 |float32 twin - float64| + 1e-6, per plane and
component): a kernel at the edge of its bar still stands clear of a mutant at half its distance.  A case that does not
separate is redrawn (ssim_scale_cases.REDRAWN), not excused."""
import numpy as np
import pytest
import torch

import ssim_ref
import ssim_scale_cases as S
from compression_amd.ops import image_ops


def pair(seed, planes, h, w, noise=20.0):
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(128.0 + 40.0 * rng.standard_normal((planes, h, w))), 0, 255)
    y = np.clip(np.round(x + noise * rng.standard_normal((planes, h, w))), 0, 255)
    return x, y


def cotangents(seed, planes, h, w, pooled):
    rng = np.random.default_rng(seed)
    g_means = rng.standard_normal((planes, 2))
    if not pooled:
        return g_means, None, None
    shape = (planes, (h + 1) // 2, (w + 1) // 2)
    return g_means, 1e-3 * rng.standard_normal(shape), 1e-3 * rng.standard_normal(shape)


def test_constants_are_read_from_the_header():
    k = image_ops.SSIM_CONSTANTS
    assert set(k) == {"SSIM_MAX_TAPS", "SSIM_TILE_SMALL_N", "SSIM_TILE_LARGE_N", "SSIM_TILE_SMALL_N_MAX", "SSIM_FIXED_TAPS"}
    assert image_ops.MAX_FILTER_SIZE == k["SSIM_MAX_TAPS"] == 31
    assert (k["SSIM_TILE_SMALL_N"], k["SSIM_TILE_LARGE_N"], k["SSIM_TILE_SMALL_N_MAX"], k["SSIM_FIXED_TAPS"]) == (32, 16, 11, 11)
    assert [S.tile_of(n) for n in (1, 2, 10, 11)] == [32] * 4 and [S.tile_of(n) for n in (12, 13, 31)] == [16] * 3


def test_scale_pass_is_scale_maps_and_halve():
    for n, h, w in [(1, 1, 1), (1, 4, 5), (2, 2, 3), (2, 7, 6), (11, 11, 11), (11, 14, 17), (11, 16, 13)]:
        check_scale_pass_is_scale_maps_and_halve(n, h, w)


def check_scale_pass_is_scale_maps_and_halve(n, h, w):
    x, y = pair(n * 100 + h, 3, h, w)
    g = ssim_ref.window(n, 1.5)
    means, hx, hy = ssim_ref.scale_pass(x, y, g, S.C1, S.C2)
    value, cs = ssim_ref.scale_maps(x, y, 255.0, g)
    assert means.shape == (3, 2) and hx.shape == hy.shape == (3, (h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(means[:, 0], value) and np.array_equal(means[:, 1], cs)
    assert np.array_equal(hx, ssim_ref.halve(x)) and np.array_equal(hy, ssim_ref.halve(y))
    assert np.array_equal(ssim_ref.scale_pass(x[1], y[1], g, S.C1, S.C2)[0], means[1])


def test_gradients_against_central_differences():
    for n, h, w, pooled in [(1, 3, 2, True), (2, 5, 4, True), (2, 4, 5, False), (3, 5, 5, True)]:
        check_gradients_against_central_differences(n, h, w, pooled)


def check_gradients_against_central_differences(n, h, w, pooled):
    """The closed form against (f(x + e) - f(x - e)) / 2e of the scalar it differentiates, pixel by pixel, in float64.
    e = 1e-3 of a pixel unit: the truncation error (e^2 f''' / 6) and the rounding error (1e-16 |f| / e) are both below
    1e-7 of the largest derivative here; the bar is 1e-6 of it."""
    x, y = pair(7 + n, 2, h, w)
    g = ssim_ref.window(n, 1.5)
    g_means, g_px, g_py = cotangents(11, 2, h, w, pooled)

    def value(a, b):
        means, ha, hb = ssim_ref.scale_pass(a, b, g, S.C1, S.C2)
        v = (means * g_means).sum()
        return v + ((ha * g_px).sum() + (hb * g_py).sum() if pooled else 0.0)

    dx, dy = ssim_ref.scale_pass_gradients(x, y, g, S.C1, S.C2, g_means, g_px, g_py)
    e = 1e-3
    for which, got in ((0, dx), (1, dy)):
        numeric = np.zeros_like(got)
        for at in np.ndindex(got.shape):
            hi, lo = [x.copy(), y.copy()], [x.copy(), y.copy()]
            hi[which][at] += e
            lo[which][at] -= e
            numeric[at] = (value(*hi) - value(*lo)) / (2 * e)
        assert np.abs(got - numeric).max() <= 1e-6 * np.abs(numeric).max()


@pytest.mark.parametrize("pooled", ["both", "x", "y", "none"])
def test_gradients_against_float64_autograd(pooled):
    """Two derivations of one gradient: the closed form in NumPy and torch autograd through
    `image_ops.scale_reference` (conv2d, replicate pad, avg_pool2d) in float64.  Relative difference <= 1e-9."""
    for n, h, w in [(1, 1, 1), (1, 6, 5), (2, 2, 2), (2, 9, 8), (2, 8, 7), (11, 11, 11), (11, 20, 23), (11, 21, 18),
                    (11, 45, 44)]:
        check_gradients_against_float64_autograd(n, h, w, pooled)


def check_gradients_against_float64_autograd(n, h, w, pooled):
    batch, c = 2, 3
    x, y = pair(31 + n + h, batch * c, h, w)
    g = ssim_ref.window(n, 1.5)
    g_means, g_px, g_py = cotangents(5, batch * c, h, w, pooled != "none")
    g_px = g_px if pooled in ("both", "x") else None
    g_py = g_py if pooled in ("both", "y") else None
    want = ssim_ref.scale_pass_gradients(x, y, g, S.C1, S.C2, g_means, g_px, g_py)
    got = S.reference_gradients(S.unplanes(x, batch, c), S.unplanes(y, batch, c), tuple(g), S.C1, S.C2, g_means, g_px,
                                g_py, torch.float64)
    for a, b in zip(got, want):
        assert S.relative_error(a, S.unplanes(b, batch, c)) <= 1e-9, (n, h, w, pooled)


def test_scale_reference_matches_the_definition():
    """`scale_reference` in float64 against `scale_pass`: means to 1e-12, the pooled pair in `scale_forward`'s layout;
    float32 for every other input type."""
    x, y = pair(3, 6, 15, 18)
    g = ssim_ref.window(7, 1.5)
    means, hx, hy = ssim_ref.scale_pass(x, y, g, S.C1, S.C2)
    tx, ty = torch.from_numpy(S.unplanes(x, 2, 3).copy()), torch.from_numpy(S.unplanes(y, 2, 3).copy())
    got, px, py = image_ops.scale_reference(tx, ty, tuple(g), S.C1, S.C2, True)
    assert got.dtype == px.dtype == torch.float64 and tuple(got.shape) == (6, 2) and tuple(px.shape) == (6, 8, 9, 1)
    assert np.abs(got.numpy() - means).max() <= 1e-12
    assert np.array_equal(px.numpy()[..., 0], hx) and np.array_equal(py.numpy()[..., 0], hy)
    got32, none_x, none_y = image_ops.scale_reference(tx.to(torch.uint8), ty.to(torch.uint8), tuple(g), S.C1, S.C2, False)
    assert got32.dtype == torch.float32 and none_x is None and none_y is None
    assert np.abs(got32.double().numpy() - means).max() <= 1e-4


def test_case_lists_reach_the_edges():
    """What the GPU file relies on: every route, grids of one tile by three and three by one, odd and even sides in both
    axes, every pixel kind of the backward, and no image larger than 2T + 1 + n - 1 on a side."""
    for route in S.ROUTES:
        n, t = S.taps_of(route), S.tile_of(S.taps_of(route))
        fwd = [c for c in S.FORWARD if c[0] == route]
        tiles = {(-(-(c[1] - n + 1) // t), -(-(c[2] - n + 1) // t)) for c in fwd}
        assert {(1, 3), (3, 1)} <= tiles, (route, tiles)
        for axis in (1, 2):
            assert {c[axis] - n + 1 for c in fwd} == {1, 2, t - 1, t, t + 1, 2 * t + 1}
        assert {c[3] for c in fwd} == {1, 3, 4} and {c[4] for c in fwd} == {1, 2} and {c[5] for c in fwd} == {True, False}
        bwd = [c for c in S.BACKWARD if c[0] == route]
        grids = [(-(-c[1] // t), -(-c[2] // t)) for c in bwd]
        assert any(a < b for a, b in grids) and any(a > b for a, b in grids), (route, grids)
        sides = {k: S.extent(k, n) for k in S.PIXEL_KINDS if S.extent(k, n) >= n}
        for axis in (1, 2):
            assert {c[axis] for c in bwd} == set(sides.values())
            assert {c[axis] % 2 for c in fwd} == {0, 1} and {c[axis] % 2 for c in bwd} == {0, 1}
        assert {c[5] for c in bwd} == {True, False} and {c[6] for c in bwd} == {"dx", "dy", "both"}
        assert max(max(c[1], c[2]) for c in fwd + bwd) <= 2 * t + 1 + n - 1
    for cases in (S.FORWARD_TYPES, S.BACKWARD_TYPES):
        assert {(c[0], c[1]) for c in cases} == {(d, r) for d in ("bfloat16", "float16", "uint8") for r in S.ROUTES}
    assert {(c[1] % 2, c[2] % 2) for c in S.FORWARD} == {(0, 0), (0, 1), (1, 0), (1, 1)}


SHAPES = list(dict.fromkeys(c[:5] for c in S.ALL_FORWARD))


def mutants(route, h, w, c, batch):
    """name -> means [planes, 2] under a wrong definition."""
    x, y = S.images("fwd", route, h, w, c, batch)
    px, py, g = S.planes(x), S.planes(y), np.asarray(S.window(route))
    lcs, cs = ssim_ref.position_maps(px, py, g, S.C1, S.C2)
    mean = lambda a, b: np.stack([a.mean(axis=(-2, -1)), b.mean(axis=(-2, -1))], axis=-1)          # noqa: E731
    found = {}
    if lcs.shape[-2] > 1:
        found["rows one short"] = mean(lcs[:, :-1, :], cs[:, :-1, :])
    if lcs.shape[-1] > 1:
        found["columns one short"] = mean(lcs[:, :, :-1], cs[:, :, :-1])
    for name, axis in (("shifted down", -2), ("shifted right", -1)):
        # one tap, or the two equal taps on a side of two pixels: the shift changes nothing, whatever the data
        if len(g) > 2 or (len(g) == 2 and px.shape[axis] > 2):
            found[name] = ssim_ref.scale_pass(np.roll(px, 1, axis=axis), np.roll(py, 1, axis=axis), g, S.C1, S.C2)[0]
    return found


@pytest.mark.parametrize("route", S.ROUTES, ids=lambda r: "n%s" % r)
def test_forward_cases_separate_mutants(route):
    """All the forward shapes of one tap count; every one that does not separate is named."""
    missed = []
    for shape in SHAPES:
        if shape[0] == route:
            try:
                check_forward_case_separates_mutants(shape)
            except AssertionError as e:
                missed.append((shape, str(e)[:300]))
    assert not missed, missed


def check_forward_case_separates_mutants(shape):
    want = S.forward_truth(*shape)[0]
    bar = S.forward_bar(*shape)
    found = mutants(*shape)
    n = S.taps_of(shape[0])
    assert found or (n <= 2 and shape[1] == shape[2] == n)      # one position of one or two taps: the seam cases carry it
    for name, means in found.items():
        ratio = (np.abs(means - want) / bar).max(axis=-1)       # per plane: the component that separates best
        print(f"ssim_scale mutant {shape} {name}: bars of distance, the worst plane {ratio.min():.1f}, largest bar {bar.max():.2e}")
        assert ratio.min() >= 4.0, (name, ratio)
