"""GPU tier: the SSIM scale-pass kernels (csrc/ssim.hip) driven directly through `image_ops.scale_forward` /
`scale_backward`, one launch per call, against the float64 definition of one scale in tests/ssim_ref.py (`scale_pass`,
`scale_pass_gradients`).

Cases (tests/ssim_scale_cases.py, shapes from csrc/ssim_params.h): tap counts 1, 2, 7, 8, 11 (the unrolled kernels), 11
with TFC_SSIM_RUNTIME_TAPS=1 (the kernels with run-time taps on the 32 tile), 12 (the first on the 16 tile) and 31.  With
T the tile of the tap count n, the forward has 1, 2, T-1, T, T+1 and 2T+1 positions per axis, the backward n, n+1, T-1,
T, T+1 and 2T+1 pixels (those >= n): a pairwise cover with channels, batch, pool on / off, the pooled pair's gradient
present / absent and dx / dy / both, plus grids of one tile by three and three by one for every tap count.  float32
everywhere, a smaller cover in bfloat16, float16 and uint8 (the uint8 backward is reachable through this entry only);
inputs are 8-bit valued, so all four share one float64 result.  tests/test_ssim_scale_cpu.py shows for every forward
case that a valid range one position short, or images shifted by one pixel, would miss the bar by a factor of 4.

Bars.  No number beyond the project's stated slack; both errors are printed for every case.
    means      |kernel - f64| <= 2 |twin - f64| + 1e-6 per plane and component, the twin `image_ops.scale_reference` in
               float32 on the CPU (2: another summation order; 1e-6: the float32 slack of tests/test_ssim_gpu.py)
    gradients  max|g - g64| / max|g64| <= 2 (the same of the twin's float32 autograd) + 1e-5 per image, the bar of
               tests/test_ssim_gpu.py; g_means random with both signs, the pooled pair's gradient scaled so that the
               pool term and the moment term are of one size

Exact probes, compared with `==`: the pooled pair on 8-bit valued inputs of all four types at every forward shape (which
tile owns which pixel, the repeated border), the pool's adjoint with g_means = 0, zeros with no gradient at all, constant
images (means within two float32 spacings of 1: the position count per tile against 1 / positions; dx = dy = 0), and two
calls giving the same bits.  The pooled pair on arbitrary float32 inputs has a derived bound
(check_pooled_pair_float32).  One test holds all the cases of a tap count, or of an input type, and reports every one
that missed."""
import numpy as np
import pytest
import torch

import ssim_ref
import ssim_scale_cases as S
from compression_amd.ops import image_ops

pytestmark = pytest.mark.gpu


def cuda(a, dtype=None):
    """A contiguous device copy: the direct entries take the data pointer of a [B, H, W, C] tensor as it lies."""
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.double().cpu().numpy()


def take_route(monkeypatch, route):
    """The kernels read TFC_SSIM_RUNTIME_TAPS on every call."""
    if S.runtime_taps(route):
        monkeypatch.setenv("TFC_SSIM_RUNTIME_TAPS", "1")
    else:
        monkeypatch.delenv("TFC_SSIM_RUNTIME_TAPS", raising=False)


def each(cases, ident, check):
    """Runs `check` on every case and fails with the list of those that missed: one test holds all the cases of a tap
    count (or of an input type), so that the suite grows by tens of tests, not by hundreds.  Only a missed assertion is
    collected; an error of the library or the device ends the test at once."""
    missed = []
    for case in cases:
        try:
            check(case)
        except AssertionError as e:
            missed.append((ident(case), str(e)[:400]))
    assert not missed, missed


def of_route(cases, route):
    return [c for c in cases if c[0] == route]


by_route = pytest.mark.parametrize("route", S.ROUTES, ids=lambda r: "n%s" % r)
by_type = pytest.mark.parametrize("dtype_name", [d for d in S.DTYPES if d != "float32"])


def pooled_planes(t):
    """[planes, H2, W2, 1] on the device -> float64 [planes, H2, W2]."""
    assert t.dtype == torch.float32 and t.shape[-1] == 1
    return host(t)[..., 0]


def check_forward(monkeypatch, case, dtype_name):
    route, h, w, c, batch, pool = case
    take_route(monkeypatch, route)
    x, y = S.images("fwd", route, h, w, c, batch)
    want, hx, hy = S.forward_truth(route, h, w, c, batch)
    twin, bar = S.forward_twin(route, h, w, c, batch), S.forward_bar(route, h, w, c, batch)
    means, px, py = image_ops.scale_forward(cuda(x, S.DTYPES[dtype_name]), cuda(y, S.DTYPES[dtype_name]),
                                            S.window(route), S.C1, S.C2, pool)
    assert means.dtype == torch.float32 and tuple(means.shape) == (batch * c, 2)
    err = np.abs(host(means) - want)
    print(f"ssim_scale_fwd {S.forward_id(case)} {dtype_name}: means {want.min():.4f} ... {want.max():.4f} "
          f"err_kernel {err.max():.3e} err_twin_f32 {np.abs(twin - want).max():.3e} worst err / bar {(err / bar).max():.3f}")
    assert (err <= bar).all(), (err / bar)
    if pool:
        assert np.array_equal(pooled_planes(px), hx) and np.array_equal(pooled_planes(py), hy)
    else:
        assert px is None and py is None


@by_route
def test_forward(monkeypatch, route):
    each(of_route(S.FORWARD, route), S.forward_id, lambda case: check_forward(monkeypatch, case, "float32"))


@by_type
def test_forward_other_types(monkeypatch, dtype_name):
    each([c[1:] for c in of_route(S.FORWARD_TYPES, dtype_name)], S.forward_id,
         lambda case: check_forward(monkeypatch, case, dtype_name))


@by_route
def test_pooled_pair_is_exact(monkeypatch, route):
    """Every forward shape, whatever its own pool flag: see check_pooled_pair_is_exact."""
    each(of_route(S.FORWARD, route), S.forward_id, lambda case: check_pooled_pair_is_exact(monkeypatch, case))


def check_pooled_pair_is_exact(monkeypatch, case):
    """8-bit valued inputs: x - cen (cen the tile's first pixel), the three additions, the scale by 1/4 and + cen are all
    exact in float32 (integers below 2^10, then quarters below 2^8), so the pooled pair is `halve` in float64 bit for
    bit, for every input type."""
    route, h, w, c, batch, _ = case
    take_route(monkeypatch, route)
    x, y = S.images("fwd", route, h, w, c, batch)
    _, hx, hy = S.forward_truth(route, h, w, c, batch)
    for name, dtype in S.DTYPES.items():
        _, px, py = image_ops.scale_forward(cuda(x, dtype), cuda(y, dtype), S.window(route), S.C1, S.C2, True)
        assert tuple(px.shape) == tuple(py.shape) == (batch * c, (h + 1) // 2, (w + 1) // 2, 1), name
        assert np.array_equal(pooled_planes(px), hx), name
        assert np.array_equal(pooled_planes(py), hy), name


@by_route
def test_pooled_pair_float32(monkeypatch, route):
    """The forward cases with the pool on: see check_pooled_pair_float32 for the bound."""
    each([c for c in of_route(S.FORWARD, route) if c[5]], S.forward_id,
         lambda case: check_pooled_pair_float32(monkeypatch, case))


def check_pooled_pair_float32(monkeypatch, case):
    """Arbitrary float32 inputs.  With u = 2^-24, M = max|pixel| of both images and cen the tile's first pixel of x, every
    rounding is at most u times the size of its result:
      a_k = fl(p_k - cen), |a_k| <= 2M:             2uM each, 8uM in the sum of four
      fl(a_0 + a_1), fl(a_2 + a_3), each <= 4M:     4uM each
      their sum, <= 8M:                             8uM
      times 1/4, exact:                             (8 + 4 + 4 + 8) / 4 = 6uM so far
      + cen, a result of size <= M:                 uM   (none where the compiler fuses the last two)
    so |pooled - halve| <= 7uM, and second-order terms are below 2^-20 of that.  Prints the multiple of uM each case needs."""
    route, h, w, c, batch, _ = case
    take_route(monkeypatch, route)
    rng = np.random.default_rng(S._seed("pool32", case))
    x = (100.0 + 60.0 * rng.standard_normal((batch, h, w, c))).astype(np.float32)
    y = (x + 30.0 * rng.standard_normal((batch, h, w, c))).astype(np.float32)
    unit = 2.0 ** -24 * max(np.abs(x).max(), np.abs(y).max())
    _, px, py = image_ops.scale_forward(cuda(x), cuda(y), S.window(route), S.C1, S.C2, True)
    need = max(np.abs(pooled_planes(px) - ssim_ref.halve(S.planes(x))).max(),
               np.abs(pooled_planes(py) - ssim_ref.halve(S.planes(y))).max()) / unit
    print(f"ssim_scale_pool32 {S.forward_id(case)}: passes at {need:.3f} x 2^-24 max|pixel| (bound 7)")
    assert need <= 7.0 * (1.0 + 2.0 ** -20)


def run_backward(route, x, y, dtype, c1, c2, g_means, g_px, g_py, which):
    """-> (dx, dy) as float64 arrays or None; the pooled pair's gradient goes in only for an image that is asked for, as
    image_ops' autograd node passes it."""
    need_x, need_y = which in ("dx", "both"), which in ("dy", "both")
    gx, gy = image_ops.scale_backward(
        cuda(x, dtype), cuda(y, dtype), S.window(route), c1, c2, cuda(g_means, torch.float32),
        cuda(g_px) if need_x and g_px is not None else None, cuda(g_py) if need_y and g_py is not None else None,
        need_x, need_y)
    for g, need in ((gx, need_x), (gy, need_y)):
        assert (g is not None) == need
        assert g is None or (g.dtype == torch.float32 and g.shape == x.shape)
    return (None if gx is None else host(gx)), (None if gy is None else host(gy))


def check_backward(monkeypatch, case, dtype_name):
    route, h, w, c, batch, pooled, which = case
    take_route(monkeypatch, route)
    x, y, g_means, g_px, g_py = S.backward_inputs(route, h, w, c, batch, pooled)
    want, twin = S.backward_truth(route, h, w, c, batch, pooled), S.backward_twin(route, h, w, c, batch, pooled)
    got = run_backward(route, x, y, S.DTYPES[dtype_name], S.C1, S.C2, g_means, g_px, g_py, which)
    failures = []
    for name, g, r, g64 in zip(("dx", "dy"), got, twin, want):
        if g is None:
            continue
        err, err_twin = S.relative_error(g, g64), S.relative_error(r, g64)
        print(f"ssim_scale_bwd {S.backward_id(case)} {dtype_name} {name}: max|g64| {np.abs(g64).max():.3e} "
              f"err_kernel {err:.3e} err_twin_f32 {err_twin:.3e}")
        if not (np.isfinite(g).all() and err <= 2.0 * err_twin + 1e-5):
            failures.append((name, err, err_twin))
    assert not failures, failures


@by_route
def test_backward(monkeypatch, route):
    each(of_route(S.BACKWARD, route), S.backward_id, lambda case: check_backward(monkeypatch, case, "float32"))


@by_type
def test_backward_other_types(monkeypatch, dtype_name):
    each([c[1:] for c in of_route(S.BACKWARD_TYPES, dtype_name)], S.backward_id,
         lambda case: check_backward(monkeypatch, case, dtype_name))


ADJOINT = [("float32",) + c for c in S.BACKWARD] + S.BACKWARD_TYPES


@by_route
def test_pool_adjoint_is_exact(monkeypatch, route):
    """Every backward shape, float32 and the smaller cover of the other types: see check_pool_adjoint_is_exact."""
    each([c for c in ADJOINT if c[1] == route], lambda c: c[0] + "-" + S.backward_id(c[1:]),
         lambda case: check_pool_adjoint_is_exact(monkeypatch, case))


def check_pool_adjoint_is_exact(monkeypatch, case):
    """g_means = 0: every derivative map is zero, so dx = w g_px[i // 2, j // 2] with w = 1/4, 1/2 on an odd last row or
    column and 1 at the corner of two odd sides, a power of two: bit for bit.  With no pooled gradient either, zeros."""
    dtype_name, route, h, w, c, batch, _, which = case
    take_route(monkeypatch, route)
    x, y = S.images("bwd", route, h, w, c, batch)
    rng = np.random.default_rng(S._seed("adjoint", case))
    shape = (batch * c, (h + 1) // 2, (w + 1) // 2)
    g_px, g_py = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    zero = np.zeros((batch * c, 2), np.float32)
    got = run_backward(route, x, y, S.DTYPES[dtype_name], S.C1, S.C2, zero, g_px, g_py, which)
    for g, gp in zip(got, (g_px, g_py)):
        if g is not None:
            want = S.unplanes(ssim_ref.halve_adjoint(gp, h, w), batch, c)
            assert np.array_equal(want.astype(np.float32), want)             # the weights are powers of two
            assert np.array_equal(g, want)
    for g in run_backward(route, x, y, S.DTYPES[dtype_name], S.C1, S.C2, zero, None, None, which):
        assert g is None or not g.any()


def seam_shapes(route):
    """One position, and a grid of two tiles by three with a last tile of one position in each axis."""
    n, t = S.taps_of(route), S.tile_of(S.taps_of(route))
    return [(n, n, 1, 1), (t + 1 + n - 1, 2 * t + 1 + n - 1, 3, 2)]


@pytest.mark.parametrize("route", S.ROUTES, ids=lambda r: "n%s" % r)
def test_constant_images(monkeypatch, route):
    """x = y = one level per plane: l = cs = 1 at every position, so a plane's means are (positions counted) times the
    float32 1 / positions: within two float32 spacings (2 x 2^-23) of 1 only if every tile counts its own positions
    and no other.  The gradient of that maximum is zero, and the kernel's is exactly: the staged x - cen, y - cen are."""
    take_route(monkeypatch, route)
    for h, w, c, batch in seam_shapes(route):
        levels = np.random.default_rng(h + w).integers(1, 256, (batch, 1, 1, c))
        x = np.broadcast_to(levels, (batch, h, w, c)).astype(np.uint8)
        g_means = np.random.default_rng(3).standard_normal((batch * c, 2)).astype(np.float32)
        for name, dtype in S.DTYPES.items():
            tx = cuda(x, dtype)
            means, _, _ = image_ops.scale_forward(tx, tx.clone(), S.window(route), S.C1, S.C2, False)
            off = np.abs(host(means) - 1.0).max() / 2.0 ** -23
            print(f"ssim_scale_constant n{route} {h}x{w} c{c} b{batch} {name}: |means - 1| up to {off:.2f} spacings")
            assert off <= 2.0
            for g in run_backward(route, x, x, dtype, S.C1, S.C2, g_means, None, None, "both"):
                assert not g.any()


@pytest.mark.parametrize("route", S.ROUTES, ids=lambda r: "n%s" % r)
def test_two_calls_give_the_same_bits(monkeypatch, route):
    take_route(monkeypatch, route)
    h, w, c, batch = seam_shapes(route)[1]
    x, y, g_means, g_px, g_py = S.backward_inputs(route, h, w, c, batch, True)
    tx, ty, taps = cuda(x, torch.float32), cuda(y, torch.float32), S.window(route)
    runs = []
    for _ in range(2):
        out = image_ops.scale_forward(tx, ty, taps, S.C1, S.C2, True)
        out += image_ops.scale_backward(tx, ty, taps, S.C1, S.C2, cuda(g_means), cuda(g_px), cuda(g_py), True, True)
        runs.append([t.clone() for t in out])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_unit_range_images(monkeypatch):
    """float32 images in [0, 1] with max_val = 1 (C1 = 1e-4, C2 = 9e-4): the same bars, means and gradients; the pooled
    pair to the bound of check_pooled_pair_float32."""
    route = S.FIXED
    take_route(monkeypatch, route)
    h, w, c, batch = seam_shapes(route)[1]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    x8, y8, g_means, _, _ = S.backward_inputs(route, h, w, c, batch, False)
    x, y = (x8 / 255.0).astype(np.float32), (y8 / 255.0).astype(np.float32)
    taps = S.window(route)
    want, hx, hy = ssim_ref.scale_pass(S.planes(x), S.planes(y), taps, c1, c2)
    twin, _, _ = image_ops.scale_reference(torch.from_numpy(x), torch.from_numpy(y), taps, c1, c2, False)
    means, px, py = image_ops.scale_forward(cuda(x), cuda(y), taps, c1, c2, True)
    err, err_twin = np.abs(host(means) - want), np.abs(twin.double().numpy() - want)
    print(f"ssim_scale_unit fwd: err_kernel {err.max():.3e} err_twin_f32 {err_twin.max():.3e}")
    assert (err <= 2.0 * err_twin + 1e-6).all()
    unit = 2.0 ** -24 * max(x.max(), y.max())
    assert max(np.abs(pooled_planes(px) - hx).max(), np.abs(pooled_planes(py) - hy).max()) <= 7.0 * (1.0 + 2.0 ** -20) * unit
    mx, my = ssim_ref.scale_pass_gradients(S.planes(x), S.planes(y), taps, c1, c2, g_means)
    shape = (batch * c, (h + 1) // 2, (w + 1) // 2)
    rng = np.random.default_rng(8)
    g_px = (2.0 * np.abs(mx).max() * rng.standard_normal(shape)).astype(np.float32)
    g_py = (2.0 * np.abs(my).max() * rng.standard_normal(shape)).astype(np.float32)
    g64 = ssim_ref.scale_pass_gradients(S.planes(x), S.planes(y), taps, c1, c2, g_means, g_px, g_py)
    g32 = S.reference_gradients(x, y, taps, c1, c2, g_means, g_px, g_py, torch.float32)
    got = run_backward(route, x, y, torch.float32, c1, c2, g_means, g_px, g_py, "both")
    for name, g, r, w64 in zip(("dx", "dy"), got, g32, g64):
        w64 = S.unplanes(w64, batch, c)
        err, err_twin = S.relative_error(g, w64), S.relative_error(r, w64)
        print(f"ssim_scale_unit bwd {name}: max|g64| {np.abs(w64).max():.3e} err_kernel {err:.3e} err_twin_f32 {err_twin:.3e}")
        assert err <= 2.0 * err_twin + 1e-5
