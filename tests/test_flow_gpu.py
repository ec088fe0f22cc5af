"""GPU tier: the scale-space kernels (csrc/scale_space.hip) against the float64 definition (tests/flow_ref.py).

The bar is the project's usual one, with no number chosen in advance: for the output and every gradient
err_kernel <= 2 err_twin + 1e-6 in relative L2 against float64, the float32 twin running on the CPU.  Both errors are
printed.  The inputs (flow_ref.make_case) put every coordinate on an odd sixteenth, so float32(j) + dx is exact and the
floor and clamp decisions of float32 and float64 agree by construction; `_assert_decisions_agree` checks that on the
CPU for every case."""
import functools

import numpy as np
import pytest
import torch

import flow_ref
from compression_amd.ops import flow_ops

pytestmark = pytest.mark.gpu

K = flow_ops.SCALE_SPACE_CONSTANTS
SHAPES = [
    (1, 1, 1, 1, 1, 1.5),                 # smallest possible
    (2, 7, 5, 3, 5, 1.5),                 # image smaller than every radius
    (1, 65, 130, 3, 5, 1.5),              # one past a wave and past two column tiles; radius 72 > H
    (1, 33, 64, 4, 3, 0.5),               # 16-byte channel path
    (2, 64, 63, 1, 2, 1.5),
    (1, 16, 16, 8, 8, 0.5),
    # tile +- 1 in each axis, from the kernels' own constants
    (1, 3, K["SS_ROW_TILE"] - 1, 1, 2, 0.5),
    (1, 3, K["SS_ROW_TILE"] + 1, 2, 2, 0.5),
    (1, K["SS_COL_TILE_H"] - 1, 5, 1, 2, 0.5),
    (1, K["SS_COL_TILE_H"] + 1, 5, 3, 2, 0.5),
    (1, 4, K["SS_COL_TILE_X"] - 1, 1, 2, 0.5),
    (1, 4, K["SS_COL_TILE_X"] + 1, 1, 2, 0.5),
    (1, 1, K["SS_WARP_TILE"] - 1, 1, 1, 0.5),
    (1, 1, K["SS_WARP_TILE"] + 1, 1, 1, 0.5),
]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


def _assert_decisions_agree(shape, flow):
    """Every float64 coordinate is an odd sixteenth (so at least 1/16 from every integer, which is where the floors and
    the clamps at 0, W - 1, H - 1 and M sit), and float32 forms the same coordinate exactly."""
    n, h, w, _, m, _ = shape
    for raw in flow_ref.coordinates(flow, m + 1):
        scaled = raw * 16.0
        assert np.all(scaled == np.round(scaled)) and np.all(np.round(scaled).astype(np.int64) % 2 != 0)
    jj = np.arange(w, dtype=np.float32)[None, None, :]
    ii = np.arange(h, dtype=np.float32)[None, :, None]
    assert np.array_equal((jj + flow[..., 0]).astype(np.float64), flow_ref.coordinates(flow, m + 1)[0])
    assert np.array_equal((ii + flow[..., 1]).astype(np.float64), flow_ref.coordinates(flow, m + 1)[1])


def _grads(fn, inputs, g):
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    grads = torch.autograd.grad(out, leaves, g, allow_unused=True)
    return out.detach(), [torch.zeros_like(l) if gr is None else gr for l, gr in zip(leaves, grads)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """Everything a shape's tests share, computed once: inputs, the float64 definition, the float32 twin on the CPU and
    the kernels' results (as numpy arrays)."""
    n, h, w, c, m, sigma0 = shape
    x, flow, g = flow_ref.make_case(shape, seed=sum(shape[:5]))
    _assert_decisions_agree(shape, flow)
    rng = np.random.default_rng(7)
    g_vol_in = rng.standard_normal((n, m + 1, h, w, c)).astype(np.float32)
    ref = {}
    vol64 = flow_ref.volume(x, m, sigma0)
    vol32 = vol64.astype(np.float32)                       # the warp-only tests' input volume
    ref["volume"] = vol64
    ref["volume_gx"] = flow_ref.volume_adjoint(g_vol_in, sigma0)
    ref["warp"] = flow_ref.warp(vol32, flow)
    ref["warp_gv"], ref["warp_gflow"] = flow_ref.warp_gradients(vol32, flow, g)
    ref["predict"] = flow_ref.predict(x, flow, m, sigma0)
    ref["predict_gx"], ref["predict_gflow"] = flow_ref.predict_gradients(x, flow, g, m, sigma0)

    def run(device, volume_fn, warp_fn, predict_fn):
        t = lambda a: torch.from_numpy(a).to(device)
        res = {}
        res["volume"], (res["volume_gx"],) = _grads(lambda a: volume_fn(a, m, sigma0), [t(x)], t(g_vol_in))
        res["warp"], (res["warp_gv"], res["warp_gflow"]) = _grads(warp_fn, [t(vol32), t(flow)], t(g))
        res["predict"], (res["predict_gx"], res["predict_gflow"]) = _grads(
            lambda a, f: predict_fn(a, f, m, sigma0), [t(x), t(flow)], t(g))
        return {k: v.cpu().numpy() for k, v in res.items()}

    twin = run("cpu", flow_ops.gaussian_scale_space_reference, flow_ops.scale_space_warp_reference,
               flow_ops.scale_space_predict_reference)
    kernel = run("cuda", flow_ops.gaussian_scale_space, flow_ops.scale_space_warp, flow_ops.scale_space_predict)
    again = run("cuda", flow_ops.gaussian_scale_space, flow_ops.scale_space_warp, flow_ops.scale_space_predict)
    return {"x": x, "flow": flow, "g": g, "vol32": vol32, "ref": ref, "twin": twin, "kernel": kernel, "again": again}


QUANTITIES = ["volume", "volume_gx", "warp", "warp_gv", "warp_gflow", "predict", "predict_gx", "predict_gflow"]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_against_float64(shape):
    data = case(shape)
    failures = []
    for q in QUANTITIES:
        err_twin = flow_ref.rel_l2(data["twin"][q], data["ref"][q])
        err_kernel = flow_ref.rel_l2(data["kernel"][q], data["ref"][q])
        print(f"{IDS[SHAPES.index(shape)]} {q}: kernel {err_kernel:.3e} twin {err_twin:.3e}")
        if not err_kernel <= 2.0 * err_twin + 1e-6:
            failures.append((q, err_kernel, err_twin))
    assert not failures, failures


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_runs_are_byte_identical(shape):
    data = case(shape)
    for q in QUANTITIES:
        assert data["kernel"][q].tobytes() == data["again"][q].tobytes(), q


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_predict_is_the_two_ops_composed(shape):
    n, h, w, c, m, sigma0 = shape
    data = case(shape)
    x, flow, g = (torch.from_numpy(data[k]).cuda() for k in ("x", "flow", "g"))
    composed = lambda a, f: flow_ops.scale_space_warp(flow_ops.gaussian_scale_space(a, m, sigma0), f)
    out, (gx, gflow) = _grads(composed, [x, flow], g)
    assert out.cpu().numpy().tobytes() == data["kernel"]["predict"].tobytes()
    assert gx.cpu().numpy().tobytes() == data["kernel"]["predict_gx"].tobytes()
    assert gflow.cpu().numpy().tobytes() == data["kernel"]["predict_gflow"].tobytes()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_zero_and_nan_output_gradient(shape):
    n, h, w, c, m, sigma0 = shape
    data = case(shape)
    x, flow, vol = (torch.from_numpy(data[k]).cuda() for k in ("x", "flow", "vol32"))
    zero = torch.zeros(n, h, w, c, device="cuda")
    _, (gv, gflow) = _grads(flow_ops.scale_space_warp, [vol, flow], zero)
    assert not gv.any() and not gflow.any()
    _, (gx, gflow) = _grads(lambda a, f: flow_ops.scale_space_predict(a, f, m, sigma0), [x, flow], zero)
    assert not gx.any() and not gflow.any()
    bad = torch.from_numpy(data["g"]).cuda()
    bad.view(-1)[bad.numel() // 2] = float("nan")
    _, (gv, gflow) = _grads(flow_ops.scale_space_warp, [vol, flow], bad)
    assert bool(torch.isnan(gv).all()) and bool(torch.isnan(gflow).all())
    _, (gx, gflow) = _grads(lambda a, f: flow_ops.scale_space_predict(a, f, m, sigma0), [x, flow], bad)
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(gflow).all())
    # and nothing else: the inputs are untouched, the next call is clean
    assert torch.equal(vol.cpu(), torch.from_numpy(data["vol32"]))
    _, (gv, _) = _grads(flow_ops.scale_space_warp, [vol, flow], torch.from_numpy(data["g"]).cuda())
    assert gv.cpu().numpy().tobytes() == data["kernel"]["warp_gv"].tobytes()


def test_non_finite_flow_follows_the_definition():
    """NaN, +-inf and +-1e30 in the flow: the kernel clamps with fminf(fmaxf(raw, 0), last) (ss_axis in
    csrc/scale_space.hip), so a NaN coordinate is 0, an infinite or huge one an edge, and the flow gradient there 0."""
    shape = SHAPES[1]
    n, h, w, c, m, sigma0 = shape
    data = case(shape)
    flow = data["flow"].copy()
    special = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
    spots = []
    for k, value in enumerate(special):
        for comp in range(3):
            i, j = (2 * k + comp) % h, (k + 2 * comp) % w
            flow[k % n, i, j, comp] = value
            spots.append((k % n, i, j, comp))
    vol32, g = data["vol32"], data["g"]
    want = flow_ref.warp(vol32, flow)
    want_gv, want_gflow = flow_ref.warp_gradients(vol32, flow, g)
    assert np.isfinite(want).all() and np.isfinite(want_gflow).all()
    t = lambda a, dev: torch.from_numpy(a).to(dev)
    res = {}
    for dev, fn in (("cpu", flow_ops.scale_space_warp_reference), ("cuda", flow_ops.scale_space_warp)):
        out, (gv, gflow) = _grads(fn, [t(vol32, dev), t(flow, dev)], t(g, dev))
        res[dev] = [a.cpu().numpy() for a in (out, gv, gflow)]
    for name, k, ref in (("out", 0, want), ("gv", 1, want_gv), ("gflow", 2, want_gflow)):
        err_twin, err_kernel = flow_ref.rel_l2(res["cpu"][k], ref), flow_ref.rel_l2(res["cuda"][k], ref)
        print(f"non-finite flow {name}: kernel {err_kernel:.3e} twin {err_twin:.3e}")
        assert err_kernel <= 2.0 * err_twin + 1e-6, name
    for spot in spots:
        assert res["cuda"][2][spot] == 0.0, spot


def test_backward_bound_and_cabi_errors():
    """The host-side checks of the C entries: a textual error, nothing launched."""
    from compression_amd import _lib
    lib = _lib.lib()
    assert lib.tfc_scale_space_workspace(2, 7, 5, 3, 5) == 8 * 2 * 6 * 7 * 5 * 3
    assert lib.tfc_scale_space_workspace(1, 7, 5, 9, 5) == -1 and "channels" in _lib.last_error()
    assert lib.tfc_scale_space_workspace(1, 7, 5, 3, 9) == -1 and "num_levels" in _lib.last_error()
    assert lib.tfc_scale_space_workspace(1, 1 << 15, 5, 3, 2) == -1 and "H and W" in _lib.last_error()
    assert lib.tfc_scale_space_workspace(1 << 20, 64, 64, 3, 5) == -1 and "2^31" in _lib.last_error()
    x = torch.zeros(1, 4, 4, 1, device="cuda")
    vol = torch.zeros(1, 3, 4, 4, 1, device="cuda")
    st = _lib.stream_ptr()
    assert lib.tfc_scale_space_volume(x.data_ptr(), vol.data_ptr(), 1, 4, 4, 1, 2, 0.0, st) != 0
    assert "sigma0" in _lib.last_error()
    assert lib.tfc_scale_space_volume(x.data_ptr(), vol.data_ptr(), 1, 4, 4, 1, 2, 40.0, st) != 0
    assert lib.tfc_scale_space_volume(x.data_ptr() + 4, vol.data_ptr(), 1, 4, 4, 1, 2, 1.0, st) != 0
    assert "aligned" in _lib.last_error()
    assert lib.tfc_scale_space_volume(0, vol.data_ptr(), 1, 4, 4, 1, 2, 1.0, st) != 0 and "null" in _lib.last_error()
    assert lib.tfc_scale_space_volume(0, 0, 0, 4, 4, 1, 2, 1.0, st) == 0            # N == 0 launches nothing
    # the scatter's H W <= 2^22 bound is checked before anything is touched (the pointers are never read)
    big = (1 << 11) + 1
    assert lib.tfc_scale_space_warp_backward(x.data_ptr(), 0, x.data_ptr(), 0, vol.data_ptr(), 0, 1.0, 1, 1 << 11, big,
                                             1, 1, st) != 0
    assert "2^22" in _lib.last_error()
    torch.cuda.synchronize()
