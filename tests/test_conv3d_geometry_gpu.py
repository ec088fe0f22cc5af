"""GPU tier of the rank-3 geometry cases (tests/conv_probe_data.py, GEOMETRY_CASES_3D and WGRAD_CASES_3D;
tests/test_conv3d_geometry_cpu.py asserts the data's conditions and, from tfc_conv3d_plan / tfc_conv3d_wgrad_plan, that
every case reaches the branch of csrc/signal_conv3d.hip it is there for — repeated here first, on the library under test).

Every comparison is EQUALITY with the float64 oracle (signal_conv_oracle.layer_oracle and its autograd); no tolerance.
  float32 forward    the three plane probes of conv_probe_data: every product a multiple of 2^-18, the abs-sum per output
                     below 2^4, so every partial sum is exact in float32 in any order
  bfloat16 forward   values in {-1, 0, +1} on both sides: each one bfloat16, every sum an integer below 16
  weight gradient    float32: x and gy of 2 + 2, 3 + 1 and 1 + 3 digits (products multiples of 2^-18, abs-sum below 2^4);
                     bfloat16: {-1, 0, +1} on both sides
A wrong tile origin, a stage that is skipped or summed twice, a chunk offset, a channel tile written to the wrong place
or a pack that reads the wrong plane changes a result by at least 2^-18."""
import pytest
import torch

import conv_probe_data as pd
import test_conv3d_geometry_cpu as geometry
from test_conv_probes_gpu import check_probe, layer

pytestmark = pytest.mark.gpu

PROBES = list(pd.PROBES)
GUARD = 4096                                         # elements before and after an output that must stay untouched
SENTINEL = 1000.0                                    # one bfloat16; no probe output reaches it (abs-sums are below 16)


@pytest.fixture(autouse=True)
def default_float32_route(monkeypatch):
    monkeypatch.delenv("TFC_CONV_F32", raising=False)
    monkeypatch.delenv("TFC_CONV_F32_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("TFC_CONV_GEN", raising=False)


def assert_equal(got, want):
    assert tuple(got.shape) == tuple(want.shape)
    got = got.detach().float().cpu().double()
    wrong = got != want
    assert torch.equal(got, want), (int(wrong.sum()), float((got - want).abs().max()), wrong.nonzero()[:4].tolist())


def test_every_case_reaches_its_branch_in_the_library_under_test():
    for c in pd.GEOMETRY_CASES_3D:
        geometry.assert_forward_plan(c)
    for c in pd.WGRAD_CASES_3D:
        geometry.assert_wgrad_plan(c)


@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("c", pd.GEOMETRY_CASES_3D, ids=pd.case_id)
def test_float32_forward_equals_the_oracle_on_plane_probes(c, probe):
    check_probe(c, probe)


@pytest.mark.parametrize("c", pd.GEOMETRY_CASES_3D, ids=pd.case_id)
def test_bfloat16_forward_equals_the_oracle_on_one_level_data(c):
    x, w, want = pd.one_level_data(c)
    assert float(pd.abs_sum(c, x, w).max()) < pd.ABS_SUM_BOUND
    assert float((want != 0).double().mean()) >= 0.5
    with torch.no_grad():
        got = layer(c)(x.bfloat16().cuda(), w.cuda())
    assert got.dtype == torch.bfloat16
    assert_equal(got, want)


@pytest.mark.parametrize("probe", PROBES)
def test_float32_integer_bias_and_relu_behind_a_partial_last_column_block(probe):
    """Seven column blocks of 32, the last with 8 channels: the bias is read at blk > 0 and the epilogue's co < Cout cut."""
    c = pd.GEOMETRY_BIAS_RELU_CASE
    check_probe(c, probe, pd.integer_bias(c, probe), "relu")


def test_float32_in_chunks_of_images_equals_the_default_budget(monkeypatch):
    """conv3d_entry's loop over chunks of images (n0 > 0: the offsets of x and y) under TFC_CONV_F32_CHUNK_BYTES: three
    chunks of one image; a chunk of two, then one."""
    c = pd.GEOMETRY_CHUNKED_CASE
    assert c["n"] == 3
    x, w, want = pd.probe_data(c, "x12_w12")
    d, h, wd = c["extent"]
    image_planes = d * h * wd * 6 * c["cin"] * 2
    with torch.no_grad():
        default = layer(c)(x.cuda(), w.cuda())
        assert_equal(default, want)
        for images in (1, 2):
            monkeypatch.setenv("TFC_CONV_F32_CHUNK_BYTES", str(images * image_planes))
            got = layer(c)(x.cuda(), w.cuda())
            assert_equal(got, want)
            assert torch.equal(got, default)


def wgrad_args(c, x, gy):
    """conv3d_wgrad's (a, b, transpose) of layer case c: down (x, gy, False), up (gy, x, True)."""
    return (gy, x, True) if c["up"] else (x, gy, False)


def check_wgrad(c, levels, dtype):
    from compression_amd.layers import functional
    x, gy, want, abs_dw = pd.wgrad_data(c, levels)
    assert float(abs_dw.max()) < pd.ABS_SUM_BOUND
    assert float((want != 0).double().mean()) >= 0.5
    a, b, transpose = wgrad_args(c, x.to(dtype).cuda(), gy.to(dtype).cuda())
    got = functional.conv3d_wgrad(a, b, c["support"], c["strides"], transpose)
    again = functional.conv3d_wgrad(a, b, c["support"], c["strides"], transpose)
    assert got.dtype == torch.float32
    assert_equal(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("levels", list(pd.WGRAD_LEVELS))
@pytest.mark.parametrize("c", pd.WGRAD_CASES_3D, ids=pd.case_id)
def test_float32_weight_gradient_equals_the_oracle(c, levels):
    """Several 64-pixel stages per chunk, a shorter last chunk whose last stage is cut, 2 x 3 / 2 x 2 channel tiles with
    the last of each side partly outside (80 = 64 + 16, 144 = 128 + 16), CA != CB through the transposed store.  The
    float32 kernel accumulates on mfma_f32_32x32x2f32: that it adds multiples of 2^-18 below 2^4 without error is what
    this equality holds it to (it does, on an MI355X)."""
    check_wgrad(c, levels, torch.float32)


@pytest.mark.parametrize("c", pd.WGRAD_CASES_3D, ids=pd.case_id)
def test_bfloat16_weight_gradient_equals_the_oracle_on_one_level_data(c):
    check_wgrad(c, "one_level", torch.bfloat16)


@pytest.mark.parametrize("c", pd.WGRAD_CASES_3D, ids=pd.case_id)
def test_layer_kernel_gradient_equals_the_oracle_at_unequal_channel_counts(c):
    """Through _ConvFunction.backward: which of x and gy is `a`, which `b`, and `transpose`, at CA != CB."""
    x, gy, want, _ = pd.wgrad_data(c, "x2_g2")
    kernel = torch.zeros(c["support"] + (c["cin"], c["cout"]), device="cuda", requires_grad=True)
    y = layer(c)(x.cuda(), kernel)
    assert tuple(y.shape) == tuple(gy.shape)
    y.backward(gy.cuda())
    assert kernel.grad.dtype == torch.float32
    assert_equal(kernel.grad, want)


def guarded(numel, dtype):
    """-> (buffer of GUARD + numel + GUARD sentinels, its middle `numel` elements)."""
    buffer = torch.full((2 * GUARD + numel,), SENTINEL, dtype=dtype, device="cuda")
    return buffer, buffer[GUARD:GUARD + numel]


def assert_guards_untouched(buffer, numel):
    assert bool((buffer[:GUARD] == SENTINEL).all()) and bool((buffer[GUARD + numel:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("name", ["down3d-133-h2-w129", "up1d-5-s2-w131"])
def test_forward_writes_nothing_outside_its_output(name, dtype):
    """The C entry on an output that is a slice of a larger buffer of sentinels: a one-sample last W tile (129 = 128 + 1)
    with a second H tile, and two phases over two W tiles."""
    from compression_amd import _lib
    c = pd._BY_NAME[name]
    x, w, want = pd.probe_data(c, "x12_w12") if dtype == torch.float32 else pd.one_level_data(c)
    xg, wg = x.to(dtype).cuda().contiguous(), w.cuda().contiguous()
    buffer, y = guarded(want.numel(), dtype)
    fn = _lib.lib().tfc_conv3d_up if c["up"] else _lib.lib().tfc_conv3d_down
    _lib.check(fn(xg.data_ptr(), wg.data_ptr(), None, y.data_ptr(), _lib.DTYPE_CODE[dtype], c["n"], *c["extent"], c["cin"],
                  c["cout"], *c["support"], *c["strides"], 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert_guards_untouched(buffer, want.numel())
    assert_equal(y.reshape(want.shape), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_weight_gradient_writes_nothing_outside_its_output(dtype):
    from compression_amd import _lib
    c = pd.WGRAD_CASES_3D[0]
    assert not c["up"] and c["cin"] % 16 == 0 and c["cout"] % 16 == 0           # no channel padding: the entry as it is
    x, gy, want, _ = pd.wgrad_data(c, "x2_g2" if dtype == torch.float32 else "one_level")
    a, b = x.to(dtype).cuda().contiguous(), gy.to(dtype).cuda().contiguous()
    buffer, dw = guarded(want.numel(), torch.float32)
    _lib.check(_lib.lib().tfc_conv3d_wgrad(
        a.data_ptr(), b.data_ptr(), dw.data_ptr(), _lib.DTYPE_CODE[dtype], c["n"], *a.shape[1:],
        *b.shape[1:], *c["support"], *c["strides"], 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert_guards_untouched(buffer, want.numel())
    assert_equal(dw.reshape(want.shape), want)
