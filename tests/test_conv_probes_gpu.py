"""GPU tier of the convolution probes (tests/conv_probe_data.py; tests/test_conv_probes_cpu.py proves the data's power).

Float32 layers on the bfloat16 matrix cores.  Probe values sign * sum_k d_k 2^(-9 k), d_k in {0, 1}: with a 9-bit digit
spacing split3 puts the i-th non-zero digit in plane i, so probe x12_w12 makes exactly the plane products 0, 1, 3, 4 of
[x1 x1 x1 x2 x2 x3] x [w1 w2 w3 w1 w2 w1] non-zero, x123_w1 the products 0, 3, 5 and x1_w123 the products 0, 1, 2; a
product that is dropped, or read from the wrong plane, in either statement of the layout (conv_split_x_kernel /
conv_split_w_kernel; x_plane / w_plane of the rank-3 pack) changes a result.  Every kept product is a multiple of
2^-18 and the per-output sum of |x| |w| (the float64 oracle on absolute values, asserted per case) is below 2^4: every
partial sum fits 22 bits, and the float32 output must EQUAL the float64 oracle — no tolerance.  Densities 2.4 / sqrt(K)
per case; the largest abs-sums the oracle reported (4 ... 11) are tabulated in conv_probe_data's docstring.

bfloat16 layers' rounding of their float32 weights.  Impulse responses: x is zeros with isolated ones, the weights are
full-mantissa float32 with planted ties, near-ties and their negatives; each output is 0 or ONE weight, so the bfloat16
output must EQUAL the oracle on w.bfloat16().float() (round to nearest, ties to even) — truncation, another tie rule
or a pack that rounds twice changes it.  One case per packing kernel, at the smallest channel count its route takes."""
import pytest
import torch

import conv_probe_data as pd

pytestmark = pytest.mark.gpu

PROBES = list(pd.PROBES)


@pytest.fixture(autouse=True)
def default_float32_route(monkeypatch):
    monkeypatch.delenv("TFC_CONV_F32", raising=False)                 # the six-plane path
    monkeypatch.delenv("TFC_CONV_F32_CHUNK_BYTES", raising=False)
    monkeypatch.delenv("TFC_CONV_GEN", raising=False)


def layer(c):
    from compression_amd.layers import conv2d_down, conv2d_up, functional
    if len(c["extent"]) == 3:
        fn = functional.conv3d_up if c["up"] else functional.conv3d_down
        return lambda x, w, bias=None, activation=None: fn(x, w, bias, c["strides"], activation)
    fn = conv2d_up if c["up"] else conv2d_down
    return lambda x, w, bias=None, activation=None: fn(x, w, bias, c["strides"][0], activation)


def check_probe(c, probe, bias=None, activation=None):
    x, w, want = pd.probe_data(c, probe)
    if bias is not None:
        want = pd.oracle(c, x, w, bias, activation)
    assert float(pd.abs_sum(c, x, w, bias).max()) < pd.ABS_SUM_BOUND
    assert float((want != 0).double().mean()) >= (0.5 if activation is None else 0.25)
    with torch.no_grad():
        got = layer(c)(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), activation)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    got = got.cpu().double()
    wrong = got != want
    assert torch.equal(got, want), (int(wrong.sum()), float((got - want).abs().max()))


# route_f32_planes admits every case here (float32, Cin % 16 == 0, Cout % 4 == 0, 6 Cin taps < 2^24) and hands ONE
# bfloat16 convolution over 6 Cin channels with float32 output to route_gemm (out_f32 keeps the transposed few-channel
# routes out).  Which inner kernel that is:
#   down-3x3-16-8, down-4x4s2-16-40   run_conv3 declines (Cout is neither 128 nor 192): second generation, one and two
#                                     column tiles, the second an even kernel with a partly filled tile
#   up-5x5s2-64-4                     second generation, transposed: 16 columns of one tile (F32_SPLIT_CASES' partly filled
#                                     column tile); Cout % 32 != 0, so K is not compacted per phase
#   up-5x5s2-16-8                     the same with 16 input channels: one channel block per plane
#   down-5x5s2-16-128-blocks          run_conv3 takes it: Cout 128, stride 2, a 16 x 64 output map (small_down), 2 x 2 blocks
#                                     of 32 x 8 pixels, all inside the map; 25 taps on the large patch loader; float32 out
#   up-5x5s2-16-128-blocks            run_conv3, transposed x2: a 16 x 64 input map = 2 x 2 blocks, phase groups of
#                                     9 / 6 / 6 / 4 taps on the small patch loader; float32 out
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("c", pd.PLANE_CASES_2D, ids=pd.case_id)
def test_float32_rank2_equals_the_oracle_on_plane_probes(c, probe):
    check_probe(c, probe)


# conv3d_entry runs every float32 call as six planes (the 2-D layer's conv_split_x_kernel, conv3d_pack_kernel by w_plane with
# planes == 6): supports (3, 3, 3) and (1, 1, 5), strides (1, 1, 1) and (1, 2, 2), both directions; the transposed
# (1, 2, 2) case has four phases with their own tap sets, the (1, 1, 5) rows are wider than one 32-sample tile row.
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("c", pd.PLANE_CASES_3D, ids=pd.case_id)
def test_float32_rank3_equals_the_oracle_on_plane_probes(c, probe):
    check_probe(c, probe)


@pytest.mark.parametrize("probe", PROBES)
def test_float32_integer_bias_and_relu_on_plane_probes(probe):
    """The epilogue behind the planes: an integer bias (counted in the abs-sum) and the fused ReLU."""
    c = pd.BIAS_RELU_CASE
    check_probe(c, probe, pd.integer_bias(c, probe), "relu")


def test_float32_plane_probe_in_several_chunks_of_images(monkeypatch):
    """route_f32_planes' loop over chunks of images (TFC_CONV_F32_CHUNK_BYTES = one image's planes: three chunks), the
    six-plane weights packed once for all of them."""
    c = pd.CHUNKED_CASE
    h, w = c["extent"]
    monkeypatch.setenv("TFC_CONV_F32_CHUNK_BYTES", str(h * w * 6 * c["cin"] * 2))
    check_probe(c, "x12_w12")


# The input gradient is the OTHER direction's kernel on the cotangent with the kernel's channel axes swapped, Cin = Cout
# = 16: the gradient of a down layer runs the transposed second-generation / rank-3 kernel on six planes of gy, that of
# an up layer the correlation.  gy is drawn from the x-side grid, the kernel from the w-side grid.  The two rank-1 cases
# (261 and 131 samples, 32 <-> 16 channels) are wider than one 128-sample tile: dx of grad-down1d-5-s2-w261 runs the
# transposed kernel's two phases over two W tiles, dx of grad-up1d-5-s2-w131 the stride-2 correlation over two.
@pytest.mark.parametrize("probe", PROBES)
@pytest.mark.parametrize("c", pd.GRADIENT_CASES, ids=pd.case_id)
def test_float32_input_gradient_equals_the_oracle_on_plane_probes(c, probe):
    x, w, gy, dx, abs_dx = pd.gradient_data(c, probe)
    assert float(abs_dx.max()) < pd.ABS_SUM_BOUND
    assert float((dx != 0).double().mean()) >= 0.5
    xg = x.cuda().requires_grad_(True)
    y = layer(c)(xg, w.cuda())
    assert tuple(y.shape) == tuple(gy.shape)
    y.backward(gy.cuda())
    got = xg.grad.cpu().double()
    assert torch.equal(got, dx), (int((got != dx).sum()), float((got - dx).abs().max()))


# Which route's eligibility test admits each impulse case (all bfloat16), and the kernel that rounds its weights:
#   gemm2-down-3x3-16-8, gemm2-down-4x4s2-16-40   route_gemm, run_conv3 declines (Cout): second generation, conv_pack_kernel
#   gemm2-up-5x5s2-16-8               the same, transposed (Cout 8 > 4 keeps route_up_gather out); K not compacted
#   gemm2-up-compact-5x5s2-16-192     Cout 192 = one six-tile group per phase: compact K; a 9 x 13 map is one block, which
#                                     run_conv3 declines below TFC_CONV_GEN=4
#   gemm3-down-5x5s2-16-128, gemm3-up-5x5s2-32-128   run_conv3 under TFC_CONV_GEN=4 (the channel-block-major pack), 2 x 2
#                                     blocks; transposed, the four-tap phase is one chunk per channel block and the
#                                     weights are requested two chunks ahead: two channel blocks, Cin 32, at the least
#   up-fused-5x5s2-64-2               route_up_fused: Cin % 64 == 0, Cout <= 4, 50 product columns <= 84
#                                     (conv_up_fused_weights_kernel).  64 -> 3 at 5x5 x2 is route_up_phase's, which is
#                                     asked first; two output channels leave it to this route
#   up-gather-5x5s2-16-3              route_up_gather: Cin 16 is no multiple of 32 or 64 (conv_up_weights_kernel, then the
#                                     1x1 product's own pack of the already rounded values)
#   up-phase-5x5s2-64-3, up-phase-9x9s4-32-3   route_up_phase: Cout 3, Cin / 32 a multiple of 2 chunks (5x5) / 1 (9x9)
#                                     (conv_up_phase_weights_kernel<5, 2> / <9, 4>)
#   image-5x5s2-3-128                 route_image: Cin 3, Cout 128 (route_image_direct wants 192), a row of one 32-pixel tile
#   image-direct-5x5s2-3-192, image-direct-9x9s4-3-192   route_image_direct: Cout 192, output rows of whole 32-pixel
#                                     tiles, W a multiple of the stride (conv_image_weights_kernel, both kernel sizes)
#   gemm1-image-9x9s4-3-32            Cout 32: neither image route; route_gemm's first generation on the packed image
#                                     (conv_pack_kernel's small_cin order)
#   down3d-335-s122, up3d-335-s122    conv3d_pack_kernel with planes == 1, both directions
@pytest.mark.parametrize("c", pd.IMPULSE_CASES, ids=pd.case_id)
def test_bfloat16_weights_are_rounded_to_nearest_even_once(c, monkeypatch):
    x, w, _, want = pd.impulse_data(c)
    if c["name"].startswith("gemm3"):
        monkeypatch.setenv("TFC_CONV_GEN", "4")
    with torch.no_grad():
        got = layer(c)(x.cuda(), w.cuda())
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(want.shape)
    got = got.float().cpu().double()
    wrong = got != want
    assert torch.equal(got, want), (int(wrong.sum()), got[wrong][:4].tolist(), want[wrong][:4].tolist())
