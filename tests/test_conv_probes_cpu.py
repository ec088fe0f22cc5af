"""CPU tier of the convolution probes (tests/conv_probe_data.py): proves, with no device, that the data the GPU tier
feeds the kernels can tell a wrong plane from a right one, and a wrong weight rounding from round-to-nearest-even.

Plane probes.  Values sign * sum_k d_k 2^(-9 k), d_k in {0, 1}: at a 9-bit digit spacing split3 puts the i-th non-zero
digit of a value in plane i.  `emulate` is the six-plane scheme in numpy / torch — split3 by torch's bfloat16 cast, the
plane tables RESTATED in conv_probe_data (x planes [1 1 1 2 2 3], w planes [1 2 3 1 2 1]; an edit of x_plane / w_plane
in csrc/conv_shared.h is not mirrored here), six float32 matrix products over the im2col of the float64 oracle's padded
input, float32 accumulation.  Probe x12_w12 isolates products 0, 1, 3, 4, x123_w1 adds 5 (x3 w1), x1_w123 adds 2
(x1 w3).  For every case and probe: the planes sum back to the value and exactly the intended ones are non-zero; the
per-output sum of |x| |w| (the oracle on absolute values) stays below 2^4, so all partial sums are multiples of 2^-18
in 22 bits and the emulation must EQUAL the oracle; leaving out a product the probe claims changes the result, leaving
out any other does not; the three probes together claim all six.  Densities are 2.4 / sqrt(K) (0.268 at K = 80 down to
0.1 at K = 576); the largest abs-sums the oracle reported for them are tabulated in conv_probe_data's docstring.

Impulse responses.  The conditions under which a bfloat16 layer's output must equal the oracle on weights rounded to
nearest even: no output sees two impulses, every weight element reaches an output, and the weights tell the rounding
rules apart: truncation on a third of them at least; of the planted ties those with an even kept bit differ from
round-half-away and those with an odd one from truncation (no tie can differ from both); rounding twice shows one
float32 unit below a tie — and each of the three wrong rules changes the oracle's output on this x."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_probe_data as pd
import signal_conv_oracle as so


def split3(a):
    """csrc/conv_shared.h split3, with torch's CPU bfloat16 cast (round to nearest even)."""
    p1 = a.bfloat16().float()
    r1 = a - p1
    p2 = r1.bfloat16().float()
    return p1, p2, (r1 - p2).bfloat16().float()


def im2col(c, x):
    """The geometry of signal_conv_oracle.layer_oracle as a matrix: -> patches [N, *out, taps Cin] in x's dtype, to be
    multiplied with weight_matrix(c, kernel)."""
    from compression_amd.ops.padding_ops import same_padding_for_kernel
    args = pd.oracle_args(c)
    k, sd, su = c["support"], args["strides_down"], args["strides_up"]
    rank = len(k)
    x = x.movedim(-1, 1)
    prepad = same_padding_for_kernel(k, args["corr"], su)
    x = F.pad(x, [p for pair in reversed(prepad) for p in pair])
    crop = None
    if all(s == 1 for s in su) and (args["corr"] or all(s % 2 == 1 for s in k)):
        step = sd
    else:
        u = x.new_zeros(tuple(x.shape[:2]) + tuple(n * s for n, s in zip(x.shape[2:], su)))      # extra_pad_end
        u[(slice(None), slice(None)) + tuple(slice(None, None, s) for s in su)] = x
        x = F.pad(u, [k[a] - 1 for a in reversed(range(rank)) for _ in range(2)])
        step = (1,) * rank
        full = [x.shape[2 + a] - k[a] + 1 for a in range(rank)]
        crop = tuple(slice(prepad[a][0] * su[a] + k[a] // 2, full[a] - (prepad[a][1] * su[a] + (k[a] - 1) // 2), sd[a])
                     for a in range(rank))
    for a in range(rank):
        x = x.unfold(2 + a, k[a], step[a])                     # [N, C, *out, *k]
    if crop is not None:
        x = x[(slice(None), slice(None)) + crop]
    x = x.permute(0, *range(2, 2 + 2 * rank), 1)               # [N, *out, *k, C]
    return x.reshape(tuple(x.shape[:1 + rank]) + (-1,))


def weight_matrix(c, kernel):
    rank = len(c["support"])
    w = kernel if not c["up"] else kernel.flip(*range(rank))   # convolution = correlation with the mirrored kernel
    return w.reshape(-1, kernel.shape[-1])


def emulate(c, x, kernel, drop=()):
    """The six-plane float32 layer: sum over the kept products q of (x plane X_PLANE[q]) (w plane W_PLANE[q]), each a
    float32 matrix product, accumulated in float32; `drop`: products left out."""
    xs = [im2col(c, p) for p in split3(x)]
    ws = [weight_matrix(c, p) for p in split3(kernel)]
    y = torch.zeros(tuple(xs[0].shape[:-1]) + (kernel.shape[-1],), dtype=torch.float32)
    for q in range(6):
        if q not in drop:
            y = y + xs[pd.X_PLANE[q]] @ ws[pd.W_PLANE[q]]
    assert y.dtype == torch.float32
    return y.double()


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_nine_bit_digits_land_in_one_plane_each(levels):
    v = pd.probe_values((4096,), levels, 0.9, np.random.default_rng(levels))
    planes = split3(v)
    assert torch.equal(planes[0].double() + planes[1].double() + planes[2].double(), v.double())
    for i, p in enumerate(planes):
        assert bool(p.any()) == (i < levels)
        nz = p[p != 0].abs().log2()
        assert torch.equal(nz, nz.round())                     # one digit: a power of two
    full = torch.tensor([1 + 2.0 ** -9 + 2.0 ** -18, -(1 + 2.0 ** -9)])
    assert [p.tolist() for p in split3(full)] == [[1.0, -1.0], [2.0 ** -9, -2.0 ** -9], [2.0 ** -18, 0.0]]
    # an 8-bit spacing would not do: the value rounds up and its remainder is one bfloat16
    assert not split3(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -16]))[2].any()


def test_the_probes_claim_all_six_products_and_none_of_the_discarded():
    claimed = set()
    for x_levels, w_levels, products in pd.PROBES.values():
        live = tuple(q for q in range(6) if pd.X_PLANE[q] < x_levels and pd.W_PLANE[q] < w_levels)
        assert live == products
        claimed.update(products)
        # x2 w3, x3 w2, x3 w3 need x_levels + w_levels >= 5 with both above 1
        assert not any(i < x_levels and j < w_levels for i, j in ((1, 2), (2, 1), (2, 2)))
    assert claimed == set(range(6))
    assert sorted(zip(pd.X_PLANE, pd.W_PLANE)) == sorted((i, j) for i in range(3) for j in range(3) if i + j <= 2)


@pytest.mark.parametrize("probe", list(pd.PROBES))
@pytest.mark.parametrize("c", pd.PLANE_CASES, ids=pd.case_id)
def test_probe_data_is_exact_and_isolates_its_products(c, probe):
    x, w, want = pd.probe_data(c, probe)
    x_levels, w_levels, products = pd.PROBES[probe]
    for value, levels in ((x, x_levels), (w, w_levels)):
        planes = split3(value)
        assert torch.equal(sum(p.double() for p in planes), value.double())
        assert [bool(p.any()) for p in planes] == [i < levels for i in range(3)]
    largest = float(pd.abs_sum(c, x, w).max())
    share = float((want != 0).double().mean())
    print(f"{c['name']} {probe}: K {pd.products_per_output(c)} density {pd.density_for(pd.products_per_output(c)):.3f} "
          f"largest abs-sum {largest:.3f} non-zero outputs {share:.3f}")
    assert largest < pd.ABS_SUM_BOUND
    assert share >= 0.5
    assert torch.equal(im2col(c, x.double()) @ weight_matrix(c, w.double()), want)      # the geometry is the oracle's
    assert torch.equal(emulate(c, x, w), want)
    for q in range(6):
        assert torch.equal(emulate(c, x, w, drop=(q,)), want) == (q not in products), q


def test_integer_bias_and_relu_keep_the_probe_exact():
    c = pd.BIAS_RELU_CASE
    for probe in pd.PROBES:
        x, w, _ = pd.probe_data(c, probe)
        bias = pd.integer_bias(c, probe)
        want = pd.oracle(c, x, w, bias, "relu")
        assert float(pd.abs_sum(c, x, w, bias).max()) < pd.ABS_SUM_BOUND
        assert float((want != 0).double().mean()) >= 0.25 and bool((pd.oracle(c, x, w, bias) < 0).any())
        assert torch.equal(torch.relu(emulate(c, x, w) + bias.double()), want)


@pytest.mark.parametrize("probe", list(pd.PROBES))
@pytest.mark.parametrize("c", pd.GRADIENT_CASES, ids=pd.case_id)
def test_gradient_probe_is_exact_and_isolates_its_products(c, probe):
    """dx is the other direction's layer on the cotangent with the kernel's channel axes swapped: the emulation of THAT
    layer on (gy, w^T) must equal the oracle's autograd, cropped to x where the transposed layer overshoots."""
    x, w, gy, dx, abs_dx = pd.gradient_data(c, probe)
    products = pd.PROBES[probe][2]
    largest, share = float(abs_dx.max()), float((dx != 0).double().mean())
    print(f"{c['name']} {probe}: largest abs-sum {largest:.3f} non-zero gradients {share:.3f}")
    assert largest < pd.ABS_SUM_BOUND and share >= 0.5
    other = dict(c, up=not c["up"], cin=c["cout"], cout=c["cin"], extent=tuple(gy.shape[1:-1]))
    crop = (slice(None),) + tuple(slice(n) for n in c["extent"])
    for q in (None,) + tuple(range(6)):
        got = emulate(other, gy, w.transpose(-1, -2), drop=() if q is None else (q,))[crop]
        assert torch.equal(got, dx) == (q is None or q not in products), q


@pytest.mark.parametrize("c", pd.IMPULSE_CASES, ids=pd.case_id)
def test_impulse_data_reads_out_every_weight_once(c):
    x, w, ties, want = pd.impulse_data(c)
    xf = x.float()
    assert set(xf.unique().tolist()) == {0.0, 1.0}
    # no output receives two impulses
    assert float(pd.oracle(c, xf, torch.ones_like(w)).max()) <= 1.0
    # every weight element reaches some output
    kernel = torch.zeros_like(w, dtype=torch.float64).requires_grad_(True)
    pd.oracle(c, xf, kernel).sum().backward()
    assert bool((kernel.grad > 0).all())
    # so every output is 0 or one rounded weight
    rne = w.bfloat16().float()
    assert bool(torch.isin(want, torch.cat([rne.double().reshape(-1), torch.zeros(1, dtype=torch.float64)])).all())
    # and the weights tell the rounding rules apart
    assert float((pd.truncated(w) != rne).double().mean()) >= 1 / 3
    flat, away = w.reshape(-1), pd.rounded_half_away(w).reshape(-1)
    # (planted in turn with an even and an odd kept bit: half-even rounds the first down, where half-away goes up, and
    # the second up, where truncation goes down — one tie cannot differ from both)
    even, odd = ties[0::2], ties[1::2]
    assert bool((away[even] != rne.reshape(-1)[even]).all())
    assert bool((away[odd] == rne.reshape(-1)[odd]).all())
    assert bool((pd.truncated(w).reshape(-1)[odd] != rne.reshape(-1)[odd]).all())
    assert bool((rne.reshape(-1)[ties] != flat[ties]).all())
    assert torch.equal(pd.rounded_twice(rne), rne)
    for wrong in (pd.truncated(w), pd.rounded_half_away(w), pd.rounded_twice(w)):       # each would show in the output
        assert not torch.equal(wrong, rne)
        assert not torch.equal(pd.oracle(c, xf, wrong), want)


def test_oracle_arguments_are_the_functional_layers_definition():
    """conv_probe_data.oracle_args against the references the existing GPU tests hold the same entry points to
    (test_signal_conv_gpu.ref_down / ref_up, test_conv3d_gpu.ref_down / ref_up), on integers."""
    import test_conv3d_gpu as t3
    import test_signal_conv_gpu as t2
    for c in pd.PLANE_CASES_2D[:4] + pd.PLANE_CASES_3D:
        x, w, _ = so.integer_data(dict(input_support=c["extent"], channels=c["cin"], filters=c["cout"],
                                       kernel_support=c["support"], channel_separable=False, use_bias=False), 3, c["n"] or 1)
        if len(c["extent"]) == 2:
            ref = (t2.ref_up if c["up"] else t2.ref_down)(x.double(), w.double(), None, c["strides"][0], False)
        else:
            ref = (t3.ref_up if c["up"] else t3.ref_down)(x, w, None, c["strides"], False)
        assert torch.equal(pd.oracle(c, x, w), ref), c["name"]
