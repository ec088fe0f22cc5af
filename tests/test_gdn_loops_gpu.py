"""GPU tier: the GDN / IGDN kernels (csrc/gdn_common.h, gdn_backward.hip, reduce_rows.h) where their persistent loops
repeat and at their edges, against the float64 definition of tests/gdn_ref.py.

Sizes come from the device.  With cus compute units the grids are capped at cus blocks, so a wave of the float32
kernels and of the fused bfloat16 backward (4 waves a block) takes a second 32-pixel tile above 32 * 4 * cus pixels,
one of the bfloat16 forward (8 waves) above 32 * 8 * cus, a block of the parameter-gradient kernel a second 64-pixel
stage above 64 * cus, and sum_rows_kernel (16 row slices) more than one row per slice above 16 blocks.
P_LOOP = 64 * 4 * cus + 231 (65767 on the MI355X) is past all of them with a ragged last tile and a ragged last stage:
2-3 tiles per wave, 4-5 stages per block, cus partial rows.  test_loop_size_repeats_every_loop asserts that.

(a) Exact family, no tolerance.  IGDN with eps = 1 has T = g x' — no division.  With x in {0, -0.0, +-1, +-2}, g in
    {+-1, +-2}, beta = 1 and Gamma in multiples of 2^-6 up to 2^-3 every product and sum is exact in float32 whatever
    the order (tests/test_gdn_ref_cpu.py proves it for these very input sets), and T, u are exact in bfloat16: dbeta
    and dGamma equal float64, and for float32 y and dx too.  (Equal as numbers: -0.0 == 0.0.)
(b) y and dx of a pixel depend on that pixel alone: about 300 rows of the P_LOOP tensor — first, last, either side of
    the tile boundaries of the second and third loop iteration, the last 40, some at random — are bit for bit what a
    second call on just those rows gives.  Every forward build and both backward paths.
(c) Random data (x with exact zeros), every variant, at P_LOOP: for y, dx, dbeta and dGamma
        err_kernel <= 2 * err_twin + 1e-6
    in relative L2 against float64, the twin being gdn_ref.twin (float32, or with the kernels' bfloat16 roundings):
    the bar of tests/test_lvac_gpu.py.  2: other summation orders and the hardware's 1-ulp rcp / rsq / sqrt; 1e-6: the
    project's float32 slack.  Float32 GDN outputs keep the 1e-5 absolute bar of tests/test_gdn_gpu.py as well.  Every
    call is made twice and must repeat byte for byte (gdn_backward.hip: "deterministic, no float atomics").

Worst (err_kernel, err_twin) per output over the cases of (c), measured on the MI355X (P_LOOP = 65767):
                 y                     dx                    dbeta                 dGamma
    float32      (1.04e-07, 1.05e-07)  (9.26e-08, 9.31e-08)  (3.83e-07, 2.48e-07)  (3.50e-07, 4.45e-07)
    bfloat16     (1.73e-03, 1.73e-03)  (2.47e-03, 2.47e-03)  (1.89e-03, 1.89e-03)  (2.42e-03, 2.42e-03)
The bfloat16 kernels never exceed their twin by more than 3 % (dbeta 1.59e-03 against 1.55e-03): the roundings are
where the twin has them.  Float32 dbeta reaches 2.3 times its twin (3.14e-07 against 1.39e-07) and passes on the 1e-6.
The largest float32 GDN |y - want| is 7.9e-07 against the 1e-5 bar.
"""
import functools

import numpy as np
import pytest
import torch

import gdn_ref
from compression_amd.layers import functional
from compression_amd.layers import gdn_backward, gdn_forward

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
PAIRS = [(False, 1), (False, 0.5), (True, 1), (True, 0.5)]          # (inverse, eps)
RECT_ALPHA = [(False, 1), (True, 2), (True, 1), (False, 2)]         # (rectify, alpha); the first is the PLAIN build
ROW_SLICES = 16                                                     # reduce_rows.h kRowSlices


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def p_loop():
    return gdn_ref.p_loop(cus())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def test_loop_size_repeats_every_loop():
    P = p_loop()
    for name, threshold in gdn_ref.loop_thresholds(cus()).items():
        assert P > threshold, (name, P, threshold)
    assert min(-(-P // 64), cus()) > ROW_SLICES             # sum_rows_kernel: rows = the parameter kernel's blocks
    assert P % 32 and P % 64                                # ragged last tile, ragged last stage
    assert -(-P // 32) > 2 * 4 * cus()                      # a third tile for some waves of the 4-wave kernels
    assert -(-P // 64) > 4 * cus()                          # a fifth stage for some blocks


# -- (a) the exact family -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def exact_set(pixels, C, dtype):
    x, g, beta, gamma = gdn_ref.exact_inputs(pixels, C, seed=pixels + C)
    dev = tuple(t.to(DTYPES[dtype]).cuda() for t in (x, g)) + (beta.cuda(), gamma.cuda())
    return tuple(t.numpy() for t in (x, g, beta, gamma)), dev


def check_exact(pixels, C, dtype):
    host, (x, g, beta, gamma) = exact_set(pixels, C, dtype)
    for rectify, alpha in gdn_ref.EXACT_VARIANTS:
        want = gdn_ref.grads(*host, inverse=True, rectify=rectify, alpha=alpha, eps=1)
        # (no summation order can round: the bound of tests/test_gdn_ref_cpu.py at this device's size)
        assert pixels * np.abs(want["u"]).max() * np.abs(want["T"]).max() < 2 ** 24
        dx, dbeta, dgamma = gdn_backward(x, g, beta, gamma, True, rectify, alpha, 1)
        where = (dtype, pixels, C, rectify, alpha)
        assert np.array_equal(dbeta.cpu().numpy().astype(np.float64), want["dbeta"]), ("dbeta",) + where
        assert np.array_equal(dgamma.cpu().numpy().astype(np.float64), want["dgamma"]), ("dgamma",) + where
        if dtype == "float32":
            y = gdn_forward(x, beta, gamma, True, rectify, alpha, 1)
            assert np.array_equal(y.cpu().numpy().astype(np.float64), want["y"]), ("y",) + where
            assert np.array_equal(dx.cpu().numpy().astype(np.float64), want["dx"]), ("dx",) + where


@pytest.mark.parametrize("C", gdn_ref.EXACT_SMALL_CHANNELS)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_exact_family_small_sizes(dtype, C):
    """One pixel, around one tile and one stage, and 16, 16 and 18 partial rows for sum_rows_kernel (exactly one row
    a slice, and two rows in some slices with others empty)."""
    for pixels in gdn_ref.EXACT_SMALL_PIXELS:
        check_exact(pixels, C, dtype)


@pytest.mark.parametrize("dtype,C", [(d, c) for d in sorted(DTYPES) for c in gdn_ref.EXACT_LOOP_CHANNELS[d]])
def test_exact_family_loop_size(dtype, C):
    """bfloat16: the fused kernel with odd and even KT (32 ... 192) and the three-pass path (224, 256)."""
    check_exact(p_loop(), C, dtype)


# -- (b) a pixel's outputs do not depend on its tile ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sampled_rows():
    P, rows = p_loop(), {0, 1, 31, 32, 33}
    rows.update(range(P - 40, P))
    # second and third iteration of the 4-wave kernels; the latter is the second of the 8-wave bfloat16 forward
    for start in (32 * 4 * cus(), 2 * 32 * 4 * cus()):
        for tile in range(16):
            edge = start + 32 * tile
            rows.update((edge - 2, edge - 1, edge, edge + 1))
    rows.update(np.random.default_rng(7).integers(0, P, 130).tolist())
    rows = sorted(r for r in rows if 0 <= r < P)
    assert 250 <= len(rows) <= 350
    return torch.tensor(rows, device="cuda")


@functools.lru_cache(maxsize=2)
def random_set(C, dtype):
    x, g = gdn_ref.random_inputs(p_loop(), C, seed=C, bf16=dtype == "bfloat16")
    beta, gamma = gdn_ref.params(C, C + 1)
    return (x, g, beta, gamma), (x.to(DTYPES[dtype]).cuda(), g.to(DTYPES[dtype]).cuda(), beta.cuda(), gamma.cuda())


PLAIN_FORWARD = [(False, 1, False), (False, 0.5, False), (True, 1, False), (False, 1, True), (True, 0.5, True),
                 (True, 0.5, False)]                                # (inverse, eps, prepared parameters)
FORWARD_CHANNELS = [("float32", c) for c in (64, 96, 160, 192)] + [("bfloat16", c) for c in (32, 96, 160, 192, 224, 256)]


@pytest.mark.parametrize("i,dtype,C", [(i,) + dc for i, dc in enumerate(FORWARD_CHANNELS)])
def test_forward_rows_do_not_depend_on_their_tile(i, dtype, C):
    """Each channel count runs its three builds — PLAIN, general (rectify, alpha 2) and learned exponents — with the
    (inverse, eps, prepared) settings spread over the channel counts."""
    _, (x, _, beta, gamma) = random_set(C, dtype)
    rows = sampled_rows()
    xs = x[rows].contiguous()
    inverse, eps, prepared = PLAIN_FORWARD[i % len(PLAIN_FORWARD)]
    prep = functional.GDNPrepared(beta, gamma, x.dtype) if prepared else None
    inv2, eps2 = PAIRS[(i + 1) % 4]
    calls = [("plain", dict(inverse=inverse, epsilon=eps, prepared=prep)),
             ("rectify alpha 2", dict(inverse=inv2, epsilon=eps2, rectify=True, alpha=2)),
             ("exponents 1.5 / 0.7", dict(inverse=bool(i & 1), rectify=True, alpha=1.5, epsilon=0.7))]
    for name, kw in calls:
        big = gdn_forward(x, beta, gamma, **kw)
        small = gdn_forward(xs, beta, gamma, **kw)
        assert bool(torch.isfinite(small.float()).all()) and bool((small != 0).any())
        assert same_bytes(big[rows], small), (name, dtype, C, kw)


BACKWARD_CHANNELS = [("float32", c) for c in (64, 96, 160, 192)] + [
    ("bfloat16", c) for c in (32, 96, 128, 160, 192, 224, 256)]      # fused up to 192, three passes above


@pytest.mark.parametrize("i,dtype,C", [(i,) + dc for i, dc in enumerate(BACKWARD_CHANNELS)])
def test_backward_dx_rows_do_not_depend_on_their_tile(i, dtype, C):
    _, (x, g, beta, gamma) = random_set(C, dtype)
    rows = sampled_rows()
    xs, gs = x[rows].contiguous(), g[rows].contiguous()
    for (inverse, eps), (rectify, alpha) in ((PAIRS[i % 4], (False, 1)), (PAIRS[(i + 2) % 4], (True, 2))):
        big = gdn_backward(x, g, beta, gamma, inverse, rectify, alpha, eps)[0]
        small = gdn_backward(xs, gs, beta, gamma, inverse, rectify, alpha, eps)[0]
        assert bool(torch.isfinite(small.float()).all()) and bool((small != 0).any())
        assert same_bytes(big[rows], small), (dtype, C, inverse, eps, rectify, alpha)


# -- (c) random data against float64 --------------------------------------------------------------------------------

def spread(channels):
    """Four variants per channel count: every (inverse, eps) pair, every (rectify, alpha) setting, shifted from one
    channel count to the next — all sixteen combinations over four channel counts."""
    return [(C,) + PAIRS[k] + RECT_ALPHA[(k + i) % 4] for i, C in enumerate(channels) for k in range(4)]


RANDOM_CASES = [("bfloat16",) + v for v in spread(gdn_ref.EXACT_LOOP_CHANNELS["bfloat16"])] + [
    ("float32",) + v for v in spread(gdn_ref.EXACT_LOOP_CHANNELS["float32"])] + [
    ("float32", 64) + PAIRS[k] + RECT_ALPHA[(k + 3) % 4] for k in range(4)]     # float32's fourth shift


def bar(err_kernel, err_twin):
    return err_kernel <= 2.0 * err_twin + 1e-6


@pytest.mark.parametrize("dtype,C,inverse,eps,rectify,alpha", RANDOM_CASES)
def test_random_data_against_float64(dtype, C, inverse, eps, rectify, alpha):
    bf16 = dtype == "bfloat16"
    (x, g, beta, gamma), (xd, gd, bd, gamd) = random_set(C, dtype)
    assert 1 / 24 < float((x == 0).float().mean()) < 1 / 12
    gam_ref = gamma.bfloat16().float() if bf16 else gamma             # what the bfloat16 kernels contract with
    want = gdn_ref.grads(x.numpy(), g.numpy(), beta.numpy(), gam_ref.numpy(), inverse, rectify, alpha, eps)
    twin = gdn_ref.twin(x, g, beta, gamma, inverse, rectify, alpha, eps, bf16=bf16)

    def run():
        y = gdn_forward(xd, bd, gamd, inverse, rectify, alpha, eps)
        return (y,) + tuple(gdn_backward(xd, gd, bd, gamd, inverse, rectify, alpha, eps))

    got, again = run(), run()
    names = ("y", "dx", "dbeta", "dgamma")
    for name, a, b in zip(names, got, again):
        assert same_bytes(a, b), f"{name}: two runs differ"
    got = {name: a.float().cpu().numpy() for name, a in zip(names, got)}
    errs = {name: (gdn_ref.rel_l2(got[name], want[name]), gdn_ref.rel_l2(twin[name], want[name])) for name in names}
    print(f"gdn {dtype} C={C} inverse={inverse} eps={eps} rectify={rectify} alpha={alpha}: "
          + "  ".join(f"{k} kernel {ek:.2e} twin {et:.2e}" for k, (ek, et) in errs.items()))
    if not bf16 and not inverse:
        absolute = np.abs(got["y"] - want["y"]).max()
        print(f"    max |y - want| = {absolute:.3e}")
        assert absolute <= 1e-5
    for name, (ek, et) in errs.items():
        assert bar(ek, et), (name, ek, et)

