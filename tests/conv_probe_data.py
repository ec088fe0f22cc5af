"""Data that is exact by construction for two places where small integers are blind (tests/test_conv_probes_cpu.py
proves its power without a device, tests/test_conv_probes_gpu.py runs it on the kernels).

1. Plane probes: the float32 layers on the bfloat16 matrix cores (csrc/conv_shared.h split3, x_plane / w_plane; the
   literal plane[6] of conv_split_w_kernel).  A float32 operand is split into three bfloat16 planes and six of the nine
   plane products are kept, q = 0 ... 5: x planes [1 1 1 2 2 3] against w planes [1 2 3 1 2 1].  An integer below 256 is
   one bfloat16, so five of the six products are zero in every integer test.

   A probe value is  sign * sum_k d_k 2^(-9 k),  d_k in {0, 1}, k < levels, a random sign, zero with probability
   1 - density.  The digit spacing is 9 bits: a bfloat16 keeps 8 significant bits, the next digit is below half a unit
   of the leading one, so split3 rounds DOWN to the leading digit and leaves the rest — the i-th non-zero digit of a
   value is its plane i (1 + 2^-9 + 2^-18 -> 1, 2^-9, 2^-18), and a value of `levels` digits has no plane beyond
   `levels`.  (At 8 bits 1 + 2^-8 + 2^-16 rounds up, and the remainder fits one bfloat16: plane 3 stays empty.)

       probe      x levels  w levels  products that are not identically zero
       x12_w12    2         2         0, 1, 3, 4   (x1 w1, x1 w2, x2 w1, x2 w2)
       x123_w1    3         1         0, 3, 5      (adds x3 w1)
       x1_w123    1         3         0, 1, 2      (adds x1 w3)

   The three products the scheme discards (x2 w3, x3 w2, x3 w3) are identically zero for all three.  Every kept product
   is a multiple of 2^-18; where the sum of absolute values per output — the float64 oracle on |x|, |w| (and |bias|),
   the way test_signal_conv_grad_gpu.check_module forms abs_y — is below ABS_SUM_BOUND = 2^4, every partial sum in any
   order is a multiple of 2^-18 below 2^4: 22 bits, two to spare in float32.  The float32 result must then EQUAL the
   float64 oracle.  The bound is a condition on the data, asserted for every case; it is no tolerance.

   Density: 2.4 / sqrt(K), K the products an output sums (taps x Cin; behind an upsampling the taps of one phase at the
   most, ceil(k / s) per axis) — about 5.8 non-zero candidates per output at every K.  Largest abs-sum the oracle
   reported over the three probes of the cases below, and the smallest share of non-zero outputs (required: above a
   half):

       K      density  largest abs-sum  non-zero outputs   cases
       80     0.268    8.0              0.88               rank 3, support (1, 1, 5), both directions
       144    0.200    9.0              0.71               3x3 16 -> 8, transposed 5x5 x2 16 -> 8 and 16 -> 128
       192    0.173    6.0              0.55               rank 3 transposed, support (3, 3, 3) x (1, 2, 2)
       256    0.150    10.0             0.73               4x4 /2 16 -> 40, and its three-image batch
       400    0.120    11.0             0.88               5x5 /2 16 -> 128
       432    0.115    7.0              0.79               rank 3, support (3, 3, 3)
       576    0.100    6.0              0.70               transposed 5x5 x2 64 -> 4

   (The transposed cases count the taps of the fullest phase; the other phases sum fewer products, hence their lower
   shares.)  The input-gradient cases, on |gy|, |w|: 8.0 at the most, 0.55 non-zero at the least.  The ten
   GEOMETRY_CASES_3D (K 48 ... 1296, densities 0.346 ... 0.067): 10.02 at the most, 0.54 non-zero at the least.

2. Impulse responses: the bfloat16 kernels' rounding of their float32 weights (pack_bf16 and the casts of the packing
   kernels).  x is bfloat16 zeros with isolated ones, the weights are full-mantissa float32, the oracle runs on
   w.bfloat16().float() (torch's CPU cast rounds to nearest, ties to even).  No output receives two impulses, so each
   output is 0 or one rounded weight and the bfloat16 output must EQUAL the oracle; every weight element reaches some
   output.  Planted among normal weights: exact ties (2 m + 1) 2^-8 2^e with both parities of the kept bit m, one
   float32 unit either side of each, and the negatives of all of these."""
import functools
import math

import numpy as np
import torch

import signal_conv_oracle as so

SPACING = 9                              # bits between a probe value's digits
ABS_SUM_BOUND = 16.0                     # per output, of |x| |w| (+ |bias|): every partial sum then fits 22 bits
# the six kept plane products, restated (not read from the library): x plane, w plane of product q, counted from 0
X_PLANE = (0, 0, 0, 1, 1, 2)
W_PLANE = (0, 1, 2, 0, 1, 0)
PROBES = {                               # name -> (x levels, w levels, products that are not identically zero)
    "x12_w12": (2, 2, (0, 1, 3, 4)),
    "x123_w1": (3, 1, (0, 3, 5)),
    "x1_w123": (1, 3, (0, 1, 2)),
}


def case(name, up, n, extent, cin, cout, support, strides):
    return dict(name=name, up=up, n=n, extent=tuple(extent), cin=cin, cout=cout, support=tuple(support),
                strides=tuple(strides))


def case_id(c):
    return c["name"]


def oracle_args(c):
    """What conv2d_down / conv3d_down (correlation, `same_zeros`, strides down) and conv2d_up / conv3d_up (transposed
    convolution, `same_zeros`, extra_pad_end) compute, in signal_conv_oracle.layer_oracle's terms."""
    one = (1,) * len(c["extent"])
    return dict(corr=not c["up"], strides_down=one if c["up"] else c["strides"],
                strides_up=c["strides"] if c["up"] else one, padding="same_zeros", extra_pad_end=True)


def oracle(c, x, w, bias=None, activation=None):
    return so.layer_oracle(x, w, bias=bias, activation=activation, **oracle_args(c))


def abs_sum(c, x, w, bias=None):
    """Per output the sum of |x| |w| over its products, plus |bias|: the float64 oracle on the absolute values."""
    return oracle(c, x.abs(), w.abs(), None if bias is None else bias.abs())


def products_per_output(c, channels=None):
    taps = math.prod(-(-k // s) for k, s in zip(c["support"], c["strides"])) if c["up"] else math.prod(c["support"])
    return taps * (c["cin"] if channels is None else channels)


def density_for(k):
    return 2.4 / math.sqrt(k)


def probe_values(shape, levels, density, rng):
    digits = rng.integers(0, 2, (levels,) + tuple(shape))
    magnitude = sum(digits[k] * 2.0 ** (-SPACING * k) for k in range(levels))
    sign = rng.choice([-1.0, 1.0], tuple(shape))
    keep = rng.random(tuple(shape)) < density
    return torch.from_numpy((sign * magnitude * keep).astype(np.float32))


def _seed(c, probe, salt=0):
    return sum(map(ord, c["name"] + probe)) * 7 + salt


@functools.lru_cache(maxsize=None)
def _probe_data(key, probe):
    c = _BY_NAME[key]
    x_levels, w_levels, _ = PROBES[probe]
    rng = np.random.default_rng(_seed(c, probe))
    density = density_for(products_per_output(c))
    x = probe_values((c["n"],) + c["extent"] + (c["cin"],), x_levels, density, rng)
    w = probe_values(c["support"] + (c["cin"], c["cout"]), w_levels, density, rng)
    return x, w, oracle(c, x, w)


def probe_data(c, probe):
    """-> (x channels-last float32, kernel [*support, Cin, Cout] float32, the float64 oracle's output), made once."""
    return _probe_data(c["name"], probe)


def integer_bias(c, probe):
    """Integers in -3 ... 3: exact in every plane-1 sum, and counted in the abs-sum condition."""
    rng = np.random.default_rng(_seed(c, probe, 1))
    return torch.from_numpy(rng.integers(-3, 4, (c["cout"],)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _gradient_data(key, probe):
    """The input gradient is the other direction's kernel on the cotangent: the cotangent from the x-side grid, the
    kernel from the w-side grid -> (x, kernel, gy, the oracle's dx, the abs-sum of dx: the oracle's autograd on |gy|, |w|)."""
    c = _BY_NAME[key]
    x_levels, w_levels, _ = PROBES[probe]
    rng = np.random.default_rng(_seed(c, probe, 2))
    other = dict(c, up=not c["up"])
    density = density_for(products_per_output(other, c["cout"]))
    w = probe_values(c["support"] + (c["cin"], c["cout"]), w_levels, density, rng)
    x = probe_values((c["n"],) + c["extent"] + (c["cin"],), 1, density, rng)
    xd = x.double().requires_grad_(True)
    y = oracle(c, xd, w)
    gy = probe_values(tuple(y.shape), x_levels, density, rng)
    y.backward(gy.double())
    xa = x.double().requires_grad_(True)
    oracle(c, xa, w.abs()).backward(gy.abs().double())
    return x, w, gy, xd.grad, xa.grad


def gradient_data(c, probe):
    return _gradient_data(c["name"], probe)


# ---- the cases of the float32 tier (the GPU file says per case which route's eligibility test admits it) -------------
PLANE_CASES_2D = [
    case("down-3x3-16-8", False, 1, (9, 11), 16, 8, (3, 3), (1, 1)),
    case("down-4x4s2-16-40", False, 1, (10, 7), 16, 40, (4, 4), (2, 2)),
    case("up-5x5s2-64-4", True, 1, (8, 7), 64, 4, (5, 5), (2, 2)),
    case("up-5x5s2-16-8", True, 1, (7, 9), 16, 8, (5, 5), (2, 2)),
    case("down-5x5s2-16-128-blocks", False, 1, (32, 128), 16, 128, (5, 5), (2, 2)),
    case("up-5x5s2-16-128-blocks", True, 1, (16, 64), 16, 128, (5, 5), (2, 2)),
]
CHUNKED_CASE = case("down-4x4s2-16-40-three-images", False, 3, (20, 20), 16, 40, (4, 4), (2, 2))
PLANE_CASES_3D = [
    case("down3d-333-s111", False, 1, (4, 6, 9), 16, 16, (3, 3, 3), (1, 1, 1)),
    case("down3d-115-s122", False, 2, (3, 8, 37), 16, 16, (1, 1, 5), (1, 2, 2)),
    case("up3d-333-s122", True, 1, (3, 5, 7), 16, 16, (3, 3, 3), (1, 2, 2)),
    case("up3d-115-s111", True, 2, (2, 3, 35), 16, 16, (1, 1, 5), (1, 1, 1)),
]
GRADIENT_CASES = [
    case("grad-down-5x5s2-16-16", False, 1, (9, 12), 16, 16, (5, 5), (2, 2)),
    case("grad-up-5x5s2-16-16", True, 1, (6, 7), 16, 16, (5, 5), (2, 2)),
    case("grad-down3d-333-s122", False, 1, (3, 6, 9), 16, 16, (3, 3, 3), (1, 2, 2)),
    case("grad-up3d-115-s122", True, 1, (2, 4, 19), 16, 16, (1, 1, 5), (1, 2, 2)),
]
GRADIENT_CASES += [
    # dx of the first runs the transposed rank-3 kernel with two phases over two W tiles, dx of the second the correlation
    case("grad-down1d-5-s2-w261", False, 1, (1, 1, 261), 32, 16, (1, 1, 5), (1, 1, 2)),
    case("grad-up1d-5-s2-w131", True, 1, (1, 1, 131), 16, 32, (1, 1, 5), (1, 1, 2)),
]
BIAS_RELU_CASE = PLANE_CASES_2D[1]

# ---- the rank-3 kernels' tile, block and chunk structure (csrc/signal_conv3d.hip) -----------------------------------
# Shapes chosen from the host's rule, which tfc_conv3d_plan reports: GEOMETRY_PLANS holds what each case must reach,
# and tests/test_conv3d_geometry_cpu.py asserts it from the library, so a retune that moves a case off its branch fails
# there and names the case.
GEOMETRY_CASES_3D = [
    case("down1d-5-s1-w300", False, 2, (1, 1, 300), 16, 32, (1, 1, 5), (1, 1, 1)),
    case("down1d-5-s2-w261", False, 1, (1, 1, 261), 32, 16, (1, 1, 5), (1, 1, 2)),
    case("up1d-5-s2-w131", True, 1, (1, 1, 131), 16, 32, (1, 1, 5), (1, 1, 2)),
    case("down3d-333-h5-w40-c128", False, 2, (2, 5, 40), 16, 128, (3, 3, 3), (1, 1, 1)),
    case("down3d-133-h2-w129", False, 1, (1, 2, 129), 32, 32, (1, 3, 3), (1, 1, 1)),
    case("down3d-199-h6-w70", False, 1, (1, 6, 70), 16, 32, (1, 9, 9), (1, 1, 1)),
    case("down3d-177-h3-w70-c128", False, 1, (1, 3, 70), 16, 128, (1, 7, 7), (1, 1, 1)),
    case("down3d-333-s122-c200", False, 1, (2, 6, 70), 16, 200, (3, 3, 3), (1, 2, 2)),
    case("up3d-335-s122-c72", True, 1, (2, 3, 70), 32, 72, (3, 3, 5), (1, 2, 2)),
    case("up3d-333-s212-w33", True, 3, (2, 3, 33), 16, 16, (3, 3, 3), (2, 1, 2)),
]
# name -> the plan fields the case is there for (TW, TH: the tile; NT: 32-column tiles per workgroup; nblk: column
# blocks; tiles_w, tiles_h; phases), and what follows from them:
#   last_tile_w   samples of the last W tile that are inside the row (of a phase's output grid)
#   last_tile_h   rows of the last H tile that are inside
#   last_blk_cols output channels of the last column block (of 32 NT)
#   tw_from, nt_from   what the row length / Cout alone would pick, where the LDS loops narrow it
#   lds_over_half True: the stage is above half the LDS (one workgroup per CU)
#   f32_cblocks_per_plane  16-channel blocks per plane in float32 (above 1: a pack that took the plane from the channel
#                 block would be wrong)
GEOMETRY_PLANS = {
    "down1d-5-s1-w300": dict(TW=128, TH=1, tiles_w=3, tiles_h=1, phases=1, last_tile_w=44),
    "down1d-5-s2-w261": dict(TW=128, tiles_w=2, phases=1, last_tile_w=3, f32_cblocks_per_plane=2),
    "up1d-5-s2-w131": dict(TW=128, tiles_w=2, phases=2, last_tile_w=3),
    "down3d-333-h5-w40-c128": dict(TW=64, TH=2, tiles_w=1, tiles_h=3, last_tile_h=1, NT=4, nblk=1, phases=1),
    "down3d-133-h2-w129": dict(TW=128, TH=1, tiles_w=2, tiles_h=2, last_tile_w=1, phases=1),
    "down3d-199-h6-w70": dict(tw_from=128, TW=32, TH=4, tiles_w=3, tiles_h=2, lds_over_half=True, phases=1),
    "down3d-177-h3-w70-c128": dict(nt_from=4, NT=1, nblk=4, TW=128, lds_over_half=False, phases=1),
    "down3d-333-s122-c200": dict(NT=1, nblk=7, last_blk_cols=8, TW=64, TH=2, phases=1),
    "up3d-335-s122-c72": dict(phases=4, NT=3, nblk=1, last_blk_cols=72, TW=128, TH=1, tiles_h=3),
    "up3d-333-s212-w33": dict(phases=4, TW=64, TH=2, tiles_w=1, tiles_h=2, last_tile_h=1),
}
GEOMETRY_BIAS_RELU_CASE = GEOMETRY_CASES_3D[7]               # the bias is read at blk > 0, the last column block is partial
GEOMETRY_CHUNKED_CASE = GEOMETRY_CASES_3D[9]                 # three images
assert set(GEOMETRY_PLANS) == {c["name"] for c in GEOMETRY_CASES_3D}

# Weight gradient: G[t][ca][cb] = sum over B's P pixels.  `up` as the layer's direction: down calls
# conv3d_wgrad(x, gy, ..., False) (A = x carries Cin, B = gy), up calls conv3d_wgrad(gy, x, ..., True) (A = gy carries
# Cout, B = x).  WGRAD_PLANS: what tfc_conv3d_wgrad_plan must report (pixels = P, stages of 64 pixels).
WGRAD_CASES_3D = [
    case("wgrad-down-335-s122-80-144", False, 2, (3, 18, 74), 80, 144, (3, 3, 5), (1, 2, 2)),
    case("wgrad-up-355-s122-128-80", True, 2, (2, 13, 33), 128, 80, (3, 5, 5), (1, 2, 2)),
]
WGRAD_PLANS = {
    "wgrad-down-335-s122-80-144": dict(pixels=1998, ca=80, cb=144, tiles_ca=2, tiles_cb=3, chunks=16, chunk_steps=2,
                                       pixels_in_last_chunk=78),
    "wgrad-up-355-s122-128-80": dict(pixels=1716, ca=80, cb=128, tiles_ca=2, tiles_cb=2, chunks=14, chunk_steps=2,
                                     pixels_in_last_chunk=52),
}
WGRAD_LEVELS = {"x2_g2": (2, 2), "x3_g1": (3, 1), "x1_g3": (1, 3)}       # float32: digits of x, of gy
# One-level data (values in {-1, 0, +1}: each one bfloat16, every sum an integer below 16, hence one bfloat16) for the
# bfloat16 kernels.  Sums of +-1 cancel to exactly zero far more often than sums of several digits do: at
# density_for(K) the forward cases have 0.35 ... 0.66 non-zero outputs (six of the ten below a half; the lowest are the
# transposed cases, whose thinner phases sum fewer products), at density_for(P) the two weight gradients 0.55 and 0.49.
# The abs-sum has room, so these probes draw denser: ONE_LEVEL_DENSITY / sqrt(K) forward, WGRAD_ONE_LEVEL_DENSITY /
# sqrt(P) for the weight gradient.  Measured (tests/test_conv3d_geometry_cpu.py prints them):
#
#       case                          K / P  density  largest abs-sum  non-zero outputs
#       down1d-5-s1-w300              80     0.402    12.0             0.766
#       down1d-5-s2-w261              160    0.285    12.0             0.774
#       up1d-5-s2-w131                48     0.520    11.0             0.734
#       down3d-333-h5-w40-c128        432    0.173    10.0             0.653
#       down3d-133-h2-w129            288    0.212    9.0              0.699
#       down3d-199-h6-w70             1296   0.100    10.0             0.690
#       down3d-177-h3-w70-c128        784    0.129    7.0              0.598
#       down3d-333-s122-c200          432    0.173    10.0             0.686
#       up3d-335-s122-c72             576    0.150    9.0              0.549
#       up3d-333-s212-w33             192    0.260    10.0             0.551
#       wgrad-down-335-s122-80-144    1998   0.0626   11.0             0.620
#       wgrad-up-355-s122-128-80      1716   0.0676   10.0             0.564
#
# and, float32, the level pairs of WGRAD_LEVELS at density_for(P): abs-sums of at most 10.02, non-zero shares 0.74 ...
# 0.87.
ONE_LEVEL_DENSITY = 3.6
WGRAD_ONE_LEVEL_DENSITY = 2.8


def wgrad_geometry(c):
    """-> (extent of B's grid, CA, CB, P) of the weight gradient call of layer case c."""
    y_extent = tuple(n * s if c["up"] else -(-n // s) for n, s in zip(c["extent"], c["strides"]))
    b_extent = c["extent"] if c["up"] else y_extent
    ca, cb = (c["cout"], c["cin"]) if c["up"] else (c["cin"], c["cout"])
    return b_extent, ca, cb, c["n"] * math.prod(b_extent)


@functools.lru_cache(maxsize=None)
def _wgrad_data(key, levels):
    c = _BY_NAME[key]
    x_levels, g_levels = WGRAD_LEVELS.get(levels, (1, 1))
    pixels = wgrad_geometry(c)[3]
    density = density_for(pixels) if levels in WGRAD_LEVELS else WGRAD_ONE_LEVEL_DENSITY / math.sqrt(pixels)
    rng = np.random.default_rng(_seed(c, levels, 3))
    x = probe_values((c["n"],) + c["extent"] + (c["cin"],), x_levels, density, rng)
    shape = c["support"] + (c["cin"], c["cout"])
    w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    y = oracle(c, x.double(), w)
    gy = probe_values(tuple(y.shape), g_levels, density, rng)
    y.backward(gy.double())
    wa = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    oracle(c, x.abs().double(), wa).backward(gy.abs().double())
    return x, gy, w.grad, wa.grad


def wgrad_data(c, levels):
    """-> (x float32, gy float32, the oracle's kernel gradient [*support, Cin, Cout] of oracle(c, x, w) against gy (float64
    autograd), its abs-sum: the same on |x|, |gy|), made once.  levels: a key of WGRAD_LEVELS, or "one_level"."""
    return _wgrad_data(c["name"], levels)


@functools.lru_cache(maxsize=None)
def _one_level_data(key):
    c = _BY_NAME[key]
    rng = np.random.default_rng(_seed(c, "one_level"))
    density = ONE_LEVEL_DENSITY / math.sqrt(products_per_output(c))
    x = probe_values((c["n"],) + c["extent"] + (c["cin"],), 1, density, rng)
    w = probe_values(c["support"] + (c["cin"], c["cout"]), 1, density, rng)
    return x, w, oracle(c, x, w)


def one_level_data(c):
    """-> (x, kernel, the float64 oracle's output), x and kernel in {-1, 0, +1} (float32 tensors; each value one bfloat16)."""
    return _one_level_data(c["name"])


PLANE_CASES = PLANE_CASES_2D + [CHUNKED_CASE] + PLANE_CASES_3D + GEOMETRY_CASES_3D


# ---- impulse responses ---------------------------------------------------------------------------------------------
def impulse_input(c):
    """bfloat16 zeros with isolated ones on a lattice, cycling over the input channels and, in front of a stride, over
    the positions modulo the stride (a tap t of a strided correlation only meets inputs at p = o s + t - k // 2); as
    many images as the cycle needs.  Margins keep every tap of an impulse inside the output."""
    k, s, extent, cin = c["support"], c["strides"], c["extent"], c["cin"]
    rank = len(k)
    if c["up"]:
        pitch = [-(-k[a] // s[a]) for a in range(rank)]
        margin = [-(-(k[a] - 1) // s[a]) for a in range(rank)]
        residues = [(0,) * rank]
    else:
        pitch = [-(-(k[a] + s[a] - 1) // s[a]) * s[a] for a in range(rank)]      # a multiple of the stride: the residues stay
        margin = [k[a] - 1 for a in range(rank)]
        residues = list(np.ndindex(*s))
    counts = [(extent[a] - 2 * margin[a] - (0 if c["up"] else s[a] - 1) - 1) // pitch[a] + 1 for a in range(rank)]
    assert all(n >= 1 for n in counts), (c["name"], counts)
    sites = list(np.ndindex(*counts))
    needed = cin * len(residues)
    images = -(-needed // len(sites))
    x = torch.zeros((images,) + tuple(extent) + (cin,))
    for j in range(images * len(sites)):
        site, residue = sites[j % len(sites)], residues[(j // cin) % len(residues)]
        at = tuple(margin[a] + site[a] * pitch[a] + residue[a] for a in range(rank))
        x[(j // len(sites),) + at + (j % cin,)] = 1.0
    return x.bfloat16()


def _bits(a):
    return a.numpy().view(np.uint32)


def truncated(w):
    return torch.from_numpy((_bits(w) & np.uint32(0xFFFF0000)).view(np.float32))


def rounded_half_away(w):
    return torch.from_numpy(((_bits(w) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32))


def rounded_twice(w):
    """To nearest even at 16 mantissa bits first, then at bfloat16's 8: up through a tie from one unit below it."""
    def nearest_even(bits, drop):
        bits = bits + np.uint32((1 << (drop - 1)) - 1) + ((bits >> np.uint32(drop)) & np.uint32(1))
        return bits & ~np.uint32((1 << drop) - 1)
    return torch.from_numpy(nearest_even(nearest_even(_bits(w).copy(), 8), 16).view(np.float32))


def rounding_weights(shape, seed):
    """-> (float32 weights, flat indices of the planted exact ties).  Normal values with full mantissas; planted at
    random places over taps, input and output channels: ties (2 m + 1) 2^-8 2^e, m in 128 ... 255 of both parities
    (the kept bit), one float32 unit below and above each, and the negatives of all of them."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(shape).astype(np.float32)
    ties = np.array([(2 * m + 1) * 2.0 ** (e - 8) for e in (-5, -2, 0) for m in (128, 129, 170, 171, 254, 255)],
                    dtype=np.float32)
    below, above = np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(4))
    planted = np.concatenate([ties, -ties, below, -below, above, -above])
    assert planted.size <= w.size // 4
    at = rng.choice(w.size, planted.size, replace=False)
    w.reshape(-1)[at] = planted
    return torch.from_numpy(w), torch.from_numpy(at[:2 * ties.size])


IMPULSE_CASES = [
    case("gemm2-down-3x3-16-8", False, 0, (12, 20), 16, 8, (3, 3), (1, 1)),
    case("gemm2-down-4x4s2-16-40", False, 0, (24, 32), 16, 40, (4, 4), (2, 2)),
    case("gemm2-up-5x5s2-16-8", True, 0, (9, 13), 16, 8, (5, 5), (2, 2)),
    case("gemm2-up-compact-5x5s2-16-192", True, 0, (9, 13), 16, 192, (5, 5), (2, 2)),
    case("gemm3-down-5x5s2-16-128", False, 0, (32, 128), 16, 128, (5, 5), (2, 2)),
    case("gemm3-up-5x5s2-32-128", True, 0, (16, 64), 32, 128, (5, 5), (2, 2)),
    case("up-fused-5x5s2-64-2", True, 0, (9, 33), 64, 2, (5, 5), (2, 2)),
    case("up-gather-5x5s2-16-3", True, 0, (9, 13), 16, 3, (5, 5), (2, 2)),
    case("up-phase-5x5s2-64-3", True, 0, (11, 35), 64, 3, (5, 5), (2, 2)),
    case("up-phase-9x9s4-32-3", True, 0, (11, 35), 32, 3, (9, 9), (4, 4)),
    case("image-5x5s2-3-128", False, 0, (20, 64), 3, 128, (5, 5), (2, 2)),
    case("image-direct-5x5s2-3-192", False, 0, (20, 64), 3, 192, (5, 5), (2, 2)),
    case("image-direct-9x9s4-3-192", False, 0, (40, 128), 3, 192, (9, 9), (4, 4)),
    case("gemm1-image-9x9s4-3-32", False, 0, (40, 60), 3, 32, (9, 9), (4, 4)),
    case("down3d-335-s122", False, 0, (6, 14, 32), 16, 16, (3, 3, 5), (1, 2, 2)),
    case("up3d-335-s122", True, 0, (5, 5, 9), 16, 16, (3, 3, 5), (1, 2, 2)),
]


@functools.lru_cache(maxsize=None)
def _impulse_data(key):
    c = _BY_NAME[key]
    x = impulse_input(c)
    w, ties = rounding_weights(c["support"] + (c["cin"], c["cout"]), _seed(c, "impulse"))
    return x, w, ties, oracle(c, x.float(), w.bfloat16().float())


def impulse_data(c):
    """-> (x bfloat16, float32 weights, indices of the planted ties, the float64 oracle on the weights rounded to nearest
    even), made once."""
    return _impulse_data(c["name"])


# ---- the rank-2 weight gradient where its loops repeat (csrc/signal_conv_backward.hip, conv_wgrad_kernel) -----------
# A workgroup owns one tap and the 64-pixel stages chunk, chunk + chunks, ... of B's grid, chunks = max(1, min(stages,
# 2 CUs / taps)) — so what a shape reaches depends on the device, and tfc_conv2d_wgrad_plan is asked for it with the CU
# count as an argument: WGRAD_PLANS_2D is what it must report for 256 CUs (tests/test_conv2d_wgrad_cpu.py; the GPU tier
# asks again with the device's own count).  Each case is named for the branch it is there for:
#   loop-tr-*          both sides wide: bfloat16 runs the transposing-read build; three trips of the stage loop (the
#                      prefetch inside the loop, the barriers around stage_to_lds, the strided walk), a ragged last stage,
#                      HA = 65 < HB s = 66 (iy < HA); the `up` one transposes the store, KTA = 1 against KTB = 6
#   loop-narrowA-*     A has 3 channels (stage_narrow; B through pair_store in bfloat16), 81 taps, stride 4, odd extents
#   loop-8x8-*         the largest tile pair and LDS stage, WB = 64 (fast_div by a power of two), every stage full
#   one-chunk-*        529 taps: (2 CUs) / taps == 0, one workgroup per tap walks every stage
#   row-1x3-*          kh != kw (tap / kw, tap % kw), HB = 1 (fast_div by 1: mul == 0), 170 chunks
#   col-4x1s2-*        kh != kw the other way round with an even kh, WB = 1, two images (n = m / (WB HB)), HA = 8193 < 8194
#   even-4x2s2-*       even supports on both axes with kh != kw (k / 2 is not (k - 1) / 2), odd extents in front of stride 2
#   edges-p63/64/65    one partial stage, one exact stage, one pixel over (a second chunk of one pixel)
#   layer-*            through SignalConv2D: conv2d_wgrad's zero channels to 96 / 160 and its channel blocks (64 + 32,
#                      128 + 32) at the loop-tr size; every block pair has the plan below
# (A WB = 1 column with an even kw cannot meet the non-zero share asked of the data: ix = tx - kw / 2 is inside a one-
# or two-column A for at most half of the taps, so half of dw is structurally zero.  Hence a (4, 1) column and the even
# kw in a case of its own.)
WGRAD_CASES_2D = [
    case("loop-tr-5x5s2-64-128", False, 2, (65, 81), 64, 128, (5, 5), (2, 2)),
    case("loop-tr-up-5x5s2-192-32", True, 2, (33, 41), 192, 32, (5, 5), (2, 2)),
    case("loop-narrowA-9x9s4-3-64", False, 1, (97, 131), 3, 64, (9, 9), (4, 4)),
    case("loop-narrowA-up-9x9s4-64-3", True, 1, (25, 33), 64, 3, (9, 9), (4, 4)),
    case("loop-8x8-5x5s1-256-256", False, 1, (41, 64), 256, 256, (5, 5), (1, 1)),
    case("one-chunk-23x23-3-32", False, 1, (29, 37), 3, 32, (23, 23), (1, 1)),
    case("row-1x3-128-64", False, 1, (1, 21900), 128, 64, (1, 3), (1, 1)),
    case("col-4x1s2-32-64", False, 2, (8193, 1), 32, 64, (4, 1), (2, 2)),
    case("even-4x2s2-32-64", False, 1, (13, 19), 32, 64, (4, 2), (2, 2)),
    case("edges-p63-3x3-32-32", False, 1, (7, 9), 32, 32, (3, 3), (1, 1)),
    case("edges-p64-3x3-32-32", False, 1, (8, 8), 32, 32, (3, 3), (1, 1)),
    case("edges-p65-3x3-32-32", False, 1, (5, 13), 32, 32, (3, 3), (1, 1)),
]
WGRAD_LAYER_CASES_2D = [
    case("layer-80-144", False, 2, (65, 81), 80, 144, (5, 5), (2, 2)),
    case("layer-up-144-80", True, 2, (33, 41), 144, 80, (5, 5), (2, 2)),
]
WGRAD_LOOP_CASES_2D = [c for c in WGRAD_CASES_2D if c["name"].startswith("loop-")]
WGRAD_WIDE_LOOP_CASES_2D = [c for c in WGRAD_LOOP_CASES_2D if min(c["cin"], c["cout"]) >= 32]
# name -> what tfc_conv2d_wgrad_plan reports at 256 CUs: pixels = P, (ca, cb) the call's channel counts, the fields of
# functional.CONV2D_WGRAD_PLAN_FIELDS that do not depend on the dtype, then (tr, lds_bytes) for float32 and bfloat16.
# The layer cases: `blocks` = the (ca, cb) pairs conv2d_wgrad launches, which share everything but the tiles.
def _plan_2d(pixels, ca, cb, tiles_ca, tiles_cb, chunks, chunk_steps, pixels_in_last_stage, float32, bfloat16):
    return dict(pixels=pixels, ca=ca, cb=cb, tiles_ca=tiles_ca, tiles_cb=tiles_cb, chunks=chunks, chunk_steps=chunk_steps,
                pixels_in_last_stage=pixels_in_last_stage, float32=dict(zip(("tr", "lds_bytes"), float32)),
                bfloat16=dict(zip(("tr", "lds_bytes"), bfloat16)))


WGRAD_PLANS_2D = {
    "loop-tr-5x5s2-64-128": _plan_2d(2706, 64, 128, 2, 4, 20, 3, 18, (0, 49152), (1, 32768)),
    "loop-tr-up-5x5s2-192-32": _plan_2d(2706, 32, 192, 1, 6, 20, 3, 18, (0, 57344), (1, 32768)),
    "loop-narrowA-9x9s4-3-64": _plan_2d(825, 3, 64, 1, 2, 6, 3, 57, (0, 24576), (0, 13824)),
    "loop-narrowA-up-9x9s4-64-3": _plan_2d(825, 3, 64, 1, 2, 6, 3, 57, (0, 24576), (0, 13824)),
    "loop-8x8-5x5s1-256-256": _plan_2d(2624, 256, 256, 8, 8, 20, 3, 64, (0, 131072), (1, 73728)),
    "one-chunk-23x23-3-32": _plan_2d(1073, 3, 32, 1, 1, 1, 17, 49, (0, 16384), (0, 9216)),
    "row-1x3-128-64": _plan_2d(21900, 128, 64, 4, 2, 170, 3, 12, (0, 49152), (1, 32768)),
    "col-4x1s2-32-64": _plan_2d(8194, 32, 64, 1, 2, 128, 2, 2, (0, 24576), (1, 16384)),
    "even-4x2s2-32-64": _plan_2d(70, 32, 64, 1, 2, 2, 1, 6, (0, 24576), (1, 16384)),
    "edges-p63-3x3-32-32": _plan_2d(63, 32, 32, 1, 1, 1, 1, 63, (0, 16384), (1, 9216)),
    "edges-p64-3x3-32-32": _plan_2d(64, 32, 32, 1, 1, 1, 1, 64, (0, 16384), (1, 9216)),
    "edges-p65-3x3-32-32": _plan_2d(65, 32, 32, 1, 1, 2, 1, 1, (0, 16384), (1, 9216)),
}
# the layer cases: conv2d_wgrad's widths and channel blocks, restated, and what every block pair's plan has in common
WGRAD_LAYER_PLANS_2D = {
    "layer-80-144": dict(pixels=2706, widths=(96, 160), blocks_ca=(64, 32), blocks_cb=(128, 32), chunks=20, chunk_steps=3,
                         pixels_in_last_stage=18),
    "layer-up-144-80": dict(pixels=2706, widths=(96, 160), blocks_ca=(64, 32), blocks_cb=(128, 32), chunks=20,
                            chunk_steps=3, pixels_in_last_stage=18),
}
assert set(WGRAD_PLANS_2D) == {c["name"] for c in WGRAD_CASES_2D}
assert set(WGRAD_LAYER_PLANS_2D) == {c["name"] for c in WGRAD_LAYER_CASES_2D}
# Measured on wgrad_data (tests/test_conv2d_wgrad_cpu.py prints them): largest abs-sum / share of non-zero entries of
# dw; one_level at WGRAD_ONE_LEVEL_DENSITY / sqrt(P), the level pairs of WGRAD_LEVELS at density_for(P).
#
#       case                          P      one_level      x2_g2          x3_g1          x1_g3
#       loop-tr-5x5s2-64-128          2706   10.0 / 0.678   9.020 / 0.920  9.012 / 0.882  9.012 / 0.880
#       loop-tr-up-5x5s2-192-32       2706   11.0 / 0.677   9.014 / 0.924  9.018 / 0.889  9.008 / 0.880
#       loop-narrowA-9x9s4-3-64       825    8.0 / 0.684    8.027 / 0.917  8.014 / 0.891  8.010 / 0.879
#       loop-narrowA-up-9x9s4-64-3    825    9.0 / 0.679    8.018 / 0.920  9.010 / 0.884  8.012 / 0.885
#       loop-8x8-5x5s1-256-256        2624   13.0 / 0.679   10.025 / 0.922 11.012 / 0.883 10.014 / 0.882
#       one-chunk-23x23-3-32          1073   8.0 / 0.578    6.023 / 0.820  9.008 / 0.764  8.012 / 0.738
#       row-1x3-128-64                21900  11.0 / 0.693   9.029 / 0.927  8.012 / 0.887  8.012 / 0.890
#       col-4x1s2-32-64               8194   11.0 / 0.683   7.016 / 0.932  9.008 / 0.896  9.018 / 0.889
#       even-4x2s2-32-64              70     9.0 / 0.663    8.016 / 0.914  8.010 / 0.836  7.004 / 0.865
#       edges-p63-3x3-32-32           63     8.0 / 0.645    8.023 / 0.901  6.010 / 0.852  6.010 / 0.864
#       edges-p64-3x3-32-32           64     7.0 / 0.645    8.020 / 0.900  6.012 / 0.865  6.012 / 0.850
#       edges-p65-3x3-32-32           65     8.0 / 0.666    7.018 / 0.887  7.010 / 0.842  6.014 / 0.844
#       layer-80-144                  2706   11.0 / 0.682   10.023 / 0.921 10.012 / 0.879 9.014 / 0.879
#       layer-up-144-80               2706   11.0 / 0.682   9.027 / 0.923  10.010 / 0.884 11.006 / 0.882
# (one-chunk: at 13 x 17 pixels most taps of a 23 x 23 kernel meet few pixels inside A and 0.39 of dw is non-zero;
# 29 x 37 is the extent at which the one-level share is above a half.)


_ALL_CASES = (PLANE_CASES + GRADIENT_CASES + IMPULSE_CASES + WGRAD_CASES_3D + WGRAD_CASES_2D + WGRAD_LAYER_CASES_2D)
_BY_NAME = {c["name"]: c for c in _ALL_CASES}
assert len(_BY_NAME) == len(_ALL_CASES)
