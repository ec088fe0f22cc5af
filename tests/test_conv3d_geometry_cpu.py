"""CPU tier of the rank-3 geometry cases (tests/conv_probe_data.py, GEOMETRY_CASES_3D and WGRAD_CASES_3D; the GPU tier is
tests/test_conv3d_geometry_gpu.py).

The cases are there for branches of csrc/signal_conv3d.hip's host code: several tiles along W and H, every tile width in
both directions, the LDS loops that narrow NT and TW, NT = 4, partial column blocks at blk > 0, several channel blocks
per float32 plane; for the weight gradient several LDS stages per chunk, a shorter last chunk, a stage cut in the middle
and several 64 x 64 channel tiles with CA != CB.  Which branch a shape takes is the host's decision, so it is ASKED, not
restated: tfc_conv3d_plan / tfc_conv3d_wgrad_plan report what the functions the launches call choose, need no device,
and assert_forward_plan / assert_wgrad_plan hold every case to conv_probe_data.GEOMETRY_PLANS / WGRAD_PLANS.  A retune of
kTile, pick_nt or the chunk rule that moves a case off its branch fails here and names the case.

The data conditions under which the GPU tier may demand EQUALITY with the float64 oracle are asserted here too: the
abs-sum per output below 2^4 and at least half of the outputs non-zero, for the one-level forward data, the bias + ReLU
case and the weight gradient probes (the three plane probes of the geometry cases run through test_conv_probes_cpu.py,
which takes them from PLANE_CASES)."""
import pytest
import torch

import conv_probe_data as pd

KIB = 1024
LDS_BYTES = 160 * KIB                                                   # a CU's LDS: two workgroups where a stage fits half


def pick_nt(cout):
    """signal_conv3d.hip's pick_nt restated: the fewest padded columns, then the widest tile — only to say what an
    LDS-narrowed case would have had (GEOMETRY_PLANS' nt_from)."""
    cols = {nt: -(-cout // (32 * nt)) * 32 * nt for nt in (1, 2, 3, 4)}
    return max(nt for nt in cols if cols[nt] == min(cols.values()))


def forward_plans(c):
    """The plan in both dtypes' terms: cin_k = Cin (bfloat16) and 6 Cin (float32's planes)."""
    from compression_amd.layers import functional
    return [functional.conv3d_plan(c["up"], c["extent"], m * c["cin"], c["cout"], c["support"], c["strides"])
            for m in (1, 6)]


def assert_forward_plan(c):
    want = pd.GEOMETRY_PLANS[c["name"]]
    # a phase's output grid: the input's in the transposed direction, ceil(in / s) otherwise
    grid = c["extent"] if c["up"] else tuple(-(-n // s) for n, s in zip(c["extent"], c["strides"]))
    for plan in forward_plans(c):
        derived = dict(plan)
        derived["last_tile_w"] = grid[2] - (plan["tiles_w"] - 1) * plan["TW"]
        derived["last_tile_h"] = grid[1] - (plan["tiles_h"] - 1) * plan["TH"]
        derived["last_blk_cols"] = c["cout"] - (plan["nblk"] - 1) * 32 * plan["NT"]
        derived["tw_from"] = 128 if grid[2] > 64 else 64 if grid[2] > 32 else 32
        derived["nt_from"] = pick_nt(c["cout"])
        derived["lds_over_half"] = plan["lds_bytes"] > LDS_BYTES // 2
        derived["f32_cblocks_per_plane"] = c["cin"] // 16
        assert plan["TW"] * plan["TH"] == 128 and plan["lds_bytes"] <= LDS_BYTES, (c["name"], plan)
        assert 0 < derived["last_tile_w"] <= plan["TW"] and 0 < derived["last_tile_h"] <= plan["TH"], (c["name"], plan)
        assert 0 < derived["last_blk_cols"] <= 32 * plan["NT"], (c["name"], plan)
        got = {k: derived[k] for k in want}
        assert got == want, (c["name"], got, want, plan)
    return plan


def assert_wgrad_plan(c):
    from compression_amd.layers import functional
    want = pd.WGRAD_PLANS[c["name"]]
    b_extent, ca, cb, pixels = pd.wgrad_geometry(c)
    plan = functional.conv3d_wgrad_plan(c["n"], b_extent, ca, cb, c["support"])
    got = dict(plan, pixels=pixels, ca=ca, cb=cb)
    assert got == want, (c["name"], got, want)
    # what the case is there for: several stages per chunk, a shorter last chunk whose last stage is cut, several channel
    # tiles on both sides, the last of each partly outside, CA != CB
    assert plan["chunk_steps"] >= 2 and plan["chunks"] >= 2
    assert (plan["chunks"] - 1) * plan["chunk_steps"] * 64 + plan["pixels_in_last_chunk"] == pixels
    assert plan["pixels_in_last_chunk"] < plan["chunk_steps"] * 64 and plan["pixels_in_last_chunk"] % 64
    assert plan["tiles_ca"] >= 2 and plan["tiles_cb"] >= 2 and ca != cb and ca % 64
    return plan


@pytest.mark.parametrize("c", pd.GEOMETRY_CASES_3D, ids=pd.case_id)
def test_forward_case_reaches_its_branch_of_the_host_rule(c):
    plan = assert_forward_plan(c)
    print(c["name"], plan)


@pytest.mark.parametrize("c", pd.WGRAD_CASES_3D, ids=pd.case_id)
def test_wgrad_case_reaches_its_branch_of_the_chunk_rule(c):
    plan = assert_wgrad_plan(c)
    print(c["name"], plan)


def test_plan_queries_check_their_arguments_on_the_host():
    from compression_amd import _lib
    from compression_amd.layers import functional
    with pytest.raises(ValueError, match="tfc_conv3d_plan: input channels must be a multiple of 16"):
        functional.conv3d_plan(False, (1, 1, 8), 24, 8, (1, 1, 3), (1, 1, 1))
    with pytest.raises(ValueError, match="tfc_conv3d_plan: strides must be >= 1"):
        functional.conv3d_plan(True, (1, 1, 8), 16, 8, (1, 1, 3), (1, 0, 1))
    with pytest.raises(ValueError, match="tfc_conv3d_plan: kernel support too large for one workgroup's LDS"):
        functional.conv3d_plan(False, (1, 40, 40), 16, 8, (1, 31, 31), (1, 1, 1))
    with pytest.raises(ValueError, match="tfc_conv3d_wgrad_plan: channel counts must be multiples of 16"):
        functional.conv3d_wgrad_plan(1, (1, 1, 8), 24, 16, (1, 1, 3))
    assert _lib.lib().tfc_conv3d_plan(0, 1, 1, 8, 16, 8, 1, 1, 3, 1, 1, 1, None) != 0 and "out must not be null" in _lib.last_error()


@pytest.mark.parametrize("c", pd.GEOMETRY_CASES_3D, ids=pd.case_id)
def test_one_level_data_sums_to_one_bfloat16(c):
    x, w, want = pd.one_level_data(c)
    assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w)
    largest, share = float(pd.abs_sum(c, x, w).max()), float((want != 0).double().mean())
    k = pd.products_per_output(c)
    print(f"{c['name']} one level: K {k} density {pd.ONE_LEVEL_DENSITY / k ** 0.5:.3f} largest abs-sum {largest:.1f} "
          f"non-zero outputs {share:.3f}")
    assert largest < pd.ABS_SUM_BOUND and share >= 0.5
    assert torch.equal(want.float().bfloat16().double(), want)          # every output is one bfloat16


def test_geometry_bias_and_relu_keep_the_probe_exact():
    c = pd.GEOMETRY_BIAS_RELU_CASE
    for probe in pd.PROBES:
        x, w, _ = pd.probe_data(c, probe)
        bias = pd.integer_bias(c, probe)
        want = pd.oracle(c, x, w, bias, "relu")
        assert float(pd.abs_sum(c, x, w, bias).max()) < pd.ABS_SUM_BOUND
        assert float((want != 0).double().mean()) >= 0.25 and bool((pd.oracle(c, x, w, bias) < 0).any())
        assert bool(bias[-8:].any())                                     # the partial last block has a bias to read


@pytest.mark.parametrize("levels", list(pd.WGRAD_LEVELS) + ["one_level"])
@pytest.mark.parametrize("c", pd.WGRAD_CASES_3D, ids=pd.case_id)
def test_wgrad_probe_data_is_exact(c, levels):
    x, gy, dw, abs_dw = pd.wgrad_data(c, levels)
    largest, share = float(abs_dw.max()), float((dw != 0).double().mean())
    print(f"{c['name']} {levels}: P {pd.wgrad_geometry(c)[3]} largest abs-sum {largest:.3f} non-zero outputs {share:.3f}")
    assert largest < pd.ABS_SUM_BOUND and share >= 0.5
    assert tuple(dw.shape) == c["support"] + (c["cin"], c["cout"])
    # every product is a multiple of 2^-18, so is every partial sum, and all stay below 2^4: 22 bits, float32 holds them
    assert torch.equal((dw * 2.0 ** 18).round(), dw * 2.0 ** 18)
    assert torch.equal(dw.float().double(), dw)
    if levels == "one_level":
        assert torch.equal(x.bfloat16().float(), x) and torch.equal(gy.bfloat16().float(), gy)
        assert torch.equal(dw.round(), dw)
    # the oracle's autograd is the definition G[t][ca][cb] = sum A[n, q s + t - k/2, ca] B[n, q, cb], checked at one tap
    a, b = (gy, x) if c["up"] else (x, gy)
    t = tuple(k // 2 for k in c["support"])                              # the centre tap: A[q s] B[q]
    sub = a[(slice(None),) + tuple(slice(None, None, s) for s in c["strides"])].double()
    g = torch.einsum("ndhwa,ndhwb->ab", sub, b.double())
    assert torch.equal(g.T if c["up"] else g, dw[t])
