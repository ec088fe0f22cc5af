"""CPU tier of the rank-2 weight gradient cases (tests/conv_probe_data.py, WGRAD_CASES_2D and WGRAD_LAYER_CASES_2D; the
GPU tier is tests/test_conv2d_wgrad_gpu.py).

conv_wgrad_kernel (csrc/signal_conv_backward.hip) gives a workgroup one tap and the 64-pixel stages chunk, chunk +
chunks, ... of B's grid, with a register prefetch one stage ahead; chunks = max(1, min(stages, 2 CUs / taps)) is the
host's choice, and below a few hundred to a few thousand pixels every workgroup's loop runs once.  The cases are there
for what only shows beyond that — the prefetch inside the loop, the barriers around the LDS stage, the strided walk, a
sum over many chunk partials, one workgroup walking every stage — and for the index arithmetic at kh != kw, even
supports, A smaller than HB s, WB = 1, HB = 1 and a power of two.  Which branch a shape takes is ASKED of
tfc_conv2d_wgrad_plan, which reports what the function the launch calls chooses for a given CU count and needs no
device; assert_plan holds every case to conv_probe_data.WGRAD_PLANS_2D at 256 CUs and to the property it is named for.
A retune of the chunk rule, the tile pairs or the transposing-read decision that moves a case off its branch fails here
and names the case.

The conditions under which the GPU tier may demand EQUALITY with the float64 oracle are asserted here: the abs-sum per
entry of dw below 2^4, at least half of dw non-zero, every value a multiple of 2^-18 — and, in one place, what that
buys: the float32 contraction of the same data over pixels in a shuffled order, on this machine's BLAS, equals the
float64 oracle, so the order in which a kernel adds its pixels, stages and chunks cannot matter.

Not reached: the kernel's M >= 2^31 branch (64-bit divisions in place of fast_div) needs more than 2^31 pixels of B, at
one channel per side 8 GB of bfloat16 — no test may be that large, and the branch has no switch to force it."""
import ctypes
import itertools

import pytest
import torch

import conv_probe_data as pd

CUS = 256                                                                # the device WGRAD_PLANS_2D is written for
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
LEVELS = list(pd.WGRAD_LEVELS) + ["one_level"]
ALL_CASES = pd.WGRAD_CASES_2D + pd.WGRAD_LAYER_CASES_2D


def wgrad_args(c, x, gy):
    """conv2d_wgrad's (a, b, transpose) of layer case c: down (x, gy, False), up (gy, x, True)."""
    return (gy, x, True) if c["up"] else (x, gy, False)


def contraction(a, b, support, stride, transpose, dtype, order=None):
    """include/tfc_hip.h, tfc_conv2d_wgrad, tap by tap in `dtype`: G[t][ca][cb] = sum over B's pixels p = (n, q) of
    A[n, q s + t - k // 2, ca] B[p, cb] with zeros outside A, as [P, CA]^T [P, CB] products (order: a permutation of the
    P pixels, the same for both sides); transpose: [.., cb, ca]."""
    (kh, kw), (hb, wb) = support, b.shape[1:3]
    ap = torch.nn.functional.pad(a.to(dtype), [0, 0, kw, kw + wb * stride, kh, kh + hb * stride])
    bp = b.to(dtype).reshape(-1, b.shape[-1])
    if order is not None:
        bp = bp[order]
    g = torch.zeros(kh, kw, a.shape[-1], b.shape[-1], dtype=dtype)
    for ty, tx in itertools.product(range(kh), range(kw)):
        y0, x0 = kh + ty - kh // 2, kw + tx - kw // 2
        win = ap[:, y0:y0 + hb * stride:stride, x0:x0 + wb * stride:stride].reshape(-1, a.shape[-1])
        g[ty, tx] = (win if order is None else win[order]).T @ bp
    return g.transpose(-1, -2) if transpose else g


def plans(c, cus, ca=None, cb=None):
    """-> {dtype name: plan} of the call of case c (or of its channel block pair (ca, cb)) on a device of `cus` CUs."""
    from compression_amd.layers import functional
    b_extent, case_ca, case_cb, _ = pd.wgrad_geometry(c)
    return {name: functional.conv2d_wgrad_plan(c["n"], b_extent, ca or case_ca, cb or case_cb, c["support"], dtype, cus)
            for name, dtype in DTYPES.items()}


def assert_named_property(c, by_dtype, ca, cb):
    """What the case is named for, on the plan of any device."""
    name, f32, bf16 = c["name"], by_dtype["float32"], by_dtype["bfloat16"]
    assert f32["tr"] == 0 and bf16["tr"] == (1 if min(ca, cb) >= 32 else 0), (name, by_dtype)
    for plan in (f32, bf16):
        stages = -(-pd.wgrad_geometry(c)[3] // 64)
        assert plan["chunk_steps"] == -(-stages // plan["chunks"]) and 1 <= plan["pixels_in_last_stage"] <= 64, (name, plan)
        if name.startswith(("loop-", "layer-", "row-")):
            assert plan["chunk_steps"] >= 3 and plan["chunks"] >= 2, (name, plan)
        if name.startswith(("loop-tr", "layer-", "row-", "col-")):
            assert plan["pixels_in_last_stage"] < 64, (name, plan)
        if name.startswith("loop-8x8"):
            assert plan["tiles_ca"] == plan["tiles_cb"] == 8 and plan["pixels_in_last_stage"] == 64, (name, plan)
        if name.startswith("one-chunk"):
            assert plan["chunks"] == 1 and plan["chunk_steps"] >= 4, (name, plan)
        if name.startswith("col-"):
            assert plan["chunk_steps"] >= 2 and plan["chunks"] >= 2, (name, plan)
        if name.startswith("edges-p63") or name.startswith("edges-p64"):
            assert (plan["chunks"], plan["chunk_steps"]) == (1, 1), (name, plan)
        if name.startswith("edges-p65"):
            assert (plan["chunks"], plan["chunk_steps"], plan["pixels_in_last_stage"]) == (2, 1, 1), (name, plan)
    assert bf16["lds_bytes"] <= f32["lds_bytes"] <= 160 * 1024, (name, by_dtype)


def assert_plan(c, cus=CUS):
    """The plan(s) of case c on `cus` CUs have the case's property; at 256 CUs they are conv_probe_data's tables."""
    name = c["name"]
    b_extent, ca, cb, pixels = pd.wgrad_geometry(c)
    if name in pd.WGRAD_PLANS_2D:
        by_dtype = plans(c, cus)
        assert_named_property(c, by_dtype, ca, cb)
        if cus == CUS:
            want = pd.WGRAD_PLANS_2D[name]
            for dname, plan in by_dtype.items():
                common = {k: v for k, v in plan.items() if k not in ("tr", "lds_bytes")}
                got = dict(common, pixels=pixels, ca=ca, cb=cb, **{dname: {k: plan[k] for k in ("tr", "lds_bytes")}})
                assert got == {k: want[k] for k in got}, (name, dname, got, want)
        return by_dtype
    from compression_amd.layers import functional
    want = pd.WGRAD_LAYER_PLANS_2D[name]
    assert (functional._wgrad_width(ca), functional._wgrad_width(cb)) == want["widths"] and pixels == want["pixels"], name
    for block_ca, block_cb in itertools.product(want["blocks_ca"], want["blocks_cb"]):
        by_dtype = plans(c, cus, block_ca, block_cb)
        assert_named_property(c, by_dtype, block_ca, block_cb)
        if cus == CUS:
            for plan in by_dtype.values():
                assert {k: plan[k] for k in ("chunks", "chunk_steps", "pixels_in_last_stage")} == \
                    {k: want[k] for k in ("chunks", "chunk_steps", "pixels_in_last_stage")}, (name, plan, want)
                assert (plan["tiles_ca"], plan["tiles_cb"]) == (block_ca // 32, block_cb // 32), (name, plan)
    return by_dtype


@pytest.mark.parametrize("c", ALL_CASES, ids=pd.case_id)
def test_case_reaches_its_branch_of_the_host_rule_at_256_cus(c):
    by_dtype = assert_plan(c)
    print(c["name"], by_dtype)


def test_geometry_the_cases_are_named_for():
    by_name = pd._BY_NAME
    for name in ("loop-tr-5x5s2-64-128", "layer-80-144", "col-4x1s2-32-64", "even-4x2s2-32-64", "loop-narrowA-9x9s4-3-64"):
        c = by_name[name]                                                # A = x is smaller than HB s on some axis
        b_extent = pd.wgrad_geometry(c)[0]
        assert any(e < q * s for e, q, s in zip(c["extent"], b_extent, c["strides"])), name
    assert pd.wgrad_geometry(by_name["row-1x3-128-64"])[0][0] == 1       # HB = 1
    assert pd.wgrad_geometry(by_name["col-4x1s2-32-64"])[0][1] == 1 and by_name["col-4x1s2-32-64"]["n"] == 2
    wb = pd.wgrad_geometry(by_name["loop-8x8-5x5s1-256-256"])[0][1]
    assert wb > 1 and wb & (wb - 1) == 0                                 # WB a power of two
    for name in ("row-1x3-128-64", "col-4x1s2-32-64", "even-4x2s2-32-64"):
        kh, kw = by_name[name]["support"]
        assert kh != kw
    assert all(k % 2 == 0 for k in by_name["even-4x2s2-32-64"]["support"])
    assert by_name["one-chunk-23x23-3-32"]["support"][0] * by_name["one-chunk-23x23-3-32"]["support"][1] > 2 * CUS


def test_plan_follows_the_cu_count():
    """chunks = max(1, min(stages, 2 cus / taps)): the same shape on other devices."""
    from compression_amd.layers import functional
    c = pd._BY_NAME["loop-tr-5x5s2-64-128"]                              # 25 taps, 43 stages
    b_extent, ca, cb, _ = pd.wgrad_geometry(c)
    got = {cus: functional.conv2d_wgrad_plan(c["n"], b_extent, ca, cb, c["support"], torch.float32, cus)
           for cus in (1, 12, 13, 64, 256, 304, 538, 4096)}
    assert {cus: (p["chunks"], p["chunk_steps"]) for cus, p in got.items()} == {
        1: (1, 43), 12: (1, 43), 13: (1, 43), 64: (5, 9), 256: (20, 3), 304: (24, 2), 538: (43, 1), 4096: (43, 1)}


def test_plan_query_checks_its_arguments_as_the_call_does():
    from compression_amd import _lib
    from compression_amd.layers import functional
    lib = _lib.lib()
    out = (ctypes.c_int32 * len(functional.CONV2D_WGRAD_PLAN_FIELDS))()
    # (dtype, n, hb, wb, ca, cb, kh, kw): the call fails on these before it touches a pointer or a device
    bad = {
        "dtype": (7, 1, 8, 8, 32, 32, 3, 3),
        "bad geometry": (0, 1, 8, 8, 32, 32, 0, 3),
        "channel counts must be <= 4 or multiples of 32 up to 256 (got 40, 32)": (0, 1, 8, 8, 40, 32, 3, 3),
        "channel counts must be <= 4 or multiples of 32 up to 256 (got 32, 288)": (1, 1, 8, 8, 32, 288, 3, 3),
        "channel pair (96, 32) is not built": (1, 1, 8, 8, 96, 32, 3, 3),
        "channel pair (3, 160) is not built": (0, 1, 8, 8, 3, 160, 3, 3),
        "channel pair (224, 224) is not built": (0, 1, 8, 8, 224, 224, 3, 3),
        "negative extent": (0, 1, -8, 8, 32, 32, 3, 3),
    }
    for text, (dtype, n, hb, wb, ca, cb, kh, kw) in bad.items():
        assert lib.tfc_conv2d_wgrad(None, None, None, dtype, n, hb, wb, ca, hb, wb, cb, kh, kw, 1, 0, None) != 0
        of_call = _lib.last_error()
        assert lib.tfc_conv2d_wgrad_plan(dtype, n, hb, wb, ca, cb, kh, kw, CUS, out) != 0
        of_plan = _lib.last_error()
        assert text in of_call and of_call.startswith("tfc_conv2d_wgrad: "), (text, of_call)
        assert of_plan == of_call.replace("tfc_conv2d_wgrad: ", "tfc_conv2d_wgrad_plan: "), (of_plan, of_call)
    with pytest.raises(ValueError, match="tfc_conv2d_wgrad_plan: an empty cotangent launches nothing"):
        functional.conv2d_wgrad_plan(0, (8, 8), 32, 32, (3, 3), torch.float32, CUS)
    with pytest.raises(ValueError, match="tfc_conv2d_wgrad_plan: an empty cotangent launches nothing"):
        functional.conv2d_wgrad_plan(1, (8, 0), 32, 32, (3, 3), torch.bfloat16, CUS)
    for cus in (0, -4):
        with pytest.raises(ValueError, match="tfc_conv2d_wgrad_plan: cus must be >= 1"):
            functional.conv2d_wgrad_plan(1, (8, 8), 32, 32, (3, 3), torch.float32, cus)
    assert lib.tfc_conv2d_wgrad_plan(0, 1, 8, 8, 32, 32, 3, 3, CUS, None) != 0 and "out must not be null" in _lib.last_error()
    # an empty call is no error and needs no device: dw is added to, so nothing is written
    assert lib.tfc_conv2d_wgrad(None, None, None, 0, 0, 8, 8, 32, 8, 8, 32, 3, 3, 1, 0, None) == 0


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("c", ALL_CASES, ids=pd.case_id)
def test_wgrad_probe_data_is_exact_in_any_order(c, levels):
    x, gy, dw, abs_dw = pd.wgrad_data(c, levels)
    pixels = pd.wgrad_geometry(c)[3]
    largest, share = float(abs_dw.max()), float((dw != 0).double().mean())
    print(f"{c['name']} {levels}: P {pixels} largest abs-sum {largest:.3f} non-zero outputs {share:.3f}")
    assert largest < pd.ABS_SUM_BOUND and share >= 0.5
    assert largest + 2 < pd.ABS_SUM_BOUND                                # room for the GPU tier's prefill of -2 ... 2
    assert tuple(dw.shape) == c["support"] + (c["cin"], c["cout"])
    # every product is a multiple of 2^-18, so is every partial sum, and all stay below 2^4: 22 bits, float32 holds them
    assert torch.equal((dw * 2.0 ** 18).round(), dw * 2.0 ** 18)
    assert torch.equal(dw.float().double(), dw)
    if levels == "one_level":
        assert torch.equal(x.bfloat16().float(), x) and torch.equal(gy.bfloat16().float(), gy)
        assert torch.equal(dw.round(), dw)
    # the oracle's autograd is the contraction the kernel is documented to compute ...
    a, b, transpose = wgrad_args(c, x, gy)
    stride = c["strides"][0]
    assert c["strides"] == (stride, stride)
    assert torch.equal(contraction(a, b, c["support"], stride, transpose, torch.float64), dw)
    # ... and float32 sums of this data do not depend on their order: the guarantee the GPU tier's equality rests on
    order = torch.randperm(pixels, generator=torch.Generator().manual_seed(pixels))
    got = contraction(a, b, c["support"], stride, transpose, torch.float32, order)
    assert got.dtype == torch.float32 and torch.equal(got.double(), dw)
