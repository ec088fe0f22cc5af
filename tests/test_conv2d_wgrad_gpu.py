"""GPU tier of the rank-2 weight gradient cases (tests/conv_probe_data.py, WGRAD_CASES_2D and WGRAD_LAYER_CASES_2D;
tests/test_conv2d_wgrad_cpu.py asserts the data's conditions and, from tfc_conv2d_wgrad_plan, that every case reaches the
branch of csrc/signal_conv_backward.hip it is named for — repeated here first, with the device's own CU count).

conv_wgrad_kernel's stage loop takes a second trip only above 2 CUs / taps stages of 64 pixels; these shapes take three
(or seventeen, in one workgroup per tap), with ragged and full last stages, so the prefetch inside the loop, the barriers
around the LDS stage, the strided walk and conv_wgrad_reduce_kernel's sum over many chunk partials are held to values.

Comparisons are EQUALITY with the float64 oracle (signal_conv_oracle.layer_oracle's autograd), no tolerance:
  float32    x and gy of 2 + 2, 3 + 1 and 1 + 3 digits 9 bits apart: products multiples of 2^-18, abs-sum below 2^4, so
             every partial sum is exact in float32 in any order (mfma_f32_32x32x2f32 adds such values without error)
  bfloat16   {-1, 0, +1} on both sides: each one bfloat16, every sum an integer below 16
A stage dropped, reused or added twice, a chunk partial left out, a tap's row taken for its column or a bound off by one
changes an entry by at least 2^-18.  Every result is computed twice and must agree bit for bit (the partials are summed
in chunk order; there are no float atomics).  Random data at the loop sizes is held to the project's usual bar against
the float32 twin.  The kernel's M >= 2^31 branch is not reached (see the CPU tier's docstring).

That these tests can fail was shown once on an MI355X with four value-only breaks of the kernels (never committed):
  the in-loop fetch(st + chunks) dropped (a stale stage reused)   55 of the 72 fail; no older test of the suite noticed
  kw / 2 for the row offset                                        the 12 tests of row-, col- and even- fail
  chunks - 1 partials summed in the reduce kernel                  71 fail (all but the plan test)
  `=` for `+=` in the reduce kernel                                the 6 raw-entry tests fail; no older test noticed"""
import os
import subprocess
import sys
import time

import pytest
import torch

import conv_probe_data as pd
import test_conv2d_wgrad_cpu as tier

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 4096                                         # elements before and after dw that must stay untouched
SENTINEL = 1000.0                                    # no result reaches it: prefill + abs-sum is below 16
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["float32", "bfloat16"]
RAW_CASES = ["loop-tr-5x5s2-64-128", "loop-tr-up-5x5s2-192-32", "loop-narrowA-9x9s4-3-64"]
TR_OFF_CASES = ["loop-tr-5x5s2-64-128", "loop-8x8-5x5s1-256-256"]


def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def assert_equal(got, want):
    assert tuple(got.shape) == tuple(want.shape)
    got = got.detach().float().cpu().double()
    wrong = got != want
    assert torch.equal(got, want), (int(wrong.sum()), float((got - want).abs().max()), wrong.nonzero()[:4].tolist())


def test_every_case_reaches_its_branch_on_this_device():
    """Fails — never skips — on a device whose CU count moves a case off its branch, and names the case."""
    cus = device_cus()
    for c in tier.ALL_CASES:
        print(c["name"], cus, tier.assert_plan(c, cus))
    if cus == tier.CUS:
        return
    print(f"{cus} CUs: the named properties hold; WGRAD_PLANS_2D is written for {tier.CUS} and was not compared")


def check_wgrad(c, levels, dtype):
    from compression_amd.layers import functional
    x, gy, want, abs_dw = pd.wgrad_data(c, levels)
    assert float(abs_dw.max()) < pd.ABS_SUM_BOUND
    assert float((want != 0).double().mean()) >= 0.5
    a, b, transpose = tier.wgrad_args(c, x.to(dtype).cuda(), gy.to(dtype).cuda())
    got = functional.conv2d_wgrad(a, b, c["support"], c["strides"][0], transpose)
    again = functional.conv2d_wgrad(a, b, c["support"], c["strides"][0], transpose)
    assert got.dtype == torch.float32
    assert_equal(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("levels", list(pd.WGRAD_LEVELS))
@pytest.mark.parametrize("c", tier.ALL_CASES, ids=pd.case_id)
def test_float32_weight_gradient_equals_the_oracle(c, levels):
    check_wgrad(c, levels, torch.float32)


@pytest.mark.parametrize("c", tier.ALL_CASES, ids=pd.case_id)
def test_bfloat16_weight_gradient_equals_the_oracle_on_one_level_data(c):
    """The transposing-read build for the wide pairs, pair_store / stage_narrow for the narrow ones."""
    check_wgrad(c, "one_level", torch.bfloat16)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_entry_adds_to_dw_and_writes_nothing_else(name, dtype):
    """include/tfc_hip.h: `dw ... is ADDED to`.  dw is a slice of a buffer of sentinels, prefilled with integers in
    -2 ... 2: the result is prefill + oracle exactly (the sums stay in the exact range), the guards stay as they were."""
    from compression_amd import _lib
    c = pd._BY_NAME[name]
    x, gy, want, abs_dw = pd.wgrad_data(c, "x2_g2" if dtype == torch.float32 else "one_level")
    assert float(abs_dw.max()) + 2 < pd.ABS_SUM_BOUND
    a, b, transpose = tier.wgrad_args(c, x.to(dtype).cuda().contiguous(), gy.to(dtype).cuda().contiguous())
    generator = torch.Generator().manual_seed(want.numel())
    prefill = torch.randint(-2, 3, tuple(want.shape), generator=generator).double()
    assert bool((prefill != 0).any())
    buffer = torch.full((2 * GUARD + want.numel(),), SENTINEL, dtype=torch.float32, device="cuda")
    for _ in range(2):
        dw = buffer[GUARD:GUARD + want.numel()]
        dw.copy_(prefill.float().reshape(-1))
        _lib.check(_lib.lib().tfc_conv2d_wgrad(
            a.data_ptr(), b.data_ptr(), dw.data_ptr(), _lib.DTYPE_CODE[dtype], c["n"], *a.shape[1:], *b.shape[1:],
            *c["support"], c["strides"][0], int(transpose), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((buffer[:GUARD] == SENTINEL).all()) and bool((buffer[GUARD + want.numel():] == SENTINEL).all())
        assert_equal(dw.reshape(want.shape), prefill + want)


@pytest.mark.parametrize("c", pd.WGRAD_LAYER_CASES_2D, ids=pd.case_id)
def test_layer_kernel_gradient_equals_the_oracle_at_loop_size(c):
    """Through SignalConv2D and _ConvFunction.backward: which of x and gy is `a`, `transpose`, conv2d_wgrad's zero
    channels (80 -> 96, 144 -> 160) and its channel blocks (64 + 32, 128 + 32)."""
    from compression_amd.layers import SignalConv2D
    x, gy, want, _ = pd.wgrad_data(c, "x2_g2")
    stride = c["strides"][0]
    layer = SignalConv2D(c["cout"], c["support"], corr=not c["up"], strides_down=1 if c["up"] else stride,
                         strides_up=stride if c["up"] else 1, padding="same_zeros", extra_pad_end=True,
                         kernel_parameter="variable", kernel_initializer=torch.zeros, in_channels=c["cin"]).cuda()
    assert layer._is_model_configuration()
    y = layer(x.cuda())
    assert tuple(y.shape) == tuple(gy.shape)
    y.backward(gy.cuda())
    grad = layer.kernel_variable.grad
    assert grad.dtype == torch.float32
    assert_equal(grad, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", pd.WGRAD_WIDE_LOOP_CASES_2D, ids=pd.case_id)
def test_random_data_at_loop_size_against_float64(c, dtype):
    """Relative L2 against the float64 contraction of the inputs as the kernel sees them; the twin is the same
    contraction in float32 on the CPU.  err_kernel <= 2 err_twin + 1e-6."""
    from compression_amd.layers import functional
    generator = torch.Generator().manual_seed(pd._seed(c, "random"))
    x = torch.randn((c["n"],) + c["extent"] + (c["cin"],), generator=generator).to(dtype)
    y_extent = tuple(e * s if c["up"] else -(-e // s) for e, s in zip(c["extent"], c["strides"]))
    gy = torch.randn((c["n"],) + y_extent + (c["cout"],), generator=generator).to(dtype)
    a, b, transpose = tier.wgrad_args(c, x, gy)
    stride = c["strides"][0]
    want = tier.contraction(a, b, c["support"], stride, transpose, torch.float64)
    twin = tier.contraction(a, b, c["support"], stride, transpose, torch.float32)
    got = functional.conv2d_wgrad(a.cuda(), b.cuda(), c["support"], stride, transpose)
    again = functional.conv2d_wgrad(a.cuda(), b.cuda(), c["support"], stride, transpose)
    assert torch.equal(got, again)
    norm = float(want.norm())
    err_kernel = float((got.cpu().double() - want).norm()) / norm
    err_twin = float((twin.double() - want).norm()) / norm
    print(f"{c['name']} {dtype}: err_kernel {err_kernel:.3e} err_twin {err_twin:.3e}")
    assert err_kernel <= 2.0 * err_twin + 1e-6, (c["name"], err_kernel, err_twin)


_WITHOUT_TRANSPOSING_READS = """
import sys
import torch
from compression_amd.layers import functional
cus = torch.cuda.get_device_properties(0).multi_processor_count
for name, (n, b_extent, support, stride, transpose, a, b, want) in torch.load(sys.argv[1]).items():
    plan = functional.conv2d_wgrad_plan(n, b_extent, a.shape[-1], b.shape[-1], support, torch.bfloat16, cus)
    assert plan["tr"] == 0, (name, plan)
    got = functional.conv2d_wgrad(a.cuda(), b.cuda(), support, stride, transpose)
    again = functional.conv2d_wgrad(a.cuda(), b.cuda(), support, stride, transpose)
    assert torch.equal(got, again), name
    wrong = got.cpu().double() != want
    assert not bool(wrong.any()), (name, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    print(name, plan, "equal")
"""


def test_hand_transposed_bfloat16_staging_under_tfc_wgrad_tr_0(tmp_path):
    """TFC_WGRAD_TR=0 is read once per process, so ONE fresh child runs the wide / wide pairs on pair_store: its plan
    says tr == 0 and its bfloat16 result equals the oracle; this process's plan says tr == 1."""
    from compression_amd.layers import functional
    assert os.environ.get("TFC_WGRAD_TR", "1")[:1] != "0"
    payload, started = {}, time.monotonic()
    for name in TR_OFF_CASES:
        c = pd._BY_NAME[name]
        b_extent, ca, cb, _ = pd.wgrad_geometry(c)
        assert functional.conv2d_wgrad_plan(c["n"], b_extent, ca, cb, c["support"], torch.bfloat16, device_cus())["tr"] == 1
        x, gy, want, _ = pd.wgrad_data(c, "one_level")
        a, b, transpose = tier.wgrad_args(c, x.bfloat16(), gy.bfloat16())
        assert_equal(functional.conv2d_wgrad(a.cuda(), b.cuda(), c["support"], c["strides"][0], transpose), want)
        payload[name] = (c["n"], b_extent, c["support"], c["strides"][0], transpose, a, b, want)
    own = time.monotonic() - started
    torch.save(payload, tmp_path / "cases.pt")
    env = dict(os.environ, TFC_WGRAD_TR="0", PYTHONPATH=ROOT)
    # the child does what this process just did, behind an interpreter, torch and a device context of its own
    r = subprocess.run([sys.executable, "-c", _WITHOUT_TRANSPOSING_READS, str(tmp_path / "cases.pt")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120 + 20 * own)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert [line.split()[0] for line in r.stdout.splitlines() if line.endswith("equal")] == TR_OFF_CASES
