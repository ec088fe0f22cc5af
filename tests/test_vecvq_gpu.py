"""GPU tier: the ECVQ kernels (csrc/vecvq.hip), `ecvq_assign` and the VECVQ model on them against the float64 definition
of tests/vecvq_ref.py.

Shapes come from the kernel's own constants (csrc/vecvq_params.h through vq_ops.VQ_CONSTANTS): each of N, K, D at 1,
around the wave size and the row tile, around one codebook chunk of either route, several chunks with a ragged last
one, and around the narrow / wide boundary; a greedy pairwise cover of those values, each with two lambdas and both
distortion kinds.

Bars.  Forward: a row's chosen codeword may cost at most 4 (D + 4) 2^-24 (|rate| + lmbda dist) more than the float64
minimum (a float32 difference-form cost in any summation order carries about (D + 4) 2^-24 relative error, two
competing costs double it, fused versus unfused multiply-adds double it again); its rate is rates[index] bit for bit;
its distortion is within 2 (D + 3) 2^-24 relative of the float64 one.  With integer data float32 is exact and the
index must be the float64 arg-min with lowest-index ties, exactly.  Backward: no number chosen in advance;
`ecvq_assign_reference` runs in float32 on the CPU under the kernel's own index and
    err_kernel <= 2 * err_composition + 1e-6
in relative L2 against the float64 formulas (2: other summation orders; 1e-6: the project's float32 slack).  Both
errors are printed."""
import functools
import itertools

import numpy as np
import pytest
import torch

import vecvq_ref
import compression_amd as tfc
from compression_amd import _lib
from compression_amd.models import toy_sources
from compression_amd.ops import vq_ops

pytestmark = pytest.mark.gpu

C = vq_ops.VQ_CONSTANTS
WAVE, ROWS, EDGE = C["VQ_WAVE"], C["VQ_ROWS"], C["VQ_NARROW_MAX_D"]
CHUNK, KB, DT = C["VQ_NARROW_CHUNK"], C["VQ_WIDE_KB"], C["VQ_WIDE_DT"]
EPS = 2.0 ** -24

N_VALUES = [1, WAVE - 1, WAVE, WAVE + 1, ROWS - 1, ROWS + 1, 1000]
K_VALUES = sorted({1, 2, KB - 1, KB + 1, WAVE - 1, WAVE + 1, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 17})
D_VALUES = sorted({1, 2, 3, 16, EDGE - 1, EDGE, EDGE + 1, 2 * EDGE})     # 2 * EDGE: the wide route's 16-byte loads


def pairwise_cover(*axes):
    """A greedy cover of every pair of values of two different axes; deterministic."""
    triples = list(itertools.product(*axes))
    pairs = lambda t: {(i, j, t[i], t[j]) for i in range(len(t)) for j in range(i + 1, len(t))}     # noqa: E731
    missing = set().union(*(pairs(t) for t in triples))
    chosen = []
    while missing:
        best = max(triples, key=lambda t: len(pairs(t) & missing))
        chosen.append(best)
        missing -= pairs(best)
    return chosen


TRIPLES = pairwise_cover(N_VALUES, K_VALUES, D_VALUES) + [(ROWS, CHUNK, EDGE), (WAVE + 1, KB + 1, 1024)]
LAMBDAS = [0.5, 37.0]
KINDS = ["sse", "mse"]


@functools.lru_cache(maxsize=None)
def inputs(n, k, d):
    """(x, codebook, rates) on the CPU: standard normal x, codewords on the data (x[random rows] + 0.05 normal), so
    near-ties are common and an expanded distance would cancel; rates from random logits."""
    gen = torch.Generator().manual_seed(100003 * n + 1009 * k + d)
    x = torch.randn(n, d, generator=gen)
    codebook = x[torch.randint(n, (k,), generator=gen)] + 0.05 * torch.randn(k, d, generator=gen)
    logits = torch.randn(k, generator=gen)
    rates = (torch.logsumexp(logits, 0) - logits) / np.log(2.0)
    return x, codebook.contiguous(), rates.contiguous()


@functools.lru_cache(maxsize=None)
def sse64(n, k, d):
    x, c, r = inputs(n, k, d)
    return vecvq_ref.costs(x, c, r, 1.0, "sse")[1]


def run_assign(x, c, r, lmbda, kind, counts=True):
    """One call of tfc_vecvq_assign -> numpy (index, rate, distortion, counts)."""
    out = vq_ops._launch_assign(x.cuda().contiguous(), c.cuda().contiguous(), r.cuda().contiguous(), float(lmbda),
                                vq_ops.DISTORTION_CODE[kind], counts)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def check_forward(x, c, r, dist64, lmbda, got):
    index, rate, dist, counts = got
    n, d = x.shape
    k = c.shape[0]
    r64 = r.double().numpy()
    cost64 = r64[None, :] + lmbda * dist64
    assert index.dtype == np.int32 and index.min() >= 0 and index.max() < k
    rows = np.arange(n)
    chosen_dist = dist64[rows, index]
    gap = cost64[rows, index] - cost64.min(axis=1)
    bound = 4 * (d + 4) * EPS * (np.abs(r64[index]) + lmbda * chosen_dist)
    worst = float((gap / np.maximum(bound, 1e-300)).max())
    print(f"cost gap / bound {worst:.3f}", end="  ")
    assert (gap <= bound).all(), f"{int((gap > bound).sum())} rows of {n} beyond the bound, worst {worst:.3f} of it"
    assert np.array_equal(rate.view(np.int32), r.numpy()[index].view(np.int32))
    err = np.abs(dist.astype(np.float64) - chosen_dist)
    dbound = 2 * (d + 3) * EPS * chosen_dist
    print(f"distortion error / bound {float((err / np.maximum(dbound, 1e-300)).max()):.3f}")
    assert (err <= dbound).all()
    if counts is not None:
        assert np.array_equal(counts, np.bincount(index, minlength=k))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lmbda", LAMBDAS)
@pytest.mark.parametrize("shape", TRIPLES, ids=lambda s: "x".join(map(str, s)))
def test_forward_random(shape, lmbda, kind):
    n, k, d = shape
    x, c, r = inputs(n, k, d)
    dist64 = sse64(n, k, d) * vecvq_ref.scale_of(kind, d)
    check_forward(x, c, r, dist64, lmbda, run_assign(x, c, r, lmbda, kind))


def test_cases_cover_the_routes_and_edges():
    ns, ks, ds = ({t[i] for t in TRIPLES} for i in range(3))
    assert {1, WAVE - 1, WAVE, WAVE + 1, ROWS - 1, ROWS, ROWS + 1} <= ns
    assert {1, CHUNK - 1, CHUNK, CHUNK + 1, KB - 1, KB + 1} <= ks and max(ks) > 2 * CHUNK and max(ks) % CHUNK
    assert {1, EDGE - 1, EDGE, EDGE + 1, 1024} <= ds
    assert any(d > EDGE and d % 4 == 0 for d in ds) and any(d > EDGE and d % DT for d in ds)
    assert any(d > EDGE and k > 2 * KB and k % KB for _, k, d in TRIPLES)


@pytest.mark.parametrize("shape", [(300, CHUNK + 40, 5), (300, 2 * KB + 7, EDGE + 9), (ROWS + 3, 3 * KB, 2 * EDGE)],
                         ids=["narrow", "wide", "wide-vec"])
def test_forward_exact_data_ties_go_to_the_lowest_index(shape):
    """Small integers, rates in eighths, lambda a power of two, sse: every float32 cost is exact, whatever the order of
    the sum, so the index is the float64 arg-min with the lowest index among equal costs.  The codebook holds
    duplicated rows (equal rates too) and different rows at equal cost."""
    n, k, d = shape
    gen = torch.Generator().manual_seed(k + d)
    x = torch.randint(-2, 3, (n, d), generator=gen).float()
    c = torch.randint(-2, 3, (k, d), generator=gen).float()
    r = torch.randint(0, 24, (k,), generator=gen).float() / 8
    c[k // 2:k // 2 + k // 4] = c[:k // 4]                  # duplicates, some of them in a later chunk
    r[k // 2:k // 2 + k // 4] = r[:k // 4]
    lmbda = 0.25
    cost64, dist64 = vecvq_ref.costs(x, c, r, lmbda, "sse")
    want = np.argmin(cost64, axis=1)
    tied = (cost64 == cost64.min(axis=1, keepdims=True)).sum(axis=1)
    assert (tied > 1).mean() > 0.2, "the data holds too few ties to test the rule"
    index, rate, dist, counts = run_assign(x, c, r, lmbda, "sse")
    assert np.array_equal(index, want)
    assert np.array_equal(rate, r.numpy()[want]) and np.array_equal(dist, dist64[np.arange(n), want].astype(np.float32))
    assert np.array_equal(counts, np.bincount(want, minlength=k))


def test_non_finite_inputs_keep_the_index_in_range():
    x, c, r = (t.clone() for t in inputs(WAVE + 1, KB + 1, 3))
    x[0] = float("nan"); x[1] = float("inf"); r[2] = float("nan"); c[3] = float("-inf")
    index, _, _, counts = run_assign(x, c, r, 1.0, "sse")
    assert index.min() >= 0 and index.max() < c.shape[0] and counts.sum() == x.shape[0]


def test_leading_axes_and_empty_input():
    x, c, r = inputs(WAVE - 1, KB + 1, 3)
    index, rate, dist = tfc.ecvq_assign(x.cuda().reshape(7, 9, 3), c.cuda(), r.cuda(), 2.0, "mse")
    flat = run_assign(x, c, r, 2.0, "mse")
    assert tuple(index.shape) == (7, 9) and np.array_equal(index.cpu().numpy().reshape(-1), flat[0])
    assert np.array_equal(dist.cpu().numpy().reshape(-1), flat[2])
    assert np.array_equal(tfc.ecvq_counts(x.cuda(), c.cuda(), r.cuda(), 2.0, "mse").cpu().numpy(), flat[3])
    index, rate, dist = tfc.ecvq_assign(x[:0].cuda(), c.cuda(), r.cuda(), 2.0)
    assert index.numel() == 0 and rate.numel() == 0 and dist.numel() == 0


# ---------------------------------------------------------------------------------------------------------------------
# backward

BWD_DT, BWD_SPLIT = C["VQ_BWD_DT"], C["VQ_BWD_SPLIT_ROWS"]
# (N, K, D, how): "data" as above; "far": all but three codewords sit far from the data (many unused codewords);
# "one": one codeword takes every row
BACKWARD_CASES = [(1, 1, 1, "data"), (WAVE + 1, 2, 3, "data"), (ROWS + 1, WAVE - 1, 16, "data"),
                  (1000, 2 * CHUNK + 17, EDGE, "far"), (1000, KB + 1, EDGE + 1, "data"), (ROWS - 1, WAVE + 1, 2 * EDGE, "far"),
                  (300, 9, BWD_DT + 44, "data"), (2 * BWD_SPLIT + 904, 5, 3, "data"), (1000, 4, 7, "one"),
                  (WAVE - 1, 17, 1024, "data")]


def rel_l2(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


def run_backward(x, c, index, g_rate, g_dist, kind, outputs=(True, True, True)):
    """One call of tfc_vecvq_backward -> numpy (d_rates, d_codebook, d_x); an output not asked for gets a null pointer
    and comes back as None."""
    n, d = x.shape
    k = c.shape[0]
    dev = [t.cuda().contiguous() if t is not None else None for t in (x, c, index, g_rate, g_dist)]
    outs = [torch.full(shape, 7.0, device="cuda") if want else None
            for want, shape in zip(outputs, ((k,), (k, d), (n, d)))]
    ptr = vq_ops._ptr
    _lib.check(_lib.lib().tfc_vecvq_backward(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), n, k, d,
                                             vq_ops.DISTORTION_CODE[kind], ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in outs)


@functools.lru_cache(maxsize=None)
def backward_inputs(n, k, d, how):
    x, c, r = (t.clone() for t in inputs(n, k, d))
    if how == "far":
        c[3:] += 100.0
    if how == "one":
        r = torch.tensor([1e4, 1e4, 0.0, 1e4])[:k].contiguous()
    gen = torch.Generator().manual_seed(n + k + d)
    return x, c, r, torch.randn(n, generator=gen), torch.randn(n, generator=gen)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_backward(case, kind):
    n, k, d, how = case
    x, c, r, g_rate, g_dist = backward_inputs(n, k, d, how)
    index = torch.from_numpy(run_assign(x, c, r, 1.5, kind, counts=False)[0])
    used = np.bincount(index.numpy(), minlength=k) > 0
    if how == "far":
        assert (~used).sum() >= k - 3 > 0
    if how == "one":
        assert used.sum() == 1
    got = run_backward(x, c, index, g_rate, g_dist, kind)
    want = vecvq_ref.gradients(x, c, index, g_rate, g_dist, kind)
    # the same-dtype composition on the CPU under the kernel's own index
    leaves = [t.clone().requires_grad_(True) for t in (r, c, x)]
    _, rate, dist = tfc.ecvq_assign_reference(leaves[2], leaves[1], leaves[0], 1.5, kind, indexes=index)
    (g_rate * rate + g_dist * dist).sum().backward()
    for name, mine, truth, leaf in zip(("d_rates", "d_codebook", "d_x"), got, want, leaves):
        assert np.isfinite(mine).all()
        if not np.linalg.norm(truth):                      # x on its codeword everywhere: nothing to be relative to
            assert not mine.any(), name
            continue
        err_kernel, err_composition = rel_l2(mine, truth), rel_l2(leaf.grad.numpy(), truth)
        print(f"{name}: kernel {err_kernel:.3e}  composition {err_composition:.3e}")
        assert err_kernel <= 2 * err_composition + 1e-6, name
    # codewords nobody chose: exact zeros
    assert not got[0][~used].any() and not got[1][~used].any()
    # deterministic: the same bits again
    again = run_backward(x, c, index, g_rate, g_dist, kind)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("case", [(ROWS + 1, WAVE - 1, 16, "data"), (2 * BWD_SPLIT + 904, 5, 3, "data")],
                         ids=lambda s: "x".join(map(str, s)))
def test_backward_null_gradients_and_outputs_are_honoured(case):
    n, k, d, how = case
    x, c, r, g_rate, g_dist = backward_inputs(n, k, d, how)
    index = torch.from_numpy(run_assign(x, c, r, 1.5, "sse", counts=False)[0])
    full = run_backward(x, c, index, g_rate, g_dist, "sse")
    same = lambda a, b: np.array_equal(a.view(np.int32), b.view(np.int32))     # noqa: E731
    d_r, d_c, d_x = run_backward(x, c, index, None, g_dist, "sse")            # g_rate null: zero
    assert not d_r.any() and same(d_c, full[1]) and same(d_x, full[2])
    d_r, d_c, d_x = run_backward(x, c, index, g_rate, None, "sse")            # g_dist null: zero
    assert same(d_r, full[0]) and not d_c.any() and not d_x.any()
    for skip in range(3):                                                      # a null output is not written
        outputs = tuple(i != skip for i in range(3))
        part = run_backward(x, c, index, g_rate, g_dist, "sse", outputs)
        assert part[skip] is None
        assert all(same(part[i], full[i]) for i in range(3) if i != skip)


# ---------------------------------------------------------------------------------------------------------------------
# the model

def _models(name):
    gen = torch.Generator().manual_seed(5)
    if name == "sphere":
        source, k = toy_sources.Sphere(order=2), 16
    else:
        source, k = toy_sources.Sawbridge(torch.linspace(0.0, 1.0, 33)), 65
    make = lambda: toy_sources.VECVQModel(k, source=source, lmbda=3.0, distortion_loss="sse",     # noqa: E731
                                          generator=torch.Generator().manual_seed(6))
    return make, source.sample(500, generator=gen)


def _mean_loss_grads(model, x, index, dtype):
    """d mean(rate + lmbda distortion) / d (codebook, _logits) on the CPU in `dtype` under the given index."""
    codebook = model.codebook.detach().cpu().to(dtype).requires_grad_(True)
    logits = model._logits.detach().cpu().to(dtype).requires_grad_(True)
    scaled = logits / model.logit_scale
    rates = (torch.logsumexp(scaled, 0) - scaled) / np.log(2.0)
    _, rate, dist = tfc.ecvq_assign_reference(x.to(dtype), codebook, rates, model.lmbda, model.distortion_loss,
                                              indexes=index)
    (rate + model.lmbda * dist).mean().backward()
    return codebook.grad.numpy(), logits.grad.numpy()


@pytest.mark.parametrize("name", ["sphere", "sawbridge"])
def test_model_on_the_gpu_against_a_cpu_copy(name):
    make, x = _models(name)
    cpu = make()
    gpu = make().cuda()
    gpu.load_state_dict(cpu.state_dict())
    xg = x.cuda()
    # quantize / test_losses: the forward rule, with the GPU model's own rates
    codebook, rates, index = gpu.quantize(xg)
    rate, dist = gpu.test_losses(xg)
    assert tuple(codebook.shape) == tuple(cpu.codebook.shape) and tuple(index.shape) == (x.shape[0],)
    dist64 = vecvq_ref.costs(x, codebook.detach().cpu(), rates.detach().cpu(), gpu.lmbda)[1]
    got = (index.cpu().numpy(), rate.detach().cpu().numpy(), dist.detach().cpu().numpy(), gpu.usage(xg).cpu().numpy())
    check_forward(x, codebook.detach().cpu(), rates.detach().cpu(), dist64, gpu.lmbda, got)
    # the CPU copy agrees wherever the two lowest costs are not within the bound of each other
    cpu_index = cpu.quantize(x)[2].numpy()
    cost64 = rates.detach().cpu().double().numpy()[None, :] + gpu.lmbda * dist64
    two = np.sort(cost64, axis=1)[:, :2]
    clear = two[:, 1] - two[:, 0] > 8 * (x.shape[1] + 4) * EPS * np.abs(two[:, 1])
    assert clear.mean() > 0.9 and np.array_equal(cpu_index[clear], got[0][clear])
    # gradients of the mean loss
    (rate + gpu.lmbda * dist).mean().backward()
    truth = _mean_loss_grads(gpu, x, index.cpu(), torch.float64)
    composition = _mean_loss_grads(gpu, x, index.cpu(), torch.float32)
    for pname, mine, want, comp in zip(("codebook", "_logits"), (gpu.codebook.grad, gpu._logits.grad), truth, composition):
        err_kernel, err_composition = rel_l2(mine.cpu().numpy(), want), rel_l2(comp, want)
        print(f"{pname}: kernel {err_kernel:.3e}  composition {err_composition:.3e}")
        assert err_kernel <= 2 * err_composition + 1e-6, pname


@pytest.mark.parametrize("name", ["sphere", "sawbridge"])
def test_train_steps_are_bit_identical(name):
    make, x = _models(name)
    state = make().state_dict()
    ends = []
    for _ in range(2):
        model = make().cuda()
        model.load_state_dict(state)
        optimizer = torch.optim.SGD(model.parameters(), lr=0.05)
        metrics = [model.train_step(x.cuda(), optimizer) for _ in range(2)]
        assert set(metrics[0]) == {"loss", "rate", "distortion", "gradient RMS"}
        ends.append([p.detach().cpu().numpy().copy() for p in model.parameters()])
    for a, b in zip(*ends):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert any(not np.array_equal(a, s.numpy()) for a, s in zip(ends[0], state.values()))
