"""GPU tier of the training ops: `crop_patches` and `KerasAdam.step` (csrc/train.hip) bit for bit against their tensor-op
twins run on CPU copies."""
import numpy as np
import pytest
import torch

import train_ref
from compression_amd import KerasAdam
from compression_amd.ops import train_ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.float32, torch.bfloat16]
GUARD = 64


def guarded_pool(shapes, lead, seed=0):
    """Images back to back behind `lead` filler bytes (so that the first pixels start at every residue mod 4), as an
    inner slice of a tensor of 0xFF: a kernel that USES a byte from outside the pool shows it in its values, since no
    byte inside is 0xFF.  -> (pool on the CPU, [(offset, H, W)])."""
    rng = np.random.default_rng(seed)
    parts, where, at = [np.full(lead, 7, np.uint8)], [], lead
    for h, w in shapes:
        parts.append(rng.integers(0, 255, 3 * h * w, dtype=np.uint8))
        where.append((at, h, w))
        at += 3 * h * w
    flat = np.concatenate(parts)
    whole = torch.full((flat.size + 2 * GUARD,), 0xFF, dtype=torch.uint8)
    whole[GUARD:GUARD + flat.size] = torch.from_numpy(flat)
    return whole, where


def crop_cases(P):
    """(name, image shapes, lead bytes, rows as (image, top, left))."""
    yield "exact", [(P, P)], 0, [(0, 0, 0)]
    yield "one odd left", [(P + 3, 67)], 0, [(0, 2, (67 - P - 1) | 1)]      # 65, 61, 51: up to the right edge or one short
    for lead in (0, 1, 2, 3):
        # 9 patches out of three images; the last one ends on the pool's last byte
        shapes = [(P + 2, 67), (P, P), (P + 5, P + 9)]
        rows = [(0, 1, 3), (1, 0, 0), (2, 5, 9), (0, 2, 67 - P), (2, 0, 1), (0, 0, 0), (1, 0, 0), (2, 3, 4),
                (2, 5, 9)]
        yield f"nine, lead {lead}", shapes, lead, rows


@pytest.mark.parametrize("P", [1, 5, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_crop_patches_equals_the_twin(dtype, P):
    for name, shapes, lead, rows in crop_cases(P):
        whole, where = guarded_pool(shapes, lead, seed=P)
        pool = whole[GUARD:whole.numel() - GUARD]
        table = torch.tensor([[where[i][0], where[i][2], top, left] for i, top, left in rows])
        if name.startswith("nine"):
            off, h, w = where[2]
            assert where[0][0] % 4 == lead                                     # first pixels at every residue mod 4
            assert off + ((5 + P - 1) * w + 9 + P) * 3 == pool.numel()         # the patch's last byte is the pool's
        want = train_ops.crop_patches_reference(pool, table, P, dtype)
        assert np.array_equal(want.float().numpy(), train_ref.crop(pool.numpy(), table.numpy(), P).astype(np.float32))
        got = train_ops.crop_patches(whole.cuda()[GUARD:whole.numel() - GUARD], table, P, dtype)
        assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got.cpu(), want), (name, dtype, P)
        assert float(got.float().max()) < 255.0, (name, "a byte from outside the pool was used")


def test_crop_patches_checks_its_table_before_the_launch():
    pool = torch.zeros(3 * 8 * 8, dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="row 0.*the pool has 192"):
        train_ops.crop_patches(pool, torch.tensor([[0, 8, 5, 4]]), 4)
    with pytest.raises(ValueError, match="negative"):
        train_ops.crop_patches(pool, torch.tensor([[0, 8, -1, 4]]), 4)
    assert train_ops.crop_patches(pool, torch.zeros((0, 4), dtype=torch.int64), 4).shape == (0, 4, 4, 3)


# ---------------------------------------------------------------------------------------------------------------------

CHUNK, CAPACITY = train_ops.KERAS_ADAM_CHUNK, train_ops.KERAS_ADAM_CAPACITY
NUMELS = [1, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 0]


def adam_problem(seed=0):
    """CAPACITY + 1 parameters (two launches) plus one without a gradient; gradients of three steps with |g| in
    [1e-6, 1e3] or exactly 0."""
    rng = np.random.default_rng(seed)
    numels = [NUMELS[k % len(NUMELS)] for k in range(CAPACITY + 1)]
    params = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in numels]

    def grads():
        out = []
        for n in numels:
            g = 10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)
            g[rng.random(n) < 0.1] = 0.0
            out.append(torch.from_numpy(g.astype(np.float32)))
        return out
    return params, [grads() for _ in range(3)]


def test_keras_adam_step_equals_the_twin_bit_for_bit():
    assert CHUNK == 4096 and CAPACITY == 64
    params, steps = adam_problem()
    lr = 1e-3
    host = [p.clone() for p in params]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    dev = [torch.nn.Parameter(p.cuda()) for p in params]
    idle = torch.nn.Parameter(torch.randn(17).cuda())
    held = idle.detach().clone()
    opt = KerasAdam(dev + [idle], lr=lr)
    for t, grads in enumerate(steps, start=1):
        train_ops.keras_adam_reference(host, grads, ms, vs, lr=lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, step=t)
        for p, g in zip(dev, grads):
            p.grad = g.cuda()
        opt.step()
        for k, (p, want) in enumerate(zip(dev, host)):
            assert torch.equal(p.detach().cpu(), want), (t, k, p.numel())
            if p.numel():
                assert torch.equal(opt.state[p]["exp_avg"].cpu(), ms[k]), (t, k)
                assert torch.equal(opt.state[p]["exp_avg_sq"].cpu(), vs[k]), (t, k)
    assert opt.param_groups[0]["step"] == 3
    assert torch.equal(idle.detach(), held) and idle not in opt.state          # no gradient: left out
    # skip != 0: nothing is written
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in dev]
    opt.step(skip=torch.ones(1, dtype=torch.int32, device="cuda"))
    for p, (w, m, v) in zip(dev, before):
        assert torch.equal(p.detach(), w) and torch.equal(opt.state[p]["exp_avg"], m)
        assert torch.equal(opt.state[p]["exp_avg_sq"], v)
    # skip == 0: the step is taken, and the parameter's version says so (caches are keyed on it)
    version = dev[5]._version
    opt.step(skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert not torch.equal(dev[5].detach(), before[5][0])
    assert dev[5]._version > version


def test_keras_adam_takes_views_that_are_not_16_byte_aligned():
    """Parameters that are slices of one buffer start on any multiple of 4 bytes: those take the one-value path."""
    rng = np.random.default_rng(3)
    flat = torch.from_numpy(rng.standard_normal(300).astype(np.float32))
    cuts = [(1, 70), (70, 75), (77, 300)]
    grads = [torch.from_numpy(rng.standard_normal(b - a).astype(np.float32)) for a, b in cuts]
    host = [flat[a:b].clone() for a, b in cuts]
    ms, vs = [torch.zeros_like(p) for p in host], [torch.zeros_like(p) for p in host]
    train_ops.keras_adam_reference(host, grads, ms, vs, lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-7, step=1)
    dflat = flat.cuda()
    dev = [dflat[a:b] for a, b in cuts]
    dm, dv = [torch.zeros_like(p) for p in dev], [torch.zeros_like(p) for p in dev]
    train_ops.keras_adam(dev, [g.cuda() for g in grads], dm, dv, lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-7, step=1)
    for p, want in zip(dev, host):
        assert torch.equal(p.cpu(), want)
    untouched = torch.ones(300, dtype=torch.bool)
    for a, b in cuts:
        untouched[a:b] = False
    assert torch.equal(dflat.cpu()[untouched], flat[untouched])
