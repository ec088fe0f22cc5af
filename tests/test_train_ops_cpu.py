"""CPU tier of the training path: the tensor-op twins of ops/train_ops.py against the definitions of tests/train_ref.py,
PatchDataset, KerasAdam and Trainer on CPU tensors."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import train_ref
from compression_amd import KerasAdam, PatchDataset, synthetic
from compression_amd.models import Trainer, write_png
from compression_amd.ops import train_ops

HYPER = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7)
KINDS = ("zero", "random", "steady", "opposed", "sparse")
STEPS = (1, 2, 3, 10, 100, 500, 1000, 2000)


def adam_case(kind, seed, n=257):
    """float32 p, g, m, v of one case: |g| log-uniform in [1e-6, 1e3] with a random sign."""
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    if kind == "sparse":
        g[rng.permutation(n)[: n // 5]] = 0.0
    if kind == "zero":
        m, v = np.zeros_like(g), np.zeros_like(g)
    elif kind in ("random", "sparse"):
        m = (g * rng.uniform(-2, 2, n)).astype(np.float32)
        v = (g.astype(np.float64) ** 2 * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
        v[g == 0] = (10.0 ** rng.uniform(-12, 2, int((g == 0).sum()))).astype(np.float32)
    elif kind == "steady":
        m, v = g.copy(), (g * g).astype(np.float32)
    else:       # opposed
        m, v = (-3 * g).astype(np.float32), (g.astype(np.float64) ** 2 * 1e-4).astype(np.float32)
    return p, g, m, v


def twin_step(p, g, m, v, lr, step):
    tp, tg, tm, tv = (torch.from_numpy(a.copy()) for a in (p, g, m, v))
    train_ops.keras_adam_reference([tp], [tg], [tm], [tv], lr=lr, step=step, **HYPER)
    assert torch.equal(tg, torch.from_numpy(g))
    return tp.numpy(), tm.numpy(), tv.numpy()


def test_keras_adam_reference_holds_the_float64_definition():
    """200 cases (5 kinds of state x 8 step counts x 5 seeds); the worst error of each quantity in units of its bound
    is printed; the worst are 0.68 of 4, 0.97 of 5 and 1.8 of 8 counted roundings."""
    worst = np.zeros(3)
    cases = 0
    for kind in KINDS:
        for step in STEPS:
            for seed in range(5):
                lr = (1e-4, 1e-3)[seed % 2]
                p, g, m, v = adam_case(kind, 1000 * step + seed)
                p1, m1, v1 = twin_step(p, g, m, v, lr, step)
                bounds = train_ref.adam_bounds(p, g, m, v, m1, v1, lr, step=step, **HYPER)
                for k, (got, (want, bound)) in enumerate(zip((m1, v1, p1), bounds)):
                    err = np.abs(got.astype(np.float64) - want)
                    ratio = err[bound > 0] / bound[bound > 0]
                    assert (err <= bound).all(), (kind, step, seed, "m' v' p'".split()[k], float(ratio.max()))
                    worst[k] = max(worst[k], float(ratio.max()))
                cases += 1
    print("worst error / bound for m', v', p':", worst, "times (4, 5, 8) roundings:", worst * (4, 5, 8))
    assert cases == 200


def test_keras_adam_reference_rounds_every_operation_once():
    """Bit for bit the numpy float32 evaluation, whose operations (the square root included) are correctly rounded:
    what the kernel is compared with on the device must itself be the definition."""
    f = np.float32
    for kind, step in (("random", 1), ("zero", 7), ("sparse", 300)):
        p, g, m, v = adam_case(kind, 5, n=20000)
        alpha, c1, c2, eps = (f(c) for c in train_ops.keras_adam_constants(1e-3, step=step, **HYPER))
        m1 = m + (g - m) * c1
        v1 = v + (g * g - v) * c2
        p1 = p - (m1 * alpha) / (np.sqrt(v1) + eps)
        assert p1.dtype == m1.dtype == v1.dtype == np.float32
        got = twin_step(p, g, m, v, 1e-3, step)
        for name, a, b in zip(("p'", "m'", "v'"), got, (p1, m1, v1)):
            assert np.array_equal(a, b), (kind, name, int((a != b).sum()))


def test_torch_adam_is_a_different_rule():
    """torch.optim.Adam with the same hyper-parameters misses the p' bound where it matters most: first step, small g."""
    rng = np.random.default_rng(7)
    n, lr = 257, 1e-4
    g = (10.0 ** rng.uniform(-6, -5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    zero = np.zeros_like(g)
    p1, m1, v1 = twin_step(p, g, zero, zero, lr, 1)
    want, bound = train_ref.adam_bounds(p, g, zero, zero, m1, v1, lr, step=1, **HYPER)[2]
    assert (np.abs(p1.astype(np.float64) - want) <= bound).all()
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    w.grad = torch.from_numpy(g.copy())
    torch.optim.Adam([w], lr=lr, betas=(HYPER["beta_1"], HYPER["beta_2"]), eps=HYPER["epsilon"]).step()
    err = np.abs(w.detach().numpy().astype(np.float64) - want)
    assert (err > bound).all()


def make_pool(shapes, seed=0, guard=0):
    """Images of the given (H, W) back to back -> (pool, [(offset, H, W)]); `guard` bytes of 0xFF around the pool, of
    which the pool is an inner slice."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 255, (h, w, 3), dtype=np.uint8) for h, w in shapes]      # 0xFF never occurs inside
    flat = np.concatenate([im.reshape(-1) for im in images])
    whole = torch.full((flat.size + 2 * guard,), 0xFF, dtype=torch.uint8)
    whole[guard:guard + flat.size] = torch.from_numpy(flat)
    where, at = [], 0
    for h, w in shapes:
        where.append((at, h, w))
        at += 3 * h * w
    return whole[guard:guard + flat.size], where


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.bfloat16])
def test_crop_patches_reference_equals_slicing(dtype):
    pool, where = make_pool([(9, 7), (16, 16), (5, 67)], guard=11)
    for P in (1, 5):
        table = torch.tensor([[off, w, (h - P) // 2, w - P] for off, h, w in where] + [[where[0][0], where[0][2], 0, 0]])
        got = train_ops.crop_patches_reference(pool, table, P, dtype)
        assert got.dtype == dtype and got.shape == (4, P, P, 3)
        assert np.array_equal(got.float().numpy(), train_ref.crop(pool.numpy(), table.numpy(), P).astype(np.float32))
        assert torch.equal(train_ops.crop_patches(pool, table, P, dtype), got)          # a CPU pool takes the twin
    assert train_ops.crop_patches_reference(pool, torch.zeros((0, 4), dtype=torch.int64), 4, dtype).shape == (0, 4, 4, 3)


def test_crop_patches_rejects_bad_rows():
    pool, where = make_pool([(8, 8), (6, 10)])
    off, h, w = where[1]
    good = [off, w, h - 4, w - 4]          # its last byte is the pool's last byte
    train_ops.crop_patches(pool, torch.tensor([good]), 4)
    for column in range(4):
        row = list(good)
        row[column] = -1
        with pytest.raises(ValueError, match="row 1 has a negative entry"):
            train_ops.crop_patches(pool, torch.tensor([good, row]), 4)
    with pytest.raises(ValueError, match=f"row 2.*ends at byte {pool.numel() + 1}, the pool has {pool.numel()}"):
        train_ops.crop_patches(pool, torch.tensor([good, good, [off + 1, w, h - 4, w - 4]]), 4)
    with pytest.raises(ValueError, match="row 0"):
        train_ops.crop_patches(pool, torch.tensor([[off, w, h - 3, w - 4]]), 4)
    with pytest.raises(ValueError, match="row 0.*must not exceed 2\\^24"):
        train_ops.crop_patches(pool, torch.tensor([[0, 2 ** 24 + 1, 0, 0]]), 1)
    with pytest.raises(TypeError):
        train_ops.crop_patches(pool, torch.tensor([good], dtype=torch.int32), 4)
    with pytest.raises(TypeError):
        train_ops.crop_patches(pool, torch.tensor([good]), 4, torch.float16)


# ---------------------------------------------------------------------------------------------------------------------
# PatchDataset

SHAPES = [(64, 64), (80, 96), (65, 67), (70, 64), (64, 90)]


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("patches")
    for k, (h, w) in enumerate(SHAPES):
        write_png(root / f"im{k}.png", synthetic.lowpass_images(1, h, w, seed=20 + k)[0])
    return root


def expected_batch(files, triples, P):
    from compression_amd.models import read_png
    return torch.stack([read_png(files[i])[t:t + P, l:l + P] for i, t, l in triples])


def test_patch_dataset_delivers_its_plan(png_dir):
    ds = PatchDataset(str(png_dir / "*.png"), 32, 2, repeat=True, seed=3, dtype=torch.uint8)
    assert len(ds.files) == 5
    plan = ds.plan(7)             # 14 items: beyond two passes of 5
    assert len(plan) == 7 and all(len(b) == 2 for b in plan)
    assert ds.plan(7) == plan     # nothing was consumed
    for triples in plan:
        batch = next(ds)
        assert batch.shape == (2, 32, 32, 3) and batch.dtype == torch.uint8
        assert torch.equal(batch, expected_batch(ds.files, triples, 32))
    items = [t for b in plan for t in b]
    for k in (0, 5):              # every pass is a permutation of the files, and the crops stay inside the images
        assert sorted(i for i, _, _ in items[k:k + 5]) == list(range(5))
    for i, top, left in items:
        assert 0 <= top <= SHAPES[i][0] - 32 and 0 <= left <= SHAPES[i][1] - 32
    assert next(PatchDataset(str(png_dir / "*.png"), 32, 2, repeat=True, seed=3)).dtype == torch.float32


def test_patch_dataset_single_pass_and_reshuffle(png_dir):
    ds = PatchDataset(str(png_dir / "*.png"), 64, 2, repeat=False, seed=1, dtype=torch.uint8)
    orders = []
    for _ in range(6):
        plan = ds.plan(10)
        assert len(plan) == 2                          # 5 files, batches of 2: the remainder is dropped
        batches = list(ds)
        assert len(batches) == 2
        used = [i for b in plan for i, _, _ in b]
        assert len(set(used)) == 4
        for triples, batch in zip(plan, batches):
            assert torch.equal(batch, expected_batch(ds.files, triples, 64))
        orders.append(tuple(used))
    assert len(set(orders)) > 1                        # reshuffle_each_iteration
    with pytest.raises(StopIteration):
        it = iter(ds)
        for _ in range(3):
            next(it)


def test_patch_dataset_seed_and_pool_limit(png_dir):
    def take(n, **kw):
        ds = PatchDataset(str(png_dir / "*.png"), 48, 2, repeat=True, dtype=torch.uint8, **kw)
        return [next(ds) for _ in range(n)]
    a = take(9, seed=5)
    b = take(9, seed=5)
    c = take(9, seed=6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))
    two_of_five = sorted(3 * h * w for h, w in SHAPES)[-1] * 2
    small = PatchDataset(str(png_dir / "*.png"), 48, 2, repeat=True, dtype=torch.uint8, seed=5, pool_limit_bytes=two_of_five)
    assert not small._fits
    d = [next(small) for _ in range(9)]
    assert all(torch.equal(x, y) for x, y in zip(a, d))
    one = PatchDataset(str(png_dir / "*.png"), 48, 2, repeat=False, dtype=torch.uint8, seed=5, pool_limit_bytes=1)
    whole = PatchDataset(str(png_dir / "*.png"), 48, 2, repeat=False, dtype=torch.uint8, seed=5)
    for _ in range(2):
        assert all(torch.equal(x, y) for x, y in zip(list(one), list(whole)))


def test_patch_dataset_errors(png_dir, tmp_path):
    pattern = str(tmp_path / "nothing" / "*.png")
    with pytest.raises(RuntimeError) as e:
        PatchDataset(pattern, 32, 2, repeat=True)
    assert str(e.value) == f"No training images found with glob '{pattern}'."
    with pytest.raises(ValueError, match=r"im3\.png is 70 x 64, smaller than the 65 x 65 patch"):
        PatchDataset([str(png_dir / f"im{k}.png") for k in (1, 2, 3)], 65, 2, repeat=True)
    with pytest.raises(TypeError):
        PatchDataset(str(png_dir / "*.png"), 32, 2, repeat=True, dtype=torch.float16)


@pytest.mark.parametrize("limit", [2 ** 32, 40000])
def test_patch_dataset_state_round_trip(png_dir, limit):
    kw = dict(repeat=True, seed=9, dtype=torch.uint8, pool_limit_bytes=limit)
    ds = PatchDataset(str(png_dir / "*.png"), 40, 2, **kw)
    for _ in range(4):            # into the second pass
        next(ds)
    ds.plan(6)                    # looking ahead does not move the state
    state = ds.state_dict()
    rest = [next(ds) for _ in range(6)]
    other = PatchDataset(str(png_dir / "*.png"), 40, 2, **kw)
    next(other)
    other.load_state_dict(state)
    assert all(torch.equal(x, next(other)) for x in rest)
    with pytest.raises(ValueError, match="batchsize"):
        PatchDataset(str(png_dir / "*.png"), 40, 3, **kw).load_state_dict(state)


# ---------------------------------------------------------------------------------------------------------------------
# KerasAdam


def test_keras_adam_state_dict_and_missing_gradients():
    torch.manual_seed(0)
    a, b, unused = (torch.nn.Parameter(torch.randn(n)) for n in (5, 70, 3))
    opt = KerasAdam([a, b, unused], lr=1e-2)
    assert opt.defaults["epsilon"] == 1e-7 and opt.defaults["beta_1"] == 0.9 and opt.defaults["beta_2"] == 0.999

    def one_step(params, optimizer):
        for p in params[:2]:
            p.grad = torch.sin(p.detach() * 3)
        optimizer.step()

    before = unused.detach().clone()
    one_step([a, b], opt)
    assert torch.equal(unused, before) and unused not in opt.state       # no gradient: left out
    assert set(opt.state[a]) == {"exp_avg", "exp_avg_sq"} and opt.param_groups[0]["step"] == 1
    # the step is the twin's
    p = torch.nn.Parameter(torch.randn(9))
    g = torch.randn(9)
    want, m, v = p.detach().clone(), torch.zeros(9), torch.zeros(9)
    train_ops.keras_adam_reference([want], [g], [m], [v], lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, step=1)
    p.grad = g
    KerasAdam([p]).step()
    assert torch.equal(p.detach(), want)
    # round trip: a copy restored from state_dict() continues bit for bit, with a changed lr
    a2, b2, unused2 = (torch.nn.Parameter(t.detach().clone()) for t in (a, b, unused))
    opt2 = KerasAdam([a2, b2, unused2], lr=1.0)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))     # as through a file: no shared tensors
    assert opt2.param_groups[0]["step"] == 1 and opt2.param_groups[0]["lr"] == 1e-2
    for o in (opt, opt2):
        o.param_groups[0]["lr"] = 3e-3
    one_step([a, b], opt)
    one_step([a2, b2], opt2)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    # skip on the CPU
    held = a.detach().clone()
    a.grad = torch.ones_like(a)
    opt.step(skip=torch.ones(1, dtype=torch.int32))
    assert torch.equal(a, held)
    assert float(opt.step(lambda: torch.tensor(2.5))) == 2.5               # torch's calling convention: the closure first
    assert not torch.equal(a, held)
    opt.zero_grad()
    assert a.grad is None


def test_keras_adam_rejects_other_types():
    p = torch.nn.Parameter(torch.randn(4, dtype=torch.float64))
    p.grad = torch.randn(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="float32"):
        KerasAdam([p]).step()
    q = torch.nn.Parameter(torch.randn(4, 6).t())
    q.grad = torch.randn(6, 4)
    assert not q.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        KerasAdam([q]).step()
    r = torch.nn.Parameter(torch.randn(4, 6))
    r.grad = torch.randn(6, 4).t()
    with pytest.raises(ValueError, match="contiguous"):
        KerasAdam([r]).step()
    with pytest.raises(ValueError):
        KerasAdam([r], beta_1=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# Trainer


class Tiny(torch.nn.Module):
    """forward(x, training) -> (loss, bpp, mse) with training-time noise from torch's generator, as the models have."""

    def __init__(self, nan_at=None):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(3))
        self.calls, self.nan_at, self.compression = 0, nan_at, 0

    def forward(self, x, training=True):
        y = x.float().mean(dim=(0, 1, 2)) / 255.0 * self.w + (torch.rand(3) * 0.01 if training else 0.0)
        bpp, mse = self.w.abs().mean(), ((y - 0.5) ** 2).mean()
        loss = bpp + 0.01 * mse
        if training:
            if self.calls == self.nan_at:
                loss = loss * float("nan")
            self.calls += 1
        return loss, bpp, mse

    def init_compression(self):
        self.compression += 1
        return self


def tiny_run(png_dir, seed=11, **kw):
    torch.manual_seed(seed)
    model = Tiny(**kw)
    data = PatchDataset(str(png_dir / "*.png"), 32, 2, repeat=True, seed=2)
    return model, data


def test_trainer_metric_means(png_dir):
    model, data = tiny_run(png_dir)
    trainer = Trainer(model)
    values = [[float(v) for v in trainer.train_step(next(data))] for _ in range(5)]
    assert isinstance(trainer.optimizer, KerasAdam) and trainer.optimizer.defaults["lr"] == 1e-4      # the default
    got = trainer.result()
    for k, name in enumerate(("loss", "bpp", "mse")):
        assert got[name] == pytest.approx(np.mean([v[k] for v in values]), rel=1e-6)
    trainer.reset_metrics()
    w = model.w.detach().clone()
    loss, bpp, mse = trainer.test_step(next(data))
    assert torch.equal(model.w, w) and not loss.requires_grad
    assert trainer.result("val_")["val_bpp"] == pytest.approx(float(bpp), rel=1e-6)


class Interrupted(Exception):
    pass


class StopsAfter:
    """A dataset that fails after `count` batches, the way a killed job stops between two epochs."""

    def __init__(self, data, count):
        self.data, self.left = data, count

    def __iter__(self):
        return self

    def __next__(self):
        if self.left == 0:
            raise Interrupted
        self.left -= 1
        return next(self.data)

    def state_dict(self):
        return self.data.state_dict()

    def load_state_dict(self, state):
        self.data.load_state_dict(state)


def test_trainer_fit_backup_and_resume(png_dir, tmp_path):
    def validation():
        return PatchDataset(str(png_dir / "*.png"), 32, 2, repeat=False, seed=3)

    # one run of two epochs
    model, data = tiny_run(png_dir)
    path = tmp_path / "whole"
    history = Trainer(model, KerasAdam(model.parameters(), lr=1e-2), train_path=path).fit(
        data, 2, 3, validation_data=validation())
    assert len(history) == 2 and set(history[0]) == {"loss", "bpp", "mse", "val_loss", "val_bpp", "val_mse"}
    assert all(np.isfinite(list(h.values())).all() for h in history)
    assert model.compression == 1                       # fit() ends with init_compression()
    lines = [json.loads(line) for line in open(path / "metrics.jsonl")]
    assert [line["epoch"] for line in lines] == [1, 2]
    assert all(lines[k][name] == history[k][name] for k in range(2) for name in history[k])
    assert not os.path.exists(path / "backup.pt")       # removed when training completes
    # the same, stopped after the first epoch ...
    first, data1 = tiny_run(png_dir)
    path = tmp_path / "parts"
    with pytest.raises(Interrupted):
        Trainer(first, KerasAdam(first.parameters(), lr=1e-2), train_path=path).fit(
            StopsAfter(data1, 3), 2, 3, validation_data=validation())
    assert os.path.exists(path / "backup.pt") and not os.path.exists(str(path / "backup.pt") + ".tmp")
    assert first.compression == 0
    # ... and continued by a fresh model, optimiser and dataset
    second, data2 = tiny_run(png_dir, seed=99)
    assert not torch.equal(second.w, first.w)
    torch.rand(5)
    resumed = Trainer(second, KerasAdam(second.parameters(), lr=1.0), train_path=path).fit(
        data2, 2, 3, validation_data=validation())
    assert resumed == history
    assert torch.equal(second.w, model.w)
    assert not os.path.exists(path / "backup.pt")
    assert [json.loads(line)["epoch"] for line in open(path / "metrics.jsonl")] == [1, 2]


def test_trainer_terminates_on_nan(png_dir, capsys, tmp_path):
    model, data = tiny_run(png_dir, nan_at=3)
    trainer = Trainer(model, KerasAdam(model.parameters(), lr=1e-2), train_path=tmp_path)
    history = trainer.fit(data, 3, 6)
    # the line of that epoch is JSON all the same: a mean that is not finite is null
    (line,) = open(tmp_path / "metrics.jsonl").read().splitlines()
    assert "NaN" not in line and json.loads(line)["loss"] is None and json.loads(line)["bpp"] is not None
    assert trainer.stop_message == "Batch 3: Invalid loss, terminating training"
    assert trainer.stop_message in capsys.readouterr().out
    assert len(history) == 1 and model.calls == 6
    # the weights are the ones after batch 2
    reference, data = tiny_run(png_dir)
    other = Trainer(reference, KerasAdam(reference.parameters(), lr=1e-2))
    for _ in range(3):
        other.train_step(next(data))
    assert torch.equal(model.w, reference.w) and torch.isfinite(model.w).all()
    # the flag is sticky within one fit() only: the next one trains on
    assert len(trainer.fit(data, 1, 2)) == 1 and trainer.stop_message is None and model.calls == 8
    assert not torch.equal(model.w, reference.w)
    # with a check after every step it stops at once
    model, data = tiny_run(png_dir, nan_at=3)
    trainer = Trainer(model, KerasAdam(model.parameters(), lr=1e-2), nan_check_every=1)
    trainer.fit(data, 3, 6)
    assert model.calls == 4 and torch.equal(model.w, reference.w)
