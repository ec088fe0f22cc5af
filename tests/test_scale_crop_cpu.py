"""CPU tier of `scale_crop_patches` and `ScaledPatchDataset`: the tensor-op twin against the float64 definition
(tests/scale_crop_ref.py), its special cases, the table checks, and the dataset on the CPU path."""
import math

import numpy as np
import pytest
import torch

import scale_crop_ref
from compression_amd import ScaledPatchDataset, models
from compression_amd.ops import train_ops

# eight float32 roundings of at most half a unit in the last place of 256 (2^-16 each)
TOLERANCE = 2.0 ** -13


def random_cases(seed, count):
    """(pool, table, P): one image each, sides 1...40, scales on both sides of 1, P from 1 to the resized short side,
    every third patch in the bottom-right corner of the resized image."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        scale = float(rng.uniform(0.5, 1.0) if k % 2 else rng.uniform(1.0, 3.0))
        OH, OW = max(1, math.ceil(scale * H)), max(1, math.ceil(scale * W))
        P = int(rng.integers(1, min(OH, OW) + 1))
        lead = int(rng.integers(0, 4))
        pool, where = scale_crop_ref.random_pool([(H, W)], seed=1000 * seed + k, lead=lead)
        rows = []
        for n in range(3):
            corner = (k + n) % 3 == 0
            top = OH - P if corner else int(rng.integers(0, OH - P + 1))
            left = OW - P if corner else int(rng.integers(0, OW - P + 1))
            rows.append([where[0][0], W, H, OW, OH, top, left])
        yield torch.from_numpy(pool), torch.tensor(rows), P


def test_twin_equals_the_float64_definition():
    worst = 0.0
    for pool, table, P in random_cases(seed=3, count=150):
        got = train_ops.scale_crop_patches_reference(pool, table, P)
        assert got.dtype == torch.float32 and got.shape == (3, P, P, 3)
        want = scale_crop_ref.scale_crop(pool.numpy(), table.numpy(), P)
        worst = max(worst, float(np.abs(got.numpy().astype(np.float64) - want).max()))
        assert torch.equal(train_ops.scale_crop_patches(pool, table, P), got)          # a CPU pool takes the twin
        bf = train_ops.scale_crop_patches_reference(pool, table, P, torch.bfloat16)
        assert bf.dtype == torch.bfloat16 and torch.equal(bf, got.to(torch.bfloat16))
    print(f"worst deviation of the twin from the float64 definition: {worst:.3e}")
    assert worst <= TOLERANCE
    empty = train_ops.scale_crop_patches_reference(pool, torch.zeros((0, 7), dtype=torch.int64), 4)
    assert empty.shape == (0, 4, 4, 3)


def test_scale_one_equals_crop_patches():
    pool, where = scale_crop_ref.random_pool([(9, 13), (6, 6), (11, 7)], seed=5, lead=1)
    pool = torch.from_numpy(pool)
    P = 5
    rows = [(0, 4, 8), (1, 1, 0), (2, 6, 2), (0, 0, 0)]
    plain = torch.tensor([[where[i][0], where[i][2], t, l] for i, t, l in rows])
    scaled = torch.tensor([[where[i][0], where[i][2], where[i][1], where[i][2], where[i][1], t, l] for i, t, l in rows])
    want = train_ops.crop_patches_reference(pool, plain, P).to(torch.float32)
    assert torch.equal(train_ops.scale_crop_patches_reference(pool, scaled, P), want)


@pytest.mark.parametrize("side", [1, 2])
def test_upscaled_tiny_images_stay_in_range_and_repeat_their_edge(side):
    pool, _ = scale_crop_ref.random_pool([(side, side)], seed=side)
    image = pool.reshape(side, side, 3).astype(np.float32)
    new = 7
    out = train_ops.scale_crop_patches_reference(torch.from_numpy(pool), torch.tensor([[0, side, side, new, new, 0, 0]]),
                                                 new)[0].numpy()
    assert (out >= image.min(axis=(0, 1))).all() and (out <= image.max(axis=(0, 1))).all()
    # source row H - 1 has no row below it: from output row ceil((H - 1) OH / H) on, the rows repeat it
    first = math.ceil((side - 1) * new / side)
    assert first < new - 1
    assert (out[first:] == out[first]).all() and (out[:, first:] == out[:, first:first + 1]).all()
    assert np.array_equal(out[-1, -1], image[-1, -1])
    if side == 2:
        assert not (out[0] == out[-1]).all()


def test_table_rows_are_checked_and_named():
    H, W, P = 9, 8, 4
    pool = torch.zeros(5 + 3 * H * W, dtype=torch.uint8)
    good = [5, W, H, 12, 13, 13 - P, 12 - P]
    train_ops.scale_crop_patches(pool, torch.tensor([good]), P)
    for k in range(7):
        row = list(good)
        row[k] = -1
        with pytest.raises(ValueError, match="row 1 has a negative entry"):
            train_ops.scale_crop_patches(pool, torch.tensor([good, row]), P)
    with pytest.raises(ValueError, match="row 2.*does not fit the resized image of 13 x 12"):
        train_ops.scale_crop_patches(pool, torch.tensor([good, good, [5, W, H, 12, 13, 13 - P + 1, 0]]), P)
    with pytest.raises(ValueError, match="row 0.*does not fit"):
        train_ops.scale_crop_patches(pool, torch.tensor([[5, W, H, 12, 13, 0, 12 - P + 1]]), P)
    with pytest.raises(ValueError, match=f"row 1.*ends at byte {6 + 3 * H * W}, the pool has {5 + 3 * H * W}"):
        train_ops.scale_crop_patches(pool, torch.tensor([good, [6] + good[1:]]), P)
    with pytest.raises(ValueError, match=r"row 0.*must be in \[1, 2\^24\]"):
        train_ops.scale_crop_patches(pool, torch.tensor([[5, W, H, 0, 13, 0, 0]]), P)
    with pytest.raises(ValueError, match=r"row 0.*must be in \[1, 2\^24\]"):
        train_ops.scale_crop_patches(pool, torch.tensor([[5, W, H, 2 ** 24 + 1, 13, 0, 0]]), P)
    with pytest.raises(ValueError, match="patchsize"):
        train_ops.scale_crop_patches(pool, torch.tensor([good]), 0)
    with pytest.raises(ValueError, match="patchsize"):
        train_ops.scale_crop_patches(pool, torch.tensor([good]), 2 ** 15 + 1)
    with pytest.raises(ValueError, match=r"\[B, 7\]"):
        train_ops.scale_crop_patches(pool, torch.tensor([good[:4]]), P)
    with pytest.raises(TypeError):
        train_ops.scale_crop_patches(pool, torch.tensor([good], dtype=torch.int32), P)
    with pytest.raises(TypeError, match="not integers"):
        train_ops.scale_crop_patches(pool, torch.tensor([good]), P, torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the dataset

SHAPES = [(40, 52), (33, 70), (20, 45), (64, 31), (50, 50)]      # (20, 45) and (64, 31) have a side below the patch
P = 32


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("scaled_images")
    for k, (h, w) in enumerate(SHAPES):
        rng = np.random.default_rng(70 + k)
        models.write_png(root / f"im{k}.png", rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return root


def dataset(png_dir, **kw):
    kw = {"repeat": True, "seed": 4, **kw}
    return ScaledPatchDataset(str(png_dir / "*.png"), P, 2, **kw)


def cut_by_hand(png_dir, items):
    rows = []
    for i, oh, ow, top, left in items:
        image = models.read_png(png_dir / f"im{i}.png")
        h, w = image.shape[:2]
        rows.append(train_ops.scale_crop_patches_reference(image.reshape(-1), torch.tensor([[0, w, h, ow, oh, top, left]]),
                                                           P)[0])
    return torch.stack(rows)


def test_dataset_same_seed_same_batches_and_the_plan_tells_them(png_dir):
    a, b, other = dataset(png_dir), dataset(png_dir), dataset(png_dir, seed=5)
    plan = a.plan(7)
    assert a.plan(7) == plan                                   # consumes nothing
    assert len(plan) == 7 and all(len(items) == 2 for items in plan)
    differs = False
    for items in plan:
        x = next(a)
        assert x.shape == (2, P, P, 3) and x.dtype == torch.float32
        assert torch.equal(next(b), x)
        assert torch.equal(cut_by_hand(png_dir, items), x)
        differs |= not torch.equal(next(other), x)
    assert differs
    # every file once per pass of five
    files = [i for items in plan for i, *_ in items]
    assert sorted(files[:5]) == sorted(files[5:10]) == list(range(5))


def test_dataset_scales_lie_in_their_range_and_small_images_are_upscaled(png_dir):
    data = dataset(png_dir)
    seen = set()
    for i, oh, ow, top, left in (item for items in data.plan(40) for item in items):
        h, w = SHAPES[i]
        lo, hi = (float(v) for v in data.scale_range(i))
        assert lo == max(0.75, float(np.float32(P) / np.float32(min(h, w)))) and hi == max(lo, float(np.float32(0.95)))
        assert oh >= P and ow >= P and 0 <= top <= oh - P and 0 <= left <= ow - P
        # OH = max(ceil(scale H), P) with scale in [lo, hi]: ceil adds less than one, float32 rounds the product
        slack = 1.0 + 1e-5 * max(oh, ow)
        assert lo * h - slack < oh < max(hi * h, P) + slack and lo * w - slack < ow < max(hi * w, P) + slack
        if min(h, w) < P:
            assert lo > 1.0 and lo == hi and min(oh, ow) == P          # upscaled so that the short side just fits
        seen.add(i)
    assert seen == set(range(len(SHAPES)))


def test_dataset_state_continues_identically_mid_pass(png_dir):
    a = dataset(png_dir)
    for _ in range(3):                   # six items: one into the second pass
        next(a)
    state = a.state_dict()
    want = [next(a) for _ in range(6)]
    b = dataset(png_dir, seed=9)
    b.load_state_dict(state)
    assert all(torch.equal(next(b), x) for x in want)


def test_dataset_pool_limit_changes_no_batch(png_dir):
    whole = dataset(png_dir, dtype=torch.bfloat16)
    sliced = dataset(png_dir, dtype=torch.bfloat16, pool_limit_bytes=2 * 3 * 33 * 70)
    assert whole._fits and not sliced._fits
    for _ in range(9):
        x = next(whole)
        assert x.dtype == torch.bfloat16 and torch.equal(next(sliced), x)
    sliced.close()
    without_repeat = dataset(png_dir, repeat=False)
    assert len(list(without_repeat)) == 2 and len(list(without_repeat)) == 2
    with pytest.raises(TypeError, match="not integers"):
        dataset(png_dir, dtype=torch.uint8)
