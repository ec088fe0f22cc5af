"""GPU tier of training: Trainer on the image models, resume from a backup, and the `train` command followed by
`compress` / `decompress` of what it wrote."""
import os

import numpy as np
import pytest
import torch

from compression_amd import KerasAdam, PatchDataset, models, synthetic
from compression_amd.models import codec_io
from compression_amd.models.train import Trainer

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (80, 96), (65, 67), (70, 64), (64, 90)]


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_images")
    for k, (h, w) in enumerate(SHAPES):
        models.write_png(root / f"im{k}.png", synthetic.lowpass_images(1, h, w, seed=40 + k)[0])
    return root


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


def fresh(png_dir, seed=0):
    torch.manual_seed(seed)
    model = models.BLS2017Model(num_filters=32).cuda()
    data = PatchDataset(str(png_dir / "*.png"), 64, 2, repeat=True, seed=1, device="cuda")
    return model, data


def validation(png_dir):
    return PatchDataset(str(png_dir / "*.png"), 64, 2, repeat=False, seed=2, device="cuda")


def weights(model):
    return {k: v.detach().cpu().clone() for k, v in model.named_parameters()}


@pytest.fixture(scope="module")
def whole_run(png_dir, tmp_path_factory):
    """Two epochs of two steps without interruption: (model, history)."""
    model, data = fresh(png_dir)
    path = tmp_path_factory.mktemp("whole")
    history = Trainer(model, train_path=path).fit(data, 2, 2, validation_data=validation(png_dir))
    assert not os.path.exists(path / "backup.pt")
    return model, history


def test_trainer_trains_bls2017_and_leaves_it_ready_to_code(whole_run, png_dir):
    model, history = whole_run
    assert len(history) == 2
    assert all(set(h) == {"loss", "bpp", "mse", "val_loss", "val_bpp", "val_mse"} for h in history)
    assert all(np.isfinite(list(h.values())).all() for h in history)
    assert model.entropy_model is not None
    x = models.read_png(png_dir / "im2.png").cuda()
    strings, x_shape, y_shape = model.compress(x)
    x_hat = model.decompress(strings, x_shape, y_shape)
    assert x_hat.shape == (1, 65, 67, 3) and x_hat.dtype == torch.uint8
    again, _, _ = model.compress(x)
    assert bytes(again[0]) == bytes(strings[0])


def test_trainer_resumes_from_its_backup(whole_run, png_dir, tmp_path):
    """An interrupted and resumed run against the uninterrupted one.  No kernel of the training step uses float atomics,
    so two uninterrupted runs are bit-equal on the device (asserted first), and the resumed run must be too."""
    model, history = whole_run
    want = weights(model)
    twin, data = fresh(png_dir)
    Trainer(twin, train_path=tmp_path / "twin").fit(data, 2, 2, validation_data=validation(png_dir))
    spread = {k: float((v - want[k]).abs().max()) for k, v in weights(twin).items()}
    assert max(spread.values()) == 0.0, f"two uninterrupted runs differ by up to {spread}"
    # stopped after the first epoch ...
    first, data1 = fresh(png_dir)
    path = tmp_path / "parts"
    with pytest.raises(Interrupted):
        Trainer(first, train_path=path).fit(StopsAfter(data1, 2), 2, 2, validation_data=validation(png_dir))
    assert os.path.exists(path / "backup.pt")
    # ... and continued by a fresh model, optimiser and dataset
    second, data2 = fresh(png_dir, seed=5)
    resumed = Trainer(second, train_path=path).fit(data2, 2, 2, validation_data=validation(png_dir))
    assert len(resumed) == 2 and not os.path.exists(path / "backup.pt")
    got = weights(second)
    assert all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])]
    assert resumed == history


def test_patch_dataset_on_the_device_equals_the_cpu_path(png_dir):
    """Both pool modes on the device (everything resident; runs of batches decoded in the background into pinned
    slices) deliver the batches of the CPU path, bit for bit."""
    kw = dict(repeat=True, seed=4, dtype=torch.bfloat16)
    want = PatchDataset(str(png_dir / "*.png"), 48, 2, **kw)
    whole = PatchDataset(str(png_dir / "*.png"), 48, 2, device="cuda", **kw)
    sliced = PatchDataset(str(png_dir / "*.png"), 48, 2, device="cuda", pool_limit_bytes=2 * 3 * 80 * 96, **kw)
    assert whole._fits and not sliced._fits
    for _ in range(9):
        x = next(want)
        a, b = next(whole), next(sliced)
        assert a.is_cuda and b.is_cuda and a.dtype == torch.bfloat16
        assert torch.equal(a.cpu(), x) and torch.equal(b.cpu(), x)
    sliced.close()


@pytest.mark.parametrize("which", ["bmshj2018", "ms2020"])
def test_one_train_step_moves_every_parameter(which):
    torch.manual_seed(3)
    model = {"bmshj2018": lambda: models.BMSHJ2018Model(num_filters=64),
             "ms2020": lambda: models.MS2020Model(num_filters=32, latent_depth=64, hyperprior_depth=32, num_slices=2,
                                                  max_support_slices=1)}[which]().cuda()
    x = torch.from_numpy(synthetic.lowpass_images(2, 64, 64, seed=7)).cuda().float()
    with torch.no_grad():
        model(x, training=False)              # the GDN layers create their parameters on the first call
        if which == "ms2020":
            # ms2020 feeds its hyper-synthesis transforms round(z) (ms2020.py:215), and a freshly initialised model
            # has |z| < 0.5 everywhere: they then see zeros, their ReLUs pass no gradient and Adam rightly leaves
            # them alone.  A trained model has a side latent; the bias-free last hyper-analysis layer is scaled so
            # that this one has too.
            z = model.hyper_analysis_transform(model.analysis_transform(x))
            for p in model.hyper_analysis_transform.layer_2.parameters():
                p.mul_(3.0 / float(z.abs().max()))
            assert float(model.hyper_analysis_transform(model.analysis_transform(x)).abs().max()) > 2.0
    before = weights(model)
    trainer = Trainer(model)
    loss, bpp, mse = trainer.train_step(x)
    assert isinstance(trainer.optimizer, KerasAdam)
    assert len(trainer.optimizer.param_groups[0]["params"]) == len(before)      # the lazily created ones included
    assert torch.isfinite(loss) and bpp > 0 and mse > 0
    missing = [n for n, p in model.named_parameters() if p.grad is None]
    assert not missing, f"parameters without gradient: {missing}"
    still = [n for n, p in model.named_parameters() if torch.equal(p.detach().cpu(), before[n])]
    assert not still, f"parameters that did not change: {still}"
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert trainer.result()["loss"] == pytest.approx(float(loss), rel=1e-6)


def test_train_command_then_compress_and_decompress(png_dir, tmp_path):
    model_path = str(tmp_path / "model.pt")
    common = ["--model_path", model_path, "--num_filters", "32"]
    assert codec_io.main(models.BLS2017Model, common + [
        "train", "--train_glob", str(png_dir / "*.png"), "--epochs", "1", "--steps_per_epoch", "2", "--patchsize", "64",
        "--batchsize", "2", "--max_validation_steps", "1", "--train_path", str(tmp_path / "train")]) == 0
    lines = open(tmp_path / "train" / "metrics.jsonl").read().splitlines()
    assert len(lines) == 1 and not os.path.exists(tmp_path / "train" / "backup.pt")
    source = str(png_dir / "im1.png")
    assert codec_io.main(models.BLS2017Model, common + ["compress", source, str(tmp_path / "im1.tfci")]) == 0
    assert codec_io.main(models.BLS2017Model, common + ["decompress", str(tmp_path / "im1.tfci"),
                                                        str(tmp_path / "im1.png")]) == 0
    assert models.read_png(tmp_path / "im1.png").shape == models.read_png(source).shape == (80, 96, 3)
    # the file carries the tables, and they are loaded, not regenerated: with another prior they stay as stored
    sd = torch.load(model_path, map_location="cpu")
    stored = [k for k in sd if k.endswith("_cdf")]
    assert stored
    prior = [k for k in sd if k.startswith("prior.") and sd[k].is_floating_point()]
    assert prior
    drifted = {k: (v + 0.05 * torch.randn_like(v) if k in prior else v) for k, v in sd.items()}
    receiver = codec_io.load_checkpoint(models.BLS2017Model(num_filters=32).cuda(), drifted)
    assert all(torch.equal(receiver.state_dict()[k].cpu(), sd[k]) for k in stored)
    with pytest.raises(SystemExit, match="TensorFlow Datasets"):
        codec_io.main(models.BLS2017Model, common + ["train"])
    with pytest.raises(ValueError, match="mixed_float16"):
        codec_io.main(models.BLS2017Model, common + ["train", "--train_glob", str(png_dir / "*.png"),
                                                     "--precision_policy", "mixed_float16"])
