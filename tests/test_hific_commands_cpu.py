"""CPU tier of HiFiC's train and evaluate commands (models/hific_train.py, models/hific_evaluate.py): the command line
and the checkpoint helpers; nothing here needs a device."""
import numpy as np
import pytest
import torch

from compression_amd import models
from compression_amd.models import hific_evaluate, hific_train


@pytest.fixture
def png_glob(tmp_path):
    rng = np.random.default_rng(0)
    models.write_png(tmp_path / "im0.png", rng.integers(0, 256, (40, 48, 3), dtype=np.uint8))
    return str(tmp_path / "*.png")


def test_parse_num_steps():
    assert hific_train._parse_num_steps("300") == 300
    assert hific_train._parse_num_steps("5k") == 5000
    assert hific_train._parse_num_steps("1M") == 1000000
    for bad in ("x", "k", "1.5k", "3G"):
        with pytest.raises(ValueError, match="Invalid num_steps"):
            hific_train._parse_num_steps(bad)


def test_flags_and_their_defaults(tmp_path):
    args = hific_train.parse_args(["--config", "hific", "--ckpt_dir", str(tmp_path)])
    assert (args.num_steps, args.batch_size, args.crop_size, args.seed) == (1000000, 8, 256, 0)
    assert args.images_glob is None and args.lpips_weight_path is None and not args.no_lpips
    assert args.init_autoencoder_from_ckpt_dir is None and args.precision_policy is None
    assert args.model_kwargs is None and args.discriminator_kwargs is None
    args = hific_train.parse_args(["--config", "mselpips", "--ckpt_dir", "a", "--num_steps", "5k", "--no-image-summaries",
                                   "--init_autoencoder_from_ckpt_dir", "b", "--crop_size", "64", "--no_lpips"])
    assert args.config == "mselpips" and args.num_steps == 5000 and args.crop_size == 64 and args.no_lpips
    with pytest.raises(SystemExit):
        hific_train.parse_args(["--config", "other", "--ckpt_dir", "a"])
    with pytest.raises(ValueError, match="Invalid num_steps"):
        hific_train.parse_args(["--config", "hific", "--ckpt_dir", "a", "--num_steps", "x"])
    args = hific_evaluate.parse_args(["--config", "hific", "--ckpt_dir", "a", "--out_dir", "o", "--max_images", "2"])
    assert args.max_images == 2 and args.images_glob is None


def test_the_same_folder_twice_raises(tmp_path):
    with pytest.raises(ValueError, match="continuing training is the default"):
        hific_train.parse_args(["--config", "hific", "--ckpt_dir", str(tmp_path), "--init_autoencoder_from_ckpt_dir",
                                str(tmp_path)])
    with pytest.raises(ValueError, match="continuing training is the default"):
        hific_train.train("hific", tmp_path, 1, images_glob="x/*.png", no_lpips=True,
                          init_autoencoder_from_ckpt_dir=tmp_path)


def test_missing_input_and_missing_lpips_stop_the_command(tmp_path, png_glob):
    common = ["--config", "hific", "--ckpt_dir", str(tmp_path / "ckpt")]
    with pytest.raises(SystemExit, match="TFDS"):
        hific_train.main(common)
    with pytest.raises(SystemExit, match="--lpips_weight_path.*--no_lpips"):
        hific_train.main(common + ["--images_glob", png_glob])
    with pytest.raises(ValueError, match="mixed_float16"):
        hific_train.main(common + ["--images_glob", png_glob, "--no_lpips", "--precision_policy", "mixed_float16"])
    with pytest.raises(SystemExit, match="TFDS"):
        hific_evaluate.main(common + ["--out_dir", str(tmp_path / "out")])
    assert not (tmp_path / "ckpt").exists() and not (tmp_path / "out").exists()


def test_checkpoint_helpers_pick_the_newest_and_keep_five(tmp_path):
    folder = tmp_path / "ckpt"
    assert hific_train.checkpoint_steps(folder) == [] and hific_train.latest_checkpoint(folder) is None
    for step in (2, 9, 10):
        path = hific_train.save_checkpoint(folder, {"step": step}, step)
        assert path == str(folder / f"ckpt-{step}.pt")
    (folder / "metrics.jsonl").write_text("{}\n")
    (folder / "ckpt-99.pt.tmp").write_text("a run that was killed while it wrote")
    (folder / "ckpt-x.pt").write_text("")
    assert hific_train.checkpoint_steps(folder) == [2, 9, 10]               # by number, not by name
    assert hific_train.latest_checkpoint(folder) == str(folder / "ckpt-10.pt")
    assert torch.load(hific_train.latest_checkpoint(folder))["step"] == 10
    for step in (11, 12, 13, 14):
        hific_train.save_checkpoint(folder, {"step": step}, step)
    assert hific_train.checkpoint_steps(folder) == [10, 11, 12, 13, 14]
    assert not list(folder.glob("ckpt-1[0-4].pt.tmp"))
    hific_train.save_checkpoint(folder, {"step": 14, "again": True}, 14)      # the same step again replaces its file
    assert hific_train.checkpoint_steps(folder) == [10, 11, 12, 13, 14]
    assert torch.load(hific_train.latest_checkpoint(folder))["again"]


def test_commands_fail_loudly_without_device(tmp_path, png_glob):
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hific_train.train("hific", tmp_path / "ckpt", 1, images_glob=png_glob, no_lpips=True)
    hific_train.save_checkpoint(tmp_path / "done", {"model": {}}, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hific_evaluate.eval_trained_model("hific", tmp_path / "done", tmp_path / "out", png_glob)
    from compression_amd import ScaledPatchDataset
    from compression_amd.ops import train_ops
    with pytest.raises(RuntimeError):
        next(ScaledPatchDataset(png_glob, 16, 1, repeat=True, device="cuda"))
    assert not train_ops.scale_crop_patches(torch.zeros(12, dtype=torch.uint8), torch.tensor([[0, 2, 2, 3, 3, 0, 0]]),
                                            2).is_cuda
