"""GPU tier of HiFiC's train and evaluate commands on small networks: resuming from a checkpoint bit for bit, the
configuration without a discriminator, the perceptual term, initialising the autoencoder from another run, evaluation
of the trained model, and both command lines as child processes."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from compression_amd import models, synthetic
from compression_amd.models import codec_io, hific_evaluate, hific_train
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODEL_KW = dict(num_filters_base=4, num_filters_bottleneck=6, num_filters_hyper=8, num_residual_blocks=1)
DISC_KW = dict(num_filters_base=16, in_channels_latent=6)
CROP = 32
SHAPES = [(48, 56), (40, 70), (30, 45), (64, 64)]           # one with a side below the crop size


@pytest.fixture(scope="module")
def png_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("hific_images")
    for k, (h, w) in enumerate(SHAPES):
        models.write_png(root / f"im{k}.png", synthetic.lowpass_images(1, h, w, seed=60 + k)[0])
    return root


def run(png_dir, ckpt_dir, num_steps, config="hific", **kw):
    kw = {"no_lpips": True, **kw}
    return hific_train.train(config, ckpt_dir, num_steps, images_glob=str(png_dir / "*.png"), batch_size=2, crop_size=CROP,
                             seed=3, save_checkpoint_steps=2, model_kwargs=MODEL_KW,
                             discriminator_kwargs=DISC_KW if config == "hific" else None, **kw)


def tensors(trainer):
    out = {"model." + k: v.detach().cpu().clone() for k, v in trainer.model.state_dict().items()}
    if trainer.discriminator is not None:
        out.update({"disc." + k: v.detach().cpu().clone() for k, v in trainer.discriminator.state_dict().items()})
    return out


def differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def steps_in(folder):
    return hific_train.checkpoint_steps(folder)


@pytest.fixture(scope="module")
def whole_run(png_dir, tmp_path_factory):
    """Four steps without interruption: (checkpoint folder, every tensor of model and discriminator)."""
    folder = tmp_path_factory.mktemp("whole")
    trainer = run(png_dir, folder, 4)
    assert trainer.step == 4 and trainer.step_disc == 4
    return folder, tensors(trainer)


def test_train_resumes_bit_for_bit(whole_run, png_dir, tmp_path):
    folder, want = whole_run
    assert any(k.endswith("_cdf") for k in want) and any(k.startswith("disc.") for k in want)
    twin = tensors(run(png_dir, tmp_path / "twin", 4))
    assert differing(twin, want) == [], "two uninterrupted runs differ"
    # stopped after step 2 ...
    first = run(png_dir, tmp_path / "parts", 2)
    assert first.step == 2 and steps_in(tmp_path / "parts") == [2]
    assert len(differing(tensors(first), want)) > 0
    # ... and continued from the folder
    second = run(png_dir, tmp_path / "parts", 4)
    assert second.step == 4 and second.step_disc == 4
    assert differing(tensors(second), want) == []
    for path in (folder, tmp_path / "parts"):
        assert steps_in(path) == [2, 4] and len(steps_in(path)) <= hific_train.KEEP_CHECKPOINTS
        lines = [json.loads(line) for line in open(path / "metrics.jsonl")]
        assert [line["step"] for line in lines] == [2, 4]
        assert {"d_loss", "g_loss", "rd_loss", "total_qbpp"} <= set(lines[-1]) and "weighted_lpips" not in lines[-1]
        assert all(np.isfinite(v) for v in lines[-1].values())
    state = torch.load(folder / "ckpt-4.pt", map_location="cpu", weights_only=False)
    assert {"model", "discriminator", "optimizers", "step", "step_disc", "dataset", "rng"} <= set(state)
    assert set(state["optimizers"]) == {"transform", "entropy", "disc"} and set(state["rng"]) == {"cpu", "device"}
    # the tables travel with the last checkpoint only
    assert any(k.endswith("_cdf") for k in state["model"])
    early = torch.load(folder / "ckpt-2.pt", map_location="cpu", weights_only=False)
    assert not any(k.endswith("_cdf") for k in early["model"])
    with pytest.raises(ValueError, match="model_kwargs"):
        hific_train.train("hific", folder, 6, images_glob=str(png_dir / "*.png"), no_lpips=True)


def test_mselpips_trains_without_a_discriminator(png_dir, tmp_path):
    trainer = run(png_dir, tmp_path / "base", 2, config="mselpips")
    assert trainer.discriminator is None and set(trainer.optimizers) == {"transform", "entropy"}
    assert trainer.step == 2 and trainer.step_disc == 0
    state = torch.load(tmp_path / "base" / "ckpt-2.pt", map_location="cpu", weights_only=False)
    assert state["discriminator"] is None and set(state["optimizers"]) == {"transform", "entropy"}
    line = json.loads(open(tmp_path / "base" / "metrics.jsonl").read().splitlines()[-1])
    assert "rd_loss" in line and "g_loss" not in line and "d_loss" not in line


def test_a_given_perceptual_loss_is_applied(png_dir, tmp_path):
    calls = []

    def perceptual(fake, real):
        calls.append((tuple(fake.shape), tuple(real.shape)))
        return (fake - real).abs().mean()
    run(png_dir, tmp_path / "lpips", 1, no_lpips=False, perceptual_loss=perceptual)
    assert calls == [((2, CROP, CROP, 3), (2, CROP, CROP, 3))]
    line = json.loads(open(tmp_path / "lpips" / "metrics.jsonl").read().splitlines()[-1])
    assert line["step"] == 1 and line["weighted_lpips"] > 0


def test_init_autoencoder_from_another_run(whole_run, png_dir, tmp_path):
    folder, _ = whole_run
    source = torch.load(folder / "ckpt-4.pt", map_location="cpu", weights_only=False)
    fresh = run(png_dir, tmp_path / "fresh", 0)
    started = run(png_dir, tmp_path / "started", 0, init_autoencoder_from_ckpt_dir=folder)
    assert started.step == 0 and steps_in(tmp_path / "started") == [0]
    names = [n for n, _ in started.model.named_parameters()]
    assert len(names) > 20
    assert all(torch.equal(p.detach().cpu(), source["model"][n]) for n, p in started.model.named_parameters())
    assert any(not torch.equal(p.detach().cpu(), source["model"][n]) for n, p in fresh.model.named_parameters())
    # the discriminator is the seed's, not the other run's
    got, new = started.discriminator.state_dict(), fresh.discriminator.state_dict()
    assert all(torch.equal(got[k], new[k]) for k in new)
    assert any(not torch.equal(got[k].cpu(), source["discriminator"][k]) for k in got)
    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        run(png_dir, tmp_path / "nothing", 0, init_autoencoder_from_ckpt_dir=tmp_path / "empty")


EVAL_SHAPES = {"a": (48, 64), "b": (37, 53), "c": (64, 80)}          # 37 x 53 is no multiple of 16


@pytest.fixture(scope="module")
def eval_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("eval_images")
    for k, (name, (h, w)) in enumerate(EVAL_SHAPES.items()):
        models.write_png(root / f"{name}.png", synthetic.lowpass_images(1, h, w, seed=80 + k)[0])
    return root


def test_eval_trained_model(whole_run, eval_dir, tmp_path, capsys):
    folder, _ = whole_run
    out = tmp_path / "out"
    results = hific_evaluate.eval_trained_model("hific", folder, out, str(eval_dir / "*.png"))
    printed = capsys.readouterr().out
    assert len(results) == 3 and all(set(r) == {"psnr", "bpp_real"} for r in results)
    model = hific_evaluate.load_trained_model(folder)
    stored = torch.load(folder / "ckpt-4.pt", map_location="cpu", weights_only=False)["model"]
    assert all(torch.equal(model.state_dict()[k].cpu(), v) for k, v in stored.items() if k.endswith("_cdf"))
    for i, ((name, (h, w)), r) in enumerate(zip(EVAL_SHAPES.items(), results)):
        data = codec_io.compress_file(model, eval_dir / f"{name}.png", tmp_path / "again.tfci")
        assert r["bpp_real"] == 8 * len(data) / (h * w)
        written = glob.glob(str(out / f"{name}_otp_*.png"))
        assert written == [str(out / f"{name}_otp_{r['bpp_real']:.3f}.png")]
        inp, otp = models.read_png(out / f"{name}_inp.png").numpy(), models.read_png(written[0]).numpy()
        assert inp.shape == otp.shape == (h, w, 3)
        assert np.array_equal(inp, models.read_png(eval_dir / f"{name}.png").numpy())
        mse = np.mean(np.square(inp.astype(np.float64) - otp.astype(np.float64)))
        assert abs(r["psnr"] - (20 * np.log10(255.0) - 10 * np.log10(mse))) <= 1e-4
        assert f"Image {i: 4d}: psnr: {r['psnr']:.5f} / bpp_real: {r['bpp_real']:.5f}, saving in {out}..." in printed
    assert f"psnr: {np.mean([r['psnr'] for r in results])}" in printed and printed.rstrip().endswith("Done!")
    two = hific_evaluate.eval_trained_model("hific", folder, tmp_path / "two", str(eval_dir / "*.png"), max_images=2)
    assert two == results[:2] and not glob.glob(str(tmp_path / "two" / "c_*"))
    with pytest.raises(FileNotFoundError, match="no checkpoint"):
        hific_evaluate.eval_trained_model("hific", tmp_path / "none", out, str(eval_dir / "*.png"))


def test_both_command_lines_run_end_to_end(png_dir, eval_dir, tmp_path):
    def command(module, *flags):
        done = subprocess.run([sys.executable, "-m", f"compression_amd.models.{module}", *flags], cwd=ROOT, timeout=240,
                              capture_output=True, text=True)
        assert done.returncode == 0, done.stdout + done.stderr
        return done.stdout
    ckpt = str(tmp_path / "ckpt")
    printed = command("hific_train", "--config", "hific", "--ckpt_dir", ckpt, "--images_glob", str(png_dir / "*.png"),
                      "--num_steps", "2", "--batch_size", "2", "--crop_size", str(CROP), "--no_lpips",
                      "--no-image-summaries", "--model_kwargs", json.dumps(MODEL_KW), "--discriminator_kwargs",
                      json.dumps(DISC_KW))
    assert "WITHOUT the perceptual" in printed and steps_in(ckpt) == [2]
    printed = command("hific_evaluate", "--config", "hific", "--ckpt_dir", ckpt, "--out_dir", str(tmp_path / "out"),
                      "--images_glob", str(eval_dir / "*.png"), "--max_images", "1")
    assert "Image    0: psnr: " in printed and "Done!" in printed
    assert os.path.exists(tmp_path / "out" / "a_inp.png") and len(glob.glob(str(tmp_path / "out" / "a_otp_*.png"))) == 1
