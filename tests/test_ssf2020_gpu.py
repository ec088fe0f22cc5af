"""GPU tier of the scale-space flow video model (models/ssf2020.py): the training form, its reproducibility, the codec's
closed loop, the file commands and Trainer with ClipDataset."""
import os

import numpy as np
import pytest
import torch

from compression_amd.datasets import Y4MWriter
from compression_amd.datasets.clip_dataset import ClipDataset
from compression_amd.models import ssf2020
from compression_amd.models.train import Trainer
from compression_amd.ops import video_ops
from compression_amd.optimizers import KerasAdam

pytestmark = pytest.mark.gpu


def small_model(seed=0):
    torch.manual_seed(seed)
    return ssf2020.SSF2020Model(num_filters=32, latent_depth=32).cuda()


def moving_clip(frames, height, width, seed):
    """uint8 [T, H, W, 3]: a smooth random image that shifts by two pixels a frame, plus a little noise."""
    rng = np.random.default_rng(seed)
    coarse = torch.from_numpy(rng.uniform(0, 255, (1, 3, height // 8 + 3, width // 8 + 3)).astype(np.float32))
    big = torch.nn.functional.interpolate(coarse, size=(height + 16, width + 16), mode="bilinear", align_corners=False)
    out = [big[0, :, 2 * t:2 * t + height, 2 * t:2 * t + width].permute(1, 2, 0) for t in range(frames)]
    clip = torch.stack(out) + torch.from_numpy(rng.normal(0, 2, (frames, height, width, 3)).astype(np.float32))
    return clip.clamp(0, 255).round().to(torch.uint8)


def training_batch():
    return torch.stack([moving_clip(3, 64, 64, 1), moving_clip(3, 64, 64, 2)]).float().cuda()


def test_forward_and_backward_are_finite():
    model = small_model()
    loss, bpp, mse = model(training_batch(), training=True)
    assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in (loss, bpp, mse))
    assert float(bpp.detach()) > 0 and float(mse.detach()) > 0
    loss.backward()
    missing = [n for n, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing
    with pytest.raises(ValueError, match="multiples of 64"):
        model(torch.zeros(1, 2, 72, 64, 3, device="cuda"))


def one_step(seed):
    model = small_model(seed)
    x = training_batch()
    with torch.no_grad():
        model(x, training=False)
    opt = KerasAdam(model.parameters(), lr=1e-4)
    torch.manual_seed(11)
    opt.zero_grad()
    loss, _, _ = model(x, training=True)
    loss.backward()
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    opt.step()
    return loss.detach().cpu(), grads, {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


def test_seeded_training_step_is_bit_identical():
    loss_a, grads_a, weights_a = one_step(4)
    loss_b, grads_b, weights_b = one_step(4)
    assert torch.equal(loss_a, loss_b)
    assert not [n for n in grads_a if not torch.equal(grads_a[n], grads_b[n])]
    assert not [n for n in weights_a if not torch.equal(weights_a[n], weights_b[n])]


@pytest.fixture(scope="module")
def coded():
    model = small_model(2).init_compression()
    clip = moving_clip(3, 72, 88, 5).cuda()
    shape, strings, recon = model.compress(clip, return_reconstruction=True)
    return model, clip, shape, strings, recon


def test_compress_decompress_closed_loop(coded):
    model, clip, shape, strings, recon = coded
    assert shape == (3, 72, 88) and [len(s) for s in strings] == [2, 4, 4]
    assert all(isinstance(s, bytes) for frame in strings for s in frame)
    x_hat = model.decompress(shape, strings)
    assert x_hat.shape == clip.shape and x_hat.dtype == torch.uint8
    assert torch.equal(x_hat, recon)                       # the decoder sees what the encoder's closed loop saw
    _, again = model.compress(clip)
    assert again == strings


def test_file_round_trip(coded, tmp_path):
    model, clip, shape, strings, recon = coded
    source, packed, rebuilt = (str(tmp_path / n) for n in ("in.y4m", "clip.tfci", "rec.y4m"))
    ssf2020.write_y4m(source, clip)
    data = ssf2020.compress_file(model, source, packed)
    assert os.path.getsize(packed) == len(data)
    decoded = ssf2020.decompress_file(model, packed, rebuilt)
    # what the container holds decodes to the closed loop of the frames the file gave
    frames = ssf2020.read_y4m(source, "cuda")
    assert frames.shape == clip.shape
    _, _, want = model.compress(frames, return_reconstruction=True)
    assert torch.equal(decoded, want)
    back = ssf2020.read_y4m(rebuilt, "cuda")
    y, cbcr = video_ops.rgb_to_ycbcr(decoded, chroma="420")
    assert torch.equal(back, video_ops.ycbcr_to_rgb(y, cbcr))


def write_training_clip(path, seed):
    clip = moving_clip(4, 80, 96, seed).cuda()
    y, cbcr = video_ops.rgb_to_ycbcr(clip, chroma="420")
    with Y4MWriter(path, 96, 80) as w:
        w.write(y, cbcr)


class Interrupted(Exception):
    pass


class StopsAfter:
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


def test_trainer_resumes_bit_for_bit(tmp_path):
    names = [str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")]
    for k, name in enumerate(names):
        write_training_clip(name, 20 + k)
    fresh = lambda seed: (small_model(seed),
                          ClipDataset(names, clip_length=3, patchsize=64, batch_size=2, device="cuda", seed=1))
    weights = lambda m: {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    whole, data = fresh(0)
    history = Trainer(whole, train_path=tmp_path / "whole").fit(data, 3, 1)
    assert len(history) == 3 and all(np.isfinite(list(h.values())).all() for h in history)
    want = weights(whole)
    first, data1 = fresh(0)
    with pytest.raises(Interrupted):
        Trainer(first, train_path=tmp_path / "parts").fit(StopsAfter(data1, 2), 3, 1)
    assert os.path.exists(tmp_path / "parts" / "backup.pt")
    second, data2 = fresh(5)
    resumed = Trainer(second, train_path=tmp_path / "parts").fit(data2, 3, 1)
    got = weights(second)
    assert not [k for k in want if not torch.equal(got[k], want[k])]
    assert resumed == history
    assert whole.em_y is not None                          # fit leaves the model ready to code


def test_train_compress_decompress_commands(tmp_path):
    names = [str(tmp_path / "a.y4m"), str(tmp_path / "b.y4m")]
    for k, name in enumerate(names):
        write_training_clip(name, 30 + k)
    model_path = str(tmp_path / "model.pt")
    common = ["--model_path", model_path, "--num_filters", "32", "--latent_depth", "32"]
    assert ssf2020.main(common + ["train", "--train_glob", str(tmp_path / "*.y4m"), "--train_path",
                                  str(tmp_path / "train"), "--batchsize", "2", "--patchsize", "64", "--epochs", "1",
                                  "--steps_per_epoch", "2", "--max_validation_steps", "1"]) == 0
    assert os.path.exists(model_path)
    packed, rebuilt = str(tmp_path / "a.tfci"), str(tmp_path / "rec.y4m")
    assert ssf2020.main(common + ["compress", names[0], packed, "--max_frames", "3"]) == 0
    assert ssf2020.main(common + ["decompress", packed, rebuilt]) == 0
    assert ssf2020.read_y4m(rebuilt, "cuda").shape == (3, 80, 96, 3)
