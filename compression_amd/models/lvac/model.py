"""LVAC, learned volumetric attribute compression of a voxelised point cloud (models/lvac/lvac.ipynb, "LVAC Model
Code").  An auto-decoder: the latents of one cloud (a DC row and the AC rows of every tree level), a small coordinate
network and the entropy models are trained on that cloud alone, so compressing IS training and the training step is
the codec's hot path.  On a HIP device the step runs on `raht_synthesize` and, for the "mlp" extractor,
`point_mlp_loss` (csrc/lvac.hip); on the CPU, and for the "linear" and "pa" extractors, on their tensor-op twins."""
from __future__ import annotations

import dataclasses
import glob
import math
import os
import re

import numpy as np
import torch

from ... import optimizers
from ...distributions import NoisyDeepFactorized
from ...entropy_models import ContinuousBatchedEntropyModel
from ...ops import lvac_ops
from .octree import build_octree_as_binarytree
from .ply import read_plyfile
from .rlgr import rlgr

__all__ = ["Config", "Model", "PositionAttentionLayer", "convert_rgb_to_yuv", "convert_yuv_to_rgb", "run_rlgr", "train",
           "test", "test_attributes", "main", "checkpoint_dir"]

SMALL_TENSOR_ROWS = 10        # at inference, a latent tensor with fewer rows is stored as bfloat16: 16 bits an element
CHECKPOINT_EVERY = 500
INFERENCE_EVERY = 10000
CHECKPOINTS_KEPT = 3
LATENT_STDDEV = 0.05          # tf.random_normal_initializer's default


@dataclasses.dataclass
class Config:
    random_seed: int = 1234
    num_channels: int = 32
    target_level: int = 24
    hidden_dim: int = 256
    lr: float = 0.01
    latent_optimizer: str = "Adam"          # "Adam", anything else is plain SGD
    extractor_model: str = "mlp"            # "mlp", "linear", "pa"
    num_epochs: int = 50000
    entropy_multiplier: float = 32.0
    normalization: bool = True
    output_colorspace: str = "yuv"          # "yuv", "rgb"
    distortion_colorspace: str = "yuv"      # "yuv", "rgb"
    position_type: str = "local"            # "local", "global", "none"
    use_rlgr: bool = False
    original_vpc: str = ""
    ckpt_dir: str = "checkpoints"
    point_cloud_name: str = "cloud"


def _channels(x):
    return x[..., 0:1], x[..., 1:2], x[..., 2:3]


def _cat(parts):
    return torch.cat(parts, dim=-1) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts, axis=-1)


def convert_rgb_to_yuv(rgb):
    """RGB in [0, 255] -> YUV in [0, 255] (BT.709 luma, the notebook's coefficients), tensors or arrays [..., 3]."""
    r, g, b = _channels(rgb)
    y = 0.212600 * r + 0.715200 * g + 0.072200 * b
    u = -0.114572 * r - 0.385428 * g + 0.5 * b + 128.0
    v = 0.5 * r - 0.454153 * g - 0.045847 * b + 128.0
    return _cat((y, u, v))


def convert_yuv_to_rgb(yuv):
    """YUV in [0, 255] -> RGB in [0, 255]."""
    y, u, v = _channels(yuv)
    u128 = u - 128.0
    v128 = v - 128.0
    r = y + 1.57480 * v128
    g = y - 0.18733 * u128 - 0.46813 * v128
    b = y + 1.85563 * u128
    return _cat((r, g, b))


def run_rlgr(coeffs):
    """The bits RLGR spends on the quantised latents: one stream per channel over all tensors stacked."""
    stacked = np.concatenate([np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c) for c in coeffs], axis=0)
    return 8 * sum(len(rlgr(stacked[:, i].astype(np.int32))) for i in range(stacked.shape[1]))


class _Dense(torch.nn.Module):
    """y = x kernel + bias with the kernel as [in, out]; Glorot-uniform unless a normal stddev is given."""

    def __init__(self, n_in, n_out, use_bias=True, normal_stddev=None):
        super().__init__()
        if normal_stddev is None:
            limit = math.sqrt(6.0 / (n_in + n_out))
            kernel = (torch.rand(n_in, n_out) * 2.0 - 1.0) * limit
        else:
            kernel = torch.randn(n_in, n_out) * normal_stddev
        self.kernel = torch.nn.Parameter(kernel)
        self.bias = torch.nn.Parameter(torch.zeros(n_out)) if use_bias else None

    def forward(self, x):
        y = x @ self.kernel
        return y + self.bias if self.bias is not None else y


class PositionAttentionLayer(torch.nn.Module):
    """inputs [N, positional_channels + latent_channels] -> dense1(latent * sin(dense0(position)))."""

    def __init__(self, positional_channels=3, latent_channels=32, output_channels=3):
        super().__init__()
        self.positional_channels = positional_channels
        self.latent_channels = latent_channels
        self.output_channels = output_channels
        self.dense0 = _Dense(positional_channels, latent_channels, normal_stddev=LATENT_STDDEV)
        self.dense1 = _Dense(latent_channels, output_channels, normal_stddev=LATENT_STDDEV)

    def forward(self, inputs):
        position = inputs[:, :self.positional_channels]
        latent = inputs[:, self.positional_channels:]
        return self.dense1(latent * torch.sin(self.dense0(position)))


class Model(torch.nn.Module):
    """`Model(config)` reads config.original_vpc; `Model(config, position, colors)` takes the cloud as arrays
    ([N, 3] float positions in ascending Morton order, [N, 3] RGB).  `force_reference = True` keeps a model on a HIP
    device off the fused kernels (what the tests compare against)."""

    def __init__(self, config, position=None, colors=None):
        super().__init__()
        self.config = config = dataclasses.replace(config)
        if config.extractor_model == "linear":
            config.num_channels = 3
            config.position_type = "none"
        if config.extractor_model not in ("mlp", "linear", "pa"):
            raise ValueError("Extractor model not implemented: " + str(config.extractor_model))
        if config.position_type not in ("local", "global", "none"):
            raise ValueError("Position type not implemented: " + str(config.position_type))
        self.force_reference = False
        if position is None:
            position, colors = read_plyfile(config.original_vpc)
            if position is None or colors is None:
                raise ValueError(f"{config.original_vpc}: the vertex element needs x, y, z and red, green, blue")
            if not np.issubdtype(position.dtype, np.floating):
                position = position.astype(np.float32)
        position, colors = np.asarray(position), np.asarray(colors)
        if len(position) != len(colors):
            raise ValueError(f"{len(position)} positions and {len(colors)} colours")
        self.original_position, self.original_colors = position, colors
        self.count = len(position)
        target = torch.from_numpy(colors.astype(np.float32))
        if config.distortion_colorspace.lower() == "yuv":
            target = convert_rgb_to_yuv(target).clamp(0.0, 255.0)
        self.register_buffer("colors", target.contiguous(), persistent=False)

        self.binlevel, self.depth = build_octree_as_binarytree(position, config.target_level)
        if len(self.binlevel[0].prefix) != 1:
            raise ValueError("the tree must have one root")
        c, levels = config.num_channels, config.target_level
        for level in self.binlevel[:levels]:
            if not config.normalization:
                level.latent_scale = np.ones_like(level.latent_scale)
        self.tree = lvac_ops.RahtTree(self.binlevel[:levels], n_root=1)
        last = self.binlevel[levels]
        self.blocks = lvac_ops.PointBlocks.from_counts(last.descendant_count)

        # latents: the DC row, then the AC rows of every level; one entropy model each
        rows = [1] + self.tree.ac_rows
        self.latent_variables = torch.nn.ParameterList(
            torch.nn.Parameter(torch.randn(n, c) * LATENT_STDDEV) for n in rows)
        self.entropy_models = torch.nn.ModuleList(
            ContinuousBatchedEntropyModel(prior=NoisyDeepFactorized(batch_shape=[c]), coding_rank=1, compression=False)
            for _ in rows)
        scales = [np.full(1, math.sqrt(self.count))] + [lv.latent_scale for lv in self.binlevel[:levels]]
        for k, s in enumerate(scales):
            self.register_buffer(f"_scale{k}", torch.from_numpy(np.asarray(s, np.float32)).reshape(-1, 1),
                                 persistent=False)
        self.delta_high = torch.nn.Parameter(torch.ones(1, c))

        if config.extractor_model == "pa" or config.position_type != "none":
            source = self.binlevel[0] if config.position_type == "global" else last
            self.register_buffer("position", torch.from_numpy(source.relative_position.astype(np.float32)).contiguous(),
                                 persistent=False)
        else:
            self.position = None
        n_in = c + (3 if self.position is not None else 0)
        if config.extractor_model == "mlp":
            self.mlp = torch.nn.ModuleList([_Dense(n_in, config.hidden_dim), _Dense(config.hidden_dim, 3)])
        elif config.extractor_model == "linear":
            self.mlp = _Dense(c, 3, use_bias=False)
        else:
            self.mlp = PositionAttentionLayer(positional_channels=3, latent_channels=c, output_channels=3)

        latent_ids = {id(p) for p in self.latent_variables}
        others = [p for p in self.parameters() if id(p) not in latent_ids]
        self.optimizer = optimizers.KerasAdam(others, lr=config.lr)
        if config.latent_optimizer == "Adam":
            self.latent_optimizer = optimizers.KerasAdam(list(self.latent_variables), lr=config.lr)
        else:
            self.latent_optimizer = torch.optim.SGD(list(self.latent_variables), lr=config.lr)

    # -- entropy coding ---------------------------------------------------------------------------------------------

    def entropy_coding(self, training):
        """-> (bits per point, the dequantised latents [DC, AC of level 0, ...], the integer latents or Nones)."""
        delta_high = torch.nn.functional.softplus(self.delta_high)
        latents, quantized, bits = [], [], []
        for k, (model, latent) in enumerate(zip(self.entropy_models, self.latent_variables)):
            if latent.shape[0] == 0:
                # a level without a two-child node: nothing to code, nothing to launch
                latents.append(latent)
                quantized.append(None if training else torch.zeros(latent.shape, dtype=torch.int32, device=latent.device))
                continue
            inv_step_size = getattr(self, f"_scale{k}") / delta_high
            if training:
                coeff, nbits = model(latent * inv_step_size, training=True)
                q = None
            elif latent.shape[0] < SMALL_TENSOR_ROWS:
                # modelling the distribution costs more than it saves here: round and keep as bfloat16
                coeff = torch.round(latent * inv_step_size).to(torch.bfloat16).to(torch.float32)
                q = coeff.to(torch.int32)
                nbits = 16.0 * torch.ones_like(latent)
            else:
                coeff, nbits = model(latent * inv_step_size, training=False)
                offset = model.quantization_offset
                q = coeff if offset is None else coeff - offset.to(coeff.device)
                q = torch.round(q).to(torch.int32)
            latents.append(coeff / inv_step_size)
            quantized.append(q)
            bits.append(nbits.sum())
        entropy_loss = torch.stack(bits).sum() / self.count
        return entropy_loss, latents, quantized

    # -- synthesis --------------------------------------------------------------------------------------------------

    def synthesize(self, latent):
        """[DC, AC of level 0, ...] -> the latent of every block of the target level [blocks, C]."""
        dc, *ac = latent
        if len(ac) != self.config.target_level:
            raise ValueError(f"{self.config.target_level} AC tensors are needed, got {len(ac)}")
        if self.force_reference:
            return lvac_ops.raht_synthesize_reference(dc, ac, self.tree)
        return lvac_ops.raht_synthesize(dc, ac, self.tree)

    def _output_map(self, training):
        """(A, o), clip: how the network's output becomes the colours the distortion is measured on."""
        out, dist = self.config.output_colorspace.lower(), self.config.distortion_colorspace.lower()
        if out == "yuv" and dist == "rgb":
            return lvac_ops.YUV_TO_RGB, False
        if out == "rgb" and dist == "yuv":
            return lvac_ops.RGB_TO_YUV, False
        return lvac_ops.IDENTITY, not training

    def _decode(self, latent, training, want_recon):
        cumulative = self.synthesize(latent)
        affine, clip = self._output_map(training)
        if self.config.extractor_model == "mlp":
            args = (cumulative, self.blocks, self.position, self.mlp[0].kernel, self.mlp[0].bias, self.mlp[1].kernel,
                    self.mlp[1].bias, self.colors)
            if self.force_reference:
                loss, recon = lvac_ops.point_mlp_loss_reference(*args, affine=affine, clip=clip)
                return loss, recon
            return lvac_ops.point_mlp_loss(*args, affine=affine, clip=clip, want_recon=want_recon)
        index = self.blocks.on(cumulative.device)[0].to(torch.int64)
        x = cumulative[index]
        if self.position is not None:
            x = torch.cat([self.position, x], dim=-1)
        recon = self.mlp(x)
        if affine is lvac_ops.YUV_TO_RGB:
            recon = convert_yuv_to_rgb(recon)
        elif affine is lvac_ops.RGB_TO_YUV:
            recon = convert_rgb_to_yuv(recon)
        elif clip:
            recon = recon.clamp(0.0, 255.0)
        return torch.mean(torch.square(self.colors - recon)), recon

    def reconstruct_at_level(self, latent, training):
        """The decoded colours [N, 3] in the distortion colour space (clipped to [0, 255] at inference when no
        conversion is applied)."""
        return self._decode(latent, training, True)[1]

    def evaluate_reconstruction_at_level(self, latent, training):
        """The mean squared error of the decoded colours."""
        return self._decode(latent, training, False)[0]

    def evaluate_attributes_at_level(self, latent, training):
        return self.reconstruct_at_level(latent, training)

    # -- training ---------------------------------------------------------------------------------------------------

    def train_step(self):
        """One step on the whole cloud -> (loss, reconstruction loss, entropy loss), detached."""
        self.optimizer.zero_grad(set_to_none=True)
        self.latent_optimizer.zero_grad(set_to_none=True)
        entropy_loss, latent, _ = self.entropy_coding(training=True)
        reconstruction_loss = self.evaluate_reconstruction_at_level(latent, training=True)
        loss = reconstruction_loss + self.config.entropy_multiplier * entropy_loss
        loss.backward()
        self.latent_optimizer.step()
        self.optimizer.step()
        return loss.detach(), reconstruction_loss.detach(), entropy_loss.detach()


# -- the commands -------------------------------------------------------------------------------------------------------

def checkpoint_dir(config):
    return "/".join((config.ckpt_dir, config.point_cloud_name, ",".join((
        config.extractor_model, config.output_colorspace, f"target_level={config.target_level}",
        f"lambda={config.entropy_multiplier}", f"lr={config.lr}"))))


def _checkpoints(directory):
    found = []
    for path in glob.glob(os.path.join(glob.escape(directory), "ckpt-*.pt")):
        m = re.fullmatch(r"ckpt-(\d+)\.pt", os.path.basename(path))
        if m:
            found.append((int(m.group(1)), path))
    return sorted(found)


def _save_checkpoint(model, directory, step):
    os.makedirs(directory, exist_ok=True)
    state = {"step": step, "model": model.state_dict(), "optimizer": model.optimizer.state_dict(),
             "latent_optimizer": model.latent_optimizer.state_dict(), "rng": torch.get_rng_state()}
    device = model.delta_high.device
    if device.type == "cuda":
        state["device_rng"] = torch.cuda.get_rng_state(device)
    path = os.path.join(directory, f"ckpt-{step}.pt")
    torch.save(state, path + ".tmp")
    os.replace(path + ".tmp", path)
    for _, old in _checkpoints(directory)[:-CHECKPOINTS_KEPT]:
        os.remove(old)


def _report_inference(model):
    with torch.no_grad():
        rate, latent, quantized = model.entropy_coding(training=False)
        rlgr_rate = run_rlgr(quantized) / model.count if model.config.use_rlgr else None
        dist = model.evaluate_reconstruction_at_level(latent, training=False)
    return float(rate), float(dist), rlgr_rate


def train(model, step, directory):
    """Steps `step` .. num_epochs - 1, a checkpoint every 500 and an inference report every 10000."""
    for i in range(step, model.config.num_epochs):
        loss, _, _ = model.train_step()
        if i % CHECKPOINT_EVERY == 0:
            float(loss)                                   # the step has finished before its state is written
            _save_checkpoint(model, directory, i)
            if i % INFERENCE_EVERY == 0:
                rate, dist, rlgr_rate = _report_inference(model)
                if rlgr_rate is not None:
                    print(f"Test: rlgr_rate={rlgr_rate}")
                print(f"Test: rate={rate}, dist={dist}")


def test(model):
    """-> (bits per point, mean squared error) at inference; the rate is RLGR's when config.use_rlgr."""
    rate, dist, rlgr_rate = _report_inference(model)
    print(f"Test: rate={rate}, dist={dist}")
    if rlgr_rate is not None:
        print(f"Test: rlgr rate={rlgr_rate}")
        return rlgr_rate, dist
    return rate, dist


def test_attributes(model):
    with torch.no_grad():
        _, latent, _ = model.entropy_coding(training=False)
        return model.evaluate_attributes_at_level(latent, training=False)


def main(config, training, return_attributes=False, device=None):
    """Builds the model, resumes from the newest checkpoint of its directory, then trains, or reports the inference
    rate and distortion, or returns the decoded colours.  Without a checkpoint, anything but training is a
    FileNotFoundError."""
    torch.manual_seed(config.random_seed)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    model = Model(config).to(device)
    print("Number of points:", model.count)
    directory = checkpoint_dir(model.config)
    print("Checkpoint directory:", directory)
    found = _checkpoints(directory)
    step = 0
    if found:
        step, path = found[-1]
        state = torch.load(path, map_location=device, weights_only=False)
        model.load_state_dict(state["model"])
        model.optimizer.load_state_dict(state["optimizer"])
        model.latent_optimizer.load_state_dict(state["latent_optimizer"])
        torch.set_rng_state(state["rng"].cpu())
        if "device_rng" in state and torch.device(device).type == "cuda":
            torch.cuda.set_rng_state(state["device_rng"].cpu(), device)
        print("Model restored from:", path)
    elif training:
        print("Model initialized from scratch.")
    else:
        raise FileNotFoundError("No checkpoint found in: " + directory)
    if training:
        return train(model, step, directory)
    if return_attributes:
        return test_attributes(model)
    return test(model)
