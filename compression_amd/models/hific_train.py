"""HiFiC's losses, its alternating discriminator / generator training step (models/hific/configs.py:20-77;
model.py:61-115, 365-455, 588-764, 800-837, 875-897) and its training command (models/hific/train.py) on this
library's kernels.

    python -m compression_amd.models.hific_train --config hific --ckpt_dir DIR --images_glob 'images/*.png' ...

`train()` feeds `HiFiCTrainer.train_step` from a `ScaledPatchDataset` (the input pipeline of model.py:260-363), and
stands in for `tf.train.MonitoredTrainingSession`: `ckpt_dir/ckpt-<step>.pt` every SAVE_CHECKPOINT_STEPS generator steps
and at the end, the newest five kept, a folder that holds checkpoints is resumed from, `StopAtStepHook(num_steps)`.
Not here: TensorFlow Datasets, TensorBoard summaries, the validation mode and hooks.  The perceptual term is
`perceptual_loss(fake_scaled, real_scaled) -> scalar`: `layers.LPIPSLoss(layers.LPIPS.from_lpips_package(...))` is LPIPS
on this library's kernels (the network is here, its trained weights are the user's), or any other callable.  The reference's third ("aux") optimiser minimises
the entropy model's auxiliary loss (model.py:807-811); the entropy models of this library have no auxiliary loss (their
tails are solved on the device, not learned), so there are three optimisers: transform, entropy, disc."""
from __future__ import annotations

import argparse
import collections
import json
import os
import re
import sys

import torch

from ..layers import gan_functional
from .hific import BppPair, Nodes  # noqa: F401

__all__ = ["CONFIGS", "Config", "LossConfig", "Schedule", "scheduled_value", "rd_loss", "gan_losses", "HiFiCTrainer",
           "SAVE_CHECKPOINT_STEPS", "KEEP_CHECKPOINTS", "checkpoint_steps", "latest_checkpoint", "save_checkpoint",
           "train", "parse_args", "main"]

Schedule = collections.namedtuple("Schedule", ["vals", "steps"])
LossConfig = collections.namedtuple("LossConfig", ["CP", "C", "CD", "target", "lpips_weight", "target_schedule",
                                                   "lmbda_a", "lmbda_b"])
Config = collections.namedtuple("Config", ["lambda_schedule", "lr", "lr_schedule", "num_steps_disc", "loss_config"])


def _config(cp, num_steps_disc):
    # Loss = C * (1 / lambda * R + CD * D) + CP * P, lambda = lmbda_a if the quantised bpp exceeds the target, else lmbda_b
    return Config(
        lambda_schedule=Schedule(vals=(2., 1.), steps=(50000,)),
        lr=1e-4,
        lr_schedule=Schedule(vals=(1., 0.1), steps=(500000,)),
        num_steps_disc=num_steps_disc,
        loss_config=LossConfig(
            CP=cp, C=0.1 * 2. ** -5, CD=0.75, target=0.14, lpips_weight=1.,
            target_schedule=Schedule(vals=(0.20 / 0.14, 1.), steps=(50000,)),
            lmbda_a=0.1 * 2. ** -6, lmbda_b=0.1 * 2. ** 1))


# configs.py:20-77
CONFIGS = {"hific": _config(0.1 * 1.5 ** 1, 1), "mselpips": _config(None, None)}


def scheduled_value(value, schedule, step):
    """model.py:875-897: value * vals[i] for the first i with step < steps[i]; the last value beyond all steps."""
    if len(schedule.steps) + 1 != len(schedule.vals):
        raise ValueError("Schedule expects one more value than steps.")
    for boundary, factor in zip(schedule.steps, schedule.vals):
        if step < int(boundary):
            return value * factor
    return value * schedule.vals[-1]


def rd_loss(distortion, bpp_pair, config, step=0, ignore_schedules=False):
    """model.py:61-102: C * CD * distortion + C * (1 / lambda) * total_nbpp, lambda = lmbda_a where total_qbpp >
    target (the rate is too high: the larger factor), else lmbda_b -> (rd_loss, weighted_rate, weighted_distortion,
    lmbda_inv).  `distortion`: the mean squared error on [0, 255] values.  The switch is taken on the device."""
    lc = config.loss_config
    if lc.lmbda_a >= lc.lmbda_b:
        raise ValueError(f"Expected lmbda_a < lmbda_b, got {lc.lmbda_a} >= {lc.lmbda_b}")

    def scheduled(value, schedule):
        return value if ignore_schedules else scheduled_value(value, schedule, step)
    lmbda_a = scheduled(lc.lmbda_a, config.lambda_schedule)
    lmbda_b = scheduled(lc.lmbda_b, config.lambda_schedule)
    target = scheduled(lc.target, lc.target_schedule)
    nbpp, qbpp = bpp_pair
    nbpp, qbpp = torch.as_tensor(nbpp, dtype=torch.float32), torch.as_tensor(qbpp, dtype=torch.float32)
    one = torch.ones_like(qbpp)
    lmbda_inv = torch.where(qbpp.detach() > target, one / lmbda_a, one / lmbda_b)
    weighted_rate = lmbda_inv * nbpp * lc.C
    weighted_distortion = distortion * lc.CD * lc.C
    return weighted_rate + weighted_distortion, weighted_rate, weighted_distortion, lmbda_inv


def gan_losses(logits):
    """compare_gan's non_saturating loss (model.py:616-638) of the discriminator's logits for concat([real, fake], 0):
    (d_loss, g_loss, mean D(real), mean D(fake)) from one launch."""
    return gan_functional.gan_losses(logits)


class HiFiCTrainer:
    """`train_step(batches)`: `num_steps_disc` discriminator steps, each on its own sub-batch, then one generator step on
    the last sub-batch with the updated discriminator (model.py:411-455).

    model: HiFiCModel; discriminator: Discriminator or None (the `mselpips` baseline); config: one of CONFIGS;
    perceptual_loss(fake_scaled, real_scaled) -> scalar or None; ignore_schedules: the lambda and target schedules are
    not applied (model.py:106-115); the learning-rate schedule always is.

    Adam optimisers as model.py:800-837: `transform` (encoder, generator, hyper-transforms), `entropy` (the
    hyper-latents' prior), `disc`; learning rate config.lr times its schedule at the generator's step (the
    discriminator's own step counter for `disc`)."""

    def __init__(self, model, discriminator, config, perceptual_loss=None, ignore_schedules=False):
        if (discriminator is None) != (config.num_steps_disc is None):
            raise ValueError("a configuration with num_steps_disc needs a discriminator, and one without has none")
        self.model, self.discriminator, self.config = model, discriminator, config
        self.perceptual_loss, self.ignore_schedules = perceptual_loss, ignore_schedules
        self.step = self.step_disc = 0
        entropy = list(model.hyperprior.side_prior.parameters())
        ids = {id(p) for p in entropy}
        transform = [p for p in model.parameters() if id(p) not in ids]
        self.optimizers = {"transform": torch.optim.Adam(transform, lr=config.lr),
                           "entropy": torch.optim.Adam(entropy, lr=config.lr)}
        if discriminator is not None:
            self.optimizers["disc"] = torch.optim.Adam(discriminator.parameters(), lr=config.lr)
        self.last_disc_latents = None        # what the discriminator was last conditioned on

    @property
    def num_sub_batches(self):
        return (self.config.num_steps_disc or 0) + 1

    def _set_lr(self, name, step):
        lr = scheduled_value(self.config.lr, self.config.lr_schedule, step)
        for group in self.optimizers[name].param_groups:
            group["lr"] = lr

    def _discriminate(self, nodes, gradients_to_generator):
        """model.py:731-764: D on concat([real, fake], 0) conditioned on the detached quantised latents, twice."""
        fake = nodes.reconstruction_scaled if gradients_to_generator else nodes.reconstruction_scaled.detach()
        real = nodes.input_image_scaled.detach().to(fake.dtype)
        latent = nodes.latent_quantized.detach()
        self.last_disc_latents = latent
        _, logits = self.discriminator(torch.cat([real, fake], 0), torch.cat([latent, latent], 0))
        return gan_losses(logits)

    def discriminator_step(self, x):
        """One Adam step on d_loss over the discriminator's variables only (model.py:641-673) -> scalars."""
        with torch.no_grad():
            nodes, _ = self.model.training_nodes(x)
        self.discriminator.train()
        d_loss, g_loss, d_real, d_fake = self._discriminate(nodes, gradients_to_generator=False)
        self._set_lr("disc", self.step_disc)
        self.optimizers["disc"].zero_grad(set_to_none=True)
        d_loss.backward()
        self.optimizers["disc"].step()
        self.step_disc += 1
        return {"d_loss": d_loss.detach(), "d_real": d_real, "d_fake": d_fake}

    def generator_step(self, x):
        """One Adam step of encoder, generator, hyperprior and prior on rd_loss + CP g_loss + lpips_weight P
        (model.py:675-729); the discriminator's variables get no gradient and are not stepped -> scalars."""
        lc = self.config.loss_config
        nodes, bpp_pair = self.model.training_nodes(x)
        distortion = torch.mean((nodes.input_image.float() - nodes.reconstruction.float()) ** 2)
        loss, weighted_rate, weighted_distortion, lmbda_inv = rd_loss(
            distortion, bpp_pair, self.config, self.step, self.ignore_schedules)
        out = {"rd_loss": loss.detach(), "weighted_R": weighted_rate.detach(),
               "weighted_D": weighted_distortion.detach(), "lmbda_inv": lmbda_inv,
               "total_nbpp": bpp_pair.total_nbpp.detach(), "total_qbpp": bpp_pair.total_qbpp.detach()}
        if self.discriminator is not None:
            frozen = [p for p in self.discriminator.parameters() if p.requires_grad]
            for p in frozen:
                p.requires_grad_(False)
            try:
                _, g_loss, _, _ = self._discriminate(nodes, gradients_to_generator=True)
            finally:
                for p in frozen:
                    p.requires_grad_(True)
            out["g_loss"] = g_loss.detach()
            loss = loss + lc.CP * g_loss
        if self.perceptual_loss is not None:
            weighted = lc.lpips_weight * self.perceptual_loss(nodes.reconstruction_scaled, nodes.input_image_scaled)
            out["weighted_lpips"] = weighted.detach()
            loss = loss + weighted
        for name in ("transform", "entropy"):
            self._set_lr(name, self.step)
            self.optimizers[name].zero_grad(set_to_none=True)
        loss.backward()
        for name in ("transform", "entropy"):
            self.optimizers[name].step()
        self.step += 1
        out["loss_enc_dec_entropy"] = loss.detach()
        return out

    def train_step(self, batches):
        """batches: `num_steps_disc + 1` image batches [B, H, W, 3] in [0, 255] -> a dict of scalar tensors: d_loss,
        d_real, d_fake (of the first discriminator step, as the reference's summaries), g_loss, rd_loss, weighted_R,
        weighted_D, lmbda_inv, total_nbpp, total_qbpp, weighted_lpips (where they apply)."""
        batches = list(batches)
        if len(batches) != self.num_sub_batches:
            raise ValueError(f"train_step takes {self.num_sub_batches} sub-batches, got {len(batches)}")
        out = {}
        self.model.train()
        for i, x in enumerate(batches[:-1]):
            scalars = self.discriminator_step(x)
            if i == 0:
                out.update(scalars)
        out.update(self.generator_step(batches[-1]))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints and the training command (models/hific/train.py)

SAVE_CHECKPOINT_STEPS = 1000        # train.py:29
KEEP_CHECKPOINTS = 5                # tf.train.Saver's max_to_keep

_CKPT = re.compile(r"ckpt-(\d+)\.pt")


def checkpoint_steps(ckpt_dir):
    """The steps of the `ckpt-<step>.pt` files in a folder, ascending; [] where there is no such folder or file."""
    if not os.path.isdir(ckpt_dir):
        return []
    found = (_CKPT.fullmatch(name) for name in os.listdir(ckpt_dir))
    return sorted(int(m.group(1)) for m in found if m)


def _checkpoint_file(ckpt_dir, step):
    return os.path.join(os.fspath(ckpt_dir), f"ckpt-{step}.pt")


def latest_checkpoint(ckpt_dir):
    """The file of the newest step, or None (tf.train.latest_checkpoint)."""
    steps = checkpoint_steps(ckpt_dir)
    return _checkpoint_file(ckpt_dir, steps[-1]) if steps else None


def save_checkpoint(ckpt_dir, state, step, keep=KEEP_CHECKPOINTS):
    """Writes `ckpt_dir/ckpt-<step>.pt` atomically (a temporary file, then os.replace) and removes all but the newest
    `keep` checkpoints."""
    os.makedirs(ckpt_dir, exist_ok=True)
    target = _checkpoint_file(ckpt_dir, step)
    torch.save(state, target + ".tmp")
    os.replace(target + ".tmp", target)
    for old in checkpoint_steps(ckpt_dir)[:-keep]:
        os.remove(_checkpoint_file(ckpt_dir, old))
    return target


def _load_latest(ckpt_dir):
    path = latest_checkpoint(ckpt_dir)
    return None if path is None else torch.load(path, map_location="cpu", weights_only=False)


def _load_model(model, state_dict):
    """Loads a checkpoint's model for further training.  The tables of a finished run are let go again: they belong
    to the parameters they were built from, and checkpoints written while those change must not carry them."""
    from .codec_io import load_checkpoint
    load_checkpoint(model, state_dict)
    model.entropy_model = model.side_entropy_model = None


def _rng_state(device):
    return {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device)}


def _perceptual_loss(lpips_weight_path, no_lpips, device):
    from ..layers import LPIPS, LPIPSLoss
    if lpips_weight_path:
        weights = torch.load(lpips_weight_path, map_location="cpu")
        return LPIPSLoss(LPIPS.from_state_dict(weights).to(device))
    if not no_lpips:
        raise SystemExit("training needs --lpips_weight_path (a state dict of layers.LPIPS: this library ships no "
                         "LPIPS weights and downloads none), or --no_lpips to train without the perceptual term")
    print("Training WITHOUT the perceptual (LPIPS) term: --no_lpips")
    return None


def train(config_name, ckpt_dir, num_steps, *, images_glob=None, init_autoencoder_from_ckpt_dir=None, batch_size=8,
          crop_size=256, lpips_weight_path=None, no_lpips=False, perceptual_loss=None, seed=0, precision_policy=None,
          save_checkpoint_steps=SAVE_CHECKPOINT_STEPS, model_kwargs=None, discriminator_kwargs=None):
    """models/hific/train.py:32-67.  Trains until `trainer.step == num_steps`, resuming from the newest checkpoint of
    `ckpt_dir` if it holds one, and returns the HiFiCTrainer.

    A checkpoint holds the model, the discriminator, the optimisers, `step`, `step_disc`, the dataset's state and the
    CPU and device RNG states: a resumed run continues bit for bit.  Training ends with `model.init_compression()`, so
    the `model` entry of the last checkpoint carries the range-coding tables and loads with
    `codec_io.load_checkpoint`.  `init_autoencoder_from_ckpt_dir`: a fresh run starts from the model (encoder,
    generator, hyperprior with its prior; model.py:472-488) of that folder's newest checkpoint; a resumed run has them
    from its own checkpoint.  `perceptual_loss`: a callable in place of LPIPS; `model_kwargs`, `discriminator_kwargs`:
    other network sizes than the paper's (kept in the checkpoint, where `hific_evaluate` reads them)."""
    from .. import _lib
    from ..datasets import ScaledPatchDataset
    from . import codec_io
    from .hific import Discriminator, HiFiCModel
    config = CONFIGS[config_name]
    ckpt_dir = os.fspath(ckpt_dir)
    if init_autoencoder_from_ckpt_dir is not None and os.path.abspath(init_autoencoder_from_ckpt_dir) == \
            os.path.abspath(ckpt_dir):
        raise ValueError(_SAME_FOLDER)
    if not images_glob:
        raise SystemExit("training needs --images_glob: TensorFlow Datasets (TFDS, the reference's default input) is "
                         "not available here")
    compute_dtype = codec_io.compute_dtype_of(precision_policy)
    if perceptual_loss is None and not lpips_weight_path and not no_lpips:
        _perceptual_loss(None, False, None)
    device = _lib.require_device()
    if perceptual_loss is None:
        perceptual_loss = _perceptual_loss(lpips_weight_path, no_lpips, device)
    model_kwargs, discriminator_kwargs = dict(model_kwargs or {}), dict(discriminator_kwargs or {})

    resumed = _load_latest(ckpt_dir)
    if resumed is not None:
        for key, mine in (("config", config_name), ("model_kwargs", model_kwargs),
                          ("discriminator_kwargs", discriminator_kwargs)):
            if resumed[key] != mine:
                raise ValueError(f"{ckpt_dir} was trained with {key} = {resumed[key]!r}, this run has {mine!r}")
    torch.manual_seed(seed)
    model = HiFiCModel(compute_dtype=compute_dtype, **model_kwargs).to(device)
    discriminator = None
    if config.num_steps_disc is not None:
        discriminator = Discriminator(**discriminator_kwargs).to(device)
    if resumed is not None:
        _load_model(model, resumed["model"])
        if discriminator is not None:
            discriminator.load_state_dict(resumed["discriminator"])
    elif init_autoencoder_from_ckpt_dir is not None:
        source = _load_latest(init_autoencoder_from_ckpt_dir)
        if source is None:
            raise FileNotFoundError(f"--init_autoencoder_from_ckpt_dir: no checkpoint in {init_autoencoder_from_ckpt_dir}")
        _load_model(model, source["model"])
        print(f"Restored encoder, generator and hyperprior from step {source['step']} of {init_autoencoder_from_ckpt_dir}")
    trainer = HiFiCTrainer(model, discriminator, config, perceptual_loss=perceptual_loss)
    dataset = ScaledPatchDataset(images_glob, crop_size, batch_size * trainer.num_sub_batches, repeat=True, seed=seed,
                                 device=device, dtype=compute_dtype)
    if resumed is not None:
        for name, optimizer in trainer.optimizers.items():
            optimizer.load_state_dict(resumed["optimizers"][name])
        trainer.step, trainer.step_disc = int(resumed["step"]), int(resumed["step_disc"])
        dataset.load_state_dict(resumed["dataset"])
        torch.set_rng_state(resumed["rng"]["cpu"])
        torch.cuda.set_rng_state(resumed["rng"]["device"], device)
        print(f"Resuming {ckpt_dir} at step {trainer.step}")

    def state(rng):
        return {"model": model.state_dict(),
                "discriminator": None if discriminator is None else discriminator.state_dict(),
                "optimizers": {name: o.state_dict() for name, o in trainer.optimizers.items()},
                "step": trainer.step, "step_disc": trainer.step_disc, "dataset": dataset.state_dict(), "rng": rng,
                "config": config_name, "model_kwargs": model_kwargs, "discriminator_kwargs": discriminator_kwargs,
                "precision_policy": precision_policy}

    def log(scalars):
        # the one host read of the step's scalars
        names = sorted(scalars)
        values = torch.stack([scalars[k].detach().float().reshape(()) for k in names]).tolist()
        with open(os.path.join(ckpt_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps({"step": trainer.step, **dict(zip(names, values))}) + "\n")

    os.makedirs(ckpt_dir, exist_ok=True)
    try:
        while trainer.step < num_steps:
            batch = next(dataset)
            # model.py:260-281: the first batch_size images are the generator's, the others the discriminator's;
            # train_step takes the generator's sub-batch last
            subs = [batch[k * batch_size:(k + 1) * batch_size] for k in range(1, trainer.num_sub_batches)]
            subs.append(batch[:batch_size])
            scalars = trainer.train_step(subs)
            n = trainer.step
            report = n > 1 and n % 100 == 1                 # train.py:65-66
            save = n % save_checkpoint_steps == 0 and n != num_steps
            if report:
                print(f"Iteration {n}")
            if report or save or n == num_steps:
                log(scalars)
            if save:
                save_checkpoint(ckpt_dir, state(_rng_state(device)), n)
    finally:
        dataset.close()
    rng = _rng_state(device)
    model.init_compression()
    save_checkpoint(ckpt_dir, state(rng), trainer.step)
    print("Training session closed.")
    return trainer


_SAME_FOLDER = ("--init_autoencoder_from_ckpt_dir should not point to the same folder as --ckpt_dir. If you simply want "
                "to continue training the model in --ckpt_dir, you do not have to pass "
                "--init_autoencoder_from_ckpt_dir, as continuing training is the default.")


def _parse_num_steps(steps):
    """train.py:117-126: an integer, or one with an `M` (million) or `k` (thousand) suffix."""
    try:
        return int(steps)
    except ValueError:
        pass
    try:
        if steps.endswith("M"):
            return int(steps[:-1]) * 1000000
        if steps.endswith("k"):
            return int(steps[:-1]) * 1000
    except ValueError:
        pass
    raise ValueError(f"Invalid num_steps value: {steps}")


def parse_args(argv=None):
    """The flags of train.py:70-126; --images_glob takes the place of the TFDS flags."""
    parser = argparse.ArgumentParser(prog="python -m compression_amd.models.hific_train",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--config", required=True, choices=sorted(CONFIGS), help="The config to use.")
    parser.add_argument("--ckpt_dir", required=True,
                        help="Path to the folder where checkpoints should be stored. Passing the same folder twice "
                             "will resume training.")
    parser.add_argument("--num_steps", default="1M",
                        help='Number of steps to train for. Supports M and k postfix for "million" and "thousand".')
    parser.add_argument("--init_autoencoder_from_ckpt_dir", metavar="AUTOENC_CKPT_DIR",
                        help="If given, restore encoder, generator and hyperprior from the latest checkpoint in "
                             "AUTOENC_CKPT_DIR.")
    parser.add_argument("--batch_size", type=int, default=8, help="Batch size for training.")
    parser.add_argument("--crop_size", type=int, default=256, help="Crop size for input pipeline.")
    parser.add_argument("--lpips_weight_path", help="A state dict of layers.LPIPS (torch.save).")
    parser.add_argument("--no_lpips", action="store_true", help="Train without the perceptual term.")
    parser.add_argument("--images_glob", help="The training images (PNG).")
    parser.add_argument("--seed", type=int, default=0, help="Seed of the initialisers and the input pipeline.")
    parser.add_argument("--precision_policy", default=None, help="float32 or mixed_bfloat16.")
    parser.add_argument("--no-image-summaries", dest="image_summaries", action="store_false",
                        help="Accepted and ignored: there are no summaries.")
    parser.add_argument("--model_kwargs", type=json.loads, default=None,
                        help="JSON: other HiFiCModel sizes than the paper's (tests and experiments).")
    parser.add_argument("--discriminator_kwargs", type=json.loads, default=None,
                        help="JSON: other Discriminator sizes than the paper's (tests and experiments).")
    args = parser.parse_args(argv)
    if args.ckpt_dir == args.init_autoencoder_from_ckpt_dir:
        raise ValueError(_SAME_FOLDER)
    args.num_steps = _parse_num_steps(args.num_steps)
    return args


def main(argv=None):
    args = parse_args(argv)
    train(args.config, args.ckpt_dir, args.num_steps, images_glob=args.images_glob,
          init_autoencoder_from_ckpt_dir=args.init_autoencoder_from_ckpt_dir, batch_size=args.batch_size,
          crop_size=args.crop_size, lpips_weight_path=args.lpips_weight_path, no_lpips=args.no_lpips, seed=args.seed,
          precision_policy=args.precision_policy, model_kwargs=args.model_kwargs,
          discriminator_kwargs=args.discriminator_kwargs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
