"""HiFiC's losses and its alternating discriminator / generator training step (models/hific/configs.py:20-77;
model.py:61-115, 365-455, 588-764, 800-837, 875-897) on this library's kernels.

Not here: datasets and the input pipeline, summaries, checkpoints and hooks.  The perceptual term is
`perceptual_loss(fake_scaled, real_scaled) -> scalar`: `layers.LPIPSLoss(layers.LPIPS.from_lpips_package(...))` is LPIPS
on this library's kernels (the network is here, its trained weights are the user's), or any other callable.  The reference's third ("aux") optimiser minimises
the entropy model's auxiliary loss (model.py:807-811); the entropy models of this library have no auxiliary loss (their
tails are solved on the device, not learned), so there are three optimisers: transform, entropy, disc."""
from __future__ import annotations

import collections

import torch

from ..layers import gan_functional
from .hific import BppPair, Nodes  # noqa: F401

__all__ = ["CONFIGS", "Config", "LossConfig", "Schedule", "scheduled_value", "rd_loss", "gan_losses", "HiFiCTrainer"]

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
