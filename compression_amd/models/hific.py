"""Mentzer, Toderici, Tschannen, Agustsson 2020, "High-Fidelity Generative Image Compression": the HiFiC codec
(models/hific/archs.py:31-33, 67-211, 300-372, 425-581; model.py:117-126, 511-590) — encoder, generator, hyperprior,
the coding path, and the conditional patch discriminator.  The losses and the alternating training step are in
hific_train.py.  Not here: LPIPS weights, datasets and the published checkpoints."""
from __future__ import annotations

import collections
import math

import torch

from .. import distributions, entropy_models, layers
from ..layers import functional, gan_functional
from ..layers.channel_norm import ChannelNorm
from ..layers.keras_conv import KerasConv2D, KerasConv2DTranspose
from ..layers.spectral_norm import SpectralNormConv2D
from ..ops import round_ops
from ..pipeline import inline_lane

__all__ = ["Encoder", "Decoder", "ResidualBlock", "Hyperprior", "HiFiCModel", "Discriminator", "Nodes", "BppPair",
           "padded_size", "latent_size", "hyper_latent_size"]

# model.py:40-52: what the training step hands from the codec to the losses and the discriminator
Nodes = collections.namedtuple("Nodes", ["input_image", "input_image_scaled", "reconstruction",
                                         "reconstruction_scaled", "latent_quantized"])
BppPair = collections.namedtuple("BppPair", ["total_nbpp", "total_qbpp"])

SCALES_MIN, SCALES_MAX, SCALES_LEVELS = 0.11, 256.0, 64          # archs.py:31-33


def padded_size(h, w, num_down=4):
    """model.py:117-126: H and W up to the next multiple of 2 ** num_down."""
    f = 2 ** num_down
    return -(-h // f) * f, -(-w // f) * f


def latent_size(h, w, num_down=4):
    ph, pw = padded_size(h, w, num_down)
    return ph >> num_down, pw >> num_down


def hyper_latent_size(h, w, num_down=4):
    """The hyper-analysis has two stride-2 `same_zeros` layers (archs.py:442-451): ceil(ceil(n / 2) / 2)."""
    lh, lw = latent_size(h, w, num_down)
    return -(-(-(-lh // 2)) // 2), -(-(-(-lw // 2)) // 2)


class Encoder(torch.nn.Module):
    """archs.py:67-109: Conv2D 7x7 -> `num_down` x (Conv2D 3x3 stride 2) each with ChannelNorm and ReLU (one launch
    behind the convolution), then Conv2D 3x3 to the bottleneck."""

    def __init__(self, num_down=4, num_filters_base=60, num_filters_bottleneck=220):
        super().__init__()
        self.num_down = num_down
        widths = [num_filters_base * 2 ** i for i in range(num_down + 1)]
        convs = [KerasConv2D(widths[0], 7, in_channels=3)]
        convs += [KerasConv2D(widths[i + 1], 3, strides=2, in_channels=widths[i]) for i in range(num_down)]
        self.convs = torch.nn.ModuleList(convs)
        self.norms = torch.nn.ModuleList(ChannelNorm(num_channels=c) for c in widths)
        self.conv_out = KerasConv2D(num_filters_bottleneck, 3, in_channels=widths[-1])

    @property
    def num_downsampling_layers(self):
        return self.num_down

    def forward(self, x):
        for conv, norm in zip(self.convs, self.norms):
            x = norm(conv(x), relu=True)
        return self.conv_out(x)


class ResidualBlock(torch.nn.Module):
    """archs.py:176-211: x + ChannelNorm(Conv2D(ReLU(ChannelNorm(Conv2D(x))))).  Fused: each convolution is followed
    by ONE launch (norm + ReLU; norm + the block's input)."""

    def __init__(self, filters, kernel_size=3):
        super().__init__()
        self.conv_0 = KerasConv2D(filters, kernel_size, in_channels=filters)
        self.norm_0 = ChannelNorm(num_channels=filters)
        self.conv_1 = KerasConv2D(filters, kernel_size, in_channels=filters)
        self.norm_1 = ChannelNorm(num_channels=filters)

    def forward(self, x, fused=True):
        if fused:
            return self.norm_1(self.conv_1(self.norm_0(self.conv_0(x), relu=True)), residual=x)
        return x + self.norm_1(self.conv_1(torch.relu(self.norm_0(self.conv_0(x)))))


class Decoder(torch.nn.Module):
    """archs.py:112-173, the generator: head (ChannelNorm, Conv2D 3x3, ChannelNorm), `num_residual_blocks` residual
    blocks, the skip over them, `num_up` x (Conv2DTranspose 3x3 stride 2, ChannelNorm, ReLU), Conv2D 7x7 to 3 channels.
    The skip `after_res += after_head` (archs.py:172) stays a tensor add: the last block's norm already carries the
    block's own input as its residual, and the kernel takes one residual pointer.  `fused = False` runs every
    ChannelNorm plain and the ReLUs / adds as tensor ops (what tests compare the fused launches against)."""

    def __init__(self, num_up=4, num_filters_base=60, num_residual_blocks=9, in_channels=220):
        super().__init__()
        wide = num_filters_base * 2 ** num_up
        self.fused = True
        self.head_norm_0 = ChannelNorm(num_channels=in_channels)
        self.head_conv = KerasConv2D(wide, 3, in_channels=in_channels)
        self.head_norm_1 = ChannelNorm(num_channels=wide)
        self.residual_blocks = torch.nn.ModuleList(ResidualBlock(wide, 3) for _ in range(num_residual_blocks))
        widths = [num_filters_base * 2 ** s for s in reversed(range(num_up))]
        self.tail_convs = torch.nn.ModuleList(
            KerasConv2DTranspose(c, 3, strides=2, in_channels=cin) for c, cin in zip(widths, [wide] + widths[:-1]))
        self.tail_norms = torch.nn.ModuleList(ChannelNorm(num_channels=c) for c in widths)
        self.conv_out = KerasConv2D(3, 7, in_channels=widths[-1] if widths else wide)

    def forward(self, y):
        after_head = self.head_norm_1(self.head_conv(self.head_norm_0(y)))
        t = after_head
        for block in self.residual_blocks:
            t = block(t, fused=self.fused)
        t = t + after_head
        for conv, norm in zip(self.tail_convs, self.tail_norms):
            t = norm(conv(t), relu=True) if self.fused else torch.relu(norm(conv(t)))
        return self.conv_out(t)


def _pad32(c):
    return c if c % 32 == 0 else -(-c // 32) * 32


class Hyperprior(torch.nn.Module):
    """archs.py:425-493: hyper-analysis (3x3, 5x5 / 2, 5x5 / 2) and two hyper-syntheses (5x5 x 2, 5x5 x 2, 3x3), one
    for the latents' scales and one for their means; SignalConv2D `same_zeros` with bias.

    A bottleneck width the convolution kernels do not take (220) is carried as the next multiple of 32 at the two
    places it meets them: the latents get zero channels in front of the analysis, and the syntheses' last layers
    produce the padded width, of which the first `num_chan_bottleneck` channels are used.  The extra weights see zeros
    or are never read; a reference checkpoint maps onto the leading channels."""

    def __init__(self, num_chan_bottleneck=220, num_filters=320):
        super().__init__()
        self.num_chan_bottleneck, self.num_filters = num_chan_bottleneck, num_filters
        C, B = num_filters, _pad32(num_chan_bottleneck)
        conv = lambda f, k, cin, **kw: layers.SignalConv2D(f, (k, k), padding="same_zeros", use_bias=True,
                                                           in_channels=cin, **kw)
        self.analysis = torch.nn.Sequential(
            conv(C, 3, B, corr=True, activation="relu"),
            conv(C, 5, C, corr=True, strides_down=2, activation="relu"),
            conv(C, 5, C, corr=True, strides_down=2, activation=None))

        def synthesis():
            kw = dict(corr=False, kernel_parameter="variable")
            return torch.nn.Sequential(
                conv(C, 5, C, strides_up=2, activation="relu", **kw),
                conv(C, 5, C, strides_up=2, activation="relu", **kw),
                conv(B, 3, C, activation=None, **kw))
        self.synthesis_scale = synthesis()
        self.synthesis_mean = synthesis()
        self.side_prior = distributions.NoisyDeepFactorized(batch_shape=(num_filters,))

    def analyse(self, y):
        extra = _pad32(self.num_chan_bottleneck) - y.shape[-1]
        return self.analysis(torch.nn.functional.pad(y, (0, extra)) if extra else y)

    def synthesise(self, z_hat, latent_shape):
        """(scale indexes, means), cropped to the latents' extent (archs.py:525-527)."""
        h, w = latent_shape
        scales = self.synthesis_scale(z_hat)[:, :h, :w, :self.num_chan_bottleneck]
        means = self.synthesis_mean(z_hat)[:, :h, :w, :self.num_chan_bottleneck]
        return scales.contiguous(), means.contiguous()


class Discriminator(torch.nn.Module):
    """archs.py:300-372, the conditional patch discriminator; every convolution is spectrally normalised
    (SpectralNormConv2D), every leaky ReLU has slope 0.2:

      latent [N, h, w, Cy] -> conv 12, 3x3 -> lrelu -> nearest resize to H x W -> concat behind x [N, H, W, 3] (15)
      -> `num_layers` x (conv 4x4 / 2, lrelu) with base, 2 base, ... filters (at most 512)
      -> conv 4x4 (the next width), lrelu -> conv 4x4 to 1 channel
      -> logits reshaped to [-1, 1] and their sigmoid: (probabilities, logits).

    `fused = True`: the front end (lrelu, resize, concat and the zero channels the next convolution wants) is one
    launch, and each leaky ReLU runs in place behind its convolution with its backward fused with the bias gradient.
    `fused = False`: the same normalised kernels with lrelu, resize, concat and padding as tensor ops (what the tests
    compare the fused launches against)."""

    def __init__(self, num_filters_base=64, num_layers=3, in_channels_latent=220):
        super().__init__()
        self.fused = True
        self.latent_conv = SpectralNormConv2D(12, 3, in_channels=in_channels_latent)
        widths, cin = [], 3 + 12
        for i in range(num_layers + 1):
            widths.append(min(num_filters_base * 2 ** i, 512))
        convs = []
        for i, c in enumerate(widths):
            convs.append(SpectralNormConv2D(c, 4, strides=2 if i < num_layers else 1, in_channels=cin))
            cin = c
        self.convs = torch.nn.ModuleList(convs)
        self.conv_out = SpectralNormConv2D(1, 4, in_channels=cin)

    def output_size(self, h, w):
        """Spatial extent of the logits for an H x W image (before they are flattened)."""
        for conv in self.convs:
            h, w = conv.output_size(h, w)
        return self.conv_out.output_size(h, w)

    def forward(self, x, latent):
        if x.dim() != 4 or latent.dim() != 4 or x.shape[0] != latent.shape[0]:
            raise ValueError(f"x [N, H, W, 3] and latent [N, h, w, C] expected, got {tuple(x.shape)}, "
                             f"{tuple(latent.shape)}")
        t = self.latent_conv(latent.to(x.dtype)).contiguous()
        front = gan_functional.disc_front if self.fused else gan_functional.disc_front_composite
        t = front(x, t, self.convs[0].padded_in_channels())
        for conv in self.convs:
            if self.fused:
                t = conv(t, lrelu=True)
            else:
                t = torch.nn.functional.leaky_relu(conv(t), gan_functional.LRELU_SLOPE)
        logits = self.conv_out(t).reshape(-1, 1)
        return torch.sigmoid(logits), logits


class HiFiCModel(torch.nn.Module):
    """The codec.  The reference's tfc.GaussianConditional(scales, scale_table, mean) (archs.py:518-532) is this
    project's LocationScaleIndexedEntropyModel over the same 64 log-spaced scales: the scale synthesis gives the table
    index, as in BMSHJ2018Model.  One deviation from the reference: the image is padded to a multiple of 2 ** num_down
    with ZEROS, where model.py:123-125 mirrors it (tf.pad REFLECT)."""
    # layout of the container: [string, side_string, x_shape, y_shape, z_shape]
    num_strings, num_packed = 2, 5

    def __init__(self, num_down=4, num_filters_base=60, num_filters_bottleneck=220, num_residual_blocks=9,
                 num_filters_hyper=320, num_scales=SCALES_LEVELS, scale_min=SCALES_MIN, scale_max=SCALES_MAX,
                 lmbda=0.01, compute_dtype=torch.float32):
        super().__init__()
        self.num_down, self.num_scales, self.lmbda = num_down, num_scales, lmbda
        self.compute_dtype = compute_dtype
        offset = math.log(scale_min)
        factor = (math.log(scale_max) - math.log(scale_min)) / (num_scales - 1.0)
        self.scale_fn = lambda i: torch.exp(offset + factor * i)
        self.encoder = Encoder(num_down, num_filters_base, num_filters_bottleneck)
        self.decoder = Decoder(num_down, num_filters_base, num_residual_blocks, num_filters_bottleneck)
        self.hyperprior = Hyperprior(num_filters_bottleneck, num_filters_hyper)
        self.entropy_model = self.side_entropy_model = None

    def _models(self, compression):
        em = entropy_models.LocationScaleIndexedEntropyModel(
            distributions.NoisyNormal, self.num_scales, self.scale_fn, coding_rank=3,
            compression=compression, bottleneck_dtype=self.compute_dtype)
        side = entropy_models.ContinuousBatchedEntropyModel(
            self.hyperprior.side_prior, coding_rank=3, compression=compression, bottleneck_dtype=self.compute_dtype)
        return em, side

    def init_compression(self):
        self.entropy_model, self.side_entropy_model = self._models(True)
        return self

    def pad_image(self, x):
        """model.py:117-126: bottom / right up to a multiple of 2 ** num_down (zeros here, mirrored there)."""
        h, w = x.shape[1:3]
        ph, pw = padded_size(h, w, self.num_down)
        if (ph, pw) == (h, w):
            return x
        return functional.pad2d(x, (0, ph - h), (0, pw - w))

    def reconstruct(self, y_hat, x_shape):
        """Generator on (quantised) latents -> the image in [0, 1] units, cropped to x_shape (model.py:562-590)."""
        return self.decoder(y_hat.to(self.compute_dtype))[:, :x_shape[0], :x_shape[1], :]

    def forward(self, x, latents=None):
        """The autoencoder path of the reference's evaluation graph with straight-through rounding (archs.py:539,
        573-581): x [B, H, W, 3] in [0, 255] -> (reconstruction in [0, 255], bits [B]), differentiable end to end.
        The bits are the noisy-likelihood estimates the reference's rate loss uses (archs.py:653-687, nbits) of latents
        and hyper-latents.  `latents`: quantised latents to decode instead of the encoder's own."""
        em, side = self._models(False)
        x_shape = tuple(x.shape[1:3])
        u = self.pad_image(x.to(self.compute_dtype) / 255.0)
        y = self.encoder(u)
        z = self.hyperprior.analyse(y)
        _, side_bits = side(z, training=True)
        z_hat = side.quantize(z).to(self.compute_dtype)
        scales, means = self.hyperprior.synthesise(z_hat, tuple(y.shape[1:3]))
        _, bits = em(y, scales, loc=means, training=True)
        y_hat = round_ops.round_st(y, means) if latents is None else latents
        x_hat = self.reconstruct(y_hat, x_shape) * 255.0
        return x_hat, bits.float() + side_bits.float()

    def training_nodes(self, x):
        """What the training step needs of one pass (model.py:365-455, archs.py:496-581, 653-687): x [B, H, W, 3] in
        [0, 255] -> (Nodes(input, input / 255, reconstruction * 255, reconstruction, latent_quantized), BppPair(
        total_nbpp, total_qbpp)).  The reconstruction comes from the straight-through quantised latents, total_nbpp
        from the noisy likelihoods and total_qbpp from the quantised ones, each of latents plus hyper-latents as
        batch-mean bits per pixel of the input."""
        em, side = self._models(False)
        x_shape = tuple(x.shape[1:3])
        scaled = x.to(self.compute_dtype) / 255.0
        y = self.encoder(self.pad_image(scaled))
        z = self.hyperprior.analyse(y)
        _, side_nbits = side(z, training=True)
        z_hat, side_qbits = side(z, training=False)
        scales, means = self.hyperprior.synthesise(z_hat.to(self.compute_dtype), tuple(y.shape[1:3]))
        _, nbits = em(y, scales, loc=means, training=True)
        _, qbits = em(y, scales, loc=means, training=False)
        y_hat = round_ops.round_st(y, means)
        rec = self.reconstruct(y_hat, x_shape)
        pixels = float(x_shape[0] * x_shape[1])
        nbpp = (nbits.float() + side_nbits.float()).mean() / pixels
        qbpp = (qbits.float() + side_qbits.float()).mean() / pixels
        return Nodes(x, scaled, rec * 255.0, rec, y_hat), BppPair(nbpp, qbpp)

    @torch.no_grad()
    def latents(self, x):
        """(y, y_hat, z, means, scale indexes) of a uint8 image batch as compress() computes them."""
        u = self.pad_image(functional.image_to_unit(x, self.compute_dtype))
        y = self.encoder(u)
        z = self.hyperprior.analyse(y)
        z_hat = self.side_entropy_model.quantize(z)
        scales, means = self.hyperprior.synthesise(z_hat.to(self.compute_dtype), tuple(y.shape[1:3]))
        return y, self.entropy_model.quantize(y, loc=means), z, means, scales

    @torch.no_grad()
    def compress(self, x, device_result=False, lane=None):
        """uint8 [B, H, W, 3] -> (string[B], side_string[B], x_shape, y_shape, z_shape) — model.py:511-545,
        archs.py:496-559.  `device_result`, `lane`: as BMSHJ2018Model.compress."""
        lane = lane or inline_lane()
        if x.dim() == 3:
            x = x[None]
        with lane.on("transform"):
            y, _, z, means, scales = self.latents(x)
            x_shape, y_shape, z_shape = tuple(x.shape[1:-1]), tuple(y.shape[1:-1]), tuple(z.shape[1:-1])
        with lane.on("coder"):
            side_string = self.side_entropy_model.compress(z, device_result=device_result)
            string = self.entropy_model.compress(y, scales, loc=means, device_result=device_result)
        if device_result:
            string._keep += [y, scales, means]
            side_string._keep += [z]
        return string, side_string, x_shape, y_shape, z_shape

    @torch.no_grad()
    def decode_latents(self, string, side_string, y_shape, z_shape, defer_sanity=False, lane=None):
        """The latents the generator gets: hyper-latents first, then the latents with their means and scales."""
        lane = lane or inline_lane()
        ok = []
        with lane.on("coder"):
            z_hat = self.side_entropy_model.decompress(side_string, z_shape, defer_sanity=defer_sanity)
        if defer_sanity:
            z_hat, okz = z_hat
            ok.append(okz)
        with lane.on("transform"):
            scales, means = self.hyperprior.synthesise(z_hat.to(self.compute_dtype), y_shape)
        with lane.on("coder"):
            y_hat = self.entropy_model.decompress(string, scales, loc=means, defer_sanity=defer_sanity)
        if defer_sanity:
            y_hat, oky = y_hat
            ok.append(oky)
        return y_hat, ok, (z_hat, scales, means)

    @torch.no_grad()
    def decompress(self, string, side_string, x_shape, y_shape, z_shape, defer_sanity=False, lane=None):
        """-> uint8 [B, H, W, 3] (model.py:562-590: crop, scale by 255, clip); `defer_sanity`: (x_hat, [ok_z, ok_y])."""
        lane = lane or inline_lane()
        y_hat, ok, keep = self.decode_latents(string, side_string, y_shape, z_shape, defer_sanity, lane)
        with lane.on("transform"):
            x_hat = functional.unit_to_image(self.reconstruct(y_hat, x_shape).contiguous())
            x_hat._tfc_keep = keep + (y_hat,)
        return (x_hat, ok) if defer_sanity else x_hat


if __name__ == "__main__":      # python -m compression_amd.models.hific compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(HiFiCModel))
