"""Scale-space flow video compression (Agustsson, Minnen, Johnston, Ballé, Hwang, Toderici, "Scale-space flow for
end-to-end optimized video compression", CVPR 2020, sections 3 and 4).

The first frame of a clip is coded by an image codec; every later frame by a motion codec, whose decoder emits a
3-channel field (dx, dy, s), and a residual codec.  The field samples the scale-space volume of the previous
reconstruction (`ops.flow_ops.scale_space_predict`, section 3.1): where motion is uncertain the network picks a
blurrier plane instead of a wrong sharp one.  All three codecs are mean-scale hyperprior codecs built from the layers
and entropy models of bmshj2018 / ms2020.

The reference tree carries no program text for this model; the layer shapes, the operator's definition
(include/tfc_hip.h) and the container layout are this project's own, and parity with the authors' trained models is
unpinned.

    python -m compression_amd.models.ssf2020 --model_path m.pt train --train_glob 'clips/*.y4m'
    python -m compression_amd.models.ssf2020 --model_path m.pt compress in.y4m out.tfci
    python -m compression_amd.models.ssf2020 --model_path m.pt decompress out.tfci rec.y4m"""
from __future__ import annotations

import argparse
import math

import numpy as np
import torch

from .. import distributions, entropy_models, layers
from ..ops import flow_ops, gen_ops
from ..util import PackedTensors
from .bmshj2018 import HyperAnalysisTransform, HyperSynthesisTransform

__all__ = ["Encoder", "Decoder", "HyperpriorCodec", "SSF2020Model", "pack_clip", "unpack_clip", "compress_file",
           "decompress_file", "main"]

FRAME_MULTIPLE = 64          # four stride-2 layers in the frame codecs, two more in the hyper codecs


def _conv(C, k, cin, **kw):
    return layers.SignalConv2D(C, (k, k), padding="same_zeros", in_channels=cin, **kw)


class Encoder(torch.nn.Module):
    """Four 5x5 stride-2 convolutions, ReLU after the first three: cin -> F -> F -> F -> latent_depth."""

    def __init__(self, cin, num_filters=128, latent_depth=192):
        super().__init__()
        F = num_filters
        kw = dict(corr=True, strides_down=2, use_bias=True)
        self.layer_0 = _conv(F, 5, cin, activation="relu", **kw)
        self.layer_1 = _conv(F, 5, F, activation="relu", **kw)
        self.layer_2 = _conv(F, 5, F, activation="relu", **kw)
        self.layer_3 = _conv(latent_depth, 5, F, activation=None, **kw)

    def forward(self, x):
        return self.layer_3(self.layer_2(self.layer_1(self.layer_0(x))))


class Decoder(torch.nn.Module):
    """The mirror: cin -> F -> F -> F -> cout with strides_up=2."""

    def __init__(self, cin, cout, num_filters=128):
        super().__init__()
        F = num_filters
        kw = dict(corr=False, strides_up=2, use_bias=True)
        self.layer_0 = _conv(F, 5, cin, activation="relu", **kw)
        self.layer_1 = _conv(F, 5, F, activation="relu", **kw)
        self.layer_2 = _conv(F, 5, F, activation="relu", **kw)
        self.layer_3 = _conv(cout, 5, F, activation=None, **kw)

    def forward(self, y):
        return self.layer_3(self.layer_2(self.layer_1(self.layer_0(y))))


class HyperpriorCodec(torch.nn.Module):
    """The mean-scale hyperprior of one latent: a hyper-analysis shaped like bmshj2018's, two hyper-syntheses (scale
    indexes and means) and the factorized prior of z."""

    def __init__(self, latent_depth):
        super().__init__()
        self.hyper_analysis = HyperAnalysisTransform(latent_depth)
        self.hyper_synthesis_scale = HyperSynthesisTransform(latent_depth)
        self.hyper_synthesis_mean = HyperSynthesisTransform(latent_depth)
        self.hyperprior = distributions.NoisyDeepFactorized(batch_shape=(latent_depth,))

    def parameters_of(self, z_hat, y_shape):
        """-> (scale indexes, means), cropped to the latent's extent."""
        indexes = self.hyper_synthesis_scale(z_hat)[:, :y_shape[0], :y_shape[1], :]
        means = self.hyper_synthesis_mean(z_hat)[:, :y_shape[0], :y_shape[1], :]
        return indexes.contiguous(), means.contiguous()


class SSF2020Model(torch.nn.Module):
    def __init__(self, lmbda=0.01, num_filters=128, latent_depth=192, num_levels=5, sigma0=1.5, num_scales=64,
                 scale_min=0.11, scale_max=256.0, compute_dtype=torch.float32):
        super().__init__()
        flow_ops._check_levels(num_levels, sigma0)
        self.lmbda, self.num_scales, self.compute_dtype = lmbda, num_scales, compute_dtype
        self.num_levels, self.sigma0, self.latent_depth = int(num_levels), float(sigma0), latent_depth
        offset = math.log(scale_min)
        factor = (math.log(scale_max) - math.log(scale_min)) / (num_scales - 1.0)
        self.scale_fn = lambda i: torch.exp(offset + factor * i)
        F, L = num_filters, latent_depth
        self.img_encoder, self.img_decoder = Encoder(3, F, L), Decoder(L, 3, F)
        self.motion_encoder, self.motion_decoder = Encoder(6, F, L), Decoder(L, 3, F)
        self.res_encoder, self.res_decoder = Encoder(3, F, L), Decoder(2 * L, 3, F)
        self.img_codec, self.motion_codec, self.res_codec = HyperpriorCodec(L), HyperpriorCodec(L), HyperpriorCodec(L)
        self.em_y = self.em_z_img = self.em_z_motion = self.em_z_res = None

    # ---------------------------------------------------------------------------------------------------------------

    def _codecs(self):
        return (("img", self.img_codec), ("motion", self.motion_codec), ("res", self.res_codec))

    def _models(self, compression):
        """(em_y, {codec name: em_z}).  The three latents share one indexed model: its tables hold no parameter."""
        em_y = entropy_models.LocationScaleIndexedEntropyModel(
            distributions.NoisyNormal, self.num_scales, self.scale_fn, coding_rank=3, compression=compression,
            bottleneck_dtype=self.compute_dtype)
        em_z = {name: entropy_models.ContinuousBatchedEntropyModel(
            codec.hyperprior, coding_rank=3, compression=compression, offset_heuristic=False,
            bottleneck_dtype=self.compute_dtype) for name, codec in self._codecs()}
        return em_y, em_z

    def init_compression(self):
        self.em_y, em_z = self._models(True)
        self.em_z_img, self.em_z_motion, self.em_z_res = em_z["img"], em_z["motion"], em_z["res"]
        return self

    def _predict(self, x_ref, flow):
        """The scale-space prediction, in float32 whatever compute_dtype is."""
        pred = flow_ops.scale_space_predict(x_ref.float().contiguous(), flow.float().contiguous(), self.num_levels,
                                            self.sigma0)
        return pred.to(self.compute_dtype)

    def _latent(self, codec, em_y, em_z, y, training):
        """One mean-scale hyperprior latent in training form -> (y_hat, bits per batch element)."""
        y_shape = tuple(y.shape[1:-1])
        z = codec.hyper_analysis(y)
        _, z_bits = em_z(z, training=training)
        z_hat = em_z.quantize(z).to(self.compute_dtype)
        indexes, means = codec.parameters_of(z_hat, y_shape)
        _, y_bits = em_y(y, indexes, loc=means, training=training)
        y_hat = em_y.quantize(y, loc=means).to(self.compute_dtype)
        return y_hat, z_bits + y_bits

    def forward(self, clip, training=True):
        """clip [B, T, H, W, 3] on the 0...255 scale -> (loss, bpp, mse), bpp and mse averaged over the T frames (mse on
        the 0...255 scale)."""
        if clip.dim() != 5 or clip.shape[-1] != 3:
            raise ValueError(f"clip must be [B, T, H, W, 3], received shape {tuple(clip.shape)}")
        _, frames, h, w, _ = clip.shape
        if h % FRAME_MULTIPLE or w % FRAME_MULTIPLE or frames < 1:
            raise ValueError(f"forward needs H and W to be multiples of {FRAME_MULTIPLE} and at least one frame, "
                             f"received shape {tuple(clip.shape)}")
        em_y, em_z = self._models(False)
        num_pixels = h * w
        x = (clip.to(self.compute_dtype) / 255.0).contiguous()
        bpp = mse = 0.0
        x_ref = None
        for t in range(frames):
            x_cur = x[:, t].contiguous()
            if t == 0:
                y_hat, bits = self._latent(self.img_codec, em_y, em_z["img"], self.img_encoder(x_cur), training)
                x_hat = self.img_decoder(y_hat)
            else:
                y_motion = self.motion_encoder(torch.cat([x_cur, x_ref], dim=-1))
                y_motion_hat, bits = self._latent(self.motion_codec, em_y, em_z["motion"], y_motion, training)
                x_pred = self._predict(x_ref, self.motion_decoder(y_motion_hat))
                y_res = self.res_encoder(x_cur - x_pred)
                y_res_hat, res_bits = self._latent(self.res_codec, em_y, em_z["res"], y_res, training)
                bits = bits + res_bits
                x_hat = x_pred + self.res_decoder(torch.cat([y_res_hat, y_motion_hat], dim=-1))
            bpp = bpp + bits.mean() / num_pixels
            mse = mse + torch.mean((255.0 * (x_cur.float() - x_hat.float())) ** 2)
            x_ref = torch.clamp(x_hat, 0.0, 1.0)              # not detached: the gradient runs down the chain
        bpp, mse = bpp / frames, (mse / frames).to(bpp.dtype)
        return bpp + self.lmbda * mse, bpp, mse

    # ---------------------------------------------------------------------------------------------------------------
    # the codec

    def _encode_latent(self, codec, em_z, y):
        """-> (z, what em_y codes (y - means), scale indexes, y_hat as the decoder will see it)."""
        y_shape, z = tuple(y.shape[1:-1]), codec.hyper_analysis(y)
        # the closed loop uses quantize() in place of a decode of the string (as ms2020's compress does)
        z_hat = em_z.quantize(z).to(self.compute_dtype)
        indexes, means = codec.parameters_of(z_hat, y_shape)
        y_hat = self.em_y.quantize(y, loc=means).to(self.compute_dtype)
        return z, (y - means).contiguous(), indexes, y_hat

    def _decode_latent(self, codec, em_z, z_string, y_string, y_shape):
        z_shape = tuple(-(-s // 4) for s in y_shape)
        z_hat = em_z.decompress(_strings([z_string]), z_shape).to(self.compute_dtype)
        indexes, means = codec.parameters_of(z_hat, y_shape)
        return self.em_y.decompress(_strings([y_string]), indexes, loc=means).to(self.compute_dtype)

    @staticmethod
    def _to_image(x_hat, shape):
        return torch.clamp(torch.round(x_hat[0, :shape[1], :shape[2]].float() * 255.0), 0, 255).to(torch.uint8)

    @torch.no_grad()
    def compress(self, clip, return_reconstruction=False):
        """uint8 [T, H, W, 3] -> (shape (T, H, W), strings): strings[0] = [z, y] of the I-frame, strings[t] =
        [z_motion, y_motion, z_res, y_res] of P-frame t.  Frames are replicate-padded to multiples of 64.  With
        `return_reconstruction` also the encoder's own closed-loop reconstruction, uint8 [T, H, W, 3]."""
        if clip.dim() != 4 or clip.shape[-1] != 3 or clip.dtype != torch.uint8 or clip.shape[0] < 1:
            raise ValueError(f"clip must be uint8 [T, H, W, 3], received {clip.dtype} {tuple(clip.shape)}")
        if self.em_y is None:
            raise RuntimeError("compress needs init_compression()")
        frames, h, w, _ = clip.shape
        shape = (int(frames), int(h), int(w))
        ph, pw = -h % FRAME_MULTIPLE, -w % FRAME_MULTIPLE
        x = clip.to(self.compute_dtype) / 255.0
        if ph or pw:
            x = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (0, pw, 0, ph), mode="replicate").permute(0, 2, 3, 1)
        x = x.contiguous()
        strings, recon, x_ref = [], [], None
        for t in range(frames):
            x_cur = x[t:t + 1].contiguous()
            if t == 0:
                z, coded, indexes, y_hat = self._encode_latent(self.img_codec, self.em_z_img, self.img_encoder(x_cur))
                x_hat = self.img_decoder(y_hat)
                zs, ys, idx = [(self.em_z_img, z)], [coded], [indexes]
            else:
                y_motion = self.motion_encoder(torch.cat([x_cur, x_ref], dim=-1))
                zm, cm, im, y_motion_hat = self._encode_latent(self.motion_codec, self.em_z_motion, y_motion)
                x_pred = self._predict(x_ref, self.motion_decoder(y_motion_hat))
                zr, cr, ir, y_res_hat = self._encode_latent(self.res_codec, self.em_z_res, self.res_encoder(x_cur - x_pred))
                x_hat = x_pred + self.res_decoder(torch.cat([y_res_hat, y_motion_hat], dim=-1))
                zs, ys, idx = [(self.em_z_motion, zm), (self.em_z_res, zr)], [cm, cr], [im, ir]
            # the coder calls of the frame go out together, behind its transforms
            y_handles = self.em_y.compress_many(ys, idx)
            z_handles = [em.compress_many([z])[0] for em, z in zs]
            frame = []
            for zh, yh in zip(z_handles, y_handles):
                frame += [bytes(gen_ops.fetch_strings(zh).reshape(-1)[0]), bytes(gen_ops.fetch_strings(yh).reshape(-1)[0])]
            strings.append(frame)
            x_ref = torch.clamp(x_hat, 0.0, 1.0)
            if return_reconstruction:
                recon.append(self._to_image(x_hat, shape))
        if return_reconstruction:
            return shape, strings, torch.stack(recon)
        return shape, strings

    @torch.no_grad()
    def decompress(self, shape, strings):
        """(T, H, W) and the strings of `compress` -> uint8 [T, H, W, 3]."""
        frames, h, w = (int(v) for v in shape)
        if len(strings) != frames or len(strings[0]) != 2 or any(len(s) != 4 for s in strings[1:]):
            raise ValueError("decompress: 2 strings for the first frame and 4 for every later one are needed")
        if self.em_y is None:
            raise RuntimeError("decompress needs init_compression()")
        y_shape = (-(-h // FRAME_MULTIPLE) * 4, -(-w // FRAME_MULTIPLE) * 4)
        out, x_ref = [], None
        for t, frame in enumerate(strings):
            if t == 0:
                y_hat = self._decode_latent(self.img_codec, self.em_z_img, frame[0], frame[1], y_shape)
                x_hat = self.img_decoder(y_hat)
            else:
                y_motion_hat = self._decode_latent(self.motion_codec, self.em_z_motion, frame[0], frame[1], y_shape)
                x_pred = self._predict(x_ref, self.motion_decoder(y_motion_hat))
                y_res_hat = self._decode_latent(self.res_codec, self.em_z_res, frame[2], frame[3], y_shape)
                x_hat = x_pred + self.res_decoder(torch.cat([y_res_hat, y_motion_hat], dim=-1))
            x_ref = torch.clamp(x_hat, 0.0, 1.0)
            out.append(self._to_image(x_hat, (frames, h, w)))
        return torch.stack(out)


def _strings(values):
    arr = np.empty(len(values), dtype=object)
    arr[:] = [bytes(v) for v in values]
    return arr


# -------------------------------------------------------------------------------------------------------------------
# the container and the commands


def pack_clip(shape, strings) -> bytes:
    """One PackedTensors container for a clip: the shape (T, H, W), then every string, frame by frame."""
    packed = PackedTensors()
    packed.pack([np.asarray(shape, dtype=np.int32), _strings([s for frame in strings for s in frame])])
    return packed.string


def unpack_clip(data):
    """-> (shape, strings) as `SSF2020Model.decompress` takes them."""
    shape, flat = PackedTensors(data).unpack([np.int32, bytes])
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or shape[0] < 1 or len(flat) != 2 + 4 * (shape[0] - 1):
        raise ValueError(f"not a clip container: shape {shape} with {len(flat)} strings")
    flat = [bytes(s) for s in flat]
    return shape, [flat[:2]] + [flat[2 + 4 * k:6 + 4 * k] for k in range(shape[0] - 1)]


def read_y4m(filename, device, max_frames=None):
    """All frames (or the first `max_frames`) of a '.y4m' file as uint8 RGB [T, H, W, 3] on `device`."""
    from ..datasets import Y4MDataset
    from ..ops import video_ops
    frames = []
    for y, cbcr in Y4MDataset(filename, device=device if torch.device(device).type == "cuda" else None).batches(8):
        frames.append(video_ops.ycbcr_to_rgb(y, cbcr))
        if max_frames is not None and sum(f.shape[0] for f in frames) >= max_frames:
            break
    if not frames:
        raise ValueError(f"Input file '{filename}' holds no frame")
    return torch.cat(frames)[:max_frames]


def write_y4m(filename, clip):
    """uint8 RGB [T, H, W, 3] -> a 4:2:0 '.y4m' file (4:4:4 when a side is odd)."""
    from ..datasets import Y4MWriter
    from ..ops import video_ops
    _, h, w, _ = clip.shape
    chroma = "444" if h % 2 or w % 2 else "420jpeg"
    with Y4MWriter(filename, w, h, chroma=chroma) as writer:
        writer.write(*video_ops.rgb_to_ycbcr(clip.contiguous(), chroma="444" if chroma == "444" else "420"))


def compress_file(model, input_file, output_file, max_frames=None):
    device = next(model.parameters()).device
    data = pack_clip(*model.compress(read_y4m(input_file, device, max_frames)))
    with open(output_file, "wb") as f:
        f.write(data)
    return data


def decompress_file(model, input_file, output_file=None):
    with open(input_file, "rb") as f:
        shape, strings = unpack_clip(f.read())
    clip = model.decompress(shape, strings)
    if output_file is not None:
        write_y4m(output_file, clip)
    return clip


MODEL_FLAGS = {"num_filters": int, "latent_depth": int, "num_levels": int, "sigma0": float, "num_scales": int,
               "scale_min": float, "scale_max": float}


def train(args):
    """Trains on random clips of the files of --train_glob and writes the state_dict, range-coding tables included, to
    --model_path."""
    import itertools

    from ..datasets.clip_dataset import ClipDataset
    from .codec_io import compute_dtype_of
    from .train import Trainer
    if not args.train_glob:
        raise SystemExit("train needs --train_glob, the '.y4m' clips to train on")
    if not args.model_path:
        raise SystemExit("train needs --model_path, where the trained model is written")
    torch.manual_seed(args.seed)
    kwargs = {name: getattr(args, name) for name in MODEL_FLAGS}
    model = SSF2020Model(lmbda=args.lmbda, compute_dtype=compute_dtype_of(args.precision_policy), **kwargs).cuda()
    device = next(model.parameters()).device
    common = dict(clip_length=args.clip_length, patchsize=args.patchsize, batch_size=args.batchsize, device=device)
    data = ClipDataset(args.train_glob, seed=args.seed, **common)
    validation = list(itertools.islice(ClipDataset(args.train_glob, seed=args.seed + 1, **common),
                                       max(args.max_validation_steps, 0)))
    trainer = Trainer(model, train_path=args.train_path, nan_check_every=1 if args.check_numerics else 100)
    trainer.fit(data, args.epochs, args.steps_per_epoch, validation_data=validation, verbose=args.verbose)
    torch.save(model.state_dict(), args.model_path)
    return model


def main(argv=None):
    import inspect

    from .codec_io import load_checkpoint
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", default=None)
    ap.add_argument("--verbose", "-V", action="store_true")
    ap.add_argument("--seed", type=int, default=0, help="initialiser seed when no --model_path is given")
    signature = inspect.signature(SSF2020Model.__init__).parameters
    for name, kind in MODEL_FLAGS.items():
        ap.add_argument("--" + name, type=kind, default=signature[name].default)
    sub = ap.add_subparsers(dest="command", required=True)
    sp = sub.add_parser("train")
    sp.add_argument("--lambda", type=float, default=0.01, dest="lmbda")
    sp.add_argument("--train_glob", type=str, default=None)
    sp.add_argument("--train_path", default="/tmp/train_ssf2020")
    sp.add_argument("--batchsize", type=int, default=8)
    sp.add_argument("--patchsize", type=int, default=256)
    sp.add_argument("--clip_length", type=int, default=3)
    sp.add_argument("--epochs", type=int, default=1000)
    sp.add_argument("--steps_per_epoch", type=int, default=1000)
    sp.add_argument("--max_validation_steps", type=int, default=16)
    sp.add_argument("--precision_policy", type=str, default=None)
    sp.add_argument("--check_numerics", action="store_true")
    for name in ("compress", "decompress"):
        sp = sub.add_parser(name)
        sp.add_argument("input_file")
        sp.add_argument("output_file", nargs="?")
        if name == "compress":
            sp.add_argument("--max_frames", type=int, default=None)
    args = ap.parse_args(argv)
    if args.command == "train":
        train(args)
        return 0
    torch.manual_seed(args.seed)
    model = SSF2020Model(**{name: getattr(args, name) for name in MODEL_FLAGS}).cuda()
    if args.model_path:
        model = load_checkpoint(model, torch.load(args.model_path, map_location="cpu"))
    else:
        model = model.init_compression()
    if args.command == "compress":
        compress_file(model, args.input_file, args.output_file or args.input_file + ".tfci", args.max_frames)
    else:
        decompress_file(model, args.input_file, args.output_file or args.input_file + ".y4m")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
