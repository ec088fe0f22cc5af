"""Indexed (conditional) entropy models
(python/entropy_models/continuous_indexed.py:30-633)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..ops import bottleneck_ops, gen_ops, math_ops, round_ops
from . import continuous_base

__all__ = ["ContinuousIndexedEntropyModel", "LocationScaleIndexedEntropyModel"]

_DTYPE_CODE = _lib.DTYPE_CODE_F16


class ContinuousIndexedEntropyModel(continuous_base.ContinuousEntropyModelBase):
    def __init__(self, prior_fn, index_ranges, parameter_fns, coding_rank, channel_axis=-1,
                 compression=False, stateless=False, expected_grads=False, tail_mass=2 ** -8,
                 range_coder_precision=12, bottleneck_dtype=None, prior_dtype=torch.float32,
                 decode_sanity_check=True, laplace_tail_mass=0, coder="range", ans_lanes=64):
        """`coder`: "range" (the reference's bytes) or "ans", the interleaved rANS format of ops.ans_ops with
        `ans_lanes` coder states per stream: other bytes, the same symbols."""
        if not callable(prior_fn):
            raise TypeError("`prior_fn` must be a class or factory function.")
        for name, fn in parameter_fns.items():
            if not isinstance(name, str):
                raise TypeError("`parameter_fns` must have string keys.")
            if not callable(fn):
                raise TypeError(f"`parameter_fns['{name}']` must be callable.")
        super().__init__(coding_rank=coding_rank, compression=compression, stateless=stateless,
                         expected_grads=expected_grads, tail_mass=tail_mass,
                         bottleneck_dtype=bottleneck_dtype, laplace_tail_mass=laplace_tail_mass, coder=coder,
                         ans_lanes=ans_lanes)
        self._index_ranges = tuple(int(r) for r in index_ranges)
        if not self.index_ranges:
            raise ValueError("`index_ranges` must have at least one element.")
        self._channel_axis = None if channel_axis is None else int(channel_axis)
        if self.channel_axis is None and len(self.index_ranges) > 1:
            raise ValueError("`channel_axis` can't be `None` for `len(index_ranges) > 1`.")
        self._prior_fn = prior_fn
        self._parameter_fns = dict(parameter_fns)
        self._prior_dtype = prior_dtype
        self.decode_sanity_check = decode_sanity_check
        self.fused = True
        if self.compression:
            if self.channel_axis is None:
                indexes = torch.arange(self.index_ranges[0], dtype=torch.int32)
            else:
                grids = torch.meshgrid(*[torch.arange(r, dtype=torch.int32) for r in self.index_ranges],
                                       indexing="ij")
                indexes = torch.stack(grids, dim=self.channel_axis)
            self._prior = self._make_prior(indexes)
            cdf, cdf_offset = self._build_tables(self.prior, range_coder_precision)
            self._init_compression(cdf, cdf_offset, None)

    index_ranges = property(lambda self: self._index_ranges)
    parameter_fns = property(lambda self: self._parameter_fns)
    prior_dtype = property(lambda self: self._prior_dtype)
    prior_fn = property(lambda self: self._prior_fn)
    channel_axis = property(lambda self: self._channel_axis)

    def _make_prior(self, indexes):
        indexes = indexes.to(self.prior_dtype)
        parameters = {k: f(indexes) for k, f in self.parameter_fns.items()}
        prior = self.prior_fn(**parameters)
        assert prior.dtype == self.prior_dtype
        if len(prior.event_shape):
            raise ValueError("`prior` must be a (batch of) scalar distribution(s).")
        return prior

    def _normalize_indexes(self, indexes):
        indexes = math_ops.lower_bound(indexes, 0)
        if self.channel_axis is None:
            bounds = self.index_ranges[0] - 1       # a number: a device tensor would cost a synchronising copy per call
        else:
            axes = [1] * indexes.dim()
            axes[self.channel_axis] = len(self.index_ranges)
            bounds = torch.tensor([s - 1 for s in self.index_ranges], dtype=indexes.dtype,
                                  device=indexes.device).reshape(axes)
        return math_ops.upper_bound(indexes, bounds)

    def _table_indexes(self, indexes):
        """The coder's int32 table indexes: `_normalize_indexes` + `_flatten_indexes` (continuous_indexed.py:272-296),
        as one kernel for a single index range over floating-point indexes."""
        if self.channel_axis is None:
            from ..layers import functional
            flat = functional.index_prepare(indexes, self.index_ranges[0])
            if flat is not None:
                return flat
        return self._flatten_indexes(self._normalize_indexes(indexes)).contiguous()

    def _flatten_indexes(self, indexes):
        indexes = indexes.to(torch.int32)
        if self.channel_axis is None:
            return indexes
        strides = np.cumprod((self.index_ranges + (1,))[::-1])[::-1][1:]
        strides = torch.tensor(strides.copy(), dtype=torch.int32, device=indexes.device)
        # elementwise: integer matmul / tensordot has no HIP kernel ("addmm_cuda" not implemented for 'Int')
        return (indexes.movedim(self.channel_axis, -1) * strides).sum(-1, dtype=torch.int32)

    def forward(self, bottleneck, indexes, training=True, noise=None):
        """`noise` (training only): the sample u in [-0.5, 0.5) to perturb with instead of a fresh one, for callers
        that condition other quantities on the same bottleneck + u (the context model of models/mbt2018.py)."""
        bottleneck = torch.as_tensor(bottleneck).to(self.bottleneck_dtype)
        indexes = self._normalize_indexes(torch.as_tensor(indexes))
        if noise is not None:
            if not training:
                raise ValueError("`noise` is the training perturbation; it has no meaning with training=False")
            noise = torch.as_tensor(noise).to(bottleneck.device, bottleneck.dtype)
            if noise.shape != bottleneck.shape:
                raise ValueError(f"`noise` must have the bottleneck's shape {tuple(bottleneck.shape)}, "
                                 f"received {tuple(noise.shape)}")
        ltm = bottleneck_ops.fused_tail_mass(self.laplace_tail_mass)
        fused = training and ltm is not None and bottleneck_ops.fused_noisy_normal_supported(
            self.prior_fn, self.parameter_fns, bottleneck, self.coding_rank)
        if fused:
            idx = indexes.to(self.prior_dtype)
            loc = self.parameter_fns["loc"](idx)
            # the Laplace component of the tail mixture sits at 0 of the UNSHIFTED bottleneck
            # (continuous_base.py:298-334): the kernel, which sees the shifted one, takes it only for loc == 0
            fused = ltm == 0 or not (torch.is_tensor(loc) or loc != 0)
        if fused:
            # NoisyNormal(loc, scale_fn(indexes)): one fused HIP kernel each way (csrc/noisy_normal_bits.hip);
            # the parameter functions stay differentiable tensor ops, their gradients flow through `scale`
            scale = torch.as_tensor(self.parameter_fns["scale"](idx), dtype=self.prior_dtype, device=bottleneck.device)
            shifted = bottleneck - loc if (torch.is_tensor(loc) or loc != 0) else bottleneck
            if noise is None:
                noise = torch.rand_like(bottleneck) - 0.5
            perturbed, bits = bottleneck_ops.noisy_normal_bits(shifted, scale, self.coding_rank, noise,
                                                               expected_grads=self.expected_grads,
                                                               laplace_tail_mass=ltm)
            if torch.is_tensor(loc) or loc != 0:
                perturbed = perturbed + loc
            return perturbed, bits
        if training:
            def log_prob_fn(perturbed, idx):
                return self._log_prob(self._make_prior(idx), perturbed)
            log_probs, perturbed = math_ops.perturb_and_apply(
                log_prob_fn, bottleneck, indexes, u=noise, expected_grads=self.expected_grads)
        else:
            prior = self._make_prior(indexes)
            perturbed = self.quantize(bottleneck)
            log_probs = self._log_prob(prior, perturbed)
        axes = tuple(range(-self.coding_rank, 0))
        # coding_rank 0: nothing to reduce (torch's sum over an empty dim tuple reduces EVERYTHING)
        bits = (log_probs.sum(dim=axes) if axes else log_probs) / (-float(np.log(2.0)))
        return perturbed, bits

    def quantize(self, bottleneck):
        return round_ops.round_st(torch.as_tensor(bottleneck).to(self.bottleneck_dtype))

    def _device_offsets(self, device):
        """cdf_offset on the device, uploaded once per table version (a pageable H->D copy in every call
        would put a host synchronisation into the coding path)."""
        key = (self.cdf_offset.data_ptr(), getattr(self.cdf_offset, "_version", 0), str(device))
        cache = getattr(self, "_dev_offsets", None)
        if cache is None or cache[0] != key:
            object.__setattr__(self, "_dev_offsets", (key, self.cdf_offset.to(device).contiguous()))
            cache = self._dev_offsets
        return cache[1]

    def _flats(self, indexes):
        device = _lib.require_device()
        return [self._table_indexes(torch.as_tensor(i).to(device)) for i in indexes]

    def _batches(self, bottlenecks, indexes):
        """compress() inputs on the device -> (contiguous batches of one shape, their table indexes, the shape of their
        handles)."""
        self._check_compression()
        device = _lib.require_device()
        bottlenecks = [torch.as_tensor(b).to(device, self.bottleneck_dtype).contiguous() for b in bottlenecks]
        flats = self._flats(indexes)
        if not bottlenecks:
            return [], [], None
        if len(flats) != len(bottlenecks):
            raise ValueError("compress_many: one index tensor per bottleneck")
        shape = tuple(flats[0].shape)
        if any(tuple(f.shape) != shape for f in flats) or any(b.shape != bottlenecks[0].shape for b in bottlenecks):
            raise ValueError("compress_many: all batches must have the same shape")
        return bottlenecks, flats, shape[:len(shape) - self.coding_rank] if self.coding_rank else shape

    def _encode(self, handles, bottlenecks, flats):
        """continuous_indexed.py:374-386 for one batch per handle, ONE coder launch per stage for all of them -> the
        handles, not finalized."""
        cdf_offset = self._device_offsets(handles[0].device)
        if self.fused and bottlenecks[0].dtype in _DTYPE_CODE:
            gen_ops.encode_values(handles, bottlenecks, cdf_offset, indexes=flats)
        else:
            symbols = [(torch.round(b).to(torch.int32) - cdf_offset[f.long()]).contiguous()
                       for b, f in zip(bottlenecks, flats)]
            gen_ops.encode_symbols(handles, symbols, flats)
        for h, b, f in zip(handles, bottlenecks, flats):
            h.coder_inputs = (b, f)              # what the coder read (values, table indexes): for checkers
        return handles

    def _decode(self, decoders, flats):
        """continuous_indexed.py:405-417 for a list of decoders, ONE coder launch per stage for all of them -> values
        per decoder, shaped like its table indexes."""
        shape = tuple(flats[0].shape)
        decode_shape = shape[len(shape) - self.coding_rank:] if self.coding_rank else ()
        cdf_offset = self._device_offsets(decoders[0].device)
        if self.fused and self.bottleneck_dtype in _DTYPE_CODE:
            return gen_ops.decode_values(decoders, decode_shape, self.bottleneck_dtype, cdf_offset, indexes=flats)
        _, symbols = gen_ops.decode_symbols(decoders, decode_shape, flats)
        return [(sym + cdf_offset[f.long()]).to(self.bottleneck_dtype) for sym, f in zip(symbols, flats)]

    def compress(self, bottleneck, indexes, device_result=False):
        """continuous_indexed.py:355-386.  `device_result=True`: see
        `ContinuousBatchedEntropyModel.compress` (nothing read back, returns the finalized handle)."""
        bottlenecks, flats, batch_shape = self._batches([bottleneck], [indexes])
        if self.coder == "ans":
            if device_result:
                self._range_only("compress(device_result=True)")
            cdf_offset = self._device_offsets(bottlenecks[0].device)
            symbols = (torch.round(bottlenecks[0]).to(torch.int32) - cdf_offset[flats[0].long()]).contiguous()
            return self._ans_compressed(symbols, flats[0], batch_shape)
        handle = gen_ops.create_range_encoder(batch_shape, self.cdf, deferred_errors=device_result)
        return self._compressed(self._encode([handle], bottlenecks, flats)[0], device_result)

    def decompress(self, strings, indexes, defer_sanity=False):
        """continuous_indexed.py:388-417.  `strings` may be a handle from `compress(device_result=True)`;
        `defer_sanity=True` returns (values, ok) without reading anything back (see
        `ContinuousBatchedEntropyModel.decompress`)."""
        self._check_compression()
        flats = self._flats([indexes])
        if self.coder == "ans":
            if defer_sanity:
                self._range_only("decompress(defer_sanity=True)")
            shape = tuple(flats[0].shape)
            decode_shape = shape[len(shape) - self.coding_rank:] if self.coding_rank else ()
            symbols, _ = self._ans_decompressed(strings, int(torch.Size(decode_shape).numel()), flats[0])
            cdf_offset = self._device_offsets(symbols.device)
            return (symbols.reshape(shape) + cdf_offset[flats[0].long()]).to(self.bottleneck_dtype)
        decoder = gen_ops.create_range_decoder(strings, self.cdf)
        return self._decompressed(decoder, self._decode([decoder], flats)[0], defer_sanity)

    def compress_many(self, bottlenecks, indexes):
        """compress() of several independent batches (same shapes) with ONE coder launch per stage
        (tfc_encoder_encode_quantized_indexed_many: the pipelined lane kernels quantise and look the tables up in
        their parallel expansion pass; the serial chain of all batches' streams is one small grid).  Nothing is read
        back: one finalized encoder handle per batch (`gen_ops.fetch_strings`, `decompress_many`); same strings as
        compress() batch by batch.  `indexes`: one tensor per batch (continuous_indexed.py:355-386)."""
        self._range_only("compress_many")
        bottlenecks, flats, batch_shape = self._batches(bottlenecks, indexes)
        if not bottlenecks:
            return []
        handles = gen_ops.create_range_encoders(len(bottlenecks), batch_shape, self.cdf, mode="throughput",
                                                deferred_errors=True)
        return gen_ops.entropy_encode_finalize_device_many(self._encode(handles, bottlenecks, flats))

    def decompress_many(self, handles, indexes):
        """decompress() for the handles of compress_many: one decoder launch per stage for all of them; returns
        ([values per batch], ok) with `ok` the device-resident EntropyDecodeFinalize flags — nothing is read back."""
        self._check_compression()
        self._range_only("decompress_many")
        handles = list(handles)
        if not handles:
            return [], None
        flats = self._flats(indexes)
        if len(flats) != len(handles):
            raise ValueError(f"decompress_many: one index tensor per handle ({len(flats)} index tensors, {len(handles)} handles)")
        if any(f.shape != flats[0].shape for f in flats):
            raise ValueError("decompress_many: all index tensors must have the same shape")
        decoders = gen_ops.create_range_decoders(handles, self.cdf, mode="throughput")
        return self._decompressed_many(decoders, self._decode(decoders, flats))

    def get_config(self):
        raise NotImplementedError("Serializing indexed entropy models is not yet implemented.")


class LocationScaleIndexedEntropyModel(ContinuousIndexedEntropyModel):
    """continuous_indexed.py:431-633: `num_scales` scale tables, location handled by
    shifting the bottleneck."""

    def __init__(self, prior_fn, num_scales, scale_fn, coding_rank, compression=False,
                 stateless=False, expected_grads=False, tail_mass=2 ** -8, range_coder_precision=12,
                 bottleneck_dtype=None, prior_dtype=torch.float32, laplace_tail_mass=0, coder="range", ans_lanes=64):
        num_scales = int(num_scales)
        super().__init__(
            prior_fn=prior_fn, index_ranges=(num_scales,),
            parameter_fns=dict(loc=lambda _: 0.0, scale=scale_fn),
            coding_rank=coding_rank, channel_axis=None, compression=compression,
            stateless=stateless, expected_grads=expected_grads, tail_mass=tail_mass,
            range_coder_precision=range_coder_precision, bottleneck_dtype=bottleneck_dtype,
            prior_dtype=prior_dtype, laplace_tail_mass=laplace_tail_mass, coder=coder, ans_lanes=ans_lanes)

    def forward(self, bottleneck, scale_indexes, loc=None, training=True, noise=None):
        if loc is None:
            return super().forward(bottleneck, scale_indexes, training=training, noise=noise)
        perturbed, bits = super().forward(bottleneck - loc, scale_indexes, training=training, noise=noise)
        return perturbed + loc, bits

    def quantize(self, bottleneck, loc=None):
        return round_ops.round_st(torch.as_tensor(bottleneck).to(self.bottleneck_dtype), loc)

    def compress(self, bottleneck, scale_indexes, loc=None, device_result=False):
        if loc is not None:
            bottleneck = bottleneck - loc
        return super().compress(bottleneck, scale_indexes, device_result=device_result)

    def decompress(self, strings, scale_indexes, loc=None, defer_sanity=False):
        values = super().decompress(strings, scale_indexes, defer_sanity=defer_sanity)
        ok = None
        if defer_sanity:
            values, ok = values
        if loc is not None:
            values = values + loc
        return (values, ok) if defer_sanity else values
