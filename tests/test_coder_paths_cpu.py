"""CPU tier: what the entropy models hand the coder, seen through a recording stand-in for the library.

compress() / compress_many() and decompress() / decompress_many() are one coding routine per model and direction
(ops/gen_ops.py encode_symbols / encode_values / decode_symbols / decode_values under them).  What must hold: one batch
reaches the same C entry with the same scalar arguments whichever public method it came through; the tensors the
kernels read or write are on the owning handle's `_keep`, each once, and a deferred handle has one replay closure that
issues the same call again; the reference's shape errors are raised on every route.  A mistake in the lifetime lists
is a use-after-free a GPU run may not show, so they are checked here, where nothing runs."""
import ctypes

import pytest
import torch

import compression_amd as tfc
from compression_amd import _lib
from compression_amd.entropy_models import continuous_base
from compression_amd.ops import gen_ops

CHANNELS, SCALES = 4, 8


class RecordingLib:
    """Every `tfc_*` entry returns 0 and is recorded as (name, its integer arguments): the pointers are left out."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name][1]

        def entry(*args):
            assert len(args) == len(argtypes), name
            self.calls.append((name, tuple(a for a, t in zip(args, argtypes) if t in (ctypes.c_int, ctypes.c_int64))))
            return 0
        return entry

    def coding(self, *prefixes):
        """The recorded calls of the entries named so, since the last look."""
        out = [c for c in self.calls if c[0].startswith(prefixes)]
        self.calls.clear()
        return out


@pytest.fixture
def lib(monkeypatch):
    rec = RecordingLib()
    monkeypatch.setattr(_lib, "require_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    # (the indexed model builds its tables with a kernel: any table will do here)
    monkeypatch.setattr(continuous_base.ContinuousEntropyModelBase, "_build_tables",
                        lambda self, prior, precision, offset=None: (torch.zeros(6 * SCALES, dtype=torch.int32),
                                                                     torch.full((SCALES,), -2, dtype=torch.int32)))
    yield rec
    gen_ops.invalidate_table_cache()


def _model(which, fused, batch=2):
    """(entropy model, compress() arguments for a [batch, 3, CHANNELS] latent, argument that sizes decompress())."""
    torch.manual_seed(0)
    y = torch.randn(batch, 3, CHANNELS) * 4
    if which == "batched":
        em = tfc.ContinuousBatchedEntropyModel(
            prior_shape=(CHANNELS,), coding_rank=2, compression=True, cdf=torch.zeros(6 * CHANNELS, dtype=torch.int32),
            cdf_offset=torch.full((CHANNELS,), -2, dtype=torch.int32),
            quantization_offset=torch.linspace(-0.4, 0.4, CHANNELS), bottleneck_dtype=torch.float32)
        args, sizes = (y,), (3,)
    else:
        em = tfc.LocationScaleIndexedEntropyModel(
            tfc.NoisyNormal, num_scales=SCALES, scale_fn=lambda i: torch.exp(0.3 * i), coding_rank=2, compression=True,
            bottleneck_dtype=torch.float32)
        sizes = torch.randint(0, SCALES, y.shape).float()
        args = (y, sizes)
    em.fused = fused
    return em, args, sizes


def _many(args):
    return [[a] for a in args]


def _roles(em, keep, values):
    """The kept objects by what they are to the coder, by identity; every object is kept once."""
    assert len({id(t) for t in keep}) == len(keep)
    tables = em._device_tables(torch.device("cpu")) if hasattr(em, "_device_tables") else (em._device_offsets("cpu"),)
    names = {id(values): "values", id(tables[0]): "cdf_offset"}
    if len(tables) > 1:
        names[id(tables[1])] = "qoffset"
    out = []
    for t in keep:
        if id(t) in names:
            out.append(names[id(t)])
        elif isinstance(t, gen_ops.EncoderHandle):
            out.append("encoder")
        else:
            assert t.dtype == torch.int32
            out.append("int32")             # symbols or table indexes, made per call
    return sorted(out)


ENTRY = {("batched", True): ("tfc_encoder_encode_quantized_many", (1, 0, CHANNELS, 3 * CHANNELS)),
         ("indexed", True): ("tfc_encoder_encode_quantized_indexed_many", (1, 0, 3 * CHANNELS)),
         ("batched", False): ("tfc_encoder_encode_many", (1, 3 * CHANNELS)),
         ("indexed", False): ("tfc_encoder_encode_many", (1, 3 * CHANNELS))}
KEPT = {("batched", True): ["cdf_offset", "qoffset", "values"], ("indexed", True): ["cdf_offset", "int32", "values"],
        ("batched", False): ["int32"], ("indexed", False): ["int32", "int32"]}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["batched", "indexed"])
def test_one_batch_is_coded_the_same_way_through_compress_and_compress_many(lib, which, fused):
    em, args, _ = _model(which, fused)
    lib.calls.clear()
    single = em.compress(*args, device_result=True)
    single_calls = lib.coding("tfc_encoder_encode")
    many, = em.compress_many(*_many(args))
    many_calls = lib.coding("tfc_encoder_encode")
    # n = 1, the dtype code of float32, the channel count (channel mode) and the elements per stream
    assert single_calls == many_calls == [ENTRY[which, fused]]
    for h in (single, many):
        assert h.coder_inputs[0] is args[0] and (h.coder_inputs[1] is None) == (which == "batched")
        assert _roles(em, h._keep, args[0]) == KEPT[which, fused]
        if which == "indexed":
            assert any(t is h.coder_inputs[1] for t in h._keep)
        # one replay closure, which issues the same call on another handle and keeps the same tensors alive on it
        assert len(h._replay) == 1
        fresh = gen_ops.EncoderHandle(h.shape, h.tables, h.device)
        lib.calls.clear()
        h._replay[0](fresh)
        assert lib.coding("tfc_encoder_encode") == single_calls and fresh._replay == []
        assert [id(t) for t in fresh._keep] == [id(t) for t in h._keep]
    # the plain call codes the same way on a handle that keeps no replay closure
    em.compress(*args)
    assert lib.coding("tfc_encoder_encode") == single_calls


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["batched", "indexed"])
def test_one_batch_is_decoded_the_same_way_through_decompress_and_decompress_many(lib, which, fused):
    em, args, sizes = _model(which, fused)
    handle = em.compress(*args, device_result=True)
    lib.calls.clear()
    out, ok = em.decompress(handle, sizes, defer_sanity=True)
    single_calls = lib.coding("tfc_decoder_decode")
    outs, oks = em.decompress_many([handle], [sizes] if which == "indexed" else sizes)
    many_calls = lib.coding("tfc_decoder_decode")
    assert single_calls == many_calls and len(single_calls) == 1
    name, scalars = single_calls[0]
    if not fused:
        assert (name, scalars) == ("tfc_decoder_decode_many", (1, 3 * CHANNELS))
    elif which == "batched":
        assert (name, scalars) == ("tfc_decoder_decode_dequantized_many", (1, 0, CHANNELS, 3 * CHANNELS))
    else:
        assert (name, scalars) == ("tfc_decoder_decode_dequantized_indexed_many", (1, 0, 3 * CHANNELS))
    assert out.shape == outs[0].shape == args[0].shape and out.dtype == outs[0].dtype == torch.float32
    want = ["encoder"] + ((["cdf_offset", "qoffset", "values"] if which == "batched" else ["cdf_offset", "int32", "values"])
                          if fused else ["int32"] * (which == "indexed"))
    assert _roles(em, ok._tfc_handle._keep, out) == sorted(want)
    assert _roles(em, oks._tfc_handle[0]._keep, outs[0]) == sorted(want)
    assert ok._tfc_handle._keep[0] is handle and oks._tfc_handle[0]._keep[0] is handle


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["batched", "indexed"])
def test_an_empty_handle_is_refused_on_every_route(lib, which, fused):
    em, args, sizes = _model(which, fused, batch=0)
    for call in (lambda: em.compress(*args), lambda: em.compress(*args, device_result=True),
                 lambda: em.compress_many(*_many(args))):
        with pytest.raises(ValueError, match="`handle` is empty"):
            call()
    assert lib.coding("tfc_encoder_encode") == []
    empty, = gen_ops.create_range_encoders(1, (0,), em.cdf)
    with pytest.raises(ValueError, match="`handle` is empty"):
        em.decompress(empty, sizes)
    with pytest.raises(ValueError, match="`handle` is empty"):
        em.decompress_many([empty], [sizes] if which == "indexed" else sizes)
    assert lib.coding("tfc_decoder_decode") == []


@pytest.mark.parametrize("fused", [True, False])
def test_indexes_that_do_not_fit_the_handle_are_refused_on_every_route(lib, fused):
    em, args, _ = _model("indexed", fused)
    handle = em.compress(*args, device_result=True)
    wrong = torch.zeros(3, 3, CHANNELS)
    lib.calls.clear()
    with pytest.raises(ValueError, match="'index' shape should match 'handle' shape \\+ 'shape'"):
        em.decompress(handle, wrong)
    with pytest.raises(ValueError, match="'index' shape should match 'handle' shape \\+ 'shape'"):
        em.decompress_many([handle], [wrong])
    assert lib.coding("tfc_decoder_decode") == []
    # a latent and indexes of different shapes: nothing may reach a kernel that reads one by the other's extent
    with pytest.raises((ValueError, RuntimeError)):
        em.compress(args[0], wrong)
    with pytest.raises((ValueError, RuntimeError)):
        em.compress_many([args[0]], [wrong])
    assert lib.coding("tfc_encoder_encode") == []


def test_the_ops_raise_the_reference_texts_singly_and_in_lists(lib):
    lookup = torch.zeros(12, dtype=torch.int32)
    value = torch.zeros(2, 5, dtype=torch.int32)
    floats, offsets = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32)

    def handle(shape=(2,)):
        return gen_ops.create_range_encoder(shape, lookup)

    for call in (lambda: tfc.entropy_encode_channel(handle((3,)), value),
                 lambda: tfc.entropy_encode_channel_many([handle(), handle((3,))], [value, value]),
                 lambda: tfc.entropy_encode_index(handle((3,)), value, value),
                 lambda: gen_ops.encode_values([handle((3,))], [floats], offsets, channels=1),
                 lambda: gen_ops.encode_values([handle((3,))], [floats], offsets, indexes=[value])):
        with pytest.raises(ValueError, match="'value' shape should start with 'handle' shape"):
            call()
    for call in (lambda: tfc.entropy_encode_index(handle(), value[:, :4], value),
                 lambda: gen_ops.encode_symbols([handle(), handle()], [value, value], [value, value[:, :4]]),
                 lambda: gen_ops.encode_values([handle()], [floats], offsets, indexes=[value[:, :4]])):
        with pytest.raises(ValueError, match="'index' shape should match 'value' shape"):
            call()
    for call in (lambda: tfc.entropy_encode_channel(handle((0,)), value[:0]),
                 lambda: tfc.entropy_encode_index(handle((0,)), value[:0], value[:0]),
                 lambda: tfc.entropy_encode_channel_many([handle((0,))], [value[:0]])):
        with pytest.raises(ValueError, match="`handle` is empty"):
            call()
    with pytest.raises(TypeError, match="expected int32"):
        tfc.entropy_encode_channel(handle(), floats)
    with pytest.raises(ValueError, match="same shape"):
        tfc.entropy_encode_channel_many([handle(), handle()], [value, value[:, :4]])
    decoder = gen_ops.create_range_decoder(handle(), lookup)
    for call in (lambda: tfc.entropy_decode_index(decoder, value, [4]),
                 lambda: gen_ops.decode_symbols([decoder], [4], [value]),
                 lambda: gen_ops.decode_values([decoder], [4], torch.float32, offsets, indexes=[value])):
        with pytest.raises(ValueError, match="'index' shape should match 'handle' shape \\+ 'shape'"):
            call()
    with pytest.raises(TypeError, match="Tdecoded must be int32"):
        tfc.entropy_decode_channel(decoder, [5], torch.int64)
    assert lib.coding("tfc_encoder_encode", "tfc_decoder_decode") == []
    # and what passes the checks is one call of the list entry
    _, out = tfc.entropy_decode_index(decoder, value, [5])
    assert out.shape == (2, 5) and out.dtype == torch.int32 and decoder._keep[-1] is value
    assert lib.coding("tfc_decoder_decode") == [("tfc_decoder_decode_many", (1, 5))]
