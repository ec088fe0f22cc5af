"""CPU tier: the `coder` / `ans_lanes` options of the entropy models and the two reference image models — what they
accept, that a config and a model file carry them, and that nothing codes without a device."""
import pytest
import torch

import compression_amd as tfc
from compression_amd import distributions, entropy_models
from compression_amd.models import bls2017, bmshj2018, codec_io

TABLE = torch.tensor([-12, 0, 1000, 3000, 4096, -12, 0, 2000, 3500, 4096], dtype=torch.int32)


def batched(**kwargs):
    return entropy_models.ContinuousBatchedEntropyModel(
        prior_shape=(2,), coding_rank=1, compression=True, cdf=TABLE, offset_heuristic=False,
        cdf_offset=torch.tensor([-1, -1], dtype=torch.int32),
        **kwargs)


def indexed(cls, **kwargs):
    if cls is entropy_models.LocationScaleIndexedEntropyModel:
        return cls(distributions.NoisyNormal, 4, lambda i: torch.exp(0.3 * i), coding_rank=1, **kwargs)
    return cls(distributions.NoisyNormal, (4,), dict(loc=lambda _: 0.0, scale=lambda i: torch.exp(0.3 * i)),
               coding_rank=1, channel_axis=None, **kwargs)


def test_unknown_coder_is_refused_everywhere():
    with pytest.raises(ValueError, match="coder"):
        batched(coder="zip")
    for cls in (entropy_models.ContinuousIndexedEntropyModel, entropy_models.LocationScaleIndexedEntropyModel):
        with pytest.raises(ValueError, match="coder"):
            indexed(cls, coder="zip")
        assert indexed(cls, coder="ans", ans_lanes=16).ans_lanes == 16
    for cls in (bls2017.BLS2017Model, bmshj2018.BMSHJ2018Model):
        with pytest.raises(ValueError, match="coder"):
            cls(num_filters=8, coder="zip")
    for lanes in (0, 3, 48, 128):
        with pytest.raises(ValueError, match="ans_lanes"):
            batched(coder="ans", ans_lanes=lanes)
        with pytest.raises(ValueError, match="ans_lanes"):
            bls2017.BLS2017Model(num_filters=8, coder="ans", ans_lanes=lanes)


def test_config_keeps_the_coder():
    em = batched(coder="ans", ans_lanes=8)
    config = em.get_config()
    assert config["coder"] == "ans" and config["ans_lanes"] == 8
    again = entropy_models.ContinuousBatchedEntropyModel.from_config(config)
    assert again.coder == "ans" and again.ans_lanes == 8
    plain = batched().get_config()
    assert plain["coder"] == "range" and plain["ans_lanes"] == 64
    del plain["coder"], plain["ans_lanes"]                  # a config written before the option existed
    old = entropy_models.ContinuousBatchedEntropyModel.from_config(plain)
    assert old.coder == "range" and old.ans_lanes == 64


def test_compress_needs_a_device():
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    em = batched(coder="ans")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        em.compress(torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tfc.ans_encode(TABLE, torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tfc.ans_decode([b""], TABLE, (1, 4))


def test_range_only_calls_name_the_option():
    em = batched(coder="ans")
    for call in (lambda: em.compress_many([torch.zeros(3, 2)]), lambda: em.decompress_many([], (3,))):
        with pytest.raises(NotImplementedError, match='coder="ans"'):
            call()


def test_the_choice_is_stored_with_the_model():
    for cls in (bls2017.BLS2017Model, bmshj2018.BMSHJ2018Model):
        _the_choice_is_stored_with_the_model(cls)


def _the_choice_is_stored_with_the_model(cls):
    model = cls(num_filters=8, coder="ans", ans_lanes=32)
    state = model.state_dict()
    assert int(state["_ans_lanes"]) == 32
    plain = cls(num_filters=8)
    assert plain.coder == "range" and "_ans_lanes" not in plain.state_dict()
    # a state_dict without the key is a file written before the option existed, or by a "range" model
    codec_io.set_model_coder(plain, "ans", 4)
    assert plain.coder == "ans" and int(plain.state_dict()["_ans_lanes"]) == 4
    codec_io.set_model_coder(plain, "range")
    assert plain.coder == "range" and "_ans_lanes" not in plain.state_dict()
    assert set(plain.state_dict()) == set(state) - {"_ans_lanes"}


def test_train_has_the_flag():
    import argparse
    ap = argparse.ArgumentParser()
    codec_io._add_train_parser(ap.add_subparsers(dest="command"), bls2017.BLS2017Model)
    args = ap.parse_args(["train", "--coder", "ans", "--ans_lanes", "16"])
    assert args.coder == "ans" and args.ans_lanes == 16
    assert ap.parse_args(["train"]).coder == "range"


def test_abi_refuses_bad_scalars_on_the_host():
    from compression_amd import _lib
    lib = _lib.lib()
    assert lib.tfc_ans_blob_capacity(1, 10, 48) == -1 and "lanes" in _lib.last_error()
    assert lib.tfc_ans_blob_capacity(-1, 10, 64) == -1 and "streams" in _lib.last_error()
    assert lib.tfc_ans_blob_capacity(3, 10, 4) == 3 * (80 + 16)
    assert lib.tfc_ans_blob_capacity(3, 2, 64) == 3 * (16 + 8)
    rc = lib.tfc_ans_encode(None, None, None, 1, 10, 3, None, None, None, None, None)
    assert rc != 0 and "lanes" in _lib.last_error()
    rc = lib.tfc_ans_encode(None, None, None, 1, 1 << 40, 64, None, None, None, None, None)
    assert rc != 0 and "elems" in _lib.last_error()
    rc = lib.tfc_ans_encode(None, None, None, 1, 10, 64, None, None, None, None, None)
    assert rc != 0 and "null tables" in _lib.last_error()
    rc = lib.tfc_ans_decode(None, None, None, None, -1, None, 1, 10, 64, None, None, None)
    assert rc != 0 and ("null tables" in _lib.last_error() or "nstrings" in _lib.last_error())
