"""CPU tier: what the layers promise besides their arithmetic: parameter names and shapes (saved models, bench.py and
tools/ address them by name), and copies / pickles that leave the cached device values behind."""
import copy
import pickle

import pytest
import torch

import keras_conv_emulation


def _names_and_shapes(module):
    return sorted((k, tuple(v.shape)) for k, v in module.state_dict().items())


def test_parameter_names_and_shapes():
    from compression_amd import layers as L
    assert _names_and_shapes(L.SignalConv1D(4, 5, use_bias=True, in_channels=3)) == [
        ("bias", (4,)), ("kernel_imag", (3, 4, 3)), ("kernel_real", (3, 4, 3))]
    assert _names_and_shapes(L.SignalConv1D(4, 5, use_bias=True, kernel_parameter="variable", in_channels=3)) == [
        ("bias", (4,)), ("kernel_variable", (5, 3, 4))]
    assert _names_and_shapes(L.SignalConv2D(4, (5, 4), use_bias=True, in_channels=3)) == [
        ("bias", (4,)), ("kernel_imag", (3, 4, 5, 3)), ("kernel_real", (3, 4, 5, 3))]
    assert _names_and_shapes(L.SignalConv2D(4, (5, 4), use_bias=True, kernel_parameter="variable", in_channels=3)) == [
        ("bias", (4,)), ("kernel_variable", (5, 4, 3, 4))]
    assert _names_and_shapes(L.SignalConv3D(4, (3, 4, 5), use_bias=True, in_channels=2)) == [
        ("bias", (4,)), ("kernel_imag", (2, 4, 3, 4, 3)), ("kernel_real", (2, 4, 3, 4, 3))]
    assert _names_and_shapes(L.SignalConv3D(4, (3, 4, 5), use_bias=True, kernel_parameter="variable", in_channels=2)) == [
        ("bias", (4,)), ("kernel_variable", (3, 4, 5, 2, 4))]
    assert _names_and_shapes(L.KerasConv2D(6, 3, 2, in_channels=5)) == [("bias", (6,)), ("kernel", (3, 3, 5, 6))]
    assert _names_and_shapes(L.KerasConv2DTranspose(6, 3, 2, in_channels=5)) == [
        ("bias", (6,)), ("kernel", (3, 3, 6, 5))]
    assert _names_and_shapes(L.GDN(num_channels=8)) == [("reparam_beta", (8,)), ("reparam_gamma", (8, 8))]
    assert _names_and_shapes(L.GDN(num_channels=8, alpha_parameter=None, epsilon_parameter=None)) == [
        ("reparam_alpha", ()), ("reparam_beta", (8,)), ("reparam_epsilon", ()), ("reparam_gamma", (8, 8))]
    # (the switches tools/ sets on the class)
    assert isinstance(L.SignalConv2D.fuse_gdn_image, bool) and isinstance(L.SignalConv2D.keyed_weights, bool)


def _layers_that_have_run(monkeypatch):
    """(layer, the cache attributes it may keep): each called once under no_grad on CPU tensors, kernels emulated."""
    from compression_amd import layers as L
    from compression_amd.layers import functional
    keras_conv_emulation.install(monkeypatch)

    def gdn_forward(x, beta, gamma, inverse=False, rectify=False, alpha=1, epsilon=1, prepared=None):
        norm = (x.abs() ** alpha @ gamma + beta) ** epsilon
        return x * norm if inverse else x / norm
    monkeypatch.setattr(functional, "gdn_forward", gdn_forward)
    torch.manual_seed(0)
    conv = L.SignalConv2D(16, 5, corr=True, strides_down=2, padding="same_zeros", use_bias=True)
    keras = L.KerasConv2D(6, 3, 2)
    gdn = L.GDN()
    with torch.no_grad():
        conv(torch.randn(1, 8, 8, 3))
        keras(torch.randn(1, 8, 8, 4))
        gdn(torch.randn(1, 4, 4, 8))
    assert "_kernel_cache" in conv.__dict__ and gdn.__dict__["_value_cache"]
    # (on the device the Keras layer keeps its padded weights and the convolution its weights key: stand-ins here,
    # with key 0 = nothing to release)
    keras.__dict__["_padded_cache"] = (("stand-in",), keras.kernel.detach(), keras.bias.detach(), 0)
    return ((conv, ("_kernel_cache", "_wkey_cache")), (keras, ("_padded_cache",)), (gdn, ("_value_cache",)))


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_copies_leave_the_caches_behind(monkeypatch, how):
    for layer, caches in _layers_that_have_run(monkeypatch):
        twin = copy.deepcopy(layer) if how == "deepcopy" else pickle.loads(pickle.dumps(layer))
        assert type(twin) is type(layer)
        for name in caches:
            assert name not in twin.__dict__, (type(layer).__name__, name)
        assert any(name in layer.__dict__ for name in caches)          # the original keeps its own
        ours, theirs = layer.state_dict(), twin.state_dict()
        assert list(ours) == list(theirs) and len(ours) >= 2
        for name in ours:
            assert torch.equal(ours[name], theirs[name]) and ours[name].data_ptr() != theirs[name].data_ptr()
        assert twin.training == layer.training


def test_a_copy_rebuilds_its_cache_on_first_use(monkeypatch):
    (conv, _), _, (gdn, _) = _layers_that_have_run(monkeypatch)
    twin = copy.deepcopy(conv)
    with torch.no_grad():
        assert torch.equal(twin.kernel, conv.kernel) and twin.kernel.data_ptr() != conv.kernel.data_ptr()
        assert "_kernel_cache" in twin.__dict__
        twin_gdn = copy.deepcopy(gdn)
        assert torch.equal(twin_gdn.beta, gdn.beta) and twin_gdn.__dict__["_value_cache"]
