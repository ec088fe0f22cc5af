"""CPU tier: `window_attention_reference` (the tensor-op twin of the kernels) against the float64 definition of
tests/window_attention_ref.py, gradients through autograd; the argument errors; the tensor-op twins of layer norm and
GELU; and the shapes of the Swin layers and of the SwinT-ChARM transforms on CPU tensors."""
import numpy as np
import pytest
import torch

import window_attention_ref as ref
from compression_amd import layers
from compression_amd.models import swint2022
from compression_amd.ops import attention_ops as A

CASES = [(4, 16, 1, 1, 0, 1, 1), (4, 16, 3, 2, 2, 5, 7), (8, 32, 1, 2, 4, 21, 10), (8, 16, 2, 1, 0, 16, 24),
         (4, 32, 1, 1, 2, 4, 4), (8, 16, 1, 1, 4, 8, 8), (4, 16, 2, 1, 2, 9, 6), (8, 32, 1, 1, 4, 9, 15)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "ws%d-d%d-h%d-b%d-s%d-%dx%d" % c)
def test_reference_is_the_definition(case):
    ws, d, heads, batch, shift, h, w = case
    gen = torch.Generator().manual_seed(sum(case))
    qkv = torch.randn(batch, h, w, 3 * heads * d, generator=gen, dtype=torch.float64, requires_grad=True)
    table = torch.randn(heads, (2 * ws - 1) ** 2, generator=gen, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(batch, h, w, heads * d, generator=gen, dtype=torch.float64)
    out = A.window_attention(qkv, table, heads, ws, shift)        # a CPU tensor takes the reference
    assert out.dtype == torch.float64 and out.shape == (batch, h, w, heads * d)
    dqkv, dtable = torch.autograd.grad(out, (qkv, table), dout)
    want = ref.forward(qkv, table, heads, ws, shift)
    want_dqkv, want_dtable = ref.backward(qkv, table, dout, heads, ws, shift)
    np.testing.assert_allclose(out.detach().numpy(), want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dqkv.numpy(), want_dqkv, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dtable.numpy(), want_dtable, rtol=0, atol=1e-12)


def test_reference_gives_excluded_keys_weight_zero():
    gen = torch.Generator().manual_seed(3)
    qkv = torch.randn(1, 9, 6, 3 * 16, generator=gen)
    table = torch.randn(1, 49, generator=gen)
    inside = torch.zeros(9, 6, dtype=torch.bool)
    for tokens, _ in ref.windows(9, 6, 4, 2):
        for tk in tokens:
            if tk[2] and tk[3] and not tk[4]:
                inside[tk[0], tk[1]] = True
    assert inside.any() and not inside.all()
    huge, zero = qkv.clone(), qkv.clone()
    huge[:, inside, 32:] = 1e30
    zero[:, inside, 32:] = 0
    a, b = A.window_attention_reference(huge, table, 1, 4, 2), A.window_attention_reference(zero, table, 1, 4, 2)
    assert torch.equal(a[:, ~inside], b[:, ~inside])


def test_argument_errors():
    qkv, table = torch.zeros(1, 8, 8, 48), torch.zeros(1, 225)
    for fn in (A.window_attention, A.window_attention_reference):
        with pytest.raises(ValueError, match=r"\(4, 8\).*\(16, 32\)"):
            fn(qkv, table, 1, 7, 0)
        with pytest.raises(ValueError, match=r"\(4, 8\).*\(16, 32\)"):
            fn(torch.zeros(1, 8, 8, 72), table, 1, 8, 0)            # d = 24
        with pytest.raises(ValueError, match="shift"):
            fn(qkv, table, 1, 8, 3)
        with pytest.raises(ValueError, match="heads"):
            fn(qkv, table, 0, 8, 0)
        with pytest.raises(ValueError, match="table"):
            fn(qkv, torch.zeros(1, 49), 1, 8, 0)
        with pytest.raises(ValueError, match="qkv must be"):
            fn(qkv[0], table, 1, 8, 0)
        with pytest.raises(TypeError):
            fn(qkv.to(torch.float16), table, 1, 8, 0)
    with pytest.raises(ValueError, match=r"\(4, 8\)"):
        layers.WindowAttention(48, 2, 8)                            # d = 24
    with pytest.raises(ValueError, match="shift"):
        layers.WindowAttention(32, 2, 8, 2)


def test_constants_are_read_from_the_header():
    for name in ("WA_FWD_WINDOWS_WS8", "WA_FWD_WINDOWS_WS4", "WA_BWD_WINDOWS_WS8", "WA_BWD_WINDOWS_WS4",
                 "WA_DTABLE_PARTIALS"):
        assert A.WA_CONSTANTS[name] >= 1


def test_layer_norm_and_gelu_twins():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, 33, generator=gen, dtype=torch.float64)
    gamma, beta = torch.randn(33, generator=gen, dtype=torch.float64), torch.randn(33, generator=gen, dtype=torch.float64)
    res = torch.randn(3, 5, 33, generator=gen, dtype=torch.float64)
    want = torch.nn.functional.layer_norm(x, (33,), gamma, beta, 1e-5) + res
    got = A.layer_norm(x, gamma, beta, 1e-5, res)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=0, atol=1e-13)
    assert torch.allclose(A.gelu(x), torch.nn.functional.gelu(x), rtol=0, atol=1e-14)
    assert A.gelu(x.float()).dtype == torch.float32 and A.layer_norm(x.bfloat16(), None, None).dtype == torch.bfloat16


def test_layer_shapes():
    x = torch.randn(2, 7, 10, 32)
    assert layers.LayerNorm(32)(x).shape == x.shape
    assert layers.WindowAttention(32, 2, 4, 2)(x).shape == x.shape
    block = layers.SwinBlock(32, 1, 8, 4)
    y = block(x)
    assert y.shape == x.shape
    y.sum().backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in block.parameters())
    assert layers.PatchMerge(32, 48)(x).shape == (2, 4, 5, 48)       # 7 rows: one zero row added
    assert layers.PatchSplit(32, 16)(x).shape == (2, 14, 20, 16)
    # merge then split puts a pixel back where it was: the two layouts are inverse
    merge, split = layers.PatchMerge(1, 4), layers.PatchSplit(4, 1)
    for layer in (merge, split):
        layer.norm.forward = lambda t, residual=None: t
    torch.nn.init.eye_(merge.reduce.kernel.data[0, 0])
    torch.nn.init.eye_(split.expand.kernel.data[0, 0])
    img = torch.randn(1, 6, 8, 1)
    assert torch.equal(split(merge(img)), img)


def test_model_transform_shapes():
    kw = dict(widths=(32, 32, 64, 64), depths=(1, 1, 2, 1), head_dim=16, num_filters=32, hyper_depths=(1, 1), num_slices=4)
    model = swint2022.SwinTCharmModel(**kw)
    x = torch.rand(2, 72, 104, 3) * 255
    with torch.no_grad():
        y = model.analysis_transform(x)
        z = model.hyper_analysis_transform(y)
        assert y.shape == (2, 8, 8, 64) and z.shape == (2, 2, 2, 32)            # 72 x 104 padded to 128 x 128
        assert model.hyper_synthesis_mean_transform(z).shape == (2, 8, 8, 320)
        assert model.hyper_synthesis_scale_transform(z).shape == (2, 8, 8, 320)
        assert model.synthesis_transform(y).shape == (2, 128, 128, 3)
    assert model.container_dtypes == [np.int32] * 3 + [bytes] * 5
    blocks = [m for m in model.analysis_transform.modules() if isinstance(m, layers.SwinBlock)]
    assert [b.attn.shift for b in blocks] == [0, 0, 0, 4, 0] and len(blocks) == 5
    assert {b.attn.window for b in model.hyper_analysis_transform.modules() if isinstance(b, layers.SwinBlock)} == {4}
    with pytest.raises(ValueError, match="head_dim"):
        swint2022.SwinTCharmModel(widths=(32, 32, 64, 72), head_dim=16)
    full = swint2022.SwinAnalysisTransform()
    assert [m.attn.dim for m in full.modules() if isinstance(m, layers.SwinBlock)] == [128] * 2 + [192] * 2 + [256] * 6 + [320] * 2
