"""GPU tier: the layer-norm and GELU kernels, a Swin block and a tiny SwinT-ChARM model.

layer_norm / gelu: forward and backward against their float64 evaluation under the comparative bar of
test_window_attention_gpu.py (relative L2; float32: <= 2 x the float32 tensor-op twin on the CPU + 1e-6; bfloat16:
<= 2 x the bfloat16 composition + 2^-9; both errors printed).  C takes 2, 31, 32, 33, 320 and the longest row of the
vector kernel +- 1 (csrc/channel_norm.hip, cnorm_plan: 512 float32 / 256 bfloat16 granules = 2048 channels), over an
odd number of rows so that the paired-row path has a last row left over.

SwinBlock: gradients on the device against the block's own CPU float64 evaluation.  Its four linear layers are the MFMA
convolutions, whose float32 gradient bar is 1e-4 max(1, max |want|) (test_keras_conv_gpu.py:61); four of them in a
chain: 4e-4 max(1, max |want|).

SwinTCharmModel (widths 32, 32, 64, 64; depths 1, 1, 2, 1; two images of 72 x 104): decompress(compress(x)) is the
evaluation-mode reconstruction bit for bit, and an image compressed in the batch decompresses alone to the same bytes."""
import pytest
import torch

import compression_amd as tfc
from compression_amd import layers, synthetic
from compression_amd.ops import attention_ops as A

pytestmark = pytest.mark.gpu

VEC_MAX_C = 2048
CHANNELS = [2, 31, 32, 33, 320, VEC_MAX_C - 1, VEC_MAX_C, VEC_MAX_C + 1]
DTYPES = [torch.float32, torch.bfloat16]
ROWS = (3, 13)          # 39 rows


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    den = b.norm().item()
    return (a - b).norm().item() / den if den else (a - b).norm().item()


def compare(names, got, base, want, dtype):
    slack = 1e-6 if dtype == torch.float32 else 2.0 ** -9
    bad = []
    for name, g, b, t in zip(names, got, base, want):
        e_kernel, e_base = rel_l2(g, t), rel_l2(b, t)
        print(f"{name}: kernel {e_kernel:.3e}  composition {e_base:.3e}")
        if not e_kernel <= 2 * e_base + slack:
            bad.append((name, e_kernel, e_base))
    assert not bad, bad


def bf16_layer_norm(x, gamma, beta, eps, residual):
    """The composition in the dtype of x, every intermediate rounded to it."""
    mean = x.mean(dim=-1, keepdim=True)
    cen = x - mean
    y = cen * torch.rsqrt((cen * cen).mean(dim=-1, keepdim=True) + eps) * gamma.to(x.dtype) + beta.to(x.dtype)
    return y if residual is None else y + residual


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("c", CHANNELS)
def test_layer_norm(c, with_residual, dtype):
    gen = torch.Generator().manual_seed(c)
    x = (torch.randn(ROWS + (c,), generator=gen) * 2 + 0.5).bfloat16().float()
    res = torch.randn(ROWS + (c,), generator=gen).bfloat16().float() if with_residual else None
    gamma, beta = torch.randn(c, generator=gen) + 1, torch.randn(c, generator=gen)
    g = torch.randn(ROWS + (c,), generator=gen).bfloat16().float()
    eps = 1e-5

    def evaluate(fn, device, dt):
        xs = x.to(device, dt).requires_grad_(True)
        gm, bt = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
        if dt == torch.float64:
            gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rs = None if res is None else res.to(device, dt).requires_grad_(True)
        y = fn(xs, gm, bt, eps, rs)
        assert y.dtype == dt and y.shape == x.shape
        grads = torch.autograd.grad(y, (xs, gm, bt) + (() if rs is None else (rs,)), g.to(device, dt))
        return (y.detach(),) + grads

    want = evaluate(A.layer_norm_reference, "cpu", torch.float64)
    base = evaluate(A.layer_norm_reference if dtype == torch.float32 else bf16_layer_norm, "cpu", dtype)
    got = evaluate(A.layer_norm, "cuda", dtype)
    names = ("y", "dx", "dgamma", "dbeta") + (("dresidual",) if with_residual else ())
    compare(names, got, base, want, dtype)
    # deterministic parameter gradients
    again = evaluate(A.layer_norm, "cuda", dtype)
    assert torch.equal(got[2], again[2]) and torch.equal(got[3], again[3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 4 * 1024 + 3, 300001])
def test_gelu(n, dtype):
    gen = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=gen) * 3).bfloat16().float()
    g = torch.randn(n, generator=gen).bfloat16().float()

    def evaluate(fn, device, dt):
        xs = x.to(device, dt).requires_grad_(True)
        y = fn(xs)
        assert y.dtype == dt and y.shape == x.shape
        return y.detach(), torch.autograd.grad(y, xs, g.to(device, dt))[0]

    def bf16_gelu(t):
        return 0.5 * t * (1.0 + torch.erf(t * (2.0 ** -0.5)))

    want = evaluate(A.gelu_reference, "cpu", torch.float64)
    base = evaluate(A.gelu_reference if dtype == torch.float32 else bf16_gelu, "cpu", dtype)
    got = evaluate(A.gelu, "cuda", dtype)
    compare(("y", "dx"), got, base, want, dtype)


def test_gelu_takes_unaligned_views():
    x = torch.randn(1027, device="cuda")[1:]                  # 4 bytes past a 16-byte boundary
    assert torch.allclose(A.gelu(x), torch.nn.functional.gelu(x), rtol=0, atol=1e-6)


@pytest.mark.parametrize("window,shift,heads", [(4, 2, 2), (8, 4, 1), (8, 0, 2)])
def test_swin_block_gradients(window, shift, heads):
    torch.manual_seed(window + shift)
    dim = 32
    block = layers.SwinBlock(dim, heads, window, shift)
    with torch.no_grad():
        for p in block.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
        block.attn.table.normal_()
    x = torch.randn(2, 11, 13, dim)
    g = torch.randn(2, 11, 13, dim)

    def evaluate(module, xs, gs):
        xs = xs.requires_grad_(True)
        y = module(xs)
        params = list(module.parameters())
        return [y.detach()] + list(torch.autograd.grad(y, [xs] + params, gs))

    import copy
    want = evaluate(copy.deepcopy(block).double(), x.double(), g.double())
    got = evaluate(block.cuda(), x.cuda(), g.cuda())
    names = ["y", "dx"] + [n for n, _ in block.named_parameters()]
    bad = []
    for name, a, b in zip(names, got, want):
        err = (a.double().cpu() - b).abs().max().item()
        bound = 4e-4 * max(1.0, b.abs().max().item())
        print(f"{name}: {err:.3e} of {bound:.3e}")
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad


def test_tiny_swint_charm_round_trip():
    torch.manual_seed(4)
    model = tfc.models.SwinTCharmModel(num_filters=32, widths=(32, 32, 64, 64), depths=(1, 1, 2, 1), head_dim=16,
                                       hyper_depths=(1, 1), num_slices=4, max_support_slices=2)
    model = model.cuda().init_compression()
    x = torch.from_numpy(synthetic.lowpass_images(2, 72, 104, seed=5)).cuda()
    out = model.compress(x)
    x_shape, y_shape, z_shape = out[:3]
    assert x_shape == (72, 104) and y_shape == (8, 8) and z_shape == (2, 2)         # padded to 128 x 128
    assert len(out) == 4 + 4 and all(s.shape == (2,) for s in out[3:])
    x_hat = model.decompress(*out)
    assert x_hat.shape == (2, 72, 104, 3) and x_hat.dtype == torch.uint8
    # the evaluation-mode reconstruction: quantised slices with the same parameters
    with torch.no_grad():
        y = model.analysis_transform(x.float())
        z = model.hyper_analysis_transform(y)
        z_hat = model.em_z.quantize(z)
        ls, lm = model._hyper_features(z_hat, y_shape)
        slices = []
        for k, ys in enumerate(torch.chunk(y, 4, dim=-1)):
            ms, mu, sigma = model._slice_params(k, lm, ls, slices, y_shape)
            slices.append(model._lrp(k, ms, model.em_y.quantize(ys, loc=mu)))
        ref = model.synthesis_transform(torch.cat(slices, dim=-1))[:, :72, :104, :]
        ref = torch.clamp(torch.round(ref), 0, 255).to(torch.uint8)
    assert torch.equal(x_hat, ref)
    # image 1 compressed in the batch decompresses alone to the same bytes, and compresses alone to the same strings
    alone = model.decompress(*out[:3], *[s[1:2] for s in out[3:]])
    assert torch.equal(alone[0], x_hat[1])
    single = model.compress(x[1:2])
    assert all(bytes(a[0]) == bytes(b[1]) for a, b in zip(single[3:], out[3:]))
    # and the model trains: one step reaches every parameter of the new transforms
    loss, bpp, mse = model(x, training=True)
    loss.backward()
    assert torch.isfinite(loss) and bpp > 0
    new = ("analysis_transform", "synthesis_transform", "hyper_")
    missing = [n for n, p in model.named_parameters() if n.startswith(new) and p.grad is None]
    assert not missing, missing
