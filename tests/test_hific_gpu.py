"""GPU tier: the HiFiC codec (compression_amd/models/hific.py; models/hific/archs.py, model.py) end to end on the
kernels, random weights, fixed seeds."""
import numpy as np
import pytest
import torch

import compression_amd as tfc
from compression_amd import synthetic
from compression_amd.models import hific

pytestmark = pytest.mark.gpu


def small(seed=0, **kw):
    torch.manual_seed(seed)
    cfg = dict(num_filters_base=16, num_filters_bottleneck=32, num_filters_hyper=32, num_residual_blocks=2)
    cfg.update(kw)
    model = hific.HiFiCModel(**cfg).cuda()
    # random ChannelNorm parameters, so that gamma and beta matter
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, tfc.ChannelNorm):
                m.gamma.uniform_(0.5, 1.5)
                m.beta.normal_(0, 0.3)
    return model.init_compression()


@pytest.mark.parametrize("batch,size", [(1, (64, 48)), (1, (50, 37)), (3, (40, 72))])
def test_round_trip_shapes_and_exact_latents(batch, size):
    model = small()
    x = torch.from_numpy(synthetic.lowpass_images(batch, size[0], size[1], seed=3)).cuda()
    out = model.compress(x)
    string, side_string, x_shape, y_shape, z_shape = out
    assert x_shape == size and y_shape == hific.latent_size(*size) and z_shape == hific.hyper_latent_size(*size)
    assert len(string) == batch == len(side_string)
    x_hat = model.decompress(*out)
    assert x_hat.shape == x.shape and x_hat.dtype == torch.uint8
    # the latents the decoder recovers are the encoder's quantised latents, exactly
    y, y_hat, z, means, scales = model.latents(x)
    got, _, _ = model.decode_latents(string, side_string, y_shape, z_shape)
    assert torch.equal(got, y_hat)
    # and decompress() is the evaluation forward fed the same quantised latents, bit for bit
    with torch.no_grad():
        rec, bits = model(x.float(), latents=y_hat)
    assert bits.shape == (batch,) and bool(torch.isfinite(bits).all())
    want = torch.clamp(torch.round(rec), 0, 255).to(torch.uint8)
    assert torch.equal(x_hat, want)
    unit = model.reconstruct(y_hat, x_shape).contiguous()
    assert torch.equal(x_hat, tfc.layers.functional.unit_to_image(unit))


def test_strings_equal_the_oracles():
    """Main and side strings are, byte for byte, what the oracle coder writes for the model's own symbols and tables (the
    way test_ms2020_strings_equal_the_oracles does it): side in channel mode (continuous_batched.py:370-383), main in
    index mode with the means subtracted (continuous_indexed.py:272-289, 355-386)."""
    from oracle import oracle
    port = oracle.best()
    model = small(seed=8)
    x = torch.from_numpy(synthetic.lowpass_images(3, 96, 64, seed=9)).cuda()
    string, side_string, x_shape, y_shape, z_shape = model.compress(x)
    with torch.no_grad():
        y, y_hat, z, means, scales = model.latents(x)
        em_z, em_y = model.side_entropy_model, model.entropy_model
        qoff = em_z.quantization_offset
        zsym = torch.round(z - qoff if qoff is not None else z).to(torch.int32) - em_z.cdf_offset.cuda()
        want_z, _, _ = port.encode(em_z.cdf.cpu().numpy(), zsym.reshape(3, -1).cpu().numpy())
        assert [bytes(s) for s in side_string] == want_z
        lookup = em_y.cdf.cpu().numpy()
        flat = em_y._table_indexes(scales.contiguous())
        sym = torch.round(y - means).to(torch.int32) - em_y.cdf_offset.cuda()[flat.long()]
        sym_h, idx_h = sym.reshape(3, -1).cpu().numpy(), flat.reshape(3, -1).cpu().numpy()
        want, _, _ = port.encode(lookup, sym_h, index=idx_h)
        assert [bytes(s) for s in string] == want
        dec, ok = port.decode(lookup, want, sym_h.shape[1], index=idx_h)
        assert ok.all() and (dec == sym_h).all()


def test_file_round_trip(tmp_path):
    from compression_amd import PackedTensors, models
    from compression_amd.models import codec_io
    model = small(seed=2)
    img = torch.from_numpy(synthetic.lowpass_images(1, 90, 70, seed=5)[0])
    models.write_png(tmp_path / "in.png", img)
    data = models.compress_file(model, tmp_path / "in.png", tmp_path / "out.tfci")
    direct = model.compress(img.cuda())
    dtypes = codec_io.container_dtypes(model)
    assert dtypes == [bytes, bytes, np.int32, np.int32, np.int32] and len(direct) == 5
    for got, want, dtype in zip(PackedTensors(data).unpack(dtypes), direct, dtypes):
        if dtype is bytes:
            assert [bytes(b) for b in got] == [bytes(b) for b in np.asarray(want, dtype=object).reshape(-1)]
        else:
            assert tuple(got.tolist()) == tuple(want)
    x_hat = models.decompress_file(model, tmp_path / "out.tfci", tmp_path / "rec.png")
    assert torch.equal(x_hat.cpu(), model.decompress(*direct)[0].cpu())
    assert x_hat.shape == img.shape


def test_device_result_and_deferred_sanity():
    model = small(seed=4)
    x = torch.from_numpy(synthetic.lowpass_images(2, 64, 64, seed=6)).cuda()
    plain = model.decompress(*model.compress(x))
    x_hat, ok = model.decompress(*model.compress(x, device_result=True), defer_sanity=True)
    assert torch.equal(x_hat, plain) and all(bool(o.all()) for o in ok)


def test_training_step_reaches_every_parameter_and_lowers_the_loss():
    """forward, MSE + bits, backward: every parameter of every ChannelNorm and convolution (and of the hyperprior) gets
    a finite, non-zero gradient; ten Adam steps on one fixed 64 x 64 batch lower the loss (as
    test_bls2017_training_steps_reduce_the_loss)."""
    model = small(seed=1)
    x = torch.from_numpy(synthetic.lowpass_images(4, 64, 64, seed=3)).cuda().float()

    def loss_of():
        rec, bits = model(x)
        return torch.mean((rec - x) ** 2) * 0.01 + bits.mean() / (64 * 64)
    loss = loss_of()
    loss.backward()
    bad = [n for n, p in model.named_parameters()
           if p.grad is None or not bool(torch.isfinite(p.grad).all()) or not bool(p.grad.abs().sum() > 0)]
    assert not bad, f"parameters without a finite non-zero gradient: {bad}"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = loss_of()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("hific training losses:", " ".join(f"{v:.4f}" for v in losses))
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_generator_equals_the_unfused_one(dtype):
    """The generator with `relu=` / `residual=` inside the ChannelNorm launch against the same layers run as ChannelNorm,
    then torch.relu / `+`.  float32: EQUAL BITS — the kernel's epilogue is the same instruction sequence either way
    (the flags only add max(y, 0) / + r behind it), and relu and add are exact or correctly rounded in both.  bfloat16:
    relu commutes with the rounding, so only the residual add differs: unfused is bf16(bf16(n) + r), fused bf16(n + r)
    with n the norm's float32 output.  A bfloat16 rounding (8 significant bits) moves a value by at most 2**-8 of it,
    so the two differ by at most 2**-8 (|n| + |unfused| + |fused|): one output rounding each.  Compared on the first
    block."""
    model = small(seed=5, compute_dtype=dtype)
    y = torch.randn(2, 5, 4, 32, device="cuda").to(dtype)
    with torch.no_grad():
        if dtype == torch.float32:
            fused = model.decoder(y)
            model.decoder.fused = False
            assert torch.equal(fused, model.decoder(y))
        else:
            t = model.decoder.head_norm_1(model.decoder.head_conv(model.decoder.head_norm_0(y)))
            block = model.decoder.residual_blocks[0]
            n = block.norm_1(block.conv_1(torch.relu(block.norm_0(block.conv_0(t))))).float()
            a, b = block(t, fused=True).float(), block(t, fused=False).float()
            assert torch.equal(b, (t + n.to(dtype)).float())
            excess = (a - b).abs() - 2 ** -8 * (n.abs() + a.abs() + b.abs())
            print(f"hific fused vs unfused bf16: max |a - b| = {(a - b).abs().max().item():.3e}, "
                  f"max excess over the bound = {excess.max().item():.3e}")
            assert excess.max() <= 0


@pytest.mark.slow
def test_reference_configuration_round_trip_bf16():
    """The reference's sizes (archs.py:67-173, 425-493: base 60, bottleneck 220, 9 blocks, hyperprior 320), one 256 x 256
    image, bfloat16: about 150 M parameters."""
    torch.manual_seed(0)
    model = hific.HiFiCModel(compute_dtype=torch.bfloat16).cuda().init_compression()
    x = torch.from_numpy(synthetic.lowpass_images(1, 256, 256, seed=7)).cuda()
    out = model.compress(x)
    assert out[2:] == ((256, 256), (16, 16), (4, 4))
    x_hat = model.decompress(*out)
    assert x_hat.shape == x.shape and x_hat.dtype == torch.uint8
    y, y_hat, *_ = model.latents(x)
    assert y.shape == (1, 16, 16, 220)
    got, _, _ = model.decode_latents(out[0], out[1], out[3], out[4])
    assert torch.equal(got, y_hat)
