#!/usr/bin/env python3
"""Same route, same bits: tools/conv_ab_bits.py <libA.so> <libB.so>

For a change that must not alter what SignalConv2D computes (a refactor of the dispatch, a move of kernels between
translation units).  Each library gets one fresh child process that points _lib.LIB_PATH at it before first use and runs
the shapes tests/test_signal_conv_gpu.py lists — every route, the smallest shape per route — on fixed seeds, and writes one
SHA-256 per case.  This process compares the two sets: different routes round differently, so equal hashes for every case
also say that no shape changed route.  Exit status 0: all equal."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    from compression_amd import _lib
    _lib.LIB_PATH = lib_path
    from compression_amd import layers
    from compression_amd.layers import conv2d_down, conv2d_up
    import test_signal_conv_gpu as T

    out = {}

    def put(name, t):
        torch.cuda.synchronize()
        t = t.detach().cpu().contiguous()
        raw = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().tobytes()
        assert name not in out, name
        out[name] = hashlib.sha256(raw).hexdigest()[:16] + " " + "x".join(map(str, t.shape))

    def env(**kw):
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def inputs(seed, shape, kshape, bf16, image=False):
        torch.manual_seed(seed)
        x = torch.rand(shape) if image else torch.randn(shape)
        ker = torch.randn(kshape) / np.sqrt(kshape[0] * kshape[1] * kshape[2])
        bias = torch.randn(kshape[3])
        if bf16:
            x, ker = x.bfloat16(), ker.bfloat16().float()
        return x.cuda(), ker, bias

    for n, h, w, cin, cout, k, s in T.CASES:                                  # float32, both TFC_CONV_F32 modes
        x, ker, bias = inputs(0, (n, h, w, cin), (k, k, cin, cout), False)
        for mode in ("split", "native"):
            env(TFC_CONV_F32=mode)
            for act in (None, "relu"):
                put("CASES %s f32 %s %s" % ((n, h, w, cin, cout, k, s), mode, act), conv2d_down(x, ker, bias, s, act))
        env(TFC_CONV_F32=None)
    for case in T.UP_CASES:
        n, h, w, cin, cout, k, s = case[:7]
        x, ker, bias = inputs(1, (n, h, w, cin), (k, k, cin, cout), False)
        for mode in ("split", "native"):
            env(TFC_CONV_F32=mode)
            put("UP_CASES %s f32 %s" % (case, mode), conv2d_up(x, ker, bias, s))
        env(TFC_CONV_F32=None)
    for up, n, h, w, cin, cout, k, s in T.GEN3_CASES:                         # bfloat16, third and second generation
        x, ker, bias = inputs(5, (n, h, w, cin), (k, k, cin, cout), True)
        for gen in ("4", "2", None):
            env(TFC_CONV_GEN=gen)
            put("GEN3_CASES %s gen %s" % ((up, n, h, w, cin, cout, k, s), gen), (conv2d_up if up else conv2d_down)(x, ker, bias, s, "relu"))
        env(TFC_CONV_GEN=None)
    for n, h, w, cin, cout, k, s in T.CASES:                                  # bfloat16 at the float32 shapes: first / second generation
        x, ker, bias = inputs(2, (n, h, w, cin), (k, k, cin, cout), True)
        put("CASES %s bf16" % ((n, h, w, cin, cout, k, s),), conv2d_down(x, ker, bias, s, "relu"))
    for k, s, cin, cout, hw in T.FEW_CHANNEL_CASES + T.FUSED_UP_CASES:       # transposed into few channels: phase, fused, gather, GEMM
        x, ker, bias = inputs(k * 10 + s, (3, hw[0], hw[1], cin), (k, k, cin, cout), True)
        for phase in (None, "0"):
            env(TFC_CONV_UP_PHASE=phase)
            for act in (None, "relu"):
                put("few %s phase %s %s" % ((k, s, cin, cout, hw), phase, act), conv2d_up(x, ker, bias, s, act))
        env(TFC_CONV_UP_PHASE=None)
    for k, s, cin, cout, hw in T.IMAGE_SIDE_CASES + [(9, 4, 3, 192, (128, 256))]:      # image side: direct (+ its 9x9 / 4 shape), patch, first kernel
        x, ker, bias = inputs(k + cout, (3, hw[0], hw[1], cin), (k, k, cin, cout), True, image=True)
        for act in (None, "relu"):
            put("image %s %s" % ((k, s, cin, cout, hw), act), conv2d_down(x, ker, bias, s, act))

    def gdn_layer(cin, cout, up, inverse, hw, batch, seed, fuse):
        torch.manual_seed(seed)
        gdn = layers.GDN(inverse=inverse)
        kw = dict(corr=False, strides_up=2) if up else dict(corr=True, strides_down=2)
        conv = layers.SignalConv2D(cout, (5, 5), padding="same_zeros", in_channels=cin, use_bias=True, activation=gdn, **kw).cuda()
        x = torch.randn(batch, hw[0], hw[1], cin, device="cuda") * 2 if cin > 4 else torch.rand(batch, hw[0], hw[1], cin, device="cuda").mul(255)
        if fuse:
            conv.fuse_gdn_activation = True
        with torch.no_grad():
            conv.build(cin, x.device)
            conv.bias.normal_()
            gdn.build(cout, x.device)
            gdn.reparam_gamma.add_(torch.rand_like(gdn.reparam_gamma) * 0.05)
            gdn.invalidate_kernel_cache()
            return conv(x.to(torch.bfloat16))

    for up, hw, cout in T.GDN_ACTIVATION_CASES:
        for inverse in (False, True):                                         # GDN / IGDN as the activation
            put("gdn activation %s" % ((up, hw, cout, inverse),), gdn_layer(192, cout, up, inverse, hw, 3, 3, True))
    for hw, batch in T.IMAGE_GDN_CASES:
        put("image gdn %s" % ((hw, batch),), gdn_layer(3, 192, False, False, hw, batch, 5, False))

    for up, n, h, w, cin, cout, k, s in T.F32_SPLIT_CASES:                    # float32 as six planes / native
        x, ker, bias = inputs(11, (n, h, w, cin), (k, k, cin, cout), False)
        for mode in ("split", "native"):
            env(TFC_CONV_F32=mode)
            put("F32_SPLIT_CASES %s %s" % ((up, n, h, w, cin, cout, k, s), mode), (conv2d_up if up else conv2d_down)(x, ker, bias, s))
        env(TFC_CONV_F32=None)
    x, ker, bias = inputs(11, (3, 20, 20, 16), (4, 4, 16, 40), False)          # three chunks of one image
    env(TFC_CONV_F32="split", TFC_CONV_F32_CHUNK_BYTES=str(20 * 20 * 6 * 16 * 2))
    put("f32 three chunks", conv2d_down(x, ker, bias, 2))
    put("f32 three chunks, keyed", conv2d_down(x, ker, bias, 2, weights_key=(1 << 41) + 7))
    env(TFC_CONV_F32=None, TFC_CONV_F32_CHUNK_BYTES=None)
    put("f32 one chunk, keyed again", conv2d_down(x, ker, bias, 2, weights_key=(1 << 41) + 7))
    _lib.lib().tfc_conv2d_drop_weights((1 << 41) + 7)

    key = (1 << 40) + 12345                                                   # keyed and unkeyed
    for up, shape, kshape, stride in T.KEYED_CASES:
        fn = conv2d_up if up else conv2d_down
        torch.manual_seed(11)
        x = torch.randn(shape, device="cuda").to(torch.bfloat16)
        w = torch.randn(kshape, device="cuda") / 30
        w2 = torch.randn(kshape, device="cuda") / 30
        name = "keyed %s %s" % (fn.__name__, kshape)
        put(name + " no key", fn(x, w, None, stride))
        put(name + " key, first", fn(x, w, None, stride, weights_key=key))
        w.copy_(w2)
        torch.cuda.synchronize()
        put(name + " key, kept fragments", fn(x, w, None, stride, weights_key=key))
        put(name + " no key, new value", fn(x, w, None, stride))
        _lib.lib().tfc_conv2d_drop_weights(key)
        put(name + " key, dropped", fn(x, w, None, stride, weights_key=key))
        _lib.lib().tfc_conv2d_drop_weights(key)
    print("CONV_AB_BITS " + json.dumps(out))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    got = []
    for path in sys.argv[1:]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(path)],
                           capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith("CONV_AB_BITS ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("conv_ab_bits: the run with %s failed (status %d); nothing further was started" % (path, r.returncode))
        got.append(json.loads(lines[-1][len("CONV_AB_BITS "):]))
    a, b = got
    differ = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in differ:
        print("DIFFERS  %-70s A %s   B %s" % (k, a.get(k), b.get(k)))
    print("conv_ab_bits: %d cases, %d bit-equal, %d differ (A = %s, B = %s)" % (len(set(a) | set(b)), len(set(a) | set(b)) - len(differ),
                                                                              len(differ), sys.argv[1], sys.argv[2]))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
