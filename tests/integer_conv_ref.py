"""The integer convolution layer (include/tfc_hip.h, tfc_integer_conv2d) stated in NumPy int64 with explicit loops:
the yardstick of the integer-layer tests.  Slow on purpose; the tests keep their shapes small.

    v[n,p,o] = bias[o] + sum over taps t and i < Cin of W[t,i,o] x[n, src(p,t), i]
    y[n,p,o] = min(max(floor((v + floor(c[o] / 2)) / c[o]), 0), out_max)

down (up = False): src = (oy s + ty - kh // 2, ox s + tx - kw // 2), out = ceil(in / s).
up (up = True):    y[q s + phi] = sum_i x[i] w[phi + (q - i) s + k // 2] per axis, out = in s.
Zeros outside the image."""
import numpy as np


def integer_conv2d_loops(x, kernel, bias, divisor, stride, up, out_max):
    """x [N, H, W, Cin] int8 / uint8, kernel [kh, kw, Cin, Cout] int8, bias / divisor [Cout] int32 -> uint8."""
    x = np.asarray(x).astype(np.int64)
    w = np.asarray(kernel).astype(np.int64)
    b = np.asarray(bias).astype(np.int64)
    c = np.asarray(divisor).astype(np.int64)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    s = int(stride)
    oh, ow = (h * s, wd * s) if up else (-(-h // s), -(-wd // s))
    v = np.zeros((n, oh, ow, cout), np.int64)
    for oy in range(oh):
        for ox in range(ow):
            for ty in range(kh):
                for tx in range(kw):
                    if up:
                        # t = phi + (q - i) s + k // 2 with o = q s + phi  <=>  i s = o + k // 2 - t
                        ny, nx = oy + kh // 2 - ty, ox + kw // 2 - tx
                        if ny % s or nx % s:
                            continue
                        iy, ix = ny // s, nx // s
                    else:
                        iy, ix = oy * s + ty - kh // 2, ox * s + tx - kw // 2
                    if 0 <= iy < h and 0 <= ix < wd:
                        v[:, oy, ox, :] += x[:, iy, ix, :] @ w[ty, tx]
    v += b
    assert np.abs(v).max() < 2 ** 31
    y = np.floor_divide(v + c // 2, c)
    return np.clip(y, 0, int(out_max)).astype(np.uint8)


def rounding_cases():
    """(v, c, out_max, expected y) of the rounding division, the expectation written out by hand: with v = q c + rem,
    rem = c - floor(c / 2) (c / 2 for an even c) is the first remainder that rounds up to q + 1 and the one below it the
    last that rounds down to q; c = 1 leaves v; a negative v gives 0; out_max caps."""
    cases = []
    for c in (2, 3, 254, 255, 256, 1000, (1 << 24) - 1, 1 << 24):
        for q in (0, 1, 5, 254):
            if q * c + c > (1 << 29):
                continue
            up = c - c // 2
            cases.append((q * c + up, c, 255, q + 1))
            cases.append((q * c + up - 1, c, 255, q))
    for v in (0, 1, 77, 255, 256):
        cases.append((v, 1, 255, min(v, 255)))
    for out_max in (1, 63, 255):
        cases.append((10 ** 6, 7, out_max, out_max))
        cases.append((1, 2, out_max, 1))
        cases.append((-1, 1, out_max, 0))
        cases.append((-1, 1 << 24, out_max, 0))
        cases.append((-(1 << 29), 1 << 24, out_max, 0))
    return cases


def rounding_operands(cases, unsigned):
    """The cases as ONE layer call: a 1x1 kernel on one pixel whose only non-zero activation is x[0] = 100, one output
    channel per case with the single non-zero weight w and bias = v - 100 w, so that v is built exactly."""
    cout = len(cases)
    x = np.zeros((1, 1, 1, 32), np.uint8 if unsigned else np.int8)
    x[..., 0] = 100
    w = np.zeros((1, 1, 32, cout), np.int8)
    b = np.zeros(cout, np.int32)
    c = np.zeros(cout, np.int32)
    for o, (v, div, _, _) in enumerate(cases):
        wv = int(np.clip(v // 100, -128, 127))
        if wv == 0:
            wv = 1
        w[0, 0, 0, o] = wv
        b[o] = v - 100 * wv
        c[o] = div
        assert abs(int(b[o])) <= 1 << 29
    return x, w, b, c
