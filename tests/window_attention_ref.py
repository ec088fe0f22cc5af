"""The definition of shifted-window attention (include/tfc_hip.h, tfc_window_attention_forward / _backward) in float64
NumPy, with explicit loops over windows and tokens, written from the text of the definition: it shares nothing with
compression_amd/ops/attention_ops.py.  Inputs are taken as the values they are.  Not a test module."""
import functools

import numpy as np


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu()
        if str(a.dtype) == "torch.bfloat16":
            a = a.float()
        a = a.numpy()
    return np.asarray(a, dtype=np.float64)


@functools.lru_cache(maxsize=8)
def windows(h, w, ws, s):
    """Every window of the padded grid -> a list of (tokens, memo): tokens a list of T entries
    (yp, xp, valid, wrap_y, wrap_x, ty, tx) in token order, memo what `_keys_of` remembers of the window."""
    hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
    found = []
    for wy in range(hp // ws):
        for wx in range(wp // ws):
            tokens = []
            for ty in range(ws):
                for tx in range(ws):
                    ry, rx = wy * ws + ty, wx * ws + tx
                    yp, xp = (ry + s) % hp, (rx + s) % wp
                    tokens.append((yp, xp, yp < h and xp < w, ry + s >= hp, rx + s >= wp, ty, tx))
            found.append((tokens, {}))
    return found


def _window_terms(x, table, heads, ws, tokens, b):
    """The per-head quantities of one window of image b: index lists and q, k, v [heads, T, d] (zeros where invalid)."""
    c = x.shape[-1] // 3
    d = c // heads
    t = len(tokens)
    q, k, v = np.zeros((heads, t, d)), np.zeros((heads, t, d)), np.zeros((heads, t, d))
    for i, (yp, xp, valid, _, _, _, _) in enumerate(tokens):
        if valid:
            row = x[b, yp, xp]
            for hd in range(heads):
                q[hd, i] = row[hd * d:(hd + 1) * d]
                k[hd, i] = row[c + hd * d:c + (hd + 1) * d]
                v[hd, i] = row[2 * c + hd * d:2 * c + (hd + 1) * d]
    return q, k, v, d, c


def _keys_of(memo, tokens, i, ws):
    """The keys that take part for query i (valid, the same two wrap flags) and their table entries; remembered per
    (window, query)."""
    if i not in memo:
        _, _, _, fy, fx, ty, tx = tokens[i]
        keys = [j for j, tk in enumerate(tokens) if tk[2] and tk[3] == fy and tk[4] == fx]
        rel = [(ty - tokens[j][5] + ws - 1) * (2 * ws - 1) + (tx - tokens[j][6] + ws - 1) for j in keys]
        memo[i] = (keys, rel)
    return memo[i]


def _row(memo, tokens, i, q, k, table, hd, ws, d):
    """Query i: the keys that take part, their table entries and P over them."""
    keys, rel = _keys_of(memo, tokens, i, ws)
    s = (k[hd, keys] @ q[hd, i]) / np.sqrt(d) + table[hd, rel]
    e = np.exp(s - s.max())
    return keys, rel, e / e.sum()


def forward(qkv, table, heads, ws, s):
    """-> out [B, H, W, C] float64."""
    x, table = _f64(qkv), _f64(table)
    bsz, h, w, c3 = x.shape
    out = np.zeros((bsz, h, w, c3 // 3))
    for b in range(bsz):
        for tokens, memo in windows(h, w, ws, s):
            q, k, v, d, c = _window_terms(x, table, heads, ws, tokens, b)
            for i, tk in enumerate(tokens):
                if not tk[2]:
                    continue
                for hd in range(heads):
                    keys, _, p = _row(memo, tokens, i, q, k, table, hd, ws, d)
                    out[b, tk[0], tk[1], hd * d:(hd + 1) * d] = p @ v[hd, keys]
    return out


def backward(qkv, table, dout, heads, ws, s):
    """dP = dO V^T, dS = P o (dP - rowsum(dP o P)), dV = P^T dO, dQ = d^-1/2 dS K, dK = d^-1/2 dS^T Q,
    dtable[head, rel] = sum of dS -> (dqkv [B, H, W, 3 C], dtable [heads, (2 ws - 1)^2]) float64."""
    x, table, g = _f64(qkv), _f64(table), _f64(dout)
    bsz, h, w, c3 = x.shape
    dqkv = np.zeros_like(x)
    dtable = np.zeros_like(table)
    for b in range(bsz):
        for tokens, memo in windows(h, w, ws, s):
            q, k, v, d, c = _window_terms(x, table, heads, ws, tokens, b)
            t = len(tokens)
            dq, dk, dv = np.zeros((heads, t, d)), np.zeros((heads, t, d)), np.zeros((heads, t, d))
            for i, tk in enumerate(tokens):
                if not tk[2]:
                    continue
                for hd in range(heads):
                    keys, rel, p = _row(memo, tokens, i, q, k, table, hd, ws, d)
                    go = g[b, tk[0], tk[1], hd * d:(hd + 1) * d]
                    dp = v[hd, keys] @ go
                    ds = p * (dp - (dp * p).sum())
                    dv[hd, keys] += p[:, None] * go[None, :]
                    dq[hd, i] += (ds @ k[hd, keys]) / np.sqrt(d)
                    dk[hd, keys] += ds[:, None] * q[hd, i][None, :] / np.sqrt(d)
                    np.add.at(dtable[hd], rel, ds)
            for i, tk in enumerate(tokens):
                if tk[2]:
                    for hd in range(heads):
                        dqkv[b, tk[0], tk[1], hd * d:(hd + 1) * d] = dq[hd, i]
                        dqkv[b, tk[0], tk[1], c + hd * d:c + (hd + 1) * d] = dk[hd, i]
                        dqkv[b, tk[0], tk[1], 2 * c + hd * d:2 * c + (hd + 1) * d] = dv[hd, i]
    return dqkv, dtable
