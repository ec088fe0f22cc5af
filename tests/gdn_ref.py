"""A float64 definition of GDN / IGDN and its gradients, written from the formulas and importing nothing of the
package: what the kernels AND their tensor-op twins are held to.

With x' = max(x, 0) under `rectify` (else x), u = |x'|^alpha, s = -eps (GDN) / +eps (IGDN) and g = dL/dy:
    n = beta + U Gamma          y = x' n^s
    T = dL/dn = s g y / n       R = g n^s
    dx = R + (T Gamma^T) d|x'|^alpha/dx'        dbeta = sum_p T        dGamma = U^T T
d|x'|^alpha/dx' is sign(x') for alpha = 1 and 2 x' for alpha = 2: the subgradient 0 at x' = 0.  Where the rectifier is
closed (x <= 0 under `rectify`) dx is 0 altogether.

The twins evaluate the same formulas with float32 CPU tensor ops.  The bfloat16 twin rounds to bfloat16 at exactly the
points where the kernels do (the headers of gdn_common.h and gdn_backward.hip): x, g and Gamma as given, u before the
contraction, T and R as stored, y and dx as stored; beta and every accumulator stay float32."""
import numpy as np
import torch


def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _parts(x, beta, gamma, inverse, rectify, alpha, eps):
    # (float64 CPU tensors: the same IEEE arithmetic as numpy's, on all cores)
    x, beta, gamma = _t64(x), _t64(beta), _t64(gamma)
    xe = torch.clamp_min(x, 0.0) if rectify else x
    u = xe.abs() if alpha == 1 else xe * xe if alpha == 2 else xe.abs() ** alpha
    n = beta + u @ gamma
    s = eps if inverse else -eps
    return x, gamma, xe, u, n, s


def forward(x, beta, gamma, inverse=False, rectify=False, alpha=1, eps=1):
    """y [pixels, C] in float64."""
    _, _, xe, _, n, s = _parts(x, beta, gamma, inverse, rectify, alpha, eps)
    return (xe * n ** s).numpy()


def grads(x, g, beta, gamma, inverse=False, rectify=False, alpha=1, eps=1):
    """-> dict(y, n, u, T, R, dx, dbeta, dgamma) in float64, alpha in {1, 2}."""
    assert alpha in (1, 2)
    x, gamma, xe, u, n, s = _parts(x, beta, gamma, inverse, rectify, alpha, eps)
    g = _t64(g)
    p = n ** s
    y = xe * p
    t = s * g * y / n
    r = g * p
    du = torch.sign(xe) if alpha == 1 else 2.0 * xe
    dx = r + (t @ gamma.T) * du
    if rectify:
        dx = torch.where(x > 0.0, dx, torch.zeros_like(dx))
    out = {"y": y, "n": n, "u": u, "T": t, "R": r, "dx": dx, "dbeta": t.sum(0), "dgamma": u.T @ t}
    return {k: v.numpy() for k, v in out.items()}


def _bf16(t):
    return t.bfloat16().float()


def twin(x, g, beta, gamma, inverse=False, rectify=False, alpha=1, eps=1, bf16=False):
    """The same formulas in float32 CPU tensor ops -> dict(y, dx, dbeta, dgamma) of float32 numpy arrays.  `bf16`:
    rounding to bfloat16 where the bfloat16 kernels round (see the module docstring); y and dx are then bfloat16
    values held in float32."""
    assert alpha in (1, 2)
    rnd = _bf16 if bf16 else (lambda t: t)
    f = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    x, g, gamma, beta = rnd(f(x)), rnd(f(g)), rnd(f(gamma)), f(beta)
    xe = torch.relu(x) if rectify else x
    u = rnd(xe.abs() if alpha == 1 else xe * xe)
    n = beta + u @ gamma
    s = eps if inverse else -eps
    if eps == 1:
        p = n if inverse else 1.0 / n
    else:
        p = n.sqrt() if inverse else n.rsqrt()
    y = xe * p
    t = rnd(s * g * y / n)
    r = rnd(g * p)
    du = torch.sign(xe) if alpha == 1 else 2.0 * xe
    dx = r + (t @ gamma.T) * du
    if rectify:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    return {"y": rnd(y).numpy(), "dx": rnd(dx).numpy(), "dbeta": t.sum(0).numpy(), "dgamma": (u.T @ t).numpy()}


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.sqrt(np.sum(want ** 2))
    num = np.sqrt(np.sum((got - want) ** 2))
    return num / den if den > 0 else num


# -- the input sets the tests share --------------------------------------------------------------------------------

def params(C, seed):
    """beta, gamma as float32 tensors: the `params()` of tests/test_gdn_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    beta = 1 + 0.1 * torch.rand(C, generator=g)
    gamma = 0.1 * torch.eye(C) + 0.01 * torch.rand(C, C, generator=g)
    return beta, gamma


def exact_inputs(pixels, C, seed):
    """x in {0, -0.0, +-1, +-2} (zeros about 1 in 8), g in {+-1, +-2}, beta = 1, Gamma multiples of 2^-6 in [0, 2^-3]:
    with IGDN and eps = 1 (T = g x', no division anywhere) every product and sum of the definition is exact in
    float32, and in bfloat16 where the bfloat16 kernels store bfloat16 on the way to dbeta and dGamma.
    -> float32 tensors x, g [pixels, C], beta [C], gamma [C, C]."""
    gen = torch.Generator().manual_seed(seed)
    xs = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 1.0, -1.0, 2.0, -2.0, 1.0, -1.0, 2.0, -2.0, 1.0, -2.0])
    x = xs[torch.randint(0, 16, (pixels, C), generator=gen)]
    g = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (pixels, C), generator=gen)]
    gamma = torch.randint(0, 9, (C, C), generator=gen).float() / 64
    return x, g, torch.ones(C), gamma


def random_inputs(pixels, C, seed, bf16):
    """x, g ~ N(0, 1) with about 1 in 16 elements of x exactly 0 (bf16: rounded to bfloat16, held in float32)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(pixels, C, generator=gen)
    g = torch.randn(pixels, C, generator=gen)
    x[torch.randint(0, 16, (pixels, C), generator=gen) == 0] = 0.0
    return (_bf16(x), _bf16(g)) if bf16 else (x, g)


# The exact family, as both the CPU and the GPU tier enumerate it.
EXACT_SMALL_PIXELS = (1, 31, 32, 33, 63, 64, 65, 64 * 15 + 1, 64 * 16, 64 * 17 + 3)
EXACT_SMALL_CHANNELS = (32, 96)
EXACT_LOOP_CHANNELS = {"bfloat16": (32, 96, 128, 192, 224, 256), "float32": (64, 160, 192)}
EXACT_VARIANTS = tuple((rectify, alpha) for alpha in (1, 2) for rectify in (False, True))


def p_loop(cus):
    """A ragged last tile and a ragged last stage past every loop threshold of a device with `cus` compute units."""
    return 64 * 4 * cus + 231


def loop_thresholds(cus):
    """Pixels (or rows) above which each persistent loop repeats: name -> threshold."""
    return {"gdn_fwd_f32_kernel": 32 * 4 * cus, "gdn_fwd_bf16_kernel": 32 * 8 * cus,
            "gdn_bwd_fused_bf16_kernel": 32 * 4 * cus, "gdn_param_grad_kernel": 64 * cus}
