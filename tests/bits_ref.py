"""The training-time rate term, written down once in plain torch: what csrc/factorized_bits.hip and
csrc/noisy_normal_bits.hip are held to.  Nothing here imports the package under test.  Every function takes
raw tensors and works in the dtype it is given: float64 is the definition, and the float32 evaluation of the
very same functions (on the host, deterministic) is the error envelope the kernels are measured against.

  logits of the deep factorized cumulative   python/distributions/deep_factorized.py:166-194
  noisy log-probability, cdf / sf switch     python/distributions/uniform_noise.py:117-156
  Laplace-mixture tail                       python/entropy_models/continuous_base.py:298-334
  perturb_and_apply, expected gradients      python/ops/math_ops.py:157-216
  bits = - sum log p / ln 2 per coding unit  python/entropy_models/continuous_batched.py:291-322

The second half generates every input set of tests/test_bits_kernels_gpu.py from seeded functions
(tests/test_bits_ref_cpu.py checks each of them on the CPU) and evaluates definition, envelope and the
per-element tolerances for a case."""
import dataclasses
import functools
import math

import torch

F = torch.nn.functional
LN2 = math.log(2.0)
EPS32 = 2.0 ** -24          # half an ulp of float32 at 1
BF16_ULP = 2.0 ** -8
TAIL_SWITCH = 1e-10         # continuous_base.py:314
MARGIN = 4.0                # kernel error allowed over the float32 host evaluation of the same formula
# The hardware exp flushes results below the smallest normal float32 to 0 (the host evaluation keeps denormals),
# so a ratio sigma' / P or phi / P below FLT_MIN is lost BEFORE it is multiplied by dL/dbits, by z / scale, by
# d logit / d weight or, under a Laplace tail, by (1 - m) / mixture <= 1e10: an absolute error of A * FLT_MIN times
# those same multipliers is always inside the tolerance A * 2^-24 * norm.
FLUSH = 2.0 ** -126 / EPS32


# ------------------------------------------------------------------------------------------------ definition
def factorized_logits(x, matrices, biases, factors):
    """Logits of the cumulative at x [..., C].  matrices[i] [C, f_{i+1}, f_i], biases[i] [C, f_{i+1}, 1],
    factors[i] [C, f_{i+1}, 1] are the RAW parameters: softplus and tanh are applied here."""
    C = x.shape[-1]
    h = x.reshape(-1, C).t()[:, None, :]                      # [C, 1, N]
    for i, (m, b) in enumerate(zip(matrices, biases)):
        h = torch.einsum("coi,cin->con", F.softplus(m), h) + b
        if i < len(factors):
            h = h + torch.tanh(factors[i]) * torch.tanh(h)
    return h[:, 0, :].t().reshape(x.shape)


def log_difference(big, small):
    """log(exp(big) - exp(small)) = big + log(-expm1(small - big)) for big >= small.  Below -ln 2 the same
    number is taken as log1p(-exp(d)): autograd differentiates expm1 as result + 1, which has no digits left
    once d < -16 (float32), and the float32 evaluation of this file is the kernels' envelope."""
    d = small - big
    near = torch.log(-torch.expm1(d.clamp(min=-LN2)))
    return big + torch.where(d > -LN2, near, torch.log1p(-torch.exp(d.clamp(max=-LN2))))


def noisy_log_prob(log_cdf_up, log_cdf_lo, log_sf_up, log_sf_lo):
    """log(c(v + .5) - c(v - .5)) from the logs of the cumulative and of the survival function at both ends:
    right of the median (log sf < log cdf at the upper end) the survival functions are differenced."""
    right = log_sf_up < log_cdf_up
    return log_difference(torch.where(right, log_sf_lo, log_cdf_up), torch.where(right, log_sf_up, log_cdf_lo))


def factorized_parts(v, matrices, biases, factors):
    up = factorized_logits(v + 0.5, matrices, biases, factors)
    lo = factorized_logits(v - 0.5, matrices, biases, factors)
    lp = noisy_log_prob(F.logsigmoid(up), F.logsigmoid(lo), F.logsigmoid(-up), F.logsigmoid(-lo))
    return lp, up, lo


def factorized_log_prob(v, matrices, biases, factors):
    return factorized_parts(v, matrices, biases, factors)[0]


def normal_parts(v, scale):
    zu, zl = (v + 0.5) / scale, (v - 0.5) / scale
    lcu, lcl = torch.special.log_ndtr(zu), torch.special.log_ndtr(zl)
    lsu, lsl = torch.special.log_ndtr(-zu), torch.special.log_ndtr(-zl)
    right = lsu < lcu
    big, small = torch.where(right, lsl, lcu), torch.where(right, lsu, lcl)
    return log_difference(big, small), zu, zl, big, small


def normal_log_prob(v, scale):
    return normal_parts(v, scale)[0]


def laplace_unit_log_mass(v):
    """log of the Laplace(0, 1) mass of [v - .5, v + .5], closed form: sinh(.5) exp(-|v|) outside the unit
    interval around 0, 1 - exp(-.5) cosh(v) inside."""
    a = v.abs()
    inside = torch.log1p(-math.exp(-0.5) * torch.cosh(v.clamp(-0.5, 0.5)))
    return torch.where(a >= 0.5, math.log(math.sinh(0.5)) - a, inside)


def laplace_tail(log_p, v, m):
    """log of the mixture (1 - m) P + m Q; below 1e-10 the branch log m + log Q."""
    lq = laplace_unit_log_mass(v)
    probs = (1.0 - m) * torch.exp(log_p) + m * torch.exp(lq)
    return torch.where(probs < TAIL_SWITCH, math.log(m) + lq, torch.log(probs.clamp(min=TAIL_SWITCH)))


def perturb_and_apply(f, x, v, expected_grads):
    """f at the perturbed v = x + u (its derivative w.r.t. x is that of x).  With expected_grads the derivative
    w.r.t. x is f(x + .5) - f(x - .5) at the unperturbed x while every other gradient stays that of f(v)."""
    if not expected_grads:
        return f(v)
    with torch.no_grad():
        slope = f(x + 0.5) - f(x - 0.5)
    return f(v.detach()) + slope * (x - x.detach())


def bits(log_prob, coding_rank):
    return log_prob.sum(dim=tuple(range(-coding_rank, 0))) / -LN2


# ------------------------------------------------------------------------------------------------ input sets
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    prior: str                       # "factorized" | "normal"
    dtype: str = "f32"               # "f32" | "bf16"
    mode: str = "plain"              # "plain" | "expected" | "tail" | "tail_expected"
    lead: tuple = (3,)               # coding units
    inner: tuple = (5, 7)            # coded dimensions in front of the channel axis
    C: int = 48
    num_filters: tuple = (3, 3)
    init_scale: float = 10.0
    far: bool = False                # factorized: 1 element in 17 multiplied by 8 or more
    scale_shape: str = "full"        # normal: "scalar" | "channel" | "full"
    wide: bool = True                # normal: scales 1e-3 .. 1e3, |z| out to ~500 (else scales .5 .. 8:
    #                                  brackets small enough that one element cannot hide in a unit's sum)
    noise: bool = True
    loss: str = "both"               # "both" | "bits" | "y_hat"
    strided: bool = False            # hand the kernel a non-contiguous bottleneck
    seed: int = 0

    @property
    def shape(self):
        return tuple(self.lead) + tuple(self.inner) + (self.C,)

    @property
    def coding_rank(self):
        return len(self.inner) + 1

    @property
    def expected(self):
        return self.mode.endswith("expected")

    @property
    def tail_mass(self):
        return 1e-3 if self.mode.startswith("tail") else 0.0

    @property
    def torch_dtype(self):
        return torch.float32 if self.dtype == "f32" else torch.bfloat16

    @property
    def regimes(self):
        """What the case claims to cover; tests/test_bits_ref_cpu.py counts >= 32 elements in each."""
        r = []
        if self.prior == "factorized":
            r.append("lp_0.1")
            if self.far:
                r += ["logit_100_left", "logit_100_right", "prob_1e-38"]
            if self.tail_mass:
                r += ["tail_switch", "tail_material"]
        else:
            if self.wide and self.scale_shape != "scalar":
                r += ["z_300", "integer", "scale_small", "scale_large"]
            if not self.wide:
                r.append("lp_0.1")
            if self.tail_mass:
                r += ["tail_switch", "tail_material"]
        return r


def _gen(seed):
    return torch.Generator().manual_seed(1000 + seed)


def factorized_raw_params(C, num_filters, init_scale, seed, jitter=0.2):
    """Raw parameters as the prior initialises them (deep_factorized.py:97-131: every matrix at
    softplus^-1(1 / s / fan), s = init_scale^(1 / layers); biases uniform in +-.5; gates 0), then jittered so
    that no two channels and no two weights are alike."""
    g = _gen(seed)
    filters = (1,) + tuple(num_filters) + (1,)
    s = init_scale ** (1.0 / (len(num_filters) + 1))
    mats, bias, fact = [], [], []
    for i in range(len(num_filters) + 1):
        init = math.log(math.expm1(1.0 / s / filters[i + 1]))
        mats.append(torch.full((C, filters[i + 1], filters[i]), init) + jitter * torch.randn(C, filters[i + 1], filters[i], generator=g))
        bias.append(torch.rand(C, filters[i + 1], 1, generator=g) - 0.5 + jitter * torch.randn(C, filters[i + 1], 1, generator=g))
        if i < len(num_filters):
            fact.append(jitter * torch.randn(C, filters[i + 1], 1, generator=g))
    return mats, bias, fact


def make_inputs(case):
    """Every tensor a case feeds the kernel, on the CPU: y and noise in the case's dtype, float32 parameters /
    scale, the weights of the units in the loss, and v = the dtype's rounding of the float32 sum y + noise
    (IEEE: the device forms the same sum)."""
    g = _gen(case.seed)
    shape = case.shape
    n = int(torch.Size(shape).numel())
    out = {}
    if case.prior == "factorized":
        out["params"] = factorized_raw_params(case.C, case.num_filters, case.init_scale, case.seed)
        y = 3.0 * case.init_scale * torch.randn(shape, generator=g)
        flat = y.reshape(-1)
        if case.tail_mass and n:
            # where the Laplace component matters or takes over: 4 <= |v| <= 32, whatever the prior's scale
            mid = flat[5::13]
            mid.copy_(torch.sign(mid) * (4.0 + 28.0 * torch.rand(mid.shape, generator=g)))
        if case.far and n:
            sel = flat[::17]
            want = case.init_scale * (120.0 + 580.0 * torch.rand(sel.shape, generator=g))
            sel.mul_(torch.maximum(torch.full_like(sel, 8.0), want / sel.abs().clamp(min=1e-3)))
    else:
        if case.scale_shape == "scalar":
            scale = torch.tensor(1.7)
        else:
            lo, hi = (-3.0, 3.0) if case.wide else (math.log10(0.5), math.log10(8.0))
            sshape = shape if case.scale_shape == "full" else (case.C,)
            scale = 10.0 ** (lo + (hi - lo) * torch.rand(sshape, generator=g))
        out["scale"] = scale
        full = torch.broadcast_to(scale, shape)
        y = 1.5 * full * torch.randn(shape, generator=g)
        flat = y.reshape(-1)
        if case.wide and n:
            far = flat[::11]                                             # |z| from 50 to ~500
            far.copy_(torch.sign(far) * full.reshape(-1)[::11] * (50.0 + 450.0 * torch.rand(far.shape, generator=g)))
            flat[3::7] = torch.round(flat[3::7])                         # integer-valued inputs
        if case.tail_mass and n:
            mid = flat[5::13]
            mid.copy_(torch.sign(mid) * (4.0 + 28.0 * torch.rand(mid.shape, generator=g)))
    y = y.to(case.torch_dtype)
    out["y"] = y
    if case.noise:
        noise = (torch.rand(shape, generator=g) - 0.5).to(case.torch_dtype)
        if case.prior == "normal" and case.wide and n:
            noise.reshape(-1)[3::14] = 0                                 # half of the integers stay integers
        out["noise"] = noise
        out["v"] = (y.float() + noise.float()).to(case.torch_dtype)
    else:
        out["noise"] = None
        out["v"] = y.clone()
    units = int(torch.Size(case.lead).numel())
    out["w"] = (torch.tensor([1.0, -2.0, 0.5]).repeat(units // 3 + 1)[:units]).reshape(case.lead)
    return out


# ------------------------------------------------------------------------------------------------ evaluation
def _bracket(num, big_minus_small, lp):
    return num / -torch.expm1(-big_minus_small.abs()) + lp.abs()


def _eval(case, inp, dtype, with_norms, full_scale=False):
    """Loss and gradients of a case in `dtype`.  with_norms (float64 only): the per-element scale of the
    rounding error of a float32 evaluation, see `reference`."""
    m = case.tail_mass
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)       # never the cached input itself
    y = leaf(inp["y"])
    v = inp["v"].to(dtype) + (y - y.detach())         # exactly the rounded sum; d v / d y = 1
    if case.prior == "factorized":
        leaves = [leaf(t) for grp in inp["params"] for t in grp]
        K = len(case.num_filters) + 1
        grp = (leaves[:K], leaves[K:2 * K], leaves[2 * K:])
        parts = lambda t: factorized_parts(t, *grp)
    else:
        leaves = [leaf(torch.broadcast_to(inp["scale"], case.shape) if full_scale else inp["scale"])]
        parts = lambda t: normal_parts(t, leaves[0])
    f = (lambda t: laplace_tail(parts(t)[0], t, m)) if m else (lambda t: parts(t)[0])
    lp = perturb_and_apply(f, y, v, case.expected)
    b = bits(lp, case.coding_rank)
    w = inp["w"].to(dtype)
    loss = 0
    if case.loss in ("both", "bits"):
        loss = loss + (b * w).sum()
    if case.loss in ("both", "y_hat"):
        loss = loss + 1e-3 * (v ** 2).sum()
    grads = torch.autograd.grad(loss, [y] + leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, [y] + leaves)]
    res = {"lp": lp.detach(), "bits": b.detach(), "dy": grads[0], "dleaves": grads[1:]}
    if not with_norms:
        return res

    # --- scales of the float32 rounding error, from the conditioning of the formula -----------------------
    def fwd(t):
        """log p, its bracket (|error| <= A 2^-24 bracket), and the pieces the gradient scales need"""
        t = t.detach().requires_grad_(True)
        if case.prior == "factorized":
            lpp, up, lo = parts(t)
            dup, dlo = torch.autograd.grad(up.sum(), t, retain_graph=True)[0], torch.autograd.grad(lo.sum(), t)[0]
            br = _bracket(1 + up.abs() + lo.abs(), up - lo, lpp)
            gu = torch.exp(F.logsigmoid(up) + F.logsigmoid(-up) - lpp)
            gl = torch.exp(F.logsigmoid(lo) + F.logsigmoid(-lo) - lpp)
            aux = dict(gu=gu, gl=gl, dup=dup, dlo=dlo, up=up, lo=lo)
        else:
            lpp, zu, zl, big, small = parts(t)
            br = _bracket(1 + zu ** 2 + zl ** 2, big - small, lpp)
            c = 0.5 * math.log(2 * math.pi)
            aux = dict(gu=torch.exp(-0.5 * zu ** 2 - c - lpp), gl=torch.exp(-0.5 * zl ** 2 - c - lpp), zu=zu, zl=zl)
        lpp, br = lpp.detach(), br.detach()
        wgt = torch.ones_like(lpp)
        if m:
            # d log(mixture) / d log P = (1 - m) P / mixture <= 1 (0 in the log m + log Q branch): the prior's
            # error enters with that weight; the Laplace term and the final log add 1 + |log mixture|
            lq = laplace_unit_log_mass(t.detach())
            probs = (1 - m) * torch.exp(lpp) + m * torch.exp(lq)
            mixed = laplace_tail(lpp, t.detach(), m)
            wgt = torch.where(probs < TAIL_SWITCH, torch.zeros_like(lpp), (1 - m) * torch.exp(lpp - mixed))
            aux.update(probs=probs, p_prior=torch.exp(lpp), p_tail=m * torch.exp(lq))
            br = wgt * br + 1 + mixed.abs()
            lpp = mixed
        return lpp, br, wgt, {k: a.detach() for k, a in aux.items()}

    lpv, br, wgt, aux = fwd(v)
    res.update(bracket=br, aux=aux, lp_prior_weight=wgt)
    gunit = (w / LN2).reshape(tuple(case.lead) + (1,) * case.coding_rank).expand(case.shape).abs()
    if case.loss == "y_hat":
        gunit = torch.zeros_like(gunit)
    flush = FLUSH * gunit
    if m:
        flush = flush * torch.where(aux["probs"] < TAIL_SWITCH, torch.zeros_like(br), (1 - m) / aux["probs"].clamp(min=TAIL_SWITCH))
    gyhat = (2e-3 * v.detach()).abs() if case.loss in ("both", "y_hat") else torch.zeros_like(gunit)
    if case.prior == "factorized":
        gross_v = wgt * (aux["gu"] * aux["dup"].abs() + aux["gl"] * aux["dlo"].abs())
        flush_v = flush * (aux["dup"].abs() + aux["dlo"].abs())
    else:
        s = torch.broadcast_to(leaves[0].detach(), case.shape)
        gross_v = wgt * (aux["gu"] + aux["gl"]) / s
        flush_v = flush / s
    if case.expected:
        _, bp, _, _ = fwd(y.detach() + 0.5)
        _, bm, _, _ = fwd(y.detach() - 0.5)
        ndy = gunit * (bp + bm)
    else:
        ndy = gunit * (br * gross_v + (1.0 if m else 0.0))
    res["n_dy"] = ndy + gyhat + grads[0].abs() + flush_v + FLUSH
    if case.prior == "factorized":
        # gross size of a channel's parameter gradient: the same sum with every element's weight made positive
        # and scaled by its bracket, taken separately left and right of 0 (where d logit / d weight changes sign)
        wel = (gunit * br * wgt * torch.maximum(aux["gu"], aux["gl"]) + flush).detach()
        vd = v.detach()
        _, up, lo = parts(vd)
        gross = [torch.zeros_like(t) for t in leaves]
        for side in (vd >= 0, vd < 0):
            gs = torch.autograd.grad((wel * side * (up + lo)).sum(), leaves, retain_graph=True, allow_unused=True)
            gross = [a + (torch.zeros_like(a) if b_ is None else b_.abs()) for a, b_ in zip(gross, gs)]
        per_channel = max(1, v.numel() // case.C)
        res["n_dleaves"] = [a + gr.abs() + FLUSH * per_channel for a, gr in zip(gross, grads[1:])]
    else:
        per = gunit * br * wgt * (aux["gu"] * aux["zu"].abs() + aux["gl"] * aux["zl"].abs()) / s
        per = per + flush * (aux["zu"].abs() + aux["zl"].abs()) / s
        red = per.sum_to_size(leaves[0].shape) if leaves[0].dim() else per.sum()
        res["n_dleaves"] = [red + grads[1].abs() + FLUSH * max(1, v.numel() // max(1, leaves[0].numel()))]
    return res


def _worst(err, norm):
    """Smallest A with err <= A 2^-24 norm everywhere (inf where the scale is 0 and the error is not)."""
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    r = torch.where(norm > 0, err / (EPS32 * norm.clamp(min=1e-300)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


@functools.lru_cache(maxsize=2)          # a case is used twice in a row; the 2.4 M-element ones hold ~1 GB each
def reference(case):
    """Definition (float64), its float32 host evaluation, and A_ref per quantity: the smallest A at which the
    float32 evaluation stays within A 2^-24 norm of the definition.  A kernel passes with MARGIN * A_ref."""
    inp = make_inputs(case)
    r64 = _eval(case, inp, torch.float64, True)
    r32 = _eval(case, inp, torch.float32, False)
    a = {"lp": _worst((r32["lp"].double() - r64["lp"]).abs(), r64["bracket"]),
         "dy": _worst((r32["dy"].double() - r64["dy"]).abs(), r64["n_dy"]),
         "dleaves": [_worst((g32.double() - g64).abs(), nn)
                     for g32, g64, nn in zip(r32["dleaves"], r64["dleaves"], r64["n_dleaves"])]}
    a["dleaves_own"] = list(a["dleaves"])
    if case.prior == "normal" and case.scale_shape == "scalar":
        # ONE number summed over every element: the float32 host error of that sum is a single draw of a sum
        # of signed per-element errors and can land anywhere below its scale (the same input set gives own
        # A_ref 4e-4 in float32 and 1.5e-3 in bfloat16), so 4 x it is no bound.  The scale of that draw is
        # the float32 evaluation's PER-ELEMENT errors added in quadrature; the envelope is the larger of the
        # two.  Every gradient with more than one entry keeps its own A_ref (the maximum over entries).
        e64 = _eval(case, inp, torch.float64, False, full_scale=True)["dleaves"][0]
        e32 = _eval(case, inp, torch.float32, False, full_scale=True)["dleaves"][0]
        quad = (e32.double() - e64).pow(2).sum().sqrt()
        a["dleaves"] = [max(a["dleaves"][0], _worst(quad.reshape(1), r64["n_dleaves"][0].reshape(1)))]
    return {"inputs": inp, "f64": r64, "f32": r32, "A_ref": a}


def worst_element(got, want, norm, extra=None):
    """(index, got, want, norm) of the element with the largest error relative to its norm, for a message."""
    got = got.detach().double().cpu()
    if got.numel() == 0:
        return None
    err = (got - want).abs()
    r = (err if extra is None else (err - extra).clamp(min=0)) / norm.clamp(min=1e-300)
    i = int(torch.nan_to_num(r, nan=float("inf")).reshape(-1).argmax())
    idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), got.shape)) if got.dim() else ()
    return idx, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]), float(norm.reshape(-1)[i])


def smallest_a(got, want, norm, extra=None):
    """The kernel's own smallest passing A; `extra` is an allowance on top (bf16 storage of dy)."""
    err = (got.double().cpu() - want).abs()
    if extra is not None:
        err = torch.where(torch.isfinite(err), (err - extra).clamp(min=0), err)
    return _worst(err, norm)


# ------------------------------------------------------------------------------------------------ the cases
_PAIRED_SCALE = {(3, 3): 10.0, (3, 3, 3): 1.0, (5, 5): 0.3}
MODES = ("plain", "expected", "tail", "tail_expected")


def _nf(num_filters):
    return "x".join(map(str, num_filters))


def factorized_matrix_cases():
    """build x mode at C = 48: 3 num_filters x 2 dtypes x 4 modes, each on a near and a far input set.  The
    init_scale goes with the build (10, 1, 0.3); the Laplace-tail modes all use 0.3, the only one of the three
    at which the unit Laplace component is ever material."""
    out = []
    for i, nf in enumerate(_PAIRED_SCALE):
        for dt in ("f32", "bf16"):
            for mode in MODES:
                for far in (False, True):
                    sc = 0.3 if mode.startswith("tail") else _PAIRED_SCALE[nf]
                    out.append(Case(f"fm-{_nf(nf)}-{dt}-{mode}-{'far' if far else 'near'}", "factorized", dtype=dt,
                                    mode=mode, num_filters=nf, init_scale=sc, far=far,
                                    loss="both" if dt == "f32" else "bits", seed=10 + i))
    return out


PLAN_THREADS = {1: 256, 3: 255, 65: 195, 128: 256, 150: 300, 192: 192, 220: 220, 257: 257, 320: 320, 512: 512}


def factorized_plan_cases():
    """Block plans: every channel count below; 150, 320 and 512 (MAXT = 512 build) on all three num_filters, f32
    and bf16.  3 units of at least 7 rows of C and at least 4000 elements, so that the far tails are populated."""
    out = []
    for C in PLAN_THREADS:
        for nf in (((3, 3), (3, 3, 3), (5, 5)) if C in (150, 320, 512) else ((3, 3),)):
            for dt in (("f32", "bf16") if C in (150, 320, 512) else ("f32",)):
                out.append(Case(f"fp-C{C}-{_nf(nf)}-{dt}", "factorized", dtype=dt, C=C, num_filters=nf, inner=(max(7, -(-4000 // C)),),
                                init_scale=_PAIRED_SCALE[nf], far=True, loss="both" if dt == "f32" else "bits",
                                seed=40 + C % 7))
    return out


def geometry_cases():
    """One row per unit; one unit of many rows with a ragged last row; 3000 units of 3 * threads + C elements
    (one block per unit, several trips of the stride loop).  Factorized at C = 48 (240 threads) and C = 150
    (300 threads, the MAXT = 512 build); the normal kernel's rows are 256 elements whatever C is."""
    out = []
    for C, thr in ((48, 240), (150, 300)):
        k = dict(prior="factorized", C=C, init_scale=10.0, loss="bits")
        out += [Case(f"fg-C{C}-onerow", lead=(6,), inner=(), **k, seed=61),
                Case(f"fg-C{C}-ragged", lead=(1,), inner=((40 * thr + C) // C,), **k, seed=62),
                Case(f"fg-C{C}-manyunits", lead=(3000,), inner=((3 * thr + C) // C,), **k, seed=63)]
    k = dict(prior="normal", wide=False, loss="bits")
    out += [Case("ng-onerow", lead=(6,), inner=(), C=256, **k, seed=64),
            Case("ng-ragged", lead=(1,), inner=(83,), C=16, **k, seed=65),        # 5.19 rows of 256
            Case("ng-manyunits", lead=(3000,), inner=(), C=3 * 256 + 48, **k, seed=66),
            Case("ng-manyunits-bf16", lead=(3000,), inner=(), C=3 * 256 + 48, dtype="bf16", **k, seed=67)]
    return out


def call_shape_cases():
    out = []
    for prior, extra in (("factorized", dict(far=True)), ("normal", dict())):
        p = prior[0]
        out += [Case(f"{p}c-nonoise", prior, noise=False, seed=71, **extra),
                Case(f"{p}c-strided", prior, strided=True, seed=72, **extra),
                Case(f"{p}c-bitsonly", prior, loss="bits", seed=73, **extra),
                Case(f"{p}c-yhatonly", prior, loss="y_hat", seed=74, **extra),
                Case(f"{p}c-nonoise-expected", prior, noise=False, mode="expected", seed=75, **extra)]
    return out


def normal_matrix_cases():
    """dtype x mode x scale shape: scalar, per-channel (C,), full; scales from 1e-3 to 1e3 in one tensor, integer
    inputs among the rest, |z| out to ~500."""
    out = []
    for dt in ("f32", "bf16"):
        for mode in MODES:
            for ss in ("scalar", "channel", "full"):
                out.append(Case(f"nm-{dt}-{mode}-{ss}", "normal", dtype=dt, mode=mode, scale_shape=ss,
                                loss="both" if dt == "f32" else "bits", seed=80))
    return out


def all_cases():
    return (factorized_matrix_cases() + factorized_plan_cases() + geometry_cases() + call_shape_cases()
            + normal_matrix_cases())


def regime_counts(case):
    """Elements of the case in each regime it claims (float64, at the perturbed v)."""
    ref = reference(case)
    r64, aux = ref["f64"], ref["f64"]["aux"]
    c = {}
    lp = r64["lp"]
    c["min_abs_lp"] = float(lp.abs().min()) if lp.numel() else float("inf")
    if case.prior == "factorized":
        c["logit_100_left"] = int((aux["up"] < -100).sum())
        c["logit_100_right"] = int((aux["lo"] > 100).sum())
        plain = factorized_log_prob(ref["inputs"]["v"].double(), *[[t.double() for t in g] for g in ref["inputs"]["params"]])
        c["prob_1e-38"] = int((plain < math.log(1e-38)).sum())
    else:
        full = torch.broadcast_to(ref["inputs"]["scale"].double(), case.shape)
        v = ref["inputs"]["v"].double()
        c["z_300"] = int(((v.abs() / full) > 300).sum())
        c["integer"] = int((v == v.round()).sum())
        c["scale_small"] = int((full < 1e-2).sum())
        c["scale_large"] = int((full > 1e2).sum())
    if case.tail_mass:
        probs, pp, pt = aux["probs"], (1 - case.tail_mass) * aux["p_prior"], aux["p_tail"]
        c["tail_switch"] = int((probs < TAIL_SWITCH).sum())
        c["tail_material"] = int(((probs >= TAIL_SWITCH) & (pt > 0.05 * pp)).sum())
        c["tail_switch_margin"] = float((probs / TAIL_SWITCH - 1).abs().min())
    return c
