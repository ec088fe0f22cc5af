"""CPU tier of the space-channel context model: the torch twin of ops/scctx_ops.py against the float64 numpy definition
of tests/scctx_ref.py, teacher forcing, causality between groups and between the passes of a group, the single group
against the checkerboard model, the stream slicing, the packed layout, the LDS fit and the argument checks."""
import numpy as np
import pytest
import torch

import checkerboard_ref
import scctx_ref
from compression_amd.ops import checkerboard_ops, scctx_ops

NUM_SCALES = 64
SHAPES = scctx_ref.GPU_SHAPES


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def params_of(weights, dtype=torch.float64, stream_positions=64):
    groups = [tuple(None if w is None else torch.from_numpy(np.asarray(w)).to(dtype) for w in group) for group in weights]
    return scctx_ops.SpaceChannelParams(groups, NUM_SCALES, stream_positions)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + "-" + "_".join(map(str, s[3])))
def case(request):
    shape = request.param
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    want = scctx_ref.scctx_scan(y, psi, weights, NUM_SCALES)
    params = params_of(weights, stream_positions=shape[4])
    got = scctx_ops.scctx_scan_reference(torch.from_numpy(y).double(), torch.from_numpy(psi).double(), params)
    return dict(shape=shape, y=y, psi=psi, weights=weights, want=want, params=params, got=got)


def test_scan_reference_equals_the_numpy_definition(case):
    got, want = case["got"], case["want"]
    for name in ("mu", "y_hat", "index_float"):
        assert rel_l2(getattr(got, name).numpy(), want[name]) <= 1e-12, name
    assert np.array_equal(got.sym.numpy(), want["sym"])
    assert np.array_equal(got.idx.numpy(), want["idx"])
    assert got.sym.dtype == torch.int32 and got.idx.dtype == torch.int32
    # the public entries take CPU tensors through the same code
    yt, pt, params = torch.from_numpy(case["y"]).double(), torch.from_numpy(case["psi"]).double(), case["params"]
    pub = scctx_ops.scctx_scan(yt, pt, params)
    assert torch.equal(pub.y_hat, got.y_hat)
    for g, (c, mg) in enumerate(zip(params.offsets, params.groups)):
        for pass_ in (0, 1):
            mu, index = scctx_ops.scctx_parameters(got.y_hat, pt, params, g, pass_)
            assert torch.equal(mu, checkerboard_ops.checkerboard_split(got.mu[..., c:c + mg])[pass_])
            assert torch.equal(index, checkerboard_ops.checkerboard_split(got.index_float[..., c:c + mg])[pass_])


def test_teacher_forcing_returns_the_scans_parameters(case):
    got, params = case["got"], case["params"]
    pt = torch.from_numpy(case["psi"]).double()
    mu, index = scctx_ops.scctx_parameters_reference(got.y_hat, pt, params)
    assert rel_l2(mu.numpy(), got.mu.numpy()) <= 1e-12
    assert rel_l2(index.numpy(), got.index_float.numpy()) <= 1e-12
    mu_np, index_np = scctx_ref.scctx_parameters(case["want"]["y_hat"], case["psi"], case["weights"])
    assert rel_l2(mu.numpy(), mu_np) <= 1e-12 and rel_l2(index.numpy(), index_np) <= 1e-12


def test_later_steps_do_not_reach_earlier_ones(case):
    """Exact in the float64 definition: a step's parameters are computed from the steps before it alone."""
    got, params = case["got"], case["params"]
    yt, pt = torch.from_numpy(case["y"]).double(), torch.from_numpy(case["psi"]).double()
    hl, wl = yt.shape[1:3]
    anchors = checkerboard_ops.anchor_mask(hl, wl)
    for g, (c, mg) in enumerate(zip(params.offsets, params.groups)):
        # another y in group g and everything after it: the steps of the groups before g keep their parameters
        changed = yt.clone()
        changed[..., c:] += 3.0
        other = scctx_ops.scctx_scan_reference(changed, pt, params)
        assert torch.equal(other.mu[..., :c], got.mu[..., :c])
        assert torch.equal(other.index_float[..., :c], got.index_float[..., :c])
        # and step (g, 0) too: group g's anchors take nothing from group g
        assert torch.equal(other.mu[:, anchors, c:c + mg], got.mu[:, anchors, c:c + mg])
        if g + 1 < len(params):
            assert not torch.equal(other.mu[..., c + mg:], got.mu[..., c + mg:])
        # another y at the pass-1 positions of group g: step (g, 0) and all before it keep their parameters
        changed = yt.clone()
        changed[:, ~anchors, c:c + mg] += 3.0
        other = scctx_ops.scctx_scan_reference(changed, pt, params)
        for name in ("mu", "index_float"):
            a, b = getattr(other, name), getattr(got, name)
            assert torch.equal(a[..., :c], b[..., :c]), name
            assert torch.equal(a[:, anchors, c:c + mg], b[:, anchors, c:c + mg]), name
            # nor do the other pass-1 positions of the group: a pass-1 position sees anchors only
            assert torch.equal(a[..., c:c + mg], b[..., c:c + mg]), name


def test_one_group_is_the_checkerboard_model():
    shape = next(s for s in SHAPES if len(s[3]) == 1)
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    yt, pt = torch.from_numpy(y).double(), torch.from_numpy(psi).double()
    got = scctx_ops.scctx_scan_reference(yt, pt, params_of(weights))
    checker = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w).double() for w in weights[0][1:]], NUM_SCALES)
    want = checkerboard_ops.checkerboard_scan_reference(yt, pt, checker)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    ref = checkerboard_ref.checkerboard_scan(y, psi, weights[0][1:], NUM_SCALES)
    assert rel_l2(got.y_hat.numpy(), ref["y_hat"]) <= 1e-12
    # and the packed buffer is the checkerboard model's, float for float
    f32 = params_of(weights, torch.float32)
    checker32 = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights[0][1:]], NUM_SCALES)
    assert torch.equal(f32.packed(0, "cpu"), checker32.packed("cpu"))


@pytest.mark.parametrize("hl,wl", [(1, 2), (3, 2), (4, 7), (9, 15), (20, 52)])
@pytest.mark.parametrize("sp", [1, 5, 16, 32, 64, 1000])
def test_stream_slicing_round_trips_and_counts_the_strings(hl, wl, sp):
    t = torch.arange(2 * hl * wl * 3, dtype=torch.float64).reshape(2, hl, wl, 3)
    total = 0
    for pass_, compact in enumerate(checkerboard_ops.checkerboard_split(t)):
        n = compact.shape[1]
        full, last = scctx_ops.stream_split(compact, sp)
        assert torch.equal(scctx_ops.stream_merge(full, last), compact)
        got = ([] if full is None else [full[:, s] for s in range(full.shape[1])]) + ([] if last is None else [last[:, 0]])
        want = scctx_ref.streams(compact.numpy(), sp)
        assert len(got) == len(want) == -(-n // sp) == scctx_ops.stream_counts(hl, wl, sp)[pass_]
        for a, b in zip(got, want):
            assert np.array_equal(a.numpy(), b)
        assert full is None or full.shape[2] == sp
        assert last is None or 0 < last.shape[2] < sp
        total += len(got)
    for groups in ((3,), (2, 1), (1, 1, 1)):
        assert len(groups) * total == scctx_ref.stream_total(hl, wl, groups, sp)
    if sp >= -(-hl * wl // 2):
        assert scctx_ops.stream_counts(hl, wl, sp) == (1, 1)                  # one stream per pass


def test_packed_layout_is_the_headers():
    """Recomputed from the two tap lists, section by section: nothing but these values, zeros elsewhere."""
    shape = (1, 1, 2, (3, 5), 64)
    _, _, weights = scctx_ref.make_case(shape, NUM_SCALES)
    params = params_of(weights, torch.float32)
    pad = lambda v: -(-v // 4) * 4
    p = 16
    c_g = 0
    for g, group in enumerate(weights):
        m_g = group[1].shape[2]
        h1, h2 = scctx_ref.hidden_widths(m_g, p)
        assert (params.own[g].h1, params.own[g].h2) == (h1, h2)
        blocks = []

        def take(values, rows, padded, cols):
            block = np.zeros(pad(padded * cols), np.float32)
            block[:rows * cols] = np.asarray(values, np.float32).reshape(-1)
            blocks.append(block)

        own = np.zeros((12, pad(m_g), 2 * m_g), np.float32)
        for k in range(12):                                                   # packed tap k is window element 2 k + 1
            own[k, :m_g] = group[1][(2 * k + 1) // 5, (2 * k + 1) % 5]
        take(own, 12 * pad(m_g), 12 * pad(m_g), 2 * m_g)
        take(group[2], 1, 1, 2 * m_g)
        take(group[3][:2 * m_g], 2 * m_g, pad(2 * m_g), h1)
        take(group[3][2 * m_g:], p, pad(p), h1)
        take(group[4], 1, 1, h1)
        take(group[5], h1, pad(h1), h2)
        take(group[6], 1, 1, h2)
        take(group[7], h2, pad(h2), 2 * m_g)
        take(group[8], 1, 1, 2 * m_g)
        full = np.zeros((25, pad(c_g), 2 * m_g), np.float32)
        for k in range(25):                                                   # packed tap k is window element k
            if c_g:
                full[k, :c_g] = group[0][k // 5, k % 5]
        take(full, 25 * pad(c_g), 25 * pad(c_g), 2 * m_g)
        want = np.concatenate(blocks)
        buf = params.packed(g, "cpu").numpy()
        assert buf.size == want.size == params.packed_floats(g)
        assert np.array_equal(buf, want), g
        c_g += m_g
    assert scctx_ops.ALL_TAPS == scctx_ref.ALL_TAPS and len(scctx_ops.ALL_TAPS) == 25
    assert list(scctx_ops.ALL_TAPS) == sorted(scctx_ops.ALL_TAPS)                                # row-major


def test_default_groups_and_hidden_widths():
    assert scctx_ops.default_groups(192) == (16, 16, 32, 64, 64)
    assert scctx_ops.default_groups(320) == (16, 16, 32, 64, 192)
    assert scctx_ops.default_groups(16) == (16,) and scctx_ops.default_groups(40) == (16, 16, 8)
    assert scctx_ops.default_groups(128) == (16, 16, 32, 64) and scctx_ops.default_groups(5) == (5,)
    for m in (8, 16, 192):
        assert scctx_ops.hidden_widths(m, 2 * m) == (10 * m // 3, 8 * m // 3)                  # mbt2018's
    assert scctx_ops.hidden_widths(64, 384) == (384, 256)
    assert scctx_ops.hidden_widths(64, 384) == scctx_ref.hidden_widths(64, 384)


def _zero_params(groups, p):
    out, c_g = [], 0
    for m_g in groups:
        h1, h2 = scctx_ops.hidden_widths(m_g, p)
        out.append((torch.zeros(5, 5, c_g, 2 * m_g) if c_g else None, torch.zeros(5, 5, m_g, 2 * m_g),
                    torch.zeros(2 * m_g), torch.zeros(2 * m_g + p, h1), torch.zeros(h1), torch.zeros(h1, h2),
                    torch.zeros(h2), torch.zeros(h2, 2 * m_g), torch.zeros(2 * m_g)))
        c_g += m_g
    return scctx_ops.SpaceChannelParams(out, NUM_SCALES)


def test_fits_kernel_is_the_lds_check_per_group():
    assert _zero_params((16, 16, 32, 64, 64), 384).fits_kernel()                  # the default groups at M = 192
    wide = _zero_params((16, 16, 32, 64, 192), 640)                               # ELIC's last group at M = 320
    assert not wide.fits_kernel()
    assert [own.fits_kernel() for own in wide.own] == [True, True, True, True, False]
    with pytest.raises(ValueError, match="does not fit the kernel"):
        scctx_ops._steps(wide, "cpu", [4])


def test_argument_errors_are_text():
    shape = (1, 2, 3, (2, 3), 64)
    y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
    groups = [tuple(None if w is None else torch.from_numpy(w) for w in group) for group in weights]
    params = scctx_ops.SpaceChannelParams(groups, NUM_SCALES)
    assert params.groups == (2, 3) and params.offsets == [0, 2] and (params.m, params.p) == (5, 10)
    with pytest.raises(ValueError, match=r"kernel_ch of group 1 must be \[5, 5, 2, 6\]"):
        scctx_ops.SpaceChannelParams([groups[0], (groups[1][0][:, :, :1],) + groups[1][1:]], NUM_SCALES)
    with pytest.raises(ValueError, match="group 0 has no earlier groups"):
        scctx_ops.SpaceChannelParams([(torch.zeros(5, 5, 1, 4),) + groups[0][1:]], NUM_SCALES)
    with pytest.raises(ValueError, match=r"kernel must be \[5, 5, M, 2M\]"):
        scctx_ops.SpaceChannelParams([(None, groups[0][1][:3]) + groups[0][2:]], NUM_SCALES)
    with pytest.raises(ValueError, match="num_scales"):
        scctx_ops.SpaceChannelParams(groups, 0)
    with pytest.raises(ValueError, match="stream_positions must be an integer >= 1"):
        scctx_ops.SpaceChannelParams(groups, NUM_SCALES, 0)
    with pytest.raises(ValueError, match="at least one group"):
        scctx_ops.SpaceChannelParams([], NUM_SCALES)
    yt, pt = torch.from_numpy(y), torch.from_numpy(psi)
    with pytest.raises(ValueError, match="psi must be"):
        scctx_ops.scctx_scan(yt, pt[..., :-1], params)
    with pytest.raises(ValueError, match="y must be"):
        scctx_ops.scctx_scan(yt[..., :-1], pt, params)
    with pytest.raises(ValueError, match="share"):
        scctx_ops.scctx_scan(yt[:, :1], pt, params)
    with pytest.raises(ValueError, match="pass_ must be 0 or 1"):
        scctx_ops.scctx_parameters(yt, pt, params, 0, 2)
    with pytest.raises(ValueError, match=r"g must be in \[0, 2\)"):
        scctx_ops.scctx_parameters(yt, pt, params, 2, 0)
    checker = checkerboard_ops.CheckerboardParams(*groups[0][1:], NUM_SCALES)
    with pytest.raises(TypeError, match="SpaceChannelParams"):
        scctx_ops.scctx_scan(yt, pt, checker)
    with pytest.raises(ValueError, match="needs float32 psi on the device"):
        scctx_ops.scctx_decode([[b""] * 4], pt, params, None)
    with pytest.raises(ValueError, match="sym and mu must be"):
        scctx_ops.scctx_place(torch.zeros(1, 2, 3), torch.zeros(1, 3, 3), torch.zeros(1, 2, 3, 5), 2, 0)
    with pytest.raises(ValueError, match="inside the latent"):
        scctx_ops.scctx_place(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3), torch.zeros(1, 2, 3, 5), 3, 0)
    # place on CPU tensors is the definition's store
    y_hat = torch.zeros(1, 2, 3, 5)
    scctx_ops.scctx_place(torch.full((1, 3, 3), 2.0), torch.full((1, 3, 3), 0.25), y_hat, 2, 1)
    anchors = checkerboard_ops.anchor_mask(2, 3)
    assert bool((y_hat[:, ~anchors, 2:] == 2.25).all()) and bool((y_hat[:, anchors] == 0).all())
    assert bool((y_hat[..., :2] == 0).all())


def test_c_abi_argument_errors_need_no_device():
    """tfc_scctx_params / _place check their arguments on the host before any launch."""
    from compression_amd import _lib
    lib = _lib.lib()
    _, _, weights = scctx_ref.make_case((1, 1, 2, (3, 5), 64), NUM_SCALES)
    params = params_of(weights, torch.float32)
    n = params.packed(1, "cpu").numel()
    h1, h2 = scctx_ref.hidden_widths(5, 16)
    args = lambda **kw: [kw.get("pass_", 0), None, None, None, None, kw.get("n", n), kw.get("batch", 1), kw.get("hl", 1),
                         kw.get("wl", 2), kw.get("m", 8), kw.get("cg", 3), kw.get("mg", 5), 16, h1, h2, NUM_SCALES, None,
                         None, None, None, None]
    assert lib.tfc_scctx_params(*args(n=3)) != 0 and "packed weights" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(n=params.packed(0, "cpu").numel())) != 0 and "packed weights" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(pass_=2)) != 0 and "pass must be 0 or 1" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(cg=4)) != 0 and "inside the latent" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(mg=0)) != 0 and "inside the latent" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(cg=-1)) != 0 and "inside the latent" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(m=0)) != 0 and "M must be in" in _lib.last_error()
    assert lib.tfc_scctx_params(*args()) != 0 and "must not be null" in _lib.last_error()
    assert lib.tfc_scctx_params(*args(batch=0)) == 0                             # nothing to do
    assert lib.tfc_scctx_params(*args(pass_=1, wl=1)) == 0                       # a 1x1 latent has no second pass
    wide = _zero_params((16, 16, 32, 64, 192), 640)
    own = wide.own[4]
    rc = lib.tfc_scctx_params(0, None, None, None, None, wide.packed_floats(4), 1, 1, 2, 320, 128, 192, 640, own.h1,
                              own.h2, NUM_SCALES, None, None, None, None, None)
    assert rc != 0 and "160 KiB" in _lib.last_error()
    assert lib.tfc_scctx_place(3, None, None, None, 1, 1, 2, 8, 3, 5, None) != 0 and "pass must be" in _lib.last_error()
    assert lib.tfc_scctx_place(0, None, None, None, 1, 1, 2, 8, 4, 5, None) != 0 and "inside the latent" in _lib.last_error()
    assert lib.tfc_scctx_place(0, None, None, None, 1, 1, 2, 8, 3, 5, None) != 0 and "must not be null" in _lib.last_error()
    assert lib.tfc_scctx_place(0, None, None, None, 0, 1, 2, 8, 3, 5, None) == 0


def test_shared_shapes_spread_over_the_tables_and_hold_escapes_in_every_group():
    """What the module docstring of scctx_ref.py records."""
    for shape, (tables, per_group, finite) in zip(SHAPES, scctx_ref.describe_shapes(NUM_SCALES)):
        y, _, _ = scctx_ref.make_case(shape, NUM_SCALES)
        assert tables >= 8, shape
        for c, m_g in zip(scctx_ref.offsets(shape[3]), shape[3]):
            assert (np.abs(y[..., c:c + m_g]) == scctx_ref.ESCAPE_VALUE).any(), (shape, c)
        assert finite, shape
