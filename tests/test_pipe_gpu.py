"""GPU tier: the pipelined lane kernels (csrc/range_pipe.h: parallel expansion into call words + chain for
encode, chain into raw rows + parallel parse for decode) that throughput-mode handles run.  Bytes and symbols must
equal the oracle's (cc/kernels/range_coder_kernels.cc:191-322, 360-471; cc/lib/range_coder.cc:37-307) — and it must
be THESE kernels that produced them: tfc_pipe_counters tells whether the lane-per-stream fallback had to take a job.
(tests/test_range_coder_gpu.py runs every golden vector through the same kernels via the "throughput" fixture.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from compression_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tfc():
    import compression_amd
    compression_amd.set_default_mode("throughput")
    yield compression_amd
    compression_amd.set_default_mode("auto")


def counters():
    from compression_amd import _lib
    a, b = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().tfc_pipe_counters(C.byref(a), C.byref(b)))
    return a.value, b.value


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def tables(port, n, prec=12, overflow=True, octave=2.0):
    pmfs, _ = synthetic.gaussian_pmfs(num_tables=n, octave=octave)
    return synthetic.assemble_lookup([port.pmf_to_quantized_cdf(p, prec) for p in pmfs], prec, overflow=overflow)


def roundtrip(tfc, port, lookup, value, index=None, calls=1):
    """encode -> bytes == oracle; decode(oracle bytes) == value; Finalize flags true.  -> (pipelined launches,
    fallback workgroups) of the calls."""
    streams, elems = value.shape
    lt = torch.from_numpy(lookup)
    want = port.encode(lookup, value, index=index, calls=calls)[0]
    l0, f0 = counters()
    h = tfc.create_range_encoder([streams], lt)
    bounds = [elems * k // calls for k in range(calls + 1)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if index is None:
            h = tfc.entropy_encode_channel(h, dev(value[:, a:b]))
        else:
            h = tfc.entropy_encode_index(h, dev(index[:, a:b]), dev(value[:, a:b]))
    got = [bytes(x) for x in tfc.entropy_encode_finalize(h).reshape(-1)]
    assert got == want
    arr = np.empty(len(want), dtype=object)
    for i, x in enumerate(want):
        arr[i] = x
    hd = tfc.create_range_decoder(arr, lt)
    outs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        if index is None:
            hd, o = tfc.entropy_decode_channel(hd, [b - a], torch.int32)
        else:
            hd, o = tfc.entropy_decode_index(hd, dev(index[:, a:b]), [b - a], torch.int32)
        outs.append(o.cpu().numpy())
    assert (np.concatenate(outs, axis=1) == value).all()
    assert bool(tfc.entropy_decode_finalize(hd).all())
    l1, f1 = counters()
    return l1 - l0, f1 - f0


@pytest.mark.parametrize("streams,elems", [(8, 2048), (70, 1000), (64, 256), (1, 17), (130, 513), (3, 4099)])
def test_channel_mode_geometries(tfc, port, streams, elems):
    """Stream counts around the 64-stream groups, element counts around the 256-symbol tiles and 16-row blocks."""
    lookup = tables(port, 16)
    launches, fallback = roundtrip(tfc, port, lookup, synthetic.sample_symbols(lookup, streams, elems, seed=streams))
    assert launches == 2 and fallback == 0


def test_escape_codes_are_rows(tfc, port):
    """1 % of the symbols far outside their tables (second run): the Elias-gamma bits are ordinary rows
    of the chain (range_coder_kernels.cc:304-321, 449-471) — also across calls on one handle."""
    lookup = tables(port, 16)
    value = synthetic.sample_symbols(lookup, 96, 3072, seed=1, escape_fraction=0.01)
    assert roundtrip(tfc, port, lookup, value) == (2, 0)
    assert roundtrip(tfc, port, lookup, value, calls=3) == (6, 0)      # (call lengths: multiples of the table count)


def test_config2_tables(tfc, port):
    """The 192 tables of BASELINE config 2 (149 KB decoder image: one workgroup per CU), escape symbols in the data."""
    lookup = tables(port, 192, octave=24.0)
    value = synthetic.sample_symbols(lookup, 512, 4096, seed=4, escape_fraction=0.004)
    assert roundtrip(tfc, port, lookup, value) == (2, 0)


def test_tables_without_escape_rows_and_few_tables(tfc, port):
    """Positive precision headers (no escape symbol; exactly one row per symbol) and fewer tables than rows in a
    block (the channel cursor wraps several times per block)."""
    lookup = tables(port, 8, overflow=False)
    assert roundtrip(tfc, port, lookup, synthetic.sample_symbols(lookup, 40, 1111, seed=3)) == (2, 0)


def test_index_mode(tfc, port):
    """EntropyEncodeIndex / EntropyDecodeIndex (range_coder_kernels.cc:217-242, 380-404): the table of every element
    from the index tensor; values drawn through the indexed table, some of them far outside it."""
    lookup = tables(port, 16)
    rng = np.random.default_rng(5)
    index = rng.integers(0, 16, (80, 1800)).astype(np.int32)
    rows = synthetic.lookup_rows(lookup)
    u = rng.integers(0, 1 << 12, index.shape)
    value = np.zeros(index.shape, np.int32)
    for t, (_, c) in enumerate(rows):
        m = index == t
        value[m] = np.searchsorted(np.asarray(c), u[m], side="right") - 1
    assert roundtrip(tfc, port, lookup, value, index=index) == (2, 0)
    wild = np.where(rng.random(index.shape) < 0.005, rng.integers(-300, 300, index.shape) * 7, value).astype(np.int32)
    assert roundtrip(tfc, port, lookup, wild, index=index) == (2, 0)
    assert roundtrip(tfc, port, lookup, wild, index=index, calls=3) == (6, 0)


def test_more_rows_than_planned_fall_back(tfc, port):
    """Every symbol an escape with a long code: far more coder calls than the launch plans rows for.  The pipelined
    kernels leave such a job untouched and the lane-per-stream kernel behind them codes it — same bytes."""
    lookup = tables(port, 16)
    rng = np.random.default_rng(21)
    big = (rng.integers(1 << 12, 1 << 30, (4, 333)) * rng.choice([-1, 1], (4, 333))).astype(np.int32)
    launches, fallback = roundtrip(tfc, port, lookup, big)
    assert launches >= 2 and fallback >= 2      # (the encode call is repeated once with the worst-case slab)


def test_precision_16_one_digit_per_symbol(tfc, port):
    """Precision-16 rows whose plain symbols have probability 2^-16 (a 16-bit digit per symbol: the encoder's slab is
    outgrown and the call repeated with the bound that cannot be), mixed with escape codes."""
    cdf = list(range(0, 9)) + [65535, 65536]
    lookup = np.array([[-16] + cdf, [-16] + cdf], np.int32)
    rng = np.random.default_rng(77)
    u = rng.random((70, 900))
    value = np.where(u < 0.03, rng.integers(9, 2000, (70, 900)), np.where(u < 0.6, 8, rng.integers(0, 8, (70, 900)))).astype(np.int32)
    roundtrip(tfc, port, lookup, value)


def test_many_handles_in_one_launch(tfc, port):
    """tfc_encoder_encode_many / tfc_decoder_decode_many: several 512-stream batches as one launch per stage."""
    lookup = tables(port, 16)
    lt = torch.from_numpy(lookup)
    values = [synthetic.sample_symbols(lookup, 130, 700, seed=40 + k, escape_fraction=0.01) for k in range(5)]
    l0, f0 = counters()
    hs = tfc.create_range_encoders(5, [130], lt, deferred_errors=True)
    hs = tfc.entropy_encode_channel_many(hs, [dev(v) for v in values])
    hs = tfc.entropy_encode_finalize_device_many(hs)
    ds = tfc.create_range_decoders(hs, lt)
    ds, decoded = tfc.entropy_decode_channel_many(ds, [700], torch.int32)
    oks = tfc.entropy_decode_finalize_device_many(ds)
    for h, v, d, ok in zip(hs, values, decoded, oks):
        assert [bytes(s) for s in tfc.fetch_strings(h)] == port.encode(lookup, v)[0]
        assert (d.cpu().numpy().reshape(130, 700) == v).all() and bool(ok.all())
    l1, f1 = counters()
    assert (l1 - l0, f1 - f0) == (2, 0)


@pytest.mark.parametrize("streams,elems", [(4096, 700), (4100, 333)])
def test_large_launches_take_the_overlapped_path(tfc, port, streams, elems):
    """64 groups and more: the encoder's chain workgroups (a chain wave, two loader waves and a storer wave per group)
    run on the library's own stream beside the expansion, the decoder's parse beside its chain with a second pass
    behind it (csrc/range_pipe.h).  Same bytes, same symbols, no fallback — with escape codes in the data, a last
    group that is not full and element counts that end inside a tile, an iteration and a block."""
    lookup = tables(port, 16)
    value = synthetic.sample_symbols(lookup, streams, elems, seed=streams, escape_fraction=0.01)
    assert roundtrip(tfc, port, lookup, value) == (2, 0)


def test_large_launch_of_many_handles_in_index_mode(tfc, port):
    """Ten 512-stream handles behind one launch per stage (80 groups), EntropyEncodeIndex / EntropyDecodeIndex with
    values far outside the tables in between."""
    lookup = tables(port, 16)
    lt = torch.from_numpy(lookup)
    rng = np.random.default_rng(9)
    rows = synthetic.lookup_rows(lookup)
    values, indexes = [], []
    for k in range(10):
        index = rng.integers(0, 16, (512, 520)).astype(np.int32)
        u = rng.integers(0, 1 << 12, index.shape)
        value = np.zeros(index.shape, np.int32)
        for t, (_, c) in enumerate(rows):
            m = index == t
            value[m] = np.searchsorted(np.asarray(c), u[m], side="right") - 1
        value = np.where(rng.random(index.shape) < 0.004, rng.integers(-300, 300, index.shape) * 5, value).astype(np.int32)
        values.append(value)
        indexes.append(index)
    from compression_amd import _lib
    l0, f0 = counters()
    hs = tfc.create_range_encoders(10, [512], lt, deferred_errors=True)
    keep = [(dev(i), dev(v)) for i, v in zip(indexes, values)]
    hp = (C.c_void_p * 10)(*[h.ptr for h in hs])
    ip = (C.c_void_p * 10)(*[i.data_ptr() for i, _ in keep])
    vp = (C.c_void_p * 10)(*[v.data_ptr() for _, v in keep])
    _lib.check(_lib.lib().tfc_encoder_encode_many(10, hp, vp, ip, 520, _lib.stream_ptr()))
    hs = tfc.entropy_encode_finalize_device_many(hs)
    ds = tfc.create_range_decoders(hs, lt)
    outs = [torch.empty(512, 520, dtype=torch.int32, device="cuda") for _ in range(10)]
    dp = (C.c_void_p * 10)(*[d.ptr for d in ds])
    op = (C.c_void_p * 10)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.lib().tfc_decoder_decode_many(10, dp, ip, op, 520, _lib.stream_ptr()))
    oks = tfc.entropy_decode_finalize_device_many(ds)
    for h, v, i, o, ok in zip(hs, values, indexes, outs, oks):
        assert [bytes(s) for s in tfc.fetch_strings(h)] == port.encode(lookup, v, index=i)[0]
        assert (o.cpu().numpy() == v).all() and bool(ok.all())
    l1, f1 = counters()
    assert (l1 - l0, f1 - f0) == (2, 0), (l1 - l0, f1 - f0)


def test_more_groups_than_the_chip_hosts_at_once(tfc, port):
    """40 handles of 512 streams behind one call per direction = 320 groups: a launch takes only as many batches as its
    chain workgroups can be resident at once (an encoder chain workgroup per 2 groups on at most half the CUs, a decoder
    chain workgroup per CU at most), so the call is several launches — and none of them leaves a job to the fallback.
    (Round 5: with two rounds of chain workgroups in ONE launch the parse next to the chain was abandoned mid-way, and
    workgroups that started at that moment went on with some of their threads: wrong elements for 16-64 streams of a
    tile.)  Every batch's bytes against the oracle, every element back."""
    lookup = tables(port, 16)
    lt = torch.from_numpy(lookup)
    n = 40
    values = [synthetic.sample_symbols(lookup, 512, 600, seed=900 + k, escape_fraction=0.01) for k in range(n)]
    l0, f0 = counters()
    hs = tfc.create_range_encoders(n, [512], lt, deferred_errors=True)
    hs = tfc.entropy_encode_channel_many(hs, [dev(v) for v in values])
    hs = tfc.entropy_encode_finalize_device_many(hs)
    ds = tfc.create_range_decoders(hs, lt)
    ds, decoded = tfc.entropy_decode_channel_many(ds, [600], torch.int32)
    oks = tfc.entropy_decode_finalize_device_many(ds)
    for k, (h, v, d, ok) in enumerate(zip(hs, values, decoded, oks)):
        assert (d.cpu().numpy().reshape(512, 600) == v).all() and bool(ok.all()), k
        if k % 8 == 0:
            assert [bytes(s) for s in tfc.fetch_strings(h)] == port.encode(lookup, v)[0], k
    l1, f1 = counters()
    assert l1 - l0 >= 3 and f1 - f0 == 0, (l1 - l0, f1 - f0)


# The split that only the temp budget causes: TFC_PIPE_TEMP_MB is read once per process, so a child process.  Three runs of
# 20 handles (64 streams x 256 elements, 1 % escape codes): eager handles (each backs its coder states up before the
# launch that codes it), deferred handles, and index mode through the raw `*_many` entries.  The child prints, per run,
# the pipelined launches and fallback workgroups of the encode call and of the decode call.
_TEMP_SPLIT = """
import ctypes as C
import json
import sys
import numpy as np
import torch
import compression_amd as tfc
from compression_amd import _lib
sys.path.insert(0, sys.argv[2])
from test_pipe_gpu import counters, dev
z = np.load(sys.argv[1], allow_pickle=True)
lookup, n = z["lookup"], int(z["n"])
streams, elems = z["value0"].shape
lt = torch.from_numpy(lookup)
tfc.set_default_mode("throughput")
lib, st = _lib.lib(), _lib.stream_ptr()
ptrs = lambda xs: (C.c_void_p * n)(*xs)
counts = []
for run in ("eager", "deferred", "indexed"):
    values = [z["%s%d" % ("ivalue" if run == "indexed" else "value", k)] for k in range(n)]
    strings = [[bytes(x) for x in z["%s%d" % ("istrings" if run == "indexed" else "strings", k)]] for k in range(n)]
    l0, f0 = counters()
    hs = tfc.create_range_encoders(n, [streams], lt, deferred_errors=run != "eager")
    if run == "indexed":
        keep = [(dev(z["index%d" % k]), dev(v)) for k, v in enumerate(values)]
        ip = ptrs([i.data_ptr() for i, _ in keep])
        _lib.check(lib.tfc_encoder_encode_many(n, ptrs([h.ptr for h in hs]), ptrs([v.data_ptr() for _, v in keep]), ip,
                                               elems, st))
    else:
        hs = tfc.entropy_encode_channel_many(hs, [dev(v) for v in values])
    torch.cuda.synchronize()
    l1, f1 = counters()
    hs = tfc.entropy_encode_finalize_device_many(hs)
    ds = tfc.create_range_decoders(hs, lt)
    l2, f2 = counters()
    if run == "indexed":
        decoded = [torch.empty(streams, elems, dtype=torch.int32, device="cuda") for _ in range(n)]
        _lib.check(lib.tfc_decoder_decode_many(n, ptrs([d.ptr for d in ds]), ip, ptrs([o.data_ptr() for o in decoded]),
                                               elems, st))
    else:
        ds, decoded = tfc.entropy_decode_channel_many(ds, [elems], torch.int32)
    oks = tfc.entropy_decode_finalize_device_many(ds)
    torch.cuda.synchronize()
    l3, f3 = counters()
    for k in range(n):
        assert [bytes(s) for s in tfc.fetch_strings(hs[k])] == strings[k], (run, k, "bytes differ")
        assert np.array_equal(decoded[k].cpu().numpy().reshape(streams, elems), values[k]), (run, k, "symbols differ")
        assert bool(oks[k].all()), (run, k, "Finalize")
    counts.append([l1 - l0, f1 - f0, l3 - l2, f3 - f2])
print("SPLIT", json.dumps(counts))
"""


def test_launches_split_by_the_temp_budget(port, tmp_path):
    """TFC_PIPE_TEMP_MB=1: a job's temporaries are ~116 KB (encode) / ~112 KB (decode, + 32 KB of row addresses in
    index mode), so 20 handles behind one call go out as 9 + 9 + 2 jobs (7 + 7 + 6 for the indexed decode): three
    pipelined launches per direction where the chip alone would host all 20 in one.  Bytes against the oracle, every
    element back, every Finalize flag, for eager handles (whose pre-call state backups are indexed across the launches),
    deferred handles and index mode; and the launch and fallback counts are what the library gave before the launch plans
    moved to range_plan.h: three launches each way and no fallback, except in the indexed encode, where one stream of
    handle 14 takes 472 coder calls against the 448 rows planned (256 + 128 + 64) and its job, the sixth of the second
    launch, goes to the lane-per-stream kernel under its own fallback flag."""
    lookup = tables(port, 16)
    n, streams, elems = 20, 64, 256
    rng = np.random.default_rng(31)
    rows = synthetic.lookup_rows(lookup)
    arrays = {"lookup": lookup, "n": np.int64(n)}
    for k in range(n):
        value = synthetic.sample_symbols(lookup, streams, elems, seed=700 + k, escape_fraction=0.01)
        # (index mode: values drawn through the indexed table, 1 % of them far outside it)
        index = rng.integers(0, 16, value.shape).astype(np.int32)
        u = rng.integers(0, 1 << 12, index.shape)
        ivalue = np.zeros(index.shape, np.int32)
        for t, (_, c) in enumerate(rows):
            m = index == t
            ivalue[m] = np.searchsorted(np.asarray(c), u[m], side="right") - 1
        ivalue = np.where(rng.random(index.shape) < 0.01, rng.integers(-300, 300, index.shape) * 5, ivalue).astype(np.int32)
        for name, strings in (("strings", port.encode(lookup, value)[0]),
                              ("istrings", port.encode(lookup, ivalue, index=index)[0])):
            arr = np.empty(len(strings), dtype=object)
            for i, x in enumerate(strings):
                arr[i] = x
            arrays["%s%d" % (name, k)] = arr
        arrays["value%d" % k], arrays["ivalue%d" % k], arrays["index%d" % k] = value, ivalue, index
    np.savez(tmp_path / "cases.npz", **arrays)
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, TFC_PIPE_TEMP_MB="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _TEMP_SPLIT, str(tmp_path / "cases.npz"), here], cwd=root, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    tag, _, text = r.stdout.strip().rpartition("\n")[2].partition(" ")
    assert tag == "SPLIT", r.stdout[-1000:]
    counts = json.loads(text)
    print("pipelined launches / fallback workgroups (encode, decode) per run:", counts)
    assert all(c[0] > 1 and c[2] > 1 for c in counts), counts
    assert counts == [[3, 0, 3, 0], [3, 0, 3, 0], [3, 1, 3, 0]], counts


@pytest.fixture(params=[1, 2], ids=["full", "compact"])
def pipe_format(request):
    """The chain's image for the decode launches of a test: 1 full, 2 compact (tfc_set_pipe_format)."""
    from compression_amd import _lib
    prev = _lib.lib().tfc_set_pipe_format(request.param, 0)
    assert prev >= 0
    yield request.param
    _lib.lib().tfc_set_pipe_format(prev, 0)


DTYPE_CODE = {"float32": (torch.float32, 0), "bfloat16": (torch.bfloat16, 1), "float16": (torch.float16, 2)}


@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("form", ["int32", "int32-indexed", "float32", "bfloat16", "float16", "float32-indexed",
                                  "bfloat16-indexed"])
def test_many_entries_match_single_entries(tfc, port, pipe_format, form, n):
    """Every `*_many` entry of the C ABI against its single-handle entry on the same inputs: per handle the same strings,
    the same decoded values and the same Finalize flags.  n = 65 crosses the 64-job grouping of the channel forms that
    quantise / dequantise."""
    from compression_amd import _lib
    lib, st = _lib.lib(), _lib.stream_ptr()
    ntab, streams, elems = 12, 64, 300
    lookup = tables(port, ntab)
    lt = torch.from_numpy(lookup)
    rng = np.random.default_rng(n)
    dtype, indexed = form.split("-")[0], form.endswith("-indexed")
    ptrs = lambda xs: (C.c_void_p * n)(*xs)                      # noqa: E731
    index = [rng.integers(0, ntab, (streams, elems)).astype(np.int32) for _ in range(n)] if indexed else [None] * n
    syms = [synthetic.sample_symbols(lookup, streams, elems, seed=100 * n + k, escape_fraction=0.01) for k in range(n)]
    di = [dev(i) if indexed else None for i in index]
    ip = [i.data_ptr() if indexed else None for i in di]
    cdf_offset = np.arange(ntab, dtype=np.int32) % 5 - 7
    qoffset = None if indexed or dtype == "int32" else rng.uniform(-0.4, 0.4, ntab).astype(np.float32)
    d_cdf = dev(cdf_offset)
    d_q = None if qoffset is None else dev(qoffset, torch.float32)
    qp = None if d_q is None else d_q.data_ptr()
    if dtype == "int32":
        xs = [dev(s) for s in syms]
    else:
        tdtype, code = DTYPE_CODE[dtype]
        tab = [i if indexed else np.broadcast_to(np.arange(elems) % ntab, (streams, elems)) for i in index]
        xs = [dev(s + cdf_offset[t] + (0 if qoffset is None else qoffset[t]), torch.float32).to(tdtype)
              for s, t in zip(syms, tab)]

    def encode(many):
        hs = [tfc.create_range_encoder([streams], lt) for _ in range(n)]
        if dtype == "int32" and many:
            _lib.check(lib.tfc_encoder_encode_many(n, ptrs([h.ptr for h in hs]), ptrs([x.data_ptr() for x in xs]),
                                                   ptrs(ip) if indexed else None, elems, st))
        elif dtype == "int32":
            for h, x, i in zip(hs, xs, ip):
                _lib.check(lib.tfc_encoder_encode(h.ptr, x.data_ptr(), i, elems, st))
        elif indexed and many:
            _lib.check(lib.tfc_encoder_encode_quantized_indexed_many(
                n, ptrs([h.ptr for h in hs]), ptrs([x.data_ptr() for x in xs]), code, ptrs(ip), d_cdf.data_ptr(), elems,
                st))
        elif indexed:
            for h, x, i in zip(hs, xs, ip):
                _lib.check(lib.tfc_encoder_encode_quantized_indexed(h.ptr, x.data_ptr(), code, i, d_cdf.data_ptr(),
                                                                    elems, st))
        elif many:
            _lib.check(lib.tfc_encoder_encode_quantized_many(
                n, ptrs([h.ptr for h in hs]), ptrs([x.data_ptr() for x in xs]), code, qp, d_cdf.data_ptr(), ntab, elems,
                st))
        else:
            for h, x in zip(hs, xs):
                _lib.check(lib.tfc_encoder_encode_quantized(h.ptr, x.data_ptr(), code, qp, d_cdf.data_ptr(), ntab,
                                                            elems, st))
        return [[bytes(s) for s in tfc.entropy_encode_finalize(h).reshape(-1)] for h in hs]

    strings = encode(many=False)
    assert encode(many=True) == strings
    if dtype == "int32" and not indexed:
        assert strings[0] == port.encode(lookup, syms[0])[0]

    def decode(many):
        ds = []
        for s in strings:
            arr = np.empty(len(s), dtype=object)
            for i, x in enumerate(s):
                arr[i] = x
            ds.append(tfc.create_range_decoder(arr, lt))
        outs = [torch.empty((streams, elems), dtype=xs[0].dtype, device="cuda") for _ in range(n)]
        dp, op = ptrs([d.ptr for d in ds]), ptrs([o.data_ptr() for o in outs])
        if dtype == "int32" and many:
            _lib.check(lib.tfc_decoder_decode_many(n, dp, ptrs(ip) if indexed else None, op, elems, st))
        elif dtype == "int32":
            for d, i, o in zip(ds, ip, outs):
                _lib.check(lib.tfc_decoder_decode(d.ptr, i, o.data_ptr(), elems, st))
        elif indexed and many:
            _lib.check(lib.tfc_decoder_decode_dequantized_indexed_many(n, dp, ptrs(ip), op, code, d_cdf.data_ptr(),
                                                                       elems, st))
        elif many:
            _lib.check(lib.tfc_decoder_decode_dequantized_many(n, dp, op, code, qp, d_cdf.data_ptr(), ntab, elems, st))
        else:
            for d, i, o in zip(ds, ip, outs):
                _lib.check(lib.tfc_decoder_decode_dequantized(d.ptr, i, o.data_ptr(), code, qp, d_cdf.data_ptr(), ntab,
                                                              elems, st))
        oks = [tfc.entropy_decode_finalize(d) for d in ds]
        return outs, oks

    want, want_ok = decode(many=False)
    got, got_ok = decode(many=True)
    for k in range(n):
        assert torch.equal(got[k], want[k]), k
        assert np.array_equal(np.asarray(got_ok[k]), np.asarray(want_ok[k])) and bool(np.asarray(want_ok[k]).all()), k
    if dtype == "int32":
        assert all(np.array_equal(w.cpu().numpy(), s) for w, s in zip(want, syms))
