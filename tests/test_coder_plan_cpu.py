"""CPU tier: compression_amd/csrc/range_plan.h (the lane path's launch plans and workspace layouts, plain functions of
numbers) compiled for the host and held to tests/coder_plan_ref.py, the transcription of what range_coder.hip computed
inline before — field by field over a grid of geometries, tables, devices and switches — and to what any layout must
satisfy: regions in bounds, disjoint, aligned, the zeroed extent exactly the flag regions, a launch's jobs within the
argument struct and the temp budget.

What this does not cover: the kernels' compile-time sizes are given as numbers (KERNELS below), so the arithmetic is
checked at those values only, and the three functions of range_coder.hip that fill the facts from the tables, the
device and the kernel headers (table_facts, device_facts, kernel_facts) are not compiled here — a field filled from the
wrong constant there would be caught by the GPU tier alone."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import coder_plan_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

# The kernels' compile-time sizes as they are today (int32 elements; EncWaveLds / DecWaveLds kBytes, kIndex; PipeDecLds
# kBytes, kRows, kStage; PipeEncChainLds kGroups, kGroup, kRows; kPipeTile, kPipeBlock, kParseRows, kExpandTabBytes).
# The job limit is 64 for int32 symbols; the quantising encoder's job struct is larger: 49.
KERNELS = dict(enc_wave_indexed=19968, enc_wave_plain=11264, dec_wave_indexed=17920, dec_wave_plain=9216,
               dec_lds_bytes=13312, dec_lds_rows=6656, dec_lds_stage=2048, enc_chain_groups=2, enc_chain_group=73792,
               enc_chain_rows=32, pipe_tile=256, pipe_block=16, parse_rows=128, expand_tab_bytes=32768)
LDS = 160 * 1024

# (lane_enc_bytes, lane_dec_bytes, pair_dec_bytes, entries): the decoder's full image fits with room for several waves /
# fits one wave per CU in channel mode and none in index mode (BASELINE config 2: 150 KB, 92 KB compact) / only the compact
# one fits (bls2017's tables: 176 KB, 115 KB) / neither fits.  The entry counts: staged in the expansion's LDS, not staged,
# too many for the pipelined encoder.
IMAGES = [(30000, 40000, 25000, 5000), (100000, 150000, 92000, 24576), (120000, 180000, 117000, 24576),
          (140000, 200000, 170000, 70000)]

TABLES = ["lane_enc_bytes", "lane_dec_bytes", "pair_dec_bytes", "pairs_ok", "any_escape", "lane_precision", "entries", "ntab"]
DEVICE = ["cus", "lds_bytes", "temp_bytes", "pipe_enabled", "format", "waves_override", "overlap", "chip_shared"]
KERNEL_IN = list(KERNELS) + ["enc_max_jobs", "dec_max_jobs"]
CALL = ["streams", "elems", "n", "indexed"]
IN = TABLES + DEVICE + KERNEL_IN + CALL

LANE = ["fits", "lds_image", "lds_wave", "block", "lds_bytes"]
ENC_PLAN = ["enabled", "nt", "rows", "groups_per_job", "job_bytes", "tab_entries", "chain_lds", "per_launch"]
DEC_PLAN = ["enabled", "pairs", "rows", "groups_per_job", "raw_bytes", "rec_bytes", "job_bytes", "lds_image", "lds_wave",
            "pblock", "plds", "tiles", "ctiles", "per_launch"]
ENC_REGIONS = ["calls", "stage_state", "stage_out", "status", "done", "fallback", "started"]
DEC_REGIONS = ["raw", "posrec", "state_out", "kend", "rowaddr", "fallback", "started", "progress", "tile_done"]
EXTENT = ["total", "zero_offset", "zero_bytes"]
LAUNCH = ["gn_enc", "overlap_enc"] + ["enc_" + k for k in ENC_REGIONS + EXTENT] + \
    ["gn_dec", "overlap_dec"] + ["dec_" + k for k in DEC_REGIONS + EXTENT]
N_OUT = 2 * len(LANE) + len(ENC_PLAN) + len(DEC_PLAN) + 1 + 2 * len(LAUNCH)

# what the kernels read a region as: uint4 coder states need 16 bytes, the rest their element; 256 where the host code
# rounded a region's start to 256
ENC_ALIGN = dict(calls=256, stage_state=16, stage_out=8, status=256, done=256, fallback=256, started=4)
DEC_ALIGN = dict(raw=256, posrec=256, state_out=256, kend=256, rowaddr=256, fallback=256, started=4, progress=4,
                 tile_done=4)
ENC_FLAGS, DEC_FLAGS = ["status", "done", "fallback", "started"], ["fallback", "started", "progress", "tile_done"]


def grid():
    """The cases: the full product of the geometries and switches, and a few facts that switch a plan off on their own."""
    for (images, escape, fmt, waves, shared, temp_mb, cus, streams, elems, n, indexed) in itertools.product(
            IMAGES, (True, False), (0, 1, 2), (0, 2), (False, True), (1, 6 * 1024), (256, 8),
            (1, 63, 64, 65, 512, 4100), (1, 17, 255, 256, 257, 4096, (1 << 29) - 1), (1, 3, 64, 65), (False, True)):
        yield dict(images=images, escape=escape, format=fmt, waves=waves, shared=shared, temp_mb=temp_mb, cus=cus,
                   streams=streams, elems=elems, n=n, indexed=indexed)
    base = dict(images=IMAGES[1], escape=True, format=0, waves=0, shared=False, temp_mb=6 * 1024, cus=256, streams=512,
                elems=4096, n=20, indexed=False)
    for extra in (dict(), dict(pairs_ok=False), dict(pairs_ok=False, images=IMAGES[2]), dict(precision=16),
                  dict(ntab=4096, indexed=True), dict(pipe_enabled=False), dict(enc_max_jobs=49, dec_max_jobs=56, n=65),
                  dict(overlap=0), dict(overlap=1, n=3)):
        yield dict(base, **extra)


def facts(case):
    enc, dec, pair, entries = case["images"]
    tables = dict(lane_enc_bytes=enc, lane_dec_bytes=dec, pair_dec_bytes=pair, pairs_ok=case.get("pairs_ok", True),
                  any_escape=case["escape"], lane_precision=case.get("precision", 12), entries=entries,
                  ntab=case.get("ntab", 192))
    device = dict(cus=case["cus"], lds_bytes=LDS, temp_bytes=case["temp_mb"] << 20,
                  pipe_enabled=case.get("pipe_enabled", True), format=case["format"], waves_override=case["waves"],
                  overlap=case.get("overlap", 2), chip_shared=case["shared"])
    kernel_in = dict(KERNELS, enc_max_jobs=case.get("enc_max_jobs", 64), dec_max_jobs=case.get("dec_max_jobs", 64))
    call = dict(streams=case["streams"], elems=case["elems"], n=case["n"], indexed=case["indexed"])
    return tables, device, kernel_in, call


def reference(tables, device, kernel_in, call):
    """Every output of coder_plan_check, from the transcription -> (flat list, per-launch region sizes)."""
    shared = {k: v for k, v in kernel_in.items() if "wave" not in k and "max_jobs" not in k}
    ke = dict(shared, lane_wave_indexed=kernel_in["enc_wave_indexed"], lane_wave_plain=kernel_in["enc_wave_plain"],
              max_jobs=kernel_in["enc_max_jobs"])
    kd = dict(shared, lane_wave_indexed=kernel_in["dec_wave_indexed"], lane_wave_plain=kernel_in["dec_wave_plain"],
              max_jobs=kernel_in["dec_max_jobs"])
    streams, elems, n, indexed = (call[k] for k in CALL)
    out = []
    lane_e = ref.lane_plan(tables, device, ke, True, streams, n, indexed)
    if lane_e["fits"]:     # (the encoder is given the lane family only where its image fits; then its own expression)
        assert lane_e["block"] == ref.encoder_block(tables, device, ke, streams, n, indexed)
    lane_d = ref.lane_plan(tables, device, kd, False, streams, n, indexed)
    out += [lane_e[k] for k in LANE] + [lane_d[k] for k in LANE]
    e = ref.enc_pipe_plan(tables, device, ke, streams, elems)
    d = ref.dec_pipe_plan(tables, device, kd, streams, elems, n, indexed)
    out += [e[k] for k in ENC_PLAN] + [d[k] for k in DEC_PLAN] + [ref.decode_fits_lanes(tables, device, kd, indexed)]
    sizes = []
    for last in (False, True):
        gn_e = n - (n - 1) // e["per_launch"] * e["per_launch"] if last else min(e["per_launch"], n)
        gn_d = n - (n - 1) // d["per_launch"] * d["per_launch"] if last else min(d["per_launch"], n)
        groups_e, groups_d = e["groups_per_job"] * gn_e, d["groups_per_job"] * gn_d
        le, se = ref.enc_layout(e, ke, groups_e)
        ld, sd = ref.dec_layout(d, kd, groups_d, gn_d, indexed, streams, elems)
        out += [gn_e, ref.launch_overlap(device, groups_e)] + [le[k] for k in ENC_REGIONS + EXTENT]
        out += [gn_d, ref.launch_overlap(device, groups_d)] + [ld[k] for k in DEC_REGIONS + EXTENT]
        sizes.append((se, sd))
    flat_sizes = [v for se, sd in sizes for v in [se[k] for k in ENC_REGIONS] + [sd[k] for k in DEC_REGIONS]]
    return [int(v) for v in out], flat_sizes, (ke["max_jobs"], kd["max_jobs"])


def check_layout(side, regions, offsets, sizes, align, flags):
    """In bounds, pairwise disjoint, aligned; the zeroed extent starts at the first flag region, ends with the workspace
    (less than a 256-byte rounding behind the last flag) and holds no other region.  Columns of all cases at once."""
    total, zero_offset, zero_bytes = (offsets[k] for k in EXTENT)
    ends = {r: offsets[r] + sizes[r] for r in regions}
    for ra, rb in itertools.combinations(regions, 2):
        apart = (ends[ra] <= offsets[rb]) | (ends[rb] <= offsets[ra])
        assert apart.all(), (side, "overlap", ra, rb, int(np.argmin(apart)))
    for r in regions:
        assert ((offsets[r] >= 0) & (ends[r] <= total)).all(), (side, "out of bounds", r)
        assert (offsets[r] % align[r] == 0).all(), (side, "alignment", r)
        inside = (zero_offset <= offsets[r]) & (ends[r] <= zero_offset + zero_bytes)
        outside = (ends[r] <= zero_offset) | (offsets[r] >= zero_offset + zero_bytes)
        assert (inside if r in flags else outside | (sizes[r] == 0)).all(), (side, "zeroed extent", r)
    assert (zero_offset == np.min([offsets[r] for r in flags], axis=0)).all(), (side, "zeroed extent starts at the flags")
    assert (zero_offset + zero_bytes == total).all(), (side, "zeroed extent ends with the workspace")
    assert (total - np.max([ends[r] for r in flags], axis=0) < 256).all(), (side, "zeroed extent ends behind the flags")


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("native") / "coder_plan_check.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so,
                    os.path.join(HERE, "native", "coder_plan_check.cc")], check=True)
    fn = C.CDLL(so).coder_plan_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def run(rows):
        rows = np.ascontiguousarray(rows, np.int64)
        out = np.zeros((len(rows), N_OUT), np.int64)
        assert fn(len(rows), rows.shape[1], N_OUT, rows.ctypes.data, out.ctypes.data) == 0
        return out
    return run


@pytest.fixture(scope="module")
def cases():
    """(inputs, reference outputs, region sizes, job limits) of every case: computed once."""
    rows, want, sizes, limits, temps = [], [], [], [], []
    for case in grid():
        tables, device, kernel_in, call = facts(case)
        rows.append([int(tables[k]) for k in TABLES] + [int(device[k]) for k in DEVICE] +
                    [int(kernel_in[k]) for k in KERNEL_IN] + [int(call[k]) for k in CALL])
        w, s, m = reference(tables, device, kernel_in, call)
        want.append(w)
        sizes.append(s)
        limits.append(m)
        temps.append(device["temp_bytes"])
    return (np.array(rows, np.int64), np.array(want, np.int64), np.array(sizes, np.int64), np.array(limits, np.int64),
            np.array(temps, np.int64))


def names():
    out = ["enc_lane." + k for k in LANE] + ["dec_lane." + k for k in LANE] + ["enc." + k for k in ENC_PLAN] + \
        ["dec." + k for k in DEC_PLAN] + ["decode_fits_lanes"]
    for which in ("first", "last"):
        out += ["%s.%s" % (which, k) for k in LAUNCH]
    return out


def test_the_header_stands_alone(tmp_path):
    """Plain C++17: g++ compiles range_plan.h with nothing else on the include path."""
    src = tmp_path / "alone.cc"
    src.write_text('#include "%s"\nint main() { return tfc::plan::lane_image_bytes(1) == 1024 ? 0 : 1; }\n'
                   % os.path.join(os.path.dirname(HERE), "compression_amd", "csrc", "range_plan.h"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(tmp_path / "alone"), str(src)], check=True)
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    text = open(os.path.join(os.path.dirname(HERE), "compression_amd", "csrc", "range_plan.h")).read()
    assert "hip/" not in text and "getenv" not in text


def test_plans_and_layouts_equal_the_transcription(native, cases):
    rows, want, _, _, _ = cases
    got = native(rows)
    cols = names()
    assert len(cols) == N_OUT == want.shape[1]
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(dict(zip(IN, rows[r].tolist())), cols[c], int(got[r, c]), int(want[r, c])) for r, c in bad[:3]]


def test_the_grid_reaches_every_branch(cases):
    """Both images and neither, plans on and off, launches split by the chip and by the budget, large and small ones."""
    _, want, _, _, _ = cases
    col = {k: want[:, i] for i, k in enumerate(names())}
    for k in ("enc.enabled", "dec.enabled", "dec.pairs", "dec_lane.fits", "decode_fits_lanes", "first.overlap_enc",
              "first.overlap_dec", "enc.tab_entries"):
        assert (col[k] != 0).any() and (col[k] == 0).any(), k
    assert ((col["dec.enabled"] != 0) & (col["dec_lane.fits"] == 0)).any()
    assert ((col["dec.enabled"] == 0) & (col["dec_lane.fits"] == 0)).any()
    assert (col["first.gn_dec"] != col["last.gn_dec"]).any() and (col["first.gn_enc"] != col["last.gn_enc"]).any()
    assert len(set(col["dec.pblock"].tolist())) >= 4


@pytest.mark.parametrize("side", ["transcription", "header"])
def test_what_every_plan_and_layout_satisfies(native, cases, side):
    rows, want, sizes, limits, temps = cases
    table = want if side == "transcription" else native(rows)
    v = {k: table[:, i] for i, k in enumerate(names())}
    for plan, kmax in zip(("enc", "dec"), limits.T):
        per_launch, job_bytes = v[plan + ".per_launch"], v[plan + ".job_bytes"]
        assert ((1 <= per_launch) & (per_launch <= kmax)).all(), (side, plan)
        assert ((v[plan + ".enabled"] == 0) | (per_launch * job_bytes <= temps) | (per_launch == 1)).all(), (side, plan)
    size_names = [w + k for w in ("first.enc_", "first.dec_", "last.enc_", "last.dec_")
                  for k in (ENC_REGIONS if "enc" in w else DEC_REGIONS)]
    size = {k: sizes[:, i] for i, k in enumerate(size_names)}
    for which in ("first", "last"):
        for plan in ("enc", "dec"):
            gn = v["%s.gn_%s" % (which, plan)]
            assert ((1 <= gn) & (gn <= v[plan + ".per_launch"])).all()
        check_layout(side, ENC_REGIONS, {k: v["%s.enc_%s" % (which, k)] for k in ENC_REGIONS + EXTENT},
                     {k: size["%s.enc_%s" % (which, k)] for k in ENC_REGIONS}, ENC_ALIGN, ENC_FLAGS)
        check_layout(side, DEC_REGIONS, {k: v["%s.dec_%s" % (which, k)] for k in DEC_REGIONS + EXTENT},
                     {k: size["%s.dec_%s" % (which, k)] for k in DEC_REGIONS}, DEC_ALIGN, DEC_FLAGS)
