"""The coder's launch plans and workspace layouts as the host code computed them before they moved to
compression_amd/csrc/range_plan.h: a transcription, expression by expression, of what encode_lanes_many, decode_lanes_many
and decodes_on_lanes (csrc/range_coder.hip) did inline.  The move is held to it (tests/test_coder_plan_cpu.py).

Integers are Python's; where the C++ divided possibly negative ints, `tdiv` truncates toward zero as C++ does.  Facts
travel as dicts with the names of range_plan.h's structs:

  tables  lane_enc_bytes, lane_dec_bytes, pair_dec_bytes, pairs_ok, any_escape, lane_precision, entries, ntab
  device  cus, lds_bytes, temp_bytes, pipe_enabled, format, waves_override, overlap, chip_shared
  kernels lane_wave_indexed, lane_wave_plain (of the direction), dec_lds_bytes, dec_lds_rows, dec_lds_stage,
          enc_chain_groups, enc_chain_group, enc_chain_rows, pipe_tile, pipe_block, parse_rows, expand_tab_bytes, max_jobs
"""

SIZEOF_UINT = 4
SIZEOF_UINT2 = 8
SIZEOF_UINT4 = 16


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def ceil_div(a, b):
    return tdiv(a + b - 1, b)


def image_bytes(nbytes):
    return (nbytes + 1023) & ~1023


def lanes_block(streams):
    waves = ceil_div(streams, 64)
    per = min(8, max(1, waves // 256))
    return 64 * per


def lane_plan(tables, device, kernels, encode, streams, n, indexed):
    """-> fits, lds_image, lds_wave, block, lds_bytes.  The decoder's form; the encoder computed `block` without asking
    whether the image fits, because select_family gives it the lane family only where it does."""
    kLds = device["lds_bytes"]
    lds_image = image_bytes(tables["lane_enc_bytes"] if encode else tables["lane_dec_bytes"])
    lds_wave = kernels["lane_wave_indexed"] if indexed else kernels["lane_wave_plain"]
    lanes_fit = lds_image + lds_wave <= kLds
    block = min(lanes_block(streams * n), 64 * tdiv(kLds - lds_image, lds_wave)) if lanes_fit else 64
    lds_bytes = lds_image + (block // 64) * lds_wave
    return dict(fits=lanes_fit, lds_image=lds_image, lds_wave=lds_wave, block=block, lds_bytes=lds_bytes)


def encoder_block(tables, device, kernels, streams, n, indexed):
    """`block` exactly as encode_lanes_many had it."""
    kLds = device["lds_bytes"]
    lds_image = image_bytes(tables["lane_enc_bytes"])
    lds_wave = kernels["lane_wave_indexed"] if indexed else kernels["lane_wave_plain"]
    return min(lanes_block(streams * n), 64 * tdiv(kLds - lds_image, lds_wave))


def enc_pipe_plan(tables, device, kernels, streams, elems):
    kMaxLaneJobs = kernels["max_jobs"]
    nt = ceil_div(elems, kernels["pipe_tile"])
    rows64 = elems + (elems // 2 + 64 if tables["any_escape"] else 0)
    rows = min((rows64 + 31) // 32 * 32, 1 << 30)
    groups_per_job = ceil_div(streams, 64)
    group_bytes = rows * 256 + (SIZEOF_UINT * 65 * nt) + 64 * (SIZEOF_UINT4 + SIZEOF_UINT2)
    job_bytes = group_bytes * groups_per_job
    kPipeTempBytes = device["temp_bytes"]
    pipe = (device["pipe_enabled"] and rows64 + 2048 < (1 << 30) and job_bytes <= kPipeTempBytes and
            tables["entries"] <= 65536 and nt * groups_per_job * kMaxLaneJobs < (1 << 31))
    cus_e = device["cus"]
    resident_jobs = max(1, (cus_e // 2) * kernels["enc_chain_groups"] // max(1, groups_per_job))
    per_launch = kMaxLaneJobs if not pipe else max(1, min(min(kMaxLaneJobs, resident_jobs),
                                                           kPipeTempBytes // max(job_bytes, 1)))
    tab_entries = tables["entries"] if tables["entries"] * 2 <= kernels["expand_tab_bytes"] else 0
    return dict(enabled=bool(pipe), nt=nt, rows=rows, groups_per_job=groups_per_job, job_bytes=job_bytes,
                tab_entries=tab_entries, chain_lds=kernels["enc_chain_groups"] * kernels["enc_chain_group"],
                per_launch=per_launch)


def enc_layout(plan, kernels, groups):
    """Offsets as encode_lanes_many summed them; zeroed: from `status` to the end."""
    nt, rows = plan["nt"], plan["rows"]
    calls_bytes = (groups * 64 * rows + 64 * kernels["enc_chain_rows"]) * SIZEOF_UINT
    stage_bytes = groups * 64 * (SIZEOF_UINT4 + SIZEOF_UINT2)
    status_bytes = groups * nt * 64 * SIZEOF_UINT
    done_bytes = (groups * nt * SIZEOF_UINT + 255) & ~255
    total = calls_bytes + stage_bytes + status_bytes + done_bytes + 512
    fallback = calls_bytes + stage_bytes + status_bytes + done_bytes
    out = dict(calls=0, stage_state=calls_bytes, stage_out=calls_bytes + groups * 64 * SIZEOF_UINT4,
               status=calls_bytes + stage_bytes, done=calls_bytes + stage_bytes + status_bytes, fallback=fallback,
               started=fallback + 64 * SIZEOF_UINT, total=total, zero_offset=calls_bytes + stage_bytes,
               zero_bytes=status_bytes + done_bytes + 512)
    sizes = dict(calls=calls_bytes, stage_state=groups * 64 * SIZEOF_UINT4, stage_out=groups * 64 * SIZEOF_UINT2,
                 status=status_bytes, done=groups * nt * SIZEOF_UINT, fallback=64 * SIZEOF_UINT,
                 started=512 - 64 * SIZEOF_UINT)
    return out, sizes


def dec_chain_wave_bytes(kernels, indexed):
    return (kernels["dec_lds_bytes"] if indexed else kernels["dec_lds_rows"]) + kernels["dec_lds_stage"]


def dec_pipe_plan(tables, device, kernels, streams, elems, n, indexed):
    kMaxLaneJobs, kPipeBlock, kParseRows = kernels["max_jobs"], kernels["pipe_block"], kernels["parse_rows"]
    kLds = device["lds_bytes"]
    ntab = tables["ntab"]
    la_lds_image = image_bytes(tables["lane_dec_bytes"])
    groups_per_job = ceil_div(streams, 64)
    rows64 = ((elems + (elems // 4 + 64 + 24 * kPipeBlock if tables["any_escape"] else 2 * kPipeBlock)) + kPipeBlock - 1) \
        // kPipeBlock * kPipeBlock
    rows = min(rows64, 1 << 30)
    raw_bytes = rows * 128
    rec_bytes = (rows // kPipeBlock + 1) * 256
    group_bytes = raw_bytes + rec_bytes + 64 * SIZEOF_UINT4 + SIZEOF_UINT
    job_bytes = group_bytes * groups_per_job + (2 * streams * elems if indexed else 0)
    pla_lds_wave = dec_chain_wave_bytes(kernels, indexed)
    pla_lds_image = la_lds_image
    kPipeTempBytes = device["temp_bytes"]
    cus_d = device["cus"]
    waves_call = groups_per_job * min(n, kMaxLaneJobs)

    def waves_fit(nbytes):
        return max(0, tdiv(kLds - nbytes, pla_lds_wave))
    pair_image = image_bytes(tables["pair_dec_bytes"])
    fit_full, fit_pairs = waves_fit(pla_lds_image), (waves_fit(pair_image) if tables["pairs_ok"] else 0)
    if device["format"] == 1:
        pairs = False
    elif device["format"] == 2:
        pairs = fit_pairs >= 1
    else:
        pairs = fit_pairs >= 1 and (fit_full < 1 or 4 * waves_call > 3 * cus_d * min(fit_full, 4))
    if pairs:
        pla_lds_image = pair_image
    fit = fit_pairs if pairs else fit_full
    per = min(8, max(1, ceil_div(waves_call, cus_d)))
    if device["chip_shared"]:
        per = max(per, min(4, groups_per_job))
    if device["waves_override"] > 0:
        per = device["waves_override"]
    per = min(per, min(fit, groups_per_job))
    pblock = 64 * max(per, 0)
    tiles = rows // kParseRows + 1
    pipe = (device["pipe_enabled"] and pblock >= 64 and rows64 < (1 << 30) and job_bytes <= kPipeTempBytes and
            (not indexed or ntab < 4096) and tables["lane_precision"] <= 15 and
            tiles * groups_per_job * kMaxLaneJobs < (1 << 31))
    plds = pla_lds_image + (pblock // 64) * pla_lds_wave
    chain_wgs_per_job = ceil_div(groups_per_job, max(1, pblock // 64))
    resident_wgs = cus_d * max(1, kLds // max(1, plds))
    resident_jobs = max(1, resident_wgs // max(1, chain_wgs_per_job))
    per_launch = kMaxLaneJobs if not pipe else max(1, min(min(kMaxLaneJobs, resident_jobs),
                                                           kPipeTempBytes // max(job_bytes, 1)))
    ctiles = min(tiles, ceil_div(elems, kParseRows))
    return dict(enabled=bool(pipe), pairs=bool(pairs), rows=rows, groups_per_job=groups_per_job, raw_bytes=raw_bytes,
                rec_bytes=rec_bytes, job_bytes=job_bytes, lds_image=pla_lds_image, lds_wave=pla_lds_wave, pblock=pblock,
                plds=plds, tiles=tiles, ctiles=ctiles, per_launch=per_launch)


def dec_layout(plan, kernels, groups, gn, indexed, streams, elems):
    """Offsets as decode_lanes_many summed them; zeroed: `flags_all` bytes from `fallback`."""
    tiles = plan["rows"] // kernels["parse_rows"] + 1
    raw_all, rec_all, st_all = plan["raw_bytes"] * groups, plan["rec_bytes"] * groups, 64 * SIZEOF_UINT4 * groups
    kend_all = (SIZEOF_UINT * groups + 255) & ~255
    addr_all = ((2 * streams * elems * gn + 255) & ~255) if indexed else 0
    flags_all = (512 + SIZEOF_UINT * groups * (1 + tiles) + 255) & ~255
    fallback = raw_all + rec_all + st_all + kend_all + addr_all
    progress = fallback + 128 * SIZEOF_UINT
    out = dict(raw=0, posrec=raw_all, state_out=raw_all + rec_all, kend=raw_all + rec_all + st_all,
               rowaddr=raw_all + rec_all + st_all + kend_all, fallback=fallback, started=fallback + 64 * SIZEOF_UINT,
               progress=progress, tile_done=progress + groups * SIZEOF_UINT,
               total=raw_all + rec_all + st_all + kend_all + addr_all + flags_all, zero_offset=fallback,
               zero_bytes=flags_all)
    sizes = dict(raw=raw_all, posrec=rec_all, state_out=st_all, kend=SIZEOF_UINT * groups,
                 rowaddr=2 * streams * elems * gn if indexed else 0, fallback=64 * SIZEOF_UINT, started=64 * SIZEOF_UINT,
                 progress=SIZEOF_UINT * groups, tile_done=SIZEOF_UINT * groups * tiles)
    return out, sizes


def decode_fits_lanes(tables, device, kernels, indexed):
    """The LDS part of decodes_on_lanes (behind its select_family question)."""
    kLds = device["lds_bytes"]
    need = image_bytes(tables["lane_dec_bytes"]) + (kernels["lane_wave_indexed"] if indexed else kernels["lane_wave_plain"])
    need_pairs = image_bytes(tables["pair_dec_bytes"]) + \
        (kernels["dec_lds_bytes"] if indexed else kernels["dec_lds_rows"]) + kernels["dec_lds_stage"]
    compact_ok = tables["pairs_ok"] and device["pipe_enabled"] and device["format"] != 1 and need_pairs <= kLds
    return bool(need <= kLds or compact_ok)


def launch_overlap(device, groups):
    """(a large launch only: 64 groups and more)"""
    return device["overlap"] if groups >= 64 else 0
