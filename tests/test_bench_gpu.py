"""GPU tier: bench.py's plain line and --dump-outputs.  The plain line holds the headline alone; two runs of the same
command write the same arrays, and those arrays are the last timed step's: its input's strings (decoded by the CPU
checker) and the decoder's output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

STEPS = 3
NAMES = ["decode_ok.npy", "decoded.npy", "string_offsets.npy", "strings.npy"]


def _bench(*argv, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    dirs = [tmp_path_factory.mktemp("dump"), tmp_path_factory.mktemp("dump")]
    lines = [_bench("--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--dump-outputs", str(d)) for d in dirs]
    return lines, dirs


def test_plain_line_is_the_headline(two_runs):
    for line in two_runs[0]:
        assert line["metric"] == "Mpixels/s encode+decode round-trip (bit-exact)" and line["unit"] == "Mpixels/s"
        assert line["higher_is_better"] is True and line["dtype"] == "int32"
        assert line["steps"] == STEPS and line["value"] > 0 and line["ms_per_step"] > 0
        for key in ("cpu_baseline", "single_batch", "roofline", "gdn_fwd", "models", "saturation"):
            assert key not in line, key


def test_dumped_outputs_repeat_and_are_the_last_step(two_runs, port):
    import bench
    (_, _), (a, b) = two_runs
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == NAMES
    total = 0
    for name in NAMES:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype in (np.float32, np.float64), name
        np.testing.assert_array_equal(x, y, err_msg=name)
        total += os.path.getsize(a / name)
    assert total <= 64e6

    offsets = np.load(a / "string_offsets.npy").astype(np.int64)
    strings = np.load(a / "strings.npy")
    assert offsets.shape == (bench.STREAMS + 1,) and offsets[0] == 0 and strings.size == offsets[-1]
    assert np.load(a / "decode_ok.npy").all()
    # the last step coded slot (STEPS - 1) % inflight of the headline's inputs (inflight = STEPS here)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lookup = bench.build_tables(device)
    value = bench.sample_symbols_device(lookup, STEPS - 1, device).cpu().numpy()
    blob = strings.astype(np.uint8).tobytes()
    decoded, ok = port.decode(lookup, [blob[offsets[i]:offsets[i + 1]] for i in range(bench.STREAMS)], bench.ELEMS,
                              threads=8)
    assert ok.all() and np.array_equal(decoded, value)
    np.testing.assert_array_equal(np.load(a / "decoded.npy"), bench.dump_sample(value, 1 << 19, seed=1))
