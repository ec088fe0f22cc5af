"""CPU tier: bench.py's options that need no device — the --dump-outputs sample and where the option is refused."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_sample_is_fixed_and_in_order():
    import bench
    a = np.arange(1000, dtype=np.int32).reshape(10, 100)
    np.testing.assert_array_equal(bench.dump_sample(a, 1000, seed=1), a.reshape(-1))
    s = bench.dump_sample(a, 100, seed=1)
    assert s.shape == (100,) and len(np.unique(s)) == 100 and (np.diff(s) > 0).all()
    np.testing.assert_array_equal(s, bench.dump_sample(a, 100, seed=1))
    assert not np.array_equal(s, bench.dump_sample(a, 100, seed=2))


def test_dump_outputs_is_refused_outside_the_headline(tmp_path):
    for extra in (["--workload", "bls2017"], ["--leg", "gdn"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--dump-outputs" in r.stderr, r.stderr[-2000:]
    assert not os.listdir(tmp_path)
