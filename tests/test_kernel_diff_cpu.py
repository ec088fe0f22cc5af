"""tools/kernel_diff.py: the built library against itself is clean, and an altered instruction is seen.  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")


@pytest.fixture(scope="module")
def kernel_diff():
    import kernel_diff
    if not os.path.exists(LIB):
        pytest.skip("libtfc_hip.so is not built")
    if not kernel_diff.objdump():
        pytest.skip("llvm-objdump not found")
    return kernel_diff


def test_library_against_itself(kernel_diff, capsys):
    assert kernel_diff.main([LIB, LIB, "noisy_normal"]) == 0
    out = capsys.readouterr().out
    for title in ("present on one side only: 0", "instruction text differs: 0", "metadata differs: 0"):
        assert title in out, out


def test_altered_instruction_is_reported(kernel_diff):
    table = {n: v for n, v in kernel_diff.listing(LIB).items() if "noisy_normal" in n}
    kernels = [n for n in table if n.endswith("_kernel") or "_kernelI" in n]
    assert len(kernels) >= 3, sorted(table)                 # forward and backward, float32 and bfloat16
    assert all(len(v) > 10 for v in table.values())
    assert not any("//" in line for v in table.values() for line in v)      # no comment (address, encoding) is left
    assert kernel_diff.compare(table, table) == ([], [])
    name = sorted(kernels)[0]
    changed = dict(table)
    changed[name] = list(table[name])
    at = next(i for i, line in enumerate(changed[name]) if line.startswith("v_"))
    changed[name][at] = changed[name][at] + " ; altered"
    assert kernel_diff.compare(table, changed) == ([], [name])
    missing = {n: v for n, v in table.items() if n != name}
    assert kernel_diff.compare(table, missing) == ([name], [])


def test_parse_drops_addresses_encodings_and_comments(kernel_diff):
    text = ("\nDisassembly of section .text:\n\n0000000000001900 <_Z1kPf>:\n"
            "\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000\n"
            "\ts_cbranch_execz 5                                          // 000000001908: BF880005 <_Z1kPf+0x20>\n"
            "\ts_endpgm                                                   // 00000000190C: BF810000\n")
    assert kernel_diff.parse(text) == {"_Z1kPf": ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_cbranch_execz 5", "s_endpgm"]}
