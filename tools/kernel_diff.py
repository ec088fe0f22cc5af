#!/usr/bin/env python
"""Compares the gfx950 device code of two builds, kernel by kernel: the evidence a refactor needs that it moved no
instruction.  Each side is a libtfc_hip.so or a build/ directory of objects.  The code objects come out of the clang
offload bundles (check_scratch.code_objects) and go through the ROCm tree's `llvm-objdump -d`; the listing is split at
the symbol labels, and addresses, raw encodings and `//` comments are dropped (a branch's comment carries an absolute
address, which moves when a neighbour disappears).  Code objects are not compared by hash: clang puts a
__hip_cuid_<hash of the source> symbol into each, so a host-only edit changes the hash and nothing else.
Prints the symbols present on one side only, those whose instruction text differs and the kernels whose
check_scratch.scan record differs; exit status 0 when all three lists are empty.  Runs nothing on a GPU.
Usage: python tools/kernel_diff.py OLD NEW [name substring ...]"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_scratch  # noqa: E402

LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def objdump():
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        exe = os.path.join(d, "llvm-objdump")
        if os.path.exists(exe):
            return exe
    return shutil.which("llvm-objdump")


def files(path):
    return sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]


def parse(listing):
    """`llvm-objdump -d` text -> {symbol: [instruction, ...]} without addresses, encodings and comments."""
    out, cur = {}, None
    for line in listing.splitlines():
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line[:1] in (" ", "\t"):
            text = " ".join(line.split("//")[0].split())
            if text:
                cur.append(text)
    return out


def listing(path):
    """{symbol: [instruction, ...]} over every gfx950 code object of a library or a directory of objects.  A symbol that
    several code objects define (a static kernel of a shared header) keeps all its texts, one behind the other."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "co.elf")
        for f in files(path):
            for elf in check_scratch.code_objects(open(f, "rb").read()):
                with open(co, "wb") as fh:
                    fh.write(elf)
                text = subprocess.run([objdump(), "-d", co], check=True, capture_output=True, text=True).stdout
                for name, ins in parse(text).items():
                    out.setdefault(name, []).extend(["--"] + ins)
    return out


def metadata(path):
    out = {}
    for f in files(path):
        out.update(check_scratch.scan(f))
    return out


def compare(old, new):
    """-> (names on one side only, names on both sides whose values differ), each sorted"""
    return sorted(set(old) ^ set(new)), sorted(n for n in set(old) & set(new) if old[n] != new[n])


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    subs = argv[2:]
    keep = lambda table: {n: v for n, v in table.items() if not subs or any(s in n for s in subs)}  # noqa: E731
    old, new = keep(listing(argv[0])), keep(listing(argv[1]))
    only, text = compare(old, new)
    _, meta = compare(keep(metadata(argv[0])), keep(metadata(argv[1])))
    print(f"{len(old)} / {len(new)} symbols compared")
    for title, names in (("present on one side only", [("old  " if n in old else "new  ") + n for n in only]),
                         ("instruction text differs", text), ("metadata differs", meta)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("  " + n)
    return 1 if only or text or meta else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
