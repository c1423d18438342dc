#!/usr/bin/env python3
"""Byte identity of every kernel of libmlgnn.so across a source change (device-only compile, no GPU needed):
    python tools/kernel_bytes.py > new.txt          one line per kernel: name, code bytes, sha256 of the code,
                                                    sha256 of the 64-byte descriptor, translation unit
    python tools/kernel_bytes.py --diff old.txt new.txt
The descriptor is hashed with bytes 16-23 zeroed: they hold the entry offset, which depends on where the function
sits in its code object.  --diff lists kernels added, removed, defined twice or changed and exits non-zero on any."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multilevel-gnn_amd")
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def kernels_of(bn, src, tmp):
    """[(name, size, code sha256, descriptor sha256)] of one translation unit"""
    co = os.path.join(tmp, os.path.basename(src)[:-4] + ".co")
    subprocess.check_call([bn.HIPCC] + bn.FLAGS + bn.FILE_FLAGS.get(os.path.basename(src), []) +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + bn.CSRC, "--offload-device-only",
                           "--no-gpu-bundle-output", "-c", src, "-o", co])
    text = subprocess.run([READELF, "-sSW", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    secs, syms = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", line)
        if m:
            secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))      # address, file offset
        m = re.match(r"\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)", line)
        if m:
            syms[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(4)))
    blob = open(co, "rb").read()

    def data(name):
        value, size, ndx = syms[name]
        at = value - secs[ndx][0] + secs[ndx][1]
        return bytearray(blob[at:at + size])

    rows = []
    for name in sorted(n[:-3] for n in syms if n.endswith(".kd") and n[:-3] in syms):
        kd = data(name + ".kd")
        assert len(kd) == 64, name
        kd[16:24] = bytes(8)
        code = data(name)
        rows.append((name, len(code), hashlib.sha256(code).hexdigest(), hashlib.sha256(kd).hexdigest()))
    return rows


def load(path):
    table = {}
    for line in open(path):
        name, size, code, kd, unit = line.split()
        table.setdefault(name, []).append((size, code, kd, unit))
    return table


def diff(old_path, new_path):
    old, new = load(old_path), load(new_path)
    bad = ["defined twice in %s: %s (%s)" % (p, k, ", ".join(d[3] for d in t[k]))
           for p, t in ((old_path, old), (new_path, new)) for k in sorted(t) if len(t[k]) > 1]
    bad += ["removed: %s (%s)" % (k, old[k][0][3]) for k in sorted(old) if k not in new]
    bad += ["added: %s (%s)" % (k, new[k][0][3]) for k in sorted(new) if k not in old]
    for k in sorted(set(old) & set(new)):
        o, n = old[k][0], new[k][0]
        if o[:2] != n[:2]:
            bad.append("code differs: %s (%s, %s bytes -> %s, %s bytes)" % (k, o[3], o[0], n[3], n[0]))
        if o[2] != n[2]:
            bad.append("descriptor differs: %s (%s -> %s)" % (k, o[3], n[3]))
    print("\n".join(bad) if bad else "%d kernels, all identical" % len(new))
    return 1 if bad else 0


def main():
    if sys.argv[1:2] == ["--diff"]:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    sys.path.insert(0, PKG)
    import build_native as bn
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as pool:
        for src, rows in zip(bn.sources(), pool.map(lambda s: kernels_of(bn, s, tmp), bn.sources())):
            for name, size, code, kd in rows:
                print(name, size, code, kd, os.path.basename(src))


if __name__ == "__main__":
    main()
