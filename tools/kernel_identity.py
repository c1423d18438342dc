#!/usr/bin/env python3
"""Are the device kernels of two trees the same?  (no GPU needed)
    python tools/kernel_identity.py <rev-or-dir A> <rev-or-dir B> [file.hip ...]

Every csrc/*.hip of both trees is compiled, device side only, to an unbundled gfx950 code object with build_native's flags.
Per kernel symbol the tool compares the instruction text (llvm-objdump -d, addresses and encoding comments stripped) and the
kernel's metadata entry (llvm-readelf --notes: registers, LDS, kernarg layout).  The comparison is keyed by symbol, so the
order in which templates are instantiated does not matter.  One line per file; exit status 1 on any difference.
A git revision is exported to a temporary directory; a directory is the root of a checkout."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
import build_native as bn  # noqa: E402


def llvm_tool(name):
    for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(bn.HIPCC))), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name) or name


def tree_of(arg, tmp):
    if os.path.isdir(arg):
        return os.path.abspath(arg)
    out = os.path.join(tmp, "rev_" + re.sub(r"\W", "_", arg))
    os.makedirs(out)
    tar = subprocess.run(["git", "-C", ROOT, "archive", arg, "include", "multilevel-gnn_amd/csrc"], stdout=subprocess.PIPE, check=True)
    subprocess.run(["tar", "-x", "-C", out], input=tar.stdout, check=True)
    return out


def code_object(tree, name, out):
    csrc = os.path.join(tree, "multilevel-gnn_amd", "csrc")
    cmd = [bn.HIPCC] + bn.FLAGS + bn.FILE_FLAGS.get(name, []) + ["-I" + os.path.join(tree, "include"), "-I" + csrc,
           "--cuda-device-only", "--no-gpu-bundle-output", "-w", "-c", os.path.join(csrc, name), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def kernels_of(obj):
    """{symbol: (sha256 of the instruction text, sha256 of the metadata entry, instructions)} of the kernels of one code object"""
    notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", obj], stdout=subprocess.PIPE, text=True, check=True).stdout
    by_name, entry = {}, None                 # the list under "amdhsa.kernels:", one "  - " item per kernel
    for line in notes.splitlines() + ["end:"]:
        if entry is not None and (line.startswith("  - ") or not line.startswith(" ")):
            text = "\n".join(entry)
            m = re.search(r"^\s+\.name:\s+(\S+)", text, re.M)
            if m:
                by_name[m.group(1)] = hashlib.sha256(text.encode()).hexdigest()
            entry = [line] if line.startswith("  - ") else None
        elif entry is not None:
            entry.append(line)
        elif line.startswith("amdhsa.kernels:"):
            entry = []
    dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", obj], stdout=subprocess.PIPE, text=True, check=True).stdout
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].strip())
    for lines in code.values():
        while lines and lines[-1] == "...":           # objdump's mark for the zero fill behind the last function of a section
            lines.pop()
    return {k: (hashlib.sha256("\n".join(code.get(k, [])).encode()).hexdigest(), v, len(code.get(k, []))) for k, v in by_name.items()}


def main():
    a_arg, b_arg = sys.argv[1], sys.argv[2]
    only = sys.argv[3:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = [tree_of(a_arg, tmp), tree_of(b_arg, tmp)]
        names = [sorted(f for f in os.listdir(os.path.join(t, "multilevel-gnn_amd", "csrc")) if f.endswith(".hip")) for t in trees]
        if names[0] != names[1]:
            print("the two trees have different translation units: %s" % sorted(set(names[0]) ^ set(names[1])))
            bad = 1
        files = [f for f in names[0] if f in names[1] and (not only or f in only)]
        jobs = [(i, f) for f in files for i in (0, 1)]
        with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 4))) as pool:
            objs = dict(zip(jobs, pool.map(lambda j: code_object(trees[j[0]], j[1], os.path.join(tmp, "%d_%s.co" % (j[0], j[1]))), jobs)))
        for f in files:
            ka, kb = kernels_of(objs[(0, f)]), kernels_of(objs[(1, f)])
            missing = sorted(set(ka) ^ set(kb))
            differ = sorted(k for k in set(ka) & set(kb) if ka[k][:2] != kb[k][:2])
            empty = sorted(k for k in ka if ka[k][2] == 0)
            if missing or differ or empty:
                bad = 1
                print("%-24s DIFFERENT: %d kernels in one tree only, %d differ, %d without code" % (f, len(missing), len(differ), len(empty)))
                for k in (missing + differ + empty)[:8]:
                    print("    " + k)
            else:
                print("%-24s %3d kernels identical" % (f, len(ka)))
    return bad


if __name__ == "__main__":
    sys.exit(main())
