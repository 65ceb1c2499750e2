#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of osvos-pytorch_amd/csrc the same?  (Host-only refactors must answer yes.)

    tools/compare_device_code.py BUILD_DIR_A BUILD_DIR_B        # two directories holding the *.o of `make`

For every object present in either directory: dump .hip_fatbin, unbundle the hipv4-amdgcn-amd-amdhsa--gfx950 entry and compare the
disassembly (minus the lines that name the file) and the metadata notes (kernel names, argument layouts, register / LDS / scratch
use).  The raw code objects are not compared: they embed a few bytes of hash that move with any edit of the source file.  Runs
nothing on a GPU.  Exit status 0 = identical."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def device_text(obj, tmp):
    """(disassembly, notes) of the gfx950 code object inside host object `obj`; None when it has no device code."""
    tag = os.path.join(tmp, "%x_%s" % (hash(obj) & 0xffffffff, os.path.basename(obj)))
    fat, co = tag + ".hipfb", tag + ".co"
    if ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-readelf"), "-S", obj):      # a translation unit without kernels
        return None
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, tag + ".host")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", co)
    dis = "\n".join(ln for ln in dis.splitlines() if "file format" not in ln and not ln.startswith(co))
    return dis, run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)


def compare(name, dir_a, dir_b, tmp):
    pa, pb = os.path.join(dir_a, name), os.path.join(dir_b, name)
    if not (os.path.exists(pa) and os.path.exists(pb)):
        return name, "only in " + (dir_a if os.path.exists(pa) else dir_b)
    a, b = device_text(pa, tmp), device_text(pb, tmp)
    if a is None and b is None:
        return name, "no device code"
    if a is None or b is None:
        return name, "device code in one build only"
    if a[0] != b[0]:
        return name, "DISASSEMBLY DIFFERS"
    if a[1] != b[1]:
        return name, "METADATA NOTES DIFFER"
    return name, "identical (%d instruction lines)" % a[0].count("\n")


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    dir_a, dir_b = sys.argv[1:]
    names = sorted({f for d in (dir_a, dir_b) for f in os.listdir(d) if f.endswith(".o")})
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, len(names) or 1)) as pool:
        results = list(pool.map(lambda n: compare(n, dir_a, dir_b, tmp), names))
    bad = 0
    for name, verdict in results:
        ok = verdict.startswith("identical") or verdict == "no device code"
        bad += not ok
        print("%-24s %s" % (name, verdict))
    print("%d objects, %d differ" % (len(results), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
