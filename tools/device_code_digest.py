#!/usr/bin/env python3
"""Digest of the gfx950 device code in every object of navierstokes3d_amd/build/ (no GPU needed).

    python tools/device_code_digest.py [BUILD_DIR] > digests.txt

For each object: the .hip_fatbin section is dumped, the gfx950 code object is unbundled from it, and the sha256 of that code
object's .text and .rodata plus the sorted list of its kernel (FUNC) symbols are printed.  Two builds whose output is equal run
the same device code.  Whole code objects cannot be compared: they carry a __hip_cuid_<hash> symbol that depends on the source
path.  The sections can (profiles/device_code_digests.txt).
"""
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata")


def _tool(name):
    for d in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    exe = shutil.which(name)
    if not exe:
        raise RuntimeError(name + " not found (it comes with the ROCm LLVM tools)")
    return exe


def _sha256(path):
    if not os.path.exists(path) or os.path.getsize(path) == 0:
        return "absent"
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def digest(obj, tmp):
    """{'.text': sha256, '.rodata': sha256, 'kernels': [names]} of the gfx950 code object inside one host object"""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    if ".hip_fatbin" not in subprocess.check_output([readelf, "--section-headers", "--wide", obj]).decode():
        return None     # a unit without kernels (host code compiled with -x hip)
    subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fatbin, obj, os.path.join(tmp, "unused.o")])
    subprocess.check_call([bundler, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + co])
    out = {}
    for sec in SECTIONS:
        f = os.path.join(tmp, "sec" + sec)
        subprocess.check_call([objcopy, "--dump-section", sec + "=" + f, co, os.path.join(tmp, "unused.co")])
        out[sec] = _sha256(f)
    syms = subprocess.check_output([readelf, "--symbols", "--wide", co]).decode()
    names = set()
    for line in syms.splitlines():
        w = line.split()       # Num: Value Size Type Bind Vis Ndx Name
        if len(w) == 8 and w[3] == "FUNC" and w[6] != "UND":
            names.add(w[7])
    out["kernels"] = sorted(names)
    return out


def main(argv):
    bdir = argv[1] if len(argv) > 1 else os.path.join(HERE, "..", "navierstokes3d_amd", "build")
    objs = sorted(glob.glob(os.path.join(bdir, "*.o")))
    if not objs:
        raise SystemExit("no objects in %s: run python -m navierstokes3d_amd.build first" % bdir)
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            d = digest(obj, tmp)
        print(os.path.basename(obj))
        if d is None:
            print("  no device code")
            continue
        names = "\n".join(d["kernels"]).encode()
        for sec in SECTIONS:
            print("  %-8s sha256 %s" % (sec, d[sec]))
        print("  kernels  %d, sha256 of the sorted names %s" % (len(d["kernels"]), hashlib.sha256(names).hexdigest()))
        for n in d["kernels"]:
            print("    " + n)


if __name__ == "__main__":
    main(sys.argv)
