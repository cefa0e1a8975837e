"""ns3d_diagnostics without a GPU: the ownership rule partitions the global index range, the ctypes mirrors of ns3d_diag /
ns3d_diag_params agree with the preprocessed header (names, order, offsets, sizes — against a C program compiled from the
header), and the built library exports the entry points."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from navierstokes3d_amd import diag as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ns3d.h")


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n", [3, 4, 5, 9, 24])
def test_ownership_partitions_the_global_range(n, P, s):
    """Rank c's array of extent n+s starts at global index c·(n−2); the global extent is P·(n−2)+2+s (IGG indexing,
    include/ns3d.h).  Every global index is owned by exactly one rank."""
    count = [0] * (P * (n - 2) + 2 + s)
    for c in range(P):
        lo_f, hi_f = D.seam_flags((P,), (c,))
        lo, hi = D.owned_range(n, s, lo_f[0], hi_f[0])
        assert 0 <= lo < hi <= n + s                    # every rank owns something, inside its array
        for i in range(lo, hi):
            count[c * (n - 2) + i] += 1
    assert count == [1] * len(count)


def test_seam_flags_and_slices():
    assert D.seam_flags((2, 1, 3), (0, 0, 1)) == ((0, 0, 1), (1, 0, 1))
    assert D.seam_flags((1, 1, 1), (0, 0, 0)) == ((0, 0, 0), (0, 0, 0))
    sl = D.owned_slices((8, 6, 5), (1, 0, 0), (1, 0, 1), (1, 0, 0))
    assert sl == (slice(2, 8), slice(0, 6), slice(1, 5))


def test_path_length_is_bounded():
    """L (the longest chain of additions of the sums) for the test grids and the flagship sizes; never above 4096."""
    for g in ((17, 9, 5), (24, 15, 15), (70, 35, 8), (131, 66, 37), (255, 153, 153), (512, 512, 512), (512, 512, 1024), (1024, 1024, 1024)):
        nb, kz = D.launch_geometry(*g)
        assert 8 <= kz <= 32 and nb >= 1
        assert D.path_length(*g) == kz + 18 + (nb + 255) // 256 <= 4096, g
    assert D.path_length(512, 512, 512) == 128


def _header_struct(txt, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
        if ctype == "long" and names.startswith("long "):
            ctype, names = "long long", names[5:]
        for nm in names.split(","):
            nm = nm.strip()
            m = re.match(r"(\w+)\[(\d+)\]$", nm)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (nm, ctype, 1))
    return fields


def _py_struct(cls):
    base = {C.c_double: "double", C.c_int: "int", C.c_longlong: "long long"}
    out = []
    for n, t in cls._fields_:
        if t in base:
            out.append((n, base[t], 1))
        else:
            out.append((n, base[t._type_], t._length_))
    return out


def test_ctypes_mirrors_match_the_header(tmp_path):
    from navierstokes3d_amd import lib as L
    txt = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HEADER], capture_output=True, text=True, check=True).stdout)
    pairs = (("ns3d_diag", L.Diag), ("ns3d_diag_params", L.DiagParams))
    for cname, py in pairs:
        assert _py_struct(py) == _header_struct(txt, cname), cname
    # offsets and sizes as the C compiler lays the header's structs out
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ns3d.h"', 'int main(void){']
    for cname, py in pairs:
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for n, _ in py._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, n, cname, n))
    src.append("return 0;}")
    cfile, exe = tmp_path / "layout.c", tmp_path / "layout"
    cfile.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(cfile), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in pairs:
        assert int(got[cname]) == C.sizeof(py), cname
        for n, _ in py._fields_:
            assert int(got["%s.%s" % (cname, n)]) == getattr(py, n).offset, (cname, n)


def test_julia_mirrors_list_the_same_fields():
    from navierstokes3d_amd import lib as L
    src = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "NS3DShim.jl"), encoding="utf-8").read())
    jt = {"Cdouble": "double", "Cint": "int", "Clonglong": "long long"}
    for jname, py in (("Diag", L.Diag), ("DiagParams", L.DiagParams)):
        body = re.search(r"\nstruct %s\b(.*?)\nend" % jname, src, re.S).group(1)
        fields = []
        for n, t in re.findall(r"(\w+)::([\w{},]+)", body):
            m = re.match(r"NTuple\{(\d+),(\w+)\}$", t)
            fields.append((n, jt[m.group(2)], int(m.group(1))) if m else (n, jt[t], 1))
        assert fields == _py_struct(py), jname


def test_entry_points_are_exported():
    from navierstokes3d_amd import lib as L
    names = ["ns3d_diagnostics_f64", "ns3d_diagnostics_f32", "ns3d_diagnostics_mgpu_f64", "ns3d_diagnostics_mgpu_f32"]
    assert set(names) <= set(L.exported_symbols())
    assert os.path.exists(L.LIB_PATH), "libns3d.so is not built (python -m navierstokes3d_amd.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(names) <= exported


def test_wide_halo_precondition_threshold():
    """The finite branch of the driver's check: courant[2] below 2 passes, 2 and above raises the named error, and so does
    a NaN; the other directions do not matter."""
    from navierstokes3d_amd import driver, lib as L
    for ok in (0.0, 1.5, math.nextafter(2.0, 0.0)):
        driver._check_wide_precondition(1, (9.0, 9.0, ok))
    for bad in (2.0, math.nextafter(2.0, 3.0), 2.5, 1e300, float("inf"), float("nan")):
        with pytest.raises(L.Ns3dError, match=r"courant\[2\].*wide_advect_halo.*2 cells"):
            driver._check_wide_precondition(3, (0.0, 0.0, bad))
