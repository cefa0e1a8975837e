"""CPU tests of the running statistics' host side: the slot order against the header's enum, the nominal traffic per cell, the
four C-ABI symbols in the ctypes binding and the Julia shim, and the null-context status (no GPU needed for any of it)."""
import ctypes as C
import os
import re

import pytest
import torch

from navierstokes3d_amd import lib as L
from navierstokes3d_amd import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ns3d.h")
SHIM = os.path.join(ROOT, "julia", "NS3DShim.jl")
SYMBOLS = ("ns3d_stats_accumulate_f64", "ns3d_stats_accumulate_f32", "ns3d_stats_reset", "ns3d_stats_finalize")


def test_slots_follow_the_header_enum():
    txt = open(HEADER, encoding="utf-8").read()
    enum = {n: int(v) for n, v in re.findall(r"\bNS3D_STATS_([A-Z]+) = (\d+)", txt)}
    assert enum.pop("SLOTS") == len(stats.SLOTS) == L.NS3D_STATS_SLOTS == 11
    assert tuple(n.lower() for n, _ in sorted(enum.items(), key=lambda kv: kv[1])) == stats.SLOTS
    assert sorted(enum.values()) == list(range(11))
    assert stats.SLOTS == ("u", "v", "w", "p", "uu", "vv", "ww", "uv", "uw", "vw", "pp")
    assert stats.MEAN == ("U", "V", "W", "P") and stats.RS == stats.SLOTS[4:]


def test_bytes_per_cell():
    assert stats.bytes_per_cell(torch.float64, True) == 208
    assert stats.bytes_per_cell(torch.float32, True) == 192
    assert stats.bytes_per_cell() == 208
    assert 512 ** 3 * stats.bytes_per_cell() == 27917287424          # the 27.9 GB of a 512³ call


def test_bytes_per_cell_without_pr():
    """The nominal figures for Pr = NULL as the interface was specified: 184 (fp64 fields) and 172 (fp32) — the Pr read and one
    accumulator's load and store less than with Pr.  The kernel skips BOTH slots p and pp (tests/test_gpu_stats.py), so what it
    moves is 3 field reads + 9 loads + 9 stores: 168 / 156 B, reported by bytes_moved_per_cell."""
    got = (stats.bytes_per_cell(torch.float64, False), stats.bytes_per_cell(torch.float32, False))
    print("bytes_per_cell without Pr: fp64 %d, fp32 %d" % got)
    assert got == (184, 172)
    assert (stats.bytes_moved_per_cell(torch.float64, False), stats.bytes_moved_per_cell(torch.float32, False)) == (168, 156)
    assert (stats.bytes_moved_per_cell(torch.float64, True), stats.bytes_moved_per_cell(torch.float32, True)) == (208, 192)


def test_symbols_are_bound_in_python_and_julia():
    exported = set(L.exported_symbols())
    shim = re.sub(r"#[^\n]*", "", open(SHIM, encoding="utf-8").read())
    ccalls = set(re.findall(r"ccall\(\(:(\w+),\s*libns3d\)", shim))
    for s in SYMBOLS:
        assert s in exported, s
    for s in ("ns3d_stats_accumulate_f64", "ns3d_stats_reset", "ns3d_stats_finalize"):
        assert s in ccalls, s
    lib = L.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_context_is_an_argument_error(name):
    """The context check comes before anything touches a device: status NS3D_ERR_ARG and a message, on a machine without a GPU."""
    lib = L.load()
    fn = getattr(lib, name)
    if "accumulate" in name:
        rc = fn(None, None, None, None, None, None, C.c_double(1.0), 3, 3, 3)
    elif name.endswith("reset"):
        rc = fn(None, None, 3, 3, 3)
    else:
        rc = fn(None, None, C.c_double(1.0), None, None, 3, 3, 3)
    assert rc == L.NS3D_ERR_ARG == 1
    assert "null context" in L.last_error() and name.replace("_f64", "").replace("_f32", "") in L.last_error()
