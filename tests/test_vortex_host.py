"""CPU tests of ns3d_vortex's contract: the NumPy reference (tests/vortex_ref.py) on flows whose vorticity and Q are known in closed
form, the byte accounting, and the boundary (header, binding, export list).  No GPU."""
import os
import re

import numpy as np
import pytest

import running_error as RE
import vortex_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(3, 3, 3), (4, 3, 5), (17, 9, 5)]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def _tol(G, dtype, spacings, shape):
    """rounding of a linear flow's samples: |V| ≤ ‖G‖∞·L on the grid, differences of neighbours divided by a spacing amplify one
    unit roundoff of |V| by 1/d; a handful of operations per entry, products of two entries for Q"""
    L = max(n * d for n, d in zip(shape, spacings)) + max(spacings)
    g = float(np.abs(G).sum(axis=1).max())
    per_entry = 16 * RE.unit(dtype) * g * L / min(spacings)
    return per_entry, 16 * per_entry * max(g, per_entry)


def _run(G, shape, dtype):
    Vx, Vy, Vz, dx, dy, dz = VR.linear_flow(G, shape, dtype)
    ref = VR.reference(Vx, Vy, Vz, dx, dy, dz)
    return ref, _tol(np.asarray(G, dtype=np.float64), dtype, (dx, dy, dz), shape)


def _boundary_is_plus_zero(ref):
    for n in VR.NAMES:
        a = np.array(ref[n], order="C")
        a[VR.I] = 1.0
        u = a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
        assert np.all(u[a != 1.0] == 0), n


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GRIDS, ids=str)
def test_solid_body_rotation(shape, dtype):
    """V = (−y, x, 0): ω = (0, 0, 2), Q = ½‖Ω‖² = 1"""
    ref, (tw, tq) = _run([[0, -1, 0], [1, 0, 0], [0, 0, 0]], shape, dtype)
    I = VR.I
    assert ref["Wz"].dtype == dtype
    assert np.abs(ref["Wz"][I] - 2.0).max() <= tw and np.abs(ref["Q"][I] - 1.0).max() <= tq
    assert np.abs(ref["Wx"][I]).max() <= tw and np.abs(ref["Wy"][I]).max() <= tw
    _boundary_is_plus_zero(ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GRIDS, ids=str)
def test_pure_strain(shape, dtype):
    """V = (x, −y, 0): ω = 0, Q = −½‖S‖² = −1"""
    ref, (tw, tq) = _run([[1, 0, 0], [0, -1, 0], [0, 0, 0]], shape, dtype)
    I = VR.I
    for n in ("Wx", "Wy", "Wz"):
        assert np.abs(ref[n][I]).max() <= tw, n
    assert np.abs(ref["Q"][I] + 1.0).max() <= tq
    _boundary_is_plus_zero(ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GRIDS, ids=str)
def test_full_gradient(shape, dtype):
    """a full, non-solenoidal G: ω_i = ε_ijk G_kj and Q = −½ tr(G²)"""
    G = np.array([[0.3, -1.1, 0.7], [0.9, -0.4, 0.2], [-0.6, 1.3, 0.8]])
    ref, (tw, tq) = _run(G, shape, dtype)
    I = VR.I
    w = (G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1])
    for n, want in zip(("Wx", "Wy", "Wz"), w):
        assert np.abs(ref[n][I] - want).max() <= tw, n
    assert np.abs(ref["Q"][I] + 0.5 * np.trace(G @ G)).max() <= tq
    _boundary_is_plus_zero(ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_reference_encloses_the_numpy_reference(dtype):
    """the Pair evaluation is the same expression: its value is within its own bound of the dtype's evaluation"""
    from util import fields
    Vx, Vy, Vz = fields(7, 6, 5, ("vx", "vy", "vz"), seed0=11, dtype=dtype)
    ref = VR.reference(Vx, Vy, Vz, 0.3, 0.11, 0.07)
    prs = VR.reference_pairs(Vx, Vy, Vz, 0.3, 0.11, 0.07)
    for n in VR.NAMES:
        assert np.all(np.abs(ref[n].astype(np.float64) - prs[n].v) <= RE.allowed(dtype) * prs[n].e), n
        assert np.all(prs[n].e[VR.I] > 0) and prs[n].e[0].max() == 0


def test_bytes_per_cell():
    import torch
    from navierstokes3d_amd import vortex as V
    assert V.bytes_per_cell(torch.float64, 4) == 56 and V.bytes_per_cell(torch.float32, 4) == 28
    assert V.bytes_per_cell(torch.float64, 1) == 32 and V.bytes_per_cell(np.float32, 2) == 20
    assert V.bytes_per_cell() == 56
    with pytest.raises(ValueError):
        V.bytes_per_cell(torch.float64, 0)
    assert V.NAMES == VR.NAMES


def test_header_declares_and_binding_lists_the_entry_point():
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    m = re.search(r"int ns3d_vortex_##S\(([^;]*)\);", src)
    assert m, "include/ns3d.h does not declare ns3d_vortex_##S"
    args = [a.strip() for a in re.sub(r"\\\n", " ", m.group(1)).split(",")]
    assert [a.split()[0] for a in args] == ["ns3d_ctx"] + ["T"] * 4 + ["const"] * 3 + ["double"] * 3 + ["int"] * 3
    syms = L.exported_symbols()
    assert "ns3d_vortex_f64" in syms and "ns3d_vortex_f32" in syms
    assert len(L.SIGNATURES) == 35 and "vortex" not in L.SIGNATURES
    assert len(L.DERIVED_SIGNATURES["vortex"]) == len(args) - 1


def test_library_exports_the_entry_point():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for suf in ("f64", "f32"):
        fn = getattr(lib, "ns3d_vortex_" + suf)
        assert fn(None, *[a() for a in L.DERIVED_SIGNATURES["vortex"]]) == L.NS3D_ERR_ARG
        assert L.last_error() == "ns3d_vortex_%s: null context" % suf
