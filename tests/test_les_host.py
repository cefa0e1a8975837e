"""CPU tests of the Smagorinsky model's contract: the NumPy statements (tests/les_ref.py) against oracle/numpy_ref.py where the
viscosity field is uniform and against closed forms where it is not, the pairs' square root, and the boundary (header, binding,
export list, the drivers' refusals).  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import les_ref as LR
import running_error as RE
import vortex_ref as VR
from oracle import numpy_ref as NR
from util import bits_equal, fields, first_bit_difference, geometry, hostile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(3, 3, 3), (4, 3, 5), (9, 7, 5), (17, 9, 5)]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NAMES = ("eddy_viscosity", "update_tau_var", "predict_var")


def _V(n, dtype, seed=3):
    return fields(*n, ("vx", "vy", "vz"), seed0=seed, dtype=dtype)


# ---- a uniform field is the scalar ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_uniform_mu_e_gives_the_bits_of_numpy_ref(n, dtype):
    """0.25*((m+m)+(m+m)) is exact: update_tau_var with a uniform field is numpy_ref.update_tau, and predict_var numpy_ref.predict_V
    behind it, bit for bit"""
    g = geometry(*n)
    T = dtype
    V = _V(n, dtype)
    m = np.full(n, T(g["mu"]), dtype=dtype, order="F")
    got = LR.tau_var(*V, m, g["dx"], g["dy"], g["dz"])
    want = LR._stress_arrays(V[0])
    NR.update_tau(*want, *V, T(g["mu"]), T(g["dx"]), T(g["dy"]), T(g["dz"]))
    for a, b in zip(got, want):
        assert a.dtype == dtype and bits_equal(a, b), first_bit_difference(a, b)
    new = LR.predict_var(*V, m, g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])
    ref = [a.copy(order="F") for a in V]
    NR.predict_V(*ref, *want, T(g["rho"]), T(g["g"]), T(g["dt"]), T(g["dx"]), T(g["dy"]), T(g["dz"]))
    for a, b in zip(new, ref):
        assert a.dtype == dtype and bits_equal(a, b), first_bit_difference(a, b)
    assert not bits_equal(new[0], V[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_smagorinsky_field_changes_the_stresses(dtype):
    """on a 9×7×5 grid a field of ordinary size moves a good share of the normal stresses and most of the shear stresses"""
    n = (9, 7, 5)
    g = geometry(*n)
    V = _V(n, dtype)
    m = LR.eddy_viscosity(*V, g["mu"], g["rho"], 0.17 * (g["dx"] * g["dy"] * g["dz"]) ** (1 / 3), g["dx"], g["dy"], g["dz"])
    got = LR.tau_var(*V, m, g["dx"], g["dy"], g["dz"])
    want = LR._stress_arrays(V[0])
    NR.update_tau(*want, *V, dtype(g["mu"]), dtype(g["dx"]), dtype(g["dy"]), dtype(g["dz"]))
    normal = np.mean([np.mean(a != b) for a, b in zip(got[:3], want[:3])])
    shear = np.mean([np.mean(a != b) for a, b in zip(got[3:], want[3:])])
    assert 0.2 < normal < 0.5 and shear > 0.7, (normal, shear)


# ---- where the model is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_length_zero_rest_and_the_boundary_layer_give_mu(n, dtype):
    g = geometry(*n)
    muT = dtype(g["mu"])
    V = _V(n, dtype)
    sp = (g["dx"], g["dy"], g["dz"])
    m = LR.eddy_viscosity(*V, g["mu"], g["rho"], 0.0, *sp)
    assert m.dtype == dtype and m.shape == n and np.all(m == muT)
    for values in ("rest0",):
        R = [hostile(a, 5 + q, values) for q, a in enumerate(V)]
        m = LR.eddy_viscosity(*R, g["mu"], g["rho"], 0.05, *sp)
        assert bits_equal(m, np.full(n, muT, dtype=dtype, order="F"))
    m = LR.eddy_viscosity(*V, g["mu"], g["rho"], 0.05, *sp)
    outer = np.ones(n, dtype=bool)
    outer[LR.I] = False
    assert np.all(m[outer] == muT)
    assert np.all(m[LR.I] > muT)
    assert np.all(m >= muT)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [(4, 3, 5), (9, 7, 5), (17, 9, 5)], ids=str)
def test_pure_shear_has_the_strain_rate_gamma(n, dtype):
    """u = γ·y: |S| = γ within 2 ulp on the interior, and mu_e = μ + ρℓ²γ there"""
    gamma = 1.375
    Vx, Vy, Vz, dx, dy, dz = LR.pure_shear(n, gamma, dtype)
    m, s2 = LR.eddy_viscosity(Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz, with_s2=True)
    S = np.sqrt(s2)
    assert S.dtype == dtype
    ulp = np.spacing(dtype(gamma))
    assert np.abs(S.astype(np.float64) - gamma).max() <= 2 * float(ulp), np.abs(S.astype(np.float64) - gamma).max()
    want = 1e-3 + 1000.0 * 0.02 * 0.02 * gamma
    assert np.abs(m[LR.I].astype(np.float64) - want).max() <= 8 * RE.unit(dtype) * want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_gradient_is_the_vortex_statement_s(dtype):
    """Q formed from this module's gradient entries is vortex_ref's Q, bit for bit: the two statements agree about the gradient"""
    n = (9, 7, 5)
    g = geometry(*n)
    V = _V(n, dtype)
    T = dtype
    gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = LR.gradient(*V, T(0.5), T(g["dx"]), T(g["dy"]), T(g["dz"]))
    Q = ((-T(0.5)) * ((gxx * gxx + gyy * gyy) + gzz * gzz)) - ((uy * vx + uz * wx) + vz * wy)
    ref = VR.reference(*V, g["dx"], g["dy"], g["dz"])
    assert bits_equal(np.asfortranarray(Q), np.asfortranarray(ref["Q"][VR.I]))
    assert bits_equal(np.asfortranarray(wy - vz), np.asfortranarray(ref["Wx"][VR.I]))


# ---- pairs ----------------------------------------------------------------------------------------------------------------------------------
def test_pair_square_root():
    u = RE.U32
    p = RE.Pair(np.array([4.0, 1e-6, 0.0, 0.0, 2.0]), np.array([1e-3, 2e-6, 0.0, 1e-8, 0.0]), u)
    r = LR.sqrt(p)
    assert np.array_equal(r.v, np.sqrt(p.v))
    # inside: the lower end of the enclosure moves furthest, plus two unit roundoffs of the result
    assert r.e[0] >= (2.0 - np.sqrt(4.0 - 1e-3)) + 2 * u * 2.0 and r.e[0] <= 1.001 * ((2.0 - np.sqrt(4.0 - 1e-3)) + 2 * u * 2.0)
    # v − e ≤ 0: the width of the enclosure's image
    assert r.e[1] >= np.sqrt(3e-6) and r.e[3] >= 1e-4
    assert r.e[2] == 0.0 and r.v[2] == 0.0                 # an exact zero stays exact
    assert r.e[4] >= 2 * u * np.sqrt(2.0) and r.e[4] <= 2.001 * u * np.sqrt(2.0)
    # every true root of the enclosure lies within the bound
    for t in np.linspace(4.0 - 1e-3, 4.0 + 1e-3, 11):
        assert abs(np.sqrt(t) - r.v[0]) <= r.e[0]
    assert np.array_equal(LR.sqrt(np.float32([2.0])), np.sqrt(np.float32([2.0])))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_statements_enclose_the_numpy_statements(dtype):
    n = (9, 7, 5)
    g = geometry(*n)
    V = _V(n, dtype, 11)
    args = (g["mu"], g["rho"], 0.02, g["dx"], g["dy"], g["dz"])
    m = LR.eddy_viscosity(*V, *args)
    pm = LR.eddy_viscosity_pairs(*V, *args)
    assert np.all(np.abs(m.astype(np.float64) - pm.v) <= RE.allowed(dtype) * pm.e)
    assert np.all(pm.e[LR.I] > 0) and pm.e[0].max() == 0
    scal = (g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])
    new = LR.predict_var(*V, m, *scal)
    pn = LR.predict_var_pairs(*V, m, *scal)
    for a, p in zip(new, pn):
        assert np.all(np.abs(a.astype(np.float64) - p.v) <= RE.allowed(dtype) * p.e)
    R = [hostile(a, 5 + q, "rest0") for q, a in enumerate(V)]
    pr = LR.eddy_viscosity_pairs(*R, *args)
    assert (pr.e == 0).all()


# ---- the whole step -------------------------------------------------------------------------------------------------------------------------
def test_the_step_with_length_zero_is_numpy_ref_s_step():
    """les_ref.step with ℓ = 0 is the step numpy_ref.run_multi_1rank composes (faithful advection), fields and iteration counts"""
    from oracle.driver_ref import multi_params
    nx, nt = 12, 2
    want, iters = NR.run_multi_1rank(nx, nt)
    p = multi_params(nx)
    p.xco_g, p.yco_g, p.zco_g = 0.0 - (p.lx - p.dx) / 2, 0.0 - (p.ly - p.dy) / 2, 0.0 - (p.lz - p.dz) / 2
    n = (p.nx, p.ny, p.nz)
    Z = lambda *s: np.zeros(s, order="F")
    f = dict(Pr=Z(*n), dPrdtau=Z(n[0] - 2, n[1] - 2, n[2] - 2), divV=Z(*n), C=Z(*n), C_o=Z(*n), Vx=Z(n[0] + 1, n[1], n[2]),
             Vy=Z(n[0], n[1] + 1, n[2]), Vz=Z(n[0], n[1], n[2] + 1), Vx_o=Z(n[0] + 1, n[1], n[2]), Vy_o=Z(n[0], n[1] + 1, n[2]),
             Vz_o=Z(n[0], n[1], n[2] + 1))
    f["Vy"][0, :, :] = p.vin
    LR.cylinder(f, p, "multi")
    got = [LR.step(f, p, 0.0, p.niter, "multi", faithful=True)[1] for _ in range(nt)]
    assert got == iters
    for k in ("Pr", "C", "Vx", "Vy", "Vz", "dPrdtau", "divV"):
        assert bits_equal(f[k], want[k]), k


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
CLASSES = {
    "eddy_viscosity": ["ns3d_ctx", "T"] + ["const"] * 3 + ["double"] * 6 + ["int"] * 3,
    "update_tau_var": ["ns3d_ctx"] + ["T"] * 6 + ["const"] * 4 + ["double"] * 3 + ["int"] * 3,
    "predict_var": ["ns3d_ctx"] + ["T"] * 3 + ["const"] * 4 + ["double"] * 6 + ["int"] * 3,
}


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_and_binding_lists_the_entry_point(name):
    import ctypes as C
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    m = re.search(r"int ns3d_%s_##S\(([^;]*)\);" % name, src)
    assert m, "include/ns3d.h does not declare ns3d_%s_##S" % name
    args = [a.strip() for a in re.sub(r"\\\n", " ", m.group(1)).split(",")]
    assert [a.split()[0] for a in args] == CLASSES[name]
    syms = L.exported_symbols()
    assert "ns3d_%s_f64" % name in syms and "ns3d_%s_f32" % name in syms
    assert len(L.SIGNATURES) == 35 and name not in L.SIGNATURES
    sig = L.DERIVED_SIGNATURES[name]
    assert len(sig) == len(args) - 1
    want = {"T": C.c_void_p, "const": C.c_void_p, "double": C.c_double, "int": C.c_int}
    assert sig == [want[c] for c in CLASSES[name][1:]]


def test_header_declares_the_knob():
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    assert re.search(r"enum \{ NS3D_TURB_NONE = 0, NS3D_TURB_SMAGORINSKY = 1 \};", src)
    assert re.search(r"int ns3d_set_turbulence\(ns3d_ctx \*\w*, int model, double length, void \*mu_e\);", src)
    assert re.search(r"int ns3d_turbulence\(const ns3d_ctx \*\w*\);", src)
    assert "ns3d_set_turbulence" in L.CONTEXT_SYMBOLS and "ns3d_turbulence" in L.CONTEXT_SYMBOLS
    assert (L.NS3D_TURB_NONE, L.NS3D_TURB_SMAGORINSKY) == (0, 1)


def test_library_exports_the_entry_points():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for name in NAMES:
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            assert fn(None, *[a() for a in L.DERIVED_SIGNATURES[name]]) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
    assert lib.ns3d_set_turbulence(None, 1, 0.1, None) == L.NS3D_ERR_ARG
    assert L.last_error() == "ns3d_set_turbulence: null context"
    assert lib.ns3d_turbulence(None) == -1


# ---- the drivers' refusals ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_allocation(monkeypatch):
    """anything that would create a context or an array fails the test"""
    from navierstokes3d_amd import driver, kernels as K

    def boom(*a, **k):
        raise AssertionError("the driver allocated before it refused")
    monkeypatch.setattr(driver, "_alloc", boom)
    monkeypatch.setattr(K, "Context", boom)
    monkeypatch.setattr(K, "zeros", boom)


def test_the_drivers_refuse_before_any_allocation(no_allocation):
    from navierstokes3d_amd import driver, lib as L
    for run in (driver.run_navierstokes3D, driver.runme):
        with pytest.raises(L.Ns3dError, match="smagorinsky"):
            run(nx=24, nt=1, device=0, turbulence="k-epsilon")
        with pytest.raises(L.Ns3dError, match="smagorinsky"):
            run(nx=24, nt=1, device=0, turbulence=dict(model="dynamic"))
        with pytest.raises(L.Ns3dError, match="smagorinsky"):
            run(nx=24, nt=1, device=0, turbulence=dict(model="smagorinsky", cs=0.1, wall="van Driest"))
        with pytest.raises(L.Ns3dError, match="cs = -0.1"):
            run(nx=24, nt=1, device=0, turbulence=dict(model="smagorinsky", cs=-0.1))
        with pytest.raises(L.Ns3dError, match="cs = nan"):
            run(nx=24, nt=1, device=0, turbulence=dict(model="smagorinsky", cs=float("nan")))
    two = SimpleNamespace(P=2, dims=(1, 1, 2), mg=None, contexts=None, local_ranks=[0, 1], local_coords=[(0, 0, 0), (0, 0, 1)],
                          is_root=lambda: True)
    with pytest.raises(L.Ns3dError, match="one rank.*seams.*halo"):
        driver.run_navierstokes3D(nx=24, nt=1, device=0, grid=two, turbulence="smagorinsky")
    assert driver._check_turbulence(None) is None and driver._check_turbulence(None, 4) is None
    assert driver._check_turbulence("smagorinsky").cs == 0.17
    assert driver._check_turbulence(dict(model="smagorinsky", cs=0.1)).cs == 0.1
