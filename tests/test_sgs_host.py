"""CPU tests of ns3d_sgs_viscosity's contract: the NumPy statements of the three operators (tests/sgs_ref.py) against
les_ref.eddy_viscosity, against closed forms — pure shear, where WALE and Vreman must vanish exactly, and solid-body rotation —, the
pairs' clamp and guarded quotient, and the boundary (header, binding, export list, the drivers' refusals and defaults).  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import les_ref as LR
import running_error as RE
import sgs_ref as SR
from util import bits_equal, fields, first_bit_difference, geometry, hostile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(3, 3, 3), (4, 3, 5), (9, 7, 5), (17, 9, 5)]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NEW = [SR.WALE, SR.VREMAN]
OPID = lambda op: SR.NAMES[op]


def _V(n, dtype, seed=3):
    return fields(*n, ("vx", "vy", "vz"), seed0=seed, dtype=dtype)


def _args(n, length=0.05):
    g = geometry(*n)
    return (g["mu"], g["rho"], length, g["dx"], g["dy"], g["dz"])


# ---- operator 0 is ns3d_eddy_viscosity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_operator_0_is_the_eddy_viscosity_statement(n, dtype):
    V = _V(n, dtype)
    a, b = SR.sgs_viscosity(SR.SMAGORINSKY, *V, *_args(n)), LR.eddy_viscosity(*V, *_args(n))
    assert a.dtype == dtype and bits_equal(a, b), first_bit_difference(a, b)


# ---- what the feature exists for --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("n", [(4, 3, 5), (9, 7, 5), (17, 9, 5)], ids=str)
def test_pure_shear_gives_mu_exactly(n, op, dtype):
    """u = γ·y: every entry of g² and every 2×2 minor of β is a sum of exact zeros, so mu_e is muT in EVERY cell, bit for bit — where
    Smagorinsky's is muT + c·γ on the whole interior"""
    gamma = 1.375
    Vx, Vy, Vz, dx, dy, dz = LR.pure_shear(n, gamma, dtype)
    m, val = SR.sgs_viscosity(op, Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz, with_op=True)
    assert m.dtype == dtype and np.all(val == 0)
    assert bits_equal(m, np.full(n, dtype(1e-3), dtype=dtype, order="F"))
    s = SR.sgs_viscosity(SR.SMAGORINSKY, Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz)
    want = 1e-3 + 1000.0 * 0.02 * 0.02 * gamma
    assert np.abs(s[LR.I].astype(np.float64) - want).max() <= 8 * RE.unit(dtype) * want and np.all(s[LR.I] > 1.5 * dtype(1e-3))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_length_zero_rest_and_the_boundary_layer_give_mu(n, op, dtype):
    muT = dtype(geometry(*n)["mu"])
    V = _V(n, dtype)
    full = np.full(n, muT, dtype=dtype, order="F")
    assert bits_equal(SR.sgs_viscosity(op, *V, *_args(n, 0.0)), full)
    R = [hostile(a, 5 + q, "rest0") for q, a in enumerate(V)]
    m, val = SR.sgs_viscosity(op, *R, *_args(n), with_op=True)
    assert bits_equal(m, full) and np.all(val == 0)                     # den == 0 / aa == 0: the guards, not 0/0
    m = SR.sgs_viscosity(op, *V, *_args(n))
    outer = np.ones(n, dtype=bool)
    outer[LR.I] = False
    assert np.all(m[outer] == muT) and np.all(m[LR.I] > muT) and np.isfinite(m).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_solid_body_rotation_has_the_closed_forms(dtype):
    """u = −ω·y, v = ω·x with ω = 11/8: the discrete gradient is uy = −ω, vx = ω exactly.  Relative errors, in unit roundoffs u (a
    bound in u is at least as strict as the same count of ulp), read off the trees:
    Vreman: p = fl(ω²) [u], B = fl(p·p) [u], aa = 2p exact, fl(B/aa) [u], the root halves those three and adds its own:
        ω/√2 within (3/2 + 1)u = 2.5u.
    WALE: q11 = q22 = −p [u], t = third·(−2p) [third's own u, the product's u], d11 = d22 = fl(−p − t) = −(p/3)(1 + η), |η| ≤ 2·2u + u
        (the cancellation doubles t's error), d33 = −t exact; squares: 2·5u + u = 11u and 2·2u + u = 5u; their sum, weights 2/6 and
        4/6: (2·11 + 4·5)/6 = 7u, + u; with p² = ω⁴(1 + 2u): dd = (2ω⁴/3)(1 + 10u).  ss = 0, so op = fl(dd·√dd)/fl(dd·√√dd) = dd^¼
        carries dd's error at weight ¼ [2.5u] plus the roundings of √dd [u], num [u], the inner root at weight ½ [u/2], the outer root
        [u], den's product [u] and the quotient [u]: 8u.
    The closed forms are evaluated in float64 (three roundings, at most 2·2⁻⁵³ relative), which the bars below add."""
    omega = 1.375
    n = (9, 7, 5)
    Vx, Vy, Vz, dx, dy, dz = SR.rotation(n, omega, dtype)
    T = dtype
    G = LR.gradient(Vx, Vy, Vz, T(0.5), T(dx), T(dy), T(dz))
    for q, want in zip(G, (0, 0, 0, -omega, 0, omega, 0, 0, 0)):
        assert np.all(q == T(want))
    u = RE.unit(dtype)
    for op, closed, bar in ((SR.VREMAN, omega / math.sqrt(2.0), 2.5), (SR.WALE, math.sqrt(math.sqrt(2.0 * omega ** 4 / 3.0)), 8.0)):
        _, val = SR.sgs_viscosity(op, Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz, with_op=True)
        err = np.abs(val.astype(np.float64) - closed).max() / closed
        print("%s %s: op within %.2f u of the closed form (bar %.1f u)" % (SR.NAMES[op], np.dtype(dtype).name, err / u, bar))
        assert val.dtype == dtype and err <= bar * u + 2 * RE.U64


def test_vreman_s_clamp_is_reached_and_holds():
    """parallel gradient rows make β singular: B is 0 in real arithmetic and its rounded value takes either sign.  The seeded search
    finds cells with B < 0 in both types; the statement returns muT there, never a NaN from the root of a negative number."""
    for dtype in DTYPES:
        found = SR.negative_B((6, 5, 5), dtype)
        assert found is not None
        (Vx, Vy, Vz, dx, dy, dz), neg = found
        m, val = SR.sgs_viscosity(SR.VREMAN, Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz, with_op=True)
        assert neg.any() and np.all(val[neg] == 0) and np.isfinite(m).all() and np.all(m[LR.I][neg] == dtype(1e-3))
    x = np.float32([-1.0, -0.0, 0.0, 2.0, np.nan])
    c = SR.clamp0(x)
    assert c.dtype == np.float32 and np.array_equal(c[:4], np.float32([0, -0.0, 0, 2])) and np.isnan(c[4])
    g = SR.guard(np.float32([0.0, -0.0, 1.0, np.nan]), np.float32([np.nan, np.inf, 3.0, np.nan]))
    assert np.array_equal(g[:3], np.float32([0, 0, 3])) and np.isnan(g[3])


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------
def test_pair_clamp_and_guard():
    u = RE.U32
    p = RE.Pair(np.array([-1.0, 1e-9, 2.0, -1e-9]), np.array([0.5, 1e-8, 0.0, 1e-8]), u)
    c = SR.clamp0(p)
    assert np.array_equal(c.v, [0.0, 1e-9, 2.0, 0.0]) and np.array_equal(c.e, p.e)
    for t in np.linspace(-1e-9 - 1e-8, -1e-9 + 1e-8, 9):                # every clamped member of the enclosure lies within the bound
        assert abs(max(t, 0.0) - c.v[3]) <= c.e[3]
    den = RE.Pair(np.array([0.0, 0.0, 4.0]), np.array([0.0, 1e-9, 0.0]), u)
    val = RE.Pair(np.array([np.nan, np.nan, 0.5]), np.array([np.inf, np.inf, 1e-7]), u)
    g = SR.guard(den, val)
    assert np.array_equal(g.v, [0.0, 0.0, 0.5]) and g.e[0] == 0.0 and g.e[1] == np.inf and g.e[2] == 1e-7


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
def test_pair_statements_enclose_the_numpy_statements(op, dtype):
    n = (9, 7, 5)
    V = _V(n, dtype, 11)
    m = SR.sgs_viscosity(op, *V, *_args(n, 0.02))
    pm = SR.sgs_viscosity_pairs(op, *V, *_args(n, 0.02))
    assert np.all(np.abs(m.astype(np.float64) - pm.v) <= RE.allowed(dtype) * pm.e)
    assert np.all(pm.e[LR.I] > 0) and np.isfinite(pm.e).all() and pm.e[0].max() == 0
    R = [hostile(a, 5 + q, "rest0") for q, a in enumerate(V)]
    pr = SR.sgs_viscosity_pairs(op, *R, *_args(n, 0.02))
    assert (pr.e == 0).all() and np.all(pr.v == float(dtype(geometry(*n)["mu"])))


def test_the_step_with_operator_0_is_les_ref_s_step():
    """sgs_ref.step restates les_ref.step with the first statement replaced: with operator 0 the two are the same step, bit for bit"""
    from oracle.driver_ref import multi_params
    p = multi_params(12)
    p.xco_g, p.yco_g, p.zco_g = 0.0 - (p.lx - p.dx) / 2, 0.0 - (p.ly - p.dy) / 2, 0.0 - (p.lz - p.dz) / 2
    n = (p.nx, p.ny, p.nz)
    Z = lambda *s: np.zeros(s, order="F")

    def state():
        f = dict(Pr=Z(*n), dPrdtau=Z(n[0] - 2, n[1] - 2, n[2] - 2), divV=Z(*n), C=Z(*n), C_o=Z(*n), Vx=Z(n[0] + 1, n[1], n[2]),
                 Vy=Z(n[0], n[1] + 1, n[2]), Vz=Z(n[0], n[1], n[2] + 1), Vx_o=Z(n[0] + 1, n[1], n[2]), Vy_o=Z(n[0], n[1] + 1, n[2]),
                 Vz_o=Z(n[0], n[1], n[2] + 1))
        f["Vy"][0, :, :] = p.vin
        LR.cylinder(f, p, "multi")
        return f
    length = LR.smagorinsky_length(0.17, p.dx, p.dy, p.dz)
    a, b, w = state(), state(), state()
    for _ in range(2):
        ra = SR.step(SR.SMAGORINSKY, a, p, length, 14)
        rb = LR.step(b, p, length, 14)
        SR.step(SR.WALE, w, p, SR.length_of(SR.WALE, p.dx, p.dy, p.dz), 14)
        assert ra[1:] == rb[1:] and bits_equal(ra[0], rb[0])
    for k in a:
        assert bits_equal(a[k], b[k]), k
    assert not bits_equal(a["Vy"], w["Vy"])


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_three_symbols():
    import ctypes as C
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    m = re.search(r"int ns3d_sgs_viscosity_##S\(([^;]*)\);", src)
    assert m, "include/ns3d.h does not declare ns3d_sgs_viscosity_##S"
    args = [a.strip() for a in re.sub(r"\\\n", " ", m.group(1)).split(",")]
    classes = ["ns3d_ctx", "int", "T"] + ["const"] * 3 + ["double"] * 6 + ["int"] * 3
    assert [a.split()[0] for a in args] == classes
    want = {"T": C.c_void_p, "const": C.c_void_p, "double": C.c_double, "int": C.c_int}
    assert L.DERIVED_SIGNATURES["sgs_viscosity"] == [want[c] for c in classes[1:]]
    assert len(L.SIGNATURES) == 35 and "sgs_viscosity" not in L.SIGNATURES
    syms = L.exported_symbols()
    assert "ns3d_sgs_viscosity_f64" in syms and "ns3d_sgs_viscosity_f32" in syms
    assert re.search(r"enum \{ NS3D_SGS_SMAGORINSKY = 0, NS3D_SGS_WALE = 1, NS3D_SGS_VREMAN = 2 \};", src)
    assert re.search(r"enum \{ NS3D_TURB_NONE = 0, NS3D_TURB_SMAGORINSKY = 1 \};", src)
    assert re.search(r"int ns3d_set_sgs_operator\(ns3d_ctx \*\w*, int op\);", src)
    assert re.search(r"int ns3d_sgs_operator\(const ns3d_ctx \*\w*\);", src)
    assert "ns3d_set_sgs_operator" in L.CONTEXT_SYMBOLS and "ns3d_sgs_operator" in L.CONTEXT_SYMBOLS
    assert (L.NS3D_SGS_SMAGORINSKY, L.NS3D_SGS_WALE, L.NS3D_SGS_VREMAN) == (0, 1, 2)
    assert L.SGS_OPERATORS == {v: k for k, v in SR.NAMES.items()}


def test_library_exports_the_entry_points():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for suf in ("f64", "f32"):
        fn = getattr(lib, "ns3d_sgs_viscosity_" + suf)
        assert fn(None, *[a() for a in L.DERIVED_SIGNATURES["sgs_viscosity"]]) == L.NS3D_ERR_ARG
        assert L.last_error() == "ns3d_sgs_viscosity_%s: null context" % suf
    assert lib.ns3d_set_sgs_operator(None, 1) == L.NS3D_ERR_ARG
    assert L.last_error() == "ns3d_set_sgs_operator: null context"
    assert lib.ns3d_sgs_operator(None) == -1


# ---- the drivers' refusals and defaults -------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_allocation(monkeypatch):
    """anything that would create a context or an array fails the test"""
    from navierstokes3d_amd import driver, kernels as K

    def boom(*a, **k):
        raise AssertionError("the driver allocated before it refused")
    monkeypatch.setattr(driver, "_alloc", boom)
    monkeypatch.setattr(K, "Context", boom)
    monkeypatch.setattr(K, "zeros", boom)


ALL_NAMES = "(?s)(?=.*smagorinsky)(?=.*wale)(?=.*vreman)"


def test_the_drivers_refuse_before_any_allocation(no_allocation):
    from navierstokes3d_amd import driver, lib as L
    refused = ["k-epsilon", "WALE", dict(model="dynamic"), dict(model="wale", cs=0.17), dict(model="vreman", cw=0.5),
               dict(model="smagorinsky", c=0.07), dict(model="wale", cw=0.5, wall="van Driest"), dict(model="vreman", wall="van Driest"),
               dict(cw=0.5), dict(model=["wale"]), 1]
    for run in (driver.run_navierstokes3D, driver.runme):
        for t in refused:
            with pytest.raises(L.Ns3dError, match=ALL_NAMES):       # every refusal lists all model names
                run(nx=24, nt=1, device=0, turbulence=t)
        for t, msg in ((dict(model="wale", cw=-0.1), "cw = -0.1"), (dict(model="wale", cw=float("nan")), "cw = nan"),
                       (dict(model="vreman", c=-0.1), "c = -0.1"), (dict(model="vreman", c=float("inf")), "c = inf"),
                       (dict(model="smagorinsky", cs=-0.1), "cs = -0.1"), (dict(model="smagorinsky", cs=float("nan")), "cs = nan")):
            with pytest.raises(L.Ns3dError, match=msg):
                run(nx=24, nt=1, device=0, turbulence=t)
    from types import SimpleNamespace
    two = SimpleNamespace(P=2, dims=(1, 1, 2), mg=None, contexts=None, local_ranks=[0, 1], local_coords=[(0, 0, 0), (0, 0, 1)],
                          is_root=lambda: True)
    for model in ("wale", "vreman"):
        with pytest.raises(L.Ns3dError, match=model + ".*one rank.*seams.*halo"):
            driver.run_navierstokes3D(nx=24, nt=1, device=0, grid=two, turbulence=model)


def test_the_defaults_are_the_published_equivalents_of_cs():
    from navierstokes3d_amd import driver
    assert driver._check_turbulence("wale").cw == 0.5535 == SR.CW and driver._check_turbulence("wale").model == "wale"
    assert driver._check_turbulence("vreman").c == 0.07225 == SR.CV and driver._check_turbulence(dict(model="vreman")).model == "vreman"
    assert driver._check_turbulence("smagorinsky").cs == 0.17 and driver._check_turbulence("smagorinsky").model == "smagorinsky"
    assert driver._check_turbulence(dict(model="wale", cw=0.4)).cw == 0.4 and driver._check_turbulence(dict(model="vreman", c=0.0)).c == 0.0
    # C_w² = 10.6·C_s² and c_v = 2.5·C_s², to the literals' four digits
    assert abs(0.5535 ** 2 - 10.6 * 0.17 ** 2) < 1e-4 and 0.07225 == pytest.approx(2.5 * 0.17 ** 2, abs=1e-15)
    d = (0.02, 0.03, 0.05)
    delta = (d[0] * d[1] * d[2]) ** (1.0 / 3.0)
    for t, op, want in (("smagorinsky", SR.SMAGORINSKY, 0.17 * delta), ("wale", SR.WALE, 0.5535 * delta),
                        ("vreman", SR.VREMAN, math.sqrt(0.07225) * delta)):
        assert driver.sgs_length(driver._check_turbulence(t), *d) == want == SR.length_of(op, *d)
