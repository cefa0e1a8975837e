"""CPU tests of the active scalar's contract: the NumPy statements (tests/scalar_ref.py) against closed forms — the discrete
eigenmodes of the zero-flux operator, conservation, the hull of the 7-point stencil —, the buoyancy range, the pairs, the step
against oracle/numpy_ref.py where the scalar is switched off, and the boundary (header, binding, export list, the drivers'
refusals).  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import les_ref as LR
import running_error as RE
import scalar_ref as SC
from oracle import numpy_ref as NR
from util import bits_equal, first_bit_difference, geometry, hostile, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(5, 4, 3), (17, 9, 5), (67, 19, 35)]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NAMES = ("scalar_diffuse", "buoyancy", "scalar_step")


def _case(n, dtype, seed=3):
    """C in (−1, 1), a varying mu_e ≥ mu, the geometry, kappa and sgs at 0.9 of the limit dt·K_max·Σ1/d² = ½"""
    g = geometry(*n)
    C = rnd(seed, n, dtype)
    mu_e = rnd(seed + 1, n, dtype, g["mu"], 5 * g["mu"])
    sgs = 1.0 / (g["rho"] * 0.7)
    s = SC.sum_inv_d2(g["dx"], g["dy"], g["dz"])
    # K_max = kappa + sgs·(max mu_e − mu) = 0.9·½/(dt·s)
    kappa = 0.45 / (g["dt"] * s) - sgs * (float(mu_e.max()) - g["mu"])
    assert kappa > 0
    return g, C, mu_e, kappa, sgs


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", [(1, 0, 0), (0, 2, 0), (0, 0, 3), (2, 1, 1), (4, 3, 2)], ids=str)
def test_a_discrete_eigenmode_is_multiplied_by_its_factor(modes):
    """C = Π cos(π p (i+½)/n) is an eigenvector of the zero-flux operator: one step multiplies it by 1 − 4·dt·κ·Σ sin²(πp/2n)/d²,
    in fp64 to within the statement's own running-error bound.  The stored C is the eigenvector rounded, C + δ with |δ| ≤ u·max|C|:
    the operator A (rows of absolute sum 1 below the limit) and the factor λ (|λ| ≤ 1) carry that to |Aδ − λδ| ≤ 2u·max|C|, and the
    product λ·C is rounded once more: 3u·max|C| beside the bound."""
    n = (17, 9, 5)
    g = geometry(*n)
    kappa = 0.2 / (g["dt"] * SC.sum_inv_d2(g["dx"], g["dy"], g["dz"]))
    C = SC.eigenmode(n, modes)
    args = (None, kappa, 0.0, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
    out = SC.scalar_diffuse(C, *args)
    pair = SC.scalar_diffuse_pairs(C, *args)
    want = SC.eigenfactor(n, modes, kappa, g["dt"], g["dx"], g["dy"], g["dz"]) * C
    assert np.all(np.abs(out - want) <= pair.e + 3 * RE.U64 * np.abs(C).max()), np.abs(out - want).max()
    assert np.abs(out - C).max() > 1e-3            # the factor is not 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_the_flux_form_conserves_the_sum(n, dtype):
    """every interior flux enters two cells with opposite signs and no flux crosses a domain face: |ΣC_out − ΣC| in fp64 is rounding
    only — at most N·eps(T)·max|C|; the statement stays below 0.7 of that"""
    g, C, mu_e, kappa, sgs = _case(n, dtype)
    N, eps = C.size, float(np.finfo(dtype).eps)
    for m in (mu_e, None):
        out = SC.scalar_diffuse(C, m, kappa if m is not None else 0.45 / (g["dt"] * SC.sum_inv_d2(g["dx"], g["dy"], g["dz"])), sgs, g["mu"],
                                g["dt"], g["dx"], g["dy"], g["dz"])
        drift = abs(float(out.astype(np.float64).sum()) - float(C.astype(np.float64).sum()))
        assert drift <= 0.7 * N * eps * float(np.abs(C).max()), (drift, N * eps)
        assert not bits_equal(out, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_at_nine_tenths_of_the_limit_the_result_stays_in_the_hull(n, dtype):
    """at 0.9 of dt·K_max·Σ1/d² = ½ the update is a convex combination of the 7-point stencil up to rounding: strictly inside
    min / max on random data, within 4 ulp of 1 on 0/1 block data"""
    g, C, mu_e, kappa, sgs = _case(n, dtype)
    args = (mu_e, kappa, sgs, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
    out = SC.scalar_diffuse(C, *args)
    lo, hi = SC.stencil_hull(C)
    assert np.all(out >= lo) and np.all(out <= hi)
    B = SC.block01(n, dtype)
    out = SC.scalar_diffuse(B, *args)
    lo, hi = SC.stencil_hull(B)
    tol = 4 * float(np.spacing(dtype(1)))
    assert np.all(out >= lo - dtype(tol)) and np.all(out <= hi + dtype(tol)), (float((lo - out).max()), float((out - hi).max()))
    assert out.max() <= 1 + tol and out.min() >= -tol and 0 < np.count_nonzero(out != B)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_uniform_mu_e_equal_mu_gives_the_bits_of_none(n, dtype):
    g, C, _, kappa, sgs = _case(n, dtype)
    m = np.full(n, dtype(g["mu"]), dtype=dtype, order="F")
    tail = (kappa, sgs, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
    a, b = SC.scalar_diffuse(C, m, *tail), SC.scalar_diffuse(C, None, *tail)
    assert bits_equal(a, b), first_bit_difference(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("values", ["seeded", "blocks", "rest0"])
def test_no_diffusivity_returns_C_by_value(dtype, values):
    """kappa = 0, sgs = 0 is a full pass of exact zeros: values, not bits (−0.0 + 0.0 is +0.0)"""
    n = (17, 9, 5)
    g = geometry(*n)
    C = rnd(5, n, dtype)
    if values != "seeded":
        C = hostile(C, 7, values)
    assert np.isfinite(C).all()
    out = SC.scalar_diffuse(C, rnd(6, n, dtype, 1e-3, 2e-3), 0.0, 0.0, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
    assert np.array_equal(out, C)


# ---- buoyancy -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_buoyancy_range_and_values(dtype):
    n = (9, 7, 6)
    T = dtype
    Vz = rnd(11, (n[0], n[1], n[2] + 1), dtype)
    # C ≡ c_ref: bg·(C − c_ref) = 0 whatever bg is, Vz by value
    same = SC.buoyancy(Vz, np.full(n, T(0.25), dtype=dtype, order="F"), 3.0, 0.25, 0.013)
    assert np.array_equal(same, Vz)
    # a block of C = 1, powers of two so that every product is exact: the faces touching it move by dt·bg·(½ or 1), no others
    C = np.zeros(n, dtype=dtype, order="F")
    C[3:5, 2:4, 2:4] = 1
    dt, bg = 0.125, 4.0
    out = SC.buoyancy(Vz, C, bg, 0.0, dt)
    moved = (out != Vz)
    want = np.zeros(Vz.shape)
    want[3:5, 2:4, 2] = want[3:5, 2:4, 4] = dt * bg * 0.5
    want[3:5, 2:4, 3] = dt * bg
    assert np.array_equal(moved, want != 0)
    assert np.allclose((out.astype(np.float64) - Vz.astype(np.float64))[moved], want[moved], rtol=0, atol=4 * float(np.finfo(dtype).eps))
    # the i/j boundary columns and the faces k = 0, k = nz never move, whatever C holds
    out = SC.buoyancy(Vz, rnd(12, n, dtype), 3.0, 0.1, 0.013)
    edge = np.ones(Vz.shape, dtype=bool)
    edge[SC.INN] = False
    assert np.array_equal(out[edge], Vz[edge]) and np.all(out[SC.INN] != Vz[SC.INN])
    assert edge[:, :, 0].all() and edge[:, :, -1].all() and edge[0].all() and edge[:, -1].all()


# ---- pairs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_statements_enclose_the_numpy_statements(dtype):
    n = (17, 9, 5)
    g, C, mu_e, kappa, sgs = _case(n, dtype, 21)
    for m in (mu_e, None):
        args = (m, kappa, sgs, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
        out, pair = SC.scalar_diffuse(C, *args), SC.scalar_diffuse_pairs(C, *args)
        assert np.all(np.abs(out.astype(np.float64) - pair.v) <= RE.allowed(dtype) * pair.e)
        assert np.all(pair.e > 0)
    Vz = rnd(23, (n[0], n[1], n[2] + 1), dtype)
    out, pair = SC.buoyancy(Vz, C, 2.5, 0.3, g["dt"]), SC.buoyancy_pairs(Vz, C, 2.5, 0.3, g["dt"])
    assert np.all(np.abs(out.astype(np.float64) - pair.v) <= RE.allowed(dtype) * pair.e)
    assert pair.e[:, :, 0].max() == 0 and np.all(pair.e[SC.INN] > 0)
    rest = SC.scalar_diffuse_pairs(np.zeros(n, dtype=dtype, order="F"), mu_e, kappa, sgs, g["mu"], g["dt"], g["dx"], g["dy"], g["dz"])
    assert (rest.e == 0).all() and (rest.v == 0).all()


# ---- the whole step -------------------------------------------------------------------------------------------------------------------------
def test_the_step_without_diffusivity_and_lift_is_numpy_ref_s_step():
    """scalar_ref.step with kappa = 0, bg = 0 is the step numpy_ref.run_multi_1rank composes: Pr and V bit for bit, C by value"""
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
    off = dict(kappa=0.0, sct=0.7, bg=0.0, c_ref=0.0)
    got = [SC.step(f, p, off, p.niter, "multi", faithful=True)[1] for _ in range(nt)]
    assert got == iters
    for k in ("Pr", "Vx", "Vy", "Vz", "dPrdtau", "divV"):
        assert bits_equal(f[k], want[k]), k
    assert np.array_equal(f["C"], want["C"])


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
CLASSES = {
    "scalar_diffuse": ["ns3d_ctx", "T"] + ["const"] * 2 + ["double"] * 7 + ["int"] * 3,
    "buoyancy": ["ns3d_ctx", "T", "const"] + ["double"] * 3 + ["int"] * 3,
    "scalar_step": ["ns3d_ctx", "T", "T"] + ["const"] * 2 + ["double"] * 9 + ["int"] * 3,
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
    assert name not in L.SIGNATURES
    want = {"T": C.c_void_p, "const": C.c_void_p, "double": C.c_double, "int": C.c_int}
    assert L.DERIVED_SIGNATURES[name] == [want[c] for c in CLASSES[name][1:]]


def test_header_declares_the_knob():
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    assert re.search(r"int ns3d_set_scalar\(ns3d_ctx \*\w*, int on, double kappa, double sct, double bg, double c_ref\);", src)
    assert re.search(r"int ns3d_scalar\(const ns3d_ctx \*\w*\);", src)
    assert "ns3d_set_scalar" in L.CONTEXT_SYMBOLS and "ns3d_scalar" in L.CONTEXT_SYMBOLS


def test_library_exports_the_entry_points():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for name in NAMES:
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            assert fn(None, *[a() for a in L.DERIVED_SIGNATURES[name]]) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
    assert lib.ns3d_set_scalar(None, 1, 0.1, 0.7, 0.0, 0.0) == L.NS3D_ERR_ARG
    assert L.last_error() == "ns3d_set_scalar: null context"
    assert lib.ns3d_scalar(None) == -1


def _function_text(src, head):
    """the text of the function that starts with `head`, up to the closing brace in column 0, comments and blanks dropped"""
    body = src[src.index(head):]
    body = body[:body.index("\n}\n") + 3]
    return [re.sub(r"\s*//.*", "", l).strip() for l in body.splitlines() if re.sub(r"\s*//.*", "", l).strip()]


def test_the_division_by_a_known_divisor_is_the_kernel_unit_s():
    """ns3d_scalar.hip restates div_by_known and its guards' limits (the kernel unit keeps them in its own text, where
    tests/div_model.py reads them): the two texts are the same"""
    csrc = os.path.join(ROOT, "navierstokes3d_amd", "csrc")
    a = open(os.path.join(csrc, "ns3d_kernels.hip")).read()
    b = open(os.path.join(csrc, "ns3d_scalar.hip")).read()
    for head in ("__device__ __forceinline__ T div_by_known(T x, T d, T r)", "__device__ __forceinline__ float div_by_known(float x, float d, float r)"):
        assert _function_text(a, head) == _function_text(b, head), head
    for line in ("template <> struct DivLim<double> { static constexpr double lo = 0x1p-900, hi = 0x1p900; };",
                 "template <> struct DivLim<float> { static constexpr float lo = 0x1p-83f, hi = 0x1p100f; };",
                 "g.rdx = (T)1 / g.dx; g.rdy = (T)1 / g.dy; g.rdz = (T)1 / g.dz;"):
        assert line in a and line in b, line
    for macro in ("#define DIV_X(v) div_by_known((v), g.dx, g.rdx)", "#define DIV_X(v) ((v) / g.dx)", "#define DIV_X(v) ((v)*g.rdx)"):
        assert macro in a and macro in b, macro


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
    monkeypatch.setattr(K, "from_numpy", boom)


def test_the_drivers_refuse_before_any_allocation(no_allocation):
    from navierstokes3d_amd import driver, lib as L
    for run in (driver.run_navierstokes3D, driver.runme):
        with pytest.raises(L.Ns3dError, match="scalar = .*kappa"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=1e-4, prandtl=0.7))
        with pytest.raises(L.Ns3dError, match="scalar = .*kappa"):
            run(nx=24, nt=1, device=0, scalar="heat")
        with pytest.raises(L.Ns3dError, match="scalar = .*kappa"):
            run(nx=24, nt=1, device=0, scalar=dict(sct=0.7))
        with pytest.raises(L.Ns3dError, match="kappa = -0.1"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=-0.1))
        with pytest.raises(L.Ns3dError, match="sct = -1"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=0.0, sct=-1))
        with pytest.raises(L.Ns3dError, match="beta_g = nan"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=0.0, beta_g=float("nan")))
        with pytest.raises(L.Ns3dError, match="c_ref = inf"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=0.0, c_ref=float("inf")))
        with pytest.raises(L.Ns3dError, match="explicit diffusion limit"):
            run(nx=24, nt=1, device=0, scalar=dict(kappa=1e3))
    two = SimpleNamespace(P=2, dims=(1, 1, 2), mg=None, contexts=None, local_ranks=[0, 1], local_coords=[(0, 0, 0), (0, 0, 1)],
                          is_root=lambda: True)
    with pytest.raises(L.Ns3dError, match="one rank.*seams.*halo"):
        driver.run_navierstokes3D(nx=24, nt=1, device=0, grid=two, scalar=dict(kappa=1e-4))
    assert driver._check_scalar(None) is None and driver._check_scalar(None, 4) is None
    s = driver._check_scalar(dict(kappa=1e-4, beta_g=2.0))
    assert (s.kappa, s.sct, s.bg, s.c_ref) == (1e-4, 0.7, 2.0, 0.0)


def test_the_limit_of_the_molecular_part_is_the_parameters_own():
    """just inside ½ passes, just outside is refused, with the script's own dt and spacings"""
    from navierstokes3d_amd import driver, lib as L
    from navierstokes3d_amd.params import gpu_params
    p = gpu_params(24)
    edge = 0.5 / (p.dt * SC.sum_inv_d2(p.dx, p.dy, p.dz))
    assert driver._check_scalar(dict(kappa=edge * (1 - 1e-12)), 1, p).kappa > 0
    with pytest.raises(L.Ns3dError, match="explicit diffusion limit"):
        driver._check_scalar(dict(kappa=edge * (1 + 1e-9)), 1, p)
