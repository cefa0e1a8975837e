"""CPU tests of the moving-obstacle contract (include/ns3d.h at ns3d_set_solid_moving, ns3d_solid_momentum_moving,
ns3d_mesh_transform): the two consequences of the statement — zero motion is ns3d_set_solid, the body is exactly divergence-free —,
the rigid transform of a mesh in physical space, solid.rigid_motion's rotation, the boundary (header, binding, export list), the
drivers' refusals before any allocation, and the physics the feature is for: a box spinning in fluid at rest drags the fluid around
with it.  No GPU."""
import os
import re

import numpy as np
import pytest

import moving_cases as MC
import moving_ref as MR
import solid_ref as SR
from util import SHAPES, bits_equal, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
EPS = 2.0 ** -52


def _state(n, dtype, seed=5):
    return [rnd(seed + q, SHAPES[k](*n), dtype) for q, k in enumerate(("c", "vx", "vy", "vz"))]


def _box_mask(n, lo, hi):
    from navierstokes3d_amd import solid as S
    return SR.voxelize(S.box_mesh(lo, hi), *n)


# ---- the statement's two consequences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_motion_is_set_solid(dtype):
    """U = ω = +0.0, any centre, any origin: solid_ref.set_solid's bits, every stored zero +0.0 by sign (0 + (±0 − ±0) is +0)"""
    n = (17, 9, 5)
    mask = _box_mask(n, (3.2, 1.5, 0.7), (11.9, 7.1, 4.4))
    a, b = _state(n, dtype), _state(n, dtype)
    SR.set_solid(*a, mask)
    MR.set_solid_moving(*b, mask, (0.0,) * 6 + (7.3, -2.1, 40.9), (0.3, 0.7, 0.2), origin=(3, 0, 5))
    for x, y in zip(a, b):
        assert bits_equal(x, y)
    for V in b[1:]:
        assert not np.signbit(V[V == 0]).any() and (V == 0).sum() > 50


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_body_has_exactly_zero_divergence(dtype):
    """vbx does not depend on X (…): the two faces of a cell hold identical bits, so update_divV's expression is exactly +0.0 in every
    cell whose six faces are masked — in the element type's own arithmetic, whatever the nine numbers are"""
    n = (17, 9, 5)
    mask = _box_mask(n, (3.2, 1.5, 0.7), (11.9, 7.1, 4.4))
    C, Vx, Vy, Vz = _state(n, dtype)
    MR.set_solid_moving(C, Vx, Vy, Vz, mask, (0.31, -0.77, 0.13, 1.9, -2.3, 0.71, 7.3, 4.1, 2.9), (0.3, 0.7, 0.2), origin=(1, 2, 3))
    bx, by, bz = MR._bits(mask, n)[1:]
    full = bx[:-1] & bx[1:] & by[:, :-1] & by[:, 1:] & bz[:, :, :-1] & bz[:, :, 1:]
    assert full.sum() >= 60
    d = [dtype(v) for v in (0.3, 0.7, 0.2)]
    div = ((Vx[1:] - Vx[:-1]) / d[0] + (Vy[:, 1:] - Vy[:, :-1]) / d[1]) + (Vz[:, :, 1:] - Vz[:, :, :-1]) / d[2]
    assert div.dtype == dtype and (div[full] == 0).all() and not np.signbit(div[full]).any()
    assert (np.abs(Vx[bx]) > 0).all() and not (div[~full] == 0).all()


def test_momentum_terms_are_what_the_store_removes():
    """Σ terms = Σ V before − Σ V after over the masked owned nodes, term by term"""
    n = (9, 7, 5)
    mask = _box_mask(n, (2.2, 1.5, 0.7), (6.9, 5.1, 4.4))
    m9, d = (0.31, -0.77, 0.13, 1.9, -2.3, 0.71, 4.3, 3.1, 2.9), (0.3, 0.7, 0.2)
    for dtype in DTYPES:
        C, Vx, Vy, Vz = _state(n, dtype)
        terms = MR.momentum_terms(Vx, Vy, Vz, mask, m9, d)
        before = [V.astype(np.float64) for V in (Vx, Vy, Vz)]
        MR.set_solid_moving(C, Vx, Vy, Vz, mask, m9, d)
        for q, (V, b) in enumerate(zip((Vx, Vy, Vz), MR._bits(mask, n)[1:])):
            assert np.array_equal(terms[q], (before[q] - V.astype(np.float64))[b]) and terms[q].size == b.sum() > 0
        zero = MR.momentum_terms(*_state(n, dtype)[1:], mask, (0.0,) * 9, d)
        for a, b in zip(zero, SR.momentum_terms(*_state(n, dtype)[1:], mask)):
            assert bits_equal(a, b)


# ---- the transform -----------------------------------------------------------------------------------------------------------------------
def test_the_identity_pose_returns_the_mesh():
    """R = I, shift = 0: by value where (p − pivot)·d/d is exact — power-of-two spacings —, and within one rounding of each of the
    three operations otherwise"""
    from navierstokes3d_amd import solid as S
    tri = S.box_mesh(*MC.BOX)
    out = MR.transform(tri, np.eye(3), (1.0, 2.0, 0.5), (0.0, 0.0, 0.0), (0.25, 0.5, 0.125))
    assert out.shape == tri.shape and np.array_equal(out, tri)
    out = MR.transform(tri, np.eye(3), MC.BOX_CENTRE, (0.0, 0.0, 0.0), (1.0 / 24, 0.04, 0.04))
    assert np.abs(out - tri).max() <= 3 * EPS * np.abs(tri).max()


def test_a_quarter_turn_about_z_on_equal_spacings():
    """the box [2,6]×[3,5]×[1,4] turned by 90° about (4, 4, ·): [3,5]×[2,6]×[1,4], exactly — compared as masks"""
    from navierstokes3d_amd import solid as S
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    out = MR.transform(S.box_mesh((2, 3, 1), (6, 5, 4)), R, (4.0, 4.0, 2.5), (0, 0, 0), (0.5, 0.5, 0.5))
    assert sorted(set(map(tuple, out.reshape(-1, 3)))) == sorted(set(map(tuple, S.box_mesh((3, 2, 1), (5, 6, 4)).reshape(-1, 3))))
    n = (9, 8, 6)
    assert np.array_equal(SR.voxelize(out, *n), SR.voxelize(S.box_mesh((3, 2, 1), (5, 6, 4)), *n))
    moved = MR.transform(S.box_mesh((2, 3, 1), (6, 5, 4)), R, (4.0, 4.0, 2.5), (1.0, 0.5, -0.25), (0.5, 0.5, 0.5))
    assert np.array_equal(moved, out + np.array([1.0, 0.5, -0.25]))


def test_with_unequal_spacings_the_rotation_is_the_physical_one():
    """dx = 2·dy: a box of 4 × 2 cells (physically 2 × 0.5) turned by 90° is physically 0.5 × 2, that is 1 × 8 cells — not the 2 × 4
    cells a rotation in index space would give"""
    from navierstokes3d_amd import solid as S
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    d = (0.5, 0.25, 1.0)
    out = MR.transform(S.box_mesh((4.3, 5.3, 1.2), (8.3, 7.3, 3.7)), R, (6.3, 6.3, 2.0), (0, 0, 0), d)
    n = (12, 12, 5)
    want = SR.voxelize(S.box_mesh((5.8, 2.3, 1.2), (6.8, 10.3, 3.7)), *n)
    assert np.array_equal(SR.voxelize(out, *n), want) and want.any()
    assert not np.array_equal(SR.voxelize(S.box_mesh((5.3, 4.3, 1.2), (7.3, 8.3, 3.7)), *n), want)


def test_rigid_motion_s_rotation_is_orthogonal_and_composes():
    """Rodrigues' formula in fp64: RᵀR = I to 4 ulp per entry; R(t1 + t2) = R(t1)·R(t2) up to the rounding of the angle |ω|·t (relative
    2⁻⁵³ each, so 2⁻⁵² of the larger angle in the entries) and of the 3 × 3 product (a few ulp): 8·2⁻⁵²·max(1, angle)"""
    from navierstokes3d_amd import solid as S
    for omega in ((0.0, 0.0, 8.4), (1.3, -0.4, 2.2), (0.0, -3.0, 0.0), (1e-3, 2e-3, -1e-3)):
        pose = S.rigid_motion(omega=omega, centre=(1, 2, 3), spacing=(0.1, 0.2, 0.3))
        rate = float(np.linalg.norm(omega))
        for t1, t2 in ((0.04, 0.08), (0.3, 1.1), (2.0, 0.013)):
            R1, R2, R12 = pose(t1)[0], pose(t2)[0], pose(t1 + t2)[0]
            for R in (R1, R2, R12):
                assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * EPS
            assert np.abs(R12 - R1 @ R2).max() <= 8 * EPS * max(1.0, rate * (t1 + t2))
    R, shift, U, w, c = S.rigid_motion(velocity=(0.2, -0.1, 0.0), centre=(1, 2, 3), spacing=(0.1, 0.2, 0.5))(2.0)
    assert np.array_equal(R, np.eye(3)) and np.array_equal(shift, [4.0, -1.0, 0.0]) and np.array_equal(c, [5.0, 1.0, 3.0])
    assert np.array_equal(U, [0.2, -0.1, 0.0]) and not w.any()
    quarter = S.rotation((0.0, 0.0, 2.0), np.pi / 4)
    assert np.abs(quarter - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() <= 2 * EPS


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree():
    import ctypes as C
    from navierstokes3d_amd import lib as L
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    want = {"T": C.c_void_p, "unsigned": C.c_void_p, "double": C.c_double, "int": C.c_int, "long": C.c_longlong}

    def classes(decl):
        m = re.search(decl + r"\(([^;]*)\);", src)
        assert m, decl
        out = []
        for a in re.sub(r"\\\n", " ", m.group(1)).split(","):
            w = a.replace("const ", "").split()
            out.append("ptr:" + w[0] if "*" in a else w[0])
        return out

    def ctype(c):
        if c.startswith("ptr:"):
            return {"double": C.POINTER(C.c_double), "int": C.POINTER(C.c_int), "long": C.POINTER(C.c_longlong)}.get(c[4:], C.c_void_p)
        return want[c]
    for name in ("set_solid_moving", "solid_momentum_moving"):
        cl = classes(r"int ns3d_%s_##S" % name)
        assert cl[0] == "ptr:ns3d_ctx" and L.DERIVED_SIGNATURES[name] == [ctype(c) for c in cl[1:]], (name, cl)
        assert name not in L.SIGNATURES and {"ns3d_%s_f64" % name, "ns3d_%s_f32" % name} <= set(L.exported_symbols())
    assert classes(r"int ns3d_mesh_transform") == ["ptr:ns3d_ctx", "ptr:double", "ptr:double", "long"] + ["ptr:double"] * 4
    assert classes(r"int ns3d_set_obstacle_motion") == ["ptr:ns3d_ctx", "ptr:double", "ptr:int"]
    assert classes(r"int ns3d_obstacle_motion") == ["ptr:ns3d_ctx", "ptr:double"]
    for s in ("ns3d_mesh_transform", "ns3d_set_obstacle_motion", "ns3d_obstacle_motion"):
        assert s in L.CONTEXT_SYMBOLS and s in L.exported_symbols()


def test_library_exports_the_entry_points():
    import ctypes as C
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for name in ("set_solid_moving", "solid_momentum_moving"):
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            assert fn(None, *[a() for a in L.DERIVED_SIGNATURES[name]]) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
    assert lib.ns3d_mesh_transform(None, None, None, 0, None, None, None, None) == L.NS3D_ERR_ARG
    assert L.last_error() == "ns3d_mesh_transform: null context"
    assert lib.ns3d_set_obstacle_motion(None, (C.c_double * 9)(), None) == L.NS3D_ERR_ARG
    assert L.last_error() == "ns3d_set_obstacle_motion: null context"
    assert lib.ns3d_obstacle_motion(None, None) == -1


# ---- the drivers' refusals ---------------------------------------------------------------------------------------------------------------
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
    from types import SimpleNamespace
    from navierstokes3d_amd import driver, lib as L
    c = (11.0, 7.0, 7.0)
    for run in (driver.run_navierstokes3D, driver.runme):
        for m in (dict(omega=(0, 0, 1)), dict(omega=(0, 0, 1), centre=c, axis=(0, 0, 1)), dict(speed=1.0, centre=c), 3, "spin", [1, 2, 3]):
            with pytest.raises(L.Ns3dError, match="(?s)motion.*velocity.*omega.*centre"):
                run(nx=24, nt=1, device=0, motion=m)
        for m, msg in ((dict(omega=(0, 0, float("nan")), centre=c), "omega"), (dict(velocity=(float("inf"), 0, 0), centre=c), "velocity"),
                       (dict(centre=(1, 2, float("nan"))), "centre"), (dict(omega=(0, 1), centre=c), "omega")):
            with pytest.raises(L.Ns3dError, match="motion: %s = .*3 finite numbers" % msg):
                run(nx=24, nt=1, device=0, motion=m)
    two = SimpleNamespace(P=2, dims=(1, 1, 2), mg=None, contexts=None, local_ranks=[0, 1], local_coords=[(0, 0, 0), (0, 0, 1)],
                          is_root=lambda: True)
    for m in (dict(omega=(0, 0, 1), centre=c), lambda t: None):
        with pytest.raises(L.Ns3dError, match="motion= runs on one rank.*origin"):
            driver.run_navierstokes3D(nx=24, nt=1, device=0, grid=two, motion=m)


# ---- what the feature is for -------------------------------------------------------------------------------------------------------------
def test_the_scenarios_are_admissible():
    """"spin" changes its mask every step, "slide" too, the cylinder's mask never; every statement stays finite and moves the fluid"""
    for script in ("multi", "gpu"):
        for name in MC.MOVERS:
            for dt in ("f32", "f64"):
                run = MC.oracle_run(script, dt, name)
                assert all(np.isfinite(a).all() for a in run.fields.values()), (script, name, dt)
            assert run.rebuilt == (0 if name == "cylinder" else MC.NT), (script, name, run.rebuilt)
            masks = run.masks[-2 * MC.NT::2]
            if name != "cylinder":
                assert all(not np.array_equal(a, b) for a, b in zip(masks, masks[1:])) and not np.array_equal(masks[0], MC.box_mask())
        assert not bits_equal(MC.oracle_run(script, "f64", "spin").fields["Vx"], MC.oracle_run(script, "f64", "slide").fields["Vx"])


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_spinning_box_drags_the_fluid_at_rest_around(sign):
    """The multi script with vin = 0 from an all-zero state, the box turning about its tilted axis, three steps of the CPU statement
    with the DIRECT pressure solve: the circulation ∮V·dl through the FLUID — on the rectangles [6,16] × [2,13] and [5,17] × [2,13] of
    cell faces, one to three cells off the turning box, none of whose nodes the final mask covers, in the planes k = 6, 7, 8 through
    the body — has the sign of ω_z.  With ns3d_set_solid the fluid would still be at rest and every loop exactly 0; the pressure
    correction adds a gradient, which carries no circulation, so what the loops see is the body's tangential velocity handed to the
    fluid: by the nodes the turning box uncovers, by the advection, by the viscous term.  Measured for ω ≷ 0: 2.6·10⁻³ … 9.7·10⁻³
    and −0.9·10⁻³ … −6.4·10⁻³ on the inner loop, 2·10⁻⁴ … 3.3·10⁻³ and −2·10⁻⁴ … −9·10⁻⁴ on the outer one, of a body whose own
    2·ω_z·area is 0.67; the bar below is only that a loop stands clear of rounding: 10⁶ ulp of (surface speed × perimeter).
    Why the direct solve: at nx = 24 the script's PT loop is unstable (Δτ²·Σ1/d² = 1.02; the checkerboard mode grows
    by 1.58 per iteration, 2·10⁸ per loop capped at 42) and the staircase of a voxelized body excites it whatever ω is — with the cap
    the first step's three residual checks read 3.2·10³, 9.5·10⁵, 3.2·10⁸, after three steps the fluid next to the body holds |V|
    up to 5.9·10²⁰ for a surface speed of 1, and the same loops return −3.3·10¹⁸ … +7.9·10⁴: that growth, not the drag of the wall.
    The capped run is the next test's."""
    run, p = MC.rest_run(sign, pressure="direct")
    f = run.fields
    assert all(np.isfinite(a).all() for a in f.values()) and max(np.abs(f[k]).max() for k in ("Vx", "Vy", "Vz")) < 2.0
    speed = MC.ANGLE / p.dt * 3.85 * p.dx               # of the box's far corner
    bx, by = MR._bits(run.masks[-1], MC.GRID)[1:3]
    for lo, hi in (((6, 2), (16, 13)), ((5, 2), (17, 13))):
        for k in (6, 7, 8):
            rows, cols = [lo[1] - 1, lo[1], hi[1] - 1, hi[1]], [lo[0] - 1, lo[0], hi[0] - 1, hi[0]]
            assert not bx[lo[0]:hi[0] + 1, rows, k].any() and not by[cols, lo[1]:hi[1] + 1, k].any(), "the loop touches the body"
            gamma = MR.circulation(f["Vx"], f["Vy"], (p.dx, p.dy), lo, hi, k)
            floor = 1e6 * EPS * speed * 2 * ((hi[0] - lo[0]) * p.dx + (hi[1] - lo[1]) * p.dy)
            print("loop %r-%r, k = %d: circulation %.4e (floor %.1e)" % (lo, hi, k, gamma, floor))
            assert gamma * sign > floor, (lo, hi, k, gamma)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_under_the_capped_pt_loop_the_body_still_turns_the_way_of_omega(sign):
    """An extra beside the fluid-side test above: three steps of the statement (the multi script with vin = 0 from an all-zero state,
    PT capped at 42 iterations) with the box turning about a tilted axis.  The circulation ∮V·dl on the rectangle of nodes [10,12] × [6,8] of the plane k = 7,
    which the turning box covers at every step, in the fields the step's second masking leaves (the *_o buffers: what advect! reads),
    is 2·ω_z·area to a few roundings per node of the loop, so it has the sign of ω — with ns3d_set_solid it would be 0, and a body
    velocity ω × r with the two terms exchanged would turn the other way.
    Measured, and the reason the loop lies ON the body: at nx = 24 the script's PT loop is unstable (§4.15: Δτ²·Σ1/d² = 1.02; the
    checkerboard mode grows by 1.58 per iteration, 2·10⁸ per capped loop — the first step's three residual checks read 3.2·10³,
    9.5·10⁵, 3.2·10⁸), and the staircase of a voxelized body excites it whatever ω is: after three steps the fluid next to the body
    holds |V| up to 5.9·10²⁰ for a surface speed of 1, and loops through the fluid measure that growth, not the drag of the wall
    ([8,14] × [4,11]: −3.3·10¹⁸ for ω > 0, +2.5·10¹⁷ for ω < 0; [5,17] × [2,13]: +7.9·10⁴ and −1.3·10³).  The statement stays finite,
    which is what the device comparisons need; a fluid-side circulation needs the direct solve or the reference's own grid."""
    run, p = MC.rest_run(sign)
    f = run.fields
    assert all(np.isfinite(a).all() for a in f.values())
    omega = sign * MC.ANGLE / p.dt * MC.AXIS[2]          # the component along z: the others add a constant to each side of the loop
    lo, hi = (10, 6), (12, 8)
    bx, by = MR._bits(run.masks[-1], MC.GRID)[1:3]
    assert bx[lo[0]:hi[0] + 1, lo[1] - 1:hi[1] + 1, 7].all() and by[lo[0] - 1:hi[0] + 1, lo[1]:hi[1] + 1, 7].all()
    want = 2.0 * omega * (hi[0] - lo[0]) * p.dx * (hi[1] - lo[1]) * p.dy
    for k in (7,):
        gamma = MR.circulation(f["Vx_o"], f["Vy_o"], (p.dx, p.dy), lo, hi, k)
        print("k = %d: circulation %.17g, 2·ω·area %.17g" % (k, gamma, want))
        assert gamma * sign > 0 and abs(gamma - want) <= 64 * EPS * abs(want)
