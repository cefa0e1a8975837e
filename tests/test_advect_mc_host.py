"""The limited MacCormack advection on the CPU (tests/advect_mc_ref.py, the NumPy statement of include/ns3d.h's definition): what the
scheme must do whatever runs it — a flow at rest and a uniform field are kept, the order of accuracy is two where the reference's
back-track has one, nothing leaves the range of the data — and that the seeded inputs of the GPU tests exercise the limiter."""
import functools

import numpy as np
import pytest

import advect_mc_ref as MC
from util import bits_equal, fields, geometry

GRIDS = [(3, 3, 3), (17, 9, 5), (70, 6, 7), (64, 8, 33), (131, 19, 38), (150, 21, 70)]       # test_gpu_advect_mc.GRIDS
CFLS = [0.3, 1.0, 2.7]
KINDS = ["vx", "vy", "vz", "c"]


def seeded(grid, cfl, dtype):
    """old fields [Vx, Vy, Vz, C], dt = cfl × the smallest spacing, geometry — the seeded case of the GPU tests"""
    g = geometry(*grid)
    return fields(*grid, KINDS, 41, dtype), cfl * min(g["dx"], g["dy"], g["dz"]), g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_flow_at_rest_keeps_its_bits(dtype):
    """Velocities +0.0, a seeded C, Â = A_o: every δ is 0, every lerp returns its first operand, the correction adds +0.0 and the
    limiter's hull is the node's own value.  (A −0.0 would come back as +0.0: −0.0 + h·(+0.0) — the definition's own arithmetic.)"""
    nx, ny, nz = 9, 7, 5
    g = geometry(nx, ny, nz)
    old = [np.zeros(a.shape, dtype=dtype, order="F") for a in fields(nx, ny, nz, KINDS[:3], 1, dtype)] + fields(nx, ny, nz, ["c"], 4, dtype)
    new = MC.correct(old, [a.copy(order="F") for a in old], 0.02, g["dx"], g["dy"], g["dz"])
    assert all(bits_equal(a, b) for a, b in zip(new, old))
    new, hat = MC.advect_mc(old, 0.02, g["dx"], g["dy"], g["dz"])
    assert all(bits_equal(a, b) for a, b in zip(new, old)) and all(bits_equal(a, b) for a, b in zip(hat, old))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_uniform_field_is_preserved(dtype):
    """C = 0.7 everywhere in a seeded flow: stage 1's lerps of equal values may be an ulp off, the limiter's hull [0.7, 0.7] is not"""
    old, dt, g = seeded((17, 9, 5), 1.0, dtype)
    old[3][...] = dtype(0.7)
    new, _ = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    assert bits_equal(new[3], old[3])


def test_scalar_step_is_the_full_scheme():
    """the C-only step of the convergence runs below is the full reference's C"""
    old, dt, g = seeded((17, 9, 5), 1.0, np.float64)
    new, hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    assert bits_equal(MC.scalar_step(old[3], old[0], old[1], old[2], dt, g["dx"], g["dy"], g["dz"]), new[3])
    assert bits_equal(MC.scalar_step(old[3], old[0], old[1], old[2], dt, g["dx"], g["dy"], g["dz"], maccormack=False), hat[3])


@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS)
def test_stage_1_references_agree_in_float64(oracle, grid, cfl):
    """numpy_ref.advect(faithful=False), stage 1 of the float64 reference, and the C oracle's advect, stage 1 of the float32 one
    (advect_mc_ref.stage1 says why), are one definition: the same bits in float64 on every seeded case"""
    old, dt, g = seeded(grid, cfl, np.float64)
    hat = MC.stage1(old, dt, g["dx"], g["dy"], g["dz"])
    ref = [a.copy(order="F") for a in old]
    oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], False)
    assert all(bits_equal(a, b) for a, b in zip(hat, ref))


def blob_errors(n, maccormack):
    """rms error and extreme values of the blob after T = 0.25"""
    C, V, dt, dx, steps, exact = MC.blob_setup(n)
    nodes = MC.node_sets(V[0], V[1], V[2], n, n, n, which=("C",))["C"]          # the same uniform velocities every step: formed once
    lo, hi = 0.0, 0.0
    for _ in range(steps):
        C = MC.scalar_step(C, V[0], V[1], V[2], dt, dx, dx, dx, maccormack=maccormack, nodes=nodes)
        lo, hi = min(lo, float(C.min())), max(hi, float(C.max()))
    return MC.rms(C, exact), lo, hi


def check_blob(err, lo, hi):
    """The issue's thresholds, shared with the device test.  err[(scheme, n)]"""
    order_mc = np.log2(err["mc", 48] / err["mc", 96])
    order_1 = np.log2(err["first", 48] / err["first", 96])
    print("rms errors %r; orders: MacCormack %.3f, first order %.3f; ratio at 48: %.2f; range [%r, %r]"
          % (err, order_mc, order_1, err["first", 48] / err["mc", 48], lo, hi))
    assert order_mc >= 1.7
    assert order_1 < 1.0
    assert err["mc", 48] < err["first", 48] / 3.0
    assert lo >= 0.0 and hi <= 1.0


def test_blob_second_order_and_bounded():
    """Gaussian blob, σ = 0.08, centre (0.3, 0.35, 0.4), unit box, uniform velocity (1, ½, ¼), dt = 0.37·dx, T = 0.25: observed order
    over n = 48 → 96 at least 1.7 (first order: below 1.0), a third of the first-order error at n = 48, all values in [0, 1]."""
    err, lo, hi = {}, 0.0, 0.0
    for n in (48, 96):
        for name, mc in (("mc", True), ("first", False)):
            err[name, n], a, b = blob_errors(n, mc)
            if mc:
                lo, hi = min(lo, a), max(hi, b)
    check_blob(err, lo, hi)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS[1:4])
def test_the_limiter_engages_on_the_seeded_fields(grid, cfl, dtype):
    """On the seeded inputs of the GPU tests the limiter raises to lo, lowers to hi, and leaves alone, each at > 0 nodes of every
    field: the bit comparisons there exercise all three outcomes."""
    old, dt, g = seeded(grid, cfl, dtype)
    counts = {}
    MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"], counts)
    for name in MC.NAMES:
        assert counts[name]["below"] > 0 and counts[name]["above"] > 0 and counts[name]["free"] > 0, (name, counts[name])


# ---- the whole step: oracle/driver_ref.py with advection="maccormack" ----------------------------------------------------------------
FIVE = ("C", "Pr", "Vx", "Vy", "Vz")


@functools.lru_cache(maxsize=None)
def ref_run(script, nt, advection=None, faithful=False, dtype=np.float64, pressure="pt", niter_cap=None):
    """(the five full local fields by name, the driver's info, its local state) of run_navierstokes3D_ref ("multi") or runme_ref
    ("gpu") at nx = 24 — 24×15×15 —, computed once per process and never modified; advection=None: the keyword is not passed"""
    from oracle.driver_ref import run_navierstokes3D_ref, runme_ref
    kw = dict(nx=24, nt=nt, faithful=faithful, dtype=dtype, pressure=pressure, niter_cap=niter_cap)
    if advection is not None:
        kw["advection"] = advection
    if script == "multi":
        out = run_navierstokes3D_ref(**kw)
        info, f = out[-1], out[-1].ranks[0]
        assert all(bits_equal(f[n][1:-1, 1:-1, 1:-1], a) for n, a in zip(FIVE, out[:5]))       # gather! strips one cell per side
    else:
        f, info = runme_ref(**kw)
    assert f.C.shape == (24, 15, 15)
    return {n: f[n] for n in FIVE}, info, f


@pytest.mark.parametrize("faithful", [True, False])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_ref_drivers_keep_their_bits_with_the_reference_scheme(oracle, script, faithful):
    """advection="reference" is the driver without the keyword: fields, iteration counts, error histories, nx = 24, two steps"""
    plain, info, f = ref_run(script, 2, None, faithful)
    named, info2, f2 = ref_run(script, 2, "reference", faithful)
    assert info.iters == info2.iters and info.errs == info2.errs and len(info.iters) == 2
    for n in FIVE + ("Vx_o", "Vy_o", "Vz_o", "C_o", "dPrdtau", "divV", "txx", "txy"):
        assert bits_equal(f[n], f2[n]), (script, faithful, n)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_ref_drivers_with_maccormack(oracle, script):
    """One step and two: C inside [0, 1], all five fields finite, and another scheme than the reference's — Vx and C differ.
    gpu.jl is the exception for C, and the test says so instead of passing it by: at 24×15×15 its PT loop diverges (|V| is of order
    1e132 after one step and 1e267 after two, in either scheme), every departure point is clamped to a wall, and the 0/1 field C —
    whose limiter hull is then a wall value as well — comes out the same in both schemes: all its marked cells after one step, none
    after two.  Only the velocities tell the schemes apart there."""
    for nt in (1, 2):
        mc, info, _ = ref_run(script, nt, "maccormack")
        ref, _, _ = ref_run(script, nt, "reference")
        assert mc["C"].min() >= 0.0 and mc["C"].max() <= 1.0
        assert all(np.isfinite(mc[n]).all() for n in FIVE)
        assert not bits_equal(mc["Vx"], ref["Vx"]) and not bits_equal(mc["Vy"], ref["Vy"]), (script, nt)
        if script == "gpu":
            assert bits_equal(mc["C"], ref["C"]) and np.isin(mc["C"], (0.0, 1.0)).all() and np.abs(mc["Vx"]).max() > 1e100
        else:
            assert mc["C"].max() > 0.0 and not bits_equal(mc["C"], ref["C"]), (script, nt)
        assert len(info.iters) == nt and all(it > 0 for it in info.iters)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_one_maccormack_step_is_the_hand_composition(oracle, script):
    """One step of the reference scheme with faithful=False leaves in X_o the fields as they are after set_bc_Vel (X_o .= X comes
    right before advect!), and everything up to there does not depend on the scheme.  advect_mc of those is the MacCormack step's X,
    bit for bit; they themselves are its X_o; Pr, dPrdτ, divV and the iteration record are the same."""
    _, info_r, fr = ref_run(script, 1, "reference")
    _, info_m, fm = ref_run(script, 1, "maccormack")
    p = info_m.params
    old = [fr[n + "_o"] for n in MC.NAMES]
    new, _ = MC.advect_mc(old, p.dt, p.dx, p.dy, p.dz)
    for n, a, b in zip(MC.NAMES, new, old):
        assert bits_equal(fm[n], a), (script, n)
        assert bits_equal(fm[n + "_o"], b), (script, n + "_o")
    assert not bits_equal(new[0], old[0]) and sum(not bits_equal(a, b) for a, b in zip(new, old)) >= 2, "the step advected next to nothing"
    for n in ("Pr", "dPrdtau", "divV"):
        assert bits_equal(fm[n], fr[n]), (script, n)
    assert info_m.iters == info_r.iters and info_m.errs == info_r.errs


def test_what_the_ref_drivers_refuse():
    from oracle.driver_ref import run_navierstokes3D_ref, runme_ref
    with pytest.raises(ValueError, match="faithful=False"):
        run_navierstokes3D_ref(nx=24, nt=1, advection="maccormack")
    with pytest.raises(ValueError, match="faithful=False"):
        runme_ref(nx=24, nt=1, advection="maccormack")
    with pytest.raises(ValueError, match="one rank"):
        run_navierstokes3D_ref(nx=24, nt=1, dims_z=2, faithful=False, advection="maccormack")
    with pytest.raises(ValueError, match="reference.*maccormack"):
        runme_ref(nx=24, nt=1, faithful=False, advection="weno")


def test_float32_steps_that_stay_finite(oracle):
    """What the float32 GPU comparisons rely on (tests/test_gpu_advect_mc.py, tests/ctx_script.py): run_navierstokes3D_ref with
    the MacCormack scheme at nx = 24 keeps all five fields finite for three steps in float32; runme_ref does not get through one (its
    PT loop diverges at this size and leaves float32's range within the step), so float32 has no gpu.jl step here."""
    mc, info, _ = ref_run("multi", 3, "maccormack", dtype=np.float32)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in mc.values()) and len(info.iters) == 3
    with np.errstate(all="ignore"):
        one, _, _ = ref_run("gpu", 1, "reference", dtype=np.float32)
    assert not any(np.isfinite(a).all() for a in one.values())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_departures_beyond_the_integer_range_clamp_at_the_right_wall(oracle, dtype):
    """Velocities of ±1e30 (and ±1e200 in float64): floor(ix − δ) is beyond ±2^63, where a conversion to int64 is undefined (x86: −2^63
    for either sign, and a clamp behind it would pick the LOW wall for a departure far beyond the HIGH one).  The references clamp
    before they convert, as oracle/ns3d_oracle.c and the kernels do: stage 1 equals the C oracle's advect in both element types, the
    departure cells are the far walls, and — δ being an integer, every weight 0 or 1 — the limited scheme returns wall values only.
    Found by the whole-step comparison of gpu.jl's script, whose flow at 24×15×15 is of this size after one step."""
    grid = (9, 7, 5)
    g = geometry(*grid)
    big = [1e30, 1e200] if dtype == np.float64 else [1e30]
    for v in big:
        old = fields(*grid, KINDS, 71, dtype)
        for q in range(3):
            sign = np.where(fields(*grid, KINDS[q:q + 1], 72 + q, dtype)[0] > 0, 1.0, -1.0)
            old[q] = np.asfortranarray((sign * v).astype(dtype))
        dt = 0.5 * g["dx"]
        ref = [a.copy(order="F") for a in old]
        oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], False)
        new, hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
        assert all(bits_equal(a, b) for a, b in zip(hat, ref)), v
        assert all(np.isfinite(a).all() for a in new + hat)
        nodes = MC.node_sets(old[0], old[1], old[2], *grid, which=("C",))["C"]
        T = dtype
        (x1, y1, z1), _, _ = MC.departure(old[3].shape, nodes[3], nodes[4], nodes[5], T(dt), T(g["dx"]), T(g["dy"]), T(g["dz"]), *nodes[:3])
        far = np.abs(nodes[3]) > 1.0                      # nodes between two opposite velocities average to 0 and stay
        assert far.any() and np.array_equal(x1[far], np.where(nodes[3][far] > 0, 1, grid[0])), v
