"""ns3d_advect_mc / ns3d_advect_correct (limited MacCormack advection) on the device, the knob of ns3d_time_step and the drivers'
`advection` keyword.  STRICT is compared bit for bit with tests/advect_mc_ref.py (whose limiter engages in all three ways on these
inputs: tests/test_advect_mc_host.py); FAST with the enclosure of tests/advect_mc_pairs.py; whole runs with oracle/driver_ref.py.
Stream order: tests/test_gpu_stream_order.py::test_advect_mc, on every kind of stream."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import advect_mc_pairs as MP
import advect_mc_ref as MC
import pair_cases as PC
from arena import Arena
from test_advect_mc_host import CFLS, GRIDS, KINDS, check_blob, ref_run, seeded
from util import bits_equal, first_bit_difference, fields, geometry, rnd

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
FORMS = ["windowed", "global"]
GID = lambda n: "%dx%dx%d" % tuple(n)
NEW, OLD, HAT = ("Vx_new", "Vy_new", "Vz_new", "C_new"), ("Vx", "Vy", "Vz", "C"), ("Vx_hat", "Vy_hat", "Vz_hat", "C_hat")


def select(form, monkeypatch):
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")                  # read per call
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)


@functools.lru_cache(maxsize=None)
def reference(grid, cfl, dtype):
    """(old, dt, geometry, new, hat) of the seeded case: computed once, never modified"""
    old, dt, g = seeded(grid, cfl, dtype)
    new, hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    return old, dt, g, new, hat


def garbage(old, seed):
    return [rnd(seed + q, a.shape, a.dtype, 5.0, 9.0) for q, a in enumerate(old)]


def interleave(new, old, hat):
    return [t for trio in zip(new, old, hat) for t in trio]


def device_mc(hip, ctx, old, dt, g, entry="advect_mc", hat=None):
    """entry on fresh device arrays, outputs (and, for advect_mc, the hat buffers) pre-filled with garbage → (new, hat, old) as
    they are afterwards"""
    d_old = [hip.from_numpy(a) for a in old]
    d_new = [hip.from_numpy(a) for a in garbage(old, 300)]
    d_hat = [hip.from_numpy(a) for a in (garbage(old, 400) if hat is None else hat)]
    getattr(hip, entry)(*interleave(d_new, d_old, d_hat), dt, g["dx"], g["dy"], g["dz"], ctx=ctx)
    ctx.sync()
    return [hip.to_numpy(t) for t in d_new], [hip.to_numpy(t) for t in d_hat], [hip.to_numpy(t) for t in d_old]


def assert_bits(got, want, what):
    for n, a, b in zip(OLD, got, want):
        assert bits_equal(a, b), (what, n, first_bit_difference(a, b))


# ---- STRICT: the reference's bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS, ids=GID)
def test_strict_bits(hip, grid, cfl, dtype, form, monkeypatch):
    """advect_mc: complete outputs over garbage, the reference's bits; the hat buffers carry copy_advect(faithful=0)'s bits; inputs
    untouched; copy_advect + advect_correct is the same thing."""
    select(form, monkeypatch)
    old, dt, g, want, want_hat = reference(grid, cfl, dtype)
    ctx = hip.Context(0, "strict")
    new, hat, after = device_mc(hip, ctx, old, dt, g)
    assert_bits(new, want, "advect_mc")
    assert_bits(hat, want_hat, "hat")
    assert_bits(after, old, "inputs")
    d_old = [hip.from_numpy(a) for a in old]
    d_hat = [hip.from_numpy(a) for a in garbage(old, 500)]
    hip.copy_advect(d_hat[0], d_old[0], d_hat[1], d_old[1], d_hat[2], d_old[2], d_hat[3], d_old[3], dt, g["dx"], g["dy"], g["dz"], False, ctx=ctx)
    stage1 = [hip.to_numpy(t) for t in d_hat]
    assert_bits(stage1, hat, "copy_advect(faithful=0) against the hat buffers")
    new2, hat2, after = device_mc(hip, ctx, old, dt, g, "advect_correct", hat=stage1)
    assert_bits(new2, new, "copy_advect + advect_correct")
    assert_bits(hat2, stage1, "advect_correct's hat inputs")
    assert_bits(after, old, "inputs")
    ctx.close()


# ---- hostile values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_in_the_old_fields(hip, dtype, form, monkeypatch):
    """a NaN and a ±Inf planted in A_o (the scalar and a velocity): NaN where the reference has NaN, its bits elsewhere"""
    select(form, monkeypatch)
    grid = (70, 6, 7)
    old, dt, g = seeded(grid, 1.0, dtype)
    old = [a.copy(order="F") for a in old]
    old[3][5, 2, 3], old[3][40, 3, 1], old[3][66, 4, 5] = np.nan, np.inf, -np.inf
    old[0][20, 1, 2], old[0][50, 4, 4] = np.nan, np.inf
    old[2][30, 3, 3] = -np.inf
    want, want_hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    assert all(np.isnan(a).any() and np.isfinite(a).sum() > a.size // 2 for a in want)
    ctx = hip.Context(0, "strict")
    new, hat, _ = device_mc(hip, ctx, old, dt, g)
    assert_bits(new, want, "advect_mc")
    assert_bits(hat, want_hat, "hat")
    ctx.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_departures_clamped_at_the_walls(hip, sign, dtype, form, monkeypatch):
    """every velocity component between 0.5 and 1 times `sign`, cfl 2.7: stage 1 leaves the array through the three low (high)
    walls, the reverse trace through the opposite ones — so both signs together clamp at all six, in both traces"""
    select(form, monkeypatch)
    grid = (17, 9, 5)
    g = geometry(*grid)
    dt = 2.7 * min(g["dx"], g["dy"], g["dz"])
    old = [np.asfortranarray((sign * (0.75 + 0.25 * a)).astype(dtype)) for a in fields(*grid, KINDS[:3], 51, dtype)] + fields(*grid, ["c"], 54, dtype)
    for q, d in enumerate(("dx", "dy", "dz")):                       # the slowest node still leaves: floor(1 − δ) < 1 and floor(n + δ) > n
        assert np.floor(1.0 - dt * 0.5 / g[d]) < 1
    want, want_hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    ctx = hip.Context(0, "strict")
    new, hat, _ = device_mc(hip, ctx, old, dt, g)
    assert_bits(new, want, "advect_mc")
    assert_bits(hat, want_hat, "hat")
    ctx.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_departures_leave_no_freedom(hip, dtype, form, monkeypatch):
    """pair_cases.planted_departures: δ on the integers, half-integers and ±0, every lerp and the correction exact — FAST and
    NS3D_IEEE_DIV return STRICT's bits, which are the reference's"""
    select(form, monkeypatch)
    old, dt, g = PC.planted_departures(dtype)
    want, want_hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    for mode, ieee in (("strict", False), ("strict", True), ("fast", False)):
        ctx = hip.Context(0, mode, ieee_div=ieee)
        new, hat, _ = device_mc(hip, ctx, old, dt, g)
        assert_bits(new, want, "advect_mc %s ieee_div=%r" % (mode, ieee))
        assert_bits(hat, want_hat, "hat %s ieee_div=%r" % (mode, ieee))
        ctx.close()


# ---- FAST: hull and running-error bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS, ids=GID)
def test_fast_within_the_enclosure(hip, grid, cfl, dtype, form, monkeypatch):
    """Every advected value inside the hull of A_o over the candidate forward stencils; where stage 1's three δ are decided, within
    the running-error bound (tests/advect_mc_pairs.py).  Entries outside the advected sets keep the old bits."""
    select(form, monkeypatch)
    old, dt, g, want, _ = reference(grid, cfl, dtype)
    pairs = MP.cached_pairs(grid, cfl, dtype)
    ctx = hip.Context(0, "fast")
    new, _, after = device_mc(hip, ctx, old, dt, g)
    ctx.close()
    n_dec, n_all, worst = MP.check(new, want, pairs, dtype, "FAST advect_mc %s cfl %g" % (GID(grid), cfl))
    print("decided %d of %d, worst err/bound %.3f" % (n_dec, n_all, worst))
    assert n_dec > 0.9 * n_all
    for q, name in enumerate(MC.NAMES):
        keep = np.ones(old[q].shape, dtype=bool)
        keep[pairs[name][0]] = False
        assert np.array_equal(new[q][keep], old[q][keep]), name
    assert_bits(after, old, "inputs")


# ---- errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["advect_mc", "advect_correct"])
def test_error_cases_leave_the_outputs_alone(hip, entry, dtype):
    """a null pointer, a grid below 3×3×3, any two of the twelve arrays equal: NS3D_ERR_ARG, nothing written"""
    from navierstokes3d_amd import lib as L
    lib = L.load()
    fn = getattr(lib, "ns3d_%s_%s" % (entry, "f64" if dtype == np.float64 else "f32"))
    grid = (5, 4, 3)
    g = geometry(*grid)
    old = fields(*grid, KINDS, 61, dtype)
    host = interleave(garbage(old, 600), old, garbage(old, 700))
    dev = [hip.from_numpy(a) for a in host]
    ctx = hip.Context(0, "strict")
    torch.cuda.synchronize()
    tail = [C.c_double(x) for x in (0.01, g["dx"], g["dy"], g["dz"])]
    ptrs = [C.c_void_p(t.data_ptr()) for t in dev]

    def refused(p, n=grid):
        assert fn(ctx.handle, *p, *tail, *n) == L.NS3D_ERR_ARG, L.last_error()
        ctx.sync()
        for t, a in zip(dev, host):
            assert bits_equal(hip.to_numpy(t), a), L.last_error()
    for q in range(12):
        refused(ptrs[:q] + [C.c_void_p(None)] + ptrs[q + 1:])
        assert "null field pointer" in L.last_error()
    for n in ((2, 4, 3), (5, 2, 3), (5, 4, 2)):
        refused(ptrs, n)
        assert "too small" in L.last_error()
    for q, r in itertools.combinations(range(12), 2):
        refused(ptrs[:r] + [ptrs[q]] + ptrs[r + 1:])
        assert "same array" in L.last_error()
    assert fn(None, *ptrs, *tail, *grid) == L.NS3D_ERR_ARG and "null context" in L.last_error()
    assert fn(ctx.handle, *ptrs, *tail, *grid) == L.NS3D_OK, L.last_error()           # and the arguments were good ones
    ctx.close()


def test_the_knob(hip):
    from navierstokes3d_amd import lib as L
    ctx = hip.Context(0, "strict")
    assert ctx.advection() == "reference"
    ctx.set_advection("maccormack")
    assert ctx.advection() == "maccormack" and L.load().ns3d_advection(ctx.handle) == L.NS3D_ADVECT_MACCORMACK
    assert L.load().ns3d_set_advection(ctx.handle, 2) == L.NS3D_ERR_ARG and ctx.advection() == "maccormack"
    with pytest.raises(L.Ns3dError):
        ctx.set_advection("weno")
    ctx.set_advection("reference")
    assert ctx.advection() == "reference"
    assert L.load().ns3d_set_advection(None, 0) == L.NS3D_ERR_ARG and L.load().ns3d_advection(None) == -1
    ctx.close()


# ---- ns3d_time_step and the drivers ----------------------------------------------------------------------------------------------------
FIELD_NAMES = ("C", "Pr", "Vx", "Vy", "Vz")


def same_run(a, b):
    return all(bits_equal(x, y) for x, y in zip(a[:5], b[:5])) and a[-1].iters == b[-1].iters


def test_time_step_with_the_knob_is_the_call_sequence(hip):
    """run_navierstokes3D(nx=24, nt=3): 24×15×15, three steps — ns3d_time_step with the knob on (one_call) against the same step call
    by call with advect_mc; C stays in [0, 1]; the scheme differs from the reference's; with the knob off the parent's bits."""
    from navierstokes3d_amd.driver import run_navierstokes3D
    kw = dict(nx=24, nt=3, mode="strict", faithful=False, return_info=True)
    one = run_navierstokes3D(advection="maccormack", one_call=True, **kw)
    seq = run_navierstokes3D(advection="maccormack", one_call=False, **kw)
    assert one[-1].params.nx == 24 and one[-1].params.ny == 15 and one[-1].params.nz == 15
    assert same_run(one, seq)
    assert one[0].min() >= 0.0 and one[0].max() <= 1.0 and all(np.isfinite(a).all() for a in one[:5])
    plain = run_navierstokes3D(**kw)
    named = run_navierstokes3D(advection="reference", **kw)
    calls = run_navierstokes3D(advection="reference", one_call=False, **kw)
    assert same_run(plain, named) and same_run(plain, calls)
    assert not bits_equal(one[2], plain[2])
    assert one[-1].ctx.advection() == "reference"                       # the driver puts the default back


def test_runme_with_maccormack(hip):
    from navierstokes3d_amd.driver import runme
    kw = dict(nx=24, nt=2, mode="strict", faithful=False, niter_cap=200)
    names = ("C", "Pr", "Vx", "Vy", "Vz", "Vx_o", "Vy_o", "Vz_o", "C_o")
    f1, i1 = runme(advection="maccormack", one_call=True, **kw)
    f2, i2 = runme(advection="maccormack", one_call=False, **kw)
    for n in names:
        assert bits_equal(hip.to_numpy(getattr(f1, n)), hip.to_numpy(getattr(f2, n))), n
    assert i1.iters == i2.iters
    c = hip.to_numpy(f1.C)
    assert c.min() >= 0.0 and c.max() <= 1.0
    f3, _ = runme(**kw)
    f4, _ = runme(advection="reference", **kw)
    for n in names:
        assert bits_equal(hip.to_numpy(getattr(f3, n)), hip.to_numpy(getattr(f4, n))), n
    assert not bits_equal(hip.to_numpy(f1.Vx), hip.to_numpy(f3.Vx))


def test_observers_keep_working_with_maccormack(hip):
    from navierstokes3d_amd.driver import run_navierstokes3D
    out = run_navierstokes3D(nx=24, nt=2, mode="strict", faithful=False, return_info=True, advection="maccormack", niter_cap=200,
                             diagnostics=True, statistics=1, vortex=True, tracers=50, probes=np.zeros((2, 3)), isosurface=0.0)
    info = out[-1]
    assert len(info.diag) == 2 and info.stats.n == 2 and info.vortex.Q.shape == out[0].shape and info.probes.u.shape == (2, 2)


def test_what_maccormack_refuses(hip):
    """faithful=True, a two-rank grid and an unknown name raise before the first step; ns3d_time_step with the knob on and
    faithful = 1 returns NS3D_ERR_ARG and leaves the fields alone"""
    from navierstokes3d_amd import driver, lib as L
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    with pytest.raises(L.Ns3dError, match="faithful=False"):
        driver.run_navierstokes3D(nx=24, nt=1, advection="maccormack")
    with pytest.raises(L.Ns3dError, match="faithful=False"):
        driver.runme(nx=24, nt=1, advection="maccormack")
    with pytest.raises(L.Ns3dError, match="reference.*maccormack"):
        driver.run_navierstokes3D(nx=24, nt=1, advection="weno")
    p0 = multi_params(24)
    mg = MultiGpu.create([0, 0], p0.nx, p0.ny, p0.nz, "strict")
    try:
        with pytest.raises(L.Ns3dError, match="one rank"):
            driver.run_navierstokes3D(nx=24, nt=1, faithful=False, advection="maccormack", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz))
    finally:
        mg.close()
    p = multi_params(24)
    f = driver._alloc(p.nx, p.ny, p.nz, torch.float64, torch.device("cuda", 0))
    f.Vx[...] = 0.5
    f.C[...] = 0.25
    names = ("Vx", "Vy", "Vz", "C", "Vx_o", "Vy_o", "Vz_o", "C_o", "Pr")
    before = {n: hip.to_numpy(getattr(f, n)) for n in names}
    ctx = hip.Context(0, "strict", async_=True)
    ctx.set_advection("maccormack")
    with pytest.raises(L.Ns3dError, match="status 1.*faithful == 0"):
        hip.time_step(f, driver._step_params(L.NS3D_BC_MULTI, p, 10, True, "pt"), ctx=ctx)
    ctx.sync()
    for n in names:
        assert bits_equal(hip.to_numpy(getattr(f, n)), before[n]), n
    ctx.close()


# ---- the whole step against its CPU statement (oracle/driver_ref.py with advection=…, tests/test_advect_mc_host.py::ref_run) -----------
STATE = FIELD_NAMES + ("Vx_o", "Vy_o", "Vz_o", "C_o", "dPrdtau", "divV", "txx", "tyy", "tzz", "txy", "txz", "tyz")
RUNME_CAP = 200                      # niter_cap of the runme cases, as in test_runme_with_maccormack above


def device_run(hip, script, nt, advection, one_call, mode="strict", dtype=torch.float64, pressure="pt"):
    """({name: host array} of the full local state, info) of run_navierstokes3D ("multi") or runme ("gpu") at nx = 24, faithful=False"""
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    kw = dict(nx=24, nt=nt, mode=mode, faithful=False, advection=advection, one_call=one_call, dtype=dtype, pressure=pressure)
    if script == "multi":
        info = run_navierstokes3D(return_info=True, **kw)[-1]
        f = info.fields
    else:
        f, info = runme(niter_cap=RUNME_CAP, **kw)
    assert tuple(f.C.shape) == (24, 15, 15)
    return {n: hip.to_numpy(getattr(f, n)) for n in STATE}, info


def cpu_run(script, nt, advection, dtype=np.float64, pressure="pt"):
    _, info, f = ref_run(script, nt, advection, False, dtype, pressure, RUNME_CAP if script == "gpu" else None)
    return f, info


def assert_state(got, want, what, names=STATE):
    for n in names:
        assert bits_equal(got[n], want[n]), (what, n, first_bit_difference(got[n], want[n]))


NT = {"multi": 3, "gpu": 2}


@pytest.mark.parametrize("one_call", [True, False], ids=["one_call", "call_by_call"])
@pytest.mark.parametrize("advection", ["maccormack", "reference"])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_driver_equals_the_oracle_driver(hip, oracle, script, advection, one_call):
    """run_navierstokes3D(nx=24, nt=3) and runme(nx=24, nt=2), faithful=False, STRICT, fp64, on one rank, in both forms of the step and
    with both schemes, against run_navierstokes3D_ref / runme_ref with the same options: C, Pr, Vx, Vy, Vz — and the previous fields,
    dPrdτ, divV and the six stresses, all as full local arrays — bit for bit, iteration counts and error histories equal.  (With the
    reference scheme this is also the suite's one-rank comparison of faithful=False with the oracle driver.)"""
    got, info = device_run(hip, script, NT[script], advection, one_call)
    want, winfo = cpu_run(script, NT[script], advection)
    assert info.iters == winfo.iters and len(info.iters) == NT[script], (info.iters, winfo.iters)
    assert [list(e) for e in info.errs] == [list(e) for e in winfo.errs], (info.errs, winfo.errs)
    assert_state(got, want, (script, advection, one_call))
    assert info.ctx.advection() == "reference" or script == "gpu"      # run_navierstokes3D puts the default back; runme's context is its own


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_driver_with_direct_pressure_and_maccormack(hip, script):
    """pressure="direct": the two solves differ in summation order, so the comparison with the oracle driver of the same options
    is that of tests/test_gpu_direct.py — its helper, its norm, its bar 1e-9 — while the two forms of the device's step, which go
    through the same entry points, agree bit for bit whatever the bar.
    multi.jl's script is held to the bar at nx = 36 (36×22×22, three steps: the size that test uses), not at 24: at nx = 24 the
    reference's outlet test `xve_g == lx/2` is false in floating point (App. B10), the pressure problem is the singular all-Neumann
    one, and the helper's first assertion — the residual of the direct solution below 1e-8 — fails in the ORACLE's own run, with
    either scheme (3.0e-4 and 7.5e-4 in steps 2 and 3).  The bit comparison of the two forms runs at 24 for both scripts."""
    from test_gpu_direct import _direct_driver_against_the_oracle_driver
    _direct_driver_against_the_oracle_driver(hip, script, 36 if script == "multi" else 24, NT[script], faithful=False, advection="maccormack")
    one, i1 = device_run(hip, script, NT[script], "maccormack", True, pressure="direct")
    seq, i2 = device_run(hip, script, NT[script], "maccormack", False, pressure="direct")
    assert i1.iters == i2.iters == [0] * NT[script] and i1.errs == i2.errs
    assert_state(one, seq, (script, "direct"))


def test_fast_step_is_the_call_sequence(hip):
    """FAST: ns3d_time_step with the knob on and the step call by call go through the same entry points — the same bits.  No
    comparison with the CPU here: the limiter's comparisons may fall the other way on FAST's values."""
    one, i1 = device_run(hip, "multi", 3, "maccormack", True, mode="fast")
    seq, i2 = device_run(hip, "multi", 3, "maccormack", False, mode="fast")
    assert i1.iters == i2.iters and i1.errs == i2.errs
    assert_state(one, seq, "fast")
    assert all(np.isfinite(a).all() for a in one.values()) and one["C"].min() >= 0.0 and one["C"].max() <= 1.0


def test_float32_step_is_the_call_sequence(hip, oracle):
    """fp32, STRICT, multi.jl's script, three steps — the largest nt ≤ 3 at which the oracle driver's float32 fields are all finite
    (tests/test_advect_mc_host.py::test_float32_steps_that_stay_finite; gpu.jl's script does not get through one step in float32 and
    is left to the single-call tests): the one-call form equals the call-by-call form, finite, and both equal the oracle driver."""
    one, i1 = device_run(hip, "multi", 3, "maccormack", True, dtype=torch.float32)
    seq, i2 = device_run(hip, "multi", 3, "maccormack", False, dtype=torch.float32)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in one.values())
    assert i1.iters == i2.iters and i1.errs == i2.errs
    assert_state(one, seq, "float32")
    want, winfo = cpu_run("multi", 3, "maccormack", np.float32)
    assert all(np.isfinite(want[n]).all() for n in FIELD_NAMES)
    assert i1.iters == winfo.iters
    assert_state(one, want, "float32 against the oracle driver", FIELD_NAMES)


def _ieee_steps(hip, nt, one_call):
    """nt steps of multi.jl's script at 24×15×15 on a STRICT context with NS3D_IEEE_DIV (the drivers have no keyword for it): as
    ns3d_time_step with the knob on, or call by call with the driver's own helpers"""
    from navierstokes3d_amd import driver as Dr, lib as L
    from navierstokes3d_amd.params import multi_params
    p = multi_params(24)
    ctx = hip.Context(0, "strict", async_=True, ieee_div=True)
    f = Dr._alloc(p.nx, p.ny, p.nz, torch.float64, torch.device("cuda", 0))
    f.Vy[0, :, :] = p.vin
    torch.cuda.synchronize()
    cyl = (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, *cyl, ctx=ctx)
    sp = Dr._step_params(L.NS3D_BC_MULTI, p, p.niter, False, "pt")
    pt = hip.pt_params(f.Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI, p.owns_outlet, 0.0, p.g)
    hats = None
    if one_call:
        ctx.set_advection("maccormack")
    else:
        hats = Dr._alloc_hats(f, ctx)
    record = []
    for it in range(1, nt + 1):
        if one_call:
            sp.write_stress = 1 if it == nt else 0
            record.append(hip.time_step(f, sp, ctx=ctx))
            continue
        if it == nt:
            hip.update_tau(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, p.mu, p.dx, p.dy, p.dz, ctx=ctx)
        Dr._predict_swap(f, p, ctx)
        hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, *cyl, ctx=ctx)
        hip.update_divV(f.divV, f.Vx, f.Vy, f.Vz, p.dx, p.dy, p.dz, ctx=ctx)
        record.append(hip.pt_solve(f.Pr, f.dPrdtau, f.divV, pt, p.eps, p.niter, p.nchk, p.ly * p.ly, p.psc, ctx=ctx))
        hip.correct_V(f.Vx, f.Vy, f.Vz, f.Pr, p.dt, p.rho, p.dx, p.dy, p.dz, ctx=ctx)
        hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, *cyl, ctx=ctx)
        hip.set_bc_Vel_multi(f.Vx, f.Vy, f.Vz, p.owns_inlet, p.vin, ctx=ctx)
        Dr._advect_mc_swap(f, hats, p, ctx)
    ctx.sync()
    out = {n: hip.to_numpy(getattr(f, n)) for n in STATE}
    ctx.close()
    return out, [it for it, _ in record], [list(e) for _, e in record]


def test_ieee_div_step_is_the_call_sequence_and_the_oracle_driver(hip, oracle):
    """NS3D_IEEE_DIV: the one-call step equals the call-by-call step, and both equal the CPU statement — its divisions are IEEE's"""
    one, it1, e1 = _ieee_steps(hip, 3, True)
    seq, it2, e2 = _ieee_steps(hip, 3, False)
    assert it1 == it2 and e1 == e2
    assert_state(one, seq, "ieee_div")
    want, winfo = cpu_run("multi", 3, "maccormack")
    assert it1 == winfo.iters and e1 == [list(e) for e in winfo.errs]
    assert_state(one, want, "ieee_div against the oracle driver")


def _knob_step(hip, ctx, before=lambda: None):
    """one ns3d_time_step of multi.jl's script at 24×15×15 on ctx AS ITS KNOB STANDS, `before` called right in front of it"""
    from navierstokes3d_amd import driver as Dr, lib as L
    from navierstokes3d_amd.params import multi_params
    p = multi_params(24)
    f = Dr._alloc(p.nx, p.ny, p.nz, torch.float64, torch.device("cuda", 0))
    f.Vy[0, :, :] = p.vin
    torch.cuda.synchronize()
    hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz, p.dx, p.dy,
                     p.dz, ctx=ctx)
    sp = Dr._step_params(L.NS3D_BC_MULTI, p, p.niter, False, "pt")
    sp.write_stress = 1
    before()
    hip.time_step(f, sp, ctx=ctx)
    ctx.sync()
    return {n: hip.to_numpy(getattr(f, n)) for n in STATE}


def test_the_knob_belongs_to_its_context(hip, oracle):
    """Two contexts, one with each scheme, set in both orders and stepped in both orders with the other's knob touched last: each
    advects with its OWN scheme — the CPU statement's bits of one step — and creating or closing a context changes nothing."""
    want = {a: cpu_run("multi", 1, a)[0] for a in ("maccormack", "reference")}
    assert not bits_equal(want["maccormack"]["Vx"], want["reference"]["Vx"])
    mc, ref = hip.Context(0, "strict", async_=True), hip.Context(0, "strict", async_=True)
    mc.set_advection("maccormack")
    ref.set_advection("reference")                                   # the last call of the process says "reference"
    assert_state(_knob_step(hip, mc), want["maccormack"], "the MacCormack context, the other one set last")
    assert_state(_knob_step(hip, ref), want["reference"], "the reference context")
    mc.set_advection("maccormack")                                   # the last call of the process says "maccormack"
    assert_state(_knob_step(hip, ref), want["reference"], "the reference context, the other one set last")
    assert_state(_knob_step(hip, mc, before=lambda: ref.set_advection("reference")), want["maccormack"], "set on the other one right before the step")
    fresh = hip.Context(0, "strict")                                 # a new context starts with the default and leaves the others alone
    assert fresh.advection() == "reference" and mc.advection() == "maccormack"
    fresh.set_advection("maccormack")
    fresh.close()
    assert_state(_knob_step(hip, ref), want["reference"], "after another context came and went")
    mc.close(); ref.close()


# ---- the harnesses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_in_a_guarded_arena(hip, form, monkeypatch):
    """twelve arrays at element alignment with guard gaps between them: guards intact, the bits of ordinary allocations"""
    select(form, monkeypatch)
    grid, cfl, dtype = (70, 6, 7), 2.7, np.float64
    old, dt, g, want, want_hat = reference(grid, cfl, dtype)
    arrays = [(n, a, True) for n, a in zip(NEW, garbage(old, 300))] + [(n, a, False) for n, a in zip(OLD, old)] + \
             [(n, a, True) for n, a in zip(HAT, garbage(old, 400))]
    A = Arena(arrays)
    ctx = hip.Context(0, "strict")
    torch.cuda.synchronize()
    hip.advect_mc(*interleave([A[n] for n in NEW], [A[n] for n in OLD], [A[n] for n in HAT]), dt, g["dx"], g["dy"], g["dz"], ctx=ctx)
    ctx.sync()
    A.assert_clean("advect_mc %s" % form)
    assert_bits([A.get(n) for n in NEW], want, "advect_mc in the arena")
    assert_bits([A.get(n) for n in HAT], want_hat, "hat in the arena")
    assert_bits([A.get(n) for n in OLD], old, "inputs in the arena")
    ctx.close()


def test_blob_on_the_device(hip):
    """the convergence case of tests/test_advect_mc_host.py on the device, with its thresholds: advect_mc (and copy_advect for the
    first-order scheme) with the uniform velocities passed in afresh every step; only C is carried over"""
    ctx = hip.Context(0, "strict", async_=True)
    err, lo, hi = {}, 0.0, 0.0
    for n in (48, 96):
        C0, V, dt, dx, steps, exact = MC.blob_setup(n)
        dV = [hip.from_numpy(a) for a in V]
        for name in ("mc", "first"):
            cur = hip.from_numpy(C0)
            new = [hip.zeros(tuple(a.shape)) for a in V] + [hip.zeros(C0.shape)]
            hat = [hip.zeros(tuple(a.shape)) for a in V] + [hip.zeros(C0.shape)]
            for _ in range(steps):
                if name == "mc":
                    hip.advect_mc(*interleave(new, dV + [cur], hat), dt, dx, dx, dx, ctx=ctx)
                else:
                    hip.copy_advect(new[0], dV[0], new[1], dV[1], new[2], dV[2], new[3], cur, dt, dx, dx, dx, False, ctx=ctx)
                cur, new[3] = new[3], cur
                if name == "mc":
                    lo, hi = min(lo, float(cur.min())), max(hi, float(cur.max()))
            ctx.sync()
            err[name, n] = MC.rms(hip.to_numpy(cur), exact)
    ctx.close()
    check_blob(err, lo, hi)
