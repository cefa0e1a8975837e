"""ns3d_advect_mc / ns3d_advect_correct (limited MacCormack advection) on the device, the knob of ns3d_time_step and the drivers'
`advection` keyword.  STRICT is compared bit for bit with tests/advect_mc_ref.py (whose limiter engages in all three ways on these
inputs: tests/test_advect_mc_host.py); FAST with the enclosure of tests/advect_mc_pairs.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import advect_mc_pairs as MP
import advect_mc_ref as MC
import pair_cases as PC
import stream_order as SO
from arena import Arena
from test_advect_mc_host import CFLS, GRIDS, KINDS, check_blob, seeded
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


@pytest.fixture(scope="module")
def delay(hip):
    return SO.Delay()


@pytest.mark.parametrize("form", FORMS)
def test_stream_order_on_a_pinned_stream(hip, delay, form, monkeypatch):
    """late inputs, an early reader and an overwrite behind the call, on a torch stream the context is pinned to"""
    from test_gpu_stream_order import run_cases
    select(form, monkeypatch)
    grid = (70, 6, 7)
    old, dt, g = seeded(grid, 2.7, np.float64)
    arrays = [(n, np.full_like(a, 777.0), "field") for n, a in zip(NEW + HAT, old + old)] + [(n, a, "field") for n, a in zip(OLD, old)]
    case = SO.Case("advect_mc %s %s" % (GID(grid), form), arrays,
                   lambda hip, ctx, t: hip.advect_mc(*interleave([t[n] for n in NEW], [t[n] for n in OLD], [t[n] for n in HAT]), dt, g["dx"],
                                                     g["dy"], g["dz"], ctx=ctx))
    run_cases(hip, [case], "torch", delay)


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
