"""GPU tests of ns3d_sample and ns3d_tracers_advance (include/ns3d.h): point samples of a field and Lagrangian tracer particles.

The reference is the header's NumPy expression (tests/tracers_ref.py), computed once per case and shared, never modified.  The
library must return its bits — positions, states and velocities — for fp64 and fp32 fields, in every arithmetic mode alike: the
calls are never contracted.  k_tracers / k_sample give one thread to a particle in 256-thread workgroups: the particle counts
straddle a wave and a workgroup.  The launch does not cap its grid, so there is no capped case."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import tracers_ref as TR
from util import bits_equal, fields, first_bit_difference, hostile

pytestmark = pytest.mark.gpu

NPDT = {"f64": np.float64, "f32": np.float32}
GRIDS = [(3, 3, 3), (4, 3, 5), (17, 9, 5), (66, 5, 4), (131, 66, 37)]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 4099]
GID = lambda n: "%dx%dx%d" % n
SMALL, LARGE = (0.4, 0.36, 0.32), (2.5, 2.25, 2.0)
LAYOUTS = (("c", (0, 0, 0)), ("vx", (1, 0, 0)), ("vy", (0, 1, 0)), ("vz", (0, 0, 1)))


@functools.lru_cache(maxsize=None)
def velocity_fields(n, dt, values="seeded"):
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=NPDT[dt])
    if values == "nonfinite":           # 2 % NaN, 1 % +Inf, 1 % −Inf
        rng = np.random.Generator(np.random.MT19937(77))
        V = [a.copy(order="F") for a in V]
        for a in V:
            r = rng.uniform(size=a.shape)
            a[r < 0.02] = np.nan
            a[(r >= 0.02) & (r < 0.03)] = np.inf
            a[(r >= 0.03) & (r < 0.04)] = -np.inf
    elif values != "seeded":
        V = [hostile(a, 5 + q, values) for q, a in enumerate(V)]
    return tuple(V)


@functools.lru_cache(maxsize=None)
def points(n, N):
    """(X, state): N uniform points; from 255 on the planted points (tracers_ref.planted_points) take the place of the last ones,
    and one uniform point in five is dead"""
    X = TR.uniform_points(n, N, 11 + N)
    rng = np.random.Generator(np.random.MT19937(N))
    state = (rng.uniform(size=N) < 0.8).astype(np.uint8)
    if N >= 255:
        P, ps = TR.planted_points(n)
        X[:, -P.shape[1]:] = P
        state[-P.shape[1]:] = ps
    return X, state


@functools.lru_cache(maxsize=None)
def advance_case(n, dt, N, c, values="seeded"):
    """X, state, reference (Xn, state_n, U) — shared, never modified"""
    X, state = points(n, N)
    return X, state, TR.advance(X, state, *velocity_fields(n, dt, values), c)


@pytest.fixture(scope="module")
def ctxs(hip):
    c = {"strict": hip.Context(0, "strict"), "ieee": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield c
    for x in c.values():
        x.close()


@functools.lru_cache(maxsize=None)
def _device_fields(n, dt, values="seeded"):
    from navierstokes3d_amd import kernels as K
    return tuple(K.from_numpy(a) for a in velocity_fields(n, dt, values))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_advance(hip, ctx, n, dt, X, state, c, values="seeded", with_u=True):
    Vd = _device_fields(n, dt, values)
    Xd, sd = dev(X), dev(state)
    Ud = torch.full((3, X.shape[1]), 777.0, dtype=torch.float64, device="cuda") if with_u else None
    hip.tracers_advance(Xd, sd, *Vd, *c, U=Ud, ctx=ctx)
    ctx.sync()
    return Xd.cpu().numpy(), sd.cpu().numpy(), None if Ud is None else Ud.cpu().numpy()


def assert_step(got, ref, what):
    Xg, sg, Ug = got
    Xr, sr, Ur = ref
    assert bits_equal(Xg, Xr), (what, "X", first_bit_difference(Xg, Xr))
    assert np.array_equal(sg, sr), (what, "state", int((sg != sr).sum()))
    if Ug is not None:
        assert bits_equal(Ug, Ur), (what, "U", first_bit_difference(Ug, Ur))


def fields_untouched(hip, n, dt, values="seeded"):
    for a, t in zip(velocity_fields(n, dt, values), _device_fields(n, dt, values)):
        assert bits_equal(hip.to_numpy(t), a), "a field was modified"


def crossed_share(n, X, ref):
    """share of the particles — all of them inside and alive at the start — that leave their cell or the box"""
    Xn, sn, _ = ref
    fin = np.isfinite(Xn).all(axis=0)
    moved = (TR.cell_of(X, n) != TR.cell_of(np.where(fin, Xn, 0.0), n)).any(axis=0) | (sn == 0)
    return float(moved.mean())


# ---- 1. ns3d_sample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_sample_returns_the_bits_of_the_reference(hip, ctxs, n, dt):
    A = dict(zip(("vx", "vy", "vz"), velocity_fields(n, dt)))
    A["c"] = fields(*n, ("c",), seed0=9, dtype=NPDT[dt])[0]
    Ad = {k: hip.from_numpy(a) for k, a in A.items()}
    for N in COUNTS:
        X, state = points(n, N)
        Xd, sd = dev(X), dev(state)
        for kind, stag in LAYOUTS:
            for st, std in ((None, None), (state, sd)):
                out = torch.full((N,), 777.0, dtype=torch.float64, device="cuda")
                hip.sample(Ad[kind], Xd, out, state=std, stagger=stag, ctx=ctxs["strict"])
                ctxs["strict"].sync()
                got, ref = out.cpu().numpy(), TR.sample(A[kind], X, st, stag)
                assert bits_equal(got, ref), (n, dt, N, kind, st is None, first_bit_difference(got, ref))
                assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert bits_equal(Xd.cpu().numpy(), X) and np.array_equal(sd.cpu().numpy(), state)
    for k in A:
        assert bits_equal(hip.to_numpy(Ad[k]), A[k]), "the field was modified"
    # the largest case has every planted decision in it, NaN results included
    assert np.isnan(TR.sample(A["c"], *points(n, 4099))).sum() > 30


# ---- 2. ns3d_tracers_advance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_advance_returns_the_bits_of_the_reference(hip, ctxs, n, dt):
    for c in (SMALL, LARGE):
        # both outcomes are exercised — asserted on the reference, with every particle alive at the start
        X = TR.uniform_points(n, 4099, 11)
        ones = np.ones(4099, dtype=np.uint8)
        ref = TR.advance(X, ones, *velocity_fields(n, dt), c)
        alive, crossed = float(ref[1].mean()), crossed_share(n, X, ref)
        print("%s %s c = %r: %.1f %% alive, %.1f %% crossed" % (GID(n), dt, c, 100 * alive, 100 * crossed))
        assert crossed >= 0.25, (n, c, crossed)
        if n == (17, 9, 5) and c == LARGE:
            assert 1.0 - alive >= 0.05 and alive >= 0.50, alive
        assert_step(run_advance(hip, ctxs["strict"], n, dt, X, ones, c), ref, (n, dt, c, "uniform"))
        for N in COUNTS:
            X, state, ref = advance_case(n, dt, N, c)
            got = run_advance(hip, ctxs["strict"], n, dt, X, state, c)
            assert_step(got, ref, (n, dt, N, c))
            inactive = np.isnan(ref[2][0])
            assert np.array_equal(got[0][:, inactive].view(np.uint64), X[:, inactive].view(np.uint64))   # NaN payloads kept too
            nou = run_advance(hip, ctxs["strict"], n, dt, X, state, c, with_u=False)                    # U = NULL: same X and state
            assert nou[2] is None
            assert_step(nou, ref, (n, dt, N, c, "U = NULL"))
    fields_untouched(hip, n, dt)


# ---- 3. chained steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [(17, 9, 5), (131, 66, 37)], ids=GID)
def test_ten_chained_steps(hip, ctxs, n, dt):
    V, Vd = velocity_fields(n, dt), _device_fields(n, dt)
    X, state = points(n, 4099)
    Xd, sd = dev(X), dev(state)
    Ud = torch.full((3, 4099), 777.0, dtype=torch.float64, device="cuda")
    Xr, sr = X, state
    for step in range(10):
        c = LARGE if step % 2 else SMALL
        hip.tracers_advance(Xd, sd, *Vd, *c, U=Ud, ctx=ctxs["strict"])
        Xn, sn, Un = TR.advance(Xr, sr, *V, c)
        ctxs["strict"].sync()
        assert_step((Xd.cpu().numpy(), sd.cpu().numpy(), Ud.cpu().numpy()), (Xn, sn, Un), (n, dt, step))
        assert not (sn > sr).any()                                                   # state only ever goes 1 → 0
        dead = sr == 0
        assert np.array_equal(Xn[:, dead].view(np.uint64), Xr[:, dead].view(np.uint64))   # dead particles keep their coordinates
        Xr, sr = Xn, sn
    assert 0 < sr.sum() < state.sum()
    fields_untouched(hip, n, dt)


# ---- 4. arithmetic modes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_strict_ieee_div_and_fast_contexts_return_identical_bits(hip, ctxs, dt):
    n = (17, 9, 5)
    assert ctxs["fast"].arith_build(0.1, 0.1, 0.1) == "fast" and ctxs["ieee"].arith_build(0.1, 0.1, 0.1) == "strict"
    for c in (SMALL, LARGE):
        X, state, ref = advance_case(n, dt, 4099, c)
        for name, ctx in ctxs.items():
            assert_step(run_advance(hip, ctx, n, dt, X, state, c), ref, (name, dt, c))
    A, Ad = velocity_fields(n, dt)[0], _device_fields(n, dt)[0]
    X, state = points(n, 4099)
    ref = TR.sample(A, X, state, (1, 0, 0))
    for name, ctx in ctxs.items():
        out = torch.full((4099,), 777.0, dtype=torch.float64, device="cuda")
        hip.sample(Ad, dev(X), out, state=dev(state), stagger=(1, 0, 0), ctx=ctx)
        ctx.sync()
        assert bits_equal(out.cpu().numpy(), ref), (name, dt)


# ---- 5. hostile fields ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("values", ["dense", "blocks", "rest0", "nonfinite"])
@pytest.mark.parametrize("n", [(17, 9, 5), (131, 66, 37)], ids=GID)
def test_hostile_fields(hip, ctxs, n, values, dt):
    for c in (SMALL, LARGE):
        X, state, ref = advance_case(n, dt, 4099, c, values)
        got = run_advance(hip, ctxs["strict"], n, dt, X, state, c, values)
        assert_step(got, ref, (n, dt, values, c))
        act = (state == 1) & TR.inside(X, n)
        if values == "dense":                   # velocities up to 1e300 (fp32: 1e30) carry particles far outside: stored there, dead
            far = (np.abs(ref[0]) > 1e20).any(axis=0) & act
            assert far.sum() > 10 and np.isfinite(ref[0][:, far]).all() and not got[1][far].any()
        if values == "nonfinite":               # NaN and ±Inf velocities: the particle dies, what was stored equals the reference
            bad = ~np.isfinite(ref[0]).all(axis=0) & act
            assert bad.sum() > 100 and not ref[1][bad].any() and not got[1][bad].any()
            assert np.isinf(ref[0][:, bad]).any() and np.isnan(ref[0][:, bad]).any()
            assert (act & ~bad & (ref[1] == 1)).sum() > 100             # and the others go on
        if values == "rest0":                   # a field at rest: every position stays (−0.0 + 0.0 is +0.0), every active particle lives
            assert np.array_equal(got[0], X, equal_nan=True)
            keep = ~((X == 0.0) & np.signbit(X))
            assert np.array_equal(got[0].view(np.uint64)[keep], X.view(np.uint64)[keep])
            assert np.array_equal(got[1], ((state == 1) & TR.inside(X, n)).astype(np.uint8))
    fields_untouched(hip, n, dt, values)


# ---- 6. error paths ------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n, N = (3, 3, 3), 65
    V = velocity_fields(n, "f64")
    Vd = [hip.from_numpy(a) for a in V]
    X, state = points(n, N)
    fill = lambda shape, dtype=torch.float64: torch.full(shape, 777, dtype=dtype, device="cuda")
    Xd, sd, Ud, od = fill((3, N)), torch.full((N,), 77, dtype=torch.uint8, device="cuda"), fill((3, N)), fill((N,))   # a byte holds 77
    P = lambda t: C.c_void_p(t.data_ptr())
    D = lambda *xs: [C.c_double(x) for x in xs]
    h = ctxs["strict"].handle
    Vp, ok, nl = [P(t) for t in Vd], D(*SMALL), C.c_long(N)
    adv, smp = lib.ns3d_tracers_advance_f64, lib.ns3d_sample_f64
    nan, inf = float("nan"), float("inf")
    calls = {
        "adv null context": lambda: adv(None, P(Xd), P(sd), P(Ud), nl, *Vp, *ok, 3, 3, 3),
        "adv null X": lambda: adv(h, None, P(sd), P(Ud), nl, *Vp, *ok, 3, 3, 3),
        "adv null state": lambda: adv(h, P(Xd), None, P(Ud), nl, *Vp, *ok, 3, 3, 3),
        "adv null Vx": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, None, Vp[1], Vp[2], *ok, 3, 3, 3),
        "adv null Vy": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, Vp[0], None, Vp[2], *ok, 3, 3, 3),
        "adv null Vz": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, Vp[0], Vp[1], None, *ok, 3, 3, 3),
        "adv n < 0": lambda: adv(h, P(Xd), P(sd), P(Ud), C.c_long(-1), *Vp, *ok, 3, 3, 3),
        "adv grid 2x3x3": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *ok, 2, 3, 3),
        "adv grid 3x2x3": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *ok, 3, 2, 3),
        "adv grid 3x3x2": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *ok, 3, 3, 2),
        "adv cx nan": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *D(nan, 0.3, 0.3), 3, 3, 3),
        "adv cy inf": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *D(0.3, inf, 0.3), 3, 3, 3),
        "adv cz -inf": lambda: adv(h, P(Xd), P(sd), P(Ud), nl, *Vp, *D(0.3, 0.3, -inf), 3, 3, 3),
        "smp null context": lambda: smp(None, P(od), P(Xd), P(sd), nl, Vp[0], 4, 3, 3, 1, 0, 0),
        "smp null out": lambda: smp(h, None, P(Xd), P(sd), nl, Vp[0], 4, 3, 3, 1, 0, 0),
        "smp null X": lambda: smp(h, P(od), None, P(sd), nl, Vp[0], 4, 3, 3, 1, 0, 0),
        "smp null field": lambda: smp(h, P(od), P(Xd), P(sd), nl, None, 4, 3, 3, 1, 0, 0),
        "smp n < 0": lambda: smp(h, P(od), P(Xd), P(sd), C.c_long(-5), Vp[0], 4, 3, 3, 1, 0, 0),
        "smp extents 1x3x3": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 1, 3, 3, 1, 0, 0),
        "smp extents 4x1x3": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 4, 1, 3, 1, 0, 0),
        "smp extents 4x3x1": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 4, 3, 1, 1, 0, 0),
        "smp stagger 2": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 4, 3, 3, 2, 0, 0),
        "smp stagger -1": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 4, 3, 3, 0, -1, 0),
        "smp stagger 3": lambda: smp(h, P(od), P(Xd), P(sd), nl, Vp[0], 4, 3, 3, 0, 0, 3),
    }
    for what, call in calls.items():
        assert call() == L.NS3D_ERR_ARG == 1, what
        who = "ns3d_tracers_advance_f64: " if what.startswith("adv") else "ns3d_sample_f64: "
        assert L.last_error().startswith(who), (what, L.last_error())
    ctxs["strict"].sync()
    for t in (Xd, Ud, od):
        assert bool((t == 777.0).all())
    assert bool((sd == 77).all())
    # n == 0 is a successful no-op, for both element types; extents of 2 are enough for a sample
    for suf in ("f64", "f32"):
        assert getattr(lib, "ns3d_tracers_advance_" + suf)(h, P(Xd), P(sd), P(Ud), C.c_long(0), *Vp, *ok, 3, 3, 3) == L.NS3D_OK
        assert getattr(lib, "ns3d_sample_" + suf)(h, P(od), P(Xd), None, C.c_long(0), Vp[0], 4, 3, 3, 1, 0, 0) == L.NS3D_OK
        assert getattr(lib, "ns3d_sample_" + suf)(None, P(od), P(Xd), None, nl, Vp[0], 4, 3, 3, 1, 0, 0) == L.NS3D_ERR_ARG
        assert L.last_error() == "ns3d_sample_%s: null context" % suf
    ctxs["strict"].sync()
    for t in (Xd, Ud, od):
        assert bool((t == 777.0).all())
    assert bool((sd == 77).all())
    two = hip.from_numpy(np.asfortranarray(np.arange(8.0).reshape(2, 2, 2, order="F")))
    pts = dev(np.array([[0.5, 1.0, 1.5], [0.5, 1.0, 1.5], [0.5, 1.0, 1.5]]))
    out = fill((3,))
    hip.sample(two, pts, out, ctx=ctxs["strict"])
    ctxs["strict"].sync()
    assert out.cpu().tolist() == [0.0, 3.5, 7.0]
    # the wrapper refuses what the library cannot see: shapes, dtypes, host arrays
    with pytest.raises(L.Ns3dError):
        hip.tracers_advance(fill((3, N + 1)), sd, *Vd, *SMALL, ctx=ctxs["strict"])
    with pytest.raises(L.Ns3dError):
        hip.tracers_advance(Xd, sd.to(torch.float64), *Vd, *SMALL, ctx=ctxs["strict"])
    with pytest.raises(L.Ns3dError):
        hip.sample(Vd[0], Xd.cpu(), od, ctx=ctxs["strict"])
    with pytest.raises(L.Ns3dError):
        hip.sample(Vd[0], Xd, od.to(torch.float32), ctx=ctxs["strict"])
    # the context is still usable
    ref = TR.advance(X, state, *V, SMALL)
    Xd, sd = dev(X), dev(state)
    hip.tracers_advance(Xd, sd, *Vd, *SMALL, U=Ud, ctx=ctxs["strict"])
    ctxs["strict"].sync()
    assert_step((Xd.cpu().numpy(), sd.cpu().numpy(), Ud.cpu().numpy()), ref, "after the errors")


# ---- 7. drivers ------------------------------------------------------------------------------------------------------------------------
def _physical(p, X):
    """tracers.Tracers.positions: origin + ξ·d with the box's low corner at (−lx/2, −ly/2, −lz/2)"""
    o, d = (-p.lx / 2, -p.ly / 2, -p.lz / 2), (p.dx, p.dy, p.dz)
    return [o[q] + X[q] * d[q] for q in range(3)]


def _index(p, xyz):
    o, d = (-p.lx / 2, -p.ly / 2, -p.lz / 2), (p.dx, p.dy, p.dz)
    return np.ascontiguousarray(np.stack([(xyz[:, q] - o[q]) / d[q] for q in range(3)]))


def _check_observers(hip, f, p, info, X0, probes_xyz, nt):
    """nt = 1: one reference step through the returned final fields / the reference samples of those fields"""
    V = [hip.to_numpy(getattr(f, nm)) for nm in ("Vx", "Vy", "Vz")]
    Xn, sn, _ = TR.advance(X0, TR.inside(X0, (p.nx, p.ny, p.nz)).astype(np.uint8), *V, (p.dt / p.dx, p.dt / p.dy, p.dt / p.dz))
    t = info.tracers
    assert t.steps == nt == 1
    for got, want, nm in zip((t.x, t.y, t.z), _physical(p, Xn), "xyz"):
        assert bits_equal(got, want), (nm, first_bit_difference(got, want))
    assert np.array_equal(t.alive, sn == 1) and t.alive.dtype == bool
    Xp = _index(p, probes_xyz)
    for nm, field, stag in (("u", V[0], (1, 0, 0)), ("v", V[1], (0, 1, 0)), ("w", V[2], (0, 0, 1)), ("p", hip.to_numpy(f.Pr), (0, 0, 0))):
        got = getattr(info.probes, nm)
        assert got.shape == (1, Xp.shape[1]) and got.dtype == np.float64
        want = TR.sample(field, Xp, None, stag)
        assert bits_equal(got[0], want), (nm, first_bit_difference(got[0], want))
    assert np.isnan(info.probes.u[0, -1]) and np.isfinite(info.probes.u[0, :-1]).all()      # the last probe sits outside the box
    assert np.abs(info.probes.u[0, :-1]).max() > 0 and (Xn != X0).any()


def _probe_points(p):
    rng = np.random.Generator(np.random.MT19937(21))
    ext = np.array([p.lx, p.ly, p.lz])
    xyz = (rng.uniform(0.02, 0.98, size=(9, 3)) - 0.5) * ext
    xyz[-1] = ext                                                       # outside
    return xyz


def test_multi_driver_on_one_rank(hip):
    from navierstokes3d_amd.driver import run_navierstokes3D
    from util import assert_bit_identical, errs_identical
    kw = dict(nx=24, mode="strict", niter_cap=40, return_info=True)
    plain = {nt: run_navierstokes3D(nt=nt, **kw) for nt in (1, 3)}
    p = plain[1][-1].params
    assert not hasattr(plain[1][-1], "tracers") and not hasattr(plain[1][-1], "probes")
    probes = _probe_points(p)
    for extra in (dict(), dict(one_call=False)):
        out = run_navierstokes3D(nt=1, tracers=300, probes=probes, **extra, **kw)
        assert_bit_identical(out[:5], plain[1][:5])
        assert out[-1].iters == plain[1][-1].iters and errs_identical(out[-1].errs, plain[1][-1].errs)
        _check_observers(hip, out[-1].fields, p, out[-1], TR.uniform_points((p.nx, p.ny, p.nz), 300, 0), probes, 1)
    # start points given as an (N,3) array of physical coordinates
    start = (np.random.Generator(np.random.MT19937(4)).uniform(0.0, 1.0, size=(70, 3)) - 0.5) * np.array([p.lx, p.ly, p.lz])
    out = run_navierstokes3D(nt=1, tracers=start, probes=probes, **kw)
    assert_bit_identical(out[:5], plain[1][:5])
    _check_observers(hip, out[-1].fields, p, out[-1], _index(p, start), probes, 1)
    out = run_navierstokes3D(nt=3, tracers=300, probes=probes, **kw)
    assert_bit_identical(out[:5], plain[3][:5])
    assert out[-1].iters == plain[3][-1].iters and errs_identical(out[-1].errs, plain[3][-1].errs)
    assert out[-1].tracers.steps == 3 and out[-1].tracers.x.shape == (300,)
    for nm in "uvwp":
        a = getattr(out[-1].probes, nm)
        assert a.shape == (3, 9) and np.isfinite(a[:, :-1]).all() and np.isnan(a[:, -1]).all(), nm
    assert (out[-1].probes.u[0] != out[-1].probes.u[2])[:-1].any()


def test_gpu_driver(hip):
    from navierstokes3d_amd.driver import runme
    from util import errs_identical
    kw = dict(nx=24, mode="strict", niter_cap=40)
    same = lambda f, g: all(np.array_equal(hip.to_numpy(getattr(f, nm)), hip.to_numpy(getattr(g, nm)), equal_nan=True)
                            for nm in ("Pr", "C", "Vx", "Vy", "Vz"))
    gf, gi = runme(nt=1, **kw)
    assert not hasattr(gi, "tracers") and not hasattr(gi, "probes")
    probes = _probe_points(gi.params)
    for extra in (dict(), dict(one_call=False)):
        f, info = runme(nt=1, tracers=300, probes=probes, **extra, **kw)
        assert same(f, gf) and info.iters == gi.iters and errs_identical(info.errs, gi.errs)
        _check_observers(hip, f, info.params, info, TR.uniform_points(tuple(f.Pr.shape), 300, 0), probes, 1)
    gf3, gi3 = runme(nt=3, **kw)
    f, info = runme(nt=3, tracers=300, probes=probes, **kw)
    assert same(f, gf3) and info.iters == gi3.iters and errs_identical(info.errs, gi3.errs)
    assert info.tracers.steps == 3 and info.probes.p.shape == (3, 9)


def test_do_save_and_do_vis_write_the_tracer_files(hip, tmp_path, monkeypatch):
    from navierstokes3d_amd.driver import run_navierstokes3D
    kw = dict(do_save=True, do_vis=True, nx=24, nt=3, mode="strict", niter_cap=40)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    run_navierstokes3D(tracers=257, **kw)
    have, drawn = set(os.listdir("out_save")), set(os.listdir("viz3D_out"))
    frames = sorted(nm[len("out_C_v_"):-4] for nm in have if nm.startswith("out_C_v_"))
    assert frames == ["0000"]                                           # nt = 3: the initial state is the one saved frame
    for fr in frames:                                                   # one dump per saved frame
        nm = "out_tracers_%s.bin" % fr
        assert nm in have and os.path.getsize(os.path.join("out_save", nm)) == 4 * 4 * 257, nm
    raw = np.fromfile(os.path.join("out_save", "out_tracers_0000.bin"), dtype=np.float32).reshape(257, 4)
    assert np.all(raw[:, 3] == 1.0) and np.abs(raw[:, :3]).max() <= 0.5
    assert "3D_NavierStokes_tracers_0000.png" in drawn
    monkeypatch.chdir(tmp_path / "b")
    run_navierstokes3D(**kw)
    assert have - set(os.listdir("out_save")) == {"out_tracers_0000.bin"}
    assert drawn - set(os.listdir("viz3D_out")) == {"3D_NavierStokes_tracers_0000.png"}


def test_two_ranks_raise(hip):
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    nx, P, nz_loc = 24, 2, 9
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        for kw in (dict(tracers=10), dict(probes=np.zeros((2, 3))), dict(tracers=np.zeros((2, 3)), probes=np.zeros((2, 3)))):
            with pytest.raises(L.Ns3dError, match="one rank"):
                run_navierstokes3D(nx=nx, nt=1, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), shape=dict(nz=nz_loc), **kw)
    finally:
        mg.sync()
        mg.close()
