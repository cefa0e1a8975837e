"""GPU tests of the active scalar (include/ns3d.h): ns3d_scalar_diffuse, ns3d_buoyancy, ns3d_scalar_step, the step under
ns3d_set_scalar and the drivers' `scalar` keyword.

The reference is the header's NumPy statements (tests/scalar_ref.py), computed once per case and shared, never modified.  STRICT must
return their bits, whichever of the three division builds the spacings select; FAST is held, element by element, to the running-error
bound of the same statements; the fused call must equal the two single calls bit for bit in every mode.  k_scalar owns 64×4 cell
columns and NS3D_SCALAR_KZ = 16 planes per workgroup and its stencil reaches one cell: SC_GRIDS has the issue's five grids and one
grid on each side of every tile edge and chunk end (extents ≡ 0, ±1 modulo 64, 4 and 16, one and two tiles each way)."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import les_ref as LR
import running_error as RE
import scalar_ref as SC
import sgs_ref as SR
import stream_order as SO
import test_gpu_les as GL
from util import bits_equal, first_bit_difference, geometry, hostile, rnd

pytestmark = pytest.mark.gpu

NPDT, DTS, GID, SPACINGS = GL.NPDT, GL.DTS, GL.GID, GL.SPACINGS
sentinel, assert_bits = GL.sentinel, GL.assert_bits
EDGE = [(63, 3, 15), (64, 4, 16), (65, 5, 17), (127, 7, 31), (128, 8, 32), (129, 9, 33)]
SC_GRIDS = [(3, 3, 3), (17, 9, 5), (66, 18, 34), (67, 19, 35), (131, 33, 67)] + EDGE
BG, C_REF = 2.5, 0.3


@functools.lru_cache(maxsize=None)
def case(n, dt, kind="geometry", values="seeded"):
    """C, a varying mu_e, Vz, the spacings, kappa and sgs at 0.9 of the explicit limit, and the statements' results with and without
    mu_e — shared, never modified"""
    T = NPDT[dt]
    g = geometry(*n)
    d = GL.spacings_of(n, kind)
    Cf, mu_e, Vz = rnd(31, n, T), rnd(32, n, T, g["mu"], 5 * g["mu"]), rnd(33, (n[0], n[1], n[2] + 1), T)
    if values in ("dense", "blocks", "rest0", "sparse0"):
        Cf, Vz = hostile(Cf, 41, values), hostile(Vz, 43, values)
        if values in ("dense", "blocks"):
            mu_e = hostile(mu_e, 42, values)
    elif values == "nanC":
        Cf = Cf.copy(order="F"); Cf[n[0] // 2, n[1] // 2, n[2] // 2] = np.nan
    elif values == "nanM":
        mu_e = mu_e.copy(order="F"); mu_e[n[0] // 2, n[1] // 2, n[2] // 2] = np.nan
    sgs = 1.0 / (g["rho"] * 0.7)
    kappa = 0.45 / (g["dt"] * SC.sum_inv_d2(*d)) - sgs * 4 * g["mu"]
    assert kappa > 0
    c = SimpleNamespace(n=n, dt=dt, C=Cf, mu_e=mu_e, Vz=Vz, d=d, mu=g["mu"], step=g["dt"], kappa=kappa, sgs=sgs)
    c.out = {True: SC.scalar_diffuse(Cf, mu_e, kappa, sgs, c.mu, c.step, *d), False: SC.scalar_diffuse(Cf, None, kappa, sgs, c.mu, c.step, *d)}
    c.lift = SC.buoyancy(Vz, Cf, BG, C_REF, c.step)
    for a in [Cf, mu_e, Vz, c.lift] + list(c.out.values()):
        a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def ctxs(hip):
    c = {"strict": hip.Context(0, "strict"), "ieee": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def delay(hip):
    return SO.Delay()


def run_three(hip, ctx, c, var, bg=BG, kappa=None, sgs=None, mu_e=None, Cf=None):
    """(C_out of scalar_diffuse, Vz of buoyancy, C_out and Vz of scalar_step) on fresh uploads; the inputs must come back untouched"""
    kappa, sgs = c.kappa if kappa is None else kappa, c.sgs if sgs is None else sgs
    hC, hM = c.C if Cf is None else Cf, c.mu_e if mu_e is None else mu_e
    Cd, Md = hip.from_numpy(hC), hip.from_numpy(hM) if var else None
    out1, out2 = hip.from_numpy(sentinel(c.n, c.dt)), hip.from_numpy(sentinel(c.n, c.dt))
    vz1, vz2 = hip.from_numpy(c.Vz), hip.from_numpy(c.Vz)
    hip.scalar_diffuse(out1, Cd, Md, kappa, sgs, c.mu, c.step, *c.d, ctx=ctx)
    hip.buoyancy(vz1, Cd, bg, C_REF, c.step, ctx=ctx)
    hip.scalar_step(out2, vz2, Cd, Md, kappa, sgs, c.mu, bg, C_REF, c.step, *c.d, ctx=ctx)
    ctx.sync()
    assert bits_equal(hip.to_numpy(Cd), hC) and (not var or bits_equal(hip.to_numpy(Md), hM)), "an input was modified"
    return [hip.to_numpy(t) for t in (out1, vz1, out2, vz2)]


# ---- 1. STRICT bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", SC_GRIDS, ids=GID)
def test_the_three_calls_return_the_bits_of_the_statement(hip, ctxs, n, dt):
    builds = set()
    for kind in SPACINGS:
        c = case(n, dt, kind)
        ctx = ctxs["ieee"] if kind == "ieee" else ctxs["strict"]
        builds.add(ctx.arith_build(*c.d))
        for var in (True, False):
            d1, b1, d2, b2 = run_three(hip, ctx, c, var)
            assert_bits([d1, b1, d2, b2], [c.out[var], c.lift, c.out[var], c.lift], (n, dt, kind, var))
    assert builds == {"strict", "strictx", "strictp"}, builds
    assert not bits_equal(c.out[True], c.out[False]) and not bits_equal(c.out[True], c.C) and not bits_equal(c.lift, c.Vz)


# ---- 2. fused equals the two single calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,values", [((70, 35, 8), "dense"), ((67, 19, 35), "blocks"), ((24, 15, 15), "rest0"), ((66, 18, 34), "sparse0")],
                         ids=str)
def test_fused_equals_the_two_single_calls(hip, ctxs, n, values, dt, mode):
    """bit for bit, NaN and Inf included, with and without mu_e; with bg = 0 the fused call leaves Vz alone"""
    c = case(n, dt, "geometry", values)
    for var in (True, False):
        d1, b1, d2, b2 = run_three(hip, ctxs[mode], c, var)
        assert_bits([d2, b2], [d1, b1], (n, values, dt, mode, var))
        d1, _, d2, b2 = run_three(hip, ctxs[mode], c, var, bg=0.0)
        assert_bits([d2, b2], [d1, np.asarray(c.Vz)], (n, values, dt, mode, var, "bg = 0"))
    Cd, out = hip.from_numpy(c.C), hip.from_numpy(sentinel(n, dt))
    hip.scalar_step(out, None, Cd, None, c.kappa, 0.0, c.mu, 0.0, 0.0, c.step, *c.d, ctx=ctxs[mode])        # Vz may be NULL with bg = 0
    ctxs[mode].sync()
    assert_bits(hip.to_numpy(out), d1, "Vz NULL")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
def test_uniform_mu_e_equal_mu_is_mu_e_null(hip, ctxs, dt, mode):
    n = (67, 19, 35)
    c = case(n, dt)
    m = np.full(n, NPDT[dt](c.mu), dtype=NPDT[dt], order="F")
    with_m = run_three(hip, ctxs[mode], c, True, mu_e=m)
    without = run_three(hip, ctxs[mode], c, False)
    assert_bits([with_m[0], with_m[2]], [without[0], without[2]], (dt, mode))
    zero = run_three(hip, ctxs[mode], c, True, kappa=0.0, sgs=0.0)        # no diffusivity at all: still a full pass, C by value
    assert np.array_equal(zero[0], c.C) and np.array_equal(zero[2], c.C)


# ---- 3. FAST ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,values", [((70, 35, 8), "seeded"), ((67, 19, 35), "blocks"), ((24, 15, 15), "rest0")], ids=str)
def test_fast_within_the_running_error_bound(hip, ctxs, n, values, dt):
    c = case(n, dt, "geometry", values)
    ctx = ctxs["fast"]
    assert ctx.arith_build(*c.d) == "fast"
    for var in (True, False):
        with np.errstate(all="ignore"):
            pd = SC.scalar_diffuse_pairs(c.C, c.mu_e if var else None, c.kappa, c.sgs, c.mu, c.step, *c.d)
            pb = SC.buoyancy_pairs(c.Vz, c.C, BG, C_REF, c.step)
        d1, b1, _, _ = run_three(hip, ctx, c, var)
        for got, ref, pm, what in ((d1, c.out[var], pd, "scalar_diffuse"), (b1, c.lift, pb, "buoyancy")):
            finite = np.isfinite(ref) & np.isfinite(pm.v) & np.isfinite(pm.e)
            sel = lambda a: np.where(finite, a, 0.0)
            worst = RE.check(np.where(finite, got, got.dtype.type(0)), np.where(finite, ref, got.dtype.type(0)),
                             RE.Pair(sel(pm.v), sel(pm.e), pm.u), NPDT[dt], "FAST %s %s %r" % (what, dt, n))
            print("FAST %s %s %r %s mu_e %s: worst err/bound %.3g, %d of %d held to a finite bound" % (what, dt, n, values, var, worst,
                                                                                                        int(finite.sum()), finite.size))
            assert finite.mean() > 0.25


# ---- 4. a single NaN ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("values", ["nanC", "nanM"])
def test_a_single_nan_shows_up_where_the_statement_has_it(hip, ctxs, values, dt):
    n = (70, 35, 8)
    c = case(n, dt, "geometry", values)
    d1, b1, d2, b2 = run_three(hip, ctxs["strict"], c, True)
    for got, want in ((d1, c.out[True]), (d2, c.out[True]), (b1, c.lift), (b2, c.lift)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert_bits(got, want, values)
    assert np.isnan(c.out[True]).sum() == 7 and np.isnan(c.lift).sum() == (2 if values == "nanC" else 0)


# ---- 5. hull and conservation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(5, 4, 3), (17, 9, 5), (67, 19, 35)], ids=GID)
def test_hull_and_conservation(hip, ctxs, n, dt, mode):
    """the bars of tests/test_scalar_host.py, which the CPU statement meets there: |ΣC_out − ΣC| ≤ N·eps·max|C| in fp64; at 0.9 of the
    limit every C_out within the min / max of its 7-point stencil, strictly on random data and within 4 ulp of 1 on 0/1 blocks"""
    c = case(n, dt)
    T = NPDT[dt]
    N, eps = c.C.size, float(np.finfo(T).eps)
    out = run_three(hip, ctxs[mode], c, True)[2]
    drift = abs(float(out.astype(np.float64).sum()) - float(c.C.astype(np.float64).sum()))
    print("conservation %s %s %s: drift %.3g of the bar %.3g" % (GID(n), dt, mode, drift, N * eps * float(np.abs(c.C).max())))
    assert drift <= N * eps * float(np.abs(c.C).max())
    lo, hi = SC.stencil_hull(np.asarray(c.C))
    assert np.all(out >= lo) and np.all(out <= hi)
    B = SC.block01(n, T)
    out = run_three(hip, ctxs[mode], c, True, Cf=B)[2]
    lo, hi = SC.stencil_hull(B)
    tol = T(4 * float(np.spacing(T(1))))
    assert np.all(out >= lo - tol) and np.all(out <= hi + tol)


# ---- 6. footprint, 7. stream order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(17, 9, 5), (67, 19, 35)], ids=GID)
def test_footprint(hip, ctxs, n, dt, mode):
    c = case(n, dt)
    ctx = ctxs[mode]
    d1, b1, _, _ = (c.out[True], c.lift, None, None) if mode == "strict" else run_three(hip, ctx, c, True)
    ins = [("C", c.C, False), ("mu_e", c.mu_e, False)]
    GL._in_arena(hip, [("C_out", sentinel(n, dt), True)] + ins,
                 lambda t: hip.scalar_diffuse(t["C_out"], t["C"], t["mu_e"], c.kappa, c.sgs, c.mu, c.step, *c.d, ctx=ctx),
                 dict(C_out=d1), ("scalar_diffuse", n, dt, mode))
    GL._in_arena(hip, [("Vz", np.asarray(c.Vz), True), ("C", c.C, False)],
                 lambda t: hip.buoyancy(t["Vz"], t["C"], BG, C_REF, c.step, ctx=ctx), dict(Vz=b1), ("buoyancy", n, dt, mode))
    GL._in_arena(hip, [("C_out", sentinel(n, dt), True), ("Vz", np.asarray(c.Vz), True)] + ins,
                 lambda t: hip.scalar_step(t["C_out"], t["Vz"], t["C"], t["mu_e"], c.kappa, c.sgs, c.mu, BG, C_REF, c.step, *c.d, ctx=ctx),
                 dict(C_out=d1, Vz=b1), ("scalar_step", n, dt, mode))


@pytest.mark.parametrize("kind", ["torch", "own", "masked"])
@pytest.mark.parametrize("dt", DTS)
def test_stream_order(hip, delay, dt, kind):
    cases = []
    for n in [(24, 15, 15), (70, 6, 7)]:
        c = case(n, dt)
        ins = [("C", c.C, "field"), ("mu_e", c.mu_e, "field")]
        cases.append(SO.Case("scalar_diffuse %s %s" % (GID(n), dt), [("C_out", sentinel(n, dt), "field")] + ins,
                             lambda hip, ctx, t, c=c: hip.scalar_diffuse(t["C_out"], t["C"], t["mu_e"], c.kappa, c.sgs, c.mu, c.step, *c.d,
                                                                         ctx=ctx)))
        cases.append(SO.Case("buoyancy %s %s" % (GID(n), dt), [("Vz", np.asarray(c.Vz), "field"), ("C", c.C, "field")],
                             lambda hip, ctx, t, c=c: hip.buoyancy(t["Vz"], t["C"], BG, C_REF, c.step, ctx=ctx)))
        cases.append(SO.Case("scalar_step %s %s" % (GID(n), dt), [("C_out", sentinel(n, dt), "field"), ("Vz", np.asarray(c.Vz), "field")] + ins,
                             lambda hip, ctx, t, c=c: hip.scalar_step(t["C_out"], t["Vz"], t["C"], t["mu_e"], c.kappa, c.sgs, c.mu, BG, C_REF,
                                                                      c.step, *c.d, ctx=ctx)))
    GL.run_cases(hip, cases, kind, delay)


# ---- 8. the step under the knob -----------------------------------------------------------------------------------------------------------
STEP_SHAPES, GRID, ELEVEN, TAU = GL.STEP_SHAPES, GL.GRID, GL.ELEVEN, GL.TAU
VARIANTS = ("alone", "wale", "maccormack", "obstacle")


def knob_values(script):
    """kappa at a quarter of the explicit limit, the default Schmidt number, a modest lift and a small reference value: under the
    capped PT loop any forcing of the free fluid grows from step to step, and three steps must stay finite"""
    p, _ = GL.step_params(script, 42)
    return dict(kappa=0.125 / (p.dt * SC.sum_inv_d2(p.dx, p.dy, p.dz)), sct=0.7, bg=0.12, c_ref=1e-4)


@functools.lru_cache(maxsize=None)
def box_mask():
    import solid_ref
    from navierstokes3d_amd import solid as S
    m = solid_ref.voxelize(S.box_mesh((8.3, 4.6, 5.2), (13.7, 10.1, 9.9)), *GRID)
    m.setflags(write=False)
    return m


def steps_on(hip, ctx, script, nt, variant, sca, pressure=0, host=None):
    """GL.host_state(script) (or `host`) uploaded, the variant's knobs and the scalar knob set through the C entry points (sca None:
    left off), nt ns3d_time_step calls, everything downloaded; the knobs are cleared before anything is read"""
    from navierstokes3d_amd import lib as L
    import test_gpu_solid_step as GS
    lib = L.load()
    p, sp = GL.step_params(script, 42, pressure)
    f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in (GL.host_state(script) if host is None else host).items()})
    mu_e = hip.from_numpy(sentinel(GRID, "f64"))
    dmask = GS.upload_mask(box_mask()) if variant == "obstacle" else None
    torch.cuda.synchronize()
    out = []
    try:
        if variant == "wale":
            ctx.set_turbulence("wale", SR.length_of(SR.WALE, p.dx, p.dy, p.dz), mu_e)
        if variant == "maccormack":
            ctx.set_advection("maccormack")
        if variant == "obstacle":
            ctx.set_obstacle(dmask)
        if sca is not None:
            L.check(lib.ns3d_set_scalar(ctx.handle, 1, sca["kappa"], sca["sct"], sca["bg"], sca["c_ref"]))
            assert ctx.scalar()
        for step in range(1, nt + 1):
            sp.write_stress = 1 if step == nt else 0
            out.append(hip.time_step(f, sp, ctx=ctx))
        ctx.sync()
    finally:
        L.check(lib.ns3d_set_scalar(ctx.handle, 0, 0.0, 0.0, 0.0, 0.0))
        ctx.set_obstacle(None); ctx.set_advection("reference"); ctx.set_turbulence(None)
    assert not ctx.scalar()
    torch.cuda.synchronize()
    return SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}, mu_e=hip.to_numpy(mu_e), p=p)


@functools.lru_cache(maxsize=None)
def statement(script, nt, variant, on=True, pressure="pt", work=np.float64):
    """scalar_ref.step nt times from GL.host_state(script) — shared, never modified"""
    p, _ = GL.step_params(script, 42)
    f = GL.host_state(script)
    kw = dict(op=SR.WALE, length=SR.length_of(SR.WALE, p.dx, p.dy, p.dz)) if variant == "wale" else {}
    steps = []
    for _ in range(nt):
        mu_e, done, errs = SC.step(f, p, knob_values(script) if on else None, 42, script, faithful=False, pressure=pressure, work=work,
                                   maccormack=variant == "maccormack", mask=box_mask() if variant == "obstacle" else None, **kw)
        steps.append((done, errs))
    for a in f.values():
        a.setflags(write=False)
    return f, steps, mu_e


@pytest.mark.parametrize("mode", ["strict", "ieee"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_under_the_knob_equals_the_statement(hip, script, variant, mode):
    """three steps of 42 PT iterations (the cap DESIGN §4.15 explains) at 24×15×15: eleven arrays, the last step's stresses, iteration
    counts and err histories, bit for bit — alone, under WALE (the eddy diffusivity acts), with MacCormack advection, with a box"""
    ctx = hip.Context(0, "strict", async_=True, ieee_div=mode == "ieee")
    got = steps_on(hip, ctx, script, 3, variant, knob_values(script))
    ctx.close()
    want, steps, mu_e = statement(script, 3, variant)
    assert all(np.isfinite(a).all() for a in got.fields.values())
    assert GL.same_steps(got.steps, steps), (got.steps, steps)
    for k in ELEVEN + TAU:
        assert bits_equal(got.fields[k], want[k]), (script, variant, mode, k, first_bit_difference(got.fields[k], want[k]))
    if variant == "wale":
        assert bits_equal(got.mu_e, mu_e)
    off, _, _ = statement(script, 3, variant, on=False)
    # the scalar acts on the flow and on itself (the gpu script's run-away velocities under the box carry every C to the same clamp)
    assert not bits_equal(want["Vz"], off["Vz"]) and (not bits_equal(want["C"], off["C"]) or (script, variant) == ("gpu", "obstacle"))


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_with_the_direct_solve(hip, script):
    """pressure = 1 under the knob against the statement with oracle/direct_ref.py's solve, within test_gpu_direct.py's bar for whole
    runs, as test_gpu_les.py applies it: per field max(1e-9, 20 × the statement's own rounding level)"""
    from util import rel_l2
    ctx = hip.Context(0, "strict", async_=True)
    got = steps_on(hip, ctx, script, 2, "alone", knob_values(script), pressure=1)
    ctx.close()
    want, steps, _ = statement(script, 2, "alone", True, "direct")
    levels = None
    if np.finfo(np.longdouble).eps < 1e-18:
        wide, _, _ = statement(script, 2, "alone", True, "direct", np.longdouble)
        vn = max(np.sqrt(np.sum(want[n] ** 2)) for n in ("Vx", "Vy", "Vz"))
        levels = {n: rel_l2(wide[n], want[n], vn if n.startswith("V") else None) for n in ("C", "Pr", "Vx", "Vy", "Vz")}
    print("the statement's own rounding level (float64 against long-double sums):", levels)
    vnorm = max(np.sqrt(np.sum(want[n] ** 2)) for n in ("Vx", "Vy", "Vz"))
    for n in ("C", "Pr", "Vx", "Vy", "Vz"):
        bar = max(1e-9, 20.0 * levels[n]) if levels else 1e-9
        e = rel_l2(got.fields[n], want[n], vnorm if n.startswith("V") else None)
        print("%s: %.3e (bar %.2e)" % (n, e, bar))
        assert np.isfinite(got.fields[n]).all() and e < bar, (n, e, bar)
    assert [s[0] for s in got.steps] == [0, 0]


def test_the_knob_belongs_to_the_steps_it_is_set_for(hip):
    """cleared, a step is a fresh context's; ns3d_set_turbulence(NONE) leaves the scalar knob alone"""
    from navierstokes3d_amd import lib as L
    lib = L.load()
    A = hip.Context(0, "strict", async_=True)
    first = steps_on(hip, A, "multi", 1, "alone", knob_values("multi"))
    again = steps_on(hip, A, "multi", 1, "alone", None, host=first.fields)
    L.check(lib.ns3d_set_scalar(A.handle, 1, 1e-4, 0.7, 0.0, 0.0))
    A.set_turbulence(None)
    assert lib.ns3d_scalar(A.handle) == 1
    A.set_scalar(None)
    assert lib.ns3d_scalar(A.handle) == 0
    A.close()
    B = hip.Context(0, "strict", async_=True)
    assert lib.ns3d_scalar(B.handle) == 0
    fresh = steps_on(hip, B, "multi", 1, "alone", None, host=first.fields)
    B.close()
    assert GL.same_steps(again.steps, fresh.steps)
    for k in STEP_SHAPES:
        assert bits_equal(again.fields[k], fresh.fields[k]), k
    D = hip.Context(0, "strict", async_=True)
    plain = GL.steps_on(hip, D, "multi", 1, None)
    D.close()
    assert not bits_equal(first.fields["C"], plain.fields["C"])


def test_stream_order_of_the_step_under_the_knob(hip, delay):
    """two ns3d_time_step calls under the knob on a pinned torch stream with every array a late input and an early reader's output,
    against the null-stream bits"""
    host = dict(GL.host_state("multi"))
    sca = knob_values("multi")

    def call(hip, ctx, t):
        f = SimpleNamespace(**t)
        _, sp = GL.step_params("multi", 42)
        try:
            ctx.set_scalar(sca["kappa"], sca["sct"], sca["bg"], sca["c_ref"])
            out = []
            for step in (1, 2):
                sp.write_stress = 1 if step == 2 else 0
                out.append(hip.time_step(f, sp, ctx=ctx))
            return out
        finally:
            ctx.set_scalar(None)
    cs = SO.Case("time_step multi under the scalar knob", [(k, a, ("field", 1e-2)) for k, a in host.items()], call, blocking=True)
    (want_r, want), _ = SO.expected(hip, cs)
    ref, steps, _ = statement("multi", 2, "alone")
    assert GL.same_steps(want_r, steps) and bits_equal(want["C"], ref["C"])
    GL.run_cases(hip, [cs], "torch", delay)


# ---- 9. the drivers -----------------------------------------------------------------------------------------------------------------------
def _run(script, nt, **kw):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    if script == "multi":
        out = run_navierstokes3D(nt=nt, return_info=True, **kw)
        return out[-1].fields, out[-1]
    return runme(nt=nt, **kw)


def _keyword(script):
    v = knob_values(script)
    return dict(kappa=v["kappa"], sct=v["sct"], beta_g=v["bg"], c_ref=v["c_ref"])


@pytest.mark.parametrize("extra", [dict(), dict(turbulence="wale"), dict(advection="maccormack")], ids=["alone", "wale", "maccormack"])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_drivers_one_call_equals_call_by_call(hip, script, extra):
    """nx = 24, three steps: ns3d_time_step under the knob against the ns3d_scalar_step call the driver issues itself — all seventeen
    arrays, counts, errs; alone, the run is the statement's"""
    kw = dict(nx=24, mode="strict", niter_cap=42, faithful=False, scalar=_keyword(script), **extra)
    f1, i1 = _run(script, 3, **kw)
    f2, i2 = _run(script, 3, one_call=False, **kw)
    a, b = GL._driver_fields(hip, f1), GL._driver_fields(hip, f2)
    for k in STEP_SHAPES:
        assert bits_equal(a[k], b[k]), (script, extra, k, first_bit_difference(a[k], b[k]))
    assert i1.iters == i2.iters and GL.same_steps(list(zip(i1.iters, i1.errs)), list(zip(i2.iters, i2.errs)))
    assert not i1.ctx.scalar() and not i2.ctx.scalar()
    v = knob_values(script)
    assert i1.scalar == i2.scalar == dict(kappa=v["kappa"], sct=0.7, bg=v["bg"], c_ref=v["c_ref"])
    if not extra:
        want, steps, _ = statement(script, 3, "alone")
        for k in ("C", "Pr", "Vx", "Vy", "Vz"):
            assert bits_equal(a[k], want[k]), (script, k)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_scalar_none_is_no_keyword(hip, script, monkeypatch):
    """scalar=None: the bits and the call trace of a run without the keyword; with it, one scalar_step per step behind the predictor"""
    from navierstokes3d_amd import kernels as K
    trace = []
    real = K.Context.call

    def spy(self, name, ref, *args):
        trace.append(name)
        return real(self, name, ref, *args)
    monkeypatch.setattr(K.Context, "call", spy)
    runs = {}
    for key, extra in (("plain", dict()), ("none", dict(scalar=None)), ("on", dict(scalar=_keyword(script)))):
        del trace[:]
        f, info = _run(script, 2, nx=24, mode="strict", niter_cap=42, faithful=False, one_call=False, **extra)
        runs[key] = (GL._driver_fields(hip, f), list(trace), info)
    plain, none, on = runs["plain"], runs["none"], runs["on"]
    assert plain[1] == none[1] and "scalar_step" not in plain[1] and not hasattr(none[2], "scalar")
    for k in STEP_SHAPES:
        assert bits_equal(plain[0][k], none[0][k]), k
    assert on[1].count("scalar_step") == 2 and [n for n in on[1] if n != "scalar_step"] == plain[1]
    assert on[1][on[1].index("scalar_step") - 1] == "predict_fused"
    assert not bits_equal(on[0]["C"], plain[0]["C"])


def test_the_monitor_stops_a_step_beyond_the_scalar_s_diffusion_limit(hip):
    """diagnostics=True under a model: a Schmidt number small enough that dt·(kappa + (mu_e_max − μ)/(ρ·sct))·Σ1/d² > ½ raises"""
    from navierstokes3d_amd import lib as L
    kw = dict(nx=24, mode="strict", niter_cap=42, faithful=False, turbulence="smagorinsky", diagnostics=True)
    f, info = _run("gpu", 1, scalar=dict(kappa=1e-6, sct=0.7), **kw)         # the power-law profile: |S| > 0 from the first step on
    assert len(info.diag) == 1 and info.diag[-1].mu_e_max > info.params.mu
    with pytest.raises(L.Ns3dError, match="explicit diffusion limit of the scalar"):
        _run("gpu", 1, scalar=dict(kappa=1e-6, sct=1e-12), **kw)


# ---- 10. error paths ----------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n = (3, 3, 3)
    c = case(n, "f64")
    ctx = ctxs["strict"]
    h = ctx.handle
    Cd, Md, Vd, out = hip.from_numpy(c.C), hip.from_numpy(c.mu_e), hip.from_numpy(sentinel((3, 3, 4), "f64")), hip.from_numpy(sentinel(n, "f64"))
    P = lambda t: C.c_void_p(t.data_ptr())
    D = lambda *xs: [C.c_double(x) for x in xs]
    nan, inf = float("nan"), float("inf")
    ok = dict(kappa=c.kappa, sgs=c.sgs, mu=c.mu, bg=BG, c_ref=C_REF, dt=c.step, dx=c.d[0], dy=c.d[1], dz=c.d[2])

    def diffuse(ctxh=h, o=P(out), i=P(Cd), m=P(Md), grid=(3, 3, 3), **kw):
        v = dict(ok, **kw)
        return lib.ns3d_scalar_diffuse_f64(ctxh, o, i, m, *D(v["kappa"], v["sgs"], v["mu"], v["dt"], v["dx"], v["dy"], v["dz"]), *grid)

    def lift(ctxh=h, vz=P(Vd), i=P(Cd), grid=(3, 3, 3), **kw):
        v = dict(ok, **kw)
        return lib.ns3d_buoyancy_f64(ctxh, vz, i, *D(v["bg"], v["c_ref"], v["dt"]), *grid)

    def fused(ctxh=h, o=P(out), vz=P(Vd), i=P(Cd), m=P(Md), grid=(3, 3, 3), **kw):
        v = dict(ok, **kw)
        return lib.ns3d_scalar_step_f64(ctxh, o, vz, i, m, *D(v["kappa"], v["sgs"], v["mu"], v["bg"], v["c_ref"], v["dt"], v["dx"], v["dy"],
                                                              v["dz"]), *grid)
    bad_values = [dict(kappa=-1e-3), dict(kappa=nan), dict(sgs=-1.0), dict(sgs=inf), dict(dt=nan), dict(dx=0.0), dict(dy=-0.1), dict(dz=nan),
                  dict(dx=inf)]
    calls = {"ns3d_scalar_diffuse_f64": [lambda: diffuse(ctxh=None), lambda: diffuse(o=None), lambda: diffuse(i=None),
                                         lambda: diffuse(o=P(Cd))] + [lambda g=g: diffuse(grid=g) for g in ((2, 3, 3), (3, 2, 3), (3, 3, 2))] +
                                        [lambda kw=kw: diffuse(**kw) for kw in bad_values],
             "ns3d_buoyancy_f64": [lambda: lift(ctxh=None), lambda: lift(vz=None), lambda: lift(i=None), lambda: lift(grid=(3, 3, 2)),
                                   lambda: lift(bg=nan), lambda: lift(c_ref=inf), lambda: lift(dt=inf)],
             "ns3d_scalar_step_f64": [lambda: fused(ctxh=None), lambda: fused(o=None), lambda: fused(i=None), lambda: fused(vz=None),
                                      lambda: fused(o=P(Cd)), lambda: fused(grid=(2, 3, 3)), lambda: fused(bg=nan), lambda: fused(c_ref=nan)] +
                                     [lambda kw=kw: fused(**kw) for kw in bad_values]}
    for name, cs in calls.items():
        for q, call in enumerate(cs):
            assert call() == L.NS3D_ERR_ARG == 1, (name, q)
            assert L.last_error().startswith(name + ": "), (name, q, L.last_error())
    knob = lib.ns3d_set_scalar
    assert knob(h, 1, 1e-4, 0.7, 2.0, 0.1) == 0 and lib.ns3d_scalar(h) == 1
    for what, args in {"null context": (None, 1, 1e-4, 0.7, 0.0, 0.0), "kappa < 0": (h, 1, -1e-4, 0.7, 0.0, 0.0), "sct < 0": (h, 1, 1e-4, -0.7, 0.0, 0.0),
                       "kappa nan": (h, 1, nan, 0.7, 0.0, 0.0), "bg inf": (h, 1, 1e-4, 0.7, inf, 0.0), "c_ref nan": (h, 0, 1e-4, 0.7, 0.0, nan)}.items():
        assert knob(*args) == L.NS3D_ERR_ARG, what
        assert L.last_error().startswith("ns3d_set_scalar: "), (what, L.last_error())
        assert lib.ns3d_scalar(h) == 1                                      # a refused call leaves the setting
    assert knob(h, 0, 0.0, 0.0, 0.0, 0.0) == 0 and lib.ns3d_scalar(h) == 0
    ctx.sync()
    assert bits_equal(hip.to_numpy(Cd), c.C) and bits_equal(hip.to_numpy(Md), c.mu_e)
    assert np.all(hip.to_numpy(out) == 777.0) and np.all(hip.to_numpy(Vd) == 777.0)
    with pytest.raises(L.Ns3dError):
        hip.scalar_diffuse(hip.zeros((3, 3, 4)), Cd, None, c.kappa, 0.0, c.mu, c.step, *c.d, ctx=ctx)             # shape
    with pytest.raises(L.Ns3dError):
        hip.scalar_step(out, hip.zeros((3, 3, 3)), Cd, None, c.kappa, 0.0, c.mu, BG, C_REF, c.step, *c.d, ctx=ctx)  # Vz's shape
    with pytest.raises(L.Ns3dError):
        hip.buoyancy(hip.zeros((3, 3, 4), torch.float32), Cd, BG, C_REF, c.step, ctx=ctx)                          # dtype
    # the context is still usable
    assert_bits(run_three(hip, ctx, c, True)[2], c.out[True], "after the errors")
