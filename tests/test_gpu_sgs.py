"""GPU tests of ns3d_sgs_viscosity (include/ns3d.h) — the WALE and Vreman operators in k_eddy_visc's place —, of the step under
ns3d_set_sgs_operator and of the drivers' turbulence="wale" | "vreman".

The reference is the header's NumPy statements (tests/sgs_ref.py), computed once per case and shared, never modified.  STRICT must
return their bits, whichever of the three division builds the spacings select; FAST is held, element by element, to the running-error
bound of the same statements.  The kernel is k_eddy_visc with the operator as a template parameter, so the grids, the value makers and
the harness helpers are tests/test_gpu_les.py's."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import les_ref as LR
import running_error as RE
import sgs_ref as SR
import stream_order as SO
import test_gpu_les as GL
from util import bits_equal, first_bit_difference

pytestmark = pytest.mark.gpu

NPDT, DTS, GID, SPACINGS, EV_GRIDS = GL.NPDT, GL.DTS, GL.GID, GL.SPACINGS, GL.EV_GRIDS
NEW = [SR.WALE, SR.VREMAN]
OPS = [SR.SMAGORINSKY] + NEW
OPID = lambda op: SR.NAMES[op]
sentinel, assert_bits = GL.sentinel, GL.assert_bits


@functools.lru_cache(maxsize=None)
def case(n, dt, kind="geometry", values="seeded"):
    """test_gpu_les.case's velocities, spacings and scalars with, per operator, the drivers' length and the statement's mu_e"""
    b = GL.case(n, dt, kind, values)
    c = SimpleNamespace(n=n, dt=dt, V=b.V, d=b.d, mu=b.mu, rho=b.rho, smagorinsky=b.mu_e)
    c.length = {op: SR.length_of(op, *c.d) for op in OPS}
    c.mu_e = {op: SR.sgs_viscosity(op, *c.V, c.mu, c.rho, c.length[op], *c.d) for op in NEW}
    for a in c.mu_e.values():
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


def run_sgs(hip, ctx, op, V, d, mu, rho, length, dt):
    dev = [hip.from_numpy(a) for a in V]
    n = (V[0].shape[0] - 1,) + V[0].shape[1:]
    out = hip.from_numpy(sentinel(n, dt))
    hip.sgs_viscosity(out, *dev, op, mu, rho, length, *d, ctx=ctx)
    ctx.sync()
    for a, t in zip(V, dev):
        assert bits_equal(hip.to_numpy(t), a), "an input was modified"
    return hip.to_numpy(out)


def run_case(hip, ctx, op, c):
    return run_sgs(hip, ctx, op, c.V, c.d, c.mu, c.rho, c.length[op], c.dt)


# ---- 1. STRICT bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("n", EV_GRIDS, ids=GID)
def test_sgs_viscosity_returns_the_bits_of_the_statement(hip, ctxs, n, op, dt):
    builds = set()
    for kind in SPACINGS:
        c = case(n, dt, kind)
        ctx = ctxs["ieee"] if kind == "ieee" else ctxs["strict"]
        builds.add(ctx.arith_build(*c.d))
        assert_bits(run_case(hip, ctx, op, c), c.mu_e[op], (n, SR.NAMES[op], dt, kind))
    assert builds == {"strict", "strictx", "strictp"}, builds
    assert not bits_equal(c.mu_e[op], c.smagorinsky)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EV_GRIDS, ids=GID)
def test_operator_0_is_ns3d_eddy_viscosity(hip, ctxs, n, dt, mode):
    """on the device, bit for bit, in STRICT (where both are the statement) and in FAST; by name and by code"""
    c = case(n, dt)
    ctx = ctxs[mode]
    dev = [hip.from_numpy(a) for a in c.V]
    want = hip.from_numpy(sentinel(n, dt))
    hip.eddy_viscosity(want, *dev, c.mu, c.rho, c.length[0], *c.d, ctx=ctx)
    ctx.sync()
    for op in (0, "smagorinsky"):
        assert_bits(run_sgs(hip, ctx, op, c.V, c.d, c.mu, c.rho, c.length[0], dt), hip.to_numpy(want), (n, dt, mode, op))
    if mode == "strict":
        assert_bits(hip.to_numpy(want), c.smagorinsky, "statement")


# ---- 2. pure shear ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(4, 3, 5), (67, 7, 19), (130, 10, 34)], ids=GID)
def test_pure_shear_returns_mu_exactly(hip, ctxs, n, dt, mode):
    """u = γ·y: WALE and Vreman return muT in EVERY cell in every arithmetic mode — the zeros are exact products and sums of zeros, so
    contraction cannot change them — where operator 0 adds c·γ on the whole interior"""
    Vx, Vy, Vz, dx, dy, dz = LR.pure_shear(n, 1.375, NPDT[dt])
    mu, rho, length = 1e-3, 1000.0, 0.02
    full = np.full(n, NPDT[dt](mu), dtype=NPDT[dt], order="F")
    for op in NEW:
        assert_bits(run_sgs(hip, ctxs[mode], op, (Vx, Vy, Vz), (dx, dy, dz), mu, rho, length, dt), full, (SR.NAMES[op], n, dt, mode))
    s = run_sgs(hip, ctxs[mode], SR.SMAGORINSKY, (Vx, Vy, Vz), (dx, dy, dz), mu, rho, length, dt)
    assert np.all(s[LR.I] > 1.5 * NPDT[dt](mu)) and not bits_equal(s, full)


# ---- 3. FAST ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("n,values", [((70, 35, 8), "dense"), ((67, 19, 35), "blocks"), ((24, 15, 15), "rest0")], ids=str)
def test_fast_within_the_running_error_bound(hip, ctxs, n, values, op, dt):
    c = case(n, dt, "geometry", values)
    ctx = ctxs["fast"]
    assert ctx.arith_build(*c.d) == "fast"
    with np.errstate(all="ignore"):
        pm = SR.sgs_viscosity_pairs(op, *c.V, c.mu, c.rho, c.length[op], *c.d)
    got = run_case(hip, ctx, op, c)
    # a statement value that left the range (dense: |G|⁶ overflows) has no distance to be held to, and the header promises none
    finite = np.isfinite(c.mu_e[op]) & np.isfinite(pm.v)
    sel = lambda a: np.where(finite, a, 0.0)
    worst = RE.check(np.where(finite, got, got.dtype.type(0)), np.where(finite, c.mu_e[op], got.dtype.type(0)),
                     RE.Pair(sel(pm.v), sel(pm.e), pm.u), NPDT[dt], "FAST sgs_viscosity %s %s %r" % (SR.NAMES[op], dt, n))
    print("FAST %s %s %r %s: worst err/bound %.3g, %d of %d cells held to a finite bound" % (
        SR.NAMES[op], dt, n, values, worst, int((finite & np.isfinite(pm.e)).sum()), finite.size))
    # a property of the inputs, not of the kernel: the case is not vacuous (dense keeps 38 % of its cells in range, blocks 61 %)
    assert (finite & np.isfinite(pm.e)).mean() > 0.25
    if values == "rest0":               # a flow at rest: bound 0, hence the bits
        assert (pm.e == 0).all()
        assert_bits(got, c.mu_e[op], "rest")


# ---- 4. a single NaN, and the guards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
def test_a_single_nan_shows_up_where_the_statement_has_it(hip, ctxs, op, dt):
    n = (70, 35, 8)
    c = case(n, dt, "geometry", "nan")
    got = run_case(hip, ctxs["strict"], op, c)
    assert np.array_equal(np.isnan(got), np.isnan(c.mu_e[op])) and 0 < np.isnan(c.mu_e[op]).sum() <= 10
    assert_bits(got, c.mu_e[op], "nan mu_e")


@functools.lru_cache(maxsize=None)
def still_block(n, dt):
    """seeded velocities with a block of cells and their neighbours at rest: an all-zero gradient there (den == 0, aa == 0)"""
    V = [a.copy(order="F") for a in case(n, dt).V]
    lo, hi = (2, 2, 2), tuple(min(q - 2, 9) for q in n)
    for a in V:
        a[lo[0] - 1:hi[0] + 2, lo[1] - 1:hi[1] + 2, lo[2] - 1:hi[2] + 2] = 0
    still = np.zeros(n, dtype=bool)
    still[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return V, still


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", NEW, ids=OPID)
def test_the_zero_guards(hip, ctxs, op, dt, mode):
    n = (67, 19, 35)
    c = case(n, dt)
    V, still = still_block(n, dt)
    want, val = SR.sgs_viscosity(op, *V, c.mu, c.rho, c.length[op], *c.d, with_op=True)
    assert still.sum() >= 100 and np.all(want[still] == NPDT[dt](c.mu)) and np.isfinite(want).all()
    got = run_sgs(hip, ctxs[mode], op, V, c.d, c.mu, c.rho, c.length[op], dt)
    assert np.all(got[still] == NPDT[dt](c.mu)) and np.isfinite(got).all()
    if mode == "strict":
        assert_bits(got, want, ("guards", SR.NAMES[op], dt))


@pytest.mark.parametrize("dt", DTS)
def test_vreman_s_clamp_where_B_is_negative(hip, ctxs, dt):
    """sgs_ref.negative_B's search finds fields whose rounded B is negative (parallel gradient rows; tests/test_sgs_host.py): the
    device clamps where the statement does, and returns its bits"""
    (Vx, Vy, Vz, dx, dy, dz), neg = SR.negative_B((70, 9, 6), NPDT[dt])
    want = SR.sgs_viscosity(SR.VREMAN, Vx, Vy, Vz, 1e-3, 1000.0, 0.02, dx, dy, dz)
    got = run_sgs(hip, ctxs["strict"], SR.VREMAN, (Vx, Vy, Vz), (dx, dy, dz), 1e-3, 1000.0, 0.02, dt)
    assert neg.sum() > 0 and np.isfinite(got).all() and np.all(got[LR.I][neg] == NPDT[dt](1e-3))
    assert_bits(got, want, ("B < 0", dt))


# ---- 5. footprint, 6. stream order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(17, 9, 5), (67, 19, 35)], ids=GID)
def test_footprint(hip, ctxs, n, dt, mode):
    c = case(n, dt)
    ctx = ctxs[mode]
    ins = [("Vx", c.V[0], False), ("Vy", c.V[1], False), ("Vz", c.V[2], False)]
    for op in NEW:
        ref = c.mu_e[op] if mode != "fast" else run_case(hip, ctx, op, c)
        GL._in_arena(hip, [("mu_e", sentinel(n, dt), True)] + ins,
                     lambda t: hip.sgs_viscosity(t["mu_e"], t["Vx"], t["Vy"], t["Vz"], op, c.mu, c.rho, c.length[op], *c.d, ctx=ctx),
                     dict(mu_e=ref), ("sgs_viscosity", SR.NAMES[op], n, dt, mode))


@pytest.mark.parametrize("kind", ["torch", "own", "masked"])
@pytest.mark.parametrize("dt", DTS)
def test_stream_order(hip, delay, dt, kind):
    cases = []
    for n in [(24, 15, 15), (70, 6, 7)]:
        c = case(n, dt)
        V = [("V%s" % q, a, "field") for q, a in zip("xyz", c.V)]
        for op in NEW:
            cases.append(SO.Case("sgs_viscosity %s %s %s" % (SR.NAMES[op], GID(n), dt), [("mu_e", sentinel(n, dt), "field")] + V,
                                 lambda hip, ctx, t, c=c, op=op: hip.sgs_viscosity(t["mu_e"], t["Vx"], t["Vy"], t["Vz"], op, c.mu, c.rho,
                                                                                   c.length[op], *c.d, ctx=ctx)))
    GL.run_cases(hip, cases, kind, delay)


# ---- 7. the step under the knob -----------------------------------------------------------------------------------------------------------
STEP_SHAPES, GRID, ELEVEN, TAU = GL.STEP_SHAPES, GL.GRID, GL.ELEVEN, GL.TAU


def _length(op, script):
    p, _ = GL.step_params(script, 42)
    return SR.length_of(op, p.dx, p.dy, p.dz)


def steps_on(hip, ctx, script, nt, op, pressure=0, host=None, stress_on=None, model=True):
    """test_gpu_les.steps_on with the operator set through the C entry points; model False: ns3d_set_turbulence is left at NONE"""
    from navierstokes3d_amd import lib as L
    lib = L.load()
    p, sp = GL.step_params(script, 42, pressure)
    f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in (GL.host_state(script) if host is None else host).items()})
    mu_e = hip.from_numpy(sentinel(GRID, "f64"))
    torch.cuda.synchronize()
    out = []
    try:
        L.check(lib.ns3d_set_sgs_operator(ctx.handle, op))
        if model:
            L.check(lib.ns3d_set_turbulence(ctx.handle, L.NS3D_TURB_SMAGORINSKY, _length(op, script), C.c_void_p(mu_e.data_ptr())))
            assert ctx.turbulence() == SR.NAMES[op]
        for step in range(1, nt + 1):
            sp.write_stress = int(step in (stress_on if stress_on is not None else (nt,)))
            out.append(hip.time_step(f, sp, ctx=ctx))
        ctx.sync()
    finally:
        L.check(lib.ns3d_set_turbulence(ctx.handle, L.NS3D_TURB_NONE, 0.0, None))
    assert ctx.turbulence() is None and lib.ns3d_sgs_operator(ctx.handle) == op      # NONE does not touch the operator
    torch.cuda.synchronize()
    return SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}, mu_e=hip.to_numpy(mu_e), p=p)


@functools.lru_cache(maxsize=None)
def statement(op, script, nt, pressure="pt", work=np.float64):
    """sgs_ref.step nt times from test_gpu_les.host_state(script) — shared, never modified"""
    p, _ = GL.step_params(script, 42)
    f = GL.host_state(script)
    steps = []
    for _ in range(nt):
        mu_e, done, errs = SR.step(op, f, p, _length(op, script), 42, script, faithful=False, pressure=pressure, work=work)
        steps.append((done, errs))
    for a in f.values():
        a.setflags(write=False)
    return f, steps, mu_e


@pytest.mark.parametrize("mode", ["strict", "ieee"])
@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_under_the_knob_equals_the_statement(hip, script, op, mode):
    """three steps of 42 PT iterations (the cap DESIGN §4.15 explains) at 24×15×15: eleven arrays, the last step's stresses and mu_e,
    iteration counts and err histories, bit for bit"""
    ctx = hip.Context(0, "strict", async_=True, ieee_div=mode == "ieee")
    got = steps_on(hip, ctx, script, 3, op)
    ctx.close()
    want, steps, mu_e = statement(op, script, 3)
    assert all(np.isfinite(a).all() for a in got.fields.values())
    assert GL.same_steps(got.steps, steps), (got.steps, steps)
    for k in ELEVEN + TAU:
        assert bits_equal(got.fields[k], want[k]), (script, mode, k, first_bit_difference(got.fields[k], want[k]))
    assert bits_equal(got.mu_e, mu_e) and mu_e.max() > got.p.mu
    smag, _, _ = GL.statement(script, 3)
    assert not bits_equal(want["Vx"], smag["Vx"])                        # another model than Smagorinsky's


@pytest.mark.parametrize("op", NEW, ids=OPID)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_with_the_direct_solve(hip, script, op):
    """pressure = 1 under the knob against the statement with oracle/direct_ref.py's solve, within test_gpu_direct.py's bar for whole
    runs, as test_gpu_les.py applies it: per field max(1e-9, 20 × the statement's own rounding level), that level being the statement
    with long-double sums against itself in float64"""
    from util import rel_l2
    ctx = hip.Context(0, "strict", async_=True)
    got = steps_on(hip, ctx, script, 2, op, pressure=1)
    ctx.close()
    want, steps, mu_e = statement(op, script, 2, "direct")
    levels = None
    if np.finfo(np.longdouble).eps < 1e-18:
        wide, _, wide_mu = statement(op, script, 2, "direct", np.longdouble)
        vn = max(np.sqrt(np.sum(want[n] ** 2)) for n in ("Vx", "Vy", "Vz"))
        levels = {n: rel_l2(wide[n], want[n], vn if n.startswith("V") else None) for n in ("C", "Pr", "Vx", "Vy", "Vz")}
        levels["mu_e"] = rel_l2(wide_mu, mu_e, None)
    print("the statement's own rounding level (float64 against long-double sums):", levels)
    pairs = [(n, got.fields[n], want[n]) for n in ("C", "Pr", "Vx", "Vy", "Vz")] + [("mu_e", got.mu_e, mu_e)]
    vnorm = max(np.sqrt(np.sum(b ** 2)) for n, a, b in pairs if n.startswith("V"))
    for n, a, b in pairs:
        bar = max(1e-9, 20.0 * levels[n]) if levels else 1e-9
        e = rel_l2(a, b, vnorm if n.startswith("V") else None)
        print("%s: %.3e (bar %.2e)" % (n, e, bar))
        assert np.isfinite(a).all() and e < bar, (n, e, bar)
    assert [s[0] for s in got.steps] == [0, 0] and all(len(s[1]) == 1 and np.isfinite(s[1][0]) for s in got.steps)


def test_the_operator_survives_none_and_the_step_then_ignores_it(hip):
    """C level: after set_turbulence(NONE) the operator is still set (steps_on asserts it) and a step is a fresh context's plain step;
    back at operator 0 the step under Smagorinsky is test_gpu_les.py's statement, bit for bit"""
    from navierstokes3d_amd import lib as L
    A = hip.Context(0, "strict", async_=True)
    first = steps_on(hip, A, "multi", 1, SR.WALE)
    again = steps_on(hip, A, "multi", 1, SR.VREMAN, host=first.fields, model=False)
    assert L.load().ns3d_sgs_operator(A.handle) == SR.VREMAN
    today = steps_on(hip, A, "multi", 3, SR.SMAGORINSKY)
    A.close()
    B = hip.Context(0, "strict", async_=True)
    assert L.load().ns3d_sgs_operator(B.handle) == 0
    fresh = GL.steps_on(hip, B, "multi", 1, None, host=first.fields)
    B.close()
    assert GL.same_steps(again.steps, fresh.steps) and np.all(again.mu_e == 777.0)
    for k in STEP_SHAPES:
        assert bits_equal(again.fields[k], fresh.fields[k]), k
    want, steps, mu_e = GL.statement("multi", 3)
    assert GL.same_steps(today.steps, steps) and bits_equal(today.mu_e, mu_e)
    for k in ELEVEN + TAU:
        assert bits_equal(today.fields[k], want[k]), k


@pytest.mark.parametrize("op", NEW, ids=OPID)
def test_stream_order_of_the_step_under_the_knob(hip, delay, op):
    """two ns3d_time_step calls under the knob on a pinned torch stream with every array — mu_e among them — a late input and an early
    reader's output, against the null-stream bits"""
    host = dict(GL.host_state("multi"))
    host["mu_e"] = sentinel(GRID, "f64")
    length = _length(op, "multi")

    def call(hip, ctx, t):
        t = dict(t)
        mu_e = t.pop("mu_e")
        f = SimpleNamespace(**t)
        _, sp = GL.step_params("multi", 42)
        try:
            ctx.set_turbulence(SR.NAMES[op], length, mu_e)
            out = []
            for step in (1, 2):
                sp.write_stress = 1 if step == 2 else 0
                out.append(hip.time_step(f, sp, ctx=ctx))
            return out
        finally:
            ctx.set_turbulence(None)
    cs = SO.Case("time_step multi under %s" % SR.NAMES[op], [(k, a, ("field", 1e-2)) for k, a in host.items()], call, blocking=True)
    (want_r, want), _ = SO.expected(hip, cs)
    ref, steps, mu_e = statement(op, "multi", 2)
    assert GL.same_steps(want_r, steps) and bits_equal(want["mu_e"], mu_e)
    GL.run_cases(hip, [cs], "torch", delay)


# ---- 8. the drivers -----------------------------------------------------------------------------------------------------------------------
def _run(script, nt, **kw):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    if script == "multi":
        out = run_navierstokes3D(nt=nt, return_info=True, **kw)
        return out[-1].fields, out[-1]
    return runme(nt=nt, **kw)


@pytest.mark.parametrize("advection", ["reference", "maccormack"])
@pytest.mark.parametrize("model", ["wale", "vreman"])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_drivers_one_call_equals_call_by_call(hip, script, model, advection):
    """nx = 24, three steps: ns3d_time_step under the two knobs against the calls the driver issues itself — all seventeen arrays,
    counts, errs, mu_e; mu_e is the statement of the last step's input velocities; info.turbulence names the model"""
    op = {v: k for k, v in SR.NAMES.items()}[model]
    kw = dict(nx=24, mode="strict", niter_cap=42, faithful=False, advection=advection, turbulence=model)
    f1, i1 = _run(script, 3, **kw)
    f2, i2 = _run(script, 3, one_call=False, **kw)
    a, b = GL._driver_fields(hip, f1), GL._driver_fields(hip, f2)
    for k in STEP_SHAPES:
        assert bits_equal(a[k], b[k]), (script, model, advection, k, first_bit_difference(a[k], b[k]))
    assert i1.iters == i2.iters and GL.same_steps(list(zip(i1.iters, i1.errs)), list(zip(i2.iters, i2.errs)))
    assert i1.ctx.turbulence() is None and i2.ctx.turbulence() is None
    from navierstokes3d_amd import lib as L
    assert L.load().ns3d_sgs_operator(i1.ctx.handle) == 0                # Context.set_turbulence(None) returns the operator to 0
    p = i1.params
    length = SR.length_of(op, p.dx, p.dy, p.dz)
    before, _ = _run(script, 2, **kw)
    want = SR.sgs_viscosity(op, *[hip.to_numpy(getattr(before, k)) for k in ("Vx", "Vy", "Vz")], p.mu, p.rho, length, p.dx, p.dy, p.dz)
    for info in (i1, i2):
        assert info.turbulence["model"] == model and info.turbulence["length"] == length
        assert bits_equal(np.asfortranarray(info.turbulence["mu_e"]), want)
    assert want.max() > p.mu
    if script == "multi" and advection == "reference":                  # the monitor works unchanged
        fd, idg = _run(script, 3, diagnostics=True, **kw)
        c = GL._driver_fields(hip, fd)
        for k in STEP_SHAPES:
            assert bits_equal(c[k], a[k]), ("diagnostics", k)
        assert len(idg.diag) == 3 and idg.diag[-1].mu_e_max == float(np.max(want)) and all(r.mu_e_max >= p.mu for r in idg.diag)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_smagorinsky_and_no_keyword_are_what_they_were(hip, script, monkeypatch):
    """turbulence="smagorinsky" still issues ns3d_eddy_viscosity, once per step, and never the new entry point; it is the dict with the
    default cs, bit for bit; info gains the model's name.  Without the keyword no viscosity call is made at all."""
    from navierstokes3d_amd import kernels as K
    trace = []
    real = K.Context.call

    def spy(self, name, ref, *args):
        trace.append(name)
        return real(self, name, ref, *args)
    monkeypatch.setattr(K.Context, "call", spy)
    runs = {}
    for key, extra in (("plain", dict()), ("name", dict(turbulence="smagorinsky")), ("dict", dict(turbulence=dict(model="smagorinsky", cs=0.17)))):
        del trace[:]
        f, info = _run(script, 2, nx=24, mode="strict", niter_cap=42, faithful=False, one_call=False, **extra)
        runs[key] = (GL._driver_fields(hip, f), list(trace), info)
    plain, name, dct = runs["plain"], runs["name"], runs["dict"]
    assert not any(n in ("eddy_viscosity", "sgs_viscosity", "update_tau_var", "predict_var") for n in plain[1])
    assert not hasattr(plain[2], "turbulence")
    assert name[1] == dct[1] and name[1].count("eddy_viscosity") == 2 and "sgs_viscosity" not in name[1]
    assert name[1].count("predict_var") == 2 and name[1].index("eddy_viscosity") < name[1].index("predict_var")
    assert name[2].turbulence["model"] == "smagorinsky" and name[2].turbulence["length"] == LR.smagorinsky_length(0.17, *[
        getattr(name[2].params, k) for k in ("dx", "dy", "dz")])
    for k in STEP_SHAPES:
        assert bits_equal(name[0][k], dct[0][k]), k
    del trace[:]
    _run(script, 2, nx=24, mode="strict", niter_cap=42, faithful=False, one_call=False, turbulence="wale")
    assert trace.count("sgs_viscosity") == 2 and "eddy_viscosity" not in trace
    assert [n for n in trace if n != "sgs_viscosity"] == [n for n in name[1] if n != "eddy_viscosity"]


# ---- 9. error paths -----------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n = (3, 3, 3)
    c = case(n, "f64")
    ctx = ctxs["strict"]
    h = ctx.handle
    dev = [hip.from_numpy(a) for a in c.V]
    out = hip.from_numpy(sentinel(n, "f64"))
    P = lambda t: C.c_void_p(t.data_ptr())
    D = lambda *xs: [C.c_double(x) for x in xs]
    Vp, ok, mo, sc = [P(t) for t in dev], D(*c.d), P(out), D(c.mu, c.rho, c.length[1])
    sv = lib.ns3d_sgs_viscosity_f64
    nan, inf = float("nan"), float("inf")
    calls = {
        "null context": lambda: sv(None, 1, mo, *Vp, *sc, *ok, 3, 3, 3),
        "op -1": lambda: sv(h, -1, mo, *Vp, *sc, *ok, 3, 3, 3),
        "op 3": lambda: sv(h, 3, mo, *Vp, *sc, *ok, 3, 3, 3),
        "null mu_e": lambda: sv(h, 1, None, *Vp, *sc, *ok, 3, 3, 3),
        "null Vx": lambda: sv(h, 1, mo, None, Vp[1], Vp[2], *sc, *ok, 3, 3, 3),
        "null Vy": lambda: sv(h, 2, mo, Vp[0], None, Vp[2], *sc, *ok, 3, 3, 3),
        "null Vz": lambda: sv(h, 2, mo, Vp[0], Vp[1], None, *sc, *ok, 3, 3, 3),
        "grid 2x3x3": lambda: sv(h, 1, mo, *Vp, *sc, *ok, 2, 3, 3),
        "grid 3x2x3": lambda: sv(h, 1, mo, *Vp, *sc, *ok, 3, 2, 3),
        "grid 3x3x2": lambda: sv(h, 2, mo, *Vp, *sc, *ok, 3, 3, 2),
        "dx 0": lambda: sv(h, 1, mo, *Vp, *sc, *D(0.0, c.d[1], c.d[2]), 3, 3, 3),
        "dy negative": lambda: sv(h, 1, mo, *Vp, *sc, *D(c.d[0], -c.d[1], c.d[2]), 3, 3, 3),
        "dz nan": lambda: sv(h, 2, mo, *Vp, *sc, *D(c.d[0], c.d[1], nan), 3, 3, 3),
        "dx inf": lambda: sv(h, 2, mo, *Vp, *sc, *D(inf, c.d[1], c.d[2]), 3, 3, 3),
        "mu negative": lambda: sv(h, 1, mo, *Vp, *D(-1e-3, c.rho, 0.01), *ok, 3, 3, 3),
        "mu nan": lambda: sv(h, 1, mo, *Vp, *D(nan, c.rho, 0.01), *ok, 3, 3, 3),
        "rho negative": lambda: sv(h, 2, mo, *Vp, *D(c.mu, -1.0, 0.01), *ok, 3, 3, 3),
        "rho inf": lambda: sv(h, 2, mo, *Vp, *D(c.mu, inf, 0.01), *ok, 3, 3, 3),
        "length negative": lambda: sv(h, 1, mo, *Vp, *D(c.mu, c.rho, -0.1), *ok, 3, 3, 3),
        "length nan": lambda: sv(h, 2, mo, *Vp, *D(c.mu, c.rho, nan), *ok, 3, 3, 3),
        "mu_e is Vx": lambda: sv(h, 1, Vp[0], *Vp, *sc, *ok, 3, 3, 3),
        "mu_e is Vy": lambda: sv(h, 2, Vp[1], *Vp, *sc, *ok, 3, 3, 3),
        "mu_e is Vz": lambda: sv(h, 1, Vp[2], *Vp, *sc, *ok, 3, 3, 3),
    }
    for what, call in calls.items():
        assert call() == L.NS3D_ERR_ARG == 1, what
        assert L.last_error().startswith("ns3d_sgs_viscosity_f64: "), (what, L.last_error())
    knob = lib.ns3d_set_sgs_operator
    assert lib.ns3d_sgs_operator(h) == 0
    assert knob(h, 2) == 0 and lib.ns3d_sgs_operator(h) == 2
    for what, args in {"null context": (None, 1), "op -1": (h, -1), "op 3": (h, 3)}.items():
        assert knob(*args) == L.NS3D_ERR_ARG, what
        assert L.last_error().startswith("ns3d_set_sgs_operator: "), (what, L.last_error())
        assert lib.ns3d_sgs_operator(h) == 2                                # a refused call leaves the setting
    assert lib.ns3d_set_turbulence(h, 2, 0.1, mo) == L.NS3D_ERR_ARG         # the operator is no third model code
    assert knob(h, 0) == 0 and lib.ns3d_sgs_operator(h) == 0
    ctx.sync()
    for t, a in zip(dev, c.V):
        assert bits_equal(hip.to_numpy(t), a)
    assert np.all(hip.to_numpy(out) == 777.0)
    with pytest.raises(L.Ns3dError):
        hip.sgs_viscosity(hip.zeros((3, 3, 4)), *dev, "wale", c.mu, c.rho, 0.01, *c.d, ctx=ctx)                 # shape
    with pytest.raises(L.Ns3dError):
        hip.sgs_viscosity(hip.zeros(n, torch.float32), *dev, "wale", c.mu, c.rho, 0.01, *c.d, ctx=ctx)          # dtype
    for bad in ("dynamic", 3, 1.0, None):
        with pytest.raises(L.Ns3dError):
            hip.sgs_viscosity(out, *dev, bad, c.mu, c.rho, 0.01, *c.d, ctx=ctx)
    with pytest.raises(L.Ns3dError):
        ctx.set_turbulence("k-epsilon")
    with pytest.raises(L.Ns3dError):
        ctx.set_turbulence("wale", 0.1)                                                                           # no mu_e
    assert ctx.turbulence() is None and lib.ns3d_sgs_operator(h) == 0       # … which leaves both settings
    assert np.all(hip.to_numpy(out) == 777.0)
    # the context is still usable
    assert_bits(run_case(hip, ctx, SR.WALE, c), c.mu_e[SR.WALE], "after the errors")
