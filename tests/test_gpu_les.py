"""GPU tests of the Smagorinsky model (include/ns3d.h): ns3d_eddy_viscosity, ns3d_update_tau_var, ns3d_predict_var, the step under
ns3d_set_turbulence and the drivers' `turbulence` keyword.

The reference is the header's NumPy statements (tests/les_ref.py), computed once per case and shared, never modified.  STRICT must
return their bits — whichever of the three division builds the spacings select; FAST is held, element by element, to the running-error
bound of the same statements.  k_eddy_visc keeps k_vortex's tiling (64×4 cell columns, 16 planes per workgroup): its grids are
test_gpu_vortex.py's EDGE list and the two smallest.  k_predict_var has k_predict_fused's 64×16 tile and z-chunks."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as AR
import les_ref as LR
import running_error as RE
import stream_order as SO
from util import SHAPES, bits_equal, fields, first_bit_difference, geometry, hostile

pytestmark = pytest.mark.gpu

NPDT = {"f64": np.float64, "f32": np.float32}
DTS = ["f64", "f32"]
# extents ≡ 0, ±1 modulo the 64×16 tile, across the z-chunk window_kz picks, two tiles each way
PV_GRIDS = [(3, 3, 3), (4, 3, 5), (17, 9, 5), (24, 15, 15), (65, 17, 5), (66, 18, 34), (67, 19, 35), (130, 34, 8), (131, 33, 67)]
# test_gpu_vortex.EDGE: extents − 2 ≡ 0, ±1 modulo the tile (64 in x, 4 in y) and the chunk (16 planes), and the extents themselves
EDGE = [(66, 6, 18), (67, 7, 19), (65, 5, 17), (130, 10, 34), (131, 11, 35), (129, 9, 33), (64, 8, 16), (128, 4, 32), (63, 3, 15)]
EV_GRIDS = [(3, 3, 3), (4, 3, 5)] + EDGE
GID = lambda n: "%dx%dx%d" % tuple(n)
SPACINGS = ("geometry", "pow2", "ieee")
CS = 0.17
TAU = ("txx", "tyy", "tzz", "txy", "txz", "tyz")


def test_the_edge_list_is_the_vortex_tests():
    from test_gpu_vortex import EDGE as theirs
    assert EDGE == theirs


def spacings_of(n, kind):
    if kind == "pow2":
        return 2.0 ** -5, 2.0 ** -7, 2.0 ** -3
    g = geometry(*n)
    return g["dx"], g["dy"], g["dz"]


@functools.lru_cache(maxsize=None)
def case(n, dt, kind="geometry", values="seeded"):
    """velocities, spacings, scalars and the statements' results — shared, never modified"""
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=NPDT[dt])
    if values in ("dense", "blocks", "rest0"):
        V = [hostile(a, 5 + q, values) for q, a in enumerate(V)]
    elif values == "nan":
        V = [a.copy(order="F") for a in V]
        V[0][n[0] // 2, n[1] // 2, n[2] // 2] = np.nan
    d = spacings_of(n, kind)
    g = geometry(*n)
    c = SimpleNamespace(n=n, dt=dt, V=V, d=d, mu=g["mu"], rho=g["rho"], g=g["g"], step=g["dt"], length=LR.smagorinsky_length(CS, *d))
    c.mu_e = LR.eddy_viscosity(*V, c.mu, c.rho, c.length, *d)
    c.tau = LR.tau_var(*V, c.mu_e, *d)
    c.new = LR.predict_var(*V, c.mu_e, c.rho, c.g, c.step, *d)
    for a in V + [c.mu_e] + c.tau + c.new:
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


def sentinel(shape, dt):
    return np.full(shape, 777.0, dtype=NPDT[dt], order="F")


def run_eddy(hip, ctx, c, V=None, length=None):
    dev = [hip.from_numpy(a) for a in (c.V if V is None else V)]
    out = hip.from_numpy(sentinel(c.n, c.dt))
    hip.eddy_viscosity(out, *dev, c.mu, c.rho, c.length if length is None else length, *c.d, ctx=ctx)
    ctx.sync()
    for a, t in zip(c.V if V is None else V, dev):
        assert bits_equal(hip.to_numpy(t), a), "an input was modified"
    return hip.to_numpy(out)


def run_tau(hip, ctx, c, mu_e):
    dev = [hip.from_numpy(a) for a in c.V]
    out = [hip.from_numpy(sentinel(a.shape, c.dt)) for a in c.tau]
    hip.update_tau_var(*out, *dev, hip.from_numpy(mu_e), *c.d, ctx=ctx)
    ctx.sync()
    return [hip.to_numpy(t) for t in out]


def run_predict(hip, ctx, c, mu_e, V=None):
    host = c.V if V is None else V
    dev = [hip.from_numpy(a) for a in host]
    m = hip.from_numpy(mu_e)
    out = [hip.from_numpy(sentinel(a.shape, c.dt)) for a in host]
    hip.predict_var(*out, *dev, m, c.rho, c.g, c.step, *c.d, ctx=ctx)
    ctx.sync()
    for a, t in zip(list(host) + [mu_e], dev + [m]):
        assert bits_equal(hip.to_numpy(t), a), "an input was modified"
    return [hip.to_numpy(t) for t in out]


def assert_bits(got, ref, what):
    got, ref = (got, ref) if isinstance(got, (list, tuple)) else ([got], [ref])
    for q, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype
        assert bits_equal(a, b), (what, q, first_bit_difference(a, b))


# ---- 1. STRICT bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EV_GRIDS, ids=GID)
def test_eddy_viscosity_returns_the_bits_of_the_statement(hip, ctxs, n, dt):
    builds = set()
    for kind in SPACINGS:
        c = case(n, dt, kind)
        ctx = ctxs["ieee"] if kind == "ieee" else ctxs["strict"]
        builds.add(ctx.arith_build(*c.d))
        assert_bits(run_eddy(hip, ctx, c), c.mu_e, (n, dt, kind))
    assert builds == {"strict", "strictx", "strictp"}, builds
    assert n[0] < 4 or (c.mu_e[LR.I] > NPDT[dt](c.mu)).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", PV_GRIDS, ids=GID)
def test_update_tau_var_and_predict_var_return_the_bits_of_the_statement(hip, ctxs, n, dt):
    builds = set()
    for kind in SPACINGS:
        c = case(n, dt, kind)
        ctx = ctxs["ieee"] if kind == "ieee" else ctxs["strict"]
        builds.add(ctx.arith_build(*c.d))
        assert_bits(run_tau(hip, ctx, c, c.mu_e), c.tau, ("update_tau_var", n, dt, kind))
        assert_bits(run_predict(hip, ctx, c, c.mu_e), c.new, ("predict_var", n, dt, kind))
    assert builds == {"strict", "strictx", "strictp"}, builds


# ---- 2. the fused kernel is the two calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("values", ["dense", "blocks", "rest0"])
@pytest.mark.parametrize("n", [(24, 15, 15), (67, 19, 35)], ids=GID)
def test_predict_var_equals_update_tau_var_then_predict_V(hip, ctxs, n, values, dt, mode):
    """on the device, bit for bit, in every arithmetic mode; mu_e is the device's own, formed from the hostile velocities"""
    c = case(n, dt, "geometry", values)
    ctx = ctxs[mode]
    dev = [hip.from_numpy(a) for a in c.V]
    m = hip.from_numpy(sentinel(n, dt))
    with np.errstate(all="ignore"):
        hip.eddy_viscosity(m, *dev, c.mu, c.rho, c.length, *c.d, ctx=ctx)
    fused = [hip.from_numpy(sentinel(a.shape, dt)) for a in c.V]
    hip.predict_var(*fused, *dev, m, c.rho, c.g, c.step, *c.d, ctx=ctx)
    tau = [hip.from_numpy(sentinel(a.shape, dt)) for a in c.tau]
    hip.update_tau_var(*tau, *dev, m, *c.d, ctx=ctx)
    hip.predict_V(*dev, *tau, c.rho, c.g, c.step, *c.d, ctx=ctx)
    ctx.sync()
    assert_bits([hip.to_numpy(t) for t in fused], [hip.to_numpy(t) for t in dev], (n, values, dt, mode))
    if mode != "fast":
        assert_bits(hip.to_numpy(m), c.mu_e, ("mu_e", n, values, dt, mode))
        assert_bits([hip.to_numpy(t) for t in fused], c.new, ("statement", n, values, dt, mode))
    if values == "dense":
        assert not np.isfinite(c.new[0]).all()          # the case does reach Inf / NaN


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(17, 9, 5), (66, 18, 34), (131, 33, 67)], ids=GID)
def test_a_uniform_mu_e_gives_the_bits_of_predict_fused(hip, ctxs, n, dt):
    c = case(n, dt)
    ctx = ctxs["strict"]
    dev = [hip.from_numpy(a) for a in c.V]
    want = [hip.from_numpy(sentinel(a.shape, dt)) for a in c.V]
    hip.predict_fused(*want, *dev, c.mu, c.rho, c.g, c.step, *c.d, ctx=ctx)
    ctx.sync()
    got = run_predict(hip, ctx, c, np.full(n, NPDT[dt](c.mu), dtype=NPDT[dt], order="F"))
    assert_bits(got, [hip.to_numpy(t) for t in want], (n, dt))
    assert_bits(run_eddy(hip, ctx, c, length=0.0), np.full(n, NPDT[dt](c.mu), dtype=NPDT[dt], order="F"), ("length 0", n, dt))


# ---- 3. FAST ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,values", [((70, 35, 8), "seeded"), ((67, 19, 35), "seeded"), ((24, 15, 15), "rest0")], ids=str)
def test_fast_within_the_running_error_bound(hip, ctxs, n, values, dt):
    c = case(n, dt, "geometry", values)
    ctx = ctxs["fast"]
    assert ctx.arith_build(*c.d) == "fast"
    pm = LR.eddy_viscosity_pairs(*c.V, c.mu, c.rho, c.length, *c.d)
    worst = RE.check(run_eddy(hip, ctx, c), c.mu_e, pm, NPDT[dt], "FAST eddy_viscosity %s %r" % (dt, n))
    pn = LR.predict_var_pairs(*c.V, c.mu_e, c.rho, c.g, c.step, *c.d)
    got = run_predict(hip, ctx, c, c.mu_e)
    for q, nm in enumerate("xyz"):
        worst = max(worst, RE.check(got[q], c.new[q], pn[q], NPDT[dt], "FAST predict_var V%s %s %r" % (nm, dt, n)))
    print("FAST les %s %r %s: worst err/bound %.3g" % (dt, n, values, worst))
    if values == "rest0":               # a flow at rest: bound 0, hence the bits
        assert (pm.e == 0).all() and (pn[0].e == 0).all() and (pn[1].e == 0).all()
        assert_bits(got[:2], c.new[:2], "rest")


# ---- 4. a single NaN ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_a_single_nan_shows_up_where_the_statement_has_it(hip, ctxs, dt):
    n = (70, 35, 8)
    c = case(n, dt, "geometry", "nan")
    got = run_eddy(hip, ctxs["strict"], c)
    assert np.array_equal(np.isnan(got), np.isnan(c.mu_e)) and 0 < np.isnan(c.mu_e).sum() <= 10
    assert_bits(got, c.mu_e, "nan mu_e")
    new = run_predict(hip, ctxs["strict"], c, got)
    for a, b in zip(new, c.new):
        assert np.array_equal(np.isnan(a), np.isnan(b))
    assert all(np.isnan(b).sum() > 0 for b in c.new) and sum(int(np.isnan(b).sum()) for b in c.new) < 400
    assert_bits(new, c.new, "nan prediction")


# ---- 5. footprint ---------------------------------------------------------------------------------------------------------------------------
def _in_arena(hip, arrays, call, ref, what):
    """the call on plain tensors and in a guarded arena (odd element offsets): guards intact, inputs untouched, the same bits, the
    statement's bits"""
    plain = {k: hip.from_numpy(a) for k, a, _ in arrays}
    ar = AR.Arena(arrays, "cuda")
    torch.cuda.synchronize()
    call(plain)
    call(ar.t)
    torch.cuda.synchronize()
    ar.assert_clean(str(what))
    for k, a, is_out in arrays:
        got = ar.get(k)
        if is_out:
            assert bits_equal(got, hip.to_numpy(plain[k])), (what, k, "differs from the call on plain arrays")
            assert bits_equal(got, ref[k]), (what, k, first_bit_difference(got, ref[k]))
        else:
            assert bits_equal(got, np.asarray(a)), (what, k, "an input was modified")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(17, 9, 5), (67, 19, 35)], ids=GID)
def test_footprint(hip, ctxs, n, dt, mode):
    c = case(n, dt)
    ctx = ctxs[mode]
    ins = [("Vx", c.V[0], False), ("Vy", c.V[1], False), ("Vz", c.V[2], False)]
    strict = mode == "strict"
    mu_ref = c.mu_e if strict else run_eddy(hip, ctx, c)
    _in_arena(hip, [("mu_e", sentinel(n, dt), True)] + ins,
              lambda t: hip.eddy_viscosity(t["mu_e"], t["Vx"], t["Vy"], t["Vz"], c.mu, c.rho, c.length, *c.d, ctx=ctx),
              dict(mu_e=mu_ref), ("eddy_viscosity", n, dt, mode))
    ins.append(("mu_e", c.mu_e, False))
    tau_ref = c.tau if strict else run_tau(hip, ctx, c, c.mu_e)
    _in_arena(hip, [(k, sentinel(a.shape, dt), True) for k, a in zip(TAU, c.tau)] + ins,
              lambda t: hip.update_tau_var(*[t[k] for k in TAU], t["Vx"], t["Vy"], t["Vz"], t["mu_e"], *c.d, ctx=ctx),
              dict(zip(TAU, tau_ref)), ("update_tau_var", n, dt, mode))
    new_ref = c.new if strict else run_predict(hip, ctx, c, c.mu_e)
    names = ("Vx_new", "Vy_new", "Vz_new")
    _in_arena(hip, [(k, sentinel(a.shape, dt), True) for k, a in zip(names, c.V)] + ins,
              lambda t: hip.predict_var(*[t[k] for k in names], t["Vx"], t["Vy"], t["Vz"], t["mu_e"], c.rho, c.g, c.step, *c.d, ctx=ctx),
              dict(zip(names, new_ref)), ("predict_var", n, dt, mode))


# ---- 6. stream order ------------------------------------------------------------------------------------------------------------------------
def run_cases(hip, cases, kind, delay, mode="strict"):
    """tests/test_gpu_stream_order.py's run_cases: expected bits on the null stream, a warm-up, then the late input and the early reader
    (and the variant that only synchronises) on an asynchronous context of `kind`"""
    msgs = []
    for cs in cases:
        (want_r, want), (dec_r, dec) = SO.expected(hip, cs, mode)
        ctx, S = SO.context_on(hip, kind, mode)
        SO.warm_up(hip, cs, ctx)
        for v in ("reader", "sync"):
            r, got, can = SO.measured(hip, cs, ctx, S, delay, v)
            msgs += SO.verdict("%s on %s, %s, %s" % (cs.name, kind, mode, v), got, want, dec, can, cs.decoy, r, want_r, dec_r)
        ctx.set_turbulence(None)
        ctx.close()
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
def test_stream_order_of_the_three_calls(hip, delay, dt, mode):
    cases = []
    for n in [(24, 15, 15), (70, 6, 7)]:
        c = case(n, dt)
        V = [("V%s" % q, a, "field") for q, a in zip("xyz", c.V)]
        cases.append(SO.Case("eddy_viscosity %s %s" % (GID(n), dt), [("mu_e", sentinel(n, dt), "field")] + V,
                             lambda hip, ctx, t, c=c: hip.eddy_viscosity(t["mu_e"], t["Vx"], t["Vy"], t["Vz"], c.mu, c.rho, c.length, *c.d,
                                                                         ctx=ctx)))
        V = V + [("mu_e", c.mu_e, "field")]
        cases.append(SO.Case("update_tau_var %s %s" % (GID(n), dt), [(k, sentinel(a.shape, dt), "field") for k, a in zip(TAU, c.tau)] + V,
                             lambda hip, ctx, t, c=c: hip.update_tau_var(*[t[k] for k in TAU], t["Vx"], t["Vy"], t["Vz"], t["mu_e"], *c.d,
                                                                         ctx=ctx)))
        cases.append(SO.Case("predict_var %s %s" % (GID(n), dt), [("V%s_new" % q, sentinel(a.shape, dt), "field") for q, a in zip("xyz", c.V)] + V,
                             lambda hip, ctx, t, c=c: hip.predict_var(t["Vx_new"], t["Vy_new"], t["Vz_new"], t["Vx"], t["Vy"], t["Vz"], t["mu_e"],
                                                                      c.rho, c.g, c.step, *c.d, ctx=ctx)))
    run_cases(hip, cases, "torch", delay, mode)


# ---- 7. the step ----------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = {"Pr": "c", "dPrdtau": "i", "divV": "c", "Vx": "vx", "Vy": "vy", "Vz": "vz", "Vx_o": "vx", "Vy_o": "vy", "Vz_o": "vz", "C": "c",
               "C_o": "c", "txx": "c", "tyy": "c", "tzz": "c", "txy": "s", "txz": "s", "tyz": "s"}
GRID = (24, 15, 15)
ELEVEN = ("C", "Pr", "Vx", "Vy", "Vz", "Vx_o", "Vy_o", "Vz_o", "C_o", "dPrdtau", "divV")


def host_state(script="multi"):
    """the seventeen arrays of ns3d_step_fields on the host, float64, in the script's own initial state at 24×15×15 — multi.jl:369-372
    (the inlet plane of Vy, the cylinder's masking before the loop) / gpu.jl:85-88 (the power-law profile, the hydrostatic pressure)"""
    from navierstokes3d_amd import driver as Dr
    p, _ = step_params(script, 42)
    host = {k: np.zeros(SHAPES[kind](*GRID), order="F") for k, kind in STEP_SHAPES.items()}
    if script == "multi":
        host["Vy"][0, :, :] = p.vin
        LR.cylinder(host, p, script)
    else:
        Vx0, Pr0 = Dr.gpu_initial_fields(p)
        host["Vx"], host["Pr"] = np.asfortranarray(Vx0), np.asfortranarray(Pr0)
    return host


def step_params(script, niter, pressure=0):
    """(the package's parameters, lib.StepParams) of the script at 24×15×15 with faithful = 0"""
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.params import gpu_params, multi_params
    p = multi_params(24) if script == "multi" else gpu_params(24)
    assert (p.nx, p.ny, p.nz) == GRID
    common = dict(nx=p.nx, ny=p.ny, nz=p.nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp, dx=p.dx, dy=p.dy, dz=p.dz,
                  eps=p.eps, niter=niter, nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc, a2=p.a2, b2=p.b2, ox=p.ox, oy=p.oy,
                  sinb=p.sinb, cosb=p.cosb, lx=p.lx, ly=p.ly, lz=p.lz, faithful=0, pressure=pressure, write_stress=0)
    if script == "multi":
        sp = L.StepParams(script=L.NS3D_BC_MULTI, xco_g=p.xco_g, yco_g=p.yco_g, zco_g=p.zco_g, owns_inlet=int(bool(p.owns_inlet)),
                          owns_outlet=int(bool(p.owns_outlet)), vin=p.vin, **common)
    else:
        sp = L.StepParams(script=L.NS3D_BC_GPU, xco_g=0.0, yco_g=0.0, zco_g=0.0, owns_inlet=0, owns_outlet=0, vin=0.0, **common)
    return p, sp


def steps_on(hip, ctx, script, nt, length, pressure=0, host=None, niter=42, stress_on=None):
    """host_state(script) (or `host`) uploaded, the knob set (length None: left off), nt ns3d_time_step calls (write_stress on the steps of
    `stress_on`, default the last), everything downloaded; the knob is cleared before anything is read"""
    p, sp = step_params(script, niter, pressure)
    f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in (host_state(script) if host is None else host).items()})
    mu_e = hip.from_numpy(sentinel(GRID, "f64"))
    torch.cuda.synchronize()
    out = []
    try:
        if length is not None:
            ctx.set_turbulence("smagorinsky", length, mu_e)
            assert ctx.turbulence() == "smagorinsky"
        for step in range(1, nt + 1):
            sp.write_stress = int(step in (stress_on if stress_on is not None else (nt,)))
            out.append(hip.time_step(f, sp, ctx=ctx))
        ctx.sync()
    finally:
        ctx.set_turbulence(None)
    assert ctx.turbulence() is None
    torch.cuda.synchronize()
    return SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}, mu_e=hip.to_numpy(mu_e), p=p)


@functools.lru_cache(maxsize=None)
def statement(script, nt, pressure="pt"):
    """les_ref.step nt times from host_state(script): (fields, [(iterations, errs)], mu_e of the last step) — shared, never modified"""
    p, _ = step_params(script, 42)
    f = host_state(script)
    length = LR.smagorinsky_length(CS, p.dx, p.dy, p.dz)
    steps = []
    for _ in range(nt):
        mu_e, done, errs = LR.step(f, p, length, 42, script, faithful=False, pressure=pressure)
        steps.append((done, errs))
    for a in f.values():
        a.setflags(write=False)
    return f, steps, mu_e


def same_steps(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and len(a[1]) == len(b[1]) and
                                         np.array_equal(np.float64(a[1]), np.float64(b[1]), equal_nan=True) for a, b in zip(got, want))


def _length(script):
    p, _ = step_params(script, 42)
    return LR.smagorinsky_length(CS, p.dx, p.dy, p.dz)


@pytest.mark.parametrize("mode", ["strict", "ieee"])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_under_the_knob_equals_the_statement(hip, script, mode):
    """three steps of 42 PT iterations at 24×15×15 from the seeded state: eleven arrays, the last step's stresses and mu_e, iteration
    counts and err histories, bit for bit"""
    ctx = hip.Context(0, "strict", async_=True, ieee_div=mode == "ieee")
    got = steps_on(hip, ctx, script, 3, _length(script))
    ctx.close()
    want, steps, mu_e = statement(script, 3)
    assert all(np.isfinite(a).all() for a in got.fields.values())
    assert same_steps(got.steps, steps), (got.steps, steps)
    for k in ELEVEN + TAU:
        assert bits_equal(got.fields[k], want[k]), (script, mode, k, first_bit_difference(got.fields[k], want[k]))
    assert bits_equal(got.mu_e, mu_e) and mu_e.max() > 2 * got.p.mu
    plain = hip.Context(0, "strict", async_=True)
    other = steps_on(hip, plain, script, 3, None)
    plain.close()
    assert not bits_equal(other.fields["Vx"], got.fields["Vx"])         # the model acts


@functools.lru_cache(maxsize=None)
def direct_levels(script, nt):
    """The statement's own rounding level under the direct solve, per field and for mu_e: the run with direct_ref's sums carried in
    long double against the run in float64, relative L2 as test_gpu_direct.py measures the oracle drivers' (velocities against the
    largest component's norm).  None where np.longdouble is not an 80-bit float."""
    if not np.finfo(np.longdouble).eps < 1e-18:
        return None
    from util import rel_l2
    p, _ = step_params(script, 42)
    runs = []
    for work in (np.float64, np.longdouble):
        f = host_state(script)
        for _ in range(nt):
            mu_e, _, _ = LR.step(f, p, _length(script), 42, script, faithful=False, pressure="direct", work=work)
        f["mu_e"] = mu_e
        runs.append(f)
    vnorm = max(np.sqrt(np.sum(runs[0][n] ** 2)) for n in ("Vx", "Vy", "Vz"))
    return {n: rel_l2(runs[1][n], runs[0][n], vnorm if n.startswith("V") else None) for n in ("C", "Pr", "Vx", "Vy", "Vz", "mu_e")}


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_the_step_with_the_direct_solve(hip, script):
    """pressure = 1 under the knob against the statement with oracle/direct_ref.py's solve, within test_gpu_direct.py's bar for whole
    runs: per field max(1e-9, 20 × the statement's own rounding level) (the direct solves differ in summation order, every other kernel
    is bit-exact).  multi.jl at this grid owns no outlet (xve_g = 0.49999999999999994), so its pressure problem is pure Neumann and
    the statement moves by 5.9e-7 (Pr), 2.7e-9 (C), 3.2e-9 (Vx) when its own sums are carried in long double; gpu.jl's stays at 1e-15."""
    import warnings
    from util import rel_l2
    ctx = hip.Context(0, "strict", async_=True)
    got = steps_on(hip, ctx, script, 2, _length(script), pressure=1)
    ctx.close()
    want, steps, mu_e = statement(script, 2, "direct")
    levels = direct_levels(script, 2)
    if levels is None:
        warnings.warn("np.longdouble is not an 80-bit float on this host: the statement's own level is not derived; the bar stays 1e-9")
    print("the statement's own rounding level (float64 against long-double sums):", levels)
    pairs = [(n, got.fields[n], want[n]) for n in ("C", "Pr", "Vx", "Vy", "Vz")] + [("mu_e", got.mu_e, mu_e)]
    vnorm = max(np.sqrt(np.sum(b ** 2)) for n, a, b in pairs if n.startswith("V"))
    for n, a, b in pairs:
        bar = max(1e-9, 20.0 * levels[n]) if levels else 1e-9
        e = rel_l2(a, b, vnorm if n.startswith("V") else None)
        print("%s: %.3e (bar %.2e)" % (n, e, bar))
        assert np.isfinite(a).all() and e < bar, (n, e, bar)
    # the reference's err measure (multi.jl:466) of the direct solution: test_gpu_direct.py's 1e-8 where the problem is regular; a pure
    # Neumann problem has no unique solution to be that close to, so there the measure is only required to exist
    print("direct-solve err per step: device %r, statement %r" % ([s[1] for s in got.steps], [s[1] for s in steps]))
    assert [s[0] for s in got.steps] == [0, 0] and all(len(s[1]) == 1 and np.isfinite(s[1][0]) for s in got.steps)
    if script == "gpu" or got.p.owns_outlet:
        assert all(s[1][0] < 1e-8 for s in got.steps), got.steps
    else:       # … and to be the statement's, as closely as the pressure is
        bar = max(1e-9, 20.0 * levels["Pr"]) if levels else 1e-9
        assert all(abs(a[1][0] - b[1][0]) <= bar * max(b[1][0], 1e-8) for a, b in zip(got.steps, steps)), (got.steps, steps)


def test_the_knob_belongs_to_the_steps_it_is_set_for(hip):
    """after set_turbulence(NONE) the same context returns a fresh context's plain step; length = 0 under the knob returns the plain
    step's bits, and mu_e = mu everywhere"""
    A = hip.Context(0, "strict", async_=True)
    first = steps_on(hip, A, "multi", 1, _length("multi"))
    again = steps_on(hip, A, "multi", 1, None, host=first.fields)
    A.close()
    B = hip.Context(0, "strict", async_=True)
    fresh = steps_on(hip, B, "multi", 1, None, host=first.fields)
    zero = steps_on(hip, B, "multi", 2, 0.0, stress_on=(1, 2))
    plain = steps_on(hip, B, "multi", 2, None, stress_on=(1, 2))
    B.close()
    assert same_steps(again.steps, fresh.steps)
    for k in STEP_SHAPES:
        assert bits_equal(again.fields[k], fresh.fields[k]), k
        assert bits_equal(zero.fields[k], plain.fields[k]), ("length 0", k)
    assert np.all(again.mu_e == 777.0) and np.all(zero.mu_e == zero.p.mu)


def test_stream_order_of_the_step_under_the_knob(hip, delay):
    """two ns3d_time_step calls under the knob on a pinned torch stream with every array — mu_e among them — a late input and an early
    reader's output, against the null-stream bits (arrays compared by buffer: the step swaps roles the same way in every run)"""
    from navierstokes3d_amd import lib as L
    p, sp0 = step_params("multi", 42)
    length = _length("multi")
    host = host_state("multi")
    host["mu_e"] = sentinel(GRID, "f64")

    def call(hip, ctx, t):
        t = dict(t)
        mu_e = t.pop("mu_e")
        f = SimpleNamespace(**t)
        _, sp = step_params("multi", 42)
        try:
            ctx.set_turbulence("smagorinsky", length, mu_e)
            out = []
            for step in (1, 2):
                sp.write_stress = 1 if step == 2 else 0
                out.append(hip.time_step(f, sp, ctx=ctx))
            return out
        finally:
            ctx.set_turbulence(None)
    cs = SO.Case("time_step multi under set_turbulence", [(k, a, ("field", 1e-2)) for k, a in host.items()], call, blocking=True)
    (want_r, want), _ = SO.expected(hip, cs)
    ref, steps, mu_e = statement("multi", 2)
    assert same_steps(want_r, steps) and bits_equal(want["mu_e"], mu_e)
    run_cases(hip, [cs], "torch", delay)


# ---- 8. the drivers -------------------------------------------------------------------------------------------------------------------------
def _driver_fields(hip, f):
    return {k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}


@pytest.mark.parametrize("advection", ["reference", "maccormack"])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_drivers_one_call_equals_call_by_call(hip, script, advection):
    """nx = 24, three steps, turbulence="smagorinsky": ns3d_time_step under the knob (write_stress on the last step only) against the
    three calls the driver issues itself — all seventeen arrays, counts, errs, mu_e; mu_e is the statement of the last step's input
    velocities; the monitor records mu_e_max; and the model acts"""
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    kw = dict(nx=24, mode="strict", niter_cap=42, faithful=False, advection=advection, turbulence="smagorinsky")

    def run(nt, **extra):
        if script == "multi":
            out = run_navierstokes3D(nt=nt, return_info=True, **kw, **extra)
            return out[-1].fields, out[-1]
        return runme(nt=nt, **kw, **extra)
    from navierstokes3d_amd import lib as L
    f1, i1 = run(3)
    f2, i2 = run(3, one_call=False)
    a, b = _driver_fields(hip, f1), _driver_fields(hip, f2)
    for k in STEP_SHAPES:
        assert bits_equal(a[k], b[k]), (script, advection, k, first_bit_difference(a[k], b[k]))
    assert i1.iters == i2.iters and same_steps(list(zip(i1.iters, i1.errs)), list(zip(i2.iters, i2.errs)))
    assert i1.ctx.turbulence() is None and i2.ctx.turbulence() is None
    p = i1.params
    length = LR.smagorinsky_length(CS, p.dx, p.dy, p.dz)
    assert i1.turbulence["length"] == length == i2.turbulence["length"]
    before, _ = run(2)
    want = LR.eddy_viscosity(*[hip.to_numpy(getattr(before, k)) for k in ("Vx", "Vy", "Vz")], p.mu, p.rho, length, p.dx, p.dy, p.dz)
    for info in (i1, i2):
        assert bits_equal(np.asfortranarray(info.turbulence["mu_e"]), want)
    assert want.max() > p.mu and not hasattr(i1, "diag")
    # the monitor: gpu.jl's flow at this grid leaves the reference's stable range within a step (|V| reaches 3e2, as without the model),
    # so its second step is where the guard speaks; multi.jl's three steps are monitored to the end
    nd = 3 if script == "multi" else 1
    if script == "gpu":
        with pytest.raises(L.Ns3dError, match="diffusion limit"):
            run(3, diagnostics=True)
    fd, idg = run(nd, diagnostics=True)
    fe, ie = (f1, i1) if nd == 3 else run(nd)
    c, e = _driver_fields(hip, fd), _driver_fields(hip, fe)
    for k in STEP_SHAPES:
        assert bits_equal(c[k], e[k]), (script, advection, "diagnostics", k)
    assert idg.iters == ie.iters and bits_equal(np.asfortranarray(idg.turbulence["mu_e"]), np.asfortranarray(ie.turbulence["mu_e"]))
    assert len(idg.diag) == nd and idg.diag[-1].mu_e_max == float(np.max(ie.turbulence["mu_e"])) and all(r.mu_e_max >= p.mu for r in idg.diag)
    # the last step's stresses are update_tau_var's of the same velocities
    tau = LR.tau_var(*[hip.to_numpy(getattr(before, k)) for k in ("Vx", "Vy", "Vz")], want, p.dx, p.dy, p.dz)
    for k, t in zip(TAU, tau):
        assert bits_equal(a[k], t), k


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_drivers_without_the_keyword_are_what_they_were(hip, script, monkeypatch):
    """turbulence=None against a run without the keyword: the same bits and the same trace of library calls"""
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    trace = []
    real = K.Context.call

    def spy(self, name, ref, *args):
        trace.append(name)
        return real(self, name, ref, *args)
    monkeypatch.setattr(K.Context, "call", spy)
    runs = []
    for extra in (dict(), dict(turbulence=None), dict(one_call=False), dict(one_call=False, turbulence=None)):
        del trace[:]
        kw = dict(nx=24, nt=2, mode="strict", niter_cap=42, **extra)
        if script == "multi":
            out = run_navierstokes3D(return_info=True, **kw)
            f, info = out[-1].fields, out[-1]
        else:
            f, info = runme(**kw)
        assert not hasattr(info, "turbulence")
        runs.append((_driver_fields(hip, f), list(trace), info))
    for q in (0, 2):
        (a, ta, ia), (b, tb, ib) = runs[q], runs[q + 1]
        assert ta == tb and not any(n in ("eddy_viscosity", "update_tau_var", "predict_var") for n in ta)
        assert ia.iters == ib.iters
        for k in STEP_SHAPES:
            assert bits_equal(a[k], b[k]), k


def test_the_monitor_stops_a_step_beyond_the_diffusion_limit(hip):
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import runme
    with pytest.raises(L.Ns3dError, match="diffusion limit"):
        runme(nx=24, nt=2, niter_cap=14, faithful=False, diagnostics=True, turbulence=dict(model="smagorinsky", cs=400.0))


# ---- 9. error paths -------------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n = (3, 3, 3)
    c = case(n, "f64")
    ctx = ctxs["strict"]
    h = ctx.handle
    dev = [hip.from_numpy(a) for a in c.V]
    m_in = hip.from_numpy(c.mu_e)
    outs = [hip.from_numpy(sentinel(n, "f64")) for _ in range(3)] + [hip.from_numpy(sentinel((2, 2, 2), "f64")) for _ in range(3)]
    newV = [hip.from_numpy(sentinel(a.shape, "f64")) for a in c.V]
    P = lambda t: C.c_void_p(t.data_ptr())
    D = lambda *xs: [C.c_double(x) for x in xs]
    Vp, ok = [P(t) for t in dev], D(*c.d)
    ev, tv, pv = lib.ns3d_eddy_viscosity_f64, lib.ns3d_update_tau_var_f64, lib.ns3d_predict_var_f64
    mo, sc = P(outs[0]), D(c.mu, c.rho, c.length)
    nan, inf = float("nan"), float("inf")
    calls = {"ns3d_eddy_viscosity_f64": {
        "null context": lambda: ev(None, mo, *Vp, *sc, *ok, 3, 3, 3),
        "null mu_e": lambda: ev(h, None, *Vp, *sc, *ok, 3, 3, 3),
        "null Vx": lambda: ev(h, mo, None, Vp[1], Vp[2], *sc, *ok, 3, 3, 3),
        "null Vy": lambda: ev(h, mo, Vp[0], None, Vp[2], *sc, *ok, 3, 3, 3),
        "null Vz": lambda: ev(h, mo, Vp[0], Vp[1], None, *sc, *ok, 3, 3, 3),
        "grid 2x3x3": lambda: ev(h, mo, *Vp, *sc, *ok, 2, 3, 3),
        "grid 3x2x3": lambda: ev(h, mo, *Vp, *sc, *ok, 3, 2, 3),
        "grid 3x3x2": lambda: ev(h, mo, *Vp, *sc, *ok, 3, 3, 2),
        "dx 0": lambda: ev(h, mo, *Vp, *sc, *D(0.0, c.d[1], c.d[2]), 3, 3, 3),
        "dy negative": lambda: ev(h, mo, *Vp, *sc, *D(c.d[0], -c.d[1], c.d[2]), 3, 3, 3),
        "dz nan": lambda: ev(h, mo, *Vp, *sc, *D(c.d[0], c.d[1], nan), 3, 3, 3),
        "dx inf": lambda: ev(h, mo, *Vp, *sc, *D(inf, c.d[1], c.d[2]), 3, 3, 3),
        "mu negative": lambda: ev(h, mo, *Vp, *D(-1e-3, c.rho, c.length), *ok, 3, 3, 3),
        "mu nan": lambda: ev(h, mo, *Vp, *D(nan, c.rho, c.length), *ok, 3, 3, 3),
        "rho negative": lambda: ev(h, mo, *Vp, *D(c.mu, -1.0, c.length), *ok, 3, 3, 3),
        "rho inf": lambda: ev(h, mo, *Vp, *D(c.mu, inf, c.length), *ok, 3, 3, 3),
        "length negative": lambda: ev(h, mo, *Vp, *D(c.mu, c.rho, -0.1), *ok, 3, 3, 3),
        "length nan": lambda: ev(h, mo, *Vp, *D(c.mu, c.rho, nan), *ok, 3, 3, 3),
        "mu_e is Vx": lambda: ev(h, Vp[0], *Vp, *sc, *ok, 3, 3, 3),
        "mu_e is Vy": lambda: ev(h, Vp[1], *Vp, *sc, *ok, 3, 3, 3),
        "mu_e is Vz": lambda: ev(h, Vp[2], *Vp, *sc, *ok, 3, 3, 3),
    }, "ns3d_update_tau_var_f64": {
        "null context": lambda: tv(None, *[P(t) for t in outs], *Vp, P(m_in), *ok, 3, 3, 3),
        "null txx": lambda: tv(h, None, *[P(t) for t in outs[1:]], *Vp, P(m_in), *ok, 3, 3, 3),
        "null mu_e": lambda: tv(h, *[P(t) for t in outs], *Vp, None, *ok, 3, 3, 3),
        "grid 1x3x3": lambda: tv(h, *[P(t) for t in outs], *Vp, P(m_in), *ok, 1, 3, 3),
    }, "ns3d_predict_var_f64": {
        "null context": lambda: pv(None, *[P(t) for t in newV], *Vp, P(m_in), *D(c.rho, c.g, c.step), *ok, 3, 3, 3),
        "null Vz_new": lambda: pv(h, P(newV[0]), P(newV[1]), None, *Vp, P(m_in), *D(c.rho, c.g, c.step), *ok, 3, 3, 3),
        "null mu_e": lambda: pv(h, *[P(t) for t in newV], *Vp, None, *D(c.rho, c.g, c.step), *ok, 3, 3, 3),
        "grid 3x3x1": lambda: pv(h, *[P(t) for t in newV], *Vp, P(m_in), *D(c.rho, c.g, c.step), *ok, 3, 3, 1),
        "Vx_new is Vx": lambda: pv(h, Vp[0], P(newV[1]), P(newV[2]), *Vp, P(m_in), *D(c.rho, c.g, c.step), *ok, 3, 3, 3),
        "Vz_new is Vz": lambda: pv(h, P(newV[0]), P(newV[1]), Vp[2], *Vp, P(m_in), *D(c.rho, c.g, c.step), *ok, 3, 3, 3),
    }}
    for name, table in calls.items():
        for what, call in table.items():
            assert call() == L.NS3D_ERR_ARG == 1, (name, what)
            assert L.last_error().startswith(name + ": "), (name, what, L.last_error())
    knob = lib.ns3d_set_turbulence
    for what, args in {"null context": (None, 1, 0.1, mo), "unknown model": (h, 2, 0.1, mo), "model -1": (h, -1, 0.1, mo),
                       "length negative": (h, 1, -0.1, mo), "length nan": (h, 1, nan, mo), "length inf": (h, 1, inf, mo),
                       "null mu_e": (h, 1, 0.1, None)}.items():
        assert knob(*args) == L.NS3D_ERR_ARG, what
        assert L.last_error().startswith("ns3d_set_turbulence: "), (what, L.last_error())
        assert what == "null context" or lib.ns3d_turbulence(h) == L.NS3D_TURB_NONE
    assert knob(h, 1, 0.1, mo) == 0 and lib.ns3d_turbulence(h) == 1
    assert knob(h, 2, 0.1, mo) == L.NS3D_ERR_ARG and lib.ns3d_turbulence(h) == 1          # a refused call leaves the setting
    assert knob(h, 0, nan, None) == 0 and lib.ns3d_turbulence(h) == 0                      # NONE ignores the other two
    ctx.sync()
    for t, a in zip(dev + [m_in], c.V + [c.mu_e]):
        assert bits_equal(hip.to_numpy(t), a)
    for t in outs + newV:
        assert np.all(hip.to_numpy(t) == 777.0)
    with pytest.raises(L.Ns3dError):
        hip.eddy_viscosity(hip.zeros((3, 3, 4)), *dev, c.mu, c.rho, c.length, *c.d, ctx=ctx)                 # shape
    with pytest.raises(L.Ns3dError):
        hip.eddy_viscosity(hip.zeros(n, torch.float32), *dev, c.mu, c.rho, c.length, *c.d, ctx=ctx)          # dtype
    with pytest.raises(L.Ns3dError):
        hip.predict_var(*newV, *dev, hip.zeros((3, 3, 2)), c.rho, c.g, c.step, *c.d, ctx=ctx)
    with pytest.raises(L.Ns3dError):
        hip.update_tau_var(*outs, *dev, hip.zeros(n, torch.float32), *c.d, ctx=ctx)
    with pytest.raises(L.Ns3dError):
        ctx.set_turbulence("k-epsilon")
    with pytest.raises(L.Ns3dError):
        ctx.set_turbulence("smagorinsky", 0.1)                                                                 # no mu_e
    # the context is still usable
    assert_bits(run_eddy(hip, ctx, c), c.mu_e, "after the errors")
