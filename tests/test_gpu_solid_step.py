"""GPU tests of the whole step with an obstacle (ns3d_set_obstacle inside ns3d_time_step) against its CPU statement: the oracle drivers
with obstacle= and initial= on the scenario of tests/solid_step_cases.py — a seeded state in which every bit of the body's mask acts on a
non-zero value (tests/test_solid_step_host.py asserts that on the CPU: a masking call left out, or a mask bit ignored, changes the
result these tests compare with).  STRICT: bit for bit.  NS3D_IEEE_DIV and FAST: the cylinder's own mask against the cylinder call on the
same context.  The knob belongs to its context.  The body force of the drivers' monitor against the momentum the statement removes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as AR
import solid_step_cases as SS
from util import SHAPES, bits_equal, first_bit_difference

pytestmark = pytest.mark.gpu

STEP_SHAPES = {"Pr": "c", "dPrdtau": "i", "divV": "c", "Vx": "vx", "Vy": "vy", "Vz": "vz", "Vx_o": "vx", "Vy_o": "vy", "Vz_o": "vz", "C": "c",
               "C_o": "c", "txx": "c", "tyy": "c", "tzz": "c", "txy": "s", "txz": "s", "tyz": "s"}
DTS = ["f64", "f32"]


def host_state(dt, initial=None):
    """the seventeen arrays of ns3d_step_fields on the host: zeros, and the scenario's state (or `initial`) in the five fields"""
    host = {k: np.zeros(SHAPES[kind](*SS.GRID), dtype=SS.DTYPES[dt], order="F") for k, kind in STEP_SHAPES.items()}
    for k, a in (SS.initial_state(dt) if initial is None else initial).items():
        host[k] = np.asfortranarray(np.asarray(a).astype(SS.DTYPES[dt]))
    return host


def step_params(script, niter, advection="reference", pressure=0):
    """(the package's parameters, lib.StepParams) of the script at 24×15×15 with faithful = 0"""
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.params import gpu_params, multi_params
    p = multi_params(SS.NX) if script == "multi" else gpu_params(SS.NX)
    assert (p.nx, p.ny, p.nz) == SS.GRID
    common = dict(nx=p.nx, ny=p.ny, nz=p.nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp, dx=p.dx, dy=p.dy, dz=p.dz,
                  eps=p.eps, niter=niter, nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc, a2=p.a2, b2=p.b2, ox=p.ox, oy=p.oy,
                  sinb=p.sinb, cosb=p.cosb, lx=p.lx, ly=p.ly, lz=p.lz, faithful=0, pressure=pressure, write_stress=0)
    if script == "multi":
        sp = L.StepParams(script=L.NS3D_BC_MULTI, xco_g=p.xco_g, yco_g=p.yco_g, zco_g=p.zco_g, owns_inlet=int(bool(p.owns_inlet)),
                          owns_outlet=int(bool(p.owns_outlet)), vin=p.vin, **common)
    else:
        sp = L.StepParams(script=L.NS3D_BC_GPU, xco_g=0.0, yco_g=0.0, zco_g=0.0, owns_inlet=0, owns_outlet=0, vin=0.0, **common)
    return p, sp


def upload_mask(mask):
    """a host mask (nx+1, ny+1, nz+1) as the flat uint8 device tensor the library reads"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(mask).reshape(-1, order="F"))).cuda()


def first_masking(hip, ctx, script, f, p, mask):
    """multi.jl:372, the masking before the time loop: ns3d_set_solid with the mask, or the cylinder call; gpu.jl has none"""
    if script != "multi":
        return
    if mask is not None:
        hip.set_solid(f.C, f.Vx, f.Vy, f.Vz, mask, ctx=ctx)
    else:
        hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz,
                         p.dx, p.dy, p.dz, ctx=ctx)


def steps_on(hip, script, dt, ctx, mask, advection="reference", in_arena=False, host=None, nt=SS.NT, first=True):
    """The scenario's state (or `host`) uploaded — on plain tensors, or with the mask in a guarded arena —, multi.jl's masking before
    the loop, ctx.set_obstacle(mask), nt ns3d_time_step calls with niter = 3·nchk (write_stress on the last), all seventeen arrays
    downloaded.  mask: a host mask, or None — the cylinder.  The context's knobs are put back before anything is read.  Returns
    steps [(iterations, errs)], fields {name: array}, and with in_arena the arena (guards checked, mask compared)."""
    sc = SS.scenario(script, dt)
    host = host_state(dt) if host is None else host
    p, sp = step_params(script, sc.niter, advection)
    ar = None
    if in_arena:
        arrays = [(k, a, True) for k, a in host.items()]
        if mask is not None:
            arrays.append(("mask", np.asfortranarray(mask), False))
        ar = AR.Arena(arrays, "cuda")
        f = SimpleNamespace(**{k: ar.t[k] for k in host})
        dmask = ar.t["mask"] if mask is not None else None
    else:
        f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in host.items()})
        dmask = None if mask is None else upload_mask(mask)
    torch.cuda.synchronize()
    ctx.set_advection(advection)
    out = []
    try:
        if first:
            first_masking(hip, ctx, script, f, p, dmask)
        ctx.set_obstacle(dmask)
        assert (ctx.obstacle() is None) == (dmask is None)
        for step in range(1, nt + 1):
            sp.write_stress = 1 if step == nt else 0
            out.append(hip.time_step(f, sp, ctx=ctx))
        ctx.sync()
    finally:
        ctx.set_obstacle(None)
        ctx.set_advection("reference")
    torch.cuda.synchronize()
    got = SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}, arena=ar)
    if in_arena:
        ar.assert_clean("time_step %s %s %s with an obstacle" % (script, dt, advection))
        if mask is not None:
            assert np.array_equal(ar.get("mask"), mask), "the step changed the mask"
    return got


def same_steps(got, want):
    return len(got) == len(want) and all(a[0] == b[0] and len(a[1]) == len(b[1]) and
                                         np.array_equal(np.float64(a[1]), np.float64(b[1]), equal_nan=True) for a, b in zip(got, want))


def assert_equals_the_oracle(got, script, dt, advection, mask="body", what=""):
    """all of C, Pr, Vx, Vy, Vz, the *_o buffers, dPrdtau and divV, the iteration counts and err histories: the oracle driver's"""
    want, info = SS.scenario_ref(script, dt, advection, mask)
    steps = [(it, list(e)) for it, e in zip(info.iters, info.errs)]
    assert same_steps(got.steps, steps), (what, script, dt, advection, got.steps, steps)
    for k in SS.ELEVEN:
        assert bits_equal(got.fields[k], want[k]), (what, script, dt, advection, k, first_bit_difference(got.fields[k], want[k]))


def assert_same_run(a, b, what=""):
    assert same_steps(a.steps, b.steps), (what, a.steps, b.steps)
    for k in STEP_SHAPES:
        assert bits_equal(a.fields[k], b.fields[k]), (what, k, first_bit_difference(a.fields[k], b.fields[k]))


# ---- STRICT against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advection", SS.SCHEMES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_step_with_an_obstacle_equals_the_oracle_driver(hip, oracle, script, dt, advection):
    """Two steps of 42 PT iterations from the scenario's state with the three-piece body: eleven arrays, iteration counts and err
    histories bit for bit, both scripts, both element types, both advection schemes.  The result is finite and is not the cylinder's."""
    ctx = hip.Context(0, "strict", async_=True)
    got = steps_on(hip, script, dt, ctx, SS.body_mask(), advection)
    ctx.close()
    assert all(np.isfinite(a).all() for a in got.fields.values())
    assert_equals_the_oracle(got, script, dt, advection)
    other, _ = SS.scenario_ref(script, dt, advection, None)
    assert not bits_equal(got.fields["Vx"], other["Vx"]) and not bits_equal(got.fields["C"], other["C"])


# ---- NS3D_IEEE_DIV and FAST --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee_div", "fast"])
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_cylinders_own_mask_is_the_cylinder_step_in_every_mode(hip, oracle, script, mode):
    """The masking is compiled once and does not depend on the arithmetic mode: from the scenario's state the step with the cylinder's
    own mask equals the SAME context's step without an obstacle, all seventeen arrays, float64.  The mask is the device's
    (solid.mask_of_cylinder) and equals the one the host tests read off the oracle's set_cylinder."""
    from navierstokes3d_amd import solid as S
    ctx = hip.Context(0, "fast", async_=True) if mode == "fast" else hip.Context(0, "strict", async_=True, ieee_div=True)
    p, _ = step_params(script, 1)
    cyl = (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb) + ((p.xco_g, p.yco_g, p.zco_g) if script == "multi" else ()) + (p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    mask = S.to_numpy(S.mask_of_cylinder(ctx, SS.GRID, *cyl))
    assert np.array_equal(mask, SS.cylinder_mask(script, "f64"))
    plain = steps_on(hip, script, "f64", ctx, None)
    masked = steps_on(hip, script, "f64", ctx, mask)
    ctx.close()
    assert all(np.isfinite(a).all() for a in plain.fields.values()) and np.abs(plain.fields["Vx"]).max() > 0
    assert_same_run(masked, plain, (script, mode))
    if mode == "ieee_div":                  # NS3D_IEEE_DIV returns STRICT's bits: the oracle's
        assert_equals_the_oracle(masked, script, "f64", "reference", "cylinder", mode)


# ---- the knob belongs to its context ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_obstacle_belongs_to_its_context(hip, oracle, script):
    """Two contexts step alternately from the same state, A with the body and B without: each equals its solo run (the oracle's).
    After set_obstacle(None) A's next step is the cylinder step: a context that never had an obstacle, started from A's state."""
    sc = SS.scenario(script, "f64")
    A, B = hip.Context(0, "strict", async_=True), hip.Context(0, "strict", async_=True)
    pa, spa = step_params(script, sc.niter)
    _, spb = step_params(script, sc.niter)
    fa = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in host_state("f64").items()})
    fb = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in host_state("f64").items()})
    dmask = upload_mask(sc.mask)
    torch.cuda.synchronize()
    ra, rb = [], []
    try:
        first_masking(hip, A, script, fa, pa, dmask)
        first_masking(hip, B, script, fb, pa, None)
        A.set_obstacle(dmask)
        assert A.obstacle() == dmask.data_ptr() and B.obstacle() is None
        for step in (1, 2):
            spa.write_stress = spb.write_stress = 1 if step == 2 else 0
            if step == 1:
                ra.append(hip.time_step(fa, spa, ctx=A)); rb.append(hip.time_step(fb, spb, ctx=B))
            else:
                rb.append(hip.time_step(fb, spb, ctx=B)); ra.append(hip.time_step(fa, spa, ctx=A))
        A.sync(); B.sync()
        get = lambda f, r: SimpleNamespace(steps=r, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES})
        ga, gb = get(fa, ra), get(fb, rb)
        assert_equals_the_oracle(ga, script, "f64", "reference", "body", "A")
        assert_equals_the_oracle(gb, script, "f64", "reference", None, "B")
        A.set_obstacle(None)
        assert A.obstacle() is None
        third = [hip.time_step(fa, spa, ctx=A)]
        A.sync()
        g3 = get(fa, third)
    finally:
        A.set_obstacle(None)
        A.close(); B.close()
    fresh = hip.Context(0, "strict", async_=True)
    want = steps_on(hip, script, "f64", fresh, None, host=ga.fields, nt=1, first=False)
    fresh.close()
    assert_same_run(g3, want, "A after set_obstacle(None)")
    assert not bits_equal(g3.fields["Vx"], ga.fields["Vx"])


# ---- the force ---------------------------------------------------------------------------------------------------------------------------
def test_the_body_force_is_the_momentum_the_statement_removes(hip, oracle):
    """runme(obstacle=body, diagnostics=True, nt=2, niter_cap=42) from gpu.jl's own initial state — the power-law inflow meets the body
    in step 1 — against runme_ref(obstacle=…): the five fields, iteration counts and err histories bit for bit, and each force[q] =
    ρ·dx·dy·dz/dt·(m₁ + m₂) against the same expression of info.removed's fsum values.  In STRICT the summed terms are the same numbers,
    so the bar is the any-order summation bound n·2⁻⁵³·Σ|term| of each of the two sums, scaled by the factor, plus one ulp (2⁻⁵² of
    the magnitude bound) for each of the six operations of the expression: four in the factor, the addition, the product."""
    from navierstokes3d_amd.driver import runme
    from oracle.driver_ref import runme_ref
    f, info = runme(nx=SS.NX, nt=2, niter_cap=42, obstacle=SS.body(), diagnostics=True)
    with np.errstate(all="ignore"):
        fr, ir = runme_ref(nx=SS.NX, nt=2, niter_cap=42, obstacle=SS.body_mask())
    for k in SS.FIVE:
        got = hip.to_numpy(getattr(f, k))
        assert np.isfinite(got).all() and bits_equal(got, fr[k]), (k, first_bit_difference(got, fr[k]))
    assert same_steps(list(zip(info.iters, info.errs)), list(zip(ir.iters, ir.errs))), (info.iters, ir.iters)
    p = ir.params
    factor = p.rho * p.dx * p.dy * p.dz / p.dt
    u = 2.0 ** -53
    assert len(info.diag) == 2 and len(ir.removed) == 2
    for step, (rec, (m1, m2)) in enumerate(zip(info.diag, ir.removed)):
        assert m1[1] == list(SS.BIT_COUNTS[1:]) and m1[2][0] > 0, "the flow does not meet the body"
        for q in range(3):
            for got, (sums, counts, mags) in ((rec.mom_predict[q], m1), (rec.mom_correct[q], m2)):
                print("step %d, direction %d: removed %r, fsum %r, bound %.3e" % (step + 1, q, got, sums[q], counts[q] * u * mags[q]))
                assert abs(got - sums[q]) <= counts[q] * u * mags[q], (step, q, got, sums[q])
            want = factor * (m1[0][q] + m2[0][q])
            bound = factor * u * (m1[1][q] * m1[2][q] + m2[1][q] * m2[2][q]) + 6 * 2.0 ** -52 * factor * (abs(m1[0][q]) + abs(m2[0][q]))
            print("step %d, force[%d] = %r, statement %r, bound %.3e" % (step + 1, q, rec.force[q], want, bound))
            assert abs(rec.force[q] - want) <= bound, (step, q, rec.force[q], want, bound)
        assert any(abs(v) > 0 for v in rec.force)
