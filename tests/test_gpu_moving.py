"""GPU tests of the moving-obstacle calls (include/ns3d.h): ns3d_set_solid_moving, ns3d_solid_momentum_moving and ns3d_mesh_transform bit
for bit against their NumPy statements (tests/moving_ref.py) on STRICT, NS3D_IEEE_DIV and FAST contexts, the masking kernel at every
address mod 16 and in a guarded arena, the body's exact zero divergence through ns3d_update_divV, ns3d_set_obstacle_motion inside
ns3d_time_step against the CPU statement of the whole step (tests/moving_cases.py: a turning box mesh, a translating one, the
cylinder's own mask spinning), the `motion` keyword of both drivers, stream order and every NS3D_ERR_ARG."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as AR
import moving_cases as MC
import moving_ref as MR
import solid_ref as SR
import solid_step_cases as SS
import stream_order as SO
import test_gpu_solid_step as GS
from util import bits_equal, fields, first_bit_difference, rel_l2, rnd

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
DTS = ["f64", "f32"]
GID = lambda n: "%dx%dx%d" % tuple(n)
MOTION = (0.31, -0.77, 0.13, 1.9, -2.3, 0.71, 7.3, 4.15, 2.9)      # nine distinct numbers, a centre off every node
SPACING = (0.3, 0.7, 0.2)
ORIGIN = (3, 1, 2)


@pytest.fixture(scope="module")
def ctxs(hip):
    out = {"strict": hip.Context(0, "strict"), "ieee_div": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def delay(hip):
    return SO.Delay()


def _masks(n, seed):
    """a body (a box: whole chunks of zeros around it), random flags at 5 % of the points, and random bytes — bits at invalid points
    and bits 4-7 included"""
    from navierstokes3d_amd import solid as S
    nx, ny, nz = n
    rng = np.random.Generator(np.random.MT19937(seed))
    shape = (nx + 1, ny + 1, nz + 1)
    box = SR.voxelize(S.box_mesh((0.2 * nx, 0.3 * ny, 0.2 * nz), (0.8 * nx, 0.9 * ny, 0.7 * nz)), *n)
    return [box, np.asfortranarray((rng.integers(0, 16, shape) * (rng.random(shape) < 0.05)).astype(np.uint8)),
            np.asfortranarray(rng.integers(0, 256, shape).astype(np.uint8))]


def _up(mask):
    return GS.upload_mask(np.array(mask))       # a writable copy: the shared masks are read-only


# ---- ns3d_set_solid_moving ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(5, 4, 3), (17, 9, 5), (67, 19, 35), (8, 6, 5)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_moving_returns_the_bits_of_the_statement(hip, ctxs, dt, n):
    """three masks per grid, every context kind: C and the three velocities equal the statement's; with C NULL the velocities still
    do; with U = ω = +0.0 the call returns ns3d_set_solid's bits.  67 crosses 64 in x; the row and plane decode act on every grid."""
    host = fields(*n, ["c", "vx", "vy", "vz"], 9, NP[dt])
    for mask in _masks(n, 3):
        ref = [h.copy() for h in host]
        MR.set_solid_moving(*ref, mask, MOTION, SPACING, ORIGIN)
        assert not bits_equal(ref[1], host[1]) and not bits_equal(ref[3], host[3])
        dm = _up(mask)
        for name, ctx in ctxs.items():
            dev = [hip.from_numpy(h) for h in host]
            hip.set_solid_moving(*dev, dm, MOTION, *SPACING, origin=ORIGIN, ctx=ctx)
            nul = [hip.from_numpy(h) for h in host[1:]]
            hip.set_solid_moving(None, *nul, dm, MOTION, *SPACING, origin=ORIGIN, ctx=ctx)
            zero, plain = [hip.from_numpy(h) for h in host], [hip.from_numpy(h) for h in host]
            hip.set_solid_moving(*zero, dm, (0.0,) * 6 + MOTION[6:], *SPACING, origin=ORIGIN, ctx=ctx)
            hip.set_solid(*plain, dm, ctx=ctx)
            ctx.sync()
            for k, d, r in zip(("C", "Vx", "Vy", "Vz"), dev, ref):
                assert bits_equal(hip.to_numpy(d), r), (name, k, first_bit_difference(hip.to_numpy(d), r))
            for k, d, r in zip(("Vx", "Vy", "Vz"), nul, ref[1:]):
                assert bits_equal(hip.to_numpy(d), r), (name, "C NULL", k)
            for k, a, b in zip(("C", "Vx", "Vy", "Vz"), zero, plain):
                assert bits_equal(hip.to_numpy(a), hip.to_numpy(b)), (name, "zero motion", k)
        assert np.array_equal(dm.cpu().numpy(), mask.reshape(-1, order="F"))
    none = [hip.from_numpy(h) for h in host]        # origin NULL: zeros
    hip.set_solid_moving(*none, dm, MOTION, *SPACING, ctx=ctxs["strict"])
    ctxs["strict"].sync()
    ref = [h.copy() for h in host]
    MR.set_solid_moving(*ref, mask, MOTION, SPACING)
    assert all(bits_equal(hip.to_numpy(d), r) for d, r in zip(none, ref))


@pytest.mark.parametrize("n", [(3, 3, 3), (5, 4, 3), (4, 4, 4)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_moving_at_every_lead(hip, ctxs, dt, n):
    """the mask at byte offsets 0…15 of a larger tensor, N = 64, 120 and 125 bytes (the lead and tail paths of the 16-byte chunks), a
    random hostile mask; the bytes around it — all ones: read as flags they would store — are unchanged"""
    nx, ny, nz = n
    N = (nx + 1) * (ny + 1) * (nz + 1)
    assert N in (64, 120, 125)
    host = fields(*n, ["c", "vx", "vy", "vz"], 9, NP[dt])
    rng = np.random.Generator(np.random.MT19937(6))
    ctx = ctxs["strict"]
    for lead in range(16):
        mask = np.asfortranarray(rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8))
        big = np.full(N + 64, 0xFF, dtype=np.uint8)
        big[16 + lead:16 + lead + N] = mask.reshape(-1, order="F")
        dbig = torch.from_numpy(big).cuda()
        view = dbig[16 + lead:16 + lead + N]
        assert dbig.data_ptr() % 16 == 0 and view.data_ptr() % 16 == lead
        dev = [hip.from_numpy(h) for h in host]
        torch.cuda.synchronize()
        hip.set_solid_moving(*dev, view, MOTION, *SPACING, origin=ORIGIN, ctx=ctx)
        ctx.sync()
        ref = [h.copy() for h in host]
        MR.set_solid_moving(*ref, mask, MOTION, SPACING, ORIGIN)
        for name, d, r in zip(("C", "Vx", "Vy", "Vz"), dev, ref):
            assert bits_equal(hip.to_numpy(d), r), (lead, name, first_bit_difference(hip.to_numpy(d), r))
        assert np.array_equal(dbig.cpu().numpy(), big), lead


@pytest.mark.parametrize("n", [(5, 4, 3), (33, 6, 5)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_moving_hostile_mask_in_a_guarded_arena(hip, ctxs, dt, n):
    """0xFF everywhere — every bit at every invalid point — touches no entry outside the four arrays, which sit at odd element offsets"""
    nx, ny, nz = n
    host = fields(*n, ["c", "vx", "vy", "vz"], 5, NP[dt])
    mask = np.full((nx + 1, ny + 1, nz + 1), 0xFF, dtype=np.uint8, order="F")
    ar = AR.Arena([(k, h, True) for k, h in zip(("C", "Vx", "Vy", "Vz"), host)] + [("mask", mask, False)], "cuda")
    ctx = ctxs["strict"]
    hip.set_solid_moving(ar["C"], ar["Vx"], ar["Vy"], ar["Vz"], ar["mask"], MOTION, *SPACING, origin=ORIGIN, ctx=ctx)
    ctx.sync()
    ar.assert_clean("set_solid_moving")
    ref = [h.copy() for h in host]
    MR.set_solid_moving(*ref, mask, MOTION, SPACING, ORIGIN)
    for k, r in zip(("C", "Vx", "Vy", "Vz"), ref):
        assert bits_equal(ar.get(k), r), k
    assert np.array_equal(ar.get("mask"), mask)


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
def test_the_body_has_exactly_zero_divergence(hip, ctxs, dt, mode):
    """ns3d_update_divV of the stored field is exactly +0.0 in every cell whose six faces are masked"""
    n = (17, 9, 5)
    mask = _masks(n, 1)[0]
    host = fields(*n, ["c", "vx", "vy", "vz"], 5, NP[dt])
    ctx = ctxs[mode]
    dev = [hip.from_numpy(h) for h in host]
    div = hip.from_numpy(rnd(77, n, NP[dt]))
    hip.set_solid_moving(*dev, _up(mask), MOTION, *SPACING, origin=ORIGIN, ctx=ctx)
    hip.update_divV(div, *dev[1:], *SPACING, ctx=ctx)
    ctx.sync()
    bx, by, bz = MR._bits(mask, n)[1:]
    full = bx[:-1] & bx[1:] & by[:, :-1] & by[:, 1:] & bz[:, :, :-1] & bz[:, :, 1:]
    got = hip.to_numpy(div)
    assert full.sum() >= 60 and (got[full] == 0).all() and not np.signbit(got[full]).any() and (got[~full] != 0).any()


# ---- ns3d_solid_momentum_moving ----------------------------------------------------------------------------------------------------------
def _within_bound(got, terms):
    """the any-order summation bound n·2⁻⁵³·Σ|term| around math.fsum of the same terms (tests/test_gpu_solid.py)"""
    exact, n, mag = math.fsum(terms.tolist()), terms.size, math.fsum(np.abs(terms).tolist())
    return abs(got - exact) <= n * 2.0 ** -53 * mag, (got, exact, n, mag)


SEAMS = [((0, 0, 0), (0, 0, 0)), ((1, 0, 0), (0, 0, 1)), ((0, 1, 0), (1, 0, 0)), ((0, 0, 1), (0, 1, 0)), ((1, 1, 1), (1, 1, 1))]


@pytest.mark.parametrize("n", [(13, 11, 9), (3, 255, 63), (3, 1023, 127)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_solid_momentum_moving_counts_and_sums(hip, ctxs, dt, n):
    """a random hostile mask, with and without seam flags: the counts exact, the sums within the any-order bound of the statement's
    terms, equal across context kinds and calls; zero motion returns ns3d_solid_momentum's bits.  (3,255,63) and (3,1023,127) leave
    512 and 2 048 partials: the second trip of k_mom_final's loop."""
    from navierstokes3d_amd import diag as D
    assert n[1] < 255 or D.launch_geometry(*n)[0] > 256
    nx, ny, nz = n
    Vx, Vy, Vz = fields(*n, ["vx", "vy", "vz"], 7, NP[dt])
    rng = np.random.Generator(np.random.MT19937(4))
    mask = np.asfortranarray(rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8))
    d, dm = [hip.from_numpy(a) for a in (Vx, Vy, Vz)], _up(mask)
    torch.cuda.synchronize()
    for lo, hi in SEAMS:
        terms = MR.momentum_terms(Vx, Vy, Vz, mask, MOTION, SPACING, ORIGIN, lo, hi)
        first = None
        for name, ctx in ctxs.items():
            mom, cnt = hip.solid_momentum_moving(*d, dm, MOTION, *SPACING, origin=ORIGIN, seam_lo=lo, seam_hi=hi, ctx=ctx)
            assert list(cnt) == [t.size for t in terms] and min(cnt) > 0, (lo, hi, name, cnt)
            for q in range(3):
                ok, fig = _within_bound(mom[q], terms[q])
                assert ok, (lo, hi, name, q, fig)
            first = first or mom
            assert np.array_equal(np.array(mom), np.array(first)), "the sums depend on the context or the call"
        again, _ = hip.solid_momentum_moving(*d, dm, MOTION, *SPACING, origin=ORIGIN, seam_lo=lo, seam_hi=hi, ctx=ctxs["strict"])
        assert np.array_equal(np.array(again), np.array(first))
        zero = hip.solid_momentum_moving(*d, dm, (0.0,) * 6 + MOTION[6:], *SPACING, origin=ORIGIN, seam_lo=lo, seam_hi=hi, ctx=ctxs["strict"])
        plain = hip.solid_momentum(*d, dm, lo, hi, ctx=ctxs["strict"])
        assert np.array_equal(np.array(zero[0]), np.array(plain[0])) and zero[1] == plain[1]
        static = SR.momentum_terms(Vx, Vy, Vz, mask, lo, hi)
        assert not np.array_equal(np.array(first), np.array(plain[0])) and all(a.size == b.size for a, b in zip(static, terms))


# ---- ns3d_mesh_transform -----------------------------------------------------------------------------------------------------------------
def _pose():
    from navierstokes3d_amd import solid as S
    return S.rotation((0.4, -1.1, 0.8), 0.9), np.array([3.3, 2.1, 4.7]), np.array([0.6, -0.25, 1.5]), np.array([1.0 / 24, 0.04, 0.05])


@pytest.mark.parametrize("n_tri", [0, 1, 63, 64, 65, 257])
def test_mesh_transform_returns_the_bits_of_the_statement(hip, ctxs, n_tri):
    """every context kind, out of place (the input untouched) and in place"""
    R, pivot, shift, d = _pose()
    tri = rnd(5, (n_tri, 3, 3), np.float64, -3.0, 30.0).reshape(-1)
    want = MR.transform(tri, R, pivot, shift, d).reshape(-1)
    for name, ctx in ctxs.items():
        src = torch.from_numpy(tri.copy()).cuda()
        out = torch.full_like(src, 777.0)
        hip.mesh_transform(out, src, R, pivot, shift, d, ctx=ctx)
        ctx.sync()
        assert bits_equal(out.cpu().numpy(), want) and bits_equal(src.cpu().numpy(), tri), name
        hip.mesh_transform(src, src, R, pivot, shift, d, ctx=ctx)
        ctx.sync()
        assert bits_equal(src.cpu().numpy(), want), (name, "in place")
    assert n_tri == 0 or not bits_equal(want, tri)


def test_mesh_transform_passes_a_nan_vertex_through_and_refuses_overlap(hip, ctxs):
    from navierstokes3d_amd import lib as L
    R, pivot, shift, d = _pose()
    tri = rnd(6, (9, 3, 3), np.float64, -3.0, 30.0).reshape(-1)
    tri[9 * 4 + 3] = np.nan
    tri[9 * 7 + 2] = np.inf
    with np.errstate(all="ignore"):
        want = MR.transform(tri, R, pivot, shift, d).reshape(-1)
    assert np.isnan(want[9 * 4 + 3:9 * 4 + 6]).all() and np.isfinite(want[:9 * 4 + 3]).all() and not np.isfinite(want[9 * 7:9 * 7 + 3]).all()
    ctx = ctxs["strict"]
    src = torch.from_numpy(tri.copy()).cuda()
    out = torch.empty_like(src)
    hip.mesh_transform(out, src, R, pivot, shift, d, ctx=ctx)
    ctx.sync()
    assert bits_equal(out.cpu().numpy(), want)
    big = torch.from_numpy(np.concatenate([tri, tri])).cuda()
    before = big.cpu().numpy()
    for a, b in ((big[9:90], big[0:81]), (big[0:81], big[9:90]), (big[72:153], big[0:81])):
        with pytest.raises(L.Ns3dError, match="overlap"):
            hip.mesh_transform(a, b, R, pivot, shift, d, ctx=ctx)
    ctx.sync()
    assert bits_equal(big.cpu().numpy(), before)
    hip.mesh_transform(big[81:162], big[0:81], R, pivot, shift, d, ctx=ctx)       # adjacent, not overlapping
    ctx.sync()
    assert bits_equal(big[81:162].cpu().numpy(), want)


# ---- the step ----------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = GS.STEP_SHAPES


def device_steps(hip, ctx, script, dt, name, host, sp, nt=MC.NT, pre=False, advection="reference", wale=None, sca=None, knob=True):
    """`host` uploaded, the mover's mask and mesh on the device, the pose of t = 0 stored first with `pre` (multi.jl:372); per step the
    mask rebuilt in place when the pose differs from the one it holds (ns3d_mesh_transform of the ORIGINAL mesh, ns3d_voxelize into
    the same buffer), ns3d_set_obstacle_motion with the pose's numbers, ns3d_time_step.  Every knob is cleared before anything is
    read.  Returns steps, fields, the mask after each step, mu_e."""
    mv = MC.mover(script, name, dt)
    f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in host.items()})
    dmask = _up(mv.mask0)
    tri0 = posed = None
    if mv.tri is not None:
        tri0 = torch.from_numpy(np.ascontiguousarray(mv.tri, dtype=np.float64).reshape(-1)).cuda()
        posed = torch.empty_like(tri0)
    mu_e = hip.from_numpy(np.full(MC.GRID, 777.0, order="F"))
    torch.cuda.synchronize()
    last = (np.eye(3), np.zeros(3))
    out, masks = [], []
    try:
        ctx.set_advection(advection)
        if wale is not None:
            ctx.set_turbulence("wale", wale, mu_e)
        if sca is not None:
            ctx.set_scalar(sca["kappa"], sca["sct"], sca["bg"], sca["c_ref"])
        if pre:
            hip.set_solid_moving(f.C, f.Vx, f.Vy, f.Vz, dmask, MR.motion9(mv.poses[0]), *mv.d, ctx=ctx)
        ctx.set_obstacle(dmask)
        for s in range(1, nt + 1):
            R, shift, U, omega, centre = mv.poses[s]
            if tri0 is not None and not (np.array_equal(R, last[0]) and np.array_equal(shift, last[1])):
                hip.mesh_transform(posed, tri0, R, centre - shift, shift, mv.d, ctx=ctx)
                hip.voxelize(dmask, posed, MC.GRID, ctx=ctx)
                last = (R, shift)
            if knob:
                ctx.set_obstacle_motion(MR.motion9(mv.poses[s]))
                assert ctx.obstacle_motion() == MR.motion9(mv.poses[s])
            sp.write_stress = 1 if s == nt else 0
            out.append(hip.time_step(f, sp, ctx=ctx))
            ctx.sync()
            masks.append(dmask.cpu().numpy().reshape(mv.mask0.shape, order="F"))
    finally:
        ctx.set_obstacle_motion(None); ctx.set_obstacle(None); ctx.set_advection("reference"); ctx.set_turbulence(None); ctx.set_scalar(None)
    assert ctx.obstacle_motion() is None
    torch.cuda.synchronize()
    return SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}, masks=masks, mu_e=hip.to_numpy(mu_e))


def _assert_run(got, want, names, what):
    for s, (a, b) in enumerate(zip(got.masks, want.masks[-2 * len(got.masks)::2])):
        assert np.array_equal(a, b), (what, "the mask of step %d" % (s + 1), int((a != b).sum()))
    assert GS.same_steps(got.steps, want.steps), (what, got.steps, want.steps)
    for k in names:
        assert bits_equal(got.fields[k], want.fields[k]), (what, k, first_bit_difference(got.fields[k], want.fields[k]))
    assert all(np.isfinite(a).all() for a in got.fields.values()), what


@pytest.mark.parametrize("mode", ["strict", "ieee"])
@pytest.mark.parametrize("name", MC.MOVERS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_step_under_motion_equals_the_statement(hip, oracle, script, dt, name, mode):
    """three steps of 42 PT iterations from solid_step_cases' seeded state: the mask of every step, eleven arrays, iteration counts
    and err histories, bit for bit — a box mesh whose mask changes every step, a translating one, the cylinder's own mask spinning"""
    ctx = hip.Context(0, "strict", async_=True, ieee_div=mode == "ieee")
    _, sp = GS.step_params(script, MC.NITER)
    got = device_steps(hip, ctx, script, dt, name, GS.host_state(dt), sp, pre=script == "multi")
    ctx.close()
    want = MC.oracle_run(script, dt, name)
    _assert_run(got, want, SS.ELEVEN, (script, dt, name, mode))
    if name != "cylinder":
        assert all(not np.array_equal(a, b) for a, b in zip(got.masks, got.masks[1:]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_step_under_motion_with_maccormack_advection(hip, oracle, script, dt):
    ctx = hip.Context(0, "strict", async_=True)
    _, sp = GS.step_params(script, MC.NITER, "maccormack")
    got = device_steps(hip, ctx, script, dt, "spin", GS.host_state(dt), sp, pre=script == "multi", advection="maccormack")
    ctx.close()
    want = MC.oracle_run(script, dt, "spin", "maccormack")
    _assert_run(got, want, SS.ELEVEN, (script, dt, "maccormack"))
    assert not bits_equal(want.fields["Vx"], MC.oracle_run(script, dt, "spin").fields["Vx"])


@pytest.mark.parametrize("mode", ["strict", "ieee"])
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_step_under_motion_with_wale_and_the_scalar(hip, script, mode):
    """from the script's own initial state, under WALE with the scalar on (float64: scalar_ref.step's statement): seventeen arrays"""
    import sgs_ref
    ctx = hip.Context(0, "strict", async_=True, ieee_div=mode == "ieee")
    p, sp = GS.step_params(script, MC.NITER)
    got = device_steps(hip, ctx, script, "f64", "spin", MC.host_state64(script), sp, wale=sgs_ref.length_of(sgs_ref.WALE, p.dx, p.dy, p.dz),
                       sca=MC.scalar_knob(script))
    ctx.close()
    want = MC.wale_scalar_run(script, "spin")
    _assert_run(got, want, tuple(STEP_SHAPES), (script, "wale + scalar", mode))
    assert bits_equal(got.mu_e, want.mu_e)


@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_step_under_motion_with_the_direct_solve(hip, script):
    """pressure = 1 against the statement with oracle/direct_ref.py's solve, within test_gpu_direct.py's bar for whole runs as
    test_gpu_les.py applies it: per field max(1e-9, 20 × the statement's own rounding level, float64 against long-double sums)"""
    ctx = hip.Context(0, "strict", async_=True)
    _, sp = GS.step_params(script, MC.NITER, pressure=1)
    got = device_steps(hip, ctx, script, "f64", "spin", MC.host_state64(script), sp, nt=2)
    ctx.close()
    want = MC.direct_run(script, "spin")
    levels = None
    vnorm = max(np.sqrt(np.sum(want.fields[n] ** 2)) for n in ("Vx", "Vy", "Vz"))
    if np.finfo(np.longdouble).eps < 1e-18:
        wide = MC.direct_run(script, "spin", np.longdouble)
        levels = {n: rel_l2(wide.fields[n], want.fields[n], vnorm if n.startswith("V") else None) for n in SS.FIVE}
    print("the statement's own rounding level (float64 against long-double sums):", levels)
    for s, (a, b) in enumerate(zip(got.masks, want.masks[::2])):
        assert np.array_equal(a, b), s
    for n in SS.FIVE:
        bar = max(1e-9, 20.0 * levels[n]) if levels else 1e-9
        e = rel_l2(got.fields[n], want.fields[n], vnorm if n.startswith("V") else None)
        print("%s: %.3e (bar %.2e)" % (n, e, bar))
        assert np.isfinite(got.fields[n]).all() and e < bar, (n, e, bar)
    assert [s[0] for s in got.steps] == [0, 0]


# ---- the knob ----------------------------------------------------------------------------------------------------------------------------
def test_the_knob(hip, oracle):
    """motion without an obstacle: NS3D_ERR_ARG, the fields untouched; ns3d_set_obstacle leaves the motion alone; cleared, the step is
    the static obstacle's, bit for bit; the context copies the numbers"""
    from navierstokes3d_amd import lib as L
    lib = L.load()
    ctx = hip.Context(0, "strict", async_=True)
    assert ctx.obstacle_motion() is None and lib.ns3d_obstacle_motion(ctx.handle, None) == 0
    _, sp = GS.step_params("multi", MC.NITER)
    host = GS.host_state("f64")
    f = SimpleNamespace(**{k: hip.from_numpy(a) for k, a in host.items()})
    torch.cuda.synchronize()
    m9 = (C.c_double * 9)(*MOTION)
    L.check(lib.ns3d_set_obstacle_motion(ctx.handle, m9, None))
    m9[0] = 99.0                                            # the caller's array may change: the context holds a copy
    assert ctx.obstacle_motion() == MOTION
    with pytest.raises(L.Ns3dError, match="without a mask"):
        hip.time_step(f, sp, ctx=ctx)
    ctx.sync()
    for k, a in host.items():
        assert bits_equal(hip.to_numpy(getattr(f, k)), a), k
    dmask = _up(MC.box_mask())
    ctx.set_obstacle(dmask)
    assert ctx.obstacle_motion() == MOTION
    ctx.set_obstacle(None)
    assert ctx.obstacle_motion() == MOTION
    for bad in ((float("nan"),) + MOTION[1:], MOTION[:5] + (float("inf"),) + MOTION[6:]):
        with pytest.raises(L.Ns3dError, match="not finite"):
            ctx.set_obstacle_motion(bad)
    with pytest.raises(L.Ns3dError, match="origin"):
        ctx.set_obstacle_motion(MOTION, origin=(0, -1, 0))
    assert ctx.obstacle_motion() == MOTION
    ctx.set_obstacle_motion(None)
    assert ctx.obstacle_motion() is None
    static = GS.steps_on(hip, "multi", "f64", ctx, MC.box_mask(), nt=1, first=False)
    ctx.close()
    fresh = hip.Context(0, "strict", async_=True)
    want = GS.steps_on(hip, "multi", "f64", fresh, MC.box_mask(), nt=1, first=False)
    moving = device_steps(hip, fresh, "multi", "f64", "slide", GS.host_state("f64"), sp, nt=1)
    fresh.close()
    GS.assert_same_run(static, want, "after the motion was cleared")
    assert not bits_equal(moving.fields["Vx"], want.fields["Vx"])


# ---- the drivers -------------------------------------------------------------------------------------------------------------------------
def _run(script, nt, **kw):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    if script == "multi":
        out = run_navierstokes3D(nt=nt, return_info=True, **kw)
        return out[-1].fields, out[-1]
    return runme(nt=nt, **kw)


def _driver_fields(hip, f):
    return {k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES}


def _obstacle(script, name):
    mv = MC.mover(script, name)
    return None if name == "cylinder" else mv.tri


@pytest.mark.parametrize("name", MC.MOVERS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_drivers_one_call_equals_call_by_call_and_the_statement(hip, oracle, script, name):
    """nx = 24, three steps with motion=: ns3d_time_step under the knob against the set_solid_moving calls the driver issues itself —
    seventeen arrays, counts, errs — and both against the oracle driver under the same poses; info.motion holds the pose per step;
    the knobs are cleared"""
    kw = dict(nx=24, mode="strict", niter_cap=MC.NITER, faithful=False, obstacle=_obstacle(script, name), motion=MC.keyword(script, name))
    f1, i1 = _run(script, MC.NT, **kw)
    f2, i2 = _run(script, MC.NT, one_call=False, **kw)
    a, b = _driver_fields(hip, f1), _driver_fields(hip, f2)
    for k in STEP_SHAPES:
        assert bits_equal(a[k], b[k]), (script, name, k, first_bit_difference(a[k], b[k]))
    assert GS.same_steps(list(zip(i1.iters, i1.errs)), list(zip(i2.iters, i2.errs)))
    want = MC.driver_run(script, name)
    assert GS.same_steps(list(zip(i1.iters, i1.errs)), want.steps)
    for k in SS.FIVE:
        assert bits_equal(a[k], want.fields[k]), (script, name, k, first_bit_difference(a[k], want.fields[k]))
    mv = MC.mover(script, name)
    for info in (i1, i2):
        assert info.ctx.obstacle_motion() is None and info.ctx.obstacle() is None
        assert [m["t"] for m in info.motion] == [s * info.params.dt for s in range(1, MC.NT + 1)]
        for m, pose in zip(info.motion, mv.poses[1:]):
            assert all(np.array_equal(m[k], v) for k, v in zip(("R", "shift", "U", "omega", "centre"), pose))
            assert m["rebuilt"] == (name != "cylinder")
    from navierstokes3d_amd import solid as S
    f3, i3 = _run(script, MC.NT, **dict(kw, motion=S.rigid_motion(spacing=mv.d, **MC.keyword(script, name))))    # any callable of that shape
    c = _driver_fields(hip, f3)
    assert all(bits_equal(a[k], c[k]) for k in STEP_SHAPES)


@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_motion_none_is_no_keyword_and_diagnostics_use_the_moving_sums(hip, script, monkeypatch):
    """motion=None: the bits and the call trace of a run without the keyword.  With motion= call by call: set_solid_moving where
    set_solid stood; with diagnostics=True solid_momentum_moving where solid_momentum stood, the same fields, and a force"""
    from navierstokes3d_amd import kernels as K
    trace = []
    real = K.Context.call

    def spy(self, name, ref, *args):
        trace.append(name)
        return real(self, name, ref, *args)
    monkeypatch.setattr(K.Context, "call", spy)
    runs = {}
    base = dict(nx=24, mode="strict", niter_cap=MC.NITER, faithful=False, one_call=False, obstacle=MC.box())
    for key, extra in (("plain", dict()), ("none", dict(motion=None)), ("on", dict(motion=MC.keyword(script, "spin"))),
                       ("static_diag", dict(diagnostics=True)), ("diag", dict(motion=MC.keyword(script, "spin"), diagnostics=True))):
        del trace[:]
        f, info = _run(script, 2, **dict(base, **extra))
        runs[key] = (_driver_fields(hip, f), list(trace), info)
    plain, none, on, sdiag, diag = (runs[k] for k in ("plain", "none", "on", "static_diag", "diag"))
    assert plain[1] == none[1] and not hasattr(none[2], "motion") and "set_solid_moving" not in plain[1]
    for k in STEP_SHAPES:
        assert bits_equal(plain[0][k], none[0][k]), k
    assert [("set_solid" if n == "set_solid_moving" else n) for n in on[1]] == plain[1] and on[1].count("set_solid_moving") == plain[1].count("set_solid")
    assert not bits_equal(on[0]["Vx"], plain[0]["Vx"])
    assert diag[1].count("solid_momentum_moving") == 4 and "solid_momentum" not in diag[1] and sdiag[1].count("solid_momentum") == 4
    for k in STEP_SHAPES:
        assert bits_equal(diag[0][k], on[0][k]), k
    assert len(diag[2].diag) == 2 and any(abs(v) > 0 for v in diag[2].diag[-1].force)
    assert not np.array_equal(np.array(diag[2].diag[0].force), np.array(sdiag[2].diag[0].force))


def test_a_mask_does_not_translate(hip):
    from navierstokes3d_amd import lib as L
    with pytest.raises(L.Ns3dError, match="shift.*needs the obstacle as triangles"):
        _run("gpu", 1, nx=24, niter_cap=MC.NITER, faithful=False, obstacle=np.array(MC.box_mask()), motion=MC.keyword("gpu", "slide"))


# ---- stream order ------------------------------------------------------------------------------------------------------------------------
def _stream_cases(hip, dt):
    from navierstokes3d_amd import solid
    n = MC.GRID
    R, pivot, shift, d = _pose()
    tri = solid.box_mesh(*MC.BOX).reshape(-1)
    C0, Vx, Vy, Vz = fields(*n, ["c", "vx", "vy", "vz"], 21, NP[dt])
    arrays = [("C", C0, "field"), ("Vx", Vx, "field"), ("Vy", Vy, "field"), ("Vz", Vz, "field"), ("mask", np.asfortranarray(MC.box_mask()), "state")]
    m9 = MOTION[:6] + MC.BOX_CENTRE
    sset = SO.Case("set_solid_moving " + dt, arrays,
                   lambda hip, ctx, t: hip.set_solid_moving(t["C"], t["Vx"], t["Vy"], t["Vz"], t["mask"], m9, *SPACING, ctx=ctx))
    mom = SO.Case("solid_momentum_moving " + dt, arrays[1:],
                  lambda hip, ctx, t: hip.solid_momentum_moving(t["Vx"], t["Vy"], t["Vz"], t["mask"], m9, *SPACING, ctx=ctx), blocking=True)
    tr = SO.Case("mesh_transform", [("tri", tri, ("field", 15.0)), ("out", np.full(tri.shape, 777.0), ("field", 15.0))],
                 lambda hip, ctx, t: hip.mesh_transform(t["out"], t["tri"], R, pivot, shift, d, ctx=ctx))
    return {"set_solid_moving": sset, "solid_momentum_moving": mom, "mesh_transform": tr}


@pytest.mark.parametrize("kind", ["torch", "own", "masked"])
@pytest.mark.parametrize("name,dt", [("set_solid_moving", "f32"), ("solid_momentum_moving", "f64"), ("mesh_transform", "f64")])
def test_stream_order(hip, delay, name, dt, kind):
    """late input, early reader, on the three kinds of non-default stream"""
    from test_gpu_stream_order import run_case
    msgs = run_case(hip, _stream_cases(hip, dt)[name], kind, delay)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("kind", ["torch", "own", "masked"])
def test_stream_order_of_the_step_under_the_knob(hip, oracle, delay, kind):
    """two ns3d_time_step calls under ns3d_set_obstacle_motion with every array, the mask included, a late input and an early reader's
    output, against the null-stream bits — which are the statement's"""
    from test_gpu_stream_order import run_case
    host = dict(GS.host_state("f64"))
    mv = MC.mover("gpu", "cylinder")

    def call(hip, ctx, t):
        f = SimpleNamespace(**{k: v for k, v in t.items() if k != "mask"})
        _, sp = GS.step_params("gpu", MC.NITER)
        try:
            ctx.set_obstacle(t["mask"])
            out = []
            for s in (1, 2):                                # an even number: the step swaps X and X_o, the case reads them by name
                ctx.set_obstacle_motion(MR.motion9(mv.poses[s]))
                out.append(hip.time_step(f, sp, ctx=ctx))
            return out
        finally:
            ctx.set_obstacle_motion(None); ctx.set_obstacle(None)
    cs = SO.Case("time_step gpu under the motion knob", [(k, a, ("field", 1e-2)) for k, a in host.items()] +
                 [("mask", np.asfortranarray(mv.mask0), "state")], call, blocking=True)
    (want_r, want), _ = SO.expected(hip, cs)
    ref = MC.oracle_run("gpu", "f64", "cylinder", nt=2)
    assert GS.same_steps(want_r, ref.steps) and all(bits_equal(want[k], ref.fields[k]) for k in SS.ELEVEN)
    msgs = run_case(hip, cs, kind, delay)
    assert not msgs, "\n".join(msgs)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    """every NS3D_ERR_ARG of the three calls, with the outputs untouched"""
    from navierstokes3d_amd import lib as L
    lib = L.load()
    ctx = ctxs["strict"]
    n = (5, 4, 3)
    nx, ny, nz = n
    host = fields(*n, ["c", "vx", "vy", "vz"], 5, np.float64)
    dev = [hip.from_numpy(h) for h in host]
    dm = _up(np.full((nx + 1, ny + 1, nz + 1), 0x0F, dtype=np.uint8, order="F"))
    ptr = [C.c_void_p(t.data_ptr()) for t in dev] + [C.c_void_p(dm.data_ptr())]
    m9, o3 = (C.c_double * 9)(*MOTION), (C.c_int * 3)(*ORIGIN)
    D = lambda *v: [C.c_double(x) for x in v]
    nan, inf = float("nan"), float("inf")

    def bad9(q, v):
        a = list(MOTION)
        a[q] = v
        return (C.c_double * 9)(*a)
    mom, cnt = (C.c_double * 3)(7.0, 7.0, 7.0), (C.c_longlong * 3)(7, 7, 7)
    sets = [(ptr[:1] + [None] + ptr[2:], m9, SPACING, o3, n, "null"), (ptr[:2] + [None] + ptr[3:], m9, SPACING, o3, n, "null"),
            (ptr[:3] + [None] + ptr[4:], m9, SPACING, o3, n, "null"), (ptr[:4] + [None], m9, SPACING, o3, n, "null"),
            (ptr, None, SPACING, o3, n, "null motion")] + \
           [(ptr, bad9(q, v), SPACING, o3, n, "not finite") for q in range(9) for v in (nan, inf)] + \
           [(ptr, m9, SPACING[:q] + (v,) + SPACING[q + 1:], o3, n, "spacings") for q in range(3) for v in (nan, inf, 0.0, -0.1)] + \
           [(ptr, m9, SPACING, (C.c_int * 3)(*[(-1 if a == q else 0) for a in range(3)]), n, "origin") for q in range(3)] + \
           [(ptr, m9, SPACING, o3, g, "too small") for g in ((2, 4, 3), (5, 2, 3), (5, 4, 2))]
    for p5, m, d, o, g, msg in sets:
        assert lib.ns3d_set_solid_moving_f64(ctx.handle, *p5, m, *D(*d), o, *g) == L.NS3D_ERR_ARG, msg
        assert msg in L.last_error(), (msg, L.last_error())
        if p5[1] is not None and p5[2] is not None and p5[3] is not None and p5[4] is not None:
            assert lib.ns3d_solid_momentum_moving_f64(ctx.handle, *p5[1:], *g, None, None, mom, cnt, m, *D(*d), o) == L.NS3D_ERR_ARG, msg
            assert msg in L.last_error(), (msg, L.last_error())
    for a, b in ((None, cnt), (mom, None)):
        assert lib.ns3d_solid_momentum_moving_f64(ctx.handle, *ptr[1:], *n, None, None, a, b, m9, *D(*SPACING), o3) == L.NS3D_ERR_ARG
    assert lib.ns3d_set_solid_moving_f32(None, *ptr, m9, *D(*SPACING), o3, *n) == L.NS3D_ERR_ARG
    ctx.sync()
    for d, h in zip(dev, host):
        assert bits_equal(hip.to_numpy(d), h)
    assert list(mom) == [7.0] * 3 and list(cnt) == [7] * 3
    # ns3d_mesh_transform
    R, pivot, shift, d = _pose()
    tri = rnd(6, (4, 3, 3), np.float64, -3.0, 30.0).reshape(-1)
    src, out = torch.from_numpy(tri.copy()).cuda(), torch.full((36,), 777.0, dtype=torch.float64, device="cuda")
    A = lambda v: (C.c_double * len(np.ravel(v)))(*np.ravel(v))
    good = dict(out=C.c_void_p(out.data_ptr()), tri=C.c_void_p(src.data_ptr()), n=4, R=A(R), pivot=A(pivot), shift=A(shift), d=A(d))

    def tr(**kw):
        a = dict(good, **kw)
        return lib.ns3d_mesh_transform(ctx.handle, a["out"], a["tri"], C.c_longlong(a["n"]), a["R"], a["pivot"], a["shift"], a["d"])
    Rn, pn, sn = R.copy(), pivot.copy(), shift.copy()
    Rn[1, 2], pn[0], sn[2] = nan, inf, nan
    for kw in (dict(n=-1), dict(out=None), dict(tri=None), dict(R=None), dict(pivot=None), dict(shift=None), dict(d=None), dict(R=A(Rn)),
               dict(pivot=A(pn)), dict(shift=A(sn)), dict(d=A([0.1, 0.0, 0.1])), dict(d=A([0.1, 0.1, -1.0])), dict(d=A([nan, 0.1, 0.1])),
               dict(d=A([0.1, inf, 0.1]))):
        assert tr(**kw) == L.NS3D_ERR_ARG, kw
    assert lib.ns3d_mesh_transform(None, good["out"], good["tri"], 4, good["R"], good["pivot"], good["shift"], good["d"]) == L.NS3D_ERR_ARG
    assert tr(n=0, out=None, tri=None) == L.NS3D_OK
    ctx.sync()
    assert (out.cpu().numpy() == 777.0).all() and bits_equal(src.cpu().numpy(), tri)
    assert tr() == L.NS3D_OK
    ctx.sync()
    assert bits_equal(out.cpu().numpy(), MR.transform(tri, R, pivot, shift, d).reshape(-1))
