"""Knobs that include/ns3d.h promises "same results" for, held to that promise bit for bit (STRICT mode, np.array_equal):

  A  ns3d_reserve_cus / NS3D_RESERVE_CUS — the context launches on a CU-masked stream and the z-chunking of launch_sweep2 /
     launch_sweepN / k_pt_sweepD and the fit rule of k_pt_persist count the CUs that are left;
  B  ns3d_mgpu_set_interior_chunks / NS3D_SLAB_INTERIOR_CHUNKS — the interior sweep of a z-slab pass in up to 16 launches.

The wide, shallow grids of A2 are the ones on which the sweep's chunk count really changes with the reservation
(launch_sweep2: c = m·slots/tiles chunks capped at nk/8, slots = (CUs − reserved)·workgroups per CU): with 256 CUs and two
workgroups of the 64×16 tile per CU, 514×258×26 goes out as 171 tile columns × 3 chunks unreserved and × 2 chunks with half the
device reserved, 386×322×42 as 161 × 5 against × 3, 258×258×50 as 95 × 6 against × 5 (and its 64×24 four-level tiles as 70 × 2
against × 1 where one workgroup fits a CU)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_pt import _oracle_iters, _params
from util import fields, geometry

pytestmark = pytest.mark.gpu

BCS = [(0, True, 0.25), (1, False, 0.0)]
SMALL = (70, 21, 23)
WIDE = [(514, 258, 26), (386, 322, 42), (258, 258, 50)]


def _half():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count // 2


def _reservations():
    return (0, 8, 64, _half())


def _depths(dtype):
    return (1, 2, 3, 4) if dtype == np.float64 else (1, 2, 3, 4, 5)


def _iterate(hip, ctx, P0, D0, dR, p, n):
    """n PT iterations on fresh device copies of (P0, D0); the copies are complete before the context's stream — a masked one of its
    own when CUs are reserved — reads them, and everything is complete before the read-back"""
    import torch
    dP, dD = hip.clone(P0), hip.clone(D0)
    torch.cuda.synchronize()
    hip.pt_iterate(dP, dD, dR, p, n, ctx=ctx)
    torch.cuda.synchronize()
    return hip.to_numpy(dP), hip.to_numpy(dD)


def _solve(hip, ctx, P0, D0, dR, p, eps, niter, nchk):
    import torch
    dP, dD = hip.clone(P0), hip.clone(D0)
    torch.cuda.synchronize()
    it, errs = hip.pt_solve(dP, dD, dR, p, eps, niter, nchk, 0.36, 1000.0, ctx=ctx)
    torch.cuda.synchronize()
    return it, errs, hip.to_numpy(dP), hip.to_numpy(dD)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- A1: the contract of ns3d_reserve_cus ----------------------------------------------------------------------------
def test_reserve_cus_contract(hip, oracle):
    """Rounding to eights, read-back, refused arguments leave the state alone, 0 goes back to PyTorch's stream, and a change of
    the reservation drops the captured residual-check blocks (they hold the z-chunking of the CU count they were captured for)."""
    import torch
    from navierstokes3d_amd import lib as L
    nx, ny, nz = SMALL
    g = geometry(nx, ny, nz)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 311)
    rhs *= 1e-3
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    p = _params(hip, P0, g, 0, True, 0.25)
    Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
    _oracle_iters(oracle, Pr, d, rhs, g, 5, 0, True, 0.25)
    half = _half()
    ctx = hip.Context(0, "strict")
    lib, h = ctx.lib, ctx.handle
    reserved = lambda: int(lib.ns3d_reserved_cus(h))
    assert reserved() == 0
    for n, want in ((1, 8), (5, 8), (8, 8), (9, 16), (64, 64), (half, (half + 7) // 8 * 8)):
        s = ctx.reserve_cus(n)
        assert reserved() == want, (n, reserved())
        assert s.cuda_stream == int(lib.ns3d_get_stream(h)) and s.cuda_stream != torch.cuda.current_stream(0).cuda_stream
    ctx.reserve_cus(64)
    masked = int(lib.ns3d_get_stream(h))
    for bad in (-1, -8, half + 1, 10 * half):
        assert lib.ns3d_reserve_cus(h, bad) == L.NS3D_ERR_ARG, bad
        assert reserved() == 64 and int(lib.ns3d_get_stream(h)) == masked        # the previous state stays
    assert _same(_iterate(hip, ctx, P0, D0, dR, p, 5), (Pr, d))                   # … and still works
    s = ctx.reserve_cus(0)
    assert reserved() == 0 and s.cuda_stream == torch.cuda.current_stream(0).cuda_stream
    assert int(lib.ns3d_get_stream(h) or 0) == torch.cuda.current_stream(0).cuda_stream      # (a null handle reads back as None)
    dP, dD = hip.clone(P0), hip.clone(D0)                                         # PyTorch's stream again: ordered with the
    hip.pt_iterate(dP, dD, dR, p, 5, ctx=ctx)                                     # copies without any synchronisation
    assert _same((hip.to_numpy(dP), hip.to_numpy(dD)), (Pr, d))
    # captured blocks: dropped by every change of the reservation, captured again by the next solve, same bits
    ctx.set_persist_mode(0)
    ctx.set_graph_mode(1)
    graphs = lambda: int(lib.ns3d_cached_graphs(h))
    first = _solve(hip, ctx, P0, D0, dR, p, -1.0, 45, 7)
    assert graphs() > 0 and first[0] == 45 and len(first[1]) == 6
    for n in (64, half, 0, 8):
        ctx.reserve_cus(n)
        assert graphs() == 0, n
        again = _solve(hip, ctx, P0, D0, dR, p, -1.0, 45, 7)
        assert graphs() > 0, n
        assert again[0] == first[0] and again[1] == first[1] and _same(again[2:], first[2:]), n
    ctx.close()


# ---- A2: pt_iterate with pinned depths ---------------------------------------------------------------------------------
def _pinned_depths_against_the_oracle(hip, oracle, grid, bc, dtype, counts):
    nx, ny, nz = grid
    g = geometry(*grid)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 313, dtype)
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    p = _params(hip, P0, g, *bc)
    ref = {}
    for n in counts:
        Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
        _oracle_iters(oracle, Pr, d, rhs, g, n, *bc)
        ref[n] = (Pr, d)
    ctx = hip.Context(0, "strict")
    ctx.set_autotune(False)
    ctx.set_persist_mode(0)
    for res in _reservations():
        ctx.reserve_cus(res)
        for depth in _depths(dtype):
            ctx.set_pt_depth(depth)
            for n in counts:
                got = _iterate(hip, ctx, P0, D0, dR, p, n)
                # reservation 0 equals the oracle's loop, and every other reservation equals reservation 0
                assert np.array_equal(got[1], ref[n][1]), "dPrdτ: %d CUs reserved, depth %d, n %d" % (res, depth, n)
                assert np.array_equal(got[0], ref[n][0]), "Pr: %d CUs reserved, depth %d, n %d" % (res, depth, n)
                if depth >= 2:
                    assert ctx.last_pt_depth() >= 2
    assert np.array_equal(hip.to_numpy(dR), rhs)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bc", BCS)
def test_pt_iterate_on_a_reserved_context_small_grid(hip, oracle, bc, dtype):
    """70×21×23, every pinned depth, 13 and 4 iterations (passes of 4+4+3+2, 3+3+3+2+2, …; 4 = 2+2 at depth 3), reservations 0, 8,
    64 and half the device."""
    _pinned_depths_against_the_oracle(hip, oracle, SMALL, bc, dtype, (13, 4))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bc,n", [(BCS[0], 13), (BCS[1], 4)])
@pytest.mark.parametrize("grid", WIDE)
def test_pt_iterate_on_a_reserved_context_wide_grids(hip, oracle, grid, bc, n, dtype):
    """The grids whose chunk count depends on the reservation (module docstring): few planes, many tile columns."""
    _pinned_depths_against_the_oracle(hip, oracle, grid, bc, dtype, (n,))


@pytest.mark.parametrize("depth", [0, 3])
def test_pt_iterate_on_a_reserved_context_with_autotune(hip, oracle, depth):
    """Autotune on: the first launch per (grid, reservation) times the tile shapes on the masked stream and keeps a winner of its
    own — free choice of the depth (3.2 M cells: deeper passes are timed) and a pinned one."""
    grid, bc, n = WIDE[0], BCS[0], 13
    nx, ny, nz = grid
    g = geometry(*grid)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 313)
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    p = _params(hip, P0, g, *bc)
    Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
    _oracle_iters(oracle, Pr, d, rhs, g, n, *bc)
    ctx = hip.Context(0, "strict")
    ctx.set_persist_mode(0)
    ctx.set_pt_depth(depth)
    for res in (0, _half(), 64):
        ctx.reserve_cus(res)
        got = _iterate(hip, ctx, P0, D0, dR, p, n)
        assert _same(got, (Pr, d)), "%d CUs reserved" % res
        assert _same(_iterate(hip, ctx, P0, D0, dR, p, n), got)                   # the remembered choice
    ctx.close()


# ---- A3: pt_solve on the masked stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("grid", [SMALL, (63, 38, 38)])
def test_pt_solve_on_a_reserved_context(hip, grid, graph, dtype):
    """Launch by launch and as replayed HIP graphs, a solve that stops early and one that runs out its budget (eps < 0): iteration
    count, residual history and both fields of a reserved context equal the unreserved context's."""
    nx, ny, nz = grid
    g = geometry(*grid)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 317, dtype)
    Pr0 *= dtype(1e-3); d0 *= dtype(1e-3); rhs *= dtype(1e-6)
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    p = _params(hip, P0, g, 0, True, 0.0)
    solves = ((2.0e-3, 400, 19), (-1.0, 45, 7))
    plain = hip.Context(0, "strict")
    ctx = hip.Context(0, "strict")
    for c in (plain, ctx):
        c.set_persist_mode(0)
        c.set_graph_mode(graph)
    want = [_solve(hip, plain, P0, D0, dR, p, *s) for s in solves]
    it, errs = want[0][:2]
    assert 19 < it < 400 and len(errs) == it // 19, (it, errs)                    # a real early exit
    assert want[1][0] == 45 and len(want[1][1]) == 6
    for res in (64, _half()):
        ctx.reserve_cus(res)
        for s, w in zip(solves, want):
            got = _solve(hip, ctx, P0, D0, dR, p, *s)
            assert got[0] == w[0] and got[1] == w[1], (res, s, got[:2], w[:2])
            assert _same(got[2:], w[2:]), (res, s)
        assert (int(ctx.lib.ns3d_cached_graphs(ctx.handle)) > 0) == bool(graph)
    plain.close(); ctx.close()


# ---- A4: k_pt_persist under a CU mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("grid", [(63, 38, 38), (40, 24, 24)])
def test_pt_persist_on_a_reserved_context(hip, grid, dtype):
    """The cooperative form sizes its grid for the CUs the mask leaves: 63×38×38 is 324 workgroups of 64×2×2 — resident together on
    256 CUs and on 192, not on 128, where the 64×4×2 shape (162) takes over.  No hand-over may expire (conftest arms
    NS3D_COOP_CHECK: an expired one fails the call), and the bits are those of the launch-per-iteration path."""
    nx, ny, nz = grid
    g = geometry(*grid)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 331, dtype)
    rhs *= dtype(1e-3)
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    off = hip.Context(0, "strict"); off.set_persist_mode(0); off.set_graph_mode(0)
    on = hip.Context(0, "strict"); on.set_persist_mode(1)
    for bc in BCS:
        p = _params(hip, P0, g, *bc)
        want_it = _iterate(hip, off, P0, D0, dR, p, 9)
        want_solve = _solve(hip, off, P0, D0, dR, p, 1e-30, 45, 7)
        for res in (64, _half()):
            on.reserve_cus(res)
            assert _same(_iterate(hip, on, P0, D0, dR, p, 9), want_it), (bc, res)
            got = _solve(hip, on, P0, D0, dR, p, 1e-30, 45, 7)
            assert got[0] == want_solve[0] and got[1] == want_solve[1] and _same(got[2:], want_solve[2:]), (bc, res)
            assert on.persist_faults() == 0, (bc, res)
    off.close(); on.close()


# ---- A5: a whole time step ----------------------------------------------------------------------------------------------
def _two_steps(hip, script, reserve, advection="reference"):
    """two ns3d_time_step calls on 24×15×15 from the driver's own initial state, on a context with `reserve` CUs left out;
    advection="maccormack": the knob on and faithful = 0"""
    import torch
    from navierstokes3d_amd import driver as Dr, lib as L
    from navierstokes3d_amd.params import gpu_params, multi_params
    p = multi_params(24) if script == "multi" else gpu_params(24)
    nx, ny, nz = p.nx, p.ny, p.nz
    assert (nx, ny, nz) == (24, 15, 15)
    f = Dr._alloc(nx, ny, nz, torch.float64, torch.device("cuda", 0))
    ctx = hip.Context(0, "strict", async_=True)
    ctx.reserve_cus(reserve)
    ctx.set_advection(advection)
    niter = 200 if (script, advection) == ("gpu", "maccormack") else p.niter        # test_gpu_footprint.mc_niter says why
    common = dict(nx=nx, ny=ny, nz=nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp, dx=p.dx, dy=p.dy, dz=p.dz,
                  eps=p.eps, niter=niter, nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc, a2=p.a2, b2=p.b2, ox=p.ox, oy=p.oy,
                  sinb=p.sinb, cosb=p.cosb, lx=p.lx, ly=p.ly, lz=p.lz, faithful=0 if advection == "maccormack" else 1, pressure=0,
                  write_stress=0)
    if script == "multi":
        f.Vy[0, :, :] = p.vin                                                                        # multi.jl:369
        torch.cuda.synchronize()
        hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz,
                         p.dx, p.dy, p.dz, ctx=ctx)                                                 # multi.jl:372
        sp = L.StepParams(script=L.NS3D_BC_MULTI, xco_g=p.xco_g, yco_g=p.yco_g, zco_g=p.zco_g, owns_inlet=int(bool(p.owns_inlet)),
                          owns_outlet=int(bool(p.owns_outlet)), vin=p.vin, **common)
    else:
        Vx0, Pr0 = Dr.gpu_initial_fields(p)                                                          # gpu.jl:85-88
        f.Vx, f.Pr = hip.from_numpy(Vx0), hip.from_numpy(Pr0)
        sp = L.StepParams(script=L.NS3D_BC_GPU, xco_g=0.0, yco_g=0.0, zco_g=0.0, owns_inlet=0, owns_outlet=0, vin=0.0, **common)
    torch.cuda.synchronize()
    out = []
    for step in (1, 2):
        sp.write_stress = 1 if step == 2 else 0
        out.append(hip.time_step(f, sp, ctx=ctx))
    torch.cuda.synchronize()
    names = ("C", "Pr", "dPrdtau", "divV", "Vx", "Vy", "Vz", "Vx_o", "Vy_o", "Vz_o", "C_o", "txx", "tyy", "tzz", "txy", "txz", "tyz")
    host = SimpleNamespace(steps=out, fields={n: hip.to_numpy(getattr(f, n)) for n in names})
    ctx.close()
    return host


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_on_a_reserved_context(hip, script, advection="reference"):
    """ns3d_time_step — predictor, PT solve, correction, advection (the reference's or the MacCormack scheme, whose two stages meet
    in the context's hat scratch), the boundary rules — 24×15×15, two steps, both scripts: iteration counts, residual histories and
    all seventeen arrays of a reserved context equal the unreserved context's."""
    want = _two_steps(hip, script, 0, advection)
    assert all(it > 0 and len(errs) > 0 for it, errs in want.steps)
    assert np.abs(want.fields["Vx"]).max() > 0 and np.abs(want.fields["Pr"]).max() > 0 and np.abs(want.fields["txx"]).max() > 0
    for res in (64, _half()):
        got = _two_steps(hip, script, res, advection)
        assert len(got.steps) == len(want.steps)
        for (it, errs), (wit, werrs) in zip(got.steps, want.steps):
            assert it == wit and np.array_equal(errs, werrs, equal_nan=True), (res, it, wit)
        for n, w in want.fields.items():
            assert np.array_equal(got.fields[n], w, equal_nan=True), (res, n)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_on_a_reserved_context_maccormack(hip, script):
    """the test above over the other value of its `advection` parameter (a test of its own: the existing cases keep their names)"""
    test_time_step_on_a_reserved_context(hip, script, "maccormack")


# ---- A6: the environment preset ------------------------------------------------------------------------------------------
def test_reserve_cus_environment_preset(hip, oracle, monkeypatch):
    """NS3D_RESERVE_CUS presets the reservation inside ns3d_create.  (kernels.Context hands the context PyTorch's stream right
    after creating it, so the preset shows through the C ABI only.)"""
    import torch
    from navierstokes3d_amd import lib as L
    nx, ny, nz = SMALL
    g = geometry(nx, ny, nz)
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 337)
    P0, D0, dR = hip.from_numpy(Pr0), hip.from_numpy(d0), hip.from_numpy(rhs)
    p = _params(hip, P0, g, 0, True, 0.25)
    plain = hip.Context(0, "strict")
    want = _iterate(hip, plain, P0, D0, dR, p, 7)
    plain.close()
    lib = L.load()
    monkeypatch.setenv("NS3D_RESERVE_CUS", "64")
    h = lib.ns3d_create(0, L.NS3D_STRICT)
    monkeypatch.delenv("NS3D_RESERVE_CUS")
    assert h
    try:
        assert lib.ns3d_reserved_cus(h) == 64
        assert int(lib.ns3d_get_stream(h) or 0) not in (0, torch.cuda.current_stream(0).cuda_stream)
        dP, dD = hip.clone(P0), hip.clone(D0)
        torch.cuda.synchronize()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert lib.ns3d_pt_iterate_f64(h, ptr(dP), ptr(dD), ptr(dR), C.byref(p), 7) == L.NS3D_OK, L.last_error()
        assert lib.ns3d_sync(h) == L.NS3D_OK
        torch.cuda.synchronize()
        assert _same((hip.to_numpy(dP), hip.to_numpy(dD)), want)
    finally:
        lib.ns3d_destroy(h)
    h = lib.ns3d_create(0, L.NS3D_STRICT)                  # without the variable: nothing reserved
    assert h and lib.ns3d_reserved_cus(h) == 0
    lib.ns3d_destroy(h)


# ---- B: interior chunks on z-slab virtual ranks ----------------------------------------------------------------------------
CHUNKS = (1, 2, 3, 4, 16)
XY = {"a": (40, 21), "b": (70, 12)}
# (P, nx×ny, local nz, set_temporal depth, element type, a compute stream per rank).  With G = depth − 1 ghost planes the interior of
# a pass is nz − G − 3 planes on an end rank and nz − 2G − 4 on a middle one (deep_pass sweeps the G + 1 planes next to a seam apart),
# and it is cut only from 8·chunks planes on: local nz 12 (at most 9) stays one launch for every chunk count, 21 (18 … 11) takes two
# chunks on some ranks and depths, 39 and 40 (37 … 29) take two and three everywhere and four except on a middle rank at the deeper
# passes — lengths that the chunk count divides and does not divide; 16 chunks never apply (128 planes).  Depths 3 and 4 meet every
# chunk count in every row.
SLAB_CASES = [
    (2, "a", 12, 1, np.float64, False), (3, "b", 12, 2, np.float32, True), (2, "b", 12, 3, np.float64, True), (3, "a", 12, 4, np.float32, False),
    (3, "a", 21, 1, np.float32, True), (2, "b", 21, 2, np.float64, False), (3, "b", 21, 3, np.float64, False), (2, "a", 21, 4, np.float32, True),
    (2, "b", 39, 1, np.float32, False), (3, "a", 39, 2, np.float64, True), (2, "a", 39, 3, np.float32, False), (3, "b", 39, 4, np.float64, True),
    (3, "b", 40, 1, np.float64, True), (2, "a", 40, 2, np.float32, False), (3, "a", 40, 3, np.float64, True), (2, "b", 40, 4, np.float32, False),
    (3, "b", 39, 3, np.float64, True), (2, "a", 39, 4, np.float64, False), (2, "b", 40, 3, np.float32, True), (3, "a", 40, 4, np.float32, False),
]


def _global_iterate(hip, Pg, Dg, Rg, g, n_iters, bc):
    import torch
    ctx = hip.Context(0, "strict")
    dP, dD = hip.from_numpy(Pg), hip.from_numpy(Dg)
    p = hip.pt_params(dP, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, *bc)
    hip.pt_iterate(dP, dD, hip.from_numpy(Rg), p, n_iters, ctx=ctx)
    torch.cuda.synchronize()
    out = hip.to_numpy(dP), hip.to_numpy(dD)
    ctx.close()
    return out


def _mg(P, nx, ny, nz, own):
    import torch
    from navierstokes3d_amd.mgpu import MultiGpu
    torch.cuda.synchronize()            # uploads made on PyTorch's stream are complete before any rank stream reads them
    return MultiGpu.create([0] * P, nx, ny, nz, "strict", own_streams=own)


def _cuts(hip, Pg, Dg, Rg, P, nz):
    cut = lambda A, r, n: hip.from_numpy(A[:, :, r * (nz - 2):r * (nz - 2) + n])
    return ([cut(Pg, r, nz) for r in range(P)], [cut(Dg, r, nz - 2) for r in range(P)], [cut(Rg, r, nz) for r in range(P)])


def _slab_run(hip, mg, Pg, Dg, Rg, g, bc, P, nz, depth, n_iters):
    """load / plan / iterate / store of the cuts of the global fields; returns the ranks' stored (Pr, dPrdτ) on the host"""
    import torch
    Pr, D, R = _cuts(hip, Pg, Dg, Rg, P, nz)
    torch.cuda.synchronize()
    p = hip.pt_params(Pr[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, *bc)
    mg.slab_load(Pr, D, R, p)
    assert mg.slab_plan() == depth
    mg.slab_iterate(n_iters)
    mg.slab_store(Pr, D)
    mg.sync()
    torch.cuda.synchronize()
    return [hip.to_numpy(t) for t in Pr], [hip.to_numpy(t) for t in D]


def _assert_slabs_equal_global(got, Pref, Dref, P, nz, what):
    for r in range(P):
        lo = r * (nz - 2)
        assert np.array_equal(got[0][r], Pref[:, :, lo:lo + nz]), "Pr of rank %d: %s" % (r, what)          # seam planes included
        assert np.array_equal(got[1][r], Dref[:, :, lo:lo + nz - 2]), "dPrdτ of rank %d: %s" % (r, what)


def _slab_setup(mg, depth):
    mg.set_temporal(depth)
    if depth >= 3:                      # forced through the ranks' contexts: the planner would only choose it on much larger grids
        for c in mg.contexts:
            c.set_pt_depth(depth)


@pytest.mark.parametrize("P,xy,nz,depth,dtype,own", SLAB_CASES)
def test_interior_chunks_leave_the_global_solve(hip, P, xy, nz, depth, dtype, own):
    """Every rank's stored planes — halo planes at the seams included — after 7 and 10 iterations with the interior sweep of each
    pass in 1, 2, 3, 4 and 16 launches: the planes of ns3d_pt_iterate on the global grid, bit for bit."""
    nx, ny = XY[xy]
    nz_g = P * (nz - 2) + 2
    g = geometry(nx, ny, nz_g)
    Pg, Dg, Rg = fields(nx, ny, nz_g, ["c", "i", "c"], 211, dtype)
    bc = (True, 0.25, 0.0)
    mg = _mg(P, nx, ny, nz, own)
    _slab_setup(mg, depth)
    for n_iters in (7, 10):
        Pref, Dref = _global_iterate(hip, Pg, Dg, Rg, g, n_iters, bc)
        for chunks in CHUNKS:
            mg.set_interior_chunks(chunks)
            got = _slab_run(hip, mg, Pg, Dg, Rg, g, bc, P, nz, depth, n_iters)
            _assert_slabs_equal_global(got, Pref, Dref, P, nz, "%d chunks, %d iterations" % (chunks, n_iters))
    mg.close()


@pytest.mark.parametrize("through", ["contexts", "c-entry"])
def test_interior_chunks_with_reserved_cus(hip, through):
    """Four chunks on CU-masked compute streams: MultiGpu.reserve_cus (context by context) and ns3d_mgpu_reserve_cus (one call)."""
    from navierstokes3d_amd import lib as L
    P, (nx, ny), nz, depth, n_iters = 2, XY["a"], 40, 3, 10
    nz_g = P * (nz - 2) + 2
    g = geometry(nx, ny, nz_g)
    Pg, Dg, Rg = fields(nx, ny, nz_g, ["c", "i", "c"], 223)
    bc = (True, 0.25, 0.0)
    Pref, Dref = _global_iterate(hip, Pg, Dg, Rg, g, n_iters, bc)
    mg = _mg(P, nx, ny, nz, True)        # a pinned compute stream per rank: the masked streams stay the ranks' streams
    _slab_setup(mg, depth)
    if through == "contexts":
        streams = mg.reserve_cus(64)
        assert len({s.cuda_stream for s in streams}) == P
    else:
        assert mg.lib.ns3d_mgpu_reserve_cus(mg.handle, 64) == L.NS3D_OK
        assert mg.lib.ns3d_mgpu_reserve_cus(mg.handle, -1) == L.NS3D_ERR_ARG
    mg.set_interior_chunks(4)
    masked = [int(mg.lib.ns3d_get_stream(c.handle)) for c in mg.contexts]
    got = _slab_run(hip, mg, Pg, Dg, Rg, g, bc, P, nz, depth, n_iters)
    _assert_slabs_equal_global(got, Pref, Dref, P, nz, "64 CUs reserved, 4 chunks")
    for c, s in zip(mg.contexts, masked):                                          # the sweeps did run under the mask
        assert mg.lib.ns3d_reserved_cus(c.handle) == 64 and int(mg.lib.ns3d_get_stream(c.handle)) == s
    mg.close()


@pytest.mark.parametrize("own", [False, True])
def test_pt_solve_slab_with_interior_chunks(hip, own):
    """ns3d_pt_solve_slab with three chunks: iteration count, residual history and stored planes of the one-chunk solve."""
    import torch
    P, (nx, ny), nz = 2, XY["a"], 40
    nz_g = P * (nz - 2) + 2
    g = geometry(nx, ny, nz_g)
    Pg, Dg, Rg = fields(nx, ny, nz_g, ["c", "i", "c"], 77)
    Pg *= 1e-3; Dg *= 1e-3; Rg *= 1e-6
    res = []
    mg = _mg(P, nx, ny, nz, own)
    for chunks in (1, 3):
        mg.set_interior_chunks(chunks)
        Pr, D, R = _cuts(hip, Pg, Dg, Rg, P, nz)
        torch.cuda.synchronize()
        p = hip.pt_params(Pr[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, True, 0.0, 0.0)
        it, errs = mg.pt_solve_slab(Pr, D, R, p, 1.0e-4, 400, 19, 0.36, 1000.0)
        mg.sync()
        torch.cuda.synchronize()
        res.append((it, errs, [hip.to_numpy(t) for t in Pr], [hip.to_numpy(t) for t in D]))
    mg.close()
    one, three = res
    assert one[0] >= 19 and len(one[1]) == one[0] // 19
    assert three[0] == one[0] and three[1] == one[1]
    assert _same(three[2], one[2]) and _same(three[3], one[3])


def test_interior_chunks_environment_preset_and_argument_errors(hip, monkeypatch):
    """NS3D_SLAB_INTERIOR_CHUNKS=4 before ns3d_mgpu_create: the same bits; 0 and 17 chunks: NS3D_ERR_ARG, the setting stays."""
    from navierstokes3d_amd import lib as L
    P, (nx, ny), nz, depth, n_iters = 3, XY["b"], 40, 2, 7
    nz_g = P * (nz - 2) + 2
    g = geometry(nx, ny, nz_g)
    Pg, Dg, Rg = fields(nx, ny, nz_g, ["c", "i", "c"], 227)
    bc = (True, 0.25, 0.0)
    Pref, Dref = _global_iterate(hip, Pg, Dg, Rg, g, n_iters, bc)
    monkeypatch.setenv("NS3D_SLAB_INTERIOR_CHUNKS", "4")
    mg = _mg(P, nx, ny, nz, False)
    monkeypatch.delenv("NS3D_SLAB_INTERIOR_CHUNKS")
    _slab_setup(mg, depth)
    for bad in (0, 17, -1):
        assert mg.lib.ns3d_mgpu_set_interior_chunks(mg.handle, bad) == L.NS3D_ERR_ARG, bad
    with pytest.raises(L.Ns3dError):
        mg.set_interior_chunks(17)
    got = _slab_run(hip, mg, Pg, Dg, Rg, g, bc, P, nz, depth, n_iters)
    _assert_slabs_equal_global(got, Pref, Dref, P, nz, "NS3D_SLAB_INTERIOR_CHUNKS=4")
    assert mg.lib.ns3d_mgpu_set_interior_chunks(mg.handle, 16) == L.NS3D_OK
    mg.close()
