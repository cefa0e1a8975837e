"""Shape 29 of the N-iteration sweep (variant 29xx): k_pt_sweepN's PACE instance, whose workgroups of one XCD group meet every pace_z
z-steps at a bounded wait.  The wait is a hint: results are those of as many single sweeps, bit for bit, whether the workgroups wait,
expire or are not paced at all; and pacing is off (ns3d_last_pt_pace == 0) wherever the workgroups of a launch are not resident
together or do not march the same planes.

Grids: 70×30×40 and 130×50×40 give 2×2 and 3×3 tiles of the 64×24 shape (stride 58×18 at four levels) and 40 planes: a bulk loop of
eight trips, so pace_z = 8 holds three rendezvous per launch and pace_z = 16 one.  The reference is the one-thread-per-cell sweep
(variant 100, k_pt_sweep_naive), computed once per (grid, element type, boundary set, levels)."""
import functools

import numpy as np
import pytest

from test_gpu_pt import _params
from util import fields, geometry

pytestmark = pytest.mark.gpu

GRIDS = [(70, 30, 40), (130, 50, 40)]
BCS = [(0, True, 0.25), (1, False, 0.0)]


@functools.lru_cache(maxsize=None)
def _case(grid, dtype, bc, nlev):
    """inputs and the result of nlev single sweeps of variant 100 (host arrays; never modified afterwards)"""
    import torch
    from navierstokes3d_amd import kernels as hip
    nx, ny, nz = grid
    g = geometry(*grid)
    P0, D0, R = fields(nx, ny, nz, ["c", "i", "c"], 29, np.dtype(dtype).type)
    ctx = hip.Context(0, "strict")
    ctx.set_pt_variant(100)
    dP, dQ, dD, dR = hip.from_numpy(P0), hip.from_numpy(P0), hip.from_numpy(D0), hip.from_numpy(R)
    p = _params(hip, dP, g, *bc)
    for _ in range(nlev):
        hip.pt_sweep(dP, dQ, dD, dR, p, 1, nz - 1, ctx=ctx)
        dP, dQ = dQ, dP
    torch.cuda.synchronize()
    ref = (hip.to_numpy(dP), hip.to_numpy(dD))
    ctx.close()
    for a in (P0, D0, R) + ref:
        a.setflags(write=False)
    return g, P0, D0, R, ref


def _pass(hip, ctx, nlev, P0, D0, R, g, bc, launches=1, stream=None):
    """`launches` passes of nlev iterations from (P0, D0) on ctx; returns the fields of the last one and the pace_z it used"""
    import torch
    dP, dD, dR = hip.from_numpy(P0), hip.from_numpy(D0), hip.from_numpy(R)
    dQ, dE = hip.from_numpy(np.full_like(P0, 555.0)), hip.from_numpy(np.full_like(D0, 444.0))
    p = _params(hip, dP, g, *bc)
    torch.cuda.synchronize()
    for _ in range(launches):
        hip.pt_sweepn(nlev, dP, dQ, dD, dE, dR, p, ctx=ctx)
    torch.cuda.synchronize()
    return hip.to_numpy(dQ), hip.to_numpy(dE), ctx.last_pt_pace()


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), "dPrdτ differs: %s" % (what,)
    assert np.array_equal(got[0], ref[0]), "Pr differs: %s" % (what,)


@pytest.mark.parametrize("nlev", [4, 3])
@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("grid", GRIDS)
def test_paced_pass_equals_single_sweeps(hip, grid, dtype, bc, nlev):
    """pace_z = 0 (not paced), 8 and 16: the same bits as nlev single sweeps, and the launch reports the pace_z it used"""
    g, P0, D0, R, ref = _case(grid, dtype, bc, nlev)
    ctx = hip.Context(0, "strict")
    ctx.set_ptn_variant(2900 + grid[2] - 2)         # one z-chunk of all 38 planes (the built-in choice cuts three levels in two)
    for pace_z in (0, 8, 16):
        ctx.set_pt_pace(pace_z)
        P, D, used = _pass(hip, ctx, nlev, P0, D0, R, g, bc)
        assert used == pace_z
        _same((P, D), ref, (grid, dtype, bc, nlev, pace_z))
    ctx.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_fifty_launches_on_one_context(hip, grid):
    """the counters only grow: launch n waits for n × (workgroups of its group), fifty times over, then with another pace_z and on
    the other grid's geometry through the same context"""
    g, P0, D0, R, ref = _case(grid, "float64", BCS[0], 4)
    ctx = hip.Context(0, "strict")
    ctx.set_ptn_variant(2900)
    ctx.set_pt_pace(8)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0], launches=50)
    assert used == 8
    _same((P, D), ref, (grid, "50 launches"))
    ctx.set_pt_pace(16)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0], launches=3)
    assert used == 16
    _same((P, D), ref, (grid, "pace_z changed"))
    other = GRIDS[1] if grid == GRIDS[0] else GRIDS[0]
    g2, P2, D2, R2, ref2 = _case(other, "float64", BCS[0], 4)
    P, D, used = _pass(hip, ctx, 4, P2, D2, R2, g2, BCS[0], launches=2)
    assert used == 16
    _same((P, D), ref2, (other, "geometry changed"))
    ctx.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("grid", GRIDS)
def test_expired_waits_are_ordinary_operation(hip, grid, dtype):
    """The target raised by one arrival nobody makes and the bound at its minimum: every wait of every workgroup expires after one
    poll, the pass returns and the results are the same.  A bounded wait: nothing in it can hang."""
    g, P0, D0, R, ref = _case(grid, dtype, BCS[0], 4)
    ctx = hip.Context(0, "strict")
    ctx.set_ptn_variant(2900)
    ctx.set_pt_pace(8)
    ctx.set_pt_pace_test(1, 1)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0], launches=3)
    assert used == 8
    _same((P, D), ref, (grid, dtype, "expired"))
    ctx.set_pt_pace_test(0, 0)                      # back to real targets and the default bound, on the same counters
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0], launches=2)
    assert used == 8
    _same((P, D), ref, (grid, dtype, "after expiry"))
    ctx.close()


def test_not_paced_in_z_chunks_and_under_the_gate(hip):
    """several z-chunks per tile column (variant 2907: chunks of seven planes) and, with the automatic setting, a grid below the
    planner's gate for deep passes: not paced, same results; the explicit setting on the same grid is"""
    grid = GRIDS[1]
    g, P0, D0, R, ref = _case(grid, "float64", BCS[0], 4)
    ctx = hip.Context(0, "strict")
    ctx.set_pt_pace(8)
    ctx.set_ptn_variant(2907)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert used == 0
    _same((P, D), ref, "z-chunks")
    ctx.set_ptn_variant(2900)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert used == 8
    ctx.set_pt_pace(-1)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert used == 0
    _same((P, D), ref, "under the gate")
    ctx.set_ptn_variant(2800)                       # a shape without the switch reports 0 whatever the setting
    ctx.set_pt_pace(8)
    P, D, used = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert used == 0
    _same((P, D), ref, "shape 28")
    ctx.close()


def test_not_paced_when_reserved_cus_leave_fewer_slots_than_tiles(hip):
    """2 × (CUs/4 + 1) tiles: one round on the whole device (paced), more than the half of it that a context with half the compute
    units reserved may count on (not paced).  Same results either way and as shape 28."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nty = cus // 4 + 1
    grid = (124, 8 + 18 * nty - 9, 24)
    nx, ny, nz = grid
    assert (nx - 8 + 57) // 58 == 2 and (ny - 8 + 17) // 18 == nty
    g = geometry(*grid)
    P0, D0, R = fields(nx, ny, nz, ["c", "i", "c"], 31)
    ctx = hip.Context(0, "strict")
    ctx.set_ptn_variant(2800)
    ref = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert ref[2] == 0
    ctx.set_ptn_variant(2900)
    ctx.set_pt_pace(8)
    got = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert got[2] == 8
    _same(got, ref, "whole device")
    s = ctx.reserve_cus(cus // 2)
    with torch.cuda.stream(s):
        got = _pass(hip, ctx, 4, P0, D0, R, g, BCS[0])
    assert got[2] == 0
    _same(got, ref, "half the device reserved")
    ctx.reserve_cus(0)
    ctx.close()


def test_not_paced_in_tile_windows(hip, monkeypatch):
    """The shell-first order of a Cartesian box pass issues the sweep as sub-rectangles of the tile grid (ns3d_tile_window): those
    launches are not paced; the same boxes swept whole are.  Same iteration count, error history and fields either way."""
    from navierstokes3d_amd.mgpu import MultiGpu
    from oracle.driver_ref import cart_coords
    dims, n = (2, 2, 1), (130, 70, 34)
    N = tuple(dims[d] * (n[d] - 2) + 2 for d in range(3))
    g = geometry(*N)
    g["dtau"] = 0.8 / np.sqrt(1.0 / g["dx"] ** 2 + 1.0 / g["dy"] ** 2 + 1.0 / g["dz"] ** 2)
    Pg, Dg, Rg = fields(*N, ["c", "i", "c"], 17)
    Pg *= 1e-3; Dg *= 1e-3; Rg *= 1e-6
    eps, niter, nchk, mul, div = -1.0, 18, 9, 0.36, 1000.0          # blocks of 9 = 4 + 4 + 1

    def cut(A, r, shrink):
        c = cart_coords(r, dims)
        return np.asfortranarray(A[tuple(slice(c[d] * (n[d] - 2), c[d] * (n[d] - 2) + n[d] - shrink) for d in range(3))])

    out = {}
    for variant, pace_z, overlap in ((2800, 0, "0"), (2900, 8, "0"), (2900, 8, "1")):
        monkeypatch.setenv("NS3D_CART_DEEP", "1")
        monkeypatch.setenv("NS3D_BOX_OVERLAP", overlap)
        mg = MultiGpu.create([0] * 4, *n, "strict", dims=dims, own_streams=True)
        mg.set_temporal(4)
        for c in mg.contexts:
            c.set_pt_depth(4); c.set_ptn_variant(variant); c.set_pt_pace(pace_z)
        Pr = [hip.from_numpy(cut(Pg, r, 0)) for r in range(4)]
        D = [hip.from_numpy(cut(Dg, r, 2)) for r in range(4)]
        R = [hip.from_numpy(cut(Rg, r, 0)) for r in range(4)]
        p = hip.pt_params(Pr[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, True, 0.25, 0.0)
        it, errs = mg.pt_solve_slab(Pr, D, R, p, eps, niter, nchk, mul, div)
        mg.sync()
        used = [c.last_pt_pace() for c in mg.contexts]
        out[(variant, overlap)] = (it, errs, [hip.to_numpy(a) for a in Pr], [hip.to_numpy(a) for a in D], used)
        mg.close()
    ref = out[(2800, "0")]
    assert ref[4] == [0] * 4
    assert out[(2900, "0")][4] == [8] * 4, "whole boxes are paced"
    assert out[(2900, "1")][4] == [0] * 4, "tile windows are not"
    for key in ((2900, "0"), (2900, "1")):
        assert out[key][0] == ref[0] and out[key][1] == ref[1], key
        for r in range(4):
            assert np.array_equal(out[key][2][r], ref[2][r]) and np.array_equal(out[key][3][r], ref[3][r]), (key, r)


def test_two_contexts_on_streams_of_their_own(hip):
    """counters belong to a context: two contexts on one device, each on its own stream, launching in alternation on the two grids"""
    import torch
    cases = [_case(GRIDS[q], "float64", BCS[0], 4) for q in (0, 1)]
    ctxs, streams, bufs = [], [], []
    for q in (0, 1):
        c = hip.Context(0, "strict")
        c.set_ptn_variant(2900)
        c.set_pt_pace(8)
        streams.append(c.use_own_stream())
        ctxs.append(c)
        g, P0, D0, R, ref = cases[q]
        dP, dD, dR = hip.from_numpy(P0), hip.from_numpy(D0), hip.from_numpy(R)
        dQ, dE = hip.from_numpy(np.full_like(P0, 555.0)), hip.from_numpy(np.full_like(D0, 444.0))
        bufs.append((dP, dQ, dD, dE, dR, _params(hip, dP, g, *BCS[0])))
    torch.cuda.synchronize()
    for _ in range(10):
        for q in (0, 1):
            dP, dQ, dD, dE, dR, p = bufs[q]
            hip.pt_sweepn(4, dP, dQ, dD, dE, dR, p, ctx=ctxs[q])
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for q in (0, 1):
        assert ctxs[q].last_pt_pace() == 8
        _same((hip.to_numpy(bufs[q][1]), hip.to_numpy(bufs[q][3])), cases[q][4], ("context", q))
        ctxs[q].close()
