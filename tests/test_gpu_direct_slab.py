"""ns3d_poisson_direct_slab (include/ns3d.h; csrc/ns3d_mgpu.cpp + csrc/ns3d_direct.hip): the direct pressure solve of the GLOBAL grid
on z-slab ranks — x and y on each rank's planes, z on a y chunk of every plane between two all-to-all transposes.  ONE process
drives P virtual ranks on device 0 (the peer-copy transport); every rank's planes, halo planes and boundary cells included, are
compared with the single-rank ns3d_poisson_direct of the global grid and with its NumPy twin (oracle/direct_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from util import fields, geometry, rel_l2

pytestmark = pytest.mark.gpu

OWN_STREAMS = False


@pytest.fixture(autouse=True, params=["torch-stream", "own-streams"])
def rank_streams(request):
    """Every test runs with all virtual ranks on PyTorch's current stream and with a non-blocking compute stream per rank (the
    all-to-all's ready / landed events then carry the ordering, as between the devices of a node)."""
    global OWN_STREAMS
    import torch
    OWN_STREAMS = request.param == "own-streams"
    torch.cuda.synchronize()
    yield
    torch.cuda.synchronize()
    OWN_STREAMS = False


def _mg(P, nx, ny, nz, own=None, dims=None):
    import torch
    from navierstokes3d_amd.mgpu import MultiGpu
    torch.cuda.synchronize()
    return MultiGpu.create([0] * P, nx, ny, nz, "strict", own_streams=OWN_STREAMS if own is None else own, dims=dims)


def _problem(P, n, owns, dtype, seed=57):
    """global right-hand side (mean-free for the all-Neumann rule), local cuts, geometry"""
    nx, ny, nz = n
    nzg = P * (nz - 2) + 2
    g = geometry(nx, ny, nzg)
    rhs = fields(nx, ny, nzg, ["c"], seed, dtype)[0]
    if not owns:
        rhs[1:-1, 1:-1, 1:-1] -= rhs[1:-1, 1:-1, 1:-1].mean(dtype=np.float64).astype(dtype)
    return rhs, g


def _cut(A, r, nz):
    lo = r * (nz - 2)
    return np.asfortranarray(A[:, :, lo:lo + nz])


def _global_direct(hip, rhs, g, owns, val):
    import torch
    nx, ny, nzg = rhs.shape
    ctx = hip.Context(0, "strict")
    dP = hip.from_numpy(np.zeros((nx, ny, nzg), rhs.dtype, order="F"))
    dD = hip.from_numpy(np.zeros((nx - 2, ny - 2, nzg - 2), rhs.dtype, order="F"))
    dR = hip.from_numpy(rhs)
    p = hip.pt_params(dP, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"])
    hip.poisson_direct(dP, dD, dR, p, ctx=ctx)
    torch.cuda.synchronize()
    out = hip.to_numpy(dP)
    ctx.close()
    return out


def _slab_direct(hip, mg, rhs, g, n, owns, val, seed=3):
    """one call of MultiGpu.poisson_direct on the cuts of rhs; returns (device Pr, dPrdτ, divV lists, params)"""
    P = mg.P
    nx, ny, nz = n
    Ps = [hip.from_numpy(fields(nx, ny, nz, ["c"], seed + r, rhs.dtype)[0]) for r in range(P)]        # whatever was there before
    Ds = [hip.from_numpy(fields(nx, ny, nz, ["i"], 40 + r, rhs.dtype)[0]) for r in range(P)]
    Rs = [hip.from_numpy(_cut(rhs, r, nz)) for r in range(P)]
    p = hip.pt_params(Ps[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"])
    mg.poisson_direct(Ps, Ds, Rs, p)
    mg.sync()
    return Ps, Ds, Rs, p


CASES = [(2, (17, 9, 6)), (3, (24, 15, 7)), (4, (70, 35, 8)), (2, (131, 66, 37)), (3, (20, 4, 6)), (4, (24, 15, 7)),
         (3, (70, 50, 8)),      # my = 48: 16 y columns per rank — the z products on the LDS-staged kernel at N = 16, with a column offset
         (2, (70, 34, 8))]      # my = 32: 16 columns per rank on two ranks


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bc", [(True, 0.0), (True, 0.75), (False, 0.0)])
@pytest.mark.parametrize("P,n", CASES)
def test_slab_solve_equals_the_global_direct_solve(hip, P, n, bc, dtype):
    """GEMM tile edges in every product (local extents below, at and above 16/32/64), a chunk table with empty chunks (ny−2 < P),
    the three x rules; every local plane against the single-rank solve of the global grid, the gathered interior against the
    NumPy twin, the reference's residual of the solution at rounding level."""
    from oracle.direct_ref import poisson_direct
    owns, val = bc
    nx, ny, nz = n
    rhs, g = _problem(P, n, owns, dtype)
    want = _global_direct(hip, rhs, g, owns, val)
    ref = poisson_direct(rhs.astype(np.float64), g["rho"], g["dt"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"])
    mg = _mg(P, nx, ny, nz)
    Ps, Ds, Rs, p = _slab_direct(hip, mg, rhs, g, n, owns, val)
    tol = 1e-11 if dtype == np.float64 else 2e-6
    for r in range(P):
        got = hip.to_numpy(Ps[r])
        assert np.isfinite(got).all()
        assert rel_l2(got, _cut(want, r, nz)) <= tol, (r, rel_l2(got, _cut(want, r, nz)))
        assert not hip.to_numpy(Ds[r]).any()
        assert np.array_equal(hip.to_numpy(Rs[r]), _cut(rhs, r, nz))
    gathered = mg.gather(Ps)
    assert rel_l2(gathered, ref[1:-1, 1:-1, 1:-1]) <= tol, rel_l2(gathered, ref[1:-1, 1:-1, 1:-1])
    if dtype == np.float64:
        loc = []
        for r in range(P):
            q = hip.pt_params(Ps[r], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"],
                              r > 0, r < P - 1)
            loc.append(hip.residual_max(Ps[r], Rs[r], q, ctx=mg.contexts[r]))
        res = mg.max_g(loc)
        scale = g["rho"] / g["dt"] * np.abs(rhs).max() + np.abs(ref).max() / min(g["dx"], g["dy"], g["dz"]) ** 2
        assert res < 1e-10 * scale, res / scale
    mg.close()


def test_determinism_plan_reuse_and_stream_setups(hip):
    """A second call gives the same bits; a call with another x rule or spacing rebuilds the rank's plan and equals a fresh
    ns3d_mgpu; the torch-stream and own-stream schedules give the same bits."""
    P, n = 3, (40, 21, 9)
    rhs, g = _problem(P, n, True, np.float64)
    outs = []
    for own in (False, True):
        mg = _mg(P, *n, own=own)
        Ps, _, _, _ = _slab_direct(hip, mg, rhs, g, n, True, 0.5)
        first = [hip.to_numpy(t) for t in Ps]
        Ps2, _, _, _ = _slab_direct(hip, mg, rhs, g, n, True, 0.5, seed=9)
        assert all(np.array_equal(hip.to_numpy(a), b) for a, b in zip(Ps2, first))
        # another x rule and spacing on the same ranks, then back
        g2 = dict(g, dx=g["dx"] * 1.25)
        Pa, _, _, _ = _slab_direct(hip, mg, rhs, g2, n, False, 0.0)
        fresh = _mg(P, *n, own=own)
        Pb, _, _, _ = _slab_direct(hip, fresh, rhs, g2, n, False, 0.0)
        assert all(np.array_equal(hip.to_numpy(a), hip.to_numpy(b)) for a, b in zip(Pa, Pb))
        fresh.close()
        Ps3, _, _, _ = _slab_direct(hip, mg, rhs, g, n, True, 0.5)
        assert all(np.array_equal(hip.to_numpy(a), b) for a, b in zip(Ps3, first))
        outs.append(first)
        mg.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [(131, 66, 37), (17, 9, 6)])
def test_one_rank_is_bitwise_the_single_rank_solve(hip, n, dtype):
    rhs, g = _problem(1, n, True, dtype)
    want = _global_direct(hip, rhs, g, True, 0.25)
    mg = _mg(1, *n)
    Ps, Ds, _, _ = _slab_direct(hip, mg, rhs, g, n, True, 0.25)
    assert np.array_equal(hip.to_numpy(Ps[0]), want) and not hip.to_numpy(Ds[0]).any()
    mg.close()


def test_errors(hip):
    """x/y-decomposed topologies, gpu.jl's boundary set, a null pointer and a too-small grid: Ns3dError, nothing crashes, and the
    ranks still work afterwards."""
    from navierstokes3d_amd import lib as L
    n = (12, 10, 8)
    rhs, g = _problem(2, n, True, np.float64)
    for dims in ((2, 1, 1), (1, 2, 1)):
        mg = _mg(2, *n, dims=dims)
        with pytest.raises(L.Ns3dError, match="z-slab"):
            _slab_direct(hip, mg, rhs, g, n, True, 0.0)
        mg.close()
    mg = _mg(2, *n)
    Ps = [hip.zeros(n) for _ in range(2)]
    Ds = [hip.zeros((n[0] - 2, n[1] - 2, n[2] - 2)) for _ in range(2)]
    Rs = [hip.from_numpy(_cut(rhs, r, n[2])) for r in range(2)]
    pg = hip.pt_params(Ps[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], L.NS3D_BC_GPU, False, 0.0, g["g"])
    with pytest.raises(L.Ns3dError, match="NS3D_BC_GPU"):
        mg.poisson_direct(Ps, Ds, Rs, pg)
    p = hip.pt_params(Ps[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, True, 0.0, g["g"])
    ptr = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    bad = (C.c_void_p * 2)(Ps[0].data_ptr(), None)
    assert mg.lib.ns3d_poisson_direct_slab_f64(mg.handle, bad, ptr(Ds), ptr(Rs), C.byref(p)) == L.NS3D_ERR_ARG
    assert mg.lib.ns3d_poisson_direct_slab_f64(mg.handle, ptr(Ps), ptr(Ds), None, C.byref(p)) == L.NS3D_ERR_ARG
    assert mg.lib.ns3d_poisson_direct_slab_f64(None, ptr(Ps), ptr(Ds), ptr(Rs), C.byref(p)) == L.NS3D_ERR_ARG
    mg.poisson_direct(Ps, Ds, Rs, p)                       # still usable
    mg.sync()
    mg.close()
    small = (12, 3, 6)
    mg = _mg(2, *small)
    Ps = [hip.zeros(small) for _ in range(2)]
    Ds = [hip.zeros((10, 1, 4)) for _ in range(2)]
    ps = hip.pt_params(Ps[0], 1000.0, 0.01, 0.01, 0.1, 0.1, 0.1, 0.1)
    with pytest.raises(L.Ns3dError, match="too small"):
        mg.poisson_direct(Ps, Ds, [hip.zeros(small) for _ in range(2)], ps)
    mg.close()


@pytest.mark.parametrize("P,nz_loc", [(2, 12), (4, 7)])
def test_driver_with_direct_pressure_on_z_slab_ranks_reproduces_the_one_rank_run(hip, P, nz_loc):
    """run_navierstokes3D(pressure="direct") on a MgpuGrid of P z-slab ranks (wide advection halo: every other kernel is
    decomposition-independent) against the one-rank direct run of the same global 36×22×22 grid: the direct solves differ in
    summation order only."""
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid
    from navierstokes3d_amd.params import multi_params
    nx, nt = 36, 3
    one = run_navierstokes3D(nx=nx, nt=nt, mode="strict", pressure="direct", return_info=True)
    assert one[-1].params.nz == P * (nz_loc - 2) + 2
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    mg = _mg(P, p0.nx, p0.ny, p0.nz)
    out = run_navierstokes3D(nx=nx, nt=nt, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), return_info=True,
                             shape=dict(nz=nz_loc), pressure="direct", wide_advect_halo=True)
    info = out[-1]
    assert info.iters == [0] * nt and all(e[0] < 1e-8 for e in info.errs), info.errs
    pairs = list(zip(("C", "Pr", "Vx", "Vy"), out[:4], one[:4]))
    vnorm = max(np.sqrt(np.sum(np.asarray(b, dtype=np.float64) ** 2)) for n_, a, b in pairs if n_.startswith("V"))
    for n_, a, b in pairs:
        assert a.shape == b.shape and np.isfinite(a).all()
        assert rel_l2(a, b, vnorm if n_.startswith("V") else None) < 1e-9, (n_, rel_l2(a, b))
    mg.close()


def test_driver_direct_pressure_on_an_x_decomposed_grid_names_mgpugrid(hip):
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid
    from navierstokes3d_amd.params import multi_params
    p0 = multi_params(20, dims=(2, 1, 1), coords=(0, 0, 0))
    mg = _mg(2, p0.nx, p0.ny, p0.nz, dims=(2, 1, 1))
    with pytest.raises(L.Ns3dError, match="MgpuGrid"):
        run_navierstokes3D(nx=20, nt=1, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), pressure="direct")
    mg.sync()
    mg.close()
