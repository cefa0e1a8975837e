"""GPU tests of tracers and probes on a decomposed grid (include/ns3d.h): ns3d_sample_at, ns3d_tracers_advance_at,
ns3d_tracers_advance_mgpu, ns3d_tracers_migrate_mgpu and MgpuTracers / MgpuProbes on top of them.  ONE process drives P virtual
ranks on device 0, as in tests/test_gpu_mgpu.py.

The claim under test is decomposition independence: with halos that agree with the global field, P ranks return the bits of the
one-rank calls on the global field — positions, states, velocities, probe series — in every arithmetic mode alike, while the
first-stage Courant number stays below 1 in the decomposed directions.  References: the one-rank entry points on the global field
(themselves pinned to tests/tracers_ref.py by tests/test_gpu_tracers.py) and the NumPy restatement of the routing rule,
tests/tracers_mgpu_ref.py.  Every comparison is array_equal; nothing here has a tolerance."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tracers_mgpu_ref as MR
import tracers_ref as TR
from arena import Arena
from util import bits_equal, first_bit_difference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPDT = {"f64": np.float64, "f32": np.float32}
SLABS = [((1, 1, 2), (13, 7, 5)), ((1, 1, 3), (13, 7, 5))]
CARTS = [((2, 2, 1), (7, 6, 5)), ((2, 1, 2), (7, 6, 5)), ((2, 2, 2), (7, 6, 5))]
TOPOLOGIES = SLABS + CARTS
TID = lambda t: "x".join(str(d) for d in t[0])
COURANT = (0.4, 0.36, 0.32)
SPACINGS = tuple(1.0 / c for c in COURANT)         # with dt = 1: MgpuTracers and Tracers form dt/d the same way
STAGS = (("Vx", (1, 0, 0)), ("Vy", (0, 1, 0)), ("Vz", (0, 0, 1)), ("Pr", (0, 0, 0)))


@functools.lru_cache(maxsize=None)
def global_fields(g, dt):
    """Vx, Vy, Vz, Pr of the global grid g, uniform in (−1, 1): |v·c| ≤ 0.4 < 1 by construction.  Shared, never modified."""
    rng = np.random.Generator(np.random.MT19937(91))
    return tuple(np.asfortranarray(rng.uniform(-1.0, 1.0, size=tuple(g[q] + s[q] for q in range(3))).astype(NPDT[dt])) for _, s in STAGS)


@functools.lru_cache(maxsize=None)
def particles(dims, n):
    """(X, state): 2000 uniform points of the global box, then the planted ones — on every seam value, one ulp beside it, on the
    global faces, with a NaN coordinate, and a dead one"""
    g = MR.n_g(dims, n)
    Xp, sp = MR.planted(dims, n)
    X = np.ascontiguousarray(np.concatenate([TR.uniform_points(g, 2000, 17), Xp], axis=1))
    return X, np.concatenate([np.ones(2000, dtype=np.uint8), sp])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_grid(dims, n, mode="strict"):
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    torch.cuda.synchronize()
    P = dims[0] * dims[1] * dims[2]
    mg = MultiGpu.create([0] * P, n[0], n[1], n[2], mode, dims=dims)
    return mg, MgpuGrid(mg, *n)


def local_fields(hip, dims, n, dt):
    """one namespace of device fields per rank, cut from the global fields with their halos: local = global[o : o + n + s]"""
    from types import SimpleNamespace
    G = global_fields(MR.n_g(dims, n), dt)
    return [SimpleNamespace(**{nm: hip.from_numpy(MR.cut(a, s, r, dims, n)) for (nm, s), a in zip(STAGS, G)})
            for r in range(dims[0] * dims[1] * dims[2])]


@functools.lru_cache(maxsize=None)
def one_rank_steps(dims, n, dt, steps=6):
    """X, state, U after each of `steps` steps of the one-rank Tracers on the global field (STRICT; the calls return the same bits in
    every mode, tests/test_gpu_tracers.py) — computed once per case and shared"""
    from types import SimpleNamespace
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd.tracers import Tracers
    g = MR.n_g(dims, n)
    ctx = K.Context(0, "strict")
    f = SimpleNamespace(**{nm: K.from_numpy(a) for (nm, _), a in zip(STAGS, global_fields(g, dt))})
    t = Tracers(g, ctx, SPACINGS, keep_velocity=True)
    t._set(*particles(dims, n))
    out = []
    for _ in range(steps):
        t.advance(f, 1.0)
        ctx.sync()
        out.append((t.X.cpu().numpy(), t.state.cpu().numpy(), t.U.cpu().numpy()))
    ctx.close()
    return out


# ---- 1. NULL origin: the one-rank bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_null_origin_gives_the_bits_of_the_one_rank_calls(hip, dt):
    n, N = (13, 7, 5), 1000
    X, state = TR.uniform_points(n, N, 5), (np.random.Generator(np.random.MT19937(6)).uniform(size=N) < 0.8).astype(np.uint8)
    Xp, sp = TR.planted_points(n)                                  # dead, NaN, ±Inf and out-of-box points
    X[:, -Xp.shape[1]:], state[-Xp.shape[1]:] = Xp, sp
    V = [hip.from_numpy(a) for a in global_fields(n, dt)]
    ctx = hip.Context(0, "strict")
    for q, (_, stag) in enumerate(STAGS):
        for st in (None, dev(state)):
            a, b = (torch.full((N,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
            hip.sample(V[q], dev(X), a, state=st, stagger=stag, ctx=ctx)
            hip.sample_at(V[q], dev(X), b, state=st, stagger=stag, origin=None, ctx=ctx)
            ctx.sync()
            assert bits_equal(a.cpu().numpy(), b.cpu().numpy()) and np.isfinite(a.cpu().numpy()).any()
            hip.sample_at(V[q], dev(X), b, state=st, stagger=stag, origin=(0, 0, 0), ctx=ctx)
            ctx.sync()
            assert bits_equal(a.cpu().numpy(), b.cpu().numpy())
    for kw in (dict(), dict(origin=(0, 0, 0), n_g=n), dict(n_g=(20, 9, 5))):
        got = []
        for fn, extra in ((hip.tracers_advance, {}), (hip.tracers_advance_at, kw)):
            Xd, sd, Ud = dev(X), dev(state), torch.full((3, N), 7.0, dtype=torch.float64, device="cuda")
            fn(Xd, sd, *V[:3], *COURANT, U=Ud, ctx=ctx, **extra)
            ctx.sync()
            got.append((Xd.cpu().numpy(), sd.cpu().numpy(), Ud.cpu().numpy()))
        if kw.get("n_g") == (20, 9, 5):      # a larger global box decides only who is active at the start and alive at the end
            act = (state == 1) & TR.inside(X, n)
            assert bits_equal(got[0][2][:, act], got[1][2][:, act]) and bits_equal(got[0][0][:, act], got[1][0][:, act])
            assert (got[1][1] >= got[0][1]).all() and got[1][1].sum() > got[0][1].sum()
        else:
            assert bits_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and bits_equal(got[0][2], got[1][2])
            assert got[0][1].sum() > 500
    ctx.close()


# ---- 2. decomposition independence -------------------------------------------------------------------------------------------------
def crossings(dims, n, X0, X1, alive1):
    """per direction: live particles whose owner coordinate changed over a step"""
    fin = np.isfinite(X0).all(axis=0) & np.isfinite(X1).all(axis=0) & (alive1 == 1)
    return [int(np.sum(MR.owner_coord(X0[q, fin], dims[q], n[q]) != MR.owner_coord(X1[q, fin], dims[q], n[q]))) for q in range(3)]


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("topo", TOPOLOGIES, ids=TID)
def test_p_ranks_reproduce_the_one_rank_tracers_bit_for_bit(hip, topo, dt, mode):
    """Six steps of advance_mgpu + migrate; after EVERY step X, state and U, compared by id, equal the one-rank Tracers on the global
    field.  Particles cross a seam in each decomposed direction and particles migrate — asserted, not assumed."""
    from navierstokes3d_amd.tracers import MgpuTracers
    dims, n = topo
    X, state = particles(dims, n)
    ref = one_rank_steps(dims, n, dt)
    mg, grid = make_grid(dims, n, mode)
    try:
        fs = local_fields(hip, dims, n, dt)
        t = MgpuTracers(grid, SPACINGS, keep_velocity=True, slack=0.1)
        t._set(X, state)
        crossed, expect_moved, prev = [0, 0, 0], 0, X
        for step, (Xr, sr, Ur) in enumerate(ref):
            t.advance(fs, 1.0)
            fin = np.isfinite(prev).all(axis=0) & np.isfinite(Xr).all(axis=0) & (sr == 1)
            expect_moved += int(np.sum(MR.owners(prev[:, fin], dims, n) != MR.owners(Xr[:, fin], dims, n)))
            assert t.moved == expect_moved, (step, t.moved, expect_moved)
            Xg, sg, Ug = t.index_positions(), t.by_id(t.state), t.velocities()
            assert np.array_equal(Xg, Xr, equal_nan=True), (step, "X", first_bit_difference(Xg, Xr))
            assert np.array_equal(sg, sr), (step, "state", int((sg != sr).sum()))
            assert np.array_equal(Ug, Ur, equal_nan=True), (step, "U", first_bit_difference(Ug, Ur))
            # a live particle sits on the rank that owns it
            for l in range(grid.P):
                ids, st = t.ids[l].cpu().numpy(), t.state[l].cpu().numpy()
                live = (ids >= 0) & (st == 1)
                assert np.all(MR.owners(t.X[l].cpu().numpy()[:, live], dims, n) == l), (step, l)
            crossed = [a + b for a, b in zip(crossed, crossings(dims, n, prev, Xr, sr))]
            prev = Xr
        for q in range(3):
            assert (crossed[q] > 0) == (dims[q] > 1), (q, crossed)
        assert expect_moved > 0 and t.steps == 6
        # sample(): the pressure at the particles, by id, is ns3d_sample's reference on the global field; sort_by_cell keeps the ids
        G = global_fields(MR.n_g(dims, n), dt)
        want = TR.sample(G[3], prev, ref[-1][1], (0, 0, 0))
        got = t.by_id(t.sample([f.Pr for f in fs]))
        assert np.array_equal(got, want, equal_nan=True) and np.isfinite(want).sum() > 1500
        t.sort_by_cell()
        assert np.array_equal(t.index_positions(), prev, equal_nan=True) and np.array_equal(t.by_id(t.state), ref[-1][1])
        assert np.array_equal(t.by_id(t.sample([f.Pr for f in fs])), want, equal_nan=True)
        assert (ref[-1][1] == 0).sum() > (state == 0).sum()             # some left through the global faces, on whatever rank
    finally:
        mg.sync()
        mg.close()


# ---- 3. migration order and capacity -----------------------------------------------------------------------------------------------
def scrambled(dims, n, seed, extra):
    """per-rank slot arrays whose particles sit ANYWHERE in the global box (not only next to their rank): leavers for every
    destination, dead ones, NaN coordinates, empty slots in the middle of the arrays, payload in U"""
    g = MR.n_g(dims, n)
    P = dims[0] * dims[1] * dims[2]
    rng = np.random.Generator(np.random.MT19937(seed))
    N = 1500
    X = TR.uniform_points(g, N, seed)
    state = (rng.uniform(size=N) < 0.9).astype(np.uint8)
    Xs, ss, ids, Us = MR.distribute(X, state, dims, n, extra=extra)
    for l in range(P):
        occ = np.nonzero(ids[l] >= 0)[0]
        far = occ[rng.uniform(size=occ.size) < 0.4]                    # 40 %: somewhere else in the box
        Xs[l][:, far] = TR.uniform_points(g, far.size, seed + 1 + l)
        if occ.size > 8:
            Xs[l][1, occ[3]] = np.nan                                  # alive with a NaN coordinate: stays
            gone = occ[5::7]                                           # holes: empty slots between occupied ones
            Xs[l][:, gone], ss[l][gone], ids[l][gone] = np.nan, 0, -1
        Us[l][:, ids[l] >= 0] = rng.uniform(size=(3, int((ids[l] >= 0).sum())))
    return Xs, ss, ids, Us


def upload(arrs):
    return [[dev(a) for a in lst] for lst in arrs]


def download(mg, darrs):
    mg.sync()
    return [[t.cpu().numpy() for t in lst] for lst in darrs]


def same_layout(got, want, what):
    for name, g_l, w_l in zip(("X", "state", "id", "U"), got, want):
        for l, (a, b) in enumerate(zip(g_l, w_l)):
            assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (what, name, l)


@pytest.mark.parametrize("topo", [SLABS[1], CARTS[2]], ids=TID)
def test_migration_equals_the_numpy_rule_slot_for_slot(hip, topo):
    dims, n = topo
    P = dims[0] * dims[1] * dims[2]
    host = scrambled(dims, n, 23, extra=700)
    want = MR.migrate(*host, dims, n)
    assert want[5] == [0] * P and want[4] > 200
    dead_before = [(i[(s == 0) & (i >= 0)], x[:, (s == 0) & (i >= 0)]) for x, s, i in zip(*host[:3])]
    mg, _ = make_grid(dims, n)
    try:
        for with_u in (True, False):
            runs = []
            for _ in range(2):                                         # two calls from the same input: the same arrays
                d = upload(host)
                moved, need = mg.tracers_migrate(d[0], d[1], d[2], d[3] if with_u else None)
                assert need is None and moved == want[4]
                runs.append(download(mg, d))
            same_layout(runs[0][:3], want[:3], "with U" if with_u else "without U")
            same_layout(runs[1][:3], runs[0][:3], "second call")
            if with_u:
                same_layout(runs[0], want[:4], "payload")
            else:
                same_layout(runs[0][3:], [host[3]], "U not passed: untouched")
        # dead particles never move, empty slots stay where no arrival lands, a second migrate finds nothing to do
        got = runs[0]
        for l in range(P):
            ids, x = got[2][l], got[0][l]
            for i, xi in zip(dead_before[l][0], dead_before[l][1].T):
                assert np.array_equal(x[:, ids == i][:, 0], xi, equal_nan=True), (l, i)
        d = upload(want[:4])
        assert mg.tracers_migrate(*d) == (0, None)
        same_layout(download(mg, d), want[:4], "nothing left to move")
    finally:
        mg.sync()
        mg.close()


def test_short_capacity_changes_nothing_and_reports_the_need(hip):
    from navierstokes3d_amd import lib as L
    dims, n = SLABS[1]
    roomy = scrambled(dims, n, 29, extra=700)
    want = MR.migrate(*roomy, dims, n)
    arrivals = [int(np.sum((want[2][l] >= 0) & ~np.isin(want[2][l], roomy[2][l]))) for l in range(3)]
    room = [int(np.sum((roomy[2][l] < 0) | MR.leavers(roomy[0][l], roomy[1][l], roomy[2][l], l, dims, n)[0])) for l in range(3)]
    cut1 = room[1] - arrivals[1] + 1                                   # rank 1 ends ONE slot short
    was_empty = np.nonzero(roomy[2][1] < 0)[0]                         # holes and the surplus at the end
    assert arrivals[1] > 0 and 0 < cut1 <= was_empty.size
    short = [[a.copy() for a in lst] for lst in roomy]
    for q in range(4):
        short[q][1] = np.ascontiguousarray(np.delete(short[q][1], was_empty[-cut1:], axis=-1))
    ref = MR.migrate(*short, dims, n)
    assert ref[5] == [0, 1, 0] and ref[4] == 0
    mg, _ = make_grid(dims, n)
    try:
        d = upload(short)
        moved, need = mg.tracers_migrate(*d)
        assert (moved, need) == (0, [0, 1, 0])
        same_layout(download(mg, d), short, "short capacity: untouched")
        # the C call itself: NS3D_ERR_STATE and the message
        caps = [int(s.numel()) for s in d[1]]
        mv, nd = C.c_longlong(-5), (C.c_long * 3)(7, 7, 7)
        rc = mg.lib.ns3d_tracers_migrate_mgpu(mg.handle, mg._slot_ptrs(d[0], 3, torch.float64, "X", caps),
                                              mg._slot_ptrs(d[1], 1, torch.uint8, "state", caps), mg._slot_ptrs(d[2], 1, torch.int64, "ids", caps),
                                              None, (C.c_long * 3)(*caps), C.byref(mv), nd)
        assert rc == L.NS3D_ERR_STATE and list(nd) == [0, 1, 0] and mv.value == 0 and "fewer empty slots" in L.last_error()
        same_layout(download(mg, d), short, "short capacity, C call: untouched")
        # after growing by the need: the reference's layout, and every particle on the rank the roomy run puts it on
        grown = [[a.copy() for a in lst] for lst in short]
        grown[0][1] = np.concatenate([grown[0][1], np.full((3, 1), np.nan)], axis=1)
        grown[1][1] = np.concatenate([grown[1][1], np.zeros(1, dtype=np.uint8)])
        grown[2][1] = np.concatenate([grown[2][1], np.full(1, -1, dtype=np.int64)])
        grown[3][1] = np.concatenate([grown[3][1], np.full((3, 1), np.nan)], axis=1)
        ref = MR.migrate(*grown, dims, n)
        assert ref[5] == [0, 0, 0] and ref[4] == want[4] and np.all(ref[2][1] >= 0)      # rank 1 is full to the last slot
        d = upload(grown)
        moved, need = mg.tracers_migrate(*d)
        assert need is None and moved == want[4]
        got = download(mg, d)
        same_layout(got, ref[:4], "grown")
        for l in range(3):
            assert np.array_equal(np.sort(got[2][l][got[2][l] >= 0]), np.sort(want[2][l][want[2][l] >= 0])), l
        assert np.array_equal(MR.by_id(got[0], got[2], 1500), MR.by_id(want[0], want[2], 1500), equal_nan=True)
        # ranks without slots: fine as long as nobody is bound for them; a rank with cap = 0 that gets arrivals reports them all
        empty = [[np.zeros((3, 0)) for _ in range(3)], [np.zeros(0, dtype=np.uint8) for _ in range(3)],
                 [np.zeros(0, dtype=np.int64) for _ in range(3)], [np.zeros((3, 0)) for _ in range(3)]]
        assert mg.tracers_migrate(*upload(empty)) == (0, None)
        mixed = [[a.copy() for a in lst] for lst in roomy]
        for q in range(4):
            mixed[q][2] = empty[q][2]
        ref = MR.migrate(*mixed, dims, n)
        assert ref[5][2] > 0 and ref[5][:2] == [0, 0]
        d = upload(mixed)
        assert mg.tracers_migrate(*d) == (0, ref[5])
        same_layout(download(mg, d), mixed, "a rank without slots: untouched")
    finally:
        mg.sync()
        mg.close()


# ---- 4. probes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("topo", TOPOLOGIES, ids=TID)
def test_mgpu_probes_equal_probes_on_the_global_field(hip, topo, dt):
    from types import SimpleNamespace
    from navierstokes3d_amd.tracers import MgpuProbes, Probes
    dims, n = topo
    g = MR.n_g(dims, n)
    sp, org = (0.5, 0.25, 0.125), (-1.0, -2.0, -0.5)                    # powers of two: physical → index space is exact
    Xi = np.concatenate([TR.uniform_points(g, 300, 41), MR.planted(dims, n)[0]], axis=1)
    Xi = np.concatenate([Xi, np.array([[-0.25, 1.0, 1.0], [1.0, g[1] + 0.5, 1.0]]).T], axis=1)      # outside the global box
    xyz = np.stack([org[q] + Xi[q] * sp[q] for q in range(3)], axis=1)
    ctx = hip.Context(0, "strict")
    mg, grid = make_grid(dims, n)
    try:
        G = global_fields(g, dt)
        one = Probes(g, ctx, sp, org, xyz, 2)
        Xone = one.X.cpu().numpy()
        for q in range(3):                                             # the points ON the seam values survive the conversion exactly
            assert all(np.any(Xone[q] == s) for s in MR.seams(dims, n, q))
        many = MgpuProbes(grid, sp, org, xyz, 2)
        assert sum(i.size for i in many.index) == Xi.shape[1] and min(i.size for i in many.index) > 0
        fs = local_fields(hip, dims, n, dt)
        for scale in (1.0, -0.5):                                       # two steps on two states
            Gs = [np.asfortranarray(a * NPDT[dt](scale)) for a in G]
            one.record(SimpleNamespace(**{nm: hip.from_numpy(a) for (nm, _), a in zip(STAGS, Gs)}))
            many.record([SimpleNamespace(**{nm: hip.from_numpy(MR.cut(a, s, r, dims, n)) for (nm, s), a in zip(STAGS, Gs)})
                         for r in range(grid.P)])
        a, b = one.gathered(), many.gathered()
        for nm in "uvwp":
            x, y = getattr(a, nm), getattr(b, nm)
            assert y.shape == (2, Xi.shape[1]) and np.array_equal(x, y, equal_nan=True), (nm, first_bit_difference(x, y))
            assert np.isnan(y[:, -2:]).all() and np.isfinite(y[:, :300]).all()
        del fs
    finally:
        mg.sync()
        mg.close()
        ctx.close()


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------
def test_driver_with_mgpu_tracers_and_probes_reproduces_the_one_rank_run(hip, nx=36, P=2, nz_loc=12, niter_cap=None):
    """run_navierstokes3D on P z-slab ranks with wide_advect_halo=True, tracers=MgpuTracers, probes=MgpuProbes against the one-rank
    run with tracers=300, probes=points, nt = 3: info.tracers (by id) and info.probes bit for bit, the flow unchanged by the
    observers, |w|·dt/dz far below 1 (asserted from the returned fields).
    The grid is the one of the test this one is modelled on, test_driver_with_wide_advect_halo_reproduces_the_one_rank_run in
    tests/test_gpu_mgpu.py: nx = 36, P = 2, nz_loc = 12 (global 36x22x22), "a size at which the reference's iteration stays finite"
    (measured on one MI355X: 21, 84, 105 iterations, max|w|·dt/dz = 8.0e-12 after step 3).  NOT nx = 24, P = 2, nz_loc = 9 (global
    24x15x16), the grid of test_two_ranks_raise: there the ONE-RANK flow itself is not finite after its third step — iterations 28,
    42, 1200 (= niter, not converged), max|u|, |v|, |w| = 6.4e300, 8.6e300, inf, so |w|·dt/dz = inf — and with niter_cap=40 (finite)
    the 2-rank flow WITHOUT any observer already differs from the one-rank flow (first in C): on that grid no P-rank run reproduces
    the one-rank run, whatever observes it.  test_driver_observers_on_the_24_grid keeps what can be asked there."""
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    from navierstokes3d_amd.tracers import MgpuProbes, MgpuTracers
    nt = 3
    nz_g = P * (nz_loc - 2) + 2
    kw = dict(nx=nx, nt=nt, mode="strict", return_info=True, **(dict(niter_cap=niter_cap) if niter_cap else {}))
    plain = run_navierstokes3D(shape=dict(nz=nz_g), **kw)
    assert all(np.isfinite(a).all() for a in plain[:5])
    p = plain[-1].params
    assert (p.nx, p.nz) == (nx, nz_g)
    rng = np.random.Generator(np.random.MT19937(21))
    ext = np.array([p.lx, p.ly, p.lz])
    points = (rng.uniform(0.02, 0.98, size=(12, 3)) - 0.5) * ext
    points[0, 2] = -p.lz / 2 + (nz_loc - 2 + 1) * p.dz                  # on the seam plane
    points[-1] = ext                                                    # outside
    one = run_navierstokes3D(shape=dict(nz=nz_g), tracers=300, probes=points, **kw)
    for a, b in zip(one[:5], plain[:5]):
        assert np.array_equal(a, b, equal_nan=True)
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    assert (p0.dx, p0.dy, p0.dz, p0.dt) == (p.dx, p.dy, p.dz, p.dt)
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        grid = MgpuGrid(mg, p0.nx, p0.ny, p0.nz)
        low = (-p0.lx / 2, -p0.ly / 2, -p0.lz / 2)
        trc = MgpuTracers(grid, (p0.dx, p0.dy, p0.dz), low).seed_random(300, 0)
        prb = MgpuProbes(grid, (p0.dx, p0.dy, p0.dz), low, points, nt)
        out = run_navierstokes3D(grid=grid, shape=dict(nz=nz_loc), wide_advect_halo=True, tracers=trc, probes=prb, **kw)
        bare = run_navierstokes3D(grid=grid, shape=dict(nz=nz_loc), wide_advect_halo=True, **kw)
        for nm, a, b, c in zip(("C", "Pr", "Vx", "Vy"), out[:4], one[:4], bare[:4]):
            assert np.array_equal(a, b, equal_nan=True), nm                      # the one-rank flow …
            assert np.array_equal(a, c, equal_nan=True), nm                      # … unchanged by the observers
        assert out[-1].iters == one[-1].iters == bare[-1].iters
        # only z is decomposed, and the flow's first-stage Courant number in z is far below 1
        w = max(float(np.abs(hip.to_numpy(f.Vz)).max()) for f in out[-1].local_fields)
        assert w * p.dt / p.dz < 0.5, w * p.dt / p.dz
        a, b = one[-1].tracers, out[-1].tracers
        assert a.steps == b.steps == nt and out[-1].tracers is not trc
        for nm in ("x", "y", "z", "alive"):
            assert np.array_equal(getattr(a, nm), getattr(b, nm), equal_nan=True), nm
        assert trc.moved >= 0 and (a.z != TR.uniform_points((p.nx, p.ny, p.nz), 300, 0)[2] * p.dz - p.lz / 2).any()
        for nm in "uvwp":
            x, y = getattr(one[-1].probes, nm), getattr(out[-1].probes, nm)
            assert x.shape == y.shape == (nt, 12) and np.array_equal(x, y, equal_nan=True), nm
        assert np.isnan(out[-1].probes.u[:, -1]).all() and np.isfinite(out[-1].probes.u[:, :-1]).all()
        # an int or an array on several ranks still raises; so does an object of another grid
        with pytest.raises(L.Ns3dError, match="one rank"):
            run_navierstokes3D(grid=grid, shape=dict(nz=nz_loc), tracers=10, **kw)
        with pytest.raises(L.Ns3dError, match="MgpuTracers"):
            run_navierstokes3D(grid=grid, shape=dict(nz=nz_loc), probes=points, **kw)
        with pytest.raises(L.Ns3dError, match="another grid"):
            run_navierstokes3D(grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), shape=dict(nz=nz_loc), tracers=trc, **kw)
    finally:
        mg.sync()
        mg.close()


def test_driver_observers_on_the_24_grid(hip):
    """nx = 24, P = 2, nz_loc = 9, wide_advect_halo=True, nt = 3, niter_cap=40 (see above for why not more): the observers leave the
    2-rank flow's bits alone, every seeded particle is accounted for, an int or an array still raises with "one rank"."""
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    from navierstokes3d_amd.tracers import MgpuProbes, MgpuTracers
    nx, P, nz_loc, nt = 24, 2, 9, 3
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    points = (np.random.Generator(np.random.MT19937(21)).uniform(0.02, 0.98, size=(12, 3)) - 0.5) * np.array([p0.lx, p0.ly, p0.lz])
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        grid = MgpuGrid(mg, p0.nx, p0.ny, p0.nz)
        kw = dict(nx=nx, nt=nt, mode="strict", return_info=True, niter_cap=40, grid=grid, shape=dict(nz=nz_loc), wide_advect_halo=True)
        low = (-p0.lx / 2, -p0.ly / 2, -p0.lz / 2)
        trc = MgpuTracers(grid, (p0.dx, p0.dy, p0.dz), low).seed_random(300, 0)
        out = run_navierstokes3D(tracers=trc, probes=MgpuProbes(grid, (p0.dx, p0.dy, p0.dz), low, points, nt), **kw)
        bare = run_navierstokes3D(**kw)
        for nm, a, c in zip(("C", "Pr", "Vx", "Vy", "Vz"), out[:5], bare[:5]):
            assert np.isfinite(a).all() and np.array_equal(a, c), nm
        t = out[-1].tracers
        assert t.steps == nt and t.x.shape == (300,) and np.isfinite(t.x).all() and t.alive.sum() > 250
        assert out[-1].probes.p.shape == (nt, 12) and np.isfinite(out[-1].probes.p).all()
        for bad in (dict(tracers=10), dict(probes=points), dict(tracers=points, probes=points)):
            with pytest.raises(L.Ns3dError, match="one rank"):
                run_navierstokes3D(**bad, **kw)
    finally:
        mg.sync()
        mg.close()


# ---- 6. footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_at_forms_touch_nothing_outside_their_arrays(hip, dt):
    """advance_at / sample_at of an interior rank of (3,2,2) ranks, every device array a view at an odd element offset of a guarded
    arena: guards intact, inputs untouched, outputs the reference's bits"""
    dims, n, rank = (3, 2, 2), (7, 6, 5), 7                            # coordinates (1,1,1): seams on five sides
    g, o = MR.n_g(dims, n), MR.origin_of(rank, dims, n)
    V = [MR.cut(a, s, rank, dims, n) for (_, s), a in zip(STAGS, global_fields(g, dt))]
    N = 777
    rng = np.random.Generator(np.random.MT19937(3))
    X = np.ascontiguousarray(np.array(o, dtype=np.float64).reshape(3, 1) + 1.0
                             + rng.uniform(size=(3, N)) * (np.array(n, dtype=np.float64).reshape(3, 1) - 2.0))
    state = (rng.uniform(size=N) < 0.9).astype(np.uint8)
    X[0, 5], X[2, 6] = np.nan, -1.0
    ctx = hip.Context(0, "strict")
    ar = Arena([("X", X, True), ("state", state, True), ("U", np.full((3, N), 5.0), True), ("Vx", V[0], False), ("Vy", V[1], False),
                ("Vz", V[2], False)])
    hip.tracers_advance_at(ar["X"], ar["state"], ar["Vx"], ar["Vy"], ar["Vz"], *COURANT, U=ar["U"], origin=o, n_g=g, ctx=ctx)
    ctx.sync()
    ar.assert_clean("tracers_advance_at")
    Xr, sr, Ur = MR.advance_rank(X, state, *V[:3], COURANT, o, g)
    assert bits_equal(ar.get("X"), Xr) and np.array_equal(ar.get("state"), sr) and bits_equal(ar.get("U"), Ur) and sr.sum() > 500
    for nm, a in zip(("Vx", "Vy", "Vz"), V):
        assert bits_equal(ar.get(nm), a), nm
    for q, (nm, stag) in enumerate(STAGS):
        ar = Arena([("out", np.full(N, 5.0), True), ("X", X, False), ("state", state, False), ("A", V[q], False)])
        hip.sample_at(ar["A"], ar["X"], ar["out"], state=ar["state"], stagger=stag, origin=o, ctx=ctx)
        ctx.sync()
        ar.assert_clean("sample_at " + nm)
        want = TR.sample(V[q], X - np.array(o, dtype=np.float64).reshape(3, 1), state, stag)
        assert bits_equal(ar.get("out"), want) and np.isfinite(want).sum() > 500, nm
        assert bits_equal(ar.get("X"), X) and np.array_equal(ar.get("state"), state) and bits_equal(ar.get("A"), V[q])
    ctx.close()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched(hip):
    from navierstokes3d_amd import lib as L
    n, N = (7, 6, 5), 40
    V = [hip.from_numpy(a) for a in global_fields(n, "f64")]
    X0 = TR.uniform_points(n, N, 2)
    ctx = hip.Context(0, "strict")
    Xd, sd, Ud, out = dev(X0), dev(np.ones(N, dtype=np.uint8)), torch.full((3, N), 3.0, dtype=torch.float64, device="cuda"), \
        torch.full((N,), 3.0, dtype=torch.float64, device="cuda")

    def untouched():
        ctx.sync()
        return bits_equal(Xd.cpu().numpy(), X0) and bool((sd == 1).all()) and bool((Ud == 3.0).all()) and bool((out == 3.0).all())

    bad = [dict(origin=(-1, 0, 0)), dict(origin=(0, 0, 1), n_g=n), dict(n_g=(7, 6, 4)), dict(origin=(5, 0, 0), n_g=(11, 6, 5))]
    for kw in bad:
        with pytest.raises(L.Ns3dError, match="origin|global grid"):
            hip.tracers_advance_at(Xd, sd, *V[:3], *COURANT, U=Ud, ctx=ctx, **kw)
        assert untouched(), kw
    with pytest.raises(L.Ns3dError, match="Courant"):
        hip.tracers_advance_at(Xd, sd, *V[:3], 0.1, float("nan"), 0.1, U=Ud, origin=(0, 0, 0), n_g=n, ctx=ctx)
    with pytest.raises(L.Ns3dError, match="origin"):
        hip.sample_at(V[3], Xd, out, origin=(0, -2, 0), ctx=ctx)
    with pytest.raises(L.Ns3dError, match="stagger"):
        hip.sample_at(V[3], Xd, out, stagger=(0, 2, 0), origin=(0, 0, 0), ctx=ctx)
    assert untouched()
    lib = L.load()
    assert lib.ns3d_sample_at_f64(ctx.handle, None, C.c_void_p(Xd.data_ptr()), None, N, C.c_void_p(V[3].data_ptr()), 7, 6, 5, 0, 0, 0,
                                  None) == L.NS3D_ERR_ARG
    assert lib.ns3d_tracers_advance_at_f64(ctx.handle, C.c_void_p(Xd.data_ptr()), None, None, N, *[C.c_void_p(v.data_ptr()) for v in V[:3]],
                                           0.1, 0.1, 0.1, 7, 6, 5, None, None) == L.NS3D_ERR_ARG
    assert lib.ns3d_tracers_advance_at_f64(ctx.handle, C.c_void_p(Xd.data_ptr()), C.c_void_p(sd.data_ptr()), None, -1,
                                           *[C.c_void_p(v.data_ptr()) for v in V[:3]], 0.1, 0.1, 0.1, 7, 6, 5, None, None) == L.NS3D_ERR_ARG
    assert untouched()
    ctx.close()
    # the two mgpu calls
    dims = (1, 1, 2)
    mg, grid = make_grid(dims, n)
    try:
        host = scrambled(dims, n, 31, extra=400)
        d = upload(host)
        fs = local_fields(hip, dims, n, "f64")
        Vl = [[getattr(f, nm) for f in fs] for nm in ("Vx", "Vy", "Vz")]
        with pytest.raises(L.Ns3dError, match="Courant"):
            mg.tracers_advance(d[0], d[1], *Vl, float("inf"), 0.1, 0.1, U=d[3])
        with pytest.raises(L.Ns3dError, match="one array per local rank"):
            mg.tracers_advance(d[0][:1], d[1], *Vl, 0.1, 0.1, 0.1)
        with pytest.raises(L.Ns3dError, match="elements"):
            mg.tracers_migrate(d[0], d[1], [d[2][0], d[2][1][:-1]], d[3])
        caps = [int(s.numel()) for s in d[1]]
        ptr = lambda q, b, t, nm: mg._slot_ptrs(d[q], b, t, nm, caps)
        Xp, sp, ip = ptr(0, 3, torch.float64, "X"), ptr(1, 1, torch.uint8, "state"), ptr(2, 1, torch.int64, "ids")
        mv, nd, cp = C.c_longlong(-5), (C.c_long * 2)(7, 7), (C.c_long * 2)(*caps)
        call = mg.lib.ns3d_tracers_migrate_mgpu
        assert call(mg.handle, None, sp, ip, None, cp, C.byref(mv), nd) == L.NS3D_ERR_ARG
        assert call(mg.handle, Xp, sp, ip, None, None, C.byref(mv), nd) == L.NS3D_ERR_ARG
        assert call(mg.handle, Xp, sp, ip, None, cp, None, nd) == L.NS3D_ERR_ARG
        assert call(mg.handle, Xp, sp, ip, None, (C.c_long * 2)(caps[0], -1), C.byref(mv), nd) == L.NS3D_ERR_ARG
        assert call(mg.handle, Xp, sp, (C.c_void_p * 2)(d[2][0].data_ptr(), None), None, cp, C.byref(mv), nd) == L.NS3D_ERR_ARG
        assert "null particle array (local rank 1)" in L.last_error()
        adv = mg.lib.ns3d_tracers_advance_mgpu_f64
        Vp = [mg._ptrs([v]) for v in Vl]
        assert adv(mg.handle, Xp, sp, None, cp, Vp[0], None, Vp[2], 0.1, 0.1, 0.1) == L.NS3D_ERR_ARG
        assert adv(mg.handle, Xp, (C.c_void_p * 2)(None, d[1][1].data_ptr()), None, cp, *Vp, 0.1, 0.1, 0.1) == L.NS3D_ERR_ARG
        assert mv.value == -5 and list(nd) == [7, 7]
        same_layout(download(mg, d), host, "argument errors: untouched")
    finally:
        mg.sync()
        mg.close()


_RCCL_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
from navierstokes3d_amd import lib as L
from navierstokes3d_amd.mgpu import MultiGpu
uid = MultiGpu.unique_id()
assert uid.startswith(b"/fake_rccl_")
mg = MultiGpu.create_rank(1, 0, 0, uid, 7, 6, 5, "strict")
assert mg.transport == "rccl"
X = [torch.full((3, 4), 1.5, dtype=torch.float64, device="cuda")]
s = [torch.ones(4, dtype=torch.uint8, device="cuda")]
i = [torch.arange(4, dtype=torch.int64, device="cuda")]
try:
    mg.tracers_migrate(X, s, i)
    print("NO ERROR")
except L.Ns3dError as e:
    print("REFUSED" if "status 3" in str(e) and "one-process form only" in str(e) else "OTHER: %s" % e)
V = [torch.zeros(sh, dtype=torch.float64, device="cuda").permute(2, 1, 0) for sh in ((5, 6, 8), (5, 7, 7), (6, 6, 7))]
mg.tracers_advance(X, s, [V[0]], [V[1]], [V[2]], 0.1, 0.1, 0.1)          # the advance works in both transports
mg.sync()
print("ADVANCED" if bool((X[0] == 1.5).all()) and bool((s[0] == 1).all()) and bool((i[0] == torch.arange(4, device="cuda")).all()) else "MOVED")
mg.close()
"""


def test_migrate_refuses_the_rccl_form(hip):
    """the one-process-per-GPU form, brought up through tests/fake_rccl in a process of its own (the library binds its RCCL once)"""
    from test_gpu_fake_rccl import FAKE_SO, build_fake
    build_fake()
    env = dict(os.environ, NS3D_RCCL_LIB=FAKE_SO, FAKE_RCCL_ARENA_MB="8")
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD, ROOT], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["REFUSED", "ADVANCED"], r.stdout + r.stderr
