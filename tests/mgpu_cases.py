"""The multi-rank calls that tests/test_gpu_stream_order_mgpu.py and tests/test_gpu_footprint_mgpu.py run, as data: for every entry
point of navierstokes3d_amd.mgpu the topology, the per-rank host arrays (seeded as tests/test_gpu_mgpu.py, test_gpu_direct_slab.py,
test_gpu_diagnostics.py and test_gpu_tracers_mgpu.py seed theirs), which of them the call writes, and the call itself on per-rank lists
of device arrays.  One table serves both modules, so both run the same calls.  Nothing here needs a GPU or torch to be BUILT: the
host tests construct every case (tests/test_stream_order_host.py)."""
from types import SimpleNamespace

import numpy as np

import stream_order as SO
import tracers_mgpu_ref as MR
import tracers_ref as TR
from util import SHAPES, fields, geometry

NP = {"f64": np.float64, "f32": np.float32}
DTS = ["f64", "f32"]
KINDS6 = ["c", "vx", "vy", "vz", "s", "i"]
GID = lambda n: "%dx%dx%d" % tuple(n)


def TID(topo):
    d, n = topo
    return ("dims%d%d%d" % tuple(d) if isinstance(d, tuple) else "P%d" % d) + "-" + GID(n)


class Spec(SimpleNamespace):
    """name, topo, arrays [(name, [host array per rank], role)], outputs {names the call writes}, call(hip, mg, t), blocking, setup;
    halo_only: the call writes nothing but the halo layers of its arrays (update_halo)"""

    def rank_case(self, blocking=None, name=None):
        return SO.RankCase(name or self.name, self.topo, self.arrays, self.call, blocking=self.blocking if blocking is None else blocking,
                           setup=self.setup)


def _spec(name, topo, arrays, outputs, call, blocking=False, setup=None, halo_only=False):
    return Spec(name=name, topo=topo, arrays=arrays, outputs=set(outputs), call=call, blocking=blocking, setup=setup, halo_only=halo_only)


def coords_of(r, dims):
    return MR.coords_of(r, dims)


def _dims(topo):
    dims, P, n = SO.topo_of(topo)
    return (1, 1, P) if dims is None else dims, P, n


def _cut(G, kind, r, dims, n):
    """rank r's local array of the global array G of stagger `kind`, halos included"""
    c = coords_of(r, dims)
    shp = SHAPES[kind](*n)
    return np.asfortranarray(G[tuple(slice(c[d] * (n[d] - 2), c[d] * (n[d] - 2) + shp[d]) for d in range(3))])


def _global(topo):
    dims, P, n = _dims(topo)
    return tuple(dims[d] * (n[d] - 2) + 2 for d in range(3))


def _ptp(hip, n, g, owns=True, val=0.25, grav=0.0):
    return hip.pt_params(SimpleNamespace(shape=tuple(n)), g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, grav)


# ---- update_halo, gather ------------------------------------------------------------------------------------------------------------
HALO_TOPOS = [(2, (13, 9, 7)), (3, (13, 9, 7)), ((2, 1, 1), (70, 6, 7)), ((1, 2, 1), (70, 6, 7)), ((2, 2, 2), (13, 9, 7))]
HALO2_TOPOS = [(3, (13, 9, 7)), ((2, 2, 1), (13, 9, 7))]
GATHER_TOPOS = [(3, (11, 8, 6)), ((2, 2, 1), (11, 8, 6))]


def halo_case(topo, dt):
    """one call with the six staggers of test_update_halo_follows_implicit_global_grid"""
    _, P, n = _dims(topo)
    host = [fields(*n, KINDS6, 100 * (r + 1), NP[dt]) for r in range(P)]
    arrays = [(k, [host[r][q] for r in range(P)], "field") for q, k in enumerate(KINDS6)]
    return _spec("update_halo %s %s" % (TID(topo), dt), topo, arrays, KINDS6, lambda hip, mg, t: mg.update_halo(*[t[k] for k in KINDS6]),
                 halo_only=True)


def halo_twice_case(topo, dt):
    """two calls back to back on different field sets: the message buffer and the three events are reused with nothing between"""
    _, P, n = _dims(topo)
    a, b = ["c", "vx", "vz"], ["vy", "c", "s"]
    ha = [fields(*n, a, 100 * (r + 1), NP[dt]) for r in range(P)]
    hb = [fields(*n, b, 100 * (r + 1) + 50, NP[dt]) for r in range(P)]
    arrays = [("a_" + k, [ha[r][q] for r in range(P)], "field") for q, k in enumerate(a)]
    arrays += [("b_" + k, [hb[r][q] for r in range(P)], "field") for q, k in enumerate(b)]

    def call(hip, mg, t):
        mg.update_halo(*[t["a_" + k] for k in a])
        mg.update_halo(*[t["b_" + k] for k in b])
    return _spec("update_halo twice %s %s" % (TID(topo), dt), topo, arrays, [nm for nm, _, _ in arrays], call, halo_only=True)


def gather_case(topo, dt):
    _, P, n = _dims(topo)
    kinds = ["c", "vz"]
    host = [fields(*n, kinds, 31 * (r + 1), NP[dt]) for r in range(P)]
    arrays = [("A_" + k, [host[r][q] for r in range(P)], "field") for q, k in enumerate(kinds)]
    return _spec("gather %s %s" % (TID(topo), dt), topo, arrays, [], lambda hip, mg, t: tuple(mg.gather(t["A_" + k]) for k in kinds), blocking=True)


# ---- the pseudo-transient loop ------------------------------------------------------------------------------------------------------
SLAB_TOPOS = [(2, (40, 21, 10)), (3, (70, 12, 6)), (4, (33, 9, 4))]
SLAB_DEPTHS = [(2, 7), (1, 4)]
SOLVE_RUNS = [((2, (40, 21, 10)), None), (((2, 1, 1), (20, 14, 10)), None), (((2, 1, 1), (20, 14, 10)), 1)]


def _pt_fields(topo, dt, seed, scale=1.0):
    dims, P, n = _dims(topo)
    N = _global(topo)
    Pg, Dg, Rg = fields(*N, ["c", "i", "c"], seed, NP[dt])
    s = NP[dt](scale)
    Pg, Dg, Rg = Pg * s, Dg * s, Rg * (s * s)
    cut = lambda G, kind: [_cut(G, kind, r, dims, n) for r in range(P)]
    return [("Pr", cut(Pg, "c"), "field"), ("D", cut(Dg, "i"), "field"), ("R", cut(Rg, "c"), "field")], geometry(*N)


def slab_case(topo, depth, n_iters, dt):
    """slab_load, slab_iterate(n), slab_store as one call (test_slab_state_equals_global_solve)"""
    _, P, n = _dims(topo)
    arrays, g = _pt_fields(topo, dt, 211)

    def call(hip, mg, t):
        mg.slab_load(t["Pr"], t["D"], t["R"], _ptp(hip, n, g))
        mg.slab_iterate(n_iters)
        mg.slab_store(t["Pr"], t["D"])
    return _spec("slab load/iterate(%d)/store depth %d %s %s" % (n_iters, depth, TID(topo), dt), topo, arrays, ["Pr", "D"], call, blocking=True,
                 setup=lambda mg: mg.set_temporal(depth))


def solve_case(topo, temporal, dt):
    """pt_solve_slab with a fixed iteration count: niter 12, a check every 4, eps < 0"""
    _, P, n = _dims(topo)
    arrays, g = _pt_fields(topo, dt, 91, 1e-3)
    g["dtau"] = 0.8 / np.sqrt(1.0 / g["dx"] ** 2 + 1.0 / g["dy"] ** 2 + 1.0 / g["dz"] ** 2)     # inside the iteration's stability limit

    def call(hip, mg, t):
        return mg.pt_solve_slab(t["Pr"], t["D"], t["R"], _ptp(hip, n, g), -1.0, 12, 4, 0.36, 1000.0)
    return _spec("pt_solve_slab%s %s %s" % ("" if temporal is None else " temporal %d" % temporal, TID(topo), dt), topo, arrays, ["Pr", "D"],
                 call, blocking=True, setup=None if temporal is None else (lambda mg: mg.set_temporal(temporal)))


CHAIN_TOPO = (2, (40, 21, 10))


def chain_case(dt):
    """update_halo(Vx,Vy,Vz), update_divV on every rank's context, update_halo(divV), pt_solve_slab — the driver's mixture of
    multi-rank calls and single-rank kernels on the ranks' contexts"""
    topo = CHAIN_TOPO
    dims, P, n = _dims(topo)
    N = _global(topo)
    g = geometry(*N)
    g["dtau"] = 0.8 / np.sqrt(1.0 / g["dx"] ** 2 + 1.0 / g["dy"] ** 2 + 1.0 / g["dz"] ** 2)
    kinds = dict(Vx="vx", Vy="vy", Vz="vz", divV="c", Pr="c", D="i")
    arrays = []
    for q, (nm, kind) in enumerate(kinds.items()):
        # every rank a field of its own (not cuts of one global field): the halo updates have something to do
        arrays.append((nm, [np.asfortranarray(fields(*n, [kind], 500 + 10 * q + r, NP[dt])[0] * NP[dt](1e-3)) for r in range(P)], "field"))

    def call(hip, mg, t):
        mg.update_halo(t["Vx"], t["Vy"], t["Vz"])
        for l, ctx in enumerate(mg.contexts):
            hip.update_divV(t["divV"][l], t["Vx"][l], t["Vy"][l], t["Vz"][l], g["dx"], g["dy"], g["dz"], ctx=ctx)
        mg.update_halo(t["divV"])
        return mg.pt_solve_slab(t["Pr"], t["D"], t["divV"], _ptp(hip, n, g), -1.0, 12, 4, 0.36, 1000.0)
    return _spec("halo, divV, halo, pt_solve_slab %s %s" % (TID(topo), dt), topo, arrays, list(kinds), call, blocking=True)


# ---- advect_wide --------------------------------------------------------------------------------------------------------------------
ADVECT_RUNS = [(2, 9, 1.9), (3, 7, 1.5)]
ADV_NAMES = ("Vx", "Vy", "Vz", "C")


def _advect_arrays(P, nz, dt, seed, tag=""):
    nx, ny = 21, 10
    topo = (P, (nx, ny, nz))
    dims, _, n = _dims(topo)
    glob = fields(*_global(topo), ["vx", "vy", "vz", "c"], seed, NP[dt])
    arrays = []
    for nm, kind, G in zip(ADV_NAMES, ("vx", "vy", "vz", "c"), glob):
        new = [_cut(G, kind, r, dims, n) for r in range(P)]
        arrays.append((tag + nm, new, "field"))
        arrays.append((tag + nm + "_o", [np.zeros_like(a) for a in new], "field"))
    return topo, arrays


def _advect_call(mg, t, cfl, g, faithful, tag=""):
    step = cfl * min(g["dx"], g["dy"], g["dz"])
    a = []
    for nm in ADV_NAMES:
        a += [t[tag + nm], t[tag + nm + "_o"]]
    mg.advect_wide(*a, step, g["dx"], g["dy"], g["dz"], faithful)


def advect_case(P, nz, cfl, faithful, dt):
    topo, arrays = _advect_arrays(P, nz, dt, 321)
    g = geometry(*_global(topo))
    return _spec("advect_wide %s cfl %g %s %s" % ("faithful" if faithful else "corrected", cfl, TID(topo), dt), topo, arrays,
                 [nm for nm, _, _ in arrays], lambda hip, mg, t: _advect_call(mg, t, cfl, g, faithful))


def advect_twice_case(dt):
    """two calls back to back on two field sets: the widened copies (wbuf) are refilled behind the first call's advection"""
    topo, a = _advect_arrays(2, 9, dt, 321, "a_")
    _, b = _advect_arrays(2, 9, dt, 421, "b_")
    g = geometry(*_global(topo))

    def call(hip, mg, t):
        _advect_call(mg, t, 1.9, g, True, "a_")
        _advect_call(mg, t, 1.9, g, False, "b_")
    return _spec("advect_wide twice %s %s" % (TID(topo), dt), topo, a + b, [nm for nm, _, _ in a + b], call)


# ---- the direct solve, the monitor --------------------------------------------------------------------------------------------------
DIRECT_RUNS = [(3, (20, 4, 6)), (2, (17, 9, 6))]            # the two smallest of test_gpu_direct_slab.py's list
DIAG_TOPO = (2, (24, 15, 9))


def direct_case(topo, dt):
    dims, P, n = _dims(topo)
    N = _global(topo)
    g = geometry(*N)
    rhs = fields(*N, ["c"], 57, NP[dt])[0]
    arrays = [("Pr", [fields(*n, ["c"], 3 + r, NP[dt])[0] for r in range(P)], "field"),
              ("D", [fields(*n, ["i"], 40 + r, NP[dt])[0] for r in range(P)], "field"),
              ("R", [_cut(rhs, "c", r, dims, n) for r in range(P)], "field")]
    return _spec("poisson_direct %s %s" % (TID(topo), dt), topo, arrays, ["Pr", "D"],
                 lambda hip, mg, t: mg.poisson_direct(t["Pr"], t["D"], t["R"], _ptp(hip, n, g, True, 0.75, g["g"])), blocking=True)


def diag_case(dt):
    topo = DIAG_TOPO
    dims, P, n = _dims(topo)
    N = _global(topo)
    g = geometry(*N)
    names, kinds = ("Vx", "Vy", "Vz", "Pr", "C"), ("vx", "vy", "vz", "c", "c")
    G = fields(*N, kinds, 11, NP[dt])
    arrays = [(nm, [_cut(A, k, r, dims, n) for r in range(P)], "field") for nm, k, A in zip(names, kinds, G)]

    def call(hip, mg, t):
        dps = [hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"]) for _ in range(P)]
        return mg.diagnostics(*[t[nm] for nm in names], dps)
    return _spec("diagnostics %s %s" % (TID(topo), dt), topo, arrays, [], call, blocking=True)


# ---- tracers ------------------------------------------------------------------------------------------------------------------------
TRACER_TOPO = ((1, 1, 2), (13, 7, 5))                       # test_gpu_tracers_mgpu.py's smallest case
COURANT = (0.4, 0.36, 0.32)
STAGS = (("Vx", (1, 0, 0)), ("Vy", (0, 1, 0)), ("Vz", (0, 0, 1)))


def _tracer_fields(dims, n, dt):
    g = MR.n_g(dims, n)
    rng = np.random.Generator(np.random.MT19937(91))
    G = [np.asfortranarray(rng.uniform(-1.0, 1.0, size=tuple(g[q] + s[q] for q in range(3))).astype(NP[dt])) for _, s in STAGS]
    P = dims[0] * dims[1] * dims[2]
    return [(nm, [MR.cut(A, s, r, dims, n) for r in range(P)], "field") for (nm, s), A in zip(STAGS, G)]


def _particles(dims, n):
    g = MR.n_g(dims, n)
    Xp, sp = MR.planted(dims, n)
    X = np.ascontiguousarray(np.concatenate([TR.uniform_points(g, 2000, 17), Xp], axis=1))
    return X, np.concatenate([np.ones(2000, dtype=np.uint8), sp])


def tracers_advance_case(dt):
    dims, n = TRACER_TOPO
    g = MR.n_g(dims, n)
    Xs, ss, _, Us = MR.distribute(*_particles(dims, n), dims, n)
    arrays = [("X", Xs, ("points", g)), ("state", ss, "state"), ("U", Us, "field")] + _tracer_fields(dims, n, dt)

    def call(hip, mg, t):
        mg.tracers_advance(t["X"], t["state"], t["Vx"], t["Vy"], t["Vz"], *COURANT, U=t["U"])
    return _spec("tracers_advance %s %s" % (TID(TRACER_TOPO), dt), TRACER_TOPO, arrays, ["X", "state", "U"], call)


def tracers_migrate_case():
    """particles anywhere in the global box on every rank: leavers for both directions, dead ones, holes, payload in U.  (Footprint
    only: the id array has no decoy that keeps the slot layout valid.)"""
    dims, n = TRACER_TOPO
    g = MR.n_g(dims, n)
    rng = np.random.Generator(np.random.MT19937(23))
    N = 1500
    X = TR.uniform_points(g, N, 23)
    state = (rng.uniform(size=N) < 0.9).astype(np.uint8)
    Xs, ss, ids, Us = MR.distribute(X, state, dims, n, extra=700)
    for l in range(len(Xs)):
        occ = np.nonzero(ids[l] >= 0)[0]
        far = occ[rng.uniform(size=occ.size) < 0.4]
        Xs[l][:, far] = TR.uniform_points(g, far.size, 24 + l)
        gone = occ[5::7]
        Xs[l][:, gone], ss[l][gone], ids[l][gone] = np.nan, 0, -1
        Us[l][:, ids[l] >= 0] = rng.uniform(size=(3, int((ids[l] >= 0).sum())))
    arrays = [("X", Xs, ("points", g)), ("state", ss, "state"), ("ids", ids, "ids"), ("U", Us, "field")]
    spec = _spec("tracers_migrate %s" % TID(TRACER_TOPO), TRACER_TOPO, arrays, ["X", "state", "ids", "U"],
                 lambda hip, mg, t: mg.tracers_migrate(t["X"], t["state"], t["ids"], t["U"]), blocking=True)
    spec.reference = MR.migrate(Xs, ss, ids, Us, dims, n)
    return spec


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def table(dt):
    """every case of the stream-order module for one element type, as (family, spec); the footprint module adds tracers_migrate"""
    out = [("update_halo", halo_case(topo, dt)) for topo in HALO_TOPOS]
    out += [("update_halo_twice", halo_twice_case(topo, dt)) for topo in HALO2_TOPOS]
    out += [("gather", gather_case(topo, dt)) for topo in GATHER_TOPOS]
    out += [("slab", slab_case(topo, depth, it, dt)) for topo in SLAB_TOPOS for depth, it in SLAB_DEPTHS]
    out += [("pt_solve_slab", solve_case(topo, temporal, dt)) for topo, temporal in SOLVE_RUNS]
    out += [("advect_wide", advect_case(P, nz, cfl, faithful, dt)) for P, nz, cfl in ADVECT_RUNS for faithful in (True, False)]
    out += [("advect_wide_twice", advect_twice_case(dt))]
    out += [("poisson_direct", direct_case(topo, dt)) for topo in DIRECT_RUNS]
    out += [("diagnostics", diag_case(dt)), ("tracers_advance", tracers_advance_case(dt)), ("chain", chain_case(dt))]
    return out


def halo_layers(spec, name, l):
    """boolean mask of rank l's array `name`: True on the layers a halo update may write — the outermost layer of every side that
    has a neighbour.  The `s` and `i` staggers have no halo: all False."""
    dims, P, n = _dims(spec.topo)
    a = [per_rank for nm, per_rank, _ in spec.arrays if nm == name][0][l]
    mask = np.zeros(a.shape, dtype=bool)
    if any(a.shape[d] < n[d] for d in range(3)):
        return mask
    c = coords_of(l, dims)
    for d in range(3):
        idx = [slice(None)] * 3
        if c[d] > 0:
            idx[d] = 0
            mask[tuple(idx)] = True
        if c[d] < dims[d] - 1:
            idx[d] = a.shape[d] - 1
            mask[tuple(idx)] = True
    return mask
