"""Host side of ns3d_tracers_advance and ns3d_sample (include/ns3d.h): Lagrangian tracer particles and point probes of a running
flow.  Every interpolation and every particle step is done on the device by libns3d; this module owns the particle arrays, converts
between physical and index-space coordinates on the host, and keeps the probes' time series on the device until the run ends.
PyTorch does no arithmetic on the hot path (sort_by_cell, seeding and the read-backs are not on it).

Index space: the cell grid occupies [0,nx]×[0,ny]×[0,nz], cell centres sit at half-integers; physical x = origin + ξ·dx, with
`origin` the low corner of cell (0,0,0) — (−lx/2, −ly/2, −lz/2) in both reference scripts."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import kernels as K
from . import lib as L


def _after_fill(ctx):
    """fresh or rewritten particle arrays: kernels.Context.after_torch_fill (ctx=None: the arrays are on the CPU)"""
    if ctx is not None:
        ctx.after_torch_fill()


def _points(xyz):
    a = np.asarray(xyz, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise L.Ns3dError("points must be an (N, 3) array of physical coordinates, got shape %r" % (a.shape,))
    return a


class Tracers:
    """N particles in the box of one rank's (nx,ny,nz) cell grid: X (3×N float64, index space, blocks ξ | η | ζ), state (N uint8:
    1 alive, 0 dead) and — with keep_velocity — U (3×N float64: the velocity at the start points of the latest step), all on the
    context's device.  ctx=None keeps the arrays on the CPU: everything but advance / sample works there."""

    def __init__(self, shape, ctx, spacings, origin=(0.0, 0.0, 0.0), keep_velocity=False):
        self.shape = tuple(int(q) for q in shape)
        self.ctx = ctx
        self.device = torch.device("cpu") if ctx is None else torch.device("cuda", ctx.device)
        self.spacings = tuple(float(q) for q in spacings)
        self.origin = tuple(float(q) for q in origin)
        self.keep_velocity = bool(keep_velocity)
        self.steps = 0
        self._set(np.zeros((3, 0)), np.zeros(0, dtype=np.uint8))

    def _set(self, X, state):
        self.X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(self.device)
        self.state = torch.from_numpy(np.ascontiguousarray(state, dtype=np.uint8)).to(self.device)
        self.U = torch.full_like(self.X, float("nan")) if self.keep_velocity else None
        _after_fill(self.ctx)

    @property
    def n(self):
        return int(self.state.numel())

    def to_index(self, xyz):
        """(N,3) physical → (3,N) index space: (x − origin)/d, on the host in double"""
        a = _points(xyz)
        return np.ascontiguousarray(np.stack([(a[:, q] - self.origin[q]) / self.spacings[q] for q in range(3)]))

    def _inside(self, X):
        with np.errstate(invalid="ignore"):
            return np.logical_and.reduce([(X[q] >= 0.0) & (X[q] <= float(self.shape[q])) for q in range(3)])

    def seed_points(self, xyz):
        """Replace the particle set by the physical points xyz (N,3); points outside the closed box start dead."""
        X = self.to_index(xyz)
        self._set(X, self._inside(X).astype(np.uint8))
        self.steps = 0
        return self

    def seed_random(self, n, seed=0):
        """n points uniform in the box, from a Mersenne Twister seeded with `seed` (reproducible on the host)"""
        rng = np.random.Generator(np.random.MT19937(int(seed)))
        X = rng.uniform(0.0, 1.0, size=(3, int(n))) * np.asarray(self.shape, dtype=np.float64).reshape(3, 1)
        self._set(X, np.ones(int(n), dtype=np.uint8))
        self.steps = 0
        return self

    def reseed(self, xyz):
        """Put the physical points xyz (M,3) into DEAD slots only, lowest slots first; returns how many were placed
        (min(M, number of dead slots)).  Live particles and their order are untouched."""
        X = self.to_index(xyz)
        if self.ctx is not None and self.ctx._pinned:
            self.ctx.sync()             # an advance still queued on the context's own stream writes state and X
        dead = torch.nonzero(self.state == 0).flatten()
        k = min(int(dead.numel()), X.shape[1])
        if k:
            slots = dead[:k]
            self.X[:, slots] = torch.from_numpy(X[:, :k]).to(self.device)
            self.state[slots] = torch.from_numpy(self._inside(X[:, :k]).astype(np.uint8)).to(self.device)
            if self.U is not None:
                self.U[:, slots] = float("nan")
            _after_fill(self.ctx)
        return k

    def advance(self, f, dt):
        """One explicit-midpoint step of every live particle through the frozen field f.Vx, f.Vy, f.Vz (ns3d_tracers_advance;
        dt/dx, dt/dy, dt/dz are formed here in double).  Enqueues only.
        The call gathers 48 field values per particle, and its rate depends on the ORDER of the particles in memory: neighbours in
        memory that are neighbours in space share cache lines.  A set that has mixed — after many steps, or seeded at random —
        runs slower than the same set sorted by cell once it outgrows the caches (DESIGN §4.11 has the measured pair and from which N
        on); sort_by_cell() is the remedy.  It is never applied silently: it permutes the particle ids."""
        if self.ctx is None:
            raise L.Ns3dError("Tracers.advance needs a context: navierstokes3d_amd has no CPU path")
        if self.n:
            cx, cy, cz = (float(dt) / d for d in self.spacings)
            K.tracers_advance(self.X, self.state, f.Vx, f.Vy, f.Vz, cx, cy, cz, U=self.U, ctx=self.ctx)
        self.steps += 1

    def sample(self, A, stagger=(0, 0, 0), out=None):
        """The field A at the particles' positions (ns3d_sample): N float64 on the device, NaN for dead particles."""
        if self.ctx is None:
            raise L.Ns3dError("Tracers.sample needs a context: navierstokes3d_amd has no CPU path")
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        if self.n:
            K.sample(A, self.X, out, state=self.state, stagger=stagger, ctx=self.ctx)
        return out

    def positions(self):
        """(N,3) physical coordinates on the host: origin + ξ·d"""
        if self.ctx is not None:
            self.ctx.sync()
        X = self.X.cpu().numpy()
        return np.stack([self.origin[q] + X[q] * self.spacings[q] for q in range(3)], axis=1)

    def alive(self):
        """(N,) bool on the host"""
        if self.ctx is not None:
            self.ctx.sync()
        return self.state.cpu().numpy() == 1

    def record(self):
        """x, y, z (physical), alive, steps — what the drivers put into info.tracers"""
        P = self.positions()
        return SimpleNamespace(x=P[:, 0].copy(), y=P[:, 1].copy(), z=P[:, 2].copy(), alive=self.alive(), steps=self.steps)

    def cell_keys(self):
        """key ((k·ny + j)·nx + i) of each particle's containing cell (coordinates clamped into the grid); nx·ny·nz for a particle
        with a non-finite coordinate, so that those sort last"""
        nx, ny, nz = self.shape
        fin = torch.isfinite(self.X).all(dim=0)
        ijk = [torch.clamp(torch.floor(torch.where(fin, self.X[q], torch.zeros_like(self.X[q]))), 0, n - 1).to(torch.int64)
               for q, n in enumerate(self.shape)]
        key = (ijk[2] * ny + ijk[1]) * nx + ijk[0]
        return torch.where(fin, key, torch.full_like(key, nx * ny * nz))

    def sort_by_cell(self):
        """Reorder the particles by cell key, stably (particles of one cell keep their order), so that neighbours in memory are
        neighbours in space.  Torch ops, not on the hot path.  Returns the permutation `perm` (int64, on the arrays' device):
        new slot s holds the particle that was in slot perm[s] — apply it to any per-particle ids kept outside."""
        perm = torch.sort(self.cell_keys(), stable=True).indices
        self.X = self.X[:, perm].contiguous()
        self.state = self.state[perm].contiguous()
        if self.U is not None:
            self.U = self.U[:, perm].contiguous()
        return perm

    @staticmethod
    def save_bins(rec, iframe, outdir="out_save"):
        """out_tracers_%04d.bin: Float32, raw column-major (4,N) — x, y, z, alive per particle — beside the drivers' own dumps"""
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, "out_tracers_%04d.bin" % iframe)
        a = np.stack([rec.x, rec.y, rec.z, rec.alive.astype(np.float64)]).astype(np.float32)
        with open(path, "wb") as fh:
            fh.write(np.asfortranarray(a).tobytes(order="F"))
        return path


PROBE_FIELDS = (("u", "Vx", (1, 0, 0)), ("v", "Vy", (0, 1, 0)), ("w", "Vz", (0, 0, 1)), ("p", "Pr", (0, 0, 0)))


class Probes:
    """M fixed points at which u, v, w, p are sampled once per step (four ns3d_sample calls): the series stay on the device —
    a (4, nt, M) float64 array — and come back in ONE read-back when the run is over."""

    def __init__(self, shape, ctx, spacings, origin, xyz, nt):
        self.ctx = ctx
        t = Tracers(shape, ctx, spacings, origin)
        self.X = torch.from_numpy(t.to_index(xyz)).to(t.device)
        self.m = int(self.X.shape[1])
        self.series = torch.full((4, max(int(nt), 0), self.m), float("nan"), dtype=torch.float64, device=t.device)
        _after_fill(ctx)
        self.steps = 0

    def record(self, f):
        """sample the four fields of the current state into row `steps`; enqueues only"""
        if self.m:
            for q, (_, field, stag) in enumerate(PROBE_FIELDS):
                K.sample(getattr(f, field), self.X, self.series[q, self.steps], stagger=stag, ctx=self.ctx)
        self.steps += 1

    def gathered(self):
        """u, v, w, p as (nt, M) host arrays"""
        self.ctx.sync()
        host = self.series.cpu().numpy()
        return SimpleNamespace(**{name: host[q] for q, (name, _, _) in enumerate(PROBE_FIELDS)})


# ---- tracers and probes on a decomposed grid ------------------------------------------------------------------
def owner_coords(X, dims, n):
    """The ownership rule of include/ns3d.h on the host: (3, N) int64 rank coordinates of the points X ((3, N), GLOBAL index space)
    on a grid of dims ranks with n = (nx,ny,nz) local cells.  Per direction, rank coordinate k owns k(n−2)+1 ≤ X_q < (k+1)(n−2)+1,
    k = 0 from 0 (and everything below), k = D−1 up to n_g (and everything above): comparisons only.  NaN compares false: k = 0."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros(X.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for q in range(3):
            for k in range(1, int(dims[q])):
                out[q] += X[q] >= float(k * (int(n[q]) - 2) + 1)
    return out


def owner_ranks(X, dims, n):
    """rank (MPI_Cart order, last dimension fastest) that owns each point of X"""
    k = owner_coords(X, dims, n)
    return (k[0] * int(dims[1]) + k[1]) * int(dims[2]) + k[2]


def _grid_geometry(grid):
    n = (int(grid.nx), int(grid.ny), int(grid.nz))
    dims = tuple(int(d) for d in grid.dims)
    n_g = tuple(d * (m - 2) + 2 for d, m in zip(dims, n))
    if len(grid.local_ranks) != grid.P or list(grid.local_ranks) != list(range(grid.P)):
        raise L.Ns3dError("MgpuTracers / MgpuProbes need every rank in this process (a mgpu.MgpuGrid in the one-process form): "
                          "this process drives %d of %d ranks" % (len(grid.local_ranks), grid.P))
    origins = [tuple(co[q] * (n[q] - 2) for q in range(3)) for co in grid.local_coords]
    ctxs = list(grid.contexts) if getattr(grid, "contexts", None) else [None] * grid.P
    return n, dims, n_g, origins, ctxs


class MgpuTracers:
    """`Tracers` on a decomposed grid (a mgpu.MgpuGrid in the one-process form): every rank holds `cap` SLOTS — X (3×cap float64 in
    the GLOBAL index space [0,n_g]), state (cap uint8), ids (cap int64: the particle's number in seeding order, −1 for an empty slot)
    and, with keep_velocity, U — on its own device.  advance() is ns3d_tracers_advance_mgpu followed by ns3d_tracers_migrate_mgpu:
    a particle lives on the rank that owns its position.  `slack`: the fraction of empty slots every rank starts with (arrays grow on
    the host side when a rank runs short).  A grid without contexts keeps the arrays on the CPU: everything but advance / sample
    works there."""

    def __init__(self, grid, spacings, origin=(0.0, 0.0, 0.0), keep_velocity=False, slack=0.25):
        self.grid = grid
        self.n_loc, self.dims, self.shape, self.origins, self.ctxs = _grid_geometry(grid)
        self.devices = [torch.device("cpu") if c is None else torch.device("cuda", c.device) for c in self.ctxs]
        self.spacings = tuple(float(q) for q in spacings)
        self.origin = tuple(float(q) for q in origin)
        self.keep_velocity = bool(keep_velocity)
        self.slack = float(slack)
        if not self.slack >= 0.0:
            raise L.Ns3dError("slack = %r (a fraction >= 0)" % (slack,))
        self._host = Tracers(self.shape, None, self.spacings, self.origin)       # to_index and the global box test
        self.steps = self.moved = self.grown = 0
        self._set(np.zeros((3, 0)), np.zeros(0, dtype=np.uint8))

    # ---- the slot arrays ---------------------------------------------------------------------------------------------
    def _room(self, count):
        return int(count) + max(int(np.ceil(count * self.slack)), 16 if self.slack > 0.0 else 0)

    def _filled(self):
        for c in self.ctxs:
            _after_fill(c)

    def _set(self, X, state):
        """distribute the particles X ((3,N), global index space) with ids 0 … N−1 to their owners, in id order"""
        own = owner_ranks(X, self.dims, self.n_loc)
        self.n = int(X.shape[1])
        self.owner0 = own
        self.X, self.state, self.ids, self.U = [], [], [], []
        for l, dev in enumerate(self.devices):
            mine = np.nonzero(own == l)[0]
            cap = self._room(mine.size)
            Xl = np.full((3, cap), np.nan)
            Xl[:, :mine.size] = X[:, mine]
            sl = np.zeros(cap, dtype=np.uint8)
            sl[:mine.size] = state[mine]
            il = np.full(cap, -1, dtype=np.int64)
            il[:mine.size] = mine
            self.X.append(torch.from_numpy(Xl).to(dev))
            self.state.append(torch.from_numpy(sl).to(dev))
            self.ids.append(torch.from_numpy(il).to(dev))
            self.U.append(torch.full((3, cap), float("nan"), dtype=torch.float64, device=dev) if self.keep_velocity else None)
        self._filled()

    def caps(self):
        return [int(s.numel()) for s in self.state]

    def _grow(self, l, extra):
        """`extra` (+ slack) more empty slots at the end of local rank l's arrays; host-side torch ops, not on the hot path"""
        add = self._room(extra) if extra else 0
        if add <= 0:
            return
        dev = self.devices[l]
        self.X[l] = torch.cat([self.X[l], torch.full((3, add), float("nan"), dtype=torch.float64, device=dev)], dim=1).contiguous()
        self.state[l] = torch.cat([self.state[l], torch.zeros(add, dtype=torch.uint8, device=dev)])
        self.ids[l] = torch.cat([self.ids[l], torch.full((add,), -1, dtype=torch.int64, device=dev)])
        if self.keep_velocity:
            self.U[l] = torch.cat([self.U[l], torch.full((3, add), float("nan"), dtype=torch.float64, device=dev)], dim=1).contiguous()
        self.grown += 1

    # ---- seeding: as Tracers on the global shape -------------------------------------------------------------------------
    def to_index(self, xyz):
        return self._host.to_index(xyz)

    def seed_points(self, xyz):
        """Replace the particle set by the physical points xyz (N,3); points outside the closed global box start dead.  The host
        assigns every point to the rank that owns it; ids are the rows of xyz."""
        X = self.to_index(xyz)
        self._set(X, self._host._inside(X).astype(np.uint8))
        self.steps = self.moved = 0
        return self

    def seed_random(self, n, seed=0):
        """n points uniform in the global box: the same X as Tracers(global shape).seed_random(n, seed)"""
        rng = np.random.Generator(np.random.MT19937(int(seed)))
        X = rng.uniform(0.0, 1.0, size=(3, int(n))) * np.asarray(self.shape, dtype=np.float64).reshape(3, 1)
        self._set(X, np.ones(int(n), dtype=np.uint8))
        self.steps = self.moved = 0
        return self

    # ---- the step --------------------------------------------------------------------------------------------------------
    def _mg(self):
        mg = getattr(self.grid, "mg", None)
        if mg is None or any(c is None for c in self.ctxs):
            raise L.Ns3dError("MgpuTracers.advance / sample need a mgpu.MgpuGrid: navierstokes3d_amd has no CPU path")
        return mg

    def migrate(self):
        """ns3d_tracers_migrate_mgpu; a rank that runs short of empty slots gets larger arrays and the call is repeated (the rule is
        a pure function of the positions).  Returns the number of particles moved."""
        mg = self._mg()
        U = self.U if self.keep_velocity else None
        moved, need = mg.tracers_migrate(self.X, self.state, self.ids, U)
        if need is not None:
            mg.sync()
            for l, k in enumerate(need):
                self._grow(l, k)
            self._filled()
            moved, need = mg.tracers_migrate(self.X, self.state, self.ids, U)
            if need is not None:
                raise L.Ns3dError("ns3d_tracers_migrate_mgpu: still short of slots after growing: %r" % (need,))
        self.moved += moved
        return moved

    def advance(self, fs, dt):
        """One explicit-midpoint step of every live particle through the frozen fields fs[l].Vx, .Vy, .Vz of the local ranks, then the
        particles that crossed a seam travel to their owners.  P ranks reproduce the one-rank step bit for bit while the first-stage
        Courant number stays below 1 in the decomposed directions (include/ns3d.h)."""
        mg = self._mg()
        if self.n:
            cx, cy, cz = (float(dt) / d for d in self.spacings)
            mg.tracers_advance(self.X, self.state, [f.Vx for f in fs], [f.Vy for f in fs], [f.Vz for f in fs], cx, cy, cz,
                               U=self.U if self.keep_velocity else None)
            self.migrate()
        self.steps += 1

    def sample(self, A, stagger=(0, 0, 0)):
        """The per-rank field A (a list) at the particles' positions (ns3d_sample_at): one (cap,) float64 device array per rank, NaN
        in dead and empty slots; by_id() brings such a list into id order on the host."""
        self._mg()
        outs = []
        for l, c in enumerate(self.ctxs):
            out = torch.empty(self.state[l].numel(), dtype=torch.float64, device=self.devices[l])
            if out.numel():
                K.sample_at(A[l], self.X[l], out, state=self.state[l], stagger=stagger, origin=self.origins[l], ctx=c)
            outs.append(out)
        return outs

    # ---- read-backs, ordered by id ----------------------------------------------------------------------------------------
    def _sync(self):
        mg = getattr(self.grid, "mg", None)
        if mg is not None:
            mg.sync()

    def by_id(self, per_rank):
        """per-rank slot arrays (the last dimension runs over the slots) → one host array whose last dimension runs over the ids"""
        self._sync()
        ids = [t.cpu().numpy() for t in self.ids]
        vals = [np.asarray(t.cpu().numpy()) for t in per_rank]
        out = np.full(vals[0].shape[:-1] + (self.n,), np.nan, dtype=vals[0].dtype) if vals[0].dtype.kind == "f" else \
            np.zeros(vals[0].shape[:-1] + (self.n,), dtype=vals[0].dtype)
        seen = np.zeros(self.n, dtype=np.int64)
        for i, v in zip(ids, vals):
            occ = i >= 0
            out[..., i[occ]] = v[..., occ]
            np.add.at(seen, i[occ], 1)
        if not np.all(seen == 1):
            raise L.Ns3dError("particle ids are not a permutation of the slots' contents (%d ids, %d held once)"
                              % (self.n, int(np.sum(seen == 1))))
        return out

    def index_positions(self):
        """(3, N) global index-space coordinates on the host, by id"""
        return self.by_id(self.X)

    def positions(self):
        """(N,3) physical coordinates on the host, by id: origin + ξ·d"""
        X = self.index_positions()
        return np.stack([self.origin[q] + X[q] * self.spacings[q] for q in range(3)], axis=1)

    def alive(self):
        """(N,) bool on the host, by id"""
        return self.by_id(self.state) == 1

    def velocities(self):
        """(3, N) on the host, by id: the velocity at the start points of the latest step (keep_velocity)"""
        return self.by_id(self.U)

    def record(self):
        """x, y, z (physical), alive, steps, ORDERED BY id — comparable with a one-rank Tracers.record() of the same seeding"""
        P = self.positions()
        return SimpleNamespace(x=P[:, 0].copy(), y=P[:, 1].copy(), z=P[:, 2].copy(), alive=self.alive(), steps=self.steps)

    def sort_by_cell(self):
        """Tracers.sort_by_cell per rank (empty slots last); the ids follow, because they are stored.  Returns the per-rank
        permutations."""
        self._sync()
        perms = []
        for l in range(len(self.X)):
            t = Tracers(self.shape, None, self.spacings, self.origin)
            t.X = self.X[l]
            perm = torch.sort(t.cell_keys(), stable=True).indices
            self.X[l] = self.X[l][:, perm].contiguous()
            self.state[l] = self.state[l][perm].contiguous()
            self.ids[l] = self.ids[l][perm].contiguous()
            if self.keep_velocity:
                self.U[l] = self.U[l][:, perm].contiguous()
            perms.append(perm)
        self._filled()
        return perms

    save_bins = staticmethod(Tracers.save_bins)


class MgpuProbes:
    """`Probes` on a decomposed grid: every point is assigned ONCE, on the host, to the rank that owns it; per step every rank that
    holds points makes four ns3d_sample_at calls into its own (4, nt, m_l) series on its device.  gathered() returns (nt, M) arrays
    in the caller's point order — the bits of Probes on the global field."""

    def __init__(self, grid, spacings, origin, xyz, nt):
        self.grid = grid
        self.n_loc, self.dims, self.shape, self.origins, self.ctxs = _grid_geometry(grid)
        if any(c is None for c in self.ctxs):
            raise L.Ns3dError("MgpuProbes needs a mgpu.MgpuGrid: navierstokes3d_amd has no CPU path")
        X = Tracers(self.shape, None, spacings, origin).to_index(xyz)
        own = owner_ranks(X, self.dims, self.n_loc)
        self.m, self.nt = int(X.shape[1]), max(int(nt), 0)
        self.index, self.X, self.series = [], [], []
        for l, c in enumerate(self.ctxs):
            mine = np.nonzero(own == l)[0]
            dev = torch.device("cuda", c.device)
            self.index.append(mine)
            self.X.append(torch.from_numpy(np.ascontiguousarray(X[:, mine])).to(dev))
            self.series.append(torch.full((4, self.nt, mine.size), float("nan"), dtype=torch.float64, device=dev))
            _after_fill(c)
        self.steps = 0

    def record(self, fs):
        """sample the four fields of the current state (fs: one namespace of fields per local rank) into row `steps`; enqueues only"""
        for l, c in enumerate(self.ctxs):
            if self.index[l].size:
                for q, (_, field, stag) in enumerate(PROBE_FIELDS):
                    K.sample_at(getattr(fs[l], field), self.X[l], self.series[l][q, self.steps], stagger=stag, origin=self.origins[l], ctx=c)
        self.steps += 1

    def gathered(self):
        """u, v, w, p as (nt, M) host arrays in the caller's point order"""
        self.grid.mg.sync()
        host = np.full((4, self.nt, self.m), np.nan)
        for mine, s in zip(self.index, self.series):
            host[:, :, mine] = s.cpu().numpy()
        return SimpleNamespace(**{name: host[q] for q, (name, _, _) in enumerate(PROBE_FIELDS)})
