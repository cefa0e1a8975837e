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
