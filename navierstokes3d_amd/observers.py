"""The drivers' read-only observers of a running flow — the keywords statistics / stats_every, vortex, tracers, probes and
isosurface of run_navierstokes3D and runme (driver.py has their description) — behind one object with one call per place a time
loop touches them: start, end_step, frame, finish.  Everything here reads the flow and writes arrays of its own: with every keyword
off, not one library call is made.  (`diagnostics` is not here: its three calls are positions inside the step, driver.py.)"""
import os
from types import SimpleNamespace

import numpy as np

from . import isosurface as ISO
from . import lib as L
from .stats import RunningStats
from .tracers import MgpuProbes, MgpuTracers, Probes, Tracers
from .vis import save_frame_tracers, save_frame_vortex
from .vortex import NAMES as _VORTEX_NAMES, VortexFields, save_bins as _save_vortex_bins

ISO_FIELDS = ("Q", "Wx", "Wy", "Wz", "Pr", "C")


def check_options(grid, statistics, stats_every, vortex, tracers, probes, isosurface):
    """The keywords' checks, for a run on `grid`: they need no device and come before anything is allocated or enqueued."""
    P, nlocal = grid.P, len(grid.local_ranks)
    if statistics is not None and (int(statistics) != statistics or statistics < 1):
        raise L.Ns3dError("statistics = %r (None, or the first step to sample: an integer >= 1)" % (statistics,))
    if int(stats_every) != stats_every or stats_every < 1:
        raise L.Ns3dError("stats_every = %r (an integer >= 1)" % (stats_every,))
    for name, val, one, many in (("tracers", tracers, Tracers, MgpuTracers), ("probes", probes, Probes, MgpuProbes)):
        if isinstance(val, many):
            if val.grid is not grid:
                raise L.Ns3dError("%s= is a %s of another grid than the run's" % (name, many.__name__))
        elif val is not None and P > 1:
            raise L.Ns3dError("%s= as a number or an array runs on one rank only (this grid has %d): particles that cross a seam "
                              "between ranks have to migrate — build a tracers.MgpuTracers / tracers.MgpuProbes on the grid (the "
                              "one-process form) and pass that object" % (name, P))
    if _iso_spec(isosurface) is not None and nlocal != P:
        raise L.Ns3dError("isosurface= needs every rank in this process (one rank, or a mgpu.MgpuGrid in the one-process form): "
                          "this process drives %d of %d ranks" % (nlocal, P))


def _iso_spec(isosurface):
    """(field, level, color) of the drivers' `isosurface=` keyword, None when it is off"""
    if isosurface is None:
        return None
    if isinstance(isosurface, dict):
        unknown = set(isosurface) - {"field", "level", "color"}
        if unknown or "level" not in isosurface:
            raise L.Ns3dError("isosurface = %r (a dict with field, level and optionally color)" % (isosurface,))
        field, level, color = isosurface.get("field", "Q"), isosurface["level"], isosurface.get("color")
    elif isinstance(isosurface, (int, float, np.integer, np.floating)) and not isinstance(isosurface, bool):
        field, level, color = "Q", isosurface, None
    else:
        raise L.Ns3dError("isosurface = %r (a level of the Q-criterion, or a dict with field, level and optionally color)" % (isosurface,))
    if field not in ISO_FIELDS or (color is not None and color not in ISO_FIELDS):
        raise L.Ns3dError("isosurface: field = %r, color = %r (each one of %s)" % (field, color, ", ".join(ISO_FIELDS)))
    if not np.isfinite(float(level)):
        raise L.Ns3dError("isosurface: level = %r is not finite" % (level,))
    return field, float(level), color


class _IsoObserver:
    """The drivers' `isosurface=` keyword: one isosurface.extract per local rank over the cubes that rank owns, concatenated in rank
    order.  Q, Wx, Wy, Wz come from the run's VortexFields (`vort`) or from a scratch set of this observer's own."""

    def __init__(self, spec, shape, ctxs, p, grid, vort, dtype):
        self.field, self.level, self.color = spec
        self.shape, self.ctxs, self.p, self.grid = tuple(shape), list(ctxs), p, grid
        self.derived = [n for n in (self.field, self.color) if n in _VORTEX_NAMES]
        self.vort = vort
        if self.derived and vort is None:
            self.vort = VortexFields(shape, ctxs, (p.dx, p.dy, p.dz), dtype)

    def _array(self, name, l, fs):
        if name is None:
            return None
        return getattr(self.vort.out[l], name) if name in _VORTEX_NAMES else getattr(fs[l], name)

    def extract(self, fs, computed=False):
        """the surface of the state in `fs` (one namespace of fields per local rank); computed: self.vort holds this state's fields"""
        n, dims = self.shape, self.grid.dims
        if self.derived:
            if not computed:
                self.vort.compute(fs)
            if len(fs) > 1:     # a seam's cubes need the neighbour's values in the halo cells, which ns3d_vortex leaves +0.0
                self.grid.update_halo(*[[getattr(o, nm) for o in self.vort.out] for nm in dict.fromkeys(self.derived)])
        pieces = []
        for l, c in enumerate(self.ctxs):
            co = self.grid.local_coords[l]
            lo = [0 if co[q] == 0 else 1 for q in range(3)]
            hi = [n[q] - 1 for q in range(3)]
            if self.derived:    # the global grid's outermost cells are +0.0 by ns3d_vortex's contract, not flow
                lo = [1, 1, 1]
                hi = [n[q] - 2 if co[q] == dims[q] - 1 else n[q] - 1 for q in range(3)]
            pieces.append(ISO.extract(c, self._array(self.field, l, fs), self.level, color=self._array(self.color, l, fs), box=lo + hi,
                                      origin=[co[q] * (n[q] - 2) for q in range(3)], spacings=(self.p.dx, self.p.dy, self.p.dz),
                                      low_corner=(-self.p.lx / 2, -self.p.ly / 2, -self.p.lz / 2)))
        return ISO.concat(pieces)


class Observers:
    """What a run observes, built once from the drivers' keywords.  `grid`: the run's grid (its ranks, coordinates and gather);
    `ctxs`: one context per local rank; `p`: the parameter record (spacings, box, dt); `gathered`: how the two drivers differ —
      True   run_navierstokes3D: frames and results are gathered through the grid, the root writes the files, out_<F>_v_%04d.bin
             included;
      False  runme: the one rank's full local arrays, gpu.jl's file names, no vortex .bin (its MAT files stay the reference's)."""

    def __init__(self, grid, ctxs, p, nt, dtype, gathered, statistics, stats_every, vortex, tracers, probes, isosurface):
        self.grid, self.ctxs, self.p, self.gathered = grid, list(ctxs), p, gathered
        self.shape = (p.nx, p.ny, p.nz)
        self.first, self.every, self.running = statistics, stats_every, None
        spacings, origin = (p.dx, p.dy, p.dz), (-p.lx / 2, -p.ly / 2, -p.lz / 2)    # the box's low corner in both scripts
        self.vort = VortexFields(self.shape, ctxs, spacings, dtype) if vortex else None
        self.trc = self.prb = None
        if isinstance(tracers, (Tracers, MgpuTracers)):
            self.trc = tracers                      # a ready object is used as it is
        elif tracers is not None:
            self.trc = Tracers(self.shape, ctxs[0], spacings, origin)
            if isinstance(tracers, (int, np.integer)) and not isinstance(tracers, bool):
                if tracers < 0:
                    raise L.Ns3dError("tracers = %r (a number of particles >= 0, or an (N,3) array of start points)" % (tracers,))
                self.trc.seed_random(int(tracers), 0)
            else:
                self.trc.seed_points(tracers)
        if isinstance(probes, (Probes, MgpuProbes)):
            self.prb = probes
        elif probes is not None:
            self.prb = Probes(self.shape, ctxs[0], spacings, origin, probes, nt)
        self.iso = _IsoObserver(_iso_spec(isosurface), self.shape, ctxs, p, grid, self.vort, dtype) if isosurface is not None else None

    def start(self):
        """The time loop begins: the statistics' sums are allocated and zeroed here, after the initial frame."""
        if self.first is not None:
            self.running = RunningStats(self.shape, self.ctxs)

    def end_step(self, it, fs):
        """End of time step `it`, after its last halo update: the statistics' sample if one is due, then the particles move through
        the step's final velocity field, then the probes sample the final state."""
        if self.running is not None and it >= self.first and (it - self.first) % self.every == 0:
            self.running.sample(fs)
        if self.trc is not None:            # the Mgpu objects take every local rank's fields, the one-rank objects the one rank's
            self.trc.advance(fs if isinstance(self.trc, MgpuTracers) else fs[0], self.p.dt)
        if self.prb is not None:
            self.prb.record(fs if isinstance(self.prb, MgpuProbes) else fs[0])

    def frame(self, fs, save=None, vis=None):
        """The observers' files of a frame of the state in `fs`: `save` / `vis` number the dumps resp. the pictures, None where the
        driver writes none of that kind now."""
        root = self.grid.is_root()
        if self.vort is not None and (self.gathered or vis is not None):
            self.vort.compute(fs)
            rec = self.vort.gathered(self.grid) if self.gathered else self.vort.local(0)
            if root and self.gathered and save is not None:
                _save_vortex_bins(rec, save)
            if root and vis is not None:
                n_g = [d * (n - 2) + 2 for d, n in zip(self.grid.dims, self.shape)]
                save_frame_vortex(rec, n_g[1], n_g[2], vis, gpu_names=not self.gathered)
        if self.trc is not None:
            rec = self.trc.record()
            if save is not None:
                Tracers.save_bins(rec, save)
            if vis is not None:
                save_frame_tracers(rec, self.p.lx, self.p.ly, vis)
        if self.iso is not None and save is not None:
            surface = self.iso.extract(fs)
            if root:
                os.makedirs("./out_save", exist_ok=True)
                surface.save_ply("out_save/out_iso_%04d.ply" % save)

    def finish(self, info, fs):
        """After the last step: info.stats, info.vortex, info.isosurface, info.tracers, info.probes of the keywords that are on."""
        if self.running is not None:
            info.stats = SimpleNamespace(n=0, wsum=0.0, mean=None, rs=None)
            if self.running.n:
                info.stats = self.running.gathered(self.grid) if self.gathered else self.running.local(0)
        if self.vort is not None:
            self.vort.compute(fs)
            info.vortex = self.vort.gathered(self.grid) if self.gathered else self.vort.local(0)
        if self.iso is not None:
            info.isosurface = self.iso.extract(fs, computed=self.vort is not None)
        if self.trc is not None:
            info.tracers = self.trc.record()
        if self.prb is not None:
            info.probes = self.prb.gathered()
