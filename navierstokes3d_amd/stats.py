"""Host side of ns3d_stats_* (include/ns3d.h): the running sums behind the time-averaged fields — mean velocity and pressure,
the Reynolds stresses u'u' … v'w', the pressure variance.  Every number is formed on the device by libns3d (one fused pass per
sample, ns3d_stats_accumulate; ns3d_stats_finalize at the end); this module owns the state arrays, counts the samples and
gathers the result through the grid.  PyTorch does no arithmetic here."""
from types import SimpleNamespace

import torch

from . import kernels as K
from . import lib as L

# slot order of the state S, as the header's enum NS3D_STATS_* publishes it
SLOTS = ("u", "v", "w", "p", "uu", "vv", "ww", "uv", "uw", "vw", "pp")
MEAN = ("U", "V", "W", "P")                                  # blocks of ns3d_stats_finalize's `mean`
RS = ("uu", "vv", "ww", "uv", "uw", "vw", "pp")               # blocks of its `rs`


def bytes_per_cell(dtype=torch.float64, with_pr=True):
    """NOMINAL memory traffic of one ns3d_stats_accumulate call per cell, the accounting the rates are quoted in: one read of each
    field, one load and one store of each accumulator (fp64 whatever the fields are) — 208 / 192 bytes for fp64 / fp32 fields.
    Without Pr the nominal figure drops the Pr read and ONE accumulator's load and store: 184 / 172.  That is the accounting this
    interface was specified with; it is 16 bytes above what the kernel then moves, because the call leaves BOTH slots p and pp
    alone — bytes_moved_per_cell gives that figure (168 / 156).  With Pr the two agree."""
    nfields, nslots = (4, len(SLOTS)) if with_pr else (3, len(SLOTS) - 1)
    return nfields * K.ESIZE[dtype] + nslots * 2 * 8


def bytes_moved_per_cell(dtype=torch.float64, with_pr=True):
    """What k_stats reads and writes per cell: the fields it reads once and a load and a store of every slot it touches — all
    eleven with Pr (208 / 192 bytes), nine without (slots p and pp are neither read nor written: 168 / 156 bytes)."""
    nfields, nslots = (4, len(SLOTS)) if with_pr else (3, len(SLOTS) - 2)
    return nfields * K.ESIZE[dtype] + nslots * 2 * 8


def _blocks(t, n):
    """the n (nx,ny,nz) blocks of a (nx,ny,n·nz) column-major array, as views"""
    nz = t.shape[2] // n
    return [t[:, :, q * nz:(q + 1) * nz] for q in range(n)]


class RunningStats:
    """The state of a run's statistics: one S per local rank (on that rank's device), the number of samples n and the sum of
    their weights.  `shape` = (nx, ny, nz) of a rank's cell-centred arrays, `ctxs` = one kernels.Context per local rank."""

    def __init__(self, shape, ctxs):
        self.shape = tuple(int(q) for q in shape)
        self.ctxs = list(ctxs)
        nx, ny, nz = self.shape
        self.S = [K.zeros((nx, ny, nz * len(SLOTS)), torch.float64, torch.device("cuda", c.device)) for c in self.ctxs]
        self.n, self.wsum = 0, 0.0
        self._after_alloc()
        self.reset()

    def _after_alloc(self):
        for c in self.ctxs:
            c.after_torch_fill()

    def reset(self):
        for S, c in zip(self.S, self.ctxs):
            K.stats_reset(S, self.shape, ctx=c)
        self.n, self.wsum = 0, 0.0

    def sample(self, fs, weight=1.0):
        """One sample of every local rank's fields (`fs`: one namespace with Vx, Vy, Vz, Pr per local rank)."""
        for S, f, c in zip(self.S, fs, self.ctxs):
            K.stats_accumulate(S, f.Vx, f.Vy, f.Vz, f.Pr, weight, ctx=c)
        self.n += 1
        self.wsum += float(weight)

    def finalize(self):
        """(mean, rs) per local rank: device arrays of 4 resp. 7 blocks.  Needs at least one sample."""
        if not self.wsum > 0.0:
            raise L.Ns3dError("statistics: no samples were taken (sum of weights = %r)" % (self.wsum,))
        nx, ny, nz = self.shape
        out = []
        for c in self.ctxs:
            dev = torch.device("cuda", c.device)
            out.append((K.zeros((nx, ny, 4 * nz), torch.float64, dev), K.zeros((nx, ny, 7 * nz), torch.float64, dev)))
        self._after_alloc()
        for S, c, (mean, rs) in zip(self.S, self.ctxs, out):
            K.stats_finalize(S, self.wsum, mean, rs, self.shape, ctx=c)
        return out

    def _record(self, mean, rs):
        return SimpleNamespace(n=self.n, wsum=self.wsum, mean=SimpleNamespace(**dict(zip(MEAN, mean))),
                               rs=SimpleNamespace(**dict(zip(RS, rs))))

    def local(self, l=0):
        """The record of local rank l's full arrays (halo and boundary cells included) as host arrays."""
        mean, rs = self.finalize()[l]
        self.ctxs[l].sync()
        return self._record([K.to_numpy(b) for b in _blocks(mean, 4)], [K.to_numpy(b) for b in _blocks(rs, 7)])

    def gathered(self, grid):
        """The record of the GLOBAL, halo-stripped statistics on the root (entries None elsewhere), gathered like the fields
        (multi.jl:399-403): grid.gather_fields."""
        fin = self.finalize()
        for c in self.ctxs:
            c.sync()
        per_block = lambda which, n: [grid.gather_fields([_blocks(f[which], n)[q] for f in fin]) for q in range(n)]
        return self._record(per_block(0, 4), per_block(1, 7))
