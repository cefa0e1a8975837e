"""Host side of ns3d_vortex (include/ns3d.h): the vorticity components Wx, Wy, Wz and the Q-criterion of the flow — what one
looks at in a cylinder wake.  Every number is formed on the device by libns3d (one fused pass over Vx, Vy, Vz per call); this
module owns the output arrays, one set per local rank, and gathers them through the grid.  PyTorch does no arithmetic here."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import kernels as K

NAMES = ("Wx", "Wy", "Wz", "Q")


def bytes_per_cell(dtype=torch.float64, n_out=4):
    """NOMINAL memory traffic of one ns3d_vortex call per cell, the accounting the rates are quoted in: one read of each velocity
    component and one write of each requested output, all of the element type — 56 / 28 bytes for fp64 / fp32 with all four."""
    if not 1 <= int(n_out) <= 4:
        raise ValueError("n_out = %r (1 … 4 outputs)" % (n_out,))
    return (3 + int(n_out)) * K.ESIZE[dtype]


class VortexFields:
    """The output arrays of a run's vortex fields: Wx, Wy, Wz, Q per local rank, on that rank's device.  `shape` = (nx, ny, nz) of a
    rank's cell-centred arrays, `ctxs` = one kernels.Context per local rank, `spacings` = (dx, dy, dz)."""

    def __init__(self, shape, ctxs, spacings, dtype=torch.float64):
        self.shape = tuple(int(q) for q in shape)
        self.ctxs = list(ctxs)
        self.spacings = tuple(float(q) for q in spacings)
        self.out = [SimpleNamespace(**{n: K.zeros(self.shape, dtype, torch.device("cuda", c.device)) for n in NAMES}) for c in self.ctxs]
        for c in self.ctxs:
            c.after_torch_fill()
        self.n = 0                  # calls made so far

    def compute(self, fs):
        """One call per local rank on its fields (`fs`: one namespace with Vx, Vy, Vz per local rank).  Enqueues only."""
        for o, f, c in zip(self.out, fs, self.ctxs):
            K.vortex(f.Vx, f.Vy, f.Vz, *self.spacings, Wx=o.Wx, Wy=o.Wy, Wz=o.Wz, Q=o.Q, ctx=c)
        self.n += 1

    def local(self, l=0):
        """Local rank l's full arrays (halo and boundary cells included) as host arrays."""
        self.ctxs[l].sync()
        return SimpleNamespace(**{n: K.to_numpy(getattr(self.out[l], n)) for n in NAMES})

    def gathered(self, grid):
        """The GLOBAL, halo-stripped fields on the root (entries None elsewhere), gathered like the flow's own fields
        (multi.jl:399-403): grid.gather_fields."""
        for c in self.ctxs:
            c.sync()
        return SimpleNamespace(**{n: grid.gather_fields([getattr(o, n) for o in self.out]) for n in NAMES})


def save_bins(rec, iframe, outdir="out_save"):
    """out_<F>_v_%04d.bin (Float32, raw column-major) of the gathered record, beside the drivers' own dumps"""
    os.makedirs(outdir, exist_ok=True)
    out = []
    for n in NAMES:
        path = os.path.join(outdir, "out_%s_v_%04d.bin" % (n, iframe))
        with open(path, "wb") as fh:
            fh.write(np.asfortranarray(getattr(rec, n).astype(np.float32)).tobytes(order="F"))
        out.append(path)
    return out
