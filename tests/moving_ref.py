"""The definitions of ns3d_set_solid_moving, ns3d_solid_momentum_moving and ns3d_mesh_transform (include/ns3d.h) as NumPy, fp64, written
from the header's text and not from the kernels — and the whole step under motion: the CPU statements of the step the suite already
has (oracle/driver_ref.py with obstacle= for both element types, tests/scalar_ref.py::step over oracle/numpy_ref.py for the subgrid
model and the scalar) with the masked store and the re-voxelized mask put where the step puts them.  Both statements mask through
solid_ref.set_solid; `masking` stands a Masking object in its place for the duration of a run, which counts the calls, takes the pose
of the call's step from a list the device run shares, rebuilds the mask (transform, then solid_ref.voxelize) when the pose differs
from the one it holds, and stores the body's velocity."""
import contextlib
import math
from types import SimpleNamespace

import numpy as np

import solid_ref as SR

STAGGER = ((0.0, 0.5, 0.5), (0.5, 0.0, 0.5), (0.5, 0.5, 0.0))       # of the nodes of Vx, Vy, Vz


def split(motion):
    m = [float(v) for v in np.asarray(motion, dtype=np.float64).reshape(-1)]
    assert len(m) == 9
    return m[0:3], m[3:6], m[6:9]


def body_velocity(q, shape, motion, d, origin=None):
    """vb of component q at every node of an array of `shape`, float64: the header's three lines, operation for operation"""
    U, w, c = split(motion)
    o = (0, 0, 0) if origin is None else tuple(int(v) for v in origin)
    I, J, K = np.ogrid[:shape[0], :shape[1], :shape[2]]
    s = STAGGER[q]
    X, Y, Z = (I + o[0]).astype(np.float64) + s[0], (J + o[1]).astype(np.float64) + s[1], (K + o[2]).astype(np.float64) + s[2]
    rx, ry, rz = (X - c[0]) * d[0], (Y - c[1]) * d[1], (Z - c[2]) * d[2]
    if q == 0:
        v = U[0] + (w[1] * rz - w[2] * ry)
    elif q == 1:
        v = U[1] + (w[2] * rx - w[0] * rz)
    else:
        v = U[2] + (w[0] * ry - w[1] * rx)
    return np.broadcast_to(v, shape)


def _bits(mask, n):
    nx, ny, nz = n
    m = np.asarray(mask).reshape((nx + 1, ny + 1, nz + 1), order="F")
    return ((m[:nx, :ny, :nz] & SR.BIT_C) != 0, (m[:, :ny, :nz] & SR.BIT_X) != 0, (m[:nx, :, :nz] & SR.BIT_Y) != 0,
            (m[:nx, :ny, :] & SR.BIT_Z) != 0)


def set_solid_moving(C, Vx, Vy, Vz, mask, motion, d, origin=None):
    """ns3d_set_solid_moving in place on host arrays of either element type: (T)vb where a velocity bit is set, C = 1 where bit 0 is;
    bits at invalid points are ignored.  C may be None."""
    n = (Vz.shape[0], Vz.shape[1], Vz.shape[2] - 1)
    bc, bx, by, bz = _bits(mask, n)
    if C is not None:
        C[bc] = 1
    for q, (V, b) in enumerate(((Vx, bx), (Vy, by), (Vz, bz))):
        V[b] = body_velocity(q, V.shape, motion, d, origin).astype(V.dtype)[b]


def momentum_terms(Vx, Vy, Vz, mask, motion, d, origin=None, seam_lo=(0, 0, 0), seam_hi=(0, 0, 0)):
    """per direction the fp64 terms (double)V − (double)(T)vb of the owned masked nodes: what ns3d_solid_momentum_moving sums"""
    n = (Vz.shape[0], Vz.shape[1], Vz.shape[2] - 1)
    bits = _bits(mask, n)[1:]
    out = []
    for q, (V, b) in enumerate(zip((Vx, Vy, Vz), bits)):
        sl = tuple(SR.owned(n[a], 1 if a == q else 0, seam_lo[a], seam_hi[a]) for a in range(3))
        V = np.asarray(V)
        vb = body_velocity(q, V.shape, motion, d, origin).astype(V.dtype).astype(np.float64)
        out.append((V.astype(np.float64) - vb)[sl][b[sl]])
    return out


def momentum(Vx, Vy, Vz, mask, motion, d, origin=None, seam_lo=(0, 0, 0), seam_hi=(0, 0, 0)):
    """(sums by math.fsum, counts, Σ|term|) per direction, as solid_ref.momentum"""
    terms = momentum_terms(Vx, Vy, Vz, mask, motion, d, origin, seam_lo, seam_hi)
    return ([math.fsum(t.tolist()) for t in terms], [int(t.size) for t in terms], [math.fsum(np.abs(t).tolist()) for t in terms])


def transform(tri, R, pivot, shift, spacing):
    """ns3d_mesh_transform: out_a = (pivot_a + shift_a) + ((R[a][0]·q_x + R[a][1]·q_y) + R[a][2]·q_z)/d_a, q = (p − pivot)·d; any
    triangle layout in, (n,3,3) out"""
    P = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    pivot, shift, d = (np.asarray(v, dtype=np.float64).reshape(3) for v in (pivot, shift, spacing))
    with np.errstate(all="ignore"):
        q = (P - pivot) * d
        out = np.stack([(pivot[a] + shift[a]) + ((R[a, 0] * q[:, 0] + R[a, 1] * q[:, 1]) + R[a, 2] * q[:, 2]) / d[a] for a in range(3)], axis=1)
    return out.reshape(-1, 3, 3)


# ---- the whole step ---------------------------------------------------------------------------------------------------------------------
def motion9(pose):
    """the nine numbers of a pose (R, shift, U, omega, centre): U, omega, centre"""
    return tuple(float(v) for a in pose[2:5] for v in a)


class Masking:
    """What stands in solid_ref.set_solid's place during a run under motion.  poses[s] is the pose of step s (poses[0]: t = 0, used by
    the `pre` maskings a script makes before its time loop); tri the original mesh or None (a fixed mask: only the velocity); mask0 the
    mask of the body as given.  Every step masks twice.  .removed collects solid-momentum results taken right before each store."""

    def __init__(self, poses, tri, mask0, grid, spacing, pre=0):
        self.poses, self.tri, self.grid, self.d, self.pre = poses, tri, tuple(grid), tuple(float(v) for v in spacing), pre
        self.mask = np.array(mask0, order="F")
        self.last = (np.eye(3), np.zeros(3))
        self.calls, self.rebuilt, self.removed, self.masks = 0, 0, [], []

    def __call__(self, C, Vx, Vy, Vz, _mask):
        step = 0 if self.calls < self.pre else (self.calls - self.pre) // 2 + 1
        self.calls += 1
        R, shift, U, omega, centre = self.poses[step]
        if self.tri is not None and not (np.array_equal(R, self.last[0]) and np.array_equal(shift, self.last[1])):
            self.mask = SR.voxelize(transform(self.tri, R, np.asarray(centre) - np.asarray(shift), shift, self.d), *self.grid)
            self.last, self.rebuilt = (R, shift), self.rebuilt + 1
        m9 = motion9(self.poses[step])
        self.removed.append(momentum(Vx, Vy, Vz, self.mask, m9, self.d))
        self.masks.append(self.mask)
        set_solid_moving(C, Vx, Vy, Vz, self.mask, m9, self.d)


@contextlib.contextmanager
def masking(fn):
    real = SR.set_solid
    SR.set_solid = fn
    try:
        yield fn
    finally:
        SR.set_solid = real


def run_oracle(script, dtype, mk, nt, initial, niter_cap, advection="reference", pressure="pt"):
    """oracle/driver_ref.py's run of `script` at nx = 24 (solid_step_cases.run_ref's keywords) with mk, a Masking, where it masks;
    returns (fields by name, info)"""
    from oracle.driver_ref import run_navierstokes3D_ref, runme_ref
    kw = dict(nx=24, nt=nt, faithful=False, dtype=dtype, niter_cap=niter_cap, advection=advection, obstacle=mk.mask.copy(order="F"),
              initial=initial, pressure=pressure)
    with masking(mk), np.errstate(all="ignore"):
        if script == "multi":
            out = run_navierstokes3D_ref(**kw)
            f, info = out[-1].ranks[0], out[-1]
        else:
            f, info = runme_ref(**kw)
    assert mk.calls == mk.pre + 2 * nt
    return f, info


def run_scalar_ref(script, f, p, mk, nt, niter, sca=None, op=None, length=0.0, maccormack=False, pressure="pt", work=np.float64):
    """tests/scalar_ref.py::step nt times on the dict f (float64, in place) with mk, a Masking, where it masks; returns
    ([(iterations, errs)], the last mu_e)"""
    import scalar_ref as SC
    steps, mu_e = [], None
    with masking(mk):
        for _ in range(nt):
            mu_e, done, errs = SC.step(f, p, sca, niter, script, faithful=False, pressure=pressure, work=work, op=op, length=length,
                                       maccormack=maccormack, mask=mk.mask)
            steps.append((done, errs))
    assert mk.calls == 2 * nt
    return steps, mu_e


def circulation(Vx, Vy, d, lo, hi, k):
    """∮ V·dl, counter-clockwise seen from +z, around the rectangle of cells [lo[0], hi[0]) × [lo[1], hi[1]) in the plane of the cell
    centres k: Vx along its two y-faces (interpolated to the faces' lines from the two rows beside them), Vy along its two x-faces"""
    i0, j0 = lo
    i1, j1 = hi
    vx = lambda j: 0.5 * (Vx[i0 + 1:i1, j - 1, k] + Vx[i0 + 1:i1, j, k]).sum() + 0.25 * sum(Vx[i, j - 1, k] + Vx[i, j, k] for i in (i0, i1))
    vy = lambda i: 0.5 * (Vy[i - 1, j0 + 1:j1, k] + Vy[i, j0 + 1:j1, k]).sum() + 0.25 * sum(Vy[i - 1, j, k] + Vy[i, j, k] for j in (j0, j1))
    return float((vx(j0) - vx(j1)) * d[0] + (vy(i1) - vy(i0)) * d[1])

