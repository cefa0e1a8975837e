"""Reference of ns3d_vortex (include/ns3d.h): the NumPy expression of the header, with every scalar cast to the arrays' dtype, and
the same expression on running_error.Pair values for the FAST bound.  Helper of tests/test_vortex_host.py and
tests/test_gpu_vortex.py."""
import numpy as np

import running_error as RE

NAMES = ("Wx", "Wy", "Wz", "Q")
I = (slice(1, -1),) * 3


def _interior(Vx, Vy, Vz, h, dx, dy, dz):
    """(Wx, Wy, Wz, Q) on the interior cells; works on ndarrays (h, dx, dy, dz scalars of their dtype) and on Pairs alike"""
    u = h * (Vx[:-1] + Vx[1:])
    v = h * (Vy[:, :-1] + Vy[:, 1:])
    w = h * (Vz[:, :, :-1] + Vz[:, :, 1:])
    gxx = ((Vx[1:] - Vx[:-1]) / dx)[I]
    gyy = ((Vy[:, 1:] - Vy[:, :-1]) / dy)[I]
    gzz = ((Vz[:, :, 1:] - Vz[:, :, :-1]) / dz)[I]
    uy = h * ((u[1:-1, 2:, 1:-1] - u[1:-1, :-2, 1:-1]) / dy)
    uz = h * ((u[1:-1, 1:-1, 2:] - u[1:-1, 1:-1, :-2]) / dz)
    vx = h * ((v[2:, 1:-1, 1:-1] - v[:-2, 1:-1, 1:-1]) / dx)
    vz = h * ((v[1:-1, 1:-1, 2:] - v[1:-1, 1:-1, :-2]) / dz)
    wx = h * ((w[2:, 1:-1, 1:-1] - w[:-2, 1:-1, 1:-1]) / dx)
    wy = h * ((w[1:-1, 2:, 1:-1] - w[1:-1, :-2, 1:-1]) / dy)
    Q = ((-h) * ((gxx * gxx + gyy * gyy) + gzz * gzz)) - ((uy * vx + uz * wx) + vz * wy)
    return wy - vz, uz - wx, vx - uy, Q


def reference(Vx, Vy, Vz, dx, dy, dz):
    """{name: (nx,ny,nz) array of the fields' dtype}: the interior values, +0.0 everywhere else"""
    T = Vx.dtype.type
    assert Vy.dtype == Vx.dtype and Vz.dtype == Vx.dtype
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    with np.errstate(all="ignore"):
        vals = _interior(Vx, Vy, Vz, T(0.5), T(dx), T(dy), T(dz))
    out = {}
    for n, a in zip(NAMES, vals):
        assert a.dtype == Vx.dtype
        full = np.zeros((nx, ny, nz), dtype=Vx.dtype, order="F")
        full[I] = a
        out[n] = full
    return out


def reference_pairs(Vx, Vy, Vz, dx, dy, dz):
    """{name: Pair of shape (nx,ny,nz)}: value in fp64 and running-error bound of the same expression in the fields' dtype; the
    spacings are divisors marked with spacing() (charged the reciprocal's three roundings).  Boundary entries: value 0, bound 0."""
    dt = Vx.dtype
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    vals = _interior(RE.field(Vx), RE.field(Vy), RE.field(Vz), 0.5, RE.spacing(dx, dt), RE.spacing(dy, dt), RE.spacing(dz, dt))
    out = {}
    for n, p in zip(NAMES, vals):
        full = RE.Pair(np.zeros((nx, ny, nz), order="F"), None, RE.unit(dt))
        full[I] = p
        out[n] = full
    return out


def linear_flow(G, shape, dtype, spacings=(0.25, 0.5, 0.125)):
    """Staggered Vx, Vy, Vz of the flow V = G·x on a grid of `shape` cells: each component sampled at its own face centres.
    Returns (Vx, Vy, Vz, dx, dy, dz)."""
    nx, ny, nz = shape
    dx, dy, dz = spacings
    G = np.asarray(G, dtype=np.float64)

    def sample(row, sx, sy, sz, ox, oy, oz):
        x = (np.arange(sx) + ox)[:, None, None] * dx
        y = (np.arange(sy) + oy)[None, :, None] * dy
        z = (np.arange(sz) + oz)[None, None, :] * dz
        return np.asfortranarray((G[row, 0] * x + G[row, 1] * y + G[row, 2] * z).astype(dtype))

    return (sample(0, nx + 1, ny, nz, 0.0, 0.5, 0.5), sample(1, nx, ny + 1, nz, 0.5, 0.0, 0.5),
            sample(2, nx, ny, nz + 1, 0.5, 0.5, 0.0), dx, dy, dz)
