"""The definitions of ns3d_voxelize, ns3d_set_solid and ns3d_solid_momentum (include/ns3d.h) as vectorised NumPy, fp64, written from
the header's text and not from the kernels.  voxelize() evaluates every (triangle, row) pair of a row family at once — no bounding-box
shortcut, no bit planes — so it shares nothing with the device's scatter / prefix design but the stated comparisons."""
import math

import numpy as np

BIT_C, BIT_X, BIT_Y, BIT_Z = 1, 2, 4, 8
# row families: (stagger of the row in y, in z, [(bit, s, ext − nx)])
FAMILIES = (
    (0.5, 0.5, ((BIT_C, 0.5, 0), (BIT_X, 0.0, 1))),
    (0.0, 0.5, ((BIT_Y, 0.5, 0),)),
    (0.5, 0.0, ((BIT_Z, 0.5, 0),)),
)


def as_tri9(tri):
    """(n,3,3) or (n,9) or flat → (n,9) float64: x0,y0,z0,x1,y1,z1,x2,y2,z2 per triangle, the layout ns3d_isosurface writes"""
    return np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 9)


def side(py, pz, qy, qz, ry, rz):
    """side(p, q, r) of the header on the yz-projections; p, q broadcast against the rows r"""
    swap = (qy < py) | ((qy == py) & (qz < pz))
    ay, az = np.where(swap, qy, py), np.where(swap, qz, pz)
    by, bz = np.where(swap, py, qy), np.where(swap, pz, qz)
    dy, dz = by - ay, bz - az
    E = dy * (rz - az) - dz * (ry - ay)
    tie = np.where(dz > 0, -1, np.where(dz < 0, 1, np.where(dy > 0, 1, 0)))
    s = np.where(E > 0, 1, np.where(E < 0, -1, tie))
    return np.where(swap, -s, s)


def _family_flips(t9, Y, Z, families, nx, ox, chunk=2048):
    """for the rows (Y[r], Z[r]): per (bit, s, ext) of `families` an int array (rows, ext+1) of flip counts at i0"""
    out = [np.zeros((Y.size, nx + dext + 1), dtype=np.int64) for _, _, dext in families]
    ry, rz = Y[None, :], Z[None, :]
    for lo in range(0, t9.shape[0], chunk):
        t = t9[lo:lo + chunk]
        ax, ay, az, bx, by, bz, cx, cy, cz = (t[:, q:q + 1] for q in range(9))
        with np.errstate(all="ignore"):
            finite = np.isfinite(t).all(axis=1)[:, None]
            miny, maxy = np.minimum(np.minimum(ay, by), cy), np.maximum(np.maximum(ay, by), cy)
            minz, maxz = np.minimum(np.minimum(az, bz), cz), np.maximum(np.maximum(az, bz), cz)
            box = (miny <= ry) & (ry <= maxy) & (minz <= rz) & (rz <= maxz)
            s1, s2, s3 = side(ay, az, by, bz, ry, rz), side(by, bz, cy, cz, ry, rz), side(cy, cz, ay, az, ry, rz)
            cover = finite & box & (s1 == s2) & (s2 == s3) & (s1 != 0)
            ux, uy, uz = bx - ax, by - ay, bz - az
            vx, vy, vz = cx - ax, cy - ay, cz - az
            n_x, n_y, n_z = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
            xs = ax - (n_y * (ry - ay) + n_z * (rz - az)) / n_x
            hit = cover & (n_x != 0) & np.isfinite(xs)
            tt, rr = np.nonzero(hit)
            x = xs[tt, rr]
            for (bit, s, dext), acc in zip(families, out):
                ext = nx + dext
                tv = x - (float(ox) + s)
                i0 = np.where(tv <= 0, 0, np.where(tv >= ext, ext, np.ceil(np.clip(tv, 0, ext)))).astype(np.int64)
                np.add.at(acc, (rr, i0), 1)
    return out


def voxelize(tri, nx, ny, nz, origin=None):
    """the mask of ns3d_voxelize: uint8, shape (nx+1, ny+1, nz+1), Fortran order"""
    t9 = as_tri9(tri)
    ox, oy, oz = (0, 0, 0) if origin is None else (int(q) for q in origin)
    mask = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    J, K = np.meshgrid(np.arange(ny + 1), np.arange(nz + 1), indexing="ij")
    J, K = J.ravel(), K.ravel()
    for sy, sz, fams in FAMILIES:
        valid = (J < (ny if sy else ny + 1)) & (K < (nz if sz else nz + 1))
        j, k = J[valid], K[valid]
        Y = (j + oy).astype(np.float64) + sy
        Z = (k + oz).astype(np.float64) + sz
        for (bit, s, dext), acc in zip(fams, _family_flips(t9, Y, Z, fams, nx, ox)):
            ext = nx + dext
            inside = (np.cumsum(acc, axis=1)[:, :ext] & 1).astype(np.uint8)      # every sample i >= i0 flips
            mask[:ext, j, k] |= (inside * bit).T
    return mask


def set_solid(C, Vx, Vy, Vz, mask):
    """ns3d_set_solid in place on host arrays; bits at invalid points are ignored.  C may be None."""
    nx, ny, nz = Vz.shape[0], Vz.shape[1], Vz.shape[2] - 1
    m = np.asarray(mask).reshape((nx + 1, ny + 1, nz + 1), order="F")
    if C is not None:
        C[(m[:nx, :ny, :nz] & BIT_C) != 0] = 1
    Vx[(m[:, :ny, :nz] & BIT_X) != 0] = 0
    Vy[(m[:nx, :, :nz] & BIT_Y) != 0] = 0
    Vz[(m[:nx, :ny, :] & BIT_Z) != 0] = 0


def owned(n, s, seam_lo, seam_hi):
    """ns3d_diagnostics' owned 0-based range of an extent n+s"""
    return slice(1 + s if seam_lo else 0, n + s - 1 if seam_hi else n + s)


def momentum_terms(Vx, Vy, Vz, mask, seam_lo=(0, 0, 0), seam_hi=(0, 0, 0)):
    """per direction the fp64 values of the owned nodes whose mask bit is set (what ns3d_solid_momentum sums and counts)"""
    nx, ny, nz = Vz.shape[0], Vz.shape[1], Vz.shape[2] - 1
    n = (nx, ny, nz)
    m = np.asarray(mask).reshape((nx + 1, ny + 1, nz + 1), order="F")
    out = []
    for q, (V, bit) in enumerate(((Vx, BIT_X), (Vy, BIT_Y), (Vz, BIT_Z))):
        sl = tuple(owned(n[d], 1 if d == q else 0, seam_lo[d], seam_hi[d]) for d in range(3))
        ext = tuple(n[d] + (1 if d == q else 0) for d in range(3))
        sel = (m[:ext[0], :ext[1], :ext[2]][sl] & bit) != 0
        out.append(np.asarray(V)[sl][sel].astype(np.float64))
    return out


def momentum(Vx, Vy, Vz, mask, seam_lo=(0, 0, 0), seam_hi=(0, 0, 0)):
    """(sums by math.fsum, counts, Σ|term|) per direction"""
    terms = momentum_terms(Vx, Vy, Vz, mask, seam_lo, seam_hi)
    return ([math.fsum(t.tolist()) for t in terms], [int(t.size) for t in terms], [math.fsum(np.abs(t).tolist()) for t in terms])
