"""Meshes and expectations shared by tests/test_solid_host.py and tests/test_gpu_solid.py."""
from fractions import Fraction

import numpy as np

import isosurface_ref as IR

ROUND_TRIP_GRIDS = (((13, 11, 9), None), ((9, 12, 10), (3, 4096, 70001)), ((16, 8, 8), None), ((7, 7, 7), (1, 2, 3)),
                    ((70, 6, 5), None), ((31, 5, 4), (0, 5, 0)), ((32, 4, 5), None))
FIELD_KINDS = ("normal", "zero_one", "integer", "ellipsoid")


def field(kind, shape, seed):
    """(A, iso): a node field whose outermost layer is outside, so that its marching-tetrahedra surface is closed"""
    rng = np.random.Generator(np.random.MT19937(seed))
    if kind == "normal":
        A, iso, low = rng.standard_normal(shape), 0.1, -10.0
    elif kind == "zero_one":                    # every vertex on a lattice midpoint, every ray along tetrahedron edges: all ties
        A, iso, low = (rng.random(shape) < 0.5).astype(np.float64), 0.5, 0.0
    elif kind == "integer":                     # no node equals iso (such a node's surface collapses into a point), means do
        A, iso, low = rng.integers(-3, 4, shape).astype(np.float64), 0.5, -5.0
    else:                                       # a rotated ellipsoid plus noise
        g = np.meshgrid(*[np.arange(n) - 0.5 * (n - 1) for n in shape], indexing="ij")
        c, s = np.cos(0.6), np.sin(0.6)
        u, v, w = c * g[0] - s * g[1], s * g[0] + c * g[1], g[2]
        r = [0.4 * n for n in shape]
        A, iso, low = 1.0 - ((u / r[0]) ** 2 + (v / r[1]) ** 2 + (w / r[2]) ** 2) + 0.05 * rng.standard_normal(shape), 0.0, -10.0
    A = np.asfortranarray(A)
    A[0], A[-1], A[:, 0], A[:, -1], A[:, :, 0], A[:, :, -1] = low, low, low, low, low, low
    return A, iso


def surface(A, iso, origin=None):
    """the closed surface of A >= iso, nodes taken as cell centres: ns3d_isosurface's triangles (its definition in NumPy) shifted by 0.5"""
    tri, _ = IR.reference(A, iso, origin=(0, 0, 0) if origin is None else origin)
    return tri + 0.5


def expected_mask(A, iso):
    """What the rule gives for surface(A, iso) on the grid A.shape, from the field alone, and `sure`, the bits this statement covers.
    C: the node is inside.  Vx, Vy, Vz: the mean of the two neighbouring nodes is >= iso — but where that mean EQUALS iso the vertex
    sits on the sample itself and the half-open rule decides: along x the sample counts as beyond the surface, so the bit is that of
    the upper node; along y and z it depends on the triangles around the vertex, and those bits are left to the exact evaluation."""
    nx, ny, nz = A.shape
    m = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    sure = np.full(m.shape, 0x0F, dtype=np.uint8, order="F")
    m[:nx, :ny, :nz] |= (A >= iso).astype(np.uint8)
    for q, (bit, lo, hi) in enumerate(((2, A[:-1], A[1:]), (4, A[:, :-1], A[:, 1:]), (8, A[:, :, :-1], A[:, :, 1:]))):
        mean = 0.5 * (lo + hi)
        val = (mean > iso) | ((mean == iso) & (hi >= iso))
        sl = [slice(0, nx), slice(0, ny), slice(0, nz)]
        sl[q] = slice(1, A.shape[q])
        m[tuple(sl)] |= val.astype(np.uint8) * np.uint8(bit)
        if q > 0:
            sure[tuple(sl)] &= np.where(mean == iso, np.uint8(0x0F ^ bit), np.uint8(0x0F))
    return m, sure


def octahedron(centre, radius):
    """8 triangles, (8,3,3)"""
    c = np.asarray(centre, dtype=np.float64)
    r = np.broadcast_to(np.asarray(radius, dtype=np.float64), (3,))
    px, mx, py, my, pz, mz = (c + np.eye(3)[q] * s * r[q] for q in range(3) for s in (1, -1))
    return np.array([[a, b, d] for a in (px, mx) for b in (py, my) for d in (pz, mz)])


# ---- the perturbed rule, evaluated exactly (Fractions): the sample is the point (x + δ, y + ε, z + ε²), δ ≫ ε ≫ ε² > 0 infinitesimal
def _sign_perturbed(py, pz, qy, qz, ry, rz):
    """the sign of the orientation determinant of (p, q, r + (ε, ε²)), p → q as given"""
    dy, dz = qy - py, qz - pz
    for v in (dy * (rz - pz) - dz * (ry - py), -dz, dy):        # the coefficients of 1, ε, ε²
        if v != 0:
            return 1 if v > 0 else -1
    return 0


def exact_inside(tris, x, y, z):
    """parity of the crossings of the ray from (x, y, z) towards −x, every quantity a Fraction"""
    flips = 0
    for a, b, c in tris:
        s = [_sign_perturbed(p[1], p[2], q[1], q[2], y, z) for p, q in ((a, b), (b, c), (c, a))]
        if not (s[0] == s[1] == s[2] != 0):
            continue
        u, v = [b[q] - a[q] for q in range(3)], [c[q] - a[q] for q in range(3)]
        n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        if n[0] == 0:
            continue
        xs = a[0] - (n[1] * (y - a[1]) + n[2] * (z - a[2])) / n[0]
        flips += x >= xs
    return flips & 1


def exact_mask(tri, nx, ny, nz, origin=None):
    """the mask of the rule in exact arithmetic; tri must hold dyadic numbers"""
    o = (0, 0, 0) if origin is None else tuple(int(q) for q in origin)
    T = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    T = T[np.isfinite(T).all(axis=(1, 2))]
    F = [[[Fraction(float(T[t, v, q])) for q in range(3)] for v in range(3)] for t in range(T.shape[0])]
    ymin, ymax, zmin, zmax = T[:, :, 1].min(1), T[:, :, 1].max(1), T[:, :, 2].min(1), T[:, :, 2].max(1)
    h = Fraction(1, 2)
    m = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    for bit, s, (ei, ej, ek) in ((1, (h, h, h), (nx, ny, nz)), (2, (0, h, h), (nx + 1, ny, nz)), (4, (h, 0, h), (nx, ny + 1, nz)),
                                 (8, (h, h, 0), (nx, ny, nz + 1))):
        for k in range(ek):
            for j in range(ej):
                y, z = j + o[1] + s[1], k + o[2] + s[2]
                near = np.nonzero((ymin <= float(y)) & (float(y) <= ymax) & (zmin <= float(z)) & (float(z) <= zmax))[0]
                if near.size == 0:
                    continue
                cand = [F[t] for t in near]
                for i in range(ei):
                    if exact_inside(cand, i + o[0] + s[0], y, z):
                        m[i, j, k] |= bit
    return m
