"""The definition of ns3d_isosurface (include/ns3d.h) as vectorised NumPy: marching tetrahedra on the Kuhn decomposition, fp64, one
pass per tetrahedron over all cubes.  Written from the header's text — the tables are derived here from its rules, the orientation
by evaluating the rule on the unit cube with inside = 1, outside = 0, iso = 0.5 — and not from the kernel."""
import itertools

import numpy as np

# tetrahedron pi: the axis orders in lexicographic order; v0 = corner 0, v1 = v0 + e_pi1, v2 = v1 + e_pi2, v3 = corner 7
TETS = [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in itertools.permutations((0, 1, 2))]


def corner_xyz(c):
    return np.array([(c >> q) & 1 for q in range(3)], dtype=np.float64)


def case_triangles(m):
    """the triangles of case m (bit n set: v_n inside), each three edges (u, v) with u < v, before orientation"""
    ins = [n for n in range(4) if m >> n & 1]
    out = [n for n in range(4) if not m >> n & 1]
    E = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (1, 3):
        a, rest = (ins[0], out) if len(ins) == 1 else (out[0], ins)
        return [[E(a, rest[0]), E(a, rest[1]), E(a, rest[2])]]
    if len(ins) == 2:
        (p, q), (r, s) = ins, out
        return [[E(p, r), E(p, s), E(q, s)], [E(p, r), E(q, s), E(q, r)]]
    return []


def derive_tables():
    """NTRI[16]; EDGE[16, 2, 3, 2] (case, triangle, vertex, (u, v)); FLIP[6, 16] and the triple products TRIPLE[6, 16, 2] behind it"""
    ntri = np.zeros(16, dtype=np.int64)
    edge = np.zeros((16, 2, 3, 2), dtype=np.int64)
    flip = np.zeros((6, 16), dtype=bool)
    triple = np.zeros((6, 16, 2))
    for m in range(16):
        tris = case_triangles(m)
        ntri[m] = len(tris)
        for q, tr in enumerate(tris):
            edge[m, q] = tr
        for t, tet in enumerate(TETS):
            a = np.array([1.0 if m >> n & 1 else 0.0 for n in range(4)])
            x = np.array([corner_xyz(c) for c in tet])
            if not tris:
                continue
            direction = x[a == 0.0].mean(axis=0) - x[a == 1.0].mean(axis=0)        # from the inside vertices towards the outside ones
            for q, tr in enumerate(tris):
                P = []
                for u, v in tr:
                    tt = (0.5 - a[u]) / (a[v] - a[u])
                    P.append(x[u] + (x[v] - x[u]) * tt)
                triple[t, m, q] = np.dot(np.cross(P[1] - P[0], P[2] - P[0]), direction)
            assert (triple[t, m, :len(tris)] != 0.0).all()
            assert len({bool(s < 0.0) for s in triple[t, m, :len(tris)]}) == 1      # both halves of a quad turn the same way
            flip[t, m] = triple[t, m, 0] < 0.0
    return ntri, edge, flip, triple


NTRI, EDGE, FLIP, TRIPLE = derive_tables()
CUBE_COUNT = np.array([sum(NTRI[sum((mask >> tet[n] & 1) << n for n in range(4))] for tet in TETS) for mask in range(256)])


def cubes_of(shape, box):
    lo = (0, 0, 0) if box is None else tuple(box[:3])
    hi = tuple(e - 1 for e in shape) if box is None else tuple(box[3:])
    I, J, K = np.meshgrid(*[np.arange(lo[q], hi[q]) for q in range(3)], indexing="ij")
    return [X.ravel(order="F") for X in (I, J, K)]                                  # x fastest, then y, then z


def corner_values(F, ijk):
    return np.stack([np.asarray(F)[ijk[0] + (c & 1), ijk[1] + (c >> 1 & 1), ijk[2] + (c >> 2 & 1)].astype(np.float64) for c in range(8)], axis=1)


def count(A, iso, box=None):
    """the number of triangles, from the inside masks alone"""
    ijk = cubes_of(A.shape, box)
    a8 = corner_values(A, ijk)
    mask = ((a8 >= iso) << np.arange(8)).sum(axis=1)
    return int(CUBE_COUNT[mask][np.isfinite(a8).all(axis=1)].sum())


def reference(A, iso, B=None, box=None, origin=None):
    """(tri (n,3,3), val (n,3) or None) in the order of the definition"""
    iso = np.float64(iso)
    origin = (0, 0, 0) if origin is None else tuple(int(q) for q in origin)
    ijk = cubes_of(A.shape, box)
    a8 = corner_values(A, ijk)
    b8 = None if B is None else corner_values(B, ijk)
    inside = a8 >= iso
    finite = np.isfinite(a8).all(axis=1)
    keys, tris, vals = [], [], []
    with np.errstate(all="ignore"):
        for t, tet in enumerate(TETS):
            tetc = np.array(tet)
            m = sum(inside[:, tet[n]].astype(np.int64) << n for n in range(4))
            for q in range(2):
                sel = np.nonzero(finite & (NTRI[m] > q))[0]
                if sel.size == 0:
                    continue
                ms = m[sel]
                P = np.empty((sel.size, 3, 3))
                V = np.empty((sel.size, 3))
                rows = np.arange(sel.size)
                for n in range(3):
                    slot = np.where(FLIP[t, ms] & (n > 0), 3 - n, n) if n else np.zeros(sel.size, dtype=np.int64)
                    clo, chi = tetc[EDGE[ms, q, n, 0]], tetc[EDGE[ms, q, n, 1]]
                    a_lo, a_hi = a8[sel, clo], a8[sel, chi]
                    tt = (iso - a_lo) / (a_hi - a_lo)
                    for ax in range(3):
                        dlo, dhi = clo >> ax & 1, chi >> ax & 1
                        P[rows, slot, ax] = (ijk[ax][sel] + dlo + origin[ax]).astype(np.float64) + np.where(dhi > dlo, tt, 0.0)
                    if b8 is not None:
                        V[rows, slot] = b8[sel, chi] * tt + b8[sel, clo] * (1.0 - tt)
                keys.append(sel * 12 + t * 2 + q)
                tris.append(P)
                vals.append(V)
    if not keys:
        return np.zeros((0, 3, 3)), (None if B is None else np.zeros((0, 3)))
    order = np.argsort(np.concatenate(keys), kind="stable")
    tri = np.concatenate(tris)[order]
    return tri, (None if B is None else np.concatenate(vals)[order])
