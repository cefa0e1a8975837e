"""CPU tests of the definition of ns3d_isosurface (include/ns3d.h) and of the Python layer, on the output of the NumPy reference
(tests/isosurface_ref.py): the independent check that what the GPU tests compare against is a watertight, consistently oriented
surface whose vertices sit where the definition puts them."""
import itertools
import os
import sys
from collections import Counter

import numpy as np
import pytest

import isosurface_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid(n):
    return np.meshgrid(*[np.arange(e, dtype=np.float64) for e in n], indexing="ij")


def sphere(n=(20, 21, 19)):
    x, y, z = grid(n)
    return 6.283 - np.sqrt((x - 9.8137) ** 2 + (y - 10.2291) ** 2 + (z - 9.1763) ** 2), 0.0


def torus(n=(22, 21, 14)):
    x, y, z = grid(n)
    rho = np.sqrt((x - 10.6137) ** 2 + (y - 10.1291) ** 2)
    return 2.2173 - np.sqrt((rho - 6.1319) ** 2 + (z - 6.4763) ** 2), 0.0


def edges_of(tri):
    """directed edges (key of a, key of b) of every triangle, the keys being the vertices' exact bits"""
    keys = [[v.tobytes() for v in t] for t in tri]
    return [(k[q], k[(q + 1) % 3]) for k in keys for q in range(3)]


def assert_watertight(tri, allow_degenerate=False):
    directed = Counter()
    for a, b in edges_of(tri):
        if a == b:
            assert allow_degenerate, "an edge of zero length"
            continue
        directed[(a, b)] += 1
    if not allow_degenerate:
        for (a, b), c in directed.items():
            assert c == 1 and directed.get((b, a), 0) == 1, "an edge that is not shared by two triangles of opposite direction"
        return
    # with zero-area triangles an edge may be traversed more than once: each direction as often as the other
    for (a, b), c in directed.items():
        assert directed.get((b, a), 0) == c


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_tetrahedra_are_the_six_axis_orders():
    assert IR.TETS == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    for tet in IR.TETS:         # a componentwise increasing chain: every edge's `lo` corner is a subset of its `hi` corner
        for u, v in itertools.combinations(range(4), 2):
            assert tet[u] & tet[v] == tet[u] and tet[u] < tet[v]


def test_table_has_six_by_sixteen_entries_and_the_specified_counts():
    assert IR.FLIP.shape == (6, 16) and IR.NTRI.shape == (16,) and IR.EDGE.shape == (16, 2, 3, 2)
    for m in range(16):
        inside = bin(m).count("1")
        assert IR.NTRI[m] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[inside]
    assert IR.CUBE_COUNT[0] == 0 and IR.CUBE_COUNT[255] == 0 and IR.CUBE_COUNT.max() == 12
    # the triple products that decide the orientation are far from zero (vertices at edge midpoints of the unit cube)
    for t in range(6):
        for m in range(1, 15):
            assert (np.abs(IR.TRIPLE[t, m, :IR.NTRI[m]]) >= 1.0 / 16).all(), (t, m)


def oriented(t, m):
    """the triangles of (tetrahedron, case) as edge triples after the orientation flip"""
    out = []
    for q in range(IR.NTRI[m]):
        e = [tuple(x) for x in IR.EDGE[m, q]]
        out.append([e[0], e[2], e[1]] if IR.FLIP[t, m] else e)
    return out


def test_complementary_cases_give_the_same_triangles_with_opposite_orientation():
    for t in range(6):
        for m in range(1, 15):
            mine, theirs = oriented(t, m), oriented(t, 15 - m)
            assert sorted(sorted(x) for x in mine) == sorted(sorted(x) for x in theirs)
            for x in mine:
                y = [y for y in theirs if sorted(y) == sorted(x)][0]
                rev = x[::-1]
                assert any(rev[s:] + rev[:s] == y for s in range(3)), (t, m)


def test_complementary_fields_give_the_mirrored_surface():
    """A and −A with −iso (no node on the level): the same triangles (a quad's two in the other order), every normal reversed"""
    A, iso = sphere()
    t0, _ = IR.reference(A, iso + 0.3)
    t1, _ = IR.reference(-A, -(iso + 0.3))
    assert t0.shape == t1.shape and t0.shape[0] > 100
    normal = lambda t: np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    key = lambda t: [tuple(sorted(v.tobytes() for v in x)) for x in t]
    k0, k1 = key(t0), key(t1)
    assert len(set(k0)) == len(k0) and sorted(k0) == sorted(k1)   # the same vertices, bit for bit, in the same triangles
    n1 = dict(zip(k1, normal(t1)))
    assert all(np.dot(a, n1[k]) < 0.0 for k, a in zip(k0, normal(t0)))


# ---- watertight ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [sphere, torus])
def test_closed_surfaces_are_watertight(make):
    A, iso = make()
    assert not (A == iso).any()
    tri, _ = IR.reference(A, iso)
    assert tri.shape[0] > 500 and tri.shape[0] == IR.count(A, iso)
    assert_watertight(tri)


@pytest.mark.parametrize("make", [sphere, torus])
def test_a_node_exactly_on_the_level_keeps_the_surface_watertight(make):
    A, iso = make()
    inside = np.argwhere((A > iso) & (A < iso + 0.4))
    i, j, k = inside[len(inside) // 2]
    A = A.copy()
    A[i, j, k] = iso
    tri, _ = IR.reference(A, iso)
    assert tri.shape[0] == IR.count(A, iso)
    area2 = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(axis=1)
    assert (area2 == 0.0).any()                 # the tie does produce zero-area triangles, and they are emitted
    assert_watertight(tri, allow_degenerate=True)
    assert_watertight(tri[area2 > 0.0], allow_degenerate=True)


# ---- orientation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signs", list(itertools.product((1.0, -1.0), repeat=3)))
def test_normals_point_towards_decreasing_values(signs):
    x, y, z = grid((7, 6, 8))
    g = np.array(signs) * np.array([0.75, 0.5, 1.25])             # exactly representable: the field and the sign test are exact
    A = g[0] * x + g[1] * y + g[2] * z
    iso = float(np.median(A)) + 0.125
    tri, _ = IR.reference(A, iso)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nz = (nrm ** 2).sum(axis=1) > 0.0
    assert nz.sum() > 50
    assert (nrm[nz] @ (-g) > 0.0).all()


# ---- vertices -----------------------------------------------------------------------------------------------------------------
def test_vertices_lie_on_kuhn_edges_between_an_inside_and_an_outside_node():
    A, iso = sphere()
    B = np.cos(0.3 * grid(A.shape)[0]) + 0.1 * grid(A.shape)[2]
    tri, val = IR.reference(A, iso, B)
    kuhn = {(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)}
    P = tri.reshape(-1, 3)
    V = val.reshape(-1)
    lo = np.floor(P).astype(np.int64)
    frac = P - lo
    for p, l, f, v in zip(P, lo, frac, V):
        moving = f > 0.0
        assert moving.any()                                 # no node is on the level
        d = tuple(int(q) for q in moving)
        assert d in kuhn
        hi = l + np.array(d)
        a_lo, a_hi = A[tuple(l)], A[tuple(hi)]
        assert (a_lo >= iso) != (a_hi >= iso)
        t = (iso - a_lo) / (a_hi - a_lo)
        assert 0.0 <= t <= 1.0
        assert (p[moving] == l[moving].astype(np.float64) + t).all()    # one t along every moving direction, added to the integer
        assert v == B[tuple(hi)] * t + B[tuple(l)] * (1.0 - t)


# ---- seams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_overlapping_boxes_make_the_whole_surface(axis):
    """a decomposed run: rank 1's array starts `start` nodes in, overlaps rank 0's by two nodes and carries origin = start; rank 0 owns
    the cubes below `cut`, rank 1 those from `cut` on"""
    A, iso = torus()
    B = np.sin(0.2 * grid(A.shape)[1])
    whole_t, whole_v = IR.reference(A, iso, B)
    e = A.shape
    cut = e[axis] // 2
    start = cut - 1
    box0 = [0, 0, 0] + [q - 1 for q in e]
    box0[3 + axis] = cut
    sl = [slice(None)] * 3
    sl[axis] = slice(start, None)
    A1, B1 = A[tuple(sl)], B[tuple(sl)]
    box1 = [0, 0, 0] + [q - 1 for q in A1.shape]
    box1[axis] = cut - start
    origin = [0, 0, 0]
    origin[axis] = start
    t0, v0 = IR.reference(A, iso, B, box0)
    t1, v1 = IR.reference(A1, iso, B1, box1, origin)
    rows = lambda t, v: Counter(r.tobytes() for r in np.concatenate([t.reshape(-1, 9), v], axis=1))
    assert t0.shape[0] > 0 and t1.shape[0] > 0
    assert rows(np.concatenate([t0, t1]), np.concatenate([v0, v1])) == rows(whole_t, whole_v)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _isosurface_module():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from navierstokes3d_amd import isosurface
    return isosurface


def read_ply(path):
    """a reader for exactly what save_ply writes"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    i0 = [q for q, l in enumerate(head) if l.startswith("element vertex")][0]
    i1 = [q for q, l in enumerate(head) if l.startswith("element face")][0]
    props = [l.split() for l in head[i0 + 1:i1]]
    assert all(p[0] == "property" and p[1] == "float" for p in props)
    names = [p[2] for p in props]
    assert head[i1 + 1] == "property list uchar int vertex_indices"
    verts = np.frombuffer(raw, dtype="<f4", count=nv * len(names), offset=end).reshape(nv, len(names))
    faces = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + 4 * nv * len(names))
    assert end + 4 * nv * len(names) + 13 * nf == len(raw) and (faces["n"] == 3).all()
    return names, verts, faces["v"]


@pytest.mark.parametrize("make,chi", [(sphere, 2), (torus, 0)])
def test_indexed_mesh_has_the_euler_characteristic_of_its_surface(make, chi):
    iso_mod = _isosurface_module()
    A, iso = make()
    tri, _ = IR.reference(A, iso)
    s = iso_mod.Isosurface(tri)
    verts, faces = s.indexed()
    edges = {tuple(sorted((f[q], f[(q + 1) % 3]))) for f in faces for q in range(3)}
    assert verts.shape[0] - len(edges) + faces.shape[0] == chi
    assert faces.shape == (tri.shape[0], 3) and np.array_equal(verts[faces], s.tri)


def test_physical_coordinates_area_and_concat():
    iso_mod = _isosurface_module()
    A, iso = sphere()
    tri, _ = IR.reference(A, iso)
    s = iso_mod.Isosurface(tri, None, stagger=(1, 0, 0), spacings=(0.5, 0.25, 2.0), low_corner=(1.0, -2.0, 3.0))
    want = np.array([1.0, -2.0, 3.0]) + (tri + np.array([0.0, 0.5, 0.5])) * np.array([0.5, 0.25, 2.0])
    assert np.array_equal(s.tri, want) and np.array_equal(s.tri_index, tri)
    unit = iso_mod.Isosurface(tri, None, stagger=(1, 1, 1))
    r = 6.283
    assert abs(unit.area() - 4 * np.pi * r * r) < 0.05 * 4 * np.pi * r * r        # a faceted sphere: a few per cent below
    half = tri.shape[0] // 2
    both = iso_mod.concat([iso_mod.Isosurface(tri[:half]), iso_mod.Isosurface(tri[half:])])
    assert np.array_equal(both.tri_index, tri) and both.val is None
    with pytest.raises(ValueError):
        iso_mod.concat([iso_mod.Isosurface(tri[:half]), iso_mod.Isosurface(tri[half:], spacings=(2.0, 1.0, 1.0))])


@pytest.mark.parametrize("coloured", [False, True])
def test_save_ply_round_trips(tmp_path, coloured):
    iso_mod = _isosurface_module()
    A, iso = torus()
    B = np.sin(0.2 * grid(A.shape)[1]) if coloured else None
    tri, val = IR.reference(A, iso, B)
    s = iso_mod.Isosurface(tri, val, spacings=(0.5, 0.25, 2.0))
    path = s.save_ply(str(tmp_path / "surface.ply"))
    names, verts, faces = read_ply(path)
    assert names == (["x", "y", "z", "value"] if coloured else ["x", "y", "z"])
    v_ref, f_ref = s.indexed()
    assert np.array_equal(faces, f_ref) and np.array_equal(verts[:, :3], v_ref.astype(np.float32))
    assert np.array_equal(verts[faces][:, :, :3], s.tri.astype(np.float32))
    if coloured:
        assert np.array_equal(verts[faces][:, :, 3], val.astype(np.float32))
