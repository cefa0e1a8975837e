"""CPU tests of the obstacle voxelizer's definition (include/ns3d.h, ns3d_voxelize) through its NumPy statement tests/solid_ref.py:
against an exact evaluation of the perturbed rule on dyadic meshes, against the fields marching-tetrahedra surfaces came from, and
the host-side plumbing of navierstokes3d_amd.solid.  No GPU."""
import os
import re

import numpy as np
import pytest

import solid_cases as SC
import solid_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(m):
    return [int(((m >> b) & 1).sum()) for b in range(4)]


DYADIC = {
    # rays through vertices (the rows through the centre), along edges and out of the grid on the low and the high side
    "octahedron": (SC.octahedron((3.5, 2.5, 2.5), 3.0), (6, 5, 4), None),
    "octahedron_on_faces": (SC.octahedron((3.0, 2.0, 2.0), (2.5, 2.0, 3.0)), (6, 5, 4), None),
    "octahedron_2^-10": (SC.octahedron((3.0 + 3 * 2.0 ** -10, 2.5 - 2.0 ** -10, 2.0 + 5 * 2.0 ** -10), (2.5, 1.5 + 2.0 ** -9, 2.75)), (6, 5, 4), None),
    "octahedron_origin": (SC.octahedron((3.5 + 7, 2.5 + 4000, 2.5 + 70000), 3.0), (6, 5, 4), (7, 4000, 70000)),
}


def _box_cases():
    from navierstokes3d_amd import solid as S
    return {
        # faces on sample points: rays lie IN the faces y = 1 and z = 0.5 and run along the box's edges; out of the grid at low x and high y
        "box_on_samples": (S.box_mesh((-1.0, 1.0, 0.5), (3.0, 7.0, 2.5)), (6, 5, 4), None),
        "box_larger": (S.box_mesh((-2.0, -2.0, -2.0), (9.0, 9.0, 9.0)), (6, 5, 4), None),
        "box_dyadic": (S.box_mesh((1.0 + 2.0 ** -10, 0.5, 1.0), (4.5, 3.0 - 2.0 ** -10, 3.5)), (6, 5, 4), None),
    }


@pytest.mark.parametrize("name", list(DYADIC) + ["box_on_samples", "box_larger", "box_dyadic"])
def test_reference_equals_the_exact_rule_on_dyadic_meshes(name):
    tri, n, origin = DYADIC[name] if name in DYADIC else _box_cases()[name]
    assert (np.abs(tri) < 2.0 ** 17).all() and (tri * 1024 == np.round(tri * 1024)).all()
    m = SR.voxelize(tri, *n, origin=origin)
    e = SC.exact_mask(tri, *n, origin=origin)
    assert np.array_equal(m, e), (name, _bits(m), _bits(e))
    assert m.any()
    assert not (m & 0xF0).any()
    assert not (m[n[0]] & 0x0D).any() and not (m[:, n[1]] & 0x0B).any() and not (m[:, :, n[2]] & 0x07).any()      # invalid points


def test_box_on_sample_points_is_half_open():
    from navierstokes3d_amd import solid as S
    m = SR.voxelize(S.box_mesh((2, 3, 1), (5, 6, 4)), 8, 8, 6)
    for b in range(4):
        idx = np.argwhere((m >> b) & 1)
        assert idx.min(0).tolist() == [2, 3, 1] and idx.max(0).tolist() == [4, 5, 3] and len(idx) == 27


@pytest.mark.parametrize("kind", SC.FIELD_KINDS)
@pytest.mark.parametrize("shape,origin", SC.ROUND_TRIP_GRIDS)
def test_round_trip_through_an_isosurface(kind, shape, origin):
    """field → marching tetrahedra → voxelize gives the field's own inside test back; permuting the triangles changes nothing"""
    A, iso = SC.field(kind, shape, seed=sum(shape))
    tri = SC.surface(A, iso, origin)
    m = SR.voxelize(tri, *shape, origin=origin)
    e, sure = SC.expected_mask(A, iso)
    assert np.array_equal(m & 1, e & 1)
    assert np.array_equal(m & sure, e & sure), [_bits((m ^ e) & sure)]
    if kind in ("normal", "ellipsoid"):
        assert (sure == 0x0F).all()                 # no mean equals iso: every bit is covered
    perm = np.random.Generator(np.random.MT19937(5)).permutation(tri.shape[0])
    assert np.array_equal(SR.voxelize(tri[perm], *shape, origin=origin), m)


@pytest.mark.parametrize("kind", ("zero_one", "integer"))
def test_all_ties_surface_equals_the_exact_rule(kind):
    """the bits expected_mask leaves open — a vertex ON a Vy / Vz sample — and all others, on a grid small enough for Fractions"""
    shape = (6, 5, 5)
    A, iso = SC.field(kind, shape, seed=11)
    tri = SC.surface(A, iso)
    m = SR.voxelize(tri, *shape)
    assert np.array_equal(m, SC.exact_mask(tri, *shape))
    _, sure = SC.expected_mask(A, iso)
    assert (sure != 0x0F).any()


def test_skipped_triangles_and_empty_mesh():
    from navierstokes3d_amd import solid as S
    n = (6, 5, 4)
    box = S.box_mesh((1.0, 1.0, 0.5), (4.0, 3.5, 3.0))
    m = SR.voxelize(box, *n)
    bad = np.array([[[np.nan, 1.0, 1.0], [3.0, 4.0, 1.0], [2.0, 1.0, 3.0]], [[1.0, np.inf, 1.0], [3.0, 4.0, 1.0], [2.0, 1.0, 3.0]]])
    flat = np.array([[[0.0, 2.0, 1.0], [5.0, 2.0, 3.0], [2.0, 2.0, 2.0]],       # projects onto a segment: n.x == 0
                     [[0.0, 2.0, 2.0], [5.0, 2.0, 2.0], [2.0, 2.0, 2.0]]])      # projects onto a point
    assert np.array_equal(SR.voxelize(np.concatenate([bad, box, flat]), *n), m)
    assert not SR.voxelize(np.zeros((0, 3, 3)), *n).any()
    assert not SR.voxelize(bad, *n).any() and not SR.voxelize(flat, *n).any()


def test_set_solid_and_momentum_statement():
    rng = np.random.Generator(np.random.MT19937(3))
    nx, ny, nz = 5, 4, 3
    mask = rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8)
    C, Vx, Vy, Vz = (rng.uniform(1, 2, s) for s in ((nx, ny, nz), (nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1)))
    V0 = [a.copy() for a in (Vx, Vy, Vz)]
    SR.set_solid(C, Vx, Vy, Vz, mask)
    assert np.array_equal(C == 1, (mask[:nx, :ny, :nz] & 1) != 0) and np.array_equal(Vx == 0, (mask[:, :ny, :nz] & 2) != 0)
    assert np.array_equal(Vy == 0, (mask[:nx, :, :nz] & 4) != 0) and np.array_equal(Vz == 0, (mask[:nx, :ny, :] & 8) != 0)
    sums, counts, _ = SR.momentum(*V0, mask)
    assert counts == [int((Vx == 0).sum()), int((Vy == 0).sum()), int((Vz == 0).sum())]
    assert abs(sums[0] - (V0[0] - Vx).sum()) < 1e-12
    _, seam, _ = SR.momentum(*V0, mask, seam_lo=(1, 0, 0), seam_hi=(0, 0, 1))
    assert seam[0] == int((Vx[2:, :, :nz - 1] == 0).sum()) and seam[2] == int((Vz[1:, :, :nz] == 0).sum())


def test_layout_and_ply_round_trip(tmp_path):
    from navierstokes3d_amd import solid as S
    from navierstokes3d_amd.isosurface import Isosurface
    tri = np.arange(36, dtype=np.float64).reshape(4, 3, 3)
    assert np.array_equal(S.tri_array(tri.reshape(4, 9)), tri) and np.array_equal(S.tri_array(tri.reshape(-1)), tri)
    assert S.tri_array(tri).reshape(-1)[9:18].tolist() == tri[1].reshape(-1).tolist()            # x0,y0,z0,x1,… per triangle
    assert np.array_equal(SR.as_tri9(tri).reshape(4, 3, 3), tri)
    with pytest.raises(Exception):
        S.tri_array(np.zeros(10))
    box = S.box_mesh((0.5, 1.0, 1.5), (2.0, 3.0, 2.5))
    assert box.shape == (12, 3, 3)
    centre, normal = box.mean(axis=(0, 1)), np.cross(box[:, 1] - box[:, 0], box[:, 2] - box[:, 0])
    assert (((box.mean(axis=1) - centre) * normal).sum(axis=1) > 0).all()                       # closed, outward
    surf = Isosurface(box - 0.5, None, (0, 0, 0), (0.25, 0.5, 0.125), (-1.0, -2.0, -0.5))       # node positions of cell centres
    assert np.array_equal(S.from_isosurface(surf), box)
    back = S.to_index(S.load_ply(surf.save_ply(str(tmp_path / "box.ply"))), surf.spacings, surf.low_corner)
    assert back.shape == box.shape
    assert np.array_equal(np.sort(back.reshape(-1, 9), axis=0), np.sort(box.reshape(-1, 9), axis=0))   # dyadic: float32 holds them
    assert np.array_equal(S.to_index(surf.tri, surf.spacings, surf.low_corner), box)


def test_header_binding_and_library_agree():
    from navierstokes3d_amd import build, lib as L
    build.build()
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    assert re.search(r"int ns3d_voxelize\(ns3d_ctx \*, unsigned char \*mask, const double \*tri, long long n_tri, int nx, int ny, int nz, "
                     r"const int \*origin\);", src)
    assert re.search(r"int ns3d_set_solid_##S\(ns3d_ctx \*, T \*C, T \*Vx, T \*Vy, T \*Vz, const unsigned char \*mask, int nx, int ny, int nz\);", src)
    assert re.search(r"int ns3d_solid_momentum_##S\(", src) and "int ns3d_set_obstacle(ns3d_ctx *ctx, const unsigned char *mask);" in src
    assert "const unsigned char *ns3d_obstacle(const ns3d_ctx *ctx);" in src
    names = {"ns3d_voxelize", "ns3d_set_obstacle", "ns3d_obstacle", "ns3d_set_solid_f64", "ns3d_set_solid_f32", "ns3d_solid_momentum_f64",
             "ns3d_solid_momentum_f32"}
    assert names <= set(L.exported_symbols())
    lib = L.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.ns3d_voxelize(None, None, None, 0, 4, 4, 4, None) == L.NS3D_ERR_ARG and L.last_error() == "ns3d_voxelize: null context"
    assert lib.ns3d_set_obstacle(None, None) == L.NS3D_ERR_ARG and lib.ns3d_obstacle(None) is None
    for name in ("set_solid", "solid_momentum"):
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            assert fn(None, *[a() for a in L.DERIVED_SIGNATURES[name]]) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
