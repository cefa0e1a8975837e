"""Host side of ns3d_voxelize / ns3d_set_solid / ns3d_solid_momentum (include/ns3d.h): obstacles from closed triangle surfaces.  The
mask — one byte per point of set_cylinder!'s thread range, bit 0 C, 1 Vx, 2 Vy, 3 Vz at their stagger locations — is made on the device
by libns3d from triangles in the INDEX space of the cell grid ([0,nx]×[0,ny]×[0,nz], cell centres at half-integers); this module
brings meshes into that space (from an isosurface.Isosurface, a PLY file it wrote, or physical coordinates) and uploads them.  For a
body in motion (ns3d_mesh_transform / ns3d_set_solid_moving): `transform` poses a mesh on the device, `rigid_motion` makes the pose(t)
callable the drivers' `motion` keyword takes.  PyTorch does no arithmetic here."""
import numpy as np
import torch

from . import kernels as K
from . import lib as L


def tri_array(tri):
    """any of (n,3,3), (n,9) or a flat array of 9 values per triangle → a contiguous (n,3,3) float64 array: triangle, vertex, (x,y,z) —
    in memory the 9-double layout ns3d_isosurface writes and ns3d_voxelize reads"""
    a = np.ascontiguousarray(tri, dtype=np.float64)
    if a.size % 9:
        raise L.Ns3dError("a triangle list holds 9 values per triangle, got %d values" % a.size)
    return a.reshape(-1, 3, 3)


def voxelize(ctx, tri, nx, ny, nz, origin=None):
    """The mask of the closed surface `tri` (index space; (n,3,3) host array or a float64 device tensor) on the cell grid (nx,ny,nz):
    a uint8 device tensor of shape (nx+1, ny+1, nz+1), column-major like the fields.  origin = coords·(n−2) on a rank of a decomposed
    grid: the ranks then agree on the entries they duplicate.  Enqueues on the context's stream."""
    dev = torch.device("cuda", ctx.device)
    if isinstance(tri, torch.Tensor):
        t = tri.to(dev, torch.float64).contiguous().reshape(-1)
    else:
        t = torch.from_numpy(tri_array(tri).reshape(-1)).to(dev)
    mask = torch.empty((nz + 1, ny + 1, nx + 1), dtype=torch.uint8, device=dev).permute(2, 1, 0)
    ctx.after_torch_fill()
    K.voxelize(mask, t, (nx, ny, nz), origin=origin, ctx=ctx)
    return mask


def box_mesh(lo, hi):
    """the 12 triangles of the axis-parallel box [lo, hi] (index space or physical: whatever lo and hi are in), (12,3,3)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c = np.array([[(hi if (n >> q) & 1 else lo)[q] for q in range(3)] for n in range(8)])       # corner n = di + 2 dj + 4 dk
    quads = ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))  # outward normals −x +x −y +y −z +z
    return np.array([[c[q[0]], c[q[a]], c[q[a + 1]]] for q in quads for a in (1, 2)])


def transform(ctx, tri_dev, R, pivot, shift, spacing, out=None):
    """The mesh `tri_dev` (a contiguous float64 device tensor of 9 values per triangle, index space) in the pose x → pivot + shift +
    R·(x − pivot), the rotation taken in PHYSICAL space (ns3d_mesh_transform; pivot and shift in index units, spacing = (dx, dy, dz)),
    into `out` — a new tensor when None, `tri_dev` itself for in place.  Apply a pose to the ORIGINAL mesh, never to the last pose's
    output.  Enqueues on the context's stream."""
    if out is None:
        out = torch.empty_like(tri_dev)
        ctx.after_torch_fill()
    K.mesh_transform(out, tri_dev, R, pivot, shift, spacing, ctx=ctx)
    return out


def rotation(omega, t):
    """Rodrigues' formula: the 3×3 rotation by the angle |omega|·t about omega's direction, NumPy fp64; the identity for omega = 0"""
    w = np.asarray(omega, dtype=np.float64).reshape(3)
    rate = float(np.sqrt(np.sum(w * w)))
    if rate == 0.0:
        return np.eye(3)
    kx, ky, kz = w / rate
    Kx = np.array([[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]])
    a = rate * float(t)
    return np.eye(3) + np.sin(a) * Kx + (1.0 - np.cos(a)) * (Kx @ Kx)


def rigid_motion(velocity=(0.0, 0.0, 0.0), omega=(0.0, 0.0, 0.0), centre=None, spacing=None):
    """A body in steady rigid motion as the drivers' `motion` keyword takes it: a callable pose(t) → (R, shift, U, omega, centre).
    velocity U and angular velocity omega are physical (length/time, rad/time); centre is the centre of rotation at t = 0 in index
    space; spacing = (dx, dy, dz).  R is the rotation by |omega|·t (rotation()), shift = U·t/spacing in index units, centre the
    centre at time t: centre(0) + shift.  Any callable with this return shape describes a motion — y(t) = A·sin(2πft) with U its
    derivative, say."""
    if centre is None or spacing is None:
        raise L.Ns3dError("rigid_motion needs centre (index space) and spacing (dx, dy, dz)")
    U, w, c0, d = (np.array(v, dtype=np.float64).reshape(-1) for v in (velocity, omega, centre, spacing))
    if any(v.size != 3 for v in (U, w, c0, d)) or not all(np.isfinite(v).all() for v in (U, w, c0, d)) or not (d > 0).all():
        raise L.Ns3dError("rigid_motion: velocity, omega, centre and spacing hold 3 finite numbers each, the spacings > 0")

    def pose(t):
        shift = U * float(t) / d
        return rotation(w, t), shift, U.copy(), w.copy(), c0 + shift
    return pose


def to_index(points, spacings, low_corner=(0.0, 0.0, 0.0)):
    """physical coordinates (…,3) → the index space of the cell grid whose low corner is `low_corner`: the inverse of what
    isosurface.extract's spacings / low_corner do, (p − low_corner)/spacings"""
    return (np.asarray(points, dtype=np.float64) - np.asarray(low_corner, dtype=np.float64)) / np.asarray(spacings, dtype=np.float64)


def from_isosurface(surf):
    """an isosurface.Isosurface → (n,3,3) triangles in the index space of the cell grid: its node positions plus half a cell in the
    directions that are not staggered (exact: no spacings involved)"""
    shift = np.array([0.0 if s else 0.5 for s in surf.stagger])
    return tri_array(surf.tri_index + shift)


def load_ply(path):
    """the triangles of a PLY file Isosurface.save_ply wrote, (n,3,3) float64 in the file's (physical, float32) coordinates; bring them
    into index space with to_index"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if head[0] != "ply" or "format binary_little_endian 1.0" not in head:
        raise L.Ns3dError("%s: not a binary little-endian PLY file" % path)
    nv = nf = 0
    props, where = [], None
    for line in head:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv, where = int(w[2]), "vertex"
        elif w[:2] == ["element", "face"]:
            nf, where = int(w[2]), "face"
        elif w[:1] == ["property"] and where == "vertex":
            if w[1] != "float":
                raise L.Ns3dError("%s: vertex property %s is not float" % (path, w[-1]))
            props.append(w[2])
    if props[:3] != ["x", "y", "z"]:
        raise L.Ns3dError("%s: vertices do not start with x, y, z" % path)
    verts = np.frombuffer(data, dtype="<f4", count=nv * len(props), offset=end).reshape(nv, len(props))[:, :3].astype(np.float64)
    rec = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + 4 * nv * len(props))
    if nf and (rec["n"] != 3).any():
        raise L.Ns3dError("%s: faces that are not triangles" % path)
    return tri_array(verts[rec["v"].reshape(-1)])


def mask_of_cylinder(ctx, n, *cyl, dtype=torch.float64):
    """The reference cylinder's own mask on the cell grid n = (nx,ny,nz): set_cylinder (cyl: its 15 scalars, multi.jl:249, or 12,
    gpu.jl:336) run on sentinel fields — C = 0, V = 1 — and read off: a uint8 device tensor like voxelize's."""
    nx, ny, nz = (int(q) for q in n)
    dev = torch.device("cuda", ctx.device)
    Cf = K.zeros((nx, ny, nz), dtype, dev)
    V = [K.from_numpy(np.ones(s, dtype=np.float64 if dtype == torch.float64 else np.float32), dev)
         for s in ((nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))]
    ctx.after_torch_fill()
    K.set_cylinder(Cf, V[0], V[1], V[2], *cyl, ctx=ctx)
    ctx.sync()
    m = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    m[:nx, :ny, :nz] |= (K.to_numpy(Cf) == 1).astype(np.uint8)
    m[:, :ny, :nz] |= (K.to_numpy(V[0]) == 0).astype(np.uint8) << 1
    m[:nx, :, :nz] |= (K.to_numpy(V[1]) == 0).astype(np.uint8) << 2
    m[:nx, :ny, :] |= (K.to_numpy(V[2]) == 0).astype(np.uint8) << 3
    mask = torch.from_numpy(np.ascontiguousarray(m.transpose(2, 1, 0))).to(dev).permute(2, 1, 0)
    ctx.after_torch_fill()
    return mask


def to_numpy(mask):
    """a mask tensor on the host: uint8, shape (nx+1, ny+1, nz+1), Fortran order"""
    return np.asfortranarray(mask.permute(2, 1, 0).contiguous().cpu().numpy().transpose(2, 1, 0))
