"""Host side of ns3d_isosurface (include/ns3d.h): the triangle surface of a level set of a field that sits on the device — the Q
isosurface of a cylinder wake, coloured by a second field — instead of copying the field off the device.  Every vertex is formed
on the device by libns3d (marching tetrahedra, fp64, the same bits in every arithmetic mode); this module sizes the output, moves
the triangles into physical coordinates and writes them out.  PyTorch does no arithmetic here."""
import numpy as np
import torch

from . import kernels as K


class Isosurface:
    """A triangle list.  `tri_index` (n,3,3): the vertices as the device returned them, in the index space of the array's nodes
    (origin included); `val` (n,3) or None: the colour field at the vertices; `tri` (n,3,3): physical coordinates
    low_corner_q + (pos_q + (0 if stagger_q else 0.5))·d_q — a node of a cell-centred direction sits half a cell in."""

    def __init__(self, tri_index, val=None, stagger=(0, 0, 0), spacings=(1.0, 1.0, 1.0), low_corner=(0.0, 0.0, 0.0)):
        self.tri_index = np.ascontiguousarray(tri_index, dtype=np.float64).reshape(-1, 3, 3)
        self.val = None if val is None else np.ascontiguousarray(val, dtype=np.float64).reshape(-1, 3)
        self.stagger = tuple(int(q) for q in stagger)
        self.spacings = tuple(float(q) for q in spacings)
        self.low_corner = tuple(float(q) for q in low_corner)
        self.tri = self.physical(self.tri_index)

    def physical(self, pos):
        """index-space positions (…, 3) in physical coordinates"""
        shift = np.array([0.0 if s else 0.5 for s in self.stagger])
        return np.array(self.low_corner) + (np.asarray(pos, dtype=np.float64) + shift) * np.array(self.spacings)

    @property
    def n(self):
        return self.tri_index.shape[0]

    def indexed(self):
        """(vertices, faces): the distinct vertices (m,3) in physical coordinates and the triangles (n,3) as indices into them.  A
        vertex depends only on its edge, so vertices are merged by exact comparison of their index-space coordinates."""
        flat = self.tri_index.reshape(-1, 3)
        if flat.shape[0] == 0:
            return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
        uniq, inv = np.unique(flat, axis=0, return_inverse=True)
        return self.physical(uniq), np.asarray(inv).reshape(-1, 3).astype(np.int64)

    def area(self):
        """the surface's area in physical units"""
        u = self.tri[:, 1] - self.tri[:, 0]
        v = self.tri[:, 2] - self.tri[:, 0]
        return float(0.5 * np.sqrt((np.cross(u, v) ** 2).sum(axis=1)).sum())

    def save_ply(self, path):
        """A binary little-endian PLY of the indexed mesh: vertices x y z (and `value` when the surface is coloured) as float32,
        faces as lists of three int32."""
        verts, faces = self.indexed()
        cols = [verts.astype("<f4")]
        props = "property float x\nproperty float y\nproperty float z\n"
        if self.val is not None:
            value = np.zeros(verts.shape[0])
            value[faces.reshape(-1)] = self.val.reshape(-1)      # one value per edge: duplicates carry the same bits
            cols.append(value.astype("<f4")[:, None])
            props += "property float value\n"
        head = ("ply\nformat binary_little_endian 1.0\ncomment ns3d_isosurface\nelement vertex %d\n%selement face %d\n"
                "property list uchar int vertex_indices\nend_header\n" % (verts.shape[0], props, faces.shape[0]))
        rec = np.zeros(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        rec["n"] = 3
        rec["v"] = faces
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes())
            fh.write(rec.tobytes())
        return path


def concat(pieces):
    """The pieces of several ranks as one surface, in the order given (they share stagger, spacings and low corner)."""
    pieces = list(pieces)
    if not pieces:
        raise ValueError("concat: no pieces")
    p0 = pieces[0]
    for p in pieces[1:]:
        if (p.stagger, p.spacings, p.low_corner) != (p0.stagger, p0.spacings, p0.low_corner) or (p.val is None) != (p0.val is None):
            raise ValueError("concat: the pieces differ in stagger, spacings, low corner or colouring")
    val = None if p0.val is None else np.concatenate([p.val for p in pieces], axis=0)
    return Isosurface(np.concatenate([p.tri_index for p in pieces], axis=0), val, p0.stagger, p0.spacings, p0.low_corner)


def extract(ctx, A, level, color=None, box=None, origin=None, stagger=(0, 0, 0), spacings=(1.0, 1.0, 1.0), low_corner=(0.0, 0.0, 0.0)):
    """The isosurface A = level of the device array A (its entries are nodes; `stagger` flags the directions whose nodes sit on cell
    faces, the others sit at cell centres), optionally coloured by `color`, over the node range `box` with `origin` added to the node
    indices.  One count-only call, an allocation of exactly that size, one filling call."""
    ctx = K._ctx(ctx, A)
    n = K.isosurface(A, level, color=color, box=box, origin=origin, ctx=ctx)
    tri = torch.empty(9 * n, dtype=torch.float64, device=A.device)
    val = None if color is None else torch.empty(3 * n, dtype=torch.float64, device=A.device)
    if n > 0:
        m = K.isosurface(A, level, color=color, box=box, origin=origin, tri=tri, val=val, cap=n, ctx=ctx)
        if m != n:
            raise K.L.Ns3dError("isosurface: %d triangles counted, %d on the filling call (the field changed in between)" % (n, m))
        ctx.sync()
    return Isosurface(tri.cpu().numpy().reshape(n, 3, 3), None if val is None else val.cpu().numpy().reshape(n, 3), stagger, spacings,
                      low_corner)
