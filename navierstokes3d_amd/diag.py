"""Host-side rules of ns3d_diagnostics (include/ns3d.h) that do not need a GPU: which entries of a rank's arrays the rank
OWNS, so that P ranks count the global array exactly once, and the length of the reduction's longest chain of additions.

ImplicitGlobalGrid's indexing (include/ns3d.h): in a decomposed dimension a rank's array of extent n+s (s = 0 cell-centred,
s = 1 staggered in that dimension) starts at global index coord·(n−2) and overlaps its upper neighbour's by 2+s entries; the
global extent is P·(n−2)+2+s.  The rule: at an interior seam a rank leaves out its first 1+s entries on its low side and its
last entry (the halo) on its high side; a physical end is counted in full.  Rank c then owns the global indices
[c·(n−2)+1+s, (c+1)·(n−2)+1+s) between two seams — the next rank starts where this one stops, for s = 0 and s = 1 alike —
and the two end ranks add [0, 1+s) and the last entry: a partition of [0, P·(n−2)+2+s).
"""


def owned_range(n, s, seam_lo, seam_hi):
    """0-based half-open range [lo, hi) of the entries a rank owns along one dimension of an array of extent n+s."""
    return ((1 + s) if seam_lo else 0, (n + s - 1) if seam_hi else (n + s))


def seam_flags(dims, coords):
    """(seam_lo, seam_hi) per dimension of the rank at MPI_Cart coordinates `coords` of a `dims` topology."""
    return (tuple(int(c > 0) for c in coords), tuple(int(c < d - 1) for c, d in zip(coords, dims)))


def owned_slices(shape_n, stagger, seam_lo, seam_hi):
    """The owned block of one array as a tuple of slices; shape_n = (nx, ny, nz) of the LOCAL cell grid, stagger = (sx, sy, sz)
    of the array (Vx: (1,0,0), Vy: (0,1,0), Vz: (0,0,1), Pr, C: (0,0,0))."""
    return tuple(slice(*owned_range(n, s, lo, hi)) for n, s, lo, hi in zip(shape_n, stagger, seam_lo, seam_hi))


def launch_geometry(nx, ny, nz):
    """(workgroups, planes per workgroup) of the monitor's launch — ns3d_diag_geometry in csrc/ns3d_launch.h."""
    gx, gy = (nx + 1 + 63) // 64, (ny + 1 + 3) // 4
    kz = 32
    while kz > 8 and gx * gy * ((nz + 1 + kz - 1) // kz) < 2048:
        kz //= 2
    return gx * gy * ((nz + 1 + kz - 1) // kz), kz


def path_length(nx, ny, nz):
    """L: additions on the longest path of the monitor's sums as built — kz per thread down its planes, 6 in the wave64
    butterfly and 3 over the workgroup's four waves; then, over the per-workgroup partials, ⌈workgroups/256⌉ per thread, 6 and 3
    again.  At most 32 + 18 + ⌈workgroups/256⌉: 128 at 512³ (19 737 workgroups)."""
    nb, kz = launch_geometry(nx, ny, nz)
    return kz + 9 + (nb + 255) // 256 + 9
