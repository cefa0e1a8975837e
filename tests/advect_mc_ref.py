"""NumPy reference of the limited MacCormack advection (ns3d_advect_mc / ns3d_advect_correct, include/ns3d.h).  TEST INFRASTRUCTURE ONLY.

Stage 1 is oracle.numpy_ref.advect(…, faithful=False) on copies of the old fields (complete outputs; float32: see stage1); stage 2
is the header's definition written out, one ufunc per operation (no contraction), in the dtype of the arrays.  Everything is evaluated on whole index
grids like numpy_ref, so the device's STRICT build must return these bits."""
import numpy as np

from oracle import numpy_ref as NR

NAMES = ("Vx", "Vy", "Vz", "C")


def _o(A, i, j, k):
    """A[i, j, k] with 1-based index grids (column-major arrays: one flat gather, the same values in less time)"""
    if isinstance(A, np.ndarray) and A.flags.f_contiguous and isinstance(i, np.ndarray):
        sx, sy, _ = A.shape
        return np.take(A.reshape(-1, order="F"), (i - 1) + sx * ((j - 1) + sy * (k - 1)))
    return A[i - 1, j - 1, k - 1]


def _grid(xs, ys, zs):
    return np.meshgrid(np.asarray(xs), np.asarray(ys), np.asarray(zs), indexing="ij")


def node_sets(Vx_o, Vy_o, Vz_o, nx, ny, nz, which=NAMES):
    """name → (IX, IY, IZ, vxc, vyc, vzc): advect!'s four branches with the third one corrected (multi.jl:218-241), 1-based index
    grids of the advected nodes and the averages of the OLD velocities advect! forms for them — numpy_ref.advect's expressions"""
    o, q, h = _o, 0.25, 0.5            # Python scalars: the arrays keep their dtype (and running_error pairs can take their place)
    out = {}
    if "Vx" in which:
        IX, IY, IZ = _grid(range(2, nx + 1), range(1, ny + 1), range(1, nz + 1))
        out["Vx"] = (IX, IY, IZ, o(Vx_o, IX, IY, IZ),
                     q * (((o(Vy_o, IX - 1, IY, IZ) + o(Vy_o, IX - 1, IY + 1, IZ)) + o(Vy_o, IX, IY, IZ)) + o(Vy_o, IX, IY + 1, IZ)),
                     q * (((o(Vz_o, IX - 1, IY, IZ) + o(Vz_o, IX - 1, IY, IZ + 1)) + o(Vz_o, IX, IY, IZ)) + o(Vz_o, IX, IY, IZ + 1)))
    if "Vy" in which:
        IX, IY, IZ = _grid(range(1, nx + 1), range(2, ny + 1), range(1, nz + 1))
        out["Vy"] = (IX, IY, IZ,
                     q * (((o(Vx_o, IX, IY - 1, IZ) + o(Vx_o, IX + 1, IY - 1, IZ)) + o(Vx_o, IX, IY, IZ)) + o(Vx_o, IX + 1, IY, IZ)),
                     o(Vy_o, IX, IY, IZ),
                     q * (((o(Vz_o, IX, IY - 1, IZ) + o(Vz_o, IX, IY - 1, IZ + 1)) + o(Vz_o, IX, IY, IZ)) + o(Vz_o, IX, IY, IZ + 1)))
    if "Vz" in which:
        IX, IY, IZ = _grid(range(1, nx + 1), range(1, ny + 1), range(2, nz + 1))
        out["Vz"] = (IX, IY, IZ,
                     q * (((o(Vx_o, IX, IY, IZ - 1) + o(Vx_o, IX + 1, IY, IZ - 1)) + o(Vx_o, IX, IY, IZ)) + o(Vx_o, IX + 1, IY, IZ)),
                     q * (((o(Vy_o, IX, IY, IZ - 1) + o(Vy_o, IX, IY + 1, IZ - 1)) + o(Vy_o, IX, IY, IZ)) + o(Vy_o, IX, IY + 1, IZ)),
                     o(Vz_o, IX, IY, IZ))
    if "C" in which:
        IX, IY, IZ = _grid(range(1, nx + 1), range(1, ny + 1), range(1, nz + 1))
        out["C"] = (IX, IY, IZ, h * (o(Vx_o, IX, IY, IZ) + o(Vx_o, IX + 1, IY, IZ)), h * (o(Vy_o, IX, IY, IZ) + o(Vy_o, IX, IY + 1, IZ)),
                    h * (o(Vz_o, IX, IY, IZ) + o(Vz_o, IX, IY, IZ + 1)))
    return out


def departure(shape, vxc, vyc, vzc, dt, dx, dy, dz, IX, IY, IZ):
    """backtrack!'s departure cell and weights (multi.jl:190-197); dt, dx, dy, dz of dtype T.  `ix − δ` is formed in T, as Julia forms
    Int − Float32 and the device does: NumPy would promote an int64 grid minus a float32 array to float64, and for a |δ| below half
    an ulp of ix the two floors differ."""
    T = vxc.dtype.type
    dd = [dt * vxc / dx, dt * vyc / dy, dt * vzc / dz]
    with np.errstate(invalid="ignore"):
        i1 = [NR.clamp_floor(I.astype(T) - d, s) for I, d, s in zip((IX, IY, IZ), dd, shape)]     # clamped before the conversion
        i2 = [np.clip(i + 1, 1, s) for i, s in zip(i1, shape)]
        w = [(d > 0).astype(T) - np.fmod(d, 1) for d in dd]
    return i1, i2, w


def hull(A_o, nodes, dt, dx, dy, dz):
    """(lo, hi) of the limiter: the eight OLD corners of stage 1's own departure cell, visited in the definition's order"""
    T = A_o.dtype.type
    IX, IY, IZ, vxc, vyc, vzc = nodes
    with np.errstate(all="ignore"):
        (x1, y1, z1), (x2, y2, z2), _ = departure(A_o.shape, vxc, vyc, vzc, T(dt), T(dx), T(dy), T(dz), IX, IY, IZ)
        lo = hi = _o(A_o, x1, y1, z1)
        for c in (_o(A_o, x2, y1, z1), _o(A_o, x1, y2, z1), _o(A_o, x2, y2, z1), _o(A_o, x1, y1, z2), _o(A_o, x2, y1, z2),
                  _o(A_o, x1, y2, z2), _o(A_o, x2, y2, z2)):
            lo = np.where(c < lo, c, lo)
            hi = np.where(c > hi, c, hi)
    return lo, hi


def wide_hull(A_o, nodes, dt, dx, dy, dz):
    """(lo, hi) of A_o over ix1−1 … ix2+1 per direction (clamped to the array): every stencil an evaluation whose δ differs from
    this one's by rounding can pick.  For finite fields."""
    T = A_o.dtype.type
    IX, IY, IZ, vxc, vyc, vzc = nodes
    (x1, y1, z1), _, _ = departure(A_o.shape, vxc, vyc, vzc, T(dt), T(dx), T(dy), T(dz), IX, IY, IZ)
    sx, sy, sz = A_o.shape
    lo = hi = _o(A_o, x1, y1, z1)
    for a in range(-1, 3):
        for b in range(-1, 3):
            for c in range(-1, 3):
                v = _o(A_o, np.clip(x1 + a, 1, sx), np.clip(y1 + b, 1, sy), np.clip(z1 + c, 1, sz))
                lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return lo, hi


def stage2_field(A_o, A_hat, nodes, dt, dx, dy, dz, count=None):
    """The new field from the old one and stage 1's complete result; nodes = (IX, IY, IZ, vxc, vyc, vzc) of its advected set.
    count (a dict) receives how many nodes the limiter moved up to lo, down to hi, and left alone."""
    T = A_o.dtype.type
    dt, dx, dy, dz, h = T(dt), T(dx), T(dy), T(dz), T(0.5)
    IX, IY, IZ, vxc, vyc, vzc = nodes
    lo, hi = hull(A_o, nodes, dt, dx, dy, dz)
    with np.errstate(all="ignore"):
        (x1, y1, z1), (x2, y2, z2), (wx, wy, wz) = departure(A_o.shape, vxc, vyc, vzc, T(-dt), dx, dy, dz, IX, IY, IZ)
        L = NR._lerp
        fz1 = L(L(_o(A_hat, x1, y1, z1), _o(A_hat, x2, y1, z1), wx), L(_o(A_hat, x1, y2, z1), _o(A_hat, x2, y2, z1), wx), wy)
        fz2 = L(L(_o(A_hat, x1, y1, z2), _o(A_hat, x2, y1, z2), wx), L(_o(A_hat, x1, y2, z2), _o(A_hat, x2, y2, z2), wx), wy)
        back = L(fz1, fz2, wz)
        s = _o(A_hat, IX, IY, IZ) + h * (_o(A_o, IX, IY, IZ) - back)
        r = np.where(s < lo, lo, s)
        new = np.where(r > hi, hi, r)
        if count is not None:
            count["below"] = int(np.sum(s < lo)); count["above"] = int(np.sum(r > hi))
            count["free"] = int(np.sum((s >= lo) & (s <= hi)))
    out = A_hat.copy(order="F")
    out[IX - 1, IY - 1, IZ - 1] = new.astype(A_o.dtype)
    return out


def stage1(old, dt, dx, dy, dz):
    """ns3d_copy_advect(…, faithful = 0): numpy_ref.advect on copies of the old fields [Vx, Vy, Vz, C] → complete hat fields.
    float32 goes through the C oracle's advect instead, the suite's bit reference of copy_advect in both types: numpy_ref forms
    `IX − δ` from an int64 grid and a float32 array, which NumPy promotes to float64, so for a |δ| below half an ulp of ix its floor
    is not the one of Julia's (and the device's) Float32 subtraction — a handful of nodes on the larger seeded grids.  In float64 the
    two agree bit for bit (tests/test_advect_mc_host.py)."""
    T = old[0].dtype.type
    hat = [a.copy(order="F") for a in old]
    if T is np.float32:
        from oracle import oracle as CO
        CO.advect(hat[0], old[0], hat[1], old[1], hat[2], old[2], hat[3], old[3], dt, dx, dy, dz, False)
        return hat
    with np.errstate(all="ignore"):
        NR.advect(hat[0], old[0], hat[1], old[1], hat[2], old[2], hat[3], old[3], T(dt), T(dx), T(dy), T(dz), faithful=False)
    return hat


def correct(old, hat, dt, dx, dy, dz, counts=None):
    """ns3d_advect_correct: [Vx, Vy, Vz, C] new from old and hat"""
    nx, ny, nz = old[3].shape
    sets = node_sets(old[0], old[1], old[2], nx, ny, nz)
    return [stage2_field(old[q], hat[q], sets[n], dt, dx, dy, dz, None if counts is None else counts.setdefault(n, {}))
            for q, n in enumerate(NAMES)]


def advect_mc(old, dt, dx, dy, dz, counts=None):
    """ns3d_advect_mc: (new, hat), each [Vx, Vy, Vz, C]"""
    hat = stage1(old, dt, dx, dy, dz)
    return correct(old, hat, dt, dx, dy, dz, counts), hat


def scalar_step(C_o, Vx_o, Vy_o, Vz_o, dt, dx, dy, dz, maccormack=True, nodes=None):
    """One step of C alone (the velocities are the caller's, given afresh every step): stage 1 by numpy_ref._backtrack, the function
    numpy_ref.advect's fourth branch calls, then stage 2 — or stage 1 alone, the first-order scheme.  nodes: node_sets(…)["C"] of
    these velocities, for a caller that passes the same ones every step."""
    T = C_o.dtype.type
    nx, ny, nz = C_o.shape
    if nodes is None:
        nodes = node_sets(Vx_o, Vy_o, Vz_o, nx, ny, nz, which=("C",))["C"]
    hat = C_o.copy(order="F")
    NR._backtrack(hat, C_o, nodes[3], nodes[4], nodes[5], T(dt), T(dx), T(dy), T(dz), nodes[0], nodes[1], nodes[2])
    return stage2_field(C_o, hat, nodes, dt, dx, dy, dz) if maccormack else hat


# ---- the convergence case of the issue: a Gaussian blob carried by a uniform flow through the unit box -----------------------------
BLOB = dict(sigma=0.08, centre=(0.3, 0.35, 0.4), velocity=(1.0, 0.5, 0.25), cfl=0.37, T=0.25)


def blob_setup(n, dtype=np.float64):
    """C at t = 0 on the n³ cell centres of the unit box, the uniform velocity fields, dt = 0.37·dx, the number of steps closest to
    T = 0.25 and the exact solution after that many steps"""
    dx = 1.0 / n
    dt = BLOB["cfl"] * dx
    steps = int(round(BLOB["T"] / dt))
    x = (np.arange(n) + 0.5) * dx
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")

    def gauss(t):
        c = [BLOB["centre"][q] + BLOB["velocity"][q] * t for q in range(3)]
        return np.asfortranarray(np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * BLOB["sigma"] ** 2)).astype(dtype))
    V = [np.full(s, v, dtype=dtype, order="F") for s, v in zip(((n + 1, n, n), (n, n + 1, n), (n, n, n + 1)), BLOB["velocity"])]
    return gauss(0.0), V, dt, dx, steps, gauss(steps * dt)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))
