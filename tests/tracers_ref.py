"""The NumPy expression of include/ns3d.h for ns3d_sample and ns3d_tracers_advance — the reference of the tracer tests.

Everything is evaluated on the subset of points that the definition evaluates (alive, finite, inside the closed box; for the second
stage: a finite midpoint), so no NaN is ever cast to an integer.  Positions are (3, N) float64 in index space; fields are column-major
arrays of float64 or float32 and are converted to float64 where they are read.  NumPy never contracts a product into a sum."""
import numpy as np

NAN = np.float64(np.nan)


def lerp(a, b, t):
    return b * t + a * (1.0 - t)


def axis(p, stag, ext):
    """lower node and weight of one direction: (i0, t)"""
    c = p - (0.0 if stag else 0.5)
    c = np.where(c > 0.0, c, 0.0)
    c = np.where(c < ext - 1.0, c, ext - 1.0)
    i0 = np.minimum(np.floor(c).astype(np.int64), ext - 2)
    return i0, c - i0


def interp(A, stag, P):
    """I(A, A.shape, stag, P) for finite points P of shape (3, m)"""
    (i, tx), (j, ty), (k, tz) = (axis(P[q], stag[q], A.shape[q]) for q in range(3))
    a = lambda di, dj, dk: A[i + di, j + dj, k + dk].astype(np.float64)
    fy1z1 = lerp(a(0, 0, 0), a(1, 0, 0), tx)
    fy1z2 = lerp(a(0, 0, 1), a(1, 0, 1), tx)
    fy2z1 = lerp(a(0, 1, 0), a(1, 1, 0), tx)
    fy2z2 = lerp(a(0, 1, 1), a(1, 1, 1), tx)
    fz1 = lerp(fy1z1, fy2z1, ty)
    fz2 = lerp(fy1z2, fy2z2, ty)
    return lerp(fz1, fz2, tz)


def velocity(Vx, Vy, Vz, P):
    return np.stack([interp(Vx, (1, 0, 0), P), interp(Vy, (0, 1, 0), P), interp(Vz, (0, 0, 1), P)])


def inside(X, hi):
    """finite and inside the closed box [0, hi_q] per direction (comparisons with NaN are False)"""
    with np.errstate(invalid="ignore"):
        return np.logical_and.reduce([(X[q] >= 0.0) & (X[q] <= float(hi[q])) for q in range(3)])


def sample(A, X, state=None, stagger=(0, 0, 0)):
    hi = [A.shape[q] - stagger[q] for q in range(3)]
    m = inside(X, hi)
    if state is not None:
        m &= state == 1
    out = np.full(X.shape[1], NAN)
    out[m] = interp(A, stagger, X[:, m])
    return out


def advance(X, state, Vx, Vy, Vz, c):
    """one step: (Xn, state_n, U) — new arrays, the inputs are left alone"""
    n = (Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2])
    c = np.asarray(c, dtype=np.float64).reshape(3, 1)
    act = (state == 1) & inside(X, n)
    Xn = X.copy()
    U = np.full(X.shape, NAN)
    with np.errstate(all="ignore"):
        X0 = X[:, act]
        v1 = velocity(Vx, Vy, Vz, X0)
        Xa = X0 + 0.5 * (v1 * c)
        fin = np.isfinite(Xa).all(axis=0)
        v2 = velocity(Vx, Vy, Vz, Xa[:, fin])
        Xa[:, fin] = X0[:, fin] + v2 * c
    U[:, act] = v1
    Xn[:, act] = Xa
    return Xn, (act & inside(Xn, n)).astype(np.uint8), U


def cell_of(X, n):
    """containing cell (clamped to the grid) of finite points"""
    return np.stack([np.clip(np.floor(X[q]), 0.0, n[q] - 1.0).astype(np.int64) for q in range(3)])


def uniform_points(n, N, seed):
    """N points uniform in the box [0,nx)×[0,ny)×[0,nz), (3, N) float64"""
    rng = np.random.Generator(np.random.MT19937(seed))
    return np.ascontiguousarray(rng.uniform(0.0, 1.0, size=(3, N)) * np.asarray(n, dtype=np.float64).reshape(3, 1))


def planted_points(n):
    """(X, state): per direction the values where the definition decides something — integers, half-integers, 0 (both signs) and n
    exactly, one ulp inside and outside each face, NaN and ±Inf — each combined with ordinary values in the other two directions,
    the corners of the box, and a dead point (state 0) at a perfectly good position"""
    cols = []
    mid = [0.37 * n[0], 0.61 * n[1], 0.43 * n[2]]
    for q in range(3):
        h = float(n[q])
        vals = [0.0, -0.0, h, 1.0, 2.0, h - 1.0, 0.5, 1.5, h - 0.5, np.nextafter(0.0, 1.0), np.nextafter(0.0, -1.0),
                np.nextafter(h, 0.0), np.nextafter(h, 2 * h), np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0),
                np.nextafter(h - 0.5, 0.0), np.nextafter(h - 0.5, h), np.nan, np.inf, -np.inf, -1.0, h + 1.0, 1e300, -1e300]
        for v in vals:
            p = list(mid)
            p[q] = v
            cols.append(p)
    for cx in (0.0, float(n[0])):
        for cy in (0.0, float(n[1])):
            for cz in (0.0, float(n[2])):
                cols.append([cx, cy, cz])
    cols.append(list(mid))
    X = np.ascontiguousarray(np.array(cols, dtype=np.float64).T)
    state = np.ones(X.shape[1], dtype=np.uint8)
    state[-1] = 0
    return X, state
