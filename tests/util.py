"""Shared helpers for the parity tests (seeded synthetic fields, comparison metrics)."""
import numpy as np

SHAPES = {
    "c": lambda nx, ny, nz: (nx, ny, nz),
    "vx": lambda nx, ny, nz: (nx + 1, ny, nz),
    "vy": lambda nx, ny, nz: (nx, ny + 1, nz),
    "vz": lambda nx, ny, nz: (nx, ny, nz + 1),
    "s": lambda nx, ny, nz: (nx - 1, ny - 1, nz - 1),
    "i": lambda nx, ny, nz: (nx - 2, ny - 2, nz - 2),
}


def rnd(seed, shape, dtype=np.float64, lo=-1.0, hi=1.0):
    """U(lo,hi) from a seeded Mersenne Twister (SURVEY.md §8d 'value distributions')."""
    rng = np.random.Generator(np.random.MT19937(seed))
    return np.asfortranarray(rng.uniform(lo, hi, size=shape).astype(dtype))


def fields(nx, ny, nz, kinds, seed0=1, dtype=np.float64):
    return [rnd(seed0 + q, SHAPES[k](nx, ny, nz), dtype) for q, k in enumerate(kinds)]


def rel_l2(a, b, den=None):
    """‖a−b‖₂ / ‖b‖₂ (or / den when a reference norm is given, e.g. the norm of the whole velocity vector for one
    component that is pure round-off by symmetry)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    den = np.sqrt(np.sum(b * b)) if den is None else float(den)
    num = np.sqrt(np.sum((a - b) ** 2))
    return float(num / den) if den > 0 else float(num)


def geometry(nx, ny, nz):
    """Non-trivial, non-power-of-two spacings so that divisions are inexact."""
    return dict(dx=1.0 / nx, dy=0.6 / ny, dz=0.7 / nz, mu=1e-3, rho=1000.0, g=9.81, dt=0.013, dtau=0.009,
                damp=2.0 / nx)


NAMES = ("C", "Pr", "Vx", "Vy", "Vz")


def assert_fields_close(got, ref, tol=1e-6):
    """BASELINE north_star bar: velocity / pressure / tracer fields within `tol` relative L2.  Velocity components are
    measured against the norm of the whole velocity vector: Vz of the z-symmetric cylinder flow is pure round-off
    (≈1e-16) and has no meaningful norm of its own."""
    g, r = dict(zip(NAMES, got)), dict(zip(NAMES, ref))
    vnorm = np.sqrt(sum(np.sum(np.asarray(r[n], dtype=np.float64) ** 2) for n in ("Vx", "Vy", "Vz")))
    for n in NAMES:
        e = rel_l2(g[n], r[n], vnorm if n.startswith("V") else None)
        assert e <= tol, (n, e)


def assert_bit_identical(got, ref, names=NAMES):
    """Values bit for bit; a NaN equals a NaN (runs that follow the reference into its instability exits)."""
    for n, a, b in zip(names, got, ref):
        assert np.array_equal(a, b, equal_nan=True), n


def errs_identical(got, ref):
    """Per-step err histories, value for value; a NaN check (the `!isfinite(err)` exit) equals a NaN check."""
    return len(got) == len(ref) and all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                                       equal_nan=True) for a, b in zip(got, ref))


def checks_inside_margin(errs, eps, margin=1e-3):
    """(step, check, err) of every recorded residual check of a REFERENCE run whose err lies within `margin` (relative) of the
    exit threshold ε.  The FAST build may deviate from the reference by 1e-12 per call and 1e-6 end to end; a check that
    sits 1e-3 away from ε cannot flip for any deviation the suite tolerates, so an empty list means that FAST must stop at
    the very same checks and its iteration counts can be asserted equal (one ulp flips the exit check)."""
    return [(s, q, e) for s, es in enumerate(errs) for q, e in enumerate(es) if not abs(e - eps) > margin * eps]


def bits_equal(a, b):
    """Bit-for-bit (signed zeros included); NaNs compare equal to NaNs whatever their payload."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(u) == b.view(u)) | nan))


def first_bit_difference(a, b):
    """(index, got, want) of the first entry whose bits differ (for assertion messages); None when bits_equal."""
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    bad = (np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)) & ~(np.isnan(a) & np.isnan(b))
    if not bad.any():
        return None
    idx = tuple(int(q) for q in np.argwhere(bad)[0])
    return idx, float(a[idx]).hex(), float(b[idx]).hex(), int(bad.sum())


def hostile(a, seed, mode):
    """A copy of the field `a` (U(−1,1) values) in one of the value patterns that pick the kernels' data-dependent paths — the
    three of test_gpu_pt.py's _extreme_fields and the two parts of a field at rest:
      dense   — 30 % of the entries replaced by zeros, −0, subnormals, tiny and huge magnitudes
      blocks  — contiguous regions scaled to the edge of the subnormal range, a region of exact zeros
      sparse0 — a zero field with a few scattered tiny values
      uniform / rest0 — the parts of a flow at rest: the value 1 everywhere / zeros, half of them −0"""
    dtype = a.dtype
    f64 = dtype == np.float64
    rng = np.random.Generator(np.random.MT19937(seed + 1000))
    edge = (1e-308, 1e-310) if f64 else (1e-38, 1e-40)
    nx, ny, nz = a.shape
    out = a.astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == "dense":
            kind = rng.integers(0, 8, size=a.shape)
            pick = rng.uniform(size=a.shape) < 0.3
            scale = {2: 1e-320 if f64 else 1e-44, 3: 1e-305 if f64 else 1e-37, 4: 1e-250 if f64 else 1e-30,
                     5: 1e-200 if f64 else 1e-12, 6: 1e250 if f64 else 1e22, 7: 1e300 if f64 else 1e30}
            for k, sc in scale.items():
                m = pick & (kind == k)
                out[m] = out[m] * sc
            out[pick & (kind == 0)] = 0.0
            out[pick & (kind == 1)] = -0.0
        elif mode == "blocks":
            out[nx // 3:2 * nx // 3] *= edge[0]
            out[:nx // 3, ny // 2:] *= edge[1]
            out[2 * nx // 3:, :max(ny // 3, 1)] = 0.0
        elif mode == "sparse0":
            pick = rng.uniform(size=a.shape) < 0.02
            for i in (1, nx // 2, 62, 63, 64):
                if i < nx:
                    pick[i] |= rng.uniform(size=(ny, nz)) < 0.2
            out = np.where(pick, out * np.where(rng.uniform(size=a.shape) < 0.5, edge[0], edge[1]), 0.0)
        elif mode == "uniform":
            out = np.full(a.shape, 1.0)
        elif mode == "rest0":
            out = np.where(rng.uniform(size=a.shape) < 0.5, -0.0, 0.0)
        else:
            raise ValueError(mode)
        return np.asfortranarray(out.astype(dtype))
