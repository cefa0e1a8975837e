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
