"""GPU parity at the VALUE edges of the exact-division build (`ns3d_strictx`: every x/d by the known-divisor sequence behind a
per-value guard, the build that runs on every grid whose spacings are not powers of two).

Every comparison here is bitwise (util.bits_equal: raw bits, +0 ≠ −0, a NaN equals a NaN) against the oracle's plain C
divisions in the element type; every case first asserts that the spacings really select the `strictx` build.

 a. planted dividends through update_∇V! and correct_V!: two components zero and the third built so that each cell's
    difference IS a dividend chosen with the exact model of tests/div_model.py — where the unguarded sequence is wrong, where
    the guard of the previous release was wrong, both sides of both guard bounds, ±0, subnormals, ±Inf, NaN;
 b. every once-per-step kernel with a division on hostile value patterns (util.hostile) and on a flow at rest;
"""
import functools
import random
import zlib

import numpy as np
import pytest

import div_model as M
from util import SHAPES, bits_equal, fields, first_bit_difference, geometry, hostile

pytestmark = pytest.mark.gpu

NPT = {"f32": np.float32, "f64": np.float64}
FMT = {np.float32: M.F32, np.float64: M.F64}
REFERENCE_SPACINGS = [1.0 / 63, 0.6 / 38, 1.0 / 255, 0.6 / 153, 0.7 / 5]
SMALL = 1.3 * 2.0 ** -19
# the single-division guard as released before this test existed (ns3d_kernels.hip DivLim): the regression values are the
# dividends at which THAT guard let a wrong quotient through
PARENT_DIVLIM = {"f32": (2.0 ** -100, 2.0 ** 100), "f64": (2.0 ** -900, 2.0 ** 900)}
PLANT_GRID = (130, 5, 4)          # rows of 130 / 131 cells: more than two wave64s, not a multiple of 64


def _assert_bits(got, ref, what):
    assert bits_equal(got, ref), "%s: first difference (index, got, want, count) %r" % (what, first_bit_difference(got, ref))


def _strictx(ctx, dx, dy, dz):
    assert ctx.arith_build(dx, dy, dz) == "strictx", (dx, dy, dz, ctx.arith_build(dx, dy, dz))


def _plant_divisors(fmt):
    ext = M.admitted_extremes(fmt)
    return REFERENCE_SPACINGS + [ext[0], ext[2], SMALL]


@functools.lru_cache(maxsize=None)
def _planted_dividends(fname, d):
    """Dividends (an array of the element type) for the divisor d, from the exact model; deterministic."""
    fmt = {"f32": M.F32, "f64": M.F64}[fname]
    rng = random.Random(zlib.crc32((fname + float(d).hex()).encode()))
    db = M.divisor_of(fmt, d)
    bits = []
    bits += M.wrong_dividends(fmt, rng, db, None, 60, tries=2000)                       # the unguarded sequence is wrong here
    parent = tuple(M.to_bits(fmt, v) for v in PARENT_DIVLIM[fname])
    bits += M.wrong_dividends(fmt, rng, db, parent, 40, tries=6000 if d < 2.0 ** -17 else 1500)   # the previous guard was wrong here
    if fname == "f32" and d == SMALL:
        bits.append(M.to_bits(fmt, 7.336370446077286e-36))                             # the recorded counter-example, by value
    for bound in M.CONST["DivLim"][fname] + parent:                                    # both sides of every bound, old and new
        bits += M.dividends_for_quotient_bound(fmt, rng, db, bound, 120)
    sub = [1, 2, fmt.hidden - 1, fmt.hidden, fmt.hidden + 1] + [rng.getrandbits(fmt.p - 1) for _ in range(20)]
    special = [0, fmt.inf - 1, fmt.inf, fmt.nan] + sub
    bits += special + [b | fmt.sign_bit for b in special] + [0, fmt.sign_bit] * 20
    bits += [M._rand_in_binade(fmt, rng, rng.randrange(-8, 8)) for _ in range(200)]     # ordinary values: fast-path lanes in every wave
    rng.shuffle(bits)
    u = np.uint32 if fname == "f32" else np.uint64
    return np.array(bits, dtype=u).view(NPT[fname])


def _planted_field(shape, axis, x):
    """A field that is 0 / x alternating along `axis`, so that consecutive differences along it are +x, −x, +x …; one x-row
    of planted values is all zeros (of both signs) and one is zeros with a single outlier (a flow at rest, and at rest but for one cell)."""
    F = np.zeros(shape, dtype=x.dtype, order="F")
    idx = [slice(None)] * 3
    idx[axis] = slice(1, None, 2)
    slots = F[tuple(idx)]
    vals = np.resize(x, slots.size).reshape(slots.shape, order="F").copy(order="F")
    if axis == 0:
        vals[:, 0, 0] = 0.0; vals[1::2, 0, 0] = -0.0
        vals[:, 1, 0] = 0.0; vals[35, 1, 0] = x[np.isfinite(x) & (x != 0)][0]
    else:
        other = [q for q in (1, 2) if q != axis][0]
        row0, row1 = [slice(None)] * 3, [slice(None)] * 3
        row0[axis], row0[other] = 0, 0
        row1[axis], row1[other] = 0, 1
        vals[tuple(row0)] = 0.0; vals[tuple(row0)][1::2] = -0.0
        vals[tuple(row1)] = 0.0
        one = list(row1); one[0] = 70
        vals[tuple(one)] = x[np.isfinite(x) & (x != 0)][0]
    F[tuple(idx)] = vals
    return F


def _signed_zero_field(shape, dtype, axis):
    """Zeros, −0 at the odd indices along `axis`: the differences along it are −0, +0, −0 … (a component at rest whose quotient
    keeps the sign of a −0 sum alive in every second cell)."""
    F = np.zeros(shape, dtype=dtype, order="F")
    idx = [slice(None)] * 3
    idx[axis] = slice(1, None, 2)
    F[tuple(idx)] = -0.0
    return F


def test_reference_spacings_stay_in_the_exact_division_build(hip):
    """The spacings of the reference's configurations (and 1/512 beside a spacing that is no power of two) select `strictx`;
    so do the admitted divisors nearest each end of the host's range, and nothing just outside it."""
    ctx = hip.Context(0, "strict")
    for d in REFERENCE_SPACINGS + [1.0 / 512, SMALL, 3.0]:
        assert ctx.arith_build(d, 0.6 / 38, 0.7 / 5) == "strictx", d
    assert ctx.arith_build(1.0 / 255, 0.6 / 153, 0.6 / 153) == "strictx" and ctx.arith_build(1.0 / 63, 0.6 / 38, 0.6 / 38) == "strictx"
    for fmt in (M.F32, M.F64):
        for d in M.admitted_extremes(fmt):
            assert ctx.arith_build(d, d, d) == "strictx", d
    lo, _, hi, _ = M.admitted_extremes(M.F64)
    for d in (float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, np.inf)), float(np.nextafter(2.0, 0.0))):
        assert ctx.arith_build(d, 0.6 / 38, 0.7 / 5) == "strict", d
    ctx.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_dividends_through_update_divV(hip, oracle, dtype, axis):
    """∇V = ((Vx[i+1]−Vx[i])/dx + 0/dy) + 0/dz with the differences planted: every cell is RN(±x/d) (or a signed zero)."""
    import torch
    nx, ny, nz = PLANT_GRID
    fmt = FMT[dtype]
    kinds = ["vx", "vy", "vz"]
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for d in _plant_divisors(fmt):
            _strictx(ctx, d, d, d)
            x = _planted_dividends(fmt.name, d)
            V = [_signed_zero_field(SHAPES[k](nx, ny, nz), dtype, q) for q, k in enumerate(kinds)]
            V[axis] = _planted_field(SHAPES[kinds[axis]](nx, ny, nz), axis, x)
            ref = np.zeros((nx, ny, nz), dtype=dtype, order="F")
            oracle.update_divV(ref, *V, d, d, d)
            out = hip.from_numpy(np.full_like(ref, 777.0))
            hip.update_divV(out, *[hip.from_numpy(a) for a in V], d, d, d, ctx=ctx)
            torch.cuda.synchronize()
            _assert_bits(hip.to_numpy(out), ref, "update_divV %s axis %d d=%r" % (fmt, axis, d))
            # the oracle's cells ARE the plain quotients of the planted differences (NumPy's x/d in the element type)
            diff = np.diff(V[axis], axis=axis)
            want = diff / dtype(d)
            m = np.isfinite(want) & (want != 0)
            assert m.sum() > 500 and bits_equal(ref[m], want[m])
    ctx.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_dividends_through_correct_V(hip, oracle, dtype, axis):
    """V − (dt/ρ·(Pr[i]−Pr[i−1]))/d with dt/ρ = 1, V = −0 and the pressure differences planted: every updated entry is
    −RN(±x/d), and a zero quotient shows its sign (−0 − (+0) = −0, −0 − (−0) = +0)."""
    import torch
    nx, ny, nz = PLANT_GRID
    fmt = FMT[dtype]
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for d in _plant_divisors(fmt):
            _strictx(ctx, d, d, d)
            Pr = _planted_field((nx, ny, nz), axis, _planted_dividends(fmt.name, d))
            V = [np.asfortranarray(np.full(SHAPES[k](nx, ny, nz), -0.0, dtype=dtype)) for k in ("vx", "vy", "vz")]
            ref = [a.copy(order="F") for a in V]
            oracle.correct_V(*ref, Pr, 1.0, 1.0, d, d, d)
            dev = [hip.from_numpy(a) for a in V]
            hip.correct_V(*dev, hip.from_numpy(Pr), 1.0, 1.0, d, d, d, ctx=ctx)
            torch.cuda.synchronize()
            for q in range(3):
                _assert_bits(hip.to_numpy(dev[q]), ref[q], "correct_V %s planted axis %d output %d d=%r" % (fmt, axis, q, d))
            assert (np.signbit(ref[axis]) & (ref[axis] == 0)).any() and (~np.signbit(ref[axis]) & (ref[axis] == 0)).any()
    ctx.close()


# ---- b. hostile value patterns through every once-per-step kernel with a division -------------------------------------------
PATTERNS = ["dense", "blocks", "sparse0", "rest"]
EDGE_GRIDS = [(70, 9, 7), (131, 6, 5)]
# what each kind of field is in a flow at rest: Vx uniform, everything else zero with −0 sprinkled in
REST = {"vx": "uniform", "vy": "rest0", "vz": "rest0", "c": "rest0", "s": "rest0", "i": "rest0"}


def _spacing_sets(grid, dtype):
    g = geometry(*grid)
    lo, lo1, hi, hi1 = M.admitted_extremes(FMT[dtype])
    return [(g["dx"], g["dy"], g["dz"]), (1.0 / 255, 0.6 / 153, 0.6 / 153), (lo, SMALL, lo1), (hi, hi1 / 2, hi1)]


def _pattern_fields(grid, kinds, dtype, seed, pattern, rest=None):
    base = fields(*grid, kinds, seed, dtype)
    return [hostile(a, seed + 17 * q, (rest or REST)[k] if pattern == "rest" else pattern) for q, (a, k) in enumerate(zip(base, kinds))]


def _both(hip, oracle, ctx, name, host, scalars, out_idx, what, kwargs=None):
    import torch
    kwargs = kwargs or {}
    ref = [a.copy(order="F") for a in host]
    getattr(oracle, name)(*ref, *scalars, **kwargs)
    dev = [hip.from_numpy(a) for a in host]
    getattr(hip, name)(*dev, *scalars, ctx=ctx, **kwargs)
    torch.cuda.synchronize()
    for q in out_idx:
        _assert_bits(hip.to_numpy(dev[q]), ref[q], "%s output %d, %s" % (name, q, what))
    for q in range(len(host)):
        if q not in out_idx:
            _assert_bits(hip.to_numpy(dev[q]), host[q], "%s input %d, %s" % (name, q, what))
    return ref, dev


def _cases(dtype):
    for grid in EDGE_GRIDS:
        for sp in _spacing_sets(grid, dtype):
            yield grid, geometry(*grid), sp


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stress_and_predictor_on_hostile_values(hip, oracle, dtype, pattern):
    """update_τ!, predict_V! and the fused predictor (update_τ! then predict_V! without storing the stresses)."""
    import torch
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for grid, g, (dx, dy, dz) in _cases(dtype):
            _strictx(ctx, dx, dy, dz)
            what = "%s %s grid %r spacings %r" % (dtype.__name__, pattern, grid, (dx, dy, dz))
            host = _pattern_fields(grid, ["c", "c", "c", "s", "s", "s", "vx", "vy", "vz"], dtype, 1, pattern)
            _both(hip, oracle, ctx, "update_tau", host, (g["mu"], dx, dy, dz), range(6), what)
            host = _pattern_fields(grid, ["vx", "vy", "vz", "c", "c", "c", "s", "s", "s"], dtype, 2, pattern)
            _both(hip, oracle, ctx, "predict_V", host, (g["rho"], g["g"], g["dt"], dx, dy, dz), range(3), what)
            # fused: complete predicted fields from the velocities alone
            V = _pattern_fields(grid, ["vx", "vy", "vz"], dtype, 3, pattern)
            nx, ny, nz = grid
            tau = [np.zeros(SHAPES[k](nx, ny, nz), dtype=dtype, order="F") for k in "cccsss"]
            ref = [a.copy(order="F") for a in V]
            oracle.update_tau(*tau, *ref, g["mu"], dx, dy, dz)
            oracle.predict_V(*ref, *tau, g["rho"], g["g"], g["dt"], dx, dy, dz)
            dV = [hip.from_numpy(a) for a in V]
            out = [hip.from_numpy(np.full_like(a, 777.0)) for a in V]
            hip.predict_fused(*out, *dV, g["mu"], g["rho"], g["g"], g["dt"], dx, dy, dz, ctx=ctx)
            torch.cuda.synchronize()
            for q in range(3):
                _assert_bits(hip.to_numpy(out[q]), ref[q], "predict_fused output %d, %s" % (q, what))
    ctx.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_divergence_and_corrector_on_hostile_values(hip, oracle, dtype, pattern):
    """update_∇V!, correct_V!, and the flow monitor's max|∇V| (= max|·| of update_∇V!'s output over the interior cells,
    NaN-propagating)."""
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for grid, g, (dx, dy, dz) in _cases(dtype):
            _strictx(ctx, dx, dy, dz)
            nx, ny, nz = grid
            what = "%s %s grid %r spacings %r" % (dtype.__name__, pattern, grid, (dx, dy, dz))
            host = _pattern_fields(grid, ["c", "vx", "vy", "vz"], dtype, 4, pattern)
            ref, dev = _both(hip, oracle, ctx, "update_divV", host, (dx, dy, dz), [0], what)
            div = ref[0][1:-1, 1:-1, 1:-1].astype(np.float64)    # div_max is taken over the interior cells (@inn(∇V))
            want = float("nan") if np.isnan(div).any() else float(np.abs(div).max())
            got = hip.diagnostics(dev[1], dev[2], dev[3], None, None, hip.diag_params(nx, ny, nz, dx, dy, dz, g["rho"]), ctx=ctx).div_max
            assert (np.isnan(want) and np.isnan(got)) or got == want, ("diagnostics div_max", what, got, want)
            host = _pattern_fields(grid, ["vx", "vy", "vz", "c"], dtype, 5, pattern)
            _both(hip, oracle, ctx, "correct_V", host, (g["dt"], g["rho"], dx, dy, dz), range(3), what)
            if pattern == "rest":                                # dt/ρ = 1 keeps a tiny or zero difference what it is
                _both(hip, oracle, ctx, "correct_V", host, (1.0, 1.0, dx, dy, dz), range(3), what + " dt/rho=1")
    ctx.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pressure_kernels_on_hostile_values(hip, oracle, dtype, pattern):
    """update_dPrdτ!, compute_res! and residual_max (= maximum(abs.(Rp)) after the oracle's compute_res!)."""
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for grid, g, (dx, dy, dz) in _cases(dtype):
            _strictx(ctx, dx, dy, dz)
            what = "%s %s grid %r spacings %r" % (dtype.__name__, pattern, grid, (dx, dy, dz))
            host = _pattern_fields(grid, ["c", "i", "c"], dtype, 6, pattern)
            _both(hip, oracle, ctx, "update_dPrdtau", host, (g["rho"], g["dt"], g["dtau"], g["damp"], dx, dy, dz), [1], what)
            host = _pattern_fields(grid, ["i", "c", "c"], dtype, 7, pattern)
            ref, dev = _both(hip, oracle, ctx, "compute_res", host, (g["rho"], g["dt"], dx, dy, dz), [0], what)
            p = hip.pt_params(dev[1], g["rho"], g["dt"], g["dtau"], g["damp"], dx, dy, dz, 0, True, 0.0, g["g"], False, False)
            got, want = hip.residual_max(dev[1], dev[2], p, ctx=ctx), oracle.max_abs(ref[0])
            assert (np.isnan(want) and np.isnan(got)) or got == want, ("residual_max", what, got, want)
    ctx.close()


def _advect_both(hip, oracle, ctx, old, dt, sp, what):
    import torch
    dx, dy, dz = sp
    do = [hip.from_numpy(a) for a in old]
    for faithful in (True, False):
        ref = [np.asfortranarray(np.full_like(a, 777.0)) for a in old]
        oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, dx, dy, dz, faithful)
        d = [hip.from_numpy(np.full_like(a, 777.0)) for a in old]
        hip.advect(d[0], do[0], d[1], do[1], d[2], do[2], d[3], do[3], dt, dx, dy, dz, faithful, ctx=ctx)
        torch.cuda.synchronize()
        for q in range(4):
            _assert_bits(hip.to_numpy(d[q]), ref[q], "advect output %d faithful=%s, %s" % (q, faithful, what))


@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_advect_on_hostile_values(hip, oracle, dtype, form, monkeypatch):
    """advect! in both forms (the LDS-windowed kernel and the global gather).  The departure offset δ = dt·v/d must stay below one
    cell, so (i) the ADVECTED tracer takes the hostile patterns under ordinary velocities, and (ii) the velocities are scaled so
    that the quotient dt·v/d lands on both sides of the guard's lower bound, on zeros and on −0 (|δ| ≪ 1)."""
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    fmt = FMT[dtype]
    lo_exp = M._exponent(fmt, M.CONST["DivLim"][fmt.name][0])
    ctx = hip.Context(0, "strict")
    with np.errstate(all="ignore"):
        for grid, g, sp in _cases(dtype):
            _strictx(ctx, *sp)
            dmin = min(sp)
            dt = 0.7 * dmin                                       # |v| < 1: |δ| < 0.7
            V = fields(*grid, ["vx", "vy", "vz"], 21, dtype)
            for pattern in PATTERNS:
                Cf = _pattern_fields(grid, ["c"], dtype, 8, pattern, rest={"c": "rest0"})[0]
                _advect_both(hip, oracle, ctx, V + [Cf], dt, sp, "%s tracer %s grid %r spacings %r" % (dtype.__name__, pattern, grid, sp))
            # (ii) velocities with the quotient dt·v/d within four binades of the guard's lower bound, and of the smallest normal
            # number (where an unguarded sequence mis-rounds; dt·v is subnormal there), zeros and −0 among them.  The tracer is
            # the dense pattern: where its west value is an exact zero the result is C_east·|δ|, the quotient itself.
            Cf = _pattern_fields(grid, ["c"], dtype, 9, "dense")[0]
            for centre in (lo_exp, fmt.emin):
                rng = np.random.Generator(np.random.MT19937(99))
                tiny = []
                for a, d in zip(V, sp):
                    e = rng.integers(centre - 4, centre + 4, size=a.shape).astype(np.float64)
                    q = (a.astype(np.float64) * np.exp2(e)).astype(dtype)       # the quotient aimed at, in the element type
                    v = q.astype(np.float64) * (d / dt)
                    z = rng.uniform(size=a.shape)
                    v = np.where(z < 0.1, 0.0, np.where(z < 0.2, -0.0, np.where(z < 0.4, a.astype(np.float64), v)))
                    tiny.append(np.asfortranarray(v.astype(dtype)))
                _advect_both(hip, oracle, ctx, tiny + [Cf], dt, sp,
                             "%s velocities with quotients around 2^%d, grid %r spacings %r" % (dtype.__name__, centre, grid, sp))
    ctx.close()
