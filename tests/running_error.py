"""Running-error reference for the FAST build: every value travels with a bound on its distance from the exact result.

A `Pair` holds an fp64 value `v` and an fp64 bound `e ≥ |v − exact|`, where `exact` is the expression evaluated in real
arithmetic on the same inputs.  Arithmetic on pairs is Higham's running error analysis (Accuracy and Stability of Numerical
Algorithms, §3.3): an operation of the element type returns fl(x∘y) = (x∘y)(1+δ), |δ| ≤ u, so the bound of a result is the
input bounds propagated through the operation plus u·|result|, u = 2⁻²⁴ (float32) or 2⁻⁵³ (float64).  Two further terms make the
bound rigorous rather than first-order: one smallest subnormal of the element type per product or quotient (gradual underflow
replaces the relative error by an absolute one; a sum that lands in the subnormal range is exact) and a factor 1+2⁻²⁰ on the whole (the rounding is relative to the value the kernel has, which
differs from `v` by at most the bound: u·e ≤ 2⁻²⁰·e; the same factor absorbs the roundings of this fp64 bookkeeping itself and a
constant rounded twice, (T)(double expression)).  An operation with an exactly-zero operand (v = 0, e = 0) is exact — x+0, x·0,
0/x — and is charged nothing: a flow at rest keeps the bound 0 and must then come out bit for bit.  Multiplying or dividing by a
power-of-two constant (0.25·Σ, dx/2) is exact up to underflow and is charged the subnormal only.

ONE BOUND FOR EVERY CONTRACTION.  FAST is compiled with -ffp-contract=fast: the compiler may fuse any product into the sum that
consumes it.  fma(a,b,c) = (a·b+c)(1+δ) makes ONE rounding where the product and the sum make two, so its error u·|a·b+c| is no
larger than what the mul and the add are charged here (u·|a·b| + u·|a·b+c|).  Contraction only ever removes terms from the sum of
roundings; it does not reassociate.  The bound of the uncontracted tree therefore holds for every choice the compiler may make,
and for STRICT and the C oracle, which make none.

DIVISIONS BY A GRID SPACING are charged 3u (`spacing()` marks such a divisor; a literal constant such as the 3.0 of ∇V/3 is
treated alike).  From make_geo (ns3d_kernels.hip), with d the double spacing the caller passed and the pair value computed as x/d:
    g.dx  = (T)d                      d(1+ε₁)                                       one rounding
    g.rdx = (T)1 / g.dx               (1/d)(1+ε₁)⁻¹(1+ε₂)                           a second
    FAST  x·g.rdx                     (x/d)(1+ε₁)⁻¹(1+ε₂)(1+ε₃)                     a third: 3u to first order
    STRICT x / g.dx                   (x/d)(1+ε₁)⁻¹(1+ε₂)                           2u
    g.rdx2 = (T)(1.0/(d·d))           (1/d²)(1+ε₄), ε₄ ≤ u(1+2⁻²⁹)                   so x·g.rdx2 is within 2u of x/d/d
    STRICT x / g.dx / g.dx            (x/d²)(1+ε₁)⁻²(1+ε₂)(1+ε₃)                    4u
x/d/d is two such divisions, 6u, and covers both.  (The second-order terms are inside the factor 1+2⁻²⁰.)

MEANING.  For float32 fields the pair value is computed in fp64 on the float32 inputs: its own error (2⁻⁵³ per operation) is
2⁻²⁹ of the bound and inside the factor, so a conforming kernel satisfies |out − v| ≤ e.  For float64 fields the pair value is
itself one conforming evaluation: it and the kernel are both within e of the exact result, hence |FAST − oracle| ≤ 2e
(`allowed()` returns the factor).

Scalars enter as 0-d pairs holding the value the kernel's launcher converts them to ((T)mu, (T)dt …), bound 0, so that
`dt / rho`, `1.0 - damp`, `rho * g` are charged the rounding the launcher makes.  The transcriptions of oracle/numpy_ref.py run on
pairs unchanged (slicing, `A[...] = expr`); `backtrack` below is the pair version of numpy_ref._backtrack, which cannot be
duck-typed (floor, clip, fancy indexing), mirrored line by line, with the classification of its comparisons.

A comparison is DECIDED when the enclosure [v−e, v+e] of its operand lies strictly on one side of every breakpoint (or e = 0:
the operand is the same number in every conforming evaluation); otherwise a conforming kernel may take either side.
"""
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
SLACK = 1.0 + 2.0 ** -20


def unit(dtype):
    return U32 if np.dtype(dtype) == np.float32 else U64


def _tiny(u):
    return 2.0 ** -149 if u == U32 else 2.0 ** -1074


def _pow2(c):
    return c != 0 and math.isfinite(c) and math.frexp(abs(c))[0] == 0.5


class Pair:
    __array_ufunc__ = None          # ndarray ∘ Pair defers to Pair.__r*__

    def __init__(self, v, e=None, u=U64, recip=False):
        self.v = v if isinstance(v, np.ndarray) and v.dtype == np.float64 else np.array(v, dtype=np.float64)
        self.e = np.zeros(self.v.shape) if e is None else (e if isinstance(e, np.ndarray) else np.full(self.v.shape, float(e)))
        self.u, self.recip = u, recip

    # ---- container behaviour ----
    shape = property(lambda self: self.v.shape)
    ndim = property(lambda self: self.v.ndim)

    def copy(self):
        return Pair(self.v.copy(order="F"), self.e.copy(order="F"), self.u, self.recip)

    def __getitem__(self, idx):
        return Pair(self.v[idx], self.e[idx], self.u)

    def __setitem__(self, idx, val):
        if isinstance(val, Pair):
            self.v[idx], self.e[idx] = val.v, val.e
        else:
            self.v[idx], self.e[idx] = val, 0.0

    # ---- arithmetic ----
    def _lift(self, o):
        """(value, bound, exact power-of-two constant?, reciprocal-style divisor?)"""
        if isinstance(o, Pair):
            return o.v, o.e, False, o.recip
        if isinstance(o, (int, float, np.integer, np.floating)):
            return np.float64(o), np.float64(0.0), _pow2(float(o)), not _pow2(float(o))
        return np.asarray(o, dtype=np.float64), np.float64(0.0), False, False

    def _out(self, v, e):
        return Pair(np.asarray(v, dtype=np.float64), np.asarray(e * SLACK, dtype=np.float64), self.u)

    def _add(self, av, ae, bv, be):
        with np.errstate(all="ignore"):
            v = av + bv
            exact = ((av == 0) & (ae == 0)) | ((bv == 0) & (be == 0))
            return self._out(v, ae + be + np.where(exact, 0.0, self.u * np.abs(v)))      # no subnormal: a sum never underflows inexactly

    def _mul(self, av, ae, bv, be, p2):
        with np.errstate(all="ignore"):
            v = av * bv
            exact = ((av == 0) & (ae == 0)) | ((bv == 0) & (be == 0))
            rnd = (0.0 if p2 else self.u * np.abs(v)) + _tiny(self.u)
            return self._out(v, np.abs(av) * be + np.abs(bv) * ae + ae * be + np.where(exact, 0.0, rnd))

    def _div(self, av, ae, bv, be, p2, recip):
        with np.errstate(all="ignore"):
            v = av / bv
            exact = (av == 0) & (ae == 0)
            if p2:
                rnd = _tiny(self.u)
            else:
                rnd = (3.0 if recip else 1.0) * self.u * np.abs(v) + _tiny(self.u)
            den = np.abs(bv) - be
            prop = np.where(den > 0, (ae + np.abs(v) * be) / den, np.inf)
            return self._out(v, np.where(exact, 0.0, prop + rnd))

    def __add__(self, o):
        bv, be, _, _ = self._lift(o)
        return self._add(self.v, self.e, bv, be)
    __radd__ = __add__

    def __sub__(self, o):
        bv, be, _, _ = self._lift(o)
        return self._add(self.v, self.e, -bv, be)

    def __rsub__(self, o):
        bv, be, _, _ = self._lift(o)
        return self._add(bv, be, -self.v, self.e)

    def __neg__(self):
        return Pair(-self.v, self.e, self.u)

    def __mul__(self, o):
        bv, be, p2, _ = self._lift(o)
        return self._mul(self.v, self.e, bv, be, p2)
    __rmul__ = __mul__

    def __truediv__(self, o):
        bv, be, p2, recip = self._lift(o)
        return self._div(self.v, self.e, bv, be, p2, recip)

    def __rtruediv__(self, o):
        av, ae, _, _ = self._lift(o)
        return self._div(av, ae, self.v, self.e, False, self.recip)

    def __lt__(self, o):
        raise TypeError("a comparison of pairs has no single answer: classify it with decided_below()")
    __le__ = __gt__ = __ge__ = __lt__


def field(a, u=None):
    """a kernel input (exact: bound 0) of the element type of `a`"""
    return Pair(np.asfortranarray(a, dtype=np.float64).copy(order="F"), None, unit(a.dtype) if u is None else u)


def scalar(x, dtype):
    """a scalar argument as the launcher hands it to the kernel: converted to the element type, exact from there on"""
    return Pair(float(np.dtype(dtype).type(x)), None, unit(dtype))


def spacing(d, dtype):
    """a grid spacing that the expression DIVIDES by: the double the caller passed, the division charged 3u (module docstring)"""
    return Pair(float(d), None, unit(dtype), recip=True)


def allowed(dtype):
    """multiple of the bound that two conforming results may differ by: 1 against the pair value (float32), 2 between two
    float64 evaluations"""
    return 1.0 if np.dtype(dtype) == np.float32 else 2.0


def check(got, ref, pair, dtype, what=""):
    """Per-element comparison of a kernel output with the pair reference.  float32: |got − v| ≤ e; float64: |got − ref| ≤ 2e with
    `ref` the oracle's output (or the pair value itself).  Where the bound is 0 the error must be 0 and, when `ref` is an array of
    the element type, the bits must be its bits.  Returns the worst err/bound (0/0 counts as 0); raises AssertionError naming the
    first offending index, the value, the reference and the bound."""
    got = np.asarray(got)
    f32 = np.dtype(dtype) == np.float32
    target = pair.v if f32 else np.asarray(ref, dtype=np.float64)
    bound = allowed(dtype) * pair.e
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - target)
        zero = bound == 0
        same = err == 0
        if ref is not None and np.asarray(ref).dtype == got.dtype:
            uint = np.uint32 if got.dtype == np.float32 else np.uint64
            same = same & (np.ascontiguousarray(got).view(uint) == np.ascontiguousarray(ref).view(uint))
        bad = np.where(zero, ~same, ~(err <= bound))
        ratio = np.where(zero, np.where(same, 0.0, np.inf), err / np.where(zero, 1.0, bound))
    if bad.any():
        idx = tuple(int(q) for q in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d outside the bound; first at %r: got %r, reference %r, bound %.3e (err %.3e)" % (
            what, int(bad.sum()), bad.size, idx, float(got[idx]), float(target[idx]), float(bound[idx]), float(err[idx])))
    return float(ratio.max()) if ratio.size else 0.0


def tightness(pair):
    """median of e/(u·|v|) over the elements whose |v| exceeds the field's median |v|"""
    a = np.abs(pair.v)
    m = a > np.median(a)
    return float(np.median(pair.e[m] / (pair.u * a[m]))) if m.any() else 0.0


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def decided_below(p, thr):
    """(certainly p < thr, certainly not p < thr) per element; neither where the enclosure reaches thr (an exact operand, e = 0,
    is decided wherever it lies: `<` is false AT thr in every evaluation)"""
    lo, hi = p.v - p.e, p.v + p.e
    return hi < thr, (lo > thr) | ((p.e == 0) & (p.v >= thr))


def _same_floor(p):
    """floor(x) is the same for every x in the enclosure of p"""
    lo, hi = p.v - p.e, p.v + p.e
    return (np.floor(lo) == np.floor(hi)) & ((lo > np.floor(lo)) | (p.e == 0))


def _same_trunc_and_sign(p):
    """δ > 0 and trunc(δ) (hence δ%1 up to the bound) are the same for every δ in the enclosure"""
    lo, hi = p.v - p.e, p.v + p.e
    exact = p.e == 0
    sign = (lo > 0) | (hi < 0) | exact
    inner = (np.trunc(lo) == np.trunc(hi)) & ((lo != np.trunc(lo)) | (lo == 0)) & ((hi != np.trunc(hi)) | (hi == 0))
    return sign & (inner | exact)


def _lerp(a, b, t):                                                 # numpy_ref._lerp
    return b * t + a * (1 - t)


def backtrack(A_o, vxc, vyc, vzc, dt, dx, dy, dz, IX, IY, IZ):
    """numpy_ref._backtrack on pairs, line by line.  Returns (value pair, decided mask, lo, hi): `decided` where every comparison of
    all three axes is decided — there the value is the pair interpolant; elsewhere [lo, hi] is the range of the old field over the
    union of the stencils a conforming evaluation may pick (the interpolant is a convex combination of whichever it picks)."""
    sx, sy, sz = A_o.shape
    one = lambda n: Pair(np.asarray(n, dtype=np.float64), None, A_o.u)
    ddx, ddy, ddz = dt * vxc / dx, dt * vyc / dy, dt * vzc / dz
    px, py, pz = one(IX) - ddx, one(IY) - ddy, one(IZ) - ddz                       # (T)ix − δ: one rounding in the element type
    decided = np.ones(IX.shape, dtype=bool)
    for p, d in ((px, ddx), (py, ddy), (pz, ddz)):
        decided &= _same_floor(p) & _same_trunc_and_sign(d)
    clipi = lambda x, hi: np.clip(np.nan_to_num(x, nan=1.0, posinf=1e18, neginf=-1e18), 1, hi).astype(np.int64)
    ix1, iy1, iz1 = clipi(np.floor(px.v), sx), clipi(np.floor(py.v), sy), clipi(np.floor(pz.v), sz)
    ix2, iy2, iz2 = np.clip(ix1 + 1, 1, sx), np.clip(iy1 + 1, 1, sy), np.clip(iz1 + 1, 1, sz)
    # δ%1 is exact in every format (fmod; the kernel's δ − trunc δ), so on a decided axis the weight inherits δ's bound and the
    # subtraction from 0 or 1 makes one rounding
    frac = lambda d: Pair(np.fmod(d.v, 1), d.e, d.u)
    wx = (ddx.v > 0).astype(np.float64) - frac(ddx)
    wy = (ddy.v > 0).astype(np.float64) - frac(ddy)
    wz = (ddz.v > 0).astype(np.float64) - frac(ddz)
    g = lambda i, j, k: A_o[i - 1, j - 1, k - 1]
    fy1z1 = _lerp(g(ix1, iy1, iz1), g(ix2, iy1, iz1), wx)
    fy1z2 = _lerp(g(ix1, iy1, iz2), g(ix2, iy1, iz2), wx)
    fy2z1 = _lerp(g(ix1, iy2, iz1), g(ix2, iy2, iz1), wx)
    fy2z2 = _lerp(g(ix1, iy2, iz2), g(ix2, iy2, iz2), wx)
    fz1 = _lerp(fy1z1, fy2z1, wy)
    fz2 = _lerp(fy1z2, fy2z2, wy)
    val = _lerp(fz1, fz2, wz)
    # undecided entries (rare): hull of the old field over every stencil the enclosure admits
    lo, hi = val.v.copy(), val.v.copy()
    for idx in np.argwhere(~decided):
        idx = tuple(idx)
        sl = []
        for p, n in ((px, sx), (py, sy), (pz, sz)):
            a = int(clipi(np.floor(p.v[idx] - p.e[idx]), n))
            b = min(int(clipi(np.floor(p.v[idx] + p.e[idx]), n)) + 1, n)
            sl.append(slice(a - 1, b))
        box = A_o.v[tuple(sl)]
        lo[idx], hi[idx] = box.min(), box.max()
    return val, decided, lo, hi


def advect(Vx_o, Vy_o, Vz_o, C_o, dt, dx, dy, dz, faithful=True):
    """numpy_ref.advect on pairs: the four back-tracks in the reference's order.  Returns a list of
    (name, index tuple of the written entries, value pair, decided, lo, hi); in faithful mode Vy is written twice and the later
    entry (branch 3) overrides the earlier one where both write."""
    nx, ny, nz = C_o.shape

    def grid(xs, ys, zs):
        return np.meshgrid(np.asarray(xs), np.asarray(ys), np.asarray(zs), indexing="ij")
    o = lambda A, i, j, k: A[i - 1, j - 1, k - 1]
    out = []

    def bt(name, A_o, vxc, vyc, vzc, IX, IY, IZ):
        out.append((name, (IX - 1, IY - 1, IZ - 1)) + backtrack(A_o, vxc, vyc, vzc, dt, dx, dy, dz, IX, IY, IZ))
    IX, IY, IZ = grid(range(2, nx + 1), range(1, ny + 1), range(1, nz + 1))
    vxc = o(Vx_o, IX, IY, IZ)
    vyc = 0.25 * (((o(Vy_o, IX - 1, IY, IZ) + o(Vy_o, IX - 1, IY + 1, IZ)) + o(Vy_o, IX, IY, IZ)) + o(Vy_o, IX, IY + 1, IZ))
    vzc = 0.25 * (((o(Vz_o, IX - 1, IY, IZ) + o(Vz_o, IX - 1, IY, IZ + 1)) + o(Vz_o, IX, IY, IZ)) + o(Vz_o, IX, IY, IZ + 1))
    bt("Vx", Vx_o, vxc, vyc, vzc, IX, IY, IZ)
    IX, IY, IZ = grid(range(1, nx + 1), range(2, ny + 1), range(1, nz + 1))
    vxc = 0.25 * (((o(Vx_o, IX, IY - 1, IZ) + o(Vx_o, IX + 1, IY - 1, IZ)) + o(Vx_o, IX, IY, IZ)) + o(Vx_o, IX + 1, IY, IZ))
    vyc = o(Vy_o, IX, IY, IZ)
    vzc = 0.25 * (((o(Vz_o, IX, IY - 1, IZ) + o(Vz_o, IX, IY - 1, IZ + 1)) + o(Vz_o, IX, IY, IZ)) + o(Vz_o, IX, IY, IZ + 1))
    bt("Vy", Vy_o, vxc, vyc, vzc, IX, IY, IZ)
    IX, IY, IZ = grid(range(1, nx + 1), range(1, ny + 1), range(2, nz + 1))
    vxc = 0.25 * (((o(Vx_o, IX, IY, IZ - 1) + o(Vx_o, IX + 1, IY, IZ - 1)) + o(Vx_o, IX, IY, IZ)) + o(Vx_o, IX + 1, IY, IZ))
    vyc = 0.25 * (((o(Vy_o, IX, IY, IZ - 1) + o(Vy_o, IX, IY + 1, IZ - 1)) + o(Vy_o, IX, IY, IZ)) + o(Vy_o, IX, IY + 1, IZ))
    vzc = o(Vz_o, IX, IY, IZ)
    if faithful:
        bt("Vy", Vy_o, vxc, vyc, vzc, IX, IY, IZ)
    else:
        bt("Vz", Vz_o, vxc, vyc, vzc, IX, IY, IZ)
    IX, IY, IZ = grid(range(1, nx + 1), range(1, ny + 1), range(1, nz + 1))
    vxc = 0.5 * (o(Vx_o, IX, IY, IZ) + o(Vx_o, IX + 1, IY, IZ))
    vyc = 0.5 * (o(Vy_o, IX, IY, IZ) + o(Vy_o, IX, IY + 1, IZ))
    vzc = 0.5 * (o(Vz_o, IX, IY, IZ) + o(Vz_o, IX, IY, IZ + 1))
    bt("C", C_o, vxc, vyc, vzc, IX, IY, IZ)
    return out
