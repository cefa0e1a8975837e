"""Reference of ns3d_sgs_viscosity (include/ns3d.h): the header's three NumPy statements — Smagorinsky's |S|, the WALE operator of
Nicoud & Ducros and Vreman's — on les_ref.gradient with every scalar cast to the arrays' dtype, the same statements on
running_error.Pair values for the FAST bound (les_ref.sqrt's treatment of the root extended to the clamp and the guarded quotient),
and the whole step: les_ref.step with its first statement replaced.  Helper of tests/test_sgs_host.py and tests/test_gpu_sgs.py."""
import math

import numpy as np

import les_ref as LR
import running_error as RE
from oracle import numpy_ref as NR

I = LR.I
SMAGORINSKY, WALE, VREMAN = 0, 1, 2
NAMES = {SMAGORINSKY: "smagorinsky", WALE: "wale", VREMAN: "vreman"}
CS, CW, CV = 0.17, 0.5535, 0.07225           # the drivers' defaults: C_w² = 10.6·C_s², c_v = 2.5·C_s²


# ---- the two value-dependent statements, for arrays and for pairs ------------------------------------------------------------------
def clamp0(x):
    """(x < 0) ? 0 : x — a comparison, so a NaN stays a NaN.  For a Pair the value is clamped and the bound kept: t → max(t, 0)
    moves no two numbers apart, so |max(v,0) − max(exact,0)| ≤ |v − exact| whichever side of 0 either lies on."""
    if not isinstance(x, RE.Pair):
        return np.where(x < 0, x.dtype.type(0), x)
    return RE.Pair(np.where(x.v < 0, 0.0, x.v), x.e.copy(), x.u)


def guard(den, val):
    """(den == 0) ? 0 : val, with val already formed from den (a NaN den is not == 0: val's NaN stands).  For a Pair: where den is
    an exact zero (v = 0, e = 0) every conforming evaluation takes the first branch, so the result is 0 with the bound 0; where den's
    value is 0 but its bound is not, the evaluations may disagree about the branch and nothing is promised (the bound is ∞)."""
    if not isinstance(val, RE.Pair):
        return np.where(den == 0, val.dtype.type(0), val)
    zero = den.v == 0
    return RE.Pair(np.where(zero, 0.0, val.v), np.where(zero, np.where(den.e == 0, 0.0, np.inf), val.e), val.u)


# ---- the operators -------------------------------------------------------------------------------------------------------------------
def strain2(G, two):
    gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
    a = uy + vx; b = uz + wx; cc = vz + wy
    return (two * ((gxx * gxx + gyy * gyy) + gzz * gzz)) + ((a * a + b * b) + cc * cc)


def wale_parts(G, h, two, third):
    """(dd, ss) of the header's WALE statement"""
    gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
    q11 = (gxx * gxx + uy * vx) + uz * wx; q12 = (gxx * uy + uy * gyy) + uz * wy; q13 = (gxx * uz + uy * vz) + uz * gzz
    q21 = (vx * gxx + gyy * vx) + vz * wx; q22 = (vx * uy + gyy * gyy) + vz * wy; q23 = (vx * uz + gyy * vz) + vz * gzz
    q31 = (wx * gxx + wy * vx) + gzz * wx; q32 = (wx * uy + wy * gyy) + gzz * wy; q33 = (wx * uz + wy * vz) + gzz * gzz
    t = third * ((q11 + q22) + q33); d11 = q11 - t; d22 = q22 - t; d33 = q33 - t
    d12 = h * (q12 + q21); d13 = h * (q13 + q31); d23 = h * (q23 + q32)
    dd = ((d11 * d11 + d22 * d22) + d33 * d33) + two * ((d12 * d12 + d13 * d13) + d23 * d23)
    return dd, h * strain2(G, two)


def wale(G, h, two, third):
    dd, ss = wale_parts(G, h, two, third)
    num = dd * LR.sqrt(dd); den = (ss * ss) * LR.sqrt(ss) + dd * LR.sqrt(LR.sqrt(dd))
    return guard(den, num / den)


def vreman_parts(G):
    """(aa, B) of the header's Vreman statement"""
    gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
    b11 = (gxx * gxx + uy * uy) + uz * uz; b22 = (vx * vx + gyy * gyy) + vz * vz; b33 = (wx * wx + wy * wy) + gzz * gzz
    b12 = (gxx * vx + uy * gyy) + uz * vz; b13 = (gxx * wx + uy * wy) + uz * gzz; b23 = (vx * wx + gyy * wy) + vz * gzz
    aa = (b11 + b22) + b33
    B = ((b11 * b22 - b12 * b12) + (b11 * b33 - b13 * b13)) + (b22 * b33 - b23 * b23)
    return aa, B


def vreman(G, h=None, two=None, third=None):
    aa, B = vreman_parts(G)
    return guard(aa, LR.sqrt(clamp0(B) / aa))


def operator(op, G, h, two, third):
    if op == SMAGORINSKY:
        return LR.sqrt(strain2(G, two))
    return {WALE: wale, VREMAN: vreman}[op](G, h, two, third)


# ---- ns3d_sgs_viscosity --------------------------------------------------------------------------------------------------------------
def sgs_viscosity(op, Vx, Vy, Vz, mu, rho, length, dx, dy, dz, with_op=False):
    """mu_e, a (nx,ny,nz) array of the fields' dtype: muT + c*op on the interior cells, muT everywhere else"""
    T = Vx.dtype.type
    assert Vy.dtype == Vx.dtype and Vz.dtype == Vx.dtype and op in NAMES
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    muT, c = T(mu), T(float(rho) * float(length) * float(length))
    h, two, third = T(0.5), T(2), T(1.0 / 3.0)
    with np.errstate(all="ignore"):
        val = operator(op, LR.gradient(Vx, Vy, Vz, h, T(dx), T(dy), T(dz)), h, two, third)
        inner = muT + c * val
    assert val.dtype == Vx.dtype and inner.dtype == Vx.dtype
    out = np.full((nx, ny, nz), muT, dtype=Vx.dtype, order="F")
    out[I] = inner
    return (out, val) if with_op else out


def sgs_viscosity_pairs(op, Vx, Vy, Vz, mu, rho, length, dx, dy, dz):
    """the same statement on pairs: value in fp64, running-error bound in the fields' dtype; boundary cells: muT, bound 0.  `third`
    enters as the element type's (T)(1.0/3.0), an exact operand from there on, like every launcher-converted scalar."""
    dt = Vx.dtype
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    muT, c = RE.scalar(mu, dt), RE.scalar(float(rho) * float(length) * float(length), dt)
    G = LR.gradient(RE.field(Vx), RE.field(Vy), RE.field(Vz), 0.5, RE.spacing(dx, dt), RE.spacing(dy, dt), RE.spacing(dz, dt))
    with np.errstate(all="ignore"):
        val = muT + c * operator(op, G, 0.5, 2.0, RE.scalar(1.0 / 3.0, dt))
    # an unbounded operand times an exact one makes 0·∞ in the bookkeeping: nothing is promised there either
    val = RE.Pair(val.v, np.where(np.isnan(val.e), np.inf, val.e), val.u)
    full = RE.Pair(np.full((nx, ny, nz), float(muT.v), order="F"), None, RE.unit(dt))
    full[I] = val
    return full


def length_of(op, dx, dy, dz, coef=None):
    """ℓ as the drivers form it: cs·Δ, cw·Δ, √c·Δ with Δ = (dx·dy·dz)^(1/3)"""
    delta = (dx * dy * dz) ** (1.0 / 3.0)
    if op == VREMAN:
        return math.sqrt(CV if coef is None else coef) * delta
    return ((CS if op == SMAGORINSKY else CW) if coef is None else coef) * delta


# ---- the whole step ------------------------------------------------------------------------------------------------------------------
def step(op, f, p, length, niter, script="multi", faithful=False, pressure="pt", work=np.float64):
    """les_ref.step — one time step in float64 on the dict f, in place — with its FIRST statement, the viscosity field, replaced by
    sgs_viscosity(op, …); every later statement is les_ref.step's, line for line.  Returns (mu_e, iterations, errs)."""
    with np.errstate(all="ignore"):
        mu_e = sgs_viscosity(op, f["Vx"], f["Vy"], f["Vz"], p.mu, p.rho, length, p.dx, p.dy, p.dz)
        tau = LR.tau_var(f["Vx"], f["Vy"], f["Vz"], mu_e, p.dx, p.dy, p.dz)
        for n, a in zip(("txx", "tyy", "tzz", "txy", "txz", "tyz"), tau):
            if n in f:
                f[n][...] = a
        NR.predict_V(f["Vx"], f["Vy"], f["Vz"], *tau, p.rho, p.g, p.dt, p.dx, p.dy, p.dz)
        LR.cylinder(f, p, script)
        NR.update_divV(f["divV"], f["Vx"], f["Vy"], f["Vz"], p.dx, p.dy, p.dz)
        if pressure == "direct":
            from oracle.direct_ref import poisson_direct
            f["Pr"][...] = poisson_direct(f["divV"], p.rho, p.dt, p.dx, p.dy, p.dz, 0 if script == "multi" else 1,
                                          script == "multi" and LR.owns(p, "outlet"), 0.0, p.g, work=work).astype(np.float64)
            f["dPrdtau"][...] = 0
            Rp = np.zeros(f["dPrdtau"].shape, order="F")
            NR.compute_res(Rp, f["Pr"], f["divV"], p.rho, p.dt, p.dx, p.dy, p.dz)
            done, errs = 0, [NR.max_abs(Rp) * (p.ly * p.ly) / p.psc]
        else:
            done, errs = LR.pt_solve(f, p, niter, script)
        NR.correct_V(f["Vx"], f["Vy"], f["Vz"], f["Pr"], p.dt, p.rho, p.dx, p.dy, p.dz)
        LR.cylinder(f, p, script)
        if script == "multi":
            NR.set_bc_Vel_multi(f["Vx"], f["Vy"], f["Vz"], LR.owns(p, "inlet"), p.vin)
        else:
            NR.set_bc_Vel_gpu(f["Vx"], f["Vy"], f["Vz"])
        for n in ("Vx", "Vy", "Vz", "C"):
            f[n + "_o"][...] = f[n]
        NR.advect(f["Vx"], f["Vx_o"], f["Vy"], f["Vy_o"], f["Vz"], f["Vz_o"], f["C"], f["C_o"], p.dt, p.dx, p.dy, p.dz, faithful)
    return mu_e, done, errs


# ---- closed forms and planted values -------------------------------------------------------------------------------------------------
def rotation(shape, omega, dtype, spacings=(0.25, 0.5, 0.125)):
    """solid-body rotation about z: u = −ω·y, v = ω·x, w = 0 at the faces' own coordinates.  With ω = 11/8 and these power-of-two
    spacings every value and every difference is exact in float32, so the discrete gradient is uy = −ω, vx = ω, all else 0."""
    nx, ny, nz = shape
    dx, dy, dz = spacings
    x = (np.arange(nx) + 0.5) * dx
    y = (np.arange(ny) + 0.5) * dy
    Vx = np.empty((nx + 1, ny, nz), dtype=dtype, order="F")
    Vx[:, :, :] = (-omega * y).astype(dtype)[None, :, None]
    Vy = np.empty((nx, ny + 1, nz), dtype=dtype, order="F")
    Vy[:, :, :] = (omega * x).astype(dtype)[:, None, None]
    return Vx, Vy, np.zeros((nx, ny, nz + 1), dtype=dtype, order="F"), dx, dy, dz


def parallel_rows(shape, dtype, seed, spacings=(0.25, 0.5, 0.125)):
    """u = a·x + b·y + c·z, v = k·u, w = 0 with seeded coefficients: the first two rows of the gradient are parallel, β has rank one
    and Vreman's B is 0 in real arithmetic — its rounded value has either sign.  Returns (Vx, Vy, Vz, dx, dy, dz)."""
    nx, ny, nz = shape
    dx, dy, dz = spacings
    r = np.random.default_rng(seed)
    a, b, c, k = r.uniform(0.5, 2.0, 4)
    lin = lambda X, Y, Z: a * X + b * Y + c * Z
    xc, yc, zc = (np.arange(nx) + 0.5) * dx, (np.arange(ny) + 0.5) * dy, (np.arange(nz) + 0.5) * dz
    xf, yf = np.arange(nx + 1) * dx, np.arange(ny + 1) * dy
    Vx = np.asfortranarray(lin(*np.meshgrid(xf, yc, zc, indexing="ij")).astype(dtype))
    Vy = np.asfortranarray((k * lin(*np.meshgrid(xc, yf, zc, indexing="ij"))).astype(dtype))
    return Vx, Vy, np.zeros((nx, ny, nz + 1), dtype=dtype, order="F"), dx, dy, dz


def negative_B(shape, dtype, seeds=range(64)):
    """the first seeded parallel_rows field whose statement has B < 0 in some interior cell: (fields…, mask of those cells), or None"""
    T = np.dtype(dtype).type
    for seed in seeds:
        case = parallel_rows(shape, dtype, seed)
        Vx, Vy, Vz, dx, dy, dz = case
        with np.errstate(all="ignore"):
            _, B = vreman_parts(LR.gradient(Vx, Vy, Vz, T(0.5), T(dx), T(dy), T(dz)))
        if (B < 0).any():
            return case, B < 0
    return None
