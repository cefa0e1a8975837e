"""Reference of the Smagorinsky model (include/ns3d.h: ns3d_eddy_viscosity, ns3d_update_tau_var, ns3d_predict_var and the step under
ns3d_set_turbulence): the header's NumPy statements with every scalar cast to the arrays' dtype, the same statements on
running_error.Pair values for the FAST bound — with a square root for pairs, defined here —, and the whole step composed from
oracle/numpy_ref.py's functions with the predictor replaced.  Helper of tests/test_les_host.py and tests/test_gpu_les.py."""
import math

import numpy as np

import running_error as RE
from oracle import numpy_ref as NR

I = (slice(1, -1),) * 3


# ---- the square root ---------------------------------------------------------------------------------------------------------------
def sqrt(x):
    """np.sqrt for arrays (the correctly rounded square root of the element type); for a Pair the value √v and the bound: the input
    bound propagated through √ — the largest |√t − √v| over the enclosure t ∈ [v − e, v + e], which is √v − √(v − e) =
    e/(√v + √(v − e)) while v − e > 0 (√ is concave: the lower end moves further) and the width of the enclosure's image,
    √(v + e) − √max(v − e, 0), where it reaches zero — plus 2u·|result|: one unit roundoff for a correctly rounded root and one more
    for a hardware root that is off by an ulp.  An exact zero (v = 0, e = 0) has the root 0 and the bound 0."""
    if not isinstance(x, RE.Pair):
        return np.sqrt(x)
    with np.errstate(all="ignore"):
        v = np.sqrt(x.v)
        lo = x.v - x.e
        inside = lo > 0
        prop = np.where(inside, x.e / (v + np.sqrt(np.where(inside, lo, 1.0))), np.sqrt(x.v + x.e) - np.sqrt(np.maximum(lo, 0.0)))
        exact = (x.v == 0) & (x.e == 0)
        return x._out(v, np.where(exact, 0.0, prop + 2.0 * x.u * np.abs(v)))


# ---- ns3d_eddy_viscosity --------------------------------------------------------------------------------------------------------------
def gradient(Vx, Vy, Vz, h, dx, dy, dz):
    """ns3d_vortex's velocity gradient on the interior cells, line by line (tests/vortex_ref.py::_interior): the diagonal, then
    uy, uz, vx, vz, wx, wy.  Works on ndarrays (h, dx, dy, dz scalars of their dtype) and on Pairs alike."""
    u = h * (Vx[:-1] + Vx[1:])
    v = h * (Vy[:, :-1] + Vy[:, 1:])
    w = h * (Vz[:, :, :-1] + Vz[:, :, 1:])
    gxx = ((Vx[1:] - Vx[:-1]) / dx)[I]
    gyy = ((Vy[:, 1:] - Vy[:, :-1]) / dy)[I]
    gzz = ((Vz[:, :, 1:] - Vz[:, :, :-1]) / dz)[I]
    uy = h * ((u[1:-1, 2:, 1:-1] - u[1:-1, :-2, 1:-1]) / dy)
    uz = h * ((u[1:-1, 1:-1, 2:] - u[1:-1, 1:-1, :-2]) / dz)
    vx = h * ((v[2:, 1:-1, 1:-1] - v[:-2, 1:-1, 1:-1]) / dx)
    vz = h * ((v[1:-1, 1:-1, 2:] - v[1:-1, 1:-1, :-2]) / dz)
    wx = h * ((w[2:, 1:-1, 1:-1] - w[:-2, 1:-1, 1:-1]) / dx)
    wy = h * ((w[1:-1, 2:, 1:-1] - w[1:-1, :-2, 1:-1]) / dy)
    return gxx, gyy, gzz, uy, uz, vx, vz, wx, wy


def _interior_mu_e(Vx, Vy, Vz, h, two, muT, c, dx, dy, dz):
    gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = gradient(Vx, Vy, Vz, h, dx, dy, dz)
    a = uy + vx; b = uz + wx; cc = vz + wy
    s2 = (two * ((gxx * gxx + gyy * gyy) + gzz * gzz)) + ((a * a + b * b) + cc * cc)
    return muT + c * sqrt(s2), s2


def eddy_viscosity(Vx, Vy, Vz, mu, rho, length, dx, dy, dz, with_s2=False):
    """mu_e, a (nx,ny,nz) array of the fields' dtype: the statement on the interior cells, muT everywhere else"""
    T = Vx.dtype.type
    assert Vy.dtype == Vx.dtype and Vz.dtype == Vx.dtype
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    muT, c = T(mu), T(float(rho) * float(length) * float(length))
    with np.errstate(all="ignore"):
        val, s2 = _interior_mu_e(Vx, Vy, Vz, T(0.5), T(2), muT, c, T(dx), T(dy), T(dz))
    assert val.dtype == Vx.dtype
    out = np.full((nx, ny, nz), muT, dtype=Vx.dtype, order="F")
    out[I] = val
    return (out, s2) if with_s2 else out


def eddy_viscosity_pairs(Vx, Vy, Vz, mu, rho, length, dx, dy, dz):
    """the same statement on pairs: value in fp64, running-error bound in the fields' dtype; boundary cells: muT, bound 0"""
    dt = Vx.dtype
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    muT, c = RE.scalar(mu, dt), RE.scalar(float(rho) * float(length) * float(length), dt)
    val, _ = _interior_mu_e(RE.field(Vx), RE.field(Vy), RE.field(Vz), 0.5, 2.0, muT, c, RE.spacing(dx, dt), RE.spacing(dy, dt),
                            RE.spacing(dz, dt))
    full = RE.Pair(np.full((nx, ny, nz), float(muT.v), order="F"), None, RE.unit(dt))
    full[I] = val
    return full


# ---- ns3d_update_tau_var ---------------------------------------------------------------------------------------------------------------
def update_tau_var(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, m, dx, dy, dz, two=None, q=None):
    """numpy_ref.update_tau with 2·mu read per cell and the shear viscosities averaged over the four cells around the edge; on
    ndarrays (dx, dy, dz scalars of their dtype) and on Pairs (two = 2.0, q = 0.25) alike"""
    if two is None:
        T = m.dtype.type
        two, q = T(2), T(0.25)
    div = NR._divV(Vx, Vy, Vz, dx, dy, dz)
    txx[...] = (two * m) * ((Vx[1:, :, :] - Vx[:-1, :, :]) / dx - div / 3.0)
    tyy[...] = (two * m) * ((Vy[:, 1:, :] - Vy[:, :-1, :]) / dy - div / 3.0)
    tzz[...] = (two * m) * ((Vz[:, :, 1:] - Vz[:, :, :-1]) / dz - div / 3.0)
    nx, ny, nz = txx.shape
    d_yi_Vx = Vx[1:nx, 1:ny, 1:nz] - Vx[1:nx, 0:ny - 1, 1:nz]
    d_xi_Vy = Vy[1:nx, 1:ny, 1:nz] - Vy[0:nx - 1, 1:ny, 1:nz]
    d_zi_Vx = Vx[1:nx, 1:ny, 1:nz] - Vx[1:nx, 1:ny, 0:nz - 1]
    d_xi_Vz = Vz[1:nx, 1:ny, 1:nz] - Vz[0:nx - 1, 1:ny, 1:nz]
    d_zi_Vy = Vy[1:nx, 1:ny, 1:nz] - Vy[1:nx, 1:ny, 0:nz - 1]
    d_yi_Vz = Vz[1:nx, 1:ny, 1:nz] - Vz[1:nx, 0:ny - 1, 1:nz]
    mxy = q * ((m[0:nx - 1, 0:ny - 1, 1:nz] + m[1:nx, 0:ny - 1, 1:nz]) + (m[0:nx - 1, 1:ny, 1:nz] + m[1:nx, 1:ny, 1:nz]))
    mxz = q * ((m[0:nx - 1, 1:ny, 0:nz - 1] + m[1:nx, 1:ny, 0:nz - 1]) + (m[0:nx - 1, 1:ny, 1:nz] + m[1:nx, 1:ny, 1:nz]))
    myz = q * ((m[1:nx, 0:ny - 1, 0:nz - 1] + m[1:nx, 1:ny, 0:nz - 1]) + (m[1:nx, 0:ny - 1, 1:nz] + m[1:nx, 1:ny, 1:nz]))
    txy[...] = mxy * (d_yi_Vx / dy + d_xi_Vy / dx)
    txz[...] = mxz * (d_zi_Vx / dz + d_xi_Vz / dx)
    tyz[...] = myz * (d_zi_Vy / dz + d_yi_Vz / dy)


def _stress_arrays(Vx):
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    z = lambda *s: np.zeros(s, dtype=Vx.dtype, order="F")
    return [z(nx, ny, nz) for _ in range(3)] + [z(nx - 1, ny - 1, nz - 1) for _ in range(3)]


def tau_var(Vx, Vy, Vz, m, dx, dy, dz):
    """the six stress arrays of update_tau_var, freshly allocated, scalars cast to the fields' dtype"""
    T = Vx.dtype.type
    tau = _stress_arrays(Vx)
    with np.errstate(all="ignore"):
        update_tau_var(*tau, Vx, Vy, Vz, m, T(dx), T(dy), T(dz))
    return tau


# ---- ns3d_predict_var --------------------------------------------------------------------------------------------------------------------
def predict_var(Vx, Vy, Vz, m, rho, g, dt, dx, dy, dz):
    """(Vx, Vy, Vz) after {update_tau_var; numpy_ref.predict_V}: complete new arrays, the inputs untouched"""
    T = Vx.dtype.type
    tau = tau_var(Vx, Vy, Vz, m, dx, dy, dz)
    out = [a.copy(order="F") for a in (Vx, Vy, Vz)]
    with np.errstate(all="ignore"):
        NR.predict_V(*out, *tau, T(rho), T(g), T(dt), T(dx), T(dy), T(dz))
    return out


def predict_var_pairs(Vx, Vy, Vz, m, rho, g, dt, dx, dy, dz):
    """the same on pairs; m: the viscosity field as the kernel reads it (an array: exact input)"""
    dtp = Vx.dtype
    V = [RE.field(a) for a in (Vx, Vy, Vz)]
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    zp = lambda *s: RE.Pair(np.zeros(s, order="F"), None, RE.unit(dtp))
    tau = [zp(nx, ny, nz) for _ in range(3)] + [zp(nx - 1, ny - 1, nz - 1) for _ in range(3)]
    sp = [RE.spacing(d, dtp) for d in (dx, dy, dz)]
    update_tau_var(*tau, *V, RE.field(m), *sp, two=2.0, q=0.25)
    NR.predict_V(*V, *tau, RE.scalar(rho, dtp), RE.scalar(g, dtp), RE.scalar(dt, dtp), *sp)
    return V


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------
def owns(p, which):
    """multi.jl:164,179: whether this rank applies the inlet / outlet rule — the parameters' own flag (the reference compares a rounded
    coordinate with ±lx/2, and on some grids the outlet test is false on every rank), True where the parameters carry none"""
    try:
        return bool(getattr(p, "owns_" + which))
    except (AttributeError, KeyError):          # oracle/driver_ref.py's Obj raises KeyError
        return True


def pt_solve(f, p, niter, script):
    """multi.jl:458-471 / gpu.jl:126-137 with numpy_ref's functions; returns (iterations, [err …])"""
    errs, done = [], niter
    for itr in range(1, niter + 1):
        NR.update_dPrdtau(f["Pr"], f["dPrdtau"], f["divV"], p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz)
        NR.update_Pr(f["Pr"], f["dPrdtau"], p.dtau)
        if script == "multi":
            NR.set_bc_Pr_multi(f["Pr"], owns(p, "outlet"), 0.0)
        else:
            NR.set_bc_Pr_gpu(f["Pr"], p.dz, p.nz, p.g, p.rho)
        if itr % p.nchk == 0:
            Rp = np.zeros(f["dPrdtau"].shape, order="F")
            NR.compute_res(Rp, f["Pr"], f["divV"], p.rho, p.dt, p.dx, p.dy, p.dz)
            err = NR.max_abs(Rp) * (p.ly * p.ly) / p.psc
            errs.append(err)
            if err < p.eps or not math.isfinite(err):
                done = itr
                break
    return done, errs


def cylinder(f, p, script):
    if script == "multi":
        NR.set_cylinder(f["C"], f["Vx"], f["Vy"], f["Vz"], p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly,
                        p.lz, p.dx, p.dy, p.dz)
    else:
        NR.set_cylinder_local(f["C"], f["Vx"], f["Vy"], f["Vz"], p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)


def step(f, p, length, niter, script="multi", faithful=False, pressure="pt", work=np.float64):
    """One time step (multi.jl:449-477 on one rank / gpu.jl:121-142) in float64 on the dict f of the step's arrays (C, Pr, Vx, Vy, Vz,
    dPrdtau, divV, the *_o buffers; the six stress arrays if present), in place, with the predictor replaced: mu_e from
    eddy_viscosity, the stresses from update_tau_var, then numpy_ref's own functions for everything else, the reference's advection
    included.  p: the script's parameters (floats).  pressure="direct": oracle/direct_ref.py's solve in place of the PT loop, as the
    oracle drivers make it, its sums carried in `work` (np.longdouble measures the statement's own rounding level, as
    tests/test_gpu_direct.py does for the oracle drivers).  Returns (mu_e, iterations, errs)."""
    with np.errstate(all="ignore"):
        mu_e = eddy_viscosity(f["Vx"], f["Vy"], f["Vz"], p.mu, p.rho, length, p.dx, p.dy, p.dz)
        tau = tau_var(f["Vx"], f["Vy"], f["Vz"], mu_e, p.dx, p.dy, p.dz)
        for n, a in zip(("txx", "tyy", "tzz", "txy", "txz", "tyz"), tau):
            if n in f:
                f[n][...] = a
        NR.predict_V(f["Vx"], f["Vy"], f["Vz"], *tau, p.rho, p.g, p.dt, p.dx, p.dy, p.dz)
        cylinder(f, p, script)
        NR.update_divV(f["divV"], f["Vx"], f["Vy"], f["Vz"], p.dx, p.dy, p.dz)
        if pressure == "direct":
            from oracle.direct_ref import poisson_direct
            f["Pr"][...] = poisson_direct(f["divV"], p.rho, p.dt, p.dx, p.dy, p.dz, 0 if script == "multi" else 1, script == "multi" and owns(p, "outlet"), 0.0,
                                          p.g, work=work).astype(np.float64)
            f["dPrdtau"][...] = 0
            Rp = np.zeros(f["dPrdtau"].shape, order="F")
            NR.compute_res(Rp, f["Pr"], f["divV"], p.rho, p.dt, p.dx, p.dy, p.dz)
            done, errs = 0, [NR.max_abs(Rp) * (p.ly * p.ly) / p.psc]
        else:
            done, errs = pt_solve(f, p, niter, script)
        NR.correct_V(f["Vx"], f["Vy"], f["Vz"], f["Pr"], p.dt, p.rho, p.dx, p.dy, p.dz)
        cylinder(f, p, script)
        if script == "multi":
            NR.set_bc_Vel_multi(f["Vx"], f["Vy"], f["Vz"], owns(p, "inlet"), p.vin)
        else:
            NR.set_bc_Vel_gpu(f["Vx"], f["Vy"], f["Vz"])
        for n in ("Vx", "Vy", "Vz", "C"):
            f[n + "_o"][...] = f[n]
        NR.advect(f["Vx"], f["Vx_o"], f["Vy"], f["Vy_o"], f["Vz"], f["Vz_o"], f["C"], f["C_o"], p.dt, p.dx, p.dy, p.dz, faithful)
    return mu_e, done, errs


def smagorinsky_length(cs, dx, dy, dz):
    """ℓ = cs·Δ as the drivers form it"""
    return cs * (dx * dy * dz) ** (1.0 / 3.0)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def pure_shear(shape, gamma, dtype, spacings=(0.25, 0.5, 0.125)):
    """u = γ·y, v = w = 0 on a grid of `shape` cells: S_xy = γ/2, |S| = γ.  Returns (Vx, Vy, Vz, dx, dy, dz)."""
    nx, ny, nz = shape
    dx, dy, dz = spacings
    y = (np.arange(ny) + 0.5) * dy
    Vx = np.empty((nx + 1, ny, nz), dtype=dtype, order="F")
    Vx[:, :, :] = (gamma * y).astype(dtype)[None, :, None]
    return Vx, np.zeros((nx, ny + 1, nz), dtype=dtype, order="F"), np.zeros((nx, ny, nz + 1), dtype=dtype, order="F"), dx, dy, dz
