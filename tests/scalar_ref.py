"""Reference of the active scalar (include/ns3d.h: ns3d_scalar_diffuse, ns3d_buoyancy, ns3d_scalar_step and the step under
ns3d_set_scalar): the header's NumPy statements with every scalar cast to the arrays' dtype, the same statements on
running_error.Pair values for the FAST bound, and the whole step composed from oracle/numpy_ref.py's functions with the scalar
statement inserted behind the predictor — the turbulent predictor, the MacCormack advection and the mask come from les_ref.py,
sgs_ref.py, advect_mc_ref.py and solid_ref.py.  Helper of tests/test_scalar_host.py and tests/test_gpu_scalar.py."""
import numpy as np

import les_ref as LR
import running_error as RE
import sgs_ref as SR
from oracle import numpy_ref as NR


# ---- ns3d_scalar_diffuse -----------------------------------------------------------------------------------------------------------
def _sl(axis, s):
    return tuple(s if a == axis else slice(None) for a in range(3))


def _pad0(F, axis):
    """one face of +0.0 at each end of `axis`"""
    if isinstance(F, RE.Pair):
        shape = list(F.shape); shape[axis] = 1
        z = np.zeros(shape)
        return RE.Pair(np.concatenate([z, F.v, z], axis=axis), np.concatenate([z, F.e, z], axis=axis), F.u)
    shape = list(F.shape); shape[axis] = 1
    z = np.zeros(shape, dtype=F.dtype)
    return np.concatenate([z, F, z], axis=axis)


def _div_flux(Kf, C, h, d, axis):
    lo, hi = _sl(axis, slice(None, -1)), _sl(axis, slice(1, None))
    F = (h * (Kf[lo] + Kf[hi])) * ((C[hi] - C[lo]) / d)
    P = _pad0(F, axis)
    return (P[hi] - P[lo]) / d


def _diffuse(C, Kf, h, dt, dx, dy, dz):
    Dx, Dy, Dz = _div_flux(Kf, C, h, dx, 0), _div_flux(Kf, C, h, dy, 1), _div_flux(Kf, C, h, dz, 2)
    return C + dt * ((Dx + Dy) + Dz)


def diffusivity(C, mu_e, kappa, sgs, mu):
    """K per cell, an array of C's dtype"""
    T = C.dtype.type
    if mu_e is None:
        return np.full(C.shape, T(kappa), dtype=C.dtype, order="F")
    assert mu_e.dtype == C.dtype and mu_e.shape == C.shape
    with np.errstate(all="ignore"):
        return np.asfortranarray(T(kappa) + T(sgs) * (mu_e - T(mu)))


def scalar_diffuse(C, mu_e, kappa, sgs, mu, dt, dx, dy, dz):
    """C_out: a new array of C's dtype, the input untouched"""
    T = C.dtype.type
    with np.errstate(all="ignore"):
        out = _diffuse(C, diffusivity(C, mu_e, kappa, sgs, mu), T(0.5), T(dt), T(dx), T(dy), T(dz))
    assert out.dtype == C.dtype
    return np.asfortranarray(out)


def scalar_diffuse_pairs(C, mu_e, kappa, sgs, mu, dt, dx, dy, dz):
    d = C.dtype
    if mu_e is None:
        Kf = RE.Pair(np.full(C.shape, float(d.type(kappa)), order="F"), None, RE.unit(d))
    else:
        Kf = RE.scalar(kappa, d) + RE.scalar(sgs, d) * (RE.field(mu_e) - RE.scalar(mu, d))
    return _diffuse(RE.field(C), Kf, 0.5, RE.scalar(dt, d), RE.spacing(dx, d), RE.spacing(dy, d), RE.spacing(dz, d))


# ---- ns3d_buoyancy -------------------------------------------------------------------------------------------------------------------
INN = (slice(1, -1), slice(1, -1), slice(1, -1))      # @inn(Vz) of the (nx,ny,nz+1) array: faces 1 … nz-1


def _lift(Vz, C, h, bg, c_ref, dt):
    Cin = C[1:-1, 1:-1, :]
    return Vz[INN] + dt * (bg * (h * (Cin[:, :, :-1] + Cin[:, :, 1:]) - c_ref))


def buoyancy(Vz, C, bg, c_ref, dt):
    """Vz after the call: a new array, the input untouched"""
    T = C.dtype.type
    out = Vz.copy(order="F")
    with np.errstate(all="ignore"):
        out[INN] = _lift(Vz, C, T(0.5), T(bg), T(c_ref), T(dt))
    return out


def buoyancy_pairs(Vz, C, bg, c_ref, dt):
    d = C.dtype
    out = RE.field(Vz)
    out[INN] = _lift(RE.field(Vz), RE.field(C), 0.5, RE.scalar(bg, d), RE.scalar(c_ref, d), RE.scalar(dt, d))
    return out


def scalar_step(Vz, C, mu_e, kappa, sgs, mu, bg, c_ref, dt, dx, dy, dz):
    """(C_out, Vz) of the fused call: the two statements, both on the input C"""
    return scalar_diffuse(C, mu_e, kappa, sgs, mu, dt, dx, dy, dz), (buoyancy(Vz, C, bg, c_ref, dt) if bg != 0.0 else Vz.copy(order="F"))


# ---- the whole step -----------------------------------------------------------------------------------------------------------------
def step(f, p, sca, niter, script="multi", faithful=False, pressure="pt", work=np.float64, op=None, length=0.0, maccormack=False,
         mask=None):
    """One time step in float64 on the dict f, in place — les_ref.step's sequence (numpy_ref's functions) with the scalar statement
    behind the predictor and before the first masking.  sca: dict(kappa, sct, bg, c_ref) or None (no statement).  op: None for the
    scalar μ (numpy_ref.update_tau), else sgs_ref's operator code with `length`.  maccormack: advect_mc_ref's advection in place of
    the reference's.  mask: solid_ref.set_solid with these four masks in place of the cylinder.  Returns (mu_e or None, iterations,
    errs)."""
    def body():
        if mask is not None:
            import solid_ref
            solid_ref.set_solid(f["C"], f["Vx"], f["Vy"], f["Vz"], mask)
        else:
            LR.cylinder(f, p, script)
    with np.errstate(all="ignore"):
        mu_e = None
        if op is None:
            tau = LR._stress_arrays(f["Vx"])
            NR.update_tau(*tau, f["Vx"], f["Vy"], f["Vz"], p.mu, p.dx, p.dy, p.dz)
        else:
            mu_e = SR.sgs_viscosity(op, f["Vx"], f["Vy"], f["Vz"], p.mu, p.rho, length, p.dx, p.dy, p.dz)
            tau = LR.tau_var(f["Vx"], f["Vy"], f["Vz"], mu_e, p.dx, p.dy, p.dz)
        for n, a in zip(("txx", "tyy", "tzz", "txy", "txz", "tyz"), tau):
            if n in f:
                f[n][...] = a
        NR.predict_V(f["Vx"], f["Vy"], f["Vz"], *tau, p.rho, p.g, p.dt, p.dx, p.dy, p.dz)
        if sca is not None:
            eddy = mu_e is not None and sca["sct"] > 0.0
            C_out, Vz = scalar_step(f["Vz"], f["C"], mu_e if eddy else None, sca["kappa"], 1.0 / (p.rho * sca["sct"]) if eddy else 0.0,
                                    p.mu, sca["bg"], sca["c_ref"], p.dt, p.dx, p.dy, p.dz)
            f["C"][...] = C_out
            f["Vz"][...] = Vz
        body()
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
        body()
        if script == "multi":
            NR.set_bc_Vel_multi(f["Vx"], f["Vy"], f["Vz"], LR.owns(p, "inlet"), p.vin)
        else:
            NR.set_bc_Vel_gpu(f["Vx"], f["Vy"], f["Vz"])
        if maccormack:
            import advect_mc_ref as MR
            new, _ = MR.advect_mc([f["Vx"], f["Vy"], f["Vz"], f["C"]], p.dt, p.dx, p.dy, p.dz)
            for n, a in zip(("Vx", "Vy", "Vz", "C"), new):
                f[n + "_o"][...] = f[n]
                f[n][...] = a
        else:
            for n in ("Vx", "Vy", "Vz", "C"):
                f[n + "_o"][...] = f[n]
            NR.advect(f["Vx"], f["Vx_o"], f["Vy"], f["Vy_o"], f["Vz"], f["Vz_o"], f["C"], f["C_o"], p.dt, p.dx, p.dy, p.dz, faithful)
    return mu_e, done, errs


# ---- closed forms and planted values ---------------------------------------------------------------------------------------------------
def eigenmode(n, modes, dtype=np.float64):
    """C = Π cos(π p (i+½)/n) over the three directions: an eigenvector of the zero-flux operator with a uniform K"""
    axes = [np.cos(np.pi * p * (np.arange(m) + 0.5) / m) for m, p in zip(n, modes)]
    return np.asfortranarray((axes[0][:, None, None] * axes[1][None, :, None] * axes[2][None, None, :]).astype(dtype))


def eigenfactor(n, modes, kappa, dt, dx, dy, dz):
    return 1.0 - 4.0 * dt * kappa * sum(np.sin(np.pi * p / (2 * m)) ** 2 / d ** 2 for m, p, d in zip(n, modes, (dx, dy, dz)))


def sum_inv_d2(dx, dy, dz):
    return 1.0 / dx ** 2 + 1.0 / dy ** 2 + 1.0 / dz ** 2


def stencil_hull(C):
    """(min, max) over each cell's 7-point stencil, neighbours outside the grid left out"""
    lo, hi = C.copy(), C.copy()
    for axis in range(3):
        a, b = _sl(axis, slice(None, -1)), _sl(axis, slice(1, None))
        lo[a] = np.minimum(lo[a], C[b]); lo[b] = np.minimum(lo[b], C[a])
        hi[a] = np.maximum(hi[a], C[b]); hi[b] = np.maximum(hi[b], C[a])
    return lo, hi


def block01(n, dtype):
    """0 everywhere, 1 in a box that touches neither boundary where the grid allows"""
    C = np.zeros(n, dtype=dtype, order="F")
    C[tuple(slice(max(1, m // 3), max(2, 2 * m // 3)) for m in n)] = 1
    return C
