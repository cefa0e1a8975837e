"""Host-side mirror of the reference's two drivers, running on libns3d.so (HIP, gfx950).

    run_navierstokes3D(; do_vis, do_save, do_print, nx, nt)  ↔ scripts/NavierStokes3D_multi_gpu.jl:287-536
    runme(; do_vis, do_save)                                  ↔ scripts/NavierStokes3D_gpu.jl:12-173

Same keyword names, same return contract (C_v,Pr_v,Vx_v,Vy_v,Vz_v: halo-stripped global host arrays on rank 0,
multi.jl:528-535).  Extra keyword-only options select the arithmetic mode, the fused PT path and the z-slab
process grid.  do_vis writes the reference's mid-plane heat maps as bare PNG files (vis.py: same names, slices and colour
limits; no axes — Plots.jl itself is out of scope).

The time loops below follow the reference line by line (cited); with `fused=True` the inner pseudo-transient
loop {update_dPrdτ!; update_Pr!; set_bc_Pr!}×n is replaced by ns3d_pt_solve / overlapped ns3d_pt_sweep calls
that produce the same iterates (the redundant halo updates multi.jl:460,462 are dropped).
What is not the reference's is marked: `monitor` (diagnostics=True: three positions inside the step) and `obs` (observers.py:
statistics, vortex, tracers, probes, isosurface — at the end of a step, at a frame, after the loop).
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import kernels as K
from . import lib as L
from .halo import ZSlabGrid
from .observers import Observers, check_options
from .slab import SlabPTSolver
from .params import gpu_params, multi_params
from .vis import save_frame_gpu, save_frame_multi


def _alloc(nx, ny, nz, dtype, device):
    """multi.jl:343-360 / gpu.jl:65-82"""
    z = lambda *s: K.zeros(s, dtype, device)
    f = SimpleNamespace()
    f.Pr = z(nx, ny, nz); f.dPrdtau = z(nx - 2, ny - 2, nz - 2)
    f.C = z(nx, ny, nz); f.C_o = z(nx, ny, nz)
    f.txx = z(nx, ny, nz); f.tyy = z(nx, ny, nz); f.tzz = z(nx, ny, nz)
    f.txy = z(nx - 1, ny - 1, nz - 1); f.txz = z(nx - 1, ny - 1, nz - 1); f.tyz = z(nx - 1, ny - 1, nz - 1)
    f.Vx = z(nx + 1, ny, nz); f.Vy = z(nx, ny + 1, nz); f.Vz = z(nx, ny, nz + 1)
    f.Vx_o = z(nx + 1, ny, nz); f.Vy_o = z(nx, ny + 1, nz); f.Vz_o = z(nx, ny, nz + 1)
    f.divV = z(nx, ny, nz); f.Rp = z(nx - 2, ny - 2, nz - 2)
    return f


def save_array(Aname, A):
    """save_array(Aname, A) (multi.jl:27-30): raw little-endian column-major dump to Aname.bin."""
    with open(Aname + ".bin", "wb") as fh:
        fh.write(np.asfortranarray(A).tobytes(order="F"))


def _gather_all(grid, fs):
    """multi.jl:399-403 / :528-532 for the local ranks' fields `fs` (halo cells stripped, :399)"""
    return tuple(grid.gather_fields([getattr(f, n) for f in fs]) for n in ("C", "Pr", "Vx", "Vy", "Vz"))


def _save_frame(grid, fields_v, iframe):
    """multi.jl:404-413 / :515-522 — rank 0 writes Float32 raw dumps of the gathered arrays."""
    if not grid.is_root():
        return
    os.makedirs("./out_save", exist_ok=True)
    for name, A in zip(("C", "Pr", "Vx", "Vy", "Vz"), fields_v):
        save_array("out_save/out_%s_v_%04d" % (name, iframe), A.astype(np.float32))


def _diag_step_record(full, mom_predict, mom_correct, p):
    """One entry of info.diag: the monitor's full set after the step's boundary rules, plus
    courant[q] = dt·max|V_q|/d_q — a bound on every |δ| backtrack! forms in that direction, which averages those very values
    (multi.jl:190-199) — and force[q] = ρ·dx·dy·dz/dt·(mom₁[q] + mom₂[q]): the momentum the two set_cylinder! calls of the step
    (:452, :473 / gpu.jl:123, :139) remove from the fluid, per unit time — the force the fluid exerts on the body (drag, lift,
    and z) as the masking method itself produces it (no surface integral)."""
    rec = SimpleNamespace(**vars(full))
    d3 = (p.dx, p.dy, p.dz)
    rec.courant = tuple(p.dt * full.vmax[q] / d3[q] for q in range(3))
    rec.mom_predict, rec.mom_correct = tuple(mom_predict), tuple(mom_correct)
    rec.force = tuple(p.rho * p.dx * p.dy * p.dz / p.dt * (mom_predict[q] + mom_correct[q]) for q in range(3))
    return rec


def _monitor(grid, ctxs, fs, cyls, p):
    """diagnostics=True: monitor(full) → the flow monitor's record of the GLOBAL arrays as they are at the call (ns3d_diagnostics on one
    rank, through the grid on an ns3d_mgpu); full=False: velocities only (the masked momentum).  `cyls`: set_cylinder!'s scalars per
    local rank."""
    dps = [K.diag_params(p.nx, p.ny, p.nz, p.dx, p.dy, p.dz, p.rho, cylinder=cyl) for cyl in cyls]   # seam flags: set by the grid
    col = lambda n: [getattr(f, n) for f in fs]

    def monitor(full):
        pr, cf = (col("Pr"), col("C")) if full else (None, None)
        if grid.mg is not None:
            return grid.diagnostics(col("Vx"), col("Vy"), col("Vz"), pr, cf, dps)[0]
        return K.diagnostics(fs[0].Vx, fs[0].Vy, fs[0].Vz, pr and pr[0], cf and cf[0], dps[0], ctx=ctxs[0])
    return monitor


def _step_params(script, p, niter, faithful, pressure):
    """lib.StepParams of ns3d_time_step on one rank.  script = lib.NS3D_BC_MULTI: p from multi_params, with the cylinder's global
    origin, the inlet and outlet flags and vin; lib.NS3D_BC_GPU: p from gpu_params, whose script has none of them."""
    multi = script == L.NS3D_BC_MULTI
    xco_g, yco_g, zco_g = (p.xco_g, p.yco_g, p.zco_g) if multi else (0.0, 0.0, 0.0)
    return L.StepParams(script=script, nx=p.nx, ny=p.ny, nz=p.nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp,
                        dx=p.dx, dy=p.dy, dz=p.dz, eps=p.eps, niter=niter, nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc,
                        a2=p.a2, b2=p.b2, ox=p.ox, oy=p.oy, sinb=p.sinb, cosb=p.cosb, xco_g=xco_g, yco_g=yco_g, zco_g=zco_g,
                        lx=p.lx, ly=p.ly, lz=p.lz, owns_inlet=int(multi and bool(p.owns_inlet)),
                        owns_outlet=int(multi and bool(p.owns_outlet)), vin=p.vin if multi else 0.0, faithful=int(bool(faithful)),
                        pressure=1 if pressure == "direct" else 0, write_stress=0)


def _print_step(it, errs, nchk, rec=None):
    """the reference's lines of a step (multi.jl:456,468 / gpu.jl:125,134), then the monitor's (diagnostics=True)"""
    print("#it = %d" % it)
    for q, e in enumerate(errs):
        print("  #iter = %d, err = %1.3e" % ((q + 1) * nchk, e))
    if rec is not None:
        print(_diag_line(rec))


def _check_wide_precondition(it, courant):
    """ns3d_advect_wide reproduces the one-rank step only while |δz| < 2 cells; courant[2] bounds |δz|.  Anything that is not
    below 2 — a NaN included — stops the run before it advects."""
    if not courant[2] < 2.0:
        raise L.Ns3dError("step %d: courant[2] = dt*max|Vz|/dz = %r is not below 2 — outside the precondition of "
                          "wide_advect_halo (ns3d_advect_wide is exact only while |δz| < 2 cells); reduce dt" % (it, courant[2]))


def _diag_line(rec):
    return ("  diag: courant = %.3f %.3f %.3f, max|divV| = %.3e, Pr in [%.3e, %.3e], ke = %.6e, force = %.4e %.4e %.4e%s"
            % (rec.courant + (rec.div_max, rec.pr_min, rec.pr_max, rec.ke) + rec.force + (", NON-FINITE" if rec.nonfinite else "",)))


def pt_loop_reference(ctxs, grid, fs, ps, niter, do_print=False):
    """The inner loop exactly as written in multi.jl:458-471 (including its redundant halo updates); `fs`, `ps`, `ctxs`
    hold one entry per local rank."""
    p = ps[0]
    errs, done = [], niter
    col = lambda n: [getattr(f, n) for f in fs]
    for it in range(1, niter + 1):
        for f, c in zip(fs, ctxs):
            K.update_dPrdtau(f.Pr, f.dPrdtau, f.divV, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, ctx=c)   # :459
        grid.update_halo(col("divV"))                                                                     # :460
        for f, c in zip(fs, ctxs):
            K.update_Pr(f.Pr, f.dPrdtau, p.dtau, ctx=c)                                                   # :461
        grid.update_halo(col("Pr"))                                                                       # :462
        for f, c, q in zip(fs, ctxs, ps):
            K.set_bc_Pr_multi(f.Pr, q.owns_outlet, 0.0, ctx=c)                                            # :463 → :176-181
        grid.update_halo(col("Pr"))                                                                       # :182
        if it % p.nchk == 0:                                                                              # :464
            loc = []
            for f, c in zip(fs, ctxs):
                K.compute_res(f.Rp, f.Pr, f.divV, p.rho, p.dt, p.dx, p.dy, p.dz, ctx=c)                   # :465
                loc.append(K.max_abs(f.Rp, ctx=c))
            err = grid.max_g(loc if len(loc) > 1 else loc[0]) * (p.ly * p.ly) / p.psc                      # :466
            errs.append(err)
            if grid.is_root() and do_print:
                print("  #iter = %d, err = %1.3e" % (it, err))                                            # :468
            if err < p.eps or not math.isfinite(err):                                                     # :469
                done = it
                break
    return done, errs


def pt_loop_fused_slab(ctx, grid, f, p, pt, niter, do_print=False, scratch=None):
    """Same iterates as pt_loop_reference on a z-slab rank: per iteration the two seam-adjacent interior planes
    are swept first, their exchange over xGMI is posted, and the interior sweep runs behind it."""
    nz = p.nz
    Pa = f.Pr
    Pb = scratch if scratch is not None else K.clone(f.Pr)
    if scratch is not None:
        K.copy(Pb, Pa, ctx=ctx)   # seeds faces/halo planes
    errs, done = [], niter
    for it in range(1, niter + 1):
        K.pt_sweep(Pa, Pb, f.dPrdtau, f.divV, pt, 1, 2, ctx=ctx)
        if nz - 2 > 1:
            K.pt_sweep(Pa, Pb, f.dPrdtau, f.divV, pt, nz - 2, nz - 1, ctx=ctx)
        work = grid.start_halo(Pb)
        if nz - 2 > 2:
            K.pt_sweep(Pa, Pb, f.dPrdtau, f.divV, pt, 2, nz - 2, ctx=ctx)
        grid.finish_halo(work)
        Pa, Pb = Pb, Pa
        if it % p.nchk == 0:
            err = grid.max_g(K.residual_max(Pa, f.divV, pt, ctx=ctx)) * (p.ly * p.ly) / p.psc
            errs.append(err)
            if grid.me == 0 and do_print:
                print("  #iter = %d, err = %1.3e" % (it, err))
            if err < p.eps or not math.isfinite(err):
                done = it
                break
    if Pa is not f.Pr:
        K.copy(f.Pr, Pa, ctx=ctx)
    return done, errs


def run_navierstokes3D(do_vis=False, do_save=False, do_print=False, nx=255, nt=10, *, mode="strict", fused=True,
                       temporal=True, dtype=torch.float64, faithful=True, grid=None, device=None, niter_cap=None,
                       return_info=False, shape=None, pressure="pt", wide_advect_halo=False, one_call=True, diagnostics=False,
                       statistics=None, stats_every=1, vortex=False, tracers=None, probes=None, isosurface=None, advection="reference",
                       obstacle=None, turbulence=None, scalar=None, motion=None):
    """run_navierstokes3D (multi.jl:287-536).  nx is the LOCAL streamwise size (ny = nz = ceil(0.6 nx) local).
    `grid` decides the decomposition: None = one rank; a halo.ZSlabGrid = this process is one z-slab rank of an
    initialised torch.distributed group; a mgpu.MgpuGrid = the C-ABI grid (this process drives every local rank of an
    ns3d_mgpu: all P of them in the one-process form, one under RCCL) — z-slabs, or any Cartesian topology with
    fused=False (ImplicitGlobalGrid's own default is MultiGpu.dims_create(P), e.g. (2,2,2) for 8 ranks).
    `shape` (dict: ny, nz, ly_lx, lz_lx) overrides the literals multi.jl:302-303,323-324 for grids the reference cannot
    produce without editing them (BASELINE configs[3]: 512×512×1024 global).
    pressure="direct" (OUTSIDE PARITY): the inner loop :458-471 is replaced by ns3d_poisson_direct, the exact
    solution of the discrete problem that loop stops short of by εit — on z-slab ranks of a MgpuGrid by
    ns3d_poisson_direct_slab, the solve of the global grid; info.iters is 0 per step and info.errs holds the (global) residual of
    the solution in the reference's own measure (:466).
    wide_advect_halo=True (OUTSIDE the reference's multi-rank semantics; z-slabs on the C-ABI grid): :475-477 run as
    ns3d_advect_wide — old fields with a two-plane z halo, C's halo updated too — so that the P-rank run reproduces the one-rank
    run of the same global grid bit for bit (the reference's backtrack! clamps to the local array).
    diagnostics=True: the flow monitor (ns3d_diagnostics, on the device) runs three times per step — before each of the two
    set_cylinder! calls :452 and :473 for the momentum they are about to remove, and after :474's halo update for the full set —
    and info.diag gets one record per step (_diag_step_record: the monitor's fields of the GLOBAL arrays, courant, force); with
    do_print the root prints one line per step after the reference's.  The step then runs call by call: `one_call` is not used.
    Fields, iteration counts and errs are those of the run without it, bit for bit.  With wide_advect_halo a step whose
    courant[2] is not below 2 raises Ns3dError instead of advecting outside ns3d_advect_wide's precondition (|δz| < 2 cells; on
    more than one rank only — on one rank wide_advect_halo has no effect and nothing is checked).
    One rank or the C-ABI grid (mgpu.MgpuGrid), any topology.
    statistics=s (default None: not one extra call): running statistics of the flow (ns3d_stats_accumulate, on the device, on every
    local rank's context) sampled with weight 1.0 at the end of the steps s, s+stats_every, … — after the step's last halo update
    :477, whichever way the step ran (`one_call` stays in use).  info.stats gets n, mean (U, V, W, P: cell-centred means) and rs
    (uu, vv, ww, uv, uw, vw: Reynolds stresses, pp: pressure variance) as halo-stripped global host arrays on the root, gathered
    like the fields.  Read-only: every other result keeps its bits.
    vortex=True (default False: not one extra call, file or attribute): the vorticity components and the Q-criterion (ns3d_vortex, on
    the device, on every local rank's context) of the final state, after the last step's halo update — and, with do_save / do_vis,
    of every frame's state.  info.vortex gets Wx, Wy, Wz, Q as halo-stripped global host arrays on the root, gathered like the
    fields; do_save adds out_Wx_v_%04d.bin, out_Wy_v_…, out_Wz_v_…, out_Q_v_… (Float32, same directory and counter), do_vis adds
    3D_NavierStokes_xy_Wz_%04d.png, …_xy_Q_…, …_xz_Wy_…, …_xz_Q_… (colour range: the data's own).  `one_call` stays in use;
    read-only: every other result keeps its bits.
    tracers=… (default None: not one extra call, file or attribute): Lagrangian tracer particles (tracers.Tracers,
    ns3d_tracers_advance on the device).  An (N,3) array gives physical start points (the box is [−lx/2, lx/2] × [−ly/2, ly/2] ×
    [−lz/2, lz/2]), an int N gives N points uniform in the box from a generator seeded with 0.  They are advanced once per time
    step, after advect! and :477's halo update, with the step's dt through the current Vx, Vy, Vz.  info.tracers gets x, y, z
    (physical), alive and steps; do_save adds out_tracers_%04d.bin per saved frame (Float32 (4,N): x, y, z, alive), do_vis
    3D_NavierStokes_tracers_%04d.png per drawn frame (an x-y scatter).
    probes=… (default None): an (M,3) array of physical points at which u, v, w, p are sampled at the end of every step (four
    ns3d_sample calls; the series stay on the device and are read back ONCE, after the last step): info.probes gets u, v, w, p
    of shape (nt, M), NaN for a point outside the box.
    Both are read-only with respect to the flow — every other result keeps its bits — and leave `one_call` in use.  As a number
    or an array they run on ONE RANK only: on more than one rank either keyword then raises Ns3dError, because a particle that
    crosses a seam has to migrate to the neighbouring rank.  For that, both keywords also take a READY OBJECT, used as it is:
    tracers.MgpuTracers / tracers.MgpuProbes built on this run's mgpu.MgpuGrid (one-process form; every local rank's fields are
    passed to them, particles migrate after each step, info.tracers is ordered by id and info.probes by point, so both compare
    with a one-rank run) — or a ready tracers.Tracers / tracers.Probes on one rank.
    isosurface=… (default None: not one extra call, file or attribute): a triangle surface of the final state, after the last
    step's halo update (ns3d_isosurface, on the device, on every local rank's context; isosurface.extract).  A float q means the
    Q-criterion at level q, uncoloured; a dict gives `field` (Q, Wx, Wy, Wz, Pr or C), `level` and optionally `color`, a field of
    the same set interpolated at the vertices.  info.isosurface gets an isosurface.Isosurface in physical coordinates (the cell
    grid's low corner is (−lx/2, −ly/2, −lz/2)).  Q, Wx, Wy, Wz are computed into scratch when `vortex` is off and extracted over
    the interior nodes 1 … n−2 of the global grid (their outermost cells are +0.0 by contract, not flow); Pr and C over the whole
    array.  The ranks of a decomposed grid extract the cubes they own — per decomposed direction the lower node runs from 1 (0 at
    a physical low end) up to and including n−2 — with origin = coords·(n−2), and the pieces are concatenated in rank order: one
    rank or a mgpu.MgpuGrid in the one-process form; in the one-process-per-GPU form the keyword raises Ns3dError (a
    variable-length gather across processes is not provided).  A rank reads its arrays as the step leaves them, halo cells
    included: :477 does not update C's halo, so next to a seam a surface of C, or coloured by it, is that of the rank's own copy.
    do_save adds out_iso_%04d.ply per saved frame (same directory
    and counter as the .bin files).  `one_call` stays in use; read-only: every other result keeps its bits.
    advection="maccormack" (default "reference": not one extra call; OUTSIDE the reference): :475-476 run as the limited MacCormack
    scheme (ns3d_advect_mc: second order where the reference's backtrack! is first order; include/ns3d.h has the definition) — with
    `one_call` inside ns3d_time_step (Context.set_advection), otherwise as one advect_mc call per step; the same bits either way.  It
    advects Vz, so it needs faithful=False, and it runs on one rank: anything else raises Ns3dError before the first step.  Every
    observer keyword keeps working.
    obstacle=… (default None: the reference's cylinder, not one extra call; OUTSIDE the reference): the body the flow goes around, in
    place of every set_cylinder! call (:372, :452, :473) — an (n,3,3) array, a closed triangle surface in the index space of the cell
    grid (solid.box_mesh, solid.from_isosurface, solid.load_ply with solid.to_index), voxelized once on the device (ns3d_voxelize),
    or a ready uint8 mask of (nx+1)(ny+1)(nz+1) bytes (solid.voxelize, solid.mask_of_cylinder).  With `one_call` the step masks
    inside ns3d_time_step (Context.set_obstacle), otherwise with one set_solid call where set_cylinder stands; the same bits either
    way.  With diagnostics=True, force comes from ns3d_solid_momentum taken before each of the step's two maskings.  One rank:
    anything else raises Ns3dError before the first step.
    turbulence=… (default None: not one extra call; OUTSIDE the reference): the subgrid-scale model of the predictor :449-451 —
    "smagorinsky", or dict(model="smagorinsky", cs=0.17).  Each step forms the effective viscosity μ_e = μ + ρ·ℓ²·|S| with
    ℓ = cs·(dx·dy·dz)^(1/3) (ns3d_eddy_viscosity, into an array this driver allocates) and predicts under it (ns3d_predict_var; the
    stress arrays of the last step come from ns3d_update_tau_var) — with `one_call` inside ns3d_time_step (Context.set_turbulence),
    otherwise as these calls; the same bits either way.  "wale" / dict(model="wale", cw=0.5535) and "vreman" /
    dict(model="vreman", c=0.07225) replace |S| by the operator of Nicoud & Ducros or of Vreman (ns3d_sgs_viscosity in place of
    ns3d_eddy_viscosity; ℓ = cw·Δ, √c·Δ): both vanish in pure shear, where |S| is largest; the defaults are the published equivalents
    of cs = 0.17.  info.turbulence gets model, length and mu_e, the field of the last step, as a host array.  With diagnostics=True
    every record gains mu_e_max, and a step whose dt·mu_e_max/ρ·(1/dx² + 1/dy² + 1/dz²) exceeds 1/2 — the explicit diffusion limit —
    raises Ns3dError.  One rank: anything else raises Ns3dError before anything is allocated.
    scalar=… (default None: C is the reference's passive dye, not one extra call; OUTSIDE the reference): dict(kappa=…, sct=0.7,
    beta_g=0.0, c_ref=0.0) makes C an active, diffusing scalar.  Behind the predictor :449-451 and before the first set_cylinder!
    :452 each step takes one explicit step of ∂C/∂t = ∇·(K ∇C), K = kappa (+ (μ_e − μ)/(ρ·sct) under a `turbulence` model with
    sct > 0), with zero flux through the domain faces, and adds dt·beta_g·(C − c_ref) to the predicted Vz (ns3d_scalar_step, both
    in one pass) — with `one_call` inside ns3d_time_step (Context.set_scalar), otherwise as this call; the same bits either way.
    The body's C = 1 is re-imposed by the masking that follows: a Dirichlet wall.  info.scalar gets kappa, sct, bg and c_ref.  A
    run whose dt·kappa·(1/dx² + 1/dy² + 1/dz²) exceeds 1/2 is refused; with diagnostics=True and a model, so is a step whose
    dt·(kappa + (mu_e_max − μ)/(ρ·sct))·(1/dx² + 1/dy² + 1/dz²) does.  One rank: anything else raises Ns3dError before anything is
    allocated.
    motion=… (default None: the body stands still, not one extra call; OUTSIDE the reference): the rigid motion of the body —
    dict(velocity=(0,0,0), omega=(0,0,0), centre=…) for a steady one (solid.rigid_motion: physical velocity and angular velocity,
    the centre of rotation at t = 0 in index space), or any callable pose(t) → (R, shift, U, omega, centre) of that shape.  The pose
    is evaluated at t = s·dt for the steps s = 1, 2, … (and at t = 0 for :372), and every masking stores the body's own velocity
    U + omega × r where it stored zero (ns3d_set_solid_moving) — with `one_call` inside ns3d_time_step (Context.set_obstacle_motion,
    set per step), otherwise as that call at the same two places; the same bits either way.  With `obstacle` given as triangles the
    original mesh stays on the device and, whenever the pose differs from the previous step's, the mask is rebuilt into the SAME
    buffer (ns3d_mesh_transform of the original mesh, ns3d_voxelize).  With `obstacle` None (the cylinder, through
    solid.mask_of_cylinder) or a uint8 mask, the mask is fixed and only the velocity is imposed — a body of revolution spinning about
    its axis — and a pose with a non-zero shift raises.  With diagnostics=True the two removed-momentum terms of force come from
    ns3d_solid_momentum_moving.  info.motion gets one dict per step: t, R, shift, U, omega, centre, rebuilt.  One rank: anything
    else, an unknown key or a number that is not finite raises Ns3dError before anything is allocated."""
    _check_advection(advection)
    _check_turbulence(turbulence)
    _check_scalar(scalar)
    _check_motion(motion)
    if pressure not in ("pt", "direct"):
        raise L.Ns3dError("pressure = %r (\"pt\" | \"direct\")" % (pressure,))
    if device is None:
        device = torch.cuda.current_device()
    shape = dict(shape or {})
    if grid is None:
        p0 = multi_params(nx, **shape)
        grid = ZSlabGrid(p0.nx, p0.ny, p0.nz)                                                  # :325
    watch = dict(statistics=statistics, stats_every=stats_every, vortex=vortex, tracers=tracers, probes=probes, isosurface=isosurface)
    check_options(grid, **watch)
    P, dims, mg, root = grid.P, tuple(grid.dims), grid.mg, grid.is_root()
    maccormack = _check_advection(advection, faithful, P)
    les = _check_turbulence(turbulence, P)
    sca = _check_scalar(scalar, P, multi_params(nx, dims=dims, coords=grid.local_coords[0], **shape))
    _check_motion(motion, P)
    # the contexts of the ns3d_mgpu's ranks (their devices), or this rank's own
    ctxs = list(grid.contexts) if grid.contexts is not None else [K.Context(device, mode, async_=True)]
    ps = [multi_params(nx, dims=dims, coords=c3, **shape) for c3 in grid.local_coords]
    p = ps[0]
    if fused and (dims[0] > 1 or dims[1] > 1) and mg is None:
        raise L.Ns3dError("a topology decomposed in x or y (dims = %r) needs the C-ABI grid (mgpu.MgpuGrid) or fused=False" % (dims,))
    # multi.jl:179 `xve_g == lx/2`: the outlet rule as the ranks on the last x coordinate evaluate it (the library applies it
    # on those ranks only; every z-slab rank is one of them)
    outlet_rule = multi_params(nx, dims=dims, coords=(dims[0] - 1, 0, 0), **shape).owns_outlet
    nx, ny, nz = p.nx, p.ny, p.nz
    niter = p.niter if niter_cap is None else min(p.niter, niter_cap)
    fs = [_alloc(nx, ny, nz, dtype, torch.device("cuda", c.device)) for c in ctxs]             # :343-360
    col = lambda n: [getattr(f, n) for f in fs]
    # initialization :369-373
    for f, q in zip(fs, ps):
        me = q.coords[2]
        f.Vy[0, :, :] = q.vin                                                                 # :369 (sic)
        # :370 Pr = -(z_g-dz/2)*ρ*g (+0+0): identically 0 because g = 1/Fr² = 0 (:316); evaluated for fidelity
        zg = np.array([(me * (nz - 2) + iz) * q.dz for iz in range(nz)])
        f.Pr[:, :, :] = torch.from_numpy(-(zg - q.dz / 2) * q.rho * q.g + 0.0).to(f.Pr.device, dtype)[None, None, :]
    if any(c._pinned for c in ctxs):                       # ranks on streams of their own: the torch writes above come first
        torch.cuda.synchronize()
    grid.update_halo(col("Pr"))                                                               # :371
    cyls = [(q.a2, q.b2, q.ox, q.oy, q.sinb, q.cosb, q.xco_g, q.yco_g, q.zco_g, q.lx, q.ly, q.lz, q.dx, q.dy, q.dz)
            for q in ps]
    solid, mesh = _obstacle_mask(obstacle, P, ctxs[0], (nx, ny, nz))
    mov = None
    if motion is not None:
        mov = _motion_start(motion, mesh, solid, ctxs[0], p, cyls[0], dtype, nt)
        solid = mov.mask
        _motion_pose(mov, 0, record=False)
    body = _body(solid, mov)
    for f, c, cyl in zip(fs, ctxs, cyls):
        body(f, cyl, c)                                                                       # :372
    grid.update_halo(col("C"), col("Vx"), col("Vy"), col("Vz"))                               # :373
    sync = lambda: [c.sync() for c in ctxs]
    iframe = 0
    nz_g_all = dims[2] * (nz - 2) + 2
    ny_g_all = dims[1] * (ny - 2) + 2
    obs = Observers(grid, ctxs, p, nt, dtype, gathered=True, **watch)

    def frame(save, vis):                           # :399-443 before the loop, :479-525 in it (one frame counter)
        nonlocal iframe
        if not (save or vis):
            return
        sync()
        gathered = _gather_all(grid, fs)                                                      # :399-403
        if save:                                                                              # :404-413 / :515-522
            _save_frame(grid, gathered, iframe)
        if vis and root:                                                                      # :416-443 / :486-513
            save_frame_multi(gathered, ny_g_all, nz_g_all, iframe)
        obs.frame(fs, iframe if save else None, iframe if vis else None)
        iframe += 1

    frame(do_save, do_vis)
    pts = [K.pt_params(f.Pr, q.rho, q.dt, q.dtau, q.damp, q.dx, q.dy, q.dz, L.NS3D_BC_MULTI, q.owns_outlet, 0.0, q.g,
                       q.coords[2] > 0, q.coords[2] < dims[2] - 1) for f, q in zip(fs, ps)]
    pt_all = K.pt_params(fs[0].Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI, outlet_rule, 0.0, p.g,
                         False, False)      # ns3d_pt_solve_slab: one set for every local rank, halo flags set inside
    if not temporal:
        for c in ctxs:
            c.set_pt2_variant(-1)
    if mg is not None:
        mg.set_temporal(4 if (temporal and nz >= 4) else 1)
    slab = None
    if fused and P > 1 and mg is None and temporal and nz >= 4:
        slab = SlabPTSolver(ctxs[0], grid, fs[0].Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI,
                            p.owns_outlet, 0.0, p.g)
    scratch = K.clone(fs[0].Pr) if (fused and P > 1 and mg is None and slab is None) else None
    info = SimpleNamespace(iters=[], errs=[], params=p)
    monitor = None
    if diagnostics:
        if P > 1 and mg is None:
            raise L.Ns3dError("diagnostics on %d ranks needs the C-ABI grid (mgpu.MgpuGrid)" % P)
        info.diag = []
        monitor = _monitor(grid, ctxs, fs, cyls if solid is None else [None], p)
    removed = _removed(monitor, solid, fs, ctxs, mov)
    obs.start()
    nsave = nvis = 10                                                                         # :330,332
    # :450's halo update of the normal stresses may only go with the stress arrays where the interior planes two ranks both compute
    # are identical.  backtrack! clamps to the LOCAL array and rounds iz − δ rank by rank, so with the fixed third branch
    # (faithful=False: Vz IS advected) on several ranks and without the wide halo the two copies of a seam's Vz plane can differ —
    # and the reference sequence would ship one rank's τzz to the other.  That combination keeps :449-451 literal.
    fuse_predictor = fused and (P == 1 or faithful or wide_advect_halo)
    # one rank, fused: the whole step :449-477 is ONE library call (ns3d_time_step: the same entry points, enqueued from C) — a step
    # of the 255×153×153 case with the direct pressure solve is otherwise mostly this loop's ≈40 calls
    step_params = None
    if fused and one_call and P == 1 and mg is None and not diagnostics:
        step_params = _step_params(L.NS3D_BC_MULTI, p, niter, faithful, pressure)
    if solid is not None and step_params is not None:
        ctxs[0].set_obstacle(solid)                             # ns3d_time_step masks with it; back to the cylinder after the loop
    if les is not None:
        _les_start(les, p, fs[0], ctxs[0], step_params is not None)     # ns3d_time_step predicts under it; cleared after the loop
    if sca is not None and step_params is not None:
        ctxs[0].set_scalar(sca.kappa, sca.sct, sca.bg, sca.c_ref)       # ns3d_time_step diffuses and lifts with it; cleared after the loop
    hats = None
    if maccormack and step_params is not None:
        ctxs[0].set_advection("maccormack")                     # ns3d_time_step advects with it; back to the default after the loop
    elif maccormack:
        hats = _alloc_hats(fs[0], ctxs[0])
    for it in range(1, nt + 1):                                                               # :446
        if mov is not None:
            _motion_pose(mov, it, step_params is not None)
        if step_params is not None:                             # :449-477 (ns3d_time_step swaps the names in fs[0] like the swaps below)
            step_params.write_stress = 1 if it == nt else 0     # the stress arrays as the reference leaves them after its last step
            done, errs = K.time_step(fs[0], step_params, ctx=ctxs[0])
        else:
            if les is not None:     # :449-451 under the Smagorinsky viscosity (one rank)
                mu_e_max = _les_predict(fs[0], p, ctxs[0], les, fused, it == nt, monitor is not None, it)
            elif fuse_predictor:
                # :449-451 in one pass (ns3d_predict_fused): the stresses evaluated on the fly, the predicted fields written into the
                # *_o buffers (free until :475), the names swapped.  :450's halo update of τxx, τyy, τzz moves values every rank has
                # already computed itself — the velocities it computes them from are consistent across ranks after :477 / :373 —
                # and is dropped with the arrays (the multi-rank driver tests compare with the oracle, which performs it)
                if it == nt:        # the stress arrays as the reference leaves them after its last step: same final state
                    for f, c in zip(fs, ctxs):
                        K.update_tau(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, p.mu, p.dx, p.dy, p.dz, ctx=c)
                    grid.update_halo(col("txx"), col("tyy"), col("tzz"))
                for f, c in zip(fs, ctxs):
                    _predict_swap(f, p, c)
            else:
                for f, c in zip(fs, ctxs):
                    K.update_tau(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, p.mu, p.dx, p.dy, p.dz, ctx=c)  # :449
                grid.update_halo(col("txx"), col("tyy"), col("tzz"))                          # :450
                for f, c in zip(fs, ctxs):
                    K.predict_V(f.Vx, f.Vy, f.Vz, f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, p.rho, p.g, p.dt, p.dx, p.dy, p.dz,
                                ctx=c)                                                        # :451
            if sca is not None:     # the active scalar (one rank): where ns3d_time_step issues it under the knob
                _scalar_step(fs[0], p, ctxs[0], sca, les, mu_e_max if les is not None else None, it)
            if monitor:
                mom_predict = removed()
            for f, c, cyl in zip(fs, ctxs, cyls):
                body(f, cyl, c)                                                               # :452
            grid.update_halo(col("C"), col("Vx"), col("Vy"), col("Vz"))                       # :453
            for f, c in zip(fs, ctxs):
                K.update_divV(f.divV, f.Vx, f.Vy, f.Vz, p.dx, p.dy, p.dz, ctx=c)              # :454
            grid.update_halo(col("divV"))                                                     # :455
            if pressure == "direct" and P > 1:                                                # (:456, :468 print after the step)
                if mg is None or not (dims[0] == 1 and dims[1] == 1):
                    raise L.Ns3dError("pressure=\"direct\" on %d ranks needs z-slab ranks on the C-ABI grid (mgpu.MgpuGrid); this grid "
                                      "is %s with dims = %r" % (P, type(grid).__name__, dims))
                mg.poisson_direct(col("Pr"), col("dPrdtau"), col("divV"), pt_all)      # ns3d_poisson_direct_slab
                loc = [K.residual_max(f.Pr, f.divV, q, ctx=c) for f, q, c in zip(fs, pts, ctxs)]
                done, errs = 0, [grid.max_g(loc if len(loc) > 1 else loc[0]) * (p.ly * p.ly) / p.psc]
            elif pressure == "direct":
                K.poisson_direct(fs[0].Pr, fs[0].dPrdtau, fs[0].divV, pts[0], ctx=ctxs[0])
                done, errs = 0, [K.residual_max(fs[0].Pr, fs[0].divV, pts[0], ctx=ctxs[0]) * (p.ly * p.ly) / p.psc]
            elif not fused:                                                                   # :458-471
                done, errs = pt_loop_reference(ctxs, grid, fs, ps, niter)
            elif P == 1:
                done, errs = K.pt_solve(fs[0].Pr, fs[0].dPrdtau, fs[0].divV, pts[0], p.eps, niter, p.nchk, p.ly * p.ly, p.psc,
                                        ctx=ctxs[0])
            elif mg is not None:                                    # the whole loop inside libns3d (ns3d_pt_solve_slab)
                done, errs = mg.pt_solve_slab(col("Pr"), col("dPrdtau"), col("divV"), pt_all, p.eps, niter, p.nchk,
                                              p.ly * p.ly, p.psc)
            elif slab is not None:                                  # z-slab rank over torch.distributed, deep ghosts
                slab.load(fs[0].Pr, fs[0].dPrdtau, fs[0].divV)
                done, errs = slab.solve(p.eps, niter, p.nchk, p.ly * p.ly, p.psc)
                slab.store(fs[0].Pr, fs[0].dPrdtau)
            else:
                done, errs = pt_loop_fused_slab(ctxs[0], grid, fs[0], p, pts[0], niter, scratch=scratch)
            for f, c in zip(fs, ctxs):
                K.correct_V(f.Vx, f.Vy, f.Vz, f.Pr, p.dt, p.rho, p.dx, p.dy, p.dz, ctx=c)     # :472
            if monitor:
                mom_correct = removed()
            for f, c, cyl, q in zip(fs, ctxs, cyls, ps):
                body(f, cyl, c)                                                               # :473
                K.set_bc_Vel_multi(f.Vx, f.Vy, f.Vz, q.owns_inlet, p.vin, ctx=c)              # :474 → :157-166
            grid.update_halo(col("Vx"), col("Vy"), col("Vz"))                                 # :167
            if monitor:
                info.diag.append(_diag_step_record(monitor(True), mom_predict, mom_correct, p))
                if les is not None:
                    info.diag[-1].mu_e_max = mu_e_max
                if wide_advect_halo and P > 1:
                    _check_wide_precondition(it, info.diag[-1].courant)
            if wide_advect_halo and P > 1:                                                    # :475-477, decomposition-independent
                if mg is None or not (dims[0] == 1 and dims[1] == 1):
                    raise L.Ns3dError("wide_advect_halo needs z-slab ranks on the C-ABI grid (mgpu.MgpuGrid)")
                mg.advect_wide(col("Vx"), col("Vx_o"), col("Vy"), col("Vy_o"), col("Vz"), col("Vz_o"), col("C"), col("C_o"),
                               p.dt, p.dx, p.dy, p.dz, faithful)
            for f, c in zip(fs, ctxs):
                if wide_advect_halo and P > 1:
                    break
                if maccormack:  # :475-476 as the limited MacCormack scheme (one rank): stage 1 into the hat buffers, stage 2, the roles swap
                    _advect_mc_swap(f, hats, p, c)
                    continue
                if fused:       # :475-476 in one pass (ns3d_copy_advect): complete new fields into the *_o buffers, then the roles swap
                    _copy_advect_swap(f, p, faithful, c)
                    continue
                K.copy(f.Vx_o, f.Vx, ctx=c); K.copy(f.Vy_o, f.Vy, ctx=c)                      # :475
                K.copy(f.Vz_o, f.Vz, ctx=c); K.copy(f.C_o, f.C, ctx=c)
                K.advect(f.Vx, f.Vx_o, f.Vy, f.Vy_o, f.Vz, f.Vz_o, f.C, f.C_o, p.dt, p.dx, p.dy, p.dz, faithful, ctx=c)  # :476
            if not (wide_advect_halo and P > 1):
                grid.update_halo(col("Vx"), col("Vy"), col("Vz"))                             # :477 (not C)
        info.iters.append(done); info.errs.append(errs)
        if root and do_print:                                                                 # :456, :468
            _print_step(it, errs if fused or pressure != "direct" else [], p.nchk, info.diag[-1] if monitor else None)
        obs.end_step(it, fs)
        frame(do_save and it % nsave == 0, do_vis and it % nvis == 0)
    if maccormack and step_params is not None:
        ctxs[0].set_advection("reference")
    if mov is not None and step_params is not None:
        ctxs[0].set_obstacle_motion(None)
    if solid is not None and step_params is not None:
        ctxs[0].set_obstacle(None)
    if les is not None:
        ctxs[0].set_turbulence(None)
    if sca is not None and step_params is not None:
        ctxs[0].set_scalar(None)
    if fused and faithful and nt > 0 and not (wide_advect_halo and P > 1):
        for f, c in zip(fs, ctxs):
            K.copy(f.Vz_o, f.Vz, ctx=c)     # the one copy of :475 the swaps skipped (Vz is never advected): same final state
    sync()
    out = _gather_all(grid, fs)                                                               # :528-532
    obs.finish(info, fs)
    if les is not None:
        info.turbulence = dict(model=les.model, length=les.length, mu_e=K.to_numpy(les.mu_e))
    if sca is not None:
        info.scalar = dict(kappa=sca.kappa, sct=sca.sct, bg=sca.bg, c_ref=sca.c_ref)
    if mov is not None:
        info.motion = mov.log
    info.fields = fs[0]
    info.local_fields = fs
    info.ctx = ctxs[0]
    return out + ((info,) if return_info else ())                                             # :535


def _predict_swap(f, p, ctx):
    """{update_τ!; predict_V!} (multi.jl:449,451 / gpu.jl:121-122) without the stress arrays: ns3d_predict_fused reads Vx, Vy, Vz
    and writes the complete predicted fields into the *_o buffers — idle between advect! and the next old-field copies — then
    the names swap."""
    K.predict_fused(f.Vx_o, f.Vy_o, f.Vz_o, f.Vx, f.Vy, f.Vz, p.mu, p.rho, p.g, p.dt, p.dx, p.dy, p.dz, ctx=ctx)
    f.Vx, f.Vx_o = f.Vx_o, f.Vx
    f.Vy, f.Vy_o = f.Vy_o, f.Vy
    f.Vz, f.Vz_o = f.Vz_o, f.Vz


def _copy_advect_swap(f, p, faithful, ctx):
    """{Vx_o,Vy_o,Vz_o,C_o .= Vx,Vy,Vz,C; advect!} (multi.jl:475-476 / gpu.jl:141-142) without the four copies:
    ns3d_copy_advect reads the current fields and writes COMPLETE new ones into the *_o buffers, then the names swap — X is
    the advected field and X_o the previous one, exactly what the copies leave behind.  Vz is never advected in faithful
    mode (App. B1): it stays where it is, and Vz_o is brought up to date once at the end of the run."""
    K.copy_advect(f.Vx_o, f.Vx, f.Vy_o, f.Vy, f.Vz if faithful else f.Vz_o, f.Vz, f.C_o, f.C, p.dt, p.dx, p.dy, p.dz, faithful,
                  ctx=ctx)
    f.Vx, f.Vx_o = f.Vx_o, f.Vx
    f.Vy, f.Vy_o = f.Vy_o, f.Vy
    f.C, f.C_o = f.C_o, f.C
    if not faithful:
        f.Vz, f.Vz_o = f.Vz_o, f.Vz


def _obstacle_mask(obstacle, P, ctx, n):
    """the `obstacle` keyword of both drivers → (mask, tri): mask None (the cylinder) or the uint8 device mask of the cell grid n;
    tri the (n,3,3) host array the mask was voxelized from, None for a ready mask; raises before anything is advanced"""
    if obstacle is None:
        return None, None
    if P != 1:
        raise L.Ns3dError("obstacle= runs on one rank (this grid has %d): the ranks of a decomposed grid voxelize with their own origin "
                          "through solid.voxelize" % P)
    from . import solid as S
    nbytes = (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
    if isinstance(obstacle, torch.Tensor) and obstacle.dtype == torch.uint8:
        mask = obstacle.to(torch.device("cuda", ctx.device))
    elif isinstance(obstacle, np.ndarray) and obstacle.dtype == np.uint8:
        mask = torch.from_numpy(np.ascontiguousarray(np.asarray(obstacle).reshape(-1, order="F"))).to(torch.device("cuda", ctx.device))
    else:
        tri = np.asarray(obstacle, dtype=np.float64)
        if tri.ndim != 3 or tri.shape[1:] != (3, 3):
            raise L.Ns3dError("obstacle: an (n,3,3) array of triangles in index space, or a uint8 mask; got shape %r" % (tri.shape,))
        return S.voxelize(ctx, tri, *n), tri
    if mask.numel() != nbytes:
        raise L.Ns3dError("obstacle: the mask has %d bytes, a %dx%dx%d grid needs %d" % ((mask.numel(),) + tuple(n) + (nbytes,)))
    ctx.after_torch_fill()
    return mask, None


def _body(solid, mov=None):
    """what stands where the reference calls set_cylinder!: the cylinder's analytic test, ns3d_set_solid with the obstacle's mask, or
    — under `motion` — ns3d_set_solid_moving with the mask and the current pose's numbers"""
    if mov is not None:
        return lambda f, cyl, c: K.set_solid_moving(f.C, f.Vx, f.Vy, f.Vz, mov.mask, mov.motion9, *mov.spacing, ctx=c)
    if solid is None:
        return lambda f, cyl, c: K.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, *cyl, ctx=c)
    return lambda f, cyl, c: K.set_solid(f.C, f.Vx, f.Vy, f.Vz, solid, ctx=c)


def _removed(monitor, solid, fs, ctxs, mov=None):
    """diagnostics=True: the momentum the next masking call removes — the monitor's masked sums, ns3d_solid_momentum for an obstacle,
    ns3d_solid_momentum_moving for one in motion"""
    if monitor is None:
        return None
    if mov is not None:
        return lambda: K.solid_momentum_moving(fs[0].Vx, fs[0].Vy, fs[0].Vz, mov.mask, mov.motion9, *mov.spacing, ctx=ctxs[0])[0]
    if solid is None:
        return lambda: monitor(False).mom
    return lambda: K.solid_momentum(fs[0].Vx, fs[0].Vy, fs[0].Vz, solid, ctx=ctxs[0])[0]


MOTION_KEYS = ("velocity", "omega", "centre")


def _check_motion(motion, P=1):
    """the `motion` keyword of both drivers: None, a dict of MOTION_KEYS (centre is required) or a callable; raises before anything is
    allocated"""
    if motion is None:
        return
    if isinstance(motion, dict):
        if set(motion) - set(MOTION_KEYS) or "centre" not in motion:
            raise L.Ns3dError("motion = %r (None | dict(velocity=…, omega=…, centre=…) with centre given | a callable pose(t))" % (motion,))
        for k, v in motion.items():
            a = np.asarray(v, dtype=np.float64).reshape(-1)
            if a.size != 3 or not np.isfinite(a).all():
                raise L.Ns3dError("motion: %s = %r (need 3 finite numbers)" % (k, v))
    elif not callable(motion):
        raise L.Ns3dError("motion = %r (None | dict(velocity=…, omega=…, centre=…) | a callable pose(t))" % (motion,))
    if P != 1:
        raise L.Ns3dError("motion= runs on one rank (this grid has %d): the ranks of a decomposed grid call ns3d_set_solid_moving with "
                          "their own origin" % P)


def _motion_start(motion, mesh, solid, ctx, p, cyl, dtype, nt):
    """What a run under `motion` keeps: the poses of t = s·dt, s = 0 … nt, evaluated and checked HERE — before a knob of the context
    is set, so that a pose that is refused leaves the context as it was —, the spacings, the mask buffer every pose is voxelized into
    (`solid`, or the cylinder's own mask when there is no obstacle) and, for an obstacle given as triangles (`mesh`), the original
    mesh and a work buffer on the device."""
    from . import solid as S
    spacing = (p.dx, p.dy, p.dz)
    pose = S.rigid_motion(spacing=spacing, **motion) if isinstance(motion, dict) else motion
    poses = []
    for s in range(nt + 1):
        t = s * p.dt
        R, shift, U, omega, centre = (np.array(v, dtype=np.float64) for v in pose(t))
        if R.shape != (3, 3) or any(v.shape != (3,) for v in (shift, U, omega, centre)) or \
                not all(np.isfinite(v).all() for v in (R, shift, U, omega, centre)):
            raise L.Ns3dError("motion: pose(%r) must return finite R (3x3), shift, U, omega, centre (3 each)" % (t,))
        if mesh is None and np.any(shift != 0.0):
            raise L.Ns3dError("motion: a shift of %r at t = %r needs the obstacle as triangles; a mask (or the cylinder) stays where it is "
                              "and only takes the body's velocity" % (tuple(shift), t))
        poses.append(dict(t=t, R=R, shift=shift, U=U, omega=omega, centre=centre))
    mov = SimpleNamespace(poses=poses, spacing=spacing, n=(p.nx, p.ny, p.nz), ctx=ctx, tri0=None, posed=None, motion9=None, log=[],
                          last=(np.eye(3), np.zeros(3)))         # the pose the mask holds: the mesh as given
    if solid is None:
        solid = S.mask_of_cylinder(ctx, mov.n, *cyl, dtype=dtype)
    if mesh is not None:
        mov.tri0 = torch.from_numpy(S.tri_array(mesh).reshape(-1)).to(solid.device)
        mov.posed = torch.empty_like(mov.tri0)
        ctx.after_torch_fill()
    mov.mask = solid
    return mov


def _motion_pose(mov, s, knob=False, record=True):
    """The pose of step s (0: before the loop): logged, its nine numbers (U, omega, centre) made current for the masking calls — and,
    with knob, for ns3d_time_step; the mask is rebuilt in place (the ORIGINAL mesh transformed, then voxelized) when the pose differs
    from the one the mask holds."""
    from . import solid as S
    q = mov.poses[s]
    R, shift = q["R"], q["shift"]
    rebuilt = False
    if mov.tri0 is not None and not (np.array_equal(R, mov.last[0]) and np.array_equal(shift, mov.last[1])):
        S.transform(mov.ctx, mov.tri0, R, q["centre"] - shift, shift, mov.spacing, out=mov.posed)     # about the centre the mesh came with
        K.voxelize(mov.mask, mov.posed, mov.n, ctx=mov.ctx)
        mov.last, rebuilt = (R, shift), True
    mov.motion9 = tuple(q["U"]) + tuple(q["omega"]) + tuple(q["centre"])
    if record:
        mov.log.append(dict(q, rebuilt=rebuilt))
    if knob:
        mov.ctx.set_obstacle_motion(mov.motion9)


def _check_advection(advection, faithful=False, P=1):
    """the `advection` keyword of both drivers → whether the MacCormack scheme runs; raises before anything is allocated or advanced"""
    if advection not in ("reference", "maccormack"):
        raise L.Ns3dError("advection = %r (\"reference\" | \"maccormack\")" % (advection,))
    if advection == "reference":
        return False
    if faithful:
        raise L.Ns3dError("advection=\"maccormack\" advects Vz: it needs faithful=False")
    if P != 1:
        raise L.Ns3dError("advection=\"maccormack\" runs on one rank (this grid has %d): the hat fields of its first stage would need "
                          "a halo exchange between the stages" % P)
    return True


def _check_turbulence(turbulence, P=1):
    """the `turbulence` keyword of both drivers → None, or a namespace with the model's cs; raises before anything is allocated"""
    if turbulence is None:
        return None
    opts = dict(model=turbulence) if isinstance(turbulence, str) else turbulence
    model = opts.get("model") if isinstance(opts, dict) else None
    if not isinstance(model, str) or model not in SGS_MODELS or set(opts) - {"model", SGS_MODELS[model][0]}:
        raise L.Ns3dError("turbulence = %r (None | %s)" % (turbulence, " | ".join(
            "\"%s\" | dict(model=\"%s\", %s=%r)" % (m, m, k, v) for m, (k, v) in SGS_MODELS.items())))
    key, default = SGS_MODELS[model]
    coef = float(opts.get(key, default))
    if not (math.isfinite(coef) and coef >= 0.0):
        raise L.Ns3dError("turbulence: %s = %r (need a finite value >= 0)" % (key, opts.get(key)))
    if P != 1:
        raise L.Ns3dError("turbulence=\"%s\" runs on one rank (this grid has %d): the boundary layer of cells where mu_e is the "
                          "molecular viscosity would sit at the seams, and mu_e's halo would have to be exchanged between the eddy-viscosity "
                          "kernel and the predictor" % (model, P))
    les = SimpleNamespace(model=model)
    setattr(les, key, coef)
    return les


# the `turbulence` keyword's models: the coefficient's key and its default.  cw and c are the published equivalents of cs = 0.17:
# C_w² = 10.6·C_s² (Nicoud & Ducros 1999), c_v = 2.5·C_s² (Vreman 2004)
SGS_MODELS = {"smagorinsky": ("cs", 0.17), "wale": ("cw", 0.5535), "vreman": ("c", 0.07225)}


def sgs_length(les, dx, dy, dz):
    """ℓ of μ_t = ρ·ℓ²·op: cs·Δ, cw·Δ or √c·Δ with Δ = (dx·dy·dz)^(1/3)"""
    delta = (dx * dy * dz) ** (1.0 / 3.0)
    if les.model == "vreman":
        return math.sqrt(les.c) * delta
    return (les.cs if les.model == "smagorinsky" else les.cw) * delta


def _les_start(les, p, f, ctx, in_step):
    """ℓ and the μ_e array of a run; in_step: ns3d_time_step issues the calls (the context's knobs), otherwise _les_predict does"""
    les.length = sgs_length(les, p.dx, p.dy, p.dz)
    les.mu_e = K.zeros(tuple(f.Pr.shape), f.Pr.dtype, f.Pr.device)
    ctx.after_torch_fill()
    if in_step:
        ctx.set_turbulence(les.model, les.length, les.mu_e)


def _les_predict(f, p, ctx, les, fused, write_stress, watch, it):
    """{update_τ!; predict_V!} under the subgrid model's viscosity, call by call — what ns3d_time_step issues under the knob: μ_e, the
    stress arrays where the plain step writes them, the predictor (in one pass, names swapped, if fused).  watch: returns max μ_e
    (the monitor's mu_e_max) and raises where the step would leave the explicit diffusion limit."""
    if les.model == "smagorinsky":
        K.eddy_viscosity(les.mu_e, f.Vx, f.Vy, f.Vz, p.mu, p.rho, les.length, p.dx, p.dy, p.dz, ctx=ctx)
    else:
        K.sgs_viscosity(les.mu_e, f.Vx, f.Vy, f.Vz, les.model, p.mu, p.rho, les.length, p.dx, p.dy, p.dz, ctx=ctx)
    mu_e_max = None
    if watch:
        mu_e_max = K.max_abs(les.mu_e, ctx=ctx)
        number = p.dt * mu_e_max / p.rho * (1.0 / p.dx ** 2 + 1.0 / p.dy ** 2 + 1.0 / p.dz ** 2)
        if not number <= 0.5:
            raise L.Ns3dError("step %d: dt*mu_e_max/rho*(1/dx^2 + 1/dy^2 + 1/dz^2) = %r with mu_e_max = %r is not within 1/2, the explicit "
                              "diffusion limit of the predictor; reduce dt or cs" % (it, number, mu_e_max))
    if write_stress or not fused:
        K.update_tau_var(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, les.mu_e, p.dx, p.dy, p.dz, ctx=ctx)
    if not fused:
        K.predict_V(f.Vx, f.Vy, f.Vz, f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, p.rho, p.g, p.dt, p.dx, p.dy, p.dz, ctx=ctx)
        return mu_e_max
    K.predict_var(f.Vx_o, f.Vy_o, f.Vz_o, f.Vx, f.Vy, f.Vz, les.mu_e, p.rho, p.g, p.dt, p.dx, p.dy, p.dz, ctx=ctx)
    f.Vx, f.Vx_o = f.Vx_o, f.Vx
    f.Vy, f.Vy_o = f.Vy_o, f.Vy
    f.Vz, f.Vz_o = f.Vz_o, f.Vz
    return mu_e_max


SCALAR_KEYS = dict(kappa=None, sct=0.7, beta_g=0.0, c_ref=0.0)      # the `scalar` keyword's keys and defaults (kappa has none)


def _check_scalar(scalar, P=1, p=None):
    """the `scalar` keyword of both drivers → None, or a namespace with kappa, sct, bg (= beta_g) and c_ref; raises before anything
    is allocated.  p: the run's parameters, for the explicit limit of the molecular part (None: not checked yet)"""
    if scalar is None:
        return None
    usage = "scalar = %r (None | dict(kappa=…, sct=0.7, beta_g=0.0, c_ref=0.0))"
    if not isinstance(scalar, dict) or set(scalar) - set(SCALAR_KEYS) or "kappa" not in scalar:
        raise L.Ns3dError(usage % (scalar,))
    vals = {}
    for key, default in SCALAR_KEYS.items():
        try:
            vals[key] = float(scalar.get(key, default))
        except (TypeError, ValueError):
            raise L.Ns3dError(usage % (scalar,)) from None
        if not math.isfinite(vals[key]) or (key in ("kappa", "sct") and vals[key] < 0.0):
            raise L.Ns3dError("scalar: %s = %r (need a finite value%s)" % (key, scalar.get(key), " >= 0" if key in ("kappa", "sct") else ""))
    if P != 1:
        raise L.Ns3dError("scalar=… runs on one rank (this grid has %d): the diffusion step reads C across the seams, so C's halo would "
                          "have to be exchanged between the advection and ns3d_scalar_step" % P)
    if p is not None:
        number = p.dt * vals["kappa"] * (1.0 / p.dx ** 2 + 1.0 / p.dy ** 2 + 1.0 / p.dz ** 2)
        if not number <= 0.5:
            raise L.Ns3dError("scalar: dt*kappa*(1/dx^2 + 1/dy^2 + 1/dz^2) = %r with kappa = %r is not within 1/2, the explicit diffusion "
                              "limit; reduce kappa or dt" % (number, vals["kappa"]))
    return SimpleNamespace(kappa=vals["kappa"], sct=vals["sct"], bg=vals["beta_g"], c_ref=vals["c_ref"])


def _scalar_step(f, p, ctx, sca, les, mu_e_max, it):
    """ns3d_scalar_step call by call — what ns3d_time_step issues under Context.set_scalar, behind the predictor: C diffuses into C_o
    (under the subgrid model's eddy diffusivity while a model is set and sct > 0) and lifts the predicted Vz; the names swap.
    mu_e_max (the monitor's, or None): raises where the step would leave the explicit diffusion limit."""
    eddy = les is not None and sca.sct > 0.0
    sgs = 1.0 / (p.rho * sca.sct) if eddy else 0.0
    if eddy and mu_e_max is not None:
        number = p.dt * (sca.kappa + sgs * (mu_e_max - p.mu)) * (1.0 / p.dx ** 2 + 1.0 / p.dy ** 2 + 1.0 / p.dz ** 2)
        if not number <= 0.5:
            raise L.Ns3dError("step %d: dt*(kappa + (mu_e_max - mu)/(rho*sct))*(1/dx^2 + 1/dy^2 + 1/dz^2) = %r with mu_e_max = %r is not "
                              "within 1/2, the explicit diffusion limit of the scalar; reduce dt or raise sct" % (it, number, mu_e_max))
    K.scalar_step(f.C_o, f.Vz, f.C, les.mu_e if eddy else None, sca.kappa, sgs, p.mu, sca.bg, sca.c_ref, p.dt, p.dx, p.dy, p.dz, ctx=ctx)
    f.C, f.C_o = f.C_o, f.C


def _alloc_hats(f, ctx):
    """buffers for stage 1 of the MacCormack advection (Vx, Vy, Vz, C) when the step runs call by call"""
    hats = tuple(K.zeros(tuple(a.shape), a.dtype, a.device) for a in (f.Vx, f.Vy, f.Vz, f.C))
    ctx.after_torch_fill()
    return hats


def _advect_mc_swap(f, hats, p, ctx):
    """{X_o .= X; advect!} (multi.jl:475-476 / gpu.jl:141-142) replaced by the limited MacCormack advection: ns3d_advect_mc reads the
    current fields, leaves stage 1 in `hats` and writes COMPLETE new fields into the *_o buffers, then all four names swap."""
    K.advect_mc(f.Vx_o, f.Vx, hats[0], f.Vy_o, f.Vy, hats[1], f.Vz_o, f.Vz, hats[2], f.C_o, f.C, hats[3], p.dt, p.dx, p.dy, p.dz, ctx=ctx)
    f.Vx, f.Vx_o = f.Vx_o, f.Vx
    f.Vy, f.Vy_o = f.Vy_o, f.Vy
    f.Vz, f.Vz_o = f.Vz_o, f.Vz
    f.C, f.C_o = f.C_o, f.C


def gpu_initial_fields(p):
    """gpu.jl:62-63,85-88: LinRange cell centres, 1/7-power-law Vx profile, hydrostatic Pr (host setup)."""
    nx, ny, nz = p.nx, p.ny, p.nz
    t = np.arange(nz, dtype=np.float64) / (nz - 1)                    # Julia LinRange: (1-t)*a + t*b
    zc = (1 - t) * (-(p.lz - p.dz) / 2) + t * ((p.lz - p.dz) / 2)
    prof = p.vin * (7.0 / 6.0) * ((zc + p.lz / 2) / p.lz) ** (1.0 / 6.0)
    Vx = np.empty((nx + 1, ny, nz), order="F"); Vx[:, :, :] = prof[None, None, :]
    Pr = np.empty((nx, ny, nz), order="F"); Pr[:, :, :] = (-(zc - p.lz / 2) * p.rho * p.g)[None, None, :]
    return Vx, Pr


def _save_mat(path, f, p, step0):
    """matwrite("out_save/step_$it.mat", Dict("Pr","Vx","Vy","Vz","C","dx","dy","dz")) (gpu.jl:168-170); the step-0 dictionary
    of gpu.jl:89 repeats the key "Vy" — the later pair wins in a Julia Dict literal, so it holds Vz's array under "Vy" and has
    no "Vz" — reproduced.  Written as MAT v5 (scipy.io.savemat; MAT.jl writes v7.3/HDF5 by default and reads both, as do MATLAB
    and Octave): same variable names, shapes and Float64 values, different container version."""
    from scipy.io import savemat
    d = {"Pr": K.to_numpy(f.Pr), "Vx": K.to_numpy(f.Vx), "C": K.to_numpy(f.C), "dx": p.dx, "dy": p.dy, "dz": p.dz}
    if step0:
        d["Vy"] = K.to_numpy(f.Vz)
    else:
        d["Vy"] = K.to_numpy(f.Vy)
        d["Vz"] = K.to_numpy(f.Vz)
    savemat(path, d, format="5", do_compression=False, oned_as="column")


def runme(do_vis=False, do_save=False, *, nx=255, nt=10000, mode="strict", fused=True, dtype=torch.float64,
          faithful=True, device=None, niter_cap=None, do_print=False, initial=None, pressure="pt", one_call=True,
          diagnostics=False, statistics=None, stats_every=1, vortex=False, tracers=None, probes=None, isosurface=None,
          advection="reference", obstacle=None, turbulence=None, scalar=None, motion=None):
    """runme (gpu.jl:12-173): single device, gravity, hydrostatic x-planes.  Returns (fields, info).
    nx/nt are literals in the reference (gpu.jl:44,51: 255, 10000) and keyword options here.  do_save writes the MAT files
    of gpu.jl:89,168-170 (step 0 and every nsave = 10 steps); do_vis the heat maps of gpu.jl:90-117,143-167 (frame 0 and
    every nvis = 10 steps).
    diagnostics=True: as in run_navierstokes3D — the monitor before the set_cylinder! calls :123 and :139 and after :140, one
    record per step in info.diag (gpu.jl's form of the cylinder test, its dx-for-dy quirk included), a line per step with
    do_print; the step runs call by call (`one_call` is not used) and returns the same bits.
    statistics / stats_every: as in run_navierstokes3D, sampled after :142; info.stats holds the FULL local arrays (boundary cells
    included).
    vortex=True: as in run_navierstokes3D, of the final state and — with do_vis — of every frame's; info.vortex holds the FULL
    local arrays Wx, Wy, Wz, Q (their boundary entries are 0); do_vis adds 3D_NavierStokes_Wz_%04d.png, …_Q_…, …_long_Wy_…,
    …_long_Q_… (do_save's MAT files are left as the reference writes them).
    tracers / probes: as in run_navierstokes3D, advanced resp. sampled after :142; do_save adds out_save/out_tracers_%04d.bin beside
    each MAT file (numbered 0, 1, … in the order the MAT files are written), do_vis 3D_NavierStokes_tracers_%04d.png per frame.
    isosurface: as in run_navierstokes3D, of the final state → info.isosurface; do_save adds out_save/out_iso_%04d.ply beside each
    MAT file (numbered like the tracer dumps).
    advection: as in run_navierstokes3D, in place of :141-142; "maccormack" needs faithful=False.
    obstacle: as in run_navierstokes3D, in place of the set_cylinder! calls :123 and :139.
    turbulence: as in run_navierstokes3D, in place of :121-122.
    scalar: as in run_navierstokes3D, between :122 and :123.
    motion: as in run_navierstokes3D, at the set_cylinder! calls :123 and :139 (gpu.jl masks nothing before its loop)."""
    maccormack = _check_advection(advection, faithful)
    les = _check_turbulence(turbulence)
    sca = _check_scalar(scalar, 1, gpu_params(nx))
    _check_motion(motion)
    if device is None:
        device = torch.cuda.current_device()
    p = gpu_params(nx)
    nx, ny, nz = p.nx, p.ny, p.nz
    grid = ZSlabGrid(nx, ny, nz, alone=True)                # the observers' view of this script: one rank
    watch = dict(statistics=statistics, stats_every=stats_every, vortex=vortex, tracers=tracers, probes=probes, isosurface=isosurface)
    check_options(grid, **watch)
    dev = torch.device("cuda", device)
    ctx = K.Context(device, mode, async_=True)
    niter = p.niter if niter_cap is None else min(p.niter, niter_cap)
    f = _alloc(nx, ny, nz, dtype, dev)
    Vx0, Pr0 = initial if initial is not None else gpu_initial_fields(p)
    f.Vx = K.from_numpy(np.asarray(Vx0).astype(np.float64 if dtype == torch.float64 else np.float32), dev)
    f.Pr = K.from_numpy(np.asarray(Pr0).astype(np.float64 if dtype == torch.float64 else np.float32), dev)
    cyl = (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    pt = K.pt_params(f.Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_GPU, False, 0.0, p.g)
    info = SimpleNamespace(iters=[], errs=[], params=p)
    solid, mesh = _obstacle_mask(obstacle, 1, ctx, (nx, ny, nz))
    mov = None
    if motion is not None:
        mov = _motion_start(motion, mesh, solid, ctx, p, cyl, dtype, nt)
        solid = mov.mask
    body = _body(solid, mov)
    nsave = nvis = 10                                                                         # :50,52
    obs = Observers(grid, [ctx], p, nt, dtype, gathered=False, **watch)
    iframe = 0

    def saved(it):                                  # :89 / :168-170; the observers' dumps are numbered in the MAT files' order
        os.makedirs("./out_save", exist_ok=True)
        ctx.sync()
        _save_mat("out_save/step_%d.mat" % it, f, p, it == 0)
        obs.frame([f], save=it // nsave)

    def drawn():                                    # :90-117 / :143-167
        nonlocal iframe
        ctx.sync()
        save_frame_gpu({n: K.to_numpy(getattr(f, n)) for n in ("Pr", "C", "Vx", "Vy", "Vz")}, ny, nz, iframe)
        obs.frame([f], vis=iframe)
        iframe += 1

    if do_save:                                                                               # :89
        saved(0)
    if do_vis:                                                                                # :90-117
        drawn()
    monitor = None
    if diagnostics:
        info.diag = []
        monitor = _monitor(grid, [ctx], [f], [cyl if solid is None else None], p)
    removed = _removed(monitor, solid, [f], [ctx], mov)
    obs.start()
    step_params = None
    if fused and one_call and not diagnostics:
        step_params = _step_params(L.NS3D_BC_GPU, p, niter, faithful, pressure)
    if solid is not None and step_params is not None:
        ctx.set_obstacle(solid)                             # ns3d_time_step masks with it (the context is this run's own)
    if les is not None:
        _les_start(les, p, f, ctx, step_params is not None)     # ns3d_time_step predicts under it; cleared after the loop
    if sca is not None and step_params is not None:
        ctx.set_scalar(sca.kappa, sca.sct, sca.bg, sca.c_ref)   # ns3d_time_step diffuses and lifts with it; cleared after the loop
    hats = None
    if maccormack and step_params is not None:
        ctx.set_advection("maccormack")                     # ns3d_time_step advects with it (the context is this run's own)
    elif maccormack:
        hats = _alloc_hats(f, ctx)
    for it in range(1, nt + 1):                                                               # :119
        if mov is not None:
            _motion_pose(mov, it, step_params is not None)
        if step_params is not None:                         # :121-142 (ns3d_time_step swaps the names in f like the swaps below)
            step_params.write_stress = 1 if it == nt else 0
            done, errs = K.time_step(f, step_params, ctx=ctx)
        else:
            if les is not None:         # :121-122 under the Smagorinsky viscosity
                mu_e_max = _les_predict(f, p, ctx, les, fused, it == nt, monitor is not None, it)
            elif fused:
                if it == nt:            # the stress arrays as the reference leaves them after its last step: same final state
                    K.update_tau(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, p.mu, p.dx, p.dy, p.dz, ctx=ctx)
                _predict_swap(f, p, ctx)                                                      # :121-122 in one pass
            else:
                K.update_tau(f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, f.Vx, f.Vy, f.Vz, p.mu, p.dx, p.dy, p.dz, ctx=ctx)  # :121
                K.predict_V(f.Vx, f.Vy, f.Vz, f.txx, f.tyy, f.tzz, f.txy, f.txz, f.tyz, p.rho, p.g, p.dt, p.dx, p.dy, p.dz,
                            ctx=ctx)                                                          # :122
            if sca is not None:         # the active scalar: where ns3d_time_step issues it under the knob
                _scalar_step(f, p, ctx, sca, les, mu_e_max if les is not None else None, it)
            if monitor:
                mom_predict = removed()
            body(f, cyl, ctx)                                                                 # :123
            K.update_divV(f.divV, f.Vx, f.Vy, f.Vz, p.dx, p.dy, p.dz, ctx=ctx)                # :124
            if pressure == "direct":        # (:125, :134 print after the step)  outside parity: the exact solution of what :126-137 iterates towards
                K.poisson_direct(f.Pr, f.dPrdtau, f.divV, pt, ctx=ctx)
                done, errs = 0, [K.residual_max(f.Pr, f.divV, pt, ctx=ctx) * (p.ly * p.ly) / p.psc]
            elif fused:
                done, errs = K.pt_solve(f.Pr, f.dPrdtau, f.divV, pt, p.eps, niter, p.nchk, p.ly * p.ly, p.psc, ctx=ctx)
            else:
                errs, done = [], niter
                for itr in range(1, niter + 1):                                               # :126
                    K.update_dPrdtau(f.Pr, f.dPrdtau, f.divV, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, ctx=ctx)  # :127
                    K.update_Pr(f.Pr, f.dPrdtau, p.dtau, ctx=ctx)                             # :128
                    K.set_bc_Pr_gpu(f.Pr, p.dz, nz, p.g, p.rho, ctx=ctx)                      # :129
                    if itr % p.nchk == 0:                                                     # :130
                        K.compute_res(f.Rp, f.Pr, f.divV, p.rho, p.dt, p.dx, p.dy, p.dz, ctx=ctx)  # :131
                        err = K.max_abs(f.Rp, ctx=ctx) * (p.ly * p.ly) / p.psc                      # :132
                        errs.append(err)
                        if err < p.eps or not math.isfinite(err):                             # :135
                            done = itr
                            break
            K.correct_V(f.Vx, f.Vy, f.Vz, f.Pr, p.dt, p.rho, p.dx, p.dy, p.dz, ctx=ctx)       # :138
            if monitor:
                mom_correct = removed()
            body(f, cyl, ctx)                                                                 # :139
            K.set_bc_Vel_gpu(f.Vx, f.Vy, f.Vz, ctx=ctx)                                       # :140
            if monitor:
                info.diag.append(_diag_step_record(monitor(True), mom_predict, mom_correct, p))
                if les is not None:
                    info.diag[-1].mu_e_max = mu_e_max
            if maccormack:
                _advect_mc_swap(f, hats, p, ctx)                                              # :141-142 as the limited MacCormack scheme
            elif fused:
                _copy_advect_swap(f, p, faithful, ctx)                                        # :141-142 in one pass
            else:
                K.copy(f.Vx_o, f.Vx, ctx=ctx); K.copy(f.Vy_o, f.Vy, ctx=ctx)                  # :141
                K.copy(f.Vz_o, f.Vz, ctx=ctx); K.copy(f.C_o, f.C, ctx=ctx)
                K.advect(f.Vx, f.Vx_o, f.Vy, f.Vy_o, f.Vz, f.Vz_o, f.C, f.C_o, p.dt, p.dx, p.dy, p.dz, faithful, ctx=ctx)  # :142
        info.iters.append(done); info.errs.append(errs)
        if do_print:                                                                          # :125, :134
            _print_step(it, errs, p.nchk, info.diag[-1] if monitor else None)
        obs.end_step(it, [f])
        if do_vis and it % nvis == 0:                                                         # :143-167
            drawn()
        if do_save and it % nsave == 0:                                                       # :168-170
            saved(it)
    if mov is not None and step_params is not None:
        ctx.set_obstacle_motion(None)
    if solid is not None and step_params is not None:
        ctx.set_obstacle(None)
    if les is not None:
        ctx.set_turbulence(None)
    if sca is not None and step_params is not None:
        ctx.set_scalar(None)
    if fused and faithful and nt > 0:
        K.copy(f.Vz_o, f.Vz, ctx=ctx)       # the one copy of :141 the swaps skipped (Vz is never advected): same final state
    ctx.sync()
    info.ctx = ctx
    obs.finish(info, [f])
    if les is not None:
        info.turbulence = dict(model=les.model, length=les.length, mu_e=K.to_numpy(les.mu_e))
    if sca is not None:
        info.scalar = dict(kappa=sca.kappa, sct=sca.sct, bg=sca.bg, c_ref=sca.c_ref)
    if mov is not None:
        info.motion = mov.log
    return f, info
