"""The moving-body step's shared scenarios (tests/test_moving_host.py, tests/test_gpu_moving.py): three bodies in motion at 24×15×15 —
a box mesh that turns fast enough for its mask to change every step, the same box translating, and the script's own cylinder (its
mask fixed) spinning about its axis — their poses per step, and the CPU statements of three steps (tests/moving_ref.py), computed once
per process and never modified.  The poses are evaluated ONCE, by navierstokes3d_amd.solid.rigid_motion, and the same list is handed
to the statement and to the device run."""
import functools
from types import SimpleNamespace

import numpy as np

import moving_ref as MR
import solid_ref as SR
import solid_step_cases as SS

GRID, NT, NITER = SS.GRID, 3, 42
BOX = ((8.3, 4.6, 5.2), (13.7, 10.1, 9.9))
BOX_CENTRE = (11.0, 7.35, 7.55)
MOVERS = ("spin", "slide", "cylinder")
ANGLE = 0.35                    # radians per step of "spin": the 5.4 × 5.5 cell box turns by more than half a cell at its corners
AXIS = (0.36, -0.48, 0.8)       # its unit axis, tilted: all three components of the body's velocity act, Vz's stagger included


def params(script):
    """the package's parameters of the script at nx = 24 (the numbers the device run is given)"""
    from navierstokes3d_amd.params import gpu_params, multi_params
    p = multi_params(SS.NX) if script == "multi" else gpu_params(SS.NX)
    assert (p.nx, p.ny, p.nz) == GRID
    return p


def box():
    from navierstokes3d_amd import solid as S
    return S.box_mesh(*BOX)


@functools.lru_cache(maxsize=None)
def box_mask():
    m = SR.voxelize(box(), *GRID)
    m.setflags(write=False)
    return m


def keyword(script, name, sign=1.0):
    """the drivers' motion= dict of a mover"""
    p = params(script)
    if name == "spin":
        return dict(omega=tuple(sign * ANGLE / p.dt * a for a in AXIS), centre=BOX_CENTRE)
    if name == "slide":
        return dict(velocity=(0.6 * p.dx / p.dt, 0.3 * p.dy / p.dt, 0.0), centre=BOX_CENTRE)
    assert name == "cylinder"       # about its own axis: (ox, oy) from the box's centre line, along z
    return dict(omega=(0.0, 0.0, sign * 2.0), centre=((p.ox + p.lx / 2) / p.dx, (p.oy + p.ly / 2) / p.dy, p.nz / 2))


@functools.lru_cache(maxsize=None)
def mover(script, name, dt="f64", sign=1.0):
    """.tri (the original mesh, or None), .mask0, .poses[0 … NT] (pose(s·dt)), .d the spacings, .keyword"""
    from navierstokes3d_amd import solid as S
    p = params(script)
    d = (p.dx, p.dy, p.dz)
    kw = keyword(script, name, sign)
    pose = S.rigid_motion(spacing=d, **kw)
    tri, mask0 = (None, SS.cylinder_mask(script, dt)) if name == "cylinder" else (box(), box_mask())
    return SimpleNamespace(name=name, tri=tri, mask0=mask0, poses=[pose(s * p.dt) for s in range(NT + 1)], d=d, keyword=kw)


def masking(script, name, dt="f64", pre=0, sign=1.0):
    mv = mover(script, name, dt, sign)
    return MR.Masking(mv.poses, mv.tri, mv.mask0, GRID, mv.d, pre=pre)


def _frozen(f, names, mk, steps):
    fields = {n: f[n] for n in names}
    for a in fields.values():
        a.setflags(write=False)
    return SimpleNamespace(fields=fields, steps=steps, masks=mk.masks, removed=mk.removed, rebuilt=mk.rebuilt)


@functools.lru_cache(maxsize=None)
def oracle_run(script, dt, name, advection="reference", pressure="pt", nt=NT):
    """oracle/driver_ref.py's run from solid_step_cases.initial_state(dt) under the mover; multi.jl's masking before the loop (:372)
    stores the pose of t = 0"""
    mk = masking(script, name, dt, pre=1 if script == "multi" else 0)
    f, info = MR.run_oracle(script, SS.DTYPES[dt], mk, nt, SS.initial_state(dt), NITER, advection, pressure)
    return _frozen(f, SS.ELEVEN, mk, [(it, list(e)) for it, e in zip(info.iters, info.errs)])


def host_state64(script):
    """test_gpu_les.host_state: the script's own initial state in the seventeen arrays, float64"""
    import test_gpu_les as GL
    return GL.host_state(script)


def scalar_knob(script):
    import test_gpu_scalar as GSC
    return GSC.knob_values(script)


@functools.lru_cache(maxsize=None)
def wale_scalar_run(script, name, nt=NT):
    """tests/scalar_ref.py::step under WALE with the scalar on, from the script's own initial state, under the mover (float64)"""
    import sgs_ref
    p = params(script)
    f = host_state64(script)
    mk = masking(script, name)
    steps, mu_e = MR.run_scalar_ref(script, f, p, mk, nt, NITER, sca=scalar_knob(script), op=sgs_ref.WALE,
                                    length=sgs_ref.length_of(sgs_ref.WALE, p.dx, p.dy, p.dz))
    out = _frozen(f, tuple(f), mk, steps)
    out.mu_e = mu_e
    return out


@functools.lru_cache(maxsize=None)
def rest_run(sign, nt=NT, pressure="pt"):
    """a spinning box in fluid at rest: the multi script with vin = 0 from an all-zero state, scalar_ref.step's plain sequence —
    with the PT loop capped at NITER, or with oracle/direct_ref.py's solve"""
    import copy
    p = copy.copy(params("multi"))
    p.vin = 0.0
    f = {k: np.zeros_like(a) for k, a in host_state64("multi").items()}
    mk = masking("multi", "spin", sign=sign)
    steps, _ = MR.run_scalar_ref("multi", f, p, mk, nt, NITER, pressure=pressure)
    return _frozen(f, tuple(f), mk, steps), p


@functools.lru_cache(maxsize=None)
def direct_run(script, name, work=np.float64, nt=2):
    """scalar_ref.step's plain sequence with oracle/direct_ref.py's solve, its sums carried in `work`, from the script's own state"""
    f = host_state64(script)
    mk = masking(script, name)
    steps, _ = MR.run_scalar_ref(script, f, params(script), mk, nt, NITER, pressure="direct", work=work)
    return _frozen(f, tuple(f), mk, steps)


@functools.lru_cache(maxsize=None)
def driver_run(script, name, nt=NT):
    """the oracle driver from the script's OWN initial state under the mover: what the package's drivers compute with motion="""
    mk = masking(script, name, "f64", pre=1 if script == "multi" else 0)
    f, info = MR.run_oracle(script, np.float64, mk, nt, None, NITER)
    return _frozen(f, SS.FIVE, mk, [(it, list(e)) for it, e in zip(info.iters, info.errs)])
