"""The obstacle step's shared scenario (tests/test_solid_step_host.py, tests/test_gpu_solid_step.py, the footprint and stream-order
harnesses): a state in which every bit of an obstacle's mask acts on a non-zero value, a body that meets five of the six outer planes,
and the CPU statement of the whole step — oracle/driver_ref.py with obstacle= and initial= — computed once per process and never
modified.  The host tests assert that the scenario is admissible (every masking call and every mask bit changes the result, every
field stays finite), so that the device comparisons built on it cannot pass vacuously."""
import functools
from types import SimpleNamespace

import numpy as np

import solid_cases as SC
import solid_ref as SR
from util import SHAPES, bits_equal

NX, NT = 24, 2
GRID = (24, 15, 15)
FIVE = ("C", "Pr", "Vx", "Vy", "Vz")
ELEVEN = FIVE + ("Vx_o", "Vy_o", "Vz_o", "C_o", "dPrdtau", "divV")
KIND = {"C": "c", "Pr": "c", "Vx": "vx", "Vy": "vy", "Vz": "vz"}
BIT_COUNTS = (355, 387, 355, 383)          # C, Vx, Vy, Vz bits of body_mask()
SCRIPTS = ("multi", "gpu")
DTYPES = {"f64": np.float64, "f32": np.float32}
SCHEMES = ("reference", "maccormack")


def box_mesh(lo, hi):
    """navierstokes3d_amd.solid.box_mesh (host code; the import is kept out of this module's load)"""
    from navierstokes3d_amd import solid as S
    return S.box_mesh(lo, hi)


def body():
    """three pieces, (32,3,3): an octahedron inside the flow, a box through the planes i = 0 and k = 0, a box through i = nx, j = ny
    and k = nz"""
    return np.concatenate([SC.octahedron((13.3, 7.4, 8.1), (4.2, 3.9, 5.3)), box_mesh((-1, 3, -1), (4, 8, 6)),
                           box_mesh((20, 9.5, 10), (25, 16, 16))])


@functools.lru_cache(maxsize=None)
def body_mask():
    m = SR.voxelize(body(), *GRID)
    m.setflags(write=False)
    return m


def params(script, dtype=np.float64):
    """the oracle's parameters of the script at nx = 24, with the cylinder's coordinates of rank 0 (multi.jl:363-365)"""
    from oracle import driver_ref as D
    if script == "multi":
        p = D.multi_params(NX, dtype=dtype)
        p.xco_g = D._x_g(1, p.dx, p.nx, p.nx, 0) - (p.lx - p.dx) / 2
        p.yco_g = D._x_g(1, p.dy, p.ny, p.ny, 0) - (p.ly - p.dy) / 2
        p.zco_g = D._x_g(1, p.dz, p.nz, p.nz, 0) - (p.lz - p.dz) / 2
    else:
        p = D.gpu_params(NX, dtype)
    assert (p.nx, p.ny, p.nz) == GRID
    return p


@functools.lru_cache(maxsize=None)
def cylinder_mask(script, dt):
    """The reference cylinder's own mask without a device (the method of navierstokes3d_amd.solid.mask_of_cylinder): the oracle's
    set_cylinder / set_cylinder_local on sentinel fields — C = 0, V = 1 — and the flags read off."""
    from oracle import oracle as K
    dtype = DTYPES[dt]
    p = params(script, dtype)
    nx, ny, nz = GRID
    Cf = K.zeros(GRID, dtype)
    V = [np.asfortranarray(np.ones(SHAPES[k](*GRID), dtype=dtype)) for k in ("vx", "vy", "vz")]
    if script == "multi":
        K.set_cylinder(Cf, *V, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    else:
        K.set_cylinder_local(Cf, *V, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    m = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    m[:nx, :ny, :nz] |= (Cf == 1).astype(np.uint8)
    m[:, :ny, :nz] |= (V[0] == 0).astype(np.uint8) << 1
    m[:nx, :, :nz] |= (V[1] == 0).astype(np.uint8) << 2
    m[:nx, :ny, :] |= (V[2] == 0).astype(np.uint8) << 3
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def initial_state(dt):
    """The seeded state, non-zero at every node of all five fields: V and Pr uniform in ±1e-2 with |value| ≥ 1e-4, C uniform in
    [1e-3, 1 − 1e-3] — so a C bit stores another value than the one it finds (1) and a velocity bit removes a non-zero one.  Drawn in
    float64 and rounded to the element type: the device and the oracle are handed the same arrays."""
    rng = np.random.Generator(np.random.MT19937(20261))
    out = {}
    for name in FIVE:
        shape = SHAPES[KIND[name]](*GRID)
        if name == "C":
            a = rng.uniform(1e-3, 1.0 - 1e-3, size=shape)
        else:
            a = rng.uniform(1e-4, 1e-2, size=shape) * np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)
        a = np.asfortranarray(a.astype(DTYPES[dt]))
        a.setflags(write=False)
        out[name] = a
    return out


@functools.lru_cache(maxsize=None)
def scenario(script, dt):
    """grid 24×15×15, nt = 2, niter_cap = 3·nchk (42 iterations), faithful = False; .mask the body's, .initial the seeded state"""
    p = params(script, DTYPES[dt])
    assert p.nchk == 14
    return SimpleNamespace(script=script, dt=dt, dtype=DTYPES[dt], p=p, grid=GRID, nt=NT, niter=3 * p.nchk, mask=body_mask(),
                           initial=initial_state(dt))


def run_ref(script, dtype, nt=NT, advection="reference", obstacle=None, initial=None, niter_cap=None, faithful=False):
    """(the driver's local state, its info) of run_navierstokes3D_ref ("multi") or runme_ref ("gpu") at nx = 24; obstacle and initial
    are passed only when given"""
    from oracle.driver_ref import run_navierstokes3D_ref, runme_ref
    kw = dict(nx=NX, nt=nt, faithful=faithful, dtype=dtype, niter_cap=niter_cap, advection=advection)
    if obstacle is not None:
        kw["obstacle"] = obstacle
    if initial is not None:
        kw["initial"] = initial
    with np.errstate(all="ignore"):
        if script == "multi":
            out = run_navierstokes3D_ref(**kw)
            info, f = out[-1], out[-1].ranks[0]
            assert all(bits_equal(f[n][1:-1, 1:-1, 1:-1], a) for n, a in zip(FIVE, out[:5]))       # gather! strips one cell per side
        else:
            f, info = runme_ref(**kw)
    return f, info


@functools.lru_cache(maxsize=None)
def scenario_ref(script, dt, advection="reference", mask="body"):
    """The oracle driver's run of the scenario, once per process, never modified: (fields by name, info).  mask: "body", "cylinder"
    (the cylinder's own mask through obstacle=) or None (no obstacle: the script's cylinder calls)."""
    sc = scenario(script, dt)
    m = {"body": sc.mask, "cylinder": cylinder_mask(script, dt), None: None}[mask]
    f, info = run_ref(script, sc.dtype, sc.nt, advection, m, sc.initial, sc.niter)
    fields = {n: f[n] for n in ELEVEN}
    for a in fields.values():
        a.setflags(write=False)
    return fields, info
