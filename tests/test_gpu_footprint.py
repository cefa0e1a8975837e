"""Footprint tests: every entry point of navierstokes3d_amd.kernels with ALL its device arrays in a guarded arena (tests/arena.py) —
views into one flat buffer per element type, each array at an odd element offset (the alignment of its element type and no better),
a NaN-filled guard gap of at least a plane plus a row on both sides, outputs interleaved with inputs.

Each case runs the call and asserts
  (a) every guard word still holds its bit pattern (nothing was stored outside the arrays; the checker names array, side, distance);
  (b) the outputs are correct: in STRICT the oracle's bits (oracle.*, _oracle_iters, vortex_ref, tracers_ref, isosurface_ref, the
      NumPy statistics), and in every mode the very bits of the same context's call on ordinarily allocated copies of the same inputs
      (the existing FAST tests hold those to their bounds).  A guard NaN that an out-of-bounds load drags into an output fails here;
  (c) the inputs are bit-identical afterwards.
No tolerance is introduced; the one bar in this file is test_gpu_direct.py's twin bar for ns3d_poisson_direct, unchanged.

What this cannot see: a stray load whose value is discarded (tests/arena.py).  The multi-rank forms are not here: their per-rank
kernels are the ones below and their exchange buffers are the library's own."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as AR
import isosurface_ref as IR
import tracers_ref as TR
import vortex_ref as VR
from test_arena_host import check_layout, check_reports, sample_arrays
from test_gpu_pt import SHAPES2, SHAPESN, VARIANTS, _oracle_iters, _params
from util import SHAPES, bits_equal, fields, first_bit_difference, geometry, rel_l2, rnd

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
DTS = ["f64", "f32"]
MODES = ["strict", "fast"]
GID = lambda n: "%dx%dx%d" % tuple(n)
RULES = [(0, True, 0.75), (1, False, 0.0)]


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def _up(hip, a):
    a = np.asarray(a)
    return hip.from_numpy(a) if a.ndim == 3 else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _down(hip, t):
    return hip.to_numpy(t) if t.dim() == 3 else t.cpu().numpy()


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _exact(a, b):
    """the same bits, NaN payloads included"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all(_words(np.asfortranarray(a)) == _words(np.asfortranarray(b))))


def _same_result(a, b):
    """scalars, tuples and lists of scalars a call returns on the host (a NaN equals a NaN)"""
    if isinstance(a, SimpleNamespace):
        a, b = vars(a), vars(b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_result(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_result(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return bool(np.array_equal(np.float64(a), np.float64(b), equal_nan=True))


def footprint(hip, arrays, call, what, ref=None, ref_result=None, part=None, ref_part=None, arena_first=False):
    """arrays: [(name, host array, is_output)]; call(t) makes the library call on the dict t of device arrays and returns what the
    call returns on the host.  Runs it on plain copies, then in an arena, and asserts (a), (b), (c) of the module docstring.
    ref: {name: oracle bits} (STRICT); part / ref_part: {name: function cutting out of an output the part that is compared with the plain
    call's / the reference's} for calls that compute a plane range only; arena_first: the call in the arena is made before the one on
    plain arrays (a call that does more the first time it sees a grid).  Returns (the arena call's result, the arena)."""
    plain = {n: _up(hip, a) for n, a, _ in arrays}
    ar = AR.Arena(arrays, "cuda")
    torch.cuda.synchronize()
    r_plain = r_arena = None
    for in_arena in ((True, False) if arena_first else (False, True)):
        if in_arena:
            r_arena = call(ar.t)
        else:
            r_plain = call(plain)
        torch.cuda.synchronize()
    ar.assert_clean(str(what))                                                                      # (a)
    cut = lambda n, a: part[n](a) if part and n in part else a
    rcut = lambda n, a: ref_part[n](a) if ref_part and n in ref_part else a
    for n, a, is_out in arrays:
        got = ar.get(n)
        if is_out:
            want = _down(hip, plain[n])
            assert _exact(cut(n, got), cut(n, want)), (what, n, "differs from the call on plain arrays",
                                                       first_bit_difference(cut(n, got), cut(n, want)) if got.dtype.itemsize > 1 else None)
            if ref is not None and n in ref:                                                        # (b)
                assert bits_equal(rcut(n, got), rcut(n, ref[n])) if got.dtype.itemsize > 1 else np.array_equal(got, ref[n]), \
                    (what, n, "differs from the reference", first_bit_difference(rcut(n, got), rcut(n, ref[n])) if got.dtype.itemsize > 1 else None)
        else:
            assert _exact(got, np.asarray(a)), (what, n, "an input was modified")                  # (c)
            assert _exact(_down(hip, plain[n]), np.asarray(a)), (what, n, "an input of the plain call was modified")
    assert _same_result(r_arena, r_plain), (what, r_arena, r_plain)
    if ref_result is not None:
        assert _same_result(r_arena, ref_result), (what, r_arena, ref_result)
    return r_arena, ar


# ---- 0. the arena itself, on the device -------------------------------------------------------------------------------------------
def test_arena_on_the_device(hip):
    arrays = sample_arrays()
    ar = AR.Arena(arrays, "cuda")
    for buf in ar.buf.values():
        assert buf.data_ptr() % 512 == 0
    check_layout(ar, arrays)
    check_reports(ar, arrays)                     # guards dirtied by plain torch index assignments
    # … and by a kernel's own stores: ns3d_copy is told that the array is three elements longer than the arena made it (a view that
    # reaches into the guard behind it, inside the buffer), and the checker reports exactly those three
    s = ar.slots["Pr"]
    n = s.numel + 3
    longer = ar.buf[s.dtype][s.offset:s.offset + n].view(1, 1, n).permute(2, 1, 0)
    exact = ar.buf[s.dtype][s.offset:s.offset + s.numel].view(1, 1, s.numel).permute(2, 1, 0)
    # the second check, a kernel's load: one guard word read along with the array poisons the result (max_abs propagates NaN)
    assert hip.max_abs(exact) == float(np.abs(ar.get("Pr")).max())
    assert math.isnan(hip.max_abs(ar.buf[s.dtype][s.offset - 1:s.offset + s.numel].view(1, 1, s.numel + 1).permute(2, 1, 0)))
    assert math.isnan(hip.max_abs(longer)) and ar.check() == []
    hip.copy(longer, hip.from_numpy(np.full((n, 1, 1), 2.5)))
    torch.cuda.synchronize()
    (f,) = ar.check()
    assert (f.array, f.side, f.first, f.last, f.count) == ("Pr", "behind", 1, 3, 3), f
    assert (ar.get("Pr") == 2.5).all()


# ---- 1. the elementary 256-thread kernels -------------------------------------------------------------------------------------------
EL_GRIDS = [(3, 3, 3), (5, 4, 3), (70, 6, 7), (130, 5, 4)]


def _cyl_scalars(beta, form, g3):
    nx, ny, nz = g3
    dx, dy, dz = 1.0 / nx, 0.6 / ny, 0.6 / nz
    sc = (0.0121, 0.0064, -0.1, 0.02, np.sin(beta), np.cos(beta))
    if form == "glob":
        return sc + (-(1 - dx) / 2, -(0.6 - dy) / 2, -(0.6 - dz) / 2, 1.0, 0.6, 0.6, dx, dy, dz)
    return sc + (1.0, 0.6, 0.6, dx, dy, dz)


def _res_max_ref(oracle, Pr, rhs, g):
    Rp = np.zeros(tuple(n - 2 for n in Pr.shape), dtype=Pr.dtype, order="F")
    oracle.compute_res(Rp, Pr, rhs, g["rho"], g["dt"], g["dx"], g["dy"], g["dz"])
    return oracle.max_abs(Rp)


def _row(name, kinds, outs, scalars, oracle_name=None, hip_name=None):
    """a call with the oracle's own name and argument list: arrays of `kinds`, then scalars(g, grid)"""
    def call(hip, ctx, t, g, grid):
        return getattr(hip, hip_name or name)(*t, *scalars(g, grid), ctx=ctx)

    def ref(oracle, a, g, grid):
        return getattr(oracle, oracle_name or name)(*a, *scalars(g, grid))
    return dict(kinds=kinds, outs=tuple(outs), call=call, ref=ref)


def _custom(kinds, outs, call, ref):
    return dict(kinds=kinds, outs=tuple(outs), call=call, ref=ref)


def _ptp(hip, t, g, rule=(0, True, 0.0)):
    return _params(hip, t, g, *rule)


ELEMENTARY = {
    "update_tau": _row("update_tau", ["c", "c", "c", "s", "s", "s", "vx", "vy", "vz"], range(6), lambda g, n: (g["mu"], g["dx"], g["dy"], g["dz"])),
    "predict_V": _row("predict_V", ["vx", "vy", "vz", "c", "c", "c", "s", "s", "s"], range(3),
                      lambda g, n: (g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])),
    "update_divV": _row("update_divV", ["c", "vx", "vy", "vz"], [0], lambda g, n: (g["dx"], g["dy"], g["dz"])),
    "update_dPrdtau": _row("update_dPrdtau", ["c", "i", "c"], [1],
                           lambda g, n: (g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"])),
    "update_Pr": _row("update_Pr", ["c", "i"], [0], lambda g, n: (g["dtau"],)),
    "compute_res": _row("compute_res", ["i", "c", "c"], [0], lambda g, n: (g["rho"], g["dt"], g["dx"], g["dy"], g["dz"])),
    "correct_V": _row("correct_V", ["vx", "vy", "vz", "c"], range(3), lambda g, n: (g["dt"], g["rho"], g["dx"], g["dy"], g["dz"])),
    "max_abs": _row("max_abs", ["c"], [], lambda g, n: ()),
    "copy": _row("copy", ["vx", "vx"], [0], lambda g, n: ()),
    "residual_max": _custom(["c", "c"], [], lambda hip, ctx, t, g, n: hip.residual_max(t[0], t[1], _ptp(hip, t[0], g), ctx=ctx),
                            lambda oracle, a, g, n: _res_max_ref(oracle, a[0], a[1], g)),
    "bc_x": _row("bc_x", ["c"], [0], lambda g, n: ()),
    "bc_y": _row("bc_y", ["vx"], [0], lambda g, n: ()),
    "bc_z": _row("bc_z", ["vy"], [0], lambda g, n: ()),
    "bc_zV": _row("bc_zV", ["vz"], [0], lambda g, n: ()),
    "bc_xhydstatic": _row("bc_xhydstatic", ["c"], [0], lambda g, n: (g["dz"], n[2], g["g"], g["rho"])),
    "bc_x_Vx": _row("bc_x_Vx", ["vx"], [0], lambda g, n: (1.0,)),
    "bc_x_Pr": _row("bc_x_Pr", ["c"], [0], lambda g, n: (0.25,)),
    "set_bc_Pr_multi-outlet": _custom(["c"], [0], lambda hip, ctx, t, g, n: hip.set_bc_Pr_multi(t[0], True, 0.25, ctx=ctx),
                                      lambda oracle, a, g, n: oracle.set_bc_Pr(a[0], 0, True, 0.25)),
    "set_bc_Pr_multi": _custom(["c"], [0], lambda hip, ctx, t, g, n: hip.set_bc_Pr_multi(t[0], False, 0.25, ctx=ctx),
                               lambda oracle, a, g, n: oracle.set_bc_Pr(a[0], 0, False, 0.25)),
    "set_bc_Pr_gpu": _custom(["c"], [0], lambda hip, ctx, t, g, n: hip.set_bc_Pr_gpu(t[0], g["dz"], n[2], g["g"], g["rho"], ctx=ctx),
                             lambda oracle, a, g, n: oracle.set_bc_Pr(a[0], 1, False, 0.0, g["dz"], n[2], g["g"], g["rho"])),
    "set_bc_Vel_multi-inlet": _custom(["vx", "vy", "vz"], range(3), lambda hip, ctx, t, g, n: hip.set_bc_Vel_multi(*t, True, 1.5, ctx=ctx),
                                      lambda oracle, a, g, n: oracle.set_bc_Vel(*a, 0, True, 1.5)),
    "set_bc_Vel_multi": _custom(["vx", "vy", "vz"], range(3), lambda hip, ctx, t, g, n: hip.set_bc_Vel_multi(*t, False, 1.5, ctx=ctx),
                                lambda oracle, a, g, n: oracle.set_bc_Vel(*a, 0, False, 1.5)),
    "set_bc_Vel_gpu": _custom(["vx", "vy", "vz"], range(3), lambda hip, ctx, t, g, n: hip.set_bc_Vel_gpu(*t, ctx=ctx),
                              lambda oracle, a, g, n: oracle.set_bc_Vel(*a, 1)),
}
for _beta in (0.0, 0.3):
    ELEMENTARY["set_cylinder-beta%g" % _beta] = _row("set_cylinder", ["c", "vx", "vy", "vz"], range(4),
                                                     lambda g, n, b=_beta: _cyl_scalars(b, "glob", n))
    ELEMENTARY["set_cylinder_local-beta%g" % _beta] = _row("set_cylinder", ["c", "vx", "vy", "vz"], range(4),
                                                           lambda g, n, b=_beta: _cyl_scalars(b, "loc", n), oracle_name="set_cylinder_local")
BC_SEQUENCES = [k for k in ELEMENTARY if k.startswith("set_bc_")]


def _elementary(hip, oracle, name, dt, mode):
    from navierstokes3d_amd import lib as L
    row = ELEMENTARY[name]
    ctx = hip.Context(0, mode)
    ran = 0
    for grid in EL_GRIDS:
        g = geometry(*grid)
        host = fields(*grid, row["kinds"], 1, NP[dt])
        names = ["%s%d" % (k, q) for q, k in enumerate(row["kinds"])]
        if grid == (3, 3, 3):                         # "where the call allows it": the call on plain arrays decides
            try:
                row["call"](hip, ctx, [hip.from_numpy(a) for a in host], g, grid)
            except L.Ns3dError as e:
                assert "too small" in str(e), e
                continue
        ref, ref_result = None, None
        if mode == "strict":
            copies = [a.copy(order="F") for a in host]
            ref_result = row["ref"](oracle, copies, g, grid)
            ref = {names[q]: copies[q] for q in row["outs"]}
        arrays = [(names[q], a, q in row["outs"]) for q, a in enumerate(host)]
        footprint(hip, arrays, lambda t: row["call"](hip, ctx, [t[n] for n in names], g, grid), (name, grid, dt, mode),
                  ref=ref, ref_result=ref_result if not row["outs"] else None)
        ran += 1
    ctx.close()
    assert ran >= 3


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", [k for k in ELEMENTARY if k not in BC_SEQUENCES])
def test_elementary(hip, oracle, name, dt, mode):
    _elementary(hip, oracle, name, dt, mode)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", BC_SEQUENCES)
def test_bc_sequences(hip, oracle, name, dt, mode, fused, monkeypatch):
    """the whole sequence as one gather launch (k_bc_fused) and rule by rule"""
    monkeypatch.setenv("NS3D_BC_FUSED", fused)
    _elementary(hip, oracle, name, dt, mode)


# ---- 2. predict_fused ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", [(3, 3, 3), (64, 16, 32), (65, 17, 33), (129, 3, 3)], ids=GID)
def test_predict_fused(hip, oracle, grid, dt, mode):
    g = geometry(*grid)
    host = fields(*grid, ["vx", "vy", "vz", "c", "c", "c", "s", "s", "s"], 5, NP[dt])
    ref = None
    if mode == "strict":
        Vx, Vy, Vz, txx, tyy, tzz, txy, txz, tyz = [a.copy(order="F") for a in host]
        oracle.update_tau(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, g["mu"], g["dx"], g["dy"], g["dz"])
        oracle.predict_V(Vx, Vy, Vz, txx, tyy, tzz, txy, txz, tyz, g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])
        ref = {"Vx_new": Vx, "Vy_new": Vy, "Vz_new": Vz}
    arrays = [("V%s_new" % c, np.full_like(a, 777.0), True) for c, a in zip("xyz", host)] + [("V%s" % c, a, False) for c, a in zip("xyz", host)]
    ctx = hip.Context(0, mode)
    footprint(hip, arrays, lambda t: hip.predict_fused(t["Vx_new"], t["Vy_new"], t["Vz_new"], t["Vx"], t["Vy"], t["Vz"], g["mu"], g["rho"],
                                                       g["g"], g["dt"], g["dx"], g["dy"], g["dz"], ctx=ctx), ("predict_fused", grid, dt, mode), ref=ref)
    ctx.close()


# ---- 3. advect and copy_advect, windowed and global gather ------------------------------------------------------------------------------
ADVECT_CASES = [((3, 3, 3), 0.8), ((63, 7, 31), 1.0), ((64, 8, 33), 0.5), ((150, 21, 70), 2.7)]


@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid,cfl", ADVECT_CASES, ids=lambda v: GID(v) if isinstance(v, tuple) else "cfl%g" % v)
def test_advect(hip, oracle, grid, cfl, dt, mode, form, monkeypatch):
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")                  # read per call, as test_copy_advect_* selects it
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    g = geometry(*grid)
    step = cfl * min(g["dx"], g["dy"], g["dz"])
    old = fields(*grid, ["vx", "vy", "vz", "c"], 21, NP[dt])
    new = fields(*grid, ["vx", "vy", "vz", "c"], 31, NP[dt])
    ctx = hip.Context(0, mode)
    for faithful in (True, False):
        ref = None
        if mode == "strict":
            r = [a.copy(order="F") for a in new]
            oracle.advect(r[0], old[0], r[1], old[1], r[2], old[2], r[3], old[3], step, g["dx"], g["dy"], g["dz"], faithful)
            ref = dict(zip(("Vx", "Vy", "Vz", "C"), r))
        arrays = [(n, a, True) for n, a in zip(("Vx", "Vy", "Vz", "C"), new)] + [(n + "_o", a, False) for n, a in zip(("Vx", "Vy", "Vz", "C"), old)]
        footprint(hip, arrays, lambda t: hip.advect(t["Vx"], t["Vx_o"], t["Vy"], t["Vy_o"], t["Vz"], t["Vz_o"], t["C"], t["C_o"], step,
                                                    g["dx"], g["dy"], g["dz"], faithful, ctx=ctx), ("advect", form, grid, cfl, dt, mode, faithful), ref=ref)
        # copy_advect: complete new fields into buffers of their own, pre-filled with garbage
        if mode == "strict":
            r = [a.copy(order="F") for a in old]
            oracle.advect(r[0], old[0], r[1], old[1], r[2], old[2], r[3], old[3], step, g["dx"], g["dy"], g["dz"], faithful)
            ref = dict(zip(("Vx_new", "Vy_new", "Vz_new", "C_new"), r))
        names = ("Vx", "Vy", "Vz", "C")
        arrays = [(n + "_new", np.full_like(a, 777.0), True) for n, a in zip(names, old)] + [(n, a, False) for n, a in zip(names, old)]
        footprint(hip, arrays, lambda t: hip.copy_advect(t["Vx_new"], t["Vx"], t["Vy_new"], t["Vy"], t["Vz_new"], t["Vz"], t["C_new"], t["C"], step,
                                                         g["dx"], g["dy"], g["dz"], faithful, ctx=ctx),
                  ("copy_advect", form, grid, cfl, dt, mode, faithful), ref=ref)
    ctx.close()


# ---- 4. the PT sweeps through their explicit-output entry points ---------------------------------------------------------------------------
PT_GRIDS = [(5, 5, 5), (63, 38, 38), (65, 33, 9), (260, 19, 9), (66, 70, 5)]
PARTIAL_GRID = (63, 38, 38)           # once per family, a partial plane range: pt_sweep on planes [1, 4) with both z planes flagged as halos
                                      # (plane 0 must stay); pt_sweep2 / pt_sweepn, which take no halo flags, on planes [5, 9)


def _pt_host(grid, dt, seed=71):
    Pr0, d0, rhs = fields(*grid, ["c", "i", "c"], seed, NP[dt])
    return Pr0, d0, rhs


def _pt_reference(oracle, Pr0, d0, rhs, g, n, rule, cache):
    """the oracle's iterates 1 … n, computed once per (grid, rule) and shared"""
    if not cache:
        Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
        cache[0] = (Pr0, d0)
        for q in range(1, 6):
            _oracle_iters(oracle, Pr, d, rhs, g, 1, *rule)
            cache[q] = (Pr.copy(order="F"), d.copy(order="F"))
    return cache[n]


def _sweep_cases(family, grid):
    """(rule, z-halo flags, k0, k1): both rules on whole grids, and the partial plane range on its grid"""
    cases = [(rule, False, None, None) for rule in RULES]
    if grid == PARTIAL_GRID:
        cases.append(((0, True, 0.0), True, 1, 4) if family == "sweep" else ((0, True, 0.0), False, 5, 9))
    return cases


def _planes(k0, k1):
    """the parts of partial-range outputs that are compared — with the plain call: Pr planes [k0,k1) and the planes behind k1, which
    stay as they were, dPrdτ likewise, one lower (as _sweepn_all_shapes of test_gpu_pt.py); with the oracle: the computed planes"""
    return ({"Pr_out": lambda a: np.concatenate([a[:, :, k0:k1], a[:, :, k1 + 1:]], axis=2),
             "d_out": lambda a: np.concatenate([a[:, :, k0 - 1:k1 - 1], a[:, :, k1:]], axis=2)},
            {"Pr_out": lambda a: a[:, :, k0:k1], "d_out": lambda a: a[:, :, k0 - 1:k1 - 1]})


def _run_sweeps(hip, oracle, family, grid, dt, mode, shapes, levels, setter):
    """every shape × level of one family on one grid: `levels` PT iterations (Pr_in, d_in) → (Pr_out, d_out) in one call"""
    from navierstokes3d_amd import lib as L
    nx, ny, nz = grid
    g = geometry(*grid)
    Pr0, d0, rhs = _pt_host(grid, dt)
    ctx = hip.Context(0, mode)
    ran = {}
    for rule, halo, k0, k1 in _sweep_cases(family, grid):
        cache = {}
        p = _params(hip, hip.from_numpy(Pr0), g, *rule, halo, halo)
        for nlev in levels:
            for shape in shapes:
                setter(ctx, shape)
                arrays = [("Pr_out", np.full_like(Pr0, 555.0), True), ("Pr_in", Pr0, False), ("d_out", np.full_like(d0, 444.0), True),
                          ("d_in", d0, False), ("rhs", rhs, False)]
                if family == "sweep":
                    arrays = [("Pr_out", np.full_like(Pr0, 555.0), True), ("Pr_in", Pr0, False), ("d_out", d0, True), ("rhs", rhs, False)]
                    call = lambda t: hip.pt_sweep(t["Pr_in"], t["Pr_out"], t["d_out"], t["rhs"], p, k0 or 1, k1 or nz - 1, ctx=ctx)
                elif family == "sweep2":
                    call = lambda t: hip.pt_sweep2(t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], p, k0, k1, ctx=ctx)
                else:
                    call = lambda t: hip.pt_sweepn(nlev, t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], p, k0, k1, ctx=ctx)
                ref = None
                if mode == "strict":
                    Pr, d = _pt_reference(oracle, Pr0, d0, rhs, g, nlev, rule, cache)
                    ref = {"Pr_out": Pr, "d_out": d}
                part, ref_part = _planes(k0, k1) if k0 is not None else (None, None)
                what = (family, grid, dt, mode, "shape %d" % shape, "levels %d" % nlev, rule, "planes %r:%r" % (k0, k1))
                try:
                    _, ar = footprint(hip, arrays, call, what, ref=ref, part=part, ref_part=ref_part)
                except L.Ns3dError as e:          # a tile too small for this many levels, a shape this element type lacks
                    assert "cannot run" in str(e), (what, e)
                    continue
                if halo:                          # the flagged planes of the output are never written
                    got = ar.get("Pr_out")
                    assert (got[:, :, 0] == 555.0).all() and (got[:, :, -1] == 555.0).all(), what
                ran[nlev, rule, k0] = ran.get((nlev, rule, k0), 0) + 1
    ctx.close()
    print("PT %s %s %s %s: shapes that ran per (levels, rule, k0): %r" % (family, GID(grid), dt, mode, ran))
    return ran


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", PT_GRIDS, ids=GID)
def test_pt_sweep(hip, oracle, grid, dt, mode):
    ran = _run_sweeps(hip, oracle, "sweep", grid, dt, mode, VARIANTS, (1,), lambda c, v: c.set_pt_variant(v))
    assert all(v >= 8 for v in ran.values()) and len(ran) >= 2, ran


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", PT_GRIDS, ids=GID)
def test_pt_sweep2(hip, oracle, grid, dt, mode):
    ran = _run_sweeps(hip, oracle, "sweep2", grid, dt, mode, SHAPES2, (2,), lambda c, v: c.set_pt2_variant(v))
    assert all(v >= 8 for v in ran.values()) and len(ran) >= 2, ran


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", PT_GRIDS, ids=GID)
def test_pt_sweepn(hip, oracle, grid, dt, mode):
    levels = (2, 3, 4) if dt == "f64" else (2, 3, 4, 5)
    ran = _run_sweeps(hip, oracle, "sweepn", grid, dt, mode, SHAPESN, levels, lambda c, v: c.set_ptn_variant(v))
    # at least eight shapes per (levels, rule); the fifth level exists on few shapes and not on every grid, so it only adds to the count
    assert all(ran.get((nlev, rule, None), 0) >= 8 for nlev in (2, 3, 4) for rule in RULES), ran


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
def test_plan_pt(hip, oracle, dt, mode):
    """ns3d_plan_pt times about a hundred launches of the two-iteration tile shapes on the caller's own arguments the first time it
    sees a (grid, element type, mode) with 1.5 M cells or more, process-wide; ns3d_pt_sweep2 then runs the winner.  The grid is used
    nowhere else in the suite and the arena's call comes first, so the timed launches are the ones that run between the guards."""
    grid = (191, 99, 83)
    nx, ny, nz = grid
    assert nx * ny * (nz - 2) >= 1500 * 1000
    g = geometry(*grid)
    rule = (0, True, 0.25)
    Pr0, d0, rhs = _pt_host(grid, dt, 101)
    ref = None
    if mode == "strict":
        Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
        _oracle_iters(oracle, Pr, d, rhs, g, 2, *rule)
        ref = {"Pr_out": Pr, "d_out": d}
    ctx = hip.Context(0, mode)
    p = _params(hip, hip.from_numpy(Pr0), g, *rule)
    arrays = [("Pr_out", np.full_like(Pr0, 555.0), True), ("Pr_in", Pr0, False), ("d_out", np.full_like(d0, 444.0), True),
              ("d_in", d0, False), ("rhs", rhs, False)]

    def call(t):
        hip.plan_pt(t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], p, ctx=ctx)
        hip.pt_sweep2(t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], p, ctx=ctx)
        return ctx.last_pt2_variant()

    variant, _ = footprint(hip, arrays, call, ("plan_pt", grid, dt, mode), ref=ref, arena_first=True)
    print("plan_pt %s %s %s: tile variant %d" % (GID(grid), dt, mode, variant))
    ctx.close()


# ---- 5. pt_iterate and pt_solve --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("grid", [(63, 38, 38), (70, 21, 23)], ids=GID)
def test_pt_iterate_and_solve(hip, oracle, grid, persist, dt, mode):
    """Launch by launch, as replayed HIP graphs and as the cooperative k_pt_persist, every pinned depth.  footprint() makes the call on
    plain arrays first and on the arena's arrays next, on the same context: a graph captured for the first pointers must not be
    replayed for the second."""
    nx, ny, nz = grid
    g = geometry(*grid)
    rule = (0, True, 0.25)
    Pr0, d0, rhs = _pt_host(grid, dt, 73)
    rhs = rhs * NP[dt](1e-3)
    n_it, solve = 13, (-1.0, 45, 7)
    ref_it = ref_solve = res_solve = None
    if mode == "strict":
        Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
        _oracle_iters(oracle, Pr, d, rhs, g, n_it, *rule)
        ref_it = {"Pr": Pr, "d": d}
        Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
        Rp = np.zeros((nx - 2, ny - 2, nz - 2), dtype=NP[dt], order="F")
        res_solve = oracle.pt_solve(Pr, d, rhs, Rp, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], *rule, g["g"],
                                    *solve, 0.36, 1000.0)
        ref_solve = {"Pr": Pr, "d": d}
    ctx = hip.Context(0, mode)
    ctx.set_persist_mode(persist)
    p = _params(hip, hip.from_numpy(Pr0), g, *rule)
    arrays = [("Pr", Pr0, True), ("rhs", rhs, False), ("d", d0, True)]
    for graph in (0, 1):
        ctx.set_graph_mode(graph)
        for depth in (1, 2, 3, 4) if dt == "f64" else (1, 2, 3, 4, 5):
            ctx.set_pt_depth(depth)
            what = (grid, dt, mode, "persist %d" % persist, "graph %d" % graph, "depth %d" % depth)
            footprint(hip, arrays, lambda t: hip.pt_iterate(t["Pr"], t["d"], t["rhs"], p, n_it, ctx=ctx), ("pt_iterate",) + what, ref=ref_it)
            footprint(hip, arrays, lambda t: hip.pt_solve(t["Pr"], t["d"], t["rhs"], p, *solve, 0.36, 1000.0, ctx=ctx), ("pt_solve",) + what,
                      ref=ref_solve, ref_result=res_solve)
    assert ctx.persist_faults() == 0
    ctx.close()


# ---- 6. poisson_direct -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rule", RULES, ids=str)
@pytest.mark.parametrize("grid", [(4, 4, 4), (33, 17, 17), (34, 18, 18), (70, 35, 12), (20, 40, 40)], ids=GID)
def test_poisson_direct(hip, oracle, grid, rule, dt, mode):
    """Both GEMM kernels, the fused and the pointwise epilogues, the hipMemsetAsync of dPrdτ.  No per-call oracle form: the bits of the
    call on plain arrays, plus the twin bar of test_gpu_direct.py (1e-11 / 2e-6 relative L2 against oracle/direct_ref.py)."""
    from oracle.direct_ref import poisson_direct
    nx, ny, nz = grid
    g = geometry(*grid)
    dtype = NP[dt]
    rhs = fields(nx, ny, nz, ["c"], 57, dtype)[0]
    twin = poisson_direct(rhs.astype(np.float64), g["rho"], g["dt"], g["dx"], g["dy"], g["dz"], *rule, g["g"])
    Pr0, d0 = fields(nx, ny, nz, ["c"], 3, dtype)[0], fields(nx, ny, nz, ["i"], 4, dtype)[0]
    ctx = hip.Context(0, mode)
    p = hip.pt_params(hip.from_numpy(Pr0), g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], *rule, g["g"])
    arrays = [("Pr", Pr0, True), ("rhs", rhs, False), ("d", d0, True)]
    _, ar = footprint(hip, arrays, lambda t: hip.poisson_direct(t["Pr"], t["d"], t["rhs"], p, ctx=ctx), ("poisson_direct", grid, rule, dt, mode))
    got = ar.get("Pr")
    tol = 1e-11 if dtype == np.float64 else 2e-6
    print("rel-L2 against the twin at %r, rule %r, %s: %.3e (bar %.1e)" % (grid, rule, dt, rel_l2(got, twin), tol))
    assert rel_l2(got, twin) < tol, rel_l2(got, twin)
    assert not ar.get("d").any()
    ctx.close()


# ---- 7. a whole time step ------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = {"Pr": "c", "dPrdtau": "i", "divV": "c", "Vx": "vx", "Vy": "vy", "Vz": "vz", "Vx_o": "vx", "Vy_o": "vy", "Vz_o": "vz", "C": "c",
               "C_o": "c", "txx": "c", "tyy": "c", "tzz": "c", "txy": "s", "txz": "s", "tyz": "s"}


MC_GPU_NITER = 200


def mc_niter(script, advection, p):
    """The iteration limit of the step: the script's own — but 200 for gpu.jl's script with the MacCormack scheme.  Its PT loop
    diverges at 24×15×15; after two steps of 750 iterations |V| is of order 1e267, which STRICT still holds and FAST's rounding puts
    over float64's range (NaN in every field, and a comparison of NaNs could not see a guard's NaN); with 200 it is of order 1e67."""
    return MC_GPU_NITER if (script, advection) == ("gpu", "maccormack") else p.niter


def _two_steps_on(hip, script, dt, mode, in_arena, advection="reference"):
    """_two_steps of test_gpu_invariance.py with the seventeen arrays of ns3d_step_fields on plain tensors or in an arena, in either
    element type and mode: the same initial state, two ns3d_time_step calls, write_stress on the second.  advection="maccormack":
    the knob on and faithful = 0 (the stage-1 fields are the context's own scratch, not part of the arena)"""
    from navierstokes3d_amd import driver as Dr, lib as L
    from navierstokes3d_amd.params import gpu_params, multi_params
    p = multi_params(24) if script == "multi" else gpu_params(24)
    n = (p.nx, p.ny, p.nz)
    assert n == (24, 15, 15)
    host = {k: np.zeros(SHAPES[kind](*n), dtype=NP[dt], order="F") for k, kind in STEP_SHAPES.items()}
    if script == "multi":
        host["Vy"][0, :, :] = p.vin                                                                  # multi.jl:369
    else:
        Vx0, Pr0 = Dr.gpu_initial_fields(p)                                                          # gpu.jl:85-88
        host["Vx"], host["Pr"] = np.asfortranarray(Vx0.astype(NP[dt])), np.asfortranarray(Pr0.astype(NP[dt]))
    ar = AR.Arena([(k, a, True) for k, a in host.items()], "cuda") if in_arena else None
    f = SimpleNamespace(**(ar.t if in_arena else {k: hip.from_numpy(a) for k, a in host.items()}))
    ctx = hip.Context(0, mode, async_=True)
    ctx.set_advection(advection)
    common = dict(nx=p.nx, ny=p.ny, nz=p.nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp, dx=p.dx, dy=p.dy, dz=p.dz,
                  eps=p.eps, niter=mc_niter(script, advection, p), nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc, a2=p.a2, b2=p.b2, ox=p.ox, oy=p.oy,
                  sinb=p.sinb, cosb=p.cosb, lx=p.lx, ly=p.ly, lz=p.lz, faithful=0 if advection == "maccormack" else 1, pressure=0,
                  write_stress=0)
    torch.cuda.synchronize()
    if script == "multi":
        hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz,
                         p.dx, p.dy, p.dz, ctx=ctx)                                                 # multi.jl:372
        sp = L.StepParams(script=L.NS3D_BC_MULTI, xco_g=p.xco_g, yco_g=p.yco_g, zco_g=p.zco_g, owns_inlet=int(bool(p.owns_inlet)),
                          owns_outlet=int(bool(p.owns_outlet)), vin=p.vin, **common)
    else:
        sp = L.StepParams(script=L.NS3D_BC_GPU, xco_g=0.0, yco_g=0.0, zco_g=0.0, owns_inlet=0, owns_outlet=0, vin=0.0, **common)
    torch.cuda.synchronize()
    out = []
    for step in (1, 2):
        sp.write_stress = 1 if step == 2 else 0
        out.append(hip.time_step(f, sp, ctx=ctx))
    torch.cuda.synchronize()
    got = SimpleNamespace(steps=out, fields={k: hip.to_numpy(getattr(f, k)) for k in STEP_SHAPES})
    ctx.close()
    if in_arena:
        ar.assert_clean("time_step %s %s %s %s" % (script, dt, mode, advection))
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step(hip, oracle, script, mode, dt="f64", advection="reference"):
    """All seventeen arrays of ns3d_step_fields in the arena: guards intact, and the iteration counts, residual histories and every
    array equal the run on plain arrays — which in STRICT is _two_steps of test_gpu_invariance.py itself.  float64 only: in float32
    both scripts leave the finite range within two steps at 24×15×15 — in the oracle's arithmetic as well (run_navierstokes3D_ref and
    runme_ref with nx=24, dtype=float32 return NaN in all five fields) — and a comparison of NaNs could not see a guard's NaN.
    With the MacCormack scheme (faithful = 0) the STRICT run also equals the oracle driver's two steps with advection="maccormack"
    (tests/test_advect_mc_host.py::ref_run), all seventeen arrays, iteration counts and residual histories."""
    got = _two_steps_on(hip, script, dt, mode, True, advection)
    want = _two_steps_on(hip, script, dt, mode, False, advection)
    assert all(it > 0 and len(errs) > 0 for it, errs in want.steps)
    assert np.abs(want.fields["Vx"]).max() > 0 and np.abs(want.fields["Pr"]).max() > 0 and np.abs(want.fields["txx"]).max() > 0
    assert all(np.isfinite(a).all() for a in want.fields.values())
    wants = [want]
    if (dt, mode) == ("f64", "strict"):
        from test_gpu_invariance import _two_steps
        wants.append(_two_steps(hip, script, 0, advection))
        if advection == "maccormack":
            from test_advect_mc_host import ref_run
            _, info, f = ref_run(script, 2, "maccormack", niter_cap=MC_GPU_NITER if script == "gpu" else None)
            wants.append(SimpleNamespace(steps=[(it, list(e)) for it, e in zip(info.iters, info.errs)], fields={k: f[k] for k in STEP_SHAPES}))
    for w in wants:
        assert _same_result(got.steps, w.steps), (got.steps, w.steps)
        for k, a in w.fields.items():
            assert _exact(got.fields[k], a), (script, dt, mode, k, first_bit_difference(got.fields[k], a))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_maccormack(hip, oracle, script, mode):
    """test_time_step over the other value of its `advection` parameter (a test of its own: the existing cases keep their names)"""
    test_time_step(hip, oracle, script, mode, advection="maccormack")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_obstacle(hip, oracle, script, mode):
    """The step with ns3d_set_obstacle: the seventeen arrays AND the mask (uint8, on an odd byte) in the arena, from the scenario of
    tests/solid_step_cases.py — a state in which every mask bit acts — with the body that meets five outer planes; multi.jl's
    ns3d_set_solid before the loop reads the arena's mask as well.  Guards intact, the mask unchanged, every array and the iteration
    record equal to the run on plain arrays, and in STRICT to the oracle driver with obstacle= (a test of its own: the existing cases
    keep their names).  float64."""
    import solid_step_cases as SS
    from test_gpu_solid_step import assert_equals_the_oracle, assert_same_run, steps_on
    ctx = hip.Context(0, mode, async_=True)
    got = steps_on(hip, script, "f64", ctx, SS.body_mask(), in_arena=True)
    want = steps_on(hip, script, "f64", ctx, SS.body_mask())
    ctx.close()
    assert got.arena["mask"].data_ptr() % 2 == 1
    assert all(np.isfinite(a).all() for a in want.fields.values()) and np.abs(want.fields["txx"]).max() > 0
    assert_same_run(got, want, (script, mode))
    if mode == "strict":
        assert_equals_the_oracle(got, script, "f64", "reference")


# ---- 8. derived fields ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["multi", "gpu"])
def test_diagnostics(hip, form, dt, mode):
    """read-only: the record has the bits of the run on plain arrays (test_gpu_diagnostics.py holds those to NumPy), cylinder term on"""
    from test_gpu_diagnostics import _cyl
    ctx = hip.Context(0, mode)
    for n in [(17, 9, 5), (70, 35, 8), (131, 11, 35)]:
        g = geometry(*n)
        F = dict(zip(("Vx", "Vy", "Vz", "Pr", "C"), fields(*n, ["vx", "vy", "vz", "c", "c"], 11, NP[dt])))
        dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=_cyl(form, n[0], n[1], g))
        rec, _ = footprint(hip, [(k, a, False) for k, a in F.items()],
                           lambda t: hip.diagnostics(t["Vx"], t["Vy"], t["Vz"], t["Pr"], t["C"], dp, ctx=ctx), ("diagnostics", n, form, dt, mode))
        assert rec.nonfinite == 0 and min(rec.n_masked) > 0 and rec.vmax[0] == float(np.abs(F["Vx"]).max())
        assert all(math.isfinite(v) for v in (rec.div_max, rec.pr_min, rec.pr_max, rec.ke, rec.c_vol) + rec.mom), rec
    ctx.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(3, 3, 3), (65, 5, 3), (70, 35, 8)], ids=GID)
def test_stats(hip, n, dt, mode):
    """stats_reset, three stats_accumulate and stats_finalize on S, mean and rs in the arena (contiguous blocks), the samples' fields too"""
    import test_gpu_stats as TS
    samples, S_ref, _ = TS.case(n, dt)
    cells = n[0] * n[1] * n[2]
    arrays = [("S", np.full(11 * cells, 777.0), True), ("mean", np.full(4 * cells, 777.0), True), ("rs", np.full(7 * cells, 777.0), True)]
    for q, F in enumerate(samples):
        arrays += [("%s%d" % (k, q), a, False) for k, a in zip(("Vx", "Vy", "Vz", "Pr"), F)]
    ctx = hip.Context(0, mode)

    def call(t):
        hip.stats_reset(t["S"], n, ctx=ctx)
        for q, wgt in enumerate(TS.WEIGHTS):
            hip.stats_accumulate(t["S"], t["Vx%d" % q], t["Vy%d" % q], t["Vz%d" % q], t["Pr%d" % q], wgt, ctx=ctx)
        hip.stats_finalize(t["S"], TS.WSUM, t["mean"], t["rs"], n, ctx=ctx)

    ref = None
    if mode == "strict":
        m_ref, r_ref = TS.finalize_ref(S_ref, TS.WSUM)
        flat = lambda blocks: np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, order="F") for b in blocks])
        ref = {"S": flat(S_ref), "mean": flat(m_ref), "rs": flat(r_ref)}
    footprint(hip, arrays, call, ("stats", n, dt, mode), ref=ref)
    ctx.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(3, 3, 3), (17, 9, 5), (66, 6, 18), (131, 11, 35)], ids=GID)
def test_vortex(hip, n, dt, mode):
    """inputs guarded as well as outputs: test_gpu_vortex.py::test_footprint_and_boundary_zeros guards the outputs only"""
    g = geometry(*n)
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=NP[dt])
    d = (g["dx"], g["dy"], g["dz"])
    arrays = [(nm, np.full(n, 777.0, dtype=NP[dt]), True) for nm in VR.NAMES] + [(k, a, False) for k, a in zip(("Vx", "Vy", "Vz"), V)]
    ctx = hip.Context(0, mode)
    ref = VR.reference(*V, *d) if mode == "strict" else None
    _, ar = footprint(hip, arrays, lambda t: hip.vortex(t["Vx"], t["Vy"], t["Vz"], *d, ctx=ctx, **{nm: t[nm] for nm in VR.NAMES}),
                      ("vortex", n, dt, mode), ref=ref)
    mask = np.ones(n, dtype=bool)
    mask[VR.I] = False
    for nm in VR.NAMES:
        assert not _words(ar.get(nm))[mask].any(), nm                     # every boundary entry is +0.0
    ctx.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [1, 255, 257])
def test_sample_and_tracers_advance(hip, N, dt, mode):
    """the (3, N) positions, the N-byte state (at an odd byte), U, the samples and the fields, all in the arena"""
    import test_gpu_tracers as TT
    ctx = hip.Context(0, mode)
    for n in [(17, 9, 5), (66, 5, 4)]:
        X, state = TT.points(n, N)
        V = TT.velocity_fields(n, dt)
        for A, (kind, stag) in zip(V + (fields(*n, ("c",), seed0=9, dtype=NP[dt])[0],), TT.LAYOUTS[1:] + TT.LAYOUTS[:1]):
            for st in (None, state):
                arrays = [("out", np.full(N, 777.0), True), ("X", X, False), ("A", A, False)] + ([("state", st, False)] if st is not None else [])
                footprint(hip, arrays, lambda t: hip.sample(t["A"], t["X"], t["out"], state=t.get("state"), stagger=stag, ctx=ctx),
                          ("sample", n, N, kind, st is not None, dt, mode), ref={"out": TR.sample(A, X, st, stag)})
        for c in (TT.SMALL, TT.LARGE):
            Xn, sn, U = TR.advance(X, state, *V, c)
            for with_u in (True, False):
                arrays = [("X", X, True), ("Vx", V[0], False), ("state", state, True), ("Vy", V[1], False), ("Vz", V[2], False)]
                arrays += [("U", np.full((3, N), 777.0), True)] if with_u else []
                footprint(hip, arrays, lambda t: hip.tracers_advance(t["X"], t["state"], t["Vx"], t["Vy"], t["Vz"], *c, U=t.get("U"), ctx=ctx),
                          ("tracers_advance", n, N, c, with_u, dt, mode), ref={"X": Xn, "state": sn, "U": U})
    ctx.close()


@functools.lru_cache(maxsize=None)
def _iso_case(n, dt):
    """A, B, iso and the reference's triangles: computed once, shared, never modified"""
    A, iso = rnd(11, n, NP[dt]), 0.1
    B = rnd(21, n, NP[dt])
    tri, val = IR.reference(A, iso, B, None, None)
    return A, B, iso, tri, val


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [(65, 5, 3), (130, 9, 17), (2, 33, 33)], ids=GID)
def test_isosurface(hip, n, dt, mode):
    """A and B in the arena, tri and val as well (exactly 9·cap and 3·cap elements: the guard is what lies behind the capacity); cap
    below, at and above the count, and the count-only form"""
    A, B, iso, tri, val = _iso_case(n, dt)
    nref = tri.shape[0]
    assert nref > 8
    ctx = hip.Context(0, mode)
    footprint(hip, [("A", A, False), ("B", B, False)], lambda t: hip.isosurface(t["A"], iso, color=t["B"], ctx=ctx), ("isosurface count", n, dt, mode),
              ref_result=nref)
    for cap in (nref - 1, nref, nref + 7):
        m = min(cap, nref)
        ref = {"tri": np.concatenate([tri[:m].reshape(-1), np.full(9 * (cap - m), 777.0)]),
               "val": np.concatenate([val[:m].reshape(-1), np.full(3 * (cap - m), 777.0)])}
        arrays = [("tri", np.full(9 * cap, 777.0), True), ("A", A, False), ("val", np.full(3 * cap, 777.0), True), ("B", B, False)]
        footprint(hip, arrays, lambda t: hip.isosurface(t["A"], iso, color=t["B"], tri=t["tri"], val=t["val"], cap=cap, ctx=ctx),
                  ("isosurface", n, dt, mode, "cap %d of %d" % (cap, nref)), ref=ref, ref_result=nref)
    ctx.close()
