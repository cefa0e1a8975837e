"""ns3d_diagnostics (the fused on-device flow monitor) against NumPy on the same inputs: maxima bit for bit, sums against
math.fsum within (L+8)·2⁻⁵³·Σ|term| with L = navierstokes3d_amd.diag.path_length (the additions on the longest path of the
reduction as built: kz + 9 in the field pass, ⌈workgroups/256⌉ + 9 over the partials — 128 at 512³, never above 4096), ownership
on virtual ranks of every topology, the drivers' records, and the error paths."""
import math

import numpy as np
import pytest

from navierstokes3d_amd import diag as D
from util import fields, geometry

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
STAG = {"Vx": (1, 0, 0), "Vy": (0, 1, 0), "Vz": (0, 0, 1), "Pr": (0, 0, 0), "C": (0, 0, 0)}
GRIDS = [(17, 9, 5), (24, 15, 15), (70, 35, 8), (131, 66, 37)]


def _cyl(form, nx, ny, g, lx=1.0, ly=0.6, xco=None, yco=None):
    """set_cylinder!'s scalars after the four arrays: an ellipse of half-axes 0.17 / 0.11 turned by 0.3 rad"""
    head = (0.17 ** 2, 0.11 ** 2, -0.1, 0.05, math.sin(0.3), math.cos(0.3))
    tail = (lx, ly, 0.7, g["dx"], g["dy"], g["dz"])
    if form == "multi":
        return head + (-(lx - g["dx"]) / 2 if xco is None else xco, -(ly - g["dy"]) / 2 if yco is None else yco, 0.0) + tail
    return head + tail if form == "gpu" else None


def _masks(hip, ctx, n, cyl, dtype):
    """the entries a real set_cylinder! call zeroes on fields of ones"""
    nx, ny, nz = n
    ones = [hip.from_numpy(np.ones(s, dtype=dtype, order="F")) for s in ((nx, ny, nz), (nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))]
    hip.set_cylinder(*ones, *cyl, ctx=ctx)
    return [hip.to_numpy(t) == 0 for t in ones[1:]]


def _reference(hip, ctx, F, n, g, seam_lo, seam_hi, masks):
    """NumPy / math.fsum on the host arrays F (dict of the five fields), the ownership rule from navierstokes3d_amd.diag;
    returns (record, Σ|term| per sum).  div_max: the STRICT value from ns3d_update_divV's interior."""
    own = {k: D.owned_slices(n, STAG[k], seam_lo, seam_hi) for k in STAG}
    f64 = {k: None if v is None else v.astype(np.float64) for k, v in F.items()}
    r, mag = {}, {}
    r["vmax"] = tuple(float(np.max(np.abs(F[k][own[k]]))) for k in ("Vx", "Vy", "Vz"))
    if F["Pr"] is not None:
        r["pr_min"], r["pr_max"] = float(np.min(F["Pr"][own["Pr"]])), float(np.max(F["Pr"][own["Pr"]]))
    u = 0.5 * (f64["Vx"][:-1] + f64["Vx"][1:]); v = 0.5 * (f64["Vy"][:, :-1] + f64["Vy"][:, 1:]); w = 0.5 * (f64["Vz"][:, :, :-1] + f64["Vz"][:, :, 1:])
    terms = ((u * u + v * v) + w * w)[own["C"]].ravel()
    dV = g["dx"] * g["dy"] * g["dz"]
    kk = 0.5 * g["rho"] * dV
    r["ke"], mag["ke"] = math.fsum(terms) * kk, math.fsum(np.abs(terms)) * kk
    if F["C"] is not None:
        t = f64["C"][own["C"]].ravel()
        r["c_vol"], mag["c_vol"] = math.fsum(t) * dV, math.fsum(np.abs(t)) * dV
    r["mom"], r["n_masked"], mag["mom"] = (0.0,) * 3, (0,) * 3, (0.0,) * 3
    if masks is not None:
        sel = [f64[k][own[k]][m[own[k]]] for k, m in zip(("Vx", "Vy", "Vz"), masks)]
        r["mom"] = tuple(math.fsum(s) for s in sel)
        mag["mom"] = tuple(math.fsum(np.abs(s)) for s in sel)
        r["n_masked"] = tuple(int(s.size) for s in sel)
    dv = hip.from_numpy(np.zeros(n, dtype=F["Vx"].dtype, order="F"))
    hip.update_divV(dv, hip.from_numpy(F["Vx"]), hip.from_numpy(F["Vy"]), hip.from_numpy(F["Vz"]), g["dx"], g["dy"], g["dz"], ctx=ctx)
    r["div_max"] = float(np.max(np.abs(hip.to_numpy(dv)[1:-1, 1:-1, 1:-1])))
    r["nonfinite"] = int(any(v is not None and not np.isfinite(v[own[k]]).all() for k, v in F.items()))
    return r, mag


def _same(a, b):
    return np.array_equal(np.float64(a), np.float64(b), equal_nan=True)


def _check_sums(got, ref, mag, L, what=""):
    for k in ("ke", "c_vol"):
        if k in ref:
            tol = (L + 8) * U53 * mag[k]
            print("%s %s: got %.17g ref %.17g |diff| %.3e tol %.3e" % (what, k, getattr(got, k), ref[k], abs(getattr(got, k) - ref[k]), tol))
            assert abs(getattr(got, k) - ref[k]) <= tol, (what, k)
    for q in range(3):
        tol = (L + 8) * U53 * mag["mom"][q]
        print("%s mom[%d]: got %.17g ref %.17g tol %.3e" % (what, q, got.mom[q], ref["mom"][q], tol))
        assert abs(got.mom[q] - ref["mom"][q]) <= tol, (what, "mom", q)


def _upload(hip, F):
    return [None if F[k] is None else hip.from_numpy(F[k]) for k in ("Vx", "Vy", "Vz", "Pr", "C")]


def _host_fields(n, dtype, seed=11):
    return dict(zip(("Vx", "Vy", "Vz", "Pr", "C"), fields(*n, ["vx", "vy", "vz", "c", "c"], seed, dtype)))


@pytest.mark.parametrize("form", [None, "multi", "gpu"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", GRIDS)
def test_one_rank_against_numpy(hip, n, dtype, form):
    """STRICT: every maximum, pr_min / pr_max, div_max and n_masked bit for bit, the sums within the tolerance, a second call
    the same bits.  FAST: the same, div_max within 16·u·vmax·(1/dx+1/dy+1/dz) of STRICT."""
    g = geometry(*n)
    F = _host_fields(n, dtype)
    cyl = _cyl(form, n[0], n[1], g)
    L = D.path_length(*n)
    assert L <= 4096
    strict, fast = hip.Context(0, "strict"), hip.Context(0, "fast")
    dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=cyl)
    dev = _upload(hip, F)
    div_strict = None
    for ctx in (strict, fast):
        masks = _masks(hip, ctx, n, cyl, dtype) if cyl else None
        ref, mag = _reference(hip, strict, F, n, g, (0, 0, 0), (0, 0, 0), masks)
        got = hip.diagnostics(*dev, dp, ctx=ctx)
        assert got.vmax == ref["vmax"] and got.pr_min == ref["pr_min"] and got.pr_max == ref["pr_max"], ctx.mode
        assert got.n_masked == ref["n_masked"] and got.nonfinite == 0, ctx.mode
        if cyl:
            assert min(got.n_masked) > 0
        if ctx is strict:
            assert got.div_max == ref["div_max"]
        else:
            u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
            bound = 16 * u * max(ref["vmax"]) * (1 / g["dx"] + 1 / g["dy"] + 1 / g["dz"])
            print("FAST div_max %.17g STRICT %.17g bound %.3e" % (got.div_max, ref["div_max"], bound))
            assert abs(got.div_max - ref["div_max"]) <= bound
        _check_sums(got, ref, mag, L, ctx.mode)
        again = hip.diagnostics(*dev, dp, ctx=ctx)
        assert all(_same(getattr(got, k), getattr(again, k)) for k in vars(got)), "a repeated call changed bits"
    strict.close(); fast.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seams", [((1, 0, 1), (0, 1, 1)), ((1, 1, 1), (1, 1, 1)), ((0, 1, 0), (1, 0, 0))])
def test_seam_flags_select_the_owned_entries(hip, seams, dtype):
    n = (70, 35, 8)
    g = geometry(*n)
    F = _host_fields(n, dtype, 23)
    cyl = _cyl("multi", n[0], n[1], g)
    ctx = hip.Context(0, "strict")
    dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], seams[0], seams[1], cylinder=cyl)
    ref, mag = _reference(hip, ctx, F, n, g, seams[0], seams[1], _masks(hip, ctx, n, cyl, dtype))
    got = hip.diagnostics(*_upload(hip, F), dp, ctx=ctx)
    assert got.vmax == ref["vmax"] and (got.pr_min, got.pr_max, got.div_max) == (ref["pr_min"], ref["pr_max"], ref["div_max"])
    assert got.n_masked == ref["n_masked"]
    _check_sums(got, ref, mag, D.path_length(*n))
    ctx.close()


def test_optional_arrays_come_back_nan(hip):
    n = (24, 15, 15)
    g = geometry(*n)
    F = _host_fields(n, np.float64)
    ctx = hip.Context(0, "strict")
    dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"])
    dev = _upload(hip, F)
    full = hip.diagnostics(*dev, dp, ctx=ctx)
    bare = hip.diagnostics(dev[0], dev[1], dev[2], None, None, dp, ctx=ctx)
    assert math.isnan(bare.pr_min) and math.isnan(bare.pr_max) and math.isnan(bare.c_vol) and bare.nonfinite == 0
    assert (bare.vmax, bare.div_max, bare.ke) == (full.vmax, full.div_max, full.ke)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_planted_non_finite_values(hip, bad, dtype):
    """An owned NaN / Inf sets `nonfinite` and reaches that array's maxima; one in an entry the seam flags exclude (the halo
    entry on the high side, the first entry on the low side) is not reported: the record is the clean one, bit for bit."""
    n = (24, 15, 15)
    g = geometry(*n)
    ctx = hip.Context(0, "strict")
    ones = (1, 1, 1)
    dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], ones, ones)
    clean_F = _host_fields(n, dtype, 5)
    clean = hip.diagnostics(*_upload(hip, clean_F), dp, ctx=ctx)
    assert clean.nonfinite == 0
    for q, k in enumerate(("Vx", "Vy", "Vz", "Pr", "C")):
        F = {a: b.copy(order="F") for a, b in clean_F.items()}
        F[k][7, 6, 5] = bad                                          # owned whatever the stagger
        got = hip.diagnostics(*_upload(hip, F), dp, ctx=ctx)
        assert got.nonfinite == 1, k
        hit = {"Vx": [got.vmax[0]], "Vy": [got.vmax[1]], "Vz": [got.vmax[2]], "Pr": [got.pr_min, got.pr_max] if bad != bad else
               [got.pr_max], "C": [got.c_vol]}[k]
        assert all(_same(h, bad) for h in hit), (k, hit)
        others = [got.vmax[j] for j in range(3) if j != q]
        assert np.isfinite(others).all(), k
        for d in range(3):
            for idx in (0, F[k].shape[d] - 1):                       # the excluded ends of dimension d
                F = {a: b.copy(order="F") for a, b in clean_F.items()}
                at = [3, 4, 5]
                at[d] = idx
                F[k][tuple(at)] = bad
                got = hip.diagnostics(*_upload(hip, F), dp, ctx=ctx)
                assert all(_same(getattr(got, f), getattr(clean, f)) for f in vars(clean)), (k, d, idx)
    ctx.close()


TOPOLOGIES = [(1, 1, 2), (1, 1, 3), (1, 1, 4), (2, 1, 1), (1, 2, 1), (2, 2, 1), (2, 2, 2)]


def _global_problem(dims, n, dtype, seed=77):
    """global arrays on power-of-two spacings (cell coordinates are then exact, so that a rank's cylinder test at its own
    xco_g + i·dx is the global one at the same cell bit for bit), the ranks' cuts and their set_cylinder! scalars"""
    ng = tuple(dims[d] * (n[d] - 2) + 2 for d in range(3))
    g = dict(dx=1.0 / 64, dy=1.0 / 32, dz=1.0 / 16, rho=1000.0)
    lx, ly = ng[0] * g["dx"], ng[1] * g["dy"]
    G = _host_fields(ng, dtype, seed)
    xco, yco = -(lx - g["dx"]) / 2, -(ly - g["dy"]) / 2
    scale = min(lx, ly)
    def cyl_at(cx, cy):
        return (((0.3 * scale) ** 2, (0.2 * scale) ** 2, 0.03, -0.02, math.sin(0.3), math.cos(0.3),
                 xco + cx * (n[0] - 2) * g["dx"], yco + cy * (n[1] - 2) * g["dy"], 0.0, lx, ly, 1.0, g["dx"], g["dy"], g["dz"]))
    return ng, g, G, cyl_at


def _cut(G, c, n):
    out = {}
    for k, A in G.items():
        sl = tuple(slice(c[d] * (n[d] - 2), c[d] * (n[d] - 2) + n[d] + STAG[k][d]) for d in range(3))
        out[k] = np.asfortranarray(A[sl])
    return out


def _check_global(hip, ctx, glob, locs, ng, n, g, G, cyl_at, dtype, P):
    one = hip.diagnostics(*_upload(hip, G), hip.diag_params(*ng, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=cyl_at(0, 0)), ctx=ctx)
    ref, mag = _reference(hip, ctx, G, ng, g, (0, 0, 0), (0, 0, 0), _masks(hip, ctx, ng, cyl_at(0, 0), dtype))
    assert one.n_masked == ref["n_masked"] and min(one.n_masked) > 0
    for k in ("vmax", "div_max", "pr_min", "pr_max", "n_masked", "nonfinite"):
        assert getattr(glob, k) == getattr(one, k), k
    _check_sums(glob, ref, mag, max(D.path_length(*n), D.path_length(*ng)), "P=%d" % P)
    if locs is not None:                                             # the local sums add up to the global ones in rank order
        for k in ("ke", "c_vol"):
            s = getattr(locs[0], k)
            for r in locs[1:]:
                s += getattr(r, k)
            assert s == getattr(glob, k), k
        for q in range(3):
            s = locs[0].mom[q]
            for r in locs[1:]:
                s += r.mom[q]
            assert s == glob.mom[q] and sum(r.n_masked[q] for r in locs) == glob.n_masked[q]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dims", TOPOLOGIES)
def test_virtual_ranks_count_the_global_arrays_once(hip, dims, dtype):
    import torch
    from navierstokes3d_amd.mgpu import MultiGpu
    from oracle.driver_ref import cart_coords
    n = (20, 13, 9)
    P = dims[0] * dims[1] * dims[2]
    ng, g, G, cyl_at = _global_problem(dims, n, dtype)
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * P, *n, "strict", dims=dims)
    coords = [cart_coords(r, dims) for r in range(P)]
    assert [tuple(c) for c in coords] == [tuple(c) for c in mg.coords]
    cuts = [_cut(G, c, n) for c in coords]
    dev = [[hip.from_numpy(cu[k]) for cu in cuts] for k in ("Vx", "Vy", "Vz", "Pr", "C")]
    dps = [hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=cyl_at(c[0], c[1])) for c in coords]
    glob, locs = mg.diagnostics(*dev, dps)
    ctx = hip.Context(0, "strict")
    _check_global(hip, ctx, glob, locs, ng, n, g, G, cyl_at, dtype, P)
    for r, c in enumerate(coords):                                   # a rank's record is the one-rank call with its seam flags
        lo, hi = D.seam_flags(dims, c)
        dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], lo, hi, cylinder=cyl_at(c[0], c[1]))
        own = hip.diagnostics(*[d[r] for d in dev], dp, ctx=ctx)
        assert all(_same(getattr(own, f), getattr(locs[r], f)) for f in vars(own)), r
    # a NaN in a halo entry no rank owns is not reported; an owned one is, by the maxima as ns3d_max_g combines them
    if P > 1:
        d = [q for q in range(3) if dims[q] > 1][0]
        at = [3, 4, 2]; at[d] = 0
        dev[0][P - 1][tuple(at)] = float("nan")                      # Vx of the last rank, whose low side in d is a seam
        assert [tuple(mg.coords[P - 1])[d] > 0, mg.diagnostics(*dev, dps)[0].nonfinite] == [True, 0]
        dev[0][P - 1][5, 5, 4] = float("nan")
        again = mg.diagnostics(*dev, dps)[0]
        assert again.nonfinite == 1 and math.isnan(again.vmax[0]) and again.vmax[1] == glob.vmax[1]
    ctx.close()
    mg.close()


REDUCTION_GRIDS = [((3, 255, 63), 8, 512), ((3, 1023, 127), 16, 2048), ((3, 2047, 127), 32, 2048)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,kz,partials", REDUCTION_GRIDS, ids=["%dx%dx%d" % n for n, _, _ in REDUCTION_GRIDS])
def test_more_than_256_partials_and_every_chunk_depth(hip, n, kz, partials, dtype):
    """k_diag_final's thread t combines the partials t, t + 256, …: GRIDS leaves at most 255 (131×66×37), so the second trip of that
    loop never ran, and ns3d_diag_geometry returned kz = 8 only.  Thin grids of under 0.8 M cells with 512 and 2 048 partials and kz =
    8, 16, 32 — asserted from the formula restated here —, against _reference with the file's bound, seams none and all."""
    nx, ny, nz = n
    gx, gy = (nx + 1 + 63) // 64, (ny + 1 + 3) // 4                  # ns3d_diag_geometry (csrc/ns3d_launch.h)
    z = 32
    while z > 8 and gx * gy * ((nz + 1 + z - 1) // z) < 2048:
        z //= 2
    assert (z, gx * gy * ((nz + 1 + z - 1) // z)) == (kz, partials) and D.launch_geometry(*n) == (partials, kz)
    assert partials > 256 and nx * ny * nz < 800000
    g = geometry(*n)
    F = _host_fields(n, dtype, 31)
    cyl = _cyl("multi", n[0], n[1], g)
    L = D.path_length(*n)
    assert L == kz + 9 + partials // 256 + 9
    ctx = hip.Context(0, "strict")
    masks = _masks(hip, ctx, n, cyl, dtype)
    dev = _upload(hip, F)
    for lo, hi in (((0, 0, 0), (0, 0, 0)), ((1, 1, 1), (1, 1, 1))):
        dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], lo, hi, cylinder=cyl)
        ref, mag = _reference(hip, ctx, F, n, g, lo, hi, masks)
        got = hip.diagnostics(*dev, dp, ctx=ctx)
        assert got.vmax == ref["vmax"] and (got.pr_min, got.pr_max, got.div_max) == (ref["pr_min"], ref["pr_max"], ref["div_max"])
        assert got.n_masked == ref["n_masked"] and got.nonfinite == 0
        if lo == (0, 0, 0):
            assert sum(got.n_masked) > 0
        _check_sums(got, ref, mag, L, "%r seams %r" % (n, lo))
        again = hip.diagnostics(*dev, dp, ctx=ctx)
        assert all(_same(getattr(got, k), getattr(again, k)) for k in vars(got)), "a repeated call changed bits"
    ctx.close()


# ---- drivers -----------------------------------------------------------------------------------------------------------
def _same_run(a, b):
    from util import errs_identical
    fa, fb = a[-1].fields, b[-1].fields
    for k in ("C", "Pr", "Vx", "Vy", "Vz", "divV", "dPrdtau"):
        assert np.array_equal(_np(getattr(fa, k)), _np(getattr(fb, k)), equal_nan=True), k
    assert a[-1].iters == b[-1].iters and errs_identical(a[-1].errs, b[-1].errs)


def _np(t):
    from navierstokes3d_amd import kernels as K
    return K.to_numpy(t)


def test_run_navierstokes3D_is_unchanged_by_diagnostics(hip, capsys):
    from navierstokes3d_amd.driver import run_navierstokes3D
    off = run_navierstokes3D(nx=24, nt=3, mode="strict", return_info=True)
    on = run_navierstokes3D(nx=24, nt=3, mode="strict", return_info=True, diagnostics=True, do_print=True)
    for a, b in zip(off[:5], on[:5]):
        assert np.array_equal(a, b, equal_nan=True)
    _same_run(off, on)
    assert len(on[-1].diag) == 3 and not hasattr(off[-1], "diag")
    p = on[-1].params
    for rec in on[-1].diag:
        assert rec.nonfinite == 0 and min(rec.n_masked) > 0 and rec.ke > 0
        assert rec.courant == tuple(p.dt * rec.vmax[q] / (p.dx, p.dy, p.dz)[q] for q in range(3))
    lines = capsys.readouterr().out.splitlines()
    assert sum(ln.startswith("  diag:") for ln in lines) == 3 and lines[0] == "#it = 1"


def test_runme_is_unchanged_by_diagnostics(hip):
    from navierstokes3d_amd.driver import runme
    f0, i0 = runme(nx=40, nt=2, mode="strict")
    f1, i1 = runme(nx=40, nt=2, mode="strict", diagnostics=True)
    for k in ("C", "Pr", "Vx", "Vy", "Vz", "divV", "dPrdtau"):
        assert np.array_equal(_np(getattr(f0, k)), _np(getattr(f1, k)), equal_nan=True), k
    from util import errs_identical
    assert i0.iters == i1.iters and errs_identical(i0.errs, i1.errs) and len(i1.diag) == 2
    assert all(min(r.n_masked) > 0 and r.nonfinite == 0 for r in i1.diag)


@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_force_is_the_momentum_the_two_set_cylinder_calls_remove(hip, script, monkeypatch):
    """info.diag[k].force against the host: the fields are captured where the unfused call-by-call step (fused=False) reaches
    its set_cylinder! calls, the mask is what a real call zeroes on fields of ones, the sums are math.fsum."""
    from navierstokes3d_amd import driver, kernels as K
    captured, real = [], K.set_cylinder

    def spy(Cf, Vx, Vy, Vz, *rest, ctx=None):
        captured.append(([K.to_numpy(t) for t in (Vx, Vy, Vz)], rest))
        real(Cf, Vx, Vy, Vz, *rest, ctx=ctx)
    monkeypatch.setattr(K, "set_cylinder", spy)
    nt = 2
    if script == "multi":
        info = driver.run_navierstokes3D(nx=24, nt=nt, mode="strict", fused=False, return_info=True, diagnostics=True)[-1]
        calls = captured[1:]                                         # the first call is the initialisation multi.jl:372
    else:
        info = driver.runme(nx=40, nt=nt, mode="strict", fused=False, diagnostics=True)[1]
        calls = captured
    monkeypatch.undo()
    assert len(calls) == 2 * nt
    p = info.params
    n = (p.nx, p.ny, p.nz)
    ctx = hip.Context(0, "strict")
    masks = _masks(hip, ctx, n, calls[0][1], np.float64)
    L = D.path_length(*n)
    for k in range(nt):
        sums, mags = [0.0] * 3, [0.0] * 3
        for V3, _ in calls[2 * k:2 * k + 2]:
            for q in range(3):
                sums[q] += math.fsum(V3[q][masks[q]]); mags[q] += math.fsum(np.abs(V3[q][masks[q]]))
        scale = p.rho * p.dx * p.dy * p.dz / p.dt
        rec = info.diag[k]
        assert rec.n_masked == tuple(int(m.sum()) for m in masks)
        for q in range(3):
            tol = (L + 8 + 4) * U53 * mags[q] * scale                # each monitor call within (L+8)·u of its own Σ|term|; + their sum and the scaling
            print("step %d force[%d] = %.17g host %.17g tol %.3e" % (k + 1, q, rec.force[q], sums[q] * scale, tol))
            assert abs(rec.force[q] - sums[q] * scale) <= tol
    assert all(any(abs(f) > 0 for f in rec.force) for rec in info.diag)      # (multi.jl's Vx is zero until :474 sets the inlet)
    ctx.close()


def _slab_grid(P, nx, nz_loc):
    import torch
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    return mg, MgpuGrid(mg, p0.nx, p0.ny, p0.nz)


def test_two_z_slab_ranks_report_what_the_one_rank_run_reports(hip, monkeypatch):
    """P = 2 z-slabs, wide advection halo, direct pressure solve, against the one-rank run of the same global 36×22×22 grid,
    step by step.  Sums — ke, c_vol, and the momentum the two set_cylinder! calls are about to remove (mom_predict,
    mom_correct), hence the force — within (L+8)·2⁻⁵³·Σ|term|, with Σ|term| from the one-rank run's own fields: captured on the
    host where that run reaches its set_cylinder! calls (ke, c_vol: non-negative terms, Σ|term| is the sum itself).  `mom` of
    the record's full set is taken AFTER :473 has zeroed the masked nodes: both runs must report exactly 0 there.  Maxima within
    1e-9 relative to the maximum itself."""
    from navierstokes3d_amd import driver, kernels as K
    nx, nt, P, nz_loc = 36, 3, 2, 12
    captured, real = [], K.set_cylinder

    def spy(Cf, Vx, Vy, Vz, *rest, ctx=None):
        captured.append(([K.to_numpy(t) for t in (Vx, Vy, Vz)], rest))
        real(Cf, Vx, Vy, Vz, *rest, ctx=ctx)
    monkeypatch.setattr(K, "set_cylinder", spy)
    one = driver.run_navierstokes3D(nx=nx, nt=nt, mode="strict", pressure="direct", return_info=True, diagnostics=True)[-1]
    monkeypatch.undo()
    calls = captured[1:]                                             # the first call is the initialisation multi.jl:372
    assert len(calls) == 2 * nt
    mg, grid = _slab_grid(P, nx, nz_loc)
    two = driver.run_navierstokes3D(nx=nx, nt=nt, mode="strict", grid=grid, return_info=True, shape=dict(nz=nz_loc), pressure="direct",
                                    wide_advect_halo=True, diagnostics=True)[-1]
    p = one.params
    assert (p.nx, p.ny, p.nz) == (36, 22, 22) and len(two.diag) == nt
    ctx = hip.Context(0, "strict")
    masks = _masks(hip, ctx, (36, 22, 22), calls[0][1], np.float64)
    ctx.close()
    L = max(D.path_length(36, 22, 22), D.path_length(36, 22, nz_loc))
    scale = p.rho * p.dx * p.dy * p.dz / p.dt
    seen = 0.0
    for k, (a, b) in enumerate(zip(one.diag, two.diag)):
        assert a.n_masked == b.n_masked == tuple(int(m.sum()) for m in masks) and a.nonfinite == b.nonfinite == 0
        for nm, x, y in [("vmax[%d]" % q, a.vmax[q], b.vmax[q]) for q in range(3)] + [("div_max", a.div_max, b.div_max),
                                                                                      ("pr_min", a.pr_min, b.pr_min), ("pr_max", a.pr_max, b.pr_max)]:
            print("step %d %s %.17g %.17g |diff| %.3e bound %.3e" % (k + 1, nm, x, y, abs(x - y), 1e-9 * abs(x)))
            assert abs(x - y) <= 1e-9 * abs(x), (k, nm)
        for nm in ("ke", "c_vol"):
            tol = (L + 8) * U53 * abs(getattr(a, nm))
            print("step %d %s %.17g %.17g |diff| %.3e tol %.3e" % (k + 1, nm, getattr(a, nm), getattr(b, nm), abs(getattr(a, nm) - getattr(b, nm)), tol))
            assert abs(getattr(a, nm) - getattr(b, nm)) <= tol, (k, nm)
        assert a.mom == b.mom == (0.0, 0.0, 0.0)                     # after :473 the masked nodes hold zeros
        for q in range(3):
            mags = [math.fsum(np.abs(V3[q][masks[q]])) for V3, _ in calls[2 * k:2 * k + 2]]
            for nm, mag in (("mom_predict", mags[0]), ("mom_correct", mags[1])):
                x, y, tol = getattr(a, nm)[q], getattr(b, nm)[q], (L + 8) * U53 * mag
                print("step %d %s[%d] %.17g %.17g |diff| %.3e tol %.3e" % (k + 1, nm, q, x, y, abs(x - y), tol))
                assert abs(x - y) <= tol, (k, nm, q)
                seen = max(seen, abs(x))
            tol = (L + 8) * U53 * (mags[0] + mags[1]) * scale
            print("step %d force[%d] %.17g %.17g |diff| %.3e tol %.3e" % (k + 1, q, a.force[q], b.force[q], abs(a.force[q] - b.force[q]), tol))
            assert abs(a.force[q] - b.force[q]) <= tol, (k, "force", q)
    assert seen > 0 and any(abs(r.force[0]) > 0 for r in two.diag) and any(abs(r.force[1]) > 0 for r in two.diag)
    mg.close()


def _run_with_vz_courant(monkeypatch, c2, wide=True):
    """one step on two z-slab ranks whose monitor reports max|Vz| = c2·dz/dt (Vz of this z-uniform case is rounding noise)"""
    from navierstokes3d_amd import driver
    from navierstokes3d_amd.mgpu import MgpuGrid
    real = MgpuGrid.diagnostics

    def forged(self, Vx, Vy, Vz, Pr, Cf, dps):
        glob, locs = real(self, Vx, Vy, Vz, Pr, Cf, dps)
        dp = dps[0]
        p = driver.multi_params(36, dims=(1, 1, 2), coords=(0, 0, 0), nz=12)
        assert dp.dz == p.dz
        glob.vmax = (glob.vmax[0], glob.vmax[1], c2 * p.dz / p.dt)
        return glob, locs
    monkeypatch.setattr(MgpuGrid, "diagnostics", forged)
    mg, grid = _slab_grid(2, 36, 12)
    try:
        return driver.run_navierstokes3D(nx=36, nt=1, mode="strict", grid=grid, shape=dict(nz=12), pressure="direct",
                                         wide_advect_halo=wide, diagnostics=True, return_info=True)[-1]
    finally:
        monkeypatch.undo()
        mg.sync()
        mg.close()


def test_wide_halo_precondition_is_enforced(hip, monkeypatch):
    """courant[2] ≥ 2 leaves ns3d_advect_wide's precondition.  Vz of this z-uniform case is rounding noise, so the finite
    branch is driven through the driver with a monitor whose max|Vz| is replaced: courant[2] = 1.5 runs to the end, 2.5 stops
    with the named error before advecting, and without wide_advect_halo 2.5 is only reported.  (The exact threshold:
    tests/test_diagnostics_host.py.)  Unforged, a dt scaled by 1e200 — noise times 1e200, or the NaN of the overflowing
    predictor — must stop the run too."""
    from navierstokes3d_amd import driver, lib as L
    info = _run_with_vz_courant(monkeypatch, 1.5)
    assert abs(info.diag[0].courant[2] - 1.5) < 1e-12
    with pytest.raises(L.Ns3dError, match=r"courant\[2\].*wide_advect_halo.*2 cells"):
        _run_with_vz_courant(monkeypatch, 2.5)
    info = _run_with_vz_courant(monkeypatch, 2.5, wide=False)
    assert abs(info.diag[0].courant[2] - 2.5) < 1e-12
    real = driver.multi_params

    def scaled(*a, **k):
        p = real(*a, **k)
        p.dt *= 1e200
        return p
    monkeypatch.setattr(driver, "multi_params", scaled)
    mg, grid = _slab_grid(2, 36, 12)
    with pytest.raises(L.Ns3dError, match=r"courant\[2\].*wide_advect_halo.*2 cells"):
        driver.run_navierstokes3D(nx=36, nt=4, mode="strict", grid=grid, shape=dict(nz=12), pressure="direct", wide_advect_halo=True,
                                  diagnostics=True)
    monkeypatch.undo()
    mg.sync()
    mg.close()


def test_error_paths_leave_the_context_usable(hip):
    import ctypes as C
    from navierstokes3d_amd import lib as L
    n = (24, 15, 15)
    g = geometry(*n)
    F = _host_fields(n, np.float64)
    ctx = hip.Context(0, "strict")
    dev = _upload(hip, F)
    dp = hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"])
    good = hip.diagnostics(*dev, dp, ctx=ctx)
    lib, out = L.load(), L.Diag()
    ptr = [C.c_void_p(t.data_ptr()) for t in dev]
    fn = lib.ns3d_diagnostics_f64
    assert fn(None, *ptr, C.byref(dp), C.byref(out)) == L.NS3D_ERR_ARG and b"null context" in lib.ns3d_last_error()
    assert fn(ctx.handle, None, *ptr[1:], C.byref(dp), C.byref(out)) == L.NS3D_ERR_ARG
    assert fn(ctx.handle, *ptr, None, C.byref(out)) == L.NS3D_ERR_ARG
    assert fn(ctx.handle, *ptr, C.byref(dp), None) == L.NS3D_ERR_ARG
    small = hip.diag_params(2, 15, 15, g["dx"], g["dy"], g["dz"], g["rho"])
    assert fn(ctx.handle, *ptr, C.byref(small), C.byref(out)) == L.NS3D_ERR_ARG and b"too small" in lib.ns3d_last_error()
    dp.cylinder = 3
    assert fn(ctx.handle, *ptr, C.byref(dp), C.byref(out)) == L.NS3D_ERR_ARG
    dp.cylinder = 0
    mfn = lib.ns3d_diagnostics_mgpu_f64
    assert mfn(None, None, None, None, None, None, C.byref(dp), C.byref(out), None) == L.NS3D_ERR_ARG
    from navierstokes3d_amd.mgpu import MultiGpu
    mg = MultiGpu.create([0, 0], *n, "strict")
    assert mfn(mg.handle, None, None, None, None, None, C.byref(dp), C.byref(out), None) == L.NS3D_ERR_ARG
    lists = [[t, t] for t in dev]
    with pytest.raises(L.Ns3dError, match="too small"):
        mg.diagnostics(*lists, [small, small])
    assert mg.diagnostics(*lists, [dp, dp])[0].nonfinite == 0
    mg.close()
    again = hip.diagnostics(*dev, dp, ctx=ctx)
    assert all(_same(getattr(good, k), getattr(again, k)) for k in vars(good))
    ctx.close()
