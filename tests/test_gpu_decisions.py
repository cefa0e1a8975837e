"""The two once-per-step kernels whose output hinges on a comparison — set_cylinder! (q < 1, q < 1.05) and advect! (floor(ix − δ),
δ > 0, δ%1) — in every mode and type, classified with the value/bound pairs of tests/running_error.py: a comparison is DECIDED when
the enclosure of its operand lies strictly on one side of every breakpoint, and only there is one answer demanded.  Undecided ones
are capped (a condition the reference alone meets on the CPU: tests/test_running_error_host.py) and must still be one of the
admissible answers.  Planted ties and exact departures, where no mode has any freedom, must match the oracle bit for bit."""
import numpy as np
import pytest

import pair_cases as PC
from util import bits_equal, first_bit_difference, rnd

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


def _hip_cyl(hip, ctx, host, sc):
    import torch
    dev = [hip.from_numpy(a) for a in host]
    hip.set_cylinder(*dev, *sc, ctx=ctx)
    torch.cuda.synchronize()
    return [hip.to_numpy(d) for d in dev]


# ---- set_cylinder! -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("grid", PC.CYL_GRIDS)
@pytest.mark.parametrize("form", ["global", "local"])
def test_set_cylinder_decided_flags_every_mode(hip, oracle, form, grid, dtype):
    """Both forms, β ∈ {0, 0.3}, the ellipse inside the array, across each of its four edges (the global form as a Cartesian rank that
    cuts the cylinder gets it: by xco_g, yco_g), across a corner, and covering no node.  STRICT: bit for bit against the C oracle in
    the same type.  STRICT and FAST: every decided column has the pair reference's four flags on every plane (k = nz of Vz included;
    63×38×38 runs two z-chunks), every cell whose flag is clear keeps its input bits (seeded fields, not ones), an undecided column
    is set or kept as a whole.  So that this cannot pass vacuously: at most 0.1 % of a case's 4·(nx+1)(ny+1) flags are undecided, each
    of the four flags is set on a decided column in every case but the empty one, and over the cases each field's four edges are
    reached by a decided set flag."""
    nx, ny, nz = grid
    host = PC.cyl_fields(grid, dtype)
    reached = [set() for _ in range(4)]
    ctxs = {m: hip.Context(0, m) for m in ("strict", "fast")}
    worst_und = 0
    for place in PC.CYL_PLACES:
        for beta in (0.0, 0.3):
            sc = PC.cyl_scalars(form, grid, place, beta)
            what = "%s %r %s β=%g %s" % (form, grid, place, beta, np.dtype(dtype).name)
            ref = [a.copy(order="F") for a in host]
            (oracle.set_cylinder if form == "global" else oracle.set_cylinder_local)(*ref, *sc)
            cls = PC.cyl_classify(form, grid, dtype, sc)
            for mode, ctx in ctxs.items():
                got = _hip_cyl(hip, ctx, host, sc)
                if mode == "strict":
                    for n, a, b in zip("C Vx Vy Vz".split(), got, ref):
                        assert bits_equal(a, b), ("STRICT " + what, n, first_bit_difference(a, b))
                und, edges = PC.cyl_check(got, host, cls, mode.upper() + " " + what)
                assert und <= 1e-3 * 4 * (nx + 1) * (ny + 1), (what, und)
                worst_und = max(worst_und, und)
                for q, (any_set, e) in enumerate(edges):
                    assert any_set == (place != "empty"), (what, "flag %d" % q)
                    reached[q] |= e
    for ctx in ctxs.values():
        ctx.close()
    print("set_cylinder %s %r %s: most undecided flags in a case %d" % (form, grid, np.dtype(dtype).name, worst_und))
    for q, e in enumerate(reached):
        assert e == {"i0", "i1", "j0", "j1"}, (PC.CYL_KINDS[q], e)


def test_set_cylinder_planted_ties(hip, oracle):
    """q exactly 1.0 on a Vx node, a Vy node and a cell centre (pair_cases.tie_cases): `<` is not `≤`, so the velocity nodes are left
    alone while C, tested against 1.05, is set — and all four mode/type combinations match the oracle bit for bit."""
    grid = PC.TIE_GRID
    for sc, nodes in PC.tie_cases():
        for f, lst in nodes.items():
            for i, j, is_set in lst:
                q32, q64 = PC.tie_q_is_one(sc, f, i, j)
                if not is_set or f == 0:
                    assert (q32 == 1.0 and q64 == 1.0) or q64 > 1.0
        for dtype in DTYPES:
            host = PC.cyl_fields(grid, dtype)
            ref = [a.copy(order="F") for a in host]
            oracle.set_cylinder_local(*ref, *sc)
            for mode in ("strict", "fast"):
                ctx = hip.Context(0, mode)
                got = _hip_cyl(hip, ctx, host, sc)
                ctx.close()
                for n, a, b in zip("C Vx Vy Vz".split(), got, ref):
                    assert bits_equal(a, b), (mode, np.dtype(dtype).name, n, first_bit_difference(a, b))
                for f, lst in nodes.items():
                    for i, j, is_set in lst:
                        col = got[f][i, j, :]
                        if is_set:
                            assert (col == PC.CYL_SET[f]).all(), (mode, f, i, j)
                        else:
                            assert bits_equal(col, host[f][i, j, :]), (mode, f, i, j, "a node with q = 1.0 exactly was set: < is not <=")


# ---- advect! / copy_advect --------------------------------------------------------------------------------------------------------
def _run_advect(hip, ctx, kernel, old, prefill, dt, g, faithful):
    """→ outputs [Vx, Vy, Vz, C] on the host; asserts the old fields untouched"""
    import torch
    do = [hip.from_numpy(a) for a in old]
    if kernel == "advect":
        d = [hip.from_numpy(a) for a in prefill]
        hip.advect(d[0], do[0], d[1], do[1], d[2], do[2], d[3], do[3], dt, g["dx"], g["dy"], g["dz"], faithful, ctx=ctx)
    else:
        d = [hip.from_numpy(np.full_like(a, 777.0)) for a in old]
        hip.copy_advect(d[0], do[0], d[1], do[1], d[2], do[2], d[3], do[3], dt, g["dx"], g["dy"], g["dz"], faithful, ctx=ctx)
    torch.cuda.synchronize()
    for a, b in zip(do, old):
        assert bits_equal(hip.to_numpy(a), b), "an input of %s changed" % kernel
    return [hip.to_numpy(a) for a in d]


@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("faithful", [True, False])
@pytest.mark.parametrize("grid,cfl", PC.ADV_CASES)
def test_fast_advect_classified_backtracks(hip, oracle, grid, cfl, faithful, dtype, form, monkeypatch):
    """FAST advect! and copy_advect, windowed and NS3D_ADVECT_GLOBAL=1: the windowed tile plus one cell, departure points inside the
    window and far outside it.  Per back-track: every axis decided → within the bound of the pair interpolant (weights and the three
    lerp levels through the pair arithmetic); otherwise → inside the hull of the old field over the candidate stencils, widened by
    the bound.  Entries advect! leaves alone keep their bits (copy_advect writes the current value through); inputs untouched;
    undecided back-tracks at most 0.1 % of the case's."""
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    old, prefill, dt, g = PC.adv_inputs(grid, cfl, dtype)
    ref = [a.copy(order="F") for a in prefill]
    oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], faithful)
    pairs = PC.adv_pairs(grid, cfl, dtype, faithful)
    ctx = hip.Context(0, "fast")
    for kernel in ("advect", "copy_advect"):
        got = _run_advect(hip, ctx, kernel, old, prefill, dt, g, faithful)
        what = "FAST %s %s %r cfl %g %s faithful=%s" % (kernel, form, grid, cfl, np.dtype(dtype).name, faithful)
        und, total, worst = PC.adv_check(got, prefill, old, pairs, dtype, ref, what, through=kernel == "copy_advect")
        print("%s: undecided %d of %d back-tracks, worst err/bound %.3g" % (what, und, total, worst))
        assert und <= 1e-3 * total
    ctx.close()


@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_advect_planted_exact_departures(hip, oracle, dtype, form, monkeypatch):
    """Power-of-two spacings, dt·v exact: δ is exactly an integer (1, 2, −1), a half-integer, 0 or −0 on a field's own axis, a
    multiple of 1/8 on the others; the advected values are small multiples of ½, so every lerp is exact under any contraction.
    FAST has no freedom: it must equal the oracle bit for bit, like STRICT, in both kernel forms and both entry points.  (Extends
    test_gpu_kernels.test_advect_integer_cfl_edge: uniform 2 / −1 / 0 velocities, float64, STRICT.)"""
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    old, dt, g = PC.planted_departures(dtype)
    prefill = [rnd(40 + q, a.shape, dtype) for q, a in enumerate(old)]
    for faithful in (True, False):
        ref = [a.copy(order="F") for a in prefill]
        oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], faithful)
        thr = [a.copy(order="F") for a in old]
        oracle.advect(thr[0], old[0], thr[1], old[1], thr[2], old[2], thr[3], old[3], dt, g["dx"], g["dy"], g["dz"], faithful)
        for mode in ("fast", "strict"):
            ctx = hip.Context(0, mode)
            for kernel, want in (("advect", ref), ("copy_advect", thr)):
                got = _run_advect(hip, ctx, kernel, old, prefill, dt, g, faithful)
                for n, a, b in zip("Vx Vy Vz C".split(), got, want):
                    assert bits_equal(a, b), (mode, kernel, form, faithful, n, first_bit_difference(a, b))
            ctx.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_advect_at_the_reference_start(hip, oracle, dtype):
    """The reference's own first step (pair_cases.start_case): δ_x sits ON the integer 1.  Which side of 1 STRICT's and FAST's δ fall
    is computed on the CPU and printed; the FAST output of the seeded tracer must be the reference's interpolant for FAST's δ, with
    the floor's operand evaluated either way a contraction allows, within the bound — and the oracle's very bits when FAST's δ is
    STRICT's and both operands select the same stencil."""
    T = dtype
    old, prefill, dt, g, d_strict, d_fast, cands = PC.start_case(T)
    side = lambda d: "below" if d < 1 else ("above" if d > 1 else "on")
    print("%s: STRICT δ = %r (%s 1), FAST δ = %r (%s 1)" % (np.dtype(T).name, float(d_strict), side(d_strict), float(d_fast), side(d_fast)))
    ctx = hip.Context(0, "fast")
    got = _run_advect(hip, ctx, "advect", old, prefill, dt, g, True)
    ctx.close()
    bad = PC.start_check(got[3], cands, T)
    assert bad is None, "C%r = %r is the interpolant of neither operand of the floor (candidates %r, %r)" % bad
    same = bits_equal(cands[0].v, cands[1].v)
    ref = [b.copy(order="F") for b in prefill]
    oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], True)
    print("%s: the two floor operands select %s; FAST C equals the oracle's bits: %s" % (
        np.dtype(T).name, "the same stencil everywhere" if same else "different stencils somewhere", bits_equal(got[3], ref[3])))
    if d_fast == d_strict and same:                                       # then FAST's δ selects the oracle's stencil and weight 1
        assert np.array_equal(got[3], ref[3])
        assert np.array_equal(got[0][1:], ref[0][1:])                     # a uniform stream stays uniform
    assert bits_equal(got[0][:1], prefill[0][:1])
