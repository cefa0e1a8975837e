"""CPU tests of the running-error reference (tests/running_error.py) that the FAST GPU tests lean on: the bound is sound
(exact rational arithmetic), the C oracle alone stays inside it on every case the GPU files use, it is tight enough to be worth
having, and it is not blind to one wrong element.  No GPU."""
import fractions
import random

import numpy as np
import pytest

import pair_cases as PC
import running_error as RE

DTYPES = [np.float32, np.float64]


# ---- (a) soundness ---------------------------------------------------------------------------------------------------------
def _round(fr, T):
    """RN of a rational to the element type (float32 through float64: the double rounding is inside the bound's 1+2⁻²⁰)"""
    return T(float(fr))


def _tree(rng, depth):
    if depth == 0 or rng.random() < 0.15:
        return ("leaf", rng.choice((-1, 1)) * rng.uniform(0.3, 3.0))
    op = rng.choice("++--**/s")                                       # s: a division by a grid spacing
    if op == "s":
        return ("s", _tree(rng, depth - 1), rng.choice((1.0 / 63, 0.6 / 38, 0.7 / 5, 1.0 / 130, 0.125)))
    return (op, _tree(rng, depth - 1), _tree(rng, depth - 1))


def _eval(t, T, rng, fast):
    """(value in the element type, exact rational, pair) of a tree; `fast`: a product feeding a sum is fused at random, a spacing
    division is x·RN(1/(T)d) — STRICT divides by (T)d"""
    if t[0] == "leaf":
        x = T(t[1])
        return x, fractions.Fraction(float(x)), RE.Pair(float(x), None, RE.unit(T))
    if t[0] == "s":
        x, fx, px = _eval(t[1], T, rng, fast)
        d = t[2]
        val = x * (T(1) / T(d)) if fast else x / T(d)
        return val, fx / fractions.Fraction(d), px / RE.spacing(d, T)
    a, fa, pa = _eval(t[1], T, rng, fast)
    b, fb, pb = _eval(t[2], T, rng, fast)
    if t[0] in "+-":
        s = 1 if t[0] == "+" else -1
        val = a + b if s > 0 else a - b
        if fast and t[2][0] == "*" and rng.random() < 0.7:            # fma(b1, b2, a): the product never rounded
            b1, fb1, _ = _eval(t[2][1], T, rng, False)
            b2, fb2, _ = _eval(t[2][2], T, rng, False)
            val = _round(fractions.Fraction(float(a)) + s * fractions.Fraction(float(b1)) * fractions.Fraction(float(b2)), T)
            return val, fa + s * fb1 * fb2, (pa + pb if s > 0 else pa - pb)
        return val, fa + s * fb, (pa + pb if s > 0 else pa - pb)
    if t[0] == "*":
        return a * b, fa * fb, pa * pb
    if fb == 0:
        return T(1), fractions.Fraction(1), RE.Pair(1.0, None, RE.unit(T))
    return a / b, fa / fb, pa / pb


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("T", DTYPES)
def test_bound_is_sound_on_random_expression_trees(T, fast):
    """300 random trees over + − · / (and divisions by a grid spacing) per type and build: the value computed in the element type
    — with products fused into sums at random and reciprocal spacings in the FAST variant — and the pair value both lie within the
    pair bound of the tree evaluated with fractions.Fraction."""
    rng = random.Random(20240 + (T == np.float32) + 2 * fast)
    checked = 0
    with np.errstate(all="ignore"):
        while checked < 300:
            val, exact, p = _eval(_tree(rng, 6), T, rng, fast)
            e = float(p.e)
            if not (np.isfinite(val) and np.isfinite(e)):             # a denominator whose enclosure reaches 0: no statement is made
                continue
            checked += 1
            assert abs(fractions.Fraction(float(val)) - exact) <= fractions.Fraction(e), (float(val), float(exact), e)
            assert abs(fractions.Fraction(float(p.v)) - exact) <= fractions.Fraction(e), (float(p.v), float(exact), e)


def test_exact_operations_are_charged_nothing():
    z, x = RE.Pair(np.zeros(3)), RE.Pair(np.array([1.0, -2.0, 3.0]))
    for p in (x + z, z + x, x - z, z - x, x * z, z / x, (x * z) * 0.3 + x):
        assert not p.e.any()
    assert ((x * 0.3).e > 0).all() and ((x / RE.spacing(0.1, np.float64)).e >= 3 * RE.U64 * 10).all()


# ---- (b) the reference alone stays inside, (c) tightness ----------------------------------------------------------------------
def _inside(a, p, dtype, what):
    """the oracle's array `a` against the pair value: within e (float32) or 2e (float64)"""
    return RE.check(a, None if dtype == np.float32 else p.v, p, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,grid", PC.all_once_per_step(), ids=lambda v: str(v).replace(" ", ""))
def test_oracle_within_bound_once_per_step(name, grid, dtype):
    host, scal, outs, ref, prs = PC.once_per_step(name, grid, dtype)
    for q in outs:
        assert _inside(ref[q], prs[q], dtype, "%s %r output %d" % (name, grid, q)) <= 1.0
    for q in range(len(host)):
        if q not in outs and name != "predict_fused":               # (the fused case's other arrays are the stresses it never stores)
            assert np.array_equal(prs[q].v, host[q]) and not prs[q].e.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(PC.KERNELS) + ["predict_fused"])
def test_flow_at_rest_has_bound_zero_and_the_oracle_matches(name, dtype):
    """uniform velocities, every other field ±0: the differences vanish exactly, so the bound is 0 wherever no constant enters, and
    there the oracle must equal the pair value"""
    grid = (24, 15, 15)
    host, scal, outs, ref, prs = PC.once_per_step(name, grid, dtype, "rest")
    zero = 0
    for q in outs:
        _inside(ref[q], prs[q], dtype, "%s at rest output %d" % (name, q))
        zero += int((prs[q].e == 0).sum())
        assert np.array_equal(ref[q][prs[q].e == 0], prs[q].v[prs[q].e == 0])
    assert zero > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("bc", PC.PT_BCS)
@pytest.mark.parametrize("grid", PC.PT_GRIDS)
def test_oracle_within_bound_pt_levels(grid, bc, dtype):
    Pr0, d0, rhs, levels = PC.pt_levels(grid, dtype, bc, 7)
    for lev, (Pr, d, pP, pd) in enumerate(levels):
        for what, a, p in (("Pr", Pr, pP), ("dPrdtau", d, pd)):
            _inside(a, p, dtype, "%s level %d" % (what, lev + 1))


def test_tightness_is_measured():
    """Median of e/(u·|v|) over the elements above the field's median magnitude, per kernel (largest over its grids and outputs;
    printed with -s).  Measured on the seeded cases, identical in float32 and float64 to the digits shown:

        update_tau 12.6    predict_V 1.59    predict_fused 1.64    update_divV 6.54    update_dPrdtau 7.77    update_Pr 1.00
        compute_res 5.53   correct_V 1.00    one PT iteration: Pr 7.91, dPrdτ 5.88

    All far below the 50 at which a bound stops being worth having (asserted).  The deeper PT levels are NOT: level 4 Pr 131,
    dPrdτ 290; level 7 Pr 3.4e3, dPrdτ 1.2e4.  That is the iteration, not the charging rule: with util.geometry's dτ the
    seeded U(−1,1) fields are far from PT's stable regime (dτ/dx² ≈ 29 on 57 columns), each level multiplies a cell's bound by the
    sum of the ABSOLUTE stencil coefficients (≈12·29) while the values, sums of as many terms of either sign, grow by about a third
    of that.  No rule that stays a bound can do better than the absolute sum, and no growth factor is guessed; the deep-level tests
    are correspondingly weaker per element (level 7, float32: ≈7e-4 relative) and still see what a norm cannot: one wrong cell."""
    worst = {}
    for dtype in DTYPES:
        for name, grid in PC.all_once_per_step():
            host, scal, outs, ref, prs = PC.once_per_step(name, grid, dtype)
            k = (name, np.dtype(dtype).name)
            worst[k] = max([worst.get(k, 0.0)] + [RE.tightness(prs[q]) for q in outs])
        Pr0, d0, rhs, levels = PC.pt_levels(PC.PT_GRIDS[0], dtype, PC.PT_BCS[0], 7)
        for lev in (0, 3, 6):
            worst[("PT level %d Pr" % (lev + 1), np.dtype(dtype).name)] = RE.tightness(levels[lev][2])
            worst[("PT level %d dPrdtau" % (lev + 1), np.dtype(dtype).name)] = RE.tightness(levels[lev][3])
    for k in sorted(worst):
        print("tightness %-22s %-8s median e/(u|v|) = %.3g" % (k + (worst[k],)))
    assert max(v for k, v in worst.items() if not k[0].startswith("PT level") or k[0].startswith("PT level 1")) < 50


# ---- (d) it is not blind -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_one_wrong_element_at_a_tile_corner_is_flagged(dtype):
    """predict_fused on 65×17×33: the element at the corner of the first 64×16×32 tile moved by 8·u·|v| (may or may not be
    flagged: it is what a bound with tightness 8 would just allow) and by 8·e (must be flagged, with its index in the message);
    the global relative-L2 norm of either is far below the 1e-5 / 1e-12 bars that the older tests hold FAST to."""
    from util import rel_l2
    host, scal, outs, ref, prs = PC.once_per_step("predict_fused", (65, 17, 33), dtype)
    idx = (63, 15, 31)
    base = ref[0].copy(order="F")
    RE.check(base, ref[0], prs[0], dtype, "unperturbed")
    u = RE.unit(dtype)
    small = base.copy(order="F"); small[idx] += dtype(8 * u * abs(prs[0].v[idx]))
    big = base.copy(order="F"); big[idx] += dtype(8 * RE.allowed(dtype) * prs[0].e[idx])
    assert big[idx] != base[idx]
    try:
        RE.check(small, ref[0], prs[0], dtype, "8u|v|")
        print("8·u·|v| passes (e/(u|v|) here: %.3g)" % (prs[0].e[idx] / (u * abs(prs[0].v[idx]))))
    except AssertionError:
        print("8·u·|v| is flagged (e/(u|v|) here: %.3g)" % (prs[0].e[idx] / (u * abs(prs[0].v[idx]))))
    with pytest.raises(AssertionError, match=r"\(63, 15, 31\)"):
        RE.check(big, ref[0], prs[0], dtype, "8e")
    assert rel_l2(big, base) < (1e-5 if dtype == np.float32 else 1e-12) / 100
    # one cell of a FAST output off by 1e-5 relative
    off = base.copy(order="F"); off[idx] *= dtype(1 + 1e-5)
    with pytest.raises(AssertionError):
        RE.check(off, ref[0], prs[0], dtype, "1e-5")


# ---- set_cylinder!: the oracle against the classification ----------------------------------------------------------------------
CYL_CASES = [(f, g, p, b) for f in ("global", "local") for g in PC.CYL_GRIDS for p in PC.CYL_PLACES for b in (0.0, 0.3)]

def _oracle_cyl(form, grid, dtype, sc):
    from oracle import oracle as K
    host = PC.cyl_fields(grid, dtype)
    out = [a.copy(order="F") for a in host]
    (K.set_cylinder if form == "global" else K.set_cylinder_local)(*out, *sc)
    return host, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form,grid,place,beta", CYL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_oracle_set_cylinder_matches_the_decided_flags(form, grid, place, beta, dtype):
    nx, ny, nz = grid
    sc = PC.cyl_scalars(form, grid, place, beta)
    host, out = _oracle_cyl(form, grid, dtype, sc)
    cls = PC.cyl_classify(form, grid, dtype, sc)
    und, edges = PC.cyl_check(out, host, cls, "%s %r %s β=%g" % (form, grid, place, beta))
    assert und <= 1e-3 * 4 * (nx + 1) * (ny + 1), und
    for q, (any_set, e) in enumerate(edges):
        assert any_set == (place != "empty"), ("flag %d" % q, place)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", ["global", "local"])
def test_every_array_edge_is_reached_by_a_set_flag(form, dtype):
    """over the cases of a form and type, each field has a DECIDED set flag on its first and last row and column"""
    reached = [set() for _ in range(4)]
    for f, grid, place, beta in CYL_CASES:
        if f == form:
            for q, (sure, clear) in enumerate(PC.cyl_classify(form, grid, dtype, PC.cyl_scalars(form, grid, place, beta))):
                sx, sy = PC.SHAPES[PC.CYL_KINDS[q]](*grid)[:2]
                reached[q] |= PC.edges_reached(sure[:sx, :sy])
    for q, e in enumerate(reached):
        assert e == {"i0", "i1", "j0", "j1"}, (PC.CYL_KINDS[q], e)


def test_mutations_of_the_cylinder_predicate_are_caught():
    """A dropped `i < nx` guard of the Vy flag fails cyl_check: the oracle's output, mutated on the CPU the way a kernel without
    the guard would leave it.  (`<` turned into `<=`: test_planted_ties_are_ties_and_the_oracle_leaves_them_alone.)"""
    form, grid, dtype = "local", (24, 15, 15), np.float64
    sc = PC.cyl_scalars(form, grid, "x_hi", 0.0)
    host, out = _oracle_cyl(form, grid, dtype, sc)
    cls = PC.cyl_classify(form, grid, dtype, sc)
    PC.cyl_check(out, host, cls, "unmutated")
    # a kernel without the guard evaluates column i = nx of Vy, which lies inside this ellipse, and stores through it: the store
    # lands on the next row's first entry, (0, j+1)
    thr, qp, own = PC.cyl_q(form, grid, dtype, sc)[2]
    inside = (qp.v < 1.0)[grid[0]]
    assert inside.any(), "the ellipse must cover a node of the column the guard protects"
    mut = [a.copy(order="F") for a in out]
    for j in np.flatnonzero(inside):
        if j + 1 <= grid[1]:
            mut[2][0, j + 1, :] = 0.0
    with pytest.raises(AssertionError):
        PC.cyl_check(mut, host, cls, "dropped guard")


# ---- advect!: the oracle against the classified back-tracks ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("faithful", [True, False])
@pytest.mark.parametrize("grid,cfl", PC.ADV_CASES)
def test_oracle_advect_matches_the_classified_backtracks(grid, cfl, faithful, dtype):
    from oracle import oracle as K
    old, outs, dt, g = PC.adv_inputs(grid, cfl, dtype)
    ref = [a.copy(order="F") for a in outs]
    K.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], faithful)
    pairs = PC.adv_pairs(grid, cfl, dtype, faithful)
    und, total, worst = PC.adv_check(ref, outs, old, pairs, dtype, ref, "oracle %r cfl %g" % (grid, cfl))
    print("oracle advect %r cfl %g %s faithful=%s: undecided %d of %d, worst err/bound %.3g" % (grid, cfl, np.dtype(dtype).name, faithful,
                                                                                             und, total, worst))
    assert und <= 1e-3 * total
    if dtype == np.float64:
        assert und == 0


def test_swapped_reciprocal_in_the_departure_is_caught():
    """rdx swapped for rdy in the departure of the x axis (dy ≠ dx) moves decided back-tracks outside their bound"""
    from oracle import oracle as K
    grid, cfl, dtype = (24, 15, 15), 1.0, np.float32
    old, outs, dt, g = PC.adv_inputs(grid, cfl, dtype)
    mut = [a.copy(order="F") for a in outs]
    K.advect(mut[0], old[0], mut[1], old[1], mut[2], old[2], mut[3], old[3], dt, g["dy"], g["dy"], g["dz"], True)
    with pytest.raises(AssertionError):
        PC.adv_check(mut, outs, old, PC.adv_pairs(grid, cfl, dtype, True), dtype, mut, "rdx→rdy")


# ---- planted cases: the assumptions the GPU tests rest on, checked against the oracle ------------------------------------------------
def test_planted_ties_are_ties_and_the_oracle_leaves_them_alone():
    """q is exactly 1.0 at the planted nodes in float32 and float64; the C oracle (`<`) leaves the velocity nodes alone and sets C;
    a `<=` in their place would set them — the mutation the GPU test is there to catch."""
    from oracle import numpy_ref as NR
    for sc, nodes in PC.tie_cases():
        for dtype in DTYPES:
            host, out = _oracle_cyl("local", PC.TIE_GRID, dtype, sc)
            for f, lst in nodes.items():
                for i, j, is_set in lst:
                    q32, q64 = PC.tie_q_is_one(sc, f, i, j)
                    tie = q32 == 1.0 and q64 == 1.0
                    assert tie or (q32 < 1.0) == (q64 < 1.0) == is_set
                    assert (out[f][i, j, :] == PC.CYL_SET[f]).all() == is_set
                    if not is_set:
                        assert np.array_equal(out[f][i, j, :], host[f][i, j, :])
                    if tie and f != 0:
                        assert not is_set and q64 <= 1.0                    # `<=` would set it
    assert sum(1 for sc, nodes in PC.tie_cases() for f, l in nodes.items() for i, j, s in l if PC.tie_q_is_one(sc, f, i, j)[0] == 1.0) >= 8


@pytest.mark.parametrize("faithful", [True, False])
def test_planted_departures_are_exact(faithful):
    """every operation of the planted advect! case is exact: the float32 oracle and the float64 oracle return the same numbers, and δ
    of each field's own axis takes the values 1, 2, −1, ±½, 1½, 0 and −0"""
    from oracle import oracle as K
    res = []
    for dtype in DTYPES:
        old, dt, g = PC.planted_departures(dtype)
        out = [np.zeros_like(a) for a in old]
        K.advect(out[0], old[0], out[1], old[1], out[2], old[2], out[3], old[3], dt, g["dx"], g["dy"], g["dz"], faithful)
        res.append(out)
        deltas = np.unique(old[0] * dtype(dt) / dtype(g["dx"]))
        assert set(deltas.tolist()) == {0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0} and np.signbit(old[0][old[0] == 0]).any()
    for a, b in zip(*res):
        assert np.array_equal(a.astype(np.float64), b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_reference_start_delta_and_candidates(dtype):
    """dx = 1/63, dt = dx/vin: STRICT's δ is exactly 1 and so is FAST's dt·v·RN(1/dx), in both types (printed); the oracle's tracer is
    the candidate that δ selects"""
    from oracle import oracle as K
    old, prefill, dt, g, d_strict, d_fast, cands = PC.start_case(dtype)
    print("%s: STRICT δ − 1 = %g, FAST δ − 1 = %g" % (np.dtype(dtype).name, float(d_strict) - 1, float(d_fast) - 1))
    assert d_strict == 1.0 and d_fast == 1.0
    ref = [b.copy(order="F") for b in prefill]
    K.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], True)
    assert PC.start_check(ref[3], cands[:1], dtype) is None
    # δ = 1 exactly: weight 1 on A_o[ix1 + 1] with ix1 = max(ix − 1, 1) — the step leaves the tracer where it is, except that the
    # clamp makes the first column a copy of the second
    assert np.array_equal(ref[3][1:], old[3][1:]) and np.array_equal(ref[3][0], old[3][1])
