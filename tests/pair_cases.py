"""The cases that tests/test_running_error_host.py (C oracle, CPU) and the GPU files test_gpu_fast_elementwise.py /
test_gpu_decisions.py share: for each kernel the seeded inputs, the oracle's output and the value/bound pairs of
tests/running_error.py, computed once per (kernel, grid, type) and never modified."""
import functools

import numpy as np

import running_error as RE
from oracle import numpy_ref as NR
from util import SHAPES, fields, geometry, hostile

GRIDS_T = [(17, 9, 5), (24, 15, 15), (5, 4, 3), (70, 6, 7), (130, 5, 4)]         # test_gpu_kernels.GRIDS_T
FUSED_GRIDS = GRIDS_T + [(64, 16, 32), (65, 17, 33), (129, 3, 3)]                 # one tile exactly, one cell more, a row of three waves
SPACINGS = ("dx", "dy", "dz")

# name → (array kinds, scalar names, output positions, seed) — kinds, scalars and seeds of test_gpu_kernels.py
KERNELS = {
    "update_tau": (["c", "c", "c", "s", "s", "s", "vx", "vy", "vz"], ("mu", "dx", "dy", "dz"), range(6), 1),
    "predict_V": (["vx", "vy", "vz", "c", "c", "c", "s", "s", "s"], ("rho", "g", "dt", "dx", "dy", "dz"), range(3), 1),
    "update_divV": (["c", "vx", "vy", "vz"], ("dx", "dy", "dz"), [0], 1),
    "update_dPrdtau": (["c", "i", "c"], ("rho", "dt", "dtau", "damp", "dx", "dy", "dz"), [1], 1),
    "update_Pr": (["c", "i"], ("dtau",), [0], 1),
    "compute_res": (["i", "c", "c"], ("rho", "dt", "dx", "dy", "dz"), [0], 1),
    "correct_V": (["vx", "vy", "vz", "c"], ("dt", "rho", "dx", "dy", "dz"), range(3), 1),
}
FUSED_KINDS = ["vx", "vy", "vz", "c", "c", "c", "s", "s", "s"]


def pair_scalars(names, g, dtype):
    return [RE.spacing(g[n], dtype) if n in SPACINGS else RE.scalar(g[n], dtype) for n in names]


def inputs(name, grid, dtype, values="seeded"):
    """host inputs of a case; values: 'seeded' (util.fields) or 'rest' (a flow at rest: velocities uniform, everything else ±0)"""
    kinds, seed = (FUSED_KINDS, 5) if name == "predict_fused" else (KERNELS[name][0], KERNELS[name][3])
    host = fields(*grid, kinds, seed, dtype)
    if values == "rest":
        host = [hostile(a, 7 + q, "uniform" if k in ("vx", "vy", "vz") else "rest0") for q, (a, k) in enumerate(zip(host, kinds))]
    return host


@functools.lru_cache(maxsize=None)
def once_per_step(name, grid, dtype, values="seeded"):
    """(host inputs, scalars, output positions, oracle outputs, pair outputs) of one once-per-step kernel"""
    from oracle import oracle as K
    g = geometry(*grid)
    host = inputs(name, grid, dtype, values)
    ref = [a.copy(order="F") for a in host]
    prs = [RE.field(a) for a in host]
    if name == "predict_fused":
        outs = range(3)
        scal = (g["mu"], g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])
        K.update_tau(*ref[3:], *ref[:3], g["mu"], g["dx"], g["dy"], g["dz"])
        K.predict_V(*ref, g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"])
        NR.update_tau(*prs[3:], *prs[:3], *pair_scalars(("mu", "dx", "dy", "dz"), g, dtype))
        NR.predict_V(*prs, *pair_scalars(("rho", "g", "dt", "dx", "dy", "dz"), g, dtype))
    else:
        _, snames, outs, _ = KERNELS[name]
        scal = tuple(g[n] for n in snames)
        getattr(K, name)(*ref, *scal)
        getattr(NR, name)(*prs, *pair_scalars(snames, g, dtype))
    for a in host + ref:
        a.setflags(write=False)
    return host, scal, list(outs), ref, prs


def all_once_per_step():
    """(kernel, grid) of §2's once-per-step cases"""
    return [(k, g) for k in KERNELS for g in GRIDS_T] + [("predict_fused", g) for g in FUSED_GRIDS]


# ---- pseudo-transient iterations -------------------------------------------------------------------------------------------
PT_GRIDS = [(57, 25, 9), (58, 26, 10)]          # the two smallest of test_gpu_pt.py that straddle the tile strides (56 columns / 24 rows)
PT_BCS = [(0, True, 0.75), (0, False, 0.0), (1, False, 0.0)]       # multi.jl's set with the outlet owned / not owned, gpu.jl's set


@functools.lru_cache(maxsize=None)
def pt_levels(grid, dtype, bc, nlev):
    """PT iterates 1…nlev of seeded (Pr, dPrdτ, rhs): the oracle's and the pairs'.  Level l+1 is the twin's update_dPrdτ /
    update_Pr / set_bc_Pr run once more on the pairs of level l — the bound grows as the arithmetic says, no factor guessed.
    Returns (Pr0, d0, rhs, [(Pr_ref, d_ref, Pr_pair, d_pair) per level])."""
    from oracle import oracle as K
    nx, ny, nz = grid
    g = geometry(*grid)
    bc_kind, owns, val = bc
    Pr0, d0, rhs = fields(nx, ny, nz, ["c", "i", "c"], 1234, dtype)
    Pr, d = Pr0.copy(order="F"), d0.copy(order="F")
    pP, pd, prhs = RE.field(Pr0), RE.field(d0), RE.field(rhs)
    sc = pair_scalars(("rho", "dt", "dtau", "damp", "dx", "dy", "dz"), g, dtype)
    levels = []
    for _ in range(nlev):
        K.update_dPrdtau(Pr, d, rhs, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"])
        K.update_Pr(Pr, d, g["dtau"])
        K.set_bc_Pr(Pr, bc_kind, owns, val, g["dz"], nz, g["g"], g["rho"])
        NR.update_dPrdtau(pP, pd, prhs, *sc)
        NR.update_Pr(pP, pd, sc[2])
        if bc_kind == 0:
            NR.set_bc_Pr_multi(pP, owns, float(np.dtype(dtype).type(val)))
        else:
            NR.set_bc_Pr_gpu(pP, RE.scalar(g["dz"], dtype), nz, RE.scalar(g["g"], dtype), RE.scalar(g["rho"], dtype))
        levels.append((Pr.copy(order="F"), d.copy(order="F"), pP.copy(), pd.copy()))
    return Pr0, d0, rhs, levels


# ---- set_cylinder! -----------------------------------------------------------------------------------------------------------
CYL_GRIDS = [(24, 15, 15), (70, 6, 7), (63, 38, 38), (130, 40, 5)]
CYL_A2, CYL_B2 = 0.0121, 0.0064                                                     # semi-axes 0.11, 0.08 (test_set_cylinder_both_forms)
# where the ellipse sits relative to the LOCAL array [−lx/2, lx/2]×[−ly/2, ly/2] (lx = 1, ly = 0.6): centre as fractions of lx, ly
CYL_PLACES = {"interior": (-0.1, 0.02 / 0.6), "x_lo": (-0.5, 0.05), "x_hi": (0.5, -0.05), "y_lo": (0.13, -0.5), "y_hi": (-0.21, 0.45),
              "corner": (0.5, 0.45), "empty": (-1.9, 0.7)}


def cyl_scalars(form, grid, place, beta):
    """The argument list after the four fields.  local form: the ellipse centre is moved.  global form: the centre stays the
    interior one and the RANK moves — xco_g, yco_g of a rank of a Cartesian topology whose local array cuts the cylinder."""
    nx, ny, nz = grid
    lx, ly, lz = 1.0, 0.6, 0.6
    dx, dy, dz = lx / nx, ly / ny, lz / nz
    fx, fy = CYL_PLACES[place]
    sb, cb = float(np.sin(beta)), float(np.cos(beta))
    if form == "local":
        return (CYL_A2, CYL_B2, fx * lx, fy * ly, sb, cb, lx, ly, lz, dx, dy, dz)
    ox, oy = CYL_PLACES["interior"][0] * lx, CYL_PLACES["interior"][1] * ly
    # the rank's first cell centre: the single-rank value shifted so that the ellipse sits at (fx, fy) of the local array
    xco, yco = -(lx - dx) / 2 + (ox - fx * lx), -(ly - dy) / 2 + (oy - fy * ly)
    return (CYL_A2, CYL_B2, ox, oy, sb, cb, xco, yco, -(lz - dz) / 2, lx, ly, lz, dx, dy, dz)


def cyl_q(form, grid, dtype, sc):
    """numpy_ref._apply_cyl's four quadratic forms on pairs, on the (nx+1, ny+1) column grid, with the mask of the columns each
    field owns: [(threshold, q pair, owned mask)] for C, Vx, Vy, Vz."""
    nx, ny, nz = grid
    S = lambda x: RE.scalar(x, dtype)
    a2, b2, ox, oy, sinb, cosb = (S(x) for x in sc[:6])
    ii, jj = np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64)
    if form == "global":
        xco, yco, dx, dy = S(sc[6]), S(sc[7]), S(sc[12]), S(sc[13])
        xc = xco + ii * dx                                          # numpy_ref.set_cylinder
        yc = yco + jj * dy
        xv, yv = xc - dx / 2, yc - dy / 2
    else:
        lx, ly, dx, dy = S(sc[6]), S(sc[7]), S(sc[9]), S(sc[10])
        xv = ii * dx - lx / 2                                       # numpy_ref.set_cylinder_local
        yv = jj * dy - ly / 2
        xc, yc = xv + dx / 2, yv + dx / 2                           # dx/2: sic
    XC, YC, XV, YV = xc[:, None], yc[None, :], xv[:, None], yv[None, :]
    own_i, own_j = (np.arange(nx + 1) < nx)[:, None], (np.arange(ny + 1) < ny)[None, :]
    every = np.ones((nx + 1, ny + 1), dtype=bool)
    q = lambda X, Y: NR._q(X, Y, ox, oy, sinb, cosb, a2, b2)
    qcc = q(XC, YC)
    return [(1.05, qcc, own_i & own_j), (1.0, q(XV, YC), every & own_j), (1.0, q(XC, YV), own_i & every), (1.0, qcc, own_i & own_j)]


def cyl_classify(form, grid, dtype, sc):
    """per field (C, Vx, Vy, Vz): (certainly set, certainly clear) on the (nx+1, ny+1) column grid"""
    out = []
    for thr, qp, own in cyl_q(form, grid, dtype, sc):
        below, above = RE.decided_below(qp, float(np.dtype(dtype).type(thr)))
        out.append((below & own, above | ~own))
    return out


CYL_SET = (1.0, 0.0, 0.0, 0.0)
CYL_KINDS = ["c", "vx", "vy", "vz"]


def edges_reached(sure):
    """which edges of a field's (i, j) extent a decided set flag lies on"""
    return {n for n, m in (("i0", sure[0]), ("i1", sure[-1]), ("j0", sure[:, 0]), ("j1", sure[:, -1])) if m.any()}


def cyl_check(got, host, cls, what):
    """The outputs of a set_cylinder! call against the classification: decided-set columns hold the set value on every plane,
    decided-clear columns keep their input bits on every plane, an undecided column is one or the other throughout.
    Returns (number of undecided flags, per field the set of array edges 'i0','i1','j0','j1' a decided set flag reaches)."""
    undecided, edges = 0, []
    for name, g, h, (sure, clear), setv in zip(("C", "Vx", "Vy", "Vz"), got, host, cls, CYL_SET):
        sx, sy, sz = g.shape
        sure, clear = sure[:sx, :sy], clear[:sx, :sy]
        is_set = g == setv
        kept = g.view(np.uint32 if g.dtype == np.float32 else np.uint64) == h.view(np.uint32 if g.dtype == np.float32 else np.uint64)
        bad = sure[:, :, None] & ~is_set
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s %s: decided column %r not set at plane %d (got %r)" % (what, name, i[:2], i[2], float(g[i])))
        bad = clear[:, :, None] & ~kept
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s %s: column %r outside the ellipse was touched at plane %d (got %r, had %r)" % (
                what, name, i[:2], i[2], float(g[i]), float(h[i])))
        und = ~sure & ~clear
        col_set, col_kept = is_set.all(axis=2), kept.all(axis=2)
        assert (col_set | col_kept)[und].all(), "%s %s: an undecided column is set on some planes only" % (what, name)
        undecided += int(und.sum())
        edges.append((bool(sure.any()), edges_reached(sure)))
    return undecided, edges


def cyl_fields(grid, dtype):
    nx, ny, nz = grid
    return fields(nx, ny, nz, CYL_KINDS, 1, dtype)


# ---- advect! -----------------------------------------------------------------------------------------------------------------
ADV_CASES = [((24, 15, 15), 1.0), ((65, 17, 33), 1.0), ((150, 21, 70), 0.9), ((150, 21, 70), 2.7)]


def adv_inputs(grid, cfl, dtype):
    """old fields, pre-filled outputs, dt and geometry as in test_advect_windowed_tiles"""
    nx, ny, nz = grid
    g = geometry(*grid)
    old = fields(nx, ny, nz, CYL_KINDS[1:] + ["c"], 21, dtype)
    outs = fields(nx, ny, nz, CYL_KINDS[1:] + ["c"], 31, dtype)
    return old, outs, cfl * min(g["dx"], g["dy"], g["dz"]), g


@functools.lru_cache(maxsize=None)
def adv_pairs(grid, cfl, dtype, faithful):
    old, outs, dt, g = adv_inputs(grid, cfl, dtype)
    P = [RE.field(a) for a in old]
    return RE.advect(*P, RE.scalar(dt, dtype), *(RE.spacing(g[n], dtype) for n in SPACINGS), faithful)


def adv_check(got, prefill, old, pairs, dtype, ref, what, through=False):
    """Outputs [Vx, Vy, Vz, C] of advect! (or copy_advect: through=True) against the pair back-tracks.  `ref`: the oracle's
    outputs (the float64 comparison is between two evaluations).  Returns (undecided, back-tracks, worst err/bound)."""
    names = ["Vx", "Vy", "Vz", "C"]
    written = [np.zeros(a.shape, dtype=bool) for a in got]
    final = {}
    for name, idx, val, dec, lo, hi in pairs:                        # a later back-track of the same field overrides an earlier one
        final.setdefault(name, []).append((idx, val, dec, lo, hi))
    undecided = total = 0
    worst = 0.0
    k = RE.allowed(dtype)
    for name, lst in final.items():
        q = names.index(name)
        sel_v, sel_e, sel_dec, sel_lo, sel_hi = (np.zeros(got[q].shape) for _ in range(5))
        for idx, val, dec, lo, hi in lst:
            sel_v[idx], sel_e[idx], sel_dec[idx], sel_lo[idx], sel_hi[idx] = val.v, val.e, dec, lo, hi
            written[q][idx] = True
            undecided += int((~dec).sum()); total += dec.size
        w, dec = written[q], sel_dec.astype(bool) & written[q]
        g64 = got[q].astype(np.float64)
        target = sel_v if np.dtype(dtype) == np.float32 else ref[q].astype(np.float64)
        err, bound = np.abs(g64 - target), k * sel_e
        ok = np.where(bound == 0, err == 0, err <= bound)
        bad = dec & ~ok
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s %s: %d decided back-tracks outside the bound; first at %r: got %r, reference %r, bound %.3e" % (
                what, name, int(bad.sum()), i, float(g64[i]), float(target[i]), float(bound[i])))
        with np.errstate(all="ignore"):
            r = np.where(dec & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
        worst = max(worst, float(r.max()))
        und = w & ~sel_dec.astype(bool)
        bad = und & ~((g64 >= sel_lo - bound) & (g64 <= sel_hi + bound))
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s %s: undecided back-track at %r = %r outside the hull [%r, %r] of its candidate stencils" % (
                what, name, i, float(g64[i]), float(sel_lo[i]), float(sel_hi[i])))
    for q, name in enumerate(names):                                 # entries advect! leaves alone
        keep = ~written[q]
        src = old[q] if through else prefill[q]
        assert np.array_equal(got[q][keep], src[keep]), "%s %s: an entry advect! leaves alone changed" % (what, name)
    return undecided, total, worst


# ---- planted ties and exact departures: FAST has no freedom ------------------------------------------------------------------------
TIE_GRID = (32, 16, 33)


def tie_cases():
    """set_cylinder! (local form, β = 0) on power-of-two spacings dx = 1/32, dy = 1/16 with the centre on a cell centre, (1/64, 1/64):
    every coordinate, difference, square and quotient below is exact in float32, and with sinb = 0 no product feeds a sum that could
    change it, so q is the same number in every mode and type.
      A: a2 = (7/64)², b2 = (11/64)² — the +x end of the ellipse is the Vx node (i=20, j=8), the +y end the Vy node (i=16, j=11):
         q = 1.0 exactly there, and `<` leaves both alone.
      B: a2 = (4/32)², b2 = (3/16)² — the axis ends are the cell centres (i=20, j=8) and (i=16, j=11): q = 1.0 exactly, so Vz stays
         (1.0 < 1.0 is false) and C is set (1.0 < 1.05).
    Returns [(scalars, {field index: [(i, j, must be set?)]})]."""
    lx, ly, lz, dx, dy, dz = 1.0, 1.0, 1.0, 1.0 / 32, 1.0 / 16, 1.0 / 32
    ox = oy = 1.0 / 64
    A = (49.0 / 4096, 121.0 / 4096, ox, oy, 0.0, 1.0, lx, ly, lz, dx, dy, dz)
    B = (1.0 / 64, 9.0 / 256, ox, oy, 0.0, 1.0, lx, ly, lz, dx, dy, dz)
    return [(A, {1: [(20, 8, False), (19, 8, True), (13, 8, False), (14, 8, True)], 2: [(16, 11, False), (16, 10, True), (16, 5, False)]}),
            (B, {0: [(20, 8, True), (16, 11, True), (12, 8, True)], 3: [(20, 8, False), (16, 11, False), (12, 8, False), (19, 8, True)]})]


def tie_q_is_one(sc, field, i, j):
    """the quadratic form of numpy_ref at that node, in float32 and float64: (q32, q64)"""
    out = []
    for T in (np.float32, np.float64):
        a2, b2, ox, oy, sinb, cosb, lx, ly, lz, dx, dy, dz = (T(x) for x in sc)
        xv, yv = T(i) * dx - lx / T(2), T(j) * dy - ly / T(2)
        xc, yc = xv + dx / T(2), yv + dx / T(2)
        X, Y = {0: (xc, yc), 1: (xv, yc), 2: (xc, yv), 3: (xc, yc)}[field]
        out.append(NR._q(X, Y, ox, oy, sinb, cosb, a2, b2))
    return out


PLANT_GRID = (70, 11, 7)


def planted_departures(dtype):
    """advect! inputs whose every δ is exact: spacings and dt = 1/8, velocities drawn from {0, −0, ±½, ±1, 1½, 2} (δ of a field's own
    axis exactly an integer, a half-integer, 0 or −0; the averaged ones multiples of 1/8), advected values multiples of ½ up to 2
    (velocities) or small integers (C): every product of every lerp is exact under any contraction."""
    nx, ny, nz = PLANT_GRID
    rng = np.random.Generator(np.random.MT19937(99))
    pick = lambda shape: np.asfortranarray(rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0]), size=shape).astype(dtype))
    old = [pick(SHAPES[k](nx, ny, nz)) for k in ("vx", "vy", "vz")]
    old.append(np.asfortranarray(rng.integers(0, 8, size=(nx, ny, nz)).astype(dtype)))
    return old, 0.125, dict(dx=0.125, dy=0.125, dz=0.125)


def start_case(T):
    """The reference's own first step: a uniform stream Vx = vin, Vy = Vz = 0, dt = dx/vin, dx = 1/63, a seeded tracer — δ_x sits ON
    the integer 1, the discontinuity of floor(ix − δ) and of the weight (δ>0) − δ%1 (at δ = 1 exactly the reference's interpolant
    is A_o[ix]; a hair to either side it is ≈ A_o[ix−1]).  STRICT forms δ = RN(RN(dt·v)/dx); FAST forms RN(RN(dt·v)·RN(1/dx)), a
    product of two roundings that no contraction can change, so its δ is known here.  What a contraction CAN change is the floor's
    operand: ix − δ may be evaluated as fma(−dt·v, 1/dx, ix).  δ_y = δ_z = 0 exactly (weight 0 keeps the first operand), so the
    tracer's interpolant is one lerp in x.  Returns (old fields, pre-filled outputs, dt, spacings, STRICT's δ, FAST's δ, the pair
    interpolants of C for FAST's δ with the floor's operand rounded twice / once)."""
    import fractions
    from util import rnd
    nx, ny, nz = 63, 38, 38
    vin, dx, dy, dz = 1.0, 1.0 / 63, 0.6 / 38, 0.6 / 38
    dt = dx / vin
    a = T(dt) * T(vin)                                                    # dt·v
    rdx = T(1) / T(dx)
    d_strict, d_fast = a / T(dx), a * rdx
    Vx = np.asfortranarray(np.full((nx + 1, ny, nz), vin, dtype=T))
    Vy, Vz = np.zeros((nx, ny + 1, nz), dtype=T, order="F"), np.zeros((nx, ny, nz + 1), dtype=T, order="F")
    Cf = rnd(63, (nx, ny, nz), T)
    old = [Vx, Vy, Vz, Cf]
    prefill = [rnd(70 + q, b.shape, T) for q, b in enumerate(old)]
    ix = np.arange(1, nx + 1)
    w = T(1.0 if d_fast > 0 else 0.0) - np.fmod(d_fast, T(1))
    once = [T(float(fractions.Fraction(int(i)) - fractions.Fraction(float(a)) * fractions.Fraction(float(rdx)))) for i in ix]
    cands = []
    for p in (ix.astype(T) - d_fast, np.array(once, dtype=T)):
        i1 = np.clip(np.floor(p.astype(np.float64)).astype(np.int64), 1, nx)
        i2 = np.clip(i1 + 1, 1, nx)
        A, wp = RE.field(Cf), RE.Pair(float(w), None, RE.unit(T))
        cands.append(A[i2 - 1] * wp + A[i1 - 1] * (1 - wp))             # numpy_ref._lerp
    return old, prefill, dt, dict(dx=dx, dy=dy, dz=dz), d_strict, d_fast, cands


def start_check(C_got, cands, T):
    """None, or (index, value, candidate values) of the first entry of C that is neither candidate within the bound"""
    g64 = np.asarray(C_got, dtype=np.float64)
    ok = np.zeros(g64.shape, dtype=bool)
    for c in cands:
        ok |= np.abs(g64 - c.v) <= RE.allowed(T) * c.e
    bad = np.argwhere(~ok)
    if not len(bad):
        return None
    i = tuple(int(x) for x in bad[0])
    return i, float(g64[i]), float(cands[0].v[i]), float(cands[1].v[i])
