"""Stream order on streams that nothing serialises: every entry point of navierstokes3d_amd.kernels on (a) a torch stream the context
is pinned to, (b) the context's own stream and (c) the CU-masked stream of reserve_cus(64), with inputs that arrive LATE on that
stream and a reader and an overwrite that follow EARLY on it (tests/stream_order.py has the technique).  PyTorch's current stream stays
the null stream throughout and nothing but the stream under test is synchronised, so a kernel on the wrong stream, a missing fence, a
scratch buffer refilled too soon or a fill on another stream shows as wrong bits.

Expected bits: the same call of a plain synchronous context of the same mode on the null stream — the path every other file of the
suite pins to the oracle.  The comparison is bit equality; there is no tolerance in this file.

Calls that block on an asynchronous context (the table beside NS3D_ASYNC in include/ns3d.h) take their canary BEFORE the call,
calls that only enqueue take it AFTER: for those it also proves that the call returned while the stream was still busy.  pt_iterate
blocks exactly when its block runs as the cooperative launch (persist mode 1 here), poisson_direct only while it builds a plan; both are
run with the canary before the call, which is valid for either behaviour.

Every case runs in both variants: the early reader, and "sync" (nothing follows the call but Context.sync()).
Canary and control streams are chosen with stream_order.independent_stream: streams share hardware queues, and a canary that queues
up behind the delay would report every delay as too short.

diag.py has no device calls: the monitor is called directly."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stream_order as SO
from util import fields, geometry, rnd

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
DTS = ["f64", "f32"]
KINDS = ["torch", "own", "masked"]
GRIDS = [(24, 15, 15), (70, 6, 7)]
GID = lambda n: "%dx%dx%d" % tuple(n)


@pytest.fixture(scope="module")
def delay(hip):
    d = SO.Delay()
    print("stream-order delay: %.1f ms = %d in-place adds of %.4f ms on %d MiB" % (d.ms, d.n, d.op_ms, SO.DELAY_BYTES >> 20))
    return d


def run_case(hip, case, kind, delay, mode="strict", variants=("reader", "sync"), cold=False):
    """expected bits, warm-up, the measured variants on an asynchronous context of `kind`; returns the complaints.  cold: the
    warm-up (modules, process-wide plans) is made on ANOTHER context of the same kind and every variant gets a fresh one, so that
    whatever the context allocates, plans or frees lazily happens inside the measured call."""
    (want_r, want), (dec_r, dec) = SO.expected(hip, case, mode)
    msgs = []
    ctx = None
    for v in variants:
        if ctx is None or cold:
            if ctx is not None:
                ctx.close()
            if cold:
                other, _ = SO.context_on(hip, kind, mode)
                if case.setup:
                    case.setup(other)
                SO.warm_up(hip, case, other)
                other.close()
            ctx, S = SO.context_on(hip, kind, mode)
            if case.setup:
                case.setup(ctx)
            if not cold:
                SO.warm_up(hip, case, ctx)
        r, got, can = SO.measured(hip, case, ctx, S, delay, v)
        msgs += SO.verdict("%s on %s, %s, %s" % (case.name, kind, mode, v), got, want, dec, can, case.decoy, r, want_r, dec_r)
    ctx.close()
    return msgs


def run_cases(hip, cases, kind, delay, mode="strict", cold=False):
    msgs = []
    for case in cases:
        msgs += run_case(hip, case, kind, delay, mode, cold=cold)
    assert not msgs, "\n".join(msgs)


def _named(kinds):
    return ["%s%d" % (k, q) for q, k in enumerate(kinds)]


# ---- 1. the elementary kernels, the boundary sequences, set_cylinder!, max_abs, residual_max ---------------------------------------
def _elementary_case(name, grid, dt):
    from test_gpu_footprint import ELEMENTARY
    row = ELEMENTARY[name]
    g = geometry(*grid)
    names = _named(row["kinds"])
    host = fields(*grid, row["kinds"], 1, NP[dt])
    return SO.Case("%s %s %s" % (name, GID(grid), dt), [(n, a, "field") for n, a in zip(names, host)],
                   lambda hip, ctx, t: row["call"](hip, ctx, [t[n] for n in names], g, grid), blocking=name in ("max_abs", "residual_max"))


def _elementary_names():
    from test_gpu_footprint import BC_SEQUENCES, ELEMENTARY
    return [k for k in ELEMENTARY if k not in BC_SEQUENCES], list(BC_SEQUENCES)


EL_NAMES, BC_NAMES = _elementary_names()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", EL_NAMES)
def test_elementary(hip, delay, name, dt, kind):
    run_cases(hip, [_elementary_case(name, grid, dt) for grid in GRIDS], kind, delay)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", BC_NAMES)
def test_bc_sequences(hip, delay, name, dt, kind, fused, monkeypatch):
    monkeypatch.setenv("NS3D_BC_FUSED", fused)
    run_cases(hip, [_elementary_case(name, grid, dt) for grid in GRIDS], kind, delay)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_max_abs_lengths(hip, delay, dt, kind):
    """one element, one more than a wave, one more than sixteen workgroups"""
    cases = [SO.Case("max_abs n=%d %s" % (n, dt), [("A", rnd(5 + n, (n, 1, 1), NP[dt]), "field")], lambda hip, ctx, t: hip.max_abs(t["A"], ctx=ctx),
                     blocking=True) for n in (1, 65, 4097)]
    run_cases(hip, cases, kind, delay)


# ---- 2. predict_fused, advect, copy_advect ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
def test_predict_fused(hip, delay, dt, mode, kind):
    cases = []
    for grid in GRIDS:
        g = geometry(*grid)
        V = fields(*grid, ["vx", "vy", "vz"], 5, NP[dt])
        arrays = [("V%s_new" % c, np.full_like(a, 777.0), "field") for c, a in zip("xyz", V)] + [("V%s" % c, a, "field") for c, a in zip("xyz", V)]
        cases.append(SO.Case("predict_fused %s %s" % (GID(grid), dt), arrays,
                             lambda hip, ctx, t, g=g: hip.predict_fused(t["Vx_new"], t["Vy_new"], t["Vz_new"], t["Vx"], t["Vy"], t["Vz"], g["mu"], g["rho"],
                                                                        g["g"], g["dt"], g["dx"], g["dy"], g["dz"], ctx=ctx)))
    run_cases(hip, cases, kind, delay, mode)


def _advect_cases(entry, grid, cfl, dt):
    g = geometry(*grid)
    step = cfl * min(g["dx"], g["dy"], g["dz"])
    names = ("Vx", "Vy", "Vz", "C")
    old = fields(*grid, ["vx", "vy", "vz", "c"], 21, NP[dt])
    what = "%s %s cfl %g %s" % (entry, GID(grid), cfl, dt)
    if entry == "advect":
        new = fields(*grid, ["vx", "vy", "vz", "c"], 31, NP[dt])
        arrays = [(n, a, "field") for n, a in zip(names, new)] + [(n + "_o", a, "field") for n, a in zip(names, old)]
        return SO.Case(what, arrays, lambda hip, ctx, t: hip.advect(t["Vx"], t["Vx_o"], t["Vy"], t["Vy_o"], t["Vz"], t["Vz_o"], t["C"], t["C_o"], step,
                                                                    g["dx"], g["dy"], g["dz"], True, ctx=ctx))
    arrays = [(n + "_new", np.full_like(a, 777.0), "field") for n, a in zip(names, old)] + [(n, a, "field") for n, a in zip(names, old)]
    return SO.Case(what, arrays, lambda hip, ctx, t: hip.copy_advect(t["Vx_new"], t["Vx"], t["Vy_new"], t["Vy"], t["Vz_new"], t["Vz"], t["C_new"], t["C"],
                                                                     step, g["dx"], g["dy"], g["dz"], True, ctx=ctx))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("entry", ["advect", "copy_advect"])
def test_advect(hip, delay, entry, dt, mode, form, kind, monkeypatch):
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    run_cases(hip, [_advect_cases(entry, grid, cfl, dt) for grid in GRIDS for cfl in (0.9, 2.7)], kind, delay, mode)


MC_NEW, MC_OLD, MC_HAT = ("Vx_new", "Vy_new", "Vz_new", "C_new"), ("Vx", "Vy", "Vz", "C"), ("Vx_hat", "Vy_hat", "Vz_hat", "C_hat")


def _mc_cases(entry, grid, cfl, dt):
    """the limited MacCormack advection: "advect_mc" — one call, outputs and hat arrays over a fill; "chain" — copy_advect(faithful=0)
    into the hat arrays, then advect_correct, whose hat inputs are what the first call has only just enqueued; "correct" —
    advect_correct alone, its hat inputs (stage 1 of the old fields, tests/advect_mc_ref.py) arriving late with the old fields"""
    import advect_mc_ref as MC
    g = geometry(*grid)
    step = cfl * min(g["dx"], g["dy"], g["dz"])
    old = fields(*grid, ["vx", "vy", "vz", "c"], 41, NP[dt])
    hat = MC.stage1(old, step, g["dx"], g["dy"], g["dz"]) if entry == "correct" else [np.full_like(a, 555.0) for a in old]
    arrays = [(n, np.full_like(a, 777.0), "field") for n, a in zip(MC_NEW, old)] + [(n, a, "field") for n, a in zip(MC_OLD, old)] + \
             [(n, a, "field") for n, a in zip(MC_HAT, hat)]
    trios = lambda t: [t[n] for trio in zip(MC_NEW, MC_OLD, MC_HAT) for n in trio]

    def call(hip, ctx, t):
        if entry == "chain":
            hip.copy_advect(t["Vx_hat"], t["Vx"], t["Vy_hat"], t["Vy"], t["Vz_hat"], t["Vz"], t["C_hat"], t["C"], step, g["dx"], g["dy"], g["dz"],
                            False, ctx=ctx)
        getattr(hip, "advect_mc" if entry == "advect_mc" else "advect_correct")(*trios(t), step, g["dx"], g["dy"], g["dz"], ctx=ctx)
    return SO.Case("%s %s cfl %g %s" % (entry, GID(grid), cfl, dt), arrays, call)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["windowed", "global"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("entry", ["advect_mc", "chain", "correct"])
def test_advect_mc(hip, delay, entry, dt, form, kind, monkeypatch):
    """late inputs, an early reader and an overwrite behind the call(s) on every kind of stream; 70×6×7 at cfl 2.7 (departures up to
    three cells away, clamped at the thin walls) and 24×15×15 at cfl 0.9"""
    if form == "global":
        monkeypatch.setenv("NS3D_ADVECT_GLOBAL", "1")
    else:
        monkeypatch.delenv("NS3D_ADVECT_GLOBAL", raising=False)
    cases = [_mc_cases(entry, (70, 6, 7), 2.7, dt), _mc_cases(entry, (24, 15, 15), 0.9, dt)]
    if entry == "correct":
        for c in cases:                  # the late hat inputs are what they claim to be: another field than the old one
            assert not any(np.array_equal(c.real[h], c.real[o]) for h, o in zip(MC_HAT, MC_OLD))
    run_cases(hip, cases, kind, delay)


# ---- 3. the observers: vortex, sample, tracers_advance, the statistics --------------------------------------------------------------
def _vortex_case(grid, dt):
    import vortex_ref as VR
    g = geometry(*grid)
    V = fields(*grid, ("vx", "vy", "vz"), seed0=3, dtype=NP[dt])
    arrays = [(nm, np.full(grid, 777.0, dtype=NP[dt], order="F"), "field") for nm in VR.NAMES] + [(k, a, "field") for k, a in zip(("Vx", "Vy", "Vz"), V)]
    return SO.Case("vortex %s %s" % (GID(grid), dt), arrays,
                   lambda hip, ctx, t: hip.vortex(t["Vx"], t["Vy"], t["Vz"], g["dx"], g["dy"], g["dz"], ctx=ctx, **{nm: t[nm] for nm in VR.NAMES}))


N_POINTS = 300


def _sample_case(grid, dt, layout=0):
    import test_gpu_tracers as TT
    kind, stag = TT.LAYOUTS[layout]
    X, state = TT.points(grid, N_POINTS)
    A = fields(*grid, (kind,), seed0=9, dtype=NP[dt])[0]
    arrays = [("out", np.full(N_POINTS, 777.0), "field"), ("X", X, ("points", grid)), ("state", state, "state"), ("A", A, "field")]
    return SO.Case("sample %s %s %s" % (kind, GID(grid), dt), arrays,
                   lambda hip, ctx, t: hip.sample(t["A"], t["X"], t["out"], state=t["state"], stagger=stag, ctx=ctx))


def _advance_case(grid, dt):
    import test_gpu_tracers as TT
    X, state = TT.points(grid, N_POINTS)
    V = TT.velocity_fields(grid, dt)
    arrays = [("X", X, ("points", grid)), ("state", state, "state"), ("U", np.full((3, N_POINTS), 777.0), "field")]
    arrays += [(k, a, "field") for k, a in zip(("Vx", "Vy", "Vz"), V)]
    return SO.Case("tracers_advance %s %s" % (GID(grid), dt), arrays,
                   lambda hip, ctx, t: hip.tracers_advance(t["X"], t["state"], t["Vx"], t["Vy"], t["Vz"], *TT.SMALL, U=t["U"], ctx=ctx))


def _stats_case(grid, dt):
    import test_gpu_stats as TS
    samples, _, _ = TS.case(grid, dt)
    cells = grid[0] * grid[1] * grid[2]
    arrays = [("S", np.full(11 * cells, 777.0), "field"), ("mean", np.full(4 * cells, 777.0), "field"), ("rs", np.full(7 * cells, 777.0), "field")]
    for q, F in enumerate(samples):
        arrays += [("%s%d" % (k, q), a, "field") for k, a in zip(("Vx", "Vy", "Vz", "Pr"), F)]

    def call(hip, ctx, t):
        hip.stats_reset(t["S"], grid, ctx=ctx)
        for q, wgt in enumerate(TS.WEIGHTS):
            hip.stats_accumulate(t["S"], t["Vx%d" % q], t["Vy%d" % q], t["Vz%d" % q], t["Pr%d" % q], wgt, ctx=ctx)
        hip.stats_finalize(t["S"], TS.WSUM, t["mean"], t["rs"], grid, ctx=ctx)
    return SO.Case("stats_reset, 3 x stats_accumulate, stats_finalize %s %s" % (GID(grid), dt), arrays, call)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("what", ["vortex", "sample", "sample_vx", "tracers_advance", "stats"])
def test_observers(hip, delay, what, dt, kind):
    make = {"vortex": _vortex_case, "sample": _sample_case, "sample_vx": lambda n, d: _sample_case(n, d, 1), "tracers_advance": _advance_case,
            "stats": _stats_case}[what]
    run_cases(hip, [make(grid, dt) for grid in GRIDS], kind, delay)


# ---- 4. the PT family ------------------------------------------------------------------------------------------------------------------
RULE = (0, True, 0.25)


def _pt_host(grid, dt, seed=71, scale=1.0):
    Pr0, d0, rhs = fields(*grid, ["c", "i", "c"], seed, NP[dt])
    return Pr0, d0, np.asfortranarray(rhs * NP[dt](scale))


def _ptp(hip, grid, rule=RULE):
    from test_gpu_pt import _params
    return _params(hip, SimpleNamespace(shape=grid), geometry(*grid), *rule)


def _sweep_case(family, nlev, grid, dt):
    Pr0, d0, rhs = _pt_host(grid, dt)
    nz = grid[2]
    if family == "sweep":
        arrays = [("Pr_out", np.full_like(Pr0, 555.0), "field"), ("Pr_in", Pr0, "field"), ("d_out", d0, "field"), ("rhs", rhs, "field")]
        call = lambda hip, ctx, t: hip.pt_sweep(t["Pr_in"], t["Pr_out"], t["d_out"], t["rhs"], _ptp(hip, grid), 1, nz - 1, ctx=ctx)
    else:
        arrays = [("Pr_out", np.full_like(Pr0, 555.0), "field"), ("Pr_in", Pr0, "field"), ("d_out", np.full_like(d0, 444.0), "field"),
                  ("d_in", d0, "field"), ("rhs", rhs, "field")]
        if family == "sweep2":
            call = lambda hip, ctx, t: hip.pt_sweep2(t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], _ptp(hip, grid), ctx=ctx)
        else:
            call = lambda hip, ctx, t: hip.pt_sweepn(nlev, t["Pr_in"], t["Pr_out"], t["d_in"], t["d_out"], t["rhs"], _ptp(hip, grid), ctx=ctx)
    return SO.Case("pt_%s levels %d %s %s" % (family, nlev, GID(grid), dt), arrays, call)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("family,nlev", [("sweep", 1), ("sweep2", 2), ("sweepn", 3), ("sweepn", 4)])
def test_pt_sweeps(hip, delay, family, nlev, dt, mode, kind):
    run_cases(hip, [_sweep_case(family, nlev, grid, dt) for grid in GRIDS], kind, delay, mode)


def _iterate_case(grid, dt, n, depth, persist):
    Pr0, d0, rhs = _pt_host(grid, dt, 73, 1e-3)

    def setup(ctx):
        ctx.set_persist_mode(persist)
        ctx.set_pt_depth(depth)
    return SO.Case("pt_iterate n=%d depth %d persist %d %s %s" % (n, depth, persist, GID(grid), dt),
                   [("Pr", Pr0, "field"), ("d", d0, "field"), ("rhs", rhs, "field")],
                   lambda hip, ctx, t: hip.pt_iterate(t["Pr"], t["d"], t["rhs"], _ptp(hip, grid), n, ctx=ctx), blocking=persist != 0, setup=setup)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("persist", [0, 1])
def test_pt_iterate(hip, delay, persist, dt, mode, kind):
    """the copy back from the ping-pong buffers (n = 9 is odd) and the hand-over of the cooperative launch, at every depth"""
    depths = (0, 1, 2, 3) if dt == "f64" else (0, 1, 2, 3, 5)
    run_cases(hip, [_iterate_case(grid, dt, 9, depth, persist) for depth in depths for grid in GRIDS], kind, delay, mode)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_pt_iterate_back_to_back(hip, delay, dt, kind):
    """n = 3, then n = 4 on other arrays, with nothing between them: the second call reuses the ping-pong buffers the first one's
    copy back still reads"""
    grid = GRIDS[0]
    a, b = _pt_host(grid, dt, 73, 1e-3), _pt_host(grid, dt, 83, 1e-3)
    arrays = [(n + "_a", x, "field") for n, x in zip(("Pr", "d", "rhs"), a)] + [(n + "_b", x, "field") for n, x in zip(("Pr", "d", "rhs"), b)]

    def call(hip, ctx, t):
        hip.pt_iterate(t["Pr_a"], t["d_a"], t["rhs_a"], _ptp(hip, grid), 3, ctx=ctx)
        hip.pt_iterate(t["Pr_b"], t["d_b"], t["rhs_b"], _ptp(hip, grid), 4, ctx=ctx)
    run_cases(hip, [SO.Case("pt_iterate 3 then 4 %s" % dt, arrays, call, setup=lambda ctx: ctx.set_persist_mode(0))], kind, delay)


def _solve_case(grid, dt, nchk, graph, persist):
    Pr0, d0, rhs = _pt_host(grid, dt, 73, 1e-3)

    def setup(ctx):
        ctx.set_persist_mode(persist)
        ctx.set_graph_mode(graph)
    return SO.Case("pt_solve nchk %d graph %d persist %d %s %s" % (nchk, graph, persist, GID(grid), dt),
                   [("Pr", Pr0, "field"), ("d", d0, "field"), ("rhs", rhs, "field")],
                   lambda hip, ctx, t: hip.pt_solve(t["Pr"], t["d"], t["rhs"], _ptp(hip, grid), 1e-30, 45, nchk, 0.36, 1000.0, ctx=ctx),
                   blocking=True, setup=setup)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("whole", ["1", "0"])
@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("graph", [0, 1])
def test_pt_solve(hip, delay, graph, persist, whole, kind, monkeypatch):
    """graph 1 on a non-null stream is the capture WITHOUT the detour through the context's own stream and its fence; the iteration
    count and the residual history are compared as well as the arrays the final copies fill"""
    monkeypatch.setenv("NS3D_PERSIST_SOLVE", whole)
    plan = [(GRIDS[0], "f64", "strict", 7), (GRIDS[1], "f64", "strict", 0), (GRIDS[1], "f32", "strict", 7), (GRIDS[0], "f64", "fast", 7),
            (GRIDS[0], "f32", "fast", 0)]
    msgs = []
    for grid, dt, mode, nchk in plan:
        msgs += run_case(hip, _solve_case(grid, dt, nchk, graph, persist), kind, delay, mode)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rule", [(0, True, 0.75), (1, False, 0.0)], ids=str)
def test_poisson_direct(hip, delay, rule, dt, kind):
    cases = []
    for grid in [(34, 18, 18), (20, 12, 6)]:
        rhs = fields(*grid, ["c"], 57, NP[dt])[0]
        Pr0, d0 = fields(*grid, ["c"], 3, NP[dt])[0], fields(*grid, ["i"], 4, NP[dt])[0]
        cases.append(SO.Case("poisson_direct %s %r %s" % (GID(grid), rule, dt), [("Pr", Pr0, "field"), ("d", d0, "field"), ("rhs", rhs, "field")],
                             lambda hip, ctx, t, grid=grid: hip.poisson_direct(t["Pr"], t["d"], t["rhs"], _ptp(hip, grid, rule), ctx=ctx), blocking=True))
    run_cases(hip, cases, kind, delay)


# ---- 5. calls that return host values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["multi", "gpu"])
def test_diagnostics(hip, delay, form, dt, kind):
    from test_gpu_diagnostics import _cyl
    cases = []
    for n in GRIDS:
        g = geometry(*n)
        F = fields(*n, ["vx", "vy", "vz", "c", "c"], 11, NP[dt])
        cyl = _cyl(form, n[0], n[1], g)
        cases.append(SO.Case("diagnostics %s %s %s" % (form, GID(n), dt), [(k, a, "field") for k, a in zip(("Vx", "Vy", "Vz", "Pr", "C"), F)],
                             lambda hip, ctx, t, n=n, g=g, cyl=cyl: hip.diagnostics(
                                 t["Vx"], t["Vy"], t["Vz"], t["Pr"], t["C"], hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=cyl), ctx=ctx),
                             blocking=True))
    run_cases(hip, cases, kind, delay)


ISO_GRID, ISO_LEVEL = (17, 9, 5), 0.1


@functools.lru_cache(maxsize=None)
def _iso_fields(dt):
    import isosurface_ref as IR
    A, B = rnd(11, ISO_GRID, NP[dt]), rnd(21, ISO_GRID, NP[dt])
    tri, _ = IR.reference(A, ISO_LEVEL, B, None, None)
    return A, B, int(tri.shape[0])


def _iso_case(dt, fill, color):
    A, B, nref = _iso_fields(dt)
    cap = nref + 7 if fill else 0
    arrays = [("A", A, "field")] + ([("B", B, "field")] if color else [])
    if fill:
        arrays += [("tri", np.full(9 * cap, 777.0), "field")] + ([("val", np.full(3 * cap, 777.0), "field")] if color else [])
    return SO.Case("isosurface %s%s %s" % ("filling" if fill else "count", " coloured" if color else "", dt), arrays,
                   lambda hip, ctx, t: hip.isosurface(t["A"], ISO_LEVEL, color=t.get("B"), tri=t.get("tri"), val=t.get("val"), cap=cap, ctx=ctx), blocking=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_isosurface(hip, delay, dt, kind):
    """the emit launch follows the count's read-back: its triangles must be there for a reader on the stream"""
    run_cases(hip, [_iso_case(dt, fill, color) for fill in (True, False) for color in (True, False)], kind, delay)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_shared_read_backs(hip, delay, dt, kind):
    """max_abs, residual_max, the isosurface count and max_abs again share one device word and one pinned host word; back to back,
    nothing between them: each value is its synchronous one"""
    grid = GRIDS[0]
    A, B, Pr, rhs = fields(*grid, ["c", "vx", "c", "c"], 91, NP[dt])
    isoA = rnd(11, ISO_GRID, NP[dt])
    arrays = [("A", A, "field"), ("B", B, "field"), ("Pr", Pr, "field"), ("rhs", rhs, "field"), ("isoA", isoA, "field")]

    def call(hip, ctx, t):
        return (hip.max_abs(t["A"], ctx=ctx), hip.residual_max(t["Pr"], t["rhs"], _ptp(hip, grid), ctx=ctx),
                hip.isosurface(t["isoA"], ISO_LEVEL, ctx=ctx), hip.max_abs(t["B"], ctx=ctx))
    run_cases(hip, [SO.Case("max_abs, residual_max, isosurface count, max_abs %s" % dt, arrays, call, blocking=True)], kind, delay)


# ---- 5b. a whole time step in one call ------------------------------------------------------------------------------------------------
def _step_case(script, pressure, advection="reference", obstacle=False):
    """two ns3d_time_step calls from the driver's own initial state at 24×15×15 (tests/test_gpu_footprint.py::_two_steps_on), fp64;
    the decoy is a gentle flow (magnitude 1e-2), so that a step taken on it stays finite.  advection="maccormack": the knob on (on
    every context the case runs on) and faithful = 0; the second step's stage 1 refills the hat scratch the first step's stage 2 read.
    obstacle: the scenario of tests/solid_step_cases.py instead — its state, its body's mask as one more late input (ns3d_set_solid
    before multi.jl's loop, ns3d_set_obstacle for the steps, the knob put back behind them), 3·nchk iterations, faithful = 0; the
    mask's decoy holds C bits only, so the decoy run masks no velocity"""
    from navierstokes3d_amd import driver as Dr, lib as L
    from navierstokes3d_amd.params import gpu_params, multi_params
    from test_gpu_footprint import STEP_SHAPES
    from util import SHAPES
    p = multi_params(24) if script == "multi" else gpu_params(24)
    n = (p.nx, p.ny, p.nz)
    assert n == (24, 15, 15)
    host = {k: np.zeros(SHAPES[kind](*n), dtype=np.float64, order="F") for k, kind in STEP_SHAPES.items()}
    if script == "multi":
        host["Vy"][0, :, :] = p.vin
    else:
        Vx0, Pr0 = Dr.gpu_initial_fields(p)
        host["Vx"], host["Pr"] = np.asfortranarray(Vx0), np.asfortranarray(Pr0)
    extra = []
    if obstacle:
        import solid_step_cases as SS
        sc = SS.scenario(script, "f64")
        for k, a in sc.initial.items():
            host[k] = np.asfortranarray(a.copy())
        extra = [("mask", np.asfortranarray(sc.mask), "state")]
    common = dict(nx=p.nx, ny=p.ny, nz=p.nz, mu=p.mu, rho=p.rho, g=p.g, dt=p.dt, dtau=p.dtau, damp=p.damp, dx=p.dx, dy=p.dy, dz=p.dz,
                  eps=p.eps, niter=sc.niter if obstacle else p.niter, nchk=p.nchk, err_mul=p.ly * p.ly, err_div=p.psc, a2=p.a2, b2=p.b2,
                  ox=p.ox, oy=p.oy, sinb=p.sinb, cosb=p.cosb, lx=p.lx, ly=p.ly, lz=p.lz,
                  faithful=0 if advection == "maccormack" or obstacle else 1, pressure=pressure, write_stress=0)

    def call(hip, ctx, t):
        if not obstacle:
            return steps(hip, ctx, t)
        try:
            return steps(hip, ctx, t)
        finally:
            ctx.set_obstacle(None)          # the knob never outlives the case's mask

    def steps(hip, ctx, t):
        assert ctx.advection() == advection and ctx.obstacle() is None
        t = dict(t)
        mask = t.pop("mask", None)
        f = SimpleNamespace(**t)
        if script == "multi":
            if obstacle:
                hip.set_solid(f.C, f.Vx, f.Vy, f.Vz, mask, ctx=ctx)
            else:
                hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly,
                                 p.lz, p.dx, p.dy, p.dz, ctx=ctx)
            sp = L.StepParams(script=L.NS3D_BC_MULTI, xco_g=p.xco_g, yco_g=p.yco_g, zco_g=p.zco_g, owns_inlet=int(bool(p.owns_inlet)),
                              owns_outlet=int(bool(p.owns_outlet)), vin=p.vin, **common)
        else:
            sp = L.StepParams(script=L.NS3D_BC_GPU, xco_g=0.0, yco_g=0.0, zco_g=0.0, owns_inlet=0, owns_outlet=0, vin=0.0, **common)
        if obstacle:
            ctx.set_obstacle(mask)
        out = []
        for step in (1, 2):
            sp.write_stress = 1 if step == 2 else 0
            out.append(hip.time_step(f, sp, ctx=ctx))
        return out
    return SO.Case("time_step %s pressure %d%s%s" % (script, pressure, "" if advection == "reference" else " " + advection,
                                                     " obstacle" if obstacle else ""),
                   [(k, a, ("field", 1e-2)) for k, a in host.items()] + extra, call, blocking=True,
                   setup=lambda ctx: ctx.set_advection(advection))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pressure", [0, 1])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step(hip, delay, script, pressure, kind, advection="reference", obstacle=False):
    """Two steps, every array of ns3d_step_fields (the arrays are compared by buffer: the step swaps roles, the same way in every
    run), iteration counts and residual histories.  pressure 1 reads its one residual back through the shared key word behind the
    rest of the step; the second step's start must not disturb it."""
    case = _step_case(script, pressure, advection, obstacle)
    (want_r, want), _ = SO.expected(hip, case)
    assert all(len(errs) > 0 for _, errs in want_r) and (pressure == 1 or all(it > 0 for it, _ in want_r)), want_r
    assert all(np.isfinite(a).all() for a in want.values()) and np.abs(want["Pr"]).max() > 0
    run_cases(hip, [case], kind, delay)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pressure", [0, 1])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_maccormack(hip, delay, script, pressure, kind):
    """test_time_step over the other value of its `advection` parameter (a test of its own: the existing cases keep their names).
    The scheme is another one: the expected bits differ from the reference step's."""
    test_time_step(hip, delay, script, pressure, kind, "maccormack")
    (_, mc), _ = SO.expected(hip, _step_case(script, pressure, "maccormack"))
    (_, ref), _ = SO.expected(hip, _step_case(script, pressure))
    assert not np.array_equal(mc["Vx"], ref["Vx"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pressure", [0, 1])
@pytest.mark.parametrize("script", ["multi", "gpu"])
def test_time_step_obstacle(hip, oracle, delay, script, pressure, kind):
    """test_time_step with ns3d_set_obstacle: the mask is one more late input — of ns3d_set_solid before multi.jl's loop and of both
    maskings of each step — and its bytes come back unchanged (a test of its own: the existing cases keep their names).  With the PT
    solve the expected bits are the oracle driver's with obstacle=; a step that read the decoy's mask cannot return them."""
    import solid_step_cases as SS
    test_time_step(hip, delay, script, pressure, kind, obstacle=True)
    case = _step_case(script, pressure, obstacle=True)
    (want_r, want), (_, dec) = SO.expected(hip, case)
    assert np.array_equal(want["mask"], SS.body_mask()) and not np.array_equal(dec["Vx"], want["Vx"])
    if pressure == 0:
        ref, info = SS.scenario_ref(script, "f64")
        assert [it for it, _ in want_r] == info.iters and all(np.array_equal(np.float64(a[1]), np.float64(b)) for a, b in zip(want_r, info.errs))
        for k in ("Pr", "dPrdtau", "divV"):
            assert np.array_equal(want[k], ref[k]), k
        # the step swaps roles: after two steps every swapped name is back on its own buffer
        for k in ("C", "Vx", "Vy", "Vz", "C_o", "Vx_o", "Vy_o", "Vz_o"):
            assert np.array_equal(want[k], ref[k]), k


# ---- 5c. the lazy paths INSIDE the window: a cold context, nothing warmed up on it ----------------------------------------------------------
BIG = (40, 17, 16)                  # more cells than either grid of GRIDS in every scratch buffer's measure


def _pt_arrays(grid, dt, tag, seed):
    Pr0, d0, rhs = _pt_host(grid, dt, seed, 1e-3)
    return [("Pr_" + tag, Pr0, "field"), ("d_" + tag, d0, "field"), ("rhs_" + tag, rhs, "field")]


def _lazy_case(name, dt):
    small = GRIDS[0]
    if name.startswith("first_pt_iterate"):
        persist = int(name[-1])
        case = _iterate_case(small, dt, 9, 2, persist)
        return SO.Case("first " + case.name, case.arrays, case.call, blocking=True, setup=case.setup)
    if name == "pingpong_grows":
        arrays = _pt_arrays(small, dt, "a", 73) + _pt_arrays(BIG, dt, "b", 83)

        def call(hip, ctx, t):                # the first is queued behind the delay when the second frees the buffers it runs in
            hip.pt_iterate(t["Pr_a"], t["d_a"], t["rhs_a"], _ptp(hip, small), 9, ctx=ctx)
            hip.pt_iterate(t["Pr_b"], t["d_b"], t["rhs_b"], _ptp(hip, BIG), 9, ctx=ctx)

        def setup(ctx):
            ctx.set_persist_mode(0)
            ctx.set_pt_depth(2)
        return SO.Case("pt_iterate 24x15x15 then 40x17x16 %s" % dt, arrays, call, blocking=True, setup=setup)
    if name == "iso_grows":
        A, B, nref = _iso_fields(dt)
        cap = nref + 7
        A2 = rnd(31, BIG, NP[dt])
        arrays = [("A", A, "field"), ("B", B, "field"), ("tri", np.full(9 * cap, 777.0), "field"), ("val", np.full(3 * cap, 777.0), "field"),
                  ("A2", A2, "field")]

        def call(hip, ctx, t):                # the first call's emit launch reads the scratch the second call replaces
            return (hip.isosurface(t["A"], ISO_LEVEL, color=t["B"], tri=t["tri"], val=t["val"], cap=cap, ctx=ctx),
                    hip.isosurface(t["A2"], ISO_LEVEL, ctx=ctx))
        return SO.Case("isosurface 17x9x5 filling then 40x17x16 %s" % dt, arrays, call, blocking=True)
    if name == "diag_grows":
        arrays, gs = [], {}
        for tag, n in (("a", small), ("b", (131, 66, 37))):
            gs[tag] = (n, geometry(*n))
            arrays += [(k + "_" + tag, a, "field") for k, a in zip(("Vx", "Vy", "Vz", "Pr", "C"), fields(*n, ["vx", "vy", "vz", "c", "c"], 11, NP[dt]))]

        def call(hip, ctx, t):
            out = []
            for tag, (n, g) in gs.items():
                out.append(hip.diagnostics(*(t[k + "_" + tag] for k in ("Vx", "Vy", "Vz", "Pr", "C")),
                                           hip.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"]), ctx=ctx))
            return out
        return SO.Case("diagnostics 24x15x15 then 131x66x37 %s" % dt, arrays, call, blocking=True)
    if name == "direct_plan_replaced":
        ga, gb = (20, 12, 6), (34, 18, 18)
        arrays = []
        for tag, n in (("a", ga), ("b", gb)):
            arrays += [("Pr_" + tag, fields(*n, ["c"], 3, NP[dt])[0], "field"), ("d_" + tag, fields(*n, ["i"], 4, NP[dt])[0], "field"),
                       ("rhs_" + tag, fields(*n, ["c"], 57, NP[dt])[0], "field")]

        def call(hip, ctx, t):                # the first solve is queued behind the delay when the second releases the plan it uses
            hip.poisson_direct(t["Pr_a"], t["d_a"], t["rhs_a"], _ptp(hip, ga), ctx=ctx)
            hip.poisson_direct(t["Pr_b"], t["d_b"], t["rhs_b"], _ptp(hip, gb), ctx=ctx)
        return SO.Case("poisson_direct 20x12x6 then 34x18x18 %s" % dt, arrays, call, blocking=True)
    raise ValueError(name)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["first_pt_iterate_persist0", "first_pt_iterate_persist1", "pingpong_grows", "iso_grows", "diag_grows",
                                  "direct_plan_replaced"])
def test_lazy_paths_inside_the_window(hip, delay, name, dt, kind):
    """hipMalloc, hipFree, hipMemset and blocking hipMemcpy between work queued on a non-blocking stream: the context under test is
    cold (the warm-up runs on another context), the canary is taken before the call, and the scratch that grows belongs to a call that
    is still queued behind the delay."""
    run_cases(hip, [_lazy_case(name, dt)], kind, delay, cold=True)


# ---- 6. a whole unfused step as one chain ---------------------------------------------------------------------------------------------
CHAIN = {"txx": "c", "tyy": "c", "tzz": "c", "txy": "s", "txz": "s", "tyz": "s", "Vx": "vx", "Vy": "vy", "Vz": "vz", "divV": "c", "Pr": "c",
         "d": "i", "Vx_n": "vx", "Vy_n": "vy", "Vz_n": "vz", "C": "c", "C_n": "c"}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS)
def test_unfused_step_chain(hip, delay, dt, kind):
    """update_tau → predict_V → set_bc_Vel → update_divV → pt_iterate(20) → correct_V → set_bc_Vel → copy_advect → set_cylinder on the
    stream with no host synchronisation, against the same chain of a synchronous context (which waits after every call)"""
    from test_gpu_footprint import _cyl_scalars
    grid = GRIDS[0]
    g = geometry(*grid)
    host = fields(*grid, list(CHAIN.values()), 201, NP[dt])
    host = [np.asfortranarray(a * NP[dt](1e-2)) for a in host]
    cyl = _cyl_scalars(0.3, "glob", grid)

    def call(hip, ctx, t):
        hip.update_tau(t["txx"], t["tyy"], t["tzz"], t["txy"], t["txz"], t["tyz"], t["Vx"], t["Vy"], t["Vz"], g["mu"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        hip.predict_V(t["Vx"], t["Vy"], t["Vz"], t["txx"], t["tyy"], t["tzz"], t["txy"], t["txz"], t["tyz"], g["rho"], g["g"], g["dt"], g["dx"], g["dy"],
                      g["dz"], ctx=ctx)
        hip.set_bc_Vel_multi(t["Vx"], t["Vy"], t["Vz"], True, 1.5, ctx=ctx)
        hip.update_divV(t["divV"], t["Vx"], t["Vy"], t["Vz"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        hip.pt_iterate(t["Pr"], t["d"], t["divV"], _ptp(hip, grid), 20, ctx=ctx)
        hip.correct_V(t["Vx"], t["Vy"], t["Vz"], t["Pr"], g["dt"], g["rho"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        hip.set_bc_Vel_multi(t["Vx"], t["Vy"], t["Vz"], True, 1.5, ctx=ctx)
        hip.copy_advect(t["Vx_n"], t["Vx"], t["Vy_n"], t["Vy"], t["Vz_n"], t["Vz"], t["C_n"], t["C"], g["dt"], g["dx"], g["dy"], g["dz"], True, ctx=ctx)
        hip.set_cylinder(t["C_n"], t["Vx_n"], t["Vy_n"], t["Vz_n"], *cyl, ctx=ctx)
    case = SO.Case("unfused step chain %s" % dt, [(n, a, "field") for n, a in zip(CHAIN, host)], call, setup=lambda ctx: ctx.set_persist_mode(0))
    run_cases(hip, [case], kind, delay)


# ---- 7. negative controls and the synchronous promise -----------------------------------------------------------------------------------
CONTROLS = {"update_divV": lambda dt: _elementary_case("update_divV", GRIDS[0], dt), "vortex": lambda dt: _vortex_case(GRIDS[0], dt),
            "sample": lambda dt: _sample_case(GRIDS[0], dt)}


@pytest.mark.parametrize("name", list(CONTROLS))
def test_negative_control(hip, delay, name):
    """The harness sees a misordered launch: the context is put on ANOTHER non-blocking stream than the one that carries the delay
    and the copy-in, so its kernel runs at once, on the decoy — and the reader on that stream must find the decoy run's bits."""
    case = CONTROLS[name]("f64")
    _, (dec_r, dec) = SO.expected(hip, case)
    late = torch.cuda.Stream(0)
    ctx = hip.Context(0, "strict", async_=True)
    S = SO.independent_stream(late, delay)                 # the launch must be FREE to run early: not behind `late` in a hardware queue
    ctx.use_torch_stream(S, pin=True)
    SO.warm_up(hip, case, ctx)
    # the canary BEFORE the call: afterwards the outputs hold what the early launch made of the decoy, as they should here
    early = SO.Case(case.name + " (control)", case.arrays, case.call, blocking=True)
    r, got, can = SO.measured(hip, early, ctx, S, delay, "reader", delay_stream=late, overwrite=False)
    ctx.close()
    msgs = SO.verdict("control %s" % name, got, dec, None, can, case.decoy, r, dec_r)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("name", list(CONTROLS))
def test_synchronous_promise(hip, delay, name):
    """A context WITHOUT NS3D_ASYNC on a pinned non-null stream: the call itself waits, so another stream may read the outputs the
    moment it returns."""
    case = CONTROLS[name]("f64")
    (want_r, want), (dec_r, dec) = SO.expected(hip, case)
    ctx, S = SO.context_on(hip, "torch", async_=False)
    SO.warm_up(hip, case, ctx)
    blocking = SO.Case(case.name + " (blocking context)", case.arrays, case.call, blocking=True)
    r, got, can = SO.measured(hip, blocking, ctx, S, delay, "return")
    ctx.close()
    msgs = SO.verdict(blocking.name, got, want, dec, can, case.decoy, r, want_r, dec_r)
    assert not msgs, "\n".join(msgs)


# ---- 8. the Python wrappers on a pinned context ----------------------------------------------------------------------------------------
def _wrapper_fields(hip, grid, seed, dt="f64"):
    Vx, Vy, Vz, Pr, Cf = fields(*grid, ["vx", "vy", "vz", "c", "c"], seed, NP[dt])
    return SimpleNamespace(Vx=hip.from_numpy(Vx), Vy=hip.from_numpy(Vy), Vz=hip.from_numpy(Vz), Pr=hip.from_numpy(Pr), C=hip.from_numpy(Cf))


def _wrappers(hip, ctx, f, grid, before=lambda: None):
    """every wrapper's calls on the fields f; `before` runs ahead of each wrapper (the measured run enqueues its delay there).
    Returns {name: host array}."""
    from navierstokes3d_amd import isosurface as ISO, stats as ST, tracers as TRC, vortex as VX
    g = geometry(*grid)
    sp = (g["dx"], g["dy"], g["dz"])
    org = (-0.5, -0.3, -0.35)
    out = {}
    before()
    tr = TRC.Tracers(grid, ctx, sp, org, keep_velocity=True).seed_random(N_POINTS, seed=4)
    tr.advance(f, 0.4 * g["dx"])
    ctx.sync()
    out["tracers U"], out["tracers positions"], out["tracers alive"] = tr.U.cpu().numpy(), tr.positions(), tr.alive().astype(np.uint8)
    tr.state[::3] = 0                                                     # dead slots for reseed to fill
    torch.cuda.current_stream(0).synchronize()
    pts = np.stack([org[q] + rnd(50 + q, (40,), lo=0.05, hi=0.95) * grid[q] * sp[q] for q in range(3)], axis=1)
    before()
    placed = tr.reseed(pts)
    tr.advance(f, 0.4 * g["dx"])
    smp = tr.sample(f.Pr)
    ctx.sync()
    out["reseed placed"] = np.array([placed])
    out["reseed U"], out["reseed positions"], out["sample"] = tr.U.cpu().numpy(), tr.positions(), smp.cpu().numpy()
    before()
    pr = TRC.Probes(grid, ctx, sp, org, pts[:17], 3)
    for _ in range(3):
        pr.record(f)
    rec = pr.gathered()
    out.update({"probes " + k: getattr(rec, k) for k in ("u", "v", "w", "p")})
    before()
    surf = ISO.extract(ctx, f.Pr, 0.1, color=f.C)
    out["isosurface tri"], out["isosurface val"] = surf.tri_index, surf.val
    before()
    st = ST.RunningStats(grid, [ctx])
    for wgt in (1.0, 0.3, 3.0):
        st.sample([f], wgt)
    rec = st.local(0)
    out.update({"stats mean " + k: v for k, v in vars(rec.mean).items()})
    out.update({"stats rs " + k: v for k, v in vars(rec.rs).items()})
    before()
    vf = VX.VortexFields(grid, [ctx], sp)
    vf.compute([f])
    out.update({"vortex " + k: v for k, v in vars(vf.local(0)).items()})
    before()
    out["diagnostics"] = np.array([float(v) for v in _flat(vars(hip.diagnostics(f.Vx, f.Vy, f.Vz, f.Pr, None,
                                                                                hip.diag_params(*grid, *sp, g["rho"]), ctx=ctx)))])
    return out


def _flat(d):
    for v in d.values():
        if isinstance(v, (tuple, list)):
            yield from v
        else:
            yield v


@pytest.mark.parametrize("kind", KINDS)
def test_wrappers_on_a_pinned_context(hip, kind):
    """Tracers, Probes, isosurface.extract, RunningStats, VortexFields and the monitor on a context pinned to a stream of its own
    return the bits of an unpinned context.  No delay here: each wrapper's first upload (`.to(device)` of pageable memory) waits for
    PyTorch's stream, so a delay enqueued ahead of a wrapper is gone before its fills; the two tests below put the delay where
    the fills and the queued kernels are."""
    grid = GRIDS[0]
    f = _wrapper_fields(hip, grid, 61)
    torch.cuda.synchronize()
    plain = hip.Context(0, "strict")
    want = _wrappers(hip, plain, f, grid)
    plain.close()
    ctx, S = SO.context_on(hip, kind)
    got = _wrappers(hip, ctx, f, grid)
    ctx.close()
    bad = ["%s %s" % (k, SO.diagnose(got[k], want[k], None)) for k in want if not SO.bits_same(got[k], want[k])]
    assert not bad, "\n".join(bad)


def _fills_run(hip, ctx, f, grid, late=None):
    """Tracers(keep_velocity=True): seed_random → advance → U; Probes: three records → the series.  late: a context manager factory
    that makes torch.full_like / torch.full arrive late on PyTorch's current stream."""
    import contextlib
    from navierstokes3d_amd import tracers as TRC
    g = geometry(*grid)
    sp, org = (g["dx"], g["dy"], g["dz"]), (-0.5, -0.3, -0.35)
    pts = np.stack([org[q] + rnd(50 + q, (17,), lo=0.05, hi=0.95) * grid[q] * sp[q] for q in range(3)], axis=1)
    late = late or contextlib.nullcontext
    with late():
        tr = TRC.Tracers(grid, ctx, sp, org, keep_velocity=True).seed_random(N_POINTS, seed=4)
    tr.advance(f, 0.4 * g["dx"])
    with late():
        pr = TRC.Probes(grid, ctx, sp, org, pts, 3)
    for _ in range(3):
        pr.record(f)
    rec = pr.gathered()
    ctx.sync()
    torch.cuda.synchronize()
    out = {"tracers U": tr.U.cpu().numpy(), "tracers positions": tr.positions()}
    out.update({"probes " + k: getattr(rec, k) for k in ("u", "v", "w", "p")})
    return out


def fills_case(hip, delay, kind):
    """(complaints, canaries) of the fills test — a function of its own so that the fix can be shown to matter (with
    tracers._after_fill replaced by a no-op the bits come back NaN)"""
    import contextlib
    grid = GRIDS[0]
    f = _wrapper_fields(hip, grid, 61)
    torch.cuda.synchronize()
    plain = hip.Context(0, "strict")
    want = _fills_run(hip, plain, f, grid)
    plain.close()
    ctx, S = SO.context_on(hip, kind)
    _fills_run(hip, ctx, f, grid)                                        # warm-up
    pending = []

    @contextlib.contextmanager
    def late():
        originals = {nm: getattr(torch, nm) for nm in ("full_like", "full")}

        def behind_the_delay(orig):
            def fill(*a, **k):
                cur = torch.cuda.current_stream(0)
                delay.enqueue(cur)                                       # after the wrapper's blocking uploads, ahead of its fill
                out = orig(*a, **k)
                ev = torch.cuda.Event()
                ev.record(cur)
                pending.append(not ev.query())                           # the fill was enqueued while the stream was still busy
                return out
            return fill
        for nm, orig in originals.items():
            setattr(torch, nm, behind_the_delay(orig))
        try:
            yield
        finally:
            for nm, orig in originals.items():
                setattr(torch, nm, orig)
    got = _fills_run(hip, ctx, f, grid, late)
    ctx.close()
    return ["%s %s" % (k, SO.diagnose(got[k], want[k], None)) for k in want if not SO.bits_same(got[k], want[k])], pending


@pytest.mark.parametrize("kind", KINDS)
def test_wrapper_fills_land_before_a_pinned_contexts_kernels(hip, delay, kind):
    """The NaN fills of Tracers (U) and Probes (the series) run on PyTorch's current stream, the kernels that write those arrays on
    the pinned context's.  The delay is put between the wrapper's uploads and its fill (torch.full_like / torch.full are wrapped for
    the constructor's duration), so the fill is still queued when the constructor would return: a wrapper that does not wait lets
    advance / record run first and the late fill wipes their results.  The re-seeded slots' fill (`U[:, slots] = nan`) follows two
    blocking uploads and cannot be delayed this way: that one is ordered by reading only."""
    bad, pending = fills_case(hip, delay, kind)
    assert len(pending) >= 2 and all(pending), "delay too short: the case proves nothing (%r)" % (pending,)
    assert not bad, "\n".join(bad)


def _reseed_run(hip, ctx, f, grid, S=None, delay=None):
    from navierstokes3d_amd import tracers as TRC
    g = geometry(*grid)
    sp, org = (g["dx"], g["dy"], g["dz"]), (-0.5, -0.3, -0.35)
    pts = np.stack([org[q] + rnd(50 + q, (40,), lo=0.05, hi=0.95) * grid[q] * sp[q] for q in range(3)], axis=1)
    tr = TRC.Tracers(grid, ctx, sp, org, keep_velocity=True).seed_random(N_POINTS, seed=4)
    ctx.sync()
    torch.cuda.synchronize()
    pending = None
    if S is not None:
        delay.enqueue(S)
    tr.advance(f, 2.5 * g["dx"])                                          # every particle alive before it, many dead after it
    if S is not None:
        ev = torch.cuda.Event()
        ev.record(S)
        pending = not ev.query()                                          # the advance is still queued when reseed is called
    placed = tr.reseed(pts)
    tr.advance(f, 0.4 * g["dx"])
    ctx.sync()
    torch.cuda.synchronize()
    return {"placed": np.array([placed]), "positions": tr.positions(), "alive": tr.alive().astype(np.uint8), "U": tr.U.cpu().numpy()}, pending


@pytest.mark.parametrize("kind", KINDS)
def test_reseed_waits_for_a_queued_advance(hip, delay, kind):
    """reseed reads `state` with torch ops on PyTorch's stream; the advance that kills particles is queued on the pinned context's
    stream behind the delay.  A reseed that does not wait finds no dead slot."""
    grid = GRIDS[0]
    f = _wrapper_fields(hip, grid, 61)
    torch.cuda.synchronize()
    plain = hip.Context(0, "strict")
    want, _ = _reseed_run(hip, plain, f, grid)
    plain.close()
    assert 0 < want["placed"][0] <= 40 and want["alive"].sum() < N_POINTS
    ctx, S = SO.context_on(hip, kind)
    _reseed_run(hip, ctx, f, grid)                                        # warm-up
    got, pending = _reseed_run(hip, ctx, f, grid, S, delay)
    ctx.close()
    assert pending, "delay too short: the case proves nothing"
    bad = ["%s %s" % (k, SO.diagnose(got[k], want[k], None)) for k in want if not SO.bits_same(got[k], want[k])]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_wrappers_with_late_fields(hip, delay, kind):
    """the mirrored arrangement: the delay and the arrival of the fields on the CONTEXT's stream, PyTorch's stream idle"""
    grid = GRIDS[0]
    real, decoy = _wrapper_fields(hip, grid, 61), _wrapper_fields(hip, grid, 161)
    f = SimpleNamespace(**{k: hip.clone(v) for k, v in vars(decoy).items()})
    torch.cuda.synchronize()
    plain = hip.Context(0, "strict")
    want = _wrappers(hip, plain, real, grid)
    early = _wrappers(hip, plain, decoy, grid)
    plain.close()
    ctx, S = SO.context_on(hip, kind)
    _wrappers(hip, ctx, real, grid)                                      # warm-up
    torch.cuda.synchronize()
    pending = []

    def before():
        torch.cuda.current_stream(0).synchronize()
        S.synchronize()
        for k, v in vars(decoy).items():
            getattr(f, k).copy_(v)
        torch.cuda.current_stream(0).synchronize()
        delay.enqueue(S)
        with torch.cuda.stream(S):
            for k, v in vars(real).items():
                getattr(f, k).copy_(v)
            ev = torch.cuda.Event()
            ev.record(S)
        pending.append(not ev.query())
    got = _wrappers(hip, ctx, f, grid, before)
    ctx.close()
    assert all(pending), "delay too short: the case proves nothing (%r)" % (pending,)
    bad = ["%s %s" % (k, SO.diagnose(got[k], want[k], early[k])) for k in want if not SO.bits_same(got[k], want[k])]
    assert not bad, "\n".join(bad)


# ---- 9. the drivers inside `with torch.cuda.stream(S)` -------------------------------------------------------------------------------------
def _driver_run(which):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    from navierstokes3d_amd import kernels as K
    opts = dict(diagnostics=True, statistics=1, vortex=True, tracers=64, probes=[(0.0, 0.0, 0.0), (0.1, 0.05, 0.02)],
                isosurface={"field": "Q", "level": 0.0, "color": "Pr"})
    if which == "multi":
        out = run_navierstokes3D(nx=24, nt=3, mode="strict", return_info=True, **opts)
        arrays, info = list(out[:5]), out[-1]
    else:
        f, info = runme(nx=20, nt=2, **opts)
        arrays = [K.to_numpy(getattr(f, n)) for n in ("C", "Pr", "Vx", "Vy", "Vz")]
    arrays += [info.tracers.x, info.tracers.y, info.tracers.z, info.probes.u, info.probes.p, info.isosurface.tri_index]
    return arrays, info


@pytest.mark.parametrize("which", ["multi", "gpu"])
def test_driver_on_a_side_stream(hip, which):
    """run_navierstokes3D(nx=24, nt=3) and runme(nx=20, nt=2) with their observers on, inside `with torch.cuda.stream(S)`: fields,
    iteration counts and residual histories are those of the run on the default stream"""
    want, winfo = _driver_run(which)
    S = torch.cuda.Stream(0)
    with torch.cuda.stream(S):
        got, ginfo = _driver_run(which)
    S.synchronize()
    for q, (a, b) in enumerate(zip(got, want)):
        assert SO.bits_same(np.asarray(a), np.asarray(b)), (which, q)
    assert SO.same_result(ginfo.iters, winfo.iters), (ginfo.iters, winfo.iters)
    assert SO.same_result(ginfo.errs, winfo.errs)
