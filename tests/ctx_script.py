"""Operation scripts for one long-lived context (tests/test_gpu_context_history.py, tests/test_gpu_host_threads.py).

A host keeps ONE context for the whole program, calls its entry points on it, changes grids, element types, knobs and streams as
it goes, and may run one such context per host thread.  include/ns3d.h promises that scratch is grown lazily, that plans and graphs
are remembered, and that contexts on different threads are independent.  What a context remembers must therefore never
show in a result: an op returns the bits it returns on a fresh context, whatever ran before it and whatever runs beside it.

An OP is a named, self-contained call or short call group.  Its inputs are seeded from its NAME (never from its place in a script);
its result is a list of (label, array): the bits of every output array, every returned scalar (iteration count, error history,
diagnostics record, triangle count, last_pt_pace …) and the bits of every input after the call, which must be unchanged.  A SETTING
op changes the context and returns nothing.

    run(script, ctx, mode)       executes the ops on one context; returns {op name: result} of the value ops (a repeated op gets
                                 "name#2", …); with a mode every result is compared with reference(op, mode) and a difference is
                                 reported by op, first differing array and index
    reference(op, mode)          the op alone on a fresh context of that mode on PyTorch's default (null) stream, cached per process

REFERENCE RULE.  In STRICT (NS3D_IEEE_DIV included) every tile variant, pass depth, graph or cooperative form, CU mask and stream
gives the same bits, so the reference of an op is what a fresh context with default settings returns, whatever the script set
before.  In FAST the FMA contraction may differ between tile shapes and kernel forms: FAST ops pin set_pt_variant, set_pt2_variant,
set_ptn_variant, set_pt_depth, graph and persist mode INSIDE the op, and so does their reference (it runs the same op).

Every PT op starts by resetting the four tile knobs to automatic (STRICT) or pinning them (FAST) and then sets the knobs its
name says; graph mode, persist mode, pacing, autotune, CU reservation and stream stay as the script left them unless the op names
them.  The ops leave their own settings behind: that is the history the next op meets.

ADVECTION KNOB (ns3d_set_advection).  It is remembered state that CHANGES a result, that of ns3d_time_step and of nothing else
(include/ns3d.h: "Nothing else reads the knob"), so it is part of a time step's NAME: every time_step op pins the scheme it names
at its start — time_step_*_mc_* the MacCormack scheme, the others the reference's — and leaves it behind.  Every other op must be
indifferent to it, the single calls advect_mc and copy_advect + advect_correct included: set_advection(0 | 1) are setting ops.
The ops of the MacCormack step and its single calls are MC_OPS, a list of their own beside VALUE_OPS (the scripts "of all value
ops" keep their composition); mc_ops(mode) are those of a mode, seeded_script(…, ops=…) shuffles any list.

Grids — the smallest at which each piece of state exists:
    A  24×15×15    HIP-graph blocks                      E  131×66×37   LDS GEMM of the direct solve
    B  63×38×38    k_pt_persist, 64×2×2 workgroups       F  70×35×12    direct-solve products on both GEMM kernels
    C  70×30×40    2×2 tiles of 64×24, one z-chunk       G  192×96×96   1.77 M cells: the planner times shapes, g_tuned is used
    D  130×50×40   3×3 tiles of the same shape           G2 200×96×96   as G; only the first-use thread test touches it
"""
import contextlib
import random
import zlib
from types import SimpleNamespace

import numpy as np

from util import SHAPES, fields, first_bit_difference, geometry, rnd

GRIDS = {"A": (24, 15, 15), "B": (63, 38, 38), "C": (70, 30, 40), "D": (130, 50, 40), "E": (131, 66, 37), "F": (70, 35, 12),
         "G": (192, 96, 96), "G2": (200, 96, 96)}
NP = {"f64": np.float64, "f32": np.float32}
MODES = {"strict": dict(mode="strict"), "ieee": dict(mode="strict", ieee_div=True), "fast": dict(mode="fast")}
BC = (0, True, 0.25)                         # multi.jl's pressure rule with an outlet value that is not zero
FAST_V2 = 100                                # the two-iteration tile FAST ops pin (shape 1, z-chunks chosen per launch)


def seed_of(name):
    """the seed of an op's inputs: a function of its name alone"""
    return zlib.crc32(name.encode("utf-8")) % 1000003


def make_context(hip, mode):
    return hip.Context(0, **MODES[mode])


def is_fast(ctx):
    return ctx.mode == "fast"


class Op:
    """name; value (False: a setting op); inputs() → {label: host array}; call(hip, ctx, inp) → [(label, array)];
    fast: the op is also part of a FAST context's scripts; cooperative: the op may run as a k_pt_persist launch"""

    def __init__(self, name, call, inputs=None, value=True, fast=False):
        self.name, self.call, self._inputs, self.value, self.fast = name, call, inputs, value, fast
        self.cooperative = value and ":B:" in name          # B is the grid of k_pt_persist: by size, or by set_persist_mode(1)

    def inputs(self):
        return self._inputs(self.name) if self._inputs else {}

    def __repr__(self):
        return "Op(%s)" % self.name


def _scalars(*xs):
    return np.asarray([float(x) for x in xs], dtype=np.float64)


def _geom(grid):
    """util.geometry with a pseudo-time step inside the PT loop's stability bound, so that iterates stay finite in fp32 too"""
    g = geometry(*grid)
    g["dtau"] = 0.8 / np.sqrt(1.0 / g["dx"] ** 2 + 1.0 / g["dy"] ** 2 + 1.0 / g["dz"] ** 2)
    return g


def _pt_inputs(grid, dt):
    def make(name):
        Pr0, d0, rhs = fields(*grid, ["c", "i", "c"], seed_of(name), NP[dt])
        rhs *= NP[dt](1e-3)
        return {"Pr0": Pr0, "d0": d0, "rhs": rhs}
    return make


def _ptp(hip, dPr, grid):
    g = _geom(grid)
    return hip.pt_params(dPr, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], BC[0], BC[1], BC[2], g["g"])


def _tiles(ctx, v1=0, v2=0, vn=0, depth=0):
    ctx.set_pt_variant(v1); ctx.set_pt2_variant(v2); ctx.set_ptn_variant(vn); ctx.set_pt_depth(depth)


def _upload(hip, ctx, inp, names):
    t = [hip.from_numpy(inp[n]) for n in names]
    ctx.after_torch_fill()                   # a pinned context (own, masked or side stream) is not ordered with PyTorch's uploads
    return t


def _download(hip, ctx, pairs):
    """[(label, tensor)] → [(label, host array)] once everything the context started is complete"""
    ctx.sync()
    return [(label, hip.to_numpy(t)) for label, t in pairs]


# ---- value ops --------------------------------------------------------------------------------------------------------------------
def _op_pt_iterate(g, dt, depth=0, vn_fast=0, persist_fast=0):
    grid = GRIDS[g]
    name = "pt_iterate%s:%s:%s" % ("" if not depth else "_depth%d" % depth, g, dt)

    def call(hip, ctx, inp):
        if is_fast(ctx):
            _tiles(ctx, 0, FAST_V2, vn_fast, depth or 2)
            ctx.set_graph_mode(0); ctx.set_persist_mode(persist_fast)
        else:
            _tiles(ctx, depth=depth)
        dP, dD, dR = _upload(hip, ctx, inp, ("Pr0", "d0", "rhs"))
        hip.pt_iterate(dP, dD, dR, _ptp(hip, dP, grid), 7, ctx=ctx)
        return _download(hip, ctx, [("Pr", dP), ("dPrdtau", dD), ("rhs unchanged", dR)])
    return Op(name, call, _pt_inputs(grid, dt), fast=True)


def _op_pt_sweepn(g, dt, nlev, variant, pace=None, fast=False):
    grid = GRIDS[g]
    name = "pt_sweepn%d_v%d%s:%s:%s" % (nlev, variant, "" if pace is None else "_pace%d" % pace, g, dt)

    def call(hip, ctx, inp):
        _tiles(ctx, 0, FAST_V2 if is_fast(ctx) else 0, variant, 0)
        if pace is not None:
            ctx.set_pt_pace(pace)
        dP, dD, dR = _upload(hip, ctx, inp, ("Pr0", "d0", "rhs"))
        dQ, dE = _upload(hip, ctx, {"q": np.full_like(inp["Pr0"], 555.0), "e": np.full_like(inp["d0"], 444.0)}, ("q", "e"))
        hip.pt_sweepn(nlev, dP, dQ, dD, dE, dR, _ptp(hip, dP, grid), ctx=ctx)
        out = _download(hip, ctx, [("Pr_out", dQ), ("dPrdtau_out", dE), ("Pr_in unchanged", dP), ("dPrdtau_in unchanged", dD),
                                   ("rhs unchanged", dR)])
        if pace is not None:
            out.append(("last_pt_pace", _scalars(ctx.last_pt_pace())))
        return out
    return Op(name, call, _pt_inputs(grid, dt), fast=fast)


def _solve_once(hip, ctx, dP, dD, dR, p):
    it, errs = hip.pt_solve(dP, dD, dR, p, -1.0, 25, 8, 0.36, 1000.0, ctx=ctx)
    return _scalars(it, *errs)


def _op_pt_solve(g, dt, form, fast=False):
    """form 'graph': set_graph_mode(1); 'persist': set_persist_mode(1)"""
    grid = GRIDS[g]
    name = "pt_solve_%s:%s:%s" % (form, g, dt)

    def call(hip, ctx, inp):
        if is_fast(ctx):
            _tiles(ctx, 0, FAST_V2, 0, 2)
            ctx.set_graph_mode(1 if form == "graph" else 0); ctx.set_persist_mode(1 if form == "persist" else 0)
        else:
            _tiles(ctx)
            if form == "graph":
                ctx.set_graph_mode(1); ctx.set_persist_mode(-1)      # an explicit graph request wins over the automatic cooperative form
            else:
                ctx.set_persist_mode(1)
        dP, dD, dR = _upload(hip, ctx, inp, ("Pr0", "d0", "rhs"))
        rec = _solve_once(hip, ctx, dP, dD, dR, _ptp(hip, dP, grid))
        return [("iterations, err history", rec)] + _download(hip, ctx, [("Pr", dP), ("dPrdtau", dD), ("rhs unchanged", dR)])
    return Op(name, call, _pt_inputs(grid, dt), fast=fast)


MANY_DTS = 18


def _op_pt_solve_many_params():
    """the graph-mode solve on A with 18 values of dt on the SAME buffers — every dt is a new cache key, so the 16-entry wipe of
    run_block_graph is passed — then the first dt again: 19 results"""
    grid = GRIDS["A"]

    def call(hip, ctx, inp):
        _tiles(ctx)
        ctx.set_graph_mode(1); ctx.set_persist_mode(-1)
        mP, mD, dR = _upload(hip, ctx, inp, ("Pr0", "d0", "rhs"))
        dP, dD = _upload(hip, ctx, inp, ("Pr0", "d0"))
        out = []
        for n, q in enumerate(list(range(MANY_DTS)) + [0]):
            ctx.sync()
            dP.copy_(mP); dD.copy_(mD)
            ctx.after_torch_fill()
            p = _ptp(hip, dP, grid)
            p.dt = p.dt * (1.0 + 0.03125 * q)
            out.append(("solve %d: iterations, err history" % n, _solve_once(hip, ctx, dP, dD, dR, p)))
            out += _download(hip, ctx, [("solve %d: Pr" % n, dP), ("solve %d: dPrdtau" % n, dD)])
        out += _download(hip, ctx, [("rhs unchanged", dR)])
        n = int(ctx.lib.ns3d_cached_graphs(ctx.handle))
        out.append(("blocks are held as graphs, fewer than the wipe's 16", _scalars(1 <= n <= 16)))
        return out
    return Op("pt_solve_many_params:A:f64", call, _pt_inputs(grid, "f64"))


def _op_poisson_direct():
    """E, then F, then E: the plan is replaced twice"""
    order = ("E", "F", "E")

    def inputs(name):
        return {"%s %s" % (k, g): a for g in ("E", "F")
                for k, a in zip(("Pr0", "d0", "rhs"), fields(*GRIDS[g], ["c", "i", "c"], seed_of(name + g)))}

    def call(hip, ctx, inp):
        out = []
        for q, g in enumerate(order):
            dP, dD, dR = _upload(hip, ctx, inp, ["%s %s" % (k, g) for k in ("Pr0", "d0", "rhs")])
            hip.poisson_direct(dP, dD, dR, _ptp(hip, dP, GRIDS[g]), ctx=ctx)
            out += _download(hip, ctx, [("%d %s: Pr" % (q, g), dP), ("%d %s: dPrdtau" % (q, g), dD), ("%d: rhs %s unchanged" % (q, g), dR)])
        return out
    return Op("poisson_direct:EFE:f64", call, inputs)


def _flow_inputs(grid, dt="f64", scale=1.0):
    def make(name):
        Vx, Vy, Vz, Pr, Cf = fields(*grid, ["vx", "vy", "vz", "c", "c"], seed_of(name), NP[dt])
        return {"Vx": Vx * NP[dt](scale), "Vy": Vy * NP[dt](scale), "Vz": Vz * NP[dt](scale), "Pr": Pr, "C": Cf}
    return make


def _op_diagnostics():
    """A then E: the monitor scratch grows in between"""
    def inputs(name):
        return {"%s %s" % (k, g): a for g in ("A", "E") for k, a in _flow_inputs(GRIDS[g])(name + g).items()}

    def call(hip, ctx, inp):
        out = []
        for g in ("A", "E"):
            nx, ny, nz = GRIDS[g]
            names = ["%s %s" % (k, g) for k in ("Vx", "Vy", "Vz", "Pr", "C")]
            t = _upload(hip, ctx, inp, names)
            ge = _geom(GRIDS[g])
            r = hip.diagnostics(*t, hip.diag_params(nx, ny, nz, ge["dx"], ge["dy"], ge["dz"], ge["rho"]), ctx=ctx)
            out.append(("%s: record" % g, _scalars(*r.vmax, r.div_max, r.pr_min, r.pr_max, r.ke, r.c_vol, *r.mom, *r.n_masked, r.nonfinite)))
            out += _download(hip, ctx, [(n + " unchanged", a) for n, a in zip(names, t)])
        return out
    return Op("diagnostics:AE:f64", call, inputs)


def _op_isosurface():
    """a sphere with a rough surface in A's then in E's cell array: the segment scratch grows in between"""
    def inputs(name):
        out = {}
        for g in ("A", "E"):
            n = GRIDS[g]
            i, j, k = np.meshgrid(*[np.arange(q, dtype=np.float64) - 0.5 * (q - 1) for q in n], indexing="ij")
            out["A " + g] = np.asfortranarray(np.sqrt(i * i + j * j + k * k) + 0.25 * rnd(seed_of(name + g), n))
            out["B " + g] = rnd(seed_of(name + g) + 1, n)
        return out

    def call(hip, ctx, inp):
        import torch
        out = []
        for g in ("A", "E"):
            level = 0.3 * min(GRIDS[g])
            A, B = _upload(hip, ctx, inp, ("A " + g, "B " + g))
            n = hip.isosurface(A, level, ctx=ctx)
            tri, val = torch.full((9 * n,), -1.0, dtype=torch.float64, device="cuda"), torch.full((3 * n,), -1.0, dtype=torch.float64, device="cuda")
            ctx.after_torch_fill()
            n2 = hip.isosurface(A, level, color=B, tri=tri, val=val, cap=n, ctx=ctx)
            ctx.sync()
            out += [("%s: triangle counts" % g, _scalars(n, n2)), ("%s: tri" % g, tri.cpu().numpy()), ("%s: val" % g, val.cpu().numpy())]
            out += _download(hip, ctx, [("A %s unchanged" % g, A), ("B %s unchanged" % g, B)])
        return out
    return Op("isosurface:AE:f64", call, inputs)


def _op_residual_and_max():
    """residual_max + max_abs on A then on E: both read back through the context's one key word"""
    def inputs(name):
        return {"%s %s" % (k, g): a for g in ("A", "E") for k, a in zip(("Pr", "rhs"), fields(*GRIDS[g], ["c", "c"], seed_of(name + g)))}

    def call(hip, ctx, inp):
        out = []
        for g in ("A", "E"):
            dP, dR = _upload(hip, ctx, inp, ("Pr " + g, "rhs " + g))
            r = hip.residual_max(dP, dR, _ptp(hip, dP, GRIDS[g]), ctx=ctx)
            m = hip.max_abs(dP, ctx=ctx)
            m2 = hip.max_abs(dR, ctx=ctx)
            out.append(("%s: residual_max, max_abs(Pr), max_abs(rhs)" % g, _scalars(r, m, m2)))
            out += _download(hip, ctx, [("Pr %s unchanged" % g, dP), ("rhs %s unchanged" % g, dR)])
        return out
    return Op("residual_max+max_abs:AE:f64", call, inputs)


STEP_SHAPES = {"Pr": "c", "dPrdtau": "i", "divV": "c", "Vx": "vx", "Vy": "vy", "Vz": "vz", "Vx_o": "vx", "Vy_o": "vy", "Vz_o": "vz", "C": "c",
               "C_o": "c", "txx": "c", "tyy": "c", "tzz": "c", "txy": "s", "txz": "s", "tyz": "s"}


def _op_time_step(script, pressure, maccormack=False, g="A", dt="f64"):
    """one ns3d_time_step from the driver's own initial state at the size of grid g (multi_params / gpu_params of its nx),
    parameters from the drivers' StepParams builder.  The op pins the advection knob it names — maccormack: the MacCormack scheme
    with faithful = 0, whose stage-1 fields live in the context's hat scratch (16× as large on B as on A; half as large in f32);
    otherwise the reference's with faithful = 1 — and leaves it behind.  A MacCormack op also returns which buffer each of the
    eight swapped names ends on: the arrays are compared by buffer, and a swap left out moves no data."""
    grid = GRIDS[g]

    def params():
        from navierstokes3d_amd.params import gpu_params, multi_params
        p = multi_params(grid[0]) if script == "multi" else gpu_params(grid[0])
        assert (p.nx, p.ny, p.nz) == grid
        return p

    def inputs(name):
        from navierstokes3d_amd import driver as Dr
        p = params()
        host = {k: np.zeros(SHAPES[kind](*grid), dtype=NP[dt], order="F") for k, kind in STEP_SHAPES.items()}
        if script == "multi":
            host["Vy"][0, :, :] = p.vin
        else:
            Vx0, Pr0 = Dr.gpu_initial_fields(p)
            host["Vx"], host["Pr"] = np.asfortranarray(Vx0.astype(NP[dt])), np.asfortranarray(Pr0.astype(NP[dt]))
        return host

    def call(hip, ctx, inp):
        from navierstokes3d_amd import driver as Dr, lib as L
        p = params()
        ctx.set_advection("maccormack" if maccormack else "reference")
        names = list(STEP_SHAPES)
        f = SimpleNamespace(**dict(zip(names, _upload(hip, ctx, inp, names))))
        held = {n: getattr(f, n) for n in names}                 # by buffer: the step swaps the roles of X and X_o
        if script == "multi":
            hip.set_cylinder(f.C, f.Vx, f.Vy, f.Vz, p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz,
                             p.dx, p.dy, p.dz, ctx=ctx)
        sp = Dr._step_params(L.NS3D_BC_MULTI if script == "multi" else L.NS3D_BC_GPU, p, p.niter, not maccormack, "direct" if pressure else "pt")
        it, errs = hip.time_step(f, sp, ctx=ctx)
        out = [("iterations, err history", _scalars(it, *errs))] + _download(hip, ctx, [("buffer " + n, held[n]) for n in names])
        if maccormack:
            swapped = ("Vx", "Vy", "Vz", "C", "Vx_o", "Vy_o", "Vz_o", "C_o")
            out.append(("the buffer each of %s ends on" % ", ".join(swapped),
                        _scalars(*[names.index(next(k for k in names if held[k] is getattr(f, n))) for n in swapped])))
        return out
    return Op("time_step_%s%s_pressure%d:%s:%s" % (script, "_mc" if maccormack else "", pressure, g, dt), call, inputs)


MC_NAMES = ("Vx", "Vy", "Vz", "C")


def _op_advect_mc(dt, two_calls):
    """the single calls of the MacCormack scheme on A — ns3d_advect_mc, or ns3d_copy_advect(faithful = 0) into the hat arrays followed
    by ns3d_advect_correct —, outputs and hat arrays over a fill: neither reads the advection knob, whatever a script left it at"""
    grid = GRIDS["A"]

    def inputs(name):
        return dict(zip((n + "_o" for n in MC_NAMES), fields(*grid, ["vx", "vy", "vz", "c"], seed_of(name), NP[dt])))

    def call(hip, ctx, inp):
        g = _geom(grid)
        old_names = [n + "_o" for n in MC_NAMES]
        o = _upload(hip, ctx, inp, old_names)
        n = _upload(hip, ctx, {k: np.full_like(a, 333.0) for k, a in inp.items()}, old_names)
        h = _upload(hip, ctx, {k: np.full_like(a, 222.0) for k, a in inp.items()}, old_names)
        trios = [t for trio in zip(n, o, h) for t in trio]
        if two_calls:
            hip.copy_advect(h[0], o[0], h[1], o[1], h[2], o[2], h[3], o[3], g["dt"], g["dx"], g["dy"], g["dz"], False, ctx=ctx)
            hip.advect_correct(*trios, g["dt"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        else:
            hip.advect_mc(*trios, g["dt"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        return _download(hip, ctx, list(zip(MC_NAMES, n)) + list(zip((k + "_hat" for k in MC_NAMES), h)) +
                         list(zip((k + " unchanged" for k in old_names), o)))
    return Op("%s:A:%s" % ("copy_advect+advect_correct" if two_calls else "advect_mc", dt), call, inputs, fast=True)


def _op_advect(dt):
    grid = GRIDS["A"]

    def inputs(name):
        a = fields(*grid, ["vx", "vy", "vz", "c"], seed_of(name), NP[dt])
        return dict(zip(("Vx_o", "Vy_o", "Vz_o", "C_o"), a))

    def call(hip, ctx, inp):
        g = _geom(grid)
        o = _upload(hip, ctx, inp, ("Vx_o", "Vy_o", "Vz_o", "C_o"))
        n = _upload(hip, ctx, inp, ("Vx_o", "Vy_o", "Vz_o", "C_o"))
        hip.advect(n[0], o[0], n[1], o[1], n[2], o[2], n[3], o[3], g["dt"], g["dx"], g["dy"], g["dz"], True, ctx=ctx)
        return _download(hip, ctx, list(zip(("Vx", "Vy", "Vz", "C"), n)) + list(zip(("Vx_o unchanged", "Vy_o unchanged", "Vz_o unchanged",
                                                                                   "C_o unchanged"), o)))
    return Op("advect:A:%s" % dt, call, inputs, fast=True)


def _op_predict_fused(dt):
    grid = GRIDS["A"]

    def inputs(name):
        return dict(zip(("Vx", "Vy", "Vz"), fields(*grid, ["vx", "vy", "vz"], seed_of(name), NP[dt])))

    def call(hip, ctx, inp):
        g = _geom(grid)
        v = _upload(hip, ctx, inp, ("Vx", "Vy", "Vz"))
        n = _upload(hip, ctx, {k: np.full_like(a, 333.0) for k, a in inp.items()}, ("Vx", "Vy", "Vz"))
        hip.predict_fused(*n, *v, g["mu"], g["rho"], g["g"], g["dt"], g["dx"], g["dy"], g["dz"], ctx=ctx)
        return _download(hip, ctx, list(zip(("Vx_new", "Vy_new", "Vz_new"), n)) + list(zip(("Vx unchanged", "Vy unchanged", "Vz unchanged"), v)))
    return Op("predict_fused:A:%s" % dt, call, inputs, fast=True)


def _build_value_ops():
    ops = []
    for g in ("A", "B", "G"):
        for dt in ("f64", "f32"):
            ops.append(_op_pt_iterate(g, dt, persist_fast=1 if g == "B" else 0))
    ops += [_op_pt_iterate("C", "f64", 3, vn_fast=2800), _op_pt_iterate("C", "f32", 3, vn_fast=2800), _op_pt_iterate("D", "f64", 4)]
    ops[-1].fast = False
    ops += [_op_pt_sweepn("C", "f64", 4, 2800),
            _op_pt_sweepn("C", "f64", 4, 2900, 8, fast=True), _op_pt_sweepn("C", "f32", 4, 2900, 8, fast=True), _op_pt_sweepn("D", "f64", 4, 2900, 8),
            _op_pt_sweepn("D", "f64", 3, 3800)]
    ops += [_op_pt_solve("A", "f64", "graph", True), _op_pt_solve("A", "f32", "graph", True), _op_pt_solve("C", "f64", "graph"),
            _op_pt_solve("B", "f64", "persist", True), _op_pt_solve("B", "f32", "persist", True)]
    ops += [_op_pt_solve_many_params(), _op_poisson_direct(), _op_diagnostics(), _op_isosurface(), _op_residual_and_max()]
    ops += [_op_time_step(s, pr) for s in ("multi", "gpu") for pr in (0, 1)]
    ops += [_op_advect("f64"), _op_advect("f32"), _op_predict_fused("f64"), _op_predict_fused("f32")]
    return ops


VALUE_OPS = _build_value_ops()
# the MacCormack step — both scripts and both pressure solves on A, the grid B whose hat is 16× A's, one float32 step (multi.jl's
# script: tests/test_advect_mc_host.py::test_float32_steps_that_stay_finite) — and the scheme's single calls in both element types
MC_OPS = [_op_time_step(s, pr, True) for s in ("multi", "gpu") for pr in (0, 1)] + \
         [_op_time_step("multi", 0, True, "B"), _op_time_step("multi", 0, True, "A", "f32")] + \
         [_op_advect_mc(dt, two) for two in (False, True) for dt in ("f64", "f32")]
OPS = {op.name: op for op in VALUE_OPS + MC_OPS}
assert len(OPS) == len(VALUE_OPS) + len(MC_OPS)


def value_ops(mode):
    """the value ops of a context of `mode`: all of them in STRICT, those that also exist in FAST otherwise"""
    return [op for op in VALUE_OPS if op.fast or mode != "fast"]


def mc_ops(mode):
    """MC_OPS of a context of `mode`: in FAST the single calls only"""
    return [op for op in MC_OPS if op.fast or mode != "fast"]


# ---- setting ops ------------------------------------------------------------------------------------------------------------------
def _setting(name, fn):
    op = Op(name, lambda hip, ctx, inp: fn(ctx), value=False)
    OPS[name] = op
    return op


def _side_stream(ctx):
    import torch
    if getattr(ctx, "_script_side_stream", None) is None:
        ctx._script_side_stream = torch.cuda.Stream(ctx.device)
    ctx.use_torch_stream(ctx._script_side_stream, pin=True)


def _reset_tiles(ctx):
    _tiles(ctx)


SETTING_OPS = [_setting("reserve_cus(32)", lambda c: c.reserve_cus(32)), _setting("reserve_cus(0)", lambda c: c.reserve_cus(0)),
               _setting("use_own_stream()", lambda c: c.use_own_stream()), _setting("use_torch_stream(side_stream)", _side_stream),
               _setting("use_torch_stream()", lambda c: c.use_torch_stream())]
SETTING_OPS += [_setting("set_autotune(%d)" % v, lambda c, v=v: c.set_autotune(v)) for v in (0, 1)]
SETTING_OPS += [_setting("set_graph_mode(%d)" % v, lambda c, v=v: c.set_graph_mode(v)) for v in (-1, 0, 1)]
SETTING_OPS += [_setting("set_persist_mode(%d)" % v, lambda c, v=v: c.set_persist_mode(v)) for v in (-1, 0, 1)]
SETTING_OPS += [_setting("set_pt_pace(%d)" % v, lambda c, v=v: c.set_pt_pace(v)) for v in (-1, 0, 8, 16)]
SETTING_OPS += [_setting("set_pt_depth(0) and variant resets", _reset_tiles)]
SETTING_OPS += [_setting("set_advection(%d)" % v, lambda c, v=v: c.set_advection(("reference", "maccormack")[v])) for v in (0, 1)]


# ---- scripts ----------------------------------------------------------------------------------------------------------------------
def seeded_script(seed, mode, settings=True, ops=None):
    """a permutation of all value ops of `mode` (or of `ops`) drawn from `seed`, with one setting op (drawn likewise) in front of
    every second value op when `settings` is set"""
    rng = random.Random(seed)
    vals = list(value_ops(mode) if ops is None else ops)
    rng.shuffle(vals)
    out = []
    for q, op in enumerate(vals):
        if settings and q % 2 == 1:
            out.append(rng.choice(SETTING_OPS))
        out.append(op)
    return out


def hostile_script():
    """every transition where it hurts, on one STRICT context (tests/test_gpu_context_history.py); the numbers are the issue's"""
    o = OPS.__getitem__
    s = []
    # 1. graphs captured on A, then G's ping-pong growth (which wipes them), then A again: captured again.  Autotune is off here, so
    #    that G's FIRST PLANNED use is step 6's (in a process in which no context has run G with autotune on before: the references
    #    are made after the script)
    s += [o("set_graph_mode(1)"), o("pt_solve_graph:A:f64"), o("set_graph_mode(-1)"), o("set_autotune(0)"), o("pt_iterate:G:f64"),
          o("pt_solve_graph:A:f64")]
    # 8. fp32 and fp64 ops of one grid alternating: the ping-pong buffer is sized in bytes, not cells
    s += [o("pt_solve_graph:A:f32"), o("pt_iterate:A:f64"), o("pt_iterate:A:f32"), o("pt_solve_graph:A:f64"), o("pt_iterate:B:f32"),
          o("pt_iterate:B:f64")]
    # 2. persist on B, CUs reserved, B again, released
    s += [o("set_persist_mode(-1)"), o("set_graph_mode(-1)"), o("set_pt_depth(0) and variant resets"), o("pt_iterate:B:f64"),
          o("pt_solve_persist:B:f64"), o("reserve_cus(32)"), o("pt_solve_persist:B:f64"), o("pt_iterate:B:f64"), o("pt_solve_persist:B:f32"),
          o("reserve_cus(0)"), o("pt_solve_persist:B:f64")]
    # 3. paced C, paced D, C at another pace, C in fp32 on the same counters
    s += [o("pt_sweepn4_v2900_pace8:C:f64"), o("pt_sweepn4_v2900_pace8:D:f64"), o("pt_sweepn4_v2900_pace16:C:f64"),
          o("pt_sweepn4_v2900_pace8:C:f32"), o("pt_sweepn4_v2900_pace8:C:f64"), o("pt_sweepn4_v2800:C:f64"), o("pt_sweepn3_v3800:D:f64"),
          o("pt_iterate_depth3:C:f64"), o("pt_iterate_depth3:C:f32"), o("pt_iterate_depth4:D:f64"), o("pt_solve_graph:C:f64")]
    # 4. direct solve on E, F, E (inside the op), twice around other work
    s += [o("poisson_direct:EFE:f64"), o("diagnostics:AE:f64"), o("isosurface:AE:f64"), o("residual_max+max_abs:AE:f64"),
          o("poisson_direct:EFE:f64")]
    # 5. the 19 solves past the graph cache's wipe, a change of stream, the same 19 again
    s += [o("pt_solve_many_params:A:f64"), o("use_own_stream()"), o("pt_solve_many_params:A:f64"), o("use_torch_stream(side_stream)"),
          o("pt_solve_graph:A:f64"), o("use_torch_stream()")]
    # 6. G with autotune on — its first planned use: the shapes are timed here, in the middle of the history —, off, on (a look-up);
    #    its fp32 first use likewise
    s += [o("set_autotune(1)"), o("pt_iterate:G:f64"), o("set_autotune(0)"), o("pt_iterate:G:f64"), o("pt_iterate:G:f32"), o("set_autotune(1)"),
          o("pt_iterate:G:f32"), o("pt_iterate:G:f64")]
    # 7. time_step between two pt_solve calls that share key_dev
    for name in ("time_step_multi_pressure0:A:f64", "time_step_multi_pressure1:A:f64", "time_step_gpu_pressure0:A:f64",
                 "time_step_gpu_pressure1:A:f64"):
        s += [o("pt_solve_graph:A:f64"), o(name), o("pt_solve_persist:B:f64")]
    s += [o("advect:A:f64"), o("advect:A:f32"), o("predict_fused:A:f64"), o("predict_fused:A:f32"), o("set_pt_pace(-1)")]
    # 9. the MacCormack step and its hat scratch.  A graph captured on A; the step on A, whose first use allocates the hat; on B: the
    #    hat grows, which frees the old buffer and wipes the graphs; the graph solve on A, captured again; the step on A again, a
    #    smaller grid in the larger buffer with another split; in float32, another split again; the reference step, which turns the
    #    knob off; the knob left ON in front of ops that must not read it; the step on the context's own stream and then on a side
    #    stream — the hat was last written on the stream just left —; the step with CUs reserved
    mc = "time_step_multi_mc_pressure0:A:f64"
    s += [o("set_graph_mode(1)"), o("pt_solve_graph:A:f64"), o(mc), o("time_step_multi_mc_pressure0:B:f64"), o("pt_solve_graph:A:f64"), o(mc),
          o("time_step_multi_mc_pressure0:A:f32"), o("time_step_multi_pressure0:A:f64"),
          o("set_advection(1)"), o("advect:A:f64"), o("advect_mc:A:f64"), o("advect_mc:A:f32"), o("copy_advect+advect_correct:A:f64"),
          o("copy_advect+advect_correct:A:f32"), o("predict_fused:A:f64"), o("pt_solve_graph:A:f64"),
          o("use_own_stream()"), o(mc), o("time_step_gpu_mc_pressure0:A:f64"), o("use_torch_stream(side_stream)"), o(mc),
          o("time_step_multi_mc_pressure1:A:f64"), o("reserve_cus(32)"), o(mc), o("time_step_gpu_mc_pressure1:A:f64"), o("reserve_cus(0)"),
          o("use_torch_stream()"), o(mc), o("set_advection(0)"), o("set_graph_mode(-1)")]
    return s


OPS["pt_sweepn4_v2900_pace16:C:f64"] = _op_pt_sweepn("C", "f64", 4, 2900, 16)        # the hostile script's own (step 3)
SMALL_OPS = ["pt_iterate:A:f64", "pt_solve_graph:A:f64", "pt_iterate:B:f64", "pt_solve_persist:B:f64", "pt_iterate_depth3:C:f64",
             "pt_sweepn4_v2900_pace8:C:f64", "pt_solve_graph:C:f64"]                  # the A-, B- and C-sized ops of the memory and churn tests
ONE_OF_EACH_KIND = ["pt_iterate:A:f64", "pt_sweepn4_v2900_pace8:C:f64", "pt_solve_graph:A:f64", "pt_solve_persist:B:f64", "advect:A:f64",
                    "predict_fused:A:f64", "time_step_multi_mc_pressure0:A:f64"]


# ---- running and comparing --------------------------------------------------------------------------------------------------------
def gpu_execute(op, ctx):
    from navierstokes3d_amd import kernels as hip
    return op.call(hip, ctx, op.inputs())


_REFERENCE = {}


def reference(op, mode, execute=gpu_execute, make=None):
    """the result of `op` alone on a fresh context of `mode` on PyTorch's default (null) stream; cached per process"""
    key = (op.name, mode, execute)
    if key not in _REFERENCE:
        if make is None:
            from navierstokes3d_amd import kernels as hip
            make = lambda m: make_context(hip, m)
        ctx = make(mode)
        try:
            _REFERENCE[key] = execute(op, ctx)
        finally:
            if hasattr(ctx, "close"):
                ctx.close()
    return _REFERENCE[key]


def difference(got, want):
    """None, or a sentence naming the first array that differs and the first index in it"""
    if [l for l, _ in got] != [l for l, _ in want]:
        return "the result has the entries %r, the reference %r" % ([l for l, _ in got], [l for l, _ in want])
    for (label, a), (_, b) in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "array %r: %s%r against %s%r" % (label, a.dtype, a.shape, b.dtype, b.shape)
        if a.dtype.kind != "f":
            if not np.array_equal(a, b):
                return "array %r: first difference at index %r" % (label, tuple(int(q) for q in np.argwhere(a != b)[0]))
            continue
        d = first_bit_difference(a, b)
        if d is not None:
            return "array %r: first difference at index %r, %s against %s (%d entries differ)" % (label, d[0], d[1], d[2], d[3])
    return None


class Mismatch(AssertionError):
    pass


def compare(results, names, mode, execute=gpu_execute, make=None):
    """results: {key: result} of run(); names: {key: op name}.  Raises Mismatch naming every op that differs from its reference."""
    bad = []
    for key, got in results.items():
        why = difference(got, reference(OPS[names[key]], mode, execute, make))
        if why:
            bad.append("op %r: %s" % (key, why))
    if bad:
        raise Mismatch("%d of %d results differ from their references (mode %s):\n  " % (len(bad), len(results), mode) + "\n  ".join(bad))
    return len(results)


def run(script, ctx, mode=None, execute=gpu_execute, make=None, names_out=None, guard=None):
    """Execute the ops of `script` in order on ctx.  Returns {key: result} for the value ops, key = the op's name ("name#2" for its
    second appearance, …).  mode given: every result is compared with reference(op, mode) once the script is through.
    guard(op): a context manager a value op runs inside (the threaded tests keep some ops of different threads apart with it)."""
    results, names, seen = {}, {}, {}
    for op in script:
        if not op.value:
            execute(op, ctx)
            continue
        seen[op.name] = seen.get(op.name, 0) + 1
        key = op.name if seen[op.name] == 1 else "%s#%d" % (op.name, seen[op.name])
        with (guard(op) if guard else contextlib.nullcontext()):
            results[key] = execute(op, ctx)
        names[key] = op.name
    if names_out is not None:
        names_out.update(names)
    if mode is not None:
        compare(results, names, mode, execute, make)
    return results
