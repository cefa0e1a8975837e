"""One context per host thread (include/ns3d.h: calls on different contexts may run concurrently from different threads).  Python
threads are enough: lib.py loads libns3d.so through ctypes.CDLL, which releases the GIL inside every call.  Every thread gets its
context passed explicitly.  What the contexts of a process share — the planner's memory g_tuned, the eigenvector cache of the
direct solve, device_cus(), the function-local statics of the launchers, stream capture in thread-local mode beside other threads'
allocations — must not show in a result: every op returns the bits of its single-threaded reference (tests/ctx_script.py).

k_pt_persist needs its workgroups resident together; a launch that finds the CUs taken by ANOTHER context's kernels ends in its
bounded waits, is voided and redone by launches (include/ns3d.h, ns3d_set_persist_mode).  Beside other threads that is ordinary
operation, so this module runs with NS3D_COOP_CHECK=0 (the suite's default 1 turns an expired wait into an error), set for the
whole module before its first thread starts.  In STRICT the redone block has the bits of the voided one, so the results must be
the reference's either way, and the number of voided launches is printed.  In FAST the two forms may differ by FMA contraction
(ctx_script pins the form inside FAST ops for that reason), so a FAST context's cooperative ops must not be voided: the waits
are bounded at 2²² polls (seconds), which ordinary kernels of other threads — milliseconds at most — never exhaust; only two
cooperative launches that each hold part of the chip and wait for the rest can.  The FAST thread therefore runs its four
cooperative ops while no other thread runs one (coop_guard: the STRICT threads still overlap theirs with each other), and its
count of voided launches is asserted to be zero.

Workers return their results and the main thread compares them.  Every worker is joined with a time limit, the measured
single-threaded duration of its script × the number of threads × 3 (and never less than LIMIT_FLOOR_SECONDS); a worker that has not
returned by then is a hang, and the session ends there (pytest.exit, return code 3) instead of going on to more GPU work."""
import threading
import time

import numpy as np
import pytest

import ctx_script as CS

pytestmark = pytest.mark.gpu

# Single-threaded seconds of the script each worker runs, as gpu_durations() at the end of this module prints them: every script in a
# child process of its own with nothing warmed up (modules not loaded, no plan made), on a context on its own stream, timed from the
# context's creation to the last download, input generation on the host included.  Measured 2026-10-20 on an MI355X machine.
SCRIPT_SECONDS = {"all value ops, strict": 0.30, "all value ops, fast": 0.13, "pt_iterate on G2, first use": 0.08, "small ops x 20": 0.21,
                  "direct solves E F": 0.11, "slab solve": 0.07, "create, solve on A, destroy x 40": 0.09, "argument errors x 50": 0.02}
# seconds × threads × 3 comes to 0.2 … 3.7 s with these figures: less than one scheduling hiccup of a shared machine, and a limit that
# trips ends the whole session.  So no limit is shorter than this; a hang is caught all the same.
LIMIT_FLOOR_SECONDS = 30.0
THREAD_MODES = ["strict", "strict", "ieee", "fast"]
THREAD_SEEDS = [21, 22, 23, 24]
MC_THREADS = (0, 2)                   # the threads whose scripts carry the MacCormack ops (tests/ctx_script.py MC_OPS); the others leave the knob off


@pytest.fixture(scope="module", autouse=True)
def expired_hand_overs_are_redone():
    """NS3D_COOP_CHECK=0 for the whole module, the module-scoped two-thread bring-up included (the library reads it per launch)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NS3D_COOP_CHECK", "0")
        yield


class CoopGuard:
    """guard(op) for ctx_script.run: cooperative ops of STRICT threads take one of `n_strict` permits — they overlap each other —,
    those of the FAST thread take all of them: no other thread's cooperative launch runs beside a FAST one"""

    def __init__(self, n_strict):
        self.n, self.permits, self.fast_turn = n_strict, threading.Semaphore(n_strict), threading.Lock()

    def guard(self, fast):
        import contextlib

        @contextlib.contextmanager
        def held(k):
            with self.fast_turn if k > 1 else contextlib.nullcontext():
                for _ in range(k):
                    self.permits.acquire()
                try:
                    yield
                finally:
                    for _ in range(k):
                        self.permits.release()
        return lambda op: held(self.n if fast else 1) if op.cooperative else contextlib.nullcontext()


def run_threads(workers, seconds_single):
    """every callable of `workers` on a thread of its own; returns their results in order.  A worker's exception is raised here;
    a worker still running after seconds_single × len(workers) × 3 (at least LIMIT_FLOOR_SECONDS) ends the session."""
    n = len(workers)
    limit = max(seconds_single * n * 3.0, LIMIT_FLOOR_SECONDS)
    out, errs = [None] * n, [None] * n

    def wrap(q):
        try:
            out[q] = workers[q]()
        except BaseException as e:            # noqa: B902 — handed to the main thread
            errs[q] = e
    threads = [threading.Thread(target=wrap, args=(q,), daemon=True) for q in range(n)]
    t0 = time.monotonic()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, t0 + limit - time.monotonic()))
    late = [q for q, t in enumerate(threads) if t.is_alive()]
    if late:
        pytest.exit("host threads %r have not returned after %.0f s (3 × %d threads × %.1f s single-threaded): a hang; no further GPU "
                    "work in this session" % (late, limit, n, seconds_single), returncode=3)
    print("%d threads: %.2f s (limit %.0f s)" % (n, time.monotonic() - t0, limit))
    for e in errs:
        if e is not None:
            raise e
    return out


def _barrier(n, seconds_single):
    return threading.Barrier(n, timeout=max(seconds_single * n * 3.0, LIMIT_FLOOR_SECONDS))


def _warm_references(names_by_mode):
    """references are computed (and cached) on the main thread before any worker starts"""
    for mode, names in names_by_mode.items():
        for n in names:
            CS.reference(CS.OPS[n], mode)


def _script_worker(hip, mode, script, barrier, own_stream, repeat=1, guard=None):
    def work():
        import torch
        torch.cuda.set_device(0)
        ctx = CS.make_context(hip, mode)
        if own_stream:
            ctx.use_own_stream()              # uploads are ordered by after_torch_fill (ctx_script._upload)
        barrier.wait()
        results, names = [], {}
        for _ in range(repeat):
            results.append(CS.run(script, ctx, names_out=names, guard=guard))
        faults = ctx.persist_faults()
        ctx.close()
        return results, names, faults
    return work


def _compare_all(done, modes):
    voided = []
    for (results, names, faults), mode in zip(done, modes):
        for r in results:
            assert CS.compare(r, names, mode) == len(names)
        voided.append(faults)
        assert mode != "fast" or faults == 0, "a cooperative launch of the FAST context was voided: its redo is another kernel form"
    print("cooperative launches voided and redone, per thread: %r" % voided)


@pytest.fixture(scope="module")
def two_threads_first(hip, expired_hand_overs_are_redone):
    """bring-up order: two threads before four"""
    names = [op.name for op in CS.value_ops("fast")]
    _warm_references({"strict": names})
    scripts = [CS.seeded_script(seed, "fast", settings=False) for seed in (31, 32)]
    b = _barrier(2, SCRIPT_SECONDS["all value ops, fast"])
    done = run_threads([_script_worker(hip, "strict", s, b, True) for s in scripts], SCRIPT_SECONDS["all value ops, fast"])
    _compare_all(done, ["strict", "strict"])
    return True


def test_last_error_belongs_to_the_calling_thread(hip):
    """two threads provoke different ARGUMENT errors (tests/api_error_cases.py: refused on the host, nothing is launched) in
    alternation; each reads its own message from ns3d_last_error; a third thread that never failed reads an empty string"""
    import api_error_cases as AE
    from navierstokes3d_amd import lib as L
    cases = {label: (fn, mods) for label, fn, mods, only in AE.cases() if "f64" in only}
    picks = ["update_Pr:small_x", "pt_solve:negative_niter"]
    ctxs = [hip.Context(0, "strict") for _ in range(3)]
    arenas = [AE.Arena(L, "f64") for _ in range(2)]
    for a in arenas:
        for label in picks:
            AE.VALID[cases[label][0]](L, a)       # the arrays exist before the threads start
    want = []
    for q, label in enumerate(picks):
        rc, msg = AE.run_case(L, ctxs[q].handle, arenas[q], "f64", *cases[label])
        assert rc == L.NS3D_ERR_ARG and msg
        want.append(msg)
    assert want[0] != want[1]
    rounds = 50
    b = _barrier(3, SCRIPT_SECONDS["argument errors x 50"])

    def failing(q):
        def work():
            seen = []
            for _ in range(rounds):
                b.wait()
                rc = AE.run_case(L, ctxs[q].handle, arenas[q], "f64", *cases[picks[q]])
                b.wait()                      # both have failed: each message must still be the thread's own
                seen.append((rc[0], rc[1], L.last_error()))
            return seen
        return work

    def innocent():
        seen = []
        for _ in range(rounds):
            b.wait()
            b.wait()
            seen.append(L.last_error())
        return seen
    a, c, none = run_threads([failing(0), failing(1), innocent], SCRIPT_SECONDS["argument errors x 50"])
    assert a == [(L.NS3D_ERR_ARG, want[0], want[0])] * rounds
    assert c == [(L.NS3D_ERR_ARG, want[1], want[1])] * rounds
    assert none == [""] * rounds
    for ctx in ctxs:
        ctx.close()


@pytest.mark.parametrize("streams", ["own", "shared"])
def test_four_threads_each_with_a_context(hip, two_threads_first, streams):
    """four contexts — two strict, one strict with NS3D_IEEE_DIV, one fast — each on its own thread through a different seeded
    order of all its value ops, started together.  own: every context on its own non-blocking stream; shared: all four on
    PyTorch's default stream.
    The first and the third thread's scripts also carry the MacCormack ops (their six time steps turn the advection knob on, their
    hat scratch is allocated and grown beside the other threads' work); the second and the fourth leave the knob off throughout and
    run the reference steps and the reference advection on the same grid A: the knob is one context's, not the process's."""
    mc_modes = {THREAD_MODES[q] for q in MC_THREADS}
    _warm_references({m: [op.name for op in CS.value_ops(m) + (CS.mc_ops(m) if m in mc_modes else [])] for m in set(THREAD_MODES)})
    scripts = [CS.seeded_script(seed, mode, settings=False, ops=CS.value_ops(mode) + (CS.mc_ops(mode) if q in MC_THREADS else []))
               for q, (seed, mode) in enumerate(zip(THREAD_SEEDS, THREAD_MODES))]
    assert [len(s) for s in scripts] == [42, 32, 42, 18]
    assert all(any("_mc_" in op.name for op in s) == (q in MC_THREADS) for q, s in enumerate(scripts))
    assert sum(op.name.startswith("time_step") for op in scripts[1]) == 4 and sum(op.name.startswith("advect:A") for op in scripts[3]) == 2
    b = _barrier(4, SCRIPT_SECONDS["all value ops, strict"])
    coop = CoopGuard(sum(m != "fast" for m in THREAD_MODES))
    done = run_threads([_script_worker(hip, m, s, b, streams == "own", guard=coop.guard(m == "fast")) for m, s in zip(THREAD_MODES, scripts)],
                       SCRIPT_SECONDS["all value ops, strict"])
    _compare_all(done, THREAD_MODES)
    assert [len(d[1]) for d in done] == [42, 32, 42, 18]


def _g2_op(dt="f64"):
    """pt_iterate on G2 = 200×96×96, which no other test tunes: the look-up of its first use misses"""
    name = "pt_iterate:G2:" + dt
    if name not in CS.OPS:
        CS.OPS[name] = CS._op_pt_iterate("G2", dt)
    return CS.OPS[name]


def test_first_use_of_one_grid_on_four_threads(hip, two_threads_first):
    """all four threads call pt_iterate on G2 at the barrier, autotune on, no context of the process having seen the grid: each
    call times the tile shapes, takes the planner's lock and writes an entry.  All four return the same bits, those of a fifth
    context created afterwards (whose look-up is answered) and of the single sweeps (variant 100, no planner)."""
    import torch
    op = _g2_op()
    b = _barrier(4, SCRIPT_SECONDS["pt_iterate on G2, first use"])
    done = run_threads([_script_worker(hip, "strict", [op], b, True) for _ in range(4)], SCRIPT_SECONDS["pt_iterate on G2, first use"])
    fifth = CS.reference(op, "strict")
    for results, names, faults in done:
        assert CS.difference(results[0][op.name], fifth) is None, CS.difference(results[0][op.name], fifth)
    # the reference of the reference: seven single sweeps, one thread per cell
    inp = op.inputs()
    ctx = hip.Context(0, "strict")
    ctx.set_pt_variant(100)
    dP, dQ, dD, dR = (hip.from_numpy(inp[n]) for n in ("Pr0", "Pr0", "d0", "rhs"))
    p = CS._ptp(hip, dP, CS.GRIDS["G2"])
    for _ in range(7):
        hip.pt_sweep(dP, dQ, dD, dR, p, 1, CS.GRIDS["G2"][2] - 1, ctx=ctx)
        dP, dQ = dQ, dP
    torch.cuda.synchronize()
    single = [("Pr", hip.to_numpy(dP)), ("dPrdtau", hip.to_numpy(dD)), ("rhs unchanged", hip.to_numpy(dR))]
    ctx.close()
    assert CS.difference(fifth, single) is None, CS.difference(fifth, single)


def _direct_ops():
    """poisson_direct on E and on F as ops of their own"""
    for g in ("E", "F"):
        name = "poisson_direct:%s:f64" % g
        if name not in CS.OPS:
            def inputs(nm, g=g):
                return dict(zip(("Pr0", "d0", "rhs"), CS.fields(*CS.GRIDS[g], ["c", "i", "c"], CS.seed_of(nm))))

            def call(hip_, ctx, inp, g=g):
                dP, dD, dR = CS._upload(hip_, ctx, inp, ("Pr0", "d0", "rhs"))
                p = CS._ptp(hip_, dP, CS.GRIDS[g])
                hip_.poisson_direct(dP, dD, dR, p, ctx=ctx)
                res = hip_.residual_max(dP, dR, p, ctx=ctx)          # compute_res! of the solution: no eigenbasis in it
                return [("residual_max", CS._scalars(res))] + CS._download(hip_, ctx, [("Pr", dP), ("dPrdtau", dD), ("rhs unchanged", dR)])
            CS.OPS[name] = CS.Op(name, call, inputs)
    return CS.OPS["poisson_direct:E:f64"], CS.OPS["poisson_direct:F:f64"]


def test_direct_solves_share_the_eigenvector_cache(hip, two_threads_first):
    """four threads call poisson_direct on E and F, two in each order: the cache of 1-D eigenbases is filled and read under its lock"""
    e, f = _direct_ops()
    b = _barrier(4, SCRIPT_SECONDS["direct solves E F"])
    orders = [[e, f, e], [f, e, f], [e, f, e], [f, e, f]]
    done = run_threads([_script_worker(hip, "strict", s, b, True) for s in orders], SCRIPT_SECONDS["direct solves E F"])
    _compare_all(done, ["strict"] * 4)            # the references are made afterwards, on the main thread, by the same cache
    # … so an entry spoilt by a racing fill would spoil them alike.  What does not go through the cache: the reference's own residual
    # (compute_res!, multi.jl:88-91) of every solution, at rounding level — the bound of tests/test_gpu_direct.py
    for results, names, faults in done:
        for key, res in results[0].items():
            r = dict(res)
            gname = names[key].split(":")[1]
            ge, inp = CS._geom(CS.GRIDS[gname]), CS.OPS[names[key]].inputs()
            scale = ge["rho"] / ge["dt"] * np.abs(inp["rhs"]).max() + np.abs(r["Pr"]).max() / min(ge["dx"], ge["dy"], ge["dz"]) ** 2
            assert 0.0 <= r["residual_max"][0] < 1e-10 * scale, (key, r["residual_max"][0] / scale)


def test_contexts_come_and_go_beside_running_ones(hip, two_threads_first):
    """two threads run the A-, B- and C-sized ops twenty times over on a context each while a third creates a context, runs one
    pt_solve on A and destroys it, forty times"""
    small = [CS.OPS[n] for n in CS.SMALL_OPS]
    _warm_references({"strict": CS.SMALL_OPS})
    b = _barrier(3, SCRIPT_SECONDS["small ops x 20"])

    def churn():
        b.wait()
        out = []
        for _ in range(40):
            ctx = CS.make_context(hip, "strict")
            out.append(CS.gpu_execute(CS.OPS["pt_solve_graph:A:f64"], ctx))
            ctx.close()
        return out
    done = run_threads([_script_worker(hip, "strict", small, b, True, repeat=20), _script_worker(hip, "strict", small[::-1], b, False, repeat=20),
                        churn], SCRIPT_SECONDS["small ops x 20"])
    _compare_all(done[:2], ["strict"] * 2)
    assert len(done[0][0]) == len(done[1][0]) == 20 and len(done[2]) == 40
    want = CS.reference(CS.OPS["pt_solve_graph:A:f64"], "strict")
    for q, got in enumerate(done[2]):
        assert CS.difference(got, want) is None, (q, CS.difference(got, want))


SLAB = (2, (40, 21, 10), 7, (True, 0.25, 0.0))
SLAB_SOLVE = (-1.0, 12, 5, 0.36, 1000.0)          # eps, niter, nchk, err_mul, err_div: two checks, then two more iterations


def _slab_inputs():
    from util import fields, geometry
    P, (nx, ny, nz), n_iters, bc = SLAB
    nz_g = P * (nz - 2) + 2
    return geometry(nx, ny, nz_g), fields(nx, ny, nz_g, ["c", "i", "c"], 211, np.float64)


def _slab_worker(hip, barrier=None):
    """a MultiGpu of two virtual z-slab ranks on device 0, created, run and closed by the calling thread"""
    def run():
        import torch
        from navierstokes3d_amd.mgpu import MultiGpu
        P, (nx, ny, nz), n_iters, bc = SLAB
        g, (Pg, Dg, Rg) = _slab_inputs()
        torch.cuda.set_device(0)
        Pr = [hip.from_numpy(Pg[:, :, r * (nz - 2):r * (nz - 2) + nz]) for r in range(P)]
        D = [hip.from_numpy(Dg[:, :, r * (nz - 2):r * (nz - 2) + nz - 2]) for r in range(P)]
        R = [hip.from_numpy(Rg[:, :, r * (nz - 2):r * (nz - 2) + nz]) for r in range(P)]
        torch.cuda.synchronize()
        if barrier is not None:
            barrier.wait()
        mg = MultiGpu.create([0] * P, nx, ny, nz, "strict", own_streams=True)
        mg.set_temporal(2)
        p = hip.pt_params(Pr[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, *bc)
        mg.slab_load(Pr, D, R, p)
        mg.slab_plan()
        mg.slab_iterate(n_iters)
        mg.slab_store(Pr, D)
        mg.sync()
        out = [hip.to_numpy(a) for a in Pr], [hip.to_numpy(a) for a in D]
        # and the whole inner loop with its residual read-backs across the ranks (ns3d_pt_solve_slab), from the same start
        Pr2 = [hip.from_numpy(Pg[:, :, r * (nz - 2):r * (nz - 2) + nz]) for r in range(P)]
        D2 = [hip.from_numpy(Dg[:, :, r * (nz - 2):r * (nz - 2) + nz - 2]) for r in range(P)]
        torch.cuda.synchronize()
        it, errs = mg.pt_solve_slab(Pr2, D2, R, p, *SLAB_SOLVE)
        mg.sync()
        out += (it, errs, [hip.to_numpy(a) for a in Pr2], [hip.to_numpy(a) for a in D2])
        mg.close()
        return out
    return run


def test_two_multigpu_objects_on_two_threads(hip, two_threads_first):
    """each thread owns a MultiGpu of two virtual z-slab ranks on device 0 and runs the (2, (40, 21, 10)) case of
    tests/test_gpu_mgpu.py::test_slab_state_equals_global_solve (slab_load / plan / iterate / store, as that test does), then
    ns3d_pt_solve_slab from the same start: both leave the planes of the global solve, with its iteration count and residuals"""
    from test_gpu_mgpu import _global_solve
    P, (nx, ny, nz), n_iters, bc = SLAB
    g, (Pg, Dg, Rg) = _slab_inputs()
    Pref, Dref = _global_solve(hip, Pg, Dg, Rg, g, n_iters, bc, np.float64)
    b = _barrier(2, SCRIPT_SECONDS["slab solve"])
    done = run_threads([_slab_worker(hip, b), _slab_worker(hip, b)], SCRIPT_SECONDS["slab solve"])
    ctx = hip.Context(0, "strict")
    dP, dD = hip.from_numpy(Pg), hip.from_numpy(Dg)
    pg = hip.pt_params(dP, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, *bc)
    it_ref, errs_ref = hip.pt_solve(dP, dD, hip.from_numpy(Rg), pg, *SLAB_SOLVE, ctx=ctx)
    ctx.sync()
    Psol, Dsol = hip.to_numpy(dP), hip.to_numpy(dD)
    ctx.close()
    assert it_ref == 12 and len(errs_ref) == 2
    for t, (Pr, D, it, errs, Pr2, D2) in enumerate(done):
        assert (it, errs) == (it_ref, errs_ref), "thread %d: pt_solve_slab made %r, the global solve %r" % (t, (it, errs), (it_ref, errs_ref))
        for r in range(P):
            lo = r * (nz - 2)
            assert np.array_equal(Pr[r], Pref[:, :, lo:lo + nz]), "thread %d: Pr of rank %d" % (t, r)
            assert np.array_equal(D[r], Dref[:, :, lo:lo + nz - 2]), "thread %d: dPrdτ of rank %d" % (t, r)
            assert np.array_equal(Pr2[r], Psol[:, :, lo:lo + nz]), "thread %d: pt_solve_slab's Pr of rank %d" % (t, r)
            assert np.array_equal(D2[r], Dsol[:, :, lo:lo + nz - 2]), "thread %d: pt_solve_slab's dPrdτ of rank %d" % (t, r)


def _duration_scripts(hip):
    """label of SCRIPT_SECONDS → the script a worker of that test runs, as a callable"""
    def script(mode, ops, repeat=1):
        def fn():
            ctx = CS.make_context(hip, mode)
            ctx.use_own_stream()
            for _ in range(repeat):
                CS.run(ops, ctx)
            ctx.close()
        return fn

    def errors():
        import api_error_cases as AE
        from navierstokes3d_amd import lib as L
        cases = {label: (fn, mods) for label, fn, mods, only in AE.cases() if "f64" in only}
        ctx, arena = hip.Context(0, "strict"), AE.Arena(L, "f64")
        for _ in range(50):
            for label in ("update_Pr:small_x", "pt_solve:negative_niter"):
                AE.run_case(L, ctx.handle, arena, "f64", *cases[label])
        ctx.close()
    e, f = _direct_ops()
    return {"all value ops, strict": script("strict", CS.value_ops("strict")), "all value ops, fast": script("fast", CS.value_ops("fast")),
            "pt_iterate on G2, first use": script("strict", [_g2_op("f32")]),
            "small ops x 20": script("strict", [CS.OPS[n] for n in CS.SMALL_OPS], 20), "direct solves E F": script("strict", [e, f, e]),
            "slab solve": _slab_worker(hip),
            "create, solve on A, destroy x 40": lambda: [script("strict", [CS.OPS["pt_solve_graph:A:f64"]])() for _ in range(40)],
            "argument errors x 50": errors}


def one_duration(label):
    """seconds of one script in THIS process, which has done nothing on the GPU yet but create a tensor"""
    import torch
    from navierstokes3d_amd import kernels as hip
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    fn = _duration_scripts(hip)[label]
    t0 = time.monotonic()
    fn()
    torch.cuda.synchronize()
    print("SCRIPT_SECONDS %-36s %.2f" % (label, time.monotonic() - t0), flush=True)


def gpu_durations():
    """The figures of SCRIPT_SECONDS: every script in a child process of its own, one after the other, under the suite's
    NS3D_COOP_CHECK=1.  On the GPU machine, from the repository root:
        python -c "import sys; sys.path.insert(0, 'tests'); import test_gpu_host_threads as T; T.gpu_durations()" """
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NS3D_COOP_CHECK="1")
    for label in SCRIPT_SECONDS:
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_host_threads as T; T.one_duration(%r)" % (here, os.path.dirname(here), label)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        print(r.stdout.strip() if r.returncode == 0 else "%s: exit %d\n%s" % (label, r.returncode, r.stderr[-2000:]), flush=True)
        if r.returncode != 0:
            break
