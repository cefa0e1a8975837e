"""One context, kept for a whole program: the entry points that keep state in it, every grid, element type, knob and stream in turn (tests/ctx_script.py).
What the context remembers between calls — ping-pong buffers, HIP graphs, k_pt_persist's exchange area, the pace counters, the
direct-solve plan, monitor and isosurface scratch, the key word, last_* and the knobs — must never show in a result:
every op returns the bits it returns alone on a fresh context."""
import numpy as np
import pytest

import ctx_script as CS

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)


def _run_compared(hip, script, mode, ctx=None):
    """the script on one context of `mode`, every value op compared with its reference; returns (results, context)"""
    ctx = ctx or CS.make_context(hip, mode)
    results = CS.run(script, ctx, mode)
    assert len(results) == sum(op.value for op in script), "a value op of the script was not executed and compared"
    return results, ctx


def test_one_context_through_the_hostile_order(hip):
    """graphs → ping-pong growth → graphs again; persist → CUs reserved → persist → released; paced C, D, C at another pace, C in
    fp32 on the same counters; direct solve E, F, E; 19 graph solves past the cache's wipe, another stream, the 19 again; G with
    autotune on (its first planned use, when this test is the first of the process to run G: it stands first in the module), off,
    on; time_step between two pt_solve calls on one key word; fp32 and fp64 alternating on one grid; the MacCormack step: its hat
    scratch allocated on A between two graph solves, grown on B (the graphs go), A again in the larger buffer, float32, the knob
    off, the knob left on in front of the single calls, the own stream and then a side stream, CUs reserved"""
    script = CS.hostile_script()
    results, ctx = _run_compared(hip, script, "strict")
    assert len(results) == sum(op.value for op in script) == 76
    assert {op.name for op in script if op.value} >= {op.name for op in CS.value_ops("strict") + CS.mc_ops("strict")}
    assert ctx.advection() == "reference", "the script's last word on the knob"
    assert ctx.persist_faults() == 0
    ctx.close()


def test_references_reach_the_paths_their_ops_are_named_for(hip):
    """a comparison of an op with itself proves nothing unless the op does what its name says: on fresh contexts the paced ops
    report their pace_z, the graph ops leave instantiated graphs behind, G runs in the planner's regime and its choice is shared, every
    solve runs its 25 iterations and 3 checks, every output moved and is finite"""
    for name, pace in (("pt_sweepn4_v2900_pace8:C:f64", 8), ("pt_sweepn4_v2900_pace8:C:f32", 8), ("pt_sweepn4_v2900_pace8:D:f64", 8),
                       ("pt_sweepn4_v2900_pace16:C:f64", 16)):
        assert dict(CS.reference(CS.OPS[name], "strict"))["last_pt_pace"][0] == pace, name
    ctx = CS.make_context(hip, "strict")
    CS.gpu_execute(CS.OPS["pt_solve_graph:A:f64"], ctx)
    assert 1 <= int(ctx.lib.ns3d_cached_graphs(ctx.handle)) <= 4
    many = dict(CS.gpu_execute(CS.OPS["pt_solve_many_params:A:f64"], ctx))
    assert many["blocks are held as graphs, fewer than the wipe's 16"][0] == 1.0
    assert not np.array_equal(many["solve 0: Pr"], many["solve 1: Pr"]) and np.array_equal(many["solve 0: Pr"], many["solve 18: Pr"])
    CS.gpu_execute(CS.OPS["pt_iterate:G:f64"], ctx)
    assert int(ctx.lib.ns3d_cached_graphs(ctx.handle)) == 0, "G's larger ping-pong buffers replace A's: the graphs captured on those go"
    # (the planner's choice may be 0, the built-in shape, which wins ties: what shows is that G runs as two-iteration passes, the
    # regime in which the planner decides, and that a second context gets the first one's choice)
    assert ctx.last_pt_depth() == 2, "G's passes were not planned"
    other = CS.make_context(hip, "strict")
    CS.gpu_execute(CS.OPS["pt_iterate:G:f64"], other)
    assert other.last_pt2_variant() == ctx.last_pt2_variant() and other.last_pt_depth() == 2
    other.close()
    CS.gpu_execute(CS.OPS["pt_iterate_depth4:D:f64"], ctx)
    assert ctx.last_pt_depth() == 4 or ctx.last_pt_depth() == 3          # 7 iterations = 4 + 3
    ctx.close()
    for op in CS.VALUE_OPS:
        res = dict(CS.reference(op, "strict"))
        inp = op.inputs()
        for label, a in res.items():
            assert np.isfinite(a).all(), (op.name, label)
            if label.endswith(" unchanged"):
                key = label[:-len(" unchanged")].split(": ")[-1]
                key = {"Pr_in": "Pr0", "dPrdtau_in": "d0"}.get(key, key)
                assert np.array_equal(a, inp[key]), (op.name, label)
        if "iterations, err history" in res and op.name.startswith("pt_solve"):
            rec = res["iterations, err history"]
            assert rec[0] == 25 and len(rec) == 4 and (rec[1:] > 0).all(), (op.name, rec)
        if op.name.startswith("time_step"):
            rec = res["iterations, err history"]
            assert len(rec) >= 2 and (rec[0] > 0 or op.name.endswith("pressure1:A:f64")), (op.name, rec)
        for out, src in (("Pr", "Pr0"), ("dPrdtau", "d0"), ("Pr_out", "Pr0")):
            if out in res and src in inp:
                assert not np.array_equal(res[out], inp[src]), (op.name, out)
    iso = dict(CS.reference(CS.OPS["isosurface:AE:f64"], "strict"))
    assert iso["A: triangle counts"][0] == iso["A: triangle counts"][1] > 100 and iso["E: triangle counts"][0] > iso["A: triangle counts"][0]
    assert (iso["E: tri"] >= 0).all()


def test_maccormack_references_reach_what_their_ops_are_named_for(hip):
    """On fresh contexts: every MacCormack op's outputs are finite and moved, its inputs are unchanged; the steps iterate, swap all
    eight names, keep C in [0, 1] and differ from the reference step of the same script and solve; the two forms of the single call
    agree with each other on equal inputs — and the hat scratch grows from A to B, which wipes the graphs, and not again for A."""
    swapped = list(range(8))
    for op in CS.MC_OPS:
        res = dict(CS.reference(op, "strict"))
        inp = op.inputs()
        for label, a in res.items():
            assert np.isfinite(a).all(), (op.name, label)
            if label.endswith(" unchanged"):
                assert np.array_equal(a, inp[label[:-len(" unchanged")]]), (op.name, label)
        if op.name.startswith("time_step"):
            rec = res["iterations, err history"]
            assert len(rec) >= 2 and (rec[0] > 0 or "pressure1" in op.name), (op.name, rec)
            names = list(CS.STEP_SHAPES)
            ends = [names[int(q)] for q in next(v for k, v in res.items() if k.startswith("the buffer each of"))]
            assert ends == ["Vx", "Vy", "Vz", "C_o", "Vx_o", "Vy_o", "Vz_o", "C"], (op.name, ends)     # V: two swaps; C: one
            new_c = res["buffer C_o"]
            assert new_c.min() >= 0.0 and new_c.max() <= 1.0 and np.abs(res["buffer Vx"]).max() > 0, op.name
            twin = op.name.replace("_mc_", "_")
            if twin in CS.OPS:
                assert not np.array_equal(dict(CS.reference(CS.OPS[twin], "strict"))["buffer Vx"], res["buffer Vx"]), op.name
        else:
            for n in CS.MC_NAMES:
                assert not np.array_equal(res[n], inp[n + "_o"]) and not np.array_equal(res[n + "_hat"], res[n]), (op.name, n)
    ctx = CS.make_context(hip, "strict")
    CS.gpu_execute(CS.OPS["set_graph_mode(1)"], ctx)
    CS.gpu_execute(CS.OPS["pt_solve_graph:A:f64"], ctx)
    held = int(ctx.lib.ns3d_cached_graphs(ctx.handle))
    assert held >= 1
    CS.gpu_execute(CS.OPS["time_step_multi_mc_pressure0:A:f64"], ctx)
    assert int(ctx.lib.ns3d_cached_graphs(ctx.handle)) >= held, "the hat's first allocation frees nothing"
    CS.gpu_execute(CS.OPS["time_step_multi_mc_pressure0:B:f64"], ctx)
    after_b = int(ctx.lib.ns3d_cached_graphs(ctx.handle))
    assert after_b == 0, "the hat grew behind the step's solve: the old buffer was freed and every graph went with it"
    CS.gpu_execute(CS.OPS["pt_solve_graph:A:f64"], ctx)
    CS.gpu_execute(CS.OPS["time_step_multi_mc_pressure0:A:f32"], ctx)
    assert int(ctx.lib.ns3d_cached_graphs(ctx.handle)) >= max(1, after_b), "a smaller hat fits the buffer: nothing is freed, no graph goes"
    ctx.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
def test_maccormack_ops_through_seeded_orders(hip, mode, seed):
    """the MacCormack ops of the mode among its A- to F-sized value ops, in a seeded order with setting ops between them — the
    advection knob's among them — on one context: every op returns its reference, so no op but a named time step reads the knob
    and no step reads anything but its own"""
    ops = [op for op in CS.value_ops(mode) if ":G:" not in op.name] + CS.mc_ops(mode)
    script = CS.seeded_script(seed, mode, ops=ops)
    assert sum(op.value for op in script) == len(ops) == (40 if mode != "fast" else 20)
    results, ctx = _run_compared(hip, script, mode)
    assert ctx.persist_faults() == 0
    ctx.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", ["strict", "ieee", "fast"])
def test_one_context_through_seeded_orders(hip, mode, seed):
    """a seeded permutation of all value ops of the mode with setting ops between them, on one context; afterwards the context
    still passes one op of each kind, no cooperative launch was voided, and a SECOND context returns the reference bits for G
    (the plan the first one tuned answers its look-up)"""
    script = CS.seeded_script(seed, mode)
    assert sum(op.value for op in script) == len(CS.value_ops(mode)) == (32 if mode != "fast" else 18)
    results, ctx = _run_compared(hip, script, mode)
    assert ctx.persist_faults() == 0
    again = [CS.OPS[n] for n in CS.ONE_OF_EACH_KIND if CS.OPS[n].fast or mode != "fast"]
    if mode != "fast":
        again += [CS.OPS[n] for n in ("poisson_direct:EFE:f64", "diagnostics:AE:f64", "isosurface:AE:f64", "residual_max+max_abs:AE:f64",
                                      "time_step_multi_pressure0:A:f64")]
    _run_compared(hip, [CS.OPS["use_torch_stream()"], CS.OPS["reserve_cus(0)"]] + again, mode, ctx)
    assert ctx.persist_faults() == 0
    ctx.close()
    _, second = _run_compared(hip, [CS.OPS["pt_iterate:G:f64"], CS.OPS["pt_iterate:G:f32"]], mode)
    second.close()


def _small_round(hip):
    """a context created, run through the A-, B- and C-sized ops and closed; returns the device's free memory afterwards"""
    import torch
    ctx = CS.make_context(hip, "strict")
    CS.run([CS.OPS[n] for n in CS.SMALL_OPS], ctx, "strict")
    ctx.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                 # PyTorch's cached blocks go back: what remains is what the library holds
    return torch.cuda.mem_get_info()[0]


# The allocator's granule, MEASURED 2026-10-20 on an MI355X through torch.cuda.mem_get_info around eight hipMalloc calls of one size:
# 1 B, 4 KiB and 64 KiB each: free memory does not move (served from a pool the runtime already holds); 1 MiB each: it falls by
# 1 MiB per call; 2 MiB + 1 B each: by 4 MiB per call — large allocations are rounded up to multiples of 2 MiB, the coarsest step seen.
# The ten rounds themselves, on the parent commit's library and on this one: free memory after every round equal to the first round's
# to the byte (308 352 647 168 of 309 220 868 096 bytes, ten times).
GRANULE = 2 << 20


def test_a_closed_context_leaves_the_next_one_alone(hip):
    """The hostile script on a context, the context closed, a new one created, the script again: the same results (both equal
    the references, op for op).  And closing gives everything back: after ten create–run–close rounds of the A-, B- and C-sized ops
    the device's free memory (torch.cuda.mem_get_info) is not lower than after the first round, within one allocator granule.

    The margin is one allocator granule, 2 MiB: measured, not assumed (GRANULE above) — on the parent commit's library the ten
    rounds left free memory where the first round left it, to the byte, and so does this one."""
    script = CS.hostile_script()
    first, ctx = _run_compared(hip, script, "strict")
    ctx.close()
    second, ctx = _run_compared(hip, script, "strict")
    ctx.close()
    assert first.keys() == second.keys()
    for key in first:
        assert CS.difference(second[key], first[key]) is None, key
    free = [_small_round(hip) for _ in range(10)]
    print("free memory after each round, relative to the first: %r" % [f - free[0] for f in free])
    assert free[-1] >= free[0] - GRANULE, (free[0] - free[-1], free)


def test_set_stream_waits_for_the_stream_it_leaves(hip):
    """include/ns3d.h: ns3d_set_stream, ns3d_use_own_stream and ns3d_reserve_cus wait for the stream the context leaves.  An
    NS3D_ASYNC context with a pass queued behind a delay on one stream is moved to another: on return the first stream is idle,
    and a larger grid — whose first call frees the ping-pong buffers the queued pass runs in — returns its reference bits, as does
    the queued pass."""
    import torch
    import stream_order as SO
    small, big = CS.OPS["pt_iterate_depth3:C:f64"], CS.OPS["pt_iterate_depth4:D:f64"]
    want_small, want_big = CS.reference(small, "strict"), CS.reference(big, "strict")
    delay = SO.Delay(ms=20.0)
    for move in ("set_stream", "use_own_stream", "reserve_cus"):
        ctx = hip.Context(0, "strict", async_=True)
        s1 = torch.cuda.Stream(0)
        ctx.use_torch_stream(s1, pin=True)
        ctx.set_pt_depth(3); ctx.set_persist_mode(0); ctx.set_graph_mode(0)
        inp = small.inputs()
        dP, dD, dR = (hip.from_numpy(inp[n]) for n in ("Pr0", "d0", "rhs"))
        torch.cuda.synchronize()
        delay.enqueue(s1)
        hip.pt_iterate(dP, dD, dR, CS._ptp(hip, dP, CS.GRIDS["C"]), 7, ctx=ctx)         # queued behind the delay: the call only enqueues
        assert not s1.query(), "the delay ended before the context moved: nothing was queued on the stream it leaves"
        if move == "set_stream":
            ctx.use_torch_stream(torch.cuda.Stream(0), pin=True)
        elif move == "use_own_stream":
            ctx.use_own_stream()
        else:
            ctx.reserve_cus(32)
        assert s1.query(), "%s returned while the stream it left was still running the context's work" % move
        got_big = CS.gpu_execute(big, ctx)
        assert CS.difference(got_big, want_big) is None, (move, CS.difference(got_big, want_big))
        got_small = [("Pr", hip.to_numpy(dP)), ("dPrdtau", hip.to_numpy(dD)), ("rhs unchanged", hip.to_numpy(dR))]
        assert CS.difference(got_small, want_small) is None, (move, CS.difference(got_small, want_small))
        if move == "reserve_cus":
            ctx.reserve_cus(0)
        ctx.close()


def test_a_context_follows_the_caller_into_a_capture(hip):
    """include/ns3d.h: while the stream moved TO is being captured there is no wait — a synchronisation of the stream left, made by
    the capturing thread, would invalidate the caller's capture.  An NS3D_ASYNC context on PyTorch's default stream follows it into
    a torch.cuda.graph capture (ns3d_set_stream to the capturing stream), enqueues advect there, and leaves again; the replayed
    graph gives the reference's bits."""
    import torch
    op = CS.OPS["advect:A:f64"]
    want = dict(CS.reference(op, "strict"))
    g = CS._geom(CS.GRIDS["A"])
    inp = op.inputs()
    names = ("Vx_o", "Vy_o", "Vz_o", "C_o")
    old = [hip.from_numpy(inp[n]) for n in names]
    new = [hip.from_numpy(np.full_like(inp[n], 7.0)) for n in names]
    ctx = hip.Context(0, "strict", async_=True)
    hip.advect(new[0], old[0], new[1], old[1], new[2], old[2], new[3], old[3], g["dt"], g["dx"], g["dy"], g["dz"], True, ctx=ctx)   # modules loaded
    ctx.sync()
    for t, n in zip(new, names):
        t.copy_(hip.from_numpy(inp[n]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.advect(new[0], old[0], new[1], old[1], new[2], old[2], new[3], old[3], g["dt"], g["dx"], g["dy"], g["dz"], True, ctx=ctx)
    torch.cuda.synchronize()
    assert all(np.array_equal(hip.to_numpy(t), inp[n]) for t, n in zip(new, names)), "a captured call must not run"
    graph.replay()
    torch.cuda.synchronize()
    for t, label in zip(new, ("Vx", "Vy", "Vz", "C")):
        assert CS.difference([(label, hip.to_numpy(t))], [(label, want[label])]) is None, label
    ctx.use_torch_stream()                  # back on the default stream: the capture stream left is idle and is waited for
    ctx.close()
