"""tests/ctx_script.py on the CPU, with a fake executor in place of the library: the scripts hold what they claim to hold, their
order is a function of the seed, an op's inputs are a function of its name, and a result that differs from its reference is
reported by op, array and index."""
import zlib

import numpy as np
import pytest

import ctx_script as CS

SEEDS = (11, 12, 13)                  # the seeds of tests/test_gpu_context_history.py
SMALL = [op for op in CS.VALUE_OPS if ":G:" not in op.name]


class FakeCtx:
    def __init__(self, mode):
        self.mode, self.log = mode, []

    def close(self):
        self.log.append("closed")


_digests = {}


def _digest(op):
    if op.name not in _digests:
        _digests[op.name] = [(label, np.asarray([zlib.crc32(np.ascontiguousarray(a).tobytes())], dtype=np.int64))
                             for label, a in sorted(op.inputs().items())]
    return _digests[op.name]


def fake(op, ctx):
    """a value op returns one digest per input array; a setting op is logged"""
    ctx.log.append(op.name)
    return _digest(op) if op.value else None


def test_every_value_op_is_in_every_script():
    strict = {op.name for op in CS.value_ops("strict")}
    assert len(strict) == len(CS.VALUE_OPS) == 32
    assert {op.name for op in CS.hostile_script() if op.value} >= strict
    for mode in CS.MODES:
        want = sorted(op.name for op in CS.value_ops(mode))
        for seed in SEEDS:
            for settings in (True, False):
                s = CS.seeded_script(seed, mode, settings)
                assert sorted(op.name for op in s if op.value) == want, (mode, seed)          # each exactly once
                assert any(not op.value for op in s) == settings
    fast = {op.name for op in CS.value_ops("fast")}
    assert fast < strict and all(CS.OPS[n].fast for n in fast)
    # what the issue marks for both element types and FAST
    for stem in ("pt_iterate:A", "pt_iterate:B", "pt_iterate:G", "pt_iterate_depth3:C", "pt_sweepn4_v2900_pace8:C", "pt_solve_graph:A",
                 "pt_solve_persist:B", "advect:A", "predict_fused:A"):
        assert {stem + ":f64", stem + ":f32"} <= fast, stem
    for name in CS.SMALL_OPS + CS.ONE_OF_EACH_KIND:
        assert CS.OPS[name].value


def test_the_hostile_script_holds_every_transition():
    names = [op.name for op in CS.hostile_script()]
    at = names.index

    def after(first, *rest):
        q = at(first)
        for n in rest:
            q = names.index(n, q + 1)
        return True
    assert after("pt_solve_graph:A:f64", "set_autotune(0)", "pt_iterate:G:f64", "pt_solve_graph:A:f64")
    assert names.index("set_autotune(1)") > at("pt_iterate:G:f64"), "G's first use with autotune on is step 6's"
    assert sorted(op.name for op in CS.VALUE_OPS + CS.MC_OPS if op.cooperative) == sorted(n for n in CS.OPS if ":B:" in n) and \
        len([op for op in CS.value_ops("fast") if op.cooperative]) == 4 and len([op for op in CS.VALUE_OPS if op.cooperative]) == 4
    assert after("pt_solve_persist:B:f64", "reserve_cus(32)", "pt_solve_persist:B:f64", "reserve_cus(0)")
    assert after("pt_sweepn4_v2900_pace8:C:f64", "pt_sweepn4_v2900_pace8:D:f64", "pt_sweepn4_v2900_pace16:C:f64", "pt_sweepn4_v2900_pace8:C:f32")
    assert after("pt_solve_many_params:A:f64", "use_own_stream()", "pt_solve_many_params:A:f64")
    assert after("set_autotune(1)", "pt_iterate:G:f64", "set_autotune(0)", "pt_iterate:G:f64", "set_autotune(1)", "pt_iterate:G:f64")
    assert after("pt_solve_graph:A:f64", "time_step_multi_pressure0:A:f64", "pt_solve_persist:B:f64")
    assert after("pt_iterate:A:f64", "pt_iterate:A:f32", "pt_solve_graph:A:f64")
    assert all(n in CS.OPS for n in names)
    # the MacCormack block, in the issue's order: a graph on A, the step on A (the hat's first use), on B (the hat grows, the graphs
    # go), the graph again, A in the larger buffer, float32, the reference step, the knob left on in front of ops that must not read
    # it, the own stream and then the side stream, CUs reserved
    mc = "time_step_multi_mc_pressure0:A:f64"
    start = names.index("set_pt_pace(-1)")
    assert mc not in names[:start] and names[start + 1] == "set_graph_mode(1)"
    block = names[start + 1:]
    assert names.index("set_graph_mode(1)", start) == start + 1

    def then(*seq):
        q = -1
        for n in seq:
            q = block.index(n, q + 1)
        return True
    assert then("set_graph_mode(1)", "pt_solve_graph:A:f64", mc, "time_step_multi_mc_pressure0:B:f64", "pt_solve_graph:A:f64", mc,
                "time_step_multi_mc_pressure0:A:f32", "time_step_multi_pressure0:A:f64", "set_advection(1)", "advect:A:f64", "advect_mc:A:f64",
                "use_own_stream()", mc, "use_torch_stream(side_stream)", mc, "reserve_cus(32)", mc, "reserve_cus(0)")
    first_b = block.index("time_step_multi_mc_pressure0:B:f64")
    assert not any(":B:" in n or ":f32" in n for n in block[:first_b]), "the hat's first use is A's, in float64"
    assert block[block.index("set_advection(1)") + 1:block.index("use_own_stream()")] == [
        "advect:A:f64", "advect_mc:A:f64", "advect_mc:A:f32", "copy_advect+advect_correct:A:f64", "copy_advect+advect_correct:A:f32",
        "predict_fused:A:f64", "pt_solve_graph:A:f64"], "nothing between set_advection(1) and these ops turns the knob off"
    assert block[-3:] == [mc, "set_advection(0)", "set_graph_mode(-1)"] and block.count(mc) == 6


def test_the_maccormack_ops():
    """their names, which of them a FAST context runs, that a script built from them holds each once, and that the hostile script
    and the one-of-each list carry them; their inputs"""
    names = [op.name for op in CS.MC_OPS]
    assert names == ["time_step_multi_mc_pressure0:A:f64", "time_step_multi_mc_pressure1:A:f64", "time_step_gpu_mc_pressure0:A:f64",
                     "time_step_gpu_mc_pressure1:A:f64", "time_step_multi_mc_pressure0:B:f64", "time_step_multi_mc_pressure0:A:f32",
                     "advect_mc:A:f64", "advect_mc:A:f32", "copy_advect+advect_correct:A:f64", "copy_advect+advect_correct:A:f32"]
    assert all(op.value and CS.OPS[op.name] is op for op in CS.MC_OPS) and not set(names) & {op.name for op in CS.VALUE_OPS}
    assert [op.name for op in CS.mc_ops("fast")] == names[6:] and CS.mc_ops("strict") == CS.mc_ops("ieee") == CS.MC_OPS
    assert [op.name for op in CS.MC_OPS if op.cooperative] == ["time_step_multi_mc_pressure0:B:f64"]
    hat = lambda n: (n[0] + 1) * n[1] * n[2] + n[0] * (n[1] + 1) * n[2] + n[0] * n[1] * (n[2] + 1) + n[0] * n[1] * n[2]
    assert CS.GRIDS["B"] == (63, 38, 38) and 15.5 < hat(CS.GRIDS["B"]) / hat(CS.GRIDS["A"]) < 16.5     # the hat grows 16-fold from A to B
    assert {op.name for op in CS.hostile_script() if op.value} >= set(names)
    assert "time_step_multi_mc_pressure0:A:f64" in CS.ONE_OF_EACH_KIND
    for mode in CS.MODES:
        mixed = [op for op in CS.value_ops(mode) if ":G:" not in op.name] + CS.mc_ops(mode)
        orders = []
        for seed in SEEDS:
            sc = CS.seeded_script(seed, mode, ops=mixed)
            assert sorted(op.name for op in sc if op.value) == sorted(op.name for op in mixed), (mode, seed)
            assert [op.name for op in sc] == [op.name for op in CS.seeded_script(seed, mode, ops=mixed)]
            orders.append([op.name for op in sc])
        assert orders[0] != orders[1] != orders[2] != orders[0]
    # the knob's setting ops are among those the seeded scripts draw, the scripts of all value ops included
    assert {"set_advection(0)", "set_advection(1)"} <= {op.name for op in CS.SETTING_OPS}
    drawn = {op.name for mode in CS.MODES for seed in range(40) for op in CS.seeded_script(seed, mode) if not op.value}
    assert {"set_advection(0)", "set_advection(1)"} <= drawn
    # seeds and inputs: a function of the name; float32 ops get float32 arrays, the B step B's shapes
    seeds = {op.name: CS.seed_of(op.name) for op in CS.VALUE_OPS + CS.MC_OPS}
    assert len(set(seeds.values())) == len(seeds)
    for op in CS.MC_OPS:
        a, b = op.inputs(), op.inputs()
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a), op.name
        assert all(v.dtype == (np.float32 if op.name.endswith(":f32") else np.float64) and v.flags.f_contiguous for v in a.values()), op.name
    f32 = CS.OPS["time_step_multi_mc_pressure0:A:f32"].inputs()
    assert f32["Vx"].shape == (25, 15, 15) and f32["Vy"][0].max() == 1.0
    assert CS.OPS["time_step_multi_mc_pressure0:B:f64"].inputs()["Vz"].shape == (63, 38, 39)
    a, b = CS.OPS["advect_mc:A:f32"].inputs(), CS.OPS["copy_advect+advect_correct:A:f32"].inputs()
    assert a.keys() == b.keys() == {"Vx_o", "Vy_o", "Vz_o", "C_o"} and not np.array_equal(a["C_o"], b["C_o"])


class KnobCtx(FakeCtx):
    """a context that remembers the advection knob as the library does"""

    def __init__(self, mode, scheme="reference"):
        super().__init__(mode)
        self.scheme = scheme

    def set_advection(self, scheme):
        assert scheme in ("reference", "maccormack")
        self.scheme = scheme


def test_time_step_ops_pin_the_knob_they_name():
    """every time_step op sets the scheme of its name first, whatever the script left, and it stays behind; the setting ops set what
    they say.  (The ops' device calls are not reached: the library object handed in raises at its first use, behind the knob.)"""
    class Reached(Exception):
        pass

    class NoLibrary:
        def __getattr__(self, name):
            raise Reached(name)
    steps = [op for op in CS.VALUE_OPS + CS.MC_OPS if op.name.startswith("time_step")]
    assert len(steps) == 10
    for op in steps:
        for left in ("reference", "maccormack"):
            ctx = KnobCtx("strict", left)
            ctx.after_torch_fill = lambda: None
            with pytest.raises(Reached):
                op.call(NoLibrary(), ctx, op.inputs())
            assert ctx.scheme == ("maccormack" if "_mc_" in op.name else "reference"), (op.name, left)
    ctx = KnobCtx("strict")
    for v, want in ((1, "maccormack"), (0, "reference"), (1, "maccormack")):
        CS.OPS["set_advection(%d)" % v].call(None, ctx, {})
        assert ctx.scheme == want


def test_shuffles_are_reproducible_from_their_seed():
    for mode in CS.MODES:
        orders = [[op.name for op in CS.seeded_script(seed, mode)] for seed in SEEDS]
        again = [[op.name for op in CS.seeded_script(seed, mode)] for seed in SEEDS]
        assert orders == again
        assert orders[0] != orders[1] != orders[2] != orders[0]
        assert [n for n in orders[0] if CS.OPS[n].value] != sorted(n for n in orders[0] if CS.OPS[n].value)


def test_inputs_depend_on_the_name_not_on_the_position():
    seeds = {op.name: CS.seed_of(op.name) for op in CS.VALUE_OPS}
    assert len(set(seeds.values())) == len(seeds)
    for op in SMALL:
        a, b = op.inputs(), op.inputs()
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a), op.name
    small = {op.name for op in SMALL}
    scripts = [[op for op in CS.seeded_script(seed, "strict") if not op.value or op.name in small] for seed in SEEDS[:2]]
    assert [op.name for op in scripts[0]] != [op.name for op in scripts[1]]
    _digests.clear()
    first = CS.run(scripts[0], FakeCtx("strict"), execute=fake)
    _digests.clear()                                  # the second script draws every input again, at another position
    second = CS.run(scripts[1], FakeCtx("strict"), execute=fake)
    assert first.keys() == second.keys() == small
    for name in small:
        assert CS.difference(first[name], second[name]) is None, name
    # two ops of one kind on one grid do not share inputs
    assert CS.difference(first["pt_iterate:A:f64"], first["pt_solve_graph:A:f64"]) is not None


def test_run_executes_in_order_and_names_repeats():
    ops = [CS.OPS[n] for n in ("set_graph_mode(1)", "advect:A:f64", "reserve_cus(32)", "advect:A:f64", "predict_fused:A:f32", "advect:A:f64")]
    ctx = FakeCtx("strict")
    names = {}
    out = CS.run(ops, ctx, execute=fake, names_out=names)
    assert ctx.log == [op.name for op in ops]
    assert list(out) == ["advect:A:f64", "advect:A:f64#2", "predict_fused:A:f32", "advect:A:f64#3"]
    assert names["advect:A:f64#3"] == "advect:A:f64" and len(out) == sum(op.value for op in ops)


def test_run_reports_the_op_the_array_and_the_index():
    """an executor whose second call of an op flips one bit of one array: the reference (a fresh context, first call) differs"""
    calls = {}

    def flaky(op, ctx):
        if not op.value:
            return None
        calls[op.name] = calls.get(op.name, 0) + 1
        a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
        b = np.ones(5, dtype=np.float32)
        if op.name == "advect:A:f32" and not getattr(ctx, "fresh", False):
            a[1, 2, 1] = np.nextafter(a[1, 2, 1], np.inf)
        return [("first", b), ("second", a)]

    def make(mode):
        ctx = FakeCtx(mode)
        ctx.fresh = True
        return ctx
    script = [CS.OPS[n] for n in ("advect:A:f64", "set_pt_pace(8)", "advect:A:f32", "predict_fused:A:f64")]
    with pytest.raises(CS.Mismatch) as e:
        CS.run(script, FakeCtx("strict"), "strict", execute=flaky, make=make)
    msg = str(e.value)
    assert "1 of 3 results" in msg and "op 'advect:A:f32'" in msg and "array 'second'" in msg and "index (1, 2, 1)" in msg
    assert "advect:A:f64" not in msg and "predict_fused" not in msg
    good = [CS.OPS[n] for n in ("advect:A:f64", "predict_fused:A:f64")]
    assert len(CS.run(good, FakeCtx("strict"), "strict", execute=flaky, make=make)) == 2
    # a result with other entries, another shape or another type is a difference too
    assert "entries" in CS.difference([("x", np.zeros(2))], [("y", np.zeros(2))])
    assert CS.difference([("x", np.zeros(2))], [("x", np.zeros(3))]) and CS.difference([("x", np.zeros(2))], [("x", np.zeros(2, np.float32))])
    assert CS.difference([("x", np.array([0.0]))], [("x", np.array([-0.0]))]) is not None            # bits, not values
    assert CS.difference([("x", np.array([np.nan]))], [("x", np.array([np.nan]))]) is None
