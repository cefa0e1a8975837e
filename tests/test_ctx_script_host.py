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
    assert sorted(op.name for op in CS.VALUE_OPS if op.cooperative) == sorted(n for n in CS.OPS if ":B:" in n) and \
        len([op for op in CS.value_ops("fast") if op.cooperative]) == 4
    assert after("pt_solve_persist:B:f64", "reserve_cus(32)", "pt_solve_persist:B:f64", "reserve_cus(0)")
    assert after("pt_sweepn4_v2900_pace8:C:f64", "pt_sweepn4_v2900_pace8:D:f64", "pt_sweepn4_v2900_pace16:C:f64", "pt_sweepn4_v2900_pace8:C:f32")
    assert after("pt_solve_many_params:A:f64", "use_own_stream()", "pt_solve_many_params:A:f64")
    assert after("set_autotune(1)", "pt_iterate:G:f64", "set_autotune(0)", "pt_iterate:G:f64", "set_autotune(1)", "pt_iterate:G:f64")
    assert after("pt_solve_graph:A:f64", "time_step_multi_pressure0:A:f64", "pt_solve_persist:B:f64")
    assert after("pt_iterate:A:f64", "pt_iterate:A:f32", "pt_solve_graph:A:f64")
    assert all(n in CS.OPS for n in names)


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
