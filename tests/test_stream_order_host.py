"""The pure parts of tests/stream_order.py (the harness of test_gpu_stream_order.py), on the host: the decoy generator, the delay's op
count, the diagnosis of a failure and the verdict's order.  No GPU, no torch."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import stream_order as SO
from util import SHAPES, fields, rnd

GRIDS = [(24, 15, 15), (70, 6, 7), (17, 9, 5), (3, 3, 3)]


def _arrays(grid, dtype):
    kinds = ["c", "vx", "vy", "vz", "s", "i"]
    out = [(k, a, "field") for k, a in zip(kinds, fields(*grid, kinds, 1, dtype))]
    rng = np.random.Generator(np.random.MT19937(3))
    n = 300
    out.append(("X", np.ascontiguousarray(rng.uniform(size=(3, n)) * np.array(grid, dtype=np.float64).reshape(3, 1)), ("points", grid)))
    out.append(("state", (rng.uniform(size=n) < 0.8).astype(np.uint8), "state"))
    out.append(("zeros", np.zeros(SHAPES["c"](*grid), dtype=dtype, order="F"), "field"))          # a field at rest
    out.append(("prefill", np.full(9 * 41, 777.0), "field"))                                          # an output's prefill
    out.append(("gentle", np.zeros(SHAPES["vx"](*grid), dtype=dtype, order="F"), ("field", 1e-2)))   # a time step's decoy: magnitude given
    out.append(("one", rnd(6, (1, 1, 1), dtype), "field"))                                            # max_abs of one element
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("grid", GRIDS)
def test_decoy_differs_and_stays_valid(grid, dtype):
    arrays = _arrays(grid, dtype)
    for seed in (0, 1, 7):
        dec = SO.decoy_set(arrays, seed)
        assert SO.check_decoy(arrays, dec) == []
        for n, a, role in arrays:
            d = dec[n]
            assert d.shape == a.shape and d.dtype == a.dtype and not SO.bits_same(d, a), n
            assert d.flags.f_contiguous if a.ndim == 3 else d.flags.c_contiguous, n
            if role == "state":
                assert set(np.unique(d)) <= {0, 1}
            elif role == ("field", 1e-2):
                assert np.isfinite(d).all() and 0 < np.abs(d).max() <= 1e-2
            elif role != "field":
                assert (d >= 0).all() and all((d[q] <= grid[q]).all() for q in range(3))
            else:
                assert np.isfinite(d).all() and np.abs(d).max() <= (np.abs(a).max() or 1.0)
    # the same seed gives the same decoy (the synchronous decoy run and the measured run see one set)
    again = SO.decoy_set(arrays, 7)
    assert all(SO.bits_same(again[n], dec[n]) for n in dec)


def test_decoy_of_a_state_that_equals_the_draw():
    a = np.ones(64, dtype=np.uint8)
    drawn = SO.decoy_array(a, "state", 5)
    again = SO.decoy_array(drawn.copy(), "state", 5)                 # the array IS what the generator draws: one entry is flipped
    assert not np.array_equal(again, drawn) and set(np.unique(again)) <= {0, 1}
    one = np.array([[[0.25]]])
    d = SO.decoy_array(one, "field", 0)
    assert SO.bits_same(SO.decoy_array(d.copy(), "field", 0), d) is False


def test_check_decoy_reports():
    grid = (5, 4, 3)
    arrays = _arrays(grid, np.float64)
    dec = SO.decoy_set(arrays, 0)
    for n, spoil, word in (("c", lambda d: arrays[0][1].copy(order="F"), "coincides"), ("X", lambda d: d + 100.0, "outside the box"),
                           ("state", lambda d: d + 2, "outside {0, 1}"), ("vx", lambda d: d * np.inf, "not finite"),
                           ("vy", lambda d: d * 4.0, "magnitude"), ("s", lambda d: d[1:], "decoy is")):
        bad = dict(dec)
        bad[n] = spoil(dec[n])
        msgs = SO.check_decoy(arrays, bad)
        assert len(msgs) >= 1 and any(word in m and m.startswith(n + ":") for m in msgs), (n, msgs)


def test_op_count_rounds_up():
    assert SO.op_count(20.0, 0.035) == math.ceil(20.0 / 0.035) == 572
    assert SO.op_count(20.0, 20.0) == 1 and SO.op_count(20.0, 19.999) == 2 and SO.op_count(20.0, 10.0) == 2 and SO.op_count(20.0, 9.99) == 3
    assert SO.op_count(1.0, 50.0) == 1                                # never below one op
    assert SO.op_count(1e9, 1.0) == int(SO.DELAY_CAP_MS)              # capped
    for ms, op in ((5.0, 0.0173), (80.0, 0.0411), (200.0, 0.3)):
        n = SO.op_count(ms, op)
        assert n * op >= min(ms, SO.DELAY_CAP_MS) > (n - 1) * op
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SO.op_count(20.0, bad)
    assert 0.0 < SO.DELAY_MS <= SO.DELAY_CAP_MS == 200.0


def test_diagnose():
    want, dec = rnd(1, (6, 5, 4)), rnd(2, (6, 5, 4))
    assert SO.diagnose(want.copy(), want, dec) == "ok"
    assert SO.diagnose(dec.copy(), want, dec) == "equals the decoy run: the inputs were read early"
    mixed = want.copy()
    mixed[:2] = dec[:2]
    msg = SO.diagnose(mixed, want, dec)
    assert msg.startswith("neither") and "(40 of 120 entries" in msg
    assert SO.diagnose(dec.copy(), want, None).startswith("neither")
    nan = want.copy()
    nan[0, 0, 0] = np.nan
    assert SO.diagnose(nan.copy(), nan, dec) == "ok"                  # a NaN equals a NaN
    assert "(1 of 120" in SO.diagnose(want, nan, dec)
    assert SO.diagnose(want.astype(np.float32), want, dec).startswith("is float32")
    s = np.array([0, 1, 1], dtype=np.uint8)
    assert SO.diagnose(s.copy(), s, 1 - s) == "ok" and "read early" in SO.diagnose(1 - s, s, 1 - s)


def test_same_result():
    rec = lambda x: SimpleNamespace(vmax=(1.0, x, 3.0), ke=0.5, n=(1, 2, 3))
    assert SO.same_result(rec(2.0), rec(2.0)) and not SO.same_result(rec(2.0), rec(2.5))
    assert SO.same_result(rec(float("nan")), rec(float("nan")))
    assert SO.same_result((7, [1.0, float("nan")]), (7, [1.0, float("nan")])) and not SO.same_result((7, [1.0]), (7, [1.0, 2.0]))
    assert SO.same_result(None, None) and not SO.same_result(None, 0.0) and not SO.same_result(3, None)


def test_verdict_judges_the_canary_first():
    want = {"out": rnd(1, (4, 3, 3)), "in": rnd(3, (4, 3, 3))}
    dec = {"out": rnd(2, (4, 3, 3)), "in": rnd(4, (4, 3, 3))}
    decoy_run = {"out": rnd(5, (4, 3, 3)), "in": dec["in"]}
    ok = SO.verdict("case", want, want, decoy_run, dec, dec, 1.5, 1.5, 2.5)
    assert ok == []
    # the canary saw the real input: whatever the outputs are, the case proves nothing and says so
    for got in (want, decoy_run):
        msgs = SO.verdict("case", got, want, decoy_run, {"out": dec["out"], "in": want["in"]}, dec)
        assert len(msgs) == 1 and "delay too short: the case proves nothing" in msgs[0] and "in" in msgs[0]
    msgs = SO.verdict("case", decoy_run, want, decoy_run, dec, dec, 2.5, 1.5, 2.5)
    assert len(msgs) == 3 and all("read early" in m for m in msgs), msgs
    msgs = SO.verdict("case", want, want, decoy_run, dec, dec, 9.0, 1.5, 2.5)
    assert len(msgs) == 1 and "returned 9.0, expected 1.5" in msgs[0] and "read early" not in msgs[0]


# ---- the multi-rank half ------------------------------------------------------------------------------------------------------------
def test_late_sets():
    f = frozenset
    assert SO.late_sets(2, "follow") == [f({0, 1})] and SO.late_sets(8, "follow") == [f(range(8))]
    assert SO.late_sets(2, "own") == [f({0, 1}), f({0}), f({1})]
    assert SO.late_sets(3, "own") == [f({0, 1, 2}), f({0}), f({2}), f({1})]                 # P = 3: the middle rank too
    assert SO.late_sets(4, "own") == [f({0, 1}), f({2, 3}), f({0}), f({3})]                 # no queue left for a canary if all four are late
    assert SO.late_sets(1, "own") == [f({0})]
    for P in (2, 3, 4):
        for setup in ("follow", "own"):
            sets = SO.late_sets(P, setup)
            assert set().union(*sets) == set(range(P)) and all(s and s <= set(range(P)) for s in sets)       # every rank is late in some run
    with pytest.raises(ValueError):
        SO.late_sets(2, "masked")


def test_topo_of():
    assert SO.topo_of((3, (13, 9, 7))) == (None, 3, (13, 9, 7))
    assert SO.topo_of(((2, 2, 1), [11, 8, 6])) == ((2, 2, 1), 4, (11, 8, 6))


def _rank_case(P=3, grid=(6, 5, 4)):
    host = [fields(*grid, ["c", "vz"], 100 * (r + 1)) for r in range(P)]
    arrays = [("c", [h[0] for h in host], "field"), ("vz", [h[1] for h in host], "field"),
              ("state", [np.ones(9 + r, dtype=np.uint8) for r in range(P)], "state")]
    return SO.RankCase("case", (P, grid), arrays, lambda hip, mg, t: None)


def test_rank_case_draws_a_decoy_per_rank():
    case = _rank_case()
    assert case.P == 3 and case.dims is None and case.names == ["c", "vz", "state"] and len(case.real) == len(case.decoy) == 3
    for l in range(3):
        assert SO.check_decoy(case.rank_arrays(l), case.decoy[l]) == []
        assert case.decoy[l]["state"].shape == (9 + l,)                                   # a rank's arrays have its own shapes
        for k in range(l):
            assert not SO.bits_same(case.decoy[l]["c"], case.decoy[k]["c"]) and not SO.bits_same(case.decoy[l]["vz"], case.decoy[k]["vz"])
            assert not SO.bits_same(case.decoy[l]["c"], case.real[k]["c"])
    again = _rank_case()
    assert all(SO.bits_same(again.decoy[l][n], case.decoy[l][n]) for l in range(3) for n in case.names)
    with pytest.raises(AssertionError):
        SO.RankCase("short", (3, (6, 5, 4)), [("c", [rnd(1, (6, 5, 4))] * 2, "field")], None)      # two arrays for three ranks


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_case_of_the_multi_rank_table_builds(dt):
    """RankCase construction (check_decoy empty for every rank: asserted by the constructor) for every row of the table"""
    import mgpu_cases as MC
    rows = MC.table(dt)
    assert {f for f, _ in rows} == {"update_halo", "update_halo_twice", "gather", "slab", "pt_solve_slab", "advect_wide", "advect_wide_twice",
                                    "poisson_direct", "diagnostics", "tracers_advance", "chain"}
    for family, spec in rows:
        case = spec.rank_case()
        assert case.P == len(case.real) >= 2 and spec.outputs <= set(case.names), spec.name
        assert all(a.dtype in (MC.NP[dt], np.float64, np.uint8) for l in range(case.P) for a in case.real[l].values()), spec.name
        for l in range(case.P):
            assert SO.check_decoy(case.rank_arrays(l), case.decoy[l]) == [], (spec.name, l)
    assert len({spec.name for _, spec in rows}) == len(rows)
    # the halo mask of update_halo: nothing on the staggers without a halo, the outermost layer of the sides with a neighbour
    spec = [s for f, s in rows if f == "update_halo" and s.topo == (3, (13, 9, 7))][0]
    assert not MC.halo_layers(spec, "s", 1).any() and not MC.halo_layers(spec, "i", 1).any()
    m = MC.halo_layers(spec, "vz", 1)
    assert m.shape == (13, 9, 8) and m[:, :, 0].all() and m[:, :, 7].all() and not m[:, :, 1:7].any()
    assert not MC.halo_layers(spec, "c", 0)[:, :, 0].any() and MC.halo_layers(spec, "c", 0)[:, :, 6].all()
    assert not MC.halo_layers(spec, "c", 2)[:, :, 6].any()
    mig = MC.tracers_migrate_case()
    assert mig.reference[4] > 200 and mig.reference[5] == [0, 0] and mig.arrays[2][1][0].dtype == np.int64


def test_verdict_ranks_names_the_rank():
    case = _rank_case(2)
    want = [{"c": rnd(11 + l, (6, 5, 4))} for l in range(2)]
    dwant = [{"c": rnd(21 + l, (6, 5, 4))} for l in range(2)]
    dec = [{"c": case.decoy[l]["c"]} for l in range(2)]
    good = {l: dec[l] for l in range(2)}
    assert SO.verdict_ranks("case", want, want, dwant, good, dec, {0, 1}, (3, [1.0]), (3, [1.0]), (4, [2.0])) == []
    # rank 1's canary saw the real input: nothing else is judged
    msgs = SO.verdict_ranks("case", dwant, want, dwant, {0: dec[0], 1: {"c": case.real[1]["c"]}}, dec, {0, 1})
    assert len(msgs) == 1 and "case, rank 1: delay too short: the case proves nothing" in msgs[0]
    # only the late ranks have a canary
    assert SO.verdict_ranks("case", want, want, dwant, {1: dec[1]}, dec, {1}) == []
    # rank 0 holds the decoy run's bits, rank 1 a mixture (a neighbour's decoy plane in its halo)
    mixed = want[1]["c"].copy(order="F")
    mixed[:, :, 0] = dwant[1]["c"][:, :, 0]
    msgs = SO.verdict_ranks("case", [dwant[0], {"c": mixed}], want, dwant, good, dec, {0, 1}, (3, [1.0]), (3, [1.0]))
    assert len(msgs) == 2 and msgs[0].startswith("case, rank 0: c equals the decoy run") and msgs[1].startswith("case, rank 1: c neither")
    assert "(30 of 120 entries" in msgs[1]
    msgs = SO.verdict_ranks("case", want, want, dwant, good, dec, {0}, (4, [2.0]), (3, [1.0]), (4, [2.0]))
    assert len(msgs) == 1 and msgs[0].startswith("case: returned") and "read early" in msgs[0]


def test_the_harness_imports_no_gpu_module():
    import ast
    import os
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_order.py")).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {n.module.split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert names <= {"math", "types", "numpy"}, names
