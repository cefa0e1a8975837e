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


def test_the_harness_imports_no_gpu_module():
    import ast
    import os
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_order.py")).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {n.module.split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert names <= {"math", "types", "numpy"}, names
