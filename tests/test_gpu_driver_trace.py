"""The library calls the two drivers make, by name and in order, against the traces of tests/golden/driver_call_trace.json
(tests/driver_trace.py: the cases, and how the traces were written).  The numerical suite pins what the calls compute; this pins
which calls are made — one more ns3d_sync or a doubled observer call changes no result and would pass everywhere else."""
import json

import pytest

import driver_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(T.GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(T.CASES)
    for case, trace in golden.items():
        assert trace and all(name.startswith("ns3d_") and n >= 1 for name, n in trace), case


@pytest.mark.parametrize("case", sorted(T.CASES))
def test_the_drivers_make_the_recorded_calls(hip, golden, tmp_path, case):
    dirs = [tmp_path / "first", tmp_path / "second"]
    for d in dirs:
        d.mkdir()
    got = T.record(case, str(dirs[0]))[0]
    diff = T.first_difference(got, golden[case])
    assert diff is None, "%s differs from the recorded trace at %s" % (case, diff)
    # the same case again in this process: the trace is no accident of which stream the first run found current
    again = T.record(case, str(dirs[1]))[0]
    diff = T.first_difference(again, got)
    assert diff is None, "%s, run a second time, differs from its first run at %s" % (case, diff)
