"""What csrc/ns3d_api.cpp decides before a kernel runs — which argument error wins, its status and its words — against the records
of tests/golden/api_errors.json (tests/api_error_cases.py: the cases, and how the records were written).  The numerical suite
pins what the kernels compute; this pins the boundary in front of them."""
import json

import pytest

import api_error_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(K.GOLDEN, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(hip):
    return K.record()


def test_the_golden_file_holds_exactly_the_cases(golden):
    for suffix in ("f64", "f32"):
        assert sorted(golden[suffix]) == sorted(label for label, _fn, _mods, only in K.cases() if suffix in only)
    assert len(golden["f64"]) == len(golden["f32"]) + 1 > 300        # nlev = 5 is an error with float64 fields only


def test_every_rejecting_case_is_an_argument_error(golden):
    """the records themselves: a defective argument is NS3D_ERR_ARG with a message that names the entry point's family, and the
    only status-0 records are the cases written as legal calls"""
    for suffix in ("f64", "f32"):
        for label, (rc, msg) in golden[suffix].items():
            if label.endswith(K.LEGAL):
                assert (rc, msg) == (0, ""), label
            else:
                assert rc == 1 and msg, label


@pytest.mark.parametrize("suffix", ["f64", "f32"])
def test_status_and_message_of_every_case(got, golden, suffix):
    diff = {label: (got[suffix].get(label), want) for label, want in golden[suffix].items() if got[suffix].get(label) != want}
    assert not diff, "\n".join("%s: got %r, recorded %r" % (k, g, w) for k, (g, w) in sorted(diff.items()))
    assert len(got[suffix]) == len(golden[suffix])
