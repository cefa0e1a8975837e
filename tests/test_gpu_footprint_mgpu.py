"""Footprint of the multi-GPU half of the C ABI (navierstokes3d_amd.mgpu → csrc/ns3d_mgpu.cpp): every call of tests/mgpu_cases.py,
and tracers_migrate, with ALL ranks' arrays carved out of one guarded arena (tests/arena.py) — named `name@rank`, outputs interleaved
with inputs, the ranks of one array next to each other, every array at an odd element offset.  The pack / unpack kernels, the
strided sub-box copies, the plane copies and the peer copies write into the caller's arrays at strided offsets: a face one row too
long, a plane copied into the neighbour rank's array or a vector access that assumes more than element alignment meets a guard word
or changes a compared bit.

Per case and stream set-up (own_streams both ways):
  - no guard word is dirtied;
  - every array of every rank, halo included, has the bits the same call leaves in ordinary allocations;
  - arrays the call only reads keep their bits;
  - a halo update writes nothing but halo layers: arrays without a halo (the `s` and `i` staggers) and every layer that is no
    halo — the physical ends included — keep every bit.
What this cannot see: the library's own buffers (hbuf, wbuf, bbuf, gbuf, the slab state) are outside the arena."""
import numpy as np
import pytest
import torch

import mgpu_cases as MC
import stream_order as SO
from arena import Arena

pytestmark = pytest.mark.gpu


def at(name, l):
    return "%s@%d" % (name, l)


def arena_of(spec):
    P = SO.topo_of(spec.topo)[1]
    return Arena([(at(n, l), per_rank[l], n in spec.outputs) for n, per_rank, _ in spec.arrays for l in range(P)])


def run_in_arena(hip, spec, own):
    """(result, arena after the call, result and arrays of the same call in ordinary allocations) on one MultiGpu"""
    case = SimpleCase(spec)
    mg, _, _ = SO.grid_on(hip, case, "own" if own else "follow")
    want_r, want = SO.sync_run_ranks(hip, case, mg, case.real)
    ar = arena_of(spec)
    torch.cuda.synchronize()
    r = spec.call(hip, mg, {n: [ar[at(n, l)] for l in range(case.P)] for n in case.names})
    mg.sync()
    torch.cuda.synchronize()
    mg.close()
    return r, ar, want_r, want


class SimpleCase:
    """what stream_order's grid_on / sync_run_ranks need of a case, without decoys (tracers_migrate has none)"""

    def __init__(self, spec):
        self.name, self.call, self.setup = spec.name, spec.call, spec.setup
        self.dims, self.P, self.n = SO.topo_of(spec.topo)
        self.names = [n for n, _, _ in spec.arrays]
        self.real = [{n: np.asarray(per_rank[l]) for n, per_rank, _ in spec.arrays} for l in range(self.P)]


def check(hip, spec, own):
    r, ar, want_r, want = run_in_arena(hip, spec, own)
    what = "%s, own_streams=%s" % (spec.name, own)
    ar.assert_clean(what)
    P = len(want)
    assert SO.same_result(r, want_r), (what, r, want_r)
    for n, per_rank, _ in spec.arrays:
        for l in range(P):
            got = ar.get(at(n, l))
            assert SO.bits_same(got, want[l][n]), (what, at(n, l), SO.diagnose(got, want[l][n], None))
            if n not in spec.outputs:
                assert SO.bits_same(got, np.asarray(per_rank[l])), (what, at(n, l), "a read-only array changed")
            elif spec.halo_only:
                keep = ~MC.halo_layers(spec, n, l)
                assert SO.bits_same(got[keep], np.asarray(per_rank[l])[keep]), (what, at(n, l), "written outside the halo layers")
    return ar, want


def _rows():
    return [pytest.param(spec, id=spec.name.replace(" ", "_").replace("/", "_")) for dt in MC.DTS for _, spec in MC.table(dt)]


@pytest.mark.parametrize("own", [False, True], ids=["torch-stream", "own-streams"])
@pytest.mark.parametrize("spec", _rows())
def test_multi_rank_call_in_an_arena(hip, spec, own):
    ar, want = check(hip, spec, own)
    if spec.halo_only:                   # the halos did arrive: the call was not a no-op that trivially keeps every bit
        n0 = [n for n, _, _ in spec.arrays][0]
        assert any(not SO.bits_same(want[l][n0], np.asarray(spec.arrays[0][1][l])) for l in range(len(want))), spec.name


@pytest.mark.parametrize("own", [False, True], ids=["torch-stream", "own-streams"])
def test_tracers_migrate_in_an_arena(hip, own):
    """X, state, U and the int64 ids of both ranks in one arena: the slot layout of the NumPy rule, slot for slot, and no guard word
    of any of the four element types dirtied"""
    spec = MC.tracers_migrate_case()
    ar, want = check(hip, spec, own)
    Xs, ss, ids, Us, moved, need = spec.reference
    assert moved > 200 and need == [0, 0]
    for l in range(2):
        for n, ref in (("X", Xs), ("state", ss), ("ids", ids), ("U", Us)):
            assert SO.bits_same(ar.get(at(n, l)), ref[l]), (n, l)
    assert ar.get("ids@0").dtype == np.int64 and torch.int64 in ar.buf
