"""tests/arena.py on CPU tensors: the layout it promises and what its checker reports.  The same self-test runs on the device in
tests/test_gpu_footprint.py."""
import numpy as np
import pytest
import torch

import arena as AR
from util import rnd

ESZ = {torch.float64: 8, torch.float32: 4, torch.uint8: 1, torch.int64: 8}


def sample_arrays():
    """a call's worth of arrays: two element types of fields, a (3, n) point list, a byte state, outputs and inputs mixed"""
    rng = np.random.Generator(np.random.MT19937(5))
    return [("Vx", rnd(1, (8, 5, 4)), True), ("Vy", rnd(2, (7, 6, 4)), True), ("Pr", rnd(3, (7, 5, 4)), False),
            ("d", rnd(4, (5, 3, 2)), True), ("rhs", rnd(5, (7, 5, 4)), False),
            ("A32", rnd(6, (6, 4, 3), np.float32), False), ("B32", rnd(7, (6, 4, 3), np.float32), True),
            ("X", rng.uniform(0, 3, (3, 9)), True), ("state", (rng.uniform(size=9) < 0.5).astype(np.uint8), True),
            ("alive", np.ones(5, dtype=np.uint8), False)]


def check_layout(ar, arrays):
    """shared with the device self-test: odd offsets, element alignment and no better, strides, gaps, interleaving, contents"""
    for name, a, is_out in arrays:
        s, t = ar.slots[name], ar.t[name]
        buf = ar.buf[s.dtype]
        assert s.offset % 2 == 1, (name, s.offset)
        assert t.data_ptr() == buf.data_ptr() + s.offset * ESZ[s.dtype]
        if buf.data_ptr() % 512 == 0:
            assert (t.data_ptr() % 512) % (2 * ESZ[s.dtype]) == ESZ[s.dtype], name       # the element's alignment and no better
        assert tuple(t.shape) == a.shape and t.dtype == s.dtype
        if a.ndim == 3:
            assert t.stride() == (1, a.shape[0], a.shape[0] * a.shape[1]), (name, t.stride())
        else:
            assert t.is_contiguous()
        got = ar.get(name)
        assert got.dtype == a.dtype and np.array_equal(got, a), name
        if a.ndim == 3:
            assert got.flags.f_contiguous
    plane_row = max(a.shape[0] * a.shape[1] + a.shape[0] for _, a, _ in arrays if a.ndim == 3)
    for dt, buf in ar.buf.items():
        slots = sorted((s for s in ar.slots.values() if s.dtype == dt), key=lambda s: s.offset)
        assert slots[0].offset >= plane_row and buf.numel() - (slots[-1].offset + slots[-1].numel) >= plane_row
        for a, b in zip(slots, slots[1:]):
            assert b.offset - (a.offset + a.numel) >= plane_row, (a.name, b.name)
        # outputs and inputs alternate for as long as there are both
        kinds = [s.output for s in slots]
        n_in = kinds.count(False)
        assert kinds[:2 * min(n_in, kinds.count(True))] == [True, False] * min(n_in, kinds.count(True)), kinds


def check_reports(ar, arrays):
    """one element written into each side of each guard: the right array, side and distance; the guard mended again, a clean pass"""
    assert ar.check() == []
    ar.assert_clean()
    for name, a, _ in arrays:
        s = ar.slots[name]
        buf = ar.buf[s.dtype]
        row = a.shape[0] if a.ndim == 3 else 0
        # next to the array, a row and an element away, and as far as this array's half of a shared gap reaches
        spots = {-1: "before", -(row + 1): "before", -(ar.gap // 2): "before", 1: "behind", row + 1: "behind", ar.gap // 2 - 1: "behind"}
        for dist, side in spots.items():
            idx = s.offset + dist if dist < 0 else s.offset + s.numel + dist - 1
            keep = buf[idx].clone()
            buf[idx] = 1                                                       # a plain index assignment
            found = ar.check()
            assert len(found) == 1, (name, dist, found)
            f = found[0]
            assert (f.array, f.side, f.first, f.last, f.count) == (name, side, dist, dist, 1), (name, dist, f)
            assert name in AR.describe(f) and side in AR.describe(f) and ("%+d" % dist) in AR.describe(f)
            with pytest.raises(AssertionError, match=name):
                ar.assert_clean("self-test")
            buf[idx] = keep
        assert ar.check() == []
    # a run of dirtied words reports its first and last offset; an in-bounds write is not a finding
    s = ar.slots["Pr"]
    buf = ar.buf[s.dtype]
    end = s.offset + s.numel
    buf[end + 2:end + 9] = 0.5
    (f,) = ar.check()
    assert (f.array, f.side, f.first, f.last, f.count) == ("Pr", "behind", 3, 9, 7)
    assert AR._split(9, f.row, f.plane) == (0, 1, 2) and AR._split(-37, 7, 35) == (-1, 0, -2)
    buf[end + 2:end + 9].view(AR._INT[s.dtype]).fill_(AR.GUARD[s.dtype])
    ar.t["Pr"][0, 0, 0] = 3.0
    ar.t["Pr"][-1, -1, -1] = 4.0
    assert ar.check() == []
    assert ar.get("Pr")[0, 0, 0] == 3.0 and ar.get("Pr")[-1, -1, -1] == 4.0


def test_guard_patterns_are_quiet_nans_with_a_payload():
    a = np.array([AR.GUARD[torch.float64]], dtype=np.uint64).view(np.float64)
    b = np.array([AR.GUARD[torch.float32]], dtype=np.uint32).view(np.float32)
    assert np.isnan(a[0]) and np.isnan(b[0])
    assert AR.GUARD[torch.float64] >> 51 == 0xFFF and AR.GUARD[torch.float64] & 0xFFFFFFFF == 0xDEADBEEF      # quiet bit set
    assert AR.GUARD[torch.float32] >> 22 == 0x1FF and AR.GUARD[torch.float32] & 0xFFFF == 0xBEEF
    assert 0 < AR.GUARD[torch.uint8] < 256


def test_layout_on_cpu_tensors():
    arrays = sample_arrays()
    check_layout(AR.Arena(arrays, "cpu"), arrays)


def test_reports_on_cpu_tensors():
    arrays = sample_arrays()
    check_reports(AR.Arena(arrays, "cpu"), arrays)


def int64_arrays():
    """the tracers' migration: per-rank id arrays (−1 = empty slot) beside positions and states"""
    ids = [np.concatenate([np.arange(7, dtype=np.int64) * 3, np.full(4, -1, dtype=np.int64)]), np.array([5, -1, 2**40], dtype=np.int64)]
    return [("ids@0", ids[0], True), ("ids@1", ids[1], True), ("X@0", np.full((3, 11), 0.5), True), ("state@0", np.ones(11, dtype=np.uint8), True),
            ("Vx", rnd(1, (8, 5, 4)), False)]


def test_int64_slot():
    """an int64 array is a slot like the others: odd element offset, 8-byte alignment and no better, its values back unchanged, a guard
    word that is no NaN business but one fixed integer, compared as an integer; the other element types keep their guards"""
    assert AR.GUARD[torch.int64] == 0x5AA5_0000_DEAD_BEEF and 0 < AR.GUARD[torch.int64] < 2**63
    assert AR.GUARD[torch.float64] == 0x7FF8_0000_DEAD_BEEF and AR.GUARD[torch.float32] == 0x7FC0_BEEF and AR.GUARD[torch.uint8] == 0xA5
    arrays = int64_arrays()
    ar = AR.Arena(arrays, "cpu")
    check_layout(ar, arrays)
    assert ar.t["ids@0"].dtype == torch.int64 and ar.get("ids@1").tolist() == [5, -1, 2**40]
    assert set(ar.buf) == {torch.int64, torch.float64, torch.uint8}                       # a buffer of its own: not mixed with the float64 arrays
    words = ar.buf[torch.int64].numpy()
    s0, s1 = ar.slots["ids@0"], ar.slots["ids@1"]
    assert (words[:s0.offset] == AR.GUARD[torch.int64]).all() and (words[s1.offset + s1.numel:] == AR.GUARD[torch.int64]).all()
    assert ar.check() == []
    # a stray id just behind rank 0's array, a −1 (an "empty slot") just before rank 1's: both found, each against its array
    ar.buf[torch.int64][s0.offset + s0.numel] = 12
    ar.buf[torch.int64][s1.offset - 1] = -1
    found = sorted(ar.check())
    assert [(f.array, f.side, f.first, f.last, f.count) for f in found] == [("ids@0", "behind", 1, 1, 1), ("ids@1", "before", -1, -1, 1)]
    with pytest.raises(AssertionError, match="ids@0"):
        ar.assert_clean("migrate")
    ar.buf[torch.int64][s0.offset + s0.numel] = AR.GUARD[torch.int64]
    ar.buf[torch.int64][s1.offset - 1] = AR.GUARD[torch.int64]
    ar.t["ids@0"][3] = -1                                                                # an in-bounds write is not a finding
    assert ar.check() == [] and ar.get("ids@0")[3] == -1


def test_fresh_arena_is_all_guard_outside_the_arrays():
    arrays = sample_arrays()
    ar = AR.Arena(arrays, "cpu")
    for dt, buf in ar.buf.items():
        mask = np.ones(buf.numel(), dtype=bool)
        for s in ar.slots.values():
            if s.dtype == dt:
                mask[s.offset:s.offset + s.numel] = False
        words = buf.view(AR._INT[dt]).numpy()
        assert (words[mask] == AR.GUARD[dt]).all() and mask.sum() > 0
