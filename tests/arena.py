"""A guarded arena: the arrays of one library call carved out of one flat buffer per element type, with guard gaps around them.

What it is for.  include/ns3d.h promises that device arrays need only the alignment of their element type and that a call touches
nothing outside the arrays it was given.  Tensors that PyTorch allocates one by one cannot test either: every base pointer is
512-byte aligned and every array is followed by allocator slack, where a stray store lands unnoticed.  Here

  - every array of a call is a view into a larger buffer: column-major (nx,ny,nz) arrays as buf[o:o+n].view(nz,ny,nx).permute(2,1,0)
    (the form kernels._chk accepts), arrays of any other rank (the tracers' X / state, tri / val, the eleven blocks of S) as
    contiguous views;
  - there is a guard gap before the first array, between neighbours and after the last; outputs are interleaved with inputs, so an
    overrun of an output meets a guard first and then, at the earliest, an input;
  - every gap is at least one plane plus one row of the largest array of the call, then widened until the next array starts at an
    ODD element offset from the 512-byte-aligned start of the buffer: float64 arrays are 8-byte aligned, float32 arrays 4-byte
    aligned, uint8 arrays sit on an odd byte, and none of them any better;
  - guards hold a quiet NaN with a fixed payload (GUARD: one bit pattern per element width, one fixed byte for uint8, one large
    positive word for int64 — the tracers' id arrays hold −1 and particle numbers, never that) and are compared as integers after
    the call.  The NaN is a second check: an out-of-bounds LOAD whose value reaches an output through arithmetic (x·0, a late
    select) poisons that output, which the caller's bit comparison of the outputs then catches.

check() names the array, the side and the first and last dirtied offsets as signed distances from the array (−1 = the element just
before its first, +1 = the element just behind its last), in elements and in planes / rows / elements of that array, so that a failure
points at a tile-edge predicate.  A gap between two arrays is split in the middle: its first half is reported against the array
before it, its second half against the array behind it.

What the harness cannot see: a stray load whose value is discarded (masked before any arithmetic, or read into a lane that never
stores), and a stray access that lands inside ANOTHER array of the same call without changing a compared value.  Arrays are
deliberately not placed at the end of an allocation to turn stray loads into faults.

Works on CPU tensors as well (tests/test_arena_host.py)."""
from collections import namedtuple

import numpy as np
import torch

GUARD = {torch.float64: 0x7FF8_0000_DEAD_BEEF, torch.float32: 0x7FC0_BEEF, torch.uint8: 0xA5, torch.int64: 0x5AA5_0000_DEAD_BEEF}
_INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}
_NPINT = {torch.float64: np.int64, torch.float32: np.int32, torch.uint8: np.uint8, torch.int64: np.int64}
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8,
          np.dtype(np.int64): torch.int64}
MIN_GAP = 64                                    # elements; what a call without a column-major array gets (never the case in the suite)

Slot = namedtuple("Slot", "name dtype offset numel shape colmajor output")
Finding = namedtuple("Finding", "array side first last count row plane")


def _split(dist, row, plane):
    """a signed element distance as (planes, rows, elements) of the array it is measured from, each with the sign of `dist`"""
    s, d = (1 if dist >= 0 else -1), abs(dist)
    p, d = divmod(d, plane) if plane else (0, d)
    r, e = divmod(d, row) if row else (0, d)
    return s * p, s * r, s * e


def describe(f):
    return ("%s: %d guard word(s) %s the array dirtied, offsets %+d … %+d elements = (planes, rows, elements) %r … %r"
            % (f.array, f.count, f.side, f.first, f.last, _split(f.first, f.row, f.plane), _split(f.last, f.row, f.plane)))


class Arena:
    """arrays: a sequence of (name, host array, is_output).  A 3-D host array becomes a column-major device view of the same shape
    (give it in any memory order); arrays of any other rank become contiguous views.  self.t[name] are the views to pass to the
    library; the initial contents are the host arrays'."""

    def __init__(self, arrays, device="cuda"):
        self.device = torch.device(device)
        arrays = [(n, np.asarray(a), bool(o)) for n, a, o in arrays]
        assert len({n for n, _, _ in arrays}) == len(arrays), "duplicate array names"
        gap = max([a.shape[0] * a.shape[1] + a.shape[0] for _, a, _ in arrays if a.ndim == 3] + [MIN_GAP])
        self.gap = gap
        self.slots, self.buf, self.t = {}, {}, {}
        for dt in sorted({_TORCH[a.dtype] for _, a, _ in arrays}, key=str):
            mine = [x for x in arrays if _TORCH[x[1].dtype] == dt]
            outs, ins = [x for x in mine if x[2]], [x for x in mine if not x[2]]
            order = []
            for q in range(max(len(outs), len(ins))):                       # out, in, out, in, …
                order += outs[q:q + 1] + ins[q:q + 1]
            o = 0
            for name, a, is_out in order:
                o += gap
                o += 1 - (o & 1)                                            # widen the gap: an odd element offset
                self.slots[name] = Slot(name, dt, o, a.size, tuple(a.shape), a.ndim == 3, is_out)
                o += a.size
            total = o + gap + 1
            buf = torch.empty(total, dtype=dt, device=self.device)
            assert buf.data_ptr() % 512 == 0 or self.device.type == "cpu", "the allocator's base pointer is not 512-byte aligned"
            buf.view(_INT[dt]).fill_(GUARD[dt])
            self.buf[dt] = buf
            for name, a, _ in order:
                s = self.slots[name]
                flat = buf[s.offset:s.offset + s.numel]
                if s.colmajor:
                    sx, sy, sz = s.shape
                    self.t[name] = flat.view(sz, sy, sx).permute(2, 1, 0)
                    src = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0)))
                    self.t[name].permute(2, 1, 0).copy_(src.to(self.device))
                else:
                    self.t[name] = flat.view(s.shape)
                    self.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.device))

    def __getitem__(self, name):
        return self.t[name]

    def get(self, name):
        """the array as it is now, on the host: Fortran-ordered for column-major arrays, C-ordered otherwise"""
        s = self.slots[name]
        flat = self.buf[s.dtype][s.offset:s.offset + s.numel].cpu().numpy().copy()
        if s.colmajor:
            sx, sy, sz = s.shape
            return np.asfortranarray(flat.reshape(sz, sy, sx).transpose(2, 1, 0))
        return flat.reshape(s.shape)

    def check(self):
        """Findings, one per dirtied (array, side); empty when every guard word still holds GUARD."""
        out = []
        for dt, buf in self.buf.items():
            host = buf.view(_INT[dt]).cpu().numpy().view(_NPINT[dt])
            want = _NPINT[dt](GUARD[dt])                                    # every guard pattern is positive as a signed integer
            slots = sorted((s for s in self.slots.values() if s.dtype == dt), key=lambda s: s.offset)
            for q, s in enumerate(slots):
                row, plane = (s.shape[0], s.shape[0] * s.shape[1]) if s.colmajor else (0, 0)
                end = s.offset + s.numel
                prev_end = slots[q - 1].offset + slots[q - 1].numel if q else 0
                next_start = slots[q + 1].offset if q + 1 < len(slots) else host.size
                lo = prev_end if q == 0 else prev_end + (s.offset - prev_end) // 2           # the second half of the gap before
                hi = next_start if q + 1 == len(slots) else end + (next_start - end) // 2    # the first half of the gap behind
                bad = np.flatnonzero(host[lo:s.offset] != want)
                if bad.size:
                    out.append(Finding(s.name, "before", int(bad[0]) + lo - s.offset, int(bad[-1]) + lo - s.offset, int(bad.size), row, plane))
                bad = np.flatnonzero(host[end:hi] != want)
                if bad.size:
                    out.append(Finding(s.name, "behind", int(bad[0]) + 1, int(bad[-1]) + 1, int(bad.size), row, plane))
        return out

    def assert_clean(self, what=""):
        found = self.check()
        assert not found, "%s stored outside its arrays:\n  %s" % (what or "the call", "\n  ".join(describe(f) for f in found))
