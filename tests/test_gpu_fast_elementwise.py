"""FAST mode, element by element.  FAST is a compilation of its own (-ffp-contract=fast, reciprocal spacings) that the older
tests hold to global relative-L2 norms; here every element of every output is held to the running-error bound of
tests/running_error.py, derived from the expression and from nothing the kernels produce: float32 within e of the pair value,
float64 within 2e of the oracle, bit for bit where the bound is 0.  Each test prints the worst err/bound; a failure names the
first offending index, the value, the reference and the bound.  tests/test_running_error_host.py proves the bound sound and
shows the C oracle inside it on the same cases, on the CPU."""
import numpy as np
import pytest

import pair_cases as PC
import running_error as RE
from util import bits_equal

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
STRICT_GRID = (70, 6, 7)            # the one grid per kernel on which STRICT goes through the same comparison


def _once(hip, name, grid, dtype, mode, values="seeded"):
    import torch
    host, scal, outs, ref, prs = PC.once_per_step(name, grid, dtype, values)
    ctx = hip.Context(0, mode)
    if name == "predict_fused":
        src = [hip.from_numpy(a) for a in host[:3]]
        dev = [hip.from_numpy(np.full_like(a, 777.0)) for a in host[:3]]
        hip.predict_fused(*dev, *src, *scal, ctx=ctx)
    else:
        dev = [hip.from_numpy(a) for a in host]
        getattr(hip, name)(*dev, *scal, ctx=ctx)
    torch.cuda.synchronize()
    worst = 0.0
    for q in outs:
        got = hip.to_numpy(dev[q])
        assert got.dtype == dtype
        worst = max(worst, RE.check(got, ref[q], prs[q], dtype, "%s %s %s %r output %d" % (mode.upper(), name, np.dtype(dtype).name, grid, q)))
    print("%s %s %s %r %s: worst err/bound %.3g" % (mode.upper(), name, np.dtype(dtype).name, grid, values, worst))
    if name == "predict_fused":
        for d, a in zip(src, host[:3]):
            assert bits_equal(hip.to_numpy(d), a)
    else:
        for q in range(len(host)):
            if q not in outs:
                assert bits_equal(hip.to_numpy(dev[q]), host[q])
    ctx.close()
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,grid", PC.all_once_per_step(), ids=lambda v: str(v).replace(" ", ""))
def test_fast_once_per_step_within_the_running_error_bound(hip, name, grid, dtype):
    _once(hip, name, grid, dtype, "fast")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(PC.KERNELS) + ["predict_fused"])
def test_strict_once_per_step_within_the_same_bound(hip, name, dtype):
    """STRICT through the same helper: it costs nothing and shows that the comparison runs"""
    _once(hip, name, STRICT_GRID, dtype, "strict")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(PC.KERNELS) + ["predict_fused"])
def test_fast_flow_at_rest_is_exact_where_the_bound_is_zero(hip, name, dtype):
    """hostile(…, 'uniform') velocities, hostile(…, 'rest0') everything else: the differences vanish exactly, the bound is 0 wherever no
    constant enters, and there FAST must return the oracle's bits (signed zeros included)"""
    host, scal, outs, ref, prs = PC.once_per_step(name, (24, 15, 15), dtype, "rest")
    assert sum(int((prs[q].e == 0).sum()) for q in outs) > 0
    _once(hip, name, (24, 15, 15), dtype, "fast", "rest")


# ---- pseudo-transient sweeps ---------------------------------------------------------------------------------------------------
def _pt_setup(hip, grid, dtype, bc, nlev, mode):
    from test_gpu_pt import _params
    from util import geometry
    Pr0, d0, rhs, levels = PC.pt_levels(grid, dtype, bc, nlev)
    ctx = hip.Context(0, mode)
    p = _params(hip, hip.from_numpy(Pr0), geometry(*grid), *bc)
    return Pr0, d0, rhs, levels, ctx, p


def _pt_check(got_P, got_d, level, dtype, what):
    Pr, d, pP, pd = level
    return max(RE.check(got_P, Pr, pP, dtype, what + " Pr"), RE.check(got_d, d, pd, dtype, what + " dPrdtau"))


def _sweep_and_iterate(hip, grid, bc, dtype, mode):
    import torch
    nx, ny, nz = grid
    Pr0, d0, rhs, levels, ctx, p = _pt_setup(hip, grid, dtype, bc, 7, mode)
    dP, dout, dd, drhs = hip.from_numpy(Pr0), hip.from_numpy(np.full_like(Pr0, 555.0)), hip.from_numpy(d0), hip.from_numpy(rhs)
    hip.pt_sweep(dP, dout, dd, drhs, p, 1, nz - 1, ctx=ctx)
    torch.cuda.synchronize()
    w1 = _pt_check(hip.to_numpy(dout), hip.to_numpy(dd), levels[0], dtype, "%s pt_sweep %r" % (mode, grid))
    assert bits_equal(hip.to_numpy(dP), Pr0)
    dP, dd = hip.from_numpy(Pr0), hip.from_numpy(d0)
    hip.pt_iterate(dP, dd, drhs, p, 7, ctx=ctx)
    torch.cuda.synchronize()
    w7 = _pt_check(hip.to_numpy(dP), hip.to_numpy(dd), levels[6], dtype, "%s pt_iterate(7) %r" % (mode, grid))
    assert bits_equal(hip.to_numpy(drhs), rhs)
    print("%s %s %r bc %r: pt_sweep worst err/bound %.3g, pt_iterate(7) %.3g" % (mode.upper(), np.dtype(dtype).name, grid, bc, w1, w7))
    ctx.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", PC.PT_BCS, ids=lambda b: "bc%d%s" % (b[0], "o" if b[1] else ""))
@pytest.mark.parametrize("grid", PC.PT_GRIDS)
def test_fast_pt_sweep_and_iterate(hip, grid, bc, dtype):
    """pt_sweep (one iteration) and pt_iterate(n=7) as the planner schedules them, FAST"""
    _sweep_and_iterate(hip, grid, bc, dtype, "fast")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strict_pt_sweep_and_iterate_within_the_same_bound(hip, dtype):
    _sweep_and_iterate(hip, PC.PT_GRIDS[0], PC.PT_BCS[0], dtype, "strict")


def _shapes(nlev, dtype):
    from test_gpu_pt import SHAPES2, SHAPESN
    if nlev == 2:
        return [("pt_sweep2", s) for s in SHAPES2] + [("pt_sweepn", s) for s in SHAPESN]
    if nlev == 5:
        return [("pt_sweepn", s) for s in (0, 2400, 2405, 2491)]
    return [("pt_sweepn", s) for s in SHAPESN]


@pytest.mark.parametrize("nlev,dtype", [(2, np.float32), (3, np.float32), (4, np.float32), (5, np.float32),
                                        (2, np.float64), (3, np.float64), (4, np.float64)],
                         ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
@pytest.mark.parametrize("bc", PC.PT_BCS, ids=lambda b: "bc%d%s" % (b[0], "o" if b[1] else ""))
@pytest.mark.parametrize("grid", PC.PT_GRIDS)
def test_fast_pt_sweep2_and_sweepn_every_tile_shape(hip, grid, bc, nlev, dtype):
    """pt_sweep2 and pt_sweepn (2…4 levels; 5 in float32) in FAST, every tile shape that test_gpu_pt.py iterates over, against the
    pairs of level nlev; the inputs untouched, nothing of the pre-filled outputs left."""
    import torch
    from navierstokes3d_amd import lib as L
    Pr0, d0, rhs, levels, ctx, p = _pt_setup(hip, grid, dtype, bc, nlev, "fast")
    drhs = hip.from_numpy(rhs)
    ran, worst = 0, 0.0
    for fn, shape in _shapes(nlev, dtype):
        dP, dout, dd = hip.from_numpy(Pr0), hip.from_numpy(np.full_like(Pr0, 555.0)), hip.from_numpy(d0)
        ddout = hip.from_numpy(np.full_like(d0, 444.0))
        try:
            if fn == "pt_sweep2":
                ctx.set_pt2_variant(shape)
                hip.pt_sweep2(dP, dout, dd, ddout, drhs, p, ctx=ctx)
            else:
                ctx.set_ptn_variant(shape)
                hip.pt_sweepn(nlev, dP, dout, dd, ddout, drhs, p, None, None, ctx=ctx)
        except L.Ns3dError as e:                                  # a tile too small for this many levels, a float32-only shape
            assert "cannot run" in str(e), e
            continue
        torch.cuda.synchronize()
        ran += 1
        worst = max(worst, _pt_check(hip.to_numpy(dout), hip.to_numpy(ddout), levels[nlev - 1], dtype,
                                     "FAST %s shape %d levels %d %r" % (fn, shape, nlev, grid)))
        assert bits_equal(hip.to_numpy(dP), Pr0) and bits_equal(hip.to_numpy(dd), d0)
    assert ran >= (4 if nlev == 5 else 8)
    print("FAST %s %r bc %r levels %d: %d shapes, worst err/bound %.3g" % (np.dtype(dtype).name, grid, bc, nlev, ran, worst))
    ctx.close()


def test_strict_pt_sweepn_within_the_same_bound(hip):
    """STRICT through the same comparison on one case per entry point"""
    import torch
    grid, bc = PC.PT_GRIDS[0], PC.PT_BCS[0]
    for dtype in DTYPES:
        Pr0, d0, rhs, levels, ctx, p = _pt_setup(hip, grid, dtype, bc, 4, "strict")
        for nlev in (2, 3, 4):
            dP, dout, dd = hip.from_numpy(Pr0), hip.from_numpy(np.full_like(Pr0, 555.0)), hip.from_numpy(d0)
            ddout = hip.from_numpy(np.full_like(d0, 444.0))
            if nlev == 2:
                hip.pt_sweep2(dP, dout, dd, ddout, hip.from_numpy(rhs), p, ctx=ctx)
            else:
                hip.pt_sweepn(nlev, dP, dout, dd, ddout, hip.from_numpy(rhs), p, None, None, ctx=ctx)
            torch.cuda.synchronize()
            w = _pt_check(hip.to_numpy(dout), hip.to_numpy(ddout), levels[nlev - 1], dtype, "STRICT levels %d" % nlev)
            print("STRICT %s levels %d: worst err/bound %.3g" % (np.dtype(dtype).name, nlev, w))
        ctx.close()
