"""CPU tests of the obstacle step's statement: oracle/driver_ref.py with obstacle= and initial= (tests/solid_step_cases.py).

The defaults change nothing; the cylinder's own mask through obstacle= returns the drivers' bits; and the shared scenario is admissible
— every field stays finite, every masking call and every bit of the mask changes the result — so that the device comparisons in
tests/test_gpu_solid_step.py, the footprint and the stream-order harness cannot pass with a masking left out or a bit ignored."""
import numpy as np
import pytest

import solid_ref as SR
import solid_step_cases as SS
from util import bits_equal

DTS = ["f64", "f32"]


def _same(a, b, names=SS.ELEVEN):
    (fa, ia), (fb, ib) = a, b
    return all(bits_equal(fa[n], fb[n]) for n in names) and ia.iters == ib.iters and \
        all(np.array_equal(np.float64(x), np.float64(y), equal_nan=True) for x, y in zip(ia.errs, ib.errs)) and len(ia.errs) == len(ib.errs)


# ---- the keywords --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advection", SS.SCHEMES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_the_cylinders_own_mask_returns_the_drivers_bits(oracle, script, dt, advection):
    """obstacle = the cylinder's mask (set_cylinder on C = 0, V = 1, read off — solid.mask_of_cylinder's method on the CPU) equals the
    driver without the keyword: all eleven arrays, iteration counts, err histories; nx = 24, nt = 2, faithful=False, the script's own
    initial state and iteration limit.  A NaN equals a NaN: in float32 both scripts leave the finite range at this size."""
    mask = SS.cylinder_mask(script, dt)
    assert all(((mask >> b) & 1).any() for b in range(4)) and not (mask & 0xF0).any()
    plain = SS.run_ref(script, SS.DTYPES[dt], advection=advection)
    masked = SS.run_ref(script, SS.DTYPES[dt], advection=advection, obstacle=mask)
    assert _same(plain, masked), (script, dt, advection)
    assert "removed" not in plain[1] and len(masked[1].removed) == 2 and all(len(r) == 2 for r in masked[1].removed)


@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_initial_replaces_the_scripts_fields_and_the_defaults_change_nothing(oracle, script):
    f0, i0 = SS.run_ref(script, np.float64, nt=1)
    f1, i1 = SS.run_ref(script, np.float64, nt=1, initial={})
    assert _same((f0, i0), (f1, i1))
    sc = SS.scenario(script, "f64")
    own = SS.run_ref(script, np.float64, nt=0)[0]
    f2, _ = SS.run_ref(script, np.float64, nt=0, initial={"Vz": sc.initial["Vz"]})
    want = sc.initial["Vz"].copy()
    if script == "multi":                   # multi.jl:372 masks behind the copy
        SR.set_solid(None, np.ones_like(own["Vx"]), np.ones_like(own["Vy"]), want, SS.cylinder_mask(script, "f64"))
        assert not bits_equal(want, sc.initial["Vz"])
    assert bits_equal(f2["Vz"], want) and all(bits_equal(f2[n], own[n]) for n in ("C", "Pr", "Vx", "Vy"))


def test_what_the_ref_drivers_refuse():
    from oracle.driver_ref import run_navierstokes3D_ref, runme_ref
    m = SS.body_mask()
    with pytest.raises(ValueError, match="one rank"):
        run_navierstokes3D_ref(nx=24, nt=1, dims_z=2, obstacle=m)
    with pytest.raises(ValueError, match="uint8 mask of shape"):
        runme_ref(nx=24, nt=1, obstacle=m[:-1])
    with pytest.raises(ValueError, match="uint8 mask of shape"):
        run_navierstokes3D_ref(nx=24, nt=1, obstacle=m.astype(np.int32))
    with pytest.raises(ValueError, match="none of C, Pr"):
        runme_ref(nx=24, nt=1, initial={"divV": np.zeros(SS.GRID)})
    with pytest.raises(ValueError, match="shape"):
        runme_ref(nx=24, nt=1, initial={"Vx": np.zeros(SS.GRID)})


# ---- the scenario ----------------------------------------------------------------------------------------------------------------------
def test_the_body_meets_the_outer_planes():
    m = SS.body_mask()
    nx, ny, nz = SS.GRID
    assert tuple(int(((m >> b) & 1).sum()) for b in range(4)) == SS.BIT_COUNTS
    assert m[0].any() and m[nx].any() and m[:, ny].any() and m[:, :, 0].any() and m[:, :, nz].any()
    assert (m[nx] & ~np.uint8(2) == 0).all() and (m[:, ny] & ~np.uint8(4) == 0).all() and (m[:, :, nz] & ~np.uint8(8) == 0).all()
    for dt in DTS:
        init = SS.initial_state(dt)
        assert all((init[n] != 0).all() and np.abs(init[n]).max() <= 1e-2 for n in ("Pr", "Vx", "Vy", "Vz"))
        assert init["C"].min() > 0 and init["C"].max() < 1


@pytest.mark.parametrize("advection", SS.SCHEMES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_every_field_stays_finite(oracle, script, dt, advection):
    f, info = SS.scenario_ref(script, dt, advection)
    assert all(f[n].dtype == SS.DTYPES[dt] and np.isfinite(f[n]).all() for n in SS.ELEVEN), (script, dt, advection)
    assert all(np.abs(f[n]).max() > 0 for n in SS.ELEVEN)
    sc = SS.scenario(script, dt)
    assert info.iters == [sc.niter] * sc.nt and all(len(e) == 3 and np.isfinite(e).all() for e in info.errs)
    assert len(info.removed) == sc.nt
    for step in info.removed:
        for sums, counts, mags in step:     # every velocity bit of every masking removes something
            assert tuple(counts) == SS.BIT_COUNTS[1:] and all(m > 0 for m in mags)
    assert not _same((f, info), SS.scenario_ref(script, dt, advection, mask=None), SS.FIVE)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_leaving_out_any_one_masking_call_changes_a_field(oracle, monkeypatch, script, dt):
    """multi.jl masks five times in two steps (:372, then :452 and :473 per step), gpu.jl four times (:123, :139)"""
    sc = SS.scenario(script, dt)
    want, _ = SS.scenario_ref(script, dt)
    calls = 5 if script == "multi" else 4
    real = SR.set_solid
    for skip in range(calls + 1):           # skip == calls: none left out — the count, and the same bits
        seen = []

        def set_solid(*a):
            seen.append(len(seen))
            if seen[-1] != skip:
                real(*a)
        monkeypatch.setattr(SR, "set_solid", set_solid)
        f, _ = SS.run_ref(script, sc.dtype, sc.nt, "reference", sc.mask, sc.initial, sc.niter)
        monkeypatch.setattr(SR, "set_solid", real)
        assert len(seen) == calls
        changed = [n for n in SS.FIVE if not bits_equal(f[n], want[n])]
        assert bool(changed) == (skip < calls), (script, dt, skip, changed)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("script", SS.SCRIPTS)
def test_every_bit_of_the_mask_acts(oracle, script, dt):
    """clearing bit 1 changes C; clearing any one of the bits 2, 4, 8 changes a velocity field and Pr"""
    sc = SS.scenario(script, dt)
    want, _ = SS.scenario_ref(script, dt)
    for bit in (1, 2, 4, 8):
        f, _ = SS.run_ref(script, sc.dtype, sc.nt, "reference", sc.mask & np.uint8(0xFF ^ bit), sc.initial, sc.niter)
        if bit == 1:
            assert not bits_equal(f["C"], want["C"]), (script, dt)
        else:
            assert any(not bits_equal(f[n], want[n]) for n in ("Vx", "Vy", "Vz")) and not bits_equal(f["Pr"], want["Pr"]), (script, dt, bit)
