"""The limited MacCormack advection on the CPU (tests/advect_mc_ref.py, the NumPy statement of include/ns3d.h's definition): what the
scheme must do whatever runs it — a flow at rest and a uniform field are kept, the order of accuracy is two where the reference's
back-track has one, nothing leaves the range of the data — and that the seeded inputs of the GPU tests exercise the limiter."""
import numpy as np
import pytest

import advect_mc_ref as MC
from util import bits_equal, fields, geometry

GRIDS = [(3, 3, 3), (17, 9, 5), (70, 6, 7), (64, 8, 33), (131, 19, 38), (150, 21, 70)]       # test_gpu_advect_mc.GRIDS
CFLS = [0.3, 1.0, 2.7]
KINDS = ["vx", "vy", "vz", "c"]


def seeded(grid, cfl, dtype):
    """old fields [Vx, Vy, Vz, C], dt = cfl × the smallest spacing, geometry — the seeded case of the GPU tests"""
    g = geometry(*grid)
    return fields(*grid, KINDS, 41, dtype), cfl * min(g["dx"], g["dy"], g["dz"]), g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_flow_at_rest_keeps_its_bits(dtype):
    """Velocities +0.0, a seeded C, Â = A_o: every δ is 0, every lerp returns its first operand, the correction adds +0.0 and the
    limiter's hull is the node's own value.  (A −0.0 would come back as +0.0: −0.0 + h·(+0.0) — the definition's own arithmetic.)"""
    nx, ny, nz = 9, 7, 5
    g = geometry(nx, ny, nz)
    old = [np.zeros(a.shape, dtype=dtype, order="F") for a in fields(nx, ny, nz, KINDS[:3], 1, dtype)] + fields(nx, ny, nz, ["c"], 4, dtype)
    new = MC.correct(old, [a.copy(order="F") for a in old], 0.02, g["dx"], g["dy"], g["dz"])
    assert all(bits_equal(a, b) for a, b in zip(new, old))
    new, hat = MC.advect_mc(old, 0.02, g["dx"], g["dy"], g["dz"])
    assert all(bits_equal(a, b) for a, b in zip(new, old)) and all(bits_equal(a, b) for a, b in zip(hat, old))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_uniform_field_is_preserved(dtype):
    """C = 0.7 everywhere in a seeded flow: stage 1's lerps of equal values may be an ulp off, the limiter's hull [0.7, 0.7] is not"""
    old, dt, g = seeded((17, 9, 5), 1.0, dtype)
    old[3][...] = dtype(0.7)
    new, _ = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    assert bits_equal(new[3], old[3])


def test_scalar_step_is_the_full_scheme():
    """the C-only step of the convergence runs below is the full reference's C"""
    old, dt, g = seeded((17, 9, 5), 1.0, np.float64)
    new, hat = MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"])
    assert bits_equal(MC.scalar_step(old[3], old[0], old[1], old[2], dt, g["dx"], g["dy"], g["dz"]), new[3])
    assert bits_equal(MC.scalar_step(old[3], old[0], old[1], old[2], dt, g["dx"], g["dy"], g["dz"], maccormack=False), hat[3])


@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS)
def test_stage_1_references_agree_in_float64(oracle, grid, cfl):
    """numpy_ref.advect(faithful=False), stage 1 of the float64 reference, and the C oracle's advect, stage 1 of the float32 one
    (advect_mc_ref.stage1 says why), are one definition: the same bits in float64 on every seeded case"""
    old, dt, g = seeded(grid, cfl, np.float64)
    hat = MC.stage1(old, dt, g["dx"], g["dy"], g["dz"])
    ref = [a.copy(order="F") for a in old]
    oracle.advect(ref[0], old[0], ref[1], old[1], ref[2], old[2], ref[3], old[3], dt, g["dx"], g["dy"], g["dz"], False)
    assert all(bits_equal(a, b) for a, b in zip(hat, ref))


def blob_errors(n, maccormack):
    """rms error and extreme values of the blob after T = 0.25"""
    C, V, dt, dx, steps, exact = MC.blob_setup(n)
    nodes = MC.node_sets(V[0], V[1], V[2], n, n, n, which=("C",))["C"]          # the same uniform velocities every step: formed once
    lo, hi = 0.0, 0.0
    for _ in range(steps):
        C = MC.scalar_step(C, V[0], V[1], V[2], dt, dx, dx, dx, maccormack=maccormack, nodes=nodes)
        lo, hi = min(lo, float(C.min())), max(hi, float(C.max()))
    return MC.rms(C, exact), lo, hi


def check_blob(err, lo, hi):
    """The issue's thresholds, shared with the device test.  err[(scheme, n)]"""
    order_mc = np.log2(err["mc", 48] / err["mc", 96])
    order_1 = np.log2(err["first", 48] / err["first", 96])
    print("rms errors %r; orders: MacCormack %.3f, first order %.3f; ratio at 48: %.2f; range [%r, %r]"
          % (err, order_mc, order_1, err["first", 48] / err["mc", 48], lo, hi))
    assert order_mc >= 1.7
    assert order_1 < 1.0
    assert err["mc", 48] < err["first", 48] / 3.0
    assert lo >= 0.0 and hi <= 1.0


def test_blob_second_order_and_bounded():
    """Gaussian blob, σ = 0.08, centre (0.3, 0.35, 0.4), unit box, uniform velocity (1, ½, ¼), dt = 0.37·dx, T = 0.25: observed order
    over n = 48 → 96 at least 1.7 (first order: below 1.0), a third of the first-order error at n = 48, all values in [0, 1]."""
    err, lo, hi = {}, 0.0, 0.0
    for n in (48, 96):
        for name, mc in (("mc", True), ("first", False)):
            err[name, n], a, b = blob_errors(n, mc)
            if mc:
                lo, hi = min(lo, a), max(hi, b)
    check_blob(err, lo, hi)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfl", CFLS)
@pytest.mark.parametrize("grid", GRIDS[1:4])
def test_the_limiter_engages_on_the_seeded_fields(grid, cfl, dtype):
    """On the seeded inputs of the GPU tests the limiter raises to lo, lowers to hi, and leaves alone, each at > 0 nodes of every
    field: the bit comparisons there exercise all three outcomes."""
    old, dt, g = seeded(grid, cfl, dtype)
    counts = {}
    MC.advect_mc(old, dt, g["dx"], g["dy"], g["dz"], counts)
    for name in MC.NAMES:
        assert counts[name]["below"] > 0 and counts[name]["above"] > 0 and counts[name]["free"] > 0, (name, counts[name])
