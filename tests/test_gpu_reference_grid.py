"""The single-GPU script (gpu.jl: gravity 9.81, hydrostatic x planes, no-slip bed, the local-coordinate cylinder with its
dx-for-dy quirk) at the grid the script itself hard-codes, 255×153×153 (gpu.jl:44), whole time steps in Float32 through both
drivers, and the literal 63×63×63 of BASELINE.json configs[0] — every run against the oracle driver run here on the same inputs.

Bars: STRICT = identical PT-iteration counts, identical err history, fields bit for bit (np.array_equal);
      FAST   = identical counts — asserted only after the REFERENCE's own err history has been shown to keep every residual check
               more than 1e-3 (relative) away from ε, so that the stop decision cannot hinge on FAST's rounding
               (util.checks_inside_margin) — and ≤ 1e-6 relative L2 per field (util.assert_fields_close).

At 255×153×153 (5.97 M cells, above the 3 M cells where HIP-graph replay ends) ns3d_pt_solve plans for itself: two-, three- and
four-iteration passes, chunked and one-round variants, the face-folding epilogue; under the gpu.jl pressure rule the x planes it
has to reproduce depend on the global iz, nz, g, ρ and dz."""
import numpy as np
import pytest

from util import NAMES, assert_bit_identical, assert_fields_close, checks_inside_margin, errs_identical

pytestmark = pytest.mark.gpu
PATHS = [(True, True), (True, False), (False, False)]           # (fused, one_call): one ns3d_time_step per step | call by call | unfused


def _host(hip, f):
    return [hip.to_numpy(getattr(f, n)) for n in NAMES]


def _ref_fields(rf):
    return [np.asarray(rf[n]) for n in NAMES]


@pytest.fixture(scope="module")
def gpu_ref_capped():
    from oracle.driver_ref import runme_ref
    return runme_ref(nx=255, nt=2, niter_cap=304)


@pytest.fixture(scope="module")
def gpu_ref_uncapped():
    from oracle.driver_ref import runme_ref
    return runme_ref(nx=255, nt=2)


# ---- A. gpu.jl semantics at 255×153×153 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,one_call", PATHS)
def test_gpu_script_255_capped_vs_oracle(hip, gpu_ref_capped, fused, one_call):
    """Two steps with the PT loop capped at two residual checks (304 iterations each: under gravity the first step iterates too):
    counts, the whole err history and the five fields bit for bit — as one ns3d_time_step call per step, fused call by call, and as
    the literal per-kernel sequence (3 × 608 launches of the single kernels plus four residual checks)."""
    from navierstokes3d_amd.driver import runme
    rf, rinfo = gpu_ref_capped
    assert rinfo.iters == [304, 304] and all(len(e) == 2 and np.isfinite(e).all() for e in rinfo.errs)
    assert all(np.isfinite(a).all() for a in _ref_fields(rf)) and np.abs(rf["Pr"]).max() > 1e3      # hydrostatic magnitudes
    f, info = runme(nx=255, nt=2, mode="strict", fused=fused, one_call=one_call, niter_cap=304)
    assert info.params.ny == 153 and info.params.nz == 153 and info.params.nchk == 152
    assert info.iters == rinfo.iters and info.errs == rinfo.errs
    assert_bit_identical(_host(hip, f), _ref_fields(rf))


def test_gpu_script_255_capped_fast_mode(hip, gpu_ref_capped):
    from navierstokes3d_amd.driver import runme
    rf, rinfo = gpu_ref_capped
    f, info = runme(nx=255, nt=2, mode="fast", niter_cap=304)
    assert info.iters == rinfo.iters == [304, 304]              # the cap ends both loops: no stop decision is involved
    assert_fields_close(_host(hip, f), _ref_fields(rf))


def test_gpu_script_255_uncapped_vs_oracle(hip, gpu_ref_uncapped):
    """gpu.jl as it ships, two steps: both run 3 952 PT iterations (26 residual checks) to err < 1e-3.  Counts, err histories
    and fields bit for bit (the oracle's 7 904 unfused iterations take about a minute of CPU time)."""
    from navierstokes3d_amd.driver import runme
    rf, rinfo = gpu_ref_uncapped
    assert rinfo.iters == [3952, 3952] and [len(e) for e in rinfo.errs] == [26, 26]
    f, info = runme(nx=255, nt=2, mode="strict")
    assert info.iters == rinfo.iters and info.errs == rinfo.errs
    assert_bit_identical(_host(hip, f), _ref_fields(rf))


def test_gpu_script_255_uncapped_fast_mode(hip, gpu_ref_uncapped):
    """FAST on the same reference run.  First, on the reference alone: no residual check lies within 1e-3 of ε (the nearest is the
    second step's last but one, err 1.0135e-3, 1.35 % above), so FAST has to stop where the reference stops."""
    from navierstokes3d_amd.driver import runme
    rf, rinfo = gpu_ref_uncapped
    assert rinfo.iters == [3952, 3952]
    assert checks_inside_margin(rinfo.errs, rinfo.params.eps) == []
    f, info = runme(nx=255, nt=2, mode="fast")
    assert info.iters == rinfo.iters
    assert_fields_close(_host(hip, f), _ref_fields(rf))


# ---- D. whole time steps in Float32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_call", [True, False])
def test_multi_script_f32_nx63_vs_oracle(hip, one_call):
    """run_navierstokes3D in Float32 against the oracle's REAL=float build: every scalar the host hands over (dt/ρ, spacings,
    cylinder constants) is a double that each side rounds to Float32 where the Julia expression evaluated in Float32 would."""
    import torch
    from navierstokes3d_amd.driver import run_navierstokes3D
    from oracle.driver_ref import run_navierstokes3D_ref
    ref = run_navierstokes3D_ref(nx=63, nt=4, dtype=np.float32)
    assert ref[-1].iters == [37, 259, 296, 333] and all(a.dtype == np.float32 and np.isfinite(a).all() for a in ref[:5])
    out = run_navierstokes3D(nx=63, nt=4, mode="strict", dtype=torch.float32, one_call=one_call, return_info=True)
    assert out[-1].iters == ref[-1].iters and out[-1].errs == ref[-1].errs
    assert_bit_identical(out[:5], ref[:5])


@pytest.mark.parametrize("nx,cap,iters", [(40, None, [1200, 1200]), (255, 304, [304, 304])])
@pytest.mark.parametrize("one_call", [True, False])
def test_gpu_script_f32_vs_oracle(hip, nx, cap, iters, one_call):
    """runme in Float32.  At 40×24×24 the Float32 residual never reaches ε under gravity and both loops end at niter = 1 200;
    at 255×153×153 the loop is capped at two checks."""
    import torch
    from navierstokes3d_amd.driver import runme
    from oracle.driver_ref import runme_ref
    rf, rinfo = runme_ref(nx=nx, nt=2, dtype=np.float32, niter_cap=cap)
    assert rinfo.iters == iters and all(rf[n].dtype == np.float32 and np.isfinite(rf[n]).all() for n in NAMES)
    f, info = runme(nx=nx, nt=2, mode="strict", dtype=torch.float32, niter_cap=cap, one_call=one_call)
    assert info.iters == rinfo.iters and info.errs == rinfo.errs
    assert_bit_identical(_host(hip, f), _ref_fields(rf))


def _f32_two_z_slab_ranks(hip, nt):
    import torch
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    from oracle.driver_ref import run_navierstokes3D_ref
    ref = run_navierstokes3D_ref(nx=63, nt=nt, dims_z=2, dtype=np.float32)
    assert ref[-1].iters == [37, 259, 74, 37][:nt]
    p0 = multi_params(63)
    mg = MultiGpu.create([0, 0], p0.nx, p0.ny, p0.nz, "strict")
    out = run_navierstokes3D(nx=63, nt=nt, mode="strict", dtype=torch.float32, grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz),
                             return_info=True)
    info = out[-1]
    assert info.iters == ref[-1].iters and errs_identical(info.errs, ref[-1].errs), (info.errs, ref[-1].errs)
    for r in range(2):
        for n in ("C", "Pr", "Vx", "Vy", "Vz", "divV", "dPrdtau"):
            got = hip.to_numpy(getattr(info.local_fields[r], n))
            assert got.dtype == np.float32 and np.array_equal(got, ref[-1].ranks[r][n], equal_nan=True), (r, n)
    assert_bit_identical(out[:5], ref[:5])
    mg.close()
    return ref


def test_multi_script_f32_on_two_z_slab_ranks_vs_oracle(hip):
    """Float32 steps on two virtual z-slab ranks (local 63×38×38, global 63×38×74) against the oracle's two virtual ranks, four
    steps: counts, err histories, every local field of either rank and the gathered return arrays, bit for bit.

    This decomposition follows the reference into its instability in the third step (err 4.17e17, then NaN at the second check; the
    fourth step stops at its first check with NaN: iters 37, 259, 74, 37 — in Float64 likewise, 37, 259, 444, 37 with err = Inf),
    so the `!isfinite(err)` exits have to be taken at the same checks, NaN for NaN.  After that exit the velocities are of order
    1e295 (1e30 in Float32) on both ranks and backtrack!'s floor(Int, ·) is out of range in most cells: Julia throws InexactError
    there, and the oracle's `(long)` conversion was undefined behaviour in C (x86 turns +1e295 into LONG_MIN and the clamp then took
    the wrong end), which made rank 0's divV differ in 2 063 of 90 972 cells and rank 1's in 22 736.  The oracle now clamps before
    it converts (ns3d_oracle.c clampf: the clamp of unbounded integers, lo for NaN) as the HIP kernels always did (clampf_i), and
    the four steps are bit-identical."""
    ref = _f32_two_z_slab_ranks(hip, 4)
    assert np.isnan(ref[-1].errs[2][-1]) and np.isfinite(ref[-1].errs[1]).all()


def test_multi_script_f32_on_two_z_slab_ranks_before_the_instability(hip):
    """The same run stopped after its second step — the last one a Julia run completes (err 9.147e-4 after 259 iterations): both
    ranks exchange halos through a whole Float32 PT loop and every local field equals the oracle's, bit for bit."""
    ref = _f32_two_z_slab_ranks(hip, 2)
    assert all(np.isfinite(a).all() for a in ref[:5]) and np.isfinite(ref[-1].errs[1]).all()


# ---- F. the literal 63×63×63 of BASELINE.json configs[0] ----------------------------------------------------------------------
@pytest.mark.parametrize("one_call", [True, False])
def test_multi_script_63_cubed_vs_oracle(hip, one_call):
    """multi.jl's nx = 63 gives 63×38×38; the cube needs the explicit-shape entry (ny = nz = 63, ly = lz = lx).  Five steps."""
    from navierstokes3d_amd.driver import run_navierstokes3D
    from oracle.driver_ref import run_navierstokes3D_ref
    shape = dict(ny=63, nz=63, ly_lx=1.0, lz_lx=1.0)
    ref = run_navierstokes3D_ref(nx=63, nt=5, shape=shape)
    p = ref[-1].params
    assert (p.nx, p.ny, p.nz, p.nchk) == (63, 63, 63, 62)
    assert ref[-1].iters == [62, 372, 372, 434, 496] and all(np.isfinite(b).all() for b in ref[:5])
    assert any(i > p.nchk for i in ref[-1].iters)               # the PT loop iterates past its first check
    out = run_navierstokes3D(nx=63, nt=5, mode="strict", shape=shape, one_call=one_call, return_info=True)
    assert out[-1].iters == ref[-1].iters and out[-1].errs == ref[-1].errs
    assert_bit_identical(out[:5], ref[:5])
