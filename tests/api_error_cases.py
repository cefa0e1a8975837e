"""What the typed single-device entry points of libns3d.so (csrc/ns3d_api.cpp, ns3d_poisson_direct of csrc/ns3d_direct.hip) decide
BEFORE a kernel runs: which argument error is reported, with which status and in which words.

A case is one call of one entry point, for f64 or f32, on real device arrays of an 8×6×5 grid (distinct extents that pass every
size check, so a transposed extent would show) in which every argument is valid and exactly one is defective.  The record of a
case is (status, message of ns3d_last_error()).  tests/golden/api_errors.json holds the records of the library as it was before
these entry points moved from macro bodies into csrc/ns3d_api_typed.h; tests/test_gpu_api_errors.py compares with it.

    python tests/api_error_cases.py        # on the GPU machine: write the records of the library in the tree to the JSON file

Safety: CHECKED, GRIDS and the explicit cases below are read off the sources, not probed.  A case nulls a pointer only where the
entry point tests it before anything is launched, or where include/ns3d.h documents NULL as allowed (Pr and C of
ns3d_diagnostics, Pr of ns3d_stats_accumulate, the outputs of ns3d_pt_solve); no case hands a kernel a bad pointer or extent.  The
few cases that are legal calls (status 0, recorded with an empty message) run their kernels on valid arguments.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_errors.json")
NX, NY, NZ = 8, 6, 5
GRID = [NX, NY, NZ]
DX, DY, DZ = 0.1, 0.125, 0.2
SPACING = [DX, DY, DZ]
NAN, INF = float("nan"), float("inf")
STATS_SLOTS = 11       # NS3D_STATS_SLOTS


class Arena:
    """Zeroed device arrays of one element type, one per name, each large enough for any field of the grid (staggered ones and
    the 11 accumulator blocks of ns3d_stats included).  arena("Vx") is the same address every time."""

    def __init__(self, L, suffix):
        import torch
        self.L = L
        self.torch = torch
        self.dtype = {"f64": torch.float64, "f32": torch.float32}[suffix]
        self.held = {}

    def __call__(self, name, dtype=None):
        if name not in self.held:
            n = STATS_SLOTS * (NX + 1) * (NY + 1) * (NZ + 1)
            self.held[name] = self.torch.zeros(n, dtype=dtype or self.dtype, device="cuda")
        return self.held[name].data_ptr()

    def ptrs(self, *names):
        return [self(n) for n in names]


def _pt_params(L):
    return L.PtParams(rho=1.0, dt=0.1, dtau=0.01, damp=0.9, dx=DX, dy=DY, dz=DZ, nx=NX, ny=NY, nz=NZ, bc_kind=L.NS3D_BC_MULTI,
                      owns_outlet=1, outlet_val=0.0, g=0.0, z_lo_is_halo=0, z_hi_is_halo=0)


def _diag_params(L):
    return L.DiagParams(nx=NX, ny=NY, nz=NZ, dx=DX, dy=DY, dz=DZ, rho=1.0, cylinder=0)


def _step_fields(L, a):
    names = [n for n, _ in L.StepFields._fields_]
    return L.StepFields(**{n: a("step_" + n) for n in names})


def _step_params(L):
    return L.StepParams(script=L.NS3D_BC_MULTI, nx=NX, ny=NY, nz=NZ, mu=1e-3, rho=1.0, g=0.0, dt=0.1, dtau=0.01, damp=0.9, dx=DX, dy=DY,
                        dz=DZ, eps=1e-6, niter=4, nchk=2, err_mul=1.0, err_div=1.0, a2=0.01, b2=0.01, ox=0.0, oy=0.0, sinb=0.0,
                        cosb=1.0, xco_g=0.0, yco_g=0.0, zco_g=0.0, lx=0.8, ly=0.75, lz=1.0, owns_inlet=1, owns_outlet=1, vin=1.0,
                        faithful=1, pressure=0, write_stress=0)


# name → valid arguments after the context (a: the arena; ctypes objects are passed by reference)
VALID = {
    "update_tau": lambda L, a: a.ptrs("txx", "tyy", "tzz", "txy", "txz", "tyz", "Vx", "Vy", "Vz") + [1e-3] + SPACING + GRID,
    "predict_V": lambda L, a: a.ptrs("Vx", "Vy", "Vz", "txx", "tyy", "tzz", "txy", "txz", "tyz") + [1.0, 0.0, 0.1] + SPACING + GRID,
    "predict_fused": lambda L, a: a.ptrs("Vx_o", "Vy_o", "Vz_o", "Vx", "Vy", "Vz") + [1e-3, 1.0, 0.0, 0.1] + SPACING + GRID,
    "set_cylinder": lambda L, a: a.ptrs("C", "Vx", "Vy", "Vz") + [0.01, 0.01, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.8, 0.75, 1.0] + SPACING + GRID,
    "set_cylinder_local": lambda L, a: a.ptrs("C", "Vx", "Vy", "Vz") + [0.01, 0.01, 0.0, 0.0, 0.0, 1.0, 0.8, 0.75, 1.0] + SPACING + GRID,
    "update_divV": lambda L, a: a.ptrs("divV", "Vx", "Vy", "Vz") + SPACING + GRID,
    "update_dPrdtau": lambda L, a: a.ptrs("Pr", "dPrdtau", "divV") + [1.0, 0.1, 0.01, 0.9] + SPACING + GRID,
    "update_Pr": lambda L, a: a.ptrs("Pr", "dPrdtau") + [0.01] + GRID,
    "compute_res": lambda L, a: a.ptrs("Rp", "Pr", "divV") + [1.0, 0.1] + SPACING + GRID,
    "max_abs": lambda L, a: [a("Pr"), NX * NY * NZ, C.c_double()],
    "correct_V": lambda L, a: a.ptrs("Vx", "Vy", "Vz", "Pr") + [0.1, 1.0] + SPACING + GRID,
    "diagnostics": lambda L, a: a.ptrs("Vx", "Vy", "Vz", "Pr", "C") + [_diag_params(L), L.Diag()],
    "stats_accumulate": lambda L, a: [a("S", a.torch.float64)] + a.ptrs("Vx", "Vy", "Vz", "Pr") + [1.0] + GRID,
    "bc_x": lambda L, a: [a("Pr")] + GRID,
    "bc_y": lambda L, a: [a("Pr")] + GRID,
    "bc_z": lambda L, a: [a("Pr")] + GRID,
    "bc_zV": lambda L, a: [a("Vx")] + [NX + 1, NY, NZ],
    "bc_xhydstatic": lambda L, a: [a("Pr"), DZ, NZ, 9.81, 1.0] + GRID,
    "bc_x_Vx": lambda L, a: [a("Vx"), 1.0] + [NX + 1, NY, NZ],
    "bc_x_Pr": lambda L, a: [a("Pr"), 0.0] + GRID,
    "copy": lambda L, a: a.ptrs("Pr_o", "Pr") + [NX * NY * NZ],
    "advect": lambda L, a: a.ptrs("Vx", "Vx_o", "Vy", "Vy_o", "Vz", "Vz_o", "C", "C_o") + [0.1] + SPACING + GRID + [1],
    "copy_advect": lambda L, a: a.ptrs("Vx_o", "Vx", "Vy_o", "Vy", "Vz_o", "Vz", "C_o", "C") + [0.1] + SPACING + GRID + [1],
    "set_bc_Pr": lambda L, a: [a("Pr"), L.NS3D_BC_MULTI, 1, 0.0, DZ, NZ, 9.81, 1.0] + GRID,
    "set_bc_Vel": lambda L, a: a.ptrs("Vx", "Vy", "Vz") + [L.NS3D_BC_MULTI, 1, 1.0] + GRID,
    "pt_iterate": lambda L, a: a.ptrs("Pr", "dPrdtau", "divV") + [_pt_params(L), 2],
    "poisson_direct": lambda L, a: a.ptrs("Pr", "dPrdtau", "divV") + [_pt_params(L)],
    "pt_sweep": lambda L, a: a.ptrs("Pr", "Pr_o", "dPrdtau", "divV") + [_pt_params(L), 1, NZ - 1],
    "pt_sweep2": lambda L, a: a.ptrs("Pr", "Pr_o", "dPrdtau", "dPrdtau_o", "divV") + [_pt_params(L), 1, NZ - 1],
    "plan_pt": lambda L, a: a.ptrs("Pr", "Pr_o", "dPrdtau", "dPrdtau_o", "divV") + [_pt_params(L), 1, NZ - 1],
    "pt_sweepn": lambda L, a: [3] + a.ptrs("Pr", "Pr_o", "dPrdtau", "dPrdtau_o", "divV") + [_pt_params(L), 1, NZ - 1],
    "residual_max": lambda L, a: a.ptrs("Pr", "divV") + [_pt_params(L), C.c_double()],
    "selftest_exact_div": lambda L, a: [0.1, 1024, 1, C.c_long()],
    "pt_solve": lambda L, a: a.ptrs("Pr", "dPrdtau", "divV") + [_pt_params(L), 1e-6, 4, 2, 1.0, 1.0, C.c_int(), (C.c_double * 4)(), 4, C.c_int()],
    "time_step": lambda L, a: [_step_fields(L, a), _step_params(L), C.c_int(), (C.c_double * 4)(), 4, C.c_int()],
}

# name → positions (after the context) of the pointers the entry point tests for NULL before anything else happens: its CHECK_PTRS
# list in list order, then the pointers it tests by hand (parameter structs)
CHECKED = {
    "update_tau": range(9), "predict_V": range(9), "predict_fused": range(6), "set_cylinder": range(4), "set_cylinder_local": range(4),
    "update_divV": range(4), "update_dPrdtau": range(3), "update_Pr": range(2), "compute_res": range(3), "max_abs": [0, 2],
    "correct_V": range(4), "diagnostics": [0, 1, 2, 6, 5], "stats_accumulate": range(4), "bc_x": [0], "bc_y": [0], "bc_z": [0],
    "bc_zV": [0], "bc_xhydstatic": [0], "bc_x_Vx": [0], "bc_x_Pr": [0], "copy": [0, 1], "advect": range(8), "copy_advect": range(8),
    "set_bc_Pr": [0], "set_bc_Vel": range(3), "pt_iterate": range(4), "poisson_direct": range(4), "pt_sweep": range(5),
    "pt_sweep2": range(6), "plan_pt": range(6), "pt_sweepn": range(1, 7), "residual_max": [0, 1, 3, 2], "selftest_exact_div": [3],
    "pt_solve": range(4), "time_step": [0, 1],
}
# name → (position of the first of the three extents, the least extent the entry point accepts)
GRIDS = {
    "update_tau": (13, 2), "predict_V": (15, 2), "predict_fused": (13, 2), "set_cylinder": (19, 1), "set_cylinder_local": (16, 1),
    "update_divV": (7, 1), "update_dPrdtau": (10, 3), "update_Pr": (3, 3), "compute_res": (8, 3), "correct_V": (9, 2),
    "stats_accumulate": (6, 3), "bc_x": (1, 2), "bc_y": (1, 2), "bc_z": (1, 2), "bc_zV": (1, 2), "bc_xhydstatic": (5, 2),
    "bc_x_Vx": (2, 2), "bc_x_Pr": (2, 2), "advect": (12, 1), "copy_advect": (12, 1), "set_bc_Pr": (8, 2), "set_bc_Vel": (6, 2),
}
# name → position of its ns3d_pt_params (ns3d_check_pt_params: extents ≥ 3, the boundary set, no z halos with gpu.jl's)
PT_PARAMS = {"pt_iterate": 3, "poisson_direct": 3, "pt_sweep": 4, "pt_sweep2": 5, "plan_pt": 5, "pt_sweepn": 6, "residual_max": 2, "pt_solve": 3}
# the sweep entry points: positions of (Pr_in, Pr_out, dPrdtau_in, dPrdtau_out or None, k0)
SWEEPS = {"pt_sweep": (0, 1, 2, None, 5), "pt_sweep2": (0, 1, 2, 3, 6), "plan_pt": (0, 1, 2, 3, 6), "pt_sweepn": (1, 2, 3, 4, 7)}
LEGAL = "legal"     # marks the cases that are valid calls


def cases():
    """[(label, entry point, modifications, suffixes)] — a modification is ("arg", position, value), ("alias", position, position
    whose value it takes) or ("field", position of the struct, field, value)."""
    out = []

    def add(fn, label, *mods, only=("f64", "f32")):
        out.append(("%s:%s" % (fn, label), fn, mods, only))

    for fn, positions in CHECKED.items():
        for q in positions:
            add(fn, "null_arg%d" % q, ("arg", q, None))
    for fn, (at, least) in GRIDS.items():
        for d in range(3):
            add(fn, "small_%s" % "xyz"[d], ("arg", at + d, least - 1))
    for d in "xyz":
        add("diagnostics", "small_" + d, ("field", 5, "n" + d, 2))
    add("diagnostics", "cylinder_form_3", ("field", 5, "cylinder", 3))
    for fn, at in PT_PARAMS.items():
        for d in "xyz":
            add(fn, "small_" + d, ("field", at, "n" + d, 2))
        add(fn, "bc_kind_7", ("field", at, "bc_kind", 7))
        for side in ("lo", "hi"):
            add(fn, "gpu_set_with_z_%s_halo" % side, ("field", at, "bc_kind", 1), ("field", at, "z_%s_is_halo" % side, 1))
    for d in "xyz":
        add("poisson_direct", "three_" + d, ("field", 3, "n" + d, 3))         # its own minimum is 4
    for side in ("lo", "hi"):
        for fn in ("pt_sweep2", "pt_sweepn", "pt_solve", "poisson_direct"):
            add(fn, "z_%s_halo" % side, ("field", PT_PARAMS[fn], "z_%s_is_halo" % side, 1))
    for fn, (pin, pout, din, dout, k0) in SWEEPS.items():
        add(fn, "Pr_in_is_Pr_out", ("alias", pout, pin))
        if dout is not None:
            add(fn, "dPrdtau_in_is_dPrdtau_out", ("alias", dout, din))
        add(fn, "k0_0", ("arg", k0, 0))
        add(fn, "k1_nz", ("arg", k0 + 1, NZ))
        add(fn, "k0_above_k1", ("arg", k0, 3), ("arg", k0 + 1, 2))
    add("pt_sweepn", "nlev_1", ("arg", 0, 1))
    add("pt_sweepn", "nlev_6", ("arg", 0, 6))
    add("pt_sweepn", "nlev_5", ("arg", 0, 5), only=("f64",))
    add("max_abs", "negative_n", ("arg", 1, -1))
    add("copy", "negative_n", ("arg", 2, -1))
    add("pt_solve", "negative_niter", ("arg", 5, -1))
    add("pt_solve", "negative_nchk", ("arg", 6, -1))
    add("set_bc_Pr", "bc_kind_7", ("arg", 1, 7))
    add("set_bc_Vel", "bc_kind_7", ("arg", 3, 7))
    for q, n in enumerate("xyz"):
        add("predict_fused", "V%s_new_is_V%s" % (n, n), ("alias", q, q + 3))
    for faithful in (0, 1):
        for q, n in ((0, "Vx"), (2, "Vy"), (6, "C")):
            add("copy_advect", "%s_new_is_%s_faithful%d" % (n, n, faithful), ("alias", q, q + 1), ("arg", 15, faithful))
    add("copy_advect", "Vz_new_is_Vz_faithful0", ("alias", 4, 5), ("arg", 15, 0))
    add("copy_advect", "Vz_new_is_Vz_faithful1_" + LEGAL, ("alias", 4, 5), ("arg", 15, 1))
    for label, d in (("zero", 0.0), ("negative", -1.0), ("nan", NAN), ("2_to_101", 2.0 ** 101), ("all_ones", 2.0 - 2.0 ** -52)):
        add("selftest_exact_div", "divisor_" + label, ("arg", 0, d))
    add("stats_accumulate", "weight_nan", ("arg", 5, NAN))
    add("stats_accumulate", "weight_inf", ("arg", 5, INF))
    add("time_step", "script_7", ("field", 1, "script", 7))
    for t in ("txx", "tyy", "tzz", "txy", "txz", "tyz"):
        add("time_step", "write_stress_without_" + t, ("field", 1, "write_stress", 1), ("field", 0, t, None))
    # NULL where include/ns3d.h allows it
    add("diagnostics", "no_Pr_" + LEGAL, ("arg", 3, None))
    add("diagnostics", "no_C_" + LEGAL, ("arg", 4, None))
    add("stats_accumulate", "no_Pr_" + LEGAL, ("arg", 4, None))
    for q, n in ((9, "iters_done"), (10, "err_hist"), (12, "n_checks")):
        add("pt_solve", "no_%s_%s" % (n, LEGAL), ("arg", q, None))
    return out


def run_case(L, handle, arena, suffix, fn, mods):
    """(status, message) of one call"""
    args = VALID[fn](L, arena)
    for m in mods:
        if m[0] == "arg":
            args[m[1]] = m[2]
        elif m[0] == "alias":
            args[m[1]] = args[m[2]]
        else:
            setattr(args[m[1]], m[2], m[3])
    call = [C.byref(x) if isinstance(x, (C.Structure, C._SimpleCData)) else x for x in args]
    lib = L.load()
    rc = getattr(lib, "ns3d_%s_%s" % (fn, suffix))(handle, *call)
    return [int(rc), L.last_error() if rc else ""]


def record():
    """{suffix: {label: [status, message]}} of the library in the tree, every case"""
    import torch
    from navierstokes3d_amd import kernels, lib as L
    ctx = kernels.Context(mode="strict")
    out = {}
    for suffix in ("f64", "f32"):
        arena = Arena(L, suffix)
        out[suffix] = {label: run_case(L, ctx.handle, arena, suffix, fn, mods) for label, fn, mods, only in cases() if suffix in only}
        ctx.sync()
        torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    got = record()
    with open(GOLDEN, "w", encoding="utf-8") as f:
        json.dump(got, f, indent=0, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d + %d records → %s" % (len(got["f64"]), len(got["f32"]), GOLDEN))
