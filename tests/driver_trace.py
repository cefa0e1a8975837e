"""The two drivers' library-call trace: which ns3d_* functions of libns3d.so a run calls, in call order.

"The loop order is the contract" (navierstokes3d_amd/driver.py), and bit-equal results pin what the calls compute — but not an extra
ns3d_sync, a doubled observer call or a reordered hook that happens to commute.  A trace is the list of function names only (no
arguments), consecutive repeats run-length encoded as [name, count].  tests/golden/driver_call_trace.json holds the traces of the
cases below; tests/test_gpu_driver_trace.py compares with it.

    python tests/driver_trace.py [file]  # on the GPU machine: write the traces of the tree's drivers to the JSON file

How: navierstokes3d_amd.lib._LIB is replaced by a proxy whose attributes are wrappers that append their name and call the real
function.  kernels.Context and mgpu.MultiGpu keep the library they were created with, so the proxy is installed before any of them
exists and taken out afterwards; a trace ends when the driver returns (the objects' destruction is not part of it).
"""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_call_trace.json")

PROBES = [(-0.2, 0.0, 0.0), (0.1, 0.1, -0.1), (0.3, -0.2, 0.2)]
ISO = {"field": "Q", "level": 2.0, "color": "Pr"}
ISO_EARLY = dict(ISO, level=1e-7)        # after two steps from rest Q is still of order 1e-7: a level that gives a surface there
OBSERVERS = dict(statistics=2, stats_every=3, vortex=True, tracers=50, probes=PROBES, isosurface=ISO, do_save=True, do_vis=True)


class _Proxy:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ns3d_"):
            return fn

        def traced(*args):
            self._log.append(name)
            return fn(*args)
        return traced


@contextlib.contextmanager
def tracing():
    """the list that receives the names, while navierstokes3d_amd.lib hands out the proxy"""
    from navierstokes3d_amd import lib as L
    real, log = L.load(), []
    L._LIB = _Proxy(real, log)
    try:
        yield log
    finally:
        L._LIB = real


def rle(names):
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return out


def _multi(**kw):
    from navierstokes3d_amd.driver import run_navierstokes3D
    with tracing() as log:
        out = run_navierstokes3D(nx=24, mode="strict", niter_cap=40, return_info=True, **kw)
        got = list(log)
    return got, out[-1]


def _gpu(**kw):
    from navierstokes3d_amd.driver import runme
    with tracing() as log:
        _f, info = runme(nx=24, mode="strict", niter_cap=40, **kw)
        got = list(log)
    return got, info


def _two_ranks():
    """two virtual z-slab ranks on one device, each on a stream of its own, as test_gpu_stats.test_driver_on_two_virtual_z_slab_ranks
    builds them"""
    import torch
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    nx, P, nz_loc = 36, 2, 12
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    torch.cuda.synchronize()
    with tracing() as log:
        mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict", own_streams=True)
        try:
            out = run_navierstokes3D(nx=nx, nt=2, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), return_info=True,
                                     shape=dict(nz=nz_loc), wide_advect_halo=True, niter_cap=40, statistics=2, vortex=True,
                                     isosurface=ISO_EARLY, diagnostics=True, do_save=True)
            got = list(log)
        finally:
            mg.sync()
            mg.close()
    return got, out[-1]


CASES = {
    "a_multi_observers": lambda: _multi(nt=11, **OBSERVERS),
    "b_multi_observers_diagnostics": lambda: _multi(nt=11, diagnostics=True, do_print=True, **OBSERVERS),
    "c_multi_reference_loop": lambda: _multi(nt=2, fused=False),
    "d_gpu_observers": lambda: _gpu(nt=11, **OBSERVERS),
    "e_gpu_diagnostics": lambda: _gpu(nt=2, diagnostics=True),
    "f_two_z_slab_ranks": _two_ranks,
}


def record(case, workdir):
    """(run-length encoded trace, info) of one case, run with `workdir` as the working directory (the frames' files go there)"""
    import torch
    here = os.getcwd()
    os.chdir(workdir)
    try:
        names, info = CASES[case]()
        torch.cuda.synchronize()
    finally:
        os.chdir(here)
    return rle(names), info


def first_difference(got, want):
    """None, or a sentence that names the first position at which two run-length encoded traces differ"""
    for q, (g, w) in enumerate(zip(got, want)):
        if list(g) != list(w):
            before = " after " + " ".join("%s×%d" % tuple(x) for x in want[max(0, q - 3):q]) if q else ""
            return "run %d%s: got %s×%d, recorded %s×%d" % (q, before, g[0], g[1], w[0], w[1])
    if len(got) != len(want):
        longer, which = (got, "got") if len(got) > len(want) else (want, "recorded")
        q = min(len(got), len(want))
        return "run %d: only the %s trace goes on, with %s×%d (%d runs against %d)" % (q, which, longer[q][0], longer[q][1], len(got), len(want))
    return None


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    out = {}
    for case in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            out[case], info = record(case, tmp)
        iso, vort = getattr(info, "isosurface", None), getattr(info, "vortex", None)
        print("%s: %d calls in %d runs; isosurface: %s triangles; max Q = %s"
              % (case, sum(n for _, n in out[case]), len(out[case]), None if iso is None else iso.n,
                 None if vort is None else float(vort.Q.max())), flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w", encoding="utf-8") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")
    print("→ %s" % path)
