"""ns3d_diagnostics_mgpu in the ONE-PROCESS-PER-GPU form: rank processes on the one GPU of the test box, the all-reduces served
by the test double tests/fake_rccl (as tests/test_gpu_fake_rccl.py runs that arm).  Every rank must receive the global record:
maxima and counts those of the one-rank call on the global arrays bit for bit, sums within (L+8)·2⁻⁵³·Σ|term|."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_gpu_fake_rccl import FAKE_SO, ROOT, _free_port, build_fake

pytestmark = pytest.mark.gpu
N_LOCAL = (20, 13, 9)


def _worker(rank, world, port, dims, dtype, q):
    try:
        import faulthandler
        faulthandler.dump_traceback_later(150, exit=True)
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ["NS3D_RCCL_LIB"] = FAKE_SO
        os.environ.setdefault("FAKE_RCCL_ARENA_MB", "8")
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from navierstokes3d_amd import kernels as K
        from navierstokes3d_amd.mgpu import MultiGpu
        from oracle.driver_ref import cart_coords
        from test_gpu_diagnostics import _cut, _global_problem
        box = [MultiGpu.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        assert box[0].startswith(b"/fake_rccl_")
        n = N_LOCAL
        ng, g, G, cyl_at = _global_problem(dims, n, dtype)
        mg = MultiGpu.create_rank(world, rank, 0, box[0], *n, "strict", dims=dims)
        assert mg.transport == "rccl" and mg.nlocal == 1
        c = cart_coords(rank, dims)
        cu = _cut(G, c, n)
        dev = [K.from_numpy(cu[k]) for k in ("Vx", "Vy", "Vz", "Pr", "C")]
        dp = K.diag_params(*n, g["dx"], g["dy"], g["dz"], g["rho"], cylinder=cyl_at(c[0], c[1]))
        glob, locs = mg.diagnostics(*dev, dp)
        bare = mg.diagnostics(dev[0], dev[1], dev[2], None, None, dp)[0]
        mg.sync()
        mg.close()
        q.put((rank, "OK", (vars(glob), vars(locs[0]), vars(bare))))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "ERROR", traceback.format_exc()))


def _run(world, dims, dtype, timeout=240):
    build_fake()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_worker, args=(r, world, port, dims, dtype, q), daemon=True) for r in range(world)]
    for pr in procs:
        pr.start()
    got = {}
    try:
        for _ in range(world):
            r = q.get(timeout=timeout)
            assert r[1] == "OK", r[2]
            got[r[0]] = r[2]
    finally:
        for pr in procs:
            pr.join(timeout=30)
            if pr.is_alive():
                pr.kill()
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dims", [(1, 1, 2), (1, 1, 3), (2, 1, 1), (2, 2, 1)])
def test_rank_processes_receive_the_global_record(hip, dims, dtype):
    from types import SimpleNamespace
    from test_gpu_diagnostics import _check_global, _global_problem
    world = dims[0] * dims[1] * dims[2]
    got = _run(world, dims, dtype)
    ng, g, G, cyl_at = _global_problem(dims, N_LOCAL, dtype)
    ctx = hip.Context(0, "strict")
    glob = SimpleNamespace(**got[0][0])
    _check_global(hip, ctx, glob, None, ng, N_LOCAL, g, G, cyl_at, dtype, world)
    locs = [SimpleNamespace(**got[r][1]) for r in range(world)]
    for r in range(world):
        assert got[r][0] == got[0][0], "rank %d received another global record" % r
        bare = got[r][2]
        assert np.isnan(bare["pr_min"]) and np.isnan(bare["pr_max"]) and np.isnan(bare["c_vol"])
        assert bare["vmax"] == got[0][0]["vmax"] and bare["ke"] == got[0][0]["ke"]
    # the double adds the ranks' contributions in rank order, so the local sums add up exactly here too
    for k in ("ke", "c_vol"):
        s = getattr(locs[0], k)
        for l in locs[1:]:
            s += getattr(l, k)
        assert s == getattr(glob, k), k
    assert tuple(sum(l.n_masked[q] for l in locs) for q in range(3)) == glob.n_masked
    ctx.close()
