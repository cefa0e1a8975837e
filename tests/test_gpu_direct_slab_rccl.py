"""ns3d_poisson_direct_slab in the ONE-PROCESS-PER-GPU form: its two all-to-all transposes as one ncclGroupStart … ncclGroupEnd of
send/recv pairs per call.  The ranks are separate processes on the one GPU of the test box, bound to tests/fake_rccl (the test
double of test_gpu_fake_rccl.py).  The transport must not change a bit: every rank's planes equal the one-process virtual-rank
result of the same grid and P bitwise, and the single-rank solve of the global grid to rounding."""
import os
import socket
import sys
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_gpu_fake_rccl import FAKE_SO, ROOT, build_fake
from util import fields, geometry, rel_l2

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _problem(world, n, owns, dtype):
    nx, ny, nz = n
    nzg = world * (nz - 2) + 2
    g = geometry(nx, ny, nzg)
    rhs = fields(nx, ny, nzg, ["c"], 91, dtype)[0]
    if not owns:
        rhs[1:-1, 1:-1, 1:-1] -= rhs[1:-1, 1:-1, 1:-1].mean(dtype=np.float64).astype(dtype)
    return rhs, g


def _cut(A, r, nz):
    lo = r * (nz - 2)
    return np.asfortranarray(A[:, :, lo:lo + nz])


def _sc_direct(rank, world, uid, n, owns, val, dtype):
    """one z-slab rank per process: two calls (the second on the plan of the first)"""
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd.mgpu import MultiGpu
    nx, ny, nz = n
    rhs, g = _problem(world, n, owns, dtype)
    mg = MultiGpu.create_rank(world, rank, 0, uid, nx, ny, nz, "strict")
    Pr = K.from_numpy(fields(nx, ny, nz, ["c"], 5 + rank, dtype)[0])
    D = K.from_numpy(fields(nx, ny, nz, ["i"], 17 + rank, dtype)[0])
    R = K.from_numpy(_cut(rhs, rank, nz))
    p = K.pt_params(Pr, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"])
    mg.poisson_direct(Pr, D, R, p)
    mg.sync()
    first = K.to_numpy(Pr)
    mg.poisson_direct(Pr, D, R, p)
    mg.sync()
    out = dict(Pr=K.to_numpy(Pr), first=first, D=K.to_numpy(D), R=K.to_numpy(R))
    mg.close()
    return out


def _worker(rank, world, port, args, q):
    try:
        import faulthandler
        faulthandler.dump_traceback_later(150, exit=True)
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        os.environ["NS3D_RCCL_LIB"] = FAKE_SO
        os.environ.setdefault("FAKE_RCCL_ARENA_MB", "32")     # one group's sends per channel: ≤ 2 MB per piece here
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from navierstokes3d_amd.mgpu import MultiGpu
        box = [MultiGpu.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        assert box[0].startswith(b"/fake_rccl_")
        out = _sc_direct(rank, world, box[0], *args)
        q.put((rank, "OK", out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "ERROR", traceback.format_exc()))


def _run(world, *args, timeout=240):
    build_fake()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_worker, args=(r, world, port, args, q), daemon=True) for r in range(world)]
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


def _virtual_ranks(hip, world, n, owns, val, dtype):
    """the same grid and P in the one-process form (virtual ranks on device 0)"""
    import torch
    from navierstokes3d_amd.mgpu import MultiGpu
    nx, ny, nz = n
    rhs, g = _problem(world, n, owns, dtype)
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * world, nx, ny, nz, "strict")
    Ps = [hip.from_numpy(fields(nx, ny, nz, ["c"], 5 + r, dtype)[0]) for r in range(world)]
    Ds = [hip.from_numpy(fields(nx, ny, nz, ["i"], 17 + r, dtype)[0]) for r in range(world)]
    Rs = [hip.from_numpy(_cut(rhs, r, nz)) for r in range(world)]
    p = hip.pt_params(Ps[0], g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"], 0, owns, val, g["g"])
    mg.poisson_direct(Ps, Ds, Rs, p)
    mg.sync()
    out = [hip.to_numpy(t) for t in Ps]
    mg.close()
    # the single-rank solve of the global grid
    ctx = hip.Context(0, "strict")
    dP = hip.from_numpy(np.zeros(rhs.shape, dtype, order="F"))
    dD = hip.from_numpy(np.zeros(tuple(s - 2 for s in rhs.shape), dtype, order="F"))
    hip.poisson_direct(dP, dD, hip.from_numpy(rhs), hip.pt_params(dP, g["rho"], g["dt"], g["dtau"], g["damp"], g["dx"], g["dy"], g["dz"],
                                                                   0, owns, val, g["g"]), ctx=ctx)
    torch.cuda.synchronize()
    glob = hip.to_numpy(dP)
    ctx.close()
    return out, glob, rhs


@pytest.mark.parametrize("world,n,bc,dtype", [
    (2, (40, 21, 12), (True, 0.25), np.float64),
    (3, (24, 15, 7), (False, 0.0), np.float64),
    (3, (20, 4, 6), (True, 0.0), np.float32),          # ny − 2 < P: an empty chunk, zero-byte pairs skipped on both sides
    (2, (70, 35, 8), (False, 0.0), np.float32),
])
def test_direct_slab_one_process_per_rank_is_bitwise_the_virtual_ranks(hip, world, n, bc, dtype):
    owns, val = bc
    nz = n[2]
    want, glob, rhs = _virtual_ranks(hip, world, n, owns, val, dtype)
    got = _run(world, n, owns, val, dtype)
    tol = 1e-11 if dtype == np.float64 else 2e-6
    for r in range(world):
        assert np.array_equal(got[r]["Pr"], want[r]), "rank %d differs from the virtual-rank result" % r
        assert np.array_equal(got[r]["first"], want[r]), "rank %d: first call" % r
        assert rel_l2(got[r]["Pr"], _cut(glob, r, nz)) <= tol
        assert not got[r]["D"].any() and np.array_equal(got[r]["R"], _cut(rhs, r, nz))
