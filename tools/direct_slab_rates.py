#!/usr/bin/env python3
"""ns3d_poisson_direct_slab with P virtual z-slab ranks on ONE GPU against the single-rank ns3d_poisson_direct of the same global
grid — the weak-scaling grids of multi.jl (255×153×(P·151+2) global; every rank 255×153×153 locally).  Device events around each
call, warm-up calls first, best and median of the timed calls.  On one GPU the ranks share the chip, so the ratio measures what the
slab form adds (two all-to-all transposes, the unpack, the per-chunk launches), not xGMI.  One JSON line per P."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navierstokes3d_amd import kernels as K  # noqa: E402
from navierstokes3d_amd.mgpu import MultiGpu  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--P", type=int, nargs="+", default=[1, 2, 4, 8])
ap.add_argument("--nx", type=int, default=255)
ap.add_argument("--ny", type=int, default=153)
ap.add_argument("--nz", type=int, default=153, help="LOCAL nz of a rank")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-single", action="store_true", help="skip the single-rank solve of the global grid")
a = ap.parse_args()


def timed(fn, stream):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), float(np.median(ts))


nx, ny, nz = a.nx, a.ny, a.nz
for P in a.P:
    nzg = P * (nz - 2) + 2
    dx, dy, dz = 1.0 / (nx - 1), 0.6 / (ny - 1), 0.6 * P / (nzg - 1)
    gen = torch.Generator(device="cuda").manual_seed(11)
    rhs = torch.rand((nzg, ny, nx), generator=gen, device="cuda", dtype=torch.float64).permute(2, 1, 0) - 0.5
    row = dict(P=P, local=[nx, ny, nz], glob=[nx, ny, nzg], warmup=a.warmup, reps=a.reps)
    stream = torch.cuda.current_stream()
    if not a.no_single:
        ctx = K.Context(0, "strict", async_=True)
        Pg, Dg = K.zeros((nx, ny, nzg)), K.zeros((nx - 2, ny - 2, nzg - 2))
        pg = K.pt_params(Pg, 1000.0, 0.01, 0.01, 0.01, dx, dy, dz, 0, True, 0.0, 0.0)
        row["single_ms"] = timed(lambda: K.poisson_direct(Pg, Dg, rhs, pg, ctx=ctx), stream)
        ctx.close()
        del Pg, Dg
    mg = MultiGpu.create([0] * P, nx, ny, nz, "strict")          # async: the ranks follow PyTorch's current stream
    Ps = [K.zeros((nx, ny, nz)) for _ in range(P)]
    Ds = [K.zeros((nx - 2, ny - 2, nz - 2)) for _ in range(P)]
    Rs = [K.clone(rhs[:, :, r * (nz - 2):r * (nz - 2) + nz]) for r in range(P)]
    p = K.pt_params(Ps[0], 1000.0, 0.01, 0.01, 0.01, dx, dy, dz, 0, True, 0.0, 0.0)
    row["slab_ms"] = timed(lambda: mg.poisson_direct(Ps, Ds, Rs, p), stream)
    mg.sync()
    mg.close()
    mx, my, mz = nx - 2, ny - 2, P * (nz - 2)
    row["field_mb"] = mx * my * mz * 8 / 1e6
    row["alltoall_mb_each"] = mx * my * mz * 8 * (P - 1) / P / 1e6          # bytes that leave their rank, per transpose
    if "single_ms" in row:
        row["ratio_best"] = row["slab_ms"][0] / row["single_ms"][0]
    print(json.dumps(row), flush=True)
    del Ps, Ds, Rs, rhs
    torch.cuda.empty_cache()
