"""Times of the obstacle calls — ns3d_voxelize, ns3d_set_solid, ns3d_solid_momentum — next to ns3d_set_cylinder and a plain copy.

    python tools/solid_rates.py [--out profiles/solid_rates.jsonl] [--grids 255x153x153,512x512x512]

Two bodies per grid: the reference cylinder's own mask (solid.mask_of_cylinder) and an ellipsoid with semi-axes of 45, 40 and 35
cells whose surface comes from ns3d_isosurface (about 10^5 triangles).  Event timing on the stream the NS3D_ASYNC context launches on:
every window holds enough back-to-back calls to last at least 5 ms (events resolve about a microsecond), best of 7 windows after a
warm-up window, the sides interleaved in one process.  ns3d_solid_momentum blocks for its read-back, so its window is a host clock
around the calls.  ns3d_set_solid reads (nx+1)(ny+1)(nz+1) mask bytes; `mask_rate_of_copy` is that byte count over its time as a
fraction of the bytes a device-to-device copy of the same array moves (read plus write) over ITS time.  One JSON line per grid, body
and element type."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_MS = 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solid_rates.jsonl"))
    ap.add_argument("--grids", default="255x153x153,512x512x512")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "solid_rates needs a GPU: there is nothing to time without one"
    from navierstokes3d_amd import isosurface as ISO, kernels as K, solid as S
    from navierstokes3d_amd.params import multi_params

    ctx = K.Context(0, "strict", async_=True)
    stream = torch.cuda.current_stream(0)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(fn, blocking=False):
        """ms per call: windows of at least WINDOW_MS, best of 7"""
        def host_window(reps):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3 / reps
        w = host_window if blocking else (lambda reps: window(fn, reps))
        one = w(3)
        reps = max(3, int(WINDOW_MS / max(one, 1e-4)) + 1)
        w(reps)
        return min(w(reps) for _ in range(7)), reps

    lines = []
    for gs in a.grids.split(","):
        nx, ny, nz = (int(q) for q in gs.split("x"))
        n = (nx, ny, nz)
        nbytes = (nx + 1) * (ny + 1) * (nz + 1)
        p = multi_params(nx, ny=ny, nz=nz)
        cyl = (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
        ax = [((np.arange(q) + 0.5 - c * q) / r) ** 2 for q, c, r in zip(n, (0.4, 0.5, 0.5), (45.0, 40.0, 35.0))]
        A = np.asfortranarray(1.0 - (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]))
        tri = S.from_isosurface(ISO.extract(ctx, K.from_numpy(A), 0.0))
        tri_d = torch.from_numpy(tri.reshape(-1)).cuda()
        del A
        for dt, tdt in (("f64", torch.float64), ("f32", torch.float32)):
            npdt = np.float64 if dt == "f64" else np.float32
            Cf, Vx, Vy, Vz = (K.from_numpy(np.random.default_rng(q).uniform(-1, 1, s).astype(npdt))
                              for q, s in enumerate(((nx, ny, nz), (nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))))
            bodies = {"cylinder": S.mask_of_cylinder(ctx, n, *cyl, dtype=tdt), "ellipsoid": S.voxelize(ctx, tri_d, *n)}
            spare = torch.empty_like(bodies["cylinder"])
            t_copy, _ = timed(lambda: spare.copy_(bodies["cylinder"]))
            t_cyl, _ = timed(lambda: K.set_cylinder(Cf, Vx, Vy, Vz, *cyl, ctx=ctx))
            for body, mask in bodies.items():
                t_set, reps = timed(lambda: K.set_solid(Cf, Vx, Vy, Vz, mask, ctx=ctx))
                t_mom, _ = timed(lambda: K.solid_momentum(Vx, Vy, Vz, mask, ctx=ctx), blocking=True)
                rec = dict(grid=gs, dtype=dt, body=body, mask_bytes=nbytes, set_solid_ms=t_set, calls_per_window=reps,
                           set_cylinder_ms=t_cyl, solid_momentum_ms=t_mom, copy_ms=t_copy,
                           mask_GBps=nbytes / t_set * 1e-6, copy_GBps=2 * nbytes / t_copy * 1e-6,
                           mask_rate_of_copy=(nbytes / t_set) / (2 * nbytes / t_copy),
                           masked=[int(q) for q in K.solid_momentum(Vx, Vy, Vz, mask, ctx=ctx)[1]])
                if body == "ellipsoid":
                    out = torch.empty_like(mask)
                    rec["n_tri"] = int(tri.shape[0])
                    rec["voxelize_ms"], _ = timed(lambda: K.voxelize(out, tri_d, n, ctx=ctx))
                    assert torch.equal(out, mask)
                    box = torch.from_numpy(S.box_mesh((0.2 * nx, 0.3 * ny, 0.25 * nz), (0.5 * nx, 0.7 * ny, 0.8 * nz)).reshape(-1)).cuda()
                    rec["voxelize_box12_ms"], _ = timed(lambda: K.voxelize(out, box, n, ctx=ctx))
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            del Cf, Vx, Vy, Vz, bodies, spare
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
