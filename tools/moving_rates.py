"""Times of the moving-obstacle calls next to what they stand beside.

    python tools/moving_rates.py [--out profiles/moving_rates.jsonl] [--rounds 9] [--skip-step]

Three measurements on one device, each with device events on the stream the NS3D_ASYNC context launches on, the two sides ALTERNATING
within every round in one process, reported as the median with the minimum and maximum over the rounds:
  masking    ns3d_set_solid_moving against ns3d_set_solid on the same mask — a sphere mesh of 35 cells radius — at 512³ and
             255×153×153, both element types; a window of back-to-back calls lasting at least 5 ms per side and round.
  remeshing  ns3d_mesh_transform + ns3d_voxelize, what a moving mesh costs per step, for spheres of about 10³ and 10⁵ triangles at
             255×153×153, against ns3d_voxelize alone.
  step       one ns3d_time_step of the multi script at 255×153×153, fp64, with the direct pressure solve: a static sphere of 10⁵
             triangles (ns3d_set_obstacle) against the same sphere translating and turning — per step ns3d_mesh_transform,
             ns3d_voxelize into the registered mask, ns3d_set_obstacle_motion, as the drivers issue them —, each as
             (t(12 steps) − t(2 steps))/10 between two events on the context's stream, from the script's initial state on arrays
             allocated outside the interval.  With the direct solve every step ends in a synchronisation, so the interval is also
             the host's.  The record says whether the fields are finite after the 12 steps.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_MS = 5.0


def sphere(centre, radius, nlat, nlon):
    """a closed latitude-longitude sphere, (2·nlon·(nlat − 1), 3, 3): index space"""
    import numpy as np
    th = np.linspace(0.0, np.pi, nlat + 1)
    ph = np.linspace(0.0, 2 * np.pi, nlon, endpoint=False)
    P = lambda i, j: np.array([np.sin(th[i]) * np.cos(ph[j % nlon]), np.sin(th[i]) * np.sin(ph[j % nlon]), np.cos(th[i])])
    tri = []
    for i in range(nlat):
        for j in range(nlon):
            a, b, c, d = P(i, j), P(i, j + 1), P(i + 1, j), P(i + 1, j + 1)
            if i > 0:
                tri.append((a, c, b))
            if i < nlat - 1:
                tri.append((b, c, d))
    return np.asarray(centre, dtype=np.float64) + radius * np.array(tri)


def spread(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moving_rates.jsonl"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "moving_rates needs a GPU: there is nothing to time without one"
    from navierstokes3d_amd import kernels as K, solid as S
    from navierstokes3d_amd.params import multi_params

    ctx = K.Context(0, "strict", async_=True)
    stream = torch.cuda.current_stream(0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(sides):
        """{name: [ms per call of each round]} — per round one window of every side, in turn"""
        reps = {k: max(3, int(WINDOW_MS / max(window(fn, 3), 1e-4)) + 1) for k, fn in sides.items()}
        for k, fn in sides.items():
            window(fn, reps[k])
        out = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():
                out[k].append(window(fn, reps[k]))
        return out

    motion = (0.3, -0.2, 0.1, 0.5, -0.4, 2.0)
    # ---- masking
    for gs in ("512x512x512", "255x153x153"):
        nx, ny, nz = n = tuple(int(q) for q in gs.split("x"))
        centre = (0.4 * nx, 0.5 * ny, 0.5 * nz)
        mask = S.voxelize(ctx, sphere(centre, 35.0, 60, 120), *n)
        p = multi_params(nx, ny=ny, nz=nz)
        for dt in ("f64", "f32"):
            npdt = np.float64 if dt == "f64" else np.float32
            Cf, Vx, Vy, Vz = (K.from_numpy(np.random.default_rng(q).uniform(-1, 1, s).astype(npdt))
                              for q, s in enumerate(((nx, ny, nz), (nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1))))
            t = alternate({"set_solid": lambda: K.set_solid(Cf, Vx, Vy, Vz, mask, ctx=ctx),
                           "set_solid_moving": lambda: K.set_solid_moving(Cf, Vx, Vy, Vz, mask, motion + centre, p.dx, p.dy, p.dz, ctx=ctx)})
            emit(dict(what="masking", grid=gs, dtype=dt, mask_bytes=(nx + 1) * (ny + 1) * (nz + 1),
                      masked=[int(q) for q in K.solid_momentum(Vx, Vy, Vz, mask, ctx=ctx)[1]], rounds=a.rounds,
                      set_solid_ms=spread(t["set_solid"]), set_solid_moving_ms=spread(t["set_solid_moving"]),
                      ratio=statistics.median(t["set_solid_moving"]) / statistics.median(t["set_solid"])))
            del Cf, Vx, Vy, Vz
        del mask
    # ---- remeshing
    nx, ny, nz = n = (255, 153, 153)
    p = multi_params(nx)
    d = (p.dx, p.dy, p.dz)
    centre = np.array([0.4 * nx, 0.5 * ny, 0.5 * nz])
    for nlat, nlon in ((17, 32), (158, 320)):
        tri = torch.from_numpy(sphere(centre, 35.0, nlat, nlon).reshape(-1)).cuda()
        posed, out = torch.empty_like(tri), torch.empty((nx + 1) * (ny + 1) * (nz + 1), dtype=torch.uint8, device="cuda")
        R, shift = S.rotation((0.2, -0.1, 1.0), 0.3), np.array([0.7, -0.4, 0.2])

        def remesh():
            K.mesh_transform(posed, tri, R, centre, shift, d, ctx=ctx)
            K.voxelize(out, posed, n, ctx=ctx)
        t = alternate({"voxelize": lambda: K.voxelize(out, tri, n, ctx=ctx), "remesh": remesh,
                       "transform": lambda: K.mesh_transform(posed, tri, R, centre, shift, d, ctx=ctx)})
        emit(dict(what="remeshing", grid="255x153x153", n_tri=tri.numel() // 9, rounds=a.rounds, voxelize_ms=spread(t["voxelize"]),
                  mesh_transform_ms=spread(t["transform"]), transform_and_voxelize_ms=spread(t["remesh"]),
                  ratio=statistics.median(t["remesh"]) / statistics.median(t["voxelize"])))
        del tri, posed, out
    # ---- the step
    if not a.skip_step:
        from navierstokes3d_amd import lib as L
        from navierstokes3d_amd.driver import _alloc, _step_params
        body = sphere(centre, 35.0, 158, 320)
        tri0 = torch.from_numpy(body.reshape(-1)).cuda()
        posed = torch.empty_like(tri0)
        mask0 = S.voxelize(ctx, tri0, *n)
        mask = torch.empty_like(mask0)
        pose = S.rigid_motion(velocity=(0.05 * p.dx / p.dt, 0.02 * p.dy / p.dt, 0.0), omega=(0.0, 0.0, 0.02 / p.dt), centre=tuple(centre),
                              spacing=d)
        sp = _step_params(L.NS3D_BC_MULTI, p, p.niter, False, "direct")
        state = {}

        def run(nt, moving):
            """ms of nt ns3d_time_step calls from the script's initial state, between two events on the context's stream; under
            motion each step first poses the mesh, re-voxelizes into the registered mask and sets the knob, as the drivers do"""
            f = _alloc(nx, ny, nz, torch.float64, torch.device("cuda", 0))
            f.Vy[0, :, :] = p.vin
            mask.copy_(mask0)
            K.set_solid(f.C, f.Vx, f.Vy, f.Vz, mask, ctx=ctx)
            ctx.set_obstacle(mask)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.sync()
            e0.record(stream)
            try:
                for s in range(1, nt + 1):
                    if moving:
                        R, shift, U, omega, c = pose(s * p.dt)
                        K.mesh_transform(posed, tri0, R, c - shift, shift, d, ctx=ctx)
                        K.voxelize(mask, posed, n, ctx=ctx)
                        ctx.set_obstacle_motion(tuple(U) + tuple(omega) + tuple(c))
                    K.time_step(f, sp, ctx=ctx)
                e1.record(stream)
                e1.synchronize()
            finally:
                ctx.set_obstacle_motion(None); ctx.set_obstacle(None)
            state[moving] = dict(finite=bool(all(torch.isfinite(getattr(f, k)).all() for k in ("Vx", "Vy", "Vz", "Pr", "C"))),
                                 vmax=float(max(getattr(f, k).abs().max() for k in ("Vx", "Vy", "Vz"))))
            return e0.elapsed_time(e1)
        run(2, False); run(2, True)         # modules, the direct solve's plan and eigenbases
        per = {"static": [], "moving": []}
        for _ in range(min(a.rounds, 5)):
            for k, m in (("static", False), ("moving", True)):
                per[k].append((run(12, m) - run(2, m)) / 10.0)
        emit(dict(what="step", grid="255x153x153", pressure="direct", dtype="f64", n_tri=int(body.shape[0]), rounds=min(a.rounds, 5),
                  static_ms=spread(per["static"]), moving_ms=spread(per["moving"]), after_12_steps=dict(static=state[False], moving=state[True]),
                  ratio=statistics.median(per["moving"]) / statistics.median(per["static"])))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
