"""Cost of an isosurface (ns3d_isosurface: count, scan, emit on the device) against what a user does without it — copying the field to
the host — and against a device copy of the field, the floor for reading it once.

    python tools/isosurface_rates.py [--out profiles/isosurface_rates.jsonl] [--grids 255x153x153,512x512x512]

The field is the Q-criterion (ns3d_vortex) of a synthetic vortex street: two staggered rows of Gaussian vortices of alternating sign
along x in a uniform stream, plus a weak seeded perturbation so that Q near zero is rough.  Two levels per grid and element type: a
sparse surface (0.2 of the maximum of Q: the vortex cores) and a dense one (0.001 of it: the perturbed background).  Per case: the
count-only call (one read of A, 4 B per 64 cubes written, the scan, the read-back of the total), the full call (count, scan and emit
into a buffer of exactly n triangles, uncoloured), n, the bytes written, a device-to-host copy of A into pinned memory and a
device-to-device copy of A.  The calls block for their read-back, so each is timed by a host clock around the call with the device
idle before it; the copies by a host clock around copy + synchronise.  Best of `reps` after `warmup` repetitions, every side in one
process, interleaved; all times are recorded.  At 255×153×153 the field (48 MB in fp64) fits the 256 MiB Infinity Cache and is
re-read every repetition: the rates there are not HBM figures.  One JSON line per case; nothing is judged.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vortex_street_q(K, torch, n, dtype, ctx):
    nx, ny, nz = n
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def field(sx, sy, sz, ox, oy, comp):
        x = (torch.arange(sx, device=dev, dtype=torch.float64) + ox) / nx
        y = (torch.arange(sy, device=dev, dtype=torch.float64) + oy) / ny - 0.5
        z = torch.arange(sz, device=dev, dtype=torch.float64) / nz
        X, Y, Z = x[:, None, None], y[None, :, None], z[None, None, :]
        out = torch.zeros((sx, sy, sz), device=dev, dtype=torch.float64)
        for q in range(8):                                  # vortex q: centre, sign, core radius; bent slightly along z
            cx, cy, s, r = 0.1 + 0.11 * q, 0.08 * (1 if q % 2 else -1), (1.0 if q % 2 else -1.0), 0.035
            dxv, dyv = X - cx - 0.02 * torch.sin(6.283 * Z), Y - cy
            w = s * torch.exp(-(dxv * dxv + dyv * dyv) / (r * r))
            out += (-dyv if comp == 0 else dxv) * w / r
        return out

    Vx = field(nx + 1, ny, nz, 0.0, 0.5, 0) + 1.0
    Vy = field(nx, ny + 1, nz, 0.5, 0.0, 1)
    Vz = torch.zeros((nx, ny, nz + 1), device=dev, dtype=torch.float64)
    V = []
    for t in (Vx, Vy, Vz):
        t = t + 0.002 * (torch.rand(t.shape, device=dev, dtype=torch.float64, generator=g) - 0.5)
        c = K.zeros(tuple(t.shape), dtype)
        c.copy_(t)
        V.append(c)
    Q = K.zeros(n, dtype)
    K.vortex(*V, 1.0 / nx, 1.0 / ny, 1.0 / nz, Q=Q, ctx=ctx)
    ctx.sync()
    return Q


def best_of(fn, torch, reps, warm):
    ts = []
    for q in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if q >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def measure(K, torch, n, dtype, reps, warm):
    ctx = K.Context(0, "strict", async_=True)
    Q = vortex_street_q(K, torch, n, dtype, ctx)
    qmax = float(Q.max())
    esize = Q.element_size()
    field_bytes = Q.numel() * esize
    box = (1, 1, 1, n[0] - 2, n[1] - 2, n[2] - 2)           # the outermost cells of Q are +0.0 by contract
    flat = Q.permute(2, 1, 0).contiguous().view(-1)         # the same memory order, as a flat tensor for the copies
    host = torch.empty(flat.shape, dtype=flat.dtype).pin_memory()
    dst = torch.empty_like(flat)
    recs = []
    for name, level in (("sparse", 0.2 * qmax), ("dense", 0.001 * qmax)):
        count = lambda: K.isosurface(Q, level, box=box, ctx=ctx)
        ntri = count()
        tri = torch.empty(9 * ntri, dtype=torch.float64, device="cuda")
        sides = dict(count=count, full=lambda: K.isosurface(Q, level, box=box, tri=tri, cap=ntri, ctx=ctx),
                     d2h=lambda: host.copy_(flat, non_blocking=True), d2d=lambda: dst.copy_(flat))
        ev = {k: [] for k in sides}
        for q in range(warm + reps):                        # interleaved
            for k, fn in sides.items():
                t = best_of(fn, torch, 1, 0)
                if q >= warm:
                    ev[k] += t
        best = {k: min(v) for k, v in ev.items()}
        cubes = (n[0] - 3) * (n[1] - 3) * (n[2] - 3)
        segs = ((n[0] - 3 + 63) // 64) * (n[1] - 3) * (n[2] - 3)
        model = field_bytes + 4 * segs                      # the counting pass: one read of A plus 4 B per row segment
        recs.append(dict(kernel="ns3d_isosurface_%s" % ("f64" if esize == 8 else "f32"), grid=list(n), surface=name, level=level,
                         q_max=qmax, cubes=cubes, n_triangles=ntri, bytes_written=72 * ntri, field_bytes=field_bytes,
                         count_model_bytes=model, reps=reps, warmups=warm,
                         count_ms=best["count"], full_ms=best["full"], d2h_pinned_ms=best["d2h"], d2d_ms=best["d2d"],
                         count_ms_all=ev["count"], full_ms_all=ev["full"], d2h_pinned_ms_all=ev["d2h"], d2d_ms_all=ev["d2d"],
                         count_call_GBps=model / best["count"] / 1e6, d2d_read_GBps=field_bytes / best["d2d"] / 1e6,
                         count_call_fraction_of_copy_read_rate=(model / best["count"]) / (field_bytes / best["d2d"]),
                         full_speedup_over_d2h=best["d2h"] / best["full"]))
        del tri
        torch.cuda.empty_cache()
    ctx.close()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface_rates.jsonl"))
    ap.add_argument("--grids", default="255x153x153,512x512x512")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                for rec in measure(K, torch, tuple(int(q) for q in gs.split("x")), dtype, a.reps, a.warmup):
                    print(json.dumps(rec))
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
