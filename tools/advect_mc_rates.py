"""Cost of the limited MacCormack advection (ns3d_advect_mc: stage 1 = ns3d_copy_advect(faithful = 0), then stage 2 =
ns3d_advect_correct) against the first-order step it stands beside, ns3d_copy_advect.

    python tools/advect_mc_rates.py [--out profiles/advect_mc_rates.jsonl] [--grids 512x512x512,255x153x153]

Event timing on the stream the calls run on (the context is NS3D_ASYNC: a call only enqueues), best of 10 after 3 warm-ups, the sides
interleaved in one process; fp64 and fp32, STRICT.  Fields: U(−1, 1) velocities and scalar, dt = 0.9 × the smallest spacing, so
every departure point lies within one cell and inside the LDS window.  Sides: copy_advect in the reference's form (faithful = 1)
and in the corrected form that is stage 1 (faithful = 0); advect_correct in its windowed form and as the global gather
(NS3D_ADVECT_GLOBAL=1); advect_mc, the whole call.  Nominal bytes per cell: copy_advect reads 4 and writes 4 arrays (8), stage 2
reads 8 and writes 4 (12), the whole call 20 — of the element type.  At 255×153×153 the working set sits partly in the 256 MiB Infinity
Cache — it is re-touched every repetition — so the rates there are not HBM figures.  One JSON line per grid and element type; the
ratio mc_over_copy_advect is recorded, not judged.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(K, torch, n, dtype, reps, warm):
    nx, ny, nz = n
    ctx = K.Context(0, "strict", async_=True)
    shapes = ((nx + 1, ny, nz), (nx, ny + 1, nz), (nx, ny, nz + 1), (nx, ny, nz))
    old = [K.zeros(s, dtype).uniform_(-1.0, 1.0) for s in shapes]
    new = [K.zeros(s, dtype) for s in shapes]
    hat = [K.zeros(s, dtype) for s in shapes]
    d = (1.0 / nx, 0.6 / ny, 0.7 / nz)
    dt = 0.9 * min(d)
    trio = [t for q in range(4) for t in (new[q], old[q], hat[q])]
    pairs = [t for q in range(4) for t in (new[q], old[q])]

    def form(glob):
        if glob:
            os.environ["NS3D_ADVECT_GLOBAL"] = "1"                   # read per call
        else:
            os.environ.pop("NS3D_ADVECT_GLOBAL", None)

    def copy_advect(faithful):
        def run():
            form(False)
            K.copy_advect(*pairs, dt, *d, faithful, ctx=ctx)
        return run

    def correct(glob):
        def run():
            form(glob)
            K.advect_correct(*trio, dt, *d, ctx=ctx)
            form(False)
        return run

    def mc():
        form(False)
        K.advect_mc(*trio, dt, *d, ctx=ctx)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    # advect_mc first: it leaves stage 1 in `hat`, which the advect_correct sides then read
    sides = (("advect_mc", mc), ("copy_advect_faithful", copy_advect(True)), ("copy_advect", copy_advect(False)),
             ("advect_correct", correct(False)), ("advect_correct_global", correct(True)))
    for _ in range(warm):
        for _, fn in sides:
            timed(fn)
    ev = {k: [] for k, _ in sides}
    for _ in range(reps):
        for name, fn in sides:
            ev[name].append(timed(fn))
    ctx.sync()
    best = {k: min(t) for k, t in ev.items()}
    f64 = dtype == torch.float64
    esize, cells = (8 if f64 else 4), nx * ny * nz
    rate = lambda arrays, ms: arrays * esize * cells / (ms * 1e-3) / 1e12
    out = dict(kernel="ns3d_advect_mc_%s" % ("f64" if f64 else "f32"), grid=[nx, ny, nz], mode="strict", arith_build=ctx.arith_build(*d),
               reps=reps, warmups=warm, cfl=0.9, element_bytes=esize,
               copy_advect_faithful_ms=best["copy_advect_faithful"], copy_advect_ms=best["copy_advect"],
               advect_correct_ms=best["advect_correct"], advect_correct_global_ms=best["advect_correct_global"], advect_mc_ms=best["advect_mc"],
               copy_advect_TBps=rate(8, best["copy_advect"]), advect_correct_TBps=rate(12, best["advect_correct"]),
               advect_mc_TBps=rate(20, best["advect_mc"]),
               mc_over_copy_advect=best["advect_mc"] / best["copy_advect"],
               mc_over_copy_advect_faithful=best["advect_mc"] / best["copy_advect_faithful"],
               correct_over_copy_advect=best["advect_correct"] / best["copy_advect"],
               windowed_correct_beats_global=best["advect_correct"] < best["advect_correct_global"],
               **{k + "_ms_all": v for k, v in ev.items()})
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advect_mc_rates.jsonl"))
    ap.add_argument("--grids", default="512x512x512,255x153x153")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                rec = measure(K, torch, tuple(int(q) for q in gs.split("x")), dtype, a.reps, a.warmup)
                print(json.dumps(rec))
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
