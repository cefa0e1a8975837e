"""Cost of the fused flow monitor (ns3d_diagnostics_f64) against the composition that gives max|V| and max|∇V| without it:
ns3d_update_divV into a scratch array, then ns3d_max_abs on it and on Vx, Vy, Vz.

    python tools/diagnostics_rates.py [--out profiles/diagnostics_rates.jsonl] [--grids 512x512x512,255x153x153]

Event timing, best of 10 after 3 warm-ups, the two sides interleaved.  The events are recorded on the stream the context
launches on, but around BLOCKING library calls: what they measure is host-synchronised time per call, read-backs and launch gaps
included (wall-clock is reported beside them and differs by microseconds) — the cost a driver pays, not kernel time.  The
fraction of 8 TB/s is nominal bytes over that time; a working set near the 256 MB Infinity Cache (255×153×153: 239 MB, re-read every
repetition) makes it a cache figure, not an HBM one.  Bytes per cell are the arrays each side must move
once: 5 × 8 for the monitor, 3 reads + 1 write + 4 reads for the composition.  One JSON line per grid.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12       # B/s, HBM3E of one MI355X


def measure(K, torch, n, mode, reps, warm):
    nx, ny, nz = n
    ctx = K.Context(0, mode)
    mk = lambda *s: K.zeros(s).uniform_(-1.0, 1.0)
    Vx, Vy, Vz, Pr, Cf, dv = mk(nx + 1, ny, nz), mk(nx, ny + 1, nz), mk(nx, ny, nz + 1), mk(nx, ny, nz), mk(nx, ny, nz), K.zeros((nx, ny, nz))
    dx, dy, dz = 1.0 / nx, 0.6 / ny, 0.6 / nz
    lx, ly = 1.0, 0.6
    cyl = (0.05 ** 2, 0.05 ** 2, -0.4, 0.0, 0.0, 1.0, -(lx - dx) / 2, -(ly - dy) / 2, 0.0, lx, ly, 0.6, dx, dy, dz)
    dp = K.diag_params(nx, ny, nz, dx, dy, dz, 1000.0, cylinder=cyl)

    def fused():
        return K.diagnostics(Vx, Vy, Vz, Pr, Cf, dp, ctx=ctx)

    def composed():
        K.update_divV(dv, Vx, Vy, Vz, dx, dy, dz, ctx=ctx)
        return [K.max_abs(a, ctx=ctx) for a in (dv, Vx, Vy, Vz)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out

    for _ in range(warm):
        timed(fused); timed(composed)
    ev = {"fused": [], "composed": []}
    wall = {"fused": [], "composed": []}
    for _ in range(reps):
        for name, fn in (("fused", fused), ("composed", composed)):
            e, w, out = timed(fn)
            ev[name].append(e); wall[name].append(w)
    rec, comp = fused(), composed()
    assert rec.div_max == comp[0] and rec.vmax == tuple(comp[1:]), "the two sides disagree"
    cells = nx * ny * nz
    best = {k: min(v) for k, v in ev.items()}
    out = dict(kernel="ns3d_diagnostics_f64", grid=[nx, ny, nz], mode=mode, arith_build=ctx.arith_build(dx, dy, dz), reps=reps, warmups=warm,
               fused_ms=best["fused"], composed_ms=best["composed"], fused_wall_ms=min(wall["fused"]), composed_wall_ms=min(wall["composed"]),
               fused_ms_all=ev["fused"], composed_ms_all=ev["composed"], fused_bytes_per_cell=40, composed_bytes_per_cell=64,
               fused_fraction_of_8TBps=40.0 * cells / (best["fused"] * 1e-3) / PEAK,
               composed_fraction_of_8TBps=64.0 * cells / (best["composed"] * 1e-3) / PEAK,
               speedup=best["composed"] / best["fused"], fused_beats_composition=best["fused"] < best["composed"])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics_rates.jsonl"))
    ap.add_argument("--grids", default="512x512x512,255x153x153")
    ap.add_argument("--mode", default="strict")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            rec = measure(K, torch, tuple(int(q) for q in gs.split("x")), a.mode, a.reps, a.warmup)
            print(json.dumps(rec))
            fh.write(json.dumps(rec) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
