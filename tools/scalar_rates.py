"""Cost of ns3d_scalar_step against the two calls it fuses (ns3d_scalar_diffuse, then ns3d_buoyancy) and against a plain device copy
of one array in the same run.

    python tools/scalar_rates.py [--out profiles/scalar_rates.jsonl] [--grids 512x512x512,255x153x153]

Device events on the stream every side runs on (the context is NS3D_ASYNC: a call only enqueues); seven rounds of five calls, the
sides alternating inside every round in one process, after one warm-up round; the figure of a side is the median over the rounds of
the per-call time, recorded with the smallest and the largest round.  fp64 and fp32, STRICT and FAST, with and without mu_e.  One
JSON line per grid, element type, mode and mu_e.

Nominal elements per cell: the fused call reads C and mu_e, reads and writes Vz and writes C_out — 5 (4 without mu_e); the two calls
in sequence read C twice — 7 (6).  `share_of_copy` is the copy's time scaled to the fused call's nominal bytes over the fused call's
time, the figure profiles/sgs_rates.jsonl records for ns3d_eddy_viscosity (4 elements per cell in a similar kernel shape);
`eddy_viscosity_share` repeats that figure from that file for the same grid, element type and mode where the file is present.
`fused_no_slower` — the fused call's median does not exceed the two calls' — is the bar the fused entry point exists by; a false
is an open item.  At 255×153×153 the working set sits partly in the 256 MiB Infinity Cache, so the rates there are not HBM figures.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def eddy_share(n, dt, mode):
    try:
        for line in open(os.path.join(ROOT, "profiles", "sgs_rates.jsonl")):
            r = json.loads(line)
            if r.get("call") == "eddy_viscosity" and r["grid"] == list(n) and r["dtype"] == dt and r["mode"] == mode:
                return r["share_of_copy"]
    except OSError:
        pass
    return None


def measure(K, torch, n, dtype, mode, var, rounds, reps, fh):
    nx, ny, nz = n
    ctx = K.Context(0, mode, async_=True)
    dt = "f64" if dtype == torch.float64 else "f32"
    d = (1.0 / (nx + 1), 1.0 / (ny + 1), 1.0 / (nz + 1))        # no power of two at 512: the exact-division build, as at 255×153×153
    mu, step = 1e-3, 1e-3
    sgs = 1.0 / 0.7
    kappa = 0.2 / (step * sum(1.0 / q ** 2 for q in d))
    Cf = K.zeros((nx, ny, nz), dtype).uniform_(0.0, 1.0)
    mu_e = K.zeros((nx, ny, nz), dtype).uniform_(mu, 2 * mu) if var else None
    Vz = K.zeros((nx, ny, nz + 1), dtype).uniform_(-1.0, 1.0)
    out, dst = K.zeros((nx, ny, nz), dtype), K.zeros((nx, ny, nz), dtype)
    bg, c_ref = 1e-3, 0.5           # small: Vz is updated in place hundreds of times
    cells = nx * ny * nz

    def two():
        K.scalar_diffuse(out, Cf, mu_e, kappa, sgs, mu, step, *d, ctx=ctx)
        K.buoyancy(Vz, Cf, bg, c_ref, step, ctx=ctx)
    sides = [("fused", lambda: K.scalar_step(out, Vz, Cf, mu_e, kappa, sgs, mu, bg, c_ref, step, *d, ctx=ctx)), ("two_calls", two),
             ("diffuse", lambda: K.scalar_diffuse(out, Cf, mu_e, kappa, sgs, mu, step, *d, ctx=ctx)),
             ("buoyancy", lambda: K.buoyancy(Vz, Cf, bg, c_ref, step, ctx=ctx)), ("copy", lambda: K.copy(dst, Cf, ctx=ctx))]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for _, fn in sides:             # the warm-up round
        timed(fn)
    ev = {k: [] for k, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            ev[name].append(timed(fn))
    ctx.sync()
    med = {k: statistics.median(v) for k, v in ev.items()}
    esz = 8 if dtype == torch.float64 else 4
    el_fused, el_two = (5, 7) if var else (4, 6)
    rate = lambda k, els: round(els * esz * cells / (med[k] * 1e-3) / 1e9, 1)
    rec = dict(call="scalar_step", grid=[nx, ny, nz], dtype=dt, mode=mode, build=ctx.arith_build(*d), mu_e=bool(var), rounds=rounds, reps=reps,
               elements_per_cell=el_fused, elements_per_cell_two_calls=el_two)
    for k in ev:
        rec[k + "_ms"] = round(med[k], 4)
        rec[k + "_ms_min"], rec[k + "_ms_max"] = round(min(ev[k]), 4), round(max(ev[k]), 4)
    rec.update(fused_gbs=rate("fused", el_fused), two_calls_gbs=rate("two_calls", el_two), copy_gbs=rate("copy", 2),
               ratio_two_over_fused=round(med["two_calls"] / med["fused"], 3), fused_no_slower=bool(med["fused"] <= med["two_calls"]),
               share_of_copy=round(med["copy"] * (el_fused / 2.0) / med["fused"], 3), eddy_viscosity_share=eddy_share(n, dt, mode))
    print(json.dumps(rec))
    fh.write(json.dumps(rec) + "\n")
    fh.flush()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_rates.jsonl"))
    ap.add_argument("--grids", default="512x512x512,255x153x153")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                for mode in ("strict", "fast"):
                    for var in (True, False):
                        measure(K, torch, tuple(int(q) for q in gs.split("x")), dtype, mode, var, a.rounds, a.reps, fh)
                        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
