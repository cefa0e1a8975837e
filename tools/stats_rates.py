"""Cost of one statistics sample (ns3d_stats_accumulate) against the composition a user has without it — the same eleven updates
by PyTorch in-place elementwise ops on the device — and against a plain device copy that moves the same nominal bytes.

    python tools/stats_rates.py [--out profiles/stats_rates.jsonl] [--grids 512x512x512,255x153x153]

Event timing on the stream all three sides run on (the context is NS3D_ASYNC: the call only enqueues), best of 10 after 3 warm-ups,
the sides interleaved; fp64 STRICT and fp32 fields.  Nominal bytes per cell (stats.bytes_per_cell): 4 field reads + 11 accumulator
loads + 11 stores = 208 B (fp64) / 192 B (fp32 fields).  The composition forms u, v, w in fp64 scratch arrays (3 passes, after a
conversion pass per field for fp32: add into scratch, mul_(0.5) in place) and then updates the eleven sums with add_ / addcmul_ (11
passes): 3·(24+16) + 4·24 + 3·24 + 4·32 = 416 B per cell in fp64, twice the fused call's, in 17 launches.  The copy moves bytes/2 in and
bytes/2 out.  At 255×153×153 the 0.75 GB working set partly lives in the
256 MiB Infinity Cache (it is re-touched every repetition), so the rates there are not HBM figures.  One JSON line per grid and
element type.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12       # B/s, HBM3E of one MI355X


def measure(K, torch, stats, n, dtype, reps, warm):
    nx, ny, nz = n
    ctx = K.Context(0, "strict", async_=True)
    mk = lambda *s: K.zeros(s, dtype).uniform_(-1.0, 1.0)
    Vx, Vy, Vz, Pr = mk(nx + 1, ny, nz), mk(nx, ny + 1, nz), mk(nx, ny, nz + 1), mk(nx, ny, nz)
    S = K.zeros((nx, ny, nz * 11), torch.float64)
    S2 = K.zeros((nx, ny, nz * 11), torch.float64)
    B = [S2[:, :, q * nz:(q + 1) * nz] for q in range(11)]
    u, v, w = (K.zeros((nx, ny, nz), torch.float64) for _ in range(3))
    f64 = dtype == torch.float64
    stage = None if f64 else [K.zeros(tuple(t.shape), torch.float64) for t in (Vx, Vy, Vz, Pr)]
    cells = nx * ny * nz
    nbytes = stats.bytes_per_cell(dtype, True) * cells
    src, dst = torch.zeros(nbytes // 16, dtype=torch.float64, device="cuda"), torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
    wgt = 1.0

    def fused():
        K.stats_accumulate(S, Vx, Vy, Vz, Pr, wgt, ctx=ctx)

    def composed():
        X, Y, Z, P = (Vx, Vy, Vz, Pr)
        if not f64:
            for d, s in zip(stage, (Vx, Vy, Vz, Pr)):
                d.copy_(s)
            X, Y, Z, P = stage
        torch.add(X[:-1], X[1:], out=u).mul_(0.5)
        torch.add(Y[:, :-1], Y[:, 1:], out=v).mul_(0.5)
        torch.add(Z[:, :, :-1], Z[:, :, 1:], out=w).mul_(0.5)
        for q, t in enumerate((u, v, w, P)):
            B[q].add_(t, alpha=wgt)
        for q, (a, b) in enumerate(((u, u), (v, v), (w, w), (u, v), (u, w), (v, w), (P, P))):
            B[4 + q].addcmul_(a, b, value=wgt)

    def copy():
        dst.copy_(src)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    sides = (("fused", fused), ("composed", composed), ("copy", copy))
    for _ in range(warm):
        for _, fn in sides:
            timed(fn)
    K.stats_reset(S, n, ctx=ctx)
    S2.zero_()
    ev = {k: [] for k, _ in sides}
    for _ in range(reps):
        for name, fn in sides:
            ev[name].append(timed(fn))
    ctx.sync()
    # both sides hold `reps` samples of the same fields: they agree to rounding (the composition's mul_(0.5) and addcmul_ round elsewhere)
    assert torch.allclose(S, S2, rtol=1e-12, atol=1e-12 * reps), "the two sides disagree"
    best = {k: min(t) for k, t in ev.items()}
    rate = lambda ms: nbytes / (ms * 1e-3)
    out = dict(kernel="ns3d_stats_accumulate_%s" % ("f64" if f64 else "f32"), grid=[nx, ny, nz], mode="strict", reps=reps, warmups=warm,
               nominal_bytes_per_cell=stats.bytes_per_cell(dtype, True), nominal_bytes=nbytes,
               fused_ms=best["fused"], composed_ms=best["composed"], copy_ms=best["copy"],
               fused_ms_all=ev["fused"], composed_ms_all=ev["composed"], copy_ms_all=ev["copy"],
               fused_TBps=rate(best["fused"]) / 1e12, copy_TBps=rate(best["copy"]) / 1e12,
               fused_fraction_of_copy_rate=best["copy"] / best["fused"], fused_fraction_of_8TBps=rate(best["fused"]) / PEAK,
               speedup_over_composition=best["composed"] / best["fused"], fused_beats_composition=best["fused"] < best["composed"])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_rates.jsonl"))
    ap.add_argument("--grids", default="512x512x512,255x153x153")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd import stats
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                rec = measure(K, torch, stats, tuple(int(q) for q in gs.split("x")), dtype, a.reps, a.warmup)
                print(json.dumps(rec))
                fh.write(json.dumps(rec) + "\n")
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
