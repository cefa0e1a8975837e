"""Rate of one tracer step (ns3d_tracers_advance: explicit midpoint through the frozen staggered velocity field) against the
composition a user has without it — the same step as PyTorch index arithmetic plus `take` on the device — and of the same particle
set in lattice order against the same set randomly permuted.

    python tools/tracers_rates.py [--out profiles/tracers_rates.jsonl] [--grids 255x153x153,512x512x512] [--counts 20,24]

Event timing on the stream every side runs on (the context is NS3D_ASYNC: the call only enqueues), best of 10 after 3 warm-ups, the
sides interleaved in one process; fp64 and fp32 fields, positions fp64.  Before every timed run the particle arrays are restored
(outside the timed window), so every repetition does the same work.  The particles sit on a regular lattice over the box, x
fastest like the cells ("lattice": neighbours in memory are neighbours in space) or the same points in a random order
("permuted"); the fields are U(−1,1), the Courant factors 0.4, 0.36, 0.32.  The composition keeps the header's expression op by op
with preallocated temporaries and counts its own launches; both sides must agree to rounding.  One JSON line per grid, element type
and N: particles/s of the library call for both orders, the composition's time and launch count, the ratios, and the
`fused_beats_composition` flag, which must be true on every line.  `fits_infinity_cache` says whether fields plus particle arrays
stay below the 256 MiB Infinity Cache: those lines re-touch a cached working set every repetition and are NOT HBM figures.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INFINITY_CACHE = 256 << 20
COURANT = (0.4, 0.36, 0.32)


class Composition:
    """one step, op by op, on preallocated arrays of N elements; counts launches"""

    def __init__(self, torch, shape, N, dtype, device="cuda"):
        self.T, self.shape, self.N = torch, shape, N
        d = lambda: torch.empty(N, dtype=torch.float64, device=device)
        l = lambda: torch.empty(N, dtype=torch.int64, device=device)
        self.c, self.fl, self.t, self.omt = [d() for _ in range(3)], d(), [d() for _ in range(3)], [d() for _ in range(3)]
        self.i, self.base, self.idx = [l() for _ in range(3)], l(), l()
        self.raw = torch.empty(N, dtype=dtype, device=device)
        self.a = [d() for _ in range(8)]
        self.x, self.y = d(), d()
        self.v = [d() for _ in range(3)]
        self.Xm = torch.empty((3, N), dtype=torch.float64, device=device)
        self.Xn = torch.empty((3, N), dtype=torch.float64, device=device)
        self.m = [torch.empty(N, dtype=torch.bool, device=device) for _ in range(4)]      # active | two scratch masks | inside after
        self.launches = 0

    def op(self, fn, *args, **kw):
        self.launches += 1
        return fn(*args, **kw)

    def lerp(self, a, b, q, out):
        T = self.T
        self.op(T.mul, b, self.t[q], out=self.x)
        self.op(T.mul, a, self.omt[q], out=self.y)
        return self.op(T.add, self.x, self.y, out=out)

    def interp(self, A, stag, P, out):
        T, a = self.T, self.a
        ext = A.shape
        flat = A.permute(2, 1, 0).reshape(-1)              # column-major storage: a view, no launch
        for q in range(3):
            self.op(T.sub, P[q], 0.0 if stag[q] else 0.5, out=self.c[q])
            self.op(self.c[q].clamp_, 0.0, ext[q] - 1.0)
            self.op(T.floor, self.c[q], out=self.fl)
            self.op(self.fl.clamp_, max=ext[q] - 2.0)
            self.op(T.sub, self.c[q], self.fl, out=self.t[q])
            self.op(T.neg, self.t[q], out=self.omt[q])
            self.op(self.omt[q].add_, 1.0)
            self.op(self.i[q].copy_, self.fl)
        self.op(T.mul, self.i[2], ext[1], out=self.base)
        self.op(self.base.add_, self.i[1])
        self.op(self.base.mul_, ext[0])
        self.op(self.base.add_, self.i[0])
        for k in range(8):
            off = (k & 1) + ext[0] * ((k >> 1) & 1) + ext[0] * ext[1] * (k >> 2)
            self.op(T.add, self.base, off, out=self.idx)
            if flat.dtype == T.float64:
                self.op(T.take, flat, self.idx, out=a[k])
            else:
                self.op(T.take, flat, self.idx, out=self.raw)
                self.op(a[k].copy_, self.raw)
        self.lerp(a[0], a[1], 0, a[0]); self.lerp(a[4], a[5], 0, a[4]); self.lerp(a[2], a[3], 0, a[2]); self.lerp(a[6], a[7], 0, a[6])
        self.lerp(a[0], a[2], 1, a[0]); self.lerp(a[4], a[6], 1, a[4])
        return self.lerp(a[0], a[4], 2, out)

    def velocity(self, V, P):
        for q, stag in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            self.interp(V[q], stag, P, self.v[q])

    def inside(self, P, out):
        T = self.T
        for q in range(3):
            self.op(T.ge, P[q], 0.0, out=self.m[1])
            self.op(T.le, P[q], float(self.shape[q]), out=self.m[2])
            self.op(T.logical_and, self.m[1], self.m[2], out=self.m[1])
            if q == 0:
                self.op(out.copy_, self.m[1])
            else:
                self.op(T.logical_and, out, self.m[1], out=out)

    def __call__(self, X, state, V):
        """in place on X (3,N) and state (N uint8); every position is finite in this benchmark, so the midpoint always is"""
        T = self.T
        self.launches = 0
        self.inside(X, self.m[0])
        self.op(T.logical_and, self.m[0], state, out=self.m[0])              # active
        self.velocity(V, X)
        for q in range(3):
            self.op(T.mul, self.v[q], COURANT[q], out=self.Xm[q])
            self.op(self.Xm[q].mul_, 0.5)
            self.op(self.Xm[q].add_, X[q])
        self.velocity(V, self.Xm)
        for q in range(3):
            self.op(T.mul, self.v[q], COURANT[q], out=self.Xn[q])
            self.op(self.Xn[q].add_, X[q])
            self.op(T.where, self.m[0], self.Xn[q], X[q], out=X[q])
        self.inside(X, self.m[3])
        self.op(T.logical_and, self.m[0], self.m[3], out=self.m[0])
        self.op(state.copy_, self.m[0])


def lattice(torch, shape, m, permute, device="cuda"):
    """m[0]·m[1]·m[2] points on a regular lattice over the box, x fastest; permute: the same points in a random order"""
    g = [((torch.arange(m[q], dtype=torch.float64, device=device) + off) * (shape[q] / m[q])) for q, off in enumerate((0.37, 0.41, 0.43))]
    X = torch.stack([g[0].repeat(m[1] * m[2]), g[1].repeat_interleave(m[0]).repeat(m[2]), g[2].repeat_interleave(m[0] * m[1])])
    if permute:
        gen = torch.Generator(device=device)
        gen.manual_seed(0)
        X = X[:, torch.randperm(X.shape[1], device=device, generator=gen)]
    return X.contiguous()


def measure(K, torch, shape, dtype, log2n, reps, warm):
    nx, ny, nz = shape
    m = {20: (128, 128, 64), 24: (256, 256, 256)}.get(log2n) or (1 << (log2n - 2 * (log2n // 3)), 1 << (log2n // 3), 1 << (log2n // 3))
    N = m[0] * m[1] * m[2]
    ctx = K.Context(0, "strict", async_=True)
    mk = lambda *s: K.zeros(s, dtype).uniform_(-1.0, 1.0)
    V = (mk(nx + 1, ny, nz), mk(nx, ny + 1, nz), mk(nx, ny, nz + 1))
    comp = Composition(torch, shape, N, dtype)
    X0 = {"lattice": lattice(torch, shape, m, False), "permuted": lattice(torch, shape, m, True)}
    X = {k: torch.empty_like(v) for k, v in X0.items()}
    Xc = torch.empty_like(X0["lattice"])
    state, state_c = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")

    def timed(order, composed):
        x, s = (Xc, state_c) if composed else (X[order], state)
        x.copy_(X0[order]); s.fill_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        if composed:
            comp(x, s, V)
        else:
            K.tracers_advance(x, s, *V, *COURANT, ctx=ctx)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    sides = [(o, c) for o in ("lattice", "permuted") for c in (False, True)]
    for _ in range(warm):
        for side in sides:
            timed(*side)
    ev = {side: [] for side in sides}
    for _ in range(reps):
        for side in sides:
            ev[side].append(timed(*side))
    # the same step on both sides (left behind by the last repetition: the permuted set)
    diff = float((X["permuted"] - Xc).abs().max())
    assert diff <= 1e-12 * max(shape), "the two sides disagree: %g" % diff
    assert bool((state == state_c).all()), "the two sides disagree on who is alive"
    best = {side: min(t) for side, t in ev.items()}
    esize = 8 if dtype == torch.float64 else 4
    field_bytes = esize * sum(t.numel() for t in V)
    particle_bytes = N * (2 * 24 + 2)                                  # X read and written, state read and written
    rec = dict(kernel="ns3d_tracers_advance_%s" % ("f64" if esize == 8 else "f32"), grid=list(shape), n_particles=N, log2_n=log2n,
               mode="strict", reps=reps, warmups=warm, courant=list(COURANT), gathers_per_particle=48,
               gathered_bytes_per_particle=48 * esize, particle_bytes_per_particle=50, field_bytes=field_bytes,
               particle_bytes=particle_bytes, fits_infinity_cache=field_bytes + particle_bytes <= INFINITY_CACHE,
               composed_launches=comp.launches, max_abs_difference=diff, alive_after=int(state.sum()))
    for o in ("lattice", "permuted"):
        f, c = best[(o, False)], best[(o, True)]
        rec[o] = dict(fused_ms=f, composed_ms=c, fused_ms_all=ev[(o, False)], composed_ms_all=ev[(o, True)],
                      fused_particles_per_s=N / (f * 1e-3), composed_particles_per_s=N / (c * 1e-3), speedup_over_composition=c / f)
    rec["permuted_over_lattice_ms"] = best[("permuted", False)] / best[("lattice", False)]
    rec["fused_beats_composition"] = all(rec[o]["fused_ms"] < rec[o]["composed_ms"] for o in ("lattice", "permuted"))
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_rates.jsonl"))
    ap.add_argument("--grids", default="255x153x153,512x512x512")
    ap.add_argument("--counts", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                for log2n in (int(q) for q in a.counts.split(",")):
                    rec = measure(K, torch, tuple(int(q) for q in gs.split("x")), dtype, log2n, a.reps, a.warmup)
                    print(json.dumps(rec))
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
