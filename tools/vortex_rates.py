"""Cost of the vortex fields (ns3d_vortex: Wx, Wy, Wz, Q in one fused pass) against the composition a user has without it — the same
expression in PyTorch elementwise ops on the device — and against a plain device copy that moves the same nominal bytes.

    python tools/vortex_rates.py [--out profiles/vortex_rates.jsonl] [--grids 512x512x512,255x153x153]

Event timing on the stream all three sides run on (the context is NS3D_ASYNC: the call only enqueues), best of 10 after 3 warm-ups,
the sides interleaved in one process; fp64 and fp32, STRICT.  Nominal bytes per cell (vortex.bytes_per_cell): 3 field reads + 4
writes of the element type = 56 B (fp64) / 28 B (fp32).  The composition keeps the header's parentheses with preallocated
temporaries — u, v, w, the three diagonal and six off-diagonal gradient entries and three scratch arrays for Q, fifteen grid-sized
arrays — and counts its own launches and the bytes each of them reads and writes (every operand of every op, once).  The copy moves
bytes/2 in and bytes/2 out.  At 255×153×153 the working set (0.33 GB in fp64 for the fused call) sits partly in the 256 MiB Infinity
Cache — it is re-touched every repetition — so the rates there are not HBM figures.  One JSON line per grid and element type;
`fused_beats_composition` must be true on every line (the composition moves several times the bytes), the ratio to the copy is
recorded, not judged.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12       # B/s, HBM3E of one MI355X


class Composition:
    """the header's expression, op by op, on preallocated arrays; counts launches and operand bytes"""

    def __init__(self, K, torch, n, dtype, d):
        nx, ny, nz = n
        self.torch, self.d = torch, d
        z = lambda *s: K.zeros(s, dtype)
        self.out = [z(nx, ny, nz) for _ in range(4)]
        self.c = [z(nx, ny, nz) for _ in range(6)]                       # u v w gxx gyy gzz
        self.g = [z(nx - 2, ny - 2, nz - 2) for _ in range(9)]           # uy uz vx vz wx wy + three scratch arrays
        self.launches = self.bytes = 0

    def op(self, fn, out, *ins, **kw):
        fn(*ins, out=out, **kw)
        self.launches += 1
        self.bytes += (out.numel() + sum(t.numel() for t in ins if hasattr(t, "numel"))) * out.element_size()
        return out

    def inplace(self, name, t, *args, **kw):
        getattr(t, name)(*args, **kw)
        self.launches += 1
        self.bytes += (2 * t.numel() + sum(a.numel() for a in args if hasattr(a, "numel"))) * t.element_size()
        return t

    def __call__(self, Vx, Vy, Vz):
        T = self.torch
        dx, dy, dz = self.d
        self.launches = self.bytes = 0
        u, v, w, gxx, gyy, gzz = self.c
        uy, uz, vx, vz, wx, wy, a, b, c = self.g
        I = (slice(1, -1),) * 3
        for t, lo, hi in ((u, Vx[:-1], Vx[1:]), (v, Vy[:, :-1], Vy[:, 1:]), (w, Vz[:, :, :-1], Vz[:, :, 1:])):
            self.inplace("mul_", self.op(T.add, t, lo, hi), 0.5)
        for t, lo, hi, s in ((gxx, Vx[:-1], Vx[1:], dx), (gyy, Vy[:, :-1], Vy[:, 1:], dy), (gzz, Vz[:, :, :-1], Vz[:, :, 1:], dz)):
            self.inplace("div_", self.op(T.sub, t, hi, lo), s)
        for t, hi, lo, s in ((uy, u[1:-1, 2:, 1:-1], u[1:-1, :-2, 1:-1], dy), (uz, u[1:-1, 1:-1, 2:], u[1:-1, 1:-1, :-2], dz),
                             (vx, v[2:, 1:-1, 1:-1], v[:-2, 1:-1, 1:-1], dx), (vz, v[1:-1, 1:-1, 2:], v[1:-1, 1:-1, :-2], dz),
                             (wx, w[2:, 1:-1, 1:-1], w[:-2, 1:-1, 1:-1], dx), (wy, w[1:-1, 2:, 1:-1], w[1:-1, :-2, 1:-1], dy)):
            self.inplace("mul_", self.inplace("div_", self.op(T.sub, t, hi, lo), s), 0.5)
        Wx, Wy, Wz, Q = self.out
        for t in self.out:
            t.zero_()
            self.launches += 1
            self.bytes += t.numel() * t.element_size()
        self.op(T.sub, Wx[I], wy, vz)
        self.op(T.sub, Wy[I], uz, wx)
        self.op(T.sub, Wz[I], vx, uy)
        self.op(T.mul, a, gxx[I], gxx[I]); self.op(T.mul, b, gyy[I], gyy[I]); self.inplace("add_", a, b)
        self.op(T.mul, b, gzz[I], gzz[I]); self.inplace("add_", a, b); self.inplace("mul_", a, -0.5)
        self.op(T.mul, b, uy, vx); self.op(T.mul, c, uz, wx); self.inplace("add_", b, c)
        self.op(T.mul, c, vz, wy); self.inplace("add_", b, c)
        self.op(T.sub, Q[I], a, b)


def measure(K, torch, vortex, n, dtype, reps, warm):
    nx, ny, nz = n
    ctx = K.Context(0, "strict", async_=True)
    mk = lambda *s: K.zeros(s, dtype).uniform_(-1.0, 1.0)
    Vx, Vy, Vz = mk(nx + 1, ny, nz), mk(nx, ny + 1, nz), mk(nx, ny, nz + 1)
    d = (1.0 / nx, 1.0 / ny, 1.0 / nz)
    W = [K.zeros((nx, ny, nz), dtype) for _ in range(4)]
    comp = Composition(K, torch, n, dtype, d)
    cells = nx * ny * nz
    nbytes = vortex.bytes_per_cell(dtype, 4) * cells
    src, dst = torch.zeros(nbytes // 16, dtype=torch.float64, device="cuda"), torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
    f64 = dtype == torch.float64

    def fused():
        K.vortex(Vx, Vy, Vz, *d, Wx=W[0], Wy=W[1], Wz=W[2], Q=W[3], ctx=ctx)

    def composed():
        comp(Vx, Vy, Vz)

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
    ev = {k: [] for k, _ in sides}
    for _ in range(reps):
        for name, fn in sides:
            ev[name].append(timed(fn))
    ctx.sync()
    # the same expression on both sides: they agree to rounding (PyTorch divides by a scalar through its reciprocal)
    eps = 1e-12 if f64 else 1e-4
    for got, want in zip(W, comp.out):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= eps * scale, "the two sides disagree"
    best = {k: min(t) for k, t in ev.items()}
    rate = lambda ms: nbytes / (ms * 1e-3)
    out = dict(kernel="ns3d_vortex_%s" % ("f64" if f64 else "f32"), grid=[nx, ny, nz], mode="strict", arith_build=ctx.arith_build(*d),
               reps=reps, warmups=warm, nominal_bytes_per_cell=vortex.bytes_per_cell(dtype, 4), nominal_bytes=nbytes,
               composed_launches=comp.launches, composed_nominal_bytes=comp.bytes, composed_bytes_over_fused=comp.bytes / nbytes,
               fused_ms=best["fused"], composed_ms=best["composed"], copy_ms=best["copy"],
               fused_ms_all=ev["fused"], composed_ms_all=ev["composed"], copy_ms_all=ev["copy"],
               fused_TBps=rate(best["fused"]) / 1e12, copy_TBps=rate(best["copy"]) / 1e12,
               fused_fraction_of_copy_rate=best["copy"] / best["fused"], fused_fraction_of_8TBps=rate(best["fused"]) / PEAK,
               speedup_over_composition=best["composed"] / best["fused"], fused_beats_composition=best["fused"] < best["composed"])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vortex_rates.jsonl"))
    ap.add_argument("--grids", default="512x512x512,255x153x153")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd import vortex
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for gs in a.grids.split(","):
            for dtype in (torch.float64, torch.float32):
                rec = measure(K, torch, vortex, tuple(int(q) for q in gs.split("x")), dtype, a.reps, a.warmup)
                print(json.dumps(rec))
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
