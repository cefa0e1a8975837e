"""Cost of ns3d_sgs_viscosity (WALE, Vreman) against ns3d_eddy_viscosity, against a plain device copy of one velocity array and
against the composition a user has without it — the same expression in PyTorch elementwise ops on the device.

    python tools/sgs_rates.py [--out profiles/sgs_rates.jsonl] [--grids 512x512x512,255x153x153]

Device events on the stream every side runs on (the context is NS3D_ASYNC: a call only enqueues); seven rounds of five calls, the
sides alternating inside every round in one process, after one warm-up round; the figure of a side is the median over the rounds of
the per-call time, recorded with the smallest and the largest round.  fp64 and fp32, STRICT and FAST.  One JSON line per grid,
element type, mode and operator.

Bytes per cell of the fused call: three field reads and one write of the element type, 32 B (fp64) / 16 B (fp32) — the same as
ns3d_eddy_viscosity's, so the difference between the two is arithmetic.  FLOOR of that difference: the VALU instructions the
operator adds to k_eddy_visc's plane loop, counted in the disassembly of the gfx950 code object as the difference of the opcode
histograms of k_eddy_visc<OP, T> and k_eddy_visc<0, T> of the same arithmetic build (EXTRA_CYCLES below), priced at the vector
throughput of one SIMD per wave64 instruction — fp32 FMA/mul/add and 32-bit selects 2 cycles (157.3 TFLOP/s = 32 lanes per clock per
SIMD), fp32 transcendentals 4, fp64 FMA/mul/add 4 (half rate), v_rcp_f64 / v_rsq_f64 8 — and spread over 1024 SIMDs at 2.4 GHz:
floor_ms = cycles · cells/64 / (1024 · 2.4e9).  It is a floor: it assumes perfect issue on every SIMD and nothing else in the way.
`hidden` says whether the measured difference to ns3d_eddy_viscosity stays within the run's own min–max spread (the arithmetic then
sits behind the loads); `open_item` whether the call exceeds Smagorinsky's time plus the floor by more than that spread.

The composition evaluates the header's statement with preallocated arrays, in-place ops and addcmul (one launch per product-and-sum,
the most favourable form PyTorch offers) and counts its launches and the bytes every op reads and writes.  `fused_beats_composition`
must be true on every line.  At 255×153×153 the working set sits partly in the 256 MiB Infinity Cache, so the rates there are not
HBM figures.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIMDS, CLOCK = 1024, 2.4e9
# priced VALU cycles per wave64 and plane the operator adds to k_eddy_visc's loop: (build, dtype, operator) → cycles
EXTRA_CYCLES = {
    ("strict", "f64", "wale"): 466, ("strict", "f64", "vreman"): 174, ("strict", "f32", "wale"): 250, ("strict", "f32", "vreman"): 84,
    ("strictx", "f64", "wale"): 466, ("strictx", "f64", "vreman"): 174, ("strictx", "f32", "wale"): 262, ("strictx", "f32", "vreman"): 90,
    ("strictp", "f64", "wale"): 464, ("strictp", "f64", "vreman"): 172, ("strictp", "f32", "wale"): 238, ("strictp", "f32", "vreman"): 82,
    ("fast", "f64", "wale"): 398, ("fast", "f64", "vreman"): 146, ("fast", "f32", "wale"): 224, ("fast", "f32", "vreman"): 70,
}


class Composition:
    """the header's statement, op by op, on preallocated arrays; counts launches and operand bytes"""

    def __init__(self, K, torch, n, dtype, d):
        nx, ny, nz = n
        self.torch, self.d, self.K = torch, d, K
        z = lambda *s: K.zeros(s, dtype)
        self.out = z(nx, ny, nz)
        self.c = [z(nx, ny, nz) for _ in range(6)]                       # u v w gxx gyy gzz
        self.g = [z(nx - 2, ny - 2, nz - 2) for _ in range(6)]           # uy uz vx vz wx wy
        self.pool, self.used = [], 0
        self.launches = self.bytes = 0

    def tmp(self):
        if self.used == len(self.pool):
            self.pool.append(self.torch.empty_like(self.g[0]))
        self.used += 1
        return self.pool[self.used - 1]

    def count(self, out, *ins):
        self.launches += 1
        self.bytes += (out.numel() + sum(t.numel() for t in ins if hasattr(t, "numel"))) * out.element_size()

    def op(self, fn, out, *ins):
        fn(*ins, out=out)
        self.count(out, *ins)
        return out

    def inplace(self, name, t, *args, **kw):
        getattr(t, name)(*args, **kw)
        self.count(t, t, *args)
        return t

    def dot3(self, a0, b0, a1, b1, a2, b2):
        """(a0*b0 + a1*b1) + a2*b2 into a fresh temporary: three launches"""
        t = self.op(self.torch.mul, self.tmp(), a0, b0)
        self.inplace("addcmul_", t, a1, b1)
        return self.inplace("addcmul_", t, a2, b2)

    def gradient(self, Vx, Vy, Vz):
        T = self.torch
        dx, dy, dz = self.d
        u, v, w, gxx, gyy, gzz = self.c
        uy, uz, vx, vz, wx, wy = self.g
        for t, lo, hi in ((u, Vx[:-1], Vx[1:]), (v, Vy[:, :-1], Vy[:, 1:]), (w, Vz[:, :, :-1], Vz[:, :, 1:])):
            self.inplace("mul_", self.op(T.add, t, lo, hi), 0.5)
        for t, lo, hi, s in ((gxx, Vx[:-1], Vx[1:], dx), (gyy, Vy[:, :-1], Vy[:, 1:], dy), (gzz, Vz[:, :, :-1], Vz[:, :, 1:], dz)):
            self.inplace("div_", self.op(T.sub, t, hi, lo), s)
        for t, hi, lo, s in ((uy, u[1:-1, 2:, 1:-1], u[1:-1, :-2, 1:-1], dy), (uz, u[1:-1, 1:-1, 2:], u[1:-1, 1:-1, :-2], dz),
                             (vx, v[2:, 1:-1, 1:-1], v[:-2, 1:-1, 1:-1], dx), (vz, v[1:-1, 1:-1, 2:], v[1:-1, 1:-1, :-2], dz),
                             (wx, w[2:, 1:-1, 1:-1], w[:-2, 1:-1, 1:-1], dx), (wy, w[1:-1, 2:, 1:-1], w[1:-1, :-2, 1:-1], dy)):
            self.inplace("mul_", self.inplace("div_", self.op(T.sub, t, hi, lo), s), 0.5)
        I = (slice(1, -1),) * 3
        return gxx[I], gyy[I], gzz[I], uy, uz, vx, vz, wx, wy

    def strain2(self, G):
        T = self.torch
        gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
        s2 = self.inplace("mul_", self.dot3(gxx, gxx, gyy, gyy, gzz, gzz), 2.0)
        for p, q in ((uy, vx), (uz, wx), (vz, wy)):
            a = self.op(T.add, self.tmp(), p, q)
            self.inplace("addcmul_", s2, a, a)
        return s2

    def wale(self, G):
        T = self.torch
        gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
        q11, q12, q13 = self.dot3(gxx, gxx, uy, vx, uz, wx), self.dot3(gxx, uy, uy, gyy, uz, wy), self.dot3(gxx, uz, uy, vz, uz, gzz)
        q21, q22, q23 = self.dot3(vx, gxx, gyy, vx, vz, wx), self.dot3(vx, uy, gyy, gyy, vz, wy), self.dot3(vx, uz, gyy, vz, vz, gzz)
        q31, q32, q33 = self.dot3(wx, gxx, wy, vx, gzz, wx), self.dot3(wx, uy, wy, gyy, gzz, wy), self.dot3(wx, uz, wy, vz, gzz, gzz)
        t = self.inplace("mul_", self.inplace("add_", self.op(T.add, self.tmp(), q11, q22), q33), 1.0 / 3.0)
        for q in (q11, q22, q33):
            self.inplace("sub_", q, t)
        for a, b in ((q12, q21), (q13, q31), (q23, q32)):
            self.inplace("mul_", self.inplace("add_", a, b), 0.5)
        dd = self.dot3(q11, q11, q22, q22, q33, q33)
        off = self.inplace("mul_", self.dot3(q12, q12, q13, q13, q23, q23), 2.0)
        self.inplace("add_", dd, off)
        ss = self.inplace("mul_", self.strain2(G), 0.5)
        r = self.op(T.sqrt, self.tmp(), dd)
        num = self.op(T.mul, self.tmp(), dd, r)
        den = self.inplace("mul_", self.inplace("sqrt_", r), dd)                   # dd·√√dd
        rs = self.op(T.sqrt, self.tmp(), ss)
        self.inplace("mul_", self.inplace("mul_", ss, ss), rs)                      # (ss·ss)·√ss
        self.inplace("add_", den, ss)
        zero = self.op(T.eq, self.torch.empty_like(den, dtype=T.bool), den, 0)
        self.inplace("div_", num, den)
        return self.inplace("masked_fill_", num, zero, 0.0)

    def vreman(self, G):
        T = self.torch
        gxx, gyy, gzz, uy, uz, vx, vz, wx, wy = G
        b11, b22, b33 = self.dot3(gxx, gxx, uy, uy, uz, uz), self.dot3(vx, vx, gyy, gyy, vz, vz), self.dot3(wx, wx, wy, wy, gzz, gzz)
        b12, b13, b23 = self.dot3(gxx, vx, uy, gyy, uz, vz), self.dot3(gxx, wx, uy, wy, uz, gzz), self.dot3(vx, wx, gyy, wy, vz, gzz)
        aa = self.inplace("add_", self.op(T.add, self.tmp(), b11, b22), b33)
        B = self.op(T.mul, self.tmp(), b11, b22)
        self.inplace("addcmul_", B, b12, b12, value=-1.0)
        for p, q, r in ((b11, b33, b13), (b22, b33, b23)):
            self.inplace("addcmul_", B, p, q)
            self.inplace("addcmul_", B, r, r, value=-1.0)
        self.inplace("clamp_", B, min=0.0)
        zero = self.op(T.eq, self.torch.empty_like(aa, dtype=T.bool), aa, 0)
        self.inplace("sqrt_", self.inplace("div_", B, aa))
        return self.inplace("masked_fill_", B, zero, 0.0)

    def __call__(self, name, Vx, Vy, Vz, mu, c):
        self.launches = self.bytes = self.used = 0
        G = self.gradient(Vx, Vy, Vz)
        val = getattr(self, name)(G)
        self.out.fill_(mu)
        self.count(self.out)
        I = (slice(1, -1),) * 3
        self.inplace("add_", self.inplace("mul_", val, c), mu)
        self.out[I].copy_(val)
        self.count(val, val)
        return self.out


def measure(K, torch, n, dtype, mode, rounds, reps, fh):
    nx, ny, nz = n
    ctx = K.Context(0, mode, async_=True)
    dt = "f64" if dtype == torch.float64 else "f32"
    mk = lambda *s: K.zeros(s, dtype).uniform_(-1.0, 1.0)
    Vx, Vy, Vz = mk(nx + 1, ny, nz), mk(nx, ny + 1, nz), mk(nx, ny, nz + 1)
    d = (1.0 / (nx + 1), 1.0 / (ny + 1), 1.0 / (nz + 1))        # no power of two at 512: the exact-division build, as at 255×153×153
    mu, rho, length = 1e-3, 1.0, 0.17 * (d[0] * d[1] * d[2]) ** (1.0 / 3.0)
    out = {k: K.zeros((nx, ny, nz), dtype) for k in ("smagorinsky", "wale", "vreman")}
    comp = Composition(K, torch, n, dtype, d)
    src, dst = Vx, torch.empty_like(Vx)
    cells = nx * ny * nz
    build = ctx.arith_build(*d)

    def fused(name):
        if name == "smagorinsky":
            return lambda: K.eddy_viscosity(out[name], Vx, Vy, Vz, mu, rho, length, *d, ctx=ctx)
        return lambda: K.sgs_viscosity(out[name], Vx, Vy, Vz, name, mu, rho, length, *d, ctx=ctx)
    T = torch.float64 if dtype == torch.float64 else torch.float32
    c = float(torch.tensor(rho * length * length, dtype=T))
    sides = [("eddy_viscosity", fused("smagorinsky")), ("sgs_wale", fused("wale")), ("sgs_vreman", fused("vreman")),
             ("copy", lambda: K.copy(dst, src, ctx=ctx)),
             ("composed_wale", lambda: comp("wale", Vx, Vy, Vz, mu, c)), ("composed_vreman", lambda: comp("vreman", Vx, Vy, Vz, mu, c))]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    counts = {}
    for name, fn in sides:          # the warm-up round; the composition's counters and its agreement with the fused call
        timed(fn)
        if name.startswith("composed_"):
            op = name.split("_")[1]
            counts[op] = (comp.launches, comp.bytes)
            got, want = out[op], comp.out
            eps = 1e-9 if dtype == torch.float64 else 2e-3
            assert float((got - want).abs().max()) <= eps * float(want.abs().max()), "the two sides disagree (%s)" % op
    ev = {k: [] for k, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            ev[name].append(timed(fn))
    ctx.sync()
    med = {k: statistics.median(v) for k, v in ev.items()}
    spread = lambda k: max(ev[k]) - min(ev[k])
    esz = 8 if dtype == torch.float64 else 4
    common = dict(grid=[nx, ny, nz], dtype=dt, mode=mode, build=build, rounds=rounds, reps=reps)

    def line(call, k, **more):
        rec = dict(call=call, **common, ms=round(med[k], 4), ms_min=round(min(ev[k]), 4), ms_max=round(max(ev[k]), 4), **more)
        print(json.dumps(rec))
        fh.write(json.dumps(rec) + "\n")
        fh.flush()
    bpc = 4 * esz
    rate = lambda k, nbytes: round(nbytes / (med[k] * 1e-3) / 1e9, 1)
    line("copy", "copy", bytes=2 * src.numel() * esz, gbs=rate("copy", 2 * src.numel() * esz))
    line("eddy_viscosity", "eddy_viscosity", bytes_per_cell=bpc, gbs=rate("eddy_viscosity", bpc * cells),
         share_of_copy=round(med["copy"] * (bpc / (2 * esz)) / med["eddy_viscosity"], 3))
    for op in ("wale", "vreman"):
        k = "sgs_" + op
        floor = EXTRA_CYCLES[(build, dt, op)] * (cells / 64.0) / (SIMDS * CLOCK) * 1e3
        extra = med[k] - med["eddy_viscosity"]
        noise = max(spread(k), spread("eddy_viscosity"))
        launches, nbytes = counts[op]
        line("sgs_viscosity", k, operator=op, bytes_per_cell=bpc, gbs=rate(k, bpc * cells),
             ratio_to_eddy_viscosity=round(med[k] / med["eddy_viscosity"], 3), extra_ms=round(extra, 4),
             arithmetic_floor_ms=round(floor, 4), ratio_floor=round((med["eddy_viscosity"] + floor) / med["eddy_viscosity"], 3),
             spread_ms=round(noise, 4), hidden=bool(extra <= noise), open_item=bool(extra > floor + noise),
             composed_ms=round(med["composed_" + op], 4), composed_ms_min=round(min(ev["composed_" + op]), 4),
             composed_ms_max=round(max(ev["composed_" + op]), 4), composed_launches=launches, composed_bytes=nbytes,
             composed_bytes_over_fused=round(nbytes / (bpc * cells), 1),
             speedup_over_composition=round(med["composed_" + op] / med[k], 1),
             fused_beats_composition=bool(max(ev[k]) < min(ev["composed_" + op])))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgs_rates.jsonl"))
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
                    measure(K, torch, tuple(int(q) for q in gs.split("x")), dtype, mode, a.rounds, a.reps, fh)
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
