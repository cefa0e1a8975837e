#!/usr/bin/env python3
"""A/B (round 3): do consecutive four-iteration passes gain from meeting in the Infinity Cache?  Instead of NP full passes over the
grid (each streams 5 arrays through HBM), a window of Z planes slides up the grid and the NP passes follow each other through it, each
four planes behind the previous one (pass q sweeps planes [a-4q, a+Z-4q) once pass q-1 has produced up to a+Z-4(q-1)): what pass q-1
wrote is re-read by pass q a few launches later — from the 256 MB memory-side cache if it is still there.  Uses the production kernel
through ns3d_pt_sweepn's plane ranges; the result is compared bit for bit with NP full passes.
    python tools/ab/mall_wavefront.py [--n 512 --passes 3 --windows 16,24,32,48,64]
With --passes 1 no pass follows another through the cache: what is left of a window launch is that it restarts every tile on the same
plane.  --runs N repeats the whole measurement; every line also gives ms per z-step (a launch of Z planes marches Z + 6 steps: six fill
the pipeline of the four levels), min and median of --reps timings.
    python tools/ab/mall_wavefront.py --passes 1 --windows 32,64,128 --runs 2 --reps 20 --variantn 2800"""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from navierstokes3d_amd import kernels as K, lib as L  # noqa: E402
from navierstokes3d_amd.params import cavity_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512); ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--windows", default="16,24,32,48,64"); ap.add_argument("--variantn", type=int, default=2891)
ap.add_argument("--runs", type=int, default=1); ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
p = cavity_params(a.n)
nx, ny, nz = p.nx, p.ny, p.nz
ctx = K.Context(0, "strict", async_=True)
ctx.set_ptn_variant(a.variantn)
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
z = lambda *s: K.zeros(s)
P = [z(nx, ny, nz) for _ in range(a.passes + 1)]
D = [z(nx - 2, ny - 2, nz - 2) for _ in range(a.passes + 1)]
R = z(nx, ny, nz); R.permute(2, 1, 0).uniform_(-1e-3, 1e-3, generator=gen)
P[0].permute(2, 1, 0).uniform_(-1, 1, generator=gen); D[0].permute(2, 1, 0).uniform_(-1, 1, generator=gen)
pt = K.pt_params(P[0], p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI, False, 0.0, 0.0)

def full():
    for q in range(a.passes):
        K.pt_sweepn(4, P[q], P[q + 1], D[q], D[q + 1], R, pt, ctx=ctx)

nsteps = [0]                                  # z-steps marched by the launches of the last wave(): planes + 6 each

def wave(Z):
    top = [1] * a.passes                      # next plane each pass has to produce
    a0 = 1
    nsteps[0] = 0
    while top[-1] < nz - 1:
        for q in range(a.passes):
            lim = nz - 1 if (q == 0 or top[q - 1] >= nz - 1) else top[q - 1] - 4      # inputs complete up to lim+4
            hi = min(lim, a0 + Z - 4 * q, nz - 1)
            if hi > top[q]:
                K.pt_sweepn(4, P[q], P[q + 1], D[q], D[q + 1], R, pt, top[q], hi, ctx=ctx)
                nsteps[0] += hi - top[q] + 6
                top[q] = hi
        a0 += Z

def timed(fn):
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[0], ts[len(ts) // 2]

full(); torch.cuda.synchronize()
ref_P, ref_D = P[-1].clone(), D[-1].clone()
rate = lambda t: nx * ny * nz * 4 * a.passes / t / 1e6
for run in range(a.runs):
    t_full, m_full = timed(full)
    s_full = a.passes * (nz - 2 + 6)
    print("run %d: %d full passes of four iterations: %.3f ms min, %.3f median (%.0f Mcells*it/s); %d z-steps, %.3f us per step min, %.3f median"
          % (run + 1, a.passes, t_full * 1e3, m_full * 1e3, rate(t_full), s_full, t_full * 1e6 / s_full, m_full * 1e6 / s_full), flush=True)
    for Z in [int(q) for q in a.windows.split(",")]:
        for q in range(1, a.passes + 1):
            P[q].zero_(); D[q].zero_()
        wave(Z); torch.cuda.synchronize()
        same = torch.equal(P[-1].view(torch.int64), ref_P.view(torch.int64)) and torch.equal(D[-1].view(torch.int64), ref_D.view(torch.int64))
        t, m = timed(lambda: wave(Z))
        print("run %d: window of %3d planes: %.3f ms min, %.3f median (%.0f Mcells*it/s) = %.3f x, bit-identical %s; %d z-steps, %.3f us per step min, "
              "%.3f median = %.3f x the full pass's" % (run + 1, Z, t * 1e3, m * 1e3, rate(t), t_full / t, same, nsteps[0], t * 1e6 / nsteps[0],
                                                       m * 1e6 / nsteps[0], (t / nsteps[0]) / (t_full / s_full)), flush=True)
