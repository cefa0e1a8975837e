"""Cost of one tracer step on a decomposed grid — ns3d_tracers_advance_mgpu followed by ns3d_tracers_migrate_mgpu on P virtual
z-slab ranks of ONE device — against the one-rank ns3d_tracers_advance of the same particle set on the global grid, in the same
process, interleaved.

    python tools/tracers_mgpu_rates.py [--out profiles/tracers_mgpu_rates.jsonl] [--ranks 2,8] [--counts 20,24]

Event timing on the stream every side runs on, best of 10 after 3 warm-ups; the particle arrays are restored before every run
(outside the timed window), so every repetition does the same work and migrates the same particles.  Global grid 256×152×154
(fp64 fields U(−1,1), Courant factors 0.4, 0.36, 0.32); the particles sit on a regular lattice over the global box, x fastest
("lattice"), or are the same points in a random order ("permuted"); every rank starts with 25 % empty slots.  There is no pass /
fail ratio: the one-rank figure of the same run is the yardstick.  `count_only_ms` is a migrate call on the state the step leaves
behind — nobody moves, so it is the classification, the scan and the BLOCKING read-back of the counts alone.  All ranks share one
device here: the peer copies are device-local, and rates across real xGMI links are out of this tool's reach.  One JSON line per P,
N and order.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
COURANT = (0.4, 0.36, 0.32)
GLOBAL = (256, 152, 154)


def measure(torch, K, P, log2n, order, reps, warm):
    from types import SimpleNamespace
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.tracers import MgpuTracers
    from tracers_rates import lattice
    gx, gy, gz = GLOBAL
    assert (gz - 2) % P == 0
    n = (gx, gy, (gz - 2) // P + 2)
    m = {20: (128, 128, 64), 24: (256, 256, 256)}[log2n]
    N = m[0] * m[1] * m[2]
    mk = lambda *s: K.zeros(s, torch.float64).uniform_(-1.0, 1.0)
    G = SimpleNamespace(Vx=mk(gx + 1, gy, gz), Vy=mk(gx, gy + 1, gz), Vz=mk(gx, gy, gz + 1))
    X0 = lattice(torch, GLOBAL, m, order == "permuted")
    ctx = K.Context(0, "strict", async_=True)
    mg = MultiGpu.create([0] * P, *n, "strict")
    grid = MgpuGrid(mg, *n)
    fs = []
    for r in range(P):
        lo = r * (n[2] - 2)
        cut = lambda A, s: A[:, :, lo:lo + n[2] + s].permute(2, 1, 0).contiguous().permute(2, 1, 0)       # column-major copies
        fs.append(SimpleNamespace(Vx=cut(G.Vx, 0), Vy=cut(G.Vy, 0), Vz=cut(G.Vz, 1)))
    t = MgpuTracers(grid, tuple(1.0 / c for c in COURANT), slack=0.25)
    t._set(X0.cpu().numpy(), torch.ones(N, dtype=torch.uint8).numpy())
    saved = [(x.clone(), s.clone(), i.clone()) for x, s, i in zip(t.X, t.state, t.ids)]
    X1, s1 = torch.empty_like(X0), torch.empty(N, dtype=torch.uint8, device="cuda")
    info = {}

    def restore():
        for l, (x, s, i) in enumerate(saved):
            t.X[l].copy_(x); t.state[l].copy_(s); t.ids[l].copy_(i)
        X1.copy_(X0); s1.fill_(1)

    def timed(side):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        if side == "one_rank":
            K.tracers_advance(X1, s1, G.Vx, G.Vy, G.Vz, *COURANT, ctx=ctx)
        elif side == "advance_only":
            mg.tracers_advance(t.X, t.state, [f.Vx for f in fs], [f.Vy for f in fs], [f.Vz for f in fs], *COURANT)
        else:
            before = t.moved
            t.advance(fs, 1.0)
            info["moved"] = t.moved - before
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def count_only():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        moved = t.migrate()
        b.record()
        torch.cuda.synchronize()
        assert moved == 0
        return a.elapsed_time(b)

    sides = ("one_rank", "advance_only", "step")
    for _ in range(warm):
        for side in sides:
            timed(side)
    ev = {side: [] for side in sides + ("count_only",)}
    for _ in range(reps):
        for side in sides:
            ev[side].append(timed(side))
        ev["count_only"].append(count_only())                  # on the state the step left behind
    # the same step on both sides, from the same start: by id, bit for bit
    restore()
    K.tracers_advance(X1, s1, G.Vx, G.Vy, G.Vz, *COURANT, ctx=ctx)
    t.advance(fs, 1.0)
    ctx.sync()
    same =bool(torch.equal(torch.from_numpy(t.index_positions()), X1.cpu())) and bool((torch.from_numpy(t.alive()) == (s1.cpu() == 1)).all())
    best = {k: min(v) for k, v in ev.items()}
    rec = dict(tool="tracers_mgpu_rates", ranks=P, dims=[1, 1, P], global_grid=list(GLOBAL), local_grid=list(n), n_particles=N, log2_n=log2n,
               order=order, reps=reps, warmups=warm, courant=list(COURANT), dtype="f64", caps=t.caps(), grown=t.grown,
               moved_per_step=info["moved"], fraction_migrated=info["moved"] / N, equals_one_rank_bits=same,
               one_rank_ms=best["one_rank"], advance_mgpu_ms=best["advance_only"], step_ms=best["step"], count_only_ms=best["count_only"],
               step_over_one_rank=best["step"] / best["one_rank"], one_rank_particles_per_s=N / (best["one_rank"] * 1e-3),
               step_particles_per_s=N / (best["step"] * 1e-3), ms_all=ev)
    mg.sync()
    mg.close()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_mgpu_rates.jsonl"))
    ap.add_argument("--ranks", default="2,8")
    ap.add_argument("--counts", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from navierstokes3d_amd import kernels as K
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for P in (int(q) for q in a.ranks.split(",")):
            for log2n in (int(q) for q in a.counts.split(",")):
                for order in ("lattice", "permuted"):
                    rec = measure(torch, K, P, log2n, order, a.reps, a.warmup)
                    print(json.dumps({k: v for k, v in rec.items() if k != "ms_all"}))
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
