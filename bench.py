#!/usr/bin/env python3
"""bench.py — headline benchmark of the hot path: the fused pseudo-transient pressure-Poisson iteration.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: set up (build check, fields, plan phase), W warm-up iterations, the K timed
ones, the outputs (--dump-outputs DIR) and the line.  --full adds everything else described below — the untimed self-check
(config.verified), the `strong` measurement, `config_b`, the CPU baseline and the live roofline.traffic — each of which the
matching --no-* option still leaves out.

Metric (BASELINE.json): Mcells·PT-iter/s (+ achieved HBM GB/s) on the 512³ lid-driven-cavity Poisson-only
configuration (BASELINE.json configs[2]; synthetic, SURVEY.md §8d Config 3).  One "step" = one PT iteration
{update_dPrdτ!; update_Pr!; set_bc_Pr!} (multi.jl:459-463) over the whole grid; the K timed steps are issued as passes
of the planned depth (two, three or four iterations per launch of k_pt_sweep2 / k_pt_sweepN; single sweeps for a
remainder).  Fields are resident in HBM before the timed region; an untimed plan phase before the warm-up lets the
library time its tile shapes once.  With --full, after the timed region the line CERTIFIES ITSELF (config.verified, untimed): one
more pass of exactly the timed kernel instance — same depth, same tile variant, same arithmetic build — from the state
the run left behind is compared on the device, bit for bit in STRICT mode (FAST: relative L2 ≤ 1e-6), with as many one-thread-per-cell single sweeps
(N>1: one pass of the slab schedule against {single sweep; update_halo!(Pr)} per iteration, multi.jl:459-463); a mismatch
prints verified: false and exits with status 3.
For N>1 every rank owns one 512×512×512 z-slab of an implicit global grid 512×512×(N·510+2) (weak scaling, the
reference's own model: local size fixed, multi.jl:325,338); per pass the `depth` outermost own planes of Pr and depth−1
of dPrdτ travel to each z neighbour behind the interior sweep — by RCCL send/recv over xGMI inside libns3d.so
(ns3d_mgpu_create_rank, ns3d_slab_iterate).  With --full the same line carries a `strong` object: the same GLOBAL grid (BASELINE:
"512³ grid, 1/2/4/8 MI355X") split into N z-slabs, measured right after the weak run with the same K and W.  `python bench.py --gpus N` without a launcher starts its N ranks itself (torch.distributed.run as a
child process, before this process touches the GPU).  The ranks agree COLLECTIVELY on the transport: a gloo group comes up
first (control plane: unique id, barriers, timing), RCCL is brought up and probed with a verified plane exchange, and only
if every rank succeeded is it used; otherwise all ranks together take the host-staged transport over gloo and the line says so.

roofline.frac is a physical fraction (SURVEY.md §8d "Roofline fraction = achieved / 8000 GB/s" with the bytes one launch
MUST move: one pass over Pr, ∇V, dPrdτ in and dPrdτ, Pr out = itemsize·(N + 4·N_inner), however many PT iterations the
launch advances) and is ≤ 1; the metric's "achieved HBM GB/s = algorithmic_bytes · iters / wall" (40 B per cell and
ITERATION, §8d) is reported next to it as hbm_gbps_algorithmic / roofline.effective_frac and exceeds the physical number by
the temporal-blocking factor.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E nominal, /opt/skills/guides/MI355X_MICROARCH.md
DUMP_SAMPLE = 2500000   # --dump-outputs: values per array beyond which a seeded sample is written (2 x 20 MB in fp64)


def algorithmic_bytes(nx, ny, nz, itemsize):
    """read Pr, read ∇V, read+write dPrdτ, write Pr = itemsize·(N + 4·N_inner) per PT iteration
    (≈40 B/cell fp64)."""
    return itemsize * (nx * ny * nz + 4 * (nx - 2) * (ny - 2) * (nz - 2))


def cpu_baseline(n, nzs, iters, dtype):
    """C/OpenMP restatement of the reference CPU (Threads) path — the oracle's UNFUSED loop — timed on the host cores
    of this box on a bounded slab sample of the same workload."""
    from oracle import oracle as O
    from navierstokes3d_amd.params import cavity_params
    cores = len(os.sched_getaffinity(0))
    try:  # respect the cgroup CPU quota of the box (e.g. "1600000 100000" = 16 cores of a 256-thread host)
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = max(1, min(cores, int(round(int(quota) / int(period)))))
    except Exception:
        pass
    os.environ["OMP_NUM_THREADS"] = str(cores)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    p = cavity_params(n, nzs)
    npdt = np.float64 if dtype == "f64" else np.float32
    rng = np.random.Generator(np.random.MT19937(12345))
    Pr = O.zeros((p.nx, p.ny, p.nz), npdt)
    d = O.zeros((p.nx - 2, p.ny - 2, p.nz - 2), npdt)
    rhs = np.asfortranarray((rng.random((p.nz, p.ny, p.nx), dtype=np.float64).transpose(2, 1, 0) * 2e-3 - 1e-3).astype(npdt))
    Rp = O.zeros((p.nx - 2, p.ny - 2, p.nz - 2), npdt)
    args = (p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, 0, False, 0.0, 0.0, -1.0)
    O.pt_solve(Pr, d, rhs, Rp, *args, 2, 0, 1.0, 1.0)  # warm-up / page-in
    t0 = time.perf_counter()
    O.pt_solve(Pr, d, rhs, Rp, *args, iters, 0, 1.0, 1.0)
    t = time.perf_counter() - t0
    if t < 8.0:  # bounded sample of ~10-20 s of CPU work
        more = int(min(max(iters * (12.0 / max(t, 1e-3)), iters), 4000))
        t0 = time.perf_counter()
        O.pt_solve(Pr, d, rhs, Rp, *args, more, 0, 1.0, 1.0)
        t = time.perf_counter() - t0
        iters = more
    cells = p.nx * p.ny * p.nz
    return {
        "value": cells * iters / t / 1e6, "unit": "Mcells*iter/s", "cores": cores, "kind": "port",
        "sample": "%dx%dx%d slab of the 512^3 workload, %d unfused PT iterations (oracle C/OpenMP restatement of the "
                  "reference Threads path, %s), %.1f s" % (p.nx, p.ny, p.nz, iters, dtype, t),
        "gbps_algorithmic": algorithmic_bytes(p.nx, p.ny, p.nz, np.dtype(npdt).itemsize) * iters / t / 1e9,
    }


def self_launch(a):
    """`python bench.py --gpus N` typed as is: start the N ranks as children (one process per GPU) and relay rank 0's line.
    Runs before this process has made any GPU call (device_count() does not initialise the GPU on this image)."""
    ndev = torch.cuda.device_count()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if ndev < a.gpus:           # rehearsal on a smaller box: ranks share devices, RCCL cannot run, the line says so
        env["NS3D_BENCH_SHARED_GPU"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if lines:
        print(lines[-1])
    else:
        sys.stderr.write(r.stdout)
    return r.returncode if (r.returncode or lines) else 1


def agree(ok):
    """every rank takes the same branch: MIN of the ranks' ok flags over the gloo control group"""
    t = torch.tensor([1 if ok else 0], dtype=torch.int32)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def bring_up_rccl(world, rank, device, nx, ny, nz, mode, tdt):
    """libns3d's own RCCL communicator (ns3d_mgpu_create_rank), probed with a verified plane exchange.  Every stage ends
    with a collective agreement, so either all ranks return a MultiGpu or all return (None, reason)."""
    # a communicator that never comes up (or a send/recv that never completes) cannot be cancelled from inside the process:
    # say so and end the rank, so that the launcher tears the job down instead of waiting for the driver's limit
    limit = float(os.environ.get("NS3D_BENCH_RCCL_TIMEOUT", "300"))
    stage = ["unique id"]

    def give_up():
        sys.stderr.write("bench.py rank %d: RCCL bring-up (%s) did not finish within %.0f s; rerun with --transport host\n"
                         % (rank, stage[0], limit))
        sys.stderr.flush()
        os._exit(17)

    dog = threading.Timer(limit, give_up)
    dog.daemon = True
    dog.start()
    try:
        return _bring_up_rccl(world, rank, device, nx, ny, nz, mode, tdt, stage)
    finally:
        dog.cancel()


def _bring_up_rccl(world, rank, device, nx, ny, nz, mode, tdt, stage):
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.mgpu import MultiGpu
    why, uid = "", None
    try:                                            # stage 1: RCCL loads everywhere (dlopen) and makes an id
        uid = MultiGpu.unique_id()
    except L.Ns3dError as e:
        why = str(e)
    if not agree(uid is not None):
        return None, "RCCL not loadable on every rank" + (": " + why if why else "")
    box = [uid]
    dist.broadcast_object_list(box, src=0)
    mg = None
    stage[0] = "ncclCommInitRank"
    try:                                            # stage 2: communicator
        mg = MultiGpu.create_rank(world, rank, device, box[0], nx, ny, nz, mode)
    except L.Ns3dError as e:
        why = str(e)
    if not agree(mg is not None):
        if mg is not None:
            mg.close()
        return None, "ncclCommInitRank failed on a rank" + (": " + why if why else "")
    ok = True
    stage[0] = "probe send/recv"
    try:                                            # stage 3: one plane to each z neighbour and back, contents checked
        probe = K.zeros((8, 8, nz), tdt, torch.device("cuda", device))      # nz planes: overlap 2 like a cell-centred field
        probe.fill_(float(rank + 1))
        mg.update_halo(probe)
        mg.sync()
        lo, hi = probe[0, 0, 0].item(), probe[7, 7, nz - 1].item()
        ok = (lo == (rank if rank > 0 else rank + 1)) and (hi == (rank + 2 if rank < world - 1 else rank + 1))
        ok = ok and mg.rccl_ranks() == world
        if not ok:
            why = "probe exchange returned wrong planes (%r, %r)" % (lo, hi)
    except L.Ns3dError as e:
        ok, why = False, str(e)
    if not agree(ok):
        mg.close()
        return None, "RCCL probe exchange failed on a rank" + (": " + why if why else "")
    return mg, ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--grid", dest="n", type=int, default=512, help="local grid is n x n x nz")
    ap.add_argument("--grid-nz", dest="nz", type=int, default=None)
    ap.add_argument("--mode", default=os.environ.get("NS3D_BENCH_MODE", "strict"), choices=["strict", "fast"])
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--variant", type=int, default=int(os.environ.get("NS3D_PT_VARIANT", "0")))
    ap.add_argument("--variant2", type=int, default=None, help="tile shape of the two-iteration sweep")
    ap.add_argument("--no-temporal-blocking", action="store_true")
    ap.add_argument("--depth", type=int, default=int(os.environ.get("NS3D_BENCH_DEPTH", "0")),
                    help="PT iterations per pass over memory: 0 = what the plan phase measures as fastest (2, 3 or 4; 5 with --dtype f32), 2…5 forced")
    ap.add_argument("--variantn", type=int, default=None, help="tile shape of the N-iteration sweep")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: n x n x nz per GPU (the reference's model); strong: n x n x nz is the GLOBAL grid, split in z")
    ap.add_argument("--no-autotune", action="store_true", help="built-in tile choice instead of timing the shapes once")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the untimed self-check of the timed kernel / schedule")
    ap.add_argument("--no-strong", action="store_true",
                    help="N>1: skip the second measurement (the same GLOBAL grid split in z) reported as `strong`")
    ap.add_argument("--cpu-iters", type=int, default=12)
    ap.add_argument("--reserve-cus", type=int, default=int(os.environ.get("NS3D_BENCH_RESERVE_CUS", "0")),
                    help="compute launches leave this many CUs out (ns3d_reserve_cus: room for RCCL's kernels beside the interior sweep)")
    ap.add_argument("--interior-chunks", type=int, default=int(os.environ.get("NS3D_BENCH_INTERIOR_CHUNKS", "1")),
                    help="N>1: the interior sweep of a z-slab pass in this many launches (ns3d_mgpu_set_interior_chunks)")
    ap.add_argument("--overlap-trial", default=os.environ.get("NS3D_BENCH_OVERLAP_TRIAL", "auto"), choices=["auto", "off"],
                    help="N>1 over RCCL, neither knob above given: time a few passes with (0 CUs, 1 chunk), (0, 2) and (8, 1) in the "
                         "untimed plan phase — all ranks together, maximum over ranks — and keep the fastest; `config.overlap_trial`")
    ap.add_argument("--no-config-b", action="store_true", default=os.environ.get("NS3D_BENCH_NO_CONFIG_B") == "1",
                    help="N=1: skip the `config_b` object (the same Poisson-only measurement on the reference's own 255x153x153 "
                         "grid and spacings, STRICT and FAST, a few seconds)")
    ap.add_argument("--no-traffic", action="store_true", default=os.environ.get("NS3D_BENCH_NO_TRAFFIC") == "1",
                    help="N=1: do not measure roofline.traffic live (two short rocprofv3 --pmc child runs of this command's kernel "
                         "instance after the timed region); the figure then comes from profiles/pt_sweep_traffic.json")
    ap.add_argument("--transport", default=os.environ.get("NS3D_BENCH_TRANSPORT", "auto"), choices=["auto", "rccl", "host"],
                    help="N>1: rccl = libns3d's RCCL communicator (fails loudly if it cannot come up), host = host-staged "
                         "over gloo, auto = rccl with a collective fall-back to host")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the self-check, `strong`, `config_b`, the CPU baseline and the live roofline.traffic "
                         "(each still subject to its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N=1: after the timed steps, write Pr and dPrdtau as the timed path left them to DIR/<name>.npy; "
                         "arrays of more than %d values as a seeded sample (dump_outputs)" % DUMP_SAMPLE)
    a = ap.parse_args()
    if a.dump_outputs is not None and a.gpus > 1:
        ap.error("--dump-outputs writes the fields of a one-GPU run")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py --gpus %d runs under a launcher with WORLD_SIZE=%d" % (a.gpus, world))
    ndev = max(torch.cuda.device_count(), 1)
    shared_gpu = os.environ.get("NS3D_BENCH_SHARED_GPU") == "1" or os.environ.get("NS3D_BENCH_BACKEND") == "gloo" or ndev < world
    device = local_rank % ndev
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("gloo")             # control plane; the data plane is libns3d's RCCL communicator

    from navierstokes3d_amd import build
    if rank == 0:
        build.build()
    if world > 1:
        dist.barrier()
    from navierstokes3d_amd.params import cavity_params

    p = cavity_params(a.n, a.nz)
    if a.scaling == "strong" and world > 1:
        p = strong_params(a.n, p.nz, world)
    head = run_case(a, world, rank, device, ndev, shared_gpu, p, a.scaling, dump=a.dump_outputs)
    strong = None
    if a.full and not a.no_strong and a.scaling == "weak":
        # BASELINE.json's metric reads "512³ grid, 1/2/4/8 MI355X": the same GLOBAL grid split in z, next to the weak headline
        if world == 1:
            strong = strong_object(head, world)
        else:
            strong = strong_object(run_case(a, world, rank, device, ndev, shared_gpu, strong_params(a.n, p.nz, world), "strong"), world)
    config_b = None
    if world == 1 and a.full and not a.no_config_b:
        config_b = config_b_object(a, device, ndev, shared_gpu)
    ok = True
    if rank == 0:
        out = json_line(a, world, head)
        if strong is not None:
            out["strong"] = strong
        if world == 1 and config_b is not None:
            out["config_b"] = config_b
        if world == 1 and a.full and not a.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(a.n, 128, a.cpu_iters, a.dtype)
            except Exception as e:  # the baseline is a report, never a reason to lose the GPU number
                out["cpu_baseline"] = {"value": None, "unit": "Mcells*iter/s", "cores": 0, "kind": "port",
                                       "sample": "failed: %r" % (e,)}
        print(json.dumps(out))
        ok = out["config"]["verified"] is not False and (strong is None or strong.get("verified") is not False)
        if config_b is not None:        # the reference's own grid is part of the gate too: a failed self-check there exits 3 as well
            ok = ok and all(v.get("verified") is not False for v in config_b.values() if isinstance(v, dict))
    if world > 1:
        ok = agree(ok)
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        sys.stderr.write("bench.py: the timed kernel / schedule did NOT reproduce the single-sweep reference (config.verified)\n")
        sys.exit(3)


def config_b_object(a, device, ndev, shared_gpu):
    """BASELINE's north_star asks for the 255×153×153 cylinder case next to the synthetic grids: the same Poisson-only measurement
    (∇V synthetic, Pr = dPrdτ = 0, all-Neumann) on the reference's own grid and SPACINGS (multi.jl:322-341 for nx = 255: dx = 1/255 …
    — not powers of two, so STRICT takes the exact-division build), in STRICT and in FAST mode (the product mode on such grids:
    within 1e-6, identical iteration counts), each self-verified like the headline.  A report beside the headline, never a reason
    to lose it."""
    import argparse
    out = {"workload": "Poisson-only PT iteration on the grid and spacings of the reference's cylinder case (BASELINE configs[1], "
                       "multi.jl nx = 255)", "unit": "Mcells*iter/s"}
    try:
        from navierstokes3d_amd.params import multi_params
        p = multi_params(255)
        out["grid"] = [p.nx, p.ny, p.nz]
        for mode in ("strict", "fast"):
            b = argparse.Namespace(**vars(a))
            b.mode, b.steps, b.warmup = mode, max(a.steps, 240), max(a.warmup, 24)
            b.depth, b.variant, b.variant2, b.variantn, b.no_temporal_blocking = 0, 0, None, None, False
            r = run_case(b, 1, 0, device, ndev, shared_gpu, p, "weak")
            itemsize = 8 if a.dtype == "f64" else 4
            kern_ms = r["dev_ms"] / r["launches"]
            out[mode] = {"value": r["value"], "ms_per_step": r["ms_per_step"], "steps": b.steps, "pt_depth": r["depth"],
                         "arith_build": r["arith_build"], "pt2_variant": r["pt2_variant"], "ptn_variant": r["ptn_variant"],
                         "verified": r["verified"], "finite": r["finite"],
                         "roofline_frac": algorithmic_bytes(p.nx, p.ny, p.nz, itemsize) / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                         "hbm_gbps_algorithmic": r["effective"]}
    except Exception as e:
        out["error"] = repr(e)
    return out


def strong_params(n, nz_g, world):
    """Global grid n x n x nz_g split into `world` z-slabs of ImplicitGlobalGrid's shape nz_g = P*(nz_loc-2)+2: the smallest
    local slab whose global grid is not smaller than the one asked for (512³ on 4: 130 planes each → 514; on 8: 66 → 514)."""
    from navierstokes3d_amd.params import cavity_params
    nz_loc = -(-(nz_g - 2) // world) + 2
    p = cavity_params(n, nz_loc)
    p.dz = p.dx
    return p


def strong_object(r, world):
    return {"value": r["value"], "unit": "Mcells*iter/s", "ms_per_step": r["ms_per_step"], "scaling": "strong",
            "global_grid": r["global_grid"], "planes_per_rank": r["local_grid"][2], "pt_depth": r["depth"],
            "ptn_variant": r["ptn_variant"], "pt2_variant": r["pt2_variant"], "transport": r["transport"],
            "hbm_gbps_algorithmic": r["effective"] * world, "verified": r["verified"], "verify": r["verify"],
            "finite": r["finite"]}


def dump_outputs(out_dir, fields):
    """--dump-outputs: each field as out_dir/<name>.npy in the run's element type — the whole array in column-major (Fortran)
    order up to DUMP_SAMPLE values, beyond that the values at DUMP_SAMPLE column-major positions drawn without replacement from a
    generator seeded by the array's size, in increasing order, so that two runs (or two builds) with the same arguments write
    the same positions."""
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    for name, t in fields.items():
        n = t.numel()
        if n <= DUMP_SAMPLE:
            v = np.asfortranarray(t.permute(2, 1, 0).cpu().numpy().transpose(2, 1, 0))
        else:
            idx = np.sort(np.random.Generator(np.random.MT19937(n)).choice(n, DUMP_SAMPLE, replace=False))
            flat = t.permute(2, 1, 0).reshape(-1)             # (nx,ny,nz) with strides (1,nx,nx*ny): a view, column-major
            v = flat[torch.from_numpy(idx).to(t.device)].cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), v)


def run_case(a, world, rank, device, ndev, shared_gpu, p, scaling, dump=None):
    """One timed measurement: plan (untimed), W warm-up iterations, EXACTLY K timed iterations between barriers + device
    synchronisation, the outputs to `dump` if given, then (--full) the untimed self-check.  Returns a dict on every rank
    (timings are the maximum over ranks)."""
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.halo import ZSlabGrid
    nx, ny, nz = p.nx, p.ny, p.nz
    tdt = torch.float64 if a.dtype == "f64" else torch.float32
    dev = torch.device("cuda", device)

    # ---- transport of the z-slab ranks, agreed collectively ---------------------------------------------------
    mg, transport, rccl_ranks = None, None, 0
    if world > 1:
        want = "host" if (shared_gpu and a.transport == "auto") else a.transport
        reason = "%d ranks share %d device(s)" % (world, ndev) if shared_gpu else "requested"
        if want in ("auto", "rccl"):
            mg, why = bring_up_rccl(world, rank, device, nx, ny, nz, a.mode, tdt)
            if mg is None:
                if want == "rccl":
                    raise SystemExit("bench.py --transport rccl: " + why)
                reason = why
        if mg is not None:
            transport, rccl_ranks = "RCCL send/recv over xGMI inside libns3d (ns3d_mgpu_create_rank)", mg.rccl_ranks()
            if os.environ.get("NS3D_RCCL_LIB"):
                transport += " [NS3D_RCCL_LIB=%s]" % os.path.basename(os.environ["NS3D_RCCL_LIB"])
        else:
            transport = "host-staged over gloo (%s)" % reason[:200]
    if mg is not None:
        ctx = mg.contexts[0]
    else:
        ctx = K.Context(device, a.mode, async_=True)
    ctx.set_pt_variant(a.variant)
    if a.variant2 is not None:
        ctx.set_pt2_variant(a.variant2)
    if a.variantn is not None:
        ctx.set_ptn_variant(a.variantn)
    if a.depth > 0:
        ctx.set_pt_depth(a.depth)
    if a.no_autotune:
        ctx.set_autotune(False)
    knobs = {"reserved_cus": 0, "interior_chunks": 1}

    def set_overlap_knobs(cus, chunks):
        """the compute launches leave `cus` CUs to the exchange's kernels (include/ns3d.h ns3d_reserve_cus) — from then on this process's
        torch work and timing events go to the same CU-masked stream — and the interior sweep of a z-slab pass runs in `chunks` launches"""
        torch.cuda.synchronize()
        if cus != knobs["reserved_cus"]:
            if cus > 0:
                st_masked = (mg.reserve_cus(cus) if mg is not None else [ctx.reserve_cus(cus)])[0]
                torch.cuda.set_stream(st_masked)
            else:                                   # back to PyTorch's default stream BEFORE the masked one is destroyed
                torch.cuda.set_stream(torch.cuda.default_stream(dev))
                (mg.reserve_cus(0) if mg is not None else ctx.reserve_cus(0))
            knobs["reserved_cus"] = cus
        if mg is not None and chunks != knobs["interior_chunks"]:
            mg.set_interior_chunks(chunks)
            knobs["interior_chunks"] = chunks

    set_overlap_knobs(a.reserve_cus, max(1, a.interior_chunks))
    grid = ZSlabGrid(nx, ny, nz, transport="host") if world > 1 else ZSlabGrid(nx, ny, nz)

    # synthetic right-hand side ∇V = U(-1e-3,1e-3), seeded per rank; Pr = dPrdτ = 0 (SURVEY §8d Config 3)
    gen = torch.Generator(device=dev); gen.manual_seed(12345 + rank)
    Pr = K.zeros((nx, ny, nz), tdt, dev)
    Pb = K.zeros((nx, ny, nz), tdt, dev)
    D = K.zeros((nx - 2, ny - 2, nz - 2), tdt, dev)
    rhs = K.zeros((nx, ny, nz), tdt, dev)
    rhs.permute(2, 1, 0).uniform_(-1e-3, 1e-3, generator=gen)
    pt = K.pt_params(Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI, False, 0.0, 0.0,
                     grid.z_lo_is_halo(), grid.z_hi_is_halo())

    depth = 1 if a.no_temporal_blocking else (a.depth if a.depth > 0 else 2)      # PT iterations per pass over memory
    use2 = (world == 1) and depth >= 2
    slab = None
    if mg is not None:                              # the whole schedule inside libns3d: ns3d_slab_load / _plan / _iterate
        mg.set_temporal(1 if a.no_temporal_blocking else 4)
        mg.update_halo(rhs)                         # update_halo!(∇V), multi.jl:455: the seam planes of the RHS agree
        mg.slab_load(Pr, D, rhs, pt)
        depth = mg.slab_plan()                      # plan phase, untimed: tile shapes and iterations per pass (all ranks agree)
        # Still the plan phase: how the exchange shares the chip with the interior sweep is a property of the node (RCCL's kernels need
        # CUs; the sweep holds them all), measured here by all ranks together instead of guessed — VERDICT r3 weak #5
        if a.overlap_trial == "auto" and a.reserve_cus == 0 and a.interior_chunks <= 1:
            cands, took = [(0, 1), (0, 2), (8, 1)], []
            for cus, chunks in cands:
                set_overlap_knobs(cus, chunks)
                mg.slab_load(Pr, D, rhs, pt)
                d = mg.slab_plan()
                mg.slab_iterate(2 * d)
                torch.cuda.synchronize(); dist.barrier()
                t0 = time.perf_counter()
                mg.slab_iterate(6 * d)
                torch.cuda.synchronize()
                t = torch.tensor([(time.perf_counter() - t0) / (6 * d) * 1e3], dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                took.append(float(t.item()))
            best = min(range(len(cands)), key=lambda q: took[q])      # the same list on every rank: the same choice
            set_overlap_knobs(*cands[best])
            mg.slab_load(Pr, D, rhs, pt)            # the trial's iterations are not part of the run: start over from the inputs
            depth = mg.slab_plan()
            knobs["trial"] = {"candidates_cus_chunks": [list(c) for c in cands], "ms_per_iteration": took, "chosen": list(cands[best])}
    elif world > 1:
        from navierstokes3d_amd.slab import SlabPTSolver
        grid.update_halo(rhs)
        slab = SlabPTSolver(ctx, grid, Pr, p.rho, p.dt, p.dtau, p.damp, p.dx, p.dy, p.dz, L.NS3D_BC_MULTI, False, 0.0, 0.0)
        depth = 2 if depth >= 2 else 1              # the torch.distributed schedule blocks two iterations at most
        slab.set_temporal_blocking(depth == 2)
        slab.load(Pr, D, rhs)
    D2 = K.zeros((nx - 2, ny - 2, nz - 2), tdt, dev) if use2 else None
    st = {"Pr": Pr, "Pb": Pb, "D": D, "D2": D2}

    def schedule(n):
        """the passes ns3d_pt_iterate makes for n iterations at `depth` iterations per pass (4 = 2+2, not 3+1)"""
        out = []
        while n > 0:
            if depth < 2 or n < 2:
                its = 1
            elif n >= depth:
                its = depth - 1 if (n == depth + 1 and depth >= 3) else depth
            else:
                its = 3 if n >= 3 else 2
            out.append(its)
            n -= its
        return out

    def run(n):
        """n PT iterations {update_dPrdτ!; update_Pr!; set_bc_Pr!}.  One GPU: what ns3d_pt_iterate does, with the buffer
        swaps visible (`depth` iterations per pass over memory where n allows).  z-slab ranks: seam planes first, their
        exchange behind the interior sweep."""
        if mg is not None:
            mg.slab_iterate(n)
            return
        if slab is not None:
            slab.iterate(n)
            return
        for its in schedule(n):
            if its == 1:
                K.pt_sweep(st["Pr"], st["Pb"], st["D"], rhs, pt, 1, nz - 1, ctx=ctx)
                st["Pr"], st["Pb"] = st["Pb"], st["Pr"]
                continue
            if its == 2:
                K.pt_sweep2(st["Pr"], st["Pb"], st["D"], st["D2"], rhs, pt, ctx=ctx)
            else:
                K.pt_sweepn(its, st["Pr"], st["Pb"], st["D"], st["D2"], rhs, pt, ctx=ctx)
            st["Pr"], st["Pb"], st["D"], st["D2"] = st["Pb"], st["Pr"], st["D2"], st["D"]

    # plan phase, untimed and outside the warmup count: ns3d_plan_pt times the tile shapes of k_pt_sweep2 / k_pt_sweepN on
    # these arguments, decides how many iterations a pass advances, and the process keeps the winner (same bits either way)
    if use2 and not a.no_autotune:
        K.plan_pt(st["Pr"], st["Pb"], st["D"], st["D2"], rhs, pt, ctx=ctx)
        depth = ctx.last_pt_depth() if a.depth <= 0 else a.depth
        st["Pb"].zero_(); st["D2"].zero_()
        torch.cuda.synchronize()
    run(a.warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    run(a.steps)
    ev1.record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    if world > 1:
        t = torch.tensor([wall, dev_ms], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, dev_ms = t[0].item(), t[1].item()
    if dump is not None:
        dump_outputs(dump, {"Pr": st["Pr"], "dPrdtau": st["D"]})
    if mg is not None:
        err = mg.slab_residual()
    elif slab is not None:
        err = slab.residual()
    else:
        err = K.residual_max(st["Pr"], rhs, pt, ctx=ctx)
    err = err * (p.ly * p.ly) / p.psc
    passes = schedule(a.steps)

    # ---- self-check, untimed: the timed kernel instance / schedule against one-thread-per-cell single sweeps ---------------
    # One GPU: ONE pass of exactly the kernel that was timed (same depth, same tile variant) from the state the run left
    # behind, against `depth` launches of k_pt_sweep_naive (multi.jl:459-463, one launch per iteration).  z-slab ranks: one
    # pass of the library's schedule (deep ghosts, seam-first, exchange behind the interior) against `depth` × {single sweep;
    # update_halo!(Pr)} — the reference's own per-iteration sequence, multi.jl:459-463.  STRICT: bit for bit on the device.
    verify = {"against": None, "iterations": 0, "bitwise": None, "rel_l2": None}
    verified = None
    if a.full and not a.no_verify:
        vd = max(passes) if passes else 0
        if vd >= 1:
            vctx = ctx
            if world == 1:
                P0, D0 = st["Pr"], st["D"]
                Pa, Da = st["Pb"], (st["D2"] if st["D2"] is not None else K.clone(D0))
                if vd == 1:
                    Da = K.clone(D0)
                    K.pt_sweep(P0, Pa, Da, rhs, pt, 1, nz - 1, ctx=ctx)
                elif vd == 2:
                    K.pt_sweep2(P0, Pa, D0, Da, rhs, pt, ctx=ctx)
                else:
                    K.pt_sweepn(vd, P0, Pa, D0, Da, rhs, pt, ctx=ctx)
                halo = lambda X: None
                verify["against"] = "%d launches of the one-thread-per-cell sweep (k_pt_sweep_naive)" % vd
            else:
                P0, D0 = K.zeros((nx, ny, nz), tdt, dev), K.zeros((nx - 2, ny - 2, nz - 2), tdt, dev)
                Pa, Da = K.zeros((nx, ny, nz), tdt, dev), K.zeros((nx - 2, ny - 2, nz - 2), tdt, dev)
                (mg.slab_store if mg is not None else slab.store)(P0, D0)
                run(vd)
                (mg.slab_store if mg is not None else slab.store)(Pa, Da)
                halo = mg.update_halo if mg is not None else grid.update_halo
                verify["against"] = "%d x {one-thread-per-cell sweep; update_halo!(Pr)} per rank" % vd
            vctx.set_pt_variant(100)
            Pq, Pw, Dq = K.clone(P0), K.clone(P0), K.clone(D0)
            for _ in range(vd):
                K.pt_sweep(Pq, Pw, Dq, rhs, pt, 1, nz - 1, ctx=vctx)
                halo(Pw)
                Pq, Pw = Pw, Pq
            vctx.set_pt_variant(a.variant)
            if os.environ.get("NS3D_BENCH_SABOTAGE") == "1":      # test hook: the check must be able to fail
                Pq[nx // 2, ny // 2, nz // 2] += 1.0
            torch.cuda.synchronize()
            bits = torch.int64 if a.dtype == "f64" else torch.int32
            bitwise = bool(torch.equal(Pa.view(bits), Pq.view(bits)) and torch.equal(Da.view(bits), Dq.view(bits)))
            den = torch.linalg.vector_norm(Pq.double()).item()
            num = torch.linalg.vector_norm((Pa - Pq).double()).item()
            rel = num / den if den > 0 else num
            okv = bitwise if a.mode == "strict" else (rel <= 1e-6 and bool(np.isfinite(rel)))
            if world > 1:
                t = torch.tensor([1.0 if okv else 0.0, 1.0 if bitwise else 0.0, -rel], dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                okv, bitwise, rel = bool(t[0].item()), bool(t[1].item()), -t[2].item()
            verify.update(iterations=vd, bitwise=bitwise, rel_l2=rel,
                          criterion="bitwise" if a.mode == "strict" else "rel_l2 <= 1e-6 (BASELINE north_star tolerance)")
            verified = okv
            del Pq, Pw, Dq
    res = {
        "value": nx * ny * grid.nz_g() * a.steps / wall / 1e6, "wall": wall, "dev_ms": dev_ms,
        "ms_per_step": wall / a.steps * 1e3, "local_grid": [nx, ny, nz], "global_grid": [nx, ny, grid.nz_g()],
        "depth": max(passes) if passes else depth, "launches": len(passes), "err": err, "finite": bool(np.isfinite(err)),
        "pt2_variant": ctx.last_pt2_variant(), "ptn_variant": ctx.last_ptn_variant(), "transport": transport,
        "rccl_ranks": rccl_ranks, "scaling": scaling, "verified": verified, "verify": verify,
        "arith_build": ctx.arith_build(p.dx, p.dy, p.dz), "knobs": dict(knobs),
        "effective": a.steps * algorithmic_bytes(nx, ny, nz, 8 if a.dtype == "f64" else 4) / (dev_ms * 1e-3) / 1e9,
    }
    ctx.sync()
    if knobs["reserved_cus"] > 0:                   # PyTorch's current stream is the context's CU-masked one: leave it before it goes
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    if mg is not None:
        mg.close()
    elif world == 1:
        ctx.close()
    del st, Pr, Pb, D, D2, rhs
    torch.cuda.empty_cache()
    return res

def measure_traffic(a, r):
    """HBM bytes per launch of the kernel instance that was just timed, measured on THIS box: two short child runs of this
    script (same grid, element type, arithmetic mode, pass depth and tile variant; no self-check, no CPU baseline) under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` — separate passes, kernel trace only, the program itself
    after `--`, as MI355X_MICROARCH.md's HBM section prescribes; FETCH_SIZE doubled (gfx950 tallies 128-B read requests at
    64 B), both counters in KiB.  One launch = the sweep kernel + the boundary-cell launches that belong to a pass.  Returns
    (bytes, source) or (None, reason); never raises: the figure is a report, not a reason to lose the bench line."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not on PATH"
    if any("ROCPROF" in k or k.startswith("ROCP_") for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        return None, "already under a profiler"
    depth = r["depth"]
    nx, ny, nz = r["local_grid"]
    args = ["--gpus", "1", "--steps", str(6 * depth), "--warmup", str(depth), "--grid", str(nx), "--grid-nz", str(nz),
            "--mode", a.mode, "--dtype", a.dtype, "--no-cpu-baseline", "--no-verify", "--no-traffic", "--no-strong", "--no-config-b"]
    if depth >= 2:
        args += ["--depth", str(depth)]
        args += ["--variant2", str(r["pt2_variant"])] if depth == 2 else ["--variantn", str(r["ptn_variant"])]
    else:
        args += ["--no-temporal-blocking", "--variant", str(a.variant)]
    per = {}
    work = None
    try:
        work = tempfile.mkdtemp(prefix="ns3d_pmc_")
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(work, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "-f", "csv", "-d", d, "-o", "p", "--",
                   sys.executable, os.path.abspath(__file__)] + args
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=ROOT, timeout=240)
            acc = {}                                    # kernel name -> {dispatch id: counter value summed over its rows}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") != counter:
                        continue
                    k = row["Kernel_Name"].split("(")[0]
                    dd = acc.setdefault(k, {})
                    did = row.get("Dispatch_Id", str(len(dd)))
                    dd[did] = dd.get(did, 0.0) + float(row["Counter_Value"])
            per[counter] = acc
        sweeps = {k: v for k, v in per["FETCH_SIZE"].items() if "k_pt_sweep" in k}
        if not sweeps:
            return None, "no k_pt_sweep dispatch in the counter files"
        main = max(sweeps, key=lambda k: len(sweeps[k]))          # the timed instance: by far the most dispatches
        n = len(sweeps[main])
        tot = {}
        for counter in per:
            t = sum(per[counter].get(main, {}).values())
            t += sum(sum(v.values()) for k, v in per[counter].items() if "k_pt_faces" in k)
            tot[counter] = t / n
        return 2.0 * 1024.0 * tot["FETCH_SIZE"] + 1024.0 * tot["WRITE_SIZE"], \
            "measured on this box: rocprofv3 --pmc FETCH_SIZE (x2, gfx950) / WRITE_SIZE, separate kernel-trace passes, %d launches of %s" % (
                n, main.replace("void ", ""))
    except Exception as e:
        return None, "live measurement failed: %r" % (e,)
    finally:
        if work is not None:
            shutil.rmtree(work, ignore_errors=True)


def json_line(a, world, r):
    nx, ny, nz = r["local_grid"]
    itemsize = 8 if a.dtype == "f64" else 4
    # the dominant kernel: k_pt_sweep2 / k_pt_sweepN advance `depth` iterations per launch (k_pt_sweep: one)
    its_per_launch, launches = r["depth"], r["launches"]
    kern_ms = r["dev_ms"] / launches                 # HIP events around the timed launches on the launch stream
    must_move = algorithmic_bytes(nx, ny, nz, itemsize)          # bytes ONE pass has to move, per launch
    physical = must_move / (kern_ms * 1e-3) / 1e9
    effective = r["effective"]                       # 40 B per cell and iteration
    traffic, traffic_source = None, "N > 1"
    if not a.full:
        traffic_source = "without --full"
    elif a.no_traffic:
        traffic_source = "--no-traffic"
    if world == 1 and a.full and not a.no_traffic:
        traffic, traffic_source = measure_traffic(a, r)
        if traffic is None:
            sys.stderr.write("bench.py: roofline.traffic not measured live (%s); falling back to profiles/\n" % traffic_source)
    tfile = os.path.join(ROOT, "profiles", "pt_sweep_traffic.json")
    if traffic is None and world == 1 and os.path.exists(tfile):
        try:
            tj = json.load(open(tfile))
            key = "%dx%dx%d_%s_%s_x%d" % (nx, ny, nz, a.dtype, a.mode, its_per_launch)
            if its_per_launch >= 2:                         # measured per tile shape (tools/collect_traffic.py)
                key += "_v%d" % (r["pt2_variant"] if its_per_launch == 2 else r["ptn_variant"])
            traffic = tj.get(key, {}).get("hbm_bytes_per_launch")
            traffic_source = "profiles lookup (%s)" % traffic_source if traffic is not None else "none"
        except Exception:
            traffic = None
    if traffic is None:
        traffic_source = "none"
    return {
        "metric": "Mcells*PT-iter/s, fused pseudo-transient Poisson iteration, %dx%dx%d per GPU" % (nx, ny, nz),
        "value": r["value"],
        "unit": "Mcells*iter/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": r["ms_per_step"],
        "higher_is_better": True, "scaling": r["scaling"], "vs_baseline": None,
        "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": "lid-driven-cavity Poisson-only PT iteration (BASELINE configs[2])",
                   "local_grid": r["local_grid"], "global_grid": r["global_grid"],
                   "decomposition": "z-slabs x%d" % world,
                   "transport": r["transport"], "rccl_ranks": r["rccl_ranks"],
                   "reserved_cus": r["knobs"]["reserved_cus"], "interior_chunks": r["knobs"]["interior_chunks"],
                   "overlap_trial": r["knobs"].get("trial"),
                   "arith_mode": a.mode, "arith_build": r["arith_build"], "variant": a.variant,
                   "pt_depth": its_per_launch, "pt2_variant": r["pt2_variant"],
                   "ptn_variant": r["ptn_variant"], "residual_after_run": r["err"], "finite": r["finite"],
                   "verified": r["verified"], "verify": r["verify"]},
        "hbm_gbps_algorithmic": effective * world,
        "roofline": {"bound": "hbm", "achieved": physical, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": physical / HBM_PEAK_GBPS,
                     "definition": "bytes one launch must move (one pass: itemsize*(N+4*N_inner)) / launch time / peak",
                     "traffic": traffic, "traffic_source": traffic_source,
                     # what the memory system actually delivered: PMC bytes of a launch / launch time (the overlap rows of
                     # neighbouring tiles are read more than once, so this exceeds `achieved`)
                     "hbm_gbps_measured": (traffic / (kern_ms * 1e-3) / 1e9) if traffic is not None else None,
                     "hbm_frac_measured": (traffic / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if traffic is not None else None,
                     "kernel": {1: "k_pt_sweep", 2: "k_pt_sweep2"}.get(its_per_launch, "k_pt_sweepN<%d levels>" % its_per_launch),
                     "kernel_ms": kern_ms,
                     "pt_iterations_per_launch": its_per_launch, "bytes_per_launch": must_move,
                     "effective_gbps": effective, "effective_frac": effective / HBM_PEAK_GBPS,
                     "effective_definition": "SURVEY 8d: 40 B per cell and PT ITERATION (itemsize*(N+4*N_inner) per "
                                             "iteration) / time / peak; exceeds frac by the temporal-blocking factor"},
    }


if __name__ == "__main__":
    main()
