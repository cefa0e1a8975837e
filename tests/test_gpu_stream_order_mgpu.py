"""Stream order of the multi-GPU half of the C ABI (navierstokes3d_amd.mgpu → csrc/ns3d_mgpu.cpp) on P virtual ranks of device 0:
every entry point with inputs that arrive LATE on the streams the ranks compute on, and a reader and an overwrite that follow EARLY
on them (tests/stream_order.py has the technique; tests/mgpu_cases.py the calls).  Nothing is synchronised between the copy-in, the
call and the reader, so the only things that order one rank's planes against its neighbours' pulls are the three event edges of
exchange_begin / exchange_end:

  1. a receiver's communication stream waits for the SENDER's ev_ready      — seen when one rank alone is late: its on-time
     neighbours would pull the decoy's planes;
  2. a receiver's compute stream waits for its own ev_landed               — seen by the early reader on that rank's stream;
  3. a sender's compute stream waits for the RECEIVER's ev_landed          — seen through the late overwrite: the sender's decoy,
     written right behind the call, must not reach its neighbour's halo.

Two stream set-ups, those of rank_streams in tests/test_gpu_mgpu.py: "follow" (all ranks on one non-default stream S, the call made
inside `with torch.cuda.stream(S)`; only the communication streams are concurrent) and "own" (a non-blocking compute stream per rank).
Which edges a family exercises: every family but gather, diagnostics and tracers_advance (no exchange between ranks: they check that
each rank's work is on its own stream) exercises all three in "own"; in "follow" edge 3 and the compute side of edge 1 are implied
by the shared stream and edges 1 (communication stream behind S) and 2 remain.  The families that call twice (update_halo twice,
advect_wide twice, the chain) and the loops (slab, pt_solve_slab) re-record every event and reuse hbuf / wbuf / bbuf / the slab state
within one window.

Expected bits: the same call on a fresh MultiGpu of the same topology made the way the value tests make it (synchronised on both
sides), which those tests tie to the oracle's virtual ranks or to the global solve.  Bit equality; no tolerance.  A case whose
canary does not hold the decoy FAILS ("proves nothing").  More than three ranks get streams of their own in one case only (the
four-rank slab): with four hardware queues an on-time rank may queue behind a late one, which weakens a run but cannot make it pass
wrongly."""
import numpy as np
import pytest
import torch

import mgpu_cases as MC
import stream_order as SO

pytestmark = pytest.mark.gpu

SETUPS = ["follow", "own"]
OWN_MAX_P = 3                   # … apart from the four-rank slab


@pytest.fixture(scope="module")
def delay(hip):
    d = SO.Delay()
    print("stream-order delay: %.1f ms = %d in-place adds of %.4f ms on %d MiB" % (d.ms, d.n, d.op_ms, SO.DELAY_BYTES >> 20))
    return d


def run_spec(hip, spec, setup, delay, cold=False, variants=("reader", "sync")):
    """expected bits, then for every late set and variant: warm-up and measured run on an asynchronous MultiGpu of `setup`.  cold:
    the warm-up is made on ANOTHER MultiGpu and every measured call is the first on a fresh one — the lazy buffers grow (and
    synchronise every rank) inside the window, so the canary is taken before the call."""
    case = spec.rank_case(blocking=True if cold else None)
    (want_r, want), (dec_r, dec) = SO.expected_ranks(hip, case, setup == "own")
    msgs = []
    mg = None
    for late in SO.late_sets(case.P, setup):
        for v in variants:
            if mg is None or cold:
                if mg is not None:
                    mg.sync()
                    mg.close()
                if cold:
                    other, _, under = SO.grid_on(hip, case, setup)
                    SO.warm_up_ranks(hip, case, other, under)
                    other.close()
                mg, streams, under = SO.grid_on(hip, case, setup)
                if not cold:
                    SO.warm_up_ranks(hip, case, mg, under)
            r, got, can = SO.measured_ranks(hip, case, mg, streams, delay, late, v, under=under)
            what = "%s%s, %s, late %s, %s" % (case.name, " (cold)" if cold else "", setup, sorted(late), v)
            msgs += SO.verdict_ranks(what, got, want, dec, can, case.decoy, late, r, want_r, dec_r)
    mg.sync()
    mg.close()
    return msgs


def _rows():
    out = []
    for dt in MC.DTS:
        for family, spec in MC.table(dt):
            P = SO.topo_of(spec.topo)[1]
            for setup in SETUPS:
                if setup == "own" and P > OWN_MAX_P and family != "slab":
                    continue
                out.append(pytest.param(spec, setup, id="%s-%s" % (spec.name.replace(" ", "_").replace("/", "_"), setup)))
    return out


@pytest.mark.parametrize("spec,setup", _rows())
def test_multi_rank_call(hip, delay, spec, setup):
    msgs = run_spec(hip, spec, setup, delay)
    assert not msgs, "\n".join(msgs)


def _cold_rows():
    out = []
    for dt in MC.DTS:
        for spec in (MC.halo_case(((2, 2, 2), (13, 9, 7)) if dt == "f64" else ((2, 1, 1), (70, 6, 7)), dt), MC.halo_case((3, (13, 9, 7)), dt),
                     MC.advect_case(2, 9, 1.9, True, dt), MC.slab_case((2, (40, 21, 10)), 2, 7, dt)):
            for setup in SETUPS:
                if setup == "own" and SO.topo_of(spec.topo)[1] > OWN_MAX_P:
                    continue
                out.append(pytest.param(spec, setup, id="%s-%s" % (spec.name.replace(" ", "_").replace("/", "_"), setup)))
    return out


@pytest.mark.parametrize("spec,setup", _cold_rows())
def test_first_call_on_a_fresh_grid(hip, delay, spec, setup):
    """update_halo, advect_wide and slab_load as the FIRST call on a MultiGpu: hbuf / wbuf / the slab state are allocated inside the
    window, behind the queued delay"""
    msgs = run_spec(hip, spec, setup, delay, cold=True)
    assert not msgs, "\n".join(msgs)


# ---- negative controls and the synchronous promise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", SETUPS)
def test_negative_control(hip, delay, setup):
    """The harness sees a misordered exchange: rank 0's delay and copy-in go on a stream the grid does NOT follow, so the exchange
    runs at once and rank 1 pulls rank 0's DECOY plane into its halo.  The verdict must name rank 1 and say that its arrays are
    neither the expected bits nor the decoy run's — and they must be exactly what a run with rank 0's decoy and rank 1's real set
    gives."""
    spec = MC.halo_case((2, (13, 9, 7)), "f64")
    case = spec.rank_case(blocking=True, name=spec.name + " (control)")      # the canary BEFORE the call
    (want_r, want), (_, dec) = SO.expected_ranks(hip, case, setup == "own")
    mg, streams, under = SO.grid_on(hip, case, setup)
    mixed_r, mixed = SO.sync_run_ranks(hip, case, mg, [case.decoy[0], case.real[1]])
    SO.warm_up_ranks(hip, case, mg, under)
    foreign = SO.independent_of_all(streams, delay)                           # the exchange must be FREE to run early
    r, got, can = SO.measured_ranks(hip, case, mg, streams, delay, {0}, "reader", under=under, delay_streams={0: foreign}, overwrite=False)
    mg.sync()
    mg.close()
    msgs = SO.verdict_ranks("control", got, want, dec, can, case.decoy, {0})
    assert not any("proves nothing" in m for m in msgs), msgs
    halo = [k for k in ("c", "vx", "vy", "vz") if any(m.startswith("control, rank 1: %s neither" % k) for m in msgs)]
    assert halo == ["c", "vx", "vy", "vz"], msgs
    assert not any(m.startswith("control, rank 1: s ") or m.startswith("control, rank 1: i ") for m in msgs), msgs
    for k in case.names:
        assert SO.bits_same(got[1][k], mixed[1][k]), k
        if k in halo:                                                        # the decoy's plane, where the real one belongs
            assert not SO.bits_same(got[1][k][:, :, 0], want[1][k][:, :, 0]) and SO.bits_same(got[1][k][:, :, 1:], want[1][k][:, :, 1:]), k


@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("family", ["update_halo", "advect_wide"])
def test_synchronous_promise(hip, delay, family, setup):
    """A MultiGpu WITHOUT NS3D_ASYNC: the call itself waits for every rank's streams, so any stream may read every rank's outputs
    the moment it returns."""
    spec = MC.halo_case((3, (13, 9, 7)), "f64") if family == "update_halo" else MC.advect_case(2, 9, 1.9, True, "f64")
    case = spec.rank_case(blocking=True, name=spec.name + " (blocking grid)")
    (want_r, want), (dec_r, dec) = SO.expected_ranks(hip, case, setup == "own")
    mg, streams, under = SO.grid_on(hip, case, setup, async_=False)
    SO.warm_up_ranks(hip, case, mg, under)
    late = SO.late_sets(case.P, setup)[0]
    r, got, can = SO.measured_ranks(hip, case, mg, streams, delay, late, "return", under=under)
    mg.close()
    msgs = SO.verdict_ranks(case.name + ", " + setup, got, want, dec, can, case.decoy, late, r, want_r, dec_r)
    assert not msgs, "\n".join(msgs)


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def _driver_run():
    from navierstokes3d_amd import kernels as K
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    p0 = multi_params(24)
    mg = MultiGpu.create([0, 0], p0.nx, p0.ny, p0.nz, "strict", own_streams=True)
    out = run_navierstokes3D(nx=24, nt=2, mode="strict", faithful=True, grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), return_info=True)
    info = out[-1]
    arrays = list(out[:5]) + [K.to_numpy(getattr(f, n)) for f in info.local_fields for n in ("C", "Pr", "Vx", "Vy", "Vz", "divV", "dPrdtau")]
    mg.sync()
    mg.close()
    return arrays, info


def test_driver_on_two_ranks_inside_a_side_stream(hip):
    """run_navierstokes3D(nx=24, nt=2, faithful=True) on a two-rank MgpuGrid with a compute stream per rank, inside `with
    torch.cuda.stream(S)`: gathered fields, every rank's local fields, iteration counts and residual histories are those of the same
    run on the default stream — the driver's torch work on S and the ranks' asynchronous steps order themselves"""
    torch.cuda.synchronize()
    want, winfo = _driver_run()
    S = torch.cuda.Stream(0)
    with torch.cuda.stream(S):
        got, ginfo = _driver_run()
    S.synchronize()
    assert len(got) == len(want) == 5 + 2 * 7 and max(winfo.iters) > 0
    for q, (a, b) in enumerate(zip(got, want)):
        assert SO.bits_same(np.asarray(a), np.asarray(b)), q
    assert SO.same_result(ginfo.iters, winfo.iters), (ginfo.iters, winfo.iters)
    assert SO.same_result(ginfo.errs, winfo.errs)
