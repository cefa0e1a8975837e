"""GPU tests of ns3d_stats_* (include/ns3d.h): the running sums behind the time-averaged fields.

The reference of every test is the header's own expression in NumPy fp64 — S = S + weight·term per slot, with
u = 0.5·(Vx[i]+Vx[i+1]) etc. — computed once per grid and element type and shared.  STRICT must return its bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from util import fields

pytestmark = pytest.mark.gpu

GRIDS = [(3, 3, 3), (17, 9, 5), (65, 5, 3), (1030, 3, 3), (24, 15, 15), (70, 35, 8), (131, 66, 37)]
WEIGHTS = (1.0, 0.3, 3.0)
WSUM = 1.0 + 0.3 + 3.0
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # uu vv ww uv uw vw
NPDT = {"f64": np.float64, "f32": np.float32}


def terms(Vx, Vy, Vz, Pr):
    """the eleven terms of one sample in slot order, fp64 (fp32 fields converted first)"""
    Vx, Vy, Vz, Pr = (np.asarray(a, dtype=np.float64) for a in (Vx, Vy, Vz, Pr))
    u = 0.5 * (Vx[:-1, :, :] + Vx[1:, :, :])
    v = 0.5 * (Vy[:, :-1, :] + Vy[:, 1:, :])
    w = 0.5 * (Vz[:, :, :-1] + Vz[:, :, 1:])
    p = Pr
    return [u, v, w, p, u * u, v * v, w * w, u * v, u * w, v * w, p * p]


def accumulate_ref(S, T, weight):
    return [s + weight * t for s, t in zip(S, T)]


def finalize_ref(S, wsum):
    mean = [S[q] / wsum for q in range(4)]
    rs = [S[4 + q] / wsum - mean[a] * mean[b] for q, (a, b) in enumerate(PAIRS)] + [S[10] / wsum - mean[3] * mean[3]]
    return mean, rs


@functools.lru_cache(maxsize=None)
def case(n, dt):
    """three seeded samples of grid n, their terms, the reference state after them and Σ|weight·term| (never modified)"""
    samples = [fields(*n, ("vx", "vy", "vz", "c"), seed0=10 + 7 * t, dtype=NPDT[dt]) for t in range(3)]
    S = [np.zeros(n) for _ in range(11)]
    mag = [np.zeros(n) for _ in range(11)]
    for F, wgt in zip(samples, WEIGHTS):
        T = terms(*F)
        S = accumulate_ref(S, T, wgt)
        mag = [m + np.abs(wgt * t) for m, t in zip(mag, T)]
    return samples, S, mag


def device_state(hip, n):
    return hip.zeros((n[0], n[1], n[2] * 11), torch.float64)


def run_device(hip, ctx, n, samples, with_pr=True, S=None):
    S = device_state(hip, n) if S is None else S
    for F, wgt in zip(samples, WEIGHTS):
        d = [hip.from_numpy(a) for a in F]
        hip.stats_accumulate(S, d[0], d[1], d[2], d[3] if with_pr else None, wgt, ctx=ctx)
    ctx.sync()
    return S


def slots(hip, S, n):
    a = hip.to_numpy(S) if S.dim() == 3 else S.cpu().numpy().reshape((n[0], n[1], n[2] * 11), order="F")
    return [a[:, :, q * n[2]:(q + 1) * n[2]] for q in range(11)]


@pytest.fixture(scope="module")
def strict(hip):
    c = hip.Context(0, "strict")
    yield c
    c.close()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "%dx%dx%d" % n)
def test_accumulate_matches_numpy_bit_for_bit(hip, strict, n, dt):
    samples, ref, _ = case(n, dt)
    S = device_state(hip, n)
    hip.stats_reset(S, n, ctx=strict)
    got = slots(hip, run_device(hip, strict, n, samples, S=S), n)
    for q in range(11):
        assert np.array_equal(got[q], ref[q]), (q, n, dt)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "%dx%dx%d" % n)
def test_fast_stays_within_the_derived_tolerance(hip, n, dt):
    """|S − S_ref| ≤ (4n+4)·2⁻⁵³·Σₜ|weightₜ·termₜ|, n = 3 samples: each update differs from the uncontracted one by at most the
    roundings of u, the product, the weighting and the sum."""
    samples, ref, mag = case(n, dt)
    ctx = hip.Context(0, "fast")
    got = slots(hip, run_device(hip, ctx, n, samples), n)
    ctx.close()
    worst = 0.0
    for q in range(11):
        bound = (4 * 3 + 4) * 2.0 ** -53 * mag[q]
        err = np.abs(got[q] - ref[q])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
    print("FAST %s %s: worst |S-S_ref| / bound = %.3f" % (n, dt, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_read_only_and_inside_S(hip, strict, dt):
    n = (70, 35, 8)
    N, pad, sent = n[0] * n[1] * n[2], 7, -12345.678
    samples, ref, _ = case(n, dt)
    buf = torch.full((pad + 11 * N + pad,), sent, dtype=torch.float64, device="cuda")
    S = buf[pad:pad + 11 * N]
    hip.stats_reset(S, n, ctx=strict)
    d = [hip.from_numpy(a) for a in samples[0]]
    hip.stats_accumulate(S, *d, WEIGHTS[0], ctx=strict)
    strict.sync()
    host = buf.cpu().numpy()
    assert np.all(host[:pad] == sent) and np.all(host[pad + 11 * N:] == sent)
    for a, t in zip(samples[0], d):
        assert np.array_equal(hip.to_numpy(t), a)
    one = accumulate_ref([np.zeros(n) for _ in range(11)], terms(*samples[0]), WEIGHTS[0])
    got = slots(hip, S, n)
    for q in range(11):
        assert np.array_equal(got[q], one[q]), q
    # Pr = None: slots p and pp are neither read nor written
    S2 = device_state(hip, n)
    hip.stats_reset(S2, n, ctx=strict)
    for q in (3, 10):
        S2[:, :, q * n[2]:(q + 1) * n[2]] = sent
    got = slots(hip, run_device(hip, strict, n, samples, with_pr=False, S=S2), n)
    for q in range(11):
        if q in (3, 10):
            assert np.all(got[q] == sent), q
        else:
            assert np.array_equal(got[q], ref[q]), q


def test_non_finite_values_stay_local(hip, strict):
    n = (17, 9, 5)
    samples, _, _ = case(n, "f64")
    F = [a.copy() for a in samples[0]]
    i, j, k = 6, 4, 2
    F[0][i, j, k] = np.nan
    S = device_state(hip, n)
    hip.stats_reset(S, n, ctx=strict)
    hip.stats_accumulate(S, *[hip.from_numpy(a) for a in F], 1.0, ctx=strict)
    strict.sync()
    got = slots(hip, S, n)
    clean = accumulate_ref([np.zeros(n) for _ in range(11)], terms(*samples[0]), 1.0)
    for q in range(11):
        expect = np.zeros(n, dtype=bool)
        if q in (0, 4, 7, 8):                      # u, uu, uv, uw
            expect[i - 1, j, k] = expect[i, j, k] = True
        assert np.array_equal(np.isnan(got[q]), expect), q
        assert np.array_equal(got[q][~expect], clean[q][~expect]), q


@pytest.mark.parametrize("n", [(17, 9, 5), (131, 66, 37)], ids=lambda n: "%dx%dx%d" % n)
def test_finalize_matches_numpy_bit_for_bit(hip, strict, n):
    from navierstokes3d_amd import lib as L
    samples, ref, _ = case(n, "f64")
    S = run_device(hip, strict, n, samples)
    mean, rs = hip.zeros((n[0], n[1], 4 * n[2]), torch.float64), hip.zeros((n[0], n[1], 7 * n[2]), torch.float64)
    hip.stats_finalize(S, WSUM, mean, rs, n, ctx=strict)
    strict.sync()
    m_ref, r_ref = finalize_ref(ref, WSUM)
    m, r = hip.to_numpy(mean), hip.to_numpy(rs)
    for q in range(4):
        assert np.array_equal(m[:, :, q * n[2]:(q + 1) * n[2]], m_ref[q]), q
    for q in range(7):
        assert np.array_equal(r[:, :, q * n[2]:(q + 1) * n[2]], r_ref[q]), q
    mean2 = hip.zeros((n[0], n[1], 4 * n[2]), torch.float64)
    hip.stats_finalize(S, WSUM, mean2, None, n, ctx=strict)              # rs = NULL
    strict.sync()
    assert np.array_equal(hip.to_numpy(mean2), m)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.Ns3dError, match=r"status 1: ns3d_stats_finalize: wsum"):
            hip.stats_finalize(S, bad, mean2, None, n, ctx=strict)
    assert np.array_equal(hip.to_numpy(mean2), m)


def test_error_paths(hip, strict):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n = (3, 3, 3)
    S = device_state(hip, n)
    d = [hip.from_numpy(a) for a in case(n, "f64")[0][0]]
    P = lambda t: C.c_void_p(t.data_ptr())
    one = C.c_double(1.0)
    acc, h = lib.ns3d_stats_accumulate_f64, strict.handle
    calls = {
        "null context": lambda: acc(None, P(S), P(d[0]), P(d[1]), P(d[2]), P(d[3]), one, 3, 3, 3),
        "null S": lambda: acc(h, None, P(d[0]), P(d[1]), P(d[2]), P(d[3]), one, 3, 3, 3),
        "null Vx": lambda: acc(h, P(S), None, P(d[1]), P(d[2]), P(d[3]), one, 3, 3, 3),
        "grid 2x3x3": lambda: acc(h, P(S), P(d[0]), P(d[1]), P(d[2]), P(d[3]), one, 2, 3, 3),
        "weight nan": lambda: acc(h, P(S), P(d[0]), P(d[1]), P(d[2]), P(d[3]), C.c_double(float("nan")), 3, 3, 3),
        "weight inf": lambda: acc(h, P(S), P(d[0]), P(d[1]), P(d[2]), P(d[3]), C.c_double(float("inf")), 3, 3, 3),
        "reset null S": lambda: lib.ns3d_stats_reset(h, None, 3, 3, 3),
        "reset grid": lambda: lib.ns3d_stats_reset(h, P(S), 3, 2, 3),
        "finalize null mean": lambda: lib.ns3d_stats_finalize(h, P(S), one, None, None, 3, 3, 3),
    }
    for what, call in calls.items():
        assert call() == L.NS3D_ERR_ARG == 1, what
        assert "ns3d_stats_" in L.last_error(), (what, L.last_error())
    # the context is still usable and S untouched
    hip.stats_accumulate(S, *d, 1.0, ctx=strict)
    strict.sync()
    assert np.array_equal(slots(hip, S, n)[0], terms(*case(n, "f64")[0][0])[0])


def _stats_of_states(states):
    """mean and rs of the header's expressions over full local states [(Vx, Vy, Vz, Pr), …], weight 1.0 each"""
    shape = states[0][3].shape
    S = [np.zeros(shape) for _ in range(11)]
    for F in states:
        S = accumulate_ref(S, terms(*F), 1.0)
    return finalize_ref(S, float(len(states)))


def _host_state(hip, info):
    f = info.fields
    return tuple(hip.to_numpy(getattr(f, nm)) for nm in ("Vx", "Vy", "Vz", "Pr"))


def _assert_stats(st, mean, rs, cut):
    from navierstokes3d_amd import stats
    for nm, a in zip(stats.MEAN, mean):
        assert np.array_equal(getattr(st.mean, nm), a[cut]), nm
    for nm, a in zip(stats.RS, rs):
        assert np.array_equal(getattr(st.rs, nm), a[cut]), nm


def test_driver_on_one_rank(hip):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    from util import assert_bit_identical, errs_identical
    kw = dict(nx=24, mode="strict", niter_cap=40, return_info=True)
    plain = {nt: run_navierstokes3D(nt=nt, **kw) for nt in (3, 4, 5, 6)}
    out = run_navierstokes3D(nt=6, statistics=3, **kw)
    assert_bit_identical(out[:5], plain[6][:5])
    assert out[-1].iters == plain[6][-1].iters and errs_identical(out[-1].errs, plain[6][-1].errs)
    assert not hasattr(plain[6][-1], "stats")
    st = out[-1].stats
    assert st.n == 4 and st.wsum == 4.0
    inner = (slice(1, -1),) * 3
    states = {nt: _host_state(hip, plain[nt][-1]) for nt in plain}
    _assert_stats(st, *_stats_of_states([states[nt] for nt in (3, 4, 5, 6)]), inner)
    assert st.mean.U.shape == out[1].shape and np.abs(st.mean.U).max() > 0 and np.abs(st.rs.uu).max() > 0
    st2 = run_navierstokes3D(nt=6, statistics=3, stats_every=2, **kw)[-1].stats
    assert st2.n == 2
    _assert_stats(st2, *_stats_of_states([states[3], states[5]]), inner)
    # the call-by-call step samples the same states
    st3 = run_navierstokes3D(nt=6, statistics=3, one_call=False, **kw)[-1].stats
    _assert_stats(st3, *_stats_of_states([states[nt] for nt in (3, 4, 5, 6)]), inner)
    # runme: the full local arrays
    gkw = dict(nx=24, mode="strict", niter_cap=40)
    gplain = {nt: runme(nt=nt, **gkw) for nt in (2, 3, 4)}
    f, info = runme(nt=4, statistics=2, **gkw)
    for nm in ("Pr", "C", "Vx", "Vy", "Vz"):
        assert np.array_equal(hip.to_numpy(getattr(f, nm)), hip.to_numpy(getattr(gplain[4][0], nm)), equal_nan=True), nm
    assert info.iters == gplain[4][1].iters and errs_identical(info.errs, gplain[4][1].errs)
    assert info.stats.n == 3
    gstates = [tuple(hip.to_numpy(getattr(gplain[nt][0], nm)) for nm in ("Vx", "Vy", "Vz", "Pr")) for nt in (2, 3, 4)]
    _assert_stats(info.stats, *_stats_of_states(gstates), (slice(None),) * 3)
    assert info.stats.mean.P.shape == gstates[0][3].shape


def test_driver_on_two_virtual_z_slab_ranks(hip):
    """P = 2 z-slab ranks on one device with the wide advection halo reproduce the one-rank run's fields bit for bit; the gathered
    statistics must too."""
    from navierstokes3d_amd import stats
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    from util import assert_bit_identical
    nx, nt, P, nz_loc = 36, 3, 2, 12
    one = run_navierstokes3D(nx=nx, nt=nt, mode="strict", return_info=True, statistics=2)
    assert one[-1].params.nz == P * (nz_loc - 2) + 2
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        two = run_navierstokes3D(nx=nx, nt=nt, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), return_info=True,
                                 shape=dict(nz=nz_loc), wide_advect_halo=True, statistics=2)
        assert_bit_identical(two[:4], one[:4], ("C", "Pr", "Vx", "Vy"))
        a, b = one[-1].stats, two[-1].stats
        assert a.n == b.n == 2
        for nm in stats.MEAN:
            x, y = getattr(a.mean, nm), getattr(b.mean, nm)
            assert x.shape == y.shape == (34, 20, 20) and np.array_equal(x, y), nm
        for nm in stats.RS:
            assert np.array_equal(getattr(a.rs, nm), getattr(b.rs, nm)), nm
        assert np.abs(a.mean.U).max() > 0
    finally:
        mg.sync()
        mg.close()
