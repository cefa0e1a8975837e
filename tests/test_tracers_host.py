"""CPU tests of the tracer / probe contract: the vectorised NumPy reference (tests/tracers_ref.py) against an independent scalar-loop
restatement of include/ns3d.h, the points where the definition decides something, the host side of navierstokes3d_amd/tracers.py,
and the boundary (header, binding, export list).  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import tracers_ref as TR
from util import bits_equal, fields, first_bit_difference, hostile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(3, 3, 3), (17, 9, 5)]
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


# ---- the definition once more, one particle at a time, in Python floats (IEEE double, never contracted) ----------------------
def s_lerp(a, b, t):
    return b * t + a * (1.0 - t)


def s_axis(p, stag, ext):
    c = p - (0.0 if stag else 0.5)
    if not c > 0.0:
        c = 0.0
    if not c < ext - 1.0:
        c = ext - 1.0
    i0 = min(int(math.floor(c)), ext - 2)
    return i0, c - i0


def s_interp(A, stag, p):
    (i, tx), (j, ty), (k, tz) = (s_axis(p[q], stag[q], A.shape[q]) for q in range(3))
    a = lambda di, dj, dk: float(A[i + di, j + dj, k + dk])
    fy1z1 = s_lerp(a(0, 0, 0), a(1, 0, 0), tx)
    fy1z2 = s_lerp(a(0, 0, 1), a(1, 0, 1), tx)
    fy2z1 = s_lerp(a(0, 1, 0), a(1, 1, 0), tx)
    fy2z2 = s_lerp(a(0, 1, 1), a(1, 1, 1), tx)
    return s_lerp(s_lerp(fy1z1, fy2z1, ty), s_lerp(fy1z2, fy2z2, ty), tz)


def s_inside(p, hi):
    return all(math.isfinite(p[q]) and 0.0 <= p[q] <= float(hi[q]) for q in range(3))


def s_velocity(V, p):
    return [s_interp(V[0], (1, 0, 0), p), s_interp(V[1], (0, 1, 0), p), s_interp(V[2], (0, 0, 1), p)]


def s_mul(a, b):
    """IEEE product of two doubles (Python raises nothing for float*float, Inf*0 is NaN)"""
    return a * b


def s_advance(X, state, V, c):
    n = (V[0].shape[0] - 1, V[0].shape[1], V[0].shape[2])
    Xn, sn, U = X.copy(), np.zeros_like(state), np.full(X.shape, np.nan)
    for m in range(X.shape[1]):
        p = [float(X[q, m]) for q in range(3)]
        if state[m] != 1 or not s_inside(p, n):
            continue
        v1 = s_velocity(V, p)
        xm = [p[q] + 0.5 * s_mul(v1[q], c[q]) for q in range(3)]
        if all(math.isfinite(x) for x in xm):
            v2 = s_velocity(V, xm)
            xm = [p[q] + s_mul(v2[q], c[q]) for q in range(3)]
        U[:, m] = v1
        Xn[:, m] = xm
        sn[m] = 1 if s_inside(xm, n) else 0
    return Xn, sn, U


def s_sample(A, X, state, stag):
    hi = [A.shape[q] - stag[q] for q in range(3)]
    out = np.full(X.shape[1], np.nan)
    for m in range(X.shape[1]):
        p = [float(X[q, m]) for q in range(3)]
        if (state is None or state[m] == 1) and s_inside(p, hi):
            out[m] = s_interp(A, stag, p)
    return out


def _points(n, N=200, seed=7):
    X, st = TR.planted_points(n)
    U = TR.uniform_points(n, N - min(N, 40), seed)
    return np.ascontiguousarray(np.concatenate([U, X[:, :40]], axis=1)), np.concatenate([np.ones(U.shape[1], np.uint8), st[:40]])


# ---- 1. the vectorised reference is the scalar definition ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_reference_equals_the_scalar_restatement(n, dtype):
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=dtype)
    X, state = _points(n)
    assert X.shape[1] == 200
    for c in ((0.4, 0.36, 0.32), (2.5, 2.25, 2.0)):
        got, want = TR.advance(X, state, *V, c), s_advance(X, state, V, c)
        for g, w, nm in zip(got, want, ("X", "state", "U")):
            if nm == "state":
                assert np.array_equal(g, w), (n, c)
            else:
                assert bits_equal(g, w), (nm, n, c, first_bit_difference(g, w))
    Cf = fields(*n, ("c",), seed0=9, dtype=dtype)[0]
    for A, stag in ((Cf, (0, 0, 0)), (V[0], (1, 0, 0)), (V[1], (0, 1, 0)), (V[2], (0, 0, 1))):
        for st in (None, state):
            assert bits_equal(TR.sample(A, X, st, stag), s_sample(A, X, st, stag)), (n, stag)


# ---- 2. planted points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GRIDS, ids=str)
def test_planted_points(n, dtype):
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=dtype)
    Cf = fields(*n, ("c",), seed0=9, dtype=dtype)[0]
    X, state = TR.planted_points(n)
    got = TR.sample(Cf, X, state)
    assert bits_equal(got, s_sample(Cf, X, state, (0, 0, 0)))
    per = 24                                                # values planted per direction (tracers_ref.planted_points)
    # order per direction: 0, −0, n, 1, 2, n−1, .5, 1.5, n−.5, 0⁺, 0⁻, n⁻, n⁺, .5⁻, .5⁺, (n−.5)⁻, (n−.5)⁺, NaN, +Inf, −Inf, −1, n+1, ±1e300
    outside = {10, 12, 17, 18, 19, 20, 21, 22, 23}
    for q in range(3):
        for v in range(per):
            assert np.isnan(got[q * per + v]) == (v in outside), (q, v, X[:, q * per + v])
    assert not np.isnan(got[3 * per:3 * per + 8]).any()     # the eight corners of the closed box are inside
    assert np.isnan(got[-1]) and state[-1] == 0             # a dead point at a good position
    assert not np.isnan(TR.sample(Cf, X, None)[-1])
    # a point on a cell centre returns that cell's value, a point on a node of a staggered field that node's
    i, j, k = n[0] // 2, n[1] // 2, n[2] // 2
    P = np.array([[i + 0.5], [j + 0.5], [k + 0.5]])
    assert TR.sample(Cf, P)[0] == np.float64(Cf[i, j, k])
    P = np.array([[float(i)], [j + 0.5], [k + 0.5]])
    assert TR.sample(V[0], P, None, (1, 0, 0))[0] == np.float64(V[0][i, j, k])
    # −0.0 is inside and is treated as +0.0
    P = np.array([[-0.0, 0.0], [j + 0.5] * 2, [k + 0.5] * 2])
    r = TR.sample(V[0], P, None, (1, 0, 0))
    assert bits_equal(r[:1], r[1:]) and r[0] == np.float64(V[0][0, j, k])
    # the advance kills exactly the inactive points and keeps their coordinates
    Xn, sn, U = TR.advance(X, state, *V, (0.4, 0.36, 0.32))
    inactive = ~((state == 1) & TR.inside(X, n))
    assert inactive.sum() == 3 * len(outside) + 1
    assert bits_equal(Xn[:, inactive], X[:, inactive]) and not sn[inactive].any() and np.isnan(U[:, inactive]).all()
    assert np.array_equal(X[:, inactive].view(np.uint64), Xn[:, inactive].view(np.uint64))      # NaN payloads too
    assert not np.isnan(U[:, ~inactive]).any()


def test_a_field_at_rest_leaves_every_position():
    n = (17, 9, 5)
    V = [hostile(a, 5 + q, "rest0") for q, a in enumerate(fields(*n, ("vx", "vy", "vz"), seed0=3))]
    X, state = _points(n)
    Xn, sn, U = TR.advance(X, state, *V, (2.5, 2.25, 2.0))
    act = (state == 1) & TR.inside(X, n)
    # bit for bit — but for an active particle's coordinate −0.0, which −0.0 + (+0.0) turns into +0.0
    negzero = (X == 0.0) & np.signbit(X) & act[None, :]
    assert negzero.sum() == 2 and not Xn[negzero].any() and not np.signbit(Xn[negzero]).any()
    assert np.array_equal(X.view(np.uint64)[~negzero], Xn.view(np.uint64)[~negzero])
    assert np.array_equal(sn, act.astype(np.uint8)) and not U[:, act].any()


def test_non_finite_velocities_kill():
    n = (17, 9, 5)
    V = [a.copy(order="F") for a in fields(*n, ("vx", "vy", "vz"), seed0=3)]
    V[0][8, 4, 2] = np.nan
    V[1][3, 3, 1] = np.inf
    X = np.array([[8.2, 3.5, 2.0], [4.4, 3.1, 1.0], [2.6, 1.4, 2.0]]).T.copy()
    Xn, sn, U = TR.advance(X, np.ones(3, np.uint8), *V, (0.4, 0.36, 0.32))
    assert list(sn) == [0, 0, 1]
    assert np.isnan(Xn[0, 0]) and np.isinf(Xn[1, 1]) and np.isfinite(Xn[:, 2]).all()
    assert np.isfinite(Xn[1:, 0]).all()             # the midpoint is stored as it is: only the x coordinate went bad


# ---- 3. navierstokes3d_amd/tracers.py on the CPU ------------------------------------------------------------------------------------
def _cpu_tracers(n=(17, 9, 5), **kw):
    from navierstokes3d_amd.tracers import Tracers
    return Tracers(n, None, (0.05, 0.07, 0.11), (-0.425, -0.315, -0.275), **kw)


def test_sort_by_cell_is_a_stable_permutation_with_non_decreasing_keys():
    import torch
    t = _cpu_tracers(keep_velocity=True)
    n = t.shape
    X = np.concatenate([TR.uniform_points(n, 500, 3), TR.uniform_points(n, 300, 3)[:, ::-1], TR.planted_points(n)[0]], axis=1)
    t._set(X, (np.arange(X.shape[1]) % 3 != 0).astype(np.uint8))
    t.U[:] = torch.arange(X.shape[1], dtype=torch.float64)[None, :]     # a per-particle tag that must travel with its particle
    X0, s0, k0 = t.X.clone(), t.state.clone(), t.cell_keys().numpy()
    perm = t.sort_by_cell().numpy()
    assert sorted(perm.tolist()) == list(range(X.shape[1]))
    keys = t.cell_keys().numpy()
    assert np.all(np.diff(keys) >= 0) and np.array_equal(keys, k0[perm])
    same = np.diff(keys) == 0
    assert same.any() and np.all(np.diff(perm)[same] > 0)               # stable: equal keys keep their order
    assert np.array_equal(t.X.numpy().view(np.uint64), X0.numpy()[:, perm].view(np.uint64))
    assert np.array_equal(t.state.numpy(), s0.numpy()[perm]) and np.array_equal(t.U[0].numpy(), perm.astype(np.float64))
    # the key is ((k·ny + j)·nx + i) of the containing cell; non-finite positions sort last
    fin = np.isfinite(X0.numpy()).all(axis=0)
    c = TR.cell_of(np.where(fin, X0.numpy(), 0.0), n)
    want = np.where(fin, (c[2] * n[1] + c[1]) * n[0] + c[0], n[0] * n[1] * n[2])
    assert np.array_equal(k0, want) and (~fin).sum() == 9 and not fin[perm][-9:].any()
    assert t.X.is_contiguous() and t.state.is_contiguous()


def test_seed_points_positions_round_trip_and_reseed():
    t = _cpu_tracers()
    rng = np.random.Generator(np.random.MT19937(5))
    lo = np.array(t.origin)
    ext = np.array(t.shape) * np.array(t.spacings)
    xyz = lo + rng.uniform(0, 1, size=(64, 3)) * ext
    xyz[3] = lo - 0.01                                                   # outside: starts dead
    t.seed_points(xyz)
    assert t.n == 64 and t.X.shape == (3, 64) and t.steps == 0
    want = np.stack([(xyz[:, q] - t.origin[q]) / t.spacings[q] for q in range(3)])
    assert np.array_equal(t.X.numpy().view(np.uint64), want.view(np.uint64))
    assert np.abs(t.positions() - xyz).max() <= 4 * np.finfo(np.float64).eps * np.abs(xyz).max()
    alive = t.alive()
    assert not alive[3] and alive.sum() == 63
    # reseed fills dead slots only, lowest first
    t.state[[10, 20]] = 0
    before = t.X.clone()
    new = lo + 0.5 * ext + np.array([[0.0, 0, 0], [0.01, 0, 0], [0.02, 0, 0], [0.03, 0, 0]])
    assert t.reseed(new) == 3
    assert t.alive().all()
    idx = t.to_index(new)
    for slot, q in ((3, 0), (10, 1), (20, 2)):
        assert np.array_equal(t.X[:, slot].numpy(), idx[:, q])
    keep = np.ones(64, bool); keep[[3, 10, 20]] = False
    assert np.array_equal(t.X.numpy()[:, keep], before.numpy()[:, keep])
    assert t.reseed(new) == 0
    with pytest.raises(Exception):
        t.seed_points(np.zeros((4, 2)))
    from navierstokes3d_amd import lib as L
    with pytest.raises(L.Ns3dError):
        t.advance(None, 0.1)


def test_seed_random_is_the_reference_generator_and_save_bins(tmp_path):
    from navierstokes3d_amd.tracers import Tracers
    t = _cpu_tracers().seed_random(100, 0)
    assert np.array_equal(t.X.numpy(), TR.uniform_points(t.shape, 100, 0)) and t.alive().all()
    rec = t.record()
    assert rec.steps == 0 and rec.x.shape == (100,)
    path = Tracers.save_bins(rec, 7, outdir=str(tmp_path))
    assert os.path.basename(path) == "out_tracers_0007.bin"
    raw = np.fromfile(path, dtype=np.float32).reshape(100, 4)            # column-major (4,N): four values per particle
    assert np.array_equal(raw[:, 0], rec.x.astype(np.float32)) and np.array_equal(raw[:, 2], rec.z.astype(np.float32))
    assert np.all(raw[:, 3] == 1.0)
    from navierstokes3d_amd.vis import save_frame_tracers
    png = save_frame_tracers(rec, 0.85, 0.63, 2, outdir=str(tmp_path))
    assert os.path.basename(png) == "3D_NavierStokes_tracers_0002.png" and open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"


# ---- 4. the boundary ----------------------------------------------------------------------------------------------------------------------
def _header_args(name):
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    m = re.search(r"int %s_##S\(([^;]*)\);" % name, src)
    assert m, "include/ns3d.h does not declare %s_##S" % name
    return [a.strip() for a in re.sub(r"\\\n", " ", m.group(1)).split(",")]


def _cls(a):
    return "ptr" if "*" in a else a.split()[0]


def test_header_declares_and_binding_lists_the_entry_points():
    import ctypes as C
    from navierstokes3d_amd import lib as L
    ctype = {"ptr": C.c_void_p, "double": C.c_double, "int": C.c_int, "long": C.c_long}
    want = {"sample": ["ptr"] * 4 + ["long", "ptr"] + ["int"] * 6,
            "tracers_advance": ["ptr"] * 4 + ["long"] + ["ptr"] * 3 + ["double"] * 3 + ["int"] * 3}
    for name, classes in want.items():
        args = _header_args("ns3d_" + name)
        assert [_cls(a) for a in args] == classes, name
        assert L.DERIVED_SIGNATURES[name] == [ctype[c] for c in classes[1:]], name
        assert name not in L.SIGNATURES
        for suf in ("f64", "f32"):
            assert "ns3d_%s_%s" % (name, suf) in L.exported_symbols()
    assert len(L.SIGNATURES) == 35
    assert "const unsigned char *state" in _header_args("ns3d_sample")[3]


def test_library_exports_the_entry_points():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for name in ("sample", "tracers_advance"):
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            assert fn(None, *[a() for a in L.DERIVED_SIGNATURES[name]]) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
