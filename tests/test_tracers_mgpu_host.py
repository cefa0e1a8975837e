"""CPU tests of tracers on a decomposed grid (include/ns3d.h): the ownership rule, the exactness claim behind
"P ranks give the one-rank bits", the host side of MgpuTracers, and the boundary (header and binding).  No GPU."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tracers_mgpu_ref as MR  # noqa: E402
import tracers_ref as TR  # noqa: E402

TOPOLOGIES = [((1, 1, 3), (13, 7, 5)), ((2, 2, 1), (7, 6, 5)), ((2, 2, 2), (7, 6, 5))]


def _grid(dims, n):
    P = dims[0] * dims[1] * dims[2]
    return SimpleNamespace(nx=n[0], ny=n[1], nz=n[2], dims=dims, P=P, local_ranks=list(range(P)),
                           local_coords=[MR.coords_of(r, dims) for r in range(P)], contexts=None, mg=None)


def _points(dims, n, N, seed):
    g = MR.n_g(dims, n)
    X = TR.uniform_points(g, N, seed)
    Xp, _ = MR.planted(dims, n)
    return np.concatenate([X, Xp[:, np.isfinite(Xp).all(axis=0)]], axis=1)


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n", TOPOLOGIES)
def test_ownership_partitions_the_closed_global_box(dims, n):
    """the header's intervals, evaluated one by one: every point of [0, n_g] is inside exactly one rank's"""
    g = MR.n_g(dims, n)
    X = _points(dims, n, 20000, 3)
    assert TR.inside(X, g).all()
    count = np.zeros(X.shape[1], dtype=np.int64)
    for r in range(dims[0] * dims[1] * dims[2]):
        co = MR.coords_of(r, dims)
        mine = np.ones(X.shape[1], dtype=bool)
        for q in range(3):
            k, D, m = co[q], dims[q], n[q] - 2
            lo = 0.0 if k == 0 else float(k * m + 1)
            mine &= X[q] >= lo
            mine &= (X[q] <= float(g[q])) if k == D - 1 else (X[q] < float((k + 1) * m + 1))
        count += mine
        assert np.array_equal(mine, MR.owners(X, dims, n) == r)
    assert np.all(count == 1)


@pytest.mark.parametrize("dims,n", TOPOLOGIES)
def test_points_on_the_seam_values_and_the_faces(dims, n):
    from navierstokes3d_amd.tracers import owner_coords, owner_ranks
    g = MR.n_g(dims, n)
    for q in range(3):
        D, m = dims[q], n[q] - 2
        for k in range(1, D):
            s = float(k * m + 1)
            assert MR.owner_coord(np.array([s]), D, n[q])[0] == k                       # exactly on k(n−2)+1: belongs to k
            assert MR.owner_coord(np.array([np.nextafter(s, 0.0)]), D, n[q])[0] == k - 1
        assert MR.owner_coord(np.array([0.0, -0.0]), D, n[q]).tolist() == [0, 0]
        assert MR.owner_coord(np.array([float(g[q])]), D, n[q])[0] == D - 1               # n_g inclusive
        assert MR.owner_coord(np.array([-3.0, g[q] + 3.0, np.nan]), D, n[q]).tolist() == [0, D - 1, 0]
    X, _ = MR.planted(dims, n)
    k = owner_coords(X, dims, n)
    for q in range(3):
        assert np.array_equal(k[q], MR.owner_coord(X[q], dims[q], n[q]))
    assert np.array_equal(owner_ranks(X, dims, n), MR.owners(X, dims, n))
    X = _points(dims, n, 5000, 5)
    assert np.array_equal(owner_ranks(X, dims, n), MR.owners(X, dims, n))


# ---- 2. why P ranks give the one-rank bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("stag", [0, 1])
def test_local_axis_is_the_global_axis_minus_origin_inside_the_margin(stag):
    """10^5 points: owned start points (local p in [1, n−1)) and midpoints up to one cell away in a decomposed direction — half a cell
    short of the first local clamp for a cell-centred direction, a whole cell for a staggered one.  axis() on X − origin gives the
    global node minus origin and the SAME bits of t.  One planted pair at the margin's edge shows that the claim stops there."""
    D, n = 5, 9
    m, g = n - 2, D * (n - 2) + 2
    rng = np.random.Generator(np.random.MT19937(11))
    k = rng.integers(0, D, size=100000)
    o = k * m
    lo = np.where(k == 0, 0.0, o + 1.0)
    hi = np.where(k == D - 1, float(g), o + m + 1.0)
    X = lo + rng.uniform(0.0, 1.0, size=k.size) * (hi - lo)                    # owned: k(n−2)+1 ≤ X < (k+1)(n−2)+1
    assert np.array_equal(MR.owner_coord(X, D, n), k)
    Xm = X + 0.5 * rng.uniform(-1.0, 1.0, size=k.size)                         # Xm = X + 0.5·(v1·c) with |v1·c| < 1
    for P in (X, Xm):
        d = P - o
        assert np.array_equal(d + o, P)                                         # the subtraction is exact
        ig, tg = TR.axis(P, stag, g + stag)
        il, tl = TR.axis(d, stag, n + stag)
        assert np.array_equal(il + o, ig)
        assert np.array_equal(tl.view(np.int64), tg.view(np.int64))
    # the margin's edge, at an interior rank's upper side: local n − 0.5 (cell-centred) resp. n (staggered) is the first clamp
    o1 = 2 * m
    edge = float(n) - (0.0 if stag else 0.5) + o1
    for G, same in ((np.nextafter(edge, 0.0), True), (edge, False)):
        ig, tg = TR.axis(np.array([G]), stag, g + stag)
        il, tl = TR.axis(np.array([G - o1]), stag, n + stag)
        assert ((il[0] + o1 == ig[0]) and (tl[0] == tg[0])) == same, (G, il, ig, tl, tg)


# ---- 3. MgpuTracers on the host --------------------------------------------------------------------------------------------------
def test_mgpu_tracers_seed_on_cpu_arrays():
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.tracers import MgpuTracers, Tracers
    dims, n = (2, 2, 2), (7, 6, 5)
    g = MR.n_g(dims, n)
    sp, org = (0.1, 0.2, 0.3), (-0.6, -0.5, -0.4)
    t = MgpuTracers(_grid(dims, n), sp, org, keep_velocity=True, slack=0.5).seed_random(500, 4)
    one = Tracers(g, None, sp, org).seed_random(500, 4)
    assert t.shape == g and t.n == 500
    X = one.X.numpy()
    assert np.array_equal(t.index_positions(), X)                               # the same X as Tracers on the global shape, by id
    own = MR.owners(X, dims, n)
    for l in range(8):
        mine = np.nonzero(own == l)[0]
        ids = t.ids[l].numpy()
        assert np.array_equal(ids[:mine.size], mine) and np.all(ids[mine.size:] == -1)       # ids are the seeding order
        assert t.caps()[l] == mine.size + max(int(np.ceil(mine.size * 0.5)), 16)
        assert np.array_equal(t.X[l].numpy()[:, :mine.size], X[:, mine]) and np.isnan(t.X[l].numpy()[:, mine.size:]).all()
        assert np.all(t.state[l].numpy()[:mine.size] == 1) and np.all(t.state[l].numpy()[mine.size:] == 0)
        assert t.U[l].shape == (3, t.caps()[l])
    rec, ref = t.record(), one.record()
    assert np.array_equal(rec.x, ref.x) and np.array_equal(rec.z, ref.z) and rec.alive.all() and rec.steps == 0
    # capacity growth keeps what is there and appends empty slots
    before = [a.clone() for a in (t.X[3], t.state[3], t.ids[3])]
    cap = t.caps()[3]
    t._grow(3, 5)
    assert t.caps()[3] == cap + 5 + 16 and t.grown == 1
    assert np.array_equal(t.X[3].numpy()[:, :cap], before[0].numpy(), equal_nan=True) and np.isnan(t.X[3].numpy()[:, cap:]).all()
    assert np.array_equal(t.ids[3].numpy()[:cap], before[2].numpy()) and np.all(t.ids[3].numpy()[cap:] == -1)
    assert np.all(t.state[3].numpy()[cap:] == 0) and t.U[3].shape == (3, cap + 21)
    assert np.array_equal(t.index_positions(), X)
    # seed_points: outside points start dead and sit on the rank the clamped rule gives; sort_by_cell keeps the ids attached
    pts = np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [-0.6, -0.5, -0.4], [0.6 - 1e-9, 0.1, 0.1], [np.nan, 0.0, 0.0]])
    t.seed_points(pts)
    assert t.alive().tolist() == [True, False, True, True, False]
    assert np.array_equal(t.positions()[:4], one.seed_points(pts).positions()[:4])
    t.seed_random(300, 1)
    X = t.index_positions()
    t.sort_by_cell()
    assert np.array_equal(t.index_positions(), X)
    for l in range(8):
        ids = t.ids[l].numpy()
        occ = int(np.sum(ids >= 0))
        assert np.all(ids[:occ] >= 0) and np.all(ids[occ:] == -1)
    with pytest.raises(L.Ns3dError, match="no CPU path"):
        t.advance([], 0.1)
    part = _grid(dims, n)
    part.local_ranks = [3]
    with pytest.raises(L.Ns3dError, match="every rank in this process"):
        MgpuTracers(part, sp, org)


# ---- 4. the boundary ---------------------------------------------------------------------------------------------------------------
def _header_args(pattern):
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    m = re.search(r"int %s\(([^;]*)\);" % pattern, src)
    assert m, "include/ns3d.h does not declare %s" % pattern
    return [a.strip() for a in re.sub(r"\\\n", " ", m.group(1)).split(",")]


def _cls(a):
    if "*const *" in a or "* const *" in a:
        return "pp"
    if "*" in a:
        return "ptr"
    return " ".join(a.split()[:-1]) if len(a.split()) > 1 else a


def test_header_declares_and_binding_lists_the_four_calls():
    from navierstokes3d_amd import lib as L
    ctype = {"ptr": C.c_void_p, "double": C.c_double, "int": C.c_int, "long": C.c_long, "pp": C.POINTER(C.c_void_p)}
    intp, longp, llp = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_longlong)
    sample = ["ptr"] * 4 + ["long", "ptr"] + ["int"] * 6
    advance = ["ptr"] * 4 + ["long"] + ["ptr"] * 3 + ["double"] * 3 + ["int"] * 3
    # single-context forms: NS3D_DECL and DERIVED_SIGNATURES — the one-rank argument list, then the origin (and n_g)
    for name, classes, extra in (("sample_at", sample, 1), ("tracers_advance_at", advance, 2)):
        args = _header_args("ns3d_%s_##S" % name)
        assert [_cls(a) for a in args] == classes + ["ptr"] * extra, name
        assert all(a.startswith("const int *") for a in args[-extra:])
        assert L.DERIVED_SIGNATURES[name] == [ctype[c] for c in classes[1:]] + [intp] * extra
        assert name not in L.SIGNATURES and name not in L.MGPU_SIGNATURES
    # typed mgpu form
    args = _header_args("ns3d_tracers_advance_mgpu_##S")
    assert [_cls(a) for a in args] == ["ptr", "pp", "pp", "pp", "ptr", "pp", "pp", "pp", "double", "double", "double"]
    assert args[4].startswith("const long *")
    assert L.MGPU_SIGNATURES["tracers_advance_mgpu"] == [ctype["pp"]] * 3 + [longp] + [ctype["pp"]] * 3 + [C.c_double] * 3
    # untyped form
    args = _header_args("ns3d_tracers_migrate_mgpu")
    assert [_cls(a) for a in args] == ["ptr", "pp", "pp", "pp", "pp", "ptr", "ptr", "ptr"]
    assert args[5].startswith("const long *") and args[6].startswith("long long *") and args[7].startswith("long *")
    assert L.MGPU_SYMBOLS["ns3d_tracers_migrate_mgpu"] == (C.c_int, [C.c_void_p] + [ctype["pp"]] * 4 + [longp, llp, longp])
    syms = L.exported_symbols()
    for s in ("ns3d_sample_at_f64", "ns3d_sample_at_f32", "ns3d_tracers_advance_at_f64", "ns3d_tracers_advance_at_f32",
              "ns3d_tracers_advance_mgpu_f64", "ns3d_tracers_advance_mgpu_f32", "ns3d_tracers_migrate_mgpu"):
        assert syms.count(s) == 1, s
    assert len(L.SIGNATURES) == 35
    src = open(os.path.join(ROOT, "include", "ns3d.h")).read()
    assert re.search(r"ns3d_tracers_migrate_mgpu\s+the counts", src)          # the table of calls that wait
    assert "bit for bit in X, state and U" in src and "below 1 in the decomposed directions" in src


def test_library_exports_the_calls_and_checks_the_handle_first():
    from navierstokes3d_amd import build, lib as L
    build.build()
    lib = L.load()
    for name in ("sample_at", "tracers_advance_at"):
        for suf in ("f64", "f32"):
            fn = getattr(lib, "ns3d_%s_%s" % (name, suf))
            args = [a() if not hasattr(a, "contents") else None for a in L.DERIVED_SIGNATURES[name]]
            assert fn(None, *args) == L.NS3D_ERR_ARG
            assert L.last_error() == "ns3d_%s_%s: null context" % (name, suf)
    moved, need = C.c_longlong(7), (C.c_long * 1)(9)
    assert lib.ns3d_tracers_migrate_mgpu(None, None, None, None, None, None, C.byref(moved), need) == L.NS3D_ERR_ARG
    assert "null ns3d_mgpu" in L.last_error() and moved.value == 7 and need[0] == 9
    for suf in ("f64", "f32"):
        fn = getattr(lib, "ns3d_tracers_advance_mgpu_" + suf)
        assert fn(None, None, None, None, None, None, None, None, 0.1, 0.1, 0.1) == L.NS3D_ERR_ARG
        assert "null ns3d_mgpu" in L.last_error()
