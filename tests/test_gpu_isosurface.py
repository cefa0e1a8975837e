"""GPU tests of ns3d_isosurface (include/ns3d.h): marching tetrahedra, compacted on the device into one ordered triangle list.

The reference is the header's definition as NumPy (tests/isosurface_ref.py), computed once per case and shared, never modified.
Every context — STRICT, NS3D_IEEE_DIV, FAST — must return its bits, triangle for triangle and in order.  The kernels work on row
segments of 64 cubes in x (one wave each), NS3D_ISO_ROWS = 4 rows per workgroup and NS3D_ISO_KZ = 8 cube planes per z-march; the
scan on NS3D_ISO_SCAN_BLOCK = 1024 segments per workgroup, whose sums one wave scans 64 at a time (so 65 536 segments reach its
carry).  The extents below are node counts: a direction of e nodes has e − 1 cubes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import isosurface_ref as IR
from util import bits_equal, first_bit_difference, rnd

pytestmark = pytest.mark.gpu

NPDT = {"f64": np.float64, "f32": np.float32}
BASE = [(2, 2, 2), (3, 3, 3), (4, 3, 5), (17, 9, 5), (64, 3, 3), (65, 5, 3), (66, 5, 4), (129, 6, 3), (130, 9, 17), (1030, 3, 3),
        (70, 35, 8), (131, 66, 37)]
# cubes ≡ 0, ±1 modulo the rows per workgroup (4) and the planes per march (8): 5 and 9, 7 and 7, 3 and 17, 4 and 8 cubes in y and z
TILE = [(5, 6, 10), (9, 8, 8), (9, 4, 18), (128, 5, 9)]
# row segments just below, equal to and just above one scan block of 1024 (one cube per row: segments = cubes in y × cubes in z)
SCAN = [(2, 32, 34), (2, 33, 33), (2, 26, 42)]
GRIDS = BASE + TILE + SCAN
DENSE_ALL_LEVELS = (2, 258, 258)        # 257² = 66 049 segments: more than 64 scan blocks, the one-wave scan of their sums carries
GID = lambda n: "%dx%dx%d" % n
KINDS = ("noise", "gyroid", "ramp", "const", "quantised", "nonfinite")
SENTINEL = 777.0
PAD = 5                                 # triangles of sentinel behind the capacity


def field(n, dt, kind):
    """(A, iso)"""
    i, j, k = np.meshgrid(*[np.arange(e, dtype=np.float64) for e in n], indexing="ij")
    if kind == "noise":
        a, iso = rnd(11, n), 0.1
    elif kind == "gyroid":
        x, y, z = 0.31 * i + 0.2, 0.27 * j + 0.5, 0.41 * k + 0.1
        a, iso = np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x), 0.3
    elif kind == "ramp":
        a = 0.37 * i + 0.11 * j - 0.23 * k
        iso = 0.5 * (a.min() + a.max()) + 0.0123
    elif kind == "const":
        a, iso = np.ones(n), 1.0
    elif kind == "quantised":
        a, iso = np.round(rnd(12, n) * 2.0) / 2.0, 0.5            # five levels, iso on one of them
    elif kind == "nonfinite":
        a, iso = rnd(13, n).copy(), -0.2
        flat = a.reshape(-1, order="F")
        m = flat.size
        for q, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
            flat[(m * (2 * q + 1)) // 9] = v
        flat[0], flat[m - 1] = np.inf, np.nan
        a = flat.reshape(n, order="F")
    return np.asfortranarray(a.astype(NPDT[dt])), float(iso)


@functools.lru_cache(maxsize=8)        # the largest cases hold 200 MB each and are used by one test
def case(n, dt, kind, box=None, origin=None):
    """A, B, iso, reference (tri, val) — shared, never modified"""
    A, iso = field(n, dt, kind)
    B = rnd(21, n, NPDT[dt])
    tri, val = IR.reference(A, iso, B, box, origin)
    return A, B, iso, tri, val


@pytest.fixture(scope="module")
def ctxs(hip):
    c = {"strict": hip.Context(0, "strict"), "ieee": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield c
    for x in c.values():
        x.close()


def run(hip, ctx, A, B, iso, cap, box=None, origin=None, color=True):
    """n and the tri / val buffers of cap + PAD triangles as they come back"""
    a = hip.from_numpy(A)
    b = hip.from_numpy(B) if color else None
    tri = torch.full((9 * (cap + PAD),), SENTINEL, dtype=torch.float64, device="cuda")
    val = torch.full((3 * (cap + PAD),), SENTINEL, dtype=torch.float64, device="cuda") if color else None
    n = hip.isosurface(a, iso, color=b, box=box, origin=origin, tri=tri, val=val, cap=cap, ctx=ctx)
    ctx.sync()
    assert bits_equal(hip.to_numpy(a), A), "A was modified"
    if color:
        assert bits_equal(hip.to_numpy(b), B), "B was modified"
    return n, tri.cpu().numpy().reshape(-1, 3, 3), (val.cpu().numpy().reshape(-1, 3) if color else None)


def assert_prefix(got_tri, got_val, ref_tri, ref_val, cap, what):
    m = min(cap, ref_tri.shape[0])
    assert bits_equal(got_tri[:m], ref_tri[:m]), (what, "tri", first_bit_difference(got_tri[:m], ref_tri[:m]))
    assert (got_tri[m:] == SENTINEL).all(), (what, "tri written beyond the prefix")
    if got_val is not None:
        assert bits_equal(got_val[:m], ref_val[:m]), (what, "val", first_bit_difference(got_val[:m], ref_val[:m]))
        assert (got_val[m:] == SENTINEL).all(), (what, "val written beyond the prefix")


def check_case(hip, ctx, n, dt, kind, what, box=None, origin=None):
    A, B, iso, tri, val = case(n, dt, kind, box, origin)
    nref = tri.shape[0]
    got_n, got_tri, got_val = run(hip, ctx, A, B, iso, nref, box, origin)
    print(what, "triangles", got_n, "reference", nref)
    assert got_n == nref, what
    assert_prefix(got_tri, got_val, tri, val, nref, what)
    return nref


# ---- 1. the bits of the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_every_context_returns_the_bits_of_the_reference(hip, ctxs, n, kind, dt):
    for name, ctx in ctxs.items():
        count = check_case(hip, ctx, n, dt, kind, (n, dt, kind, name))
    cubes = (n[0] - 1) * (n[1] - 1) * (n[2] - 1)
    if kind == "const":
        assert count == 0
    elif kind == "noise" and cubes >= 64:
        assert count > 4 * cubes                      # dense: nearly every cube emits
    elif cubes >= 1000:
        assert 0 < count < 8 * cubes


def test_noise_reaches_twelve_triangles_per_cube():
    A, _, iso, _, _ = case((17, 9, 5), "f64", "noise")
    a8 = IR.corner_values(A, IR.cubes_of(A.shape, None))
    mask = ((a8 >= iso) << np.arange(8)).sum(axis=1)
    assert IR.CUBE_COUNT[mask].max() == 12


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_dense_field_through_every_level_of_the_scan(hip, ctxs, dt):
    n = DENSE_ALL_LEVELS
    assert (n[1] - 1) * (n[2] - 1) > 64 * 1024
    nref = check_case(hip, ctxs["strict"], n, dt, "noise", (n, dt))
    assert nref > 4 * 257 * 257


def test_uncoloured_surface_has_the_same_triangles(hip, ctxs):
    n = (70, 35, 8)
    A, B, iso, tri, _ = case(n, "f64", "gyroid")
    got_n, got_tri, _ = run(hip, ctxs["strict"], A, B, iso, tri.shape[0], color=False)
    assert got_n == tri.shape[0]
    assert_prefix(got_tri, None, tri, None, got_n, "uncoloured")


# ---- 2. capacity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["noise", "gyroid"])
def test_capacity(hip, ctxs, kind, dt):
    n = (130, 9, 17)
    A, B, iso, tri, val = case(n, dt, kind)
    nref = tri.shape[0]
    assert nref > 8
    a = hip.from_numpy(A)
    assert hip.isosurface(a, iso, ctx=ctxs["strict"]) == nref                                   # count-only, uncoloured
    assert hip.isosurface(a, iso, color=hip.from_numpy(B), ctx=ctxs["strict"]) == nref          # count-only with B
    for cap in (nref - 1, 1, nref + 7):
        got_n, got_tri, got_val = run(hip, ctxs["strict"], A, B, iso, cap)
        assert got_n == nref, cap
        assert_prefix(got_tri, got_val, tri, val, cap, (kind, dt, cap))


# ---- 3. box and origin --------------------------------------------------------------------------------------------------------
BOXES = [(0, 0, 0, 1, 1, 1), (129, 8, 16, 130, 9, 17), (37, 2, 3, 38, 3, 4), (37, 1, 2, 120, 7, 13), (63, 0, 0, 65, 9, 17), (1, 1, 1, 129, 8, 16),
         (64, 3, 5, 130, 8, 6)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "-".join(map(str, b)))
def test_sub_boxes(hip, ctxs, box, dt):
    n = (131, 10, 18)
    for kind, origin in (("noise", None), ("gyroid", (1000, -7, 129))):
        check_case(hip, ctxs["strict"], n, dt, kind, (box, dt, kind), box, origin)


def test_overlapping_boxes_agree_on_the_shared_face(hip, ctxs):
    """two ranks' views of one global array: rank 1's array starts 60 nodes in and carries origin 60; the vertices on the plane x = 70
    of both pieces are the same set, bit for bit, and both pieces together are the whole surface"""
    n = (131, 10, 18)
    A, B, iso, tri, val = case(n, "f64", "gyroid")
    lo = run(hip, ctxs["strict"], A, B, iso, tri.shape[0], box=(0, 0, 0, 70, 9, 17))
    A1, B1 = np.asfortranarray(A[60:]), np.asfortranarray(B[60:])
    hi = run(hip, ctxs["strict"], A1, B1, iso, tri.shape[0], box=(10, 0, 0, 70, 9, 17), origin=(60, 0, 0))
    t_lo, t_hi = lo[1][:lo[0]], hi[1][:hi[0]]
    assert lo[0] + hi[0] == tri.shape[0]
    face = lambda t: {v.tobytes() for v in t.reshape(-1, 3)[t.reshape(-1, 3)[:, 0] == 70.0]}
    assert len(face(t_lo)) > 10 and face(t_lo) == face(t_hi)
    rows = lambda t, v: sorted(r.tobytes() for r in np.concatenate([t.reshape(-1, 9), v.reshape(-1, 3)], axis=1))
    both_t, both_v = np.concatenate([t_lo, t_hi]), np.concatenate([lo[2][:lo[0]], hi[2][:hi[0]]])
    assert rows(both_t, both_v) == rows(tri, val)


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_contexts_return_the_same_bits(hip, ctxs):
    n = (131, 66, 37)
    A, B, iso, tri, _ = case(n, "f64", "noise")
    first = run(hip, ctxs["strict"], A, B, iso, tri.shape[0])
    again = run(hip, ctxs["strict"], A, B, iso, tri.shape[0])
    other = hip.Context(0, "strict")
    third = run(hip, other, A, B, iso, tri.shape[0])
    other.close()
    for r in (again, third):
        assert r[0] == first[0] and bits_equal(r[1], first[1]) and bits_equal(r[2], first[2])


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_everything_untouched(hip, ctxs):
    from navierstokes3d_amd import lib as L
    n = (17, 9, 5)
    A, B, iso, tri, _ = case(n, "f64", "noise")
    ctx = ctxs["strict"]
    a, b = hip.from_numpy(A), hip.from_numpy(B)
    cap = tri.shape[0]
    t = torch.full((9 * cap,), SENTINEL, dtype=torch.float64, device="cuda")
    v = torch.full((3 * cap,), SENTINEL, dtype=torch.float64, device="cuda")
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    box6 = lambda *q: (C.c_int * 6)(*q)
    good = dict(ctx=ctx.handle, A=P(a), B=P(b), e=n, box=None, iso=iso, tri=P(t), val=P(v), cap=cap, out=True)
    bad = [dict(ctx=None), dict(A=None), dict(out=False), dict(e=(1, 9, 5)), dict(e=(17, 1, 5)), dict(e=(17, 9, 1)),
           dict(box=box6(0, 0, 0, 17, 8, 4)), dict(box=box6(-1, 0, 0, 16, 8, 4)), dict(box=box6(0, 3, 0, 16, 3, 4)),
           dict(box=box6(0, 0, 4, 16, 8, 2)), dict(cap=-1), dict(tri=None), dict(B=None), dict(iso=float("nan")), dict(iso=float("inf"))]
    fn = ctx.lib.ns3d_isosurface_f64
    for change in bad:
        k = dict(good, **change)
        out = C.c_longlong(-12345)
        rc = fn(k["ctx"], k["A"], k["B"], *k["e"], k["box"], None, C.c_double(k["iso"]), k["tri"], k["val"], C.c_longlong(k["cap"]),
                C.byref(out) if k["out"] else None)
        assert rc == L.NS3D_ERR_ARG, (change, rc, L.last_error())
        ctx.sync()
        assert out.value == -12345, change
        assert (t == SENTINEL).all().item() and (v == SENTINEL).all().item(), change
    # the same arguments unchanged are accepted
    out = C.c_longlong(-1)
    assert fn(good["ctx"], good["A"], good["B"], *n, None, None, C.c_double(iso), good["tri"], good["val"], C.c_longlong(cap), C.byref(out)) == 0
    assert out.value == cap


# ---- 6. the drivers -----------------------------------------------------------------------------------------------------------
def _same_surface(a, b):
    assert a.n == b.n and a.n > 0
    assert bits_equal(a.tri_index, b.tri_index) and bits_equal(a.tri, b.tri)
    assert (a.val is None) == (b.val is None) and (a.val is None or bits_equal(a.val, b.val))


def test_multi_driver_on_one_rank(hip, tmp_path, monkeypatch):
    from navierstokes3d_amd import isosurface as ISO
    from navierstokes3d_amd.driver import run_navierstokes3D
    from util import assert_bit_identical, errs_identical
    monkeypatch.chdir(tmp_path)
    kw = dict(nx=24, nt=2, mode="strict", niter_cap=40, return_info=True)
    plain = run_navierstokes3D(vortex=True, **kw)
    assert not hasattr(plain[-1], "isosurface")
    Q = plain[-1].vortex.Q
    level = 0.25 * float(Q.max())
    assert level > 0.0
    p, ctx = plain[-1].params, plain[-1].ctx
    geo = dict(spacings=(p.dx, p.dy, p.dz), low_corner=(-p.lx / 2, -p.ly / 2, -p.lz / 2))
    # info.vortex holds the halo-stripped array: its node 0 is node 1 of the rank's array
    want = ISO.extract(ctx, hip.from_numpy(Q), level, origin=(1, 1, 1), **geo)
    for extra in (dict(vortex=True), dict(), dict(one_call=False)):
        out = run_navierstokes3D(isosurface=level, **extra, **kw)
        assert_bit_identical(out[:5], plain[:5])
        assert out[-1].iters == plain[-1].iters and errs_identical(out[-1].errs, plain[-1].errs)
        assert hasattr(out[-1], "vortex") == ("vortex" in extra)
        _same_surface(out[-1].isosurface, want)
    assert not os.path.exists("out_save")
    # coloured, from a field of the flow
    out = run_navierstokes3D(isosurface=dict(field="Q", level=level, color="Pr"), **kw)
    pr = hip.from_numpy(np.asfortranarray(hip.to_numpy(out[-1].fields.Pr)[1:-1, 1:-1, 1:-1]))
    _same_surface(out[-1].isosurface, ISO.extract(ctx, hip.from_numpy(Q), level, color=pr, origin=(1, 1, 1), **geo))
    assert_bit_identical(out[:5], plain[:5])


def test_gpu_driver(hip, tmp_path, monkeypatch):
    from navierstokes3d_amd import isosurface as ISO
    from navierstokes3d_amd.driver import runme
    from util import errs_identical
    monkeypatch.chdir(tmp_path)
    kw = dict(nx=24, nt=2, mode="strict", niter_cap=40)
    gf, gi = runme(vortex=True, **kw)
    assert not hasattr(gi, "isosurface")
    Q = gi.vortex.Q
    level = 0.25 * float(Q.max())
    p = gi.params
    n = Q.shape
    want = ISO.extract(gi.ctx, hip.from_numpy(Q), level, box=(1, 1, 1, n[0] - 2, n[1] - 2, n[2] - 2), spacings=(p.dx, p.dy, p.dz),
                       low_corner=(-p.lx / 2, -p.ly / 2, -p.lz / 2))
    for extra in (dict(vortex=True), dict()):
        f, info = runme(isosurface=level, **extra, **kw)
        for nm in ("Pr", "C", "Vx", "Vy", "Vz"):
            assert np.array_equal(hip.to_numpy(getattr(f, nm)), hip.to_numpy(getattr(gf, nm)), equal_nan=True), nm
        assert info.iters == gi.iters and errs_identical(info.errs, gi.errs)
        _same_surface(info.isosurface, want)
    assert not os.path.exists("out_save")


def test_ply_files_appear_only_with_do_save_and_the_keyword(hip, tmp_path, monkeypatch):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    kw = dict(do_save=True, nx=24, nt=1, mode="strict", niter_cap=40)
    spec = dict(field="Pr", level=0.0, color="C")
    for name, call in (("multi", run_navierstokes3D), ("gpu", runme)):
        (tmp_path / name / "a").mkdir(parents=True); (tmp_path / name / "b").mkdir()
        monkeypatch.chdir(tmp_path / name / "a")
        call(isosurface=spec, **kw)
        have = set(os.listdir("out_save"))
        assert "out_iso_0000.ply" in have and open("out_save/out_iso_0000.ply", "rb").read(4) == b"ply\n"
        monkeypatch.chdir(tmp_path / name / "b")
        call(**kw)
        assert have - set(os.listdir("out_save")) == {"out_iso_0000.ply"}


def test_two_virtual_z_slab_ranks_give_the_surface_of_the_gathered_array(hip):
    from navierstokes3d_amd import isosurface as ISO
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    nx, nt, P, nz_loc = 24, 2, 2, 9
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        kw = dict(nx=nx, nt=nt, mode="strict", niter_cap=40, return_info=True, shape=dict(nz=nz_loc))
        plain = run_navierstokes3D(grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), **kw)
        Pr = plain[1]                               # the gathered, halo-stripped global array
        level = 0.5 * (float(Pr.min()) + float(Pr.max()))
        two = run_navierstokes3D(grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), isosurface=dict(field="Pr", level=level), **kw)
        for a, b in zip(two[:5], plain[:5]):
            assert np.array_equal(a, b, equal_nan=True)
        got = two[-1].isosurface
        # the global array with its outermost cells: the ranks' own boundary planes around the gathered interior
        loc = [hip.to_numpy(f.Pr) for f in two[-1].local_fields]
        glob = np.asfortranarray(np.concatenate([loc[0][:, :, :nz_loc - 1], loc[1][:, :, 1:]], axis=2))
        assert glob.shape[2] == P * (nz_loc - 2) + 2 and bits_equal(np.asfortranarray(glob[1:-1, 1:-1, 1:-1]), np.asfortranarray(Pr))
        p = two[-1].params
        want = ISO.extract(two[-1].ctx, hip.from_numpy(glob), level, spacings=(p.dx, p.dy, p.dz), low_corner=(-p.lx / 2, -p.ly / 2, -p.lz / 2))
        rows = lambda s: sorted(r.tobytes() for r in np.concatenate([s.tri_index.reshape(-1, 9), s.tri.reshape(-1, 9)], axis=1))
        assert got.val is None and got.n == want.n and got.n > 0 and rows(got) == rows(want)
    finally:
        mg.sync()
        mg.close()


def test_tracers_on_several_ranks_still_raise(hip):
    from navierstokes3d_amd import lib as L
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    p0 = multi_params(24, dims=(1, 1, 2), coords=(0, 0, 0), nz=9)
    mg = MultiGpu.create([0, 0], p0.nx, p0.ny, p0.nz, "strict")
    try:
        for kw in (dict(tracers=8), dict(probes=np.zeros((1, 3)))):
            with pytest.raises(L.Ns3dError):
                run_navierstokes3D(nx=24, nt=1, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), shape=dict(nz=9), isosurface=0.1, **kw)
    finally:
        mg.sync()
        mg.close()
