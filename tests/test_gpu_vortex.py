"""GPU tests of ns3d_vortex (include/ns3d.h): vorticity and Q-criterion in one fused pass.

The reference is the header's NumPy expression (tests/vortex_ref.py), computed once per case and shared, never modified.  STRICT must
return its bits — whichever of the three division builds the spacings select; FAST is held, element by element, to the running-error
bound of the same expression.  k_vortex owns 64×4 cell columns per workgroup and marches 16 planes: the grids straddle those
extents."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import running_error as RE
import vortex_ref as VR
from util import bits_equal, fields, first_bit_difference, geometry, hostile

pytestmark = pytest.mark.gpu

NPDT = {"f64": np.float64, "f32": np.float32}
BASE = [(3, 3, 3), (4, 3, 5), (17, 9, 5), (65, 5, 3), (66, 5, 4), (67, 6, 3), (1030, 3, 3), (24, 15, 15), (70, 35, 8), (131, 66, 37)]
# extents − 2 ≡ 0, +1, −1 modulo the tile (64 in x, 4 in y) and the chunk (16 planes), one and two tiles; and the extents themselves
EDGE = [(66, 6, 18), (67, 7, 19), (65, 5, 17), (130, 10, 34), (131, 11, 35), (129, 9, 33), (64, 8, 16), (128, 4, 32), (63, 3, 15)]
GRIDS = BASE + EDGE
GID = lambda n: "%dx%dx%d" % n
SPACINGS = ("geometry", "pow2", "ieee")


def spacings_of(n, kind):
    if kind == "pow2":
        return 2.0 ** -5, 2.0 ** -7, 2.0 ** -3
    g = geometry(*n)
    return g["dx"], g["dy"], g["dz"]


@functools.lru_cache(maxsize=None)
def case(n, dt, kind="geometry", values="seeded"):
    """(Vx, Vy, Vz), (dx, dy, dz), reference — shared, never modified"""
    V = fields(*n, ("vx", "vy", "vz"), seed0=3, dtype=NPDT[dt])
    if values in ("dense", "blocks", "rest0"):
        V = [hostile(a, 5 + q, values) for q, a in enumerate(V)]
    elif values == "nan":
        V = [a.copy(order="F") for a in V]
        V[0][n[0] // 2, n[1] // 2, n[2] // 2] = np.nan
    d = spacings_of(n, kind)
    with np.errstate(all="ignore"):
        ref = VR.reference(*V, *d)
    return V, d, ref


@pytest.fixture(scope="module")
def ctxs(hip):
    c = {"strict": hip.Context(0, "strict"), "ieee": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield c
    for x in c.values():
        x.close()


def run(hip, ctx, V, d, n, dt, which=VR.NAMES):
    dev = [hip.from_numpy(a) for a in V]
    out = {nm: hip.from_numpy(np.full(n, 777.0, dtype=NPDT[dt])) for nm in which}
    hip.vortex(*dev, *d, ctx=ctx, **out)
    ctx.sync()
    for a, t in zip(V, dev):
        assert bits_equal(hip.to_numpy(t), a), "an input was modified"
    return {nm: hip.to_numpy(t) for nm, t in out.items()}


def assert_bits(got, ref, what):
    for nm in got:
        assert got[nm].dtype == ref[nm].dtype
        assert bits_equal(got[nm], ref[nm]), (what, nm, first_bit_difference(got[nm], ref[nm]))


# ---- 1. STRICT bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_strict_returns_the_bits_of_the_numpy_expression(hip, ctxs, n, dt):
    builds = set()
    for kind in SPACINGS:
        V, d, ref = case(n, dt, kind)
        ctx = ctxs["ieee"] if kind == "ieee" else ctxs["strict"]
        builds.add(ctx.arith_build(*d))
        assert_bits(run(hip, ctx, V, d, n, dt), ref, (n, dt, kind))
    # builds 0, 1 and 3: plain IEEE divisions, exact division by a known divisor, power-of-two spacings
    assert builds == {"strict", "strictx", "strictp"}, builds


# ---- 2. hostile values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("values", ["dense", "blocks", "rest0"])
@pytest.mark.parametrize("n", [(70, 35, 8), (130, 10, 34)], ids=GID)
def test_hostile_values(hip, ctxs, n, values, dt):
    for kind in ("geometry", "pow2"):
        V, d, ref = case(n, dt, kind, values)
        assert_bits(run(hip, ctxs["strict"], V, d, n, dt), ref, (n, dt, kind, values))
        if values == "rest0":
            for nm in VR.NAMES:
                assert not ref[nm].any(), nm
    if values == "dense":
        assert any(not np.isfinite(ref[nm]).all() for nm in VR.NAMES)      # the case does reach Inf / NaN


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_single_nan_shows_up_where_the_reference_has_it(hip, ctxs, dt):
    n = (70, 35, 8)
    V, d, ref = case(n, dt, "geometry", "nan")
    got = run(hip, ctxs["strict"], V, d, n, dt)
    for nm in VR.NAMES:
        assert np.array_equal(np.isnan(got[nm]), np.isnan(ref[nm])), nm
    # Vx feeds u and gxx: uy, uz of the neighbours in y and z (Wy, Wz, Q) and Q of the two cells the face belongs to; never Wx
    assert not np.isnan(ref["Wx"]).any() and np.isnan(ref["Wy"]).sum() == 4 and np.isnan(ref["Wz"]).sum() == 4
    assert np.isnan(ref["Q"]).sum() == 10
    assert_bits(got, ref, "nan")


# ---- 3. output selection and footprint ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_every_subset_of_one_or_two_outputs_equals_the_full_result(hip, ctxs, dt):
    n = (67, 7, 19)
    V, d, ref = case(n, dt)
    for which in [(a,) for a in VR.NAMES] + list(itertools.combinations(VR.NAMES, 2)):
        got = run(hip, ctxs["strict"], V, d, n, dt, which)
        assert set(got) == set(which)
        assert_bits(got, ref, which)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [(17, 9, 5), (131, 11, 35)], ids=GID)
def test_footprint_and_boundary_zeros(hip, ctxs, n, dt):
    """outputs carved out of a sentinel-filled buffer: the padding on both sides stays, every boundary entry is +0.0"""
    V, d, ref = case(n, dt)
    cells, pad = n[0] * n[1] * n[2], 97
    tdt = torch.float64 if dt == "f64" else torch.float32
    buf = torch.full((4 * cells + 5 * pad,), 777.0, dtype=tdt, device="cuda")
    out = {}
    for q, nm in enumerate(VR.NAMES):
        o = pad + q * (cells + pad)
        out[nm] = buf[o:o + cells].view(n[2], n[1], n[0]).permute(2, 1, 0)
    dev = [hip.from_numpy(a) for a in V]
    hip.vortex(*dev, *d, ctx=ctxs["strict"], **out)
    ctxs["strict"].sync()
    host = buf.cpu().numpy()
    uint = np.uint64 if dt == "f64" else np.uint32
    for q, nm in enumerate(VR.NAMES):
        o = pad + q * (cells + pad)
        assert np.all(host[o - pad:o] == 777.0) and np.all(host[o + cells:o + cells + pad] == 777.0), nm
        got = host[o:o + cells].reshape(n[2], n[1], n[0]).transpose(2, 1, 0)
        assert bits_equal(np.asfortranarray(got), ref[nm]), nm
        mask = np.ones(n, dtype=bool)
        mask[VR.I] = False
        assert np.all(np.ascontiguousarray(got).view(uint)[mask] == 0), nm
    for a, t in zip(V, dev):
        assert bits_equal(hip.to_numpy(t), a)


# ---- 4. FAST -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n,values", [((70, 35, 8), "seeded"), ((67, 7, 19), "seeded"), ((24, 15, 15), "rest0")], ids=str)
def test_fast_within_the_running_error_bound(hip, ctxs, n, values, dt):
    V, d, ref = case(n, dt, "geometry", values)
    prs = VR.reference_pairs(*V, *d)
    got = run(hip, ctxs["fast"], V, d, n, dt)
    assert ctxs["fast"].arith_build(*d) == "fast"
    worst = 0.0
    for nm in VR.NAMES:
        worst = max(worst, RE.check(got[nm], ref[nm], prs[nm], NPDT[dt], "FAST vortex %s %s %r" % (nm, dt, n)))
    print("FAST vortex %s %r %s: worst err/bound %.3g" % (dt, n, values, worst))
    if values == "rest0":
        assert all((prs[nm].e == 0).all() for nm in VR.NAMES)          # a flow at rest: bound 0 everywhere, hence the bits


# ---- 5. decomposition invariance without a grid object -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("dims", [(1, 1, 2), (2, 1, 1), (2, 2, 2)], ids=str)
def test_local_boxes_tile_the_global_result(hip, ctxs, dims, dt):
    """ImplicitGlobalGrid's index rule: cell-centred extents overlap by 2, the staggered direction by 3"""
    n = (34, 20, 20)
    V, d, ref = case(n, dt)
    nl = [(n[a] - 2) // dims[a] + 2 for a in range(3)]
    assert all((n[a] - 2) % dims[a] == 0 for a in range(3))
    glob = {nm: np.zeros(n, dtype=NPDT[dt], order="F") for nm in VR.NAMES}
    for c in itertools.product(*[range(q) for q in dims]):
        lo = [c[a] * (nl[a] - 2) for a in range(3)]
        box = lambda stag: tuple(slice(lo[a], lo[a] + nl[a] + (1 if a == stag else 0)) for a in range(3))
        loc = [np.asfortranarray(V[q][box(q)]) for q in range(3)]
        got = run(hip, ctxs["strict"], loc, d, tuple(nl), dt)
        dst = tuple(slice(lo[a] + 1, lo[a] + nl[a] - 1) for a in range(3))
        for nm in VR.NAMES:
            glob[nm][dst] = got[nm][VR.I]
    for nm in VR.NAMES:
        assert bits_equal(glob[nm][VR.I], ref[nm][VR.I]), (nm, dims)


# ---- 6. error paths -----------------------------------------------------------------------------------------------------------------
def test_error_paths(hip, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    n = (3, 3, 3)
    V, d, ref = case(n, "f64")
    dev = [hip.from_numpy(a) for a in V]
    out = [hip.from_numpy(np.full(n, 777.0)) for _ in range(4)]
    P = lambda t: C.c_void_p(t.data_ptr())
    D = lambda *xs: [C.c_double(x) for x in xs]
    fn, h = lib.ns3d_vortex_f64, ctxs["strict"].handle
    W, Vp, ok = [P(t) for t in out], [P(t) for t in dev], D(*d)
    calls = {
        "null context": lambda: fn(None, *W, *Vp, *ok, 3, 3, 3),
        "null Vx": lambda: fn(h, *W, None, Vp[1], Vp[2], *ok, 3, 3, 3),
        "null Vy": lambda: fn(h, *W, Vp[0], None, Vp[2], *ok, 3, 3, 3),
        "null Vz": lambda: fn(h, *W, Vp[0], Vp[1], None, *ok, 3, 3, 3),
        "no output": lambda: fn(h, None, None, None, None, *Vp, *ok, 3, 3, 3),
        "grid 2x3x3": lambda: fn(h, *W, *Vp, *ok, 2, 3, 3),
        "grid 3x2x3": lambda: fn(h, *W, *Vp, *ok, 3, 2, 3),
        "grid 3x3x2": lambda: fn(h, *W, *Vp, *ok, 3, 3, 2),
        "dx 0": lambda: fn(h, *W, *Vp, *D(0.0, d[1], d[2]), 3, 3, 3),
        "dy negative": lambda: fn(h, *W, *Vp, *D(d[0], -d[1], d[2]), 3, 3, 3),
        "dz nan": lambda: fn(h, *W, *Vp, *D(d[0], d[1], float("nan")), 3, 3, 3),
        "dx inf": lambda: fn(h, *W, *Vp, *D(float("inf"), d[1], d[2]), 3, 3, 3),
    }
    for what, call in calls.items():
        assert call() == L.NS3D_ERR_ARG == 1, what
        assert L.last_error().startswith("ns3d_vortex_f64: "), (what, L.last_error())
    ctxs["strict"].sync()
    for t in out:
        assert np.all(hip.to_numpy(t) == 777.0)
    for suf in ("f64", "f32"):
        assert getattr(lib, "ns3d_vortex_" + suf)(None, *W, *Vp, *ok, 3, 3, 3) == L.NS3D_ERR_ARG
        assert L.last_error() == "ns3d_vortex_%s: null context" % suf
    with pytest.raises(L.Ns3dError):
        hip.vortex(*dev, *d, ctx=ctxs["strict"])                        # no output
    with pytest.raises(L.Ns3dError):
        hip.vortex(*dev, *d, ctx=ctxs["strict"], Q=hip.zeros((3, 3, 4)))  # shape
    with pytest.raises(L.Ns3dError):
        hip.vortex(*dev, *d, ctx=ctxs["strict"], Q=hip.zeros(n, torch.float32))  # dtype
    # the context is still usable
    hip.vortex(*dev, *d, ctx=ctxs["strict"], Wx=out[0], Wy=out[1], Wz=out[2], Q=out[3])
    ctxs["strict"].sync()
    assert_bits(dict(zip(VR.NAMES, [hip.to_numpy(t) for t in out])), ref, "after the errors")


# ---- 7. drivers -----------------------------------------------------------------------------------------------------------------
def _ref_of_fields(hip, f, p):
    return VR.reference(*[hip.to_numpy(getattr(f, nm)) for nm in ("Vx", "Vy", "Vz")], p.dx, p.dy, p.dz)


def test_driver_on_one_rank(hip):
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    from util import assert_bit_identical, errs_identical
    kw = dict(nx=24, nt=3, mode="strict", niter_cap=40, return_info=True)
    plain = run_navierstokes3D(**kw)
    assert not hasattr(plain[-1], "vortex")
    for extra in (dict(), dict(one_call=False)):
        out = run_navierstokes3D(vortex=True, **extra, **kw)
        assert_bit_identical(out[:5], plain[:5])
        assert out[-1].iters == plain[-1].iters and errs_identical(out[-1].errs, plain[-1].errs)
        ref = _ref_of_fields(hip, out[-1].fields, out[-1].params)
        for nm in VR.NAMES:
            got = getattr(out[-1].vortex, nm)
            assert got.shape == out[1].shape and bits_equal(np.asfortranarray(got), np.asfortranarray(ref[nm][VR.I])), nm
        assert max(np.abs(getattr(out[-1].vortex, nm)).max() for nm in ("Wx", "Wy", "Wz")) > 0
    gkw = dict(nx=24, nt=3, mode="strict", niter_cap=40)
    gf, gi = runme(**gkw)
    f, info = runme(vortex=True, **gkw)
    assert not hasattr(gi, "vortex")
    for nm in ("Pr", "C", "Vx", "Vy", "Vz"):
        assert np.array_equal(hip.to_numpy(getattr(f, nm)), hip.to_numpy(getattr(gf, nm)), equal_nan=True), nm
    assert info.iters == gi.iters and errs_identical(info.errs, gi.errs)
    ref = _ref_of_fields(hip, f, info.params)
    for nm in VR.NAMES:
        assert getattr(info.vortex, nm).shape == tuple(f.Pr.shape) and bits_equal(getattr(info.vortex, nm), ref[nm]), nm


def test_driver_on_two_virtual_z_slab_ranks(hip):
    """P = 2 z-slab ranks on one device with the wide advection halo reproduce the one-rank run's fields bit for bit; the gathered
    vortex fields must too."""
    from navierstokes3d_amd.driver import run_navierstokes3D
    from navierstokes3d_amd.mgpu import MgpuGrid, MultiGpu
    from navierstokes3d_amd.params import multi_params
    nx, nt, P, nz_loc = 36, 3, 2, 12
    one = run_navierstokes3D(nx=nx, nt=nt, mode="strict", return_info=True, vortex=True)
    assert one[-1].params.nz == P * (nz_loc - 2) + 2
    p0 = multi_params(nx, dims=(1, 1, P), coords=(0, 0, 0), nz=nz_loc)
    mg = MultiGpu.create([0] * P, p0.nx, p0.ny, p0.nz, "strict")
    try:
        two = run_navierstokes3D(nx=nx, nt=nt, mode="strict", grid=MgpuGrid(mg, p0.nx, p0.ny, p0.nz), return_info=True,
                                 shape=dict(nz=nz_loc), wide_advect_halo=True, vortex=True)
        for nm in VR.NAMES:
            a, b = getattr(one[-1].vortex, nm), getattr(two[-1].vortex, nm)
            assert a.shape == b.shape == (34, 20, 20), nm
            assert bits_equal(np.asfortranarray(a), np.asfortranarray(b)), (nm, first_bit_difference(a, b))
        assert np.abs(one[-1].vortex.Wz).max() > 0
    finally:
        mg.sync()
        mg.close()


def test_do_save_writes_the_four_extra_files(hip, tmp_path, monkeypatch):
    from navierstokes3d_amd.driver import run_navierstokes3D
    names = ["out_%s_v_0000.bin" % nm for nm in VR.NAMES]
    pngs = ["3D_NavierStokes_%s_0000.png" % t for t in ("xy_Wz", "xy_Q", "xz_Wy", "xz_Q")]
    kw = dict(do_save=True, do_vis=True, nx=24, nt=1, mode="strict", niter_cap=40)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    monkeypatch.chdir(tmp_path / "a")
    out = run_navierstokes3D(vortex=True, **kw)
    have = set(os.listdir("out_save"))
    for nm in names:
        assert nm in have and os.path.getsize(os.path.join("out_save", nm)) == 4 * out[1].size, nm
    drawn = set(os.listdir("viz3D_out"))
    assert set(pngs) <= drawn
    monkeypatch.chdir(tmp_path / "b")
    run_navierstokes3D(**kw)
    assert have - set(os.listdir("out_save")) == set(names)
    assert drawn - set(os.listdir("viz3D_out")) == set(pngs)
