"""GPU tests of the obstacle calls (include/ns3d.h): ns3d_voxelize byte for byte against its NumPy statement tests/solid_ref.py,
ns3d_set_solid against set_cylinder! and in a guarded arena under a hostile mask, ns3d_solid_momentum against math.fsum and the
monitor, ns3d_set_obstacle inside ns3d_time_step and the `obstacle` keyword of both drivers, and each call once in stream order.
Every context kind (STRICT, NS3D_IEEE_DIV, FAST) must return the same bytes.  The kernels' edges: rows of up to three 64-word passes of
k_vox_prefix, more than 256 partials in k_mom_final, ns3d_set_solid's mask at every address mod 16.  The whole step against its CPU
statement is in tests/test_gpu_solid_step.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import arena as AR
import solid_cases as SC
import solid_ref as SR
import stream_order as SO
from util import fields, rnd

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32}
TD = {"f64": torch.float64, "f32": torch.float32}
DTS = ["f64", "f32"]
GRIDS = [(13, 11, 9), (70, 6, 5), (31, 5, 4), (32, 4, 5), (3, 3, 3)]
GID = lambda n: "%dx%dx%d" % tuple(n)


@pytest.fixture(scope="module")
def S(hip):
    from navierstokes3d_amd import solid
    return solid


@pytest.fixture(scope="module")
def ctxs(hip):
    """one context per arithmetic mode: the calls below must not depend on it"""
    out = {"strict": hip.Context(0, "strict"), "ieee_div": hip.Context(0, "strict", ieee_div=True), "fast": hip.Context(0, "fast")}
    yield out
    for c in out.values():
        c.close()


def _vox(S, ctx, tri, n, origin=None):
    m = S.voxelize(ctx, tri, *n, origin=origin)
    ctx.sync()
    return S.to_numpy(m)


def _check_all(S, ctxs, tri, n, origin=None, what=""):
    want = SR.voxelize(tri, *n, origin=origin)
    for name, ctx in ctxs.items():
        got = _vox(S, ctx, tri, n, origin)
        assert np.array_equal(got, want), (what, GID(n), name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    return want


# ---- ns3d_voxelize ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "zero_one"])
@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_voxelize_device_isosurfaces(hip, S, ctxs, n, kind):
    """marching-tetrahedra surfaces taken from ns3d_isosurface itself on the device, shifted by 0.5: a random field, and a 0/1 field
    whose every vertex sits on a lattice midpoint (all ties); the same triangles permuted; the call repeated"""
    from navierstokes3d_amd import isosurface as ISO
    A, iso = SC.field(kind, n, seed=sum(n) + 1)
    A[n[0] // 2, n[1] // 2, n[2] // 2] = 1.0          # never an empty surface (3x3x3 has one interior node)
    surf = ISO.extract(ctxs["strict"], hip.from_numpy(A), iso)
    tri = S.from_isosurface(surf)
    assert np.array_equal(tri, SC.surface(A, iso)) and tri.shape[0] > 0
    want = _check_all(S, ctxs, tri, n, what=kind)
    e, sure = SC.expected_mask(A, iso)
    assert np.array_equal(want & sure, e & sure)
    perm = np.random.Generator(np.random.MT19937(9)).permutation(tri.shape[0])
    assert np.array_equal(_vox(S, ctxs["strict"], tri[perm], n), want)
    assert np.array_equal(_vox(S, ctxs["strict"], tri, n), want)


@pytest.mark.parametrize("n", GRIDS, ids=GID)
def test_voxelize_boxes_outside_bodies_and_origin(hip, S, ctxs, n):
    nx, ny, nz = n
    big = S.box_mesh((-3.0, -2.5, -4.0), (nx + 2.0, ny + 3.5, nz + 1.0))
    want = _check_all(S, ctxs, big, n, what="box larger than the grid")
    assert (want[:nx, :ny, :nz] & 1).all() and (want[:, :ny, :nz] & 2).all() and (want[:nx, :, :nz] & 4).all() and (want[:nx, :ny, :] & 8).all()
    ext = np.array(n, dtype=np.float64)
    for q in range(3):
        for sign in (-1, 1):
            c = 0.5 * ext
            c[q] = -4.0 if sign < 0 else ext[q] + 4.0
            out = _check_all(S, ctxs, SC.octahedron(c, 2.5), n, what="outside %d %+d" % (q, sign))
            assert not out.any()
    origin = (3, 4096, 70001)
    body = np.concatenate([SC.octahedron(0.5 * ext + origin, 0.45 * ext + 0.3), S.box_mesh(np.array(origin) + 0.5, np.array(origin) + (1.0, 2.0, 1.5))])
    assert _check_all(S, ctxs, body, n, origin=origin, what="origin").any()
    assert not _check_all(S, ctxs, np.zeros((0, 3, 3)), n, what="empty").any()
    bad = np.full((2, 3, 3), np.nan)
    flat = np.array([[[0.0, 1.0, 1.0], [2.0, 1.0, 2.0], [1.0, 1.0, 0.5]]])
    assert np.array_equal(_check_all(S, ctxs, np.concatenate([bad, big, flat]), n, what="skipped"), want)


def test_voxelize_two_ranks_split_in_z(hip, S, ctxs):
    """two origins that split a grid in z reproduce the one-rank mask on their parts, the duplicated planes included"""
    nx, ny, nzl = 13, 7, 6
    nzg = 2 * (nzl - 2) + 2
    tri = np.concatenate([SC.octahedron((6.3, 3.4, 5.0), (5.0, 2.9, 3.7)), S.box_mesh((2.0, 1.0, 3.0), (4.0, 2.5, 7.0))])
    whole = _vox(S, ctxs["strict"], tri, (nx, ny, nzg))
    assert np.array_equal(whole, SR.voxelize(tri, nx, ny, nzg)) and whole.any()
    for r in (0, 1):
        k0 = r * (nzl - 2)
        for ctx in ctxs.values():
            part = _vox(S, ctx, tri, (nx, ny, nzl), origin=(0, 0, k0))
            want = whole[:, :, k0:k0 + nzl + 1].copy()
            want[:, :, nzl] &= 8                    # the local plane nz holds Vz nodes only
            assert np.array_equal(part, want), r
            assert part[:, :, :nzl].any()


def test_voxelize_scratch_growth_and_rezeroing(hip, S):
    """a small grid, a larger one, the small one again on ONE context: each result is that of a fresh context"""
    ctx = hip.Context(0, "strict", async_=True)
    for n in ((5, 4, 3), (70, 9, 8), (5, 4, 3), (33, 5, 4)):
        tri = SC.octahedron(0.5 * np.array(n, dtype=np.float64), 0.4 * np.array(n) + 0.2)
        got = _vox(S, ctx, tri, n)
        fresh = hip.Context(0, "strict")
        assert np.array_equal(got, _vox(S, fresh, tri, n)) and np.array_equal(got, SR.voxelize(tri, *n)) and got.any()
        fresh.close()
    ctx.close()


def test_voxelize_errors_leave_the_mask_untouched(hip, S, ctxs):
    from navierstokes3d_amd import lib as L
    lib = L.load()
    ctx = ctxs["strict"]
    n = (5, 4, 3)
    mask = torch.full((6 * 5 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    tri = torch.from_numpy(S.box_mesh((1, 1, 1), (3, 3, 2)).reshape(-1)).cuda()
    torch.cuda.synchronize()
    mp, tp = C.c_void_p(mask.data_ptr()), C.c_void_p(tri.data_ptr())
    neg = (C.c_int * 3)(0, -1, 0)
    cases = [("null context", (None, mp, tp, 12, 5, 4, 3, None)), ("null mask", (ctx.handle, None, tp, 12, 5, 4, 3, None)),
             ("tri is NULL", (ctx.handle, mp, None, 12, 5, 4, 3, None)), ("negative", (ctx.handle, mp, tp, -1, 5, 4, 3, None)),
             ("too small", (ctx.handle, mp, tp, 12, 2, 4, 3, None)), ("too small", (ctx.handle, mp, tp, 12, 5, 2, 3, None)),
             ("too small", (ctx.handle, mp, tp, 12, 5, 4, 2, None)), ("origin", (ctx.handle, mp, tp, 12, 5, 4, 3, neg))]
    for text, args in cases:
        assert lib.ns3d_voxelize(*args) == L.NS3D_ERR_ARG, text
        assert text in L.last_error(), (text, L.last_error())
    ctx.sync()
    assert (mask.cpu().numpy() == 0xA5).all()
    assert lib.ns3d_voxelize(ctx.handle, mp, None, 0, 5, 4, 3, None) == L.NS3D_OK      # n_tri == 0: an all-zero mask
    ctx.sync()
    assert not mask.cpu().numpy().any()


def test_voxelize_in_a_guarded_arena(hip, S, ctxs):
    n = (33, 5, 4)
    tri = SC.octahedron((16.2, 2.4, 2.1), (15.0, 2.2, 1.8))
    host = [("mask", np.full((n[0] + 1, n[1] + 1, n[2] + 1), 0x5A, dtype=np.uint8), True), ("tri", tri.reshape(-1).copy(), False)]
    ar = AR.Arena(host, "cuda")
    hip.voxelize(ar["mask"], ar["tri"], n, ctx=ctxs["strict"])
    ctxs["strict"].sync()
    ar.assert_clean("voxelize")
    assert np.array_equal(ar.get("mask"), SR.voxelize(tri, *n)) and np.array_equal(ar.get("tri"), tri.reshape(-1))


LONG_ROWS = [((1100, 5, 3), 35, (7, 4096, 70001)), ((2046, 3, 3), 64, None), ((2047, 4, 3), 65, None), ((4200, 3, 3), 132, None)]


@pytest.mark.parametrize("n,W,origin", LONG_ROWS, ids=[GID(n) for n, _, _ in LONG_ROWS])
def test_voxelize_long_rows(hip, S, ctxs, n, W, origin):
    """Rows of more than 96 samples: k_vox_prefix's ballot lanes ≥ 32 (W = 35 words per row), exactly one pass of 64 words (W = 64), a
    second pass with one live lane (W = 65), three passes (W = 132) with the row parity carried from pass to pass; one grid with an
    origin.  Bodies: an octahedron spanning the row (inside across every pass boundary), a box that leaves the grid at high x, and —
    where the row has a sample 2048 — boxes whose x faces put a flip on samples 2047 and 2048 of the C and of the Vx family: bit 31
    of word 63 and bit 0 of word 64."""
    nx, ny, nz = n
    assert (nx + 2 + 31) // 32 == W
    o = np.zeros(3) if origin is None else np.array(origin, dtype=np.float64)
    ext = np.array(n, dtype=np.float64)
    j, k = (ny - 1) // 2, (nz - 1) // 2      # the row next to the octahedron's axis
    span = SC.octahedron(o + (0.5 * nx + 0.2, j + 0.51, k + 0.505), (0.5 * nx - 1.3, j + 0.3, k + 0.3))
    m = _check_all(S, ctxs, span, n, origin=origin, what="spanning octahedron")
    assert (m[nx // 2, j, k] & 3) == 3 and (m[nx - 64, j, k] & 3) == 3 and not m[0, j, k] and not (m[nx - 1, j, k] & 1)
    for b in range(2048, nx - 64, 2048):    # inside on both sides of every pass boundary of the central row: the parity is carried
        assert (m[b - 1, j, k] & 3) == 3 and (m[b, j, k] & 3) == 3, (b, int(m[b - 1, j, k]), int(m[b, j, k]))
    high = S.box_mesh(o + (nx - 40.5, 0.7, 0.6), o + (nx + 5.0, 1.9, 1.8))
    m = _check_all(S, ctxs, high, n, origin=origin, what="box through the high x end")
    assert (m[nx, 1, 1] & 2) and (m[nx - 1, 1, 1] & 1) and not m[nx - 42, 1, 1]
    if nx > 2048:
        flips = np.concatenate([S.box_mesh(o + (2046.75, 0.2, 0.2), o + (2047.75, 0.9, 2.8)),      # C and Vx: sample 2047 alone
                                S.box_mesh(o + (100.3, 1.2, 0.2), o + (2047.25, 1.9, 2.8)),        # C ends on 2046, Vx on 2047
                                S.box_mesh(o + (2047.75, 2.1, 0.2), o + (2100.4, 2.9, 2.8))])      # C and Vx begin on 2048
        m = _check_all(S, ctxs, flips, n, origin=origin, what="flips on samples 2047 and 2048")
        assert [int(m[i, 0, 1] & 3) for i in (2046, 2047, 2048)] == [0, 3, 0]
        assert [int(m[i, 1, 1] & 3) for i in (2046, 2047, 2048, 2049)] == [3, 2, 0, 0]          # a dropped carry sets 2048 … of Vx
        assert [int(m[i, 2, 1] & 3) for i in (2047, 2048, 2100, 2101)] == [0, 3, 2, 0]
        assert (m[2047] != m[2048]).any()


# ---- ns3d_set_solid --------------------------------------------------------------------------------------------------------------------
def _cyl(script, nx):
    from navierstokes3d_amd.params import gpu_params, multi_params
    if script == "multi":
        p = multi_params(nx)
        return p, (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.xco_g, p.yco_g, p.zco_g, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)
    p = gpu_params(nx)
    return p, (p.a2, p.b2, p.ox, p.oy, p.sinb, p.cosb, p.lx, p.ly, p.lz, p.dx, p.dy, p.dz)


@pytest.mark.parametrize("script", ["multi", "gpu"])
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_equals_set_cylinder(hip, S, ctxs, dt, script):
    """with mask_of_cylinder, set_solid equals ns3d_set_cylinder (multi.jl form) and ns3d_set_cylinder_local (gpu.jl form) bit for bit"""
    p, cyl = _cyl(script, 24)
    n = (p.nx, p.ny, p.nz)
    host = fields(*n, ["c", "vx", "vy", "vz"], 3, NP[dt])
    for name, ctx in ctxs.items():
        mask = S.mask_of_cylinder(ctx, n, *cyl, dtype=TD[dt])
        mh = S.to_numpy(mask)
        assert all(((mh >> b) & 1).any() for b in range(4)) and not (mh & 0xF0).any()
        a, b = [hip.from_numpy(h) for h in host], [hip.from_numpy(h) for h in host]
        hip.set_cylinder(*a, *cyl, ctx=ctx)
        hip.set_solid(*b, mask, ctx=ctx)
        ctx.sync()
        for x, y, h in zip(a, b, host):
            assert np.array_equal(hip.to_numpy(x), hip.to_numpy(y)) and not np.array_equal(hip.to_numpy(y), h), name
        ref = [h.copy() for h in host]
        SR.set_solid(*ref, mh)
        assert all(np.array_equal(hip.to_numpy(y), r) for y, r in zip(b, ref))
        c0 = hip.from_numpy(host[1])                  # C may be NULL
        hip.set_solid(None, c0, b[2], b[3], mask, ctx=ctx)
        ctx.sync()
        assert np.array_equal(hip.to_numpy(c0), ref[1])


@pytest.mark.parametrize("n", [(5, 4, 3), (33, 6, 5), (16, 3, 7)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_hostile_mask_in_a_guarded_arena(hip, ctxs, dt, n):
    """0xFF everywhere — every bit at every invalid point — touches no entry outside the four arrays; a random mask stores exactly what
    the statement stores.  The arrays, the uint8 mask included, sit at odd element offsets."""
    nx, ny, nz = n
    host = fields(*n, ["c", "vx", "vy", "vz"], 5, NP[dt])
    rng = np.random.Generator(np.random.MT19937(2))
    for mask in (np.full((nx + 1, ny + 1, nz + 1), 0xFF, dtype=np.uint8), rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8),
                 (rng.integers(0, 16, (nx + 1, ny + 1, nz + 1)) * (rng.random((nx + 1, ny + 1, nz + 1)) < 0.05)).astype(np.uint8)):
        arrays = [(k, h, True) for k, h in zip(("C", "Vx", "Vy", "Vz"), host)] + [("mask", np.asfortranarray(mask), False)]
        ar = AR.Arena(arrays, "cuda")
        assert ar["mask"].data_ptr() % 2 == 1
        ctx = ctxs["strict"]
        hip.set_solid(ar["C"], ar["Vx"], ar["Vy"], ar["Vz"], ar["mask"], ctx=ctx)
        ctx.sync()
        ar.assert_clean("set_solid")
        ref = [h.copy() for h in host]
        SR.set_solid(*ref, mask)
        for k, r in zip(("C", "Vx", "Vy", "Vz"), ref):
            assert np.array_equal(ar.get(k), r), k
        assert np.array_equal(ar.get("mask"), mask)


@pytest.mark.parametrize("n", [(3, 3, 3), (5, 4, 3), (4, 4, 4)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_set_solid_at_every_lead(hip, ctxs, dt, n):
    """k_set_solid shifts its 16-byte chunks by lead = address mod 16 and loads the first and the last chunk byte by byte: the mask at
    byte offsets 0…15 of a larger tensor, N = 64, 120 and 125 bytes (N mod 16 = 0, 8, 13), a random hostile mask.  The four arrays
    equal the statement's, and the bytes around the mask — all bits set: read as flags they would store — are unchanged."""
    nx, ny, nz = n
    N = (nx + 1) * (ny + 1) * (nz + 1)
    assert N in (64, 120, 125)
    host = fields(*n, ["c", "vx", "vy", "vz"], 9, NP[dt])
    rng = np.random.Generator(np.random.MT19937(6))
    ctx = ctxs["strict"]
    for lead in range(16):
        mask = np.asfortranarray(rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8))
        big = np.full(N + 64, 0xFF, dtype=np.uint8)
        big[16 + lead:16 + lead + N] = mask.reshape(-1, order="F")
        dbig = torch.from_numpy(big).cuda()
        assert dbig.data_ptr() % 16 == 0
        view = dbig[16 + lead:16 + lead + N]
        assert view.data_ptr() % 16 == lead
        dev = [hip.from_numpy(h) for h in host]
        torch.cuda.synchronize()
        hip.set_solid(*dev, view, ctx=ctx)
        ctx.sync()
        ref = [h.copy() for h in host]
        SR.set_solid(*ref, mask)
        for name, d, r, h in zip(("C", "Vx", "Vy", "Vz"), dev, ref, host):
            assert np.array_equal(hip.to_numpy(d), r), (lead, name, np.argwhere(hip.to_numpy(d) != r)[:4].tolist())
            assert not np.array_equal(r, h)
        assert np.array_equal(dbig.cpu().numpy(), big), lead


# ---- ns3d_solid_momentum ---------------------------------------------------------------------------------------------------------------
def _within_bound(got, terms):
    """the any-order summation bound n·2⁻⁵³·Σ|term| around math.fsum of the same terms"""
    exact, n, mag = math.fsum(terms.tolist()), terms.size, math.fsum(np.abs(terms).tolist())
    return abs(got - exact) <= n * 2.0 ** -53 * mag, (got, exact, n, mag)


SEAMS = [((0, 0, 0), (0, 0, 0)), ((1, 0, 0), (0, 0, 0)), ((0, 1, 0), (0, 0, 0)), ((0, 0, 1), (0, 0, 0)), ((0, 0, 0), (1, 0, 0)),
         ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, 0, 1)), ((1, 1, 1), (1, 1, 1))]


@pytest.mark.parametrize("n", [(13, 11, 9), (70, 6, 5), (3, 3, 3)], ids=GID)
@pytest.mark.parametrize("dt", DTS)
def test_solid_momentum_counts_and_sums(hip, ctxs, dt, n):
    nx, ny, nz = n
    Vx, Vy, Vz = fields(*n, ["vx", "vy", "vz"], 7, NP[dt])
    rng = np.random.Generator(np.random.MT19937(4))
    mask = np.asfortranarray(rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8))       # hostile bits included
    ar = AR.Arena([("Vx", Vx, False), ("Vy", Vy, False), ("Vz", Vz, False), ("mask", mask, False)], "cuda")
    for lo, hi in SEAMS:
        terms = SR.momentum_terms(Vx, Vy, Vz, mask, lo, hi)
        first = None
        for name, ctx in ctxs.items():
            mom, cnt = hip.solid_momentum(ar["Vx"], ar["Vy"], ar["Vz"], ar["mask"], lo, hi, ctx=ctx)
            assert list(cnt) == [t.size for t in terms], (lo, hi, name)
            for q in range(3):
                ok, fig = _within_bound(mom[q], terms[q])
                assert ok, (lo, hi, name, q, fig)
            first = first or mom
            assert np.array_equal(np.array(mom), np.array(first)), "the sums depend on the context or the call"
    mom, cnt = hip.solid_momentum(ar["Vx"], ar["Vy"], ar["Vz"], ar["mask"], ctx=ctxs["strict"])      # NULL seam arrays: no seams
    assert list(cnt) == [t.size for t in SR.momentum_terms(Vx, Vy, Vz, mask)]
    ar.assert_clean("solid_momentum")


def diag_geometry(nx, ny, nz):
    """(planes per workgroup kz, per-workgroup partials) of ns3d_solid_momentum and ns3d_diagnostics: ns3d_diag_geometry's formula
    (csrc/ns3d_launch.h) restated — 64×4 columns per workgroup over (nx+1)×(ny+1), kz = 32 halved down to 8 while the launch has fewer
    than 2 048 workgroups"""
    gx, gy = (nx + 1 + 63) // 64, (ny + 1 + 3) // 4
    kz = 32
    while kz > 8 and gx * gy * ((nz + 1 + kz - 1) // kz) < 2048:
        kz //= 2
    return kz, gx * gy * ((nz + 1 + kz - 1) // kz)


REDUCTION_GRIDS = [((3, 255, 63), 8, 512), ((3, 1023, 127), 16, 2048), ((3, 2047, 127), 32, 2048)]


@pytest.mark.parametrize("n,kz,partials", REDUCTION_GRIDS, ids=[GID(n) for n, _, _ in REDUCTION_GRIDS])
@pytest.mark.parametrize("dt", DTS)
def test_solid_momentum_over_more_than_256_partials(hip, ctxs, dt, n, kz, partials):
    """k_mom_final's thread t combines the partials t, t + 256, …: the grids of the other tests leave at most 6, so the second trip of
    that loop never ran.  Here 512 and 2 048 partials, and kz = 8, 16 and 32 planes per workgroup; a random hostile mask; the counts
    exact, the sums within the any-order bound, with no seams and with all six."""
    from navierstokes3d_amd import diag as D
    assert diag_geometry(*n) == (kz, partials) and D.launch_geometry(*n) == (partials, kz) and partials > 256
    nx, ny, nz = n
    Vx, Vy, Vz = fields(*n, ["vx", "vy", "vz"], 17, NP[dt])
    rng = np.random.Generator(np.random.MT19937(8))
    mask = np.asfortranarray(rng.integers(0, 256, (nx + 1, ny + 1, nz + 1)).astype(np.uint8))
    d = [hip.from_numpy(a) for a in (Vx, Vy, Vz)]
    dm = torch.from_numpy(np.ascontiguousarray(mask.reshape(-1, order="F"))).cuda()
    torch.cuda.synchronize()
    for lo, hi in (((0, 0, 0), (0, 0, 0)), ((1, 1, 1), (1, 1, 1))):
        terms = SR.momentum_terms(Vx, Vy, Vz, mask, lo, hi)
        first = None
        for name, ctx in ctxs.items():
            mom, cnt = hip.solid_momentum(*d, dm, lo, hi, ctx=ctx)
            assert list(cnt) == [t.size for t in terms] and min(cnt) > 256, (lo, hi, name, cnt)
            for q in range(3):
                ok, fig = _within_bound(mom[q], terms[q])
                assert ok, (lo, hi, name, q, fig)
            first = first or mom
            assert np.array_equal(np.array(mom), np.array(first)), "the sums depend on the context or the call"


@pytest.mark.parametrize("script", ["multi", "gpu"])
@pytest.mark.parametrize("dt", DTS)
def test_solid_momentum_against_the_monitor(hip, S, ctxs, dt, script):
    p, cyl = _cyl(script, 24)
    n = (p.nx, p.ny, p.nz)
    Vx, Vy, Vz = fields(*n, ["vx", "vy", "vz"], 8, NP[dt])
    d = [hip.from_numpy(a) for a in (Vx, Vy, Vz)]
    ctx = ctxs["strict"]
    mask = S.mask_of_cylinder(ctx, n, *cyl, dtype=TD[dt])
    mh = S.to_numpy(mask)
    for lo, hi in SEAMS:
        dp = hip.diag_params(*n, p.dx, p.dy, p.dz, p.rho, seam_lo=lo, seam_hi=hi, cylinder=cyl)
        rec = hip.diagnostics(*d, None, None, dp, ctx=ctx)
        mom, cnt = hip.solid_momentum(*d, mask, lo, hi, ctx=ctx)
        assert tuple(cnt) == tuple(rec.n_masked) and sum(cnt) > 0, (lo, hi)
        terms = SR.momentum_terms(Vx, Vy, Vz, mh, lo, hi)
        for q in range(3):
            assert _within_bound(mom[q], terms[q])[0] and _within_bound(rec.mom[q], terms[q])[0], (lo, hi, q)


# ---- the step and the drivers --------------------------------------------------------------------------------------------------------
def _same_run(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:5], b[:5])) and a[-1].iters == b[-1].iters and a[-1].errs == b[-1].errs


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_multi_driver_with_the_cylinders_own_mask(hip, S, dt, fused):
    from navierstokes3d_amd.driver import run_navierstokes3D
    p, cyl = _cyl("multi", 24)
    kw = dict(nx=24, nt=2, dtype=TD[dt], fused=fused, niter_cap=40, return_info=True)
    ref = run_navierstokes3D(**kw)
    ctx = hip.Context(0, "strict")
    mask = S.mask_of_cylinder(ctx, (p.nx, p.ny, p.nz), *cyl, dtype=TD[dt])
    assert _same_run(run_navierstokes3D(obstacle=mask, **kw), ref)
    assert _same_run(run_navierstokes3D(obstacle=S.to_numpy(mask), **kw), ref)
    if fused:
        assert _same_run(run_navierstokes3D(obstacle=mask, one_call=False, **kw), ref)
        got = run_navierstokes3D(obstacle=mask, diagnostics=True, **kw)
        want = run_navierstokes3D(diagnostics=True, **kw)
        assert _same_run(got, ref)
        for a, b in zip(got[-1].diag, want[-1].diag):       # force: ns3d_solid_momentum's sums against the monitor's, same terms
            assert np.allclose(a.force, b.force, rtol=1e-9, atol=1e-9 * max(abs(q) for q in b.force))
    ctx.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", DTS)
def test_gpu_driver_with_the_cylinders_own_mask(hip, S, dt, fused):
    from navierstokes3d_amd.driver import runme
    p, cyl = _cyl("gpu", 24)
    kw = dict(nx=24, nt=3, dtype=TD[dt], fused=fused, niter_cap=40)
    get = lambda r: [hip.to_numpy(getattr(r[0], k)) for k in ("C", "Pr", "Vx", "Vy", "Vz")] + [r[1]]
    ref = runme(**kw)
    ctx = hip.Context(0, "strict")
    mask = S.mask_of_cylinder(ctx, (p.nx, p.ny, p.nz), *cyl, dtype=TD[dt])
    got = runme(obstacle=mask, **kw)
    assert _same_run(get(got), get(ref))
    assert got[1].ctx.obstacle() is None            # the driver leaves the knob at its default
    if fused:
        assert _same_run(get(runme(obstacle=mask, one_call=False, **kw)), get(ref))
    ctx.close()


@pytest.mark.parametrize("dt", DTS)
def test_box_obstacle_in_one_call_equals_call_by_call(hip, S, dt):
    """a box_mesh obstacle through ns3d_time_step (ns3d_set_obstacle) equals the same steps made call by call, bit for bit — and is not
    the cylinder's flow; ns3d_set_obstacle(NULL) restores the default"""
    from navierstokes3d_amd.driver import run_navierstokes3D, runme
    box = S.box_mesh((5.0, 4.5, 2.0), (9.0, 10.0, 13.5))
    kw = dict(nx=24, nt=2, dtype=TD[dt], niter_cap=40, return_info=True)
    a = run_navierstokes3D(obstacle=box, one_call=True, **kw)
    b = run_navierstokes3D(obstacle=box, one_call=False, **kw)
    c = run_navierstokes3D(obstacle=box, diagnostics=True, **kw)
    ref = run_navierstokes3D(**kw)
    assert _same_run(a, b) and _same_run(a, c) and not np.array_equal(a[0], ref[0])
    assert any(abs(q) > 0 for q in c[-1].diag[-1].force)
    ctx = a[-1].ctx
    assert ctx.obstacle() is None
    m = S.voxelize(ctx, box, 24, 15, 15)
    ctx.set_obstacle(m)
    assert ctx.obstacle() == m.data_ptr()
    ctx.set_obstacle(None)
    assert ctx.obstacle() is None
    get = lambda r: [hip.to_numpy(getattr(r[0], k)) for k in ("C", "Pr", "Vx", "Vy", "Vz")] + [r[1]]
    g = dict(nx=24, nt=2, dtype=TD[dt], niter_cap=40)
    assert _same_run(get(runme(obstacle=box, one_call=True, **g)), get(runme(obstacle=box, one_call=False, **g)))


# ---- stream order ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(hip):
    return SO.Delay()


def _stream_cases(hip, dt):
    n = (24, 15, 15)
    nx, ny, nz = n
    from navierstokes3d_amd import solid
    tri = np.concatenate([SC.octahedron((11.3, 7.4, 7.0), (9.0, 5.9, 6.2)), solid.box_mesh((2.0, 1.0, 3.0), (4.0, 2.5, 7.0))]).reshape(-1)
    mask0 = np.zeros((nx + 1, ny + 1, nz + 1), dtype=np.uint8, order="F")
    vox = SO.Case("voxelize", [("tri", tri, ("field", 15.0)), ("mask", mask0, "state")],
                  lambda hip, ctx, t: hip.voxelize(t["mask"], t["tri"], n, ctx=ctx))
    C0, Vx, Vy, Vz = fields(*n, ["c", "vx", "vy", "vz"], 21, NP[dt])
    mask = np.asfortranarray(SR.voxelize(tri, *n))
    arrays = [("C", C0, "field"), ("Vx", Vx, "field"), ("Vy", Vy, "field"), ("Vz", Vz, "field"), ("mask", mask, "state")]
    sset = SO.Case("set_solid " + dt, arrays, lambda hip, ctx, t: hip.set_solid(t["C"], t["Vx"], t["Vy"], t["Vz"], t["mask"], ctx=ctx))
    mom = SO.Case("solid_momentum " + dt, arrays[1:], lambda hip, ctx, t: hip.solid_momentum(t["Vx"], t["Vy"], t["Vz"], t["mask"], ctx=ctx),
                  blocking=True)
    return {"voxelize": vox, "set_solid": sset, "solid_momentum": mom}


@pytest.mark.parametrize("name,kind,dt", [("voxelize", "own", "f64"), ("set_solid", "torch", "f32"), ("solid_momentum", "masked", "f64")])
def test_stream_order(hip, delay, name, kind, dt):
    """late input, early reader, on a non-default stream"""
    from test_gpu_stream_order import run_case
    msgs = run_case(hip, _stream_cases(hip, dt)[name], kind, delay)
    assert not msgs, "\n".join(msgs)
