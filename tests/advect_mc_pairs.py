"""Running-error enclosure of the limited MacCormack advection for the FAST build, derived with tests/running_error.py alone.

Per advected node of a field A the pair arithmetic of running_error follows the definition (include/ns3d.h):
  stage 1   Â = running_error.backtrack(A_o, …, dt): where all its comparisons are decided the pair interpolant; elsewhere any
            conforming value lies in the hull [lo, hi] of the candidate stencils, up to the interpolant's bound: the pair
            (mid, half-width + bound)
  stage 2   back = running_error.backtrack(Â, …, −dt) on those pairs (its own undecided nodes: the hull again, widened by the
            largest bound of Â, since that hull is taken over Â's values); s = Â + 0.5·(A_o − back) in pair arithmetic
  limiter   lo, hi are OLD values, exact, and the same in every evaluation that picks stage 1's stencil — it does wherever stage 1's
            three δ are decided; clamping is 1-Lipschitz, so the bound of s is the bound of the result.
Nothing here is fitted to a device's output."""
import functools

import numpy as np

import advect_mc_ref as MC
import running_error as RE

SPACINGS = ("dx", "dy", "dz")


def mc_pairs(old, dt, g, dtype):
    """name → (index tuple of the advected nodes, pair of s, stage 1 decided there, (lo, hi) of the limiter, (lo, hi) over the
    candidate stencils ix1−1 … ix2+1)"""
    P = [RE.field(a) for a in old]
    pdt, sp = RE.scalar(dt, dtype), [RE.spacing(g[n], dtype) for n in SPACINGS]
    nx, ny, nz = old[3].shape
    sets = MC.node_sets(P[0], P[1], P[2], nx, ny, nz)
    exact = MC.node_sets(old[0], old[1], old[2], nx, ny, nz)
    out = {}
    for q, name in enumerate(MC.NAMES):
        IX, IY, IZ, vxc, vyc, vzc = sets[name]
        idx = (IX - 1, IY - 1, IZ - 1)
        val, dec, lo_u, hi_u = RE.backtrack(P[q], vxc, vyc, vzc, pdt, *sp, IX, IY, IZ)
        hat = P[q].copy()
        hat[idx] = RE.Pair(np.where(dec, val.v, 0.5 * (lo_u + hi_u)), np.where(dec, val.e, 0.5 * (hi_u - lo_u) + val.e), hat.u)
        bval, bdec, blo, bhi = RE.backtrack(hat, vxc, vyc, vzc, -pdt, *sp, IX, IY, IZ)
        widest = float(hat.e.max())
        back = RE.Pair(np.where(bdec, bval.v, 0.5 * (blo + bhi)), np.where(bdec, bval.e, 0.5 * (bhi - blo) + widest + bval.e), hat.u)
        s = hat[idx] + 0.5 * (P[q][idx] - back)
        args = (old[q], exact[name], dt, g["dx"], g["dy"], g["dz"])
        out[name] = (idx, s, dec, MC.hull(*args), MC.wide_hull(*args))
    return out


def check(got, ref, pairs, dtype, what):
    """FAST outputs [Vx, Vy, Vz, C] against the enclosure: every advected value inside the hull of the candidate stencils; where stage
    1's δ are decided, within the bound of the limited pair value (float32) or of the reference's output (float64: two conforming
    evaluations).  Returns (decided nodes, all advected nodes, worst err/bound)."""
    k = RE.allowed(dtype)
    n_dec = n_all = 0
    worst = 0.0
    for q, name in enumerate(MC.NAMES):
        idx, s, dec, (lo, hi), (wlo, whi) = pairs[name]
        g64 = got[q][idx].astype(np.float64)
        outside = ~((g64 >= wlo) & (g64 <= whi))
        assert not outside.any(), "%s %s: %d advected values outside the hull of their candidate stencils; first %r" % (
            what, name, int(outside.sum()), tuple(int(x) for x in np.argwhere(outside)[0]))
        lim = np.minimum(np.maximum(s.v, lo.astype(np.float64)), hi.astype(np.float64))
        target = lim if np.dtype(dtype) == np.float32 else ref[q][idx].astype(np.float64)
        err, bound = np.abs(g64 - target), k * s.e
        bad = dec & ~np.where(bound == 0, err == 0, err <= bound)
        if bad.any():
            i = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s %s: %d decided nodes outside the bound; first at %r: got %r, reference %r, bound %.3e" % (
                what, name, int(bad.sum()), i, float(g64[i]), float(target[i]), float(bound[i])))
        with np.errstate(all="ignore"):
            r = np.where(dec & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
        worst = max(worst, float(r.max()))
        n_dec += int(dec.sum()); n_all += dec.size
    return n_dec, n_all, worst


@functools.lru_cache(maxsize=None)
def cached_pairs(grid, cfl, dtype):
    from test_advect_mc_host import seeded
    old, dt, g = seeded(grid, cfl, dtype)
    return mc_pairs(old, dt, g, dtype)
