"""The NumPy restatement of include/ns3d.h for tracers on a decomposed grid — the ownership rule, the migration order and the cut of
a global field into the ranks' local arrays — on top of tests/tracers_ref.py.  Ranks are numbered in MPI_Cart order (last dimension
fastest); positions are (3, N) float64 in the GLOBAL index space."""
import numpy as np

import tracers_ref as TR


def n_g(dims, n):
    return tuple(int(d) * (int(m) - 2) + 2 for d, m in zip(dims, n))


def coords_of(rank, dims):
    return (rank // (dims[1] * dims[2]), (rank // dims[2]) % dims[1], rank % dims[2])


def origin_of(rank, dims, n):
    return tuple(c * (m - 2) for c, m in zip(coords_of(rank, dims), n))


def seams(dims, n, q):
    """the values k(n−2)+1, k = 1 … D−1, of direction q: a point exactly there belongs to k"""
    return [float(k * (n[q] - 2) + 1) for k in range(1, dims[q])]


def owner_coord(x, D, m):
    """rank coordinate of one direction, written as the header writes it: k owns k(m−2)+1 ≤ x < (k+1)(m−2)+1, k = 0 from 0 (and
    below), k = D−1 up to n_g (and above).  One comparison chain per k, no division.  NaN: 0."""
    x = np.asarray(x, dtype=np.float64)
    k = np.zeros(x.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for kk in range(D):
            lo = x >= float(kk * (m - 2) + 1) if kk > 0 else np.ones(x.shape, dtype=bool)
            hi = x < float((kk + 1) * (m - 2) + 1) if kk < D - 1 else np.ones(x.shape, dtype=bool)
            k[lo & hi] = kk
    return k


def owners(X, dims, n):
    k = [owner_coord(X[q], dims[q], n[q]) for q in range(3)]
    return (k[0] * dims[1] + k[1]) * dims[2] + k[2]


def cut(G, stag, rank, dims, n):
    """the local array of `rank` with its halo: global[o : o + n + s] per direction (a copy, column-major)"""
    o = origin_of(rank, dims, n)
    sl = tuple(slice(o[q], o[q] + n[q] + stag[q]) for q in range(3))
    return np.asfortranarray(G[sl])


def leavers(X, state, ids, me, dims, n):
    """bool per slot: occupied, alive, finite, and owned by another rank"""
    fin = np.isfinite(X).all(axis=0)
    own = owners(np.where(fin, X, 0.0), dims, n)
    return (ids >= 0) & (state == 1) & fin & (own != me), own


def migrate(Xs, states, idss, Us, dims, n):
    """One ns3d_tracers_migrate_mgpu on per-rank slot arrays (lists; Us may be None).  Returns (Xs, states, idss, Us, moved, need):
    new arrays — or, when some rank is short of empty slots, the inputs' copies unchanged with need[l] > 0 there and moved = 0.
    Arrivals at a rank: by source rank ascending, within a source by slot ascending, into the empty slots (those vacated in this
    call included) in ascending slot order."""
    P = len(Xs)
    Xs = [x.copy() for x in Xs]
    states = [s.copy() for s in states]
    idss = [i.copy() for i in idss]
    Us = None if Us is None else [u.copy() for u in Us]
    lv = [leavers(Xs[l], states[l], idss[l], l, dims, n) for l in range(P)]
    arrivals = [[] for _ in range(P)]                      # per destination: (source, slot) in the order of the rule
    for s in range(P):
        go, own = lv[s]
        for slot in np.nonzero(go)[0]:
            arrivals[own[slot]].append((s, slot))
    empty = [np.nonzero((idss[l] < 0) | lv[l][0])[0] for l in range(P)]
    need = [max(0, len(arrivals[l]) - empty[l].size) for l in range(P)]
    if any(need):
        return Xs, states, idss, Us, 0, need
    recs = [[(Xs[s][:, slot].copy(), idss[s][slot], None if Us is None else Us[s][:, slot].copy()) for s, slot in arrivals[l]]
            for l in range(P)]
    for l in range(P):
        go = lv[l][0]
        Xs[l][:, go] = np.nan
        states[l][go] = 0
        idss[l][go] = -1
        if Us is not None:
            Us[l][:, go] = np.nan
    for l in range(P):
        for slot, (x, i, u) in zip(empty[l], recs[l]):
            Xs[l][:, slot] = x
            states[l][slot] = 1
            idss[l][slot] = i
            if Us is not None:
                Us[l][:, slot] = u
    return Xs, states, idss, Us, sum(len(a) for a in arrivals), need


def advance_rank(X, state, Vx, Vy, Vz, c, origin, ng):
    """ns3d_tracers_advance_at on one rank's slots: tests on the global box, interpolation at X − origin"""
    o = np.asarray(origin, dtype=np.float64).reshape(3, 1)
    c = np.asarray(c, dtype=np.float64).reshape(3, 1)
    act = (state == 1) & TR.inside(X, ng)
    Xn = X.copy()
    U = np.full(X.shape, TR.NAN)
    with np.errstate(all="ignore"):
        X0 = X[:, act]
        v1 = TR.velocity(Vx, Vy, Vz, X0 - o)
        Xa = X0 + 0.5 * (v1 * c)
        fin = np.isfinite(Xa).all(axis=0)
        v2 = TR.velocity(Vx, Vy, Vz, Xa[:, fin] - o)
        Xa[:, fin] = X0[:, fin] + v2 * c
    U[:, act] = v1
    Xn[:, act] = Xa
    return Xn, (act & TR.inside(Xn, ng)).astype(np.uint8), U


def distribute(X, state, dims, n, extra=8, keep_velocity=True):
    """per-rank slot arrays of the particles X with ids 0 … N−1, each rank with `extra` empty slots at the end"""
    P = dims[0] * dims[1] * dims[2]
    own = owners(X, dims, n)
    Xs, states, idss, Us = [], [], [], []
    for l in range(P):
        mine = np.nonzero(own == l)[0]
        cap = mine.size + extra
        x = np.full((3, cap), np.nan); x[:, :mine.size] = X[:, mine]
        s = np.zeros(cap, dtype=np.uint8); s[:mine.size] = state[mine]
        i = np.full(cap, -1, dtype=np.int64); i[:mine.size] = mine
        Xs.append(x); states.append(s); idss.append(i); Us.append(np.full((3, cap), np.nan))
    return Xs, states, idss, (Us if keep_velocity else None)


def by_id(per_rank, idss, N, fill=np.nan):
    """per-rank slot arrays → one array over the ids"""
    out = np.full(per_rank[0].shape[:-1] + (N,), fill, dtype=per_rank[0].dtype)
    for v, i in zip(per_rank, idss):
        occ = i >= 0
        out[..., i[occ]] = v[..., occ]
    return out


def planted(dims, n):
    """(X, state): points exactly on every seam value, one ulp below and above, on the global faces, NaN coordinates, a dead one"""
    g = n_g(dims, n)
    mid = [0.37 * g[0], 0.61 * g[1], 0.43 * g[2]]
    cols = []
    for q in range(3):
        vals = [0.0, float(g[q]), np.nextafter(float(g[q]), 0.0), np.nan]
        for s in seams(dims, n, q):
            vals += [s, np.nextafter(s, 0.0), np.nextafter(s, 2 * s), s - 0.5, s + 0.5]
        for v in vals:
            p = list(mid); p[q] = v
            cols.append(p)
    cols.append(list(mid))
    X = np.ascontiguousarray(np.array(cols, dtype=np.float64).T)
    state = np.ones(X.shape[1], dtype=np.uint8)
    state[-1] = 0
    return X, state
