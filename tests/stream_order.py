"""Harness of tests/test_gpu_stream_order.py: does a call read its inputs late enough and finish its outputs early enough — in STREAM
order, on a stream that nothing else serialises?

A case names its device arrays and makes one library call on them.  Every array exists twice on the host: the REAL set (seeded as
the other tests seed theirs) and a DECOY of the same shape and type from another seed — finite, of the same magnitude, tracer
positions inside the box, states in {0, 1}: a call that reads it computes a wrong but harmless result.  The measured run:

  1. the device arrays hold the decoy;
  2. on the context's stream S a DELAY is enqueued (a chain of in-place adds on a scratch tensor), then the copy of the real set into
     the arrays — the inputs arrive late;
  3. the call, with no host synchronisation before it;
  4. on S: a copy of every array into result buffers — the early reader — then the decoy back over every array — the late overwrite;
     S alone is synchronised.  In the variant "sync" nothing follows the call but Context.sync(), and the arrays are read afterwards;
  5. a CANARY on a second stream copies the arrays while the delay should still be running (after the call for calls that only
     enqueue, before it for calls that block): it must hold the decoy's bits, or the delay was too short and the case proves nothing.

The expected bits are those of the same call on the null stream with the real inputs and a synchronisation after it; the same run of
the decoy tells a failure what it is looking at.  Nothing here imports torch at module level: the pure parts are tested on the host
(tests/test_stream_order_host.py).

The multi-rank half (RankCase, expected_ranks, measured_ranks; tests/test_gpu_stream_order_mgpu.py) runs the same five steps on the P
virtual ranks of one MultiGpu: every array exists once per rank, every rank has a decoy set of its own seed, and the delay and the
late copy-in go on the stream each LATE rank computes on — all ranks, or one rank alone, so that its neighbours are on time and only
the wait for the late sender's "ready" event keeps them from pulling the decoy's planes.  Two stream set-ups:
  "follow"  own_streams=False, the call made inside `with torch.cuda.stream(S)`: every rank computes on S;
  "own"     own_streams=True: rank l computes on mg._own[l].  In this set-up MultiGpu._follow_torch_streams synchronises PyTorch's
            CURRENT stream on the host before every call, so the delay and the copy-in must go on mg._own[l], never on the current
            stream: a delay enqueued there would simply be waited for, and the run would prove nothing.
The canary copies the late ranks' arrays on a stream that shares a hardware queue with none of the late ranks' streams — and, when
it is taken after a call that only enqueues, with none of the on-time ranks' either: those wait for the late rank's events by then
(independent_of_all); the verdict is taken rank by rank with the rank in the message (verdict_ranks)."""
import math
from types import SimpleNamespace

import numpy as np

# Target length of the delay per measured call, in milliseconds: four times the smallest value of 5, 10, 20, … at which every canary
# of test_gpu_stream_order.py saw the decoy in three consecutive runs of the module on the MI355X (profiles/stream_order_delay.txt),
# capped at DELAY_CAP_MS.  Measured: 5 ms passed three times, so 4 × 5.  test_gpu_stream_order_mgpu.py is measured by the same rule
# and uses the same constant: the larger of the two modules' values (both measurements are in the profile).
DELAY_MS = 20.0
DELAY_CAP_MS = 200.0
DELAY_BYTES = 64 << 20          # the scratch tensor of the delay's in-place adds
PROBE_MS = 2.0                  # the short delay independent_stream asks its question with


def op_count(target_ms, op_ms):
    """in-place adds of `op_ms` each that last at least `target_ms` (capped): rounds UP, never below one"""
    if not (op_ms > 0.0 and math.isfinite(op_ms)):
        raise ValueError("op_count: one op took %r ms" % (op_ms,))
    return max(1, int(math.ceil(min(float(target_ms), DELAY_CAP_MS) / op_ms)))


# ---- the decoy ---------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.MT19937(int(seed)))


def _magnitude(a, role):
    if isinstance(role, tuple):
        return float(role[1])
    fin = np.abs(a[np.isfinite(a)]) if a.size else np.zeros(0)
    return float(fin.max()) if fin.size and float(fin.max()) > 0.0 else 1.0


def decoy_array(a, role="field", seed=0):
    """A valid stand-in for `a` that differs from it in its bits.  role: 'field' — U(−m, m) with m = max|a| (1 where a is zero), or
    ('field', m) with the magnitude given (a whole time step is run on the decoy: it stays a gentle flow);
    ('points', (ex, ey, ez)) — (3, n) index-space positions uniform in the closed box [0,ex]×[0,ey]×[0,ez]; 'state' — n bytes in
    {0, 1}.  Same shape, type and memory order."""
    a = np.asarray(a)
    rng = _rng(1000003 + seed)
    if role == "state":
        d = (rng.uniform(size=a.shape) < 0.7).astype(a.dtype)
        if a.size and np.array_equal(d, a):
            d.reshape(-1)[0] ^= 1
    elif isinstance(role, tuple) and role[0] == "points":
        ext = np.asarray(role[1], dtype=np.float64).reshape(3, 1)
        d = (rng.uniform(0.0, 1.0, size=a.shape) * ext).astype(a.dtype)
    elif role == "field" or (isinstance(role, tuple) and role[0] == "field"):
        m = _magnitude(a, role)
        d = (rng.uniform(-1.0, 1.0, size=a.shape) * m).astype(a.dtype)
        if a.size and bits_same(d, a):                                   # a one-element array drawn onto its own value
            d.reshape(-1)[0] = a.dtype.type(0.5 * m) if float(a.reshape(-1)[0]) != 0.5 * m else a.dtype.type(-0.5 * m)
    else:
        raise ValueError("decoy_array: role %r" % (role,))
    return np.asfortranarray(d) if a.ndim == 3 else np.ascontiguousarray(d)


def decoy_set(arrays, seed=0):
    """arrays: [(name, host array, role)] → {name: decoy}"""
    return {n: decoy_array(a, role, seed + 17 * q) for q, (n, a, role) in enumerate(arrays)}


def check_decoy(arrays, dec):
    """the properties the cases rely on, as a list of complaints (empty: fine)"""
    bad = []
    for n, a, role in arrays:
        a, d = np.asarray(a), dec[n]
        if d.shape != a.shape or d.dtype != a.dtype:
            bad.append("%s: decoy is %s %s, the array %s %s" % (n, d.dtype, d.shape, a.dtype, a.shape))
            continue
        if a.size and bits_same(d, a):
            bad.append("%s: decoy coincides with the real array" % n)
        if d.dtype.kind == "f" and not np.isfinite(d).all():
            bad.append("%s: decoy is not finite" % n)
        if role == "state" and not np.isin(d, (0, 1)).all():
            bad.append("%s: decoy state outside {0, 1}" % n)
        if isinstance(role, tuple) and role[0] == "points":
            ext = np.asarray(role[1], dtype=np.float64).reshape(3, 1)
            if not ((d >= 0.0) & (d <= ext)).all():
                bad.append("%s: decoy positions outside the box" % n)
        if (role == "field" or (isinstance(role, tuple) and role[0] == "field")) and a.size:
            if float(np.abs(d).max()) > _magnitude(a, role):
                bad.append("%s: decoy exceeds the array's magnitude" % n)
    return bad


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
def bits_same(a, b):
    """np.array_equal(..., equal_nan=True) on arrays of one shape and type (bytes compare as they are)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def same_result(a, b):
    """what a call returns on the host — numbers, tuples, lists, namespaces of them; a NaN equals a NaN"""
    if isinstance(a, SimpleNamespace) and isinstance(b, SimpleNamespace):
        a, b = vars(a), vars(b)
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same_result(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(same_result(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    try:
        return bool(np.array_equal(np.float64(a), np.float64(b), equal_nan=True))
    except (TypeError, ValueError):
        return False


def diagnose(got, want, decoy_run):
    """one of 'ok' | 'equals the decoy run: the inputs were read early' | 'neither the expected bits nor the decoy run's (n of m
    entries differ from the expected ones)'"""
    if bits_same(got, want):
        return "ok"
    if decoy_run is not None and bits_same(got, decoy_run):
        return "equals the decoy run: the inputs were read early"
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "is %s %s, expected %s %s" % (got.dtype, got.shape, want.dtype, want.shape)
    differ = ~((got == want) | ((got != got) & (want != want)))
    return "neither the expected bits nor the decoy run's (%d of %d entries differ from the expected ones)" % (int(differ.sum()), got.size)


def canary_complaints(canary, dec):
    """arrays whose canary copy does not hold the decoy: the delay had run out before the copy-in was overtaken"""
    return [n for n in dec if not bits_same(canary[n], dec[n])]


def verdict(what, got, want, decoy_want, canary, dec, result=None, want_result=None, decoy_result=None):
    """The whole judgement of one measured run as a list of messages (empty: passed).  The canary is judged first: without it the
    rest proves nothing."""
    late = canary_complaints(canary, dec)
    if late:
        return ["%s: delay too short: the case proves nothing (canary of %s does not hold the decoy)" % (what, ", ".join(late))]
    out = []
    for n in want:
        d = diagnose(got[n], want[n], None if decoy_want is None else decoy_want.get(n))
        if d != "ok":
            out.append("%s: %s %s" % (what, n, d))
    if want_result is not None or result is not None:
        if not same_result(result, want_result):
            early = decoy_result is not None and same_result(result, decoy_result)
            out.append("%s: returned %r, expected %r%s" % (what, result, want_result,
                                                           " — equals the decoy run: the inputs were read early" if early else ""))
    return out


# ---- the multi-rank pure parts -----------------------------------------------------------------------------------------------------
RANK_SEED = 1009                # rank l's decoy set is drawn from seed + RANK_SEED·(l + 1): no two ranks share a decoy


def topo_of(topo):
    """(dims or P, (nx, ny, nz)) → (dims or None for z-slabs, P, local grid)"""
    d, n = topo
    n = tuple(int(q) for q in n)
    if isinstance(d, (tuple, list)):
        d = tuple(int(q) for q in d)
        return d, d[0] * d[1] * d[2], n
    return None, int(d), n


def late_sets(P, setup):
    """The sets of late ranks of one case.  "follow": all ranks (they share the stream).  "own": all ranks, then single ranks — rank
    0, rank P−1 and for P = 3 the middle one: the others are on time and would pull early but for the sender's "ready" event.
    More than three ranks with streams of their own leave no hardware queue (four here) for the canary when ALL are late: the lower
    and the upper half are late in turn instead."""
    P = int(P)
    allr = frozenset(range(P))
    if setup == "follow" or P == 1:
        return [allr]
    if setup != "own":
        raise ValueError("late_sets: set-up %r" % (setup,))
    sets = [allr] if P <= 3 else [frozenset(range(P // 2)), frozenset(range(P // 2, P))]
    singles = [0, P - 1] + ([1] if P == 3 else [])
    return sets + [frozenset([l]) for l in singles]


class RankCase:
    """name; topo (dims or P, local grid); arrays [(name, [real host array per rank], role)]; call(hip, mg, t) → host result, t[name]
    the list of device arrays in local-rank order; blocking: the call blocks (canary before it); setup(mg): settings the case needs
    on every MultiGpu it runs on; seed: of the decoys.  real[l] / decoy[l]: {name: array} of rank l."""

    def __init__(self, name, topo, arrays, call, blocking=False, setup=None, seed=0):
        self.name, self.topo, self.call, self.blocking, self.setup, self.seed = name, topo, call, bool(blocking), setup, seed
        self.dims, self.P, self.n = topo_of(topo)
        self.arrays = [(n, [np.asarray(a) for a in per_rank], role) for n, per_rank, role in arrays]
        assert all(len(per_rank) == self.P for _, per_rank, _ in self.arrays), (name, "one array per rank")
        self.names = [n for n, _, _ in self.arrays]
        self.real, self.decoy = [], []
        for l in range(self.P):
            mine = self.rank_arrays(l)
            dec = decoy_set(mine, seed + RANK_SEED * (l + 1))
            bad = check_decoy(mine, dec)
            assert not bad, (name, l, bad)
            self.real.append({n: a for n, a, _ in mine})
            self.decoy.append(dec)
        for n in self.names:                    # … and no rank's decoy is another rank's
            for l in range(self.P):
                for k in range(l):
                    assert not (self.decoy[l][n].size and bits_same(self.decoy[l][n], self.decoy[k][n])), (name, n, l, k)

    def rank_arrays(self, l):
        return [(n, per_rank[l], role) for n, per_rank, role in self.arrays]


def verdict_ranks(what, got, want, decoy_want, canary, decoys, late, result=None, want_result=None, decoy_result=None):
    """verdict() rank by rank.  got / want / decoy_want / decoys: one {name: array} per rank; canary: {rank: {name: array}} of the
    LATE ranks.  Every late rank's canary is judged before anything else: one that does not hold the decoy ends the judgement.  The
    host result belongs to no rank: it is judged once."""
    out = []
    for l in sorted(late):
        out += verdict("%s, rank %d" % (what, l), {}, {}, None, canary[l], decoys[l])
    if out:
        return out
    for l in range(len(want)):
        out += verdict("%s, rank %d" % (what, l), got[l], want[l], None if decoy_want is None else decoy_want[l], {}, {})
    if want_result is not None or result is not None:
        out += verdict(what, {}, {}, None, {}, {}, result, want_result, decoy_result)
    return out


# ---- the device side (torch is imported here, never at module level) -----------------------------------------------------------------
class Case:
    """name; arrays [(name, real host array, role)]; call(hip, ctx, t) → host result, t the dict of device arrays; blocking: the call
    blocks by contract (canary before it); setup(ctx): settings the case needs on every context it runs on; seed: of the decoy."""

    def __init__(self, name, arrays, call, blocking=False, setup=None, seed=0):
        self.name, self.arrays, self.call, self.blocking, self.setup, self.seed = name, list(arrays), call, bool(blocking), setup, seed
        self.real = {n: np.asarray(a) for n, a, _ in self.arrays}
        self.decoy = decoy_set(self.arrays, seed)
        bad = check_decoy(self.arrays, self.decoy)
        assert not bad, (name, bad)


def upload(hip, a):
    import torch
    a = np.asarray(a)
    return hip.from_numpy(a) if a.ndim == 3 else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(hip, t):
    return hip.to_numpy(t) if t.dim() == 3 else t.cpu().numpy()


class Delay:
    """`ms` milliseconds of in-place adds on a scratch tensor, enqueued on whichever stream is asked for.  One op is timed with
    events when the object is made; the number of ops follows from it (op_count)."""

    def __init__(self, ms=None, device=0):
        import torch
        self.ms = DELAY_MS if ms is None else float(ms)
        self.scratch = torch.zeros(DELAY_BYTES // 4, dtype=torch.float32, device="cuda:%d" % device)
        s = torch.cuda.Stream(device)
        reps = 50
        with torch.cuda.stream(s):
            for _ in range(10):
                self.scratch.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                self.scratch.add_(1.0)
            e1.record(s)
        s.synchronize()
        self.op_ms = e0.elapsed_time(e1) / reps
        self.n = op_count(self.ms, self.op_ms)
        self.n_probe = op_count(PROBE_MS, self.op_ms)

    def enqueue(self, stream, ops=None):
        import torch
        with torch.cuda.stream(stream):
            for _ in range(self.n if ops is None else ops):
                self.scratch.add_(1.0)


def independent_stream(busy, delay, avoid=(), tries=12):
    """A torch stream whose work is not held up by work queued on `busy`.  Streams are multiplexed onto a few hardware queues (four by
    default) and a queue takes its streams' work in order, so two non-blocking streams can still serialise; which ones do is the
    runtime's business.  Asked of the device itself: a short delay goes on `busy`, an event on the candidate — free if the event
    completes while `busy` is still at it."""
    import torch
    seen = {busy.cuda_stream} | {a.cuda_stream for a in avoid}
    for _ in range(tries):
        X = torch.cuda.Stream(0)
        if X.cuda_stream in seen:
            continue
        seen.add(X.cuda_stream)
        delay.enqueue(busy, delay.n_probe)
        eb, ex = torch.cuda.Event(), torch.cuda.Event()
        eb.record(busy)
        ex.record(X)
        ex.synchronize()
        free = not eb.query()
        busy.synchronize()
        if free:
            return X
    raise AssertionError("no stream independent of the busy one among %d candidates" % tries)


def context_on(hip, kind, mode="strict", async_=True):
    """(context, the torch stream its launches go to) for kind 'torch' — a torch.cuda.Stream() the context is pinned to, 'own' — the
    context's own stream, 'masked' — the CU-masked stream of reserve_cus(64).  All three are non-blocking streams."""
    import torch
    ctx = hip.Context(0, mode, async_=async_)
    if kind == "torch":
        S = torch.cuda.Stream(0)
        ctx.use_torch_stream(S, pin=True)
    elif kind == "own":
        S = ctx.use_own_stream()
    elif kind == "masked":
        S = ctx.reserve_cus(64)
    else:
        raise ValueError(kind)
    return ctx, S


def sync_run(hip, case, ctx, host):
    """the call on the null stream with `host` as inputs and a synchronisation after it: (result, {name: array})"""
    import torch
    t = {n: upload(hip, host[n]) for n, _, _ in case.arrays}
    torch.cuda.synchronize()
    r = case.call(hip, ctx, t)
    ctx.sync()
    torch.cuda.synchronize()
    return r, {n: download(hip, t[n]) for n in t}


def expected(hip, case, mode="strict"):
    """(result, arrays) of the real set and of the decoy set on a plain synchronous context of `mode`"""
    ctx = hip.Context(0, mode)
    if case.setup:
        case.setup(ctx)
    want = sync_run(hip, case, ctx, case.real)
    dwant = sync_run(hip, case, ctx, case.decoy)
    ctx.close()
    return want, dwant


def warm_up(hip, case, ctx):
    """the same call once on scratch copies, synchronised: modules, lazy scratch and plans exist before the measured call"""
    import torch
    t = {n: upload(hip, case.real[n]) for n, _, _ in case.arrays}
    torch.cuda.current_stream(0).synchronize()
    case.call(hip, ctx, t)
    ctx.sync()


def measured(hip, case, ctx, S, delay, variant="reader", delay_stream=None, read_stream=None, overwrite=True):
    """Steps 1-5 of the module docstring.  delay_stream: where the delay and the copy-in go (default S; another stream in the negative
    controls); read_stream: where the early reader goes (default S).  Returns (result, arrays read, canary)."""
    import torch
    names = [n for n, _, _ in case.arrays]
    t = {n: upload(hip, case.decoy[n]) for n in names}
    real_d = {n: upload(hip, case.real[n]) for n in names}
    dec_d = {n: upload(hip, case.decoy[n]) for n in names}
    res = {n: torch.empty_like(t[n]) for n in names}
    can = {n: torch.empty_like(t[n]) for n in names}
    D = S if delay_stream is None else delay_stream
    R = S if read_stream is None else read_stream
    S2 = independent_stream(D, delay, avoid=(S, R))     # the canary's: must not queue up behind the delay
    torch.cuda.current_stream(0).synchronize()          # the uploads (null stream) are done; from here on no stream waits for another

    def canary():
        with torch.cuda.stream(S2):
            for n in names:
                can[n].copy_(t[n])

    delay.enqueue(D)
    with torch.cuda.stream(D):
        for n in names:
            t[n].copy_(real_d[n])
    if case.blocking:
        canary()
    r = case.call(hip, ctx, t)
    if not case.blocking:
        canary()
    if variant == "reader":
        with torch.cuda.stream(R):
            for n in names:
                res[n].copy_(t[n])
            if overwrite:
                for n in names:
                    t[n].copy_(dec_d[n])
        R.synchronize()
    elif variant in ("sync", "return"):     # "return": a context without NS3D_ASYNC — the call itself has waited
        if variant == "sync":
            ctx.sync()
        with torch.cuda.stream(S2):
            for n in names:
                res[n].copy_(t[n])
    else:
        raise ValueError(variant)
    S2.synchronize()
    D.synchronize()
    S.synchronize()
    return r, {n: download(hip, res[n]) for n in names}, {n: download(hip, can[n]) for n in names}


# ---- the multi-rank device side ----------------------------------------------------------------------------------------------------
def independent_of_all(busy, delay, avoid=(), tries=16):
    """independent_stream for several busy streams: a torch stream that shares a hardware queue with NONE of them (each is asked
    in turn, as independent_stream asks one)."""
    import torch
    distinct = []
    for b in busy:
        if b.cuda_stream not in {d.cuda_stream for d in distinct}:
            distinct.append(b)
    seen = {b.cuda_stream for b in distinct} | {a.cuda_stream for a in avoid}
    for _ in range(tries):
        X = torch.cuda.Stream(0)
        if X.cuda_stream in seen:
            continue
        seen.add(X.cuda_stream)
        free = True
        for b in distinct:
            delay.enqueue(b, delay.n_probe)
            eb, ex = torch.cuda.Event(), torch.cuda.Event()
            eb.record(b)
            ex.record(X)
            ex.synchronize()
            free = not eb.query()
            b.synchronize()
            if not free:
                break
        if free:
            return X
    raise AssertionError("no stream independent of the %d busy ones among %d candidates" % (len(distinct), tries))


def grid_on(hip, case, setup, async_=True):
    """(MultiGpu of the case's topology, [the torch stream rank l computes on], the stream to make the call under or None) for the
    set-up "follow" — every rank follows PyTorch's current stream, which is a new non-default stream S while the call is made — or
    "own" — own_streams=True, rank l on mg._own[l]."""
    import torch
    from navierstokes3d_amd.mgpu import MultiGpu
    torch.cuda.synchronize()
    mg = MultiGpu.create([0] * case.P, *case.n, "strict", async_=async_, dims=case.dims, own_streams=(setup == "own"))
    if case.setup:
        case.setup(mg)
    if setup == "own":
        return mg, list(mg._own), None
    if setup != "follow":
        raise ValueError(setup)
    S = torch.cuda.Stream(0)
    return mg, [S] * case.P, S


def _call(hip, case, mg, t, under):
    import contextlib
    import torch
    with (torch.cuda.stream(under) if under is not None else contextlib.nullcontext()):
        return case.call(hip, mg, t)


def upload_ranks(hip, case, host):
    return {n: [upload(hip, host[l][n]) for l in range(case.P)] for n in case.names}


def sync_run_ranks(hip, case, mg, host):
    """the call as the value tests make it — inputs uploaded, torch.cuda.synchronize(), the call, mg.sync() — with host[l] as rank
    l's arrays: (result, [{name: array} per rank])"""
    import torch
    t = upload_ranks(hip, case, host)
    torch.cuda.synchronize()
    r = case.call(hip, mg, t)
    mg.sync()
    torch.cuda.synchronize()
    return r, [{n: download(hip, t[n][l]) for n in case.names} for l in range(case.P)]


def expected_ranks(hip, case, own):
    """(result, arrays per rank) of the real sets and of the decoy sets on a fresh MultiGpu of the case's topology"""
    mg, _, _ = grid_on(hip, case, "own" if own else "follow")
    want = sync_run_ranks(hip, case, mg, case.real)
    dwant = sync_run_ranks(hip, case, mg, case.decoy)
    mg.sync()
    mg.close()
    return want, dwant


def warm_up_ranks(hip, case, mg, under=None):
    """the same call once on scratch copies, synchronised: lazy buffers (which synchronise every rank when they grow), modules and
    plans exist before the measured call"""
    import torch
    t = upload_ranks(hip, case, case.real)
    torch.cuda.synchronize()
    _call(hip, case, mg, t, under)
    mg.sync()
    torch.cuda.synchronize()


def measured_ranks(hip, case, mg, streams, delay, late, variant="reader", under=None, delay_streams=None, overwrite=True):
    """Steps 1-5 of the module docstring on the ranks of `mg`.  streams[l]: the torch stream rank l computes on; late: the ranks whose
    inputs arrive behind the delay (the others' are copied in on their own stream at once); under: the stream the call is made
    under (set-up "follow"); delay_streams {rank: stream}: where a late rank's delay and copy-in go instead of streams[l] (the
    negative controls).  Returns (result, [arrays read per rank], {late rank: canary})."""
    import torch
    P, names = case.P, case.names
    late = sorted(late)
    t = upload_ranks(hip, case, case.decoy)
    real_d, dec_d = upload_ranks(hip, case, case.real), upload_ranks(hip, case, case.decoy)
    res = {n: [torch.empty_like(x) for x in t[n]] for n in names}
    can = {n: {l: torch.empty_like(t[n][l]) for l in late} for n in names}
    D = [streams[l] if not (delay_streams and l in delay_streams) else delay_streams[l] for l in range(P)]
    # The canary's stream: behind none of the delays.  Taken AFTER a call that only enqueues, it must not queue up behind an on-time
    # rank either: that rank's stream is by then waiting for the late neighbour's events, that is for the delay
    busy = [D[l] for l in late] + ([] if case.blocking else list(streams))
    S2 = independent_of_all(busy, delay, avoid=list(streams) + D)
    torch.cuda.synchronize()                # the uploads (null stream) are done; from here on no stream waits for another

    def canary():
        with torch.cuda.stream(S2):
            for n in names:
                for l in late:
                    can[n][l].copy_(t[n][l])

    delayed = set()
    for l in late:
        if D[l].cuda_stream not in delayed:
            delayed.add(D[l].cuda_stream)
            delay.enqueue(D[l])
    for l in range(P):
        with torch.cuda.stream(D[l]):
            for n in names:
                t[n][l].copy_(real_d[n][l])
    if case.blocking:
        canary()
    r = _call(hip, case, mg, t, under)
    if not case.blocking:
        canary()
    if variant == "reader":
        for l in range(P):
            with torch.cuda.stream(streams[l]):
                for n in names:
                    res[n][l].copy_(t[n][l])
        if overwrite:                       # every rank has read before any rank overwrites only in stream order: that is the point
            for l in range(P):
                with torch.cuda.stream(streams[l]):
                    for n in names:
                        t[n][l].copy_(dec_d[n][l])
        for s in streams:
            s.synchronize()
    elif variant in ("sync", "return"):     # "return": a MultiGpu without NS3D_ASYNC — the call itself has waited
        if variant == "sync":
            mg.sync()
        with torch.cuda.stream(S2):
            for n in names:
                for l in range(P):
                    res[n][l].copy_(t[n][l])
    else:
        raise ValueError(variant)
    S2.synchronize()
    for s in D + list(streams):
        s.synchronize()
    got = [{n: download(hip, res[n][l]) for n in names} for l in range(P)]
    return r, got, {l: {n: download(hip, can[n][l]) for n in names} for l in late}
