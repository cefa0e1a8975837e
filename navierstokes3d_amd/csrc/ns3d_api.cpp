// ns3d_api.cpp — the extern "C" boundary of libns3d.so (see include/ns3d.h for the contract and the
// reference file:line each entry point replaces).  Host-only logic: argument checks, mode dispatch
// (strict / fast kernels), the context (stream, reduction scratch, ping-pong buffer) and the
// pseudo-transient loop of multi.jl:458-471 / gpu.jl:126-137.  The typed entry points (ns3d_<name>_f64 / _f32) are
// ns3d_api_typed.h, included once per element type at the end of this file.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <vector>

#include "ns3d_internal.h"

static thread_local char g_err[512] = "";

int ns3d_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// tile choices measured so far in this process (per device and grid): contexts come and go (one per driver call), the
// measurement should not be repeated
// `pinned`: the pass depth that was FORCED when the entry was measured (ns3d_set_pt_depth, or ns3d_slab_plan / box_plan pinning the
// depth their ghosts allow) — 0 for a free choice; `cus_off`: compute units left out of the launches (ns3d_reserve_cus).  Both are
// part of the key: an entry tuned under a pin or a CU mask must not answer a lookup made without it, nor the other way round
// (a forced-depth entry used to supply its depth to later unpinned lookups).
struct Tuned { int device, nx, ny, nz, nk, esize, mode, pinned, cus_off, variant, depth, variantn; };
static std::vector<Tuned> g_tuned;
static std::mutex g_tuned_mutex;

// launch + (unless NS3D_ASYNC) block like `@parallel` does
static int finish(ns3d_ctx *ctx, hipError_t e, const char *what)
{
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e)); }
    if (!(ctx->flags & NS3D_ASYNC)) {
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
    }
    return NS3D_OK;
}

// arithmetic mode of a launch: 2 = FAST, 1 = STRICT with the exact division-by-known-divisor sequence (bit-identical
// to 0, chosen when every spacing passes recip_ok), 0 = STRICT with plain IEEE divisions
static bool recip_ok(double d)
{
    if (!(d > 0x1p-100 && d < 0x1p100)) return false;           // also rejects NaN, 0, negatives
    unsigned long long bits;
    std::memcpy(&bits, &d, sizeof bits);
    if ((bits & 0x000FFFFFFFFFFFFFull) == 0x000FFFFFFFFFFFFFull) return false; // significand all ones
    const float f = (float)d;                                     // the f32 kernels divide by (float)d
    unsigned int fb;
    std::memcpy(&fb, &f, sizeof fb);
    if (!(f > 0x1p-20f && f < 0x1p20f) || (fb & 0x007FFFFFu) == 0x007FFFFFu) return false;
    return true;
}
// d = 2^e exactly with -30 ≤ e ≤ 0: 1/d and 1/d² are exact powers of two ≥ 1 in double and float alike (ns3d_strictp)
static bool pow2_ok(double d)
{
    if (!(d >= 0x1p-30 && d <= 1.0)) return false;
    int e;
    return std::frexp(d, &e) == 0.5;
}
// 3 = STRICT on power-of-two spacings (x/d ≡ x·(1/d), same bits as 0 and 1 with plain multiplications)
static int mode_of(const ns3d_ctx *c, double dx, double dy, double dz)
{
    if (c->flags & NS3D_FAST) return 2;
    if (c->flags & NS3D_IEEE_DIV) return 0;
    if (pow2_ok(dx) && pow2_ok(dy) && pow2_ok(dz)) return 3;
    return (recip_ok(dx) && recip_ok(dy) && recip_ok(dz)) ? 1 : 0;
}
#define DISPATCHM(mode, call)                                                                               \
    ((mode) == 2 ? ns3d_fast::call : (mode) == 3 ? ns3d_strictp::call : (mode) == 1 ? ns3d_strictx::call : ns3d_strict::call)
#define DISPATCH(ctx, call) DISPATCHM(((ctx)->flags & NS3D_FAST) ? 2 : 0, call)      /* kernels without divisions */
#define DISPATCHG(ctx, dx, dy, dz, call) DISPATCHM(mode_of((ctx), (dx), (dy), (dz)), call)

extern "C" {

int ns3d_version(void) { return NS3D_VERSION; }
const char *ns3d_last_error(void) { return g_err; }

ns3d_ctx *ns3d_create(int device, int flags)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        fail(NS3D_ERR_HIP, "ns3d_create: no HIP device (%s) — libns3d has no CPU path", hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(NS3D_ERR_ARG, "ns3d_create: device %d out of range [0,%d)", device, ndev);
        return nullptr;
    }
    ns3d_device_guard guard(device);        // the caller's current device is put back on return
    if (guard.err != hipSuccess) {
        fail(NS3D_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(guard.err));
        return nullptr;
    }
    ns3d_ctx *c = new ns3d_ctx();
    c->device = device;
    c->flags = flags;
    if (const char *ev = std::getenv("NS3D_PT2_VARIANT")) c->pt2_variant = std::atoi(ev);   // experiments without an API call
    if (const char *ev = std::getenv("NS3D_PTN_VARIANT")) c->ptn_variant = std::atoi(ev);
    if (const char *ev = std::getenv("NS3D_PT_DEPTH")) c->pt_depth = std::atoi(ev);
    if (const char *ev = std::getenv("NS3D_GRAPH_MODE")) c->graph_mode = std::atoi(ev);     // A/B without an API call
    if (const char *ev = std::getenv("NS3D_PT_PERSIST")) c->persist_mode = std::atoi(ev);
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc((void **)&c->key_dev, 64)) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->key_host, 64, hipHostMallocDefault)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->fence, hipEventDisableTiming)) != hipSuccess) {
        fail(NS3D_ERR_HIP, "ns3d_create: %s", hipGetErrorString(e));
        ns3d_destroy(c);                    // releases whatever was created so far
        return nullptr;
    }
    c->stream = c->own_stream;
    if (const char *ev = std::getenv("NS3D_RESERVE_CUS"))
        if (std::atoi(ev) > 0 && ns3d_reserve_cus(c, std::atoi(ev)) != NS3D_OK) { ns3d_destroy(c); return nullptr; }
    return c;
}

void ns3d_destroy(ns3d_ctx *c)
{
    if (!c) return;
    ns3d_device_guard guard(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    c->clear_graphs();
    if (c->persist.H) (void)hipFree(c->persist.H);
    if (c->pace.ctr) (void)hipFree(c->pace.ctr);
    if (c->persist.err_host) (void)hipHostFree(c->persist.err_host);
    if (c->persist.ev) (void)hipEventDestroy(c->persist.ev);
    c->direct.release();
    if (c->fence) (void)hipEventDestroy(c->fence);
    for (int q = 0; q < 2; ++q)
        if (c->tune_ev[q]) (void)hipEventDestroy(c->tune_ev[q]);
    if (c->diag_host) (void)hipHostFree(c->diag_host);
    if (c->key_dev) (void)hipFree(c->key_dev);
    if (c->key_host) (void)hipHostFree(c->key_host);
    if (c->masked_stream) { (void)hipStreamSynchronize(c->masked_stream); (void)hipStreamDestroy(c->masked_stream); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                               // the ns3d_scratch members go here: the device is current, the streams have been waited for
}

int ns3d_flags(const ns3d_ctx *c) { return c ? c->flags : -1; }

// A context waits for the stream it leaves.  What it remembers is ordered by the stream it launches on and by nothing else: the
// ping-pong, advection-hat, monitor, isosurface and voxelizer scratch (freed when it grows, after a wait for c->stream — and, for
// the ping-pong and the hat, c->own_stream — only), the key word of the residual read-backs, k_pt_persist's exchange area and the
// pace counters (reset by fills on the launch's stream).  Work of an NS3D_ASYNC context still queued on a stream the context no longer names would meet all of these unordered.  A stream that
// is being captured runs nothing and is not waited for, and there is no wait either while the stream moved TO is being captured.
static int leave_stream(ns3d_ctx *c, hipStream_t next)
{
    if (c->stream == next) return NS3D_OK;
    ns3d_device_guard guard(c->device);
    // neither end of the move may be under capture: a captured stream runs nothing, and a synchronisation made by the thread that
    // is capturing `next` (a context following the caller's stream into the caller's capture) would invalidate that capture
    for (hipStream_t q : {c->stream, next}) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(q, &cap) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (cap != hipStreamCaptureStatusNone) return NS3D_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NS3D_OK;
}
int ns3d_set_stream(ns3d_ctx *c, void *s)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_stream: null context");
    if (const int rc = leave_stream(c, (hipStream_t)s)) return rc;
    c->stream = (hipStream_t)s;
    return NS3D_OK;
}
int ns3d_use_own_stream(ns3d_ctx *c)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_use_own_stream: null context");
    if (const int rc = leave_stream(c, c->own_stream)) return rc;
    c->stream = c->own_stream;
    return NS3D_OK;
}
void *ns3d_get_stream(ns3d_ctx *c) { return c ? (void *)c->stream : nullptr; }

// CU mask: bit i of the mask words = compute unit i as the runtime numbers them.  How those numbers map onto the 8 XCDs is not
// documented for this part, so both plausible layouts exist (NS3D_RESERVE_CUS_LAYOUT): 0 = numbers interleave the XCDs (CU i sits
// on XCD i mod 8: drop the n highest numbers), 1 = 32 consecutive numbers per XCD (drop the n/8 highest of every 32).  Measured
// (profiles/r4_cu_mask_ab.log): the interleaved reading is the one under which the masked sweep loses time in proportion to the CUs.
int ns3d_reserve_cus(ns3d_ctx *c, int n)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_reserve_cus: null context");
    ns3d_device_guard guard(c->device);
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    if (n < 0 || n > cus / 2) return fail(NS3D_ERR_ARG, "ns3d_reserve_cus: %d of %d compute units (0 … half the device)", n, cus);
    n = (n + 7) / 8 * 8;
    if (n != c->reserved_cus && !c->graphs.empty()) {
        // a captured block holds the z-chunking of the CU count it was captured for: it is captured again for the new one
        if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        c->clear_graphs();
    }
    if (c->masked_stream) {
        HIPCHK(c, hipStreamSynchronize(c->masked_stream));
        if (c->stream == c->masked_stream) c->stream = c->own_stream;
        c->clear_graphs();
        HIPCHK(c, hipStreamDestroy(c->masked_stream));
        c->masked_stream = nullptr;
        c->reserved_cus = 0;
    }
    if (n == 0) return NS3D_OK;
    static const int layout = std::getenv("NS3D_RESERVE_CUS_LAYOUT") ? std::atoi(std::getenv("NS3D_RESERVE_CUS_LAYOUT")) : 0;
    const int words = (cus + 31) / 32;
    std::vector<uint32_t> mask((size_t)words, 0u);
    for (int i = 0; i < cus; ++i) {
        bool keep;
        if (layout == 1) keep = (i % 32) < 32 - n / 8 || cus % 32 != 0;      // n/8 off the top of every 32-CU group
        else keep = i < cus - n;                                               // the n highest numbers
        if (keep) mask[(size_t)(i / 32)] |= 1u << (i % 32);
    }
    HIPCHK(c, hipExtStreamCreateWithCUMask(&c->masked_stream, (uint32_t)words, mask.data()));
    if (const int rc = leave_stream(c, c->masked_stream)) {
        (void)hipStreamDestroy(c->masked_stream);
        c->masked_stream = nullptr;
        return rc;
    }
    c->reserved_cus = n;
    c->stream = c->masked_stream;
    return NS3D_OK;
}
int ns3d_reserved_cus(const ns3d_ctx *c) { return c ? c->reserved_cus : -1; }

int ns3d_sync(ns3d_ctx *c)
{
    CHECK_CTX(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return NS3D_OK;
}

int ns3d_set_pt_variant(ns3d_ctx *c, int v)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_pt_variant: null context");
    if (v < 0 || v >= 10000) return fail(NS3D_ERR_ARG, "ns3d_set_pt_variant: unknown variant %d", v);
    c->pt_variant = v;
    return NS3D_OK;
}

int ns3d_set_graph_mode(ns3d_ctx *c, int mode)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_graph_mode: null context");
    c->graph_mode = mode < 0 ? -1 : (mode > 0 ? 1 : 0);
    return NS3D_OK;
}

int ns3d_set_autotune(ns3d_ctx *c, int on)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_autotune: null context");
    c->autotune = on ? 1 : 0;
    return NS3D_OK;
}

int ns3d_last_pt2_variant(const ns3d_ctx *c) { return c ? c->last_pt2 : -1; }
int ns3d_last_ptn_variant(const ns3d_ctx *c) { return c ? c->last_ptn : -1; }
int ns3d_last_pt_depth(const ns3d_ctx *c) { return c ? c->last_depth : -1; }
int ns3d_set_persist_mode(ns3d_ctx *c, int mode)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_persist_mode: null context");
    if (mode < -1 || mode > 1) return fail(NS3D_ERR_ARG, "ns3d_set_persist_mode: %d (-1 auto, 0 off, 1 on)", mode);
    c->persist_mode = mode;
    return NS3D_OK;
}
int ns3d_cached_graphs(const ns3d_ctx *c) { return c ? (int)c->graphs.size() : -1; }
int ns3d_arith_build(const ns3d_ctx *c, double dx, double dy, double dz) { return c ? mode_of(c, dx, dy, dz) : -1; }

int ns3d_set_ptn_variant(ns3d_ctx *c, int v)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_ptn_variant: null context");
    if (v < 0 || v >= 10000) return fail(NS3D_ERR_ARG, "ns3d_set_ptn_variant: unknown variant %d", v);
    c->ptn_variant = v;
    return NS3D_OK;
}

int ns3d_persist_faults(const ns3d_ctx *c) { return c ? (int)c->persist.faults : -1; }
int ns3d_last_pt_pace(const ns3d_ctx *c) { return c ? c->pace.last : -1; }
int ns3d_set_pt_pace(ns3d_ctx *c, int pace_z)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_pt_pace: null context");
    if (pace_z < -1 || (pace_z > 0 && pace_z % 4 != 0)) return fail(NS3D_ERR_ARG, "ns3d_set_pt_pace: %d z-steps (-1, 0 or a multiple of 4)", pace_z);
    c->pace.pace_z = pace_z;
    return NS3D_OK;
}
int ns3d_set_pt_pace_test(ns3d_ctx *c, int extra_arrivals, int ticks)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_pt_pace_test: null context");
    if (extra_arrivals < 0) return fail(NS3D_ERR_ARG, "ns3d_set_pt_pace_test: %d extra arrivals", extra_arrivals);
    c->pace.test_extra = extra_arrivals;
    c->pace.ticks = ticks > 0 ? ticks : NS3D_PACE_TICKS_DEFAULT;
    return NS3D_OK;
}
int ns3d_set_pt_depth(ns3d_ctx *c, int depth)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_pt_depth: null context");
    if (depth < 0 || depth > 5) return fail(NS3D_ERR_ARG, "ns3d_set_pt_depth: depth %d (0 = automatic, 1…4; 5: float32 fields only)", depth);
    c->pt_depth = depth;
    return NS3D_OK;
}

int ns3d_set_advection(ns3d_ctx *c, int scheme)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_advection: null context");
    if (scheme != NS3D_ADVECT_REFERENCE && scheme != NS3D_ADVECT_MACCORMACK)
        return fail(NS3D_ERR_ARG, "ns3d_set_advection: scheme %d (NS3D_ADVECT_REFERENCE | NS3D_ADVECT_MACCORMACK)", scheme);
    c->advection = scheme;
    return NS3D_OK;
}
int ns3d_advection(const ns3d_ctx *c) { return c ? c->advection : -1; }

int ns3d_set_obstacle(ns3d_ctx *c, const unsigned char *mask)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_obstacle: null context");
    c->obstacle = mask;
    return NS3D_OK;
}
const unsigned char *ns3d_obstacle(const ns3d_ctx *c) { return c ? c->obstacle : nullptr; }

int ns3d_set_obstacle_motion(ns3d_ctx *c, const double *motion9, const int *origin)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_obstacle_motion: null context");
    if (!motion9) {
        c->motion_on = 0;
        for (int q = 0; q < 9; ++q) c->motion[q] = 0.0;
        for (int q = 0; q < 3; ++q) c->motion_origin[q] = 0;
        return NS3D_OK;
    }
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(motion9[q])) return fail(NS3D_ERR_ARG, "ns3d_set_obstacle_motion: motion[%d] = %g is not finite", q, motion9[q]);
    if (origin && (origin[0] < 0 || origin[1] < 0 || origin[2] < 0))
        return fail(NS3D_ERR_ARG, "ns3d_set_obstacle_motion: origin %d, %d, %d (each >= 0)", origin[0], origin[1], origin[2]);
    c->motion_on = 1;
    for (int q = 0; q < 9; ++q) c->motion[q] = motion9[q];
    for (int q = 0; q < 3; ++q) c->motion_origin[q] = origin ? origin[q] : 0;
    return NS3D_OK;
}
int ns3d_obstacle_motion(const ns3d_ctx *c, double *out9)
{
    if (!c) return -1;
    if (c->motion_on && out9)
        for (int q = 0; q < 9; ++q) out9[q] = c->motion[q];
    return c->motion_on;
}

int ns3d_set_turbulence(ns3d_ctx *c, int model, double length, void *mu_e)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_turbulence: null context");
    if (model == NS3D_TURB_NONE) {
        c->turbulence = NS3D_TURB_NONE; c->turb_length = 0.0; c->turb_mu_e = nullptr;
        return NS3D_OK;
    }
    if (model != NS3D_TURB_SMAGORINSKY)
        return fail(NS3D_ERR_ARG, "ns3d_set_turbulence: model %d (NS3D_TURB_NONE | NS3D_TURB_SMAGORINSKY)", model);
    if (!(std::isfinite(length) && length >= 0.0))
        return fail(NS3D_ERR_ARG, "ns3d_set_turbulence: length = %g (need a finite value >= 0)", length);
    if (!mu_e) return fail(NS3D_ERR_ARG, "ns3d_set_turbulence: a model needs the mu_e array");
    c->turbulence = model; c->turb_length = length; c->turb_mu_e = mu_e;
    return NS3D_OK;
}
int ns3d_turbulence(const ns3d_ctx *c) { return c ? c->turbulence : -1; }
int ns3d_set_sgs_operator(ns3d_ctx *c, int op)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_sgs_operator: null context");
    if (op != NS3D_SGS_SMAGORINSKY && op != NS3D_SGS_WALE && op != NS3D_SGS_VREMAN)
        return fail(NS3D_ERR_ARG, "ns3d_set_sgs_operator: operator %d (NS3D_SGS_SMAGORINSKY | NS3D_SGS_WALE | NS3D_SGS_VREMAN)", op);
    c->sgs_operator = op;
    return NS3D_OK;
}
int ns3d_sgs_operator(const ns3d_ctx *c) { return c ? c->sgs_operator : -1; }

int ns3d_set_scalar(ns3d_ctx *c, int on, double kappa, double sct, double bg, double c_ref)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_scalar: null context");
    if (!(std::isfinite(kappa) && std::isfinite(sct) && std::isfinite(bg) && std::isfinite(c_ref)))
        return fail(NS3D_ERR_ARG, "ns3d_set_scalar: kappa = %g, sct = %g, bg = %g, c_ref = %g (need finite values)", kappa, sct, bg, c_ref);
    if (!(kappa >= 0.0 && sct >= 0.0))
        return fail(NS3D_ERR_ARG, "ns3d_set_scalar: kappa = %g, sct = %g (need values >= 0)", kappa, sct);
    if (!on) {
        c->scalar_on = 0; c->scalar_kappa = c->scalar_sct = c->scalar_bg = c->scalar_c_ref = 0.0;
        return NS3D_OK;
    }
    c->scalar_on = 1; c->scalar_kappa = kappa; c->scalar_sct = sct; c->scalar_bg = bg; c->scalar_c_ref = c_ref;
    return NS3D_OK;
}
int ns3d_scalar(const ns3d_ctx *c) { return c ? c->scalar_on : -1; }

int ns3d_set_pt2_variant(ns3d_ctx *c, int v)
{
    if (!c) return fail(NS3D_ERR_ARG, "ns3d_set_pt2_variant: null context");
    if (v >= 10000) return fail(NS3D_ERR_ARG, "ns3d_set_pt2_variant: unknown variant %d", v);
    c->pt2_variant = v;
    return NS3D_OK;
}

} // extern "C"

// read back a reduction key: 8-byte D2H into pinned memory + stream sync (the only host round trip of the PT loop)
static int fetch_key(ns3d_ctx *c, hipStream_t s, double *out)
{
    HIPCHK(c, hipMemcpyAsync(c->key_host, c->key_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    double v;
    std::memcpy(&v, c->key_host, sizeof v);
    *out = v;
    return NS3D_OK;
}

// ---- ns3d_diagnostics ------------------------------------------------------------------------------------------------
int ns3d_diag_check(const ns3d_diag_params *p, const char *fn)
{
    if (!p) return fail(NS3D_ERR_ARG, "%s: null parameters", fn);
    if (p->nx < 3 || p->ny < 3 || p->nz < 3)
        return fail(NS3D_ERR_ARG, "%s: grid %dx%dx%d too small (need >= 3 per direction)", fn, p->nx, p->ny, p->nz);
    if (p->cylinder < 0 || p->cylinder > 2) return fail(NS3D_ERR_ARG, "%s: cylinder form %d (0 none | 1 multi.jl | 2 gpu.jl)", fn, p->cylinder);
    return NS3D_OK;
}
template <class T>
int ns3d_diag_enqueue(ns3d_ctx *c, const T *Vx, const T *Vy, const T *Vz, const T *Pr, const T *C, const ns3d_diag_params *p)
{
    const size_t need = NS3D_DIAG_RESULT_WORDS + (size_t)NS3D_DIAG_SLOTS * ns3d_diag_geometry(p->nx, p->ny, p->nz, nullptr);
    if (!c->diag_host) HIPCHK(c, hipHostMalloc((void **)&c->diag_host, NS3D_DIAG_RESULT_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
    if (const int rc = c->diag_dev.reserve(need * sizeof(unsigned long long), ns3d_drain_stream(c))) return rc;
    unsigned long long *words = c->diag_dev.as<unsigned long long>();
    hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz, diagnostics<T>(c->stream, Vx, Vy, Vz, Pr, C, *p, words + NS3D_DIAG_RESULT_WORDS, words));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "diagnostics launch: %s", hipGetErrorString(e)); }
    HIPCHK(c, hipMemcpyAsync(c->diag_host, words, NS3D_DIAG_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return NS3D_OK;
}
template int ns3d_diag_enqueue<double>(ns3d_ctx *, const double *, const double *, const double *, const double *, const double *, const ns3d_diag_params *);
template int ns3d_diag_enqueue<float>(ns3d_ctx *, const float *, const float *, const float *, const float *, const float *, const ns3d_diag_params *);
static double diag_f64(unsigned long long w) { double v; std::memcpy(&v, &w, sizeof v); return v; }
static double diag_unkey(unsigned long long k)      // inverse of ord_key (ns3d_kernels.hip); 0 = nothing was reduced
{
    if (k == ~0ull || k == 0ull) return NAN;
    return diag_f64((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}
void ns3d_diag_decode(const unsigned long long *w, const ns3d_diag_params *p, bool has_pr, bool has_c, ns3d_diag *out)
{
    const double dV = p->dx * p->dy * p->dz;
    out->ke = diag_f64(w[0]) * (0.5 * p->rho * dV);
    out->c_vol = has_c ? diag_f64(w[1]) * dV : NAN;
    for (int q = 0; q < 3; ++q) {
        out->mom[q] = diag_f64(w[2 + q]);
        out->n_masked[q] = (long long)w[5 + q];
        out->vmax[q] = diag_f64(w[8 + q]);          // abs_key: the bit pattern of a non-negative double, NaN = 0x7FF8…
    }
    out->div_max = diag_f64(w[11]);
    out->pr_max = has_pr ? diag_unkey(w[12]) : NAN;
    out->pr_min = has_pr ? -diag_unkey(w[13]) : NAN;
    out->nonfinite = w[14] != 0ull;
}

// ---- ns3d_stats_* : running mean / Reynolds-stress fields (the state belongs to the caller) ----------------------------------
static int stats_grid_check(int nx, int ny, int nz, const char *fn)
{
    if (nx < 3 || ny < 3 || nz < 3) return fail(NS3D_ERR_ARG, "%s: grid %dx%dx%d too small (need >= 3 per direction)", fn, nx, ny, nz);
    return NS3D_OK;
}
extern "C" int ns3d_stats_reset(ns3d_ctx *c, double *S, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(S);
    const int rc = stats_grid_check(nx, ny, nz, "ns3d_stats_reset");
    if (rc) return rc;
    return finish(c, hipMemsetAsync(S, 0, (size_t)NS3D_STATS_SLOTS * nx * ny * nz * sizeof(double), c->stream), "stats_reset");
}
extern "C" int ns3d_stats_finalize(ns3d_ctx *c, const double *S, double wsum, double *mean, double *rs, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(S, mean);
    const int rc = stats_grid_check(nx, ny, nz, "ns3d_stats_finalize");
    if (rc) return rc;
    if (!std::isfinite(wsum) || !(wsum > 0.0)) return fail(NS3D_ERR_ARG, "ns3d_stats_finalize: wsum = %g (need a finite sum of weights > 0)", wsum);
    return finish(c, DISPATCH(c, stats_finalize(c->stream, S, wsum, mean, rs, (long)nx * ny * nz)), "stats_finalize");
}

// After a synchronisation of the stream the persist launches ran on: did a bounded wait expire in any of them since the last check?
// (k_pt_persist writes its ticket into pinned host memory when one does.)  A failure turns the cooperative form off for this context:
// what made the workgroups non-resident — another context or process holding CUs — is unlikely to have gone away.
static bool persist_failed(ns3d_ctx *c)
{
    ns3d_persist_state &ps = c->persist;
    if (!ps.err_host || ps.checked == ps.ticket) return false;
    const unsigned seen = *(volatile unsigned *)ps.err_host;
    const bool failed = seen != 0u && (int)(seen - ps.checked) > 0 && (int)(seen - ps.ticket) <= 0;
    ps.checked = ps.ticket;
    if (failed) { ++ps.faults; c->persist_mode = 0; }
    return failed;
}

int ns3d_check_pt_params(const ns3d_pt_params *p, const char *fn)
{
    if (!p) return fail(NS3D_ERR_ARG, "%s: null params", fn);
    if (p->nx < 3 || p->ny < 3 || p->nz < 3)
        return fail(NS3D_ERR_ARG, "%s: grid %dx%dx%d too small for the fused PT sweep (need >= 3)", fn, p->nx, p->ny,
                    p->nz);
    if (p->bc_kind != NS3D_BC_MULTI && p->bc_kind != NS3D_BC_GPU) return fail(NS3D_ERR_ARG, "%s: bad bc_kind %d", fn, p->bc_kind);
    if (p->bc_kind == NS3D_BC_GPU && (p->z_lo_is_halo || p->z_hi_is_halo))
        return fail(NS3D_ERR_ARG, "%s: gpu.jl boundary set is single-device (no z halos)", fn);
    return NS3D_OK;
}

// Temporal blocking pays from ≈1.5 M cells on (128³: 137 000 against 113 000 Mcells·iter/s, 160³: 169 000 against 124 000;
// 127×76×76 = 0.7 M cells: 55 000 against 70 000 — there the one-thread-per-cell sweep has more parallelism);
// an explicit ns3d_set_pt2_variant(ctx, v>0) forces it, v<0 disables it.
static const long long NS3D_TWO_MIN_CELLS = 1500ll * 1000;
static bool use_two(const ns3d_ctx *c, const ns3d_pt_params *p)
{
    if (c->pt2_variant < 0 || c->pt_depth == 1) return false;
    if (c->pt2_variant > 0 || c->pt_depth >= 2) return true;
    return (long long)p->nx * p->ny * p->nz >= NS3D_TWO_MIN_CELLS;
}

// The drain of the ping-pong and hat buffers: whatever may still use the old one — either stream, a captured block — goes first
static auto drain_streams_and_graphs(ns3d_ctx *c)
{
    return [c]() -> int {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        c->clear_graphs();
        return NS3D_OK;
    };
}
// the second Pr buffer (every cell) and the second dPrdτ buffer (interior cells) of the PT loop
template <class T>
static int ensure_pingpong(ns3d_ctx *c, const ns3d_pt_params *p, T **buf)
{
    const int rc = c->pingpong.reserve((size_t)p->nx * p->ny * p->nz * sizeof(T), drain_streams_and_graphs(c));
    if (!rc) *buf = c->pingpong.as<T>();
    return rc;
}
template <class T>
static int ensure_pingpong_d(ns3d_ctx *c, const ns3d_pt_params *p, T **buf)
{
    const int rc = c->pingpong_d.reserve((size_t)(p->nx - 2) * (p->ny - 2) * (p->nz - 2) * sizeof(T), drain_streams_and_graphs(c));
    if (!rc) *buf = c->pingpong_d.as<T>();
    return rc;
}

// the hat fields of ns3d_time_step's MacCormack advection: stage 1's Vx, Vy, Vz, C of an nx×ny×nz grid, one after the other
template <class T>
static int ensure_mc_hat(ns3d_ctx *c, int nx, int ny, int nz, T *hat[4])
{
    const size_t n[4] = {(size_t)(nx + 1) * ny * nz, (size_t)nx * (ny + 1) * nz, (size_t)nx * ny * (nz + 1), (size_t)nx * ny * nz};
    const int rc = c->mc_hat.reserve((n[0] + n[1] + n[2] + n[3]) * sizeof(T), drain_streams_and_graphs(c));
    if (rc) return rc;
    T *p = c->mc_hat.as<T>();
    for (int q = 0; q < 4; ++q) { hat[q] = p; p += n[q]; }
    return NS3D_OK;
}

// ---- tile shape of the two-iteration sweep ------------------------------------------------------------------
// Every shape gives the same bits (tests/test_gpu_pt.py), and which one is fastest depends on how the row length
// divides into 64/128/256-wide tiles and on how many workgroups the grid yields (profiles/r1b_shapes.log: 128×8 with
// two workgroups per CU wins at 255×153×153 and 384³, 256×8 at 512³ and 1024³).  So the first automatic launch on a
// grid times the candidates on the caller's own arguments — the operation is idempotent: inputs and outputs are
// distinct buffers — and remembers the winner in the context.  Skipped (built-in choice by grid instead) while the
// stream is being captured, for launches under 1.5 M cells, after ns3d_set_autotune(ctx, 0), or with an explicit variant.
// How a pass over memory is made: PT iterations per pass (depth 2: k_pt_sweep2 with tile variant v2; 3, 4: k_pt_sweepN with
// tile variant vn).  Explicit settings (ns3d_set_pt2_variant / _ptn_variant / _pt_depth) always win.
struct Plan { int depth, v2, vn; bool known; };
// Below this the planner does not time deeper passes.  Round 4 lowered it from 8 M to 3 M cells: on the reference's own 255×153×153
// grid (6.0 M cells) three iterations per pass run 34 % faster than two in FAST mode (2800: 17.8 against 23.8 µs per iteration;
// profiles/r4_midsize.log) — the round-2 finding "stays at two" held for the exact-division STRICT build only, which is
// VALU-bound there (29.8 against 28.4) and keeps two because the planner measures head to head.  127×77×77 (0.75 M): two.
static const long long NS3D_DEEP_MIN_CELLS = 3ll * 1000 * 1000;
template <class T>
static Plan lookup_plan(const ns3d_ctx *c, int mode, const ns3d_pt_params *p, int k0, int k1)
{
    Plan pl{c->pt_depth > 0 ? c->pt_depth : 2, c->pt2_variant > 0 ? c->pt2_variant : 0, c->ptn_variant, true};
    if (sizeof(T) == 8 && pl.depth > 4) pl.depth = 4;       // the fifth level exists for float32 fields only
    const int nk = k1 - k0;
    const long long cells = (long long)p->nx * p->ny * nk;
    if (!c->autotune || cells < NS3D_TWO_MIN_CELLS) return pl;
    if (c->pt2_variant > 0 && (c->pt_depth > 0 || cells < NS3D_DEEP_MIN_CELLS)) return pl;      // nothing left to decide
    if (c->pt_depth >= 3 && c->ptn_variant > 0) return pl;                                      // deep passes, shape given
    std::lock_guard<std::mutex> lock(g_tuned_mutex);
    for (const auto &t : g_tuned)
        if (t.device == c->device && t.nx == p->nx && t.ny == p->ny && t.nz == p->nz && t.nk == nk &&
            t.esize == (int)sizeof(T) && t.mode == mode && t.pinned == c->pt_depth && t.cus_off == c->reserved_cus) {
            if (c->pt2_variant <= 0) pl.v2 = t.variant;
            if (c->pt_depth <= 0) pl.depth = t.depth;
            if (c->ptn_variant <= 0) pl.vn = t.variantn;
            return pl;
        }
    pl.known = false;
    return pl;
}
// the measurement: runs on the caller's own arguments (idempotent: inputs and outputs are distinct buffers), blocks on
// its events.  Called from ns3d_plan_pt, ns3d_pt_iterate and ns3d_pt_solve only — never from ns3d_pt_sweep2 / _sweepn, whose
// callers (z-slab schedules with an exchange in flight) must not be stalled by ≈100 extra launches.
template <class T>
static Plan tune_plan(ns3d_ctx *c, hipStream_t s, int mode, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                      const ns3d_pt_params *p, int k0, int k1)
{
    Plan pl = lookup_plan<T>(c, mode, p, k0, k1);
    pl.known = true;
    const int nk = k1 - k0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return pl; }
    if (cap != hipStreamCaptureStatusNone) return pl;
    for (int q = 0; q < 2; ++q)
        if (!c->tune_ev[q] && hipEventCreate(&c->tune_ev[q]) != hipSuccess) { (void)hipGetLastError(); return pl; }
    // `depth` iterations per launch; ms = time of ONE launch
    auto time_launch = [&](int depth, int v, float &ms, int timed = 3) -> bool {
        bool ok = true;
        for (int rep = 0; rep <= timed && ok; ++rep) {     // one untimed launch, then `timed` timed ones
            if (rep == 1) ok = hipEventRecord(c->tune_ev[0], s) == hipSuccess;
            const int tf = ns3d_pass_flags_cus(c->reserved_cus);      // compute units the launch must not count on
            hipError_t e = depth == 2 ? DISPATCHM(mode, pt_sweep2<T>(s, v, src, dst, dsrc, ddst, divV, *p, k0, k1, tf))
                                      : DISPATCHM(mode, pt_sweepn<T>(s, depth, v, src, dst, dsrc, ddst, divV, *p, k0, k1, tf, nullptr, &c->pace));
            ok = ok && e == hipSuccess;
        }
        ok = ok && hipEventRecord(c->tune_ev[1], s) == hipSuccess && hipEventSynchronize(c->tune_ev[1]) == hipSuccess &&
             hipEventElapsedTime(&ms, c->tune_ev[0], c->tune_ev[1]) == hipSuccess;
        ms /= (float)timed;
        if (!ok) (void)hipGetLastError();
        return ok;
    };
    // ---- two iterations per pass: variant = shape*100 + kz (ns3d.h).  Stage 1: every shape with round-filling chunks (92)
    // and with short 16-plane chunks (which keep neighbouring tiles close in time: their overlaps then hit the L2); stage 2:
    // the other chunk lengths for the three best shapes.  0 = the built-in choice; it wins ties.
    float ms2 = 0.f;                                       // per launch of the chosen two-iteration variant
    if (c->pt2_variant > 0) {
        if (!time_launch(2, pl.v2, ms2, 6) || !time_launch(2, pl.v2, ms2)) return pl;
    } else {
        static const int shapes[] = {11, 8, 9, 7, 13, 19, 12};
        static const int stage1[] = {92, 16}, stage2[] = {94, 91, 98, 32};
        constexpr int NS = (int)(sizeof shapes / sizeof shapes[0]);
        int best = 0;
        float best_ms = 0.f, ms = 0.f, shape_ms[NS];
        if (!time_launch(2, 0, best_ms, 6)) return pl;     // also brings the clocks up
        if (!time_launch(2, 0, best_ms)) return pl;
        for (int q = 0; q < NS; ++q) {
            shape_ms[q] = 0.f;
            for (int kz : stage1) {
                if (!time_launch(2, shapes[q] * 100 + kz, ms)) return pl;
                if (shape_ms[q] == 0.f || ms < shape_ms[q]) shape_ms[q] = ms;
                if (ms < 0.99f * best_ms) { best_ms = ms; best = shapes[q] * 100 + kz; }
            }
        }
        for (int pick = 0; pick < 3; ++pick) {
            int q = -1;
            for (int r = 0; r < NS; ++r)
                if (shape_ms[r] > 0.f && (q < 0 || shape_ms[r] < shape_ms[q])) q = r;
            if (q < 0) break;
            shape_ms[q] = 0.f;                             // taken
            for (int kz : stage2) {
                if (!time_launch(2, shapes[q] * 100 + kz, ms)) return pl;
                if (ms < 0.99f * best_ms) { best_ms = ms; best = shapes[q] * 100 + kz; }
            }
        }
        if (best != 0) {                                   // head to head against the built-in choice, longer runs
            float ms0 = 0.f, ms1 = 0.f;
            if (!time_launch(2, 0, ms0, 6) || !time_launch(2, best, ms1, 6)) return pl;
            if (!(ms1 < 0.97f * ms0)) { best = 0; best_ms = ms0; } else best_ms = ms1;
        }
        pl.v2 = best;
        ms2 = best_ms;
    }
    // ---- three iterations per pass (k_pt_sweepN): fewer bytes per iteration, more arithmetic per byte — pays where the
    // two-iteration pass is bandwidth-bound (FAST mode, power-of-two spacings), not where it is VALU-bound.  Taken only for
    // a clear per-ITERATION gain (≥ 2 %), head to head.
    const long long cells = (long long)p->nx * p->ny * nk;
    if (c->pt_depth <= 0 && cells >= NS3D_DEEP_MIN_CELLS && nk >= 12) {
        static const int cand[] = {1100, 2800, 2300, 100, 1600, 600, 2200, 1132, 3800};   // the first one is the built-in shape: it wins near-ties
        int bestn = c->ptn_variant;
        float best3 = 0.f, ms = 0.f;
        if (c->ptn_variant > 0) { if (!time_launch(3, bestn, best3)) best3 = 0.f; }
        else
            for (int v : cand) {
                if (!time_launch(3, v, ms)) continue;      // a shape that cannot run here (LDS / tile size)
                if (best3 == 0.f || ms < 0.98f * best3) { best3 = ms; bestn = v; }
            }
        if (best3 > 0.f && best3 / 3.f < 0.99f * ms2 / 2.f) {
            float a2 = 0.f, a3 = 0.f;
            if (time_launch(2, pl.v2, a2, 6) && time_launch(3, bestn, a3, 6) && a3 / 3.f < 0.98f * a2 / 2.f) {
                pl.depth = 3;
                pl.vn = bestn;
            }
        }
        // four iterations per pass: needs three or four waves per SIMD to pay — in fp64 768-thread workgroups of 64×24 columns
        // (two rows per thread: 154 registers), in fp32 1024-thread workgroups of 64×32 columns (two rows per thread, ≤ 128
        // registers) or 768 threads on 64×48; 2391 / 2891 = ONE round of workgroups, each marching the whole z range
        if (nk >= 16) {
            // 3800 (round 4): k_pt_sweepD, the planes of P⁰ through an LDS-DMA ring — what lets fp64 fit a 1024-thread 64×32 tile;
            // ties 2800 at 512³ (180 tiles for 256 CUs), so it has to win its place by 2 % like every later candidate
            // 12900 / 22900 / 42900: 2900 — 2800 with its XCD groups' tiles re-aligned every 32 / 64 / 128 z-steps (k_pt_sweepN's PACE);
            // where the launch cannot be paced they are 2800 again and lose the 2 %
            static const int cand4_f32[] = {2400, 2200, 1100, 0, 0, 0, 0, 0}, cand4_f64[] = {2800, 2891, 2300, 2391, 3800, 12900, 22900, 42900};
            const int *cand4 = sizeof(T) == 4 ? cand4_f32 : cand4_f64;
            const float cur_per_it = pl.depth == 3 ? best3 / 3.f : ms2 / 2.f;
            int best4v = 0;
            float best4 = 0.f;
            for (int q4 = 0; q4 < 8; ++q4) {
                const int v = cand4[q4];
                if (v == 0) continue;
                if (c->ptn_variant > 0 && v != c->ptn_variant) continue;
                if (v >= 10000 && c->pace.pace_z >= 0) continue;      // the context's own pace_z (or none) overrides the plan's
                if (!time_launch(4, v, ms)) continue;
                if (best4 == 0.f || ms < 0.98f * best4) { best4 = ms; best4v = v; }
            }
            if (best4 > 0.f && best4 / 4.f < 0.98f * cur_per_it) {
                float a = 0.f, b4 = 0.f;
                const bool ok = (pl.depth == 3 ? time_launch(3, pl.vn, a, 6) : time_launch(2, pl.v2, a, 6)) && time_launch(4, best4v, b4, 6);
                if (ok && b4 / 4.f < 0.97f * a / (float)pl.depth) {
                    pl.depth = 4;
                    pl.vn = best4v;
                }
            }
            // a fifth level: fp32 only, on the 1024-thread shape (registers to spare there and nowhere else): +6 % at 512³, +9.5 % at
            // 1024³ per iteration
            if (sizeof(T) == 4 && pl.depth == 4 && nk >= 24 && (c->ptn_variant <= 0 || c->ptn_variant / 100 == 24)) {
                const int v5 = c->ptn_variant > 0 ? c->ptn_variant : 2400;
                float a4 = 0.f, b5 = 0.f;
                if (time_launch(5, v5, ms) && ms / 5.f < 0.99f * best4 / 4.f && time_launch(4, pl.vn, a4, 6) && time_launch(5, v5, b5, 6) &&
                    b5 / 5.f < 0.98f * a4 / 4.f) {
                    pl.depth = 5;
                    pl.vn = v5;
                }
            }
        }
    } else if (c->pt_depth >= 3 && c->ptn_variant <= 0 && cells >= NS3D_TWO_MIN_CELLS) {
        // (24xx: float32 only, 28xx / 23xx with 768 threads: both element types; a shape that cannot run the depth is skipped)
        static const int cand[] = {1100, 2400, 2491, 2300, 2391, 2800, 2891, 100, 1600, 600, 2200, 1132, 3800};
        float bestd = 0.f, ms = 0.f;
        for (int v : cand) {
            if (!time_launch(c->pt_depth, v, ms)) continue;
            if (bestd == 0.f || ms < bestd) { bestd = ms; pl.vn = v; }
        }
    }
    {
        std::lock_guard<std::mutex> lock(g_tuned_mutex);
        g_tuned.push_back({c->device, p->nx, p->ny, p->nz, nk, (int)sizeof(T), mode, c->pt_depth, c->reserved_cus, pl.v2, pl.depth, pl.vn});
    }
    return pl;
}
template <class T>
static Plan pick_plan(ns3d_ctx *c, hipStream_t s, int mode, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                      const ns3d_pt_params *p, int k0, int k1, bool may_tune)
{
    Plan pl = lookup_plan<T>(c, mode, p, k0, k1);
    if (!pl.known && may_tune) pl = tune_plan<T>(c, s, mode, src, dst, dsrc, ddst, divV, p, k0, k1);
    return pl;
}
// one pass of `depth` (2…4, fp32: 5) PT iterations
template <class T>
static hipError_t launch_pass(ns3d_ctx *c, hipStream_t s, int depth, const Plan &pl, const T *src, T *dst, const T *dsrc, T *ddst,
                              const T *divV, const ns3d_pt_params *p, int k0, int k1, const ns3d_tile_window *win = nullptr,
                              int more_flags = 0)
{
    const int mode = mode_of(c, p->dx, p->dy, p->dz);
    c->last_depth = depth;
    const int flags = more_flags | ns3d_pass_flags_cus(c->reserved_cus);   // bits 8…: compute units the launch must not count on (in eights)
    if (depth == 2) {
        c->last_pt2 = pl.v2;
        return DISPATCHM(mode, pt_sweep2<T>(s, pl.v2, src, dst, dsrc, ddst, divV, *p, k0, k1, flags, win));
    }
    c->last_ptn = pl.vn % 10000;                            // above: the planned pace_z of shape 29, in units of 32 z-steps
    return DISPATCHM(mode, pt_sweepn<T>(s, depth, pl.vn, src, dst, dsrc, ddst, divV, *p, k0, k1, flags, win, &c->pace));
}
// iterations of the next pass when `rem` remain until the next residual check / the end
static int next_depth(const Plan &pl, bool blocked, int rem)
{
    if (!blocked || rem < 2) return 1;
    if (rem >= pl.depth) return (rem == pl.depth + 1 && pl.depth >= 3) ? pl.depth - 1 : pl.depth;   // 4 = 2+2, not 3+1
    return rem;                                             // 2 … depth−1 left: one pass of exactly that many
}
template <class T>
static hipError_t launch_pt2(ns3d_ctx *c, hipStream_t s, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                             const ns3d_pt_params *p, int k0, int k1, bool may_tune)
{
    const Plan pl = pick_plan<T>(c, s, mode_of(c, p->dx, p->dy, p->dz), src, dst, dsrc, ddst, divV, p, k0, k1, may_tune);
    return launch_pass<T>(c, s, 2, pl, src, dst, dsrc, ddst, divV, p, k0, k1);
}

// ---- what the multi-GPU layer enqueues on its ranks' contexts (ns3d_internal.h) ----------------------------------
template <class T>
hipError_t ns3d_enqueue_pt2(ns3d_ctx *c, hipStream_t s, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                            const ns3d_pt_params *p, int k0, int k1)
{
    return launch_pt2<T>(c, s, src, dst, dsrc, ddst, divV, p, k0, k1, false);
}
template <class T>
hipError_t ns3d_enqueue_pass(ns3d_ctx *c, hipStream_t s, int depth, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                             const ns3d_pt_params *p, int k0, int k1, int v2, int vn, const ns3d_tile_window *win, int skip_faces)
{
    Plan pl = lookup_plan<T>(c, mode_of(c, p->dx, p->dy, p->dz), p, k0, k1);
    if (v2 >= 0 && c->pt2_variant <= 0) pl.v2 = v2;        // the caller's own plan; explicit context settings still win
    if (vn >= 0 && c->ptn_variant <= 0) pl.vn = vn;
    return launch_pass<T>(c, s, depth, pl, src, dst, dsrc, ddst, divV, p, k0, k1, win, skip_faces ? NS3D_PASS_SKIP_FACES : 0);
}
template <class T>
hipError_t ns3d_enqueue_faces_region(ns3d_ctx *c, hipStream_t s, T *Pout, const ns3d_pt_params *p, const int c0[3], const int c1[3],
                                     int want_core)
{
    return DISPATCHG(c, p->dx, p->dy, p->dz, pt_faces_region<T>(s, Pout, *p, c0, c1, want_core));
}
template <class T>
int ns3d_plan_pt_internal(ns3d_ctx *c, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV, const ns3d_pt_params *p,
                          int k0, int k1)
{
    const Plan pl = pick_plan<T>(c, c->stream, mode_of(c, p->dx, p->dy, p->dz), src, dst, dsrc, ddst, divV, p, k0, k1, true);
    c->last_pt2 = pl.v2; c->last_ptn = pl.vn % 10000; c->last_depth = pl.depth;
    return pl.depth;
}
template <class T>
hipError_t ns3d_enqueue_pt1(ns3d_ctx *c, hipStream_t s, const T *src, T *dst, T *d, const T *divV, const ns3d_pt_params *p,
                            int k0, int k1)
{
    return DISPATCHG(c, p->dx, p->dy, p->dz, pt_sweep<T>(s, c->pt_variant, src, dst, d, divV, *p, k0, k1));
}
template <class T>
hipError_t ns3d_enqueue_residual_key(ns3d_ctx *c, hipStream_t s, const T *Pr, const T *divV, const ns3d_pt_params *p,
                                     unsigned long long *key_dev)
{
    return DISPATCHG(c, p->dx, p->dy, p->dz, residual_max_key<T>(s, Pr, divV, *p, key_dev));
}
template <class T>
hipError_t ns3d_enqueue_strip_inner(ns3d_ctx *c, hipStream_t s, const T *A, T *out, int sx, int sy, int sz)
{
    return DISPATCH(c, strip_inner<T>(s, A, out, sx, sy, sz));
}
template <class T>
hipError_t ns3d_enqueue_face_copy(ns3d_ctx *c, hipStream_t s, T *A, T *buf, int sx, int sy, int sz, int dim, int idx, int unpack)
{
    return DISPATCH(c, face_copy<T>(s, A, buf, sx, sy, sz, dim, idx, unpack));
}
template <class T>
hipError_t ns3d_enqueue_subbox_copy(ns3d_ctx *c, hipStream_t s, const ns3d_subbox_batch<T> &batch)
{
    return DISPATCH(c, subbox_copy<T>(s, batch));
}
template <class T>
hipError_t ns3d_enqueue_advect(ns3d_ctx *c, hipStream_t s, T *Vx, const T *Vx_o, T *Vy, const T *Vy_o, T *Vz, const T *Vz_o, T *C,
                               const T *C_o, double dt, double dx, double dy, double dz, int nx, int ny, int nz, int flags, int koff,
                               int nzg)
{
    return DISPATCHG(c, dx, dy, dz, advect<T>(s, Vx, Vx_o, Vy, Vy_o, Vz, Vz_o, C, C_o, dt, dx, dy, dz, nx, ny, nz, flags, koff, nzg));
}
#define NS3D_INST_INTERNAL(T)                                                                                       \
    template hipError_t ns3d_enqueue_advect<T>(ns3d_ctx *, hipStream_t, T *, const T *, T *, const T *, T *, const T *, T *, \
                                               const T *, double, double, double, double, int, int, int, int, int, int); \
    template hipError_t ns3d_enqueue_pt2<T>(ns3d_ctx *, hipStream_t, const T *, T *, const T *, T *, const T *,      \
                                            const ns3d_pt_params *, int, int);                                      \
    template hipError_t ns3d_enqueue_pass<T>(ns3d_ctx *, hipStream_t, int, const T *, T *, const T *, T *, const T *, \
                                             const ns3d_pt_params *, int, int, int, int, const ns3d_tile_window *, int); \
    template hipError_t ns3d_enqueue_faces_region<T>(ns3d_ctx *, hipStream_t, T *, const ns3d_pt_params *, const int *, const int *, int); \
    template int ns3d_plan_pt_internal<T>(ns3d_ctx *, const T *, T *, const T *, T *, const T *,                     \
                                          const ns3d_pt_params *, int, int);                                        \
    template hipError_t ns3d_enqueue_pt1<T>(ns3d_ctx *, hipStream_t, const T *, T *, T *, const T *,                 \
                                            const ns3d_pt_params *, int, int);                                      \
    template hipError_t ns3d_enqueue_residual_key<T>(ns3d_ctx *, hipStream_t, const T *, const T *,                  \
                                                     const ns3d_pt_params *, unsigned long long *);                 \
    template hipError_t ns3d_enqueue_strip_inner<T>(ns3d_ctx *, hipStream_t, const T *, T *, int, int, int);         \
    template hipError_t ns3d_enqueue_face_copy<T>(ns3d_ctx *, hipStream_t, T *, T *, int, int, int, int, int, int);  \
    template hipError_t ns3d_enqueue_subbox_copy<T>(ns3d_ctx *, hipStream_t, const ns3d_subbox_batch<T> &);
NS3D_INST_INTERNAL(double)
NS3D_INST_INTERNAL(float)
#undef NS3D_INST_INTERNAL

// The PT loop's buffers: Pr and dPrdτ as the next sweep reads them (src, dsrc) and where it writes them (dst, ddst).  ddst may be
// null: the one-iteration sweep updates dPrdτ in place.
template <class T>
struct PtBufs {
    T *src, *dst, *dsrc, *ddst;
    void swap_p() { std::swap(src, dst); }
    void swap_d() { std::swap(dsrc, ddst); }
};
template <class T>
static bool use_persist(const ns3d_ctx *c, const ns3d_pt_params *p);
template <class T>
static hipError_t enqueue_iters(ns3d_ctx *c, hipStream_t s, int n, bool two, PtBufs<T> &b, const T *divV, const ns3d_pt_params *p,
                                bool may_tune);
// the same as a status: what both loops below do with a block, the first time and when they redo one
template <class T>
static int enqueue_block(ns3d_ctx *c, hipStream_t s, int n, bool two, PtBufs<T> &b, const T *divV, const ns3d_pt_params *p)
{
    const hipError_t e = enqueue_iters<T>(c, s, n, two, b, divV, p, true);
    return e == hipSuccess ? NS3D_OK : fail(NS3D_ERR_HIP, "pt_sweep launch: %s", hipGetErrorString(e));
}

// n_iters fused sweeps, result left in Pr (one D2D copy when n_iters is odd).  With z halos the scratch
// buffer's halo planes are seeded from Pr first (a sweep never writes them).
template <class T>
static int pt_iterate_impl(ns3d_ctx *c, T *Pr, T *D, const T *divV, const ns3d_pt_params *p, int n_iters)
{
    if (n_iters <= 0) return NS3D_OK;
    T *other = nullptr;
    int rc = ensure_pingpong<T>(c, p, &other);
    if (rc) return rc;
    const size_t plane = (size_t)p->nx * p->ny;
    if (p->z_lo_is_halo) HIPCHK(c, hipMemcpyAsync(other, Pr, plane * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    if (p->z_hi_is_halo)
        HIPCHK(c, hipMemcpyAsync(other + plane * (p->nz - 1), Pr + plane * (p->nz - 1), plane * sizeof(T),
                                 hipMemcpyDeviceToDevice, c->stream));
    PtBufs<T> b{Pr, other, D, nullptr};
    const bool two = use_two(c, p) && !p->z_lo_is_halo && !p->z_hi_is_halo && n_iters >= 2;
    if (two && (rc = ensure_pingpong_d<T>(c, p, &b.ddst))) return rc;
    const PtBufs<T> in = b;                 // the block's inputs
    const unsigned ticket0 = c->persist.ticket;
    if ((rc = enqueue_block<T>(c, c->stream, n_iters, two, b, divV, p))) return rc;
    if (c->persist.ticket != ticket0) {
        // the block ran as ONE cooperative launch: before its result replaces the caller's arrays, make sure no hand-over timed out
        // (a stream synchronisation: these are launch-bound grids, the wait is the block itself); if one did, the inputs are
        // untouched — redo the block by launches (the cooperative form is off for this context from here on)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (persist_failed(c)) {
            b = in;
            if ((rc = enqueue_block<T>(c, c->stream, n_iters, two, b, divV, p))) return rc;
        }
    }
    if (b.dsrc != D)
        HIPCHK(c, hipMemcpyAsync(D, b.dsrc, (size_t)(p->nx - 2) * (p->ny - 2) * (p->nz - 2) * sizeof(T),
                                 hipMemcpyDeviceToDevice, c->stream));
    if (b.src != Pr)
        HIPCHK(c, hipMemcpyAsync(Pr, b.src, plane * p->nz * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    return NS3D_OK;
}

// NS3D_BC_FUSED=0 (read per call: tests compare the two forms): set_bc_Vel! / set_bc_Pr! rule by rule, a launch each, as rounds 1-3
static bool bc_fused_enabled()
{
    const char *v = std::getenv("NS3D_BC_FUSED");
    return !(v && *v == '0');
}

// ---- the PT loop of multi.jl:458-471 ----------------------------------------------------------------------
// enqueue exactly n iterations on stream s (two per pass where allowed) and leave the result pointers in b.src / b.dsrc
template <class T>
static hipError_t enqueue_iters(ns3d_ctx *c, hipStream_t s, int n, bool two, PtBufs<T> &b, const T *divV, const ns3d_pt_params *p,
                                bool may_tune)
{
    hipError_t e = hipSuccess;
    // small grids: the whole block of n iterations in one cooperative launch (k_pt_persist), where it applies
    if (n >= 2 && use_persist<T>(c, p)) {
        // outputs in buffers of their own (dPrdτ too): a launch whose bounded waits expire — its workgroups were not all resident at
        // once: another context or process on the device — leaves the block's inputs intact, and whoever synchronises the stream
        // next (persist_failed below) redoes the block by launches
        T *dout = b.ddst;
        if (!dout && ensure_pingpong_d<T>(c, p, &dout) != NS3D_OK) return hipErrorOutOfMemory;
        e = DISPATCHG(c, p->dx, p->dy, p->dz, pt_persist<T>(s, b.src, b.dst, b.dsrc, dout, divV, *p, n, &c->persist, ns3d_pass_flags_cus(c->reserved_cus)));
        if (e == hipSuccess) {
            b.swap_p();
            if (b.ddst) b.swap_d();
            else { b.ddst = b.dsrc; b.dsrc = dout; } // the caller had no second dPrdτ buffer: it has one now (copied back at the end)
            return e;
        }
        if (e != hipErrorInvalidValue) return e;     // invalid value: the form does not apply here → the ordinary path
        (void)hipGetLastError();
        e = hipSuccess;
    }
    Plan pl{2, 0, 0, true};
    if (two && n >= 2)
        pl = pick_plan<T>(c, s, mode_of(c, p->dx, p->dy, p->dz), b.src, b.dst, b.dsrc, b.ddst, divV, p, 1, p->nz - 1, may_tune);
    for (int it = 0; it < n && e == hipSuccess;) {
        const int d = next_depth(pl, two, n - it);
        if (d >= 2) {
            e = launch_pass<T>(c, s, d, pl, b.src, b.dst, b.dsrc, b.ddst, divV, p, 1, p->nz - 1);
            b.swap_d();
        } else
            e = DISPATCHG(c, p->dx, p->dy, p->dz, pt_sweep<T>(s, c->pt_variant, b.src, b.dst, b.dsrc, divV, *p, 1, p->nz - 1));
        it += d;
        b.swap_p();
    }
    return e;
}

// Field by field: the struct has four bytes of padding after owns_outlet that a C caller's stack struct or Julia's
// Ref(PtParams(…)) leaves indeterminate — a memcmp would miss the cache on every call and re-capture a graph each time.
static bool same_pt_params(const ns3d_pt_params &a, const ns3d_pt_params &b)
{
    return a.rho == b.rho && a.dt == b.dt && a.dtau == b.dtau && a.damp == b.damp && a.dx == b.dx && a.dy == b.dy && a.dz == b.dz &&
           a.nx == b.nx && a.ny == b.ny && a.nz == b.nz && a.bc_kind == b.bc_kind && a.owns_outlet == b.owns_outlet &&
           a.outlet_val == b.outlet_val && a.g == b.g && a.z_lo_is_halo == b.z_lo_is_halo && a.z_hi_is_halo == b.z_hi_is_halo;
}
template <class T>
static bool same_bufs(const ns3d_ctx::BlockGraph::Bufs &a, const PtBufs<T> &b)
{
    return a.src == b.src && a.dst == b.dst && a.dsrc == b.dsrc && a.ddst == b.ddst;
}

// One residual-check block (nchk iterations) as a HIP graph: launch-bound grids (63×38×38: ≈2 µs of kernel per ≈5 µs
// launch) replay the whole block with one host call.  Graphs are cached per buffer state in the context.
template <class T>
static int run_block_graph(ns3d_ctx *c, hipStream_t s, int n, bool two, PtBufs<T> &b, const T *divV, const ns3d_pt_params *p)
{
    const int mode = mode_of(c, p->dx, p->dy, p->dz);
    for (auto &g : c->graphs)
        if (same_bufs(g.in, b) && g.rhs == divV && g.n == n && g.two == two && g.mode == mode && g.v1 == c->pt_variant &&
            g.v2 == c->pt2_variant && g.vn == c->ptn_variant && g.depth == c->pt_depth && g.esize == (int)sizeof(T) &&
            same_pt_params(g.p, *p)) {
            HIPCHK(c, hipGraphLaunch(g.exec, s));
            b = {(T *)g.out.src, (T *)g.out.dst, (T *)g.out.dsrc, (T *)g.out.ddst};
            return NS3D_OK;
        }
    if (c->graphs.size() >= 16) c->clear_graphs();
    ns3d_ctx::BlockGraph g;
    g.in = {b.src, b.dst, b.dsrc, b.ddst}; g.rhs = divV; g.n = n; g.two = two; g.mode = mode;
    g.v1 = c->pt_variant; g.v2 = c->pt2_variant; g.vn = c->ptn_variant; g.depth = c->pt_depth; g.esize = (int)sizeof(T); g.p = *p;
    hipGraph_t graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipError_t e = enqueue_iters<T>(c, s, n, two, b, divV, p, false);
    hipError_t e2 = hipStreamEndCapture(s, &graph);
    if (e != hipSuccess || e2 != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return fail(NS3D_ERR_HIP, "PT block graph capture: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(NS3D_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    g.out = {b.src, b.dst, b.dsrc, b.ddst};
    c->graphs.push_back(g);
    HIPCHK(c, hipGraphLaunch(g.exec, s));
    return NS3D_OK;
}

// k_pt_persist: the launch-bound regime only (a cell per thread, the grid resident for the whole block)
template <class T>
static bool use_persist(const ns3d_ctx *c, const ns3d_pt_params *p)
{
    if (c->persist_mode == 0 || p->z_lo_is_halo || p->z_hi_is_halo) return false;
    if (c->persist_mode < 0) {
        // an explicit request (graph replay, iterations per pass, a tile shape) wins over the automatic choice
        if (c->graph_mode > 0 || c->pt_depth > 0 || c->ptn_variant > 0 || c->pt2_variant != 0) return false;
        // where it was measured to win (profiles/r3_persist_ab.log): up to ≈170 000 cells, one workgroup across x
        if ((long long)p->nx * p->ny * p->nz > 170ll * 1000 || p->nx > 66) return false;
    }
    const hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz, pt_persist<T>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, *p, 2, nullptr,
                                                                      ns3d_pass_flags_cus(c->reserved_cus)));
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;                                         // the CUs this context launches on hold the whole grid at once
}
template <class T>
static bool use_graphs(const ns3d_ctx *c, const ns3d_pt_params *p, int nchk)
{
    if (use_persist<T>(c, p)) return false;                         // one launch per block already (and no capture of a cooperative launch)
    if (c->graph_mode == 0 || nchk < 4) return false;
    if (c->graph_mode > 0) return true;
    return (long long)p->nx * p->ny * p->nz < 3ll * 1000 * 1000;    // launch-bound regime
}

template <class T>
static int pt_solve_impl(ns3d_ctx *c, T *Pr, T *D, const T *divV, const ns3d_pt_params *p, double eps, int niter,
                         int nchk, double err_mul, double err_div, int *iters_done, double *err_hist, int max_checks,
                         int *n_checks)
{
    T *other = nullptr;
    int rc = ensure_pingpong<T>(c, p, &other);
    if (rc) return rc;
    const size_t plane = (size_t)p->nx * p->ny;
    PtBufs<T> b{Pr, other, D, nullptr};
    int checks = 0, iter = 0, done = niter;
    bool converged = false;
    const bool two = use_two(c, p) && niter >= 2;
    if (two && (rc = ensure_pingpong_d<T>(c, p, &b.ddst))) return rc;
    // graphs cannot be captured on HIP's null stream: run the loop on the context's own stream, fenced by events
    const bool graphs = use_graphs<T>(c, p, nchk);
    hipStream_t s = c->stream;
    const bool fenced = graphs && (s == nullptr);
    if (fenced) {
        s = c->own_stream;
        HIPCHK(c, hipEventRecord(c->fence, c->stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->fence, 0));
    }
    // settle the tile choice of the two-iteration sweep now (eagerly, into the scratch buffers): inside a stream capture
    // it could only be looked up
    if (two) (void)pick_plan<T>(c, s, mode_of(c, p->dx, p->dy, p->dz), b.src, b.dst, b.dsrc, b.ddst, divV, p, 1, p->nz - 1, true);
    // Small grids (round 4): the WHOLE loop — iterations, residual checks, the decision of :467-469 — as one launch of k_pt_persist.  The
    // checks' maxima come back through pinned host memory behind one synchronisation; a launch whose bounded waits expired left its
    // inputs intact and the loop below redoes the solve by launches.  NS3D_PERSIST_SOLVE=0: a launch per residual-check block (A/B).
    const char *wv = std::getenv("NS3D_PERSIST_SOLVE");         // read per solve: tests flip it
    const bool whole = !(wv && *wv == '0');
    if (whole && nchk > 0 && niter >= nchk && niter / nchk <= NS3D_PERSIST_MAXCHK && use_persist<T>(c, p)) {
        T *dout = b.ddst;
        if (!dout && (rc = ensure_pingpong_d<T>(c, p, &dout))) return rc;
        hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz,
                                 pt_persist<T>(s, b.src, b.dst, b.dsrc, dout, divV, *p, niter, &c->persist, ns3d_pass_flags_cus(c->reserved_cus), nchk, eps,
                                               err_mul, err_div));
        if (e == hipSuccess) {
            HIPCHK(c, hipStreamSynchronize(s));
            if (!persist_failed(c)) {
                const unsigned long long *res = c->persist.res_host;
                done = (int)res[0];
                checks = (int)res[1];
                for (int q = 0; q < checks && q < max_checks && err_hist; ++q) {
                    double mx;
                    std::memcpy(&mx, &res[2 + q], sizeof mx);
                    err_hist[q] = mx * err_mul / err_div;
                }
                b.src = b.dst; b.dsrc = dout;
                iter = niter;                   // nothing left for the loop below
            }
        } else if (e != hipErrorInvalidValue)
            return fail(NS3D_ERR_HIP, "pt_persist launch: %s", hipGetErrorString(e));
        else
            (void)hipGetLastError();
    }
    while (iter < niter) {
        // iterations until the next residual check (multi.jl:464) or the end of the budget
        const int n = nchk > 0 ? std::min(nchk - iter % nchk, niter - iter) : niter - iter;
        const PtBufs<T> in = b;                 // the block's inputs
        const unsigned ticket0 = c->persist.ticket;
        if ((rc = graphs && n == nchk ? run_block_graph<T>(c, s, n, two, b, divV, p) : enqueue_block<T>(c, s, n, two, b, divV, p))) return rc;
        iter += n;
        const bool check_now = nchk > 0 && iter % nchk == 0;
        if (c->persist.ticket != ticket0 && !check_now) HIPCHK(c, hipStreamSynchronize(s));     // a last, partial block: no read-back follows
        for (int attempt = 0; attempt < 2; ++attempt) {
            double mx = 0.0;
            if (check_now) { // multi.jl:464-469
                hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz, residual_max_key<T>(s, b.src, divV, *p, c->key_dev));
                if (e != hipSuccess) return fail(NS3D_ERR_HIP, "residual launch: %s", hipGetErrorString(e));
                if ((rc = fetch_key(c, s, &mx))) return rc;
            }
            // the read-back synchronised the stream: if the block ran as one cooperative launch and a hand-over in it timed out, its
            // inputs are still there — redo it by launches (once; the cooperative form is off for this context afterwards)
            if (attempt == 0 && c->persist.ticket != ticket0 && persist_failed(c)) {
                b = in;
                if ((rc = enqueue_block<T>(c, s, n, two, b, divV, p))) return rc;
                continue;
            }
            if (!check_now) break;
            const double err = mx * err_mul / err_div; // maximum(abs.(Rp))*ly^2/psc, multi.jl:466
            if (err_hist && checks < max_checks) err_hist[checks] = err;
            ++checks;
            if (eps >= 0 && (err < eps || !std::isfinite(err))) { done = iter; converged = true; }
            break;
        }
        if (converged) break;
    }
    if (b.src != Pr)
        HIPCHK(c, hipMemcpyAsync(Pr, b.src, plane * p->nz * sizeof(T), hipMemcpyDeviceToDevice, s));
    if (b.dsrc != D)
        HIPCHK(c, hipMemcpyAsync(D, b.dsrc, (size_t)(p->nx - 2) * (p->ny - 2) * (p->nz - 2) * sizeof(T),
                                 hipMemcpyDeviceToDevice, s));
    if (fenced) {
        HIPCHK(c, hipEventRecord(c->fence, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->fence, 0));
    }
    if (iters_done) *iters_done = done;
    if (n_checks) *n_checks = checks;
    return NS3D_OK;
}

// ---- the typed entry points: ns3d_api_typed.h, plain code, compiled once per element type ----------------------------------------
// plane range of a sweep entry point: interior planes only
static int check_planes(const ns3d_pt_params *p, int k0, int k1, const char *fn)
{
    if (k0 < 1 || k1 > p->nz - 1 || k0 > k1) return fail(NS3D_ERR_ARG, "%s: plane range [%d,%d) outside [1,%d)", fn, k0, k1, p->nz - 1);
    return NS3D_OK;
}
static int check_no_halos(const ns3d_pt_params *p, const char *fn)
{
    if (p->z_lo_is_halo || p->z_hi_is_halo) return fail(NS3D_ERR_ARG, "%s: z-slab ranks pass ghost-extended buffers, not halo flags", fn);
    return NS3D_OK;
}
// ns3d_isosurface: the argument checks that do not depend on the element type, the geometry of the launch and the context's scratch
// (8 B for the total, 8 B per scan workgroup, 12 B per row segment of 64 cubes: counts and their scan), grown lazily
static int iso_prepare(ns3d_ctx *c, int ex, int ey, int ez, const int *box, const int *origin, double iso, const void *tri, const void *val,
                       const void *B, long long cap, const char *fn, ns3d_iso_geom *g, ns3d_iso_scratch *w)
{
    if (ex < 2 || ey < 2 || ez < 2) return fail(NS3D_ERR_ARG, "%s: extents %dx%dx%d too small (need >= 2 per direction)", fn, ex, ey, ez);
    const int e[3] = {ex, ey, ez};
    int lo[3] = {0, 0, 0}, hi[3] = {ex - 1, ey - 1, ez - 1};
    if (box)
        for (int q = 0; q < 3; ++q) {
            lo[q] = box[q];
            hi[q] = box[3 + q];
            if (lo[q] < 0 || hi[q] <= lo[q] || hi[q] > e[q] - 1)
                return fail(NS3D_ERR_ARG, "%s: box [%d,%d] in direction %d (need 0 <= lo < hi <= %d)", fn, lo[q], hi[q], q, e[q] - 1);
        }
    if (cap < 0) return fail(NS3D_ERR_ARG, "%s: cap = %lld is negative", fn, cap);
    if (!tri && cap > 0) return fail(NS3D_ERR_ARG, "%s: tri is NULL with cap = %lld", fn, cap);
    if (val && !B) return fail(NS3D_ERR_ARG, "%s: val given without B", fn);
    if (!std::isfinite(iso)) return fail(NS3D_ERR_ARG, "%s: iso = %g is not finite", fn, iso);
    g->ex = ex; g->ey = ey;
    g->lox = lo[0]; g->loy = lo[1]; g->loz = lo[2];
    g->cx = hi[0] - lo[0]; g->cy = hi[1] - lo[1]; g->cz = hi[2] - lo[2];
    g->nseg = (g->cx + 63) / 64;
    g->gy = (g->cy + NS3D_ISO_ROWS - 1) / NS3D_ISO_ROWS;
    g->gz = (g->cz + NS3D_ISO_KZ - 1) / NS3D_ISO_KZ;
    g->ox = origin ? origin[0] : 0; g->oy = origin ? origin[1] : 0; g->oz = origin ? origin[2] : 0;
    if ((unsigned long long)g->nseg * g->gy * g->gz > 0x7fffffffull)
        return fail(NS3D_ERR_ARG, "%s: a box of %dx%dx%d cubes exceeds one launch", fn, g->cx, g->cy, g->cz);
    w->nsegs = (unsigned long long)g->nseg * g->cy * g->cz;
    w->nblk = (unsigned)((w->nsegs + NS3D_ISO_SCAN_BLOCK - 1) / NS3D_ISO_SCAN_BLOCK);
    const size_t need = 8 * (size_t)(1 + w->nblk + w->nsegs) + 4 * (size_t)w->nsegs;
    if (const int rc = c->iso_dev.reserve(need, ns3d_drain_stream(c))) return rc;
    w->total = c->iso_dev.as<unsigned long long>();
    w->bsum = w->total + 1;
    w->segbase = w->bsum + w->nblk;
    w->segcnt = (unsigned *)(w->segbase + w->nsegs);
    return NS3D_OK;
}
// ---- ns3d_voxelize / ns3d_set_solid / ns3d_solid_momentum (ns3d_solid.hip) ----------------------------------------------------------
// voxelize and solid_momentum share c->solid_dev: grown lazily, after a wait for the stream (the header's table)
extern "C" int ns3d_voxelize(ns3d_ctx *c, unsigned char *mask, const double *tri, long long n_tri, int nx, int ny, int nz, const int *origin)
{
    CHECK_CTX(c);
    if (!mask) return fail(NS3D_ERR_ARG, "%s: null mask", __func__);
    if (n_tri < 0) return fail(NS3D_ERR_ARG, "%s: n_tri = %lld is negative", __func__, n_tri);
    if (!tri && n_tri > 0) return fail(NS3D_ERR_ARG, "%s: tri is NULL with n_tri = %lld", __func__, n_tri);
    if (n_tri > 4ll * 0x7fffffffll) return fail(NS3D_ERR_ARG, "%s: n_tri = %lld exceeds one launch (4 x 2^31 triangles)", __func__, n_tri);
    CHECK_GRID(nx, ny, nz, 3);
    const int zero[3] = {0, 0, 0};
    const int *o = origin ? origin : zero;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0) return fail(NS3D_ERR_ARG, "%s: origin %d, %d, %d (each >= 0)", __func__, o[0], o[1], o[2]);
    const int rc = c->solid_dev.reserve(ns3d_solid::voxelize_scratch_bytes(nx, ny, nz), ns3d_drain_stream(c));
    if (rc) return rc;
    return finish(c, ns3d_solid::voxelize(c->stream, mask, tri, n_tri, nx, ny, nz, o, c->solid_dev.ptr), "voxelize");
}
// the checks ns3d_set_solid_moving and ns3d_solid_momentum_moving share, and the kernels' form of what they take
static int make_motion(const char *fn, const double *motion, double dx, double dy, double dz, const int *origin, ns3d_solid::Motion *mo)
{
    if (!motion) return fail(NS3D_ERR_ARG, "%s: null motion", fn);
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(motion[q])) return fail(NS3D_ERR_ARG, "%s: motion[%d] = %g is not finite", fn, q, motion[q]);
    if (!(std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dz) && dx > 0.0 && dy > 0.0 && dz > 0.0))
        return fail(NS3D_ERR_ARG, "%s: spacings %g, %g, %g (each finite and > 0)", fn, dx, dy, dz);
    const int zero[3] = {0, 0, 0};
    const int *o = origin ? origin : zero;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0) return fail(NS3D_ERR_ARG, "%s: origin %d, %d, %d (each >= 0)", fn, o[0], o[1], o[2]);
    for (int q = 0; q < 3; ++q) { mo->U[q] = motion[q]; mo->w[q] = motion[3 + q]; mo->c[q] = motion[6 + q]; mo->o[q] = o[q]; }
    mo->d[0] = dx; mo->d[1] = dy; mo->d[2] = dz;
    return NS3D_OK;
}
extern "C" int ns3d_mesh_transform(ns3d_ctx *c, double *out, const double *tri, long long n_tri, const double *R, const double *pivot,
                                   const double *shift, const double *spacing)
{
    CHECK_CTX(c);
    if (n_tri < 0) return fail(NS3D_ERR_ARG, "%s: n_tri = %lld is negative", __func__, n_tri);
    if (n_tri > 4ll * 0x7fffffffll) return fail(NS3D_ERR_ARG, "%s: n_tri = %lld exceeds one launch (4 x 2^31 triangles)", __func__, n_tri);
    if (!R || !pivot || !shift || !spacing) return fail(NS3D_ERR_ARG, "%s: null R, pivot, shift or spacing", __func__);
    for (int q = 0; q < 9; ++q)
        if (!std::isfinite(R[q])) return fail(NS3D_ERR_ARG, "%s: R[%d] = %g is not finite", __func__, q, R[q]);
    for (int q = 0; q < 3; ++q) {
        if (!(std::isfinite(pivot[q]) && std::isfinite(shift[q])))
            return fail(NS3D_ERR_ARG, "%s: pivot[%d] = %g, shift[%d] = %g (need finite values)", __func__, q, pivot[q], q, shift[q]);
        if (!(std::isfinite(spacing[q]) && spacing[q] > 0.0))
            return fail(NS3D_ERR_ARG, "%s: spacing[%d] = %g (finite and > 0)", __func__, q, spacing[q]);
    }
    if (n_tri == 0) return NS3D_OK;
    if (!out || !tri) return fail(NS3D_ERR_ARG, "%s: null %s with n_tri = %lld", __func__, out ? "tri" : "out", n_tri);
    if (out != tri) {
        const uintptr_t a = (uintptr_t)out, b = (uintptr_t)tri, len = (uintptr_t)n_tri * 9 * sizeof(double);
        if (a < b + len && b < a + len)
            return fail(NS3D_ERR_ARG, "%s: out and tri overlap (in place, out == tri, or apart)", __func__);
    }
    return finish(c, ns3d_solid::mesh_transform(c->stream, out, tri, n_tri, R, pivot, shift, spacing), "mesh_transform");
}
extern "C" int ns3d_poisson_direct_f64(ns3d_ctx *, double *, double *, const double *, const ns3d_pt_params *);      // ns3d_direct.hip
extern "C" int ns3d_poisson_direct_f32(ns3d_ctx *, float *, float *, const float *, const ns3d_pt_params *);
namespace ns3d_api_f64 { using T = double;
#define NS3D_FN(name) ns3d_##name##_f64
#define NS3D_BC_RULE bc_f64       // the name its messages carry (__func__)
#include "ns3d_api_typed.h"
#undef NS3D_BC_RULE
#undef NS3D_FN
}
namespace ns3d_api_f32 { using T = float;
#define NS3D_FN(name) ns3d_##name##_f32
#define NS3D_BC_RULE bc_f32
#include "ns3d_api_typed.h"
#undef NS3D_BC_RULE
#undef NS3D_FN
}
