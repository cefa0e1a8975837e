// ns3d_tracers.hip — ns3d_sample and ns3d_tracers_advance (include/ns3d.h has the definition): a field interpolated at points the
// caller chooses, and one explicit-midpoint step of Lagrangian particles through the frozen staggered velocity field; their origin
// forms for the ranks of a decomposed grid (ns3d_sample_at, ns3d_tracers_advance_at) and the routing kernels of
// ns3d_tracers_migrate_mgpu at the end of the file.
//
// Compiled ONCE, with -ffp-contract=off (build.py), and not as part of the four-times-compiled kernel unit: the contract is that
// STRICT, NS3D_IEEE_DIV and FAST contexts return the same bits, so there is nothing for an arithmetic mode to select — and the
// FAST compilation's -ffp-contract=fast lets the backend fuse whatever a `#pragma clang fp contract(off)` says (only
// fast-honor-pragmas listens to it).  The pragma below is kept for a build whose flags are changed.
//
// Shape: one thread per particle, 256-thread workgroups, SoA positions (ξ | η | ζ blocks of n doubles: a wave's three position
// loads are 512 contiguous bytes each).  Per stage a thread issues 24 independent gathers (8 corners × 3 components) before any
// arithmetic of the stage, so that they are in flight together; the gathers are element-granular and uncoalesced by nature —
// locality comes from the order of the particles in memory (Tracers.sort_by_cell) and from L2 / the Infinity Cache.  No LDS, no
// atomics, no division.  Measured against three threads per particle and 64-thread workgroups: tools/ab/tracers_ab.hip,
// profiles/tracers_variants_ab.log, DESIGN §4.11.
#include <cmath>

#include "ns3d_internal.h"

#pragma clang fp contract(off)

namespace ns3d_tracers {

typedef long long idx_t;

// one direction of I(A, ext, stag, p): the lower node i0 and the weight t of the upper one.  max / min are written as comparisons
// so that −0.0 becomes +0.0 and the result never depends on a library's choice between two zeros; c is finite from the clamp on
// (a caller passes no NaN), so the conversion to int is defined.
struct Axis {
    int i0;
    double t;
};
__device__ __forceinline__ Axis axis_of(double p, int stag, int ext)
{
    double c = p - (stag ? 0.0 : 0.5);
    c = c > 0.0 ? c : 0.0;
    const double hi = (double)(ext - 1);
    c = c < hi ? c : hi;
    Axis a;
    a.i0 = min((int)floor(c), ext - 2);
    a.t = c - (double)a.i0;
    return a;
}
__device__ __forceinline__ double lerp(double a, double b, double t) { return b * t + a * (1.0 - t); }

// The interpolation routine of both kernels, in two halves so that a caller can issue the loads of several fields before the
// arithmetic of the first: issue() forms the indices and loads the 8 corners (converted to double), value() is backtrack!'s
// four x-lerps, two y-lerps and the z-lerp (multi.jl:200-214).
struct Interp {
    double v[8];        // [i + 2j + 4k] of the corner (i0+i, j0+j, k0+k)
    double tx, ty, tz;
    template <class T>
    __device__ __forceinline__ void issue(const T *__restrict__ A, int ex, int ey, int ez, int sx, int sy, int sz, double px, double py,
                                          double pz)
    {
        const Axis x = axis_of(px, sx, ex), y = axis_of(py, sy, ey), z = axis_of(pz, sz, ez);
        const idx_t row = ex, plane = (idx_t)ex * ey;
        const T *q = A + ((idx_t)x.i0 + row * y.i0 + plane * z.i0);
        const T a0 = q[0], a1 = q[1], a2 = q[row], a3 = q[row + 1];
        const T a4 = q[plane], a5 = q[plane + 1], a6 = q[plane + row], a7 = q[plane + row + 1];
        v[0] = (double)a0; v[1] = (double)a1; v[2] = (double)a2; v[3] = (double)a3;
        v[4] = (double)a4; v[5] = (double)a5; v[6] = (double)a6; v[7] = (double)a7;
        tx = x.t; ty = y.t; tz = z.t;
    }
    __device__ __forceinline__ double value() const
    {
        const double fy1z1 = lerp(v[0], v[1], tx);
        const double fy1z2 = lerp(v[4], v[5], tx);
        const double fy2z1 = lerp(v[2], v[3], tx);
        const double fy2z2 = lerp(v[6], v[7], tx);
        const double fz1 = lerp(fy1z1, fy2z1, ty);
        const double fz2 = lerp(fy1z2, fy2z2, ty);
        return lerp(fz1, fz2, tz);
    }
};

// inside the closed interval [0, hi]; false for NaN and ±Inf
__device__ __forceinline__ bool inside(double p, int hi) { return p >= 0.0 && p <= (double)hi; }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

template <class T>
__device__ __forceinline__ void velocity(const T *__restrict__ Vx, const T *__restrict__ Vy, const T *__restrict__ Vz, int nx, int ny,
                                         int nz, double px, double py, double pz, double &u, double &v, double &w)
{
    Interp a, b, c;
    a.issue(Vx, nx + 1, ny, nz, 1, 0, 0, px, py, pz);
    b.issue(Vy, nx, ny + 1, nz, 0, 1, 0, px, py, pz);
    c.issue(Vz, nx, ny, nz + 1, 0, 0, 1, px, py, pz);
    u = a.value();
    v = b.value();
    w = c.value();
}

template <class T>
__global__ __launch_bounds__(256) void k_sample(double *__restrict__ out, const double *__restrict__ X,
                                                const unsigned char *__restrict__ state, idx_t n, const T *__restrict__ A, int ex,
                                                int ey, int ez, int sx, int sy, int sz)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = X[p], y = X[n + p], z = X[2 * n + p];
    const bool alive = (state == nullptr || state[p] == 1) && inside(x, ex - sx) && inside(y, ey - sy) && inside(z, ez - sz);
    double r = quiet_nan();
    if (alive) {
        Interp a;
        a.issue(A, ex, ey, ez, sx, sy, sz, x, y, z);
        r = a.value();
    }
    out[p] = r;
}

template <class T>
__global__ __launch_bounds__(256) void k_tracers(double *X, unsigned char *state, double *U, idx_t n, const T *__restrict__ Vx,
                                                 const T *__restrict__ Vy, const T *__restrict__ Vz, double cx, double cy, double cz,
                                                 int nx, int ny, int nz)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = X[p], y = X[n + p], z = X[2 * n + p];
    if (!(state[p] == 1 && inside(x, nx) && inside(y, ny) && inside(z, nz))) {     // inactive: the coordinates stay
        state[p] = 0;
        if (U) { U[p] = quiet_nan(); U[n + p] = quiet_nan(); U[2 * n + p] = quiet_nan(); }
        return;
    }
    double u, v, w;
    velocity<T>(Vx, Vy, Vz, nx, ny, nz, x, y, z, u, v, w);
    if (U) { U[p] = u; U[n + p] = v; U[2 * n + p] = w; }
    double xn = x + 0.5 * (u * cx), yn = y + 0.5 * (v * cy), zn = z + 0.5 * (w * cz);
    if (isfinite(xn) && isfinite(yn) && isfinite(zn)) {    // the midpoint may lie outside the box: the clamp of axis_of covers that
        velocity<T>(Vx, Vy, Vz, nx, ny, nz, xn, yn, zn, u, v, w);
        xn = x + u * cx;
        yn = y + v * cy;
        zn = z + w * cz;
    }
    X[p] = xn; X[n + p] = yn; X[2 * n + p] = zn;
    state[p] = inside(xn, nx) && inside(yn, ny) && inside(zn, nz) ? 1 : 0;
}

// The origin forms of a decomposed grid: k_sample / k_tracers with positions in the GLOBAL index space.  The rank interpolates at
// X − origin (exact for 0 ≤ origin ≤ X: the local node is the global one minus origin, the weights have the same bits), and the
// advance takes its "inside" tests on the global box.  Kernels of their own: sharing one body with the one-rank kernels changed
// THEIR register allocation (DESIGN §4.11.1 has the reports).
struct Box3 { int o[3], g[3]; };     // a rank's origin and the global cell grid
template <class T>
__global__ __launch_bounds__(256) void k_sample_at(double *__restrict__ out, const double *__restrict__ X,
                                                   const unsigned char *__restrict__ state, idx_t n, const T *__restrict__ A, int ex,
                                                   int ey, int ez, int sx, int sy, int sz, int ox, int oy, int oz)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = X[p] - (double)ox, y = X[n + p] - (double)oy, z = X[2 * n + p] - (double)oz;
    const bool alive = (state == nullptr || state[p] == 1) && inside(x, ex - sx) && inside(y, ey - sy) && inside(z, ez - sz);
    double r = quiet_nan();
    if (alive) {
        Interp a;
        a.issue(A, ex, ey, ez, sx, sy, sz, x, y, z);
        r = a.value();
    }
    out[p] = r;
}

template <class T>
__global__ __launch_bounds__(256) void k_tracers_at(double *X, unsigned char *state, double *U, idx_t n, const T *__restrict__ Vx,
                                                    const T *__restrict__ Vy, const T *__restrict__ Vz, double cx, double cy, double cz,
                                                    int nx, int ny, int nz, Box3 b)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = X[p], y = X[n + p], z = X[2 * n + p];
    if (!(state[p] == 1 && inside(x, b.g[0]) && inside(y, b.g[1]) && inside(z, b.g[2]))) {     // inactive: the coordinates stay
        state[p] = 0;
        if (U) { U[p] = quiet_nan(); U[n + p] = quiet_nan(); U[2 * n + p] = quiet_nan(); }
        return;
    }
    const double ox = (double)b.o[0], oy = (double)b.o[1], oz = (double)b.o[2];
    double u, v, w;
    velocity<T>(Vx, Vy, Vz, nx, ny, nz, x - ox, y - oy, z - oz, u, v, w);
    if (U) { U[p] = u; U[n + p] = v; U[2 * n + p] = w; }
    double xn = x + 0.5 * (u * cx), yn = y + 0.5 * (v * cy), zn = z + 0.5 * (w * cz);
    if (isfinite(xn) && isfinite(yn) && isfinite(zn)) {    // a midpoint beyond the rank's margin is clamped to the LOCAL array
        velocity<T>(Vx, Vy, Vz, nx, ny, nz, xn - ox, yn - oy, zn - oz, u, v, w);
        xn = x + u * cx;
        yn = y + v * cy;
        zn = z + w * cz;
    }
    X[p] = xn; X[n + p] = yn; X[2 * n + p] = zn;
    state[p] = inside(xn, b.g[0]) && inside(yn, b.g[1]) && inside(zn, b.g[2]) ? 1 : 0;
}

template <class T>
hipError_t sample(hipStream_t s, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey, int ez,
                  int sx, int sy, int sz)
{
    hipLaunchKernelGGL(k_sample<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, X, state, (idx_t)n, A, ex, ey, ez, sx, sy, sz);
    return hipGetLastError();
}
template <class T>
hipError_t advance(hipStream_t s, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy, const T *Vz, double cx,
                   double cy, double cz, int nx, int ny, int nz)
{
    hipLaunchKernelGGL(k_tracers<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, state, U, (idx_t)n, Vx, Vy, Vz, cx, cy, cz, nx,
                       ny, nz);
    return hipGetLastError();
}
template <class T>
hipError_t sample_at(hipStream_t s, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey, int ez,
                     int sx, int sy, int sz, const int *origin)
{
    hipLaunchKernelGGL(k_sample_at<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, X, state, (idx_t)n, A, ex, ey, ez, sx, sy,
                       sz, origin[0], origin[1], origin[2]);
    return hipGetLastError();
}
template <class T>
hipError_t advance_at(hipStream_t s, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy, const T *Vz, double cx,
                      double cy, double cz, int nx, int ny, int nz, const int *origin, const int *n_g)
{
    Box3 b;
    for (int q = 0; q < 3; ++q) { b.o[q] = origin[q]; b.g[q] = n_g[q]; }
    hipLaunchKernelGGL(k_tracers_at<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, state, U, (idx_t)n, Vx, Vy, Vz, cx, cy, cz,
                       nx, ny, nz, b);
    return hipGetLastError();
}

#define INST(T)                                                                                                                   \
    template hipError_t sample<T>(hipStream_t, double *, const double *, const unsigned char *, long, const T *, int, int, int, int, \
                                  int, int);                                                                                      \
    template hipError_t advance<T>(hipStream_t, double *, unsigned char *, double *, long, const T *, const T *, const T *, double, \
                                   double, double, int, int, int);                                                                \
    template hipError_t sample_at<T>(hipStream_t, double *, const double *, const unsigned char *, long, const T *, int, int, int,  \
                                     int, int, int, const int *);                                                                 \
    template hipError_t advance_at<T>(hipStream_t, double *, unsigned char *, double *, long, const T *, const T *, const T *,      \
                                      double, double, double, int, int, int, const int *, const int *);
INST(double)
INST(float)
#undef INST

// ---- ns3d_tracers_migrate_mgpu: routing particles to the ranks that own them (include/ns3d.h has the rule; ns3d_mgpu.cpp the host
// side).  Count / scan / compact like k_iso_count / k_iso_emit: no atomic decides a position.  One thread per slot, 256-thread
// workgroups; `counts` and `offs` hold P+1 rows of one entry per workgroup — row d < P: this rank's leavers bound for rank d, row P:
// the slots that are empty once the leavers have gone.
__device__ __forceinline__ int owner_coord(double x, int D, int m, double inv)      // m = n − 2 owned cells per rank, inv ≈ 1/m
{
    double e = (x - 1.0) * inv;                 // an estimate only: the comparisons below decide
    e = e > 0.0 ? e : 0.0;
    const double hi = (double)(D - 1);
    e = e < hi ? e : hi;
    int k = (int)e;
    while (k > 0 && x < (double)(k * m + 1)) --k;
    while (k < D - 1 && x >= (double)((k + 1) * m + 1)) ++k;
    return k;
}

// dest[p]: the rank slot p leaves for, −1 if it stays; code[p]: −1 for a slot that stays occupied, else (rank among the workgroup's
// empty slots) + 256·(rank among the workgroup's leavers for the same destination)
__global__ __launch_bounds__(256) void k_mig_classify(int *__restrict__ dest, int *__restrict__ code, unsigned *__restrict__ counts,
                                                      const double *__restrict__ X, const unsigned char *__restrict__ state,
                                                      const long long *__restrict__ id, idx_t cap, ns3d_mig_geom g)
{
    __shared__ int sd[256];
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x;
    const idx_t p = (idx_t)blockIdx.x * 256 + t;
    const idx_t nwg = gridDim.x;
    int d = -1;
    bool empty = false;
    if (p < cap) {
        if (id[p] < 0) empty = true;
        else if (state[p] == 1) {
            const double x = X[p], y = X[cap + p], z = X[2 * cap + p];
            if (isfinite(x) && isfinite(y) && isfinite(z)) {
                const int kx = owner_coord(x, g.dims[0], g.n[0] - 2, g.inv[0]), ky = owner_coord(y, g.dims[1], g.n[1] - 2, g.inv[1]),
                          kz = owner_coord(z, g.dims[2], g.n[2] - 2, g.inv[2]);
                const int owner = (kx * g.dims[1] + ky) * g.dims[2] + kz;
                if (owner != g.me) { d = owner; empty = true; }
            }
        }
    }
    sd[t] = d;
    const unsigned long long b = __ballot(empty);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) wsum[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned er = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) er += wsum[w];
    if (t == 0) counts[(idx_t)g.P * nwg + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    int lr = 0;
    if (d >= 0) {
        bool last = true;
        for (int q = 0; q < t; ++q) lr += sd[q] == d ? 1 : 0;
        for (int q = t + 1; q < 256; ++q) last = last && sd[q] != d;
        if (last) counts[(idx_t)d * nwg + blockIdx.x] = (unsigned)(lr + 1);
    }
    if (p < cap) {
        dest[p] = d;
        code[p] = empty ? (int)er + 256 * lr : -1;
    }
}

// one workgroup per row: offs = the exclusive prefix sums of the row's counts, totals[row] their sum
__global__ __launch_bounds__(256) void k_mig_scan(const unsigned *__restrict__ counts, unsigned long long *__restrict__ offs,
                                                  unsigned long long *__restrict__ totals, idx_t nwg)
{
    __shared__ unsigned long long buf[256];
    const int t = threadIdx.x;
    const idx_t row = blockIdx.x;
    unsigned long long carry = 0ull;
    for (idx_t base = 0; base < nwg; base += 256) {
        const idx_t i = base + t;
        const unsigned long long v = i < nwg ? (unsigned long long)counts[row * nwg + i] : 0ull;
        buf[t] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const unsigned long long u = t >= s ? buf[t - s] : 0ull;
            __syncthreads();
            buf[t] += u;
            __syncthreads();
        }
        if (i < nwg) offs[row * nwg + i] = carry + buf[t] - v;
        carry += buf[255];
        __syncthreads();
    }
    if (t == 0) totals[row] = carry;
}

// a leaver becomes a record of NS3D_MIG_REC doubles (x, y, z, the id's bits, u, v, w, unused) in the send buffer — the records for
// rank d start at dbase[d] and are in slot order — and its slot becomes empty
__global__ __launch_bounds__(256) void k_mig_pack(double *__restrict__ rec, double *X, unsigned char *state, long long *id, double *U,
                                                  idx_t cap, const int *__restrict__ dest, const int *__restrict__ code,
                                                  const unsigned long long *__restrict__ offs,
                                                  const unsigned long long *__restrict__ dbase)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= cap) return;
    const int d = dest[p];
    if (d < 0) return;
    const idx_t nwg = gridDim.x;
    double *r = rec + NS3D_MIG_REC * (idx_t)(dbase[d] + offs[(idx_t)d * nwg + blockIdx.x] + (unsigned long long)(code[p] >> 8));
    const double nan = quiet_nan();
    r[0] = X[p]; r[1] = X[cap + p]; r[2] = X[2 * cap + p];
    r[3] = __longlong_as_double(id[p]);
    r[4] = U ? U[p] : nan; r[5] = U ? U[cap + p] : nan; r[6] = U ? U[2 * cap + p] : nan;
    r[7] = 0.0;
    X[p] = nan; X[cap + p] = nan; X[2 * cap + p] = nan;
    if (U) { U[p] = nan; U[cap + p] = nan; U[2 * cap + p] = nan; }
    id[p] = -1;
    state[p] = 0;
}

// the n_arr received records go into the empty slots in ascending slot order
__global__ __launch_bounds__(256) void k_mig_insert(double *X, unsigned char *state, long long *id, double *U, idx_t cap,
                                                    const int *__restrict__ code, const unsigned long long *__restrict__ offs_empty,
                                                    const double *__restrict__ rec, idx_t n_arr)
{
    const idx_t p = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= cap) return;
    const int c = code[p];
    if (c < 0) return;
    const idx_t e = (idx_t)offs_empty[blockIdx.x] + (c & 255);
    if (e >= n_arr) return;
    const double *r = rec + NS3D_MIG_REC * e;
    X[p] = r[0]; X[cap + p] = r[1]; X[2 * cap + p] = r[2];
    id[p] = __double_as_longlong(r[3]);
    if (U) { U[p] = r[4]; U[cap + p] = r[5]; U[2 * cap + p] = r[6]; }
    state[p] = 1;
}

hipError_t mig_count(hipStream_t s, const ns3d_mig_scratch &w, const double *X, const unsigned char *state, const long long *id, long cap,
                     const ns3d_mig_geom &g)
{
    const unsigned nwg = (unsigned)((cap + 255) / 256);
    if (nwg) {
        hipError_t e = hipMemsetAsync(w.counts, 0, (size_t)(g.P + 1) * nwg * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mig_classify, dim3(nwg), dim3(256), 0, s, w.dest, w.code, w.counts, X, state, id, (idx_t)cap, g);
    }
    hipLaunchKernelGGL(k_mig_scan, dim3((unsigned)(g.P + 1)), dim3(256), 0, s, w.counts, w.offs, w.totals, (idx_t)nwg);
    return hipGetLastError();
}
hipError_t mig_pack(hipStream_t s, const ns3d_mig_scratch &w, double *rec, double *X, unsigned char *state, long long *id, double *U,
                    long cap)
{
    hipLaunchKernelGGL(k_mig_pack, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, rec, X, state, id, U, (idx_t)cap, w.dest, w.code,
                       w.offs, w.dbase);
    return hipGetLastError();
}
hipError_t mig_insert(hipStream_t s, const ns3d_mig_scratch &w, int P, const double *rec, long n_arr, double *X, unsigned char *state,
                      long long *id, double *U, long cap)
{
    const unsigned nwg = (unsigned)((cap + 255) / 256);
    hipLaunchKernelGGL(k_mig_insert, dim3(nwg), dim3(256), 0, s, X, state, id, U, (idx_t)cap, w.code, w.offs + (size_t)P * nwg, rec,
                       (idx_t)n_arr);
    return hipGetLastError();
}

} // namespace ns3d_tracers
