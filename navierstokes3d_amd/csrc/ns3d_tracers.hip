// ns3d_tracers.hip — ns3d_sample and ns3d_tracers_advance (include/ns3d.h has the definition): a field interpolated at points the
// caller chooses, and one explicit-midpoint step of Lagrangian particles through the frozen staggered velocity field.
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

#define INST(T)                                                                                                                   \
    template hipError_t sample<T>(hipStream_t, double *, const double *, const unsigned char *, long, const T *, int, int, int, int, \
                                  int, int);                                                                                      \
    template hipError_t advance<T>(hipStream_t, double *, unsigned char *, double *, long, const T *, const T *, const T *, double, \
                                   double, double, int, int, int);
INST(double)
INST(float)
#undef INST

} // namespace ns3d_tracers
