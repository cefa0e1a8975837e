// ns3d_scalar.hip — the active scalar (include/ns3d.h has the statements): ns3d_scalar_diffuse, one explicit step of
// ∂C/∂t = ∇·(K ∇C) in flux form with zero flux through the six domain faces, ns3d_buoyancy, the Boussinesq term of the vertical
// momentum, and ns3d_scalar_step, both in one pass.  ONE kernel template, k_scalar<DIFF, BUOY, VAR>, serves the three entry points:
// the fused call and the single calls share their arithmetic by construction.
//
// Compiled four times by navierstokes3d_amd/build.py with the switches of ns3d_kernels.hip (STRICT, NS3D_EXACT_RECIP,
// NS3D_POW2_RECIP, FAST) into the same four namespaces, and with -ffp-contract=off in ALL of them: where FAST fuses, the code says
// fma.  A product that the compiler may fuse into whichever sum consumes it is what made a fused kernel and its unfused statement
// differ by an ulp in DESIGN §4.15; here no instantiation leaves that choice open.  FAST therefore differs from STRICT by the
// reciprocal spacings and by the three fma of mad() below (K, C_out, Vz) — nothing else.
#include "ns3d_launch.h"

#if defined(NS3D_MODE_FAST)
#define NS3D_NS ns3d_fast
#define NS3D_FASTMATH 1
#elif defined(NS3D_MODE_STRICT) && defined(NS3D_EXACT_RECIP)
#define NS3D_NS ns3d_strictx
#define NS3D_FASTMATH 0
#elif defined(NS3D_MODE_STRICT) && defined(NS3D_POW2_RECIP)
#define NS3D_NS ns3d_strictp
#define NS3D_FASTMATH 0
#elif defined(NS3D_MODE_STRICT)
#define NS3D_NS ns3d_strict
#define NS3D_FASTMATH 0
#else
#error "compile with -DNS3D_MODE_STRICT or -DNS3D_MODE_FAST"
#endif

namespace NS3D_NS {
namespace scalar_detail {

typedef long long idx_t;

// The spacings and the division x/d of each build: ns3d_kernels.hip's, restated because that unit keeps them in its own text (its
// division guards are read from there by tests/div_model.py).  tests/test_scalar_host.py holds the two texts equal.
template <class T>
struct Geo {
    T dx, dy, dz;
    T rdx, rdy, rdz;    // 1/dx …
};
template <class T>
static Geo<T> make_geo(double dx, double dy, double dz)
{
    Geo<T> g;
    g.dx = (T)dx; g.dy = (T)dy; g.dz = (T)dz;
    g.rdx = (T)1 / g.dx; g.rdy = (T)1 / g.dy; g.rdz = (T)1 / g.dz;   // RN(1/d) in the element type
    return g;
}
template <class T> struct DivLim;
template <> struct DivLim<double> { static constexpr double lo = 0x1p-900, hi = 0x1p900; };
template <> struct DivLim<float> { static constexpr float lo = 0x1p-83f, hi = 0x1p100f; };
template <class T>
__device__ __forceinline__ T div_by_known(T x, T d, T r)
{
    const T q = x * r;
    const T e = __builtin_fma(-q, d, x);
    T q1 = __builtin_fma(e, r, q);
    const T aq = __builtin_fabs(q);
    if (__builtin_expect(!(aq > DivLim<T>::lo && aq < DivLim<T>::hi), 0)) {
        q1 = x;                                 // ±0 / d = ±0: a wave whose only outliers are zeros skips the division
        if (x != (T)0) q1 = x / d;
    }
    return q1;
}
__device__ __forceinline__ float div_by_known(float x, float d, float r)
{
    const float q = x * r;
    const float e = __builtin_fmaf(-q, d, x);
    float q1 = __builtin_fmaf(e, r, q);
    const float aq = __builtin_fabsf(q);
    if (__builtin_expect(!(aq > DivLim<float>::lo && aq < DivLim<float>::hi), 0)) {
        q1 = x;
        if (x != 0.0f) q1 = x / d;
    }
    return q1;
}
#if NS3D_FASTMATH || defined(NS3D_POW2_RECIP)
#define DIV_X(v) ((v)*g.rdx)
#define DIV_Y(v) ((v)*g.rdy)
#define DIV_Z(v) ((v)*g.rdz)
#elif defined(NS3D_EXACT_RECIP)
#define DIV_X(v) div_by_known((v), g.dx, g.rdx)
#define DIV_Y(v) div_by_known((v), g.dy, g.rdy)
#define DIV_Z(v) div_by_known((v), g.dz, g.rdz)
#else
#define DIV_X(v) ((v) / g.dx)
#define DIV_Y(v) ((v) / g.dy)
#define DIV_Z(v) ((v) / g.dz)
#endif

// a·b + c: two roundings in STRICT, one in FAST — the ONLY places where FAST contracts (the unit is built without contraction)
__device__ __forceinline__ double mad(double a, double b, double c)
{
#if NS3D_FASTMATH
    return __builtin_fma(a, b, c);
#else
    return a * b + c;
#endif
}
__device__ __forceinline__ float mad(float a, float b, float c)
{
#if NS3D_FASTMATH
    return __builtin_fmaf(a, b, c);
#else
    return a * b + c;
#endif
}

template <class T>
struct Par {
    T kappa, sgs, mu, bg, c_ref, dt;
};
// the statements, each written once
template <class T>
__device__ __forceinline__ T diffusivity(const Par<T> &p, T m) { return mad(p.sgs, m - p.mu, p.kappa); }   // K = κ + sgs·(μ_e − μ)
template <class T>
__device__ __forceinline__ T face_mean(T ka, T kb) { return (T)0.5 * (ka + kb); }
template <class T>
__device__ __forceinline__ T diffuse_update(const Par<T> &p, T c, T Dx, T Dy, T Dz) { return mad(p.dt, (Dx + Dy) + Dz, c); }
template <class T>
__device__ __forceinline__ T buoyancy_update(const Par<T> &p, T vz, T c_lo, T c_hi)
{
    return mad(p.dt, p.bg * ((T)0.5 * (c_lo + c_hi) - p.c_ref), vz);
}

// ---------------------------------------------------------------------------------------------------------
// k_scalar<DIFF, BUOY, VAR>: a workgroup owns 64×4 cell columns (one per thread, a wave is an x-contiguous row of 64) and marches
// NS3D_SCALAR_KZ planes of its chunk [kb, ke):
//   z — C of planes k−1, k, k+1 (and K with VAR) travel in registers; plane k+1 is loaded while plane k is worked on;
//   x, y — C (and K) of plane k are staged in LDS with a one-cell ring, no corners, rows of 66 elements (consecutive lanes,
//       consecutive banks).  The ring cells are loaded by the waves themselves, k_vortex's way: wave 0 / 1 the row below / above
//       the tile, wave 2 / 3 lanes 0…3 the column left / right of it.  Two buffers, so ONE barrier per plane.
// A face's flux is formed by both cells that share it from the same operands through the same function: the same bits on both
// sides.  A domain face's flux is +0.0 by selection, so ring cells outside the grid are neither loaded nor used.
// BUOY: face k of Vz (between cells k−1 and k, both in registers) for k ≥ 1 belongs to the chunk that holds plane k; face nz and
// face 0 to nobody.  Without DIFF there is no LDS and no barrier.
// ---------------------------------------------------------------------------------------------------------
template <bool DIFF, bool BUOY, bool VAR, class T>
__global__ __launch_bounds__(256) void k_scalar(T *__restrict__ C_out, T *__restrict__ Vz, const T *__restrict__ C,
                                                const T *__restrict__ mu_e, Par<T> p, Geo<T> g, int nx, int ny, int nz, int kz)
{
    constexpr int TY = 4, S = 66, NP = (TY + 2) * S, NB = (VAR ? 2 : 1) * NP;      // C | K of one buffer
    __shared__ T lds[DIFF ? 2 * NB : 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * TY, i = i0 + tx, j = j0 + ty;
    const int kb = blockIdx.z * kz, ke = min(kb + kz, nz);
    const idx_t pC = (idx_t)nx * ny, oC = (idx_t)i + (idx_t)nx * j;
    const bool live = i < nx && j < ny;
    const bool lift = BUOY && i >= 1 && i <= nx - 2 && j >= 1 && j <= ny - 2;     // @inn(Vz) in x and y
    const T kconst = face_mean(p.kappa, p.kappa);          // every face's diffusivity without a field

    T cm = 0, cc = 0, km = 0, kc = 0;
    if (live) {
        if (kb > 0) {
            cm = C[oC + pC * (kb - 1)];
            if constexpr (DIFF && VAR) km = diffusivity(p, mu_e[oC + pC * (kb - 1)]);
        }
        cc = C[oC + pC * kb];
        if constexpr (DIFF && VAR) kc = diffusivity(p, mu_e[oC + pC * kb]);
    }
    // the ring cell this thread stages besides its own
    const bool ring_row = ty < 2;
    const int ei = ring_row ? i : (ty == 2 ? i0 - 1 : i0 + 64), ej = ring_row ? (ty == 0 ? j0 - 1 : j0 + TY) : j0 + tx;
    const bool ring = DIFF && (ring_row || tx < TY) && ei >= 0 && ei < nx && ej >= 0 && ej < ny;
    const int ring_s = ring_row ? (ty == 0 ? 0 : TY + 1) * S + tx + 1 : (tx + 1) * S + (ty == 2 ? 0 : 65);
    const idx_t eC = (idx_t)ei + (idx_t)nx * ej;
    T ec = 0, ek = 0;
    if (ring) {
        ec = C[eC + pC * kb];
        if constexpr (VAR) ek = diffusivity(p, mu_e[eC + pC * kb]);
    }

    for (int k = kb; k < ke; ++k) {
        const bool up = k + 1 < nz;
        T cp = 0, kp = 0;
        if (live && up) {
            if constexpr (DIFF) {
                cp = C[oC + pC * (k + 1)];
                if constexpr (VAR) kp = diffusivity(p, mu_e[oC + pC * (k + 1)]);
            } else if (k + 1 < ke) {
                cp = C[oC + pC * (k + 1)];
            }
        }
        if constexpr (BUOY) {
            if (lift && k >= 1) {
                const idx_t v = oC + pC * k;
                Vz[v] = buoyancy_update(p, Vz[v], cm, cc);
            }
        }
        if constexpr (DIFF) {
            T *buf = lds + ((k - kb) & 1) * NB;
            const int own = (ty + 1) * S + tx + 1;
            buf[own] = cc;
            if constexpr (VAR) buf[NP + own] = kc;
            if (ring) {
                buf[ring_s] = ec;
                if constexpr (VAR) buf[NP + ring_s] = ek;
                if (k + 1 < ke) {
                    ec = C[eC + pC * (k + 1)];
                    if constexpr (VAR) ek = diffusivity(p, mu_e[eC + pC * (k + 1)]);
                }
            }
            __syncthreads();
            if (live) {
                const T *sc = buf + own, *sk = buf + NP + own;
                const T zero = (T)0;
                // flux through the face between a lower cell (c0, k0) and an upper one (c1, k1); +0.0 through a domain face
                const T kxl = VAR ? face_mean(sk[-1], kc) : kconst, kxr = VAR ? face_mean(kc, sk[1]) : kconst;
                const T kyl = VAR ? face_mean(sk[-S], kc) : kconst, kyr = VAR ? face_mean(kc, sk[S]) : kconst;
                const T kzl = VAR ? face_mean(km, kc) : kconst, kzr = VAR ? face_mean(kc, kp) : kconst;
                const T fxl = i > 0 ? kxl * DIV_X(cc - sc[-1]) : zero, fxr = i < nx - 1 ? kxr * DIV_X(sc[1] - cc) : zero;
                const T fyl = j > 0 ? kyl * DIV_Y(cc - sc[-S]) : zero, fyr = j < ny - 1 ? kyr * DIV_Y(sc[S] - cc) : zero;
                const T fzl = k > 0 ? kzl * DIV_Z(cc - cm) : zero, fzr = up ? kzr * DIV_Z(cp - cc) : zero;
                const T Dx = DIV_X(fxr - fxl), Dy = DIV_Y(fyr - fyl), Dz = DIV_Z(fzr - fzl);
                C_out[oC + pC * k] = diffuse_update(p, cc, Dx, Dy, Dz);
            }
        }
        cm = cc; cc = cp; km = kc; kc = kp;
    }
}

template <bool DIFF, bool BUOY, bool VAR, class T>
static hipError_t launch(hipStream_t s, T *C_out, T *Vz, const T *C, const T *mu_e, const Par<T> &p, const Geo<T> &g, int nx, int ny,
                         int nz)
{
    const int kz = NS3D_SCALAR_KZ;
    const dim3 blk(64, 4, 1);
    const dim3 grd((unsigned)((nx + 63) / 64), (unsigned)((ny + 3) / 4), (unsigned)((nz + kz - 1) / kz));
    hipLaunchKernelGGL((k_scalar<DIFF, BUOY, VAR, T>), grd, blk, 0, s, C_out, Vz, C, mu_e, p, g, nx, ny, nz, kz);
    return hipGetLastError();
}
} // namespace scalar_detail

// what: bit 0 the diffusion (C_out from C, mu_e may be null), bit 1 the buoyancy (Vz in place).  The API has checked the arguments.
template <class T>
hipError_t scalar_step(hipStream_t s, int what, T *C_out, T *Vz, const T *C, const T *mu_e, double kappa, double sgs, double mu, double bg,
                       double c_ref, double dt, double dx, double dy, double dz, int nx, int ny, int nz)
{
    using namespace scalar_detail;
    const Par<T> p = {(T)kappa, (T)sgs, (T)mu, (T)bg, (T)c_ref, (T)dt};
    const Geo<T> g = make_geo<T>(dx, dy, dz);
    const bool var = mu_e != nullptr;
    switch (what & 3) {
    case 1: return var ? launch<true, false, true>(s, C_out, Vz, C, mu_e, p, g, nx, ny, nz)
                       : launch<true, false, false>(s, C_out, Vz, C, mu_e, p, g, nx, ny, nz);
    case 2: return launch<false, true, false>(s, C_out, Vz, C, mu_e, p, g, nx, ny, nz);
    case 3: return var ? launch<true, true, true>(s, C_out, Vz, C, mu_e, p, g, nx, ny, nz)
                       : launch<true, true, false>(s, C_out, Vz, C, mu_e, p, g, nx, ny, nz);
    default: return hipErrorInvalidValue;
    }
}
template hipError_t scalar_step<double>(hipStream_t, int, double *, double *, const double *, const double *, double, double, double, double,
                                        double, double, double, double, double, int, int, int);
template hipError_t scalar_step<float>(hipStream_t, int, float *, float *, const float *, const float *, double, double, double, double,
                                       double, double, double, double, double, int, int, int);

} // namespace NS3D_NS
