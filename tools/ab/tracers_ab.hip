// tracers_ab.hip — stand-alone A/B of the forms k_tracers (navierstokes3d_amd/csrc/ns3d_tracers.hip) could take:
//   1t/256 — one thread per particle, 256-thread workgroups (the base form, the one built into the library);
//   1t/64  — one thread per particle, 64-thread workgroups;
//   3t/256, 3t/64 — three threads per particle, one per velocity component, in workgroups of 256×3 resp. 64×3 threads (a wave holds
//            one component of 64 consecutive particles; v1 and Xn pass through LDS, two barriers per step);
// and of the ORDER of the particles in memory: the same set in lattice order (x fastest, like the cells) and randomly permuted.
// Every variant is first compared bit for bit (X, state, U) with the base form on 131×66×37 — 100 003 particles, some dead, outside or
// not finite, Courant factors 2.5, 2.25, 2.0 so that many leave — then timed with events: best of 10 after 3 warm-ups, the particle
// arrays restored before every run (outside the timed window), N = 2^20 and 2^24 on 255×153×153 and 512³, fp64 and fp32 fields,
// Courant factors 0.4, 0.36, 0.32, fields U(−1,1).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ab/tracers_ab.hip -o tools/ab/tracers_ab
//   tools/ab/tracers_ab > profiles/tracers_variants_ab.log
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#pragma clang fp contract(off)

typedef long long idx_t;

#define CK(e)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (e);                                                                   \
        if (e_ != hipSuccess) { std::printf("%s: %s\n", #e, hipGetErrorString(e_)); std::exit(2); } \
    } while (0)

// ---- the definition, as in ns3d_tracers.hip --------------------------------------------------------------------------------------
struct Axis { int i0; double t; };
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
struct Interp {
    double v[8], tx, ty, tz;
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
        const double fy1z1 = lerp(v[0], v[1], tx), fy1z2 = lerp(v[4], v[5], tx), fy2z1 = lerp(v[2], v[3], tx), fy2z2 = lerp(v[6], v[7], tx);
        return lerp(lerp(fy1z1, fy2z1, ty), lerp(fy1z2, fy2z2, ty), tz);
    }
};
__device__ __forceinline__ bool inside(double p, int hi) { return p >= 0.0 && p <= (double)hi; }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

template <class T>
struct Args {
    double *X;
    unsigned char *state;
    double *U;
    idx_t n;
    const T *V[3];
    double c[3];
    int nx, ny, nz;
};

// one thread per particle, WG threads per workgroup
template <class T, int WG>
__global__ __launch_bounds__(WG) void k_one(Args<T> a)
{
    const idx_t p = (idx_t)blockIdx.x * WG + threadIdx.x, n = a.n;
    if (p >= n) return;
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const double x = a.X[p], y = a.X[n + p], z = a.X[2 * n + p];
    if (!(a.state[p] == 1 && inside(x, nx) && inside(y, ny) && inside(z, nz))) {
        a.state[p] = 0;
        a.U[p] = quiet_nan(); a.U[n + p] = quiet_nan(); a.U[2 * n + p] = quiet_nan();
        return;
    }
    Interp fx, fy, fz;
    fx.issue(a.V[0], nx + 1, ny, nz, 1, 0, 0, x, y, z);
    fy.issue(a.V[1], nx, ny + 1, nz, 0, 1, 0, x, y, z);
    fz.issue(a.V[2], nx, ny, nz + 1, 0, 0, 1, x, y, z);
    double u = fx.value(), v = fy.value(), w = fz.value();
    a.U[p] = u; a.U[n + p] = v; a.U[2 * n + p] = w;
    double xn = x + 0.5 * (u * a.c[0]), yn = y + 0.5 * (v * a.c[1]), zn = z + 0.5 * (w * a.c[2]);
    if (isfinite(xn) && isfinite(yn) && isfinite(zn)) {
        fx.issue(a.V[0], nx + 1, ny, nz, 1, 0, 0, xn, yn, zn);
        fy.issue(a.V[1], nx, ny + 1, nz, 0, 1, 0, xn, yn, zn);
        fz.issue(a.V[2], nx, ny, nz + 1, 0, 0, 1, xn, yn, zn);
        u = fx.value(); v = fy.value(); w = fz.value();
        xn = x + u * a.c[0]; yn = y + v * a.c[1]; zn = z + w * a.c[2];
    }
    a.X[p] = xn; a.X[n + p] = yn; a.X[2 * n + p] = zn;
    a.state[p] = inside(xn, nx) && inside(yn, ny) && inside(zn, nz) ? 1 : 0;
}

// three threads per particle: threadIdx.y = component; PB particles per workgroup.  No thread leaves before the last barrier.
template <class T, int PB>
__global__ __launch_bounds__(PB * 3) void k_three(Args<T> a)
{
    __shared__ double sh[3][PB];
    const int q = threadIdx.y, l = threadIdx.x;
    const idx_t p = (idx_t)blockIdx.x * PB + l, n = a.n;
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const bool in_range = p < n;
    double x = 0.0, y = 0.0, z = 0.0;
    bool act = false;
    if (in_range) {
        x = a.X[p]; y = a.X[n + p]; z = a.X[2 * n + p];
        act = a.state[p] == 1 && inside(x, nx) && inside(y, ny) && inside(z, nz);
    }
    const int ex = nx + (q == 0), ey = ny + (q == 1), ez = nz + (q == 2);
    const T *__restrict__ A = a.V[q];
    const double own = q == 0 ? x : q == 1 ? y : z, cq = a.c[q];
    double v1 = quiet_nan();
    if (act) {
        Interp f;
        f.issue(A, ex, ey, ez, q == 0, q == 1, q == 2, x, y, z);
        v1 = f.value();
    }
    if (in_range) a.U[q * n + p] = v1;
    sh[q][l] = own + 0.5 * (v1 * cq);
    __syncthreads();
    const double xm = sh[0][l], ym = sh[1][l], zm = sh[2][l];
    __syncthreads();
    double outq = own;
    if (act) {
        outq = q == 0 ? xm : q == 1 ? ym : zm;
        if (isfinite(xm) && isfinite(ym) && isfinite(zm)) {
            Interp f;
            f.issue(A, ex, ey, ez, q == 0, q == 1, q == 2, xm, ym, zm);
            outq = own + f.value() * cq;
        }
        a.X[q * n + p] = outq;
    }
    sh[q][l] = outq;
    __syncthreads();
    if (in_range && q == 0)
        a.state[p] = act && inside(sh[0][l], nx) && inside(sh[1][l], ny) && inside(sh[2][l], nz) ? 1 : 0;
}

template <class T>
struct Variant {
    const char *name;
    void (*fn)(const Args<T> &);
};
template <class T, int WG>
static void launch_one(const Args<T> &a) { hipLaunchKernelGGL((k_one<T, WG>), dim3((unsigned)((a.n + WG - 1) / WG)), dim3(WG), 0, 0, a); }
template <class T, int PB>
static void launch_three(const Args<T> &a) { hipLaunchKernelGGL((k_three<T, PB>), dim3((unsigned)((a.n + PB - 1) / PB)), dim3(PB, 3), 0, 0, a); }
template <class T>
static std::vector<Variant<T>> variants()
{
    return {{"1 thread/particle, wg 256 (base)", launch_one<T, 256>}, {"1 thread/particle, wg 64", launch_one<T, 64>},
            {"3 threads/particle, wg 256x3", launch_three<T, 256>}, {"3 threads/particle, wg 64x3", launch_three<T, 64>}};
}

// ---- fields and particle sets -----------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
template <class T>
__global__ void k_fill(T *A, idx_t n, unsigned long long seed)
{
    const idx_t i = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) A[i] = (T)((double)(mix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1)) >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}
template <class T>
struct Fields {
    T *V[3];
    int nx, ny, nz;
    Fields(int nx_, int ny_, int nz_) : nx(nx_), ny(ny_), nz(nz_)
    {
        const idx_t nV[3] = {(idx_t)(nx + 1) * ny * nz, (idx_t)nx * (ny + 1) * nz, (idx_t)nx * ny * (nz + 1)};
        for (int q = 0; q < 3; ++q) {
            CK(hipMalloc(&V[q], (size_t)nV[q] * sizeof(T)));
            hipLaunchKernelGGL(k_fill<T>, dim3((unsigned)((nV[q] + 255) / 256)), dim3(256), 0, 0, V[q], nV[q], 1000ull + q);
        }
        CK(hipDeviceSynchronize());
    }
    ~Fields() { for (int q = 0; q < 3; ++q) (void)hipFree(V[q]); }
};
struct Particles {      // pristine copies X0 / S0 and the working arrays
    double *X0, *X, *U;
    unsigned char *S0, *S;
    idx_t n;
    explicit Particles(idx_t n_) : n(n_)
    {
        CK(hipMalloc(&X0, 3 * n * sizeof(double))); CK(hipMalloc(&X, 3 * n * sizeof(double))); CK(hipMalloc(&U, 3 * n * sizeof(double)));
        CK(hipMalloc(&S0, n)); CK(hipMalloc(&S, n));
    }
    ~Particles() { (void)hipFree(X0); (void)hipFree(X); (void)hipFree(U); (void)hipFree(S0); (void)hipFree(S); }
    void upload(const std::vector<double> &x, const std::vector<unsigned char> &s)
    {
        CK(hipMemcpy(X0, x.data(), 3 * n * sizeof(double), hipMemcpyHostToDevice));
        CK(hipMemcpy(S0, s.data(), n, hipMemcpyHostToDevice));
    }
    void restore()
    {
        CK(hipMemcpyAsync(X, X0, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, 0));
        CK(hipMemcpyAsync(S, S0, n, hipMemcpyDeviceToDevice, 0));
        CK(hipMemsetAsync(U, 0xff, 3 * n * sizeof(double), 0));
    }
};
template <class T>
static Args<T> args_of(const Fields<T> &f, const Particles &p, double cx, double cy, double cz)
{
    return {p.X, p.S, p.U, p.n, {f.V[0], f.V[1], f.V[2]}, {cx, cy, cz}, f.nx, f.ny, f.nz};
}

template <class T>
static int check(const char *tname)
{
    const int nx = 131, ny = 66, nz = 37;
    const idx_t n = 100003;
    Fields<T> f(nx, ny, nz);
    Particles p(n);
    std::vector<double> x(3 * n);
    std::vector<unsigned char> s(n);
    const double ext[3] = {(double)nx, (double)ny, (double)nz};
    for (idx_t i = 0; i < n; ++i) {
        for (int q = 0; q < 3; ++q) x[q * n + i] = (double)(mix64(7919ull * (i + 1) + q) >> 11) / 9007199254740992.0 * ext[q];
        s[i] = i % 7 != 3;
        if (i % 101 == 5) x[(i % 3) * n + i] = ext[i % 3] + 0.25;          // outside
        if (i % 211 == 9) x[(i % 3) * n + i] = i % 2 ? NAN : INFINITY;      // not finite
        if (i % 307 == 1) x[(i % 3) * n + i] = i % 2 ? 0.0 : ext[i % 3];    // on a face
    }
    p.upload(x, s);
    const Args<T> a = args_of(f, p, 2.5, 2.25, 2.0);
    std::vector<double> rx(3 * n), ru(3 * n), gx(3 * n), gu(3 * n);
    std::vector<unsigned char> rs(n), gs(n);
    int bad = 0;
    bool first = true;
    long dead = 0;
    for (auto &v : variants<T>()) {
        p.restore();
        v.fn(a);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(gx.data(), p.X, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        CK(hipMemcpy(gu.data(), p.U, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        CK(hipMemcpy(gs.data(), p.S, n, hipMemcpyDeviceToHost));
        if (first) {
            rx = gx; ru = gu; rs = gs; first = false;
            for (idx_t i = 0; i < n; ++i) dead += s[i] == 1 && gs[i] == 0;
            continue;
        }
        const bool same = !std::memcmp(rx.data(), gx.data(), 3 * n * sizeof(double)) && !std::memcmp(ru.data(), gu.data(), 3 * n * sizeof(double)) &&
                          !std::memcmp(rs.data(), gs.data(), n);
        if (!same) { ++bad; std::printf("MISMATCH %s %s\n", tname, v.name); }
    }
    std::printf("check %s 131x66x37, %lld particles (%ld die in the step): %d of %zu variants differ from the base form in X, state or U\n",
                tname, (long long)n, dead, bad, variants<T>().size() - 1);
    return bad;
}

// N = mx·my·mz particles on a regular lattice over the box, x fastest; `permute`: the same set in random order
static void lattice(std::vector<double> &x, idx_t n, int mx, int my, int mz, int nx, int ny, int nz, bool permute)
{
    std::vector<unsigned> slot((size_t)n);
    std::iota(slot.begin(), slot.end(), 0u);
    if (permute) {
        unsigned long long st = 0x243F6A8885A308D3ull;
        for (idx_t i = n - 1; i > 0; --i) {
            st += 0x9E3779B97F4A7C15ull;
            const idx_t j = (idx_t)(mix64(st) % (unsigned long long)(i + 1));
            std::swap(slot[(size_t)i], slot[(size_t)j]);
        }
    }
    x.resize(3 * (size_t)n);
    for (idx_t s = 0; s < n; ++s) {
        const idx_t m = slot[(size_t)s];
        const int i = (int)(m % mx), j = (int)((m / mx) % my), k = (int)(m / ((idx_t)mx * my));
        x[(size_t)s] = (i + 0.37) * nx / mx;
        x[(size_t)(n + s)] = (j + 0.41) * ny / my;
        x[(size_t)(2 * n + s)] = (k + 0.43) * nz / mz;
    }
}

template <class T>
static void time_grid(const char *tname, int nx, int ny, int nz)
{
    Fields<T> f(nx, ny, nz);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double field_mb = 3.0 * sizeof(T) * (double)nx * ny * nz / 1048576.0;
    const int lat[2][3] = {{128, 128, 64}, {256, 256, 256}};
    for (int c = 0; c < 2; ++c) {
        const idx_t n = (idx_t)lat[c][0] * lat[c][1] * lat[c][2];
        Particles p(n);
        std::vector<unsigned char> s((size_t)n, 1);
        for (int permute = 0; permute < 2; ++permute) {
            std::vector<double> x;
            lattice(x, n, lat[c][0], lat[c][1], lat[c][2], nx, ny, nz, permute != 0);
            p.upload(x, s);
            const Args<T> a = args_of(f, p, 0.4, 0.36, 0.32);
            std::printf("%s %dx%dx%d (fields %.0f MiB)  N = 2^%d  %s  (particle arrays: %.0f MiB read + written)\n", tname, nx, ny, nz, field_mb,
                        c ? 24 : 20, permute ? "randomly permuted" : "lattice order", 2.0 * 25.0 * (double)n / 1048576.0 + 24.0 * (double)n / 1048576.0);
            for (auto &v : variants<T>()) {
                float best = 1e30f;
                for (int it = 0; it < 13; ++it) {
                    p.restore();
                    CK(hipEventRecord(e0, 0));
                    v.fn(a);
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float ms;
                    CK(hipEventElapsedTime(&ms, e0, e1));
                    if (it >= 3 && ms < best) best = ms;
                }
                CK(hipGetLastError());
                std::printf("  %-34s %9.4f ms  %9.1f M particles/s\n", v.name, best, (double)n / best / 1e3);
                std::fflush(stdout);
            }
        }
    }
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

int main()
{
    if (check<double>("fp64") + check<float>("fp32")) return 1;
    time_grid<double>("fp64", 255, 153, 153);
    time_grid<float>("fp32", 255, 153, 153);
    time_grid<double>("fp64", 512, 512, 512);
    time_grid<float>("fp32", 512, 512, 512);
    return 0;
}
