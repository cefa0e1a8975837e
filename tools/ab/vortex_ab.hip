// vortex_ab.hip — stand-alone A/B of the forms k_vortex (navierstokes3d_amd/csrc/ns3d_kernels.hip) could take:
//   staged — the centred u, v, w of the current plane go through LDS with a one-cell ring (u in y, v in x, w in both);
//   plain  — every x / y neighbour is formed from global loads of its own that L1 / L2 serve (k_stats' way);
// each over tiles of 64 × TY·R cell columns (TY waves, R rows per thread) marching KZ planes per workgroup, with the centred u and v
// of planes k−1, k, k+1 in a register ring.  Divisions are multiplications by the reciprocal without contraction (the power-of-two
// STRICT build's form).  Every variant is first compared bit for bit with a one-thread-per-cell kernel on 131×66×37, then timed with
// events: best of 10 after 3 warm-ups, 512³ and 255×153×153, fp64 and fp32, all four outputs.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ab/vortex_ab.hip -o vortex_ab && ./vortex_ab > profiles/vortex_variants_ab.log
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef long long idx_t;
template <class T>
struct Geo { T rdx, rdy, rdz; };
#define DIV_X(v) ((v)*g.rdx)
#define DIV_Y(v) ((v)*g.rdy)
#define DIV_Z(v) ((v)*g.rdz)

#define CK(e)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (e);                                                                   \
        if (e_ != hipSuccess) { std::printf("%s: %s\n", #e, hipGetErrorString(e_)); std::exit(2); } \
    } while (0)

// the definition, one thread per cell, every value from global memory
template <class T>
__global__ void k_naive(T *Wx, T *Wy, T *Wz, T *Q, const T *Vx, const T *Vy, const T *Vz, Geo<T> g, int nx, int ny, int nz)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i >= nx || j >= ny) return;
    const T h = (T)0.5;
    const idx_t c = i + (idx_t)nx * (j + (idx_t)ny * k);
    if (i < 1 || i > nx - 2 || j < 1 || j > ny - 2 || k < 1 || k > nz - 2) { Wx[c] = Wy[c] = Wz[c] = Q[c] = (T)0; return; }
    auto X = [&](int a, int b, int d) { return Vx[a + (idx_t)(nx + 1) * (b + (idx_t)ny * d)]; };
    auto Y = [&](int a, int b, int d) { return Vy[a + (idx_t)nx * (b + (idx_t)(ny + 1) * d)]; };
    auto Z = [&](int a, int b, int d) { return Vz[a + (idx_t)nx * (b + (idx_t)ny * d)]; };
    auto u = [&](int a, int b, int d) { return h * (X(a, b, d) + X(a + 1, b, d)); };
    auto v = [&](int a, int b, int d) { return h * (Y(a, b, d) + Y(a, b + 1, d)); };
    auto w = [&](int a, int b, int d) { return h * (Z(a, b, d) + Z(a, b, d + 1)); };
    const T gxx = DIV_X(X(i + 1, j, k) - X(i, j, k)), gyy = DIV_Y(Y(i, j + 1, k) - Y(i, j, k)), gzz = DIV_Z(Z(i, j, k + 1) - Z(i, j, k));
    const T uy = h * DIV_Y(u(i, j + 1, k) - u(i, j - 1, k)), uz = h * DIV_Z(u(i, j, k + 1) - u(i, j, k - 1));
    const T vx = h * DIV_X(v(i + 1, j, k) - v(i - 1, j, k)), vz = h * DIV_Z(v(i, j, k + 1) - v(i, j, k - 1));
    const T wx = h * DIV_X(w(i + 1, j, k) - w(i - 1, j, k)), wy = h * DIV_Y(w(i, j + 1, k) - w(i, j - 1, k));
    Wx[c] = wy - vz; Wy[c] = uz - wx; Wz[c] = vx - uy;
    Q[c] = ((-h) * ((gxx * gxx + gyy * gyy) + gzz * gzz)) - ((uy * vx + uz * wx) + vz * wy);
}

template <class T, int TY, int R, bool STAGE>
__global__ __launch_bounds__(64 * TY) void k_vortex(T *__restrict__ Wx, T *__restrict__ Wy, T *__restrict__ Wz, T *__restrict__ Q,
                                                    const T *__restrict__ Vx, const T *__restrict__ Vy, const T *__restrict__ Vz,
                                                    Geo<T> g, int nx, int ny, int nz, int kz)
{
    constexpr int TYR = TY * R, SU = 64, SV = 66;
    constexpr int NU = (TYR + 2) * SU, NV = TYR * SV, NW = (TYR + 2) * SV, NB = NU + NV + NW;
    __shared__ T lds[STAGE ? 2 * NB : 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.x * 64 + tx, j0 = blockIdx.y * TYR;
    const int kb = blockIdx.z * kz, ke = min(kb + kz, nz);
    const int ks = max(kb, 1), kt = min(ke, nz - 1);       // the chunk's interior planes [ks, kt)
    const T h = (T)0.5;
    const idx_t pVx = (idx_t)(nx + 1) * ny, pVy = (idx_t)nx * (ny + 1), pC = (idx_t)nx * ny;
    const bool want_wx = Wx != nullptr, want_wy = Wy != nullptr, want_wz = Wz != nullptr, want_q = Q != nullptr;

    bool live[R], inner[R];
    idx_t oVx[R], oC[R];
    T up[R], uc[R], vp[R], vc[R], dxc[R], dyc[R], zk[R], zk1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = j0 + r * TY + ty;
        live[r] = i < nx && j < ny;
        inner[r] = i >= 1 && i <= nx - 2 && j >= 1 && j <= ny - 2;
        oVx[r] = (idx_t)i + (idx_t)(nx + 1) * j;
        oC[r] = (idx_t)i + (idx_t)nx * j;
        up[r] = uc[r] = vp[r] = vc[r] = dxc[r] = dyc[r] = zk[r] = zk1[r] = (T)0;
        if (live[r] && ks < kt) {
            const T *x = Vx + oVx[r] + pVx * (ks - 1), *y = Vy + oC[r] + pVy * (ks - 1);
            up[r] = h * (x[0] + x[1]);
            vp[r] = h * (y[0] + y[nx]);
            const T x0 = x[pVx], x1 = x[pVx + 1], y0 = y[pVy], y1 = y[pVy + nx];
            uc[r] = h * (x0 + x1); dxc[r] = x1 - x0;
            vc[r] = h * (y0 + y1); dyc[r] = y1 - y0;
            zk[r] = Vz[oC[r] + pC * ks];
            zk1[r] = Vz[oC[r] + pC * (ks + 1)];
        }
    }
    // the ring cell this thread stages besides its own: wave 0 / 1 the row below / above the tile (u and w), wave 2 / 3 the column
    // left / right of it (v and w)
    const bool ring_u = ty < 2;
    const int ei = ring_u ? i : (int)blockIdx.x * 64 + (ty == 2 ? -1 : 64), ej = ring_u ? (ty == 0 ? j0 - 1 : j0 + TYR) : j0 + tx;
    const bool ring = STAGE && ty < 4 && (ring_u || tx < TYR) && ei >= 0 && ei < nx && ej >= 0 && ej < ny && ks < kt;
    const int ring_c = ring_u ? (ty == 0 ? 0 : TYR + 1) * SU + tx : NU + tx * SV + (ty == 2 ? 0 : 65);
    const int ring_w = NU + NV + (ring_u ? (ty == 0 ? 0 : TYR + 1) * SV + tx + 1 : (tx + 1) * SV + (ty == 2 ? 0 : 65));
    const idx_t eF = ring_u ? (idx_t)ei + (idx_t)(nx + 1) * ej : (idx_t)ei + (idx_t)nx * ej, eC = (idx_t)ei + (idx_t)nx * ej;
    const T *eV = ring_u ? Vx : Vy;
    const idx_t ePl = ring_u ? pVx : pVy;
    const int eStep = ring_u ? 1 : nx;
    T ec = (T)0, ez = (T)0, ez1 = (T)0;
    if (ring) {
        ec = h * (eV[eF + ePl * ks] + eV[eF + eStep + ePl * ks]);
        ez = Vz[eC + pC * ks];
        ez1 = Vz[eC + pC * (ks + 1)];
    }

    if (kb == 0 || ke == nz) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (live[r])
                for (int q = 0; q < 2; ++q) {
                    if (q == 0 ? kb != 0 : ke != nz) continue;
                    const idx_t c = oC[r] + pC * (q == 0 ? 0 : nz - 1);
                    if (want_wx) Wx[c] = (T)0;
                    if (want_wy) Wy[c] = (T)0;
                    if (want_wz) Wz[c] = (T)0;
                    if (want_q) Q[c] = (T)0;
                }
    }

    for (int k = ks; k < kt; ++k) {
        T un[R], vn[R], dxn[R], dyn[R], zk2[R], wc[R];
        const bool more = k + 1 < kt;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            un[r] = vn[r] = dxn[r] = dyn[r] = zk2[r] = (T)0;
            if (live[r]) {
                const T *x = Vx + oVx[r] + pVx * (k + 1), *y = Vy + oC[r] + pVy * (k + 1);
                const T x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[nx];
                un[r] = h * (x0 + x1); dxn[r] = x1 - x0;
                vn[r] = h * (y0 + y1); dyn[r] = y1 - y0;
                if (more) zk2[r] = Vz[oC[r] + pC * (k + 2)];
            }
            wc[r] = h * (zk[r] + zk1[r]);
        }
        T *buf = lds + (STAGE ? ((k - ks) & 1) * NB : 0);
        if (STAGE) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int jj = r * TY + ty;
                buf[(jj + 1) * SU + tx] = uc[r];
                buf[NU + jj * SV + tx + 1] = vc[r];
                buf[NU + NV + (jj + 1) * SV + tx + 1] = wc[r];
            }
            if (ring) {
                buf[ring_c] = ec;
                buf[ring_w] = h * (ez + ez1);
                if (more) {
                    ec = h * (eV[eF + ePl * (k + 1)] + eV[eF + eStep + ePl * (k + 1)]);
                    ez = ez1;
                    ez1 = Vz[eC + pC * (k + 2)];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int jj = r * TY + ty;
            T u_jm = 0, u_jp = 0, v_im = 0, v_ip = 0, w_im = 0, w_ip = 0, w_jm = 0, w_jp = 0;
            if (STAGE) {
                u_jm = buf[jj * SU + tx]; u_jp = buf[(jj + 2) * SU + tx];
                v_im = buf[NU + jj * SV + tx]; v_ip = buf[NU + jj * SV + tx + 2];
                const T *sw = buf + NU + NV + (jj + 1) * SV + tx + 1;
                w_im = sw[-1]; w_ip = sw[1]; w_jm = sw[-SV]; w_jp = sw[SV];
            } else if (inner[r] && live[r]) {
                const T *x = Vx + oVx[r] + pVx * k, *y = Vy + oC[r] + pVy * k, *z = Vz + oC[r] + pC * k;
                u_jm = h * (x[-(nx + 1)] + x[-(nx + 1) + 1]); u_jp = h * (x[nx + 1] + x[nx + 2]);
                v_im = h * (y[-1] + y[-1 + nx]); v_ip = h * (y[1] + y[1 + nx]);
                w_im = h * (z[-1] + z[-1 + pC]); w_ip = h * (z[1] + z[1 + pC]);
                w_jm = h * (z[-nx] + z[-nx + pC]); w_jp = h * (z[nx] + z[nx + pC]);
            }
            if (live[r]) {
                const idx_t c = oC[r] + pC * k;
                const bool in = inner[r];
                const T uy = h * DIV_Y(u_jp - u_jm), uz = h * DIV_Z(un[r] - up[r]);
                const T vx = h * DIV_X(v_ip - v_im), vz = h * DIV_Z(vn[r] - vp[r]);
                const T wx = h * DIV_X(w_ip - w_im), wy = h * DIV_Y(w_jp - w_jm);
                if (want_wx) Wx[c] = in ? wy - vz : (T)0;
                if (want_wy) Wy[c] = in ? uz - wx : (T)0;
                if (want_wz) Wz[c] = in ? vx - uy : (T)0;
                if (want_q) {
                    const T gxx = DIV_X(dxc[r]), gyy = DIV_Y(dyc[r]), gzz = DIV_Z(zk1[r] - zk[r]);
                    const T q = ((-h) * ((gxx * gxx + gyy * gyy) + gzz * gzz)) - ((uy * vx + uz * wx) + vz * wy);
                    Q[c] = in ? q : (T)0;
                }
            }
            up[r] = uc[r]; uc[r] = un[r]; vp[r] = vc[r]; vc[r] = vn[r]; dxc[r] = dxn[r]; dyc[r] = dyn[r];
            zk[r] = zk1[r]; zk1[r] = zk2[r];
        }
    }
}

template <class T>
struct Bufs { T *W[4], *V[3]; };

template <class T, int TY, int R, bool STAGE>
static void launch(const Bufs<T> &b, Geo<T> g, int nx, int ny, int nz, int kz)
{
    const dim3 blk(64, TY, 1), grd((nx + 63) / 64, (ny + TY * R - 1) / (TY * R), (nz + kz - 1) / kz);
    hipLaunchKernelGGL((k_vortex<T, TY, R, STAGE>), grd, blk, 0, 0, b.W[0], b.W[1], b.W[2], b.W[3], b.V[0], b.V[1], b.V[2], g, nx, ny, nz, kz);
}
template <class T>
static void launch_naive(const Bufs<T> &b, Geo<T> g, int nx, int ny, int nz)
{
    hipLaunchKernelGGL(k_naive<T>, dim3((nx + 63) / 64, (ny + 3) / 4, nz), dim3(64, 4, 1), 0, 0, b.W[0], b.W[1], b.W[2], b.W[3], b.V[0], b.V[1],
                       b.V[2], g, nx, ny, nz);
}

template <class T>
struct Variant { const char *name; void (*fn)(const Bufs<T> &, Geo<T>, int, int, int, int); int kz; };

template <class T>
static std::vector<Variant<T>> variants()
{
    std::vector<Variant<T>> v;
#define V_(TY, R, ST, KZ, NAME) v.push_back({NAME, launch<T, TY, R, ST>, KZ})
    V_(4, 1, true, 8, "staged 64x4  kz8 "); V_(4, 1, true, 16, "staged 64x4  kz16"); V_(4, 1, true, 32, "staged 64x4  kz32");
    V_(8, 1, true, 16, "staged 64x8  kz16"); V_(8, 1, true, 32, "staged 64x8  kz32");
    V_(8, 2, true, 16, "staged 64x16 r2 kz16"); V_(8, 2, true, 32, "staged 64x16 r2 kz32");
    V_(4, 4, true, 16, "staged 64x16 r4 kz16"); V_(4, 4, true, 32, "staged 64x16 r4 kz32");
    V_(4, 1, false, 8, "plain  64x4  kz8 "); V_(4, 1, false, 16, "plain  64x4  kz16"); V_(4, 1, false, 32, "plain  64x4  kz32");
    V_(8, 1, false, 16, "plain  64x8  kz16");
    V_(8, 2, false, 16, "plain  64x16 r2 kz16");
#undef V_
    return v;
}

template <class T>
static void alloc(Bufs<T> &b, int nx, int ny, int nz, bool fill)
{
    const size_t nV[3] = {(size_t)(nx + 1) * ny * nz, (size_t)nx * (ny + 1) * nz, (size_t)nx * ny * (nz + 1)};
    for (int q = 0; q < 3; ++q) {
        CK(hipMalloc(&b.V[q], nV[q] * sizeof(T)));
        if (fill) {
            std::vector<T> hbuf(nV[q]);
            unsigned long long s = 88172645463325252ull + q;
            for (auto &x : hbuf) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; x = (T)((double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
            CK(hipMemcpy(b.V[q], hbuf.data(), nV[q] * sizeof(T), hipMemcpyHostToDevice));
        } else
            CK(hipMemset(b.V[q], 0x3c, nV[q] * sizeof(T)));      // finite values of either type
    }
    for (int q = 0; q < 4; ++q) CK(hipMalloc(&b.W[q], (size_t)nx * ny * nz * sizeof(T)));
}
template <class T>
static void release(Bufs<T> &b)
{
    for (int q = 0; q < 3; ++q) CK(hipFree(b.V[q]));
    for (int q = 0; q < 4; ++q) CK(hipFree(b.W[q]));
}

template <class T>
static int check(const char *tname)
{
    const int nx = 131, ny = 66, nz = 37;
    const size_t n = (size_t)nx * ny * nz;
    Bufs<T> b;
    alloc(b, nx, ny, nz, true);
    const Geo<T> g = {(T)(1.0 / 0.37), (T)(1.0 / 0.11), (T)(1.0 / 0.23)};
    std::vector<T> ref(4 * n), got(4 * n);
    launch_naive(b, g, nx, ny, nz);
    CK(hipDeviceSynchronize());
    for (int q = 0; q < 4; ++q) CK(hipMemcpy(ref.data() + q * n, b.W[q], n * sizeof(T), hipMemcpyDeviceToHost));
    int bad = 0;
    for (auto &v : variants<T>()) {
        for (int q = 0; q < 4; ++q) CK(hipMemset(b.W[q], 0xff, n * sizeof(T)));
        v.fn(b, g, nx, ny, nz, v.kz);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        for (int q = 0; q < 4; ++q) CK(hipMemcpy(got.data() + q * n, b.W[q], n * sizeof(T), hipMemcpyDeviceToHost));
        const bool same = std::memcmp(ref.data(), got.data(), 4 * n * sizeof(T)) == 0;
        if (!same) { ++bad; std::printf("MISMATCH %s %s\n", tname, v.name); }
    }
    release(b);
    std::printf("check %s 131x66x37: %d of %zu variants differ from the one-thread-per-cell kernel\n", tname, bad, variants<T>().size());
    return bad;
}

template <class T>
static void time_grid(const char *tname, int nx, int ny, int nz)
{
    Bufs<T> b;
    alloc(b, nx, ny, nz, false);
    const Geo<T> g = {(T)nx, (T)ny, (T)nz};
    const double bytes = 7.0 * sizeof(T) * (double)nx * ny * nz;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::printf("%s %dx%dx%d  (nominal %.0f MB = 3 reads + 4 writes per cell)\n", tname, nx, ny, nz, bytes / 1e6);
    auto run = [&](const char *name, auto &&fn) {
        float best = 1e30f;
        for (int it = 0; it < 13; ++it) {
            CK(hipEventRecord(e0, 0));
            fn();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (it >= 3 && ms < best) best = ms;
        }
        CK(hipGetLastError());
        std::printf("  %-22s %9.4f ms  %8.1f GB/s nominal\n", name, best, bytes / best / 1e6);
        std::fflush(stdout);
    };
    for (auto &v : variants<T>()) run(v.name, [&] { v.fn(b, g, nx, ny, nz, v.kz); });
    run("naive (1 thread/cell)", [&] { launch_naive(b, g, nx, ny, nz); });
    release(b);
}

int main()
{
    if (check<double>("fp64") + check<float>("fp32")) return 1;
    time_grid<double>("fp64", 512, 512, 512);
    time_grid<float>("fp32", 512, 512, 512);
    time_grid<double>("fp64", 255, 153, 153);
    time_grid<float>("fp32", 255, 153, 153);
    return 0;
}
