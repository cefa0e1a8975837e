// ns3d_solid.hip — obstacles from triangle meshes (include/ns3d.h has the definitions): ns3d_voxelize turns a closed triangle surface
// into the four staggered masks of set_cylinder!'s thread range, ns3d_set_solid stores what k_set_cylinder stores with the flags read
// from such a mask, ns3d_solid_momentum sums what the next ns3d_set_solid removes.  Moving bodies: ns3d_set_solid_moving stores a rigid
// body's velocity where ns3d_set_solid stores zero, ns3d_solid_momentum_moving sums what it removes, ns3d_mesh_transform poses a mesh.
//
// Compiled ONCE, with -ffp-contract=off (build.py), like ns3d_tracers.hip: every decision of the voxelizer is a stated fp64
// comparison, so STRICT, NS3D_IEEE_DIV and FAST contexts return the same bytes and there is no arithmetic mode to select.
//
// Voxelizer, two launches behind a memset of the bit planes:
//   k_vox_scatter   one wave per triangle, its lanes over the rows (j, k) of the triangle's yz bounding box in each of the three row
//                   families; a covered row XORs ONE bit, at i0, into the row's packed bit plane (atomicXor on a 32-bit word: XOR
//                   commutes, arrival order decides nothing).  Four planes (C, Vx, Vy, Vz) of (ny+1)(nz+1) rows × W words.
//   k_vox_prefix    one wave per row: lane l takes word l of each plane, forms the word's inclusive prefix XOR by shifts and takes the
//                   carry of the words before it from a ballot of the words' parities; the four prefix words go through LDS and the
//                   wave stores the row's mask bytes, 64 consecutive bytes per store.
#include <cmath>

#include "ns3d_internal.h"

#pragma clang fp contract(off)

namespace ns3d_solid {

typedef long long idx_t;

// side(p, q, r) on the yz-projections: the sign of E at r + (ε, ε²), formed from the lexicographically ordered end points so that
// both triangles of a shared edge evaluate the same expression
__device__ __forceinline__ int side(double py, double pz, double qy, double qz, double ry, double rz)
{
    const bool swap = qy < py || (qy == py && qz < pz);
    const double ay = swap ? qy : py, az = swap ? qz : pz, by = swap ? py : qy, bz = swap ? pz : qz;
    const double dy = by - ay, dz = bz - az;
    const double E = dy * (rz - az) - dz * (ry - ay);
    int s;
    if (E > 0.0) s = 1;
    else if (E < 0.0) s = -1;
    else s = dz > 0.0 ? -1 : dz < 0.0 ? 1 : dy > 0.0 ? 1 : 0;
    return swap ? -s : s;
}

// i0 of a sample family with x positions (i + ox) + s, 0 ≤ i < ext
__device__ __forceinline__ int flip_index(double xs, double x0, int ext)
{
    const double t = xs - x0;
    return t <= 0.0 ? 0 : t >= (double)ext ? ext : (int)ceil(t);
}

// row index range [lo, hi] of a family whose rows sit at (double)(j + o) + s, 0 ≤ j ≤ jmax, around [vmin, vmax]: rounded outward by
// one row (the cover test decides), clipped to the rank's rows; empty when lo > hi.  vmin, vmax are finite.
__device__ __forceinline__ void row_range(double vmin, double vmax, int o, double s, int jmax, int &lo, int &hi)
{
    const double base = (double)o + s;
    double a = floor(vmin - base) - 1.0, b = ceil(vmax - base) + 1.0;
    const double top = (double)jmax;
    a = a > 0.0 ? a : 0.0;
    a = a < top + 1.0 ? a : top + 1.0;
    b = b < top ? b : top;
    b = b > -1.0 ? b : -1.0;
    lo = (int)a;
    hi = (int)b;
}

struct VoxGeom {
    int nx, ny, nz, W;          // W: 32-bit words per row of a plane, ceil((nx+2)/32)
    int ox, oy, oz;
    idx_t plane;                // words per plane: (ny+1)(nz+1)·W
};

__global__ __launch_bounds__(256) void k_vox_scatter(unsigned *__restrict__ planes, const double *__restrict__ tri, idx_t n_tri,
                                                     const VoxGeom g)
{
    const int lane = threadIdx.x & 63;
    const idx_t t = (idx_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n_tri) return;
    const double *p = tri + 9 * t;
    const double ax = p[0], ay = p[1], az = p[2], bx = p[3], by = p[4], bz = p[5], cx = p[6], cy = p[7], cz = p[8];
    if (!(isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) && isfinite(cy) &&
          isfinite(cz)))
        return;
    double miny = ay < by ? ay : by, maxy = ay > by ? ay : by, minz = az < bz ? az : bz, maxz = az > bz ? az : bz;
    miny = cy < miny ? cy : miny; maxy = cy > maxy ? cy : maxy;
    minz = cz < minz ? cz : minz; maxz = cz > maxz ? cz : maxz;
    const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const double n_x = uy * vz - uz * vy, n_y = uz * vx - ux * vz, n_z = ux * vy - uy * vx;
    if (n_x == 0.0) return;                                     // ignored for every row
    const int nx = g.nx, ny = g.ny, nz = g.nz;
    const double xc = (double)g.ox + 0.5, xv = (double)g.ox;    // x of sample 0: cell-centred / on the x faces
#pragma unroll 1
    for (int f = 0; f < 3; ++f) {                               // (j+.5, k+.5): C and Vx | (j, k+.5): Vy | (j+.5, k): Vz
        const double sy = f == 1 ? 0.0 : 0.5, sz = f == 2 ? 0.0 : 0.5;
        const int jmax = f == 1 ? ny : ny - 1, kmax = f == 2 ? nz : nz - 1;
        int j0, j1, k0, k1;
        row_range(miny, maxy, g.oy, sy, jmax, j0, j1);
        row_range(minz, maxz, g.oz, sz, kmax, k0, k1);
        if (j0 > j1 || k0 > k1) continue;
        const idx_t nj = j1 - j0 + 1, total = nj * (idx_t)(k1 - k0 + 1);
        unsigned *pl = planes + (f == 0 ? 0 : f + 1) * g.plane;
        for (idx_t q = lane; q < total; q += 64) {
            const int j = j0 + (int)(q % nj), k = k0 + (int)(q / nj);
            const double y = (double)((idx_t)j + g.oy) + sy, z = (double)((idx_t)k + g.oz) + sz;
            if (!(miny <= y && y <= maxy && minz <= z && z <= maxz)) continue;
            const int s1 = side(ay, az, by, bz, y, z);
            if (s1 == 0) continue;
            if (side(by, bz, cy, cz, y, z) != s1 || side(cy, cz, ay, az, y, z) != s1) continue;
            const double xs = ax - (n_y * (y - ay) + n_z * (z - az)) / n_x;
            if (!isfinite(xs)) continue;
            unsigned *row = pl + ((idx_t)j + (idx_t)(ny + 1) * k) * g.W;
            const int i0 = flip_index(xs, xc, nx);              // 0 ≤ i0 ≤ nx < 32·W
            atomicXor(row + (i0 >> 5), 1u << (i0 & 31));
            if (f == 0) {                                       // the same cover test serves Vx: plane 1, s = 0, ext = nx+1
                const int i1 = flip_index(xs, xv, nx + 1);      // 0 ≤ i1 ≤ nx+1 < 32·W
                atomicXor(row + g.plane + (i1 >> 5), 1u << (i1 & 31));
            }
        }
    }
}

__device__ __forceinline__ unsigned prefix_xor32(unsigned w)
{
    w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
    return w;
}

__global__ __launch_bounds__(256) void k_vox_prefix(unsigned char *__restrict__ mask, const unsigned *__restrict__ planes, const VoxGeom g,
                                                    idx_t rows)
{
    __shared__ unsigned sw[4][4][64];                           // [wave][plane][word of the chunk]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nx = g.nx, ny = g.ny, nz = g.nz;
    for (idx_t rb = (idx_t)blockIdx.x * 4; rb < rows; rb += (idx_t)gridDim.x * 4) {      // uniform per workgroup: barriers inside
        const idx_t r = rb + wave;
        const bool live = r < rows;
        const int j = (int)(r % (ny + 1)), k = (int)(r / (ny + 1));
        // bits at invalid points are 0: C i<nx, j<ny, k<nz | Vx j<ny, k<nz | Vy i<nx, k<nz | Vz i<nx, j<ny
        const bool vj = j < ny, vk = k < nz;
        const bool rowok[4] = {vj && vk, vj && vk, vk, vj};
        unsigned carry[4] = {0u, 0u, 0u, 0u};
        for (int c0 = 0; c0 < g.W; c0 += 64) {                  // 64 words = 2048 samples per pass
            const int w = c0 + lane;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned v = live && w < g.W ? planes[q * g.plane + r * g.W + w] : 0u;
                unsigned pfx = prefix_xor32(v);
                const unsigned long long odd = __ballot((pfx >> 31) != 0u);
                const unsigned before = (unsigned)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
                if ((before ^ carry[q]) != 0u) pfx = ~pfx;
                carry[q] ^= (unsigned)__popcll(odd) & 1u;
                sw[wave][q][lane] = rowok[q] ? pfx : 0u;
            }
            __syncthreads();
            const int xend = live ? min(nx + 1, 32 * (c0 + 64)) : 0;
            for (int i = 32 * c0 + lane; i < xend; i += 64) {
                const int wl = (i >> 5) - c0, b = i & 31;
                unsigned m = ((sw[wave][1][wl] >> b) & 1u) << 1;
                if (i < nx) m |= ((sw[wave][0][wl] >> b) & 1u) | (((sw[wave][2][wl] >> b) & 1u) << 2) | (((sw[wave][3][wl] >> b) & 1u) << 3);
                mask[r * (idx_t)(nx + 1) + i] = (unsigned char)m;
            }
            __syncthreads();
        }
    }
}

size_t voxelize_scratch_bytes(int nx, int ny, int nz)
{
    const size_t W = ((size_t)nx + 2 + 31) / 32;
    return 4 * (size_t)(ny + 1) * (size_t)(nz + 1) * W * sizeof(unsigned);
}

hipError_t voxelize(hipStream_t s, unsigned char *mask, const double *tri, long long n_tri, int nx, int ny, int nz, const int *origin,
                    void *scratch)
{
    VoxGeom g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.W = (nx + 2 + 31) / 32;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    const idx_t rows = (idx_t)(ny + 1) * (nz + 1);
    g.plane = rows * g.W;
    hipError_t e = hipMemsetAsync(scratch, 0, voxelize_scratch_bytes(nx, ny, nz), s);
    if (e != hipSuccess) return e;
    if (n_tri > 0) {
        hipLaunchKernelGGL(k_vox_scatter, dim3((unsigned)((n_tri + 3) / 4)), dim3(256), 0, s, (unsigned *)scratch, tri, (idx_t)n_tri, g);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const idx_t blocks = (rows + 3) / 4;
    hipLaunchKernelGGL(k_vox_prefix, dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, s, mask,
                       (const unsigned *)scratch, g, rows);
    return hipGetLastError();
}

// ---- ns3d_set_solid: the mask is read as one flat array of N = (nx+1)(ny+1)(nz+1) bytes, 16 per thread — one 16-byte load where the
// thread's chunk is whole and the pointer allows it, byte loads inside [0, N) otherwise (the mask needs no alignment, and nothing
// outside it is read).  Nearly every chunk is all zeros and the thread leaves; a set byte is decoded into (i, j, k) and stored where
// k_set_cylinder stores.  Bits at invalid points are tested against the extents like everything else: no address outside the arrays.
template <class T>
__global__ __launch_bounds__(256) void k_set_solid(T *__restrict__ C, T *__restrict__ Vx, T *__restrict__ Vy, T *__restrict__ Vz,
                                                   const unsigned char *__restrict__ mask, int nx, int ny, int nz, idx_t N, int lead)
{
    // chunk c covers the bytes [16c − lead, 16c − lead + 16) ∩ [0, N), lead = address mod 16: whole chunks are 16-byte aligned
    const idx_t c = (idx_t)blockIdx.x * 256 + threadIdx.x;
    const idx_t b0 = 16 * c - lead;
    if (b0 >= N) return;
    unsigned long long lo = 0ull, hi = 0ull;                    // bytes 0-7 and 8-15 of the chunk, the first in the low bits
    if (b0 >= 0 && b0 + 16 <= N) {
        const uint4 v = *reinterpret_cast<const uint4 *>(mask + b0);
        lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    } else {
        for (int q = 0; q < 8; ++q) {
            const idx_t b = b0 + q;
            if (b >= 0 && b < N) lo |= (unsigned long long)mask[b] << (8 * q);
            if (b + 8 >= 0 && b + 8 < N) hi |= (unsigned long long)mask[b + 8] << (8 * q);
        }
    }
    if ((lo | hi) == 0ull) return;
    const idx_t row = nx + 1, plane = row * (ny + 1);
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
        const unsigned m = (unsigned)((q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8))) & 0xFFull);
        if (!m) continue;
        const idx_t b = b0 + q;
        const int k = (int)(b / plane);
        const idx_t rem = b - (idx_t)k * plane;
        const int j = (int)(rem / row), i = (int)(rem - (idx_t)j * row);
        const bool ci = i < nx, cj = j < ny, ck = k < nz;
        if ((m & 1u) && C && ci && cj && ck) C[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)ny * k)] = (T)1.0;
        if ((m & 2u) && cj && ck) Vx[(idx_t)i + (idx_t)(nx + 1) * ((idx_t)j + (idx_t)ny * k)] = (T)0.0;
        if ((m & 4u) && ci && ck) Vy[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)(ny + 1) * k)] = (T)0.0;
        if ((m & 8u) && ci && cj) Vz[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)ny * k)] = (T)0.0;
    }
}

template <class T>
hipError_t set_solid(hipStream_t s, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, int nx, int ny, int nz)
{
    const idx_t N = (idx_t)(nx + 1) * (ny + 1) * (nz + 1);
    const int lead = (int)((size_t)mask & 15);
    const idx_t chunks = (N + lead + 15) / 16;
    hipLaunchKernelGGL(k_set_solid<T>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, C, Vx, Vy, Vz, mask, nx, ny, nz, N, lead);
    return hipGetLastError();
}

// ---- ns3d_solid_momentum: k_diag's scheme for the three masked sums and counts.  Thread (i, j) of the (nx+1)×(ny+1) column range
// marches kz planes; fp64 sums in a FIXED order — per thread down its planes, wave64 butterfly, one LDS slot per wave, the four waves
// in order, per-workgroup partials, k_mom_final over the partials.  No float atomics: two calls give the same bits.
#define NS3D_MOM_SLOTS 6        /* 0-2 sums, 3-5 counts */
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long mom_combine(int slot, unsigned long long a, unsigned long long b)
{
    if (slot < 3) return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    return a + b;
}
struct MomGeom {
    int nx, ny, nz, kz;
    int own[3][2][2];           // [dimension][s][lo, hi): owned 0-based index range of an extent n+s, as ns3d_diagnostics
    unsigned nblocks;
};
template <class T>
__global__ __launch_bounds__(256) void k_mom(const T *__restrict__ Vx, const T *__restrict__ Vy, const T *__restrict__ Vz,
                                             const unsigned char *__restrict__ mask, const MomGeom a, unsigned long long *__restrict__ part)
{
    typedef unsigned long long u64;
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    const int kb = blockIdx.z * a.kz, ke = min(kb + a.kz, nz + 1);
    double s[3] = {0.0, 0.0, 0.0};
    u64 n[3] = {0, 0, 0};
    if (i <= nx && j <= ny) {
        const bool cx = i < nx, cy = j < ny;
        const bool ox0 = i >= a.own[0][0][0] && i < a.own[0][0][1], ox1 = i >= a.own[0][1][0] && i < a.own[0][1][1];
        const bool oy0 = j >= a.own[1][0][0] && j < a.own[1][0][1], oy1 = j >= a.own[1][1][0] && j < a.own[1][1][1];
        const idx_t pM = (idx_t)(nx + 1) * (ny + 1), oM = (idx_t)i + (idx_t)(nx + 1) * j;
        const idx_t pVx = (idx_t)(nx + 1) * ny, pVy = (idx_t)nx * (ny + 1), pC = (idx_t)nx * ny;
        const idx_t oVx = (idx_t)i + (idx_t)(nx + 1) * j, oVy = (idx_t)i + (idx_t)nx * j;
        for (int k = kb; k < ke; ++k) {
            const unsigned m = mask[oM + pM * k];
            if (!m) continue;
            const bool oz0 = k >= a.own[2][0][0] && k < a.own[2][0][1], oz1 = k >= a.own[2][1][0] && k < a.own[2][1][1];
            if ((m & 2u) && cy && k < nz && ox1 && oy0 && oz0) { s[0] += (double)Vx[oVx + pVx * k]; ++n[0]; }
            if ((m & 4u) && cx && k < nz && ox0 && oy1 && oz0) { s[1] += (double)Vy[oVy + pVy * k]; ++n[1]; }
            if ((m & 8u) && cx && cy && ox0 && oy0 && oz1) { s[2] += (double)Vz[oVy + pC * k]; ++n[2]; }
        }
    }
    __shared__ u64 wpart[NS3D_MOM_SLOTS][4];
    const int tid = threadIdx.x + 64 * threadIdx.y, w = tid >> 6;
    u64 v[NS3D_MOM_SLOTS];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        v[q] = (u64)__double_as_longlong(wave_sum_f64(s[q]));
        v[3 + q] = wave_sum_u64(n[q]);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NS3D_MOM_SLOTS; ++q) wpart[q][w] = v[q];
    }
    __syncthreads();
    if (tid < NS3D_MOM_SLOTS) {
        u64 r = wpart[tid][0];
        for (int q = 1; q < 4; ++q) r = mom_combine(tid, r, wpart[tid][q]);
        const unsigned bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        part[(size_t)tid * a.nblocks + bid] = r;
    }
}
// one workgroup per slot: thread t combines partials t, t+256, … in order, then the butterfly, then the four waves in order
__global__ __launch_bounds__(256) void k_mom_final(const unsigned long long *__restrict__ part, unsigned nblocks,
                                                   unsigned long long *__restrict__ result)
{
    typedef unsigned long long u64;
    const int slot = blockIdx.x, tid = threadIdx.x;
    const u64 *p = part + (size_t)slot * nblocks;
    u64 r = slot < 3 ? (u64)__double_as_longlong(0.0) : 0ull;
    for (unsigned q = tid; q < nblocks; q += 256) r = mom_combine(slot, r, p[q]);
    if (slot < 3) r = (u64)__double_as_longlong(wave_sum_f64(__longlong_as_double((long long)r)));
    else r = wave_sum_u64(r);
    __shared__ u64 wv[4];
    if ((tid & 63) == 0) wv[tid >> 6] = r;
    __syncthreads();
    if (tid == 0) {
        u64 t = wv[0];
        for (int q = 1; q < 4; ++q) t = mom_combine(slot, t, wv[q]);
        result[slot] = t;
    }
}

size_t momentum_scratch_bytes(int nx, int ny, int nz)
{
    return (size_t)NS3D_MOM_SLOTS * ns3d_diag_geometry(nx, ny, nz, nullptr) * sizeof(unsigned long long);
}

template <class T>
hipError_t momentum(hipStream_t s, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny, int nz,
                    const int *seam_lo, const int *seam_hi, void *scratch, unsigned long long *result)
{
    MomGeom a;
    a.nx = nx; a.ny = ny; a.nz = nz;
    const int n[3] = {nx, ny, nz};
    for (int d = 0; d < 3; ++d)
        for (int st = 0; st < 2; ++st) {
            a.own[d][st][0] = seam_lo[d] ? 1 + st : 0;
            a.own[d][st][1] = seam_hi[d] ? n[d] + st - 1 : n[d] + st;
        }
    a.nblocks = ns3d_diag_geometry(nx, ny, nz, &a.kz);
    const dim3 blk(64, 4, 1);
    const dim3 grd((unsigned)((nx + 1 + 63) / 64), (unsigned)((ny + 1 + 3) / 4), (unsigned)((nz + 1 + a.kz - 1) / a.kz));
    hipLaunchKernelGGL(k_mom<T>, grd, blk, 0, s, Vx, Vy, Vz, mask, a, (unsigned long long *)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mom_final, dim3(NS3D_MOM_SLOTS), dim3(256), 0, s, (const unsigned long long *)scratch, a.nblocks, result);
    return hipGetLastError();
}

// ---- moving bodies: ns3d_set_solid_moving / ns3d_solid_momentum_moving / ns3d_mesh_transform.  The rigid-body velocity of a node is
// the header's statement, operation for operation, in fp64 and never contracted; q picks the component and with it the node's stagger.
__device__ __forceinline__ double body_velocity(int q, const Motion &m, int i, int j, int k)
{
    const double X = (double)((idx_t)i + m.o[0]) + (q == 0 ? 0.0 : 0.5);
    const double Y = (double)((idx_t)j + m.o[1]) + (q == 1 ? 0.0 : 0.5);
    const double Z = (double)((idx_t)k + m.o[2]) + (q == 2 ? 0.0 : 0.5);
    const double rx = (X - m.c[0]) * m.d[0], ry = (Y - m.c[1]) * m.d[1], rz = (Z - m.c[2]) * m.d[2];
    if (q == 0) return m.U[0] + (m.w[1] * rz - m.w[2] * ry);
    if (q == 1) return m.U[1] + (m.w[2] * rx - m.w[0] * rz);
    return m.U[2] + (m.w[0] * ry - m.w[1] * rx);
}

// k_set_solid's shape — 16 mask bytes per thread, one 16-byte load where the chunk is whole and aligned, out at once on an all-zero
// chunk — with the body's velocity formed for the set bits only: the cost stays the read of the mask
template <class T>
__global__ __launch_bounds__(256) void k_set_solid_moving(T *__restrict__ C, T *__restrict__ Vx, T *__restrict__ Vy, T *__restrict__ Vz,
                                                          const unsigned char *__restrict__ mask, const Motion mo, int nx, int ny, int nz,
                                                          idx_t N, int lead)
{
    const idx_t c = (idx_t)blockIdx.x * 256 + threadIdx.x;
    const idx_t b0 = 16 * c - lead;
    if (b0 >= N) return;
    unsigned long long lo = 0ull, hi = 0ull;
    if (b0 >= 0 && b0 + 16 <= N) {
        const uint4 v = *reinterpret_cast<const uint4 *>(mask + b0);
        lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    } else {
        for (int q = 0; q < 8; ++q) {
            const idx_t b = b0 + q;
            if (b >= 0 && b < N) lo |= (unsigned long long)mask[b] << (8 * q);
            if (b + 8 >= 0 && b + 8 < N) hi |= (unsigned long long)mask[b + 8] << (8 * q);
        }
    }
    if ((lo | hi) == 0ull) return;
    const idx_t row = nx + 1, plane = row * (ny + 1);
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
        const unsigned m = (unsigned)((q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8))) & 0xFFull);
        if (!m) continue;
        const idx_t b = b0 + q;
        const int k = (int)(b / plane);
        const idx_t rem = b - (idx_t)k * plane;
        const int j = (int)(rem / row), i = (int)(rem - (idx_t)j * row);
        const bool ci = i < nx, cj = j < ny, ck = k < nz;
        if ((m & 1u) && C && ci && cj && ck) C[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)ny * k)] = (T)1.0;
        if ((m & 2u) && cj && ck) Vx[(idx_t)i + (idx_t)(nx + 1) * ((idx_t)j + (idx_t)ny * k)] = (T)body_velocity(0, mo, i, j, k);
        if ((m & 4u) && ci && ck) Vy[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)(ny + 1) * k)] = (T)body_velocity(1, mo, i, j, k);
        if ((m & 8u) && ci && cj) Vz[(idx_t)i + (idx_t)nx * ((idx_t)j + (idx_t)ny * k)] = (T)body_velocity(2, mo, i, j, k);
    }
}

template <class T>
hipError_t set_solid_moving(hipStream_t s, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, const Motion &mo, int nx, int ny, int nz)
{
    const idx_t N = (idx_t)(nx + 1) * (ny + 1) * (nz + 1);
    const int lead = (int)((size_t)mask & 15);
    const idx_t chunks = (N + lead + 15) / 16;
    hipLaunchKernelGGL(k_set_solid_moving<T>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, C, Vx, Vy, Vz, mask, mo, nx, ny, nz, N,
                       lead);
    return hipGetLastError();
}

// k_mom with the subtraction: each term is (double)V − (double)(T)vb, what the next ns3d_set_solid_moving removes from that node; the
// ranges, the counts, the order of the sums and the partials' layout are k_mom's, and k_mom_final finishes both
template <class T>
__global__ __launch_bounds__(256) void k_mom_moving(const T *__restrict__ Vx, const T *__restrict__ Vy, const T *__restrict__ Vz,
                                                    const unsigned char *__restrict__ mask, const MomGeom a, const Motion mo,
                                                    unsigned long long *__restrict__ part)
{
    typedef unsigned long long u64;
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    const int kb = blockIdx.z * a.kz, ke = min(kb + a.kz, nz + 1);
    double s[3] = {0.0, 0.0, 0.0};
    u64 n[3] = {0, 0, 0};
    if (i <= nx && j <= ny) {
        const bool cx = i < nx, cy = j < ny;
        const bool ox0 = i >= a.own[0][0][0] && i < a.own[0][0][1], ox1 = i >= a.own[0][1][0] && i < a.own[0][1][1];
        const bool oy0 = j >= a.own[1][0][0] && j < a.own[1][0][1], oy1 = j >= a.own[1][1][0] && j < a.own[1][1][1];
        const idx_t pM = (idx_t)(nx + 1) * (ny + 1), oM = (idx_t)i + (idx_t)(nx + 1) * j;
        const idx_t pVx = (idx_t)(nx + 1) * ny, pVy = (idx_t)nx * (ny + 1), pC = (idx_t)nx * ny;
        const idx_t oVx = (idx_t)i + (idx_t)(nx + 1) * j, oVy = (idx_t)i + (idx_t)nx * j;
        for (int k = kb; k < ke; ++k) {
            const unsigned m = mask[oM + pM * k];
            if (!m) continue;
            const bool oz0 = k >= a.own[2][0][0] && k < a.own[2][0][1], oz1 = k >= a.own[2][1][0] && k < a.own[2][1][1];
            if ((m & 2u) && cy && k < nz && ox1 && oy0 && oz0) {
                s[0] += (double)Vx[oVx + pVx * k] - (double)(T)body_velocity(0, mo, i, j, k); ++n[0];
            }
            if ((m & 4u) && cx && k < nz && ox0 && oy1 && oz0) {
                s[1] += (double)Vy[oVy + pVy * k] - (double)(T)body_velocity(1, mo, i, j, k); ++n[1];
            }
            if ((m & 8u) && cx && cy && ox0 && oy0 && oz1) {
                s[2] += (double)Vz[oVy + pC * k] - (double)(T)body_velocity(2, mo, i, j, k); ++n[2];
            }
        }
    }
    __shared__ u64 wpart[NS3D_MOM_SLOTS][4];
    const int tid = threadIdx.x + 64 * threadIdx.y, w = tid >> 6;
    u64 v[NS3D_MOM_SLOTS];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        v[q] = (u64)__double_as_longlong(wave_sum_f64(s[q]));
        v[3 + q] = wave_sum_u64(n[q]);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NS3D_MOM_SLOTS; ++q) wpart[q][w] = v[q];
    }
    __syncthreads();
    if (tid < NS3D_MOM_SLOTS) {
        u64 r = wpart[tid][0];
        for (int q = 1; q < 4; ++q) r = mom_combine(tid, r, wpart[tid][q]);
        const unsigned bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        part[(size_t)tid * a.nblocks + bid] = r;
    }
}

template <class T>
hipError_t momentum_moving(hipStream_t s, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, const Motion &mo, int nx, int ny,
                           int nz, const int *seam_lo, const int *seam_hi, void *scratch, unsigned long long *result)
{
    MomGeom a;
    a.nx = nx; a.ny = ny; a.nz = nz;
    const int n[3] = {nx, ny, nz};
    for (int d = 0; d < 3; ++d)
        for (int st = 0; st < 2; ++st) {
            a.own[d][st][0] = seam_lo[d] ? 1 + st : 0;
            a.own[d][st][1] = seam_hi[d] ? n[d] + st - 1 : n[d] + st;
        }
    a.nblocks = ns3d_diag_geometry(nx, ny, nz, &a.kz);
    const dim3 blk(64, 4, 1);
    const dim3 grd((unsigned)((nx + 1 + 63) / 64), (unsigned)((ny + 1 + 3) / 4), (unsigned)((nz + 1 + a.kz - 1) / a.kz));
    hipLaunchKernelGGL(k_mom_moving<T>, grd, blk, 0, s, Vx, Vy, Vz, mask, a, mo, (unsigned long long *)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mom_final, dim3(NS3D_MOM_SLOTS), dim3(256), 0, s, (const unsigned long long *)scratch, a.nblocks, result);
    return hipGetLastError();
}

// one thread per vertex: its three coordinates are read before any is stored, so out == tri is in order
struct Pose {
    double R[9], pivot[3], shift[3], d[3];
};
__global__ __launch_bounds__(256) void k_mesh_transform(double *out, const double *tri, idx_t n_vert, const Pose p)
{
    const idx_t v = (idx_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vert) return;
    const double qx = (tri[3 * v] - p.pivot[0]) * p.d[0], qy = (tri[3 * v + 1] - p.pivot[1]) * p.d[1],
                 qz = (tri[3 * v + 2] - p.pivot[2]) * p.d[2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[3 * v + a] = (p.pivot[a] + p.shift[a]) + ((p.R[3 * a] * qx + p.R[3 * a + 1] * qy) + p.R[3 * a + 2] * qz) / p.d[a];
}

hipError_t mesh_transform(hipStream_t s, double *out, const double *tri, long long n_tri, const double *R, const double *pivot,
                          const double *shift, const double *spacing)
{
    Pose p;
    for (int q = 0; q < 9; ++q) p.R[q] = R[q];
    for (int q = 0; q < 3; ++q) { p.pivot[q] = pivot[q]; p.shift[q] = shift[q]; p.d[q] = spacing[q]; }
    const idx_t n_vert = 3 * (idx_t)n_tri;
    hipLaunchKernelGGL(k_mesh_transform, dim3((unsigned)((n_vert + 255) / 256)), dim3(256), 0, s, out, tri, n_vert, p);
    return hipGetLastError();
}

#define INST(T)                                                                                                              \
    template hipError_t set_solid<T>(hipStream_t, T *, T *, T *, T *, const unsigned char *, int, int, int);                 \
    template hipError_t momentum<T>(hipStream_t, const T *, const T *, const T *, const unsigned char *, int, int, int,      \
                                    const int *, const int *, void *, unsigned long long *);                                 \
    template hipError_t set_solid_moving<T>(hipStream_t, T *, T *, T *, T *, const unsigned char *, const Motion &, int, int, int); \
    template hipError_t momentum_moving<T>(hipStream_t, const T *, const T *, const T *, const unsigned char *, const Motion &, int, int, \
                                           int, const int *, const int *, void *, unsigned long long *);
INST(double)
INST(float)
#undef INST

} // namespace ns3d_solid
