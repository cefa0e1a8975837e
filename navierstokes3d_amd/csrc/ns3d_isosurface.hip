// ns3d_isosurface.hip — ns3d_isosurface (include/ns3d.h has the definition): the triangles of the level set A = iso by marching
// tetrahedra on the Kuhn decomposition, compacted on the device into one ordered list.
//
// Compiled ONCE, with -ffp-contract=off (build.py), like ns3d_tracers.hip and for the same reason: STRICT, NS3D_IEEE_DIV and FAST
// contexts return the same bits, so there is nothing for an arithmetic mode to select.  The pragma below is kept for a build whose
// flags are changed.
//
// Shape: three phases, all with ordinary vector stores and without atomics, so that a triangle's position is a function of the input.
//   count  k_iso_count: one wave per row segment of 64 consecutive cubes in x, NS3D_ISO_ROWS (j) rows per workgroup, marching
//          NS3D_ISO_KZ planes in z so that a plane's four node values per lane become the next cube's lower face.  A lane loads its own
//          node column of rows j and j+1 and takes its +x neighbour's from the next lane (lane 63 loads it), forms the 8-bit inside
//          mask and looks the triangle count up in a 256-entry table — only where the mask is neither 0 nor 255, which a ballot
//          settles for the whole wave on most of a real field.  One uint32 per (segment, j, k).
//   scan   exclusive 64-bit scan of the segment counts in linear (segment, j, k) order: per-block sums (NS3D_ISO_SCAN_BLOCK segments per
//          workgroup), a scan of the sums by one wave in chunks of 64 with a carry, then the add.  The total is the read-back.
//   emit   k_iso_emit: the tiling of the count.  A lane recomputes its mask from A, takes its offset from the segment's scanned base
//          plus the wave's exclusive prefix of the per-cube counts, and writes its triangles while their index is below cap; B's eight
//          corners are loaded only by lanes that emit.
// The wave sum and prefix are four ballots of the count's bits (a cube has at most 12 triangles) and population counts below the
// lane, instead of six dependent cross-lane steps.
#include <cmath>

#include "ns3d_internal.h"

#pragma clang fp contract(off)

namespace ns3d_iso {

typedef long long idx_t;

// corner (di + 2 dj + 4 dk) of vertex n of tetrahedron t: the axis orders xyz, xzy, yxz, yzx, zxy, zyx; v0 = 0, v1 = e1, v2 = e1 + e2, v3 = 7
__host__ __device__ constexpr int tet_corner(int t, int n)
{
    const int e1 = t < 2 ? 1 : t < 4 ? 2 : 4;
    const int e2 = t == 0 ? 2 : t == 1 ? 4 : t == 2 ? 1 : t == 3 ? 4 : t == 4 ? 1 : 2;
    return n == 0 ? 0 : n == 1 ? e1 : n == 2 ? (e1 | e2) : 7;
}

// The tables of the definition, derived at compile time from its text.  A tetrahedron's case is the 4-bit mask of its inside vertices
// v0..v3; an edge E(u,v), u < v, is stored as u | v << 2 (u is its `lo` end: the vertices form an increasing chain).
struct Tables {
    unsigned char cube[256];   // triangles of a cube by its 8-bit inside mask
    unsigned char ntri[16];    // triangles of a tetrahedron by case
    unsigned char edge[16][6]; // the edges of triangle q at [3q .. 3q+2]
    unsigned short flip[6];    // per tetrahedron, bit `case`: the last two vertices are swapped
    bool ok;                   // every orientation was decided by a non-zero triple product, the same for both halves of a quad
};
constexpr int edge_code(int a, int b) { return a < b ? (a | b << 2) : (b | a << 2); }
constexpr Tables make_tables()
{
    Tables T{};
    T.ok = true;
    for (int m = 0; m < 16; ++m) {
        int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
        for (int n = 0; n < 4; ++n) {
            if (m >> n & 1) in[ni++] = n;
            else out[no++] = n;
        }
        if (ni == 1 || ni == 3) {
            const int a = ni == 1 ? in[0] : out[0];
            const int *o = ni == 1 ? out : in;
            T.ntri[m] = 1;
            for (int q = 0; q < 3; ++q) T.edge[m][q] = (unsigned char)edge_code(a, o[q]);
        } else if (ni == 2) {
            const int p = in[0], q = in[1], r = out[0], s = out[1];
            T.ntri[m] = 2;
            T.edge[m][0] = (unsigned char)edge_code(p, r); T.edge[m][1] = (unsigned char)edge_code(p, s); T.edge[m][2] = (unsigned char)edge_code(q, s);
            T.edge[m][3] = (unsigned char)edge_code(p, r); T.edge[m][4] = (unsigned char)edge_code(q, s); T.edge[m][5] = (unsigned char)edge_code(q, r);
        }
        // orientation on the unit cube with inside = 1, outside = 0, iso = 0.5: every vertex is an edge midpoint; coordinates doubled
        for (int t = 0; t < 6; ++t) {
            int d[3] = {0, 0, 0};       // ni·no·(centroid of the outside vertices − centroid of the inside ones)
            for (int n = 0; n < 4; ++n)
                for (int q = 0; q < 3; ++q) d[q] += (tet_corner(t, n) >> q & 1) * ((m >> n & 1) ? -no : ni);
            for (int k = 0; k < T.ntri[m]; ++k) {
                int P[3][3] = {};
                for (int v = 0; v < 3; ++v)
                    for (int q = 0; q < 3; ++q)
                        P[v][q] = (tet_corner(t, T.edge[m][3 * k + v] & 3) >> q & 1) + (tet_corner(t, T.edge[m][3 * k + v] >> 2) >> q & 1);
                const int ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
                const int vx = P[2][0] - P[0][0], vy = P[2][1] - P[0][1], vz = P[2][2] - P[0][2];
                const int dot = (uy * vz - uz * vy) * d[0] + (uz * vx - ux * vz) * d[1] + (ux * vy - uy * vx) * d[2];
                if (dot == 0) T.ok = false;
                const bool f = dot < 0;
                if (k == 0) { if (f) T.flip[t] = (unsigned short)(T.flip[t] | 1u << m); }
                else if (f != ((T.flip[t] >> m & 1) != 0)) T.ok = false;
            }
        }
    }
    for (int mask = 0; mask < 256; ++mask) {
        int n = 0;
        for (int t = 0; t < 6; ++t) {
            int m = 0;
            for (int v = 0; v < 4; ++v) m |= (mask >> tet_corner(t, v) & 1) << v;
            n += T.ntri[m];
        }
        T.cube[mask] = (unsigned char)n;
    }
    return T;
}
constexpr Tables kHostTables = make_tables();
static_assert(kHostTables.ok, "marching-tetrahedra orientation table: a triple product vanished or a quad's halves disagree");
static_assert(kHostTables.cube[0] == 0 && kHostTables.cube[255] == 0 && kHostTables.cube[1] == 6, "cube count table");
__constant__ Tables kT = make_tables();

// the four node values of a cube face in plane p (corner order i + 2j): own column from memory, the +x column from the next lane.
// Every lane of the wave calls it (the cross-lane read needs them all); lanes whose node lies outside the box load nothing.
template <class T>
__device__ __forceinline__ void load_face(const T *__restrict__ p, idx_t row, bool node_ok, bool cube_ok, int lane, double v[4])
{
    double a0 = 0.0, a2 = 0.0;
    if (node_ok) { a0 = (double)p[0]; a2 = (double)p[row]; }
    double a1 = __shfl_down(a0, 1), a3 = __shfl_down(a2, 1);
    if (lane == 63 && cube_ok) { a1 = (double)p[1]; a3 = (double)p[row + 1]; }
    v[0] = a0; v[1] = a1; v[2] = a2; v[3] = a3;
}
__device__ __forceinline__ unsigned face_bits(const double v[4], double iso)
{
    return (v[0] >= iso ? 1u : 0u) | (v[1] >= iso ? 2u : 0u) | (v[2] >= iso ? 4u : 0u) | (v[3] >= iso ? 8u : 0u);
}
__device__ __forceinline__ bool face_finite(const double v[4]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]); }

// what a wave of either kernel works on: row segment s of row j, planes k0 … k1−1 of the box's cubes
struct Work {
    int lane, j, k0, k1, c;
    bool node_ok, cube_ok, any;
    idx_t q;                    // index of the cube's corner 0 in plane k0
    unsigned long long seg;     // linear segment index at k0; + kstride per plane
    unsigned long long kstride;
};
__device__ __forceinline__ Work work_of(const ns3d_iso_geom &g)
{
    Work w;
    w.lane = threadIdx.x & 63;
    unsigned b = blockIdx.x;
    const int s = (int)(b % (unsigned)g.nseg);
    b /= (unsigned)g.nseg;
    const int jb = (int)(b % (unsigned)g.gy), kb = (int)(b / (unsigned)g.gy);
    w.j = jb * NS3D_ISO_ROWS + (int)(threadIdx.x >> 6);
    w.any = w.j < g.cy;
    w.k0 = kb * NS3D_ISO_KZ;
    w.k1 = min(w.k0 + NS3D_ISO_KZ, g.cz);
    w.c = s * 64 + w.lane;
    w.node_ok = w.c <= g.cx;
    w.cube_ok = w.c < g.cx;
    w.q = (idx_t)(g.lox + w.c) + (idx_t)g.ex * ((idx_t)(g.loy + w.j) + (idx_t)g.ey * (idx_t)(g.loz + w.k0));
    w.kstride = (unsigned long long)g.nseg * (unsigned long long)g.cy;
    w.seg = (unsigned long long)s + (unsigned long long)g.nseg * (unsigned long long)w.j + w.kstride * (unsigned long long)w.k0;
    return w;
}

template <class T>
__global__ __launch_bounds__(64 * NS3D_ISO_ROWS) void k_iso_count(unsigned *__restrict__ segcnt, const T *__restrict__ A, ns3d_iso_geom g,
                                                                  double iso)
{
    const Work w = work_of(g);
    if (!w.any) return;         // the whole wave: its row lies outside the box
    const idx_t row = g.ex, plane = (idx_t)g.ex * g.ey;
    const T *p = A + w.q;
    double v[4];
    load_face(p, row, w.node_ok, w.cube_ok, w.lane, v);
    unsigned lob = face_bits(v, iso);
    bool lof = face_finite(v);
    unsigned long long seg = w.seg;
    for (int k = w.k0; k < w.k1; ++k) {
        p += plane;
        load_face(p, row, w.node_ok, w.cube_ok, w.lane, v);
        const unsigned upb = face_bits(v, iso);
        const bool upf = face_finite(v);
        const unsigned mask = lob | upb << 4;
        const bool mixed = w.cube_ok && mask != 0u && mask != 255u && lof && upf;
        unsigned total = 0;
        if (__ballot(mixed) != 0ull) {
            const unsigned cnt = mixed ? kT.cube[mask] : 0u;
            total = (unsigned)__popcll(__ballot(cnt & 1u)) + 2u * (unsigned)__popcll(__ballot(cnt & 2u)) +
                    4u * (unsigned)__popcll(__ballot(cnt & 4u)) + 8u * (unsigned)__popcll(__ballot(cnt & 8u));
        }
        if (w.lane == 0) segcnt[seg] = total;
        seg += w.kstride;
        lob = upb;
        lof = upf;
    }
}

__device__ __forceinline__ double sel4(int n, double x0, double x1, double x2, double x3) { return n == 0 ? x0 : n == 1 ? x1 : n == 2 ? x2 : x3; }
__device__ __forceinline__ int sel4i(int n, int x0, int x1, int x2, int x3) { return n == 0 ? x0 : n == 1 ? x1 : n == 2 ? x2 : x3; }

// the triangles of one cube from index `off` on, while off < cap.  a, b: the corner values; (ix,iy,iz): corner 0 with the origin added
template <bool COLOR>
__device__ __forceinline__ void emit_cube(const double (&a)[8], const double (&b)[8], unsigned mask, double iso, idx_t ix, idx_t iy,
                                          idx_t iz, double *__restrict__ tri, double *__restrict__ val, idx_t off, idx_t cap)
{
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int c1 = tet_corner(t, 1), c2 = tet_corner(t, 2);
        const unsigned m = (mask & 1u) | (mask >> c1 & 1u) << 1 | (mask >> c2 & 1u) << 2 | (mask >> 7 & 1u) << 3;
        const int nt = kT.ntri[m];
        const bool flip = (kT.flip[t] >> m & 1) != 0;
        for (int q = 0; q < nt; ++q) {
            if (off >= cap) return;
            double *o = tri + off * 9;
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int slot = n == 0 ? 0 : (flip ? 3 - n : n);
                const unsigned e = kT.edge[m][3 * q + n];
                const int u = (int)(e & 3u), v = (int)(e >> 2);
                const double a_lo = sel4(u, a[0], a[c1], a[c2], a[7]), a_hi = sel4(v, a[0], a[c1], a[c2], a[7]);
                const int clo = sel4i(u, 0, c1, c2, 7), inc = sel4i(v, 0, c1, c2, 7) & ~clo;
                const double tt = (iso - a_lo) / (a_hi - a_lo);
                o[3 * slot + 0] = (double)(ix + (clo & 1)) + ((inc & 1) ? tt : 0.0);
                o[3 * slot + 1] = (double)(iy + (clo >> 1 & 1)) + ((inc & 2) ? tt : 0.0);
                o[3 * slot + 2] = (double)(iz + (clo >> 2 & 1)) + ((inc & 4) ? tt : 0.0);
                if (COLOR) {
                    const double b_lo = sel4(u, b[0], b[c1], b[c2], b[7]), b_hi = sel4(v, b[0], b[c1], b[c2], b[7]);
                    val[off * 3 + slot] = b_hi * tt + b_lo * (1.0 - tt);
                }
            }
            ++off;
        }
    }
}

template <class T, bool COLOR>
__global__ __launch_bounds__(64 * NS3D_ISO_ROWS) void k_iso_emit(double *__restrict__ tri, double *__restrict__ val, idx_t cap,
                                                                 const unsigned long long *__restrict__ segbase, const T *__restrict__ A,
                                                                 const T *__restrict__ B, ns3d_iso_geom g, double iso)
{
    const Work w = work_of(g);
    if (!w.any) return;
    const idx_t row = g.ex, plane = (idx_t)g.ex * g.ey;
    idx_t q = w.q;
    double a[8];
    {
        double v[4];
        load_face(A + q, row, w.node_ok, w.cube_ok, w.lane, v);
        a[4] = v[0]; a[5] = v[1]; a[6] = v[2]; a[7] = v[3];
    }
    unsigned upb = face_bits(a + 4, iso);
    bool upf = face_finite(a + 4);
    unsigned long long seg = w.seg;
    const unsigned long long below = (1ull << w.lane) - 1ull;
    for (int k = w.k0; k < w.k1; ++k, q += plane, seg += w.kstride) {
        const unsigned lob = upb;
        const bool lof = upf;
        a[0] = a[4]; a[1] = a[5]; a[2] = a[6]; a[3] = a[7];
        load_face(A + (q + plane), row, w.node_ok, w.cube_ok, w.lane, a + 4);
        upb = face_bits(a + 4, iso);
        upf = face_finite(a + 4);
        const unsigned mask = lob | upb << 4;
        const bool mixed = w.cube_ok && mask != 0u && mask != 255u && lof && upf;
        if (__ballot(mixed) == 0ull) continue;
        const unsigned cnt = mixed ? kT.cube[mask] : 0u;
        const idx_t off = (idx_t)segbase[seg] + (idx_t)(__popcll(__ballot(cnt & 1u) & below) + 2 * __popcll(__ballot(cnt & 2u) & below) +
                                                        4 * __popcll(__ballot(cnt & 4u) & below) + 8 * __popcll(__ballot(cnt & 8u) & below));
        if (cnt == 0u || off >= cap) continue;
        double b[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (COLOR) {
            const T *bq = B + q;
            const T b0 = bq[0], b1 = bq[1], b2 = bq[row], b3 = bq[row + 1];
            const T b4 = bq[plane], b5 = bq[plane + 1], b6 = bq[plane + row], b7 = bq[plane + row + 1];
            b[0] = (double)b0; b[1] = (double)b1; b[2] = (double)b2; b[3] = (double)b3;
            b[4] = (double)b4; b[5] = (double)b5; b[6] = (double)b6; b[7] = (double)b7;
        }
        emit_cube<COLOR>(a, b, mask, iso, (idx_t)(g.lox + w.c) + g.ox, (idx_t)(g.loy + w.j) + g.oy, (idx_t)(g.loz + k) + g.oz, tri, val, off,
                         cap);
    }
}

// ---- the scan: NS3D_ISO_SCAN_BLOCK = 256 threads × 4 consecutive segments per workgroup ---------------------------------------
typedef unsigned long long u64;
__device__ __forceinline__ u64 wave_inclusive(u64 x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}
// the exclusive prefix of x over the workgroup's 256 threads; *total receives the workgroup's sum
__device__ __forceinline__ u64 block_exclusive(u64 x, u64 *total)
{
    __shared__ u64 wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 inc = wave_inclusive(x, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    u64 base = 0, all = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < wv) base += wsum[q];
        all += wsum[q];
    }
    *total = all;
    return base + inc - x;
}
__device__ __forceinline__ void load_items(const unsigned *__restrict__ cnt, u64 n, u64 first, unsigned it[4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) it[q] = first + q < n ? cnt[first + q] : 0u;
}
__global__ __launch_bounds__(256) void k_iso_blocksum(const unsigned *__restrict__ cnt, u64 n, u64 *__restrict__ bsum)
{
    unsigned it[4];
    load_items(cnt, n, (u64)blockIdx.x * NS3D_ISO_SCAN_BLOCK + 4u * threadIdx.x, it);
    u64 total;
    (void)block_exclusive((u64)it[0] + it[1] + it[2] + it[3], &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one wave: the block sums become their exclusive prefix, in chunks of 64 with a carry; result[0] = the total
__global__ __launch_bounds__(64) void k_iso_scansums(u64 *__restrict__ bsum, unsigned nblk, u64 *__restrict__ result)
{
    const int lane = threadIdx.x;
    u64 carry = 0;
    for (unsigned base = 0; base < nblk; base += 64u) {
        const unsigned i = base + (unsigned)lane;
        const u64 x = i < nblk ? bsum[i] : 0ull;
        const u64 inc = wave_inclusive(x, lane);
        if (i < nblk) bsum[i] = carry + inc - x;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) result[0] = carry;
}
__global__ __launch_bounds__(256) void k_iso_scanadd(const unsigned *__restrict__ cnt, u64 n, const u64 *__restrict__ bsum,
                                                     u64 *__restrict__ segbase)
{
    const u64 first = (u64)blockIdx.x * NS3D_ISO_SCAN_BLOCK + 4u * threadIdx.x;
    unsigned it[4];
    load_items(cnt, n, first, it);
    u64 total;
    u64 run = bsum[blockIdx.x] + block_exclusive((u64)it[0] + it[1] + it[2] + it[3], &total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (first + q < n) segbase[first + q] = run;
        run += it[q];
    }
}

static unsigned work_blocks(const ns3d_iso_geom &g) { return (unsigned)g.nseg * (unsigned)g.gy * (unsigned)g.gz; }

template <class T>
hipError_t count_scan(hipStream_t s, const T *A, const ns3d_iso_geom &g, double iso, const ns3d_iso_scratch &w)
{
    hipLaunchKernelGGL(k_iso_count<T>, dim3(work_blocks(g)), dim3(64 * NS3D_ISO_ROWS), 0, s, w.segcnt, A, g, iso);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_iso_blocksum, dim3(w.nblk), dim3(256), 0, s, w.segcnt, w.nsegs, w.bsum);
    hipLaunchKernelGGL(k_iso_scansums, dim3(1), dim3(64), 0, s, w.bsum, w.nblk, w.total);
    hipLaunchKernelGGL(k_iso_scanadd, dim3(w.nblk), dim3(256), 0, s, w.segcnt, w.nsegs, w.bsum, w.segbase);
    return hipGetLastError();
}
template <class T>
hipError_t emit(hipStream_t s, const T *A, const T *B, const ns3d_iso_geom &g, double iso, const ns3d_iso_scratch &w, double *tri,
                double *val, long long cap)
{
    if (val)
        hipLaunchKernelGGL((k_iso_emit<T, true>), dim3(work_blocks(g)), dim3(64 * NS3D_ISO_ROWS), 0, s, tri, val, (idx_t)cap, w.segbase, A, B, g,
                           iso);
    else
        hipLaunchKernelGGL((k_iso_emit<T, false>), dim3(work_blocks(g)), dim3(64 * NS3D_ISO_ROWS), 0, s, tri, val, (idx_t)cap, w.segbase, A, B, g,
                           iso);
    return hipGetLastError();
}

#define INST(T)                                                                                                                   \
    template hipError_t count_scan<T>(hipStream_t, const T *, const ns3d_iso_geom &, double, const ns3d_iso_scratch &);            \
    template hipError_t emit<T>(hipStream_t, const T *, const T *, const ns3d_iso_geom &, double, const ns3d_iso_scratch &, double *, \
                                double *, long long);
INST(double)
INST(float)
#undef INST

} // namespace ns3d_iso
