// ns3d_internal.h — what the host-side translation units of libns3d.so share (ns3d_api.cpp with ns3d_api_typed.h: single-device
// entry points and the PT loop; ns3d_mgpu.cpp: the z-slab multi-GPU layer).  Internal; the public boundary is include/ns3d.h.
#pragma once
#include <cstring>
#include <vector>

#include "ns3d_launch.h"
#include "ns3d_scratch.h"

// ns3d_fail (declared in ns3d_scratch.h) records the message behind ns3d_last_error() and returns `code`
#define fail ns3d_fail

// What a direct Poisson solve keeps while its key — grid, x boundary kind, spacings — stays the same: the three eigenbases with their
// eigenvalues (x, y, z).  ns3d_direct_basis allocates V and lam and hands them to the caller, so release() frees them, explicitly:
// the struct is plain data.  ns3d_direct.hip adds one rank's work buffers (below), ns3d_mgpu.cpp a z-slab rank's (DirectSlab).
struct ns3d_direct_bases {
    int nx = 0, ny = 0, nz = 0, xkind = -1;
    double dx = 0, dy = 0, dz = 0;
    double *V[3] = {nullptr, nullptr, nullptr}, *lam[3] = {nullptr, nullptr, nullptr};
    bool matches(const ns3d_pt_params *p, int kind) const
    {
        return nx == p->nx && ny == p->ny && nz == p->nz && xkind == kind && dx == p->dx && dy == p->dy && dz == p->dz;
    }
    void set_key(const ns3d_pt_params *p, int kind) { nx = p->nx; ny = p->ny; nz = p->nz; xkind = kind; dx = p->dx; dy = p->dy; dz = p->dz; }
    void release()
    {
        for (int q = 0; q < 3; ++q) { if (V[q]) (void)hipFree(V[q]); if (lam[q]) (void)hipFree(lam[q]); V[q] = lam[q] = nullptr; }
        nx = ny = nz = 0; xkind = -1;
    }
};
struct ns3d_direct_plan : ns3d_direct_bases {      // ns3d_poisson_direct: the bases and two work arrays of the interior cells
    ns3d_scratch W[2];
    void release() { ns3d_direct_bases::release(); for (ns3d_scratch &w : W) w.release(); }
};

struct ns3d_ctx {
    int device = 0;
    int flags = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t masked_stream = nullptr;  // ns3d_reserve_cus: a stream whose CU mask leaves `reserved_cus` compute units out
    int reserved_cus = 0;
    hipStream_t stream = nullptr;
    unsigned long long *key_dev = nullptr;  // device scratch for max reductions
    unsigned long long *key_host = nullptr; // pinned host mirror
    // Scratch grown lazily (ns3d_scratch: freed with the context).  What is waited for before an old buffer goes is the site's choice:
    // ns3d_drain_stream below, or both streams and the captured blocks for what the PT loop and the step use (ns3d_api.cpp).
    ns3d_scratch pingpong;        // second Pr buffer of the fused PT path
    ns3d_scratch pingpong_d;      // second dPrdτ buffer (temporal blocking only)
    int pt_variant = 0;
    int pt2_variant = 0; // tile shape of the two-iteration sweep; <0: temporal blocking off (on by default: ns3d_set_pt2_variant(ctx,-1) turns it off)
    int ptn_variant = 0; // tile shape of the N-iteration sweep (k_pt_sweepN); 0: built-in
    int pt_depth = 0;    // PT iterations per pass in pt_iterate / pt_solve: 0 automatic, 1…4 forced
    int graph_mode = -1; // HIP-graph replay of residual-check blocks: -1 auto (launch-bound grids), 0 off, 1 on
    int persist_mode = -1; // k_pt_persist (a whole residual-check block in one cooperative launch): -1 auto (small grids), 0 off, 1 on
    int autotune = 1;    // time the tile shapes of the two-iteration sweep on first use of a grid (pt2_variant == 0 only)
    int last_pt2 = 0;    // variant of the latest two-iteration launch (0: built-in choice by grid)
    int last_ptn = 0;    // variant of the latest N-iteration launch
    int last_depth = 0;  // PT iterations of the latest multi-iteration pass
    hipEvent_t tune_ev[2] = {nullptr, nullptr};
    hipEvent_t fence = nullptr;
    struct BlockGraph {
        struct Bufs { void *src, *dst, *dsrc, *ddst; } in, out;   // PtBufs<T> (ns3d_api.cpp) the block was captured on / leaves behind
        const void *rhs;
        int n, mode, v1, v2, vn, depth, esize;
        bool two;
        ns3d_pt_params p;
        hipGraphExec_t exec;
    };
    std::vector<BlockGraph> graphs;
    ns3d_persist_state persist;             // k_pt_persist's exchange area
    ns3d_pt_pace pace;                      // k_pt_sweepN's PACE instance (shape 29): arrival counters, launch number, settings
    ns3d_scratch diag_dev;                  // ns3d_diagnostics: NS3D_DIAG_RESULT_WORDS result / staging words, then the workgroups' partials
    unsigned long long *diag_host = nullptr; // pinned mirror of the result / staging words
    ns3d_direct_plan direct;                // ns3d_direct.hip: eigenvector matrices and scratch of the direct Poisson solve
    ns3d_scratch iso_dev;                   // ns3d_isosurface: segment counts, their scan and the total
    int advection = 0;                      // ns3d_set_advection: what ns3d_time_step advects with (NS3D_ADVECT_*)
    ns3d_scratch mc_hat;                    // ns3d_time_step under NS3D_ADVECT_MACCORMACK: stage 1's four complete fields
    ns3d_scratch solid_dev;                 // ns3d_voxelize's bit planes / ns3d_solid_momentum's partials (one stream orders both)
    const unsigned char *obstacle = nullptr; // ns3d_set_obstacle: the caller's mask ns3d_time_step masks with; null: the cylinder
    int motion_on = 0;                      // ns3d_set_obstacle_motion: ns3d_time_step masks with ns3d_set_solid_moving and these copies
    double motion[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   //   U, ω, the centre (index space)
    int motion_origin[3] = {0, 0, 0};       //   the rank's origin
    int turbulence = 0;                     // ns3d_set_turbulence: the subgrid model of ns3d_time_step's predictor (NS3D_TURB_*)
    double turb_length = 0.0;               //   its length ℓ = C_s·Δ
    void *turb_mu_e = nullptr;              //   the caller's nx·ny·nz array the step writes μ_e to
    int sgs_operator = 0;                   // ns3d_set_sgs_operator: the operator the step forms μ_e with while a model is set (NS3D_SGS_*)
    int scalar_on = 0;                      // ns3d_set_scalar: ns3d_time_step diffuses C and lifts Vz (ns3d_scalar_step) behind its predictor
    double scalar_kappa = 0.0, scalar_sct = 0.0, scalar_bg = 0.0, scalar_c_ref = 0.0;   //   κ, Sc_t (0: no eddy diffusivity), g·β, C_ref
    void clear_graphs()
    {
        for (auto &g : graphs) (void)hipGraphExecDestroy(g.exec);
        graphs.clear();
    }
};

// Every entry point runs with its context's device current and puts the caller's device back on return: a process
// that drives several devices (ns3d_mgpu_create, or PyTorch beside us) keeps its own notion of "current device".
struct ns3d_device_guard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit ns3d_device_guard(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != device) {
            err = hipSetDevice(device);
            if (err != hipSuccess) { (void)hipGetLastError(); prev = -1; }   // leave no sticky error behind for the host framework
        } else prev = -1;                    // nothing to restore
    }
    ~ns3d_device_guard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    ns3d_device_guard(const ns3d_device_guard &) = delete;
    ns3d_device_guard &operator=(const ns3d_device_guard &) = delete;
};

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) {                                                                             \
            (void)hipGetLastError(); /* reported through our status: leave no sticky error for the host framework */ \
            return fail(NS3D_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));                              \
        }                                                                                                   \
    } while (0)

// The drain (ns3d_scratch::reserve) of what only launches on c->stream ever touch — monitor, isosurface and voxelizer scratch, the
// direct solve's plan: a wait for that stream.  Captured blocks never hold these pointers, so the graphs stay.
inline auto ns3d_drain_stream(ns3d_ctx *c)
{
    return [c]() -> int { HIPCHK(c, hipStreamSynchronize(c->stream)); return NS3D_OK; };
}

#define CHECK_CTX(ctx)                                                                                    \
    if (!(ctx)) return fail(NS3D_ERR_ARG, "%s: null context", __func__);                                    \
    ns3d_device_guard dev_guard_((ctx)->device);                                                            \
    if (dev_guard_.err != hipSuccess) return fail(NS3D_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(dev_guard_.err))

#define CHECK_PTRS(...)                                                                                     \
    do {                                                                                                    \
        const void *ps_[] = {__VA_ARGS__};                                                                  \
        for (size_t q_ = 0; q_ < sizeof ps_ / sizeof ps_[0]; ++q_)                                          \
            if (!ps_[q_]) return fail(NS3D_ERR_ARG, "%s: null field pointer (argument %zu)", __func__, q_); \
    } while (0)

#define CHECK_GRID(nx, ny, nz, m)                                                                           \
    do {                                                                                                    \
        if ((nx) < (m) || (ny) < (m) || (nz) < (m))                                                         \
            return fail(NS3D_ERR_ARG, "%s: grid %dx%dx%d too small (need >= %d per direction)", __func__,   \
                        (nx), (ny), (nz), (m));                                                             \
    } while (0)

// ---- pieces of ns3d_api.cpp that the multi-GPU layer drives on its ranks' contexts (no host synchronisation) ----------
int ns3d_check_pt_params(const ns3d_pt_params *p, const char *fn);
// two fused PT iterations on stream s, tile shape as the context would choose it (looked up or built-in; never tuned here)
template <class T>
hipError_t ns3d_enqueue_pt2(ns3d_ctx *c, hipStream_t s, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                            const ns3d_pt_params *p, int k0, int k1);
// one pass of `depth` (2…4) PT iterations on stream s with the planned tile shapes (looked up; never measured here) — or with the
// shapes the caller kept from its own plan phase (v2 / vn ≥ 0: ns3d_slab_plan and box_plan measure under a depth they pin for the
// measurement only, and such entries do not answer unpinned look-ups)
template <class T>
hipError_t ns3d_enqueue_pass(ns3d_ctx *c, hipStream_t s, int depth, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV,
                             const ns3d_pt_params *p, int k0, int k1, int v2 = -1, int vn = -1, const ns3d_tile_window *win = nullptr,
                             int skip_faces = 0);
// win: a sub-rectangle of the plane's tiles, or (win->geom) a query of the tile grid this pass would use — nothing is launched then;
// skip_faces: no boundary-cell launch behind the sweep (the caller completes them with ns3d_enqueue_faces_region)
template <class T>
hipError_t ns3d_enqueue_faces_region(ns3d_ctx *c, hipStream_t s, T *Pout, const ns3d_pt_params *p, const int c0[3], const int c1[3],
                                     int want_core);
// the plan phase of ns3d_plan_pt on the context's stream (blocks on its own events); returns the planned depth
template <class T>
int ns3d_plan_pt_internal(ns3d_ctx *c, const T *src, T *dst, const T *dsrc, T *ddst, const T *divV, const ns3d_pt_params *p,
                          int k0, int k1);
// one fused PT iteration on stream s
template <class T>
hipError_t ns3d_enqueue_pt1(ns3d_ctx *c, hipStream_t s, const T *src, T *dst, T *d, const T *divV, const ns3d_pt_params *p,
                            int k0, int k1);
// max|∇²Pr − ρ/dt ∇V| as the IEEE bit pattern of a non-negative double (NaN → 0x7FF8…) into key_dev, on stream s
template <class T>
hipError_t ns3d_enqueue_residual_key(ns3d_ctx *c, hipStream_t s, const T *Pr, const T *divV, const ns3d_pt_params *p,
                                     unsigned long long *key_dev);
// halo-stripped copy A[1:sx-1,1:sy-1,1:sz-1] → packed out (gather!, multi.jl:399)
template <class T>
hipError_t ns3d_enqueue_strip_inner(ns3d_ctx *c, hipStream_t s, const T *A, T *out, int sx, int sy, int sz);
// advect! on stream s; flags: bit 0 faithful, bit 1 write-through (ns3d_kernels.hip, advect())
template <class T>
hipError_t ns3d_enqueue_advect(ns3d_ctx *c, hipStream_t s, T *Vx, const T *Vx_o, T *Vy, const T *Vy_o, T *Vz, const T *Vz_o, T *C,
                               const T *C_o, double dt, double dx, double dy, double dz, int nx, int ny, int nz, int flags, int koff,
                               int nzg);       // koff / nzg > 0: the arrays are a window koff planes into a global grid of nzg cell planes
// x (dim 0) or y (dim 1) face `idx` of A ↔ packed buffer (update_halo! of a 3-D topology)
template <class T>
hipError_t ns3d_enqueue_face_copy(ns3d_ctx *c, hipStream_t s, T *A, T *buf, int sx, int sy, int sz, int dim, int idx, int unpack);
// up to NS3D_SUBBOX_MAX blocks between column-major arrays of different pitches in one launch (ns3d_launch.h: ns3d_subbox_batch)
template <class T>
hipError_t ns3d_enqueue_subbox_copy(ns3d_ctx *c, hipStream_t s, const ns3d_subbox_batch<T> &batch);

// ns3d_diagnostics in pieces, for the multi-GPU layer: argument check; the two launches and the copy of the result words into
// c->diag_host on the context's stream (no synchronisation); the record from those words once the stream has been synchronised
int ns3d_diag_check(const ns3d_diag_params *p, const char *fn);
template <class T>
int ns3d_diag_enqueue(ns3d_ctx *c, const T *Vx, const T *Vy, const T *Vz, const T *Pr, const T *C, const ns3d_diag_params *p);
void ns3d_diag_decode(const unsigned long long *words, const ns3d_diag_params *p, bool has_pr, bool has_c, ns3d_diag *out);

// ---- ns3d_direct.hip: the stages of the direct Poisson solve, shared by ns3d_poisson_direct (one rank) and ns3d_poisson_direct_slab
// (z-slab ranks, ns3d_mgpu.cpp).  Fields in fp64 scratch, plane-major [k][i + mx·j] over a rank's mz interior planes unless said
// otherwise; every stage is enqueued on stream s and returns the launch status.
// x boundary kind of the eigenbasis: 0 Neumann on both ends, 1 Neumann / outlet value (multi.jl:179-180), 2 gpu.jl's given values
inline int ns3d_direct_xkind(const ns3d_pt_params *p) { return p->bc_kind == NS3D_BC_GPU ? 2 : (p->owns_outlet ? 1 : 0); }
// y modes of chunk c when my modes are split into P contiguous chunks whose widths differ by at most one (empty when my < P)
__host__ __device__ inline void ns3d_direct_ychunk(int my, int P, int c, int *ky0, int *nky)
{
    const int base = my / P, rem = my % P;
    *nky = base + (c < rem ? 1 : 0);
    *ky0 = c * base + (c < rem ? c : rem);
}
// eigenbasis (V: m×m, column q = mode q; lam: m eigenvalues) of the 1-D second difference on m cells, uploaded to the current device
int ns3d_direct_basis(int m, double d, int kind, double **V, double **lam);
// F ← the right-hand side of the rank's interior cells, U ← Vxᵀ·F
template <class T>
hipError_t ns3d_direct_rhs_x(hipStream_t s, const T *divV, const ns3d_pt_params *p, const double *Vx, double *F, double *U);
// out[k][i + mx·(ky − ky0)] = Σ_j U[k][i + mx·j]·Vy(j, ky) for the y modes ky0 … ky0+nky−1
hipError_t ns3d_direct_fwd_y(hipStream_t s, const double *U, const double *Vy, double *out, int mx, int my, int mz, int ky0, int nky);
// mx·nky columns over mz planes ([k][i + mx·(ky − ky0)]): U ← Vz·((Vzᵀ·U) ⊘ (λx + λy + λz)), the null mode set to 0; ly points at the
// λy of mode ky0; tmp: scratch of U's size
hipError_t ns3d_direct_z(hipStream_t s, double *U, double *tmp, const double *Vz, const double *lx, const double *ly, const double *lz,
                         int mx, int nky, int mz);
// Pr's interior ← Vx·(U_k·Vyᵀ) of the rank's planes, dPrdτ ← 0 (U and tmp are overwritten; Pr's boundary cells are not touched)
template <class T>
hipError_t ns3d_direct_inv_yx(hipStream_t s, double *U, double *tmp, const double *Vx, const double *Vy, T *Pr, T *D, int nx, int ny,
                              int nz);
// chunk-major [c][k][i + mx·(ky − ky0_c)] (ns3d_direct_ychunk's P chunks, each over the mz planes) → plane-major dst
hipError_t ns3d_direct_unpack(hipStream_t s, const double *src, double *dst, int mx, int my, int mz, int P);

// ---- ns3d_tracers.hip: ns3d_sample / ns3d_tracers_advance.  One compilation without contraction serves every arithmetic mode (the
// entry points' contract: the same bits from STRICT, NS3D_IEEE_DIV and FAST contexts).  n > 0; state (sample) and U (advance) may be null.
// The _at forms take positions in the GLOBAL index space of a decomposed grid: origin (3 ints, not null) is the rank's first cell,
// n_g (3 ints, not null) the global cell grid of the advance's "inside" tests.
// ns3d_tracers_migrate_mgpu's routing (ns3d_mgpu.cpp drives it): mig_count classifies a rank's slots and leaves the per-workgroup
// counts, their prefix sums and the P+1 totals in the scratch; mig_pack moves the leavers into records and empties their slots;
// mig_insert puts received records into the empty slots.
#define NS3D_MIG_REC 8             // doubles per travelling particle: x, y, z, the id's bits, u, v, w, unused
struct ns3d_mig_geom {
    int dims[3], n[3];             // topology and local cell grid
    double inv[3];                 // 1/(n−2): the owner's first estimate (comparisons decide)
    int me, P;
};
struct ns3d_mig_scratch {          // device scratch of one rank and one call, carved out of the rank's buffer; nwg = ceil(cap/256)
    int *dest, *code;              // per slot
    unsigned *counts;              // (P+1) rows × nwg
    unsigned long long *offs;      // (P+1) rows × nwg
    unsigned long long *totals;    // P+1
    unsigned long long *dbase;     // P: where the records for each destination start in the send buffer
};
namespace ns3d_tracers {
template <class T>
hipError_t sample(hipStream_t s, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey, int ez,
                  int stag_x, int stag_y, int stag_z);
template <class T>
hipError_t advance(hipStream_t s, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy, const T *Vz, double cx,
                   double cy, double cz, int nx, int ny, int nz);
template <class T>
hipError_t sample_at(hipStream_t s, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey, int ez,
                     int stag_x, int stag_y, int stag_z, const int *origin);
template <class T>
hipError_t advance_at(hipStream_t s, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy, const T *Vz, double cx,
                      double cy, double cz, int nx, int ny, int nz, const int *origin, const int *n_g);
hipError_t mig_count(hipStream_t s, const ns3d_mig_scratch &w, const double *X, const unsigned char *state, const long long *id, long cap,
                     const ns3d_mig_geom &g);
hipError_t mig_pack(hipStream_t s, const ns3d_mig_scratch &w, double *rec, double *X, unsigned char *state, long long *id, double *U,
                    long cap);
hipError_t mig_insert(hipStream_t s, const ns3d_mig_scratch &w, int P, const double *rec, long n_arr, double *X, unsigned char *state,
                      long long *id, double *U, long cap);
}

// ---- ns3d_solid.hip: ns3d_voxelize / ns3d_set_solid / ns3d_solid_momentum.  One compilation without contraction serves every
// arithmetic mode.  voxelize: origin is three ints (not null), scratch holds voxelize_scratch_bytes (zeroed inside, on s); momentum:
// seam flags not null, scratch holds momentum_scratch_bytes, result receives 3 sums (fp64 bit patterns) and 3 counts.
namespace ns3d_solid {
size_t voxelize_scratch_bytes(int nx, int ny, int nz);
hipError_t voxelize(hipStream_t s, unsigned char *mask, const double *tri, long long n_tri, int nx, int ny, int nz, const int *origin,
                    void *scratch);
template <class T>
hipError_t set_solid(hipStream_t s, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, int nx, int ny, int nz);
size_t momentum_scratch_bytes(int nx, int ny, int nz);
template <class T>
hipError_t momentum(hipStream_t s, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny, int nz,
                    const int *seam_lo, const int *seam_hi, void *scratch, unsigned long long *result);
// moving bodies: a rigid motion as the kernels take it — U, ω, the centre (index space), the spacings and the rank's origin — checked by
// the entry points; set_solid_moving / momentum_moving are set_solid / momentum with it; mesh_transform: out == tri or disjoint
struct Motion {
    double U[3], w[3], c[3], d[3];
    int o[3];
};
template <class T>
hipError_t set_solid_moving(hipStream_t s, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, const Motion &mo, int nx, int ny, int nz);
template <class T>
hipError_t momentum_moving(hipStream_t s, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, const Motion &mo, int nx, int ny,
                           int nz, const int *seam_lo, const int *seam_hi, void *scratch, unsigned long long *result);
hipError_t mesh_transform(hipStream_t s, double *out, const double *tri, long long n_tri, const double *R, const double *pivot,
                          const double *shift, const double *spacing);
}
