// ns3d_launch.h — host-side launcher declarations shared by ns3d_kernels.hip (compiled twice: once per
// arithmetic mode) and ns3d_api.cpp.  Internal header; the public boundary is include/ns3d.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ns3d.h"

// k_pt_persist's exchange area (face values handed between workgroups) and error word: owned by a context, freed with it
// A sweep over a sub-rectangle of a plane's tiles (ns3d_mgpu.cpp box_pass_overlapped: the shells next to decomposed faces first, the core while
// the exchange runs).  Tiles [x0,x1) × [y0,y1) of the tile grid the launch would otherwise cover; x1 <= x0 means the whole grid.
// geom != nullptr: nothing is launched — the launcher reports the tile grid this depth / variant / grid would use.
// pass_flags of pt_sweep2 / pt_sweepn: bit 1 — no boundary-cell launch behind the sweep; bits 8… — compute units (in eights) the stream's
// CU mask leaves out (ns3d_reserve_cus), which the z-chunking must not count on
#define NS3D_PASS_SKIP_FACES 2
static inline int ns3d_pass_flags_cus(int reserved_cus) { return (reserved_cus / 8) << 8; }    // the CU field of pass_flags, and back:
static inline int ns3d_pass_cus_off(int pass_flags) { return ((pass_flags >> 8) & 0xff) * 8; } // compute units to leave out
#define NS3D_FACES_FOLDED 2             /* SweepArgs::no_faces: the sweep kernel forms the boundary cells itself (fold_faces) */
#define NS3D_FOLD_MAX_CELLS 20000000L   /* … by default on grids up to this many cells */
struct ns3d_tile_geom { int TX, TY, OV, ntx, nty; };      // columns × rows per tile, overlap 2(NL−1), tiles per plane
struct ns3d_tile_window { int x0, x1, y0, y1; ns3d_tile_geom *geom; };
struct ns3d_persist_state {
    void *H = nullptr;
    unsigned *err = nullptr;            // device word: ticket of the latest launch in which a bounded wait expired
    unsigned *err_host = nullptr;       // the same, in pinned host memory the device writes straight into: the host reads it after any
    unsigned *err_host_dev = nullptr;   //   synchronisation of the stream, without a copy (device-side address of err_host)
    size_t bytes = 0;
    unsigned long long launches = 0;    // key epoch: a launch never accepts a value an earlier one left in a slot
    unsigned ticket = 0;                // number of the latest launch (what a failing launch leaves in the error words)
    unsigned checked = 0;               // launches up to this ticket have been checked by the host
    unsigned faults = 0;                // launches found failed (and redone by the launch-per-iteration path) so far
    hipEvent_t ev = nullptr;            // recorded behind every launch: a launch on ANOTHER stream waits for it (two grids must
                                        // not meet in the same slots) — no stream handle is kept
    // the whole-solve form (residual checks inside the launch): a value/key pair per workgroup on the device, and what the host reads
    // after synchronising — [0] iterations done, [1] checks made, [2+q] the key of max|Rp| at check q — in pinned host memory
    unsigned long long *red = nullptr;
    unsigned long long *res_host = nullptr, *res_host_dev = nullptr;
};
// Pacing of k_pt_sweepN's PACE instance (shape 29): the workgroups of one XCD group (blockIdx & 7) meet every pace_z z-steps at an arrival
// counter per (rendezvous, group).  Counters only grow: launch number `seq` since they were last zeroed waits for seq × (workgroups of
// the group).  A launch whose geometry differs from the one before zeroes them first, on its own stream.  A hint: waits are bounded and
// no result depends on them.  Owned by a context, freed with it.
#define NS3D_PACE_SLOTS 256            /* rendezvous per launch that have a counter; later ones are skipped */
#define NS3D_PACE_HEADER 4             /* 64-bit words before the counters; 32-bit words 0…2: pace_z, the bound of a wait, the test offset */
#define NS3D_PACE_TICKS_DEFAULT 65536  /* bound of one wait in s_memtime ticks: 14 µs, about five z-steps of the 512³ fp64 pass (profiles/pt_realign_ab.log) */
struct ns3d_pt_pace {
    unsigned long long *ctr = nullptr;  // device: NS3D_PACE_HEADER header words, then 8 × NS3D_PACE_SLOTS counters
    int hdr[3] = {-1, -1, -1};          // what the header holds
    unsigned long long seq = 0;         // paced launches since the counters were zeroed
    int sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // geometry of those launches: nx, ny, nz, k0, k1, workgroups, levels·1000 + element size, pace_z
    int pace_z = -1;                    // ns3d_set_pt_pace: −1 automatic (the plan's value, never below the planner's gate), 0 off, else z-steps
    int ticks = NS3D_PACE_TICKS_DEFAULT;
    int test_extra = 0;                 // test hook: arrivals the target is raised by, so that every wait expires
    int last = 0;                       // pace_z of the latest N-iteration launch, 0: not paced
};
#define NS3D_PERSIST_MAXCHK 2048
#define NS3D_PERSIST_MAXWG 1024        /* < MAXCHK: the workgroups' pairs, the result pair and the parameters share one block */

// k_subbox_copy: one cx·cy·cz block between two column-major arrays (pitches in elements), and a batch of them for one launch
#define NS3D_SUBBOX_MAX 8
template <class T>
struct ns3d_subbox {
    T *dst;
    const T *src;
    long dpx, dpl, spx, spl;
    int cx, cy, cz;
    unsigned blocks;               // filled by the launcher
};
template <class T>
struct ns3d_subbox_batch {
    ns3d_subbox<T> p[NS3D_SUBBOX_MAX];
    int n = 0;
    bool add(T *dst, long dpx, long dpl, const T *src, long spx, long spl, int cx, int cy, int cz)
    {
        if (n >= NS3D_SUBBOX_MAX) return false;
        p[n++] = {dst, src, dpx, dpl, spx, spl, cx, cy, cz, 0u};
        return true;
    }
};

// ns3d_diagnostics (k_diag): 64×4 columns per workgroup over the (nx+1)×(ny+1) column range, kz planes of the nz+1 plane range per
// workgroup — 32, halved down to 8 while the launch has fewer than 2 048 workgroups.  Every workgroup leaves NS3D_DIAG_SLOTS 8-byte
// partials ([slot][workgroup]); k_diag_final (one workgroup per slot) combines them into NS3D_DIAG_SLOTS result words.
#define NS3D_DIAG_SLOTS 15      /* 0 ke, 1 c, 2-4 mom | 5-7 n_masked | 8-10 vmax keys, 11 div, 12 pr_max, 13 -pr_min, 14 nonfinite */
#define NS3D_DIAG_RESULT_WORDS 32   /* result words, then a staging area for the all-reduce of the one-process-per-GPU form */
inline unsigned ns3d_diag_geometry(int nx, int ny, int nz, int *kz_out)
{
    const unsigned gx = (unsigned)(nx + 1 + 63) / 64, gy = (unsigned)(ny + 1 + 3) / 4;
    int kz = 32;
    while (kz > 8 && gx * gy * ((unsigned)(nz + 1 + kz - 1) / kz) < 2048u) kz /= 2;
    if (kz_out) *kz_out = kz;
    return gx * gy * ((unsigned)(nz + 1 + kz - 1) / kz);
}

// ns3d_stats_accumulate (k_stats): 64×4 columns per workgroup over the nx×ny cell columns, NS3D_STATS_KZ planes of the nz cell planes
// per workgroup.  4 was the fastest of 4 / 8 / 16 / 32 at 512³ and at 255×153×153 alike (profiles/stats_variants_ab.log): short
// chunks keep every CU busy on small grids (a rank of the 255×153×153 case: 6 240 workgroups) and cost one extra Vz plane in four.
#define NS3D_STATS_KZ 4

// ns3d_vortex (k_vortex): 64×4 cell columns per workgroup over the nx×ny columns, NS3D_VORTEX_KZ of the nz planes per workgroup (two
// further planes of Vx and Vy are read per chunk for the z ring).  64×4 with 16 planes was the fastest of 64×4 / 64×8 / 64×16 with
// 8 / 16 / 32 planes at 512³ in fp64 and within 7 % of the best elsewhere (profiles/vortex_variants_ab.log).
#define NS3D_VORTEX_KZ 16

// ns3d_scalar_diffuse / ns3d_buoyancy / ns3d_scalar_step (ns3d_scalar.hip, k_scalar): the same 64×4 cell columns per workgroup over the
// nx×ny columns, NS3D_SCALAR_KZ of the nz planes per workgroup (one further plane of C, and of mu_e, is read at each end of a chunk).
#define NS3D_SCALAR_KZ 16

// ns3d_isosurface (ns3d_isosurface.hip, compiled once: no arithmetic mode to select).  k_iso_count / k_iso_emit: one wave per row
// segment of 64 cubes in x, NS3D_ISO_ROWS rows (j) per workgroup, NS3D_ISO_KZ cube planes marched in z per workgroup; the scan
// works on NS3D_ISO_SCAN_BLOCK segments per workgroup and scans the workgroups' sums with one wave, 64 at a time.
#define NS3D_ISO_ROWS 4
#define NS3D_ISO_KZ 8
#define NS3D_ISO_SCAN_BLOCK 1024
struct ns3d_iso_geom {
    int ex, ey;                 // pitches of A and B
    int lox, loy, loz;          // lowest node of the box
    int cx, cy, cz;             // cubes per direction
    int nseg, gy, gz;           // row segments per row; workgroups in y and z (launch: nseg·gy·gz workgroups, x fastest)
    int ox, oy, oz;             // origin
};
struct ns3d_iso_scratch {       // device scratch of one call, carved out of the context's buffer
    unsigned long long nsegs;   // nseg·cy·cz
    unsigned nblk;              // scan workgroups
    unsigned long long *total;  // [0]: the number of triangles
    unsigned long long *bsum;   // nblk sums, then their exclusive prefix
    unsigned long long *segbase; // nsegs: exclusive prefix of segcnt
    unsigned *segcnt;           // nsegs: triangles per (segment, j, k)
};
namespace ns3d_iso {
// count + scan: fills w.segbase and w.total[0]
template <class T>
hipError_t count_scan(hipStream_t, const T *A, const ns3d_iso_geom &, double iso, const ns3d_iso_scratch &w);
// after count_scan on the same input: the first `cap` triangles into tri (and val, from B, when val is not null)
template <class T>
hipError_t emit(hipStream_t, const T *A, const T *B, const ns3d_iso_geom &, double iso, const ns3d_iso_scratch &w, double *tri,
                double *val, long long cap);
}

#define NS3D_LAUNCHER_DECLS(NS)                                                                              \
    namespace NS {                                                                                           \
    template <class T>                                                                                       \
    hipError_t update_tau(hipStream_t, T *, T *, T *, T *, T *, T *, const T *, const T *, const T *, double,\
                          double, double, double, int, int, int);                                            \
    template <class T>                                                                                       \
    hipError_t predict_V(hipStream_t, T *, T *, T *, const T *, const T *, const T *, const T *, const T *,  \
                         const T *, double, double, double, double, double, double, int, int, int);          \
    template <class T>                                                                                       \
    hipError_t set_cylinder(hipStream_t, T *, T *, T *, T *, double, double, double, double, double, double, \
                            int local_form, double, double, double, double, double, double, int, int, int);  \
    template <class T>                                                                                       \
    hipError_t update_divV(hipStream_t, T *, const T *, const T *, const T *, double, double, double, int,   \
                           int, int);                                                                        \
    template <class T>                                                                                       \
    hipError_t update_dPrdtau(hipStream_t, const T *, T *, const T *, double, double, double, double, double,\
                              double, double, int, int, int);                                                \
    template <class T>                                                                                       \
    hipError_t update_Pr(hipStream_t, T *, const T *, double, int, int, int);                                \
    template <class T>                                                                                       \
    hipError_t compute_res(hipStream_t, T *, const T *, const T *, double, double, double, double, double,   \
                           int, int, int);                                                                   \
    template <class T>                                                                                       \
    hipError_t max_abs_key(hipStream_t, const T *, long, unsigned long long *key_dev);                       \
    template <class T>                                                                                       \
    hipError_t correct_V(hipStream_t, T *, T *, T *, const T *, double, double, double, double, double, int, \
                         int, int);                                                                          \
    /* which: 0 bc_x 1 bc_y 2 bc_z 3 bc_zV 4 bc_xhydstatic 5 bc_x_Vx 6 bc_x_Pr */                            \
    template <class T>                                                                                       \
    hipError_t bc_plane(hipStream_t, int which, T *, int, int, int, double a, double b, double c, int nz_arg);\
    /* set_bc_Vel! (what 0: A0..A2 = Vx, Vy, Vz) or set_bc_Pr! (what 1: A0 = Pr) as one gather launch; hipErrorInvalidValue where an \
     * extent is too small for that form (the caller then launches rule by rule) */                           \
    template <class T>                                                                                       \
    hipError_t bc_fused(hipStream_t, int what, int bc_kind, T *A0, T *A1, T *A2, int nx, int ny, int nz, int owns, double val, \
                        double rho_g, double dz, int nz_arg);                                                \
    template <class T>                                                                                       \
    hipError_t advect(hipStream_t, T *, const T *, T *, const T *, T *, const T *, T *, const T *, double,   \
                      double, double, double, int, int, int, int, int koff, int nzg);                        \
    /* stage 2 of the limited MacCormack advection: new fields from the old ones (*_o) and stage 1's complete result (*_h) */ \
    template <class T>                                                                                       \
    hipError_t advect_mc(hipStream_t, T *Vx, const T *Vx_o, const T *Vx_h, T *Vy, const T *Vy_o, const T *Vy_h, T *Vz, \
                         const T *Vz_o, const T *Vz_h, T *C, const T *C_o, const T *C_h, double dt, double dx, double dy, \
                         double dz, int nx, int ny, int nz);                                                  \
    template <class T>                                                                                       \
    hipError_t pt_sweep(hipStream_t, int variant, const T *, T *, T *, const T *, const ns3d_pt_params &,    \
                        int k0, int k1);                                                                     \
    template <class T>                                                                                       \
    hipError_t predict_fused(hipStream_t, T *, T *, T *, const T *, const T *, const T *, double mu, double rho, \
                             double g, double dt, double dx, double dy, double dz, int, int, int);           \
    /* pass_flags: bits 8… = compute units the launch must not count on, in eights (as pt_sweep2 / pt_sweepn take them) */ \
    template <class T>                                                                                       \
    hipError_t pt_persist(hipStream_t, const T *, T *, const T *, T *, const T *, const ns3d_pt_params &,    \
                          int n_iters, ns3d_persist_state *, int pass_flags, int nchk = 0, double eps = -1.0,\
                          double err_mul = 1.0, double err_div = 1.0);                                        \
    template <class T>                                                                                       \
    hipError_t pt_sweep2(hipStream_t, int variant, const T *, T *, const T *, T *, const T *,                \
                         const ns3d_pt_params &, int k0, int k1, int pass_flags, const ns3d_tile_window *win = nullptr); \
    template <class T>                                                                                       \
    hipError_t pt_sweepn(hipStream_t, int nlev, int variant, const T *, T *, const T *, T *, const T *,      \
                         const ns3d_pt_params &, int k0, int k1, int pass_flags, const ns3d_tile_window *win = nullptr, \
                         ns3d_pt_pace *pace = nullptr);                                                       \
    /* the boundary cells of Pout whose SOURCE cell (the interior cell they clamp onto) lies inside (want_core) or outside the  \
     * box [c0,c1) of cells: the partial boundary-cell launches of a split pass (box_pass_overlapped) */      \
    template <class T>                                                                                       \
    hipError_t pt_faces_region(hipStream_t, T *Pout, const ns3d_pt_params &, const int c0[3], const int c1[3], int want_core); \
    template <class T>                                                                                       \
    hipError_t residual_max_key(hipStream_t, const T *, const T *, const ns3d_pt_params &,                   \
                                unsigned long long *key_dev);                                                \
    /* part: NS3D_DIAG_SLOTS × ns3d_diag_geometry() words, result: NS3D_DIAG_SLOTS words (both on the device) */ \
    template <class T>                                                                                       \
    hipError_t diagnostics(hipStream_t, const T *Vx, const T *Vy, const T *Vz, const T *Pr, const T *C,     \
                           const ns3d_diag_params &, unsigned long long *part, unsigned long long *result); \
    /* S: NS3D_STATS_SLOTS blocks of nx·ny·nz doubles; Pr may be null */                                     \
    template <class T>                                                                                       \
    hipError_t stats_accumulate(hipStream_t, double *S, const T *Vx, const T *Vy, const T *Vz, const T *Pr, \
                                double weight, int nx, int ny, int nz);                                      \
    hipError_t stats_finalize(hipStream_t, const double *S, double wsum, double *mean, double *rs, long n_cells); \
    /* any of Wx, Wy, Wz, Q may be null (not all) */                                                          \
    template <class T>                                                                                       \
    hipError_t vortex(hipStream_t, T *Wx, T *Wy, T *Wz, T *Q, const T *Vx, const T *Vy, const T *Vz,        \
                      double dx, double dy, double dz, int nx, int ny, int nz);                              \
    /* Smagorinsky: mu_e = mu + rho·length²·|S| on interior cells, mu elsewhere; then the stresses and the predictor under it */ \
    template <class T>                                                                                       \
    hipError_t eddy_viscosity(hipStream_t, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho, \
                              double length, double dx, double dy, double dz, int nx, int ny, int nz);       \
    /* the same with |S| replaced by the operator `op` (NS3D_SGS_*, checked by the caller); op 0 IS eddy_viscosity */ \
    template <class T>                                                                                       \
    hipError_t sgs_viscosity(hipStream_t, int op, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho, \
                             double length, double dx, double dy, double dz, int nx, int ny, int nz);        \
    template <class T>                                                                                       \
    hipError_t update_tau_var(hipStream_t, T *, T *, T *, T *, T *, T *, const T *, const T *, const T *, const T *mu_e, \
                              double dx, double dy, double dz, int, int, int);                               \
    template <class T>                                                                                       \
    hipError_t predict_var(hipStream_t, T *, T *, T *, const T *, const T *, const T *, const T *mu_e, double rho, \
                           double g, double dt, double dx, double dy, double dz, int, int, int);             \
    /* ns3d_scalar.hip.  what: bit 0 the diffusion step C_out from C (mu_e may be null), bit 1 the buoyancy term into Vz */ \
    template <class T>                                                                                       \
    hipError_t scalar_step(hipStream_t, int what, T *C_out, T *Vz, const T *C, const T *mu_e, double kappa, double sgs, \
                           double mu, double bg, double c_ref, double dt, double dx, double dy, double dz, int nx, int ny, int nz); \
    template <class T>                                                                                       \
    hipError_t divtest(hipStream_t, double d, long n, unsigned long long seed, unsigned long long *bad_dev); \
    template <class T>                                                                                       \
    hipError_t strip_inner(hipStream_t, const T *A, T *out, int sx, int sy, int sz);                         \
    template <class T>                                                                                       \
    hipError_t face_copy(hipStream_t, T *A, T *buf, int sx, int sy, int sz, int dim, int idx, int unpack);   \
    template <class T>                                                                                       \
    hipError_t subbox_copy(hipStream_t, const ns3d_subbox_batch<T> &);                                       \
    }

NS3D_LAUNCHER_DECLS(ns3d_strict)
NS3D_LAUNCHER_DECLS(ns3d_strictx)
NS3D_LAUNCHER_DECLS(ns3d_strictp)
NS3D_LAUNCHER_DECLS(ns3d_fast)
