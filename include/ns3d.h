/*
 * ns3d.h — C ABI of libns3d.so: hand-written HIP (gfx950 / MI355X) kernels for the hot path of
 * mattbuergler/NavierStokes3D, behind the reference's own kernel call signatures.
 *
 * The reference has no FFI: its "operator API" is ParallelStencil's calling convention
 *     @parallel kernel!(arrays…, scalars…)
 * used by the time loops scripts/NavierStokes3D_gpu.jl:119-142 ("gpu.jl") and
 * scripts/NavierStokes3D_multi_gpu.jl:446-477 ("multi.jl").  Every entry point below replaces one of
 * those kernels (cited per function) with the SAME positional argument order, followed by the cell grid
 * (nx,ny,nz) that ParallelStencil derives from the array sizes.  INTEGRATION.md shows the Julia `ccall`
 * stubs that bind them so the reference time loops run unchanged.
 *
 * Conventions
 *  - All field pointers are DEVICE pointers to packed column-major arrays (x fastest) with exactly the
 *    reference shapes (multi.jl:343-360):
 *        Pr,C,C_o,τxx,τyy,τzz,∇V : (nx,ny,nz)      Vx,Vx_o : (nx+1,ny,nz)   Vy,Vy_o : (nx,ny+1,nz)
 *        Vz,Vz_o : (nx,ny,nz+1)    τxy,τxz,τyz : (nx-1,ny-1,nz-1)           dPrdτ,Rp : (nx-2,ny-2,nz-2)
 *    The caller owns every field buffer.  The library owns only its context (stream, reduction scratch,
 *    lazily allocated ping-pong Pr / dPrdτ buffers for the fused PT path).
 *  - Suffix _f64 / _f32 = element type of the arrays; scalar parameters are always C double (Julia
 *    Float64 host values) and are converted to the element type on entry.
 *  - Every function returns 0 (NS3D_OK) or a non-zero status; the message is available from
 *    ns3d_last_error().  Nothing throws or aborts across the boundary.
 *  - Like `@parallel`, every call is synchronous to the caller unless the context was created with
 *    NS3D_ASYNC (then calls only enqueue on the context's stream; use ns3d_sync()).  The same holds on whichever stream
 *    the context launches on (ns3d_set_stream, ns3d_use_own_stream, ns3d_reserve_cus): inputs are read and outputs
 *    written in that stream's order, and ns3d_sync() waits for everything a call started.
 *    These calls wait for the stream even on an NS3D_ASYNC context (tests/test_gpu_stream_order.py takes each entry point
 *    on three non-blocking streams, with inputs that arrive late and readers that follow early, and sorts them the same way):
 *        call                                   waits for                          device outputs complete on return?
 *        ns3d_max_abs, ns3d_residual_max        the value it returns               (none)
 *        ns3d_diagnostics                       the record it returns              (none)
 *        ns3d_selftest_exact_div                the count it returns               (none)
 *        ns3d_solid_momentum,                   the sums and counts it returns     (none)
 *        ns3d_solid_momentum_moving
 *        ns3d_isosurface                        the triangle count                 no: tri / val are enqueued behind the count
 *        ns3d_tracers_migrate_mgpu              the counts of leavers and empty    no: pack, exchange and insert are enqueued behind them
 *                                               slots of every rank
 *        ns3d_pt_solve                          every residual check              no: the copies into Pr / dPrdtau are enqueued
 *        ns3d_time_step                         as ns3d_pt_solve (pressure 0);     no: the rest of the step is enqueued behind the solve;
 *                                               the whole step (pressure 1)        yes with pressure 1
 *        ns3d_pt_iterate                        the block, WHEN it runs as the     no: the copies into Pr / dPrdtau are enqueued
 *                                               one k_pt_persist launch (small
 *                                               grids or persist mode 1)
 *        ns3d_plan_pt, and the first            the timed launches of the tile     as the call otherwise
 *        pt_iterate / pt_solve / pt_sweep2      shapes (grids of 1.5 M cells up,
 *        of a grid                              autotune on)
 *        ns3d_poisson_direct                    the stream, WHEN it builds or      no
 *                                               replaces its plan (a new grid)
 *        any call that grows a scratch buffer   the stream, before the old         as the call otherwise
 *        of the context (ping-pong, advection   buffer is freed
 *        hat, monitor, isosurface, voxelizer)
 *        and ns3d_reserve_cus
 *        ns3d_set_stream, ns3d_use_own_stream,  the stream the context LEAVES       (none)
 *        ns3d_reserve_cus                       (when it differs from the new one)
 *    Everything else only enqueues.
 *  - One host thread AT A TIME per context (as in the reference: one thread per rank): a context is not thread-safe, two
 *    threads must not be inside calls on the same context together.  Calls on DIFFERENT contexts may run concurrently from
 *    different host threads, on one device or several; such contexts share nothing a result depends on.  What the contexts of
 *    a process do share is guarded inside the library: the planner's memory (the tile shapes timed on first use of a grid
 *    are remembered per process, device, grid, element type, arithmetic build, pinned depth and CU mask, and answer the
 *    look-ups of every context) and the eigenvector cache of ns3d_poisson_direct.  ns3d_last_error() is per THREAD: it
 *    returns the message of the latest failed call made by the calling thread, on whichever context.
 *    A cooperative launch (ns3d_set_persist_mode) beside other contexts' kernels may find compute units taken; it is then
 *    voided and redone as described there, with the same result.
 *    (tests/test_gpu_context_history.py runs one context through the entry points that keep state in it — every PT form, the
 *    direct solve, monitor, isosurface, read-backs, whole steps — on seven grids, in both element types, between changes of
 *    every knob and stream, in hostile and seeded orders; tests/test_gpu_host_threads.py runs four such contexts on four threads.)
 *  - Arithmetic modes: NS3D_STRICT reproduces the reference's operation order with correctly rounded division
 *    and no FMA contraction (bit-identical to the CPU oracle); NS3D_FAST uses reciprocal constants and FMA
 *    (≤1e-6 relative L2 at equal iteration counts).  In STRICT mode x/dx is evaluated as the correctly rounded
 *    quotient by the divisor-known-in-advance sequence q=RN(x·r), e=x−q·dx (FMA), RN(q+e·r) with r=RN(1/dx)
 *    whenever dx,dy,dz are eligible (same bits as the division instruction sequence, ≈⅓ of the instructions;
 *    ns3d_selftest_exact_div compares the two on the device, with quotients drawn across the whole range in which
 *    the sequence runs, both of its bounds and the plain-division range beyond them); NS3D_IEEE_DIV forces the plain sequence.
 */
#ifndef NS3D_H
#define NS3D_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ns3d_ctx ns3d_ctx;

enum {
    NS3D_OK = 0,
    NS3D_ERR_ARG = 1,   /* bad argument (null pointer, extent too small, …) */
    NS3D_ERR_HIP = 2,   /* a HIP runtime call or kernel launch failed */
    NS3D_ERR_STATE = 3, /* context misuse */
    NS3D_ERR_RCCL = 4   /* RCCL could not be loaded, or an RCCL call failed */
};

enum {
    NS3D_STRICT = 0x0,
    NS3D_FAST = 0x1,
    NS3D_ASYNC = 0x2,
    NS3D_IEEE_DIV = 0x4 /* STRICT only: always use the plain IEEE division instruction sequence (see below) */
};

/* bc_kind for the pressure / velocity boundary sequences */
enum {
    NS3D_BC_MULTI = 0, /* multi.jl:175-181 / :156-166 */
    NS3D_BC_GPU = 1    /* gpu.jl:281-286 / :264-279 */
};

#define NS3D_VERSION 1
int ns3d_version(void);
const char *ns3d_last_error(void);

/* Context = device + stream + scratch.  Replaces @init_parallel_stencil (gpu.jl:4-8).
 * Device arrays need only the alignment of their element type (8 bytes for _f64 arrays, 4 for _f32, 1 for the tracers' uint8 state):
 * a view into a larger buffer is a valid argument.  A call neither loads from nor stores to addresses outside the arrays passed
 * to it and the context's own scratch (tests/test_gpu_footprint.py runs every single-rank entry point in guarded arenas at that
 * alignment, tests/test_gpu_footprint_mgpu.py the ns3d_mgpu entry points with all ranks' arrays in one arena). */
ns3d_ctx *ns3d_create(int device, int flags);
void ns3d_destroy(ns3d_ctx *ctx);
int ns3d_flags(const ns3d_ctx *ctx);
/* Launch on an existing hipStream_t (e.g. PyTorch's current stream; NULL is HIP's null stream).  A new context
 * launches on a private non-blocking stream; ns3d_use_own_stream() returns to it.  Both WAIT for the stream the context
 * leaves (as does ns3d_reserve_cus): whatever an NS3D_ASYNC context queued there is complete before the context launches
 * anywhere else, so its scratch, counters and read-back words are never used from two streams at once.  The stream being
 * left must still exist (a host that destroys a stream moves its contexts off it first).  While either stream — the one left
 * or the one moved to — is being captured there is no wait: a captured stream runs nothing, and a synchronisation beside the
 * caller's capture would invalidate it; a host that moves an NS3D_ASYNC context into a capture has synchronised it before
 * the capture began.  Naming the stream the context is already on costs nothing. */
int ns3d_set_stream(ns3d_ctx *ctx, void *hip_stream);
int ns3d_use_own_stream(ns3d_ctx *ctx);
/* Leave `n_cus` compute units of the device OUT of this context's launches: the context gets a stream of its own created with a CU
 * mask (hipExtStreamCreateWithCUMask) and launches there from now on; 0 = back to the unmasked own stream.  Why: the interior sweep
 * of a z-slab rank holds every CU of the chip for ≈150 µs per pass (one workgroup per CU), and RCCL's send/recv kernels on the
 * communication stream need CUs to start — the reference reserves `b_width` cells "for comm / comp overlap" (multi.jl:326) and never
 * uses them; this is the knob that makes room on the device instead.  n_cus is spread over the 8 XCDs (rounded up to a multiple
 * of 8, at most half the device).  NS3D_RESERVE_CUS=n presets it for every context created afterwards.  Results do not depend
 * on it.  Cost measured on one MI355X: profiles/r4_cu_mask_ab.log.  ns3d_get_stream returns the stream (wrap it to order other
 * work with it). */
int ns3d_reserve_cus(ns3d_ctx *ctx, int n_cus);
int ns3d_reserved_cus(const ns3d_ctx *ctx);
void *ns3d_get_stream(ns3d_ctx *ctx);
int ns3d_sync(ns3d_ctx *ctx);
/* Tuning knob for the fused PT sweep (0 = default); see DESIGN.md. */
int ns3d_set_pt_variant(ns3d_ctx *ctx, int variant);
/* Temporal blocking: ns3d_pt_iterate / ns3d_pt_solve advance SEVERAL PT iterations per pass over memory where the
 * schedule allows it (same results): two (this knob), or three / four on large grids where the plan phase measures a gain
 * (ns3d_set_pt_depth, ns3d_set_ptn_variant below).  variant < 0 disables, 0 = automatic; otherwise shape*100 + kz with the tile
 * shapes of DESIGN.md §4.2 and kz = planes per z-chunk (1..89 literal; 0 or 91..99: as many chunks as fill two /
 * kz-90 whole rounds of workgroups on the chip).  The environment variable NS3D_PT2_VARIANT presets it at ns3d_create. */
int ns3d_set_pt2_variant(ns3d_ctx *ctx, int variant);
/* Tile shape of the two-iteration sweep when no explicit variant is set: with autotune on (the default) the first
 * launch on a grid of >= 1.5 M cells times the candidate shapes on the caller's own arguments (the operation is idempotent,
 * every shape gives the same bits) and the process remembers the winner per device and grid; that first call therefore
 * synchronises the stream.  Off: a built-in choice by grid size.  ns3d_last_pt2_variant: the variant of the latest two-iteration launch
 * (0 = built-in choice). */
/* N-iteration sweep (ns3d_pt_sweepn): variant = shape*100 + kz.  Shapes (columns per workgroup): 1: 64×32 (512 threads, four
 * rows per thread), 2: 128×16, 6: 64×16 with 256-thread workgroups; +10 (11, 12, 16): the next step's loads issued before level 1;
 * 22: fp32 only, 64×48 with 768 threads; 23 / 28: 64×24 with 768 threads and two rows per thread (three waves per SIMD; loads
 * before level 1 / between the levels); 24: fp32 only, 64×32 with 1024 threads.  kz as above (0: chosen per launch).  0 = built-in.
 * A shape that cannot hold `nlev` levels (tile too small, LDS) or does not exist for the element type makes the call fail. */
int ns3d_set_ptn_variant(ns3d_ctx *ctx, int variant);
/* PT iterations per pass over memory in ns3d_pt_iterate / ns3d_pt_solve: 0 = automatic, 1…4 forced (same results); 5 is
 * available with float32 fields only (k_pt_sweepN has registers for a fifth level there and nowhere else). */
int ns3d_set_pt_depth(ns3d_ctx *ctx, int depth);
int ns3d_set_autotune(ns3d_ctx *ctx, int on);
int ns3d_last_pt2_variant(const ns3d_ctx *ctx);
int ns3d_last_ptn_variant(const ns3d_ctx *ctx);   /* tile variant of the latest N-iteration launch */
int ns3d_last_pt_depth(const ns3d_ctx *ctx);      /* PT iterations of the latest multi-iteration pass; after ns3d_plan_pt: the planned depth */
/* Which of the four compilations of the kernels a call with these grid spacings runs on this context: 0 = `strict` (plain IEEE
 * divisions), 1 = `strictx` (same bits, divisions by the spacings through the correctly rounded divisor-known-in-advance sequence),
 * 3 = `strictp` (same bits; every spacing a power of two, x/d = x*(1/d) exactly), 2 = `fast` (reciprocals + FMA, NS3D_FAST).
 * The reference has no counterpart (its arithmetic is whatever Julia emits for `x/dx/dx`, multi.jl:71); reported by bench.py. */
int ns3d_arith_build(const ns3d_ctx *ctx, double dx, double dy, double dz);
/* ns3d_pt_solve replays each residual-check block (nchk iterations) as one HIP graph: -1 = automatically on
 * launch-bound grids (< 3 M cells), 0 = never, 1 = always.  Same results either way. */
int ns3d_set_graph_mode(ns3d_ctx *ctx, int mode);
/* ns3d_pt_iterate / ns3d_pt_solve on launch-bound grids: a whole block of iterations (up to the next residual check) in ONE
 * cooperative launch that keeps the grid on the chip (k_pt_persist: a cell per thread, faces handed between workgroups through
 * global memory after every iteration): -1 = automatically where it was measured to win (up to 170 000 cells, nx <= 66, no
 * explicit depth / tile / graph request) and the workgroups fit the chip together, 0 = never, 1 = wherever they fit.  Same
 * results either way.  A hand-over that never arrives (bounded wait: the workgroups were not all resident at once — another context
 * or process holding CUs) voids that launch only: it writes its outputs to buffers of its own, the library reads the launch's error
 * word where it synchronises anyway (the residual read-back of ns3d_pt_solve; ns3d_pt_iterate synchronises once for it), redoes
 * the block by launches from the untouched inputs and leaves the cooperative form off for this context; ns3d_persist_faults counts
 * such launches.  (NS3D_COOP_CHECK=1: the launch itself blocks, checks and fails with NS3D_ERR_HIP instead.)  Env NS3D_PT_PERSIST sets the default. */
int ns3d_set_persist_mode(ns3d_ctx *ctx, int mode);
int ns3d_persist_faults(const ns3d_ctx *ctx);
/* Shape 29 of the N-iteration sweep (variant 29xx) is shape 28 whose workgroups re-align in z: the tiles of one XCD meet every pace_z
 * z-steps at a bounded wait, so that the rows neighbouring tiles both read are still in that XCD's L2.  A hint — results never depend
 * on it — used only when all workgroups of the launch are resident together (one z-chunk, no tile window, not during stream capture).
 * ns3d_set_pt_pace: -1 automatic (the planner's value, grids from 3 M cells), 0 off, otherwise a multiple of 4.
 * ns3d_last_pt_pace: the pace_z the latest N-iteration launch really used, 0 when it was not paced.
 * ns3d_set_pt_pace_test (tests): raise every wait's target by extra_arrivals and bound it by `ticks` shader clocks (<= 0: the default). */
int ns3d_set_pt_pace(ns3d_ctx *ctx, int pace_z);
int ns3d_last_pt_pace(const ns3d_ctx *ctx);
int ns3d_set_pt_pace_test(ns3d_ctx *ctx, int extra_arrivals, int ticks);
int ns3d_cached_graphs(const ns3d_ctx *ctx);      /* residual-check blocks this context holds as instantiated HIP graphs */
/* Which advection ns3d_time_step runs in place of {X_o .= X; advect!}.  NS3D_ADVECT_REFERENCE (the default): ns3d_copy_advect, the
 * reference's first-order semi-Lagrangian step.  NS3D_ADVECT_MACCORMACK: {ns3d_copy_advect(faithful = 0) into hat fields held in the
 * context's scratch; ns3d_advect_correct; swap all four names} — the limited second-order scheme defined at ns3d_advect_mc, one rank;
 * ns3d_time_step then requires p->faithful == 0 (NS3D_ERR_ARG otherwise, the fields untouched).  ns3d_advection returns the setting
 * (-1 for a null context).  Nothing else reads the knob: the single calls are what their names say. */
#define NS3D_ADVECT_REFERENCE 0
#define NS3D_ADVECT_MACCORMACK 1
int ns3d_set_advection(ns3d_ctx *ctx, int scheme);
int ns3d_advection(const ns3d_ctx *ctx);
/* What ns3d_time_step masks with.  NULL (the default): set_cylinder! with the scalars of ns3d_step_params.  A mask (device memory, the
 * bytes ns3d_voxelize writes for the grid the step is called on; the caller keeps it alive): ns3d_set_solid with it in place of BOTH
 * set_cylinder! calls of the step, in either script; the cylinder scalars of ns3d_step_params are then ignored.  ns3d_obstacle returns
 * the setting (NULL for a null context).  Nothing else reads the knob: the single calls are what their names say. */
int ns3d_set_obstacle(ns3d_ctx *ctx, const unsigned char *mask);
const unsigned char *ns3d_obstacle(const ns3d_ctx *ctx);
/* The rigid motion of the obstacle ns3d_time_step masks with (outside parity, like the knobs around it).  NULL motion9 (the default)
 * clears the setting: the step issues exactly the calls described above.  motion9 = U[3], omega[3], centre[3] as ns3d_set_solid_moving
 * takes them, origin (may be NULL: zeros) likewise: the context COPIES the twelve numbers and keeps no pointer.  While the setting is
 * on, the step calls ns3d_set_solid_moving through the public entry point at BOTH masking places, in either script, with the mask of
 * ns3d_set_obstacle, these numbers and the spacings of ns3d_step_params; with no mask set the step returns NS3D_ERR_ARG before anything
 * is enqueued, the fields untouched.  Between steps the caller may rewrite the BYTES of the mask it registered (ns3d_voxelize into the
 * same buffer, on the context's stream: a body that moves through the grid) and call this again with the pose's numbers; the address
 * stays registered.  ns3d_set_obstacle does not touch the setting, and nothing but ns3d_time_step reads it.  ns3d_obstacle_motion
 * returns 1 (and the nine numbers in out9, which may be NULL) or 0, -1 for a null context.
 * NS3D_ERR_ARG, the setting unchanged: a null context, a number that is not finite, a negative origin entry. */
int ns3d_set_obstacle_motion(ns3d_ctx *ctx, const double *motion9, const int *origin);
int ns3d_obstacle_motion(const ns3d_ctx *ctx, double *out9);
/* The subgrid-scale model of ns3d_time_step's predictor (outside parity with the reference, like the two knobs above).
 * NS3D_TURB_NONE (the default): the step's first two statements are update_τ! (if write_stress) and ns3d_predict_fused with the scalar
 * μ of ns3d_step_params — not one extra call.  NS3D_TURB_SMAGORINSKY: they are replaced, through the public entry points, by
 *   ns3d_eddy_viscosity into mu_e, with μ, ρ and the spacings of ns3d_step_params and this `length` (ℓ = C_s·Δ; a caller forms it as
 *   C_s·(dx·dy·dz)^(1/3));  ns3d_update_tau_var if write_stress;  ns3d_predict_var.
 * mu_e is CALLER-OWNED device memory of nx·ny·nz elements of the element type the step is called with; the caller keeps it alive, and
 * may read it after the step (it then holds the field the step's predictor used).  The context keeps no scratch for it and there is no
 * accessor.  NS3D_TURB_NONE ignores `length` and `mu_e` and clears the setting.  The step runs on ONE rank: the boundary layer of
 * cells where the model is off would sit at the seams of a decomposed grid.  ns3d_turbulence returns the model (-1 for a null context).
 * Nothing else reads the knob: the single calls are what their names say.
 * NS3D_ERR_ARG, the setting unchanged: a null context, an unknown model, a length that is negative or not finite, a null mu_e with a
 * model. */
enum { NS3D_TURB_NONE = 0, NS3D_TURB_SMAGORINSKY = 1 };
int ns3d_set_turbulence(ns3d_ctx *ctx, int model, double length, void *mu_e);
int ns3d_turbulence(const ns3d_ctx *ctx);
/* The differential operator the step forms mu_e with WHILE ns3d_set_turbulence has a model set (codes and expressions at
 * ns3d_sgs_viscosity).  NS3D_SGS_SMAGORINSKY (the default of a fresh context): the step's first statement is the ns3d_eddy_viscosity
 * call described above, and nothing else.  NS3D_SGS_WALE, NS3D_SGS_VREMAN: it is ns3d_sgs_viscosity with that operator and the same
 * arguments; `length` of ns3d_set_turbulence is then C_w·Δ or √c_v·Δ.  The operator is a setting of its own, not a model code: a
 * plain int that holds no scratch.  ns3d_set_turbulence(NS3D_TURB_NONE) does NOT touch it — the step then ignores it — and
 * ns3d_set_turbulence with a model does not either.  ns3d_sgs_operator returns the setting (-1 for a null context).  Nothing but
 * ns3d_time_step reads the knob.  NS3D_ERR_ARG, the setting unchanged: a null context, an unknown operator. */
enum { NS3D_SGS_SMAGORINSKY = 0, NS3D_SGS_WALE = 1, NS3D_SGS_VREMAN = 2 };
int ns3d_set_sgs_operator(ns3d_ctx *ctx, int op);
int ns3d_sgs_operator(const ns3d_ctx *ctx);
/* The active scalar of ns3d_time_step (outside parity, like the knobs above): diffusion of C and Boussinesq buoyancy.  on = 0 (the
 * default) clears the setting: C is the passive dye of the reference and the step makes not one extra call.  on != 0: the step calls
 * ns3d_scalar_step (below) through the public entry point BEHIND the predictor's name swap and BEFORE the first set_cylinder! /
 * ns3d_set_solid, in either script: from C into the C_o buffer of ns3d_step_fields — it must then be given —, with Vz the freshly
 * predicted field, kappa, bg and c_ref of this call and dt, the spacings and μ of ns3d_step_params; C and C_o then swap names.  The
 * masking call that follows re-imposes C = 1 in the body: the body is a Dirichlet wall of the scalar.  sct is the turbulent Schmidt
 * number: while ns3d_set_turbulence has a model set and sct > 0 the step passes that model's mu_e (the field its predictor used) and
 * sgs = 1/(ρ·sct); otherwise NULL and 0.  bg = g·β is formed by the caller.  The settings are plain numbers: no scratch, no accessor
 * beyond ns3d_scalar, which returns 1 / 0 (-1 for a null context).  ns3d_set_turbulence does not touch them.  One rank: C's halo
 * would have to be exchanged between the advection and this call.  Nothing but ns3d_time_step reads the knob.  The explicit limit
 * dt·K·(1/dx² + 1/dy² + 1/dz²) ≤ 1/2 is the caller's to keep (the Python drivers check the molecular part before a run).
 * NS3D_ERR_ARG, the setting unchanged: a null context; kappa < 0 or sct < 0; any value not finite. */
int ns3d_set_scalar(ns3d_ctx *ctx, int on, double kappa, double sct, double bg, double c_ref);
int ns3d_scalar(const ns3d_ctx *ctx);

/* Parameters of the fused pseudo-transient path (ns3d_pt_iterate / ns3d_pt_solve). */
typedef struct ns3d_pt_params {
    double rho, dt, dtau, damp; /* update_dPrdτ!(…,ρ,dt,dτ,damp,…)  multi.jl:70 */
    double dx, dy, dz;
    int nx, ny, nz;             /* local cell grid */
    int bc_kind;                /* NS3D_BC_MULTI | NS3D_BC_GPU */
    int owns_outlet;            /* multi.jl:179  `xve_g == lx/2`  → Pr[end,:,:] = outlet_val */
    double outlet_val;          /* multi.jl:463  0.0 */
    double g;                   /* gpu.jl:284 bc_xhydstatic!(Pr,dz,nz,g,ρ) */
    int z_lo_is_halo;           /* z-slab seams: plane 1 / plane nz belong to the neighbour rank and are */
    int z_hi_is_halo;           /*   filled by the halo exchange instead of bc_z! (multi.jl:182)        */
} ns3d_pt_params;

/* One whole time step in ONE call (round 4): ns3d_time_step enqueues multi.jl:449-477 (one rank) or gpu.jl:121-142 — predictor,
 * set_cylinder!, update_∇V!, the pressure solve, correct_V!, set_cylinder!, set_bc_Vel!, {X_o .= X; advect!} — on the context's
 * stream in its fused form (ns3d_predict_fused, ns3d_pt_solve, ns3d_copy_advect); the residual read-backs of the pressure loop are
 * its only synchronisations.  The fields are device pointers to the reference's arrays (multi.jl:343-360); the struct is IN/OUT:
 * the fused step swaps the roles of X and X_o instead of copying (multi.jl:475 `X_o .= X` becomes a change of names), so after the
 * call `Vx` is the current field and `Vx_o` the previous one, wherever they live.  In `faithful` mode Vz is never advected
 * (App. B1): it keeps its buffer, and Vz_o is what the caller brings up to date once at the end of a run (ns3d_copy).  The stress
 * arrays may be NULL unless write_stress is set (the reference's τ after its last step).  Results: those of the same sequence
 * of single calls, bit for bit (tests/test_gpu_driver.py). */
typedef struct ns3d_step_fields {
    void *Pr, *dPrdtau, *divV;
    void *Vx, *Vy, *Vz, *Vx_o, *Vy_o, *Vz_o, *C, *C_o;
    void *txx, *tyy, *tzz, *txy, *txz, *tyz;
} ns3d_step_fields;
typedef struct ns3d_step_params {
    int script;                 /* NS3D_BC_MULTI: multi.jl:449-477 on one rank; NS3D_BC_GPU: gpu.jl:121-142 */
    int nx, ny, nz;
    double mu, rho, g, dt, dtau, damp, dx, dy, dz;
    double eps; int niter, nchk; double err_mul, err_div;    /* multi.jl:458-471: err = max|Rp|·err_mul/err_div (ly², psc) */
    double a2, b2, ox, oy, sinb, cosb;                       /* set_cylinder! */
    double xco_g, yco_g, zco_g;                              /*   multi.jl form: global coordinates of the rank's first cell centre */
    double lx, ly, lz;
    int owns_inlet, owns_outlet; double vin;                 /* multi.jl:164,179 */
    int faithful;               /* advect!'s third branch as committed (1) or re-writing Vz (0) */
    int pressure;               /* 0: the PT loop (parity); 1: ns3d_poisson_direct (outside parity) */
    int write_stress;           /* also run update_τ! into txx … tyz (the reference's state after its last step) */
} ns3d_step_params;

/* ns3d_diagnostics: what a run reports about itself, in ONE read-only pass over Vx, Vy, Vz, Pr, C where they live (nothing is
 * stored into the fields, no full-size scratch).  Every quantity covers the part of the arrays this rank OWNS, so that P ranks
 * count the global array exactly once: in a decomposed dimension an array of extent n+s (s = 0 cell-centred, 1 staggered)
 * overlaps its neighbour by 2+s entries; at an interior seam (seam_lo / seam_hi) a rank leaves out its first 1+s entries on the
 * low side and its last entry (the halo) on the high side — owned 0-based range [seam_lo ? 1+s : 0, seam_hi ? n+s-1 : n+s) —
 * and physical ends are counted in full.
 *   vmax[q]      maximum(abs.(Vx)) / Vy / Vz over the owned entries, NaN-propagating like ns3d_max_abs
 *   div_max      max|∇V| over the interior cells (@inn(∇V): 1 ≤ i ≤ n−2 per direction, which partition the global interior whatever
 *                the seam flags), ∇V formed on the fly with ns3d_update_divV's expression and arithmetic build; NaN-propagating
 *   pr_min/max   over the owned cells, NaN-propagating               c_vol   Σ C·dx·dy·dz over the owned cells
 *   ke           Σ ½ρ(u²+v²+w²)·dx·dy·dz over the owned cells, u = 0.5·(Vx[i,j,k]+Vx[i+1,j,k]) etc.; terms and sums in fp64
 *   mom[q], n_masked[q]   Σ Vx (Vy, Vz) over the owned nodes set_cylinder!'s velocity test q < 1.0 selects at that field's own
 *                stagger location — what the next set_cylinder! call zeroes — and their number; 0 unless `cylinder` is set
 *                (1: the predicate of ns3d_set_cylinder, multi.jl:249-281; 2: ns3d_set_cylinder_local, gpu.jl:336-368)
 *   nonfinite    1 if an owned entry of any of the five arrays is NaN or ±Inf.  ke and div_max read one entry beyond the owned
 *                ones where a low side is a seam (the staggered entry 1 of Vx / Vy / Vz in that direction, which the lower
 *                neighbour owns and reports): a NaN only there reaches this rank's ke / div_max without setting its flag —
 *                with consistent halos the neighbour's flag and the global record carry it
 * The sums are reduced in a fixed order (per thread down its planes, wave64 butterfly, one LDS slot per wave, per-workgroup
 * partials in the context's scratch, a second small launch over the partials): two calls on the same input return the same
 * bits.  fp32 fields are converted on load and reduced in fp64. */
typedef struct ns3d_diag {
    double vmax[3], div_max, pr_min, pr_max, ke, c_vol, mom[3];
    long long n_masked[3];
    int nonfinite;
} ns3d_diag;
typedef struct ns3d_diag_params {
    int nx, ny, nz;
    double dx, dy, dz, rho;
    int seam_lo[3], seam_hi[3]; /* side is an interior seam (ignored by the mgpu form: set per rank inside) */
    int cylinder;               /* 0 none | 1 multi.jl form | 2 gpu.jl form */
    double a2, b2, ox, oy, sinb, cosb, xco_g, yco_g, zco_g, lx, ly, lz;
} ns3d_diag_params;

/* Running statistics: the companion of the monitor above — that one gives the time series, this one the time-averaged FIELDS
 * (mean velocity and pressure, the Reynolds stresses u'u' … v'w', the pressure variance).  The caller owns the state S: a `double`
 * device array of NS3D_STATS_SLOTS consecutive column-major blocks of extent (nx,ny,nz), one per slot below, fp64 whatever the
 * element type of the fields.  The cell-centred values are those of the monitor's kinetic energy,
 *     u = 0.5·(Vx[i,j,k] + Vx[i+1,j,k])   v = 0.5·(Vy[i,j,k] + Vy[i,j+1,k])   w = 0.5·(Vz[i,j,k] + Vz[i,j,k+1])   p = Pr[i,j,k]
 * (fp32 fields are converted on load, everything after that is fp64).  EVERY cell of the local array is accumulated, halo and
 * boundary cells included: a rank's S has the shape of a cell-centred field, and ns3d_gather_f64 assembles the global,
 * halo-stripped statistics of a multi-rank run unchanged.  There is no ns3d_mgpu form: a multi-rank caller makes the calls below
 * on the context of each local rank (ns3d_mgpu_ctx), like every once-per-step kernel, and gathers the blocks of `mean` / `rs`.
 * Read-only with respect to the flow. */
enum {
    NS3D_STATS_U = 0,
    NS3D_STATS_V = 1,
    NS3D_STATS_W = 2,
    NS3D_STATS_P = 3,
    NS3D_STATS_UU = 4,
    NS3D_STATS_VV = 5,
    NS3D_STATS_WW = 6,
    NS3D_STATS_UV = 7,
    NS3D_STATS_UW = 8,
    NS3D_STATS_VW = 9,
    NS3D_STATS_PP = 10,
    NS3D_STATS_SLOTS = 11
};
/* S = 0 (all NS3D_STATS_SLOTS blocks) on the context's stream. */
int ns3d_stats_reset(ns3d_ctx *, double *S, int nx, int ny, int nz);
/* From sums to statistics: `mean` receives 4 blocks S[q]/wsum (q = U, V, W, P), `rs` — 7 blocks, may be NULL — the blocks
 * S[UU … VW]/wsum − ā·b̄ of the six velocity pairs in slot order, then S[PP]/wsum − p̄·p̄ (ā, b̄, p̄: the entries of `mean`).  The
 * division is the plain IEEE quotient; product and subtraction are not contracted in STRICT.  wsum is the sum of the weights
 * accumulated so far.  NS3D_ERR_ARG: null context / S / mean, a grid below 3×3×3, wsum not finite or not greater than 0. */
int ns3d_stats_finalize(ns3d_ctx *, const double *S, double wsum, double *mean, double *rs, int nx, int ny, int nz);

/* Obstacles from triangle meshes: the way back from a closed triangle surface (what ns3d_isosurface emits) to the four staggered
 * masks of set_cylinder!, made on the device.  The masking method needs no more than the analytic test replaced by a stored one.
 * THE MASK is one unsigned char per point of set_cylinder!'s thread range (nx+1, ny+1, nz+1), column-major, x fastest:
 *   bit 0  C   cell centre (i+.5, j+.5, k+.5)   valid for i<nx, j<ny, k<nz        bit 1  Vx  (i, j+.5, k+.5)   valid for j<ny, k<nz
 *   bit 2  Vy  (i+.5, j, k+.5)                  valid for i<nx, k<nz              bit 3  Vz  (i+.5, j+.5, k)   valid for i<nx, j<ny
 * Positions are in the index space of ns3d_sample: the cell grid occupies [0,nx] x [0,ny] x [0,nz].  Bits at invalid points and bits
 * 4-7 are always 0; one call writes the mask completely.
 * ns3d_voxelize: tri holds 9 doubles per triangle (x0,y0,z0,x1,y1,z1,x2,y2,z2), fp64 whatever the fields are.  origin (may be NULL:
 * zeros) is three ints: the sample point of local (i,j,k) is (double)(i+origin_x) + s, likewise in y and z, s = 0 or 0.5 — exact, so
 * the ranks of a decomposed grid, each with origin[q] = co[q]*(n[q]-2), compute identical bits at the entries they duplicate.  The
 * mesh must be closed; orientation is not used; an open mesh gives a well-defined but meaningless mask.
 * A sample point is INSIDE if a ray from it towards -x crosses the surface an odd number of times.  Every decision is a stated fp64
 * comparison and nothing is contracted, in any build: STRICT, NS3D_IEEE_DIV and FAST contexts return the same bytes.  For a row
 * r = (y, z) and a triangle (a, b, c) as stored:
 *   side(p, q, r) on the yz-projections: if (q.y, q.z) < (p.y, p.z) lexicographically, it is -side(q, p, r).  Otherwise dy = q.y-p.y,
 *     dz = q.z-p.z, E = dy*(r.z-p.z) - dz*(r.y-p.y); +1 if E > 0, -1 if E < 0, and if E == 0 the tie dz>0 ? -1 : dz<0 ? +1 : dy>0 ? +1 : 0
 *     (the sign of E at r + (eps, eps^2)).  An edge shared by two triangles is evaluated from the same ordered end points by both: a
 *     point on the edge belongs to exactly one of them.
 *   the triangle COVERS r when its nine coordinates are finite, min y <= r.y <= max y and min z <= r.z <= max z over its vertices (by
 *     comparisons), and side(a,b,r) == side(b,c,r) == side(c,a,r) != 0.
 *   CROSSING: u = b-a, v = c-a, n = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x),
 *     xs = a.x - (n.y*(y - a.y) + n.z*(z - a.z))/n.x with a plain IEEE quotient; the triangle is ignored for this row if n.x == 0 or xs
 *     is not finite.
 *   FLIP: for a sample family with x positions (i + origin_x) + s, 0 <= i < ext: t = xs - (double)(origin_x + s),
 *     i0 = t <= 0 ? 0 : t >= ext ? ext : (int)ceil(t); every sample i >= i0 flips (a sample exactly on the surface counts as beyond it).
 *   A bit is the parity of the flips of all triangles.
 * Row families (with an origin the rows are (j+origin_y ..., k+origin_z ...)): (j+.5, k+.5) serves bit 0 with s = .5, ext = nx and bit 1
 * with s = 0, ext = nx+1 (one cover test, two flips); (j, k+.5) serves bit 2 and (j+.5, k) bit 3, both with s = .5, ext = nx.
 * For an axis-parallel box with faces on sample points the set is half-open: lo <= p < hi in every direction.  In general a sample on
 * the surface is decided as the point (x + d, y + eps, z + eps^2) with d >> eps: first along +x, then +y, then +z.
 * As NumPy, for the rows Y, Z (1, R) of a family and the triangles' coordinate columns ax ... cz (T, 1), all float64:
 *   def side(py, pz, qy, qz):
 *       sw = (qy < py) | ((qy == py) & (qz < pz));  ay, az, by, bz = where(sw, qy, py), where(sw, qz, pz), where(sw, py, qy), where(sw, pz, qz)
 *       dy, dz = by - ay, bz - az;  E = dy*(Z - az) - dz*(Y - ay)
 *       s = where(E > 0, 1, where(E < 0, -1, where(dz > 0, -1, where(dz < 0, 1, where(dy > 0, 1, 0)))));  return where(sw, -s, s)
 *   cover = finite & (miny <= Y) & (Y <= maxy) & (minz <= Z) & (Z <= maxz) & (s1 == s2) & (s2 == s3) & (s1 != 0)
 *   xs = ax - (n_y*(Y - ay) + n_z*(Z - az))/n_x;  hit = cover & (n_x != 0) & isfinite(xs);  t = xs - (origin_x + s)
 *   i0 = where(t <= 0, 0, where(t >= ext, ext, ceil(t)));  bit[i, row] = (number of hits of the row with i0 <= i) & 1
 * (tests/solid_ref.py is this statement.)  Two calls on the same input return the same bytes, and permuting the triangles changes
 * nothing: each covered (triangle, row) XORs one bit into a packed bit plane of the context's scratch — four planes of (ny+1)(nz+1)
 * rows x ceil((nx+2)/32) words, grown lazily and zeroed on the context's stream — and a prefix parity along x makes the bytes.  The
 * call only enqueues (it blocks as every call does without NS3D_ASYNC).  n_tri == 0 writes an all-zero mask.
 * NS3D_ERR_ARG, with nothing written: a null context, a null mask, a null tri with n_tri > 0, n_tri < 0, a grid below 3x3x3, a negative
 * origin entry. */
int ns3d_voxelize(ns3d_ctx *, unsigned char *mask, const double *tri, long long n_tri, int nx, int ny, int nz, const int *origin);
/* A rigid motion in PHYSICAL space applied to a mesh stored in INDEX space (ns3d_voxelize's tri layout; a rotation is not rigid in
 * index space when the spacings differ).  R is a 3x3 matrix, row-major; pivot and shift are in index units; spacing = dx, dy, dz.  Per
 * vertex p and output component a, with q_b = (p_b - pivot_b)*d_b, all fp64, nothing contracted, the quotient the plain IEEE one:
 *   out_a = (pivot_a + shift_a) + ((R[a][0]*q_x + R[a][1]*q_y) + R[a][2]*q_z) / d_a
 * As NumPy, for P of shape (n, 3): q = (P - pivot)*d;  out = (pivot + shift) + ((R[:,0]*q[:,:1] + R[:,1]*q[:,1:2]) + R[:,2]*q[:,2:])/d.
 * STRICT, NS3D_IEEE_DIV and FAST contexts return the same bits.  Coordinates that are not finite propagate (ns3d_voxelize ignores such
 * triangles).  out == tri is allowed (a vertex is read whole before it is stored); any other overlap of the two ranges of 72*n_tri
 * bytes is refused.  n_tri == 0 is a no-op that returns NS3D_OK (out and tri may then be NULL).  Device memory only; enqueued on the
 * context's stream, no scratch, no read-back.  A pose is applied to the ORIGINAL mesh with the accumulated rotation and shift, never
 * to the previous pose's output: a mask at step s then does not depend on how many steps preceded it.
 * NS3D_ERR_ARG, with nothing written: a null context; n_tri < 0; a null R, pivot, shift or spacing; one of their numbers not finite; a
 * spacing not > 0; a null out or tri with n_tri > 0; buffers that overlap without being equal. */
int ns3d_mesh_transform(ns3d_ctx *, double *out, const double *tri, long long n_tri, const double *R, const double *pivot,
                        const double *shift, const double *spacing);

#define NS3D_DECL(T, S)                                                                                     \
    /* One sample: per cell and slot S = S + weight·term, term = u, v, w, p, u·u, v·v, w·w, u·v, u·w, v·w, p·p evaluated in   \
     * exactly that written order (STRICT: no contraction — the bits of the same NumPy expression; FAST may contract).  One   \
     * pass that reads the four fields once and updates the accumulators in place.  Pr may be NULL: the slots P and PP are    \
     * then neither read nor written.  Enqueued on the context's stream, no read-back (blocks only as every call does          \
     * without NS3D_ASYNC).  NS3D_ERR_ARG: null context / S / velocity, a grid below 3×3×3, a weight that is not finite. */    \
    int ns3d_stats_accumulate_##S(ns3d_ctx *, double *S_, const T *Vx, const T *Vy, const T *Vz, const T *Pr,  \
                                  double weight, int nx, int ny, int nz);                                    \
    /* Vorticity and Q-criterion: the third observer — what one looks at in a cylinder wake.  Four cell-centred (nx,ny,nz)    \
     * fields of the element type T, formed in ONE pass over Vx, Vy, Vz.  All arithmetic is in T, like ns3d_update_divV and   \
     * unlike the statistics: h = (T)0.5, and dx, dy, dz are converted to T on entry.                                         \
     *   cell-centred velocities   u = h·(Vx[i,j,k] + Vx[i+1,j,k])   v = h·(Vy[i,j,k] + Vy[i,j+1,k])   w = h·(Vz[i,j,k] + Vz[i,j,k+1]) \
     *   diagonal of ∇V (update_∇V!'s terms)   gxx = (Vx[i+1,j,k] − Vx[i,j,k])/dx   gyy = (Vy[i,j+1,k] − Vy[i,j,k])/dy      \
     *                                         gzz = (Vz[i,j,k+1] − Vz[i,j,k])/dz                                              \
     *   off-diagonal entries, central differences of the cell-centred values                                                 \
     *     uy = h·((u[i,j+1,k] − u[i,j−1,k])/dy)   uz = h·((u[i,j,k+1] − u[i,j,k−1])/dz)   vx = h·((v[i+1,j,k] − v[i−1,j,k])/dx) \
     *     vz = h·((v[i,j,k+1] − v[i,j,k−1])/dz)   wx = h·((w[i+1,j,k] − w[i−1,j,k])/dx)   wy = h·((w[i,j+1,k] − w[i,j−1,k])/dy) \
     *   Wx = wy − vz     Wy = uz − wx     Wz = vx − uy                                                                        \
     *   Q  = ((−h)·((gxx·gxx + gyy·gyy) + gzz·gzz)) − ((uy·vx + uz·wx) + vz·wy)                                              \
     * (Q = −½·G_ij·G_ji = ½(‖Ω‖² − ‖S‖²) whatever ∇·V is; the parentheses are as written.)  As NumPy, on arrays of dtype T   \
     * with h, dx, dy, dz scalars of that dtype, I = [1:-1,1:-1,1:-1]:                                                         \
     *   u = h*(Vx[:-1] + Vx[1:]);  v = h*(Vy[:,:-1] + Vy[:,1:]);  w = h*(Vz[:,:,:-1] + Vz[:,:,1:])                           \
     *   gxx = ((Vx[1:] − Vx[:-1])/dx)[I];  gyy = ((Vy[:,1:] − Vy[:,:-1])/dy)[I];  gzz = ((Vz[:,:,1:] − Vz[:,:,:-1])/dz)[I]   \
     *   uy = h*((u[1:-1,2:,1:-1] − u[1:-1,:-2,1:-1])/dy);  uz = h*((u[1:-1,1:-1,2:] − u[1:-1,1:-1,:-2])/dz)                  \
     *   vx = h*((v[2:,1:-1,1:-1] − v[:-2,1:-1,1:-1])/dx);  vz = h*((v[1:-1,1:-1,2:] − v[1:-1,1:-1,:-2])/dz)                  \
     *   wx = h*((w[2:,1:-1,1:-1] − w[:-2,1:-1,1:-1])/dx);  wy = h*((w[1:-1,2:,1:-1] − w[1:-1,:-2,1:-1])/dy)                  \
     *   Wx[I] = wy − vz;  Wy[I] = uz − wx;  Wz[I] = vx − uy                                                                   \
     *   Q[I] = ((−h)*((gxx*gxx + gyy*gyy) + gzz*gzz)) − ((uy*vx + uz*wx) + vz*wy)                                            \
     * Interior cells (1 ≤ i ≤ nx−2, the same in y and z) receive these values, EVERY other entry +0.0: one call writes an    \
     * output completely.  STRICT returns the bits of that expression (float64 and float32, no contraction, whichever of the  \
     * three division builds the spacings select; NS3D_IEEE_DIV is honoured); FAST multiplies by reciprocals and may contract. \
     * Any of Wx, Wy, Wz, Q may be NULL — it is then neither computed nor stored — but not all four.  Outputs must not alias   \
     * the inputs or each other.  Enqueued on the context's stream, no read-back (blocks only as every call does without       \
     * NS3D_ASYNC).  The interior of a rank needs only that rank's own arrays with their one-cell halo, so there is no        \
     * ns3d_mgpu form: a multi-rank caller makes this call on each local rank's context (ns3d_mgpu_ctx) after the step's last \
     * halo update, and ns3d_gather_* assembles the halo-stripped global fields.  The gathered result equals the one-rank      \
     * result wherever the ranks' duplicated velocity entries agree — they do after update_halo! unless several ranks run the \
     * corrected advection (faithful = 0) without the wide halo.                                                   \
     * NS3D_ERR_ARG: null context / velocity pointer, all four outputs NULL, a grid below 3×3×3, a spacing that is not finite  \
     * or not greater than 0; the outputs are then untouched. */                                                              \
    int ns3d_vortex_##S(ns3d_ctx *, T *Wx, T *Wy, T *Wz, T *Q, const T *Vx, const T *Vy, const T *Vz,       \
                        double dx, double dy, double dz, int nx, int ny, int nz);                            \
    /* Point samples and Lagrangian tracers: the observers that do not live on the grid.  Both rest on ONE definition, the \
     * trilinear interpolation of backtrack! (multi.jl:190-214: clamp, floor, lerp(a,b,t) = b*t + a*(1-t), x then y then z), evaluated \
     * at points the caller chooses.  Positions are fp64 and in INDEX space whatever T is: X holds three consecutive blocks of n \
     * doubles, xi | eta | zeta; the cell grid occupies the closed box [0,nx] x [0,ny] x [0,nz], cell centres sit at half-integers, \
     * and a field staggered in a direction has its nodes at the integers of that direction.  `state` is one byte per point: 1 alive, \
     * 0 dead.  Field values are converted to double on load; all arithmetic after that is fp64 and is NEVER contracted, in any \
     * build: STRICT, NS3D_IEEE_DIV and FAST contexts return the same bits (the calls are bound by gather latency, an FMA would buy \
     * nothing, and whether a particle is alive does not depend on the arithmetic mode).  The device performs no division. \
     *   I(A, ext, stag, p), per direction q:   c = p_q - (stag_q ? 0.0 : 0.5);   c = c > 0.0 ? c : 0.0;   c = c < ext_q-1 ? c : ext_q-1 \
     *                                          i0 = min((int)floor(c), ext_q-2);   t = c - i0                            \
     *     (max and min written as comparisons: -0.0 becomes +0.0), then with a_ijk = A[i0+i, j0+j, k0+k]                 \
     *     fy1z1 = lerp(a000,a100,tx)  fy1z2 = lerp(a001,a101,tx)  fy2z1 = lerp(a010,a110,tx)  fy2z2 = lerp(a011,a111,tx) \
     *     fz1 = lerp(fy1z1,fy2z1,ty)  fz2 = lerp(fy1z2,fy2z2,ty)  I = lerp(fz1,fz2,tz)                                   \
     *   velocity at p:   u = I(Vx,(nx+1,ny,nz),(1,0,0),p)   v = I(Vy,(nx,ny+1,nz),(0,1,0),p)   w = I(Vz,(nx,ny,nz+1),(0,0,1),p) \
     * As NumPy, on the points m that are evaluated (X of shape (3,N), A column-major of extents e, s the stagger flags): \
     *   c = [np.where(X[q,m] - (0.0 if s[q] else 0.5) > 0.0, X[q,m] - (0.0 if s[q] else 0.5), 0.0) for q in range(3)]    \
     *   c = [np.where(c[q] < e[q]-1.0, c[q], e[q]-1.0) for q in range(3)]                                                \
     *   i = [np.minimum(np.floor(c[q]).astype(np.int64), e[q]-2) for q in range(3)];  t = [c[q] - i[q] for q in range(3)] \
     *   a = lambda di,dj,dk: A[i[0]+di, i[1]+dj, i[2]+dk].astype(np.float64);  lerp = lambda a,b,t: b*t + a*(1.0-t)      \
     *   fz1 = lerp(lerp(a(0,0,0),a(1,0,0),t[0]), lerp(a(0,1,0),a(1,1,0),t[0]), t[1])                                     \
     *   fz2 = lerp(lerp(a(0,0,1),a(1,0,1),t[0]), lerp(a(0,1,1),a(1,1,1),t[0]), t[1]);   I = lerp(fz1, fz2, t[2])         \
     * ns3d_sample_*: out[p] = I(A, (ex,ey,ez), stag, X_p) for the points that are alive (state NULL: all of them), finite and inside the \
     *   closed box [0, e_q - stag_q] per direction; every other point receives NaN.  One call writes `out` (n doubles) completely; \
     *   X, state and A are read-only.                                                                                    \
     * ns3d_tracers_advance_*: one explicit midpoint (RK2) step through the frozen field; cx, cy, cz are the Courant factors dt/dx, \
     *   dt/dy, dt/dz, formed by the caller in double (backtrack!'s dt*vxc/dx with the division taken out).  A particle is ACTIVE if \
     *   state == 1, its three coordinates are finite and it is inside the closed box.  An inactive particle keeps its coordinates \
     *   bit for bit, its state becomes 0, its U entries NaN.  An active one:                                             \
     *     v1 = V(X);   Xm_q = X_q + 0.5*(v1_q*c_q);   if any Xm_q is not finite: Xn = Xm;   else v2 = V(Xm) (the midpoint may lie \
     *     outside the box: the clamp of I covers that) and Xn_q = X_q + v2_q*c_q.                                        \
     *   Xn is stored even when it lies outside the box (it records where the particle left); state becomes 1 if Xn is finite and \
     *   inside the closed box, else 0.  U may be NULL; otherwise it is three blocks of n doubles and receives v1.  The fields are \
     *   read-only.  X, state and U must not overlap the fields.  Through a field at rest every position keeps its bits, but for a \
     *   coordinate -0.0 of an active particle, which -0.0 + (+0.0) turns into +0.0.                                      \
     * Both are enqueued on the context's stream without a read-back (they block only as every call does without NS3D_ASYNC). \
     * NS3D_ERR_ARG, with every output untouched: a null context, X, field or `out`; a null `state` in the advance; n < 0 (n == 0 is \
     * a successful no-op); a grid below 3x3x3 resp. extents below 2 in the sample; a stagger flag other than 0 or 1; a Courant \
     * factor that is not finite.                                                                                         \
     * Positions are local to the arrays passed in: these two calls know one rank.  On a decomposed grid a particle that crosses a \
     * seam between ranks has to migrate to its neighbour — the _at forms below and the two ns3d_mgpu calls further down are that \
     * design. */                                                                                                         \
    int ns3d_sample_##S(ns3d_ctx *, double *out, const double *X, const unsigned char *state, long n, const T *A, \
                        int ex, int ey, int ez, int stag_x, int stag_y, int stag_z);                          \
    int ns3d_tracers_advance_##S(ns3d_ctx *, double *X, unsigned char *state, double *U, long n, const T *Vx, \
                                 const T *Vy, const T *Vz, double cx, double cy, double cz, int nx, int ny, int nz); \
    /* The ORIGIN forms, for the ranks of a decomposed grid.  X is in the GLOBAL index space of the cell grid \
     * n_g[q] = dims[q]*(n[q]-2)+2, whatever rank holds the particle; the rank with coordinates co has origin[q] = co[q]*(n[q]-2) and \
     * interpolates at p_q = X_q - (double)origin_q — exact for 0 <= origin <= X, so the local node is the global one minus origin \
     * and the weights have the same bits — with the same I as above.                                                       \
     * ns3d_sample_at_*: the sample call evaluated at X - origin; the inside test is the local one, 0 <= p_q <= e_q - stag_q, NaN \
     *   otherwise.  origin NULL means zeros, and then the call returns the bits of the one-rank form.                      \
     * ns3d_tracers_advance_at_*: the advance with its "inside the closed box" tests taken on the GLOBAL box [0, n_g] and the  \
     *   interpolation at X - origin (the midpoint too); Xn, U and the state are stored as above.  origin / n_g NULL mean zeros \
     *   resp. (nx,ny,nz), and then the call returns the bits of the one-rank form.  A live particle the rank does not own is the \
     *   caller's mistake: it is advanced with the clamped interpolation.                                                   \
     * OWNERSHIP, per direction with D = dims[q], n = n[q]: rank coordinate k owns k(n-2)+1 <= X_q < (k+1)(n-2)+1, k = 0 from 0 and \
     * k = D-1 up to n_g inclusive: a partition of the closed global box, decided by comparisons.                          \
     * GUARANTEE (of the form of the wide advection's |dz| < 2 cells): with halos that agree with the global field, P ranks \
     * reproduce the one-rank step bit for bit in X, state and U while every active particle's first-stage Courant number \
     * |v1_q*c_q| is below 1 in the decomposed directions (undecomposed directions are unrestricted).  Beyond that the midpoint is \
     * clamped to the local array, as backtrack! clamps.  No address outside the arrays is ever read.                      \
     * NS3D_ERR_ARG as for the one-rank forms, and for origin_q < 0 or n_g[q] < origin_q + n_q. */                         \
    int ns3d_sample_at_##S(ns3d_ctx *, double *out, const double *X, const unsigned char *state, long n, const T *A, \
                           int ex, int ey, int ez, int stag_x, int stag_y, int stag_z, const int *origin);        \
    int ns3d_tracers_advance_at_##S(ns3d_ctx *, double *X, unsigned char *state, double *U, long n, const T *Vx, \
                                    const T *Vy, const T *Vz, double cx, double cy, double cz, int nx, int ny, int nz, \
                                    const int *origin, const int *n_g);                                        \
    /* Isosurface: the triangles of the level set A = iso, extracted and compacted on the device — what one looks at instead of the field.  \
     * A is any packed column-major array of extents (ex,ey,ez), each >= 2; its entries are NODES at the integer positions (i,j,k) (the     \
     * caller knows where they sit physically: stagger and spacings are applied by the caller).  B (may be NULL) is a second array of the   \
     * same extents whose values are interpolated at the surface's vertices.  box (may be NULL: the whole array) is six ints lo_x, lo_y,    \
     * lo_z, hi_x, hi_y, hi_z, a closed node range with 0 <= lo_q < hi_q <= e_q-1; the CUBES processed are those whose eight corners lie    \
     * in it (lower corner lo_q <= i_q <= hi_q-1).  origin (may be NULL: 0,0,0) is three ints added to the integer node indices BEFORE any  \
     * fractional part, so that the ranks of a decomposed grid emit bit-identical vertices on a shared face.                                \
     * Values are converted to double on load; all arithmetic after that is fp64 and NEVER contracted, in any build: STRICT, NS3D_IEEE_DIV  \
     * and FAST contexts return the same bits, as for ns3d_sample.  The one division per vertex is the plain IEEE quotient.                 \
     * MARCHING TETRAHEDRA on the Kuhn decomposition.  A cube's corners are numbered c = di + 2 dj + 4 dk.  Its six tetrahedra are the      \
     * six axis orders pi in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx; tetrahedron pi has the vertices v0 = corner 0, v1 = v0 +     \
     * e_pi1, v2 = v1 + e_pi2, v3 = corner 7: a componentwise increasing chain, so every tetrahedron edge runs from a node `lo` to a node   \
     * `hi` with hi_q - lo_q in {0,1}, hi being the end with the larger linear index.  The decomposition is the same in every cube:         \
     * neighbouring cubes agree on their shared face diagonals, the surface is watertight.                                                  \
     * A node is INSIDE if a >= iso, else OUTSIDE.  A cube with a non-finite corner (NaN, +-Inf) emits nothing.  iso must be finite.        \
     * VERTEX on an edge with one inside and one outside end, always formed from lo towards hi, whichever tetrahedron or cube asks:         \
     *   t = (iso - a_lo) / (a_hi - a_lo)            (the denominator is never 0)                                                           \
     *   pos_q = (double)(lo_q + origin_q) + (hi_q > lo_q ? t : 0.0)                                                                        \
     *   value = b_hi*t + b_lo*(1.0 - t)              (backtrack!'s lerp)                                                                   \
     * A vertex depends only on its edge: every tetrahedron sharing the edge produces the same bits, a mesh can be indexed by exact         \
     * comparison.  As NumPy, for the cubes with lower corner (I,J,K) (index arrays), a tetrahedron edge from corner clo to corner chi:     \
     *   d = lambda c: ((c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1);  at = lambda F, c: F[I+d(c)[0], J+d(c)[1], K+d(c)[2]].astype(np.float64) \
     *   t = (iso - at(A,clo)) / (at(A,chi) - at(A,clo))                                                                                    \
     *   pos = [((I,J,K)[q] + d(clo)[q] + origin[q]).astype(np.float64) + (t if d(chi)[q] > d(clo)[q] else 0.0) for q in range(3)]          \
     *   value = at(B,chi)*t + at(B,clo)*(1.0 - t)                                                                                          \
     * TRIANGLES per tetrahedron, v0..v3 in the tetrahedron-local order, E(u,v) the vertex on the edge between v_u and v_v:                 \
     *   0 or 4 inside: none.   1 or 3 inside: one; a the single vertex on its side, b < c < d the other three: E(a,b), E(a,c), E(a,d).     \
     *   2 and 2: two; p < q inside, r < s outside: the quad E(p,r), E(p,s), E(q,s), E(q,r) split along E(p,r)-E(q,s) into                  \
     *   (E(p,r), E(p,s), E(q,s)) and (E(p,r), E(q,s), E(q,r)).                                                                             \
     * Each triangle is then oriented so that its right-hand normal points from the inside vertices towards the outside ones (towards       \
     * decreasing A); it is flipped by swapping its last two vertices.  The orientation is COMBINATORIAL: a fixed bit per (tetrahedron,     \
     * case), derived once by evaluating the rule on the unit cube with inside = 1, outside = 0, iso = 0.5, never a floating-point test     \
     * at run time.  A node value equal to iso gives t = 0 or t = 1 and possibly zero-area triangles; they are emitted like any other:      \
     * the count is a function of the inside masks alone.                                                                                   \
     * ORDER: cubes in linear order over the box, x fastest, then y, then z; within a cube tetrahedra 0..5; within a tetrahedron as         \
     * listed.  At most 12 triangles per cube.                                                                                              \
     * OUTPUTS (device memory): tri holds 9 doubles per triangle, x0,y0,z0,x1,y1,z1,x2,y2,z2; val (may be NULL, must be NULL if B is) 3     \
     * doubles per triangle.  *n_tri_host (host memory) receives the number of triangles the surface HAS; the call blocks for this          \
     * read-back like ns3d_diagnostics.  Only the first min(n, cap) triangles, a complete prefix in the order above, are written;           \
     * nothing is written beyond cap triangles.  cap = 0 with tri = NULL is the count-only form.  n > cap is NS3D_OK: the caller            \
     * compares the two numbers.  Two calls on the same input return the same bits in the same order (no atomics decide a position).        \
     * The inputs are read-only.  The context keeps 12 bytes of scratch per row segment of 64 cubes, grown lazily.                          \
     * NS3D_ERR_ARG, with every output and *n_tri_host untouched: a null context, A or n_tri_host; an extent below 2; a box outside the     \
     * array or with hi_q <= lo_q; cap < 0; tri == NULL with cap > 0; val != NULL with B == NULL; iso not finite.                           \
     * There is no ns3d_mgpu form: a rank extracts the cubes it owns with its own box and origin, the pieces are concatenated. */           \
    int ns3d_isosurface_##S(ns3d_ctx *, const T *A, const T *B, int ex, int ey, int ez, const int *box, const int *origin, \
                            double iso, double *tri, double *val, long long cap, long long *n_tri_host);          \
    /* The monitor above on one rank.  Pr or C may be NULL: pr_min / pr_max resp. c_vol then come back as NaN (and take no    \
     * part in `nonfinite`).  Blocks for its read-back like ns3d_max_abs.  NS3D_ERR_ARG: null context / velocity / params /   \
     * output, a grid below 3×3×3, a cylinder form other than 0, 1, 2. */                                    \
    int ns3d_diagnostics_##S(ns3d_ctx *, const T *Vx, const T *Vy, const T *Vz, const T *Pr, const T *C,    \
                             const ns3d_diag_params *p, ns3d_diag *out_host);                               \
    /* the whole step (above); iters_done / err_hist / n_checks as in ns3d_pt_solve */                          \
    int ns3d_time_step_##S(ns3d_ctx *, ns3d_step_fields *f, const ns3d_step_params *p, int *iters_done,        \
                           double *err_hist, int max_checks, int *n_checks);                                   \
    /* update_τ!(τxx,τyy,τzz,τxy,τxz,τyz,Vx,Vy,Vz,μ,dx,dy,dz)      multi.jl:36-44   gpu.jl:177-185 */         \
    int ns3d_update_tau_##S(ns3d_ctx *, T *txx, T *tyy, T *tzz, T *txy, T *txz, T *tyz, const T *Vx,         \
                            const T *Vy, const T *Vz, double mu, double dx, double dy, double dz, int nx,    \
                            int ny, int nz);                                                                 \
    /* predict_V!(Vx,Vy,Vz,τxx,τyy,τzz,τxy,τxz,τyz,ρ,g,dt,dx,dy,dz) multi.jl:50-55   gpu.jl:187-192 */        \
    int ns3d_predict_V_##S(ns3d_ctx *, T *Vx, T *Vy, T *Vz, const T *txx, const T *tyy, const T *tzz,        \
                           const T *txy, const T *txz, const T *tyz, double rho, double g, double dt,         \
                           double dx, double dy, double dz, int nx, int ny, int nz);                         \
    /* {update_τ!; predict_V!} (multi.jl:449,451 / gpu.jl:121-122) in one pass for a driver that does not look at the stress \
     * arrays: reads Vx, Vy, Vz, writes COMPLETE predicted fields into Vx_new, Vy_new, Vz_new (buffers of their own: the     \
     * entries predict_V! leaves alone are written through) — the caller swaps the names.  Bit for bit what the two calls    \
     * leave in Vx, Vy, Vz.  The stresses are not stored.  Not for ranks that exchange τ halos between the two calls with     \
     * velocities that differ across ranks (multi.jl:450). */                                                \
    int ns3d_predict_fused_##S(ns3d_ctx *, T *Vx_new, T *Vy_new, T *Vz_new, const T *Vx, const T *Vy, const T *Vz,          \
                               double mu, double rho, double g, double dt, double dx, double dy, double dz, int nx, int ny,  \
                               int nz);                                                                      \
    /* Smagorinsky's effective viscosity (outside parity): mu_e = μ + ρ·ℓ²·|S|, |S| = √(2 S_ij S_ij), a cell-centred (nx,ny,nz) field \
     * of the element type formed in ONE pass over Vx, Vy, Vz.  `length` is ℓ = C_s·Δ, formed by the caller: no cube root runs on the \
     * device.  The velocity gradient at the cell centre is EXACTLY ns3d_vortex's (above): its diagonal update_∇V!'s terms, its        \
     * off-diagonal entries central differences of the cell-centred averages — |S| and the Q field a user plots agree about what the  \
     * gradient is.  All arithmetic in T: h = (T)0.5, two = (T)2, muT = (T)mu, c = (T)(rho·length·length) (the product in double, one  \
     * conversion), dx, dy, dz converted to T on entry.  As NumPy, with I = [1:-1,1:-1,1:-1]:                                          \
     *   u, v, w, gxx, gyy, gzz, uy, uz, vx, vz, wx, wy      as in ns3d_vortex's NumPy statement, verbatim                             \
     *   a = uy + vx;  b = uz + wx;  cc = vz + wy                                                                                      \
     *   s2 = (two*((gxx*gxx + gyy*gyy) + gzz*gzz)) + ((a*a + b*b) + cc*cc)                                                            \
     *   mu_e[...] = muT;   mu_e[I] = muT + c*sqrt(s2)                                                                                 \
     * Interior cells receive this value, EVERY other cell muT exactly — the model is off in the boundary layer of cells, whose stencil \
     * would leave the arrays; one call writes mu_e completely.  STRICT returns the bits of that statement (float64 and float32, no    \
     * contraction, whichever of the three division builds the spacings select; NS3D_IEEE_DIV is honoured) with the correctly rounded   \
     * square root of the element type, which is what np.sqrt is.  FAST multiplies by reciprocals and may contract.  length == 0 gives \
     * muT in every cell whose s2 is finite; a non-finite s2 propagates as NaN or Inf.  Enqueued on the context's stream, no read-back. \
     * NS3D_ERR_ARG, with nothing written: a null context or pointer; a grid below 3×3×3; a spacing that is not finite or not > 0; mu, \
     * rho or length not finite or negative; mu_e overlapping an input. */                                                             \
    int ns3d_eddy_viscosity_##S(ns3d_ctx *, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho, double length, \
                                double dx, double dy, double dz, int nx, int ny, int nz);                    \
    /* ns3d_eddy_viscosity with |S| replaced by the differential operator `op` (outside parity): mu_e = muT + c*op(G) on the interior   \
     * cells, muT exactly in the boundary layer of cells; one call writes mu_e completely, in ONE pass with the same three reads and   \
     * one write per cell.  G is ns3d_eddy_viscosity's gradient, gxx, gyy, gzz, uy, uz, vx, vz, wx, wy, verbatim, and h, two, muT, c   \
     * are its constants; third = (T)(1.0/3.0).  All arithmetic in T, nothing contracted in STRICT.  `length` is the caller's ℓ in      \
     * μ_t = ρ·ℓ²·op: C_s·Δ, C_w·Δ (C_w² ≈ 10.6·C_s²) or √c_v·Δ (c_v ≈ 2.5·C_s²).                                                      \
     * NS3D_SGS_SMAGORINSKY (0): op = sqrt(s2) with ns3d_eddy_viscosity's s2 — the call returns that call's bits.                      \
     * NS3D_SGS_WALE (1), Nicoud & Ducros 1999: g² = G·G with G = [[gxx,uy,uz],[vx,gyy,vz],[wx,wy,gzz]], its traceless symmetric part: \
     *   q11 = (gxx*gxx + uy*vx) + uz*wx    q12 = (gxx*uy + uy*gyy) + uz*wy    q13 = (gxx*uz + uy*vz) + uz*gzz                          \
     *   q21 = (vx*gxx + gyy*vx) + vz*wx    q22 = (vx*uy + gyy*gyy) + vz*wy    q23 = (vx*uz + gyy*vz) + vz*gzz                          \
     *   q31 = (wx*gxx + wy*vx) + gzz*wx    q32 = (wx*uy + wy*gyy) + gzz*wy    q33 = (wx*uz + wy*vz) + gzz*gzz                          \
     *   t = third*((q11 + q22) + q33);  d11 = q11 - t;  d22 = q22 - t;  d33 = q33 - t                                                 \
     *   d12 = h*(q12 + q21);  d13 = h*(q13 + q31);  d23 = h*(q23 + q32)                                                               \
     *   dd = ((d11*d11 + d22*d22) + d33*d33) + two*((d12*d12 + d13*d13) + d23*d23)                                                    \
     *   ss = h*s2                                                                                                                     \
     *   num = dd*sqrt(dd);   den = (ss*ss)*sqrt(ss) + dd*sqrt(sqrt(dd))                                                               \
     *   op = (den == 0) ? 0 : num/den          the plain IEEE quotient; a NaN den is not == 0 and propagates                          \
     * NS3D_SGS_VREMAN (2), Vreman 2004, with the isotropic filter width: β = G·Gᵀ,                                                     \
     *   b11 = (gxx*gxx + uy*uy) + uz*uz    b22 = (vx*vx + gyy*gyy) + vz*vz    b33 = (wx*wx + wy*wy) + gzz*gzz                          \
     *   b12 = (gxx*vx + uy*gyy) + uz*vz    b13 = (gxx*wx + uy*wy) + uz*gzz    b23 = (vx*wx + gyy*wy) + vz*gzz                          \
     *   aa = (b11 + b22) + b33                                                                                                        \
     *   B  = ((b11*b22 - b12*b12) + (b11*b33 - b13*b13)) + (b22*b33 - b23*b23)                                                        \
     *   Bc = (B < 0) ? 0 : B                   a comparison: a NaN stays a NaN                                                        \
     *   op = (aa == 0) ? 0 : sqrt(Bc/aa)                                                                                              \
     * The fractional powers are products of the element type's correctly rounded square root; there is no pow.  Both operators are    \
     * EXACTLY 0 in pure shear (u = γ·y: every q and B is a sum of exact zeros), where |S| = γ is largest; WALE also falls as y³ at a  \
     * wall.  STRICT returns the bits of these statements (float64 and float32, whichever of the three division builds the spacings    \
     * select; NS3D_IEEE_DIV is honoured); the quotient is the IEEE division in every build.  FAST multiplies the spacing divisions by \
     * reciprocals and may contract; its quotient and roots are the same IEEE operations.  When an intermediate overflows or is        \
     * subnormal (dd·√dd in float32 leaves the range near |G| ≈ 1e6 and 1e-8) NOTHING is promised beyond IEEE propagation through the   \
     * tree: Inf/Inf gives NaN, a den that underflows to 0 gives 0.  Enqueued on the context's stream, no read-back.                    \
     * NS3D_ERR_ARG, with nothing written: the cases of ns3d_eddy_viscosity, and an unknown op. */                                      \
    int ns3d_sgs_viscosity_##S(ns3d_ctx *, int op, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho, double length, \
                               double dx, double dy, double dz, int nx, int ny, int nz);                     \
    /* update_τ! with the scalar μ replaced by the field mu_e ((nx,ny,nz), e.g. ns3d_eddy_viscosity's).  Normal stresses use the cell's \
     * own value, (two*mu_e)*(…): update_τ!'s expression tree with 2μ read per cell.  Shear stresses use the mean of the four cells    \
     * around the edge; with q = (T)0.25, m = mu_e, for the (nx-1,ny-1,nz-1) shear arrays:                                             \
     *   mxy = q*((m[0:nx-1,0:ny-1,1:nz] + m[1:nx,0:ny-1,1:nz]) + (m[0:nx-1,1:ny,1:nz] + m[1:nx,1:ny,1:nz]))                          \
     *   mxz = q*((m[0:nx-1,1:ny,0:nz-1] + m[1:nx,1:ny,0:nz-1]) + (m[0:nx-1,1:ny,1:nz] + m[1:nx,1:ny,1:nz]))                          \
     *   myz = q*((m[1:nx,0:ny-1,0:nz-1] + m[1:nx,1:ny,0:nz-1]) + (m[1:nx,0:ny-1,1:nz] + m[1:nx,1:ny,1:nz]))                          \
     *   τxy = mxy*(d_yi(Vx)/dy + d_xi(Vy)/dx)   τxz = mxz*(d_zi(Vx)/dz + d_xi(Vz)/dx)   τyz = myz*(d_zi(Vy)/dz + d_yi(Vz)/dy)         \
     * A uniform mu_e returns the bits of ns3d_update_tau with that μ (q*((m+m)+(m+m)) is exact).  STRICT: the bits of this statement; \
     * FAST: reciprocals, every product rounded on its own (so that the fused form below can match it).  NS3D_ERR_ARG: a null context  \
     * or pointer, a grid below 2×2×2. */                                                                                              \
    int ns3d_update_tau_var_##S(ns3d_ctx *, T *txx, T *tyy, T *tzz, T *txy, T *txz, T *tyz, const T *Vx, const T *Vy, const T *Vz, \
                                const T *mu_e, double dx, double dy, double dz, int nx, int ny, int nz);     \
    /* {ns3d_update_tau_var; predict_V!} in one pass, with ns3d_predict_fused's contract: reads Vx, Vy, Vz and mu_e, writes COMPLETE    \
     * predicted fields into Vx_new, Vy_new, Vz_new (buffers of their own), the caller swaps the names, the stresses are not stored.  \
     * Bit for bit what those two calls leave in Vx, Vy, Vz, in every arithmetic mode.  NS3D_ERR_ARG, with nothing written: a null     \
     * context or pointer, a grid below 2×2×2, an output that is its own input. */                                                     \
    int ns3d_predict_var_##S(ns3d_ctx *, T *Vx_new, T *Vy_new, T *Vz_new, const T *Vx, const T *Vy, const T *Vz, const T *mu_e, \
                             double rho, double g, double dt, double dx, double dy, double dz, int nx, int ny, int nz); \
    /* The active scalar (outside parity).  ns3d_scalar_diffuse: ONE explicit step of ∂C/∂t = ∇·(K ∇C) in flux form on the cell-centred \
     * (nx,ny,nz) field C, out of place — every cell of C_out is written — with ZERO flux through all six domain faces.  mu_e, an    \
     * (nx,ny,nz) field such as ns3d_eddy_viscosity's, may be NULL.  All arithmetic in T: the scalars arrive as double and are converted \
     * once, h = (T)0.5.  As NumPy:                                                                                                  \
     *   K  = kappa                         (mu_e NULL)      |      kappa + sgs*(mu_e - mu)       per cell                           \
     *   Fx = (h*(K[:-1] + K[1:])) * ((C[1:] - C[:-1])/dx)           the nx-1 faces between cells in x; Fy, Fz likewise in y, z      \
     *   Dx = (pad0(Fx)[1:] - pad0(Fx)[:-1]) / dx                    pad0: one face of +0.0 at each end, through the SAME subtraction \
     *   C_out = C + dt*((Dx + Dy) + Dz)                                                                                             \
     * sgs = 1/(ρ·Sc_t) is formed by the caller in double (0: no eddy diffusivity): no division by it runs on the device.  The divisions \
     * by dx, dy, dz follow the context's arithmetic build exactly as in update_τ! (STRICT, NS3D_IEEE_DIV honoured: the bits of the  \
     * statement in float64 and float32; FAST: reciprocals).  STRICT contracts nothing; FAST fuses exactly three sums, a·b + c in one\
     * rounding: K = fma(sgs, mu_e - mu, kappa), C_out = fma(dt, (Dx + Dy) + Dz, C) and the one of ns3d_buoyancy below.  A face's flux is \
     * the same bits for both cells that share it.  kappa == 0 with no eddy diffusivity is still a full pass (C_out = C by value).  A \
     * uniform mu_e == mu returns the bits of mu_e NULL.  Stability (dt·K·Σ1/d² ≤ 1/2) is the caller's.  Enqueued on the context's   \
     * stream, no read-back.  NS3D_ERR_ARG, with nothing written, for this call and the two below: a null context or array (mu_e     \
     * excepted); a grid below 3×3×3; kappa, sgs, mu, bg, c_ref, dt or a spacing not finite; kappa < 0, sgs < 0, a spacing <= 0;     \
     * C_out == C. */                                                                                                                \
    int ns3d_scalar_diffuse_##S(ns3d_ctx *, T *C_out, const T *C, const T *mu_e, double kappa, double sgs, double mu, double dt,     \
                                double dx, double dy, double dz, int nx, int ny, int nz);                                            \
    /* The Boussinesq term of the vertical momentum, in place on @inn(Vz) — predict_V!'s range, 0-based 1 <= i <= nx-2, 1 <= j <= ny-2, \
     * 1 <= k <= nz-1 of the (nx,ny,nz+1) array; every other entry is untouched:                                                     \
     *   Vz[i,j,k] = Vz[i,j,k] + dt*(bg*(h*(C[i,j,k-1] + C[i,j,k]) - c_ref))                                                         \
     * bg = g·β is formed by the caller; a positive bg lifts fluid whose C exceeds c_ref.  FAST: fma(dt, bg*(h*(…) - c_ref), Vz). */    \
    int ns3d_buoyancy_##S(ns3d_ctx *, T *Vz, const T *C, double bg, double c_ref, double dt, int nx, int ny, int nz);                \
    /* ns3d_scalar_diffuse and ns3d_buoyancy in ONE pass (the form ns3d_time_step uses under ns3d_set_scalar), both reading the input C: \
     * C_out and Vz are left bit for bit what the two single calls leave, in every arithmetic mode and both element types — one kernel \
     * template serves the three calls.  5 elements of traffic per cell (read C, mu_e; read and write Vz; write C_out) against 7 for the \
     * two calls.  bg == 0 skips the Vz traffic (Vz may then be NULL). */                                                            \
    int ns3d_scalar_step_##S(ns3d_ctx *, T *C_out, T *Vz, const T *C, const T *mu_e, double kappa, double sgs, double mu, double bg, \
                             double c_ref, double dt, double dx, double dy, double dz, int nx, int ny, int nz);                      \
    /* set_cylinder!(C,Vx,Vy,Vz,a2,b2,ox,oy,sinβ,cosβ,xco_g,yco_g,zco_g,lx,ly,lz,dx,dy,dz) multi.jl:249-281 */\
    int ns3d_set_cylinder_##S(ns3d_ctx *, T *C, T *Vx, T *Vy, T *Vz, double a2, double b2, double ox,        \
                              double oy, double sinb, double cosb, double xco_g, double yco_g, double zco_g, \
                              double lx, double ly, double lz, double dx, double dy, double dz, int nx,      \
                              int ny, int nz);                                                               \
    /* set_cylinder!(C,Vx,Vy,Vz,a2,b2,ox,oy,sinβ,cosβ,lx,ly,lz,dx,dy,dz)  gpu.jl:336-368 (incl. its dx-for-dy */\
    int ns3d_set_cylinder_local_##S(ns3d_ctx *, T *C, T *Vx, T *Vy, T *Vz, double a2, double b2, double ox,  \
                                    double oy, double sinb, double cosb, double lx, double ly, double lz,    \
                                    double dx, double dy, double dz, int nx, int ny, int nz);                \
    /* What set_cylinder! stores, with the flags read from a mask (ns3d_voxelize above): where bit 0 is set C = 1, bit 1 Vx = 0, bit 2      \
     * Vy = 0, bit 3 Vz = 0; everything else is untouched.  Bits at invalid points are ignored, not trusted: no address outside the      \
     * arrays is touched whatever the bytes hold.  C may be NULL.  Enqueued on the context's stream, no read-back.  NS3D_ERR_ARG: a null   \
     * context, velocity or mask. */                                                                                                    \
    int ns3d_set_solid_##S(ns3d_ctx *, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, int nx, int ny, int nz);                    \
    /* The monitor's mom[q] / n_masked[q] for a mask: the sum and the number of the OWNED nodes of Vx (Vy, Vz) whose mask bit is set —   \
     * what the next ns3d_set_solid removes.  The owned ranges are those of ns3d_diagnostics; seam_lo / seam_hi (three ints each) may be \
     * NULL: no seams.  Values are converted to double on load and reduced in fp64 in the monitor's fixed order (per thread down its    \
     * planes, wave64 butterfly, one LDS slot per wave, per-workgroup partials in the context's scratch, a second small launch): two     \
     * calls return the same bits, in every arithmetic mode.  mom_host and n_host (host memory, three entries each) receive the results; \
     * the call blocks for this read-back like ns3d_max_abs.  NS3D_ERR_ARG: a null context or pointer, a grid below 3x3x3. */            \
    int ns3d_solid_momentum_##S(ns3d_ctx *, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny, int nz,    \
                                const int *seam_lo, const int *seam_hi, double *mom_host, long long *n_host);                           \
    /* ns3d_set_solid for a body in rigid motion: the bits, the valid ranges and the treatment of bits at invalid points are its own,   \
     * C = 1 where bit 0 is set (C may be NULL), and where a velocity bit is set the store is the body's velocity at that node.         \
     * motion = U[3], omega[3], centre[3] (centre in index space); origin (may be NULL: zeros) as ns3d_voxelize.  A node's position is  \
     * X = (i+origin_x)+s_x, ... with the stagger s of ns3d_voxelize (exact).  All in fp64, nothing contracted, converted ONCE to T:    \
     *   rx = (X - cx)*dx;  ry = (Y - cy)*dy;  rz = (Z - cz)*dz                                                                         \
     *   vbx = Ux + (wy*rz - wz*ry);  vby = Uy + (wz*rx - wx*rz);  vbz = Uz + (wx*ry - wy*rx)                                           \
     *   Vx[node] = (T)vbx (bit 1)    Vy[node] = (T)vby (bit 2)    Vz[node] = (T)vbz (bit 3)                                            \
     * As NumPy, for Vx with I, J, K = ogrid of its shape: rz = ((K+oz)+.5 - cz)*dz; ry = ((J+oy)+.5 - cy)*dy;                          \
     *   Vx[bit1] = (Ux + (wy*rz - wz*ry)).astype(T)[bit1]  (tests/moving_ref.py is this statement).                                   \
     * STRICT, NS3D_IEEE_DIV and FAST contexts return the same bits.  Two consequences: with U = omega = +0.0 every store is +0.0      \
     * (0 + (±0 − ±0) is +0 in round-to-nearest), so the call returns ns3d_set_solid's bits; and vbx does not depend on X, vby not on  \
     * Y, vbz not on Z, so the two faces of a cell in each direction hold identical bits and ns3d_update_divV is exactly +0.0 in every \
     * cell whose six faces are masked, in both element types.  Enqueued on the context's stream, no read-back.                        \
     * NS3D_ERR_ARG, with nothing written: the cases of ns3d_set_solid; a null motion; one of the nine numbers or a spacing not finite; \
     * a spacing not > 0; a negative origin entry; a grid below 3x3x3. */                                                              \
    int ns3d_set_solid_moving_##S(ns3d_ctx *, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, const double *motion, double dx,    \
                                  double dy, double dz, const int *origin, int nx, int ny, int nz);                                     \
    /* ns3d_solid_momentum for a body in rigid motion: per direction the sum of (double)V[node] - (double)(T)vb over the owned masked   \
     * nodes — exactly what the next ns3d_set_solid_moving with the same motion removes — and the same counts.  The same fixed order,  \
     * the same scratch and the same read-back: two calls return the same bits, and zero motion returns ns3d_solid_momentum's bits.     \
     * NS3D_ERR_ARG: the cases of ns3d_solid_momentum and the motion, spacing and origin cases of ns3d_set_solid_moving. */             \
    int ns3d_solid_momentum_moving_##S(ns3d_ctx *, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny,    \
                                       int nz, const int *seam_lo, const int *seam_hi, double *mom_host, long long *n_host,             \
                                       const double *motion, double dx, double dy, double dz, const int *origin);                       \
    /* update_∇V!(∇V,Vx,Vy,Vz,dx,dy,dz)                             multi.jl:61-64   gpu.jl:194-197 */        \
    int ns3d_update_divV_##S(ns3d_ctx *, T *divV, const T *Vx, const T *Vy, const T *Vz, double dx,          \
                             double dy, double dz, int nx, int ny, int nz);                                  \
    /* update_dPrdτ!(Pr,dPrdτ,∇V,ρ,dt,dτ,damp,dx,dy,dz)            multi.jl:70-73   gpu.jl:199-202 */        \
    int ns3d_update_dPrdtau_##S(ns3d_ctx *, const T *Pr, T *dPrdtau, const T *divV, double rho, double dt,   \
                                double dtau, double damp, double dx, double dy, double dz, int nx, int ny,   \
                                int nz);                                                                     \
    /* update_Pr!(Pr,dPrdτ,dτ)                                     multi.jl:79-82   gpu.jl:204-207 */        \
    int ns3d_update_Pr_##S(ns3d_ctx *, T *Pr, const T *dPrdtau, double dtau, int nx, int ny, int nz);        \
    /* compute_res!(Rp,Pr,∇V,ρ,dt,dx,dy,dz)                        multi.jl:88-91   gpu.jl:209-212 */        \
    int ns3d_compute_res_##S(ns3d_ctx *, T *Rp, const T *Pr, const T *divV, double rho, double dt,           \
                             double dx, double dy, double dz, int nx, int ny, int nz);                       \
    /* maximum(abs.(A)) — NaN-propagating like Julia's maximum     multi.jl:466     gpu.jl:132 */            \
    int ns3d_max_abs_##S(ns3d_ctx *, const T *A, long n_elems, double *out_host);                            \
    /* correct_V!(Vx,Vy,Vz,Pr,dt,ρ,dx,dy,dz)                        multi.jl:97-102  gpu.jl:214-219 */        \
    int ns3d_correct_V_##S(ns3d_ctx *, T *Vx, T *Vy, T *Vz, const T *Pr, double dt, double rho, double dx,   \
                           double dy, double dz, int nx, int ny, int nz);                                    \
    /* bc_x!/bc_y!/bc_z!(A) on an array of extents (sx,sy,sz)       multi.jl:108-132 gpu.jl:221-237 */        \
    int ns3d_bc_x_##S(ns3d_ctx *, T *A, int sx, int sy, int sz);                                             \
    int ns3d_bc_y_##S(ns3d_ctx *, T *A, int sx, int sy, int sz);                                             \
    int ns3d_bc_z_##S(ns3d_ctx *, T *A, int sx, int sy, int sz);                                             \
    /* bc_zV!(A)                                                    gpu.jl:239-243 */                        \
    int ns3d_bc_zV_##S(ns3d_ctx *, T *A, int sx, int sy, int sz);                                            \
    /* bc_xhydstatic!(A,dz,nz,g,ρ)                                  gpu.jl:257-261 */                        \
    int ns3d_bc_xhydstatic_##S(ns3d_ctx *, T *A, double dz, int nz, double g, double rho, int sx, int sy,    \
                               int sz);                                                                      \
    /* bc_x_Vx!(A,V)                                                multi.jl:138-141 */                      \
    int ns3d_bc_x_Vx_##S(ns3d_ctx *, T *A, double V, int sx, int sy, int sz);                                \
    /* bc_x_Pr!(A,val)                                              multi.jl:147-150 */                      \
    int ns3d_bc_x_Pr_##S(ns3d_ctx *, T *A, double val, int sx, int sy, int sz);                              \
    /* X_o .= X                                                     multi.jl:475     gpu.jl:141 */            \
    int ns3d_copy_##S(ns3d_ctx *, T *dst, const T *src, long n_elems);                                       \
    /* advect!(Vx,Vx_o,Vy,Vy_o,Vz,Vz_o,C,C_o,dt,dx,dy,dz)           multi.jl:217-243 gpu.jl:308-334           \
     * faithful!=0 reproduces the reference (third branch back-tracks Vy, Vz never advected).            */  \
    int ns3d_advect_##S(ns3d_ctx *, T *Vx, const T *Vx_o, T *Vy, const T *Vy_o, T *Vz, const T *Vz_o, T *C,  \
                        const T *C_o, double dt, double dx, double dy, double dz, int nx, int ny, int nz,    \
                        int faithful);                                                                       \
    /* {Vx_o .= Vx; Vy_o .= Vy; Vz_o .= Vz; C_o .= C; advect!(…)}  multi.jl:475-476 / gpu.jl:141-142 in ONE pass: the caller    \
     * passes the CURRENT fields (read only) and receives COMPLETE new fields in buffers of its own — every entry is stored, the \
     * ones advect! leaves alone with the current value — and swaps the roles of the buffers afterwards (the four    \
     * copies are "avoidable by pointer swap").  Vz_new may be Vz itself in faithful mode (Vz is never advected there).  Same    \
     * values as ns3d_copy ×4 + ns3d_advect, bit for bit. */                                                 \
    int ns3d_copy_advect_##S(ns3d_ctx *, T *Vx_new, const T *Vx, T *Vy_new, const T *Vy, T *Vz_new, const T *Vz, T *C_new, \
                             const T *C, double dt, double dx, double dy, double dz, int nx, int ny, int nz, \
                             int faithful);                                                                  \
    /* Limited MacCormack advection (Selle et al. 2008), second order, built from backtrack! itself — NOT in the reference, an    \
     * option beside ns3d_copy_advect, one rank.  All arithmetic is in T, like advect!.  For a field A with old values A_o the    \
     * advected nodes and their velocities (vxc, vyc, vzc: averages of the OLD velocities) are advect!'s four branches with the   \
     * third one corrected: Vx ix = 2…nx, Vy iy = 2…ny, Vz iz = 2…nz, C every cell.                                              \
     *   stage 1   Â = backtrack!(Â, A_o, vxc, vyc, vzc, dt, …): what ns3d_copy_advect(…, faithful = 0) returns, complete          \
     *   stage 2   back = backtrack! on the complete Â with (T)(−dt) in place of dt and the same vxc, vyc, vzc                    \
     *             s = Â[ix,iy,iz] + h·(A_o[ix,iy,iz] − back),  h = (T)0.5  (this order; STRICT does not contract it)             \
     *             lo, hi = the smallest and largest of the eight OLD values stage 1 interpolated between: with stage 1's own     \
     *             ix1 = clamp(floor(ix − δx), 1, sx), ix2 = clamp(ix1 + 1, 1, sx) (likewise y, z) start from c = A_o[ix1,iy1,iz1] \
     *             and visit (2,1,1), (1,2,1), (2,2,1), (1,1,2), (2,1,2), (1,2,2), (2,2,2): lo = c < lo ? c : lo, hi = c > hi ? c : hi \
     *             A_new = s < lo ? lo : s;  A_new = A_new > hi ? hi : A_new   (comparisons: a NaN s stays NaN)                   \
     * Entries outside the advected set receive Â's value (the current one).  No address outside the arrays is read: every index \
     * is clamped as in backtrack!.  A field at rest keeps its values in every mode.  Stage 2 as NumPy, for one field on its     \
     * advected nodes IX, IY, IZ (1-based index grids), arrays and scalars of dtype T, lerp(a, b, t) = b*t + a*(1 − t):            \
     *   def departure(dt):                                                                                                       \
     *       dd = [dt*vxc/dx, dt*vyc/dy, dt*vzc/dz]                                                                                \
     *       i1 = [np.clip(np.floor(I − d).astype(np.int64), 1, s) for I, d, s in zip((IX, IY, IZ), dd, A_o.shape)]               \
     *       i2 = [np.clip(i + 1, 1, s) for i, s in zip(i1, A_o.shape)]                                                           \
     *       return i1, i2, [(d > 0).astype(T) − np.fmod(d, 1) for d in dd]                                                       \
     *   (x1, y1, z1), (x2, y2, z2), _ = departure(dt);  o = lambda i, j, k: A_o[i − 1, j − 1, k − 1]                                \
     *   lo = hi = o(x1, y1, z1)                                                                                                   \
     *   for c in (o(x2,y1,z1), o(x1,y2,z1), o(x2,y2,z1), o(x1,y1,z2), o(x2,y1,z2), o(x1,y2,z2), o(x2,y2,z2)):                     \
     *       lo = np.where(c < lo, c, lo);  hi = np.where(c > hi, c, hi)                                                          \
     *   (x1, y1, z1), (x2, y2, z2), (wx, wy, wz) = departure(−dt);  a = lambda i, j, k: A_hat[i − 1, j − 1, k − 1]                  \
     *   fz1 = lerp(lerp(a(x1,y1,z1), a(x2,y1,z1), wx), lerp(a(x1,y2,z1), a(x2,y2,z1), wx), wy)                                    \
     *   fz2 = lerp(lerp(a(x1,y1,z2), a(x2,y1,z2), wx), lerp(a(x1,y2,z2), a(x2,y2,z2), wx), wy)                                    \
     *   s = a(IX, IY, IZ) + h*(o(IX, IY, IZ) − lerp(fz1, fz2, wz))                                                                \
     *   A_new = A_hat.copy();  r = np.where(s < lo, lo, s);  A_new[IX − 1, IY − 1, IZ − 1] = np.where(r > hi, hi, r)                \
     * STRICT returns these bits (whichever division build the spacings select); FAST multiplies by reciprocals, may contract,   \
     * and limits against the stencil ITS stage 1 chose.                                                                          \
     * ns3d_advect_correct is stage 2 alone: X_hat is stage 1's complete result for the old field X, X_new receives the new field \
     * (every entry).  ns3d_advect_mc runs stage 1 into the caller's X_hat buffers, then stage 2; afterwards the X_hat hold stage  \
     * 1's complete result.  Both are enqueued on the context's stream without a read-back (they block only as every call does    \
     * without NS3D_ASYNC).  NS3D_ERR_ARG, nothing written: a null context or pointer, a grid below 3×3×3, any two of the twelve   \
     * arrays equal. */                                                                                                            \
    int ns3d_advect_correct_##S(ns3d_ctx *, T *Vx_new, const T *Vx, const T *Vx_hat, T *Vy_new, const T *Vy, const T *Vy_hat,      \
                                T *Vz_new, const T *Vz, const T *Vz_hat, T *C_new, const T *C, const T *C_hat, double dt,          \
                                double dx, double dy, double dz, int nx, int ny, int nz);                                        \
    int ns3d_advect_mc_##S(ns3d_ctx *, T *Vx_new, const T *Vx, T *Vx_hat, T *Vy_new, const T *Vy, T *Vy_hat, T *Vz_new,            \
                           const T *Vz, T *Vz_hat, T *C_new, const T *C, T *C_hat, double dt, double dx, double dy, double dz,    \
                           int nx, int ny, int nz);                                                                              \
    /* DIRECT solve of what the pseudo-transient loop multi.jl:458-471 / gpu.jl:126-137 iterates towards (an   \
     * option OUTSIDE parity: the reference stops at err < 1e-3, this solves the same discrete system to rounding): Pr's      \
     * interior becomes the solution of ∇²_h Pr = ρ/dt·∇V with the boundary cells of set_bc_Pr! (p->bc_kind, p->owns_outlet,  \
     * p->outlet_val, p->g), the boundary cells are set accordingly, dPrdτ = 0.  Exact diagonalisation of the box Laplacian   \
     * (closed-form eigenvectors per direction) by six fp64 MFMA matrix products; fp32 fields are solved in fp64.  Single-rank \
     * grids (no z halo flags).  All-Neumann problems (no outlet): the zero-mean solution. */                \
    int ns3d_poisson_direct_##S(ns3d_ctx *, T *Pr, T *dPrdtau, const T *divV, const ns3d_pt_params *p);      \
    /* ---- host sequences of the reference, one call each ---- */                                           \
    /* set_bc_Pr!  multi.jl:175-181 (kind 0, without the halo update) / gpu.jl:281-286 (kind 1).  Both set_bc_* run the      \
     * reference's rule sequence as ONE gather launch (same values on every cell, edges and corners included;                \
     * NS3D_BC_FUSED=0 or an extent below 3: a launch per rule) */                                            \
    int ns3d_set_bc_Pr_##S(ns3d_ctx *, T *Pr, int bc_kind, int owns_outlet, double outlet_val, double dz,    \
                           int nz_arg, double g, double rho, int nx, int ny, int nz);                        \
    /* set_bc_Vel! multi.jl:156-166 (kind 0, without the halo update) / gpu.jl:264-279 (kind 1) */           \
    int ns3d_set_bc_Vel_##S(ns3d_ctx *, T *Vx, T *Vy, T *Vz, int bc_kind, int owns_inlet, double vin,        \
                            int nx, int ny, int nz);                                                         \
    /* ---- fused fast path (not in the reference; same results) ----                                        \
     * n_iters × { update_dPrdτ! ; update_Pr! ; set_bc_Pr! }  (multi.jl:459-463 / gpu.jl:127-129) as ONE     \
     * ping-pong sweep per iteration with the boundary planes folded in.  Pr holds the result on return. */  \
    int ns3d_pt_iterate_##S(ns3d_ctx *, T *Pr, T *dPrdtau, const T *divV, const ns3d_pt_params *p,           \
                            int n_iters);                                                                    \
    /* One sweep Pr_in → Pr_out (distinct buffers; halo planes of Pr_out are NOT written when               \
     * z_*_is_halo) restricted to interior planes k0 ≤ k < k1 (0-based Pr plane index, 1 ≤ k0, k1 ≤ nz-1).  \
     * Building block for the z-slab overlap schedule (boundary planes first, interior behind the halo     \
     * exchange). */                                                                                         \
    int ns3d_pt_sweep_##S(ns3d_ctx *, const T *Pr_in, T *Pr_out, T *dPrdtau, const T *divV,                  \
                          const ns3d_pt_params *p, int k0, int k1);                                          \
    /* TWO fused PT iterations (Pr_in,dPrdtau_in) → (Pr_out,dPrdtau_out), all four buffers distinct (tiles       \
     * overlap, so nothing is updated in place); results identical to two ns3d_pt_sweep calls with a buffer     \
     * swap, for the output planes k0 ≤ k < k1 (reads planes k0-2 … k1+1 of Pr_in).  z_*_is_halo must be 0:   \
     * z-slab ranks run it on buffers extended by a second ghost plane per seam. */              \
    int ns3d_pt_sweep2_##S(ns3d_ctx *, const T *Pr_in, T *Pr_out, const T *dPrdtau_in, T *dPrdtau_out,       \
                           const T *divV, const ns3d_pt_params *p, int k0, int k1);                          \
    /* nlev (2…4; 5 in the _f32 form) fused PT iterations in one pass over memory, otherwise as ns3d_pt_sweep2: results identical to nlev   \
     * ns3d_pt_sweep calls, output planes k0 ≤ k < k1 (reads planes k0-nlev … k1+nlev-1 of Pr_in, clamped to the grid). */ \
    int ns3d_pt_sweepn_##S(ns3d_ctx *, int nlev, const T *Pr_in, T *Pr_out, const T *dPrdtau_in, T *dPrdtau_out,  \
                           const T *divV, const ns3d_pt_params *p, int k0, int k1);                          \
    /* Plan phase of the two-iteration sweep (ns3d_set_autotune): times the tile shapes NOW on these very arguments  \
     * (idempotent: inputs and outputs are distinct buffers; every shape gives the same bits) and remembers the       \
     * winner per device, grid and plane range for the rest of the process.  Blocks.  ns3d_pt_iterate / ns3d_pt_solve \
     * plan on first use by themselves; ns3d_pt_sweep2 never measures — it looks the choice up (built-in shape when   \
     * nothing was planned).  Pr_out / dPrdtau_out hold the result of one two-iteration pass afterwards. */           \
    int ns3d_plan_pt_##S(ns3d_ctx *, const T *Pr_in, T *Pr_out, const T *dPrdtau_in, T *dPrdtau_out,         \
                         const T *divV, const ns3d_pt_params *p, int k0, int k1);                            \
    /* max|∇²Pr − ρ/dt ∇V| over the interior = maximum(abs.(Rp)) after compute_res!, without writing Rp.   \
     * NaN-propagating.  (multi.jl:465-466) */                                                               \
    int ns3d_residual_max_##S(ns3d_ctx *, const T *Pr, const T *divV, const ns3d_pt_params *p,               \
                              double *out_host);                                                             \
    /* Compares the divisor-known-in-advance division with the plain IEEE division for n pseudo-random dividends  \
     * (bitwise); *mismatches must come back 0.  The dividends are x = RN(q*d) with the QUOTIENT's binade drawn: half \
     * within 2^+-60 (f32: 2^+-20), the rest over the guard's whole range, eight binades beyond each end, within six    \
     * binades of each bound of the one- and two-division guards; every other one planted next to a rounding midpoint. */ \
    int ns3d_selftest_exact_div_##S(ns3d_ctx *, double d, long n, unsigned long long seed, long *mismatches);\
    /* The whole inner loop multi.jl:458-471 / gpu.jl:126-137 on one rank: at most niter iterations, every   \
     * nchk-th computes err = max|Rp|*err_mul/err_div (= maximum(abs.(Rp))*ly^2/psc, multi.jl:466), stops  \
     * on err<eps || !isfinite(err) (eps<0: never stop).                                                      \
     * err_hist (capacity max_checks) may be NULL. */                                                        \
    int ns3d_pt_solve_##S(ns3d_ctx *, T *Pr, T *dPrdtau, const T *divV, const ns3d_pt_params *p, double eps, \
                          int niter, int nchk, double err_mul, double err_div, int *iters_done,              \
                          double *err_hist, int max_checks, int *n_checks);

NS3D_DECL(double, f64)
NS3D_DECL(float, f32)
#undef NS3D_DECL

/* =====================================================================================================================
 * Multi-GPU: the implicit global grid.  Replaces what multi.jl gets from ImplicitGlobalGrid.jl + MPI.jl:
 *     init_global_grid(nx,ny,nz)   multi.jl:325      →  ns3d_mgpu_create / ns3d_mgpu_create_rank   (dims = (1,1,P): z-slabs)
 *                                                       ns3d_mgpu_create_cart / _create_rank_cart  (any dims; ns3d_dims_create =
 *                                                       the MPI_Dims_create default of init_global_grid)
 *     update_halo!(A…)             multi.jl:371,373,450,453,455,460,462,182,167,477  →  ns3d_update_halo
 *     max_g(A)                     multi.jl:21,466   →  ns3d_max_g
 *     gather!(A_inn, A_v)          multi.jl:399-403,528-532  →  ns3d_gather
 *     nz_g()                       multi.jl:328,338  →  ns3d_mgpu_nz_g            finalize_global_grid() :534 → ns3d_mgpu_destroy
 * ImplicitGlobalGrid's indexing is kept: overlap 2, halo width 1, nz_g = P·(nz−2)+2; an array with nz+s planes has overlap
 * 2+s (sends plane 2+s / size−(1+s), receives into 1 / size, 1-based); arrays with overlap < 2 have no halo; physical ends
 * are left untouched; the same rule per dimension for a Cartesian topology, dimensions in the order x, y, z so that edge and
 * corner values arrive in two / three hops.  Column-major xy-planes are contiguous, so a z message is one block as it lies;
 * x and y faces are packed / unpacked by a kernel on both ends.  ns3d_pt_solve_slab runs the loop multi.jl:458-471 on any
 * topology with deep ghosts — several iterations per pass over memory, one round of exchanges per pass: on z-slabs with the state
 * below (seam planes first, their exchange behind the interior sweep), on a grid decomposed in x or y with every rank's state in a
 * box extended by depth−1 ghost cells in each decomposed direction, the ghost layers exchanged dimension by dimension (x / y
 * layers packed by a kernel); with depth 1 (ns3d_mgpu_set_temporal) or NS3D_CART_DEEP=0 such a grid runs one fused sweep and one
 * halo update per iteration instead.  ns3d_slab_load / _iterate / _store are z-slab only.
 *
 * An ns3d_mgpu holds `nlocal` of the P ranks: all P in the one-process form (ns3d_mgpu_create; planes move by
 * hipMemcpyPeerAsync over xGMI; a device may appear several times — virtual ranks), exactly one in the one-process-per-GPU
 * form (ns3d_mgpu_create_rank; planes move by RCCL send/recv on a dedicated stream, the residual by ncclAllReduce).
 * Every per-rank argument is an array of nlocal entries in local-rank order; field lists are field-major:
 * fields[f*nlocal + l].  Kernels for local rank l run on ns3d_mgpu_ctx(m, l).  Calls are ordered with the work already
 * enqueued on those contexts' streams and block unless `flags` had NS3D_ASYNC.
 * ===================================================================================================================== */
typedef struct ns3d_mgpu ns3d_mgpu;
#define NS3D_UNIQUE_ID_BYTES 128

ns3d_mgpu *ns3d_mgpu_create(int P, const int *devices, int nx, int ny, int nz_local, int flags);
/* dims[3] = ranks per dimension; rank order is MPI_Cart's (rank = (cx·dims[1] + cy)·dims[2] + cz); devices[rank] */
ns3d_mgpu *ns3d_mgpu_create_cart(const int *dims, const int *devices, int nx, int ny, int nz, int flags);
/* MPI_Dims_create: entries > 0 of dims[3] are kept, zeros are filled with the most balanced factorisation, non-increasing
 * (P = 8 → 2,2,2; 4 → 2,2,1; 2 → 2,1,1; 12 → 3,2,2) — what init_global_grid(nx,ny,nz) uses when dimx/dimy/dimz are not given */
int ns3d_dims_create(int P, int *dims);
/* One process per GPU: rank 0 calls ns3d_mgpu_unique_id and distributes the NS3D_UNIQUE_ID_BYTES bytes (MPI.Bcast in the
 * reference's setting), then every rank calls ns3d_mgpu_create_rank (collective).  RCCL is loaded at run time. */
int ns3d_mgpu_unique_id(void *id_out);
ns3d_mgpu *ns3d_mgpu_create_rank(int P, int rank, int device, const void *unique_id, int nx, int ny, int nz_local, int flags);
ns3d_mgpu *ns3d_mgpu_create_rank_cart(const int *dims, int rank, int device, const void *unique_id, int nx, int ny, int nz,
                                      int flags);
void ns3d_mgpu_destroy(ns3d_mgpu *m);
int ns3d_mgpu_world(const ns3d_mgpu *m);               /* P */
int ns3d_mgpu_nlocal(const ns3d_mgpu *m);
int ns3d_mgpu_rank(const ns3d_mgpu *m, int local);     /* "me" of a local rank (= its z coordinate for z-slabs) */
int ns3d_mgpu_dims(const ns3d_mgpu *m, int *dims_out);                 /* 3 ints */
int ns3d_mgpu_coords(const ns3d_mgpu *m, int local, int *coords_out);  /* 3 ints: MPI_Cart_coords of a local rank */
int ns3d_mgpu_n_g(const ns3d_mgpu *m, int *n_g_out);                   /* nx_g(), ny_g(), nz_g(): dims·(n−2)+2 */
ns3d_ctx *ns3d_mgpu_ctx(ns3d_mgpu *m, int local);
int ns3d_mgpu_nz_g(const ns3d_mgpu *m);
const char *ns3d_mgpu_transport(const ns3d_mgpu *m);   /* "peer" | "rccl" */
int ns3d_mgpu_rccl_ranks(const ns3d_mgpu *m);          /* ncclCommCount of the communicator (0 in the one-process form) */
int ns3d_mgpu_sync(ns3d_mgpu *m);
int ns3d_max_g(ns3d_mgpu *m, const double *local_max, double *out);    /* NaN-propagating */
/* Most PT iterations a pass over memory may advance in ns3d_slab_* / ns3d_pt_solve_slab = ghost planes per seam + 1: 4 (default),
 * 3, 2 or 1 (plain one-plane halo, single sweeps).  Passes run two iterations until ns3d_slab_plan has measured whether three
 * or four pay on this grid; every rank uses the same depth. */
int ns3d_mgpu_set_temporal(ns3d_mgpu *m, int depth);
int ns3d_mgpu_pass_depth(const ns3d_mgpu *m);
/* Making room for the exchange's kernels while the interior sweep runs (round 4; results do not depend on either):
 * ns3d_mgpu_reserve_cus — ns3d_reserve_cus on every local rank's context (the seam sweeps and the exchange stay on the unmasked
 * high-priority communication stream); ns3d_mgpu_set_interior_chunks — the interior sweep of a z-slab pass goes out as `chunks`
 * launches over consecutive plane ranges (1 = one launch; NS3D_SLAB_INTERIOR_CHUNKS presets it), so that a pending send/recv
 * finds CUs at the latest when a chunk ends. */
int ns3d_mgpu_reserve_cus(ns3d_mgpu *m, int n_cus);
int ns3d_mgpu_set_interior_chunks(ns3d_mgpu *m, int chunks);
/* ghost planes per seam of the loaded solve state: (deepest pass allowed) - 1 after ns3d_slab_load, pass depth - 1 once
 * ns3d_slab_plan has agreed on the iterations per pass; -1 when nothing is loaded */
int ns3d_mgpu_ghost_depth(const ns3d_mgpu *m);
/* The pseudo-transient state of a z-slab rank lives in library-owned buffers extended by the ghost planes temporal
 * blocking needs: load → iterate / residual → store; ns3d_pt_solve_slab is the whole inner loop multi.jl:458-471
 * (load, plan, iterate with a global residual check every nchk iterations, store).  Iterates are bit-identical to the
 * single-device solve of the global grid.  p describes the local grid of every rank; p->owns_outlet says whether the GLOBAL
 * x-hi face carries the outlet rule (multi.jl:179) — the library applies it on the ranks that hold that face (all of them on
 * z-slabs) — and the z halo flags of p are ignored (set per rank inside).  (The seam planes of divV are exchanged at load: multi.jl:455's update_halo!(∇V)
 * may but need not have run.) */
int ns3d_slab_iterate(ns3d_mgpu *m, int n_iters);
int ns3d_slab_plan(ns3d_mgpu *m);
int ns3d_slab_residual(ns3d_mgpu *m, double *out);
/* Tracers on a decomposed grid, second half: after the advance on every rank, ns3d_tracers_advance_mgpu below, every particle that left its rank's part of
 * the global box travels to its owner (the ownership rule is with ns3d_tracers_advance_at).  No element type: no field is touched.
 * Each local rank l has cap[l] SLOTS: X[l] three blocks of cap[l] doubles, state[l] one byte per slot, id[l] one long long per slot
 * (>= 0 occupied, -1 empty), U[l] (the list may be NULL) three blocks of payload carried along.  A LEAVER is an occupied slot with
 * state 1 and finite coordinates whose owner is another rank; dead particles never move (they record where they left).  A leaver's
 * slot becomes empty: id -1, state 0, its X and U entries NaN.  The arrivals at a rank are ordered by source rank ascending and
 * within a source by slot ascending, and go into that rank's empty slots in ascending slot order, the slots vacated in this call
 * included.  Count, scan, compact: no atomic decides a position, two calls on the same input give the same arrays.
 * *moved_host receives the number of particles moved.  If some rank has fewer empty slots than arrivals NOTHING is modified on any
 * rank, need_host[l] is the shortfall of local rank l (0 where there is room), *moved_host is 0 and the call returns NS3D_ERR_STATE:
 * the rule is a pure function of the positions, so the caller enlarges its arrays and calls again.  Blocks for the counts like
 * ns3d_diagnostics_mgpu.  One-process form only (peer copies, virtual ranks on one device included); in the one-process-per-GPU
 * form the call returns NS3D_ERR_STATE.  NS3D_ERR_ARG, nothing touched: a null list or output, cap[l] < 0, a null array of a rank
 * with cap[l] > 0 (a rank with cap[l] = 0 is fine). */
int ns3d_tracers_migrate_mgpu(ns3d_mgpu *m, double *const *X, unsigned char *const *state, long long *const *id, double *const *U,
                              const long *cap, long long *moved_host, long *need_host);

#define NS3D_MGPU_DECL(T, S)                                                                                \
    /* extents: 3 ints (sx,sy,sz) per field */                                                              \
    int ns3d_update_halo_##S(ns3d_mgpu *m, T *const *fields, const int *extents, int nfields);              \
    /* halo-stripped blocks A[2:end-1,2:end-1,2:end-1] of every rank, placed side by side in rank-coordinate \
     * order, into the column-major out_host (dims[0]·(sx-2) × dims[1]·(sy-2) × dims[2]·(sz-2) elements;     \
     * rank 0's process only in the one-process-per-GPU form) */                                             \
    int ns3d_gather_##S(ns3d_mgpu *m, const T *const *A, int sx, int sy, int sz, T *out_host);              \
    int ns3d_slab_load_##S(ns3d_mgpu *m, const T *const *Pr, const T *const *dPrdtau, const T *const *divV, \
                           const ns3d_pt_params *p);                                                        \
    int ns3d_slab_store_##S(ns3d_mgpu *m, T *const *Pr, T *const *dPrdtau);                                 \
    /* {X_o .= X; advect!; update_halo!} (multi.jl:475-477) on z-slab ranks with the old fields' z halo widened to TWO planes — \
     * an option OUTSIDE the reference's multi-rank semantics: backtrack! clamps to the local array (multi.jl:192-195), so a      \
     * departure point beyond the one-plane halo is clamped on a rank where the one-rank run reads the neighbour.  Here every   \
     * rank advects on copies extended by one more plane per seam, all four new fields (C too) get their halo, and P ranks      \
     * reproduce the one-rank time step bit for bit while |δz| < 2 cells.  Per-rank pointer lists as everywhere. */            \
    int ns3d_advect_wide_##S(ns3d_mgpu *m, T *const *Vx, T *const *Vx_o, T *const *Vy, T *const *Vy_o, T *const *Vz,           \
                             T *const *Vz_o, T *const *C, T *const *C_o, double dt, double dx, double dy, double dz,          \
                             int faithful);                                                                  \
    int ns3d_pt_solve_slab_##S(ns3d_mgpu *m, T *const *Pr, T *const *dPrdtau, const T *const *divV,         \
                               const ns3d_pt_params *p, double eps, int niter, int nchk, double err_mul,    \
                               double err_div, int *iters_done, double *err_hist, int max_checks,           \
                               int *n_checks);                                                      \
    /* The direct pressure solve (ns3d_poisson_direct) of the GLOBAL grid on z-slab ranks (dims = (1,1,P)): the interior of the \
     * nx × ny × nz_g grid becomes the solution of ∇²_h Pr = ρ/dt·∇V with set_bc_Pr!'s rule (NS3D_BC_MULTI; all-Neumann: the     \
     * zero-mean solution), every local plane — seam halo planes and boundary cells included — what the single-rank solve of \
     * the global grid leaves there (to rounding; P = 1: bit for bit), dPrdtau = 0, divV untouched: multi.jl:175-182 on the   \
     * solution.  p describes the local grid of every rank, p->owns_outlet / p->outlet_val the global x-hi rule, the z halo   \
     * flags of p are ignored.  x and y are transformed on each rank's planes, z on a y chunk of every plane between two      \
     * all-to-all transposes; eigenbases and scratch stay with the ranks while the grid, P, the spacings and \
     * the x rule stay the same.  fp32 fields are solved in fp64.  NS3D_ERR_ARG: NS3D_BC_GPU, x/y-decomposed topologies, null \
     * pointers, local grids below 4×4×3. */                                                                \
    int ns3d_poisson_direct_slab_##S(ns3d_mgpu *m, T *const *Pr, T *const *dPrdtau, const T *const *divV,   \
                                     const ns3d_pt_params *p);                                              \
    /* ns3d_diagnostics of the GLOBAL arrays on any topology (z-slabs or Cartesian dims): every local rank runs the monitor on \
     * its own arrays with the seam flags of its coordinates (those of per_rank are ignored; per_rank[l] carries the rank's     \
     * grid, spacings and cylinder origin xco_g …), out_local[l] (may be NULL) receives the rank's own record.  out_global:    \
     * maxima, pr_min and nonfinite combined as ns3d_max_g does (NaN included), sums and counts added in rank order in the     \
     * one-process form — out_local's sums add up to out_global's exactly in that order — and by an all-reduce in the          \
     * one-process-per-GPU form (every process receives the global record).  Pr or C may be NULL (as a list).  Blocks. */      \
    int ns3d_diagnostics_mgpu_##S(ns3d_mgpu *m, const T *const *Vx, const T *const *Vy, const T *const *Vz,  \
                                  const T *const *Pr, const T *const *C, const ns3d_diag_params *per_rank,   \
                                  ns3d_diag *out_global, ns3d_diag *out_local);                              \
    /* Tracers on a decomposed grid, first half: ns3d_tracers_advance_at on every local rank's context with that rank's origin and \
     * the grid's n_g; cap[l] slots per rank (empty and dead slots are inactive particles), U may be NULL.  Both transports.  \
     * Enqueues; blocks only as every mgpu call does without NS3D_ASYNC.  Everything is checked before the first launch. */  \
    int ns3d_tracers_advance_mgpu_##S(ns3d_mgpu *m, double *const *X, unsigned char *const *state, double *const *U, \
                                      const long *cap, T *const *Vx, T *const *Vy, T *const *Vz, double cx, double cy, \
                                      double cz);
NS3D_MGPU_DECL(double, f64)
NS3D_MGPU_DECL(float, f32)
#undef NS3D_MGPU_DECL

#ifdef __cplusplus
}
#endif
#endif /* NS3D_H */
