// ns3d_api_typed.h — the typed entry points of include/ns3d.h (ns3d_<name>_f64 / _f32) as plain code.  ns3d_api.cpp includes this file
// once per element type, inside a namespace that sets T, with NS3D_FN(name) spelling the exported name and NS3D_BC_RULE the shared
// body of the ns3d_bc_* rules: hence no include guard — and no preprocessor conditional, an unset T or NS3D_FN fails to compile.

extern "C" int NS3D_FN(update_tau)(ns3d_ctx *c, T *txx, T *tyy, T *tzz, T *txy, T *txz, T *tyz, const T *Vx, const T *Vy, const T *Vz,
                                   double mu, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 2);
    return finish(c, DISPATCHG(c, dx, dy, dz, update_tau<T>(c->stream, txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, mu, dx, dy, dz, nx, ny, nz)),
                  "update_tau");
}
extern "C" int NS3D_FN(predict_V)(ns3d_ctx *c, T *Vx, T *Vy, T *Vz, const T *txx, const T *tyy, const T *tzz, const T *txy, const T *txz,
                                  const T *tyz, double rho, double g, double dt, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, txx, tyy, tzz, txy, txz, tyz); CHECK_GRID(nx, ny, nz, 2);
    return finish(c, DISPATCHG(c, dx, dy, dz, predict_V<T>(c->stream, Vx, Vy, Vz, txx, tyy, tzz, txy, txz, tyz, rho, g, dt, dx, dy, dz, nx, ny, nz)),
                  "predict_V");
}
extern "C" int NS3D_FN(predict_fused)(ns3d_ctx *c, T *Vx_new, T *Vy_new, T *Vz_new, const T *Vx, const T *Vy, const T *Vz, double mu,
                                      double rho, double g, double dt, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx_new, Vy_new, Vz_new, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 2);
    if (Vx_new == Vx || Vy_new == Vy || Vz_new == Vz)
        return fail(NS3D_ERR_ARG, "ns3d_predict_fused: the predicted velocities need buffers of their own");
    return finish(c, DISPATCHG(c, dx, dy, dz, predict_fused<T>(c->stream, Vx_new, Vy_new, Vz_new, Vx, Vy, Vz, mu, rho, g, dt, dx, dy, dz, nx, ny, nz)),
                  "predict_fused");
}
extern "C" int NS3D_FN(set_cylinder)(ns3d_ctx *c, T *C, T *Vx, T *Vy, T *Vz, double a2, double b2, double ox, double oy, double sinb,
                                     double cosb, double xco_g, double yco_g, double zco_g, double lx, double ly, double lz, double dx,
                                     double dy, double dz, int nx, int ny, int nz)
{
    (void)zco_g; (void)lz; (void)dz;
    CHECK_CTX(c); CHECK_PTRS(C, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 1);
    return finish(c, DISPATCH(c, set_cylinder<T>(c->stream, C, Vx, Vy, Vz, a2, b2, ox, oy, sinb, cosb, 0, xco_g, yco_g, lx, ly, dx, dy, nx, ny, nz)),
                  "set_cylinder");
}
extern "C" int NS3D_FN(set_cylinder_local)(ns3d_ctx *c, T *C, T *Vx, T *Vy, T *Vz, double a2, double b2, double ox, double oy, double sinb,
                                           double cosb, double lx, double ly, double lz, double dx, double dy, double dz, int nx, int ny,
                                           int nz)
{
    (void)lz; (void)dz;
    CHECK_CTX(c); CHECK_PTRS(C, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 1);
    return finish(c, DISPATCH(c, set_cylinder<T>(c->stream, C, Vx, Vy, Vz, a2, b2, ox, oy, sinb, cosb, 1, 0.0, 0.0, lx, ly, dx, dy, nx, ny, nz)),
                  "set_cylinder_local");
}
// ns3d_set_solid / ns3d_solid_momentum: one kernel build for every arithmetic mode (ns3d_solid.hip), hence no DISPATCH
extern "C" int NS3D_FN(set_solid)(ns3d_ctx *c, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, mask); CHECK_GRID(nx, ny, nz, 1);
    return finish(c, ns3d_solid::set_solid<T>(c->stream, C, Vx, Vy, Vz, mask, nx, ny, nz), "set_solid");
}
extern "C" int NS3D_FN(solid_momentum)(ns3d_ctx *c, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny, int nz,
                                       const int *seam_lo, const int *seam_hi, double *mom_host, long long *n_host)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, mask, mom_host, n_host); CHECK_GRID(nx, ny, nz, 3);
    const int zero[3] = {0, 0, 0};
    const int rc = c->solid_dev.reserve(ns3d_solid::momentum_scratch_bytes(nx, ny, nz), ns3d_drain_stream(c));
    if (rc) return rc;
    hipError_t e = ns3d_solid::momentum<T>(c->stream, Vx, Vy, Vz, mask, nx, ny, nz, seam_lo ? seam_lo : zero, seam_hi ? seam_hi : zero,
                                           c->solid_dev.ptr, c->key_dev);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "solid_momentum launch: %s", hipGetErrorString(e)); }
    HIPCHK(c, hipMemcpyAsync(c->key_host, c->key_dev, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 3; ++q) {
        std::memcpy(&mom_host[q], &c->key_host[q], sizeof(double));
        n_host[q] = (long long)c->key_host[3 + q];
    }
    return NS3D_OK;
}
// moving bodies: the same two with a rigid motion (make_motion checks it: nothing is enqueued on a refusal)
extern "C" int NS3D_FN(set_solid_moving)(ns3d_ctx *c, T *C, T *Vx, T *Vy, T *Vz, const unsigned char *mask, const double *motion, double dx,
                                         double dy, double dz, const int *origin, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, mask); CHECK_GRID(nx, ny, nz, 3);
    ns3d_solid::Motion mo;
    if (const int rc = make_motion(__func__, motion, dx, dy, dz, origin, &mo)) return rc;
    return finish(c, ns3d_solid::set_solid_moving<T>(c->stream, C, Vx, Vy, Vz, mask, mo, nx, ny, nz), "set_solid_moving");
}
extern "C" int NS3D_FN(solid_momentum_moving)(ns3d_ctx *c, const T *Vx, const T *Vy, const T *Vz, const unsigned char *mask, int nx, int ny,
                                              int nz, const int *seam_lo, const int *seam_hi, double *mom_host, long long *n_host,
                                              const double *motion, double dx, double dy, double dz, const int *origin)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, mask, mom_host, n_host); CHECK_GRID(nx, ny, nz, 3);
    ns3d_solid::Motion mo;
    if (const int rc0 = make_motion(__func__, motion, dx, dy, dz, origin, &mo)) return rc0;
    const int zero[3] = {0, 0, 0};
    const int rc = c->solid_dev.reserve(ns3d_solid::momentum_scratch_bytes(nx, ny, nz), ns3d_drain_stream(c));
    if (rc) return rc;
    hipError_t e = ns3d_solid::momentum_moving<T>(c->stream, Vx, Vy, Vz, mask, mo, nx, ny, nz, seam_lo ? seam_lo : zero,
                                                  seam_hi ? seam_hi : zero, c->solid_dev.ptr, c->key_dev);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "solid_momentum_moving launch: %s", hipGetErrorString(e)); }
    HIPCHK(c, hipMemcpyAsync(c->key_host, c->key_dev, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < 3; ++q) {
        std::memcpy(&mom_host[q], &c->key_host[q], sizeof(double));
        n_host[q] = (long long)c->key_host[3 + q];
    }
    return NS3D_OK;
}
extern "C" int NS3D_FN(update_divV)(ns3d_ctx *c, T *divV, const T *Vx, const T *Vy, const T *Vz, double dx, double dy, double dz, int nx,
                                    int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(divV, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 1);
    return finish(c, DISPATCHG(c, dx, dy, dz, update_divV<T>(c->stream, divV, Vx, Vy, Vz, dx, dy, dz, nx, ny, nz)), "update_divV");
}
extern "C" int NS3D_FN(update_dPrdtau)(ns3d_ctx *c, const T *Pr, T *dPrdtau, const T *divV, double rho, double dt, double dtau, double damp,
                                       double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Pr, dPrdtau, divV); CHECK_GRID(nx, ny, nz, 3);
    return finish(c, DISPATCHG(c, dx, dy, dz, update_dPrdtau<T>(c->stream, Pr, dPrdtau, divV, rho, dt, dtau, damp, dx, dy, dz, nx, ny, nz)),
                  "update_dPrdtau");
}
extern "C" int NS3D_FN(update_Pr)(ns3d_ctx *c, T *Pr, const T *dPrdtau, double dtau, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Pr, dPrdtau); CHECK_GRID(nx, ny, nz, 3);
    return finish(c, DISPATCH(c, update_Pr<T>(c->stream, Pr, dPrdtau, dtau, nx, ny, nz)), "update_Pr");
}
extern "C" int NS3D_FN(compute_res)(ns3d_ctx *c, T *Rp, const T *Pr, const T *divV, double rho, double dt, double dx, double dy, double dz,
                                    int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Rp, Pr, divV); CHECK_GRID(nx, ny, nz, 3);
    return finish(c, DISPATCHG(c, dx, dy, dz, compute_res<T>(c->stream, Rp, Pr, divV, rho, dt, dx, dy, dz, nx, ny, nz)), "compute_res");
}
extern "C" int NS3D_FN(max_abs)(ns3d_ctx *c, const T *A, long n, double *out_host)
{
    CHECK_CTX(c); CHECK_PTRS(A, out_host);
    if (n < 0) return fail(NS3D_ERR_ARG, "ns3d_max_abs: negative length");
    hipError_t e = DISPATCH(c, max_abs_key<T>(c->stream, A, n, c->key_dev));
    if (e != hipSuccess) return fail(NS3D_ERR_HIP, "max_abs launch: %s", hipGetErrorString(e));
    return fetch_key(c, c->stream, out_host);
}
extern "C" int NS3D_FN(diagnostics)(ns3d_ctx *c, const T *Vx, const T *Vy, const T *Vz, const T *Pr, const T *C, const ns3d_diag_params *p,
                                    ns3d_diag *out_host)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, out_host);
    int rc = ns3d_diag_check(p, "ns3d_diagnostics");
    if (rc) return rc;
    rc = ns3d_diag_enqueue<T>(c, Vx, Vy, Vz, Pr, C, p);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ns3d_diag_decode(c->diag_host, p, Pr != nullptr, C != nullptr, out_host);
    return NS3D_OK;
}
extern "C" int NS3D_FN(stats_accumulate)(ns3d_ctx *c, double *St, const T *Vx, const T *Vy, const T *Vz, const T *Pr, double weight, int nx,
                                         int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(St, Vx, Vy, Vz);
    const int rc = stats_grid_check(nx, ny, nz, "ns3d_stats_accumulate");
    if (rc) return rc;
    if (!std::isfinite(weight)) return fail(NS3D_ERR_ARG, "ns3d_stats_accumulate: weight = %g is not finite", weight);
    return finish(c, DISPATCH(c, stats_accumulate<T>(c->stream, St, Vx, Vy, Vz, Pr, weight, nx, ny, nz)), "stats_accumulate");
}
extern "C" int NS3D_FN(vortex)(ns3d_ctx *c, T *Wx, T *Wy, T *Wz, T *Q, const T *Vx, const T *Vy, const T *Vz, double dx, double dy, double dz,
                               int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz);
    if (!Wx && !Wy && !Wz && !Q) return fail(NS3D_ERR_ARG, "%s: all four outputs are NULL", __func__);
    CHECK_GRID(nx, ny, nz, 3);
    if (!(std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dz) && dx > 0.0 && dy > 0.0 && dz > 0.0))
        return fail(NS3D_ERR_ARG, "%s: spacings %g, %g, %g (need finite values > 0)", __func__, dx, dy, dz);
    return finish(c, DISPATCHG(c, dx, dy, dz, vortex<T>(c->stream, Wx, Wy, Wz, Q, Vx, Vy, Vz, dx, dy, dz, nx, ny, nz)), "vortex");
}
// ns3d_eddy_viscosity / ns3d_update_tau_var / ns3d_predict_var: the Smagorinsky model and the predictor under a viscosity field
static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const char *p = (const char *)a, *q = (const char *)b;
    return p < q + nb && q < p + na;
}
extern "C" int NS3D_FN(eddy_viscosity)(ns3d_ctx *c, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho, double length,
                                       double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(mu_e, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 3);
    if (!(std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dz) && dx > 0.0 && dy > 0.0 && dz > 0.0))
        return fail(NS3D_ERR_ARG, "%s: spacings %g, %g, %g (need finite values > 0)", __func__, dx, dy, dz);
    if (!(std::isfinite(mu) && std::isfinite(rho) && std::isfinite(length) && mu >= 0.0 && rho >= 0.0 && length >= 0.0))
        return fail(NS3D_ERR_ARG, "%s: mu = %g, rho = %g, length = %g (need finite values >= 0)", __func__, mu, rho, length);
    const size_t cells = (size_t)nx * ny * nz * sizeof(T);
    if (overlaps(mu_e, cells, Vx, cells + (size_t)ny * nz * sizeof(T)) || overlaps(mu_e, cells, Vy, cells + (size_t)nx * nz * sizeof(T)) ||
        overlaps(mu_e, cells, Vz, cells + (size_t)nx * ny * sizeof(T)))
        return fail(NS3D_ERR_ARG, "%s: mu_e must not alias a velocity array", __func__);
    return finish(c, DISPATCHG(c, dx, dy, dz, eddy_viscosity<T>(c->stream, mu_e, Vx, Vy, Vz, mu, rho, length, dx, dy, dz, nx, ny, nz)),
                  "eddy_viscosity");
}
extern "C" int NS3D_FN(sgs_viscosity)(ns3d_ctx *c, int op, T *mu_e, const T *Vx, const T *Vy, const T *Vz, double mu, double rho,
                                      double length, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(mu_e, Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 3);
    if (op != NS3D_SGS_SMAGORINSKY && op != NS3D_SGS_WALE && op != NS3D_SGS_VREMAN)
        return fail(NS3D_ERR_ARG, "%s: operator %d (NS3D_SGS_SMAGORINSKY | NS3D_SGS_WALE | NS3D_SGS_VREMAN)", __func__, op);
    if (!(std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dz) && dx > 0.0 && dy > 0.0 && dz > 0.0))
        return fail(NS3D_ERR_ARG, "%s: spacings %g, %g, %g (need finite values > 0)", __func__, dx, dy, dz);
    if (!(std::isfinite(mu) && std::isfinite(rho) && std::isfinite(length) && mu >= 0.0 && rho >= 0.0 && length >= 0.0))
        return fail(NS3D_ERR_ARG, "%s: mu = %g, rho = %g, length = %g (need finite values >= 0)", __func__, mu, rho, length);
    const size_t cells = (size_t)nx * ny * nz * sizeof(T);
    if (overlaps(mu_e, cells, Vx, cells + (size_t)ny * nz * sizeof(T)) || overlaps(mu_e, cells, Vy, cells + (size_t)nx * nz * sizeof(T)) ||
        overlaps(mu_e, cells, Vz, cells + (size_t)nx * ny * sizeof(T)))
        return fail(NS3D_ERR_ARG, "%s: mu_e must not alias a velocity array", __func__);
    return finish(c, DISPATCHG(c, dx, dy, dz, sgs_viscosity<T>(c->stream, op, mu_e, Vx, Vy, Vz, mu, rho, length, dx, dy, dz, nx, ny, nz)),
                  "sgs_viscosity");
}
extern "C" int NS3D_FN(update_tau_var)(ns3d_ctx *c, T *txx, T *tyy, T *tzz, T *txy, T *txz, T *tyz, const T *Vx, const T *Vy, const T *Vz,
                                       const T *mu_e, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, mu_e); CHECK_GRID(nx, ny, nz, 2);
    return finish(c, DISPATCHG(c, dx, dy, dz, update_tau_var<T>(c->stream, txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, mu_e, dx, dy, dz, nx, ny, nz)),
                  "update_tau_var");
}
extern "C" int NS3D_FN(predict_var)(ns3d_ctx *c, T *Vx_new, T *Vy_new, T *Vz_new, const T *Vx, const T *Vy, const T *Vz, const T *mu_e,
                                    double rho, double g, double dt, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx_new, Vy_new, Vz_new, Vx, Vy, Vz, mu_e); CHECK_GRID(nx, ny, nz, 2);
    if (Vx_new == Vx || Vy_new == Vy || Vz_new == Vz)
        return fail(NS3D_ERR_ARG, "%s: the predicted velocities need buffers of their own", __func__);
    return finish(c, DISPATCHG(c, dx, dy, dz, predict_var<T>(c->stream, Vx_new, Vy_new, Vz_new, Vx, Vy, Vz, mu_e, rho, g, dt, dx, dy, dz, nx, ny, nz)),
                  "predict_var");
}
// ns3d_scalar_diffuse / ns3d_buoyancy / ns3d_scalar_step (ns3d_scalar.hip): one kernel template, `what` selects its halves
static int scalar_check(const char *fn, double kappa, double sgs, double mu, double bg, double c_ref, double dt, double dx, double dy,
                        double dz)
{
    if (!(std::isfinite(dx) && std::isfinite(dy) && std::isfinite(dz) && dx > 0.0 && dy > 0.0 && dz > 0.0))
        return fail(NS3D_ERR_ARG, "%s: spacings %g, %g, %g (need finite values > 0)", fn, dx, dy, dz);
    if (!(std::isfinite(kappa) && std::isfinite(sgs) && kappa >= 0.0 && sgs >= 0.0))
        return fail(NS3D_ERR_ARG, "%s: kappa = %g, sgs = %g (need finite values >= 0)", fn, kappa, sgs);
    if (!(std::isfinite(mu) && std::isfinite(bg) && std::isfinite(c_ref) && std::isfinite(dt)))
        return fail(NS3D_ERR_ARG, "%s: mu = %g, bg = %g, c_ref = %g, dt = %g (need finite values)", fn, mu, bg, c_ref, dt);
    return NS3D_OK;
}
extern "C" int NS3D_FN(scalar_diffuse)(ns3d_ctx *c, T *C_out, const T *C, const T *mu_e, double kappa, double sgs, double mu, double dt,
                                       double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(C_out, C); CHECK_GRID(nx, ny, nz, 3);
    const int rc = scalar_check(__func__, kappa, sgs, mu, 0.0, 0.0, dt, dx, dy, dz);
    if (rc) return rc;
    if (C_out == C) return fail(NS3D_ERR_ARG, "%s: C_out needs a buffer of its own", __func__);
    return finish(c, DISPATCHG(c, dx, dy, dz, scalar_step<T>(c->stream, 1, C_out, (T *)nullptr, C, mu_e, kappa, sgs, mu, 0.0, 0.0, dt, dx, dy, dz,
                                                             nx, ny, nz)), "scalar_diffuse");
}
extern "C" int NS3D_FN(buoyancy)(ns3d_ctx *c, T *Vz, const T *C, double bg, double c_ref, double dt, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vz, C); CHECK_GRID(nx, ny, nz, 3);
    const int rc = scalar_check(__func__, 0.0, 0.0, 0.0, bg, c_ref, dt, 1.0, 1.0, 1.0);
    if (rc) return rc;
    // no division in this half: the spacings only pick a build, and every build of it is the same statement
    return finish(c, DISPATCH(c, scalar_step<T>(c->stream, 2, (T *)nullptr, Vz, C, (const T *)nullptr, 0.0, 0.0, 0.0, bg, c_ref, dt, 1.0, 1.0,
                                                1.0, nx, ny, nz)), "buoyancy");
}
extern "C" int NS3D_FN(scalar_step)(ns3d_ctx *c, T *C_out, T *Vz, const T *C, const T *mu_e, double kappa, double sgs, double mu, double bg,
                                    double c_ref, double dt, double dx, double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(C_out, C); CHECK_GRID(nx, ny, nz, 3);
    const int rc = scalar_check(__func__, kappa, sgs, mu, bg, c_ref, dt, dx, dy, dz);
    if (rc) return rc;
    if (bg != 0.0 && !Vz) return fail(NS3D_ERR_ARG, "%s: null field pointer (Vz, with bg != 0)", __func__);
    if (C_out == C) return fail(NS3D_ERR_ARG, "%s: C_out needs a buffer of its own", __func__);
    return finish(c, DISPATCHG(c, dx, dy, dz, scalar_step<T>(c->stream, bg != 0.0 ? 3 : 1, C_out, Vz, C, mu_e, kappa, sgs, mu, bg, c_ref, dt, dx,
                                                             dy, dz, nx, ny, nz)), "scalar_step");
}
// ns3d_sample / ns3d_tracers_advance: one kernel build for every arithmetic mode (ns3d_tracers.hip), hence no DISPATCH
static int tracers_count_check(long n, const char *fn)
{
    if (n < 0) return fail(NS3D_ERR_ARG, "%s: n = %ld is negative", fn, n);
    if (n > 256L * 0x7fffffffL) return fail(NS3D_ERR_ARG, "%s: n = %ld exceeds one launch (256 x 2^31 points)", fn, n);
    return NS3D_OK;
}
extern "C" int NS3D_FN(sample)(ns3d_ctx *c, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey,
                               int ez, int stag_x, int stag_y, int stag_z)
{
    CHECK_CTX(c); CHECK_PTRS(out, X, A);
    const int rc = tracers_count_check(n, __func__);
    if (rc) return rc;
    if (ex < 2 || ey < 2 || ez < 2) return fail(NS3D_ERR_ARG, "%s: extents %dx%dx%d too small (need >= 2 per direction)", __func__, ex, ey, ez);
    if ((stag_x | stag_y | stag_z) & ~1)
        return fail(NS3D_ERR_ARG, "%s: stagger flags %d, %d, %d (each 0 or 1)", __func__, stag_x, stag_y, stag_z);
    if (n == 0) return NS3D_OK;
    return finish(c, ns3d_tracers::sample<T>(c->stream, out, X, state, n, A, ex, ey, ez, stag_x, stag_y, stag_z), "sample");
}
extern "C" int NS3D_FN(tracers_advance)(ns3d_ctx *c, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy,
                                        const T *Vz, double cx, double cy, double cz, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(X, state, Vx, Vy, Vz);
    const int rc = tracers_count_check(n, __func__);
    if (rc) return rc;
    CHECK_GRID(nx, ny, nz, 3);
    if (!(std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz)))
        return fail(NS3D_ERR_ARG, "%s: Courant factors %g, %g, %g (need finite values)", __func__, cx, cy, cz);
    if (n == 0) return NS3D_OK;
    return finish(c, ns3d_tracers::advance<T>(c->stream, X, state, U, n, Vx, Vy, Vz, cx, cy, cz, nx, ny, nz), "tracers_advance");
}
// the origin forms for the ranks of a decomposed grid: positions in the global index space, interpolation at X - origin
extern "C" int NS3D_FN(sample_at)(ns3d_ctx *c, double *out, const double *X, const unsigned char *state, long n, const T *A, int ex, int ey,
                                  int ez, int stag_x, int stag_y, int stag_z, const int *origin)
{
    CHECK_CTX(c); CHECK_PTRS(out, X, A);
    const int rc = tracers_count_check(n, __func__);
    if (rc) return rc;
    if (ex < 2 || ey < 2 || ez < 2) return fail(NS3D_ERR_ARG, "%s: extents %dx%dx%d too small (need >= 2 per direction)", __func__, ex, ey, ez);
    if ((stag_x | stag_y | stag_z) & ~1)
        return fail(NS3D_ERR_ARG, "%s: stagger flags %d, %d, %d (each 0 or 1)", __func__, stag_x, stag_y, stag_z);
    const int zero[3] = {0, 0, 0};
    const int *o = origin ? origin : zero;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0) return fail(NS3D_ERR_ARG, "%s: origin %d, %d, %d (each >= 0)", __func__, o[0], o[1], o[2]);
    if (n == 0) return NS3D_OK;
    return finish(c, ns3d_tracers::sample_at<T>(c->stream, out, X, state, n, A, ex, ey, ez, stag_x, stag_y, stag_z, o), "sample_at");
}
extern "C" int NS3D_FN(tracers_advance_at)(ns3d_ctx *c, double *X, unsigned char *state, double *U, long n, const T *Vx, const T *Vy,
                                           const T *Vz, double cx, double cy, double cz, int nx, int ny, int nz, const int *origin,
                                           const int *n_g)
{
    CHECK_CTX(c); CHECK_PTRS(X, state, Vx, Vy, Vz);
    const int rc = tracers_count_check(n, __func__);
    if (rc) return rc;
    CHECK_GRID(nx, ny, nz, 3);
    if (!(std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz)))
        return fail(NS3D_ERR_ARG, "%s: Courant factors %g, %g, %g (need finite values)", __func__, cx, cy, cz);
    const int zero[3] = {0, 0, 0}, loc[3] = {nx, ny, nz};
    const int *o = origin ? origin : zero;
    if (o[0] < 0 || o[1] < 0 || o[2] < 0) return fail(NS3D_ERR_ARG, "%s: origin %d, %d, %d (each >= 0)", __func__, o[0], o[1], o[2]);
    int g[3];
    for (int q = 0; q < 3; ++q) {
        g[q] = n_g ? n_g[q] : loc[q];
        if ((long)g[q] < (long)o[q] + loc[q])
            return fail(NS3D_ERR_ARG, "%s: global grid %d in direction %d is smaller than origin %d + local grid %d", __func__, g[q], q, o[q],
                        loc[q]);
    }
    if (n == 0) return NS3D_OK;
    return finish(c, ns3d_tracers::advance_at<T>(c->stream, X, state, U, n, Vx, Vy, Vz, cx, cy, cz, nx, ny, nz, o, g), "tracers_advance_at");
}
// ns3d_isosurface: count, scan and read the total back (blocking); then, where there is room for triangles, the emit launch
extern "C" int NS3D_FN(isosurface)(ns3d_ctx *c, const T *A, const T *B, int ex, int ey, int ez, const int *box, const int *origin, double iso,
                                   double *tri, double *val, long long cap, long long *n_tri_host)
{
    CHECK_CTX(c); CHECK_PTRS(A, n_tri_host);
    ns3d_iso_geom g;
    ns3d_iso_scratch w;
    const int rc = iso_prepare(c, ex, ey, ez, box, origin, iso, tri, val, B, cap, __func__, &g, &w);
    if (rc) return rc;
    hipError_t e = ns3d_iso::count_scan<T>(c->stream, A, g, iso, w);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(NS3D_ERR_HIP, "isosurface count launch: %s", hipGetErrorString(e)); }
    HIPCHK(c, hipMemcpyAsync(c->key_host, w.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const long long n = (long long)c->key_host[0];
    *n_tri_host = n;
    if (n == 0 || cap == 0) return NS3D_OK;
    return finish(c, ns3d_iso::emit<T>(c->stream, A, B, g, iso, w, tri, val, cap), "isosurface");
}
extern "C" int NS3D_FN(correct_V)(ns3d_ctx *c, T *Vx, T *Vy, T *Vz, const T *Pr, double dt, double rho, double dx, double dy, double dz,
                                  int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz, Pr); CHECK_GRID(nx, ny, nz, 2);
    return finish(c, DISPATCHG(c, dx, dy, dz, correct_V<T>(c->stream, Vx, Vy, Vz, Pr, dt, rho, dx, dy, dz, nx, ny, nz)), "correct_V");
}
// one boundary-plane rule; its context and pointer errors carry THIS function's name (__func__), not the entry point's
static int NS3D_BC_RULE(ns3d_ctx *c, int which, T *A, int sx, int sy, int sz, double a, double b, int nz_arg, const char *name)
{
    CHECK_CTX(c); CHECK_PTRS(A);
    if (sx < 2 || sy < 2 || sz < 2) return fail(NS3D_ERR_ARG, "%s: extents %dx%dx%d too small", name, sx, sy, sz);
    return finish(c, DISPATCH(c, bc_plane<T>(c->stream, which, A, sx, sy, sz, a, b, 0.0, nz_arg)), name);
}
extern "C" int NS3D_FN(bc_x)(ns3d_ctx *c, T *A, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 0, A, sx, sy, sz, 0, 0, 0, "bc_x"); }
extern "C" int NS3D_FN(bc_y)(ns3d_ctx *c, T *A, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 1, A, sx, sy, sz, 0, 0, 0, "bc_y"); }
extern "C" int NS3D_FN(bc_z)(ns3d_ctx *c, T *A, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 2, A, sx, sy, sz, 0, 0, 0, "bc_z"); }
extern "C" int NS3D_FN(bc_zV)(ns3d_ctx *c, T *A, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 3, A, sx, sy, sz, 0, 0, 0, "bc_zV"); }
extern "C" int NS3D_FN(bc_xhydstatic)(ns3d_ctx *c, T *A, double dz, int nz, double g, double rho, int sx, int sy, int sz)
{
    return NS3D_BC_RULE(c, 4, A, sx, sy, sz, (double)((T)rho * (T)g), dz, nz, "bc_xhydstatic");
}
extern "C" int NS3D_FN(bc_x_Vx)(ns3d_ctx *c, T *A, double V, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 5, A, sx, sy, sz, V, 0, 0, "bc_x_Vx"); }
extern "C" int NS3D_FN(bc_x_Pr)(ns3d_ctx *c, T *A, double v, int sx, int sy, int sz) { return NS3D_BC_RULE(c, 6, A, sx, sy, sz, v, 0, 0, "bc_x_Pr"); }
extern "C" int NS3D_FN(copy)(ns3d_ctx *c, T *dst, const T *src, long n)
{
    CHECK_CTX(c); CHECK_PTRS(dst, src);
    if (n < 0) return fail(NS3D_ERR_ARG, "ns3d_copy: negative length");
    return finish(c, hipMemcpyAsync(dst, src, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, c->stream), "copy");
}
extern "C" int NS3D_FN(advect)(ns3d_ctx *c, T *Vx, const T *Vx_o, T *Vy, const T *Vy_o, T *Vz, const T *Vz_o, T *C, const T *C_o, double dt,
                               double dx, double dy, double dz, int nx, int ny, int nz, int faithful)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vx_o, Vy, Vy_o, Vz, Vz_o, C, C_o); CHECK_GRID(nx, ny, nz, 1);
    return finish(c, DISPATCHG(c, dx, dy, dz, advect<T>(c->stream, Vx, Vx_o, Vy, Vy_o, Vz, Vz_o, C, C_o, dt, dx, dy, dz, nx, ny, nz,
                                                        faithful ? 1 : 0, 0, 0)), "advect");
}
extern "C" int NS3D_FN(copy_advect)(ns3d_ctx *c, T *Vx_new, const T *Vx, T *Vy_new, const T *Vy, T *Vz_new, const T *Vz, T *C_new,
                                    const T *C, double dt, double dx, double dy, double dz, int nx, int ny, int nz, int faithful)
{
    CHECK_CTX(c); CHECK_PTRS(Vx_new, Vx, Vy_new, Vy, Vz_new, Vz, C_new, C); CHECK_GRID(nx, ny, nz, 1);
    if (Vx_new == Vx || Vy_new == Vy || C_new == C || (!faithful && Vz_new == Vz))
        return fail(NS3D_ERR_ARG, "ns3d_copy_advect: outputs must be buffers of their own (only Vz_new may be Vz, and only "
                                  "in faithful mode, where Vz is never advected)");
    return finish(c, DISPATCHG(c, dx, dy, dz, advect<T>(c->stream, Vx_new, Vx, Vy_new, Vy, Vz_new, Vz, C_new, C, dt, dx, dy, dz, nx, ny, nz,
                                                        (faithful ? 1 : 0) | 2, 0, 0)), "copy_advect");
}
// ns3d_advect_correct / ns3d_advect_mc: the checks both share, under the entry point's name
static int advect_mc_check(const char *fn, const void *const (&a)[12], int nx, int ny, int nz)
{
    for (int q = 0; q < 12; ++q)
        if (!a[q]) return fail(NS3D_ERR_ARG, "%s: null field pointer (argument %d)", fn, q);
    if (nx < 3 || ny < 3 || nz < 3) return fail(NS3D_ERR_ARG, "%s: grid %dx%dx%d too small (need >= 3 per direction)", fn, nx, ny, nz);
    for (int q = 0; q < 12; ++q)
        for (int r = q + 1; r < 12; ++r)
            if (a[q] == a[r]) return fail(NS3D_ERR_ARG, "%s: arguments %d and %d are the same array (twelve distinct arrays)", fn, q, r);
    return NS3D_OK;
}
extern "C" int NS3D_FN(advect_correct)(ns3d_ctx *c, T *Vx_new, const T *Vx, const T *Vx_hat, T *Vy_new, const T *Vy, const T *Vy_hat,
                                       T *Vz_new, const T *Vz, const T *Vz_hat, T *C_new, const T *C, const T *C_hat, double dt, double dx,
                                       double dy, double dz, int nx, int ny, int nz)
{
    CHECK_CTX(c);
    const void *const a[12] = {Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, C, C_hat};
    if (const int rc = advect_mc_check(__func__, a, nx, ny, nz)) return rc;
    return finish(c, DISPATCHG(c, dx, dy, dz, advect_mc<T>(c->stream, Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, C,
                                                           C_hat, dt, dx, dy, dz, nx, ny, nz)), "advect_correct");
}
extern "C" int NS3D_FN(advect_mc)(ns3d_ctx *c, T *Vx_new, const T *Vx, T *Vx_hat, T *Vy_new, const T *Vy, T *Vy_hat, T *Vz_new, const T *Vz,
                                  T *Vz_hat, T *C_new, const T *C, T *C_hat, double dt, double dx, double dy, double dz, int nx, int ny,
                                  int nz)
{
    CHECK_CTX(c);
    const void *const a[12] = {Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, C, C_hat};
    if (const int rc = advect_mc_check(__func__, a, nx, ny, nz)) return rc;
    // stage 1: ns3d_copy_advect(faithful = 0) into the hat buffers; stage 2 behind it on the same stream
    hipError_t e = DISPATCHG(c, dx, dy, dz, advect<T>(c->stream, Vx_hat, Vx, Vy_hat, Vy, Vz_hat, Vz, C_hat, C, dt, dx, dy, dz, nx, ny, nz, 2, 0, 0));
    if (e == hipSuccess)
        e = DISPATCHG(c, dx, dy, dz, advect_mc<T>(c->stream, Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, C, C_hat, dt,
                                                  dx, dy, dz, nx, ny, nz));
    return finish(c, e, "advect_mc");
}
extern "C" int NS3D_FN(set_bc_Pr)(ns3d_ctx *c, T *Pr, int bc_kind, int owns_outlet, double outlet_val, double dz, int nz_arg, double g,
                                  double rho, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Pr); CHECK_GRID(nx, ny, nz, 2);
    hipError_t e = hipSuccess;
    hipStream_t s = c->stream;
    if (bc_kind != NS3D_BC_MULTI && bc_kind != NS3D_BC_GPU) return fail(NS3D_ERR_ARG, "ns3d_set_bc_Pr: bad bc_kind %d", bc_kind);
    if (bc_fused_enabled()) {       // the whole sequence as one gather launch (k_bc_fused)
        e = DISPATCH(c, bc_fused<T>(s, 1, bc_kind, Pr, (T *)nullptr, (T *)nullptr, nx, ny, nz, owns_outlet, outlet_val,
                                    (double)((T)rho * (T)g), dz, nz_arg));
        if (e != hipErrorInvalidValue) return finish(c, e, "set_bc_Pr");
        (void)hipGetLastError();
        e = hipSuccess;
    }
    if (bc_kind == NS3D_BC_MULTI) { // multi.jl:176-181
        e = DISPATCH(c, bc_plane<T>(s, 0, Pr, nx, ny, nz, 0, 0, 0, 0));
        if (e == hipSuccess) e = DISPATCH(c, bc_plane<T>(s, 1, Pr, nx, ny, nz, 0, 0, 0, 0));
        if (e == hipSuccess) e = DISPATCH(c, bc_plane<T>(s, 2, Pr, nx, ny, nz, 0, 0, 0, 0));
        if (e == hipSuccess && owns_outlet) e = DISPATCH(c, bc_plane<T>(s, 6, Pr, nx, ny, nz, outlet_val, 0, 0, 0));
    } else if (bc_kind == NS3D_BC_GPU) { // gpu.jl:282-284
        e = DISPATCH(c, bc_plane<T>(s, 1, Pr, nx, ny, nz, 0, 0, 0, 0));
        if (e == hipSuccess) e = DISPATCH(c, bc_plane<T>(s, 2, Pr, nx, ny, nz, 0, 0, 0, 0));
        if (e == hipSuccess) e = DISPATCH(c, bc_plane<T>(s, 4, Pr, nx, ny, nz, (double)((T)rho * (T)g), dz, 0, nz_arg));
    }
    return finish(c, e, "set_bc_Pr");
}
extern "C" int NS3D_FN(set_bc_Vel)(ns3d_ctx *c, T *Vx, T *Vy, T *Vz, int bc_kind, int owns_inlet, double vin, int nx, int ny, int nz)
{
    CHECK_CTX(c); CHECK_PTRS(Vx, Vy, Vz); CHECK_GRID(nx, ny, nz, 2);
    hipStream_t s = c->stream;
    hipError_t e = hipSuccess;
    if (bc_kind != NS3D_BC_MULTI && bc_kind != NS3D_BC_GPU) return fail(NS3D_ERR_ARG, "ns3d_set_bc_Vel: bad bc_kind %d", bc_kind);
    if (bc_fused_enabled()) {       // the whole sequence as one gather launch (k_bc_fused)
        e = DISPATCH(c, bc_fused<T>(s, 0, bc_kind, Vx, Vy, Vz, nx, ny, nz, bc_kind == NS3D_BC_MULTI && owns_inlet, vin, 0.0, 0.0, 0));
        if (e != hipErrorInvalidValue) return finish(c, e, "set_bc_Vel");
        (void)hipGetLastError();
        e = hipSuccess;
    }
    struct { int which; T *A; int sx, sy, sz; } seq[9];
    int n = 0;
    if (bc_kind == NS3D_BC_MULTI) { // multi.jl:157-163
        seq[n++] = {0, Vx, nx + 1, ny, nz}; seq[n++] = {1, Vx, nx + 1, ny, nz}; seq[n++] = {2, Vx, nx + 1, ny, nz};
        seq[n++] = {0, Vy, nx, ny + 1, nz}; seq[n++] = {2, Vy, nx, ny + 1, nz};
        seq[n++] = {0, Vz, nx, ny, nz + 1}; seq[n++] = {1, Vz, nx, ny, nz + 1};
    } else if (bc_kind == NS3D_BC_GPU) { // gpu.jl:265-276
        seq[n++] = {0, Vx, nx + 1, ny, nz}; seq[n++] = {1, Vx, nx + 1, ny, nz}; seq[n++] = {3, Vx, nx + 1, ny, nz};
        seq[n++] = {0, Vy, nx, ny + 1, nz}; seq[n++] = {1, Vy, nx, ny + 1, nz}; seq[n++] = {3, Vy, nx, ny + 1, nz};
        seq[n++] = {0, Vz, nx, ny, nz + 1}; seq[n++] = {1, Vz, nx, ny, nz + 1}; seq[n++] = {3, Vz, nx, ny, nz + 1};
    }
    for (int q = 0; q < n && e == hipSuccess; ++q)
        e = DISPATCH(c, bc_plane<T>(s, seq[q].which, seq[q].A, seq[q].sx, seq[q].sy, seq[q].sz, 0, 0, 0, 0));
    if (e == hipSuccess && bc_kind == NS3D_BC_MULTI && owns_inlet) // multi.jl:164-166
        e = DISPATCH(c, bc_plane<T>(s, 5, Vx, nx + 1, ny, nz, vin, 0, 0, 0));
    return finish(c, e, "set_bc_Vel");
}
extern "C" int NS3D_FN(pt_iterate)(ns3d_ctx *c, T *Pr, T *dPrdtau, const T *divV, const ns3d_pt_params *p, int n_iters)
{
    CHECK_CTX(c); CHECK_PTRS(Pr, dPrdtau, divV);
    int rc = ns3d_check_pt_params(p, "ns3d_pt_iterate");
    if (rc) return rc;
    if ((rc = pt_iterate_impl<T>(c, Pr, dPrdtau, divV, p, n_iters))) return rc;
    return finish(c, hipSuccess, "pt_iterate");
}
extern "C" int NS3D_FN(pt_sweep)(ns3d_ctx *c, const T *Pr_in, T *Pr_out, T *dPrdtau, const T *divV, const ns3d_pt_params *p, int k0, int k1)
{
    CHECK_CTX(c); CHECK_PTRS(Pr_in, Pr_out, dPrdtau, divV);
    int rc = ns3d_check_pt_params(p, "ns3d_pt_sweep");
    if (rc) return rc;
    if (Pr_in == Pr_out) return fail(NS3D_ERR_ARG, "ns3d_pt_sweep: Pr_in and Pr_out must differ");
    if ((rc = check_planes(p, k0, k1, "ns3d_pt_sweep"))) return rc;
    return finish(c, DISPATCHG(c, p->dx, p->dy, p->dz, pt_sweep<T>(c->stream, c->pt_variant, Pr_in, Pr_out, dPrdtau, divV, *p, k0, k1)), "pt_sweep");
}
extern "C" int NS3D_FN(pt_sweep2)(ns3d_ctx *c, const T *Pr_in, T *Pr_out, const T *dPrdtau, T *dPrdtau_out, const T *divV,
                                  const ns3d_pt_params *p, int k0, int k1)
{
    CHECK_CTX(c); CHECK_PTRS(Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV);
    if (dPrdtau == dPrdtau_out) return fail(NS3D_ERR_ARG, "ns3d_pt_sweep2: dPrdtau_in and dPrdtau_out must differ");
    int rc = ns3d_check_pt_params(p, "ns3d_pt_sweep2");
    if (rc) return rc;
    if (Pr_in == Pr_out) return fail(NS3D_ERR_ARG, "ns3d_pt_sweep2: Pr_in and Pr_out must differ");
    if ((rc = check_no_halos(p, "ns3d_pt_sweep2")) || (rc = check_planes(p, k0, k1, "ns3d_pt_sweep2"))) return rc;
    return finish(c, launch_pt2<T>(c, c->stream, Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV, p, k0, k1, false), "pt_sweep2");
}
extern "C" int NS3D_FN(pt_sweepn)(ns3d_ctx *c, int nlev, const T *Pr_in, T *Pr_out, const T *dPrdtau, T *dPrdtau_out, const T *divV,
                                  const ns3d_pt_params *p, int k0, int k1)
{
    CHECK_CTX(c); CHECK_PTRS(Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV);
    int rc = ns3d_check_pt_params(p, "ns3d_pt_sweepn");
    if (rc) return rc;
    if (nlev < 2 || nlev > (sizeof(T) == 4 ? 5 : 4)) return fail(NS3D_ERR_ARG, "ns3d_pt_sweepn: %d levels (2…4; 5 with float32 fields)", nlev);
    if (Pr_in == Pr_out || dPrdtau == dPrdtau_out) return fail(NS3D_ERR_ARG, "ns3d_pt_sweepn: input and output buffers must differ");
    if ((rc = check_no_halos(p, "ns3d_pt_sweepn")) || (rc = check_planes(p, k0, k1, "ns3d_pt_sweepn"))) return rc;
    hipError_t e = ns3d_enqueue_pass<T>(c, c->stream, nlev, Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV, p, k0, k1);
    if (e == hipErrorInvalidValue) return fail(NS3D_ERR_ARG, "ns3d_pt_sweepn: tile variant %d cannot run %d levels", c->ptn_variant, nlev);
    return finish(c, e, "pt_sweepn");
}
extern "C" int NS3D_FN(plan_pt)(ns3d_ctx *c, const T *Pr_in, T *Pr_out, const T *dPrdtau, T *dPrdtau_out, const T *divV,
                                const ns3d_pt_params *p, int k0, int k1)
{
    CHECK_CTX(c); CHECK_PTRS(Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV);
    int rc = ns3d_check_pt_params(p, "ns3d_plan_pt");
    if (rc) return rc;
    if (Pr_in == Pr_out || dPrdtau == dPrdtau_out) return fail(NS3D_ERR_ARG, "ns3d_plan_pt: input and output buffers must differ");
    if ((rc = check_planes(p, k0, k1, "ns3d_plan_pt"))) return rc;
    (void)ns3d_plan_pt_internal<T>(c, Pr_in, Pr_out, dPrdtau, dPrdtau_out, divV, p, k0, k1);
    return finish(c, hipSuccess, "plan_pt");
}
extern "C" int NS3D_FN(residual_max)(ns3d_ctx *c, const T *Pr, const T *divV, const ns3d_pt_params *p, double *out_host)
{
    CHECK_CTX(c); CHECK_PTRS(Pr, divV, out_host);
    int rc = ns3d_check_pt_params(p, "ns3d_residual_max");
    if (rc) return rc;
    hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz, residual_max_key<T>(c->stream, Pr, divV, *p, c->key_dev));
    if (e != hipSuccess) return fail(NS3D_ERR_HIP, "residual launch: %s", hipGetErrorString(e));
    return fetch_key(c, c->stream, out_host);
}
extern "C" int NS3D_FN(selftest_exact_div)(ns3d_ctx *c, double d, long n, unsigned long long seed, long *mismatches)
{
    CHECK_CTX(c); CHECK_PTRS(mismatches);
    if (!recip_ok(d)) return fail(NS3D_ERR_ARG, "ns3d_selftest_exact_div: divisor %g is not eligible", d);
    hipError_t e = ns3d_strictx::divtest<T>(c->stream, d, n, seed, c->key_dev);
    if (e != hipSuccess) return fail(NS3D_ERR_HIP, "divtest launch: %s", hipGetErrorString(e));
    HIPCHK(c, hipMemcpyAsync(c->key_host, c->key_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mismatches = (long)*c->key_host;
    return NS3D_OK;
}
extern "C" int NS3D_FN(pt_solve)(ns3d_ctx *c, T *Pr, T *dPrdtau, const T *divV, const ns3d_pt_params *p, double eps, int niter, int nchk,
                                 double err_mul, double err_div, int *iters_done, double *err_hist, int max_checks, int *n_checks)
{
    CHECK_CTX(c); CHECK_PTRS(Pr, dPrdtau, divV);
    int rc = ns3d_check_pt_params(p, "ns3d_pt_solve");
    if (rc) return rc;
    if (p->z_lo_is_halo || p->z_hi_is_halo)
        return fail(NS3D_ERR_ARG, "ns3d_pt_solve: single-rank loop; drive z-slab ranks with ns3d_pt_sweep + halo exchange");
    if (niter < 0 || nchk < 0) return fail(NS3D_ERR_ARG, "ns3d_pt_solve: negative niter/nchk");
    if ((rc = pt_solve_impl<T>(c, Pr, dPrdtau, divV, p, eps, niter, nchk, err_mul, err_div, iters_done, err_hist, max_checks, n_checks))) return rc;
    return finish(c, hipSuccess, "pt_solve");
}

// ---- one whole time step per call (include/ns3d.h ns3d_time_step) -----------------------------------------------------------
// multi.jl:449-477 on one rank / gpu.jl:121-142 as the fused sequence the Python driver issues call by call — through the SAME entry
// points (argument checks, arithmetic builds and all), with the context switched to non-blocking for the duration so that the residual
// read-backs inside ns3d_pt_solve are the only synchronisations; one synchronisation at the end restores a blocking context's
// contract.  ≈40 host calls per step become one: with the direct pressure solve a step of the 255×153×153 case is otherwise mostly
// the driver's calls.
extern "C" int NS3D_FN(time_step)(ns3d_ctx *c, ns3d_step_fields *f, const ns3d_step_params *p, int *iters_done, double *err_hist,
                                  int max_checks, int *n_checks)
{
    CHECK_CTX(c);
    if (!f || !p) return fail(NS3D_ERR_ARG, "ns3d_time_step: null argument");
    if (p->script != NS3D_BC_MULTI && p->script != NS3D_BC_GPU)
        return fail(NS3D_ERR_ARG, "ns3d_time_step: script %d (NS3D_BC_MULTI: multi.jl, NS3D_BC_GPU: gpu.jl)", p->script);
    if (p->write_stress && !(f->txx && f->tyy && f->tzz && f->txy && f->txz && f->tyz))
        return fail(NS3D_ERR_ARG, "ns3d_time_step: write_stress needs the six stress arrays");
    const int nx = p->nx, ny = p->ny, nz = p->nz;
    const bool maccormack = c->advection == NS3D_ADVECT_MACCORMACK;
    if (maccormack && p->faithful)
        return fail(NS3D_ERR_ARG, "ns3d_time_step: NS3D_ADVECT_MACCORMACK advects Vz: it needs faithful == 0");
    if (c->motion_on && !c->obstacle)
        return fail(NS3D_ERR_ARG, "ns3d_time_step: ns3d_set_obstacle_motion is set without a mask (ns3d_set_obstacle)");
    const int was = c->flags;
    c->flags |= NS3D_ASYNC;
    int rc = NS3D_OK;
    bool deferred_residual = false;
    T *Vx = (T *)f->Vx, *Vy = (T *)f->Vy, *Vz = (T *)f->Vz, *Vxo = (T *)f->Vx_o, *Vyo = (T *)f->Vy_o, *Vzo = (T *)f->Vz_o;
    T *C = (T *)f->C, *Co = (T *)f->C_o, *Pr = (T *)f->Pr, *D = (T *)f->dPrdtau, *divV = (T *)f->divV;
    auto cylinder = [&]() -> int {          // multi.jl:249-281 (global coordinates) / gpu.jl:336-368 (local); ns3d_set_obstacle: the mask
        if (c->motion_on)                   // ns3d_set_obstacle_motion: the body's own velocity where the mask is set
            return NS3D_FN(set_solid_moving)(c, C, Vx, Vy, Vz, c->obstacle, c->motion, p->dx, p->dy, p->dz, c->motion_origin, nx, ny, nz);
        if (c->obstacle) return NS3D_FN(set_solid)(c, C, Vx, Vy, Vz, c->obstacle, nx, ny, nz);
        return p->script == NS3D_BC_MULTI
                   ? NS3D_FN(set_cylinder)(c, C, Vx, Vy, Vz, p->a2, p->b2, p->ox, p->oy, p->sinb, p->cosb, p->xco_g, p->yco_g, p->zco_g, p->lx,
                                           p->ly, p->lz, p->dx, p->dy, p->dz, nx, ny, nz)
                   : NS3D_FN(set_cylinder_local)(c, C, Vx, Vy, Vz, p->a2, p->b2, p->ox, p->oy, p->sinb, p->cosb, p->lx, p->ly, p->lz, p->dx,
                                                 p->dy, p->dz, nx, ny, nz);
    };
    do {
        if (c->turbulence != NS3D_TURB_NONE) {  // ns3d_set_turbulence: μ_e into the caller's array, then the same two statements under it
            T *mu_e = (T *)c->turb_mu_e;
            if ((rc = c->sgs_operator == NS3D_SGS_SMAGORINSKY     // ns3d_set_sgs_operator: which operator forms it
                          ? NS3D_FN(eddy_viscosity)(c, mu_e, Vx, Vy, Vz, p->mu, p->rho, c->turb_length, p->dx, p->dy, p->dz, nx, ny, nz)
                          : NS3D_FN(sgs_viscosity)(c, c->sgs_operator, mu_e, Vx, Vy, Vz, p->mu, p->rho, c->turb_length, p->dx, p->dy, p->dz, nx,
                                                   ny, nz))) break;
            if (p->write_stress && (rc = NS3D_FN(update_tau_var)(c, (T *)f->txx, (T *)f->tyy, (T *)f->tzz, (T *)f->txy, (T *)f->txz,
                                                                 (T *)f->tyz, Vx, Vy, Vz, mu_e, p->dx, p->dy, p->dz, nx, ny, nz))) break;
            if ((rc = NS3D_FN(predict_var)(c, Vxo, Vyo, Vzo, Vx, Vy, Vz, mu_e, p->rho, p->g, p->dt, p->dx, p->dy, p->dz, nx, ny, nz))) break;
        } else {
            if (p->write_stress && (rc = NS3D_FN(update_tau)(c, (T *)f->txx, (T *)f->tyy, (T *)f->tzz, (T *)f->txy, (T *)f->txz, (T *)f->tyz, Vx,
                                                             Vy, Vz, p->mu, p->dx, p->dy, p->dz, nx, ny, nz))) break;
            // :449-451 / :121-122 in one pass; the predicted fields land in the *_o buffers and the names swap
            if ((rc = NS3D_FN(predict_fused)(c, Vxo, Vyo, Vzo, Vx, Vy, Vz, p->mu, p->rho, p->g, p->dt, p->dx, p->dy, p->dz, nx, ny, nz))) break;
        }
        std::swap(Vx, Vxo); std::swap(Vy, Vyo); std::swap(Vz, Vzo);
        if (c->scalar_on) {     // ns3d_set_scalar: C diffuses and lifts the predicted Vz in one pass; the masking below is its Dirichlet wall
            const bool eddy = c->turbulence != NS3D_TURB_NONE && c->scalar_sct > 0.0;
            if ((rc = NS3D_FN(scalar_step)(c, Co, Vz, C, eddy ? (const T *)c->turb_mu_e : nullptr, c->scalar_kappa,
                                           eddy ? 1.0 / (p->rho * c->scalar_sct) : 0.0, p->mu, c->scalar_bg, c->scalar_c_ref, p->dt, p->dx, p->dy,
                                           p->dz, nx, ny, nz))) break;
            std::swap(C, Co);
        }
        if ((rc = cylinder())) break;                                                                               // :452 / :123
        if ((rc = NS3D_FN(update_divV)(c, divV, Vx, Vy, Vz, p->dx, p->dy, p->dz, nx, ny, nz))) break;               // :454 / :124
        ns3d_pt_params pt;
        pt.rho = p->rho; pt.dt = p->dt; pt.dtau = p->dtau; pt.damp = p->damp; pt.dx = p->dx; pt.dy = p->dy; pt.dz = p->dz;
        pt.nx = nx; pt.ny = ny; pt.nz = nz; pt.bc_kind = p->script; pt.owns_outlet = p->script == NS3D_BC_MULTI ? p->owns_outlet : 0;
        pt.outlet_val = 0.0; pt.g = p->g; pt.z_lo_is_halo = 0; pt.z_hi_is_halo = 0;
        if (p->pressure == 1) {             // outside parity: the exact solution of what :458-471 iterates towards
            if ((rc = NS3D_FN(poisson_direct)(c, Pr, D, divV, &pt))) break;
            // its residual steers nothing: the 8 bytes come back behind the REST of the step (read after the final synchronisation)
            // instead of stalling the stream in the middle of it
            hipError_t e = DISPATCHG(c, p->dx, p->dy, p->dz, residual_max_key<T>(c->stream, Pr, divV, pt, c->key_dev));
            if (e == hipSuccess) e = hipMemcpyAsync(c->key_host, c->key_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) { rc = fail(NS3D_ERR_HIP, "ns3d_time_step: residual launch: %s", hipGetErrorString(e)); break; }
            deferred_residual = true;
        } else if ((rc = NS3D_FN(pt_solve)(c, Pr, D, divV, &pt, p->eps, p->niter, p->nchk, p->err_mul, p->err_div, iters_done, err_hist,
                                           max_checks, n_checks))) break;                                           // :458-471 / :126-137
        if ((rc = NS3D_FN(correct_V)(c, Vx, Vy, Vz, Pr, p->dt, p->rho, p->dx, p->dy, p->dz, nx, ny, nz))) break;    // :472 / :138
        if ((rc = cylinder())) break;                                                                               // :473 / :139
        if ((rc = NS3D_FN(set_bc_Vel)(c, Vx, Vy, Vz, p->script, p->script == NS3D_BC_MULTI ? p->owns_inlet : 0, p->vin, nx, ny, nz))) break;
        if (maccormack) {       // ns3d_set_advection: stage 1 into the context's hat fields, stage 2 into the *_o buffers, all four names swap
            T *hat[4];
            if ((rc = ensure_mc_hat<T>(c, nx, ny, nz, hat))) break;
            if ((rc = NS3D_FN(copy_advect)(c, hat[0], Vx, hat[1], Vy, hat[2], Vz, hat[3], C, p->dt, p->dx, p->dy, p->dz, nx, ny, nz, 0))) break;
            if ((rc = NS3D_FN(advect_correct)(c, Vxo, Vx, hat[0], Vyo, Vy, hat[1], Vzo, Vz, hat[2], Co, C, hat[3], p->dt, p->dx, p->dy, p->dz, nx,
                                              ny, nz))) break;
            std::swap(Vx, Vxo); std::swap(Vy, Vyo); std::swap(Vz, Vzo); std::swap(C, Co);
            break;
        }
        // :475-476 / :141-142 in one pass: complete new fields into the *_o buffers, then the roles swap
        if ((rc = NS3D_FN(copy_advect)(c, Vxo, Vx, Vyo, Vy, p->faithful ? Vz : Vzo, Vz, Co, C, p->dt, p->dx, p->dy, p->dz, nx, ny, nz,
                                       p->faithful ? 1 : 0))) break;
        std::swap(Vx, Vxo); std::swap(Vy, Vyo); std::swap(C, Co);
        if (!p->faithful) std::swap(Vz, Vzo);
    } while (0);
    c->flags = was;
    f->Vx = Vx; f->Vy = Vy; f->Vz = Vz; f->Vx_o = Vxo; f->Vy_o = Vyo; f->Vz_o = Vzo; f->C = C; f->C_o = Co;
    if (rc) return rc;
    if (deferred_residual) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double mx;
        std::memcpy(&mx, c->key_host, sizeof mx);
        if (iters_done) *iters_done = 0;
        if (err_hist && max_checks > 0) err_hist[0] = mx * p->err_mul / p->err_div;
        if (n_checks) *n_checks = 1;
        return NS3D_OK;
    }
    return finish(c, hipSuccess, "time_step");
}
