"""Host-side mirror of the reference's kernel layer (scripts/NavierStokes3D_multi_gpu.jl:15-281,
scripts/NavierStokes3D_gpu.jl:175-368): the same kernel names and positional argument lists, each one a
thin call into libns3d.so (hand-written HIP, include/ns3d.h).  `!` is dropped, τ→tau, ∇V→divV.

Arrays are torch CUDA tensors used purely as device-memory handles, shaped like the reference
(nx,ny,nz) and laid out column-major (x fastest) like Julia arrays: create them with `zeros`/`from_numpy`.
The launch grid (nx,ny,nz) is derived from the array shapes like ParallelStencil's `@parallel` does.

PyTorch does no arithmetic here and there is no CPU fallback: without the HIP library / a GPU every call
raises (lib.Ns3dError).
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L

_DT = {torch.float64: "f64", torch.float32: "f32"}
ESIZE = {torch.float64: 8, torch.float32: 4, np.float64: 8, np.float32: 4, "f64": 8, "f32": 4}     # bytes per element


# ---- column-major device arrays -------------------------------------------------------------------------
def zeros(shape, dtype=torch.float64, device="cuda"):
    """@zeros(nx,ny,nz) (multi.jl:343): a (nx,ny,nz) tensor with strides (1,nx,nx*ny)."""
    sx, sy, sz = shape
    return torch.zeros((sz, sy, sx), dtype=dtype, device=device).permute(2, 1, 0)


def from_numpy(a, device="cuda"):
    """Upload a numpy array (any order) as a column-major device array of the same shape."""
    a = np.asfortranarray(a)
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0))).to(device)
    return t.permute(2, 1, 0)


def to_numpy(t):
    """Download to a Fortran-ordered numpy array of the same shape."""
    return np.asfortranarray(t.permute(2, 1, 0).contiguous().cpu().numpy().transpose(2, 1, 0))


def clone(t):
    return t.permute(2, 1, 0).contiguous().clone().permute(2, 1, 0)


def _chk(t, shape=None, name="array"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.Ns3dError("%s must be a CUDA/HIP tensor (navierstokes3d_amd has no CPU path)" % name)
    if t.dtype not in _DT:
        raise L.Ns3dError("%s: unsupported dtype %s" % (name, t.dtype))
    sx, sy, sz = t.shape
    want = (1, sx, sx * sy)
    if any(n > 1 and s != w for n, s, w in zip(t.shape, t.stride(), want)):   # strides of extent-1 dims are free
        raise L.Ns3dError("%s must be column-major (x fastest): use kernels.zeros / from_numpy" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.Ns3dError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return C.c_void_p(t.data_ptr())


def _chk_V(Vx, Vy, Vz, n, tag=""):
    """the three staggered velocity arrays of an n = (nx,ny,nz) cell grid, checked in this order"""
    nx, ny, nz = n
    return _chk(Vx, (nx + 1, ny, nz), "Vx" + tag), _chk(Vy, (nx, ny + 1, nz), "Vy" + tag), _chk(Vz, (nx, ny, nz + 1), "Vz" + tag)


class Context:
    """ns3d_ctx wrapper = what `@init_parallel_stencil(CUDA, Float64, 3)` sets up in the reference
    (gpu.jl:4-8): device + arithmetic mode.  mode: 'strict' (bit-identical to the reference operation
    order) or 'fast' (reciprocals + FMA)."""

    _owns = True

    @classmethod
    def from_handle(cls, handle, device, mode):
        """Wrap an ns3d_ctx owned by someone else (a rank of an ns3d_mgpu): same calls, never destroyed from here."""
        self = cls.__new__(cls)
        self.lib = L.load()
        self.device, self.mode, self.handle, self._owns = int(device), mode, handle, False
        self.use_torch_stream()
        return self

    def __init__(self, device=None, mode="strict", async_=False, ieee_div=False):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.Ns3dError("no GPU visible: libns3d has no CPU path")
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        flags = {"strict": L.NS3D_STRICT, "fast": L.NS3D_FAST}[mode] | (L.NS3D_ASYNC if async_ else 0)
        flags |= L.NS3D_IEEE_DIV if ieee_div else 0
        self.mode = mode
        self.handle = self.lib.ns3d_create(self.device, flags)
        if not self.handle:
            raise L.Ns3dError("ns3d_create failed: " + L.last_error())
        self.use_torch_stream()

    def use_torch_stream(self, stream=None, pin=False):
        """Launch on PyTorch's current stream so that tensor ops (uploads, copies) are ordered with kernels.  pin: stay on
        `stream` whatever PyTorch's current stream becomes (a rank of a MultiGpu created with own_streams)."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._pinned = bool(pin and stream is not None)
        self._stream = s.cuda_stream
        L.check(self.lib.ns3d_set_stream(self.handle, C.c_void_p(s.cuda_stream)))

    def _pin_to_library_stream(self):
        """the stream the library now launches on, as a torch stream; the context stays on it whatever PyTorch's current stream becomes"""
        self._ext = torch.cuda.ExternalStream(int(self.lib.ns3d_get_stream(self.handle)), device=self.device)
        self._pinned, self._stream = True, self._ext.cuda_stream
        return self._ext

    def use_own_stream(self):
        """Back to the stream the context was created with (ns3d_use_own_stream: non-blocking, the context's own) and stay on it
        whatever PyTorch's current stream becomes.  Returns it as a torch stream, like reserve_cus."""
        L.check(self.lib.ns3d_use_own_stream(self.handle))
        return self._pin_to_library_stream()

    def follow_torch_stream(self):
        """Launch where PyTorch launches now (`with torch.cuda.stream(...)` blocks), unless the context is pinned."""
        if not self._pinned and torch.cuda.current_stream(self.device).cuda_stream != self._stream:
            self.use_torch_stream()

    def after_torch_fill(self):
        """Fresh arrays on a pinned context: PyTorch fills a new array (zeros, uploads) on ITS current stream, which nothing orders with
        a pinned context's kernels — so that stream is waited for first.  A context that follows PyTorch's stream needs nothing."""
        if self._pinned:
            torch.cuda.current_stream(self.device).synchronize()

    def sync(self):
        L.check(self.lib.ns3d_sync(self.handle))

    def reserve_cus(self, n):
        """Leave n compute units out of this context's launches (ns3d_reserve_cus: a stream with a CU mask, so that RCCL's kernels
        find room beside a sweep that would hold every CU).  Returns the stream as a torch stream — tensor work that must be
        ordered with the kernels belongs on it (`with torch.cuda.stream(s): …`); n = 0 goes back to PyTorch's current stream."""
        L.check(self.lib.ns3d_reserve_cus(self.handle, int(n)))
        if int(n) <= 0:
            self._ext = None
            self.use_torch_stream()
            return torch.cuda.current_stream(self.device)
        return self._pin_to_library_stream()

    def set_pt_variant(self, v):
        L.check(self.lib.ns3d_set_pt_variant(self.handle, int(v)))

    def set_graph_mode(self, mode):
        """HIP-graph replay of residual-check blocks in pt_solve: -1 auto (launch-bound grids), 0 off, 1 on."""
        L.check(self.lib.ns3d_set_graph_mode(self.handle, int(mode)))

    def set_persist_mode(self, mode):
        """pt_iterate / pt_solve on launch-bound grids: a whole block of iterations in one cooperative launch (k_pt_persist);
        -1 automatic (small grids), 0 never, 1 wherever it applies.  Same results."""
        L.check(self.lib.ns3d_set_persist_mode(self.handle, int(mode)))

    def persist_faults(self):
        """Cooperative launches (k_pt_persist) of this context in which a hand-over timed out; each was redone by launches."""
        return int(self.lib.ns3d_persist_faults(self.handle))

    def set_autotune(self, on):
        """Time the tile shapes of the two-iteration sweep on the first launch per grid (default on; same results)."""
        L.check(self.lib.ns3d_set_autotune(self.handle, int(bool(on))))

    def last_pt2_variant(self):
        """Variant (shape·100 + z-chunk) of the latest two-iteration launch; 0 = built-in choice by grid."""
        return int(self.lib.ns3d_last_pt2_variant(self.handle))

    def last_ptn_variant(self):
        return int(self.lib.ns3d_last_ptn_variant(self.handle))

    def last_pt_depth(self):
        """PT iterations of the latest multi-iteration pass (after plan_pt: the planned depth)."""
        return int(self.lib.ns3d_last_pt_depth(self.handle))

    def arith_build(self, dx, dy, dz):
        """Which compilation of the kernels these grid spacings select: 'strict' | 'strictx' | 'strictp' | 'fast'."""
        return {0: "strict", 1: "strictx", 2: "fast", 3: "strictp"}[int(self.lib.ns3d_arith_build(self.handle, dx, dy, dz))]

    def set_pt2_variant(self, v):
        """Temporal blocking (two PT iterations per pass) in pt_iterate / pt_solve: v < 0 off, 0 default tile."""
        L.check(self.lib.ns3d_set_pt2_variant(self.handle, int(v)))

    def set_ptn_variant(self, v):
        """Tile shape of the N-iteration sweep (pt_sweepn): shape*100 + kz, 0 = built-in."""
        L.check(self.lib.ns3d_set_ptn_variant(self.handle, int(v)))

    def set_pt_pace(self, pace_z):
        """Shape 29 of the N-iteration sweep (variant 29xx): z-steps between the rendezvous of an XCD's tiles; -1 automatic (the
        planner's value, large grids only), 0 off, otherwise a multiple of 4.  Same results."""
        L.check(self.lib.ns3d_set_pt_pace(self.handle, int(pace_z)))

    def last_pt_pace(self):
        """The pace_z the latest N-iteration launch really used; 0: it was not paced."""
        return int(self.lib.ns3d_last_pt_pace(self.handle))

    def set_pt_pace_test(self, extra_arrivals, ticks):
        """Tests: raise the target of every pacing wait by extra_arrivals (it then expires) and bound it by `ticks` shader clocks
        (<= 0: the default bound)."""
        L.check(self.lib.ns3d_set_pt_pace_test(self.handle, int(extra_arrivals), int(ticks)))

    def set_advection(self, scheme):
        """What ns3d_time_step advects with: "reference" (ns3d_copy_advect, the default) or "maccormack" (the limited second-order
        scheme of advect_mc; the step then needs faithful = 0).  The single calls do not read it."""
        codes = {"reference": L.NS3D_ADVECT_REFERENCE, "maccormack": L.NS3D_ADVECT_MACCORMACK}
        if scheme not in codes:
            raise L.Ns3dError("advection = %r (\"reference\" | \"maccormack\")" % (scheme,))
        L.check(self.lib.ns3d_set_advection(self.handle, codes[scheme]))

    def advection(self):
        return {L.NS3D_ADVECT_REFERENCE: "reference", L.NS3D_ADVECT_MACCORMACK: "maccormack"}[int(self.lib.ns3d_advection(self.handle))]

    def set_obstacle(self, mask):
        """What ns3d_time_step masks with: a uint8 mask tensor (voxelize's, of the grid the step runs on; kept alive here until it is
        replaced) in place of both set_cylinder! calls, or None: back to the cylinder.  The single calls do not read it."""
        ptr = None if mask is None else _chk_mask(mask, None, mask)
        L.check(self.lib.ns3d_set_obstacle(self.handle, ptr))
        self._obstacle = mask

    def obstacle(self):
        """the device address ns3d_time_step masks with; None: the cylinder"""
        return self.lib.ns3d_obstacle(self.handle)

    def set_obstacle_motion(self, motion, origin=None):
        """The rigid motion of the obstacle ns3d_time_step masks with: 9 numbers (U, omega, centre; the centre in index space) — the
        step then stores the body's velocity where the mask is set (set_solid_moving at both masking places) — or None: the static
        obstacle.  The context copies the numbers.  Needs set_obstacle; the single calls do not read it."""
        if motion is None:
            L.check(self.lib.ns3d_set_obstacle_motion(self.handle, None, None))
        else:
            L.check(self.lib.ns3d_set_obstacle_motion(self.handle, _motion9(motion), _int3(origin)))

    def obstacle_motion(self):
        """the nine numbers of set_obstacle_motion as a tuple; None: no motion set"""
        out = (C.c_double * 9)()
        return tuple(out) if int(self.lib.ns3d_obstacle_motion(self.handle, out)) == 1 else None

    def set_turbulence(self, model, length=0.0, mu_e=None):
        """The subgrid model of ns3d_time_step's predictor: None / "none" (the default: the scalar μ, not one extra call) or
        "smagorinsky" | "wale" | "vreman" with length = C·Δ (C_s, C_w, √c_v) and mu_e, a column-major (nx,ny,nz) tensor of the step's
        dtype that the step writes the effective viscosity to (kept alive here until the setting is replaced).  The name sets the
        differential operator (ns3d_set_sgs_operator), then the model; None also returns the operator to Smagorinsky's.  The single
        calls do not read it."""
        codes = {None: L.NS3D_TURB_NONE, "none": L.NS3D_TURB_NONE}
        codes.update((name, L.NS3D_TURB_SMAGORINSKY) for name in L.SGS_OPERATORS)
        if model not in codes:
            raise L.Ns3dError("turbulence model = %r (None | \"smagorinsky\" | \"wale\" | \"vreman\")" % (model,))
        off = codes[model] == L.NS3D_TURB_NONE
        ptr = None if off or mu_e is None else _chk(mu_e, None, "mu_e")
        before = int(self.lib.ns3d_sgs_operator(self.handle))
        L.check(self.lib.ns3d_set_sgs_operator(self.handle, L.SGS_OPERATORS.get(model, L.NS3D_SGS_SMAGORINSKY)))
        rc = self.lib.ns3d_set_turbulence(self.handle, codes[model], C.c_double(float(length)), ptr)
        if rc != L.NS3D_OK:         # a refused model leaves both settings
            msg = L.last_error()
            self.lib.ns3d_set_sgs_operator(self.handle, before)
            raise L.Ns3dError("libns3d status %d: %s" % (rc, msg))
        self._mu_e = None if off else mu_e

    def turbulence(self):
        """None, or the name of the operator the step forms mu_e with"""
        if int(self.lib.ns3d_turbulence(self.handle)) == L.NS3D_TURB_NONE:
            return None
        return {code: name for name, code in L.SGS_OPERATORS.items()}[int(self.lib.ns3d_sgs_operator(self.handle))]

    def set_scalar(self, kappa=None, sct=0.0, bg=0.0, c_ref=0.0):
        """The active scalar of ns3d_time_step: kappa=None (the default: C is the reference's passive dye, not one extra call) clears
        the setting; a number makes every step diffuse C with diffusivity kappa (plus the subgrid model's eddy diffusivity
        (mu_e − μ)/(ρ·sct) while set_turbulence has a model and sct > 0) and lift the predicted Vz by dt·bg·(C − c_ref), bg = g·β, in
        one ns3d_scalar_step call behind the predictor.  The single calls do not read it."""
        if kappa is None:
            L.check(self.lib.ns3d_set_scalar(self.handle, 0, 0.0, 0.0, 0.0, 0.0))
        else:
            L.check(self.lib.ns3d_set_scalar(self.handle, 1, float(kappa), float(sct), float(bg), float(c_ref)))

    def scalar(self):
        """whether ns3d_time_step runs the active scalar"""
        return bool(self.lib.ns3d_scalar(self.handle))

    def set_pt_depth(self, depth):
        """PT iterations per pass over memory in pt_iterate / pt_solve: 0 automatic, 1…4 forced (5: float32 fields only)."""
        L.check(self.lib.ns3d_set_pt_depth(self.handle, int(depth)))

    def selftest_exact_div(self, d, n=1 << 24, seed=1, dtype=torch.float64):
        """Mismatches between the divisor-known-in-advance division and the plain IEEE division over n dividends."""
        out = C.c_long(-1)
        fn = getattr(self.lib, "ns3d_selftest_exact_div_" + _DT[dtype])
        L.check(fn(self.handle, C.c_double(d), C.c_long(n), C.c_ulonglong(seed), C.byref(out)))
        return out.value

    def close(self):
        if getattr(self, "handle", None):
            if self._owns:
                self.lib.ns3d_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, ref, *args):
        self.follow_torch_stream()
        fn = getattr(self.lib, "ns3d_%s_%s" % (name, _DT[ref.dtype]))
        L.check(fn(self.handle, *args))


_DEFAULT = {}


def init_parallel_stencil(device=None, mode="strict", async_=False):
    """Create (or replace) the default context for `device`; mirrors @init_parallel_stencil (gpu.jl:4-8)."""
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    old = _DEFAULT.pop(int(device), None)
    if old is not None:
        old.close()
    ctx = Context(device, mode, async_)
    _DEFAULT[int(device)] = ctx
    return ctx


def default_context(t=None):
    dev = t.device.index if t is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    ctx = _DEFAULT.get(dev)
    if ctx is None:
        ctx = init_parallel_stencil(dev)
    return ctx


def _ctx(ctx, t):
    return ctx if ctx is not None else default_context(t)


def _d(*xs):
    return [C.c_double(float(x)) for x in xs]


# ---- the reference's kernels ----------------------------------------------------------------------------
def update_tau(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, mu, dx, dy, dz, ctx=None):
    """update_τ!  multi.jl:36-44 / gpu.jl:177-185"""
    nx, ny, nz = txx.shape
    c = (nx, ny, nz); s = (nx - 1, ny - 1, nz - 1)
    _ctx(ctx, txx).call("update_tau", txx, _chk(txx, c, "txx"), _chk(tyy, c, "tyy"), _chk(tzz, c, "tzz"),
                        _chk(txy, s, "txy"), _chk(txz, s, "txz"), _chk(tyz, s, "tyz"), *_chk_V(Vx, Vy, Vz, c), *_d(mu, dx, dy, dz), nx, ny, nz)


def predict_V(Vx, Vy, Vz, txx, tyy, tzz, txy, txz, tyz, rho, g, dt, dx, dy, dz, ctx=None):
    """predict_V!  multi.jl:50-55 / gpu.jl:187-192"""
    nx, ny, nz = txx.shape
    c = (nx, ny, nz); s = (nx - 1, ny - 1, nz - 1)
    _ctx(ctx, txx).call("predict_V", txx, *_chk_V(Vx, Vy, Vz, c), _chk(txx, c, "txx"), _chk(tyy, c, "tyy"),
                        _chk(tzz, c, "tzz"), _chk(txy, s, "txy"), _chk(txz, s, "txz"), _chk(tyz, s, "tyz"), *_d(rho, g, dt, dx, dy, dz), nx, ny, nz)


def predict_fused(Vx_new, Vy_new, Vz_new, Vx, Vy, Vz, mu, rho, g, dt, dx, dy, dz, ctx=None):
    """{update_τ!; predict_V!} (multi.jl:449,451) in one pass: complete predicted fields into buffers of their own, the stress
    arrays neither read nor written; the caller swaps the names."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("predict_fused", Vx, *_chk_V(Vx_new, Vy_new, Vz_new, (nx, ny, nz), "_new"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)),
                       *_d(mu, rho, g, dt, dx, dy, dz), nx, ny, nz)


def _chk_like(t, shape, name, ref):
    """_chk, and the dtype and device of the velocities"""
    p = _chk(t, shape, name)
    if t.dtype != ref.dtype or t.device != ref.device:
        raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, ref.dtype, ref.device))
    return p


def eddy_viscosity(mu_e, Vx, Vy, Vz, mu, rho, length, dx, dy, dz, ctx=None):
    """ns3d_eddy_viscosity: Smagorinsky's effective viscosity mu_e = μ + ρ·length²·|S| of the staggered velocity field, a cell-centred
    (nx,ny,nz) array of the fields' dtype, in one fused pass on the device (include/ns3d.h has the expression; the gradient is
    vortex's).  length = C_s·Δ.  Interior cells receive the value, every other cell μ.  Enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    out = _chk_like(mu_e, (nx, ny, nz), "mu_e", Vx)
    V = _chk_V(Vx, Vy, Vz, (nx, ny, nz))
    for name, t in (("Vy", Vy), ("Vz", Vz)):
        if t.dtype != Vx.dtype or t.device != Vx.device:
            raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    _ctx(ctx, Vx).call("eddy_viscosity", Vx, out, *V, *_d(mu, rho, length, dx, dy, dz), nx, ny, nz)


def sgs_viscosity(mu_e, Vx, Vy, Vz, op, mu, rho, length, dx, dy, dz, ctx=None):
    """ns3d_sgs_viscosity: mu_e = μ + ρ·length²·op(∇V) with the differential operator `op` — "smagorinsky" (eddy_viscosity's bits),
    "wale" or "vreman", or its NS3D_SGS_* code — from eddy_viscosity's velocity gradient, in one fused pass (include/ns3d.h has the
    expressions).  WALE and Vreman vanish exactly in pure shear.  length = C_w·Δ / √c_v·Δ.  Enqueues; no read-back."""
    code = L.SGS_OPERATORS.get(op, op) if isinstance(op, str) else op
    if isinstance(code, bool) or not isinstance(code, int):
        raise L.Ns3dError("sgs operator = %r (\"smagorinsky\" | \"wale\" | \"vreman\", or an NS3D_SGS_* code)" % (op,))
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    out = _chk_like(mu_e, (nx, ny, nz), "mu_e", Vx)
    V = _chk_V(Vx, Vy, Vz, (nx, ny, nz))
    for name, t in (("Vy", Vy), ("Vz", Vz)):
        if t.dtype != Vx.dtype or t.device != Vx.device:
            raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    _ctx(ctx, Vx).call("sgs_viscosity", Vx, code, out, *V, *_d(mu, rho, length, dx, dy, dz), nx, ny, nz)


def scalar_diffuse(C_out, Cf, mu_e, kappa, sgs, mu, dt, dx, dy, dz, ctx=None):
    """ns3d_scalar_diffuse: one explicit step of ∂C/∂t = ∇·(K ∇C) in flux form, out of place into C_out, zero flux through the domain
    faces; K = kappa, or kappa + sgs·(mu_e − mu) per cell with the (nx,ny,nz) field mu_e (None: none).  include/ns3d.h has the
    statement.  Enqueues; no read-back."""
    nx, ny, nz = Cf.shape
    _ctx(ctx, Cf).call("scalar_diffuse", Cf, _chk_like(C_out, (nx, ny, nz), "C_out", Cf), _chk(Cf, None, "C"),
                       None if mu_e is None else _chk_like(mu_e, (nx, ny, nz), "mu_e", Cf), *_d(kappa, sgs, mu, dt, dx, dy, dz), nx, ny, nz)


def buoyancy(Vz, Cf, bg, c_ref, dt, ctx=None):
    """ns3d_buoyancy: Vz += dt·bg·(½(C[k−1] + C[k]) − c_ref) in place on predict_V!'s range of the (nx,ny,nz+1) array; bg = g·β."""
    nx, ny, nz = Cf.shape
    _ctx(ctx, Cf).call("buoyancy", Cf, _chk_like(Vz, (nx, ny, nz + 1), "Vz", Cf), _chk(Cf, None, "C"), *_d(bg, c_ref, dt), nx, ny, nz)


def scalar_step(C_out, Vz, Cf, mu_e, kappa, sgs, mu, bg, c_ref, dt, dx, dy, dz, ctx=None):
    """ns3d_scalar_step: scalar_diffuse and buoyancy in one pass, both reading Cf — the bits of the two calls.  Vz may be None when
    bg == 0."""
    nx, ny, nz = Cf.shape
    _ctx(ctx, Cf).call("scalar_step", Cf, _chk_like(C_out, (nx, ny, nz), "C_out", Cf),
                       None if Vz is None else _chk_like(Vz, (nx, ny, nz + 1), "Vz", Cf), _chk(Cf, None, "C"),
                       None if mu_e is None else _chk_like(mu_e, (nx, ny, nz), "mu_e", Cf),
                       *_d(kappa, sgs, mu, bg, c_ref, dt, dx, dy, dz), nx, ny, nz)


def update_tau_var(txx, tyy, tzz, txy, txz, tyz, Vx, Vy, Vz, mu_e, dx, dy, dz, ctx=None):
    """ns3d_update_tau_var: update_τ! with the scalar μ replaced by the (nx,ny,nz) field mu_e — the cell's own value in the normal
    stresses, the mean of the four cells around the edge in the shear stresses."""
    nx, ny, nz = txx.shape
    c = (nx, ny, nz); s = (nx - 1, ny - 1, nz - 1)
    _ctx(ctx, txx).call("update_tau_var", txx, _chk(txx, c, "txx"), _chk(tyy, c, "tyy"), _chk(tzz, c, "tzz"),
                        _chk(txy, s, "txy"), _chk(txz, s, "txz"), _chk(tyz, s, "tyz"), *_chk_V(Vx, Vy, Vz, c), _chk_like(mu_e, c, "mu_e", txx),
                        *_d(dx, dy, dz), nx, ny, nz)


def predict_var(Vx_new, Vy_new, Vz_new, Vx, Vy, Vz, mu_e, rho, g, dt, dx, dy, dz, ctx=None):
    """{update_tau_var; predict_V!} in one pass, predict_fused's contract: complete predicted fields into buffers of their own, the
    stress arrays neither read nor written; the caller swaps the names."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("predict_var", Vx, *_chk_V(Vx_new, Vy_new, Vz_new, (nx, ny, nz), "_new"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)),
                       _chk_like(mu_e, (nx, ny, nz), "mu_e", Vx), *_d(rho, g, dt, dx, dy, dz), nx, ny, nz)


def set_cylinder(Cf, Vx, Vy, Vz, a2, b2, ox, oy, sinb, cosb, *rest, ctx=None):
    """set_cylinder!  multi.jl:249-281 (19 arguments: …,xco_g,yco_g,zco_g,lx,ly,lz,dx,dy,dz) or
    gpu.jl:336-368 (16 arguments: …,lx,ly,lz,dx,dy,dz) — dispatched on the argument count like the two
    scripts' definitions."""
    nx, ny, nz = Cf.shape
    ptrs = (_chk(Cf, (nx, ny, nz), "C"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)))
    if len(rest) == 9:
        _ctx(ctx, Cf).call("set_cylinder", Cf, *ptrs, *_d(a2, b2, ox, oy, sinb, cosb, *rest), nx, ny, nz)
    elif len(rest) == 6:
        _ctx(ctx, Cf).call("set_cylinder_local", Cf, *ptrs, *_d(a2, b2, ox, oy, sinb, cosb, *rest), nx, ny, nz)
    else:
        raise TypeError("set_cylinder: expected 19 (multi.jl) or 16 (gpu.jl) positional arguments")


def _chk_mask(mask, n, ref):
    """a contiguous uint8 device array of (nx+1)(ny+1)(nz+1) bytes on ref's device (any shape; column-major, x fastest, in memory)"""
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.uint8:
        raise L.Ns3dError("mask must be a uint8 CUDA/HIP tensor")
    if mask.device != ref.device:
        raise L.Ns3dError("mask is on %s, the fields on %s" % (mask.device, ref.device))
    if n is not None and mask.numel() != (n[0] + 1) * (n[1] + 1) * (n[2] + 1):
        raise L.Ns3dError("mask has %d bytes, a %dx%dx%d grid needs %d" % ((mask.numel(),) + tuple(n) + ((n[0] + 1) * (n[1] + 1) * (n[2] + 1),)))
    if not (mask.is_contiguous() or (mask.dim() == 3 and mask.permute(2, 1, 0).is_contiguous())):
        raise L.Ns3dError("mask must be contiguous, or column-major like the fields")
    return C.c_void_p(mask.data_ptr())


def voxelize(mask, tri, n, origin=None, ctx=None):
    """ns3d_voxelize: the four staggered masks of the closed triangle surface `tri` (a contiguous float64 device array of 9 doubles per
    triangle, index space) on the cell grid n = (nx, ny, nz), into `mask` ((nx+1)(ny+1)(nz+1) uint8: bit 0 C, 1 Vx, 2 Vy, 3 Vz at their
    stagger locations; include/ns3d.h has the rule, the same bytes in every arithmetic mode).  origin: the rank's first cell in the
    global index space.  Enqueues; no read-back."""
    nx, ny, nz = (int(q) for q in n)
    n_tri = 0
    ptr = None
    if tri is not None:
        if not isinstance(tri, torch.Tensor) or not tri.is_cuda or tri.dtype != torch.float64 or not tri.is_contiguous() or tri.numel() % 9:
            raise L.Ns3dError("tri must be a contiguous float64 CUDA/HIP tensor of 9 values per triangle")
        if tri.device != mask.device:
            raise L.Ns3dError("tri is on %s, the mask on %s" % (tri.device, mask.device))
        n_tri = tri.numel() // 9
        ptr = C.c_void_p(tri.data_ptr()) if n_tri else None
    _untyped(ctx, mask, "ns3d_voxelize", _chk_mask(mask, (nx, ny, nz), mask), ptr, C.c_longlong(n_tri), nx, ny, nz, _int3(origin))


def set_solid(Cf, Vx, Vy, Vz, mask, ctx=None):
    """ns3d_set_solid: what set_cylinder! stores, with the flags read from `mask` (voxelize's bytes): C = 1, Vx = Vy = Vz = 0 where their
    bits are set.  Cf may be None.  Enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("set_solid", Vx, None if Cf is None else _chk(Cf, (nx, ny, nz), "C"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)),
                       _chk_mask(mask, (nx, ny, nz), Vx), nx, ny, nz)


def solid_momentum(Vx, Vy, Vz, mask, seam_lo=None, seam_hi=None, ctx=None):
    """ns3d_solid_momentum: (mom, n) — per direction the fp64 sum and the number of the owned nodes of Vx, Vy, Vz whose mask bit is set:
    what the next set_solid removes (the monitor's mom / n_masked for a mask).  Blocks for the read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    mom, cnt = (C.c_double * 3)(), (C.c_longlong * 3)()
    _ctx(ctx, Vx).call("solid_momentum", Vx, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), _chk_mask(mask, (nx, ny, nz), Vx), nx, ny, nz,
                       _int3(seam_lo), _int3(seam_hi), mom, cnt)
    return tuple(mom), tuple(int(q) for q in cnt)


def _motion9(motion):
    """U, omega, centre (9 numbers, any nesting) as the C array the moving calls take"""
    m = np.asarray(motion, dtype=np.float64).reshape(-1)
    if m.size != 9:
        raise L.Ns3dError("motion holds 9 numbers (U, omega, centre), got %d" % m.size)
    return (C.c_double * 9)(*m)


def set_solid_moving(Cf, Vx, Vy, Vz, mask, motion, dx, dy, dz, origin=None, ctx=None):
    """ns3d_set_solid_moving: set_solid for a body in rigid motion — where a velocity bit is set the store is the body's velocity at
    that node, U + omega × r with r = (node − centre)·spacing (include/ns3d.h has the statement; motion = U, omega, centre, the centre
    in index space).  Zero motion gives set_solid's bits.  Cf may be None.  Enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("set_solid_moving", Vx, None if Cf is None else _chk(Cf, (nx, ny, nz), "C"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)),
                       _chk_mask(mask, (nx, ny, nz), Vx), _motion9(motion), *_d(dx, dy, dz), _int3(origin), nx, ny, nz)


def solid_momentum_moving(Vx, Vy, Vz, mask, motion, dx, dy, dz, origin=None, seam_lo=None, seam_hi=None, ctx=None):
    """ns3d_solid_momentum_moving: (mom, n) as solid_momentum, each term less the body's own velocity at the node: what the next
    set_solid_moving with this motion removes.  Blocks for the read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    mom, cnt = (C.c_double * 3)(), (C.c_longlong * 3)()
    _ctx(ctx, Vx).call("solid_momentum_moving", Vx, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), _chk_mask(mask, (nx, ny, nz), Vx), nx, ny, nz,
                       _int3(seam_lo), _int3(seam_hi), mom, cnt, _motion9(motion), *_d(dx, dy, dz), _int3(origin))
    return tuple(mom), tuple(int(q) for q in cnt)


def mesh_transform(out, tri, R, pivot, shift, spacing, ctx=None):
    """ns3d_mesh_transform: the rigid motion x → pivot + shift + R·(x − pivot), taken in PHYSICAL space, of a mesh stored in index
    space (`tri`: a contiguous float64 device array of 9 doubles per triangle) into `out` (the same size; `out is tri` works in place).
    R: 3×3, pivot and shift in index units, spacing = (dx, dy, dz).  Enqueues; no read-back."""
    for name, t in (("out", out), ("tri", tri)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() % 9:
            raise L.Ns3dError("%s must be a contiguous float64 CUDA/HIP tensor of 9 values per triangle" % name)
    if out.device != tri.device or out.numel() != tri.numel():
        raise L.Ns3dError("out holds %d values on %s, tri %d on %s" % (out.numel(), out.device, tri.numel(), tri.device))
    r = np.asarray(R, dtype=np.float64)
    vec = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (pivot, shift, spacing)]
    if r.shape != (3, 3) or any(v.size != 3 for v in vec):
        raise L.Ns3dError("mesh_transform: R is 3x3, pivot, shift and spacing hold 3 numbers each")
    n_tri = tri.numel() // 9
    _untyped(ctx, tri, "ns3d_mesh_transform", C.c_void_p(out.data_ptr()) if n_tri else None, C.c_void_p(tri.data_ptr()) if n_tri else None,
             C.c_longlong(n_tri), (C.c_double * 9)(*r.reshape(-1)), *((C.c_double * 3)(*v) for v in vec))


def update_divV(divV, Vx, Vy, Vz, dx, dy, dz, ctx=None):
    """update_∇V!  multi.jl:61-64 / gpu.jl:194-197"""
    nx, ny, nz = divV.shape
    _ctx(ctx, divV).call("update_divV", divV, _chk(divV, None, "divV"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), *_d(dx, dy, dz), nx, ny, nz)


def update_dPrdtau(Pr, dPrdtau, divV, rho, dt, dtau, damp, dx, dy, dz, ctx=None):
    """update_dPrdτ!  multi.jl:70-73 / gpu.jl:199-202"""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("update_dPrdtau", Pr, _chk(Pr, None, "Pr"), _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"),
                       _chk(divV, (nx, ny, nz), "divV"), *_d(rho, dt, dtau, damp, dx, dy, dz), nx, ny, nz)


def update_Pr(Pr, dPrdtau, dtau, ctx=None):
    """update_Pr!  multi.jl:79-82 / gpu.jl:204-207"""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("update_Pr", Pr, _chk(Pr, None, "Pr"), _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"),
                       *_d(dtau), nx, ny, nz)


def compute_res(Rp, Pr, divV, rho, dt, dx, dy, dz, ctx=None):
    """compute_res!  multi.jl:88-91 / gpu.jl:209-212"""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("compute_res", Pr, _chk(Rp, (nx - 2, ny - 2, nz - 2), "Rp"), _chk(Pr, None, "Pr"),
                       _chk(divV, (nx, ny, nz), "divV"), *_d(rho, dt, dx, dy, dz), nx, ny, nz)


def max_abs(A, ctx=None):
    """maximum(abs.(A)) — NaN-propagating  (multi.jl:466 / gpu.jl:132)"""
    out = C.c_double(0.0)
    _ctx(ctx, A).call("max_abs", A, _chk(A, None, "A"), C.c_long(A.numel()), C.byref(out))
    return out.value


def correct_V(Vx, Vy, Vz, Pr, dt, rho, dx, dy, dz, ctx=None):
    """correct_V!  multi.jl:97-102 / gpu.jl:214-219"""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("correct_V", Pr, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), _chk(Pr, None, "Pr"), *_d(dt, rho, dx, dy, dz), nx, ny, nz)


def _bc(name, A, *extra, ctx=None):
    _ctx(ctx, A).call(name, A, _chk(A, None, "A"), *extra, *A.shape)


def bc_x(A, ctx=None):
    """bc_x!  multi.jl:108-112"""
    _bc("bc_x", A, ctx=ctx)


def bc_y(A, ctx=None):
    """bc_y!  multi.jl:118-122"""
    _bc("bc_y", A, ctx=ctx)


def bc_z(A, ctx=None):
    """bc_z!  multi.jl:128-132"""
    _bc("bc_z", A, ctx=ctx)


def bc_zV(A, ctx=None):
    """bc_zV!  gpu.jl:239-243"""
    _bc("bc_zV", A, ctx=ctx)


def bc_xhydstatic(A, dz, nz, g, rho, ctx=None):
    """bc_xhydstatic!  gpu.jl:257-261"""
    _bc("bc_xhydstatic", A, C.c_double(dz), C.c_int(nz), C.c_double(g), C.c_double(rho), ctx=ctx)


def bc_x_Vx(A, V, ctx=None):
    """bc_x_Vx!  multi.jl:138-141"""
    _bc("bc_x_Vx", A, C.c_double(V), ctx=ctx)


def bc_x_Pr(A, val, ctx=None):
    """bc_x_Pr!  multi.jl:147-150"""
    _bc("bc_x_Pr", A, C.c_double(val), ctx=ctx)


def copy(dst, src, ctx=None):
    """X_o .= X  (multi.jl:475 / gpu.jl:141)"""
    _ctx(ctx, dst).call("copy", dst, _chk(dst, src.shape, "dst"), _chk(src, None, "src"), C.c_long(src.numel()))


def advect(Vx, Vx_o, Vy, Vy_o, Vz, Vz_o, Cf, C_o, dt, dx, dy, dz, faithful=True, ctx=None):
    """advect!  multi.jl:217-243 / gpu.jl:308-334.  faithful=True reproduces the reference's third branch
    (back-tracks Vy, never Vz — SURVEY.md App. B1)."""
    nx, ny, nz = Cf.shape
    _ctx(ctx, Cf).call("advect", Cf, _chk(Vx, (nx + 1, ny, nz), "Vx"), _chk(Vx_o, (nx + 1, ny, nz), "Vx_o"),
                       _chk(Vy, (nx, ny + 1, nz), "Vy"), _chk(Vy_o, (nx, ny + 1, nz), "Vy_o"),
                       _chk(Vz, (nx, ny, nz + 1), "Vz"), _chk(Vz_o, (nx, ny, nz + 1), "Vz_o"),
                       _chk(Cf, None, "C"), _chk(C_o, (nx, ny, nz), "C_o"), *_d(dt, dx, dy, dz), nx, ny, nz,
                       1 if faithful else 0)


def copy_advect(Vx_new, Vx, Vy_new, Vy, Vz_new, Vz, C_new, Cf, dt, dx, dy, dz, faithful=True, ctx=None):
    """{X_o .= X; advect!} (multi.jl:475-476 / gpu.jl:141-142) in one pass: reads the current fields, writes COMPLETE new
    fields into buffers of their own; the caller swaps the roles afterwards.  Vz_new may be Vz in faithful mode."""
    nx, ny, nz = Cf.shape
    _ctx(ctx, Cf).call("copy_advect", Cf, _chk(Vx_new, (nx + 1, ny, nz), "Vx_new"), _chk(Vx, (nx + 1, ny, nz), "Vx"),
                       _chk(Vy_new, (nx, ny + 1, nz), "Vy_new"), _chk(Vy, (nx, ny + 1, nz), "Vy"),
                       _chk(Vz_new, (nx, ny, nz + 1), "Vz_new"), _chk(Vz, (nx, ny, nz + 1), "Vz"),
                       _chk(C_new, (nx, ny, nz), "C_new"), _chk(Cf, None, "C"), *_d(dt, dx, dy, dz), nx, ny, nz,
                       1 if faithful else 0)


def _mc_args(Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, Cf, C_hat):
    nx, ny, nz = Cf.shape
    out = []
    for shape, name, trio in (((nx + 1, ny, nz), "Vx", (Vx_new, Vx, Vx_hat)), ((nx, ny + 1, nz), "Vy", (Vy_new, Vy, Vy_hat)),
                              ((nx, ny, nz + 1), "Vz", (Vz_new, Vz, Vz_hat)), ((nx, ny, nz), "C", (C_new, Cf, C_hat))):
        out += [_chk(t, shape, name + tag) for t, tag in zip(trio, ("_new", "", "_hat"))]
    return out, (nx, ny, nz)


def advect_correct(Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, Cf, C_hat, dt, dx, dy, dz, ctx=None):
    """Stage 2 of the limited MacCormack advection (ns3d_advect_correct; include/ns3d.h has the definition): the *_hat arrays hold
    copy_advect(…, faithful=False) of the current fields, the *_new arrays receive the complete new fields.  Twelve distinct arrays."""
    args, n = _mc_args(Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, Cf, C_hat)
    _ctx(ctx, Cf).call("advect_correct", Cf, *args, *_d(dt, dx, dy, dz), *n)


def advect_mc(Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, Cf, C_hat, dt, dx, dy, dz, ctx=None):
    """Limited MacCormack advection, second order (ns3d_advect_mc): stage 1 — copy_advect(…, faithful=False) — into the *_hat
    arrays, then stage 2 into the *_new arrays; the caller swaps the roles of X_new and X afterwards, like after copy_advect."""
    args, n = _mc_args(Vx_new, Vx, Vx_hat, Vy_new, Vy, Vy_hat, Vz_new, Vz, Vz_hat, C_new, Cf, C_hat)
    _ctx(ctx, Cf).call("advect_mc", Cf, *args, *_d(dt, dx, dy, dz), *n)


# ---- the reference's host sequences, one library call each ----------------------------------------------
def set_bc_Pr_multi(Pr, owns_outlet, val=0.0, ctx=None):
    """set_bc_Pr!(Pr, xve_g, lx, val) of multi.jl:175-181 with `xve_g == lx/2` passed as a flag; the trailing
    update_halo!(Pr) (multi.jl:182) is the caller's."""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("set_bc_Pr", Pr, _chk(Pr, None, "Pr"), L.NS3D_BC_MULTI, int(bool(owns_outlet)),
                       *_d(val, 0.0), 0, *_d(0.0, 0.0), nx, ny, nz)


def set_bc_Pr_gpu(Pr, dz, nz_arg, g, rho, ctx=None):
    """set_bc_Pr!(Pr, dz, nz, g, ρ) of gpu.jl:281-286"""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("set_bc_Pr", Pr, _chk(Pr, None, "Pr"), L.NS3D_BC_GPU, 0, *_d(0.0, dz), int(nz_arg),
                       *_d(g, rho), nx, ny, nz)


def set_bc_Vel_multi(Vx, Vy, Vz, owns_inlet, vin, ctx=None):
    """set_bc_Vel!(Vx,Vy,Vz,xvo_g,lx,vin) of multi.jl:156-166 (flag instead of `xvo_g == -lx/2`; halo update
    multi.jl:167 is the caller's)."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("set_bc_Vel", Vx, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), L.NS3D_BC_MULTI, int(bool(owns_inlet)), *_d(vin), nx, ny, nz)


def set_bc_Vel_gpu(Vx, Vy, Vz, ctx=None):
    """set_bc_Vel!(Vx,Vy,Vz,Vprof) of gpu.jl:264-279 (Vprof is unused there)."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    _ctx(ctx, Vx).call("set_bc_Vel", Vx, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), L.NS3D_BC_GPU, 0, *_d(0.0), nx, ny, nz)


# ---- fused pseudo-transient path ------------------------------------------------------------------------
def pt_params(Pr, rho, dt, dtau, damp, dx, dy, dz, bc_kind=L.NS3D_BC_MULTI, owns_outlet=True, outlet_val=0.0,
              g=0.0, z_lo_is_halo=False, z_hi_is_halo=False):
    nx, ny, nz = Pr.shape
    return L.PtParams(rho, dt, dtau, damp, dx, dy, dz, nx, ny, nz, int(bc_kind), int(bool(owns_outlet)),
                      outlet_val, g, int(bool(z_lo_is_halo)), int(bool(z_hi_is_halo)))


def pt_iterate(Pr, dPrdtau, divV, p, n_iters, ctx=None):
    """n_iters × {update_dPrdτ!; update_Pr!; set_bc_Pr!} (multi.jl:459-463 / gpu.jl:127-129) as fused sweeps."""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("pt_iterate", Pr, _chk(Pr, None, "Pr"), _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"),
                       _chk(divV, (nx, ny, nz), "divV"), C.byref(p), int(n_iters))


def poisson_direct(Pr, dPrdtau, divV, p, ctx=None):
    """OUTSIDE PARITY: the discrete pressure-Poisson problem the PT loop multi.jl:458-471 / gpu.jl:126-137 iterates
    towards, solved directly (exact diagonalisation, six fp64 MFMA matrix products): Pr ← solution with set_bc_Pr!'s boundary
    cells, dPrdτ ← 0."""
    nx, ny, nz = Pr.shape
    _ctx(ctx, Pr).call("poisson_direct", Pr, _chk(Pr, None, "Pr"), _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"),
                       _chk(divV, (nx, ny, nz), "divV"), C.byref(p))


def pt_sweep(Pr_in, Pr_out, dPrdtau, divV, p, k0, k1, ctx=None):
    """One fused sweep Pr_in → Pr_out over interior planes k0 ≤ k < k1 (0-based)."""
    nx, ny, nz = Pr_in.shape
    _ctx(ctx, Pr_in).call("pt_sweep", Pr_in, _chk(Pr_in, None, "Pr_in"), _chk(Pr_out, (nx, ny, nz), "Pr_out"),
                          _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"), _chk(divV, (nx, ny, nz), "divV"),
                          C.byref(p), int(k0), int(k1))


def pt_sweep2(Pr_in, Pr_out, dPrdtau_in, dPrdtau_out, divV, p, k0=None, k1=None, ctx=None):
    """TWO fused PT iterations (Pr_in, dPrdtau_in) → (Pr_out, dPrdtau_out) in one pass over memory (same result
    as two pt_sweep calls); all four buffers distinct."""
    nx, ny, nz = Pr_in.shape
    _ctx(ctx, Pr_in).call("pt_sweep2", Pr_in, _chk(Pr_in, None, "Pr_in"), _chk(Pr_out, (nx, ny, nz), "Pr_out"),
                          _chk(dPrdtau_in, (nx - 2, ny - 2, nz - 2), "dPrdtau_in"),
                          _chk(dPrdtau_out, (nx - 2, ny - 2, nz - 2), "dPrdtau_out"), _chk(divV, (nx, ny, nz), "divV"),
                          C.byref(p), 1 if k0 is None else int(k0), nz - 1 if k1 is None else int(k1))


def pt_sweepn(nlev, Pr_in, Pr_out, dPrdtau_in, dPrdtau_out, divV, p, k0=None, k1=None, ctx=None):
    """nlev (2…4; float32 also 5) fused PT iterations (Pr_in, dPrdtau_in) → (Pr_out, dPrdtau_out) in one pass over memory (same result as
    nlev pt_sweep calls); all four buffers distinct."""
    nx, ny, nz = Pr_in.shape
    _ctx(ctx, Pr_in).call("pt_sweepn", Pr_in, int(nlev), _chk(Pr_in, None, "Pr_in"), _chk(Pr_out, (nx, ny, nz), "Pr_out"),
                          _chk(dPrdtau_in, (nx - 2, ny - 2, nz - 2), "dPrdtau_in"),
                          _chk(dPrdtau_out, (nx - 2, ny - 2, nz - 2), "dPrdtau_out"), _chk(divV, (nx, ny, nz), "divV"),
                          C.byref(p), 1 if k0 is None else int(k0), nz - 1 if k1 is None else int(k1))


def plan_pt(Pr_in, Pr_out, dPrdtau_in, dPrdtau_out, divV, p, k0=None, k1=None, ctx=None):
    """Plan phase of the two-iteration sweep: time the tile shapes now, on these arguments, and remember the winner
    (ns3d_plan_pt).  pt_iterate / pt_solve plan by themselves on first use; pt_sweep2 only looks the choice up."""
    nx, ny, nz = Pr_in.shape
    _ctx(ctx, Pr_in).call("plan_pt", Pr_in, _chk(Pr_in, None, "Pr_in"), _chk(Pr_out, (nx, ny, nz), "Pr_out"),
                          _chk(dPrdtau_in, (nx - 2, ny - 2, nz - 2), "dPrdtau_in"),
                          _chk(dPrdtau_out, (nx - 2, ny - 2, nz - 2), "dPrdtau_out"), _chk(divV, (nx, ny, nz), "divV"),
                          C.byref(p), 1 if k0 is None else int(k0), nz - 1 if k1 is None else int(k1))


def residual_max(Pr, divV, p, ctx=None):
    """maximum(abs.(Rp)) after compute_res! (multi.jl:465-466) without materialising Rp."""
    out = C.c_double(0.0)
    _ctx(ctx, Pr).call("residual_max", Pr, _chk(Pr, None, "Pr"), _chk(divV, tuple(Pr.shape), "divV"), C.byref(p),
                       C.byref(out))
    return out.value


_STEP_SWAP = ("Vx", "Vy", "Vz", "Vx_o", "Vy_o", "Vz_o", "C", "C_o")


def time_step(f, sp, ctx=None):
    """One whole time step in one library call (ns3d_time_step: multi.jl:449-477 on one rank / gpu.jl:121-142 in its fused form).
    f: a namespace of the reference's arrays as tensors (Pr, dPrdtau, divV, Vx, …, C_o, txx … tyz); sp: lib.StepParams.  The step
    swaps the roles of X and X_o instead of copying: on return f.Vx is the current field and f.Vx_o the previous one.  Returns
    (iters_done, [err …]) like pt_solve."""
    nx, ny, nz = f.Pr.shape
    if (sp.nx, sp.ny, sp.nz) != (nx, ny, nz):
        raise L.Ns3dError("time_step: params grid %r differs from Pr's %r" % ((sp.nx, sp.ny, sp.nz), (nx, ny, nz)))
    shapes = {"Pr": (nx, ny, nz), "dPrdtau": (nx - 2, ny - 2, nz - 2), "divV": (nx, ny, nz), "Vx": (nx + 1, ny, nz),
              "Vy": (nx, ny + 1, nz), "Vz": (nx, ny, nz + 1), "Vx_o": (nx + 1, ny, nz), "Vy_o": (nx, ny + 1, nz),
              "Vz_o": (nx, ny, nz + 1), "C": (nx, ny, nz), "C_o": (nx, ny, nz), "txx": (nx, ny, nz), "tyy": (nx, ny, nz),
              "tzz": (nx, ny, nz), "txy": (nx - 1, ny - 1, nz - 1), "txz": (nx - 1, ny - 1, nz - 1), "tyz": (nx - 1, ny - 1, nz - 1)}
    sf = L.StepFields()
    for n, shp in shapes.items():
        t = getattr(f, n, None)
        setattr(sf, n, None if t is None else _chk(t, shp, n))
    by_ptr = {getattr(f, n).data_ptr(): getattr(f, n) for n in _STEP_SWAP}
    cap = sp.niter // max(sp.nchk, 1) + 1
    hist = (C.c_double * cap)()
    it, nchecks = C.c_int(0), C.c_int(0)
    _ctx(ctx, f.Pr).call("time_step", f.Pr, C.byref(sf), C.byref(sp), C.byref(it), hist, cap, C.byref(nchecks))
    for n in _STEP_SWAP:
        setattr(f, n, by_ptr[getattr(sf, n)])
    return it.value, list(hist[: nchecks.value])


def pt_solve(Pr, dPrdtau, divV, p, eps, niter, nchk, err_mul, err_div, ctx=None):
    """The inner loop multi.jl:458-471 / gpu.jl:126-137 on one rank; err = max|Rp|*err_mul/err_div
    (= maximum(abs.(Rp))*ly^2/psc). Returns (iters_done, [err …])."""
    nx, ny, nz = Pr.shape
    cap = niter // max(nchk, 1) + 1
    hist = (C.c_double * cap)()
    it, nchecks = C.c_int(0), C.c_int(0)
    _ctx(ctx, Pr).call("pt_solve", Pr, _chk(Pr, None, "Pr"), _chk(dPrdtau, (nx - 2, ny - 2, nz - 2), "dPrdtau"),
                       _chk(divV, (nx, ny, nz), "divV"), C.byref(p), C.c_double(eps), int(niter), int(nchk),
                       C.c_double(err_mul), C.c_double(err_div), C.byref(it), hist, cap, C.byref(nchecks))
    return it.value, list(hist[: nchecks.value])


# ---- observers of a running flow: monitor, statistics, vortex fields, tracers and probes, isosurfaces ----------------
def diag_params(nx, ny, nz, dx, dy, dz, rho, seam_lo=(0, 0, 0), seam_hi=(0, 0, 0), cylinder=None):
    """lib.DiagParams for ns3d_diagnostics.  cylinder: None, or set_cylinder!'s scalars in the reference's own order —
    15 values (a2,b2,ox,oy,sinβ,cosβ,xco_g,yco_g,zco_g,lx,ly,lz,dx,dy,dz: multi.jl:249) or 12 (…,cosβ,lx,ly,lz,dx,dy,dz: gpu.jl:336),
    told apart by their number like set_cylinder's own arguments."""
    dp = L.DiagParams(nx=int(nx), ny=int(ny), nz=int(nz), dx=dx, dy=dy, dz=dz, rho=rho)
    dp.seam_lo[:] = [int(bool(q)) for q in seam_lo]
    dp.seam_hi[:] = [int(bool(q)) for q in seam_hi]
    if cylinder is not None:
        cyl = tuple(float(q) for q in cylinder)
        if len(cyl) == 15:
            dp.cylinder = 1
            dp.a2, dp.b2, dp.ox, dp.oy, dp.sinb, dp.cosb, dp.xco_g, dp.yco_g, dp.zco_g, dp.lx, dp.ly, dp.lz = cyl[:12]
        elif len(cyl) == 12:
            dp.cylinder = 2
            dp.a2, dp.b2, dp.ox, dp.oy, dp.sinb, dp.cosb, dp.lx, dp.ly, dp.lz = cyl[:9]
        else:
            raise TypeError("diag_params: cylinder takes set_cylinder!'s 15 (multi.jl) or 12 (gpu.jl) scalars")
    return dp


def diag_record(d):
    """lib.Diag → a namespace of Python values (vmax, mom, n_masked: tuples per direction)."""
    from types import SimpleNamespace
    return SimpleNamespace(vmax=tuple(d.vmax), div_max=d.div_max, pr_min=d.pr_min, pr_max=d.pr_max, ke=d.ke, c_vol=d.c_vol,
                           mom=tuple(d.mom), n_masked=tuple(int(q) for q in d.n_masked), nonfinite=int(d.nonfinite))


def diagnostics(Vx, Vy, Vz, Pr, Cf, dp, ctx=None):
    """ns3d_diagnostics: the flow monitor — one read-only pass over the fields on the device (include/ns3d.h): max|V| per
    direction, max|∇V|, min / max Pr, kinetic energy, Σ C·dV, the momentum set_cylinder! is about to remove and a non-finite flag,
    over the entries this rank owns (dp.seam_lo / seam_hi).  Pr or Cf may be None (their entries come back NaN).  Blocks."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    if (dp.nx, dp.ny, dp.nz) != (nx, ny, nz):
        raise L.Ns3dError("diagnostics: params grid %r differs from the fields' %r" % ((dp.nx, dp.ny, dp.nz), (nx, ny, nz)))
    out = L.Diag()
    opt = lambda t, n: None if t is None else _chk(t, (nx, ny, nz), n)
    _ctx(ctx, Vx).call("diagnostics", Vx, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), opt(Pr, "Pr"), opt(Cf, "C"), C.byref(dp), C.byref(out))
    return diag_record(out)


def _chk_blocks(t, nblocks, cells, name):
    """a float64 device array of `nblocks` consecutive column-major (nx,ny,nz) blocks: kernels.zeros((nx, ny, nz·nblocks)) or any
    contiguous float64 tensor of that many elements"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
        raise L.Ns3dError("%s must be a float64 CUDA/HIP tensor" % name)
    if t.numel() != nblocks * cells:
        raise L.Ns3dError("%s has %d elements, expected %d blocks of %d" % (name, t.numel(), nblocks, cells))
    if t.dim() == 3:
        return _chk(t, None, name)
    if not t.is_contiguous():
        raise L.Ns3dError("%s must be contiguous" % name)
    return C.c_void_p(t.data_ptr())


def stats_accumulate(S, Vx, Vy, Vz, Pr, weight=1.0, ctx=None):
    """ns3d_stats_accumulate: one sample into the running sums S (lib.NS3D_STATS_SLOTS blocks of (nx,ny,nz) float64, slot order
    stats.SLOTS): S += weight·(u, v, w, p, uu, vv, ww, uv, uw, vw, pp) of the cell-centred values, one fused pass on the device.
    Pr may be None (slots p and pp are left alone).  Enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    c = _ctx(ctx, Vx)
    c.call("stats_accumulate", Vx, _chk_blocks(S, L.NS3D_STATS_SLOTS, nx * ny * nz, "S"), *_chk_V(Vx, Vy, Vz, (nx, ny, nz)),
           None if Pr is None else _chk(Pr, (nx, ny, nz), "Pr"), C.c_double(float(weight)), nx, ny, nz)


def vortex(Vx, Vy, Vz, dx, dy, dz, *, Wx=None, Wy=None, Wz=None, Q=None, ctx=None):
    """ns3d_vortex: the vorticity components Wx, Wy, Wz and the Q-criterion of the staggered velocity field, each a cell-centred
    (nx,ny,nz) array of the fields' dtype, in one fused pass on the device (include/ns3d.h has the expression).  Interior cells
    receive the values, every other entry +0.0.  Only the outputs that are given are computed; at least one is needed.
    Enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    outs = []
    for name, t in (("Wx", Wx), ("Wy", Wy), ("Wz", Wz), ("Q", Q)):
        if t is None:
            outs.append(None)
            continue
        outs.append(_chk(t, (nx, ny, nz), name))
        if t.dtype != Vx.dtype or t.device != Vx.device:
            raise L.Ns3dError("%s is %s on %s, the velocities are %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    if all(o is None for o in outs):
        raise L.Ns3dError("vortex: give at least one of Wx, Wy, Wz, Q")
    for name, t in (("Vy", Vy), ("Vz", Vz)):
        if isinstance(t, torch.Tensor) and (t.dtype != Vx.dtype or t.device != Vx.device):
            raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    _ctx(ctx, Vx).call("vortex", Vx, *outs, *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), *_d(dx, dy, dz), nx, ny, nz)


def _chk_points(t, n, blocks, dtype, name, ref):
    """a contiguous device array of `blocks`·n elements of `dtype` on the fields' device: X and U are (3, n) float64, state (n,) uint8"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        raise L.Ns3dError("%s must be a %s CUDA/HIP tensor" % (name, dtype))
    if t.device != ref.device:
        raise L.Ns3dError("%s is on %s, the field on %s" % (name, t.device, ref.device))
    if not t.is_contiguous() or t.numel() != blocks * n:
        raise L.Ns3dError("%s must be contiguous with %d x %d elements, got shape %s" % (name, blocks, n, tuple(t.shape)))
    return C.c_void_p(t.data_ptr())


def sample(A, X, out, state=None, stagger=(0, 0, 0), ctx=None):
    """ns3d_sample: the field A (any extents ≥ 2; `stagger` flags the directions whose nodes sit at integers) interpolated at the
    points X — a (3, n) float64 array of INDEX-space coordinates ξ | η | ζ — into out (n float64), trilinear as backtrack!
    (include/ns3d.h has the definition; the same bits in every arithmetic mode).  Points that are dead (state, n uint8, optional),
    not finite or outside the closed box receive NaN.  Enqueues; no read-back."""
    n = out.numel() if isinstance(out, torch.Tensor) else 0
    ex, ey, ez = A.shape
    sx, sy, sz = (int(q) for q in stagger)
    _ctx(ctx, A).call("sample", A, _chk_points(out, n, 1, torch.float64, "out", A), _chk_points(X, n, 3, torch.float64, "X", A),
                      None if state is None else _chk_points(state, n, 1, torch.uint8, "state", A), C.c_long(n),
                      _chk(A, None, "A"), ex, ey, ez, sx, sy, sz)


def tracers_advance(X, state, Vx, Vy, Vz, cx, cy, cz, U=None, ctx=None):
    """ns3d_tracers_advance: one explicit-midpoint step of the particles X ((3, n) float64, index space) with state (n uint8: 1 alive)
    through the frozen field Vx, Vy, Vz; cx, cy, cz = dt/dx, dt/dy, dt/dz.  Particles that leave the closed box [0,nx]×[0,ny]×[0,nz]
    or reach a non-finite position die where they are; U ((3, n) float64, optional) receives the velocity at the start points.
    In place; enqueues; no read-back."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    n = state.numel() if isinstance(state, torch.Tensor) else 0
    for name, t in (("Vy", Vy), ("Vz", Vz)):
        if isinstance(t, torch.Tensor) and (t.dtype != Vx.dtype or t.device != Vx.device):
            raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    _ctx(ctx, Vx).call("tracers_advance", Vx, _chk_points(X, n, 3, torch.float64, "X", Vx), _chk_points(state, n, 1, torch.uint8, "state", Vx),
                       None if U is None else _chk_points(U, n, 3, torch.float64, "U", Vx), C.c_long(n),
                       *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), *_d(cx, cy, cz), nx, ny, nz)


def _int3(v):
    return None if v is None else (C.c_int * 3)(*(int(q) for q in v))


def sample_at(A, X, out, state=None, stagger=(0, 0, 0), origin=None, ctx=None):
    """ns3d_sample_at: `sample` for a rank of a decomposed grid — X holds GLOBAL index-space coordinates, A is the rank's local array
    and origin = coords·(n−2) its first cell; the field is interpolated at X − origin, points outside the LOCAL array receive NaN.
    origin=None: zeros, the bits of `sample`."""
    n = out.numel() if isinstance(out, torch.Tensor) else 0
    ex, ey, ez = A.shape
    sx, sy, sz = (int(q) for q in stagger)
    _ctx(ctx, A).call("sample_at", A, _chk_points(out, n, 1, torch.float64, "out", A), _chk_points(X, n, 3, torch.float64, "X", A),
                      None if state is None else _chk_points(state, n, 1, torch.uint8, "state", A), C.c_long(n),
                      _chk(A, None, "A"), ex, ey, ez, sx, sy, sz, _int3(origin))


def tracers_advance_at(X, state, Vx, Vy, Vz, cx, cy, cz, U=None, origin=None, n_g=None, ctx=None):
    """ns3d_tracers_advance_at: `tracers_advance` for a rank of a decomposed grid — X holds GLOBAL index-space coordinates, the
    fields are the rank's local arrays, origin = coords·(n−2), n_g the global cell grid whose closed box decides who is alive; the
    velocity is interpolated at X − origin.  origin / n_g None: zeros resp. the local grid, the bits of `tracers_advance`."""
    nx, ny, nz = Vx.shape[0] - 1, Vx.shape[1], Vx.shape[2]
    n = state.numel() if isinstance(state, torch.Tensor) else 0
    for name, t in (("Vy", Vy), ("Vz", Vz)):
        if isinstance(t, torch.Tensor) and (t.dtype != Vx.dtype or t.device != Vx.device):
            raise L.Ns3dError("%s is %s on %s, Vx is %s on %s" % (name, t.dtype, t.device, Vx.dtype, Vx.device))
    _ctx(ctx, Vx).call("tracers_advance_at", Vx, _chk_points(X, n, 3, torch.float64, "X", Vx),
                       _chk_points(state, n, 1, torch.uint8, "state", Vx),
                       None if U is None else _chk_points(U, n, 3, torch.float64, "U", Vx), C.c_long(n),
                       *_chk_V(Vx, Vy, Vz, (nx, ny, nz)), *_d(cx, cy, cz), nx, ny, nz, _int3(origin), _int3(n_g))


def isosurface(A, level, color=None, box=None, origin=None, tri=None, val=None, cap=0, ctx=None):
    """ns3d_isosurface: the triangles of the level set A = level by marching tetrahedra (include/ns3d.h has the definition; the same
    bits in every arithmetic mode), in index space.  A: any column-major array of extents ≥ 2 whose entries are nodes at integer
    positions; color: a second array of the same shape, interpolated at the vertices into val; box = (lo_x, lo_y, lo_z, hi_x, hi_y,
    hi_z), a closed node range (None: the whole array); origin: three ints added to the node indices.  tri (≥ 9·cap float64) and val
    (≥ 3·cap float64) receive the first min(n, cap) triangles; cap = 0 without tri is the count-only form.  Returns n, the number
    of triangles the surface has; blocks for that read-back."""
    ex, ey, ez = A.shape
    cap = int(cap)
    if isinstance(color, torch.Tensor) and (color.dtype != A.dtype or color.device != A.device):
        raise L.Ns3dError("color is %s on %s, A is %s on %s" % (color.dtype, color.device, A.dtype, A.device))
    ptrs = []
    for name, t, per in (("tri", tri, 9), ("val", val, 3)):
        if t is None:
            ptrs.append(None)
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.device != A.device:
            raise L.Ns3dError("%s must be a contiguous float64 CUDA/HIP tensor on A's device" % name)
        if t.numel() < per * cap:
            raise L.Ns3dError("%s holds %d elements, cap = %d needs %d" % (name, t.numel(), cap, per * cap))
        ptrs.append(C.c_void_p(t.data_ptr()))
    b = None if box is None else (C.c_int * 6)(*(int(q) for q in box))
    o = None if origin is None else (C.c_int * 3)(*(int(q) for q in origin))
    n = C.c_longlong(-1)
    _ctx(ctx, A).call("isosurface", A, _chk(A, None, "A"), None if color is None else _chk(color, (ex, ey, ez), "color"), ex, ey, ez, b, o,
                      C.c_double(float(level)), ptrs[0], ptrs[1], C.c_longlong(cap), C.byref(n))
    return n.value


def _untyped(ctx, ref, name, *args):
    c = _ctx(ctx, ref)
    c.follow_torch_stream()
    L.check(getattr(c.lib, name)(c.handle, *args))


def stats_reset(S, shape, ctx=None):
    """ns3d_stats_reset: S = 0 on the context's stream; shape = (nx, ny, nz) of one block."""
    nx, ny, nz = (int(q) for q in shape)
    _untyped(ctx, S, "ns3d_stats_reset", _chk_blocks(S, L.NS3D_STATS_SLOTS, nx * ny * nz, "S"), nx, ny, nz)


def stats_finalize(S, wsum, mean, rs, shape, ctx=None):
    """ns3d_stats_finalize: mean (4 blocks) = S[u,v,w,p]/wsum; rs (7 blocks, or None) = S[uu…vw,pp]/wsum − ā·b̄."""
    nx, ny, nz = (int(q) for q in shape)
    n = nx * ny * nz
    _untyped(ctx, S, "ns3d_stats_finalize", _chk_blocks(S, L.NS3D_STATS_SLOTS, n, "S"), C.c_double(float(wsum)),
             _chk_blocks(mean, 4, n, "mean"), None if rs is None else _chk_blocks(rs, 7, n, "rs"), nx, ny, nz)
