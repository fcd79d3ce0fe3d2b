"""Reference-named device kernels: drop-ins for the @njit functions of v5.py.

Each function keeps the name, argument order and meaning, and the ownership
rules of its reference counterpart in
``python/flow_over_cylinder (Fischer)/v5.py``.  Allocating kernels return fresh
arrays with a zero boundary ring (``np.zeros_like``).  GS, IBM and
divergence cleaning mutate their inputs in place and return them.  The arrays
are torch tensors on the HIP device.  The work runs in the hand-written gfx950
kernels of libcfdsim.so, on the current torch stream.  Nothing here falls back
to the CPU: CPU tensors raise ``TypeError``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import CfdError, call, ptr, stream_handle, lib

__all__ = [
    "compute_convection_fast", "compute_convection_supg_fast", "compute_supg_stabilization_fast",
    "compute_laplacian_fast", "compute_divergence_fast", "compute_gradient_fast",
    "solve_pressure_gauss_seidel_fast", "solve_pressure_jacobi", "apply_ibm_fast",
    "clean_divergence_fast", "predictor_fused", "project_velocity", "solve_pressure_jacobi3d",
    "compute_smagorinsky_viscosity_fast", "predictor_fused_les", "mean64",
    "solve_pressure_jacobi3d_zero",
    "solve_pressure_gauss_seidel3d", "persistent_failures",
    "predictor3d_fused", "compute_divergence3d", "project_velocity3d", "apply_lid_bc3d",
    "predictor3d_fused_les", "compute_smagorinsky_viscosity3d",
    "apply_channel_bc_ibm3d", "compute_vorticity3d", "solve_pressure_gauss_seidel3d_zper",
    "accumulate_flow_stats3d", "scalar_advance3d", "apply_scalar_bc_heat3d",
    "accumulate_flow_scalar_stats3d",
]


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (memory_efficient fields), got {t.dtype}")
    return t


_SFX = {torch.float32: "_f32", torch.float64: "_f64"}


def _fields(name, *ts):
    """Entry point `name` + _f32 / _f64 for the fields' dtype: float32
    (memory_efficient=True, v5.py:287) or float64 (False); every field of one
    call must share it."""
    dt = ts[0].dtype
    if dt not in _SFX:
        raise TypeError(f"{name}: fields must be float32 or float64, got {dt}")
    for t in ts[1:]:
        if t is not None and t.dtype != dt:
            raise TypeError(f"{name}: mixed field dtypes {dt} and {t.dtype}")
    return name + _SFX[dt]


def _dt_arg(dt, field_dtype):
    """The step's dt as it meets the fields (NEP 50): float32 fields round it
    to float32 (np.float32 or a Python float dt_base alike); float64 fields
    take it exactly (the f64 entry points take a double)."""
    return float(np.float32(dt)) if field_dtype == torch.float32 else float(dt)


def _like(phi: torch.Tensor, t, name: str):
    """A companion array of phi (div, scratch, workspace): same shape, dtype,
    device, C-contiguous -- the kernels index it with phi's strides, so a
    mismatch would read or write out of bounds.  None passes through."""
    if t is None:
        return None
    if tuple(t.shape) != tuple(phi.shape) or t.dtype != phi.dtype or t.device != phi.device:
        raise ValueError(f"{name} must match phi: got {tuple(t.shape)} {t.dtype} on {t.device}, "
                         f"phi is {tuple(phi.shape)} {phi.dtype} on {phi.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be C-contiguous")
    return t


def _shape2d(t: torch.Tensor):
    if t.dim() != 2:
        raise ValueError(f"expected a 2-D (ny, nx) array, got shape {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1])


def _mask_u8(mask, shape):
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask shape {tuple(mask.shape)} != field shape {tuple(shape)}")
    m = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
    return m.contiguous()


def _nu(nu_eff, dtype=torch.float32):
    """nu_eff as (array_or_None, scalar): an array is passed through, a scalar
    (LES off: nu + 0 + art_visc, v5.py:388) is broadcast by the kernel, in the
    fields' precision."""
    if isinstance(nu_eff, torch.Tensor) and nu_eff.dim() > 0:
        if nu_eff.dtype != dtype:
            raise TypeError(f"nu_eff must be {dtype}, got {nu_eff.dtype}")
        return nu_eff.contiguous(), 0.0
    return None, float(np.float32(nu_eff)) if dtype == torch.float32 else float(nu_eff)


def compute_smagorinsky_viscosity_fast(u, v, dx, dy, cs, out=None):
    """v5.py:96-110: the Smagorinsky eddy viscosity nu_t = (cs sqrt(dx dy))**2 |S|
    from forward differences, 0 on the boundary ring.  ``out``: an optional
    array of u's shape and dtype to write into.  Returns nu_t."""
    ny, nx = _shape2d(u)
    _like(u, v, "v")
    nu_t = torch.empty_like(u) if out is None else _like(u, out, "out")
    call(_fields("cfd_smagorinsky2d", u, v, nu_t), ptr(u), ptr(v), ptr(nu_t), ny, nx, float(dx), float(dy),
         float(cs), stream_handle())
    return nu_t


def mean64(a, out=None):
    """np.mean(a, dtype=np.float64) of a float32 / float64 device array into a
    float64 device scalar (``out``: a 1-element float64 tensor, allocated if
    omitted), without a host read; partial sums in a fixed order, the same
    bits run to run.  Returns ``out``."""
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=a.device)
    if out.dtype != torch.float64 or out.numel() != 1:
        raise TypeError("mean64: out must be one float64 element")
    call(_fields("cfd_mean", a), ptr(a), int(a.numel()), ptr(out), stream_handle())
    return out


def compute_supg_stabilization_fast(u, v, dx, dy, dt, nu_eff):
    """v5.py:149-162."""
    ny, nx = _shape2d(u)
    tau = torch.empty_like(u)
    nu_a, nu_s = _nu(nu_eff, u.dtype)
    call(_fields("cfd_supg_tau2d", u, v), ptr(u), ptr(v), ptr(nu_a), nu_s, ptr(tau), ny, nx, float(dx), float(dy),
         _dt_arg(dt, u.dtype), stream_handle())
    return tau


def compute_convection_supg_fast(u, v, phi, dx, dy, tau_supg):
    """v5.py:127-147 (derivative factors 1/(4dx), 1/(4dx^2): the reference's quirk)."""
    ny, nx = _shape2d(phi)
    conv = torch.empty_like(phi)
    call(_fields("cfd_convection_supg2d", phi, u, v, tau_supg), ptr(u), ptr(v), ptr(phi), ptr(tau_supg), ptr(conv),
         ny, nx, float(dx), float(dy), stream_handle())
    return conv


def compute_convection_fast(u, v, phi, dx, dy):
    """First-order upwind convection, v5.py:112-125."""
    ny, nx = _shape2d(phi)
    conv = torch.empty_like(phi)
    call(_fields("cfd_convection_upwind2d", phi, u, v), ptr(u), ptr(v), ptr(phi), ptr(conv), ny, nx, float(dx),
         float(dy), stream_handle())
    return conv


def compute_laplacian_fast(phi, dx, dy, nu_eff):
    """v5.py:164-176."""
    ny, nx = _shape2d(phi)
    lap = torch.empty_like(phi)
    nu_a, nu_s = _nu(nu_eff, phi.dtype)
    call(_fields("cfd_laplacian2d", phi), ptr(phi), ptr(nu_a), nu_s, ptr(lap), ny, nx, float(dx), float(dy),
         stream_handle())
    return lap


def compute_divergence_fast(u, v, dx, dy, absmax=None):
    """v5.py:178-187.  ``absmax``: optional zeroed device scalar of the
    fields' dtype that receives max|div| (the v5.py:410 diagnostic) without a
    host sync."""
    ny, nx = _shape2d(u)
    div = torch.empty_like(u)
    call(_fields("cfd_divergence2d", u, v, absmax), ptr(u), ptr(v), ptr(div), ny, nx, float(dx), float(dy),
         ptr(absmax), stream_handle())
    return div


def compute_gradient_fast(phi, dx, dy):
    """v5.py:189-200."""
    ny, nx = _shape2d(phi)
    gx, gy = torch.empty_like(phi), torch.empty_like(phi)
    call(_fields("cfd_gradient2d", phi), ptr(phi), ptr(gx), ptr(gy), ny, nx, float(dx), float(dy), stream_handle())
    return gx, gy


def solve_pressure_gauss_seidel_fast(phi, div_u_star, dx, dy, dt, mask, iterations, tolerance,
                                     workspace=None, iters_done=None, phi_tmp=None, zero_start=False):
    """v5.py:202-226: red-black GS, in place on ``phi``; returns ``phi``.
    ``zero_start``: phi = zeros first (v5.py:337) inside the solve
    (cfd_rbgs2d_zero_f32_ws: the persistent small-grid solve reads nothing of
    phi; other paths zero-fill it first).
    ``iters_done`` (optional int32 device scalar) receives the iteration count.
    float32: ``phi_tmp`` (same-size scratch field, allocated if omitted) lets
    every iteration run as one fused out-of-place pass; the result still lands
    in ``phi``, bit-identical to the in-place colour passes.  float64
    (memory_efficient=False): in-place colour passes (phi_tmp unused)."""
    ny, nx = _shape2d(phi)
    m = _mask_u8(mask, phi.shape)
    ws = workspace
    # the grid-sized workspace (small grids: the persistent solve's exchange
    # rings, cfd_rbgs2d_workspace_bytes) when float32, the base one otherwise
    need = int(lib().cfd_rbgs2d_workspace_bytes(ny, nx, int(iterations)) if phi.dtype == torch.float32
               else lib().cfd_rbgs_workspace_bytes(int(iterations)))
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=phi.device)
    _like(phi, div_u_star, "div_u_star")
    if phi.dtype == torch.float64:
        if zero_start:
            phi.zero_()
        call("cfd_rbgs2d_f64", ptr(phi), ptr(div_u_star), ptr(m), ny, nx, float(dx), float(dy),
             float(np.float32(dt)), int(iterations), float(tolerance), ptr(ws), ptr(iters_done), stream_handle())
        return phi
    tmp = torch.empty_like(phi) if phi_tmp is None else _like(phi, phi_tmp, "phi_tmp")
    call("cfd_rbgs2d_zero_f32_ws" if zero_start else "cfd_rbgs2d_f32_ws", ptr(_f32(phi, "phi")), ptr(_f32(div_u_star, "div_u_star")), ptr(m), ny, nx,
         float(dx), float(dy), float(np.float32(dt)), int(iterations), float(tolerance), ptr(_f32(tmp, "phi_tmp")),
         ptr(ws), ws.numel() * ws.element_size(), ptr(iters_done), stream_handle())
    return phi


def solve_pressure_jacobi(phi, div_u_star, dx, dt, mask, iterations, phi_tmp=None,
                          resid_every=0, resid_out=None, rhs_ws=None, zero_start=False):
    """Jacobi branch of solve_pressure_fast, v5.py:336-346, bit-exact; in place
    on ``phi`` (float32 or float64 fields); returns ``phi``.  ``rhs_ws``: an
    optional same-size workspace that lets the sweeps skip the division.
    ``zero_start``: phi = zeros first (v5.py:337) inside the solve
    (cfd_jacobi2d_zero_*: the persistent small-grid solve reads nothing of
    phi, no fill launch)."""
    ny, nx = _shape2d(phi)
    if div_u_star.dtype != phi.dtype:
        raise TypeError("phi and div_u_star must share a dtype")
    _like(phi, div_u_star, "div_u_star")
    _like(phi, rhs_ws, "rhs_ws")
    tmp = torch.empty_like(phi) if phi_tmp is None else _like(phi, phi_tmp, "phi_tmp")
    m = _mask_u8(mask, phi.shape)
    z = "_zero" if zero_start else ""
    fn = {torch.float32: f"cfd_jacobi2d{z}_f32", torch.float64: f"cfd_jacobi2d{z}_f64"}.get(phi.dtype)
    if fn is None:
        raise TypeError(f"unsupported dtype {phi.dtype}")
    call(fn, ptr(div_u_star), ptr(phi), ptr(tmp), ptr(rhs_ws), ptr(m), ny, nx, float(dx),
         float(np.float32(dt)), int(iterations), int(resid_every), ptr(resid_out), stream_handle())
    return phi


def solve_pressure_jacobi3d(phi, div, h, dt, mask, iterations, phi_tmp=None, resid_every=0,
                            resid_out=None, rhs_ws=None):
    """7-point generalisation of the Jacobi branch on an (nz, ny, nx) float32 grid."""
    if phi.dim() != 3:
        raise ValueError("expected (nz, ny, nx)")
    nz, ny, nx = (int(s) for s in phi.shape)
    _like(phi, _f32(div, "div"), "div")
    _like(phi, rhs_ws, "rhs_ws")
    tmp = torch.empty_like(phi) if phi_tmp is None else _like(phi, phi_tmp, "phi_tmp")
    m = _mask_u8(mask, phi.shape)
    call("cfd_jacobi3d_f32", ptr(_f32(div, "div")), ptr(_f32(phi, "phi")), ptr(tmp), ptr(rhs_ws), ptr(m),
         nz, ny, nx, float(h), float(np.float32(dt)), int(iterations), int(resid_every), ptr(resid_out),
         stream_handle())
    return phi


def solve_pressure_jacobi3d_zero(phi, div, h, dt, iterations, phi_tmp=None, rhs_ws=None):
    """The Jacobi branch of solve_pressure_fast in 3-D, zero fill included
    (v5.py:337-346): phi = zeros, then `iterations` sweeps.  With ``rhs_ws``
    the first pass starts from the zeros itself (no fill, no RHS prologue, no
    final copy; cfd_jacobi3d_zero_f32).  Returns phi."""
    if phi.dim() != 3:
        raise ValueError("expected (nz, ny, nx)")
    nz, ny, nx = (int(s) for s in phi.shape)
    tmp = torch.empty_like(phi) if phi_tmp is None else phi_tmp
    _f32(phi, "phi")
    for t, name in ((tmp, "phi_tmp"), (rhs_ws, "rhs_ws"), (div, "div")):
        _like(phi, t, name)
    call("cfd_jacobi3d_zero_f32", ptr(_f32(div, "div")), ptr(_f32(phi, "phi")), ptr(tmp), ptr(rhs_ws),
         nz, ny, nx, float(h), float(np.float32(dt)), int(iterations), stream_handle())
    return phi


def solve_pressure_gauss_seidel3d(phi, div, dx, dy, dz, dt, mask, iterations, tolerance,
                                  workspace=None, iters_done=None, phi_tmp=None):
    """3-D red-black generalisation of v5.py:202-226, in place on ``phi``
    (``phi_tmp``: as in solve_pressure_gauss_seidel_fast).  ``mask``: None, an
    (nz, ny, nx) solid mask (in-place colour passes), or an (ny, nx) mask that
    applies to every plane (cfd_rbgs3d_mask2d_f32: fused passes, the same bits
    as the expanded mask)."""
    nz, ny, nx = (int(s) for s in phi.shape)
    mask2d = mask is not None and mask.dim() == 2
    m = _mask_u8(mask, (ny, nx) if mask2d else phi.shape)
    need = int(lib().cfd_rbgs_workspace_bytes(int(iterations)))
    ws = workspace
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=phi.device)
    tmp = torch.empty_like(phi) if phi_tmp is None else _like(phi, phi_tmp, "phi_tmp")
    _like(phi, div, "div")
    call("cfd_rbgs3d_mask2d_f32" if mask2d else "cfd_rbgs3d_f32", ptr(_f32(phi, "phi")), ptr(_f32(div, "div")),
         ptr(m), nz, ny, nx, float(dx),
         float(dy), float(dz), float(np.float32(dt)), int(iterations), float(tolerance), ptr(_f32(tmp, "phi_tmp")),
         ptr(ws), ptr(iters_done), stream_handle())
    return phi


def solve_pressure_gauss_seidel3d_zper(phi_pad, div_pad, dx, dy, dz, dt, mask2d, iterations, tolerance,
                                       workspace=None, iters_done=None, phi_tmp=None, nz=None):
    """solve_pressure_gauss_seidel3d with a periodic z (cfd_rbgs3d_zper_f32):
    all nz planes are updated, plane nz-1's U neighbour is plane 0; nz even
    and >= 4.  ``phi_pad``, ``div_pad`` and ``phi_tmp`` are (nz + 2G, ny, nx)
    with G = cfd_rbgs3d_zper_ghost(); the caller fills planes G .. G+nz-1
    (``phi_pad[G:G+nz]`` is the solution afterwards), the ghost planes of all
    three are the solver's and ``div_pad``'s are written.  ``mask2d``: None or
    the (ny, nx) solid mask of every plane.  ``nz``: the number of periodic
    planes (default: phi_pad's planes minus 2G); arrays that are not padded to
    it raise CfdError.  Without ``phi_tmp`` the solve runs in-place colour
    passes (the same bits).  Returns phi_pad."""
    G = int(lib().cfd_rbgs3d_zper_ghost())
    nzt, ny, nx = _shape3d(_f32(phi_pad, "phi_pad"))
    nz = nzt - 2 * G if nz is None else int(nz)
    for name, t in (("phi_pad", phi_pad), ("div_pad", div_pad), ("phi_tmp", phi_tmp)):
        if t is not None and (tuple(t.shape) != (nz + 2 * G, ny, nx) or t.dtype != torch.float32
                              or t.device != phi_pad.device):
            raise CfdError(f"solve_pressure_gauss_seidel3d_zper: {name} must be a float32 ({nz + 2 * G}, {ny}, {nx}) "
                           f"array (nz = {nz} planes plus {G} ghost planes at each end) on {phi_pad.device}, "
                           f"got {tuple(t.shape)} {t.dtype} on {t.device}")
    m = _mask_u8(mask2d, (ny, nx))
    need = int(lib().cfd_rbgs_workspace_bytes(int(iterations)))
    ws = workspace
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=phi_pad.device)
    call("cfd_rbgs3d_zper_f32", ptr(phi_pad), ptr(_f32(div_pad, "div_pad")), ptr(m), nz, ny, nx, float(dx),
         float(dy), float(dz), float(np.float32(dt)), int(iterations), float(tolerance), ptr(phi_tmp), ptr(ws),
         ptr(iters_done), stream_handle())
    return phi_pad


def apply_ibm_fast(u, v, ibm_mask, force_strength):
    """v5.py:228-237, in place; ``ibm_mask`` is the float64 mask. Returns (u, v)."""
    if ibm_mask.dtype != torch.float64:
        raise TypeError("ibm_mask is float64 in the reference (v5.py:281-283)")
    call(_fields("cfd_apply_ibm2d", u, v), ptr(u), ptr(v), ptr(ibm_mask), int(u.numel()), float(force_strength),
         stream_handle())
    return u, v


def clean_divergence_fast(u, v, dx, dy, iterations=2, workspace=None):
    """v5.py:239-257, in place; serial (lexicographic) order of the phi sweep."""
    ny, nx = _shape2d(u)
    need = int(lib().cfd_clean_divergence_workspace_bytes(ny, nx))
    ws = workspace
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=u.device)
    call(_fields("cfd_clean_divergence2d", u, v), ptr(u), ptr(v), ny, nx, float(dx), float(dy), int(iterations),
         ptr(ws), stream_handle())
    return u, v


TAU_MODES = {"exact": 0, "fast": 1}


def _with_tau_mode(tau_mode, fn):
    """Run fn() under tau_mode ("exact" / "fast"; None: the thread's current
    setting), restoring the calling thread's setting afterwards."""
    prev = None
    if tau_mode is not None:
        prev = int(lib().cfd_get_predictor2d_tau_mode())
        if prev != TAU_MODES[tau_mode]:
            call("cfd_set_predictor2d_tau_mode", TAU_MODES[tau_mode])
        else:
            prev = None
    try:
        fn()
    finally:
        if prev is not None:
            call("cfd_set_predictor2d_tau_mode", prev)


def predictor_fused_les(u, v, dx, dy, dt, nu, art_visc, cs, use_supg=True, u_star=None, v_star=None, tau=None,
                        nu_t=None, tau_mode=None):
    """The LES predictor (use_les=True, v5.py:381-403) in one pass: nu_t =
    compute_smagorinsky_viscosity_fast(u, v, dx, dy, cs), nu_eff = (nu + nu_t)
    + art_visc per cell in the fields' dtype, then predictor_fused's
    arithmetic -- the same bits as those calls, with nu_t formed in the row
    march's registers.  Returns (u_star, v_star, tau, nu_t).  ``nu_t`` None:
    nu_t is not stored (the row march only; the one-thread-per-cell path
    needs the array and raises).  tau_mode: as in predictor_fused."""
    ny, nx = _shape2d(u)
    if tau_mode is not None and tau_mode not in TAU_MODES:
        raise ValueError(f"tau_mode must be one of {sorted(TAU_MODES)}, not {tau_mode!r}")
    us = torch.empty_like(u) if u_star is None else u_star
    vs = torch.empty_like(v) if v_star is None else v_star
    if tau is None and use_supg:
        tau = torch.empty_like(u)
    nt = nu_t
    for t, name in ((v, "v"), (us, "u_star"), (vs, "v_star"), (tau, "tau"), (nt, "nu_t")):
        _like(u, t, name)
    f32 = u.dtype == torch.float32
    sc = (lambda x: float(np.float32(x))) if f32 else float
    _with_tau_mode(tau_mode, lambda: call(
        _fields("cfd_predictor2d_les", u, v, us, vs, tau, nt), ptr(u), ptr(v), sc(nu), sc(art_visc), float(cs),
        ptr(us), ptr(vs), ptr(tau), ptr(nt), ny, nx, float(dx), float(dy), _dt_arg(dt, u.dtype),
        int(bool(use_supg)), stream_handle()))
    return us, vs, tau, nt


def predictor_fused(u, v, dx, dy, dt, nu_eff, use_supg=True, u_star=None, v_star=None, tau=None, tau_mode=None):
    """v5.py:388-403 in one pass: returns (u_star, v_star, tau).

    tau_mode: "exact" (the reference's NumPy scalar `**`: glibc powf / pow,
    bit-exact), "fast" (the compiled reference's fastmath x*x / sqrt, within
    1e-6 relative L-inf), or None (the calling thread's current setting,
    cfd_set_predictor2d_tau_mode; "exact" unless changed).  A given mode
    applies to this call only: the thread's setting is restored after it.
    Without SUPG a given tau is filled with zeros (the reference's
    never-assigned np.zeros, v5.py:292)."""
    ny, nx = _shape2d(u)
    if tau_mode is not None and tau_mode not in TAU_MODES:
        raise ValueError(f"tau_mode must be one of {sorted(TAU_MODES)}, not {tau_mode!r}")
    us = torch.empty_like(u) if u_star is None else u_star
    vs = torch.empty_like(v) if v_star is None else v_star
    if tau is None and use_supg:
        tau = torch.empty_like(u)
    nu_a, nu_s = _nu(nu_eff, u.dtype)
    _with_tau_mode(tau_mode, lambda: call(
        _fields("cfd_predictor2d", u, v, us, vs, tau), ptr(u), ptr(v), ptr(nu_a), nu_s, ptr(us), ptr(vs),
        ptr(tau), ny, nx, float(dx), float(dy), _dt_arg(dt, u.dtype), int(bool(use_supg)), stream_handle()))
    return us, vs, tau


def project_velocity(phi, u_star, v_star, dx, dy, dt, u=None, v=None, gradmax=None):
    """v5.py:413-417: u = u* - dt*dphi/dx, v = v* - dt*dphi/dy.  Returns (u, v)."""
    ny, nx = _shape2d(phi)
    u = torch.empty_like(u_star) if u is None else u
    v = torch.empty_like(v_star) if v is None else v
    call(_fields("cfd_project2d", phi, u_star, v_star, u, v, gradmax), ptr(phi), ptr(u_star), ptr(v_star), ptr(u),
         ptr(v), ny, nx, float(dx), float(dy), _dt_arg(dt, phi.dtype), ptr(gradmax), stream_handle())
    return u, v


# ------------------------------------------------------ 3-D projection step
def _shape3d(t: torch.Tensor):
    if t.dim() != 3:
        raise ValueError(f"expected a 3-D (nz, ny, nx) array, got shape {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def _fields3d(model, /, **others):
    """model as the (nz, ny, nx) float32 pattern; every other array (None
    passes) must match its shape, dtype, device and be C-contiguous."""
    shape = _shape3d(_f32(model, "field"))
    ptr(model)  # device and contiguity
    for name, t in others.items():
        _like(model, t, name)
    return shape


def _buoyancy_args(who, buoyancy, t_ref):
    """(bx, by, bz, t_ref) as Python floats of float32 values for the buoyant
    predictor entry points."""
    if buoyancy is None or len(buoyancy) != 3:
        raise ValueError(f"{who}: with T, buoyancy is the three float32 coefficients (bx, by, bz)")
    return tuple(float(np.float32(b)) for b in buoyancy) + (float(np.float32(t_ref)),)


def predictor3d_fused(u, v, w, dx, dy, dz, dt, nu_eff, use_supg=True, u_star=None, v_star=None, w_star=None,
                      tau=None, store_tau=True, periodic_z=False, T=None, buoyancy=None, t_ref=0.0):
    """The 3-D fused predictor (cfd_predictor3d_f32): SUPG tau, convection and
    Laplacian of u, v, w and f_star = f + dt*(-conv + lap) in one pass, the six
    faces copied through.  ``nu_eff`` is a scalar, or a tensor of the fields'
    shape read per cell (cfd_predictor3d_nu_f32).  Returns (u_star, v_star,
    w_star, tau); arrays not given are allocated.  ``store_tau=False`` with no
    ``tau`` given: tau is not stored (24 B per cell instead of 28) and None is
    returned for it.  Without SUPG a stored tau is zeros.  ``periodic_z``:
    every plane is interior in z and plane nz-1's U neighbour is plane 0
    (cfd_predictor3d_zper_f32; scalar ``nu_eff`` only).  ``T`` (a tensor of the
    fields' shape; scalar ``nu_eff`` only): Boussinesq buoyancy, the interior
    cells' f_star gains dt * (b_f * (T - t_ref)) in float32 with ``buoyancy`` =
    (bx, by, bz) (cfd_predictor3d_buoy_f32 / _buoy_zper_f32); without ``T``
    the calls are the plain ones."""
    us = torch.empty_like(u) if u_star is None else u_star
    vs = torch.empty_like(u) if v_star is None else v_star
    ws = torch.empty_like(u) if w_star is None else w_star
    if tau is None and store_tau:
        tau = torch.empty_like(u)
    if T is not None:
        if isinstance(nu_eff, torch.Tensor) and nu_eff.dim() > 0:
            raise ValueError("predictor3d_fused: buoyancy (T) takes a scalar nu_eff (LES: predictor3d_fused_les)")
        b = _buoyancy_args("predictor3d_fused", buoyancy, t_ref)
        nz, ny, nx = _fields3d(u, v=v, w=w, T=T, u_star=us, v_star=vs, w_star=ws, tau=tau)
        call("cfd_predictor3d_buoy_zper_f32" if periodic_z else "cfd_predictor3d_buoy_f32", ptr(u), ptr(v), ptr(w),
             ptr(T), float(np.float32(nu_eff)), *b, ptr(us), ptr(vs), ptr(ws), ptr(tau), nz, ny, nx, float(dx),
             float(dy), float(dz), _dt_arg(dt, u.dtype), int(bool(use_supg)), stream_handle())
        return us, vs, ws, tau
    if isinstance(nu_eff, torch.Tensor) and nu_eff.dim() > 0:
        if periodic_z:
            raise ValueError("predictor3d_fused: periodic_z takes a scalar nu_eff (LES: predictor3d_fused_les)")
        nz, ny, nx = _fields3d(u, v=v, w=w, nu_eff=nu_eff, u_star=us, v_star=vs, w_star=ws, tau=tau)
        call("cfd_predictor3d_nu_f32", ptr(u), ptr(v), ptr(w), ptr(nu_eff), ptr(us), ptr(vs), ptr(ws), ptr(tau),
             nz, ny, nx, float(dx), float(dy), float(dz), _dt_arg(dt, u.dtype), int(bool(use_supg)), stream_handle())
        return us, vs, ws, tau
    nz, ny, nx = _fields3d(u, v=v, w=w, u_star=us, v_star=vs, w_star=ws, tau=tau)
    call("cfd_predictor3d_zper_f32" if periodic_z else "cfd_predictor3d_f32", ptr(u), ptr(v), ptr(w),
         float(np.float32(nu_eff)), ptr(us), ptr(vs), ptr(ws),
         ptr(tau), nz, ny, nx, float(dx), float(dy), float(dz), _dt_arg(dt, u.dtype), int(bool(use_supg)),
         stream_handle())
    return us, vs, ws, tau


def compute_smagorinsky_viscosity3d(u, v, w, dx, dy, dz, cs, out=None):
    """The Smagorinsky eddy viscosity in 3-D (cfd_smagorinsky3d_f32): nu_t =
    (cs (dx dy dz)**(1/3))**2 |S| from forward differences to the east, north
    and up neighbours, 0 on the six faces -- the project's own 3-D form of
    compute_smagorinsky_viscosity_fast (the reference is 2-D; the arithmetic
    is stated in tests/les3d_reference.py).  ``out``: an optional array of
    u's shape to write into (not an input).  Returns nu_t."""
    nu_t = torch.empty_like(u) if out is None else out
    nz, ny, nx = _fields3d(u, v=v, w=w, out=nu_t)
    call("cfd_smagorinsky3d_f32", ptr(u), ptr(v), ptr(w), ptr(nu_t), nz, ny, nx, float(dx), float(dy), float(dz),
         float(cs), stream_handle())
    return nu_t


def predictor3d_fused_les(u, v, w, dx, dy, dz, dt, nu, art_visc, cs, use_supg=True, u_star=None, v_star=None,
                          w_star=None, tau=None, nu_t=None, store_tau=True, store_nu_t=True, periodic_z=False,
                          T=None, buoyancy=None, t_ref=0.0):
    """The 3-D LES predictor (cfd_predictor3d_les_f32) in one pass: nu_t =
    compute_smagorinsky_viscosity3d(u, v, w, ...), nu_eff = (nu + nu_t) +
    art_visc per cell in float32, then predictor3d_fused with that array --
    the same bits as those calls, with nu_t formed from the values the kernel
    holds anyway.  Returns (u_star, v_star, w_star, tau, nu_t); arrays not
    given are allocated, unless ``store_tau`` / ``store_nu_t`` is False: that
    array is then not stored and None is returned for it.  ``periodic_z``: as
    in predictor3d_fused (cfd_predictor3d_les_zper_f32; nu_t on all planes).
    ``T``, ``buoyancy``, ``t_ref``: Boussinesq buoyancy as in predictor3d_fused
    (cfd_predictor3d_les_buoy_f32 / _les_buoy_zper_f32); tau and nu_t are
    what they are without it."""
    us = torch.empty_like(u) if u_star is None else u_star
    vs = torch.empty_like(u) if v_star is None else v_star
    ws = torch.empty_like(u) if w_star is None else w_star
    if tau is None and store_tau:
        tau = torch.empty_like(u)
    if nu_t is None and store_nu_t:
        nu_t = torch.empty_like(u)
    if T is not None:
        b = _buoyancy_args("predictor3d_fused_les", buoyancy, t_ref)
        nz, ny, nx = _fields3d(u, v=v, w=w, T=T, u_star=us, v_star=vs, w_star=ws, tau=tau, nu_t=nu_t)
        call("cfd_predictor3d_les_buoy_zper_f32" if periodic_z else "cfd_predictor3d_les_buoy_f32", ptr(u), ptr(v),
             ptr(w), ptr(T), float(np.float32(nu)), float(np.float32(art_visc)), float(cs), *b, ptr(us), ptr(vs),
             ptr(ws), ptr(tau), ptr(nu_t), nz, ny, nx, float(dx), float(dy), float(dz), _dt_arg(dt, u.dtype),
             int(bool(use_supg)), stream_handle())
        return us, vs, ws, tau, nu_t
    nz, ny, nx = _fields3d(u, v=v, w=w, u_star=us, v_star=vs, w_star=ws, tau=tau, nu_t=nu_t)
    call("cfd_predictor3d_les_zper_f32" if periodic_z else "cfd_predictor3d_les_f32", ptr(u), ptr(v), ptr(w),
         float(np.float32(nu)), float(np.float32(art_visc)),
         float(cs), ptr(us), ptr(vs), ptr(ws), ptr(tau), ptr(nu_t), nz, ny, nx, float(dx), float(dy), float(dz),
         _dt_arg(dt, u.dtype), int(bool(use_supg)), stream_handle())
    return us, vs, ws, tau, nu_t


def compute_divergence3d(u, v, w, dx, dy, dz, out=None, absmax=None, periodic_z=False):
    """div = ((uE-uW) cx + (vN-vS) cy) + (wU-wD) cz, 0 on the six faces.
    ``absmax``: optional zeroed float32 device scalar that receives max|div|
    without a host sync.  ``periodic_z``: z wraps and only the four x / y
    faces are 0 (cfd_divergence3d_zper_f32).  Returns div (``out`` if given)."""
    div = torch.empty_like(u) if out is None else out
    nz, ny, nx = _fields3d(u, v=v, w=w, div=div)
    if absmax is not None:
        _f32(absmax, "absmax")
    call("cfd_divergence3d_zper_f32" if periodic_z else "cfd_divergence3d_f32", ptr(u), ptr(v), ptr(w), ptr(div),
         nz, ny, nx, float(dx), float(dy), float(dz), ptr(absmax), stream_handle())
    return div


def project_velocity3d(phi, u_star, v_star, w_star, dx, dy, dz, dt, u=None, v=None, w=None, gradmax=None,
                       periodic_z=False):
    """u = u* - dt dphi/dx, v = v* - dt dphi/dy, w = w* - dt dphi/dz on the
    interior, the faces copied through.  ``gradmax``: optional zeroed float32
    device scalar for max|grad phi|.  ``periodic_z``: z wraps and only the
    four x / y faces are copied through (cfd_project3d_zper_f32).  Returns
    (u, v, w)."""
    u = torch.empty_like(phi) if u is None else u
    v = torch.empty_like(phi) if v is None else v
    w = torch.empty_like(phi) if w is None else w
    nz, ny, nx = _fields3d(phi, u_star=u_star, v_star=v_star, w_star=w_star, u=u, v=v, w=w)
    if gradmax is not None:
        _f32(gradmax, "gradmax")
    call("cfd_project3d_zper_f32" if periodic_z else "cfd_project3d_f32", ptr(phi), ptr(u_star), ptr(v_star),
         ptr(w_star), ptr(u), ptr(v), ptr(w), nz, ny, nx, float(dx), float(dy), float(dz), _dt_arg(dt, phi.dtype),
         ptr(gradmax), stream_handle())
    return u, v, w


def apply_lid_bc3d(u, v, w, u_lid):
    """Cavity walls in place: u = v = w = 0 on the six faces, then u = u_lid,
    v = w = 0 on the face y = ny - 1 (the lid owns its edges).  Returns (u, v, w)."""
    nz, ny, nx = _fields3d(u, v=v, w=w)
    call("cfd_apply_lid_bc3d_f32", ptr(u), ptr(v), ptr(w), nz, ny, nx, float(np.float32(u_lid)), stream_handle())
    return u, v, w


def apply_channel_bc_ibm3d(u, v, w, y, ibm_mask2d, y_max, v_inf, step, force_strength, bbox=None, force_out=None,
                           periodic_z=False):
    """The cylinder channel's boundary conditions and immersed-boundary forcing
    in place on (nz, ny, nx) float32 u, v, w, one launch
    (cfd_apply_channel_bc_ibm3d_f32): inlet column (``y``: the float64 row
    coordinates, ``step`` drives the perturbation), outlet copy, free-slip
    spanwise faces, channel walls, then the factor 1 - m*force_strength where
    the float64 (ny, nx) ``ibm_mask2d`` (None: no IBM) is positive, on every
    plane.  ``bbox`` = (i0, i1, j0, j1): half-open rows and columns holding
    every m > 0 (None: the whole plane); only that box is visited for the
    forcing.  ``force_out``: optional float64 device tensor of 3 elements,
    accumulated into (zero it first): the sums of before - after of u, v, w
    over the forced cells.  ``periodic_z``: no spanwise faces -- the other
    assignments on every plane (cfd_apply_channel_bc_ibm3d_zper_f32).
    Returns (u, v, w)."""
    nz, ny, nx = _fields3d(u, v=v, w=w)
    if y.dtype != torch.float64 or y.numel() != ny:
        raise ValueError(f"y must be {ny} float64 row coordinates, got {tuple(y.shape)} {y.dtype}")
    if ibm_mask2d is not None and (ibm_mask2d.dtype != torch.float64 or tuple(ibm_mask2d.shape) != (ny, nx)):
        raise ValueError(f"ibm_mask2d must be a float64 ({ny}, {nx}) array, got {tuple(ibm_mask2d.shape)} "
                         f"{ibm_mask2d.dtype}")
    if force_out is not None and (force_out.dtype != torch.float64 or force_out.numel() != 3):
        raise ValueError("force_out must be three float64 elements")
    i0, i1, j0, j1 = (0, ny, 0, nx) if bbox is None else (int(b) for b in bbox)
    call("cfd_apply_channel_bc_ibm3d_zper_f32" if periodic_z else "cfd_apply_channel_bc_ibm3d_f32", ptr(u), ptr(v),
         ptr(w), ptr(y), ptr(ibm_mask2d), nz, ny, nx, float(y_max), float(v_inf), int(step), float(force_strength),
         i0, i1, j0, j1, ptr(force_out), stream_handle())
    return u, v, w


def scalar_advance3d(T, u, v, w, alpha, dt, dx, dy, dz, use_supg=True, *, nu_t=None, inv_prt=0.0, out,
                     periodic_z=False):
    """The passive scalar's advance (cfd_scalar_advance3d_f32), one launch:
    out = T + dt*(-conv + lap) on the interior with the 3-D predictor's
    per-field arithmetic applied to T, advected by the cell's own u, v, w, the
    diffusivity ``alpha`` (a scalar, rounded to float32) in place of nu -- or,
    with ``nu_t`` (an array of the fields' shape), alpha + nu_t * inv_prt per
    cell in float32 (``inv_prt``: float32(1 / turbulent Prandtl number)).  The
    six faces copy T through.  ``out`` must be given and be none of the
    inputs.  ``periodic_z``: every plane is interior in z and z wraps
    (cfd_scalar_advance3d_zper_f32).  Returns out."""
    nz, ny, nx = _fields3d(T, u=u, v=v, w=w, nu_t=nu_t, out=out)
    call("cfd_scalar_advance3d_zper_f32" if periodic_z else "cfd_scalar_advance3d_f32", ptr(T), ptr(u), ptr(v),
         ptr(w), float(np.float32(alpha)), ptr(nu_t), float(np.float32(inv_prt)), ptr(out), nz, ny, nx, float(dx),
         float(dy), float(dz), _dt_arg(dt, T.dtype), int(bool(use_supg)), stream_handle())
    return out


def apply_scalar_bc_heat3d(T, ibm_mask2d, t_in, t_cyl, force_strength, *, bbox=None, heat_out=None,
                           periodic_z=False):
    """Heating by the immersed boundary, then the scalar's faces, in place on
    the (nz, ny, nx) float32 ``T`` (cfd_scalar_bc_heat3d_f32): every non-face
    cell where the float64 (ny, nx) ``ibm_mask2d`` (None: no heating) is
    positive relaxes towards ``t_cyl``, T += (m * force_strength)(t_cyl - T)
    formed in float64 and rounded once; then the spanwise faces, the adiabatic
    channel walls and the outlet copy their interior neighbour and the inlet
    column is ``t_in``.  ``bbox`` = (i0, i1, j0, j1): half-open rows and
    columns holding every m > 0 (None: the whole plane); only that box is
    visited for the heating.  ``heat_out``: optional float64 device tensor of
    one element, added to: the sum of after - before over the heated cells.
    ``periodic_z``: no spanwise faces (cfd_scalar_bc_heat3d_zper_f32).
    Returns T."""
    nz, ny, nx = _fields3d(T)
    if ibm_mask2d is not None and (ibm_mask2d.dtype != torch.float64 or tuple(ibm_mask2d.shape) != (ny, nx)
                                   or ibm_mask2d.device != T.device):
        raise ValueError(f"ibm_mask2d must be a float64 ({ny}, {nx}) array on {T.device}, got "
                         f"{tuple(ibm_mask2d.shape)} {ibm_mask2d.dtype} on {ibm_mask2d.device}")
    if heat_out is not None and (heat_out.dtype != torch.float64 or heat_out.numel() != 1
                                 or heat_out.device != T.device):
        raise ValueError("heat_out must be one float64 element on the field's device")
    i0, i1, j0, j1 = (0, ny, 0, nx) if bbox is None else (int(b) for b in bbox)
    call("cfd_scalar_bc_heat3d_zper_f32" if periodic_z else "cfd_scalar_bc_heat3d_f32", ptr(T), ptr(ibm_mask2d), nz,
         ny, nx, float(t_in), float(t_cyl), float(force_strength), i0, i1, j0, j1, ptr(heat_out), stream_handle())
    return T


def compute_vorticity3d(u, v, w, dx, dy, dz, mask=None, components=False, absmax=None, periodic_z=False):
    """The vorticity magnitude of (nz, ny, nx) float32 u, v, w
    (cfd_vorticity3d_f32): central differences on the interior, 0 on the six
    faces, NaN where the (nz, ny, nx) ``mask`` is set.  Returns mag, or
    (ox, oy, oz, mag) with ``components=True``.  ``absmax``: optional zeroed
    float32 device scalar that receives nanmax(mag) without a host sync.
    ``periodic_z``: z wraps and only the four x / y faces are 0
    (cfd_vorticity3d_zper_f32)."""
    mag = torch.empty_like(u)
    nz, ny, nx = _fields3d(u, v=v, w=w)
    comp = [torch.empty_like(u) for _ in range(3)] if components else [None] * 3
    if absmax is not None:
        _f32(absmax, "absmax")
    m = _mask_u8(mask, u.shape)
    call("cfd_vorticity3d_zper_f32" if periodic_z else "cfd_vorticity3d_f32", ptr(u), ptr(v), ptr(w), ptr(m),
         ptr(comp[0]), ptr(comp[1]), ptr(comp[2]), ptr(mag), ptr(absmax), nz, ny, nx, float(dx), float(dy), float(dz),
         stream_handle())
    return (comp[0], comp[1], comp[2], mag) if components else mag


def _accumulate_stats3d(symbol, fields, nm, shape, acc, weight, span_average):
    """Check ``acc`` ((nm, ny, nx) with ``span_average``, else (nm, nz, ny, nx),
    float64, on the fields' device) and call ``symbol`` on ``fields``."""
    nz, ny, nx = shape
    want = (nm, ny, nx) if span_average else (nm, nz, ny, nx)
    dev = fields[0].device
    if acc.dtype != torch.float64 or tuple(acc.shape) != want or acc.device != dev:
        raise ValueError(f"acc must be a float64 {want} array on {dev}, got {tuple(acc.shape)} {acc.dtype} "
                         f"on {acc.device}")
    call(symbol, *(ptr(f) for f in fields), ptr(acc), nz, ny, nx, float(weight), 1 if span_average else 0,
         stream_handle())
    return acc


def accumulate_flow_stats3d(u, v, w, acc, weight, span_average, nu_t=None):
    """acc += weight * moments of (nz, ny, nx) float32 u, v, w
    (cfd_flow_stats3d_f32).  The moments are u, v, w, uu, vv, ww, uv, uw, vw
    and, with ``nu_t``, nu_t as a tenth, each formed in float64.  ``acc`` is
    float64: (nm, nz, ny, nx), or with ``span_average`` (nm, ny, nx), which
    receives weight times the float64 sum over z.  Deterministic (no atomics);
    every cell counts.  Returns acc."""
    shape = _fields3d(u, v=v, w=w, nu_t=nu_t)
    return _accumulate_stats3d("cfd_flow_stats3d_f32", (u, v, w, nu_t), 9 if nu_t is None else 10, shape, acc, weight,
                               span_average)


def accumulate_flow_scalar_stats3d(u, v, w, T, acc, weight, span_average, nu_t=None):
    """accumulate_flow_stats3d with the scalar ``T`` (cfd_flow_scalar_stats3d_f32):
    after its moments (u .. vw, then nu_t when given) come T, TT, uT, vT, wT,
    so ``acc`` has 14 planes, or 15 with ``nu_t``.  The first 9 (10) planes
    get exactly the bits accumulate_flow_stats3d gives them.  ``T`` may be
    one of u, v, w.  Returns acc."""
    shape = _fields3d(u, v=v, w=w, nu_t=nu_t, T=T)
    return _accumulate_stats3d("cfd_flow_scalar_stats3d_f32", (u, v, w, nu_t, T), 14 if nu_t is None else 15, shape,
                               acc, weight, span_average)


def persistent_failures(stream=None) -> int:
    """How many persistent small-grid solves (the one-launch 2-D Jacobi /
    red-black GS) run on ``stream`` (default: the current stream) had a tile
    wait expire since the last call; their phi is all NaN.  Reads and clears
    that stream's failure word with an async copy and synchronises that
    stream only (cfd_persistent_status_stream): solvers on other streams keep
    running and keep their own counts."""
    import ctypes
    n = ctypes.c_int(0)
    call("cfd_persistent_status_stream", stream_handle(stream), ctypes.byref(n))
    return int(n.value)
