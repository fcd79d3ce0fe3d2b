"""NumPy statement of the passive scalar (temperature) of the 3-D cylinder
channel (TEST INFRASTRUCTURE ONLY).

What cfd_scalar_advance3d_f32 and cfd_scalar_bc_heat3d_f32 (and their *_zper
forms) implement, as float32 array code on (nz, ny, nx) fields in the style of
tests/ref3d.py.  The reference project has no scalar, so the GPU path is
pinned to these functions; tests/test_scalar3d_host.py pins them in turn to
the statements the project already trusts (predictor3d_numpy with f = T, the
LES predictor, the pad rule).

Every constant is formed in double and rounded once to float32; every
operation is a float32 operation in the order written here (the heating: a
float64 operation rounded once).

``ScalarCylinder3DReference`` / ``ScalarPeriodicCylinder3DReference`` are the
CPU forms of CylinderChannel3DSolver.time_step with scalar=True.
"""
import numpy as np

from cyl3d_reference import Cylinder3DReference
from ref3d import C, _nb, pred_constants, supg_tau3d_numpy
from zper_reference import PeriodicCylinder3DReference, crop_z, pad_z

F = np.float32


def scalar_advance3d_numpy(T, u, v, w, alpha, nu_t=None, inv_prt=None, *, dx, dy, dz, dt, use_supg,
                           periodic_z=False):
    """T_new: on the interior T + dt * (-conv + lap), the body of
    predictor3d_numpy's per-field loop with f = T, the cell's own (uc, vc, wc)
    and the cell's diffusivity ae in place of nu: ae = F(alpha), or with
    ``nu_t`` ae = F(alpha) + nu_t * F(inv_prt) per cell.  The SUPG tau is
    supg_tau3d_numpy formed with ae.  The faces copy T through.  periodic_z:
    the pad rule of tests/zper_reference.py."""
    if periodic_z:
        nt = None if nu_t is None else pad_z(nu_t)
        return crop_z(scalar_advance3d_numpy(pad_z(T), pad_z(u), pad_z(v), pad_z(w), alpha, nt, inv_prt, dx=dx,
                                             dy=dy, dz=dz, dt=dt, use_supg=use_supg))
    T, u, v, w = (np.ascontiguousarray(a, F) for a in (T, u, v, w))
    k = pred_constants(dx, dy, dz)
    dt, two, zero = F(dt), F(2), F(0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ae = F(alpha)
        if nu_t is not None:
            ae = F(alpha) + np.ascontiguousarray(nu_t, F)[C] * F(inv_prt)
            assert ae.dtype == F
        uc, vc, wc = u[C], v[C], w[C]
        c, e, wst, n, s, up, dn = _nb(T)
        x2 = (e - two * c) + wst
        y2 = (n - two * c) + s
        z2 = (up - two * c) + dn
        if use_supg:
            t = supg_tau3d_numpy(u, v, w, ae, dt, k)
            ddx = (e - wst) * k["c1x"]
            ddy = (n - s) * k["c1y"]
            ddz = (up - dn) * k["c1z"]
            cs = (uc * ddx + vc * ddy) + wc * ddz
            d2x, d2y, d2z = x2 * k["c2x"], y2 * k["c2y"], z2 * k["c2z"]
            cd = cs - t * ((uc * d2x + vc * d2y) + wc * d2z)
            conv = np.where(t > zero, cd, cs)
        else:
            ddx = np.where(uc > zero, (c - wst) * k["ux"], (e - c) * k["ux"])
            ddy = np.where(vc > zero, (c - s) * k["uy"], (n - c) * k["uy"])
            ddz = np.where(wc > zero, (c - dn) * k["uz"], (up - c) * k["uz"])
            conv = (uc * ddx + vc * ddy) + wc * ddz
        l1, l2, l3 = x2 * k["lx"], y2 * k["ly"], z2 * k["lz"]
        lap = ae * ((l1 + l2) + l3)
        out = T.copy()
        out[C] = c + dt * (-conv + lap)
    assert out.dtype == F
    return out


def face_mask(shape, periodic_z=False):
    """True on the face cells: rows 0 and ny-1, columns 0 and nx-1 and (not
    periodic) planes 0 and nz-1."""
    f = np.zeros(shape, bool)
    f[:, 0, :] = f[:, -1, :] = True
    f[:, :, 0] = f[:, :, -1] = True
    if not periodic_z:
        f[0] = f[-1] = True
    return f


def scalar_heat3d_numpy(T, ibm, t_cyl, force_strength, periodic_z=False):
    """Step 1 alone, in place: every non-face cell (k, i, j) with ibm[i, j] > 0
    relaxes towards t_cyl, after = F(before + (ibm * force_strength) * (t_cyl -
    before)) in float64.  Returns {"heat": sum(t), "abs": sum(|t|), "n":
    count} with t = after - before in float64."""
    out = {"heat": 0.0, "abs": 0.0, "n": 0}
    if ibm is None:
        return out
    ibm = np.asarray(ibm, np.float64)
    sel = np.broadcast_to(ibm > 0, T.shape) & ~face_mask(T.shape, periodic_z)
    m = np.broadcast_to(ibm, T.shape)[sel]
    before = T[sel].astype(np.float64)
    after = (before + (m * float(force_strength)) * (float(t_cyl) - before)).astype(F)
    T[sel] = after
    t = after.astype(np.float64) - before
    return {"heat": float(np.sum(t)), "abs": float(np.sum(np.abs(t))), "n": int(t.size)}


def scalar_faces3d_numpy(T, t_in, periodic_z=False):
    """Steps 2-5, in place, as ordered assignments: spanwise faces (not
    periodic), adiabatic channel walls, outlet, inlet written last."""
    if not periodic_z:
        T[0] = T[1]
        T[-1] = T[-2]
    T[:, 0, :] = T[:, 1, :]
    T[:, -1, :] = T[:, -2, :]
    T[:, :, -1] = T[:, :, -2]
    T[:, :, 0] = F(t_in)


def scalar_faces3d_gather_numpy(T, t_in, periodic_z=False):
    """Steps 2-5 as the gather the kernel uses (returns a new array): a face
    cell (k, i, j >= 1) takes the cell (clamp(k, 1, nz-2), clamp(i, 1, ny-2),
    min(j, nx-2)) of T (periodic: plane k itself), a cell with j = 0 takes
    F(t_in); the other cells keep their value."""
    nz, ny, nx = T.shape
    k, i, j = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ks = k if periodic_z else np.clip(k, 1, nz - 2)
    out = T[ks, np.clip(i, 1, ny - 2), np.minimum(np.maximum(j, 1), nx - 2)]
    out[:, :, 0] = F(t_in)
    assert out.dtype == F
    return out


def scalar_bc_heat3d_numpy(T, ibm, t_in, t_cyl, force_strength, periodic_z=False):
    """In place, in this order: heating (scalar_heat3d_numpy), then the faces
    (scalar_faces3d_numpy).  Returns the heating's sums."""
    stats = scalar_heat3d_numpy(T, ibm, t_cyl, force_strength, periodic_z)
    scalar_faces3d_numpy(T, t_in, periodic_z)
    return stats


def heat_bound(stats):
    """force_bound for the heat sum: |device sum - NumPy sum| <= 2 (n - 1)
    2^-53 sum|t| (the same float64 terms in two orders)."""
    return 2.0 * max(stats["n"] - 1, 0) * 2.0 ** -53 * stats["abs"]


def nusselt_numpy(cfg, q, dt):
    """Nu = Q dx dy dz / (dt (nu / Pr) (T_cyl - T_in) pi Lz)."""
    alpha = float(cfg.nu) / cfg.prandtl
    return q * cfg.dx * cfg.dy * cfg.dz / (dt * alpha * (cfg.scalar_cylinder - cfg.scalar_inlet) * np.pi
                                           * (cfg.z_max - cfg.z_min))


class _ScalarStep:
    """time_step of a cylinder reference with the scalar: the advance with the
    step's incoming u, v, w (and the step's nu_t with LES), then the heating
    with the step's force_strength and the faces."""

    _periodic = False

    def __init__(self, cfg):
        super().__init__(cfg)
        self.T = np.full(self.u.shape, F(cfg.scalar_inlet), F)
        self.alpha = F(float(cfg.nu) / cfg.prandtl)   # cfg.nu is a float32: the division in double
        self.inv_prt = F(1.0 / cfg.turbulent_prandtl)
        self.heat_history, self.heat_stats = [], []

    def time_step(self):
        c = self.cfg
        u, v, w, step = self.u, self.v, self.w, self.step  # the projection binds new arrays
        dt = super().time_step()
        self.T = scalar_advance3d_numpy(self.T, u, v, w, self.alpha, self.nu_t if c.use_les else None,
                                        self.inv_prt, dx=c.dx, dy=c.dy, dz=c.dz, dt=dt, use_supg=c.use_supg,
                                        periodic_z=self._periodic)
        stats = scalar_bc_heat3d_numpy(self.T, self.ibm, c.scalar_inlet, c.scalar_cylinder,
                                       min(1.0, step / c.initial_steps), self._periodic)
        self.heat_history.append((step, stats["heat"]))
        self.heat_stats.append(stats)
        return dt


class ScalarCylinder3DReference(_ScalarStep, Cylinder3DReference):
    """CPU form of CylinderChannel3DSolver.time_step with scalar=True."""


class ScalarPeriodicCylinder3DReference(_ScalarStep, PeriodicCylinder3DReference):
    """The same with spanwise_bc="periodic"."""
    _periodic = True
