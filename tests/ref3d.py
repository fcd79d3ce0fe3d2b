"""NumPy statement of the 3-D projection step (TEST INFRASTRUCTURE ONLY).

The arithmetic cfd_predictor3d_f32, cfd_divergence3d_f32, cfd_project3d_f32
and cfd_apply_lid_bc3d_f32 implement, as float32 array code: the project's own
generalisation of the v5 templates to (nz, ny, nx) fields u, v, w (x fastest;
E/W = x+-1, N/S = y+-1, U/D = z+-1), every 2-D coefficient kept and a z term
appended to each sum.  Every constant is formed in double and rounded once to
float32; every operation is a float32 operation in the order written here.
``Cavity3DReference`` is the CPU form of LidDrivenCavity3DSolver.time_step,
with the pressure solve from the pinned C oracle (oracle.jacobi3d / rbgs3d).
"""
import numpy as np

import oracle

F = np.float32
C = (slice(1, -1),) * 3  # the interior


def _nb(f):
    """Centre and the six neighbours of the interior cells of f."""
    return (f[1:-1, 1:-1, 1:-1], f[1:-1, 1:-1, 2:], f[1:-1, 1:-1, :-2], f[1:-1, 2:, 1:-1], f[1:-1, :-2, 1:-1],
            f[2:, 1:-1, 1:-1], f[:-2, 1:-1, 1:-1])


def pred_constants(dx, dy, dz):
    k = {"h": F(min(dx, dy, dz)), "eps": F(1e-10)}
    for a, d in (("x", dx), ("y", dy), ("z", dz)):
        sd = 0.5 / d
        k["c1" + a] = F(0.5 * sd)
        k["c2" + a] = F(sd * sd)
        k["u" + a] = F(1.0 / d)
        k["l" + a] = F(1.0 / (d * d))
    return k


def supg_tau3d_numpy(u, v, w, nu, dt, k):
    """tau of the interior cells (an array of the interior's shape)."""
    uc, vc, wc = u[C], v[C], w[C]
    nu, dt, two, one = F(nu), F(dt), F(2), F(1)
    vm = np.sqrt((uc * uc + vc * vc) + wc * wc)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pe = (vm * k["h"]) / (nu + k["eps"])
        half = pe / two
        lim = np.where(half < one, half, one)
        t = (k["h"] / (two * vm)) * lim
    return np.where(vm > k["eps"], t, dt / two).astype(F)


def predictor3d_numpy(u, v, w, nu_eff, *, dx, dy, dz, dt, use_supg=True):
    """Returns {"u_star", "v_star", "w_star", "tau"} (tau: zeros without SUPG)."""
    u, v, w = (np.ascontiguousarray(a, F) for a in (u, v, w))
    k = pred_constants(dx, dy, dz)
    nu, dt, two, zero = F(nu_eff), F(dt), F(2), F(0)
    uc, vc, wc = u[C], v[C], w[C]
    tau = np.zeros_like(u)
    if use_supg:
        tau[C] = supg_tau3d_numpy(u, v, w, nu, dt, k)
    t = tau[C]
    out = {"tau": tau}
    for name, f in (("u_star", u), ("v_star", v), ("w_star", w)):
        c, e, wst, n, s, up, dn = _nb(f)
        x2 = (e - two * c) + wst
        y2 = (n - two * c) + s
        z2 = (up - two * c) + dn
        if use_supg:
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
        lap = nu * ((l1 + l2) + l3)
        star = f.copy()
        star[C] = c + dt * (-conv + lap)
        assert star.dtype == F
        out[name] = star
    return out


def divergence3d_numpy(u, v, w, *, dx, dy, dz):
    u, v, w = (np.ascontiguousarray(a, F) for a in (u, v, w))
    cx, cy, cz = F(0.5 / dx), F(0.5 / dy), F(0.5 / dz)
    d = np.zeros_like(u)
    d[C] = (((u[1:-1, 1:-1, 2:] - u[1:-1, 1:-1, :-2]) * cx + (v[1:-1, 2:, 1:-1] - v[1:-1, :-2, 1:-1]) * cy)
            + (w[2:, 1:-1, 1:-1] - w[:-2, 1:-1, 1:-1]) * cz)
    return d


def gradient3d_numpy(phi, *, dx, dy, dz):
    phi = np.ascontiguousarray(phi, F)
    cx, cy, cz = F(0.5 / dx), F(0.5 / dy), F(0.5 / dz)
    gx, gy, gz = np.zeros_like(phi), np.zeros_like(phi), np.zeros_like(phi)
    gx[C] = (phi[1:-1, 1:-1, 2:] - phi[1:-1, 1:-1, :-2]) * cx
    gy[C] = (phi[1:-1, 2:, 1:-1] - phi[1:-1, :-2, 1:-1]) * cy
    gz[C] = (phi[2:, 1:-1, 1:-1] - phi[:-2, 1:-1, 1:-1]) * cz
    return gx, gy, gz


def project3d_numpy(phi, u_star, v_star, w_star, *, dx, dy, dz, dt):
    """(u, v, w, grad_max): u = u_star - dt gx on the interior, the faces
    copied through; grad_max = max sqrt((gx gx + gy gy) + gz gz) (float32)."""
    gx, gy, gz = gradient3d_numpy(phi, dx=dx, dy=dy, dz=dz)
    dt = F(dt)
    out = []
    for s, g in ((u_star, gx), (v_star, gy), (w_star, gz)):
        f = np.array(s, F, copy=True)
        f[C] = s[C] - dt * g[C]
        out.append(f)
    gmax = np.max(np.sqrt((gx * gx + gy * gy) + gz * gz))
    return out[0], out[1], out[2], F(gmax)


def lid_bc3d_numpy(u, v, w, u_lid):
    """In place: u = v = w = 0 on the six faces, then the face y = ny - 1
    gets u = u_lid, v = w = 0, written last (the lid owns its edges)."""
    for f in (u, v, w):
        f[0], f[-1] = 0, 0
        f[:, 0], f[:, -1] = 0, 0
        f[:, :, 0], f[:, :, -1] = 0, 0
    u[:, -1, :] = F(u_lid)
    v[:, -1, :] = 0
    w[:, -1, :] = 0


class Cavity3DReference:
    """CPU form of LidDrivenCavity3DSolver.time_step on the same config."""

    def __init__(self, cfg):
        self.cfg = cfg
        shape = (cfg.nz, cfg.ny, cfg.nx)
        self.u, self.v, self.w = (np.zeros(shape, F) for _ in range(3))
        self.phi = np.zeros(shape, F)
        self.step = 0
        self.energy_history = []
        self.diagnostics = {}

    def adaptive_time_step(self):
        c = self.cfg
        if not c.adaptive_dt:
            return c.dt_base
        if self.step < 1000:
            return F(0.00002)
        h = min(c.dx, c.dy, c.dz)
        vel_max = max(np.max(np.abs(self.u)), np.max(np.abs(self.v)), np.max(np.abs(self.w)), 1e-10)
        dt_cfl = c.cfl_target * h / vel_max
        nu_total = c.nu + F(0.0) + c.artificial_viscosity
        dt_visc = 0.4 * h ** 2 / nu_total
        return F(np.clip(min(dt_cfl, dt_visc), c.dt_min, c.dt_max))

    def solve_pressure(self, div):
        c = self.cfg
        if c.use_fast_pressure:
            phi, _ = oracle.rbgs3d(div, dx=c.dx, dy=c.dy, dz=c.dz, dt=c.dt, iters=c.pressure_iterations,
                                   tol=c.pressure_tolerance)
            return phi
        if not (c.dx == c.dy == c.dz):
            raise ValueError("the 3-D Jacobi solve needs dx == dy == dz")
        return oracle.jacobi3d(div, h=c.dx, dt=c.dt, iters=c.pressure_iterations)

    def time_step(self):
        c = self.cfg
        sp = dict(dx=c.dx, dy=c.dy, dz=c.dz)
        dt = self.adaptive_time_step()
        nu_eff = F(F(c.nu) + F(0.0)) + F(c.artificial_viscosity)
        pr = predictor3d_numpy(self.u, self.v, self.w, nu_eff, dt=dt, use_supg=c.use_supg, **sp)
        self.u_star, self.v_star, self.w_star = pr["u_star"], pr["v_star"], pr["w_star"]
        lid_bc3d_numpy(self.u_star, self.v_star, self.w_star, c.lid_velocity)
        self.div_u_star = divergence3d_numpy(self.u_star, self.v_star, self.w_star, **sp)
        diag = {"pre_div_max": np.max(np.abs(self.div_u_star))}
        self.phi = self.solve_pressure(self.div_u_star)
        self.u, self.v, self.w, diag["grad_max"] = project3d_numpy(self.phi, self.u_star, self.v_star, self.w_star,
                                                                   dt=dt, **sp)
        lid_bc3d_numpy(self.u, self.v, self.w, c.lid_velocity)
        self.diagnostics = diag
        e = F(0.5) * ((self.u * self.u + self.v * self.v) + self.w * self.w)
        self.energy_history.append((self.step, float(np.mean(e, dtype=np.float64))))
        for f in (self.u, self.v, self.w):
            np.clip(f, -c.max_velocity, c.max_velocity, out=f)
        self.step += 1
        return dt


def monitor_health3d_numpy(u, v, w, cfg, step) -> bool:
    """The 2-D check's thresholds (v5.py:599-613) on three fields."""
    if any(np.any(~np.isfinite(f)) for f in (u, v, w)):
        return False
    if max(np.max(np.abs(f)) for f in (u, v, w)) > cfg.max_velocity:
        return False
    div_max = np.max(np.abs(divergence3d_numpy(u, v, w, dx=cfg.dx, dy=cfg.dy, dz=cfg.dz)))
    return not (div_max > (20.0 if step <= 1000 else 2.0))
