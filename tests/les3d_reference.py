"""NumPy statement of the 3-D LES arithmetic (TEST INFRASTRUCTURE ONLY).

The project's own 3-D form of compute_smagorinsky_viscosity_fast (v5.py:96-110)
and of the step's nu_eff (v5.py:388): what cfd_smagorinsky3d_f32,
cfd_predictor3d_nu_f32 and cfd_predictor3d_les_f32 implement, as float32 array
code on (nz, ny, nx) fields.  The reference project is 2-D and ships with LES
switched off, so the GPU path is pinned to these functions and not to the
reference; tests/test_les3d_host.py checks them against a per-cell scalar loop
and against the 2-D statement (tests/les_reference.py) on z-invariant fields.

Every operation is a float32 operation in the order written here.
``Cavity3DLesReference`` is the CPU form of LidDrivenCavity3DSolver.time_step
on a LesCavity3DConfig.
"""
import numpy as np

from ref3d import (Cavity3DReference, divergence3d_numpy, lid_bc3d_numpy, predictor3d_numpy, project3d_numpy)

F = np.float32


def smag3d_constant(dx, dy, dz, cs):
    """c2 = (cs * cbrt(dx dy dz))**2 in Python floats (libm pow), rounded once."""
    return F((cs * (dx * dy * dz) ** (1.0 / 3.0)) ** 2)


def smag3d_q_numpy(u, v, w, dx, dy, dz):
    """q = 2 S_ij S_ij of the interior cells from forward differences to the
    east (x + 1), north (y + 1) and up (z + 1) neighbours."""
    kx, ky, kz = F(1.0 / dx), F(1.0 / dy), F(1.0 / dz)  # pred_constants' ux, uy, uz
    g = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for n, f in (("u", u), ("v", v), ("w", w)):
            c = f[1:-1, 1:-1, 1:-1]
            g[n + "x"] = (f[1:-1, 1:-1, 2:] - c) * kx
            g[n + "y"] = (f[1:-1, 2:, 1:-1] - c) * ky
            g[n + "z"] = (f[2:, 1:-1, 1:-1] - c) * kz
        d = (g["ux"] * g["ux"] + g["vy"] * g["vy"]) + g["wz"] * g["wz"]
        sxy = g["uy"] + g["vx"]
        sxz = g["uz"] + g["wx"]
        syz = g["vz"] + g["wy"]
        o = (sxy * sxy + sxz * sxz) + syz * syz
        q = F(2) * d + o
    assert q.dtype == F
    return q


def smagorinsky3d_numpy(u, v, w, dx, dy, dz, cs):
    """nu_t = c2 sqrt(q) on the interior, 0 on the six faces."""
    u, v, w = (np.ascontiguousarray(a, F) for a in (u, v, w))
    nu_t = np.zeros_like(u)
    with np.errstate(over="ignore", invalid="ignore"):
        nu_t[1:-1, 1:-1, 1:-1] = smag3d_constant(dx, dy, dz, cs) * np.sqrt(smag3d_q_numpy(u, v, w, dx, dy, dz))
    return nu_t


def nu_eff3d_numpy(nu_t, nu, art_visc):
    """(F(nu) + nu_t) + F(art_visc) per cell."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = (F(nu) + nu_t) + F(art_visc)
    assert r.dtype == F
    return r


def predictor3d_nu_numpy(u, v, w, nu_eff, *, dx, dy, dz, dt, use_supg=True):
    """predictor3d_numpy with nu_eff an array of the fields' shape: each
    interior cell's own value enters its tau and its Laplacian factor."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return predictor3d_numpy(u, v, w, np.ascontiguousarray(nu_eff, F)[1:-1, 1:-1, 1:-1], dx=dx, dy=dy, dz=dz,
                                 dt=dt, use_supg=use_supg)


def predictor3d_les_numpy(u, v, w, nu, art_visc, cs, *, dx, dy, dz, dt, use_supg=True):
    """{"u_star", "v_star", "w_star", "tau", "nu_t"} of the LES predictor."""
    nu_t = smagorinsky3d_numpy(u, v, w, dx, dy, dz, cs)
    out = predictor3d_nu_numpy(u, v, w, nu_eff3d_numpy(nu_t, nu, art_visc), dx=dx, dy=dy, dz=dz, dt=dt,
                               use_supg=use_supg)
    out["nu_t"] = nu_t
    return out


class Cavity3DLesReference(Cavity3DReference):
    """CPU form of LidDrivenCavity3DSolver.time_step on a LesCavity3DConfig."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.nu_t = np.zeros_like(self.u)

    def adaptive_time_step(self):
        c = self.cfg
        if not c.use_les or not c.adaptive_dt or self.step < 1000:
            return super().adaptive_time_step()
        h = min(c.dx, c.dy, c.dz)
        vel_max = max(np.max(np.abs(self.u)), np.max(np.abs(self.v)), np.max(np.abs(self.w)), 1e-10)
        dt_cfl = c.cfl_target * h / vel_max
        nu_total = c.nu + F(np.mean(self.nu_t, dtype=np.float64)) + c.artificial_viscosity
        dt_visc = 0.4 * h ** 2 / nu_total
        return F(np.clip(min(dt_cfl, dt_visc), c.dt_min, c.dt_max))

    def time_step(self):
        c = self.cfg
        if not c.use_les:
            return super().time_step()
        sp = dict(dx=c.dx, dy=c.dy, dz=c.dz)
        dt = self.adaptive_time_step()
        pr = predictor3d_les_numpy(self.u, self.v, self.w, c.nu, c.artificial_viscosity, c.smagorinsky_constant,
                                   dt=dt, use_supg=c.use_supg, **sp)
        self.nu_t = pr["nu_t"]
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
