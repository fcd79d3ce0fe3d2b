"""NumPy statement of the Boussinesq buoyancy of the 3-D cylinder channel
(TEST INFRASTRUCTURE ONLY).

What cfd_predictor3d_buoy_f32, cfd_predictor3d_les_buoy_f32 and their *_zper
forms implement, as float32 array code on (nz, ny, nx) fields.  The reference
project is 2-D and has no scalar, so the GPU path is pinned to these
functions; tests/test_buoyancy3d_host.py pins them in turn to a literal
per-cell loop.

    theta = T - F(t_ref)
    f*    = p + dt * (b_f * theta)        f in {u, v, w}

on the cells the plain predictor updates (the interior; with periodic z every
plane), p the plain predictor's value (tests/ref3d.py, tests/les3d_reference.py,
the pad rule of tests/zper_reference.py); every operation is a float32
operation in the order written.  tau and nu_t are the plain predictor's.

``BuoyantCylinder3DReference`` / ``BuoyantPeriodicCylinder3DReference`` are
the CPU forms of CylinderChannel3DSolver.time_step with richardson != 0.
"""
import numpy as np

from cyl3d_reference import vorticity3d_numpy
from les3d_reference import predictor3d_les_numpy
from ref3d import C, divergence3d_numpy, predictor3d_numpy, project3d_numpy
from scalar3d_reference import (ScalarCylinder3DReference, ScalarPeriodicCylinder3DReference, scalar_advance3d_numpy,
                                scalar_bc_heat3d_numpy)
from zper_reference import (crop_z, divergence3d_zper_numpy, pad_z, project3d_zper_numpy, vorticity3d_zper_numpy)

F = np.float32


def buoyancy_vector_numpy(cfg):
    """(b, t_ref): b_i = F(k g_i / |g|) with k = -Ri V_inf^2 / (2 R_cylinder
    (scalar_cylinder - scalar_inlet)) in double, rounded once per component;
    t_ref = F(scalar_reference, else scalar_inlet)."""
    dT = cfg.scalar_cylinder - cfg.scalar_inlet
    k = -cfg.richardson * cfg.V_inf ** 2 / (2.0 * cfg.R_cylinder * dT)
    gx, gy, gz = (float(g) for g in cfg.gravity_direction)
    n = np.sqrt(gx * gx + gy * gy + gz * gz)
    b = tuple(F(k * (g / n)) for g in (gx, gy, gz))
    t_ref = F(cfg.scalar_inlet if cfg.scalar_reference is None else cfg.scalar_reference)
    return b, t_ref


def add_buoyancy_numpy(pr, T, b, t_ref, dt):
    """pr's u_star, v_star, w_star with dt * (b_f * (T - t_ref)) added on the
    interior, in place; returns pr."""
    T = np.ascontiguousarray(T, F)
    dt = F(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        theta = T[C] - F(t_ref)
        for name, bf in zip(("u_star", "v_star", "w_star"), b):
            star = pr[name]
            star[C] = star[C] + dt * (F(bf) * theta)
            assert star.dtype == F
    return pr


def predictor3d_buoyant_numpy(u, v, w, T, nu_eff, b, t_ref, *, dx, dy, dz, dt, use_supg, periodic_z=False):
    """{"u_star", "v_star", "w_star", "tau"}: predictor3d_numpy plus the
    buoyant term on the interior.  periodic_z: the pad rule, T padded like the
    fields (every plane is interior in z)."""
    if periodic_z:
        out = predictor3d_buoyant_numpy(pad_z(u), pad_z(v), pad_z(w), pad_z(T), nu_eff, b, t_ref, dx=dx, dy=dy,
                                        dz=dz, dt=dt, use_supg=use_supg)
        return {k: crop_z(a) for k, a in out.items()}
    pr = predictor3d_numpy(u, v, w, nu_eff, dx=dx, dy=dy, dz=dz, dt=dt, use_supg=use_supg)
    return add_buoyancy_numpy(pr, T, b, t_ref, dt)


def predictor3d_les_buoyant_numpy(u, v, w, T, nu, art_visc, cs, b, t_ref, *, dx, dy, dz, dt, use_supg,
                                  periodic_z=False):
    """The same on predictor3d_les_numpy (also "nu_t")."""
    if periodic_z:
        out = predictor3d_les_buoyant_numpy(pad_z(u), pad_z(v), pad_z(w), pad_z(T), nu, art_visc, cs, b, t_ref,
                                            dx=dx, dy=dy, dz=dz, dt=dt, use_supg=use_supg)
        return {k: crop_z(a) for k, a in out.items()}
    pr = predictor3d_les_numpy(u, v, w, nu, art_visc, cs, dx=dx, dy=dy, dz=dz, dt=dt, use_supg=use_supg)
    return add_buoyancy_numpy(pr, T, b, t_ref, dt)


class _BuoyantStep:
    """time_step of a scalar cylinder reference restated with the buoyant
    predictor (the classes below it call the plain predictor inline): the
    predictor reads the step's incoming T, then the step is
    Cylinder3DReference's / PeriodicCylinder3DReference's, then the scalar's
    advance, heating and faces as in scalar3d_reference._ScalarStep."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.b, self.t_ref = buoyancy_vector_numpy(cfg)

    def time_step(self):
        c = self.cfg
        per = self._periodic
        sp = dict(dx=c.dx, dy=c.dy, dz=c.dz)
        u, v, w, step = self.u, self.v, self.w, self.step  # the projection binds new arrays
        dt = self.adaptive_time_step()
        if c.use_les:
            pr = predictor3d_les_buoyant_numpy(u, v, w, self.T, c.nu, c.artificial_viscosity, c.smagorinsky_constant,
                                               self.b, self.t_ref, dt=dt, use_supg=c.use_supg, periodic_z=per, **sp)
            self.nu_t = pr["nu_t"]
        else:
            nu_eff = F(F(c.nu) + F(0.0)) + F(c.artificial_viscosity)
            pr = predictor3d_buoyant_numpy(u, v, w, self.T, nu_eff, self.b, self.t_ref, dt=dt, use_supg=c.use_supg,
                                           periodic_z=per, **sp)
        self.u_star, self.v_star, self.w_star = pr["u_star"], pr["v_star"], pr["w_star"]
        self.bc_ibm(self.u_star, self.v_star, self.w_star)
        div = divergence3d_zper_numpy if per else divergence3d_numpy
        proj = project3d_zper_numpy if per else project3d_numpy
        vort = vorticity3d_zper_numpy if per else vorticity3d_numpy
        self.div_u_star = div(self.u_star, self.v_star, self.w_star, **sp)
        diag = {"pre_div_max": np.max(np.abs(self.div_u_star))}
        self.phi = self.solve_pressure(self.div_u_star)
        self.u, self.v, self.w, diag["grad_max"] = proj(self.phi, self.u_star, self.v_star, self.w_star, dt=dt, **sp)
        stats = self.bc_ibm(self.u, self.v, self.w)
        self.force_history.append((self.step, *(float(x) for x in stats["force"])))
        self.force_stats.append(stats)
        self.dts.append(float(dt))
        diag["vorticity_max"] = np.nanmax(vort(self.u, self.v, self.w, c.dx, c.dy, c.dz, self.mask)[3])
        self.diagnostics = diag
        e = F(0.5) * ((self.u * self.u + self.v * self.v) + self.w * self.w)
        self.energy_history.append((self.step, float(np.mean(e, dtype=np.float64))))
        for f in (self.u, self.v, self.w):
            np.clip(f, -c.max_velocity, c.max_velocity, out=f)
        self.step += 1
        # the scalar's step, with the step's incoming u, v, w and force_strength
        self.T = scalar_advance3d_numpy(self.T, u, v, w, self.alpha, self.nu_t if c.use_les else None, self.inv_prt,
                                        dt=dt, use_supg=c.use_supg, periodic_z=per, **sp)
        hs = scalar_bc_heat3d_numpy(self.T, self.ibm, c.scalar_inlet, c.scalar_cylinder,
                                    min(1.0, step / c.initial_steps), per)
        self.heat_history.append((step, hs["heat"]))
        self.heat_stats.append(hs)
        return dt


class BuoyantCylinder3DReference(_BuoyantStep, ScalarCylinder3DReference):
    """CPU form of CylinderChannel3DSolver.time_step with richardson != 0."""


class BuoyantPeriodicCylinder3DReference(_BuoyantStep, ScalarPeriodicCylinder3DReference):
    """The same with spanwise_bc="periodic"."""
