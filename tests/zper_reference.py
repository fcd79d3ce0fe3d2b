"""NumPy statement of the spanwise-periodic 3-D cylinder channel (TEST
INFRASTRUCTURE ONLY).

With a periodic z all nz planes of an (nz, ny, nx) field are interior in z:
the U neighbour of plane nz-1 is plane 0 and the D neighbour of plane 0 is
plane nz-1; the four x / y faces behave as in the non-periodic step.

Pad rule.  The periodic form of a field operator Op is crop_z(Op(pad_z(f))):
pad_z puts plane nz-1 in front and plane 0 behind (nz + 2 planes), Op is the
existing NumPy statement (tests/ref3d.py, tests/les3d_reference.py,
vorticity3d_numpy of tests/cyl3d_reference.py) and crop_z drops the first and
last plane.  This is what the cfd_*_zper_f32 field kernels are pinned to, bit
for bit.  The boundary stage is channel_bc_ibm3d_numpy without its face
assignments, and the pressure solve is the arithmetic of oracle_rbgs3d_f32
with z over all planes and the plane neighbours taken modulo nz
(``rbgs3d_zper_numpy``; periodic=False is the oracle itself, which
tests/test_zper_host.py checks).

``PeriodicCylinder3DReference`` is the CPU form of
CylinderChannel3DSolver.time_step with spanwise_bc="periodic".
"""
import numpy as np

from cyl3d_reference import Cylinder3DReference, inlet_numpy, vorticity3d_numpy
from les3d_reference import predictor3d_les_numpy
from ref3d import divergence3d_numpy, predictor3d_numpy, project3d_numpy

F = np.float32


def pad_z(f):
    """Plane nz-1 in front, plane 0 behind: (nz + 2, ny, nx)."""
    f = np.asarray(f)
    return np.ascontiguousarray(np.concatenate([f[-1:], f, f[:1]], axis=0))


def crop_z(f):
    return np.ascontiguousarray(f[1:-1])


def predictor3d_zper_numpy(u, v, w, nu_eff, *, dx, dy, dz, dt, use_supg=True):
    out = predictor3d_numpy(pad_z(u), pad_z(v), pad_z(w), nu_eff, dx=dx, dy=dy, dz=dz, dt=dt, use_supg=use_supg)
    return {k: crop_z(a) for k, a in out.items()}


def predictor3d_les_zper_numpy(u, v, w, nu, art_visc, cs, *, dx, dy, dz, dt, use_supg=True):
    out = predictor3d_les_numpy(pad_z(u), pad_z(v), pad_z(w), nu, art_visc, cs, dx=dx, dy=dy, dz=dz, dt=dt,
                                use_supg=use_supg)
    return {k: crop_z(a) for k, a in out.items()}


def divergence3d_zper_numpy(u, v, w, *, dx, dy, dz):
    return crop_z(divergence3d_numpy(pad_z(u), pad_z(v), pad_z(w), dx=dx, dy=dy, dz=dz))


def project3d_zper_numpy(phi, u_star, v_star, w_star, *, dx, dy, dz, dt):
    """(u, v, w, grad_max); the padded planes' gradient is 0, so the maximum
    over the padded array is the maximum over the nz planes."""
    u, v, w, gmax = project3d_numpy(pad_z(phi), pad_z(u_star), pad_z(v_star), pad_z(w_star), dx=dx, dy=dy, dz=dz,
                                    dt=dt)
    return crop_z(u), crop_z(v), crop_z(w), gmax


def vorticity3d_zper_numpy(u, v, w, dx, dy, dz, mask=None):
    m = None if mask is None else pad_z(mask)
    return tuple(crop_z(a) for a in vorticity3d_numpy(pad_z(u), pad_z(v), pad_z(w), dx, dy, dz, m))


def channel_bc_ibm3d_zper_numpy(u, v, w, y, ibm, y_max, v_inf, step, force_strength):
    """channel_bc_ibm3d_numpy without its third assignment (there are no
    spanwise faces): inlet, outlet copy, channel walls written last, then the
    IBM factor on every plane.  The same return value."""
    u[:, :, 0] = inlet_numpy(y, y_max, v_inf, step)[None, :]
    v[:, :, 0] = 0
    w[:, :, 0] = 0
    for f in (u, v, w):
        f[:, :, -1] = f[:, :, -2]
    for f in (u, v, w):
        f[:, 0, :] = 0
        f[:, -1, :] = 0
    out = {"force": np.zeros(3), "abs": np.zeros(3), "n": 0}
    if ibm is None:
        return out
    ibm = np.asarray(ibm, np.float64)
    sel = ibm > 0
    fac = 1.0 - ibm[sel] * float(force_strength)
    for q, f in enumerate((u, v, w)):
        before = f[:, sel].astype(np.float64)
        after = (before * fac).astype(F)
        f[:, sel] = after
        t = before - after.astype(np.float64)
        out["force"][q] = np.sum(t)
        out["abs"][q] = np.sum(np.abs(t))
        out["n"] = t.size
    return out


def rbgs3d_zper_numpy(div, phi0, *, dx, dy, dz, dt, iters, tol, mask2d=None, periodic=True, maxc=None):
    """oracle_rbgs3d_f32's arithmetic, vectorised per colour (a cell of one
    colour reads only cells of the other, so the order inside a colour does
    not matter): float32 in the order (((a + b) + e) - rhs) * cd with the
    oracle's constants; cell colour (z + i + j + 1 + colour) even, colour 0
    before colour 1, solid cells (``mask2d``, every plane's) skipped,
    max|change| over the updated cells of both colours, stop after the first
    iteration whose max|change| < f32(tol).  periodic: z over all planes with
    the plane neighbours modulo nz (np.roll); else planes 1 .. nz-2 (the
    oracle).  ``maxc``: an optional list that receives each iteration's
    max|change|.  Returns (phi, iterations done)."""
    div = np.ascontiguousarray(div, F)
    phi = np.zeros_like(div) if phi0 is None else np.array(phi0, F, copy=True)
    nz, ny, nx = div.shape
    dx2_inv, dy2_inv, dz2_inv = 1.0 / (dx * dx), 1.0 / (dy * dy), 1.0 / (dz * dz)
    cx, cy, cz = F(dx2_inv), F(dy2_inv), F(dz2_inv)
    cd = F(1.0 / (2.0 * (dx2_inv + dy2_inv + dz2_inv)))
    dt_inv = F(1.0) / F(dt)
    ftol = F(tol)
    z, i, j = np.meshgrid(np.arange(nz), np.arange(1, ny - 1), np.arange(1, nx - 1), indexing="ij")
    live = np.ones(z.shape, bool)
    if not periodic:
        live &= (z >= 1) & (z <= nz - 2)
    if mask2d is not None:
        live &= ~np.asarray(mask2d, bool)[None, 1:-1, 1:-1]
    sel = [live & (((z + i + j + 1 + c) % 2) == 0) for c in (0, 1)]
    rhs = (-div[:, 1:-1, 1:-1]) * dt_inv
    I = (slice(None), slice(1, -1), slice(1, -1))
    done = 0
    for it in range(iters):
        mx = F(0.0)
        for c in (0, 1):
            a = cx * (phi[:, 1:-1, 2:] + phi[:, 1:-1, :-2])
            b = cy * (phi[:, 2:, 1:-1] + phi[:, :-2, 1:-1])
            e = cz * (np.roll(phi, -1, axis=0)[I] + np.roll(phi, 1, axis=0)[I])
            pn = (((a + b) + e) - rhs) * cd
            assert pn.dtype == F
            s = sel[c]
            if s.any():
                ch = np.abs(pn[s] - phi[I][s])
                m = ch[ch == ch]  # the oracle's `change > max_change` never takes a NaN
                if m.size and m.max() > mx:
                    mx = m.max()
                phi[I][s] = pn[s]
        done = it + 1
        if maxc is not None:
            maxc.append(F(mx))
        if mx < ftol:
            break
    return phi, done


def perturbed_u(u2d, z, z_min, z_max, a):
    """The initial u of spanwise_perturbation = a: plane k is
    f32(f64(u2d) (1 + a cos(2 pi (z_k - z_min) / (z_max - z_min))))."""
    ph = 2.0 * np.pi * (np.asarray(z, np.float64) - z_min) / (z_max - z_min)
    return (np.asarray(u2d, F).astype(np.float64)[None] * (1.0 + a * np.cos(ph))[:, None, None]).astype(F)


def perturb_start(ref, z):
    """Apply cfg.spanwise_perturbation to a Cylinder3DReference's start."""
    c = ref.cfg
    if c.spanwise_perturbation != 0.0:
        ref.u = perturbed_u(ref.u[0], z, c.z_min, c.z_max, c.spanwise_perturbation)
    return ref


class PeriodicCylinder3DReference(Cylinder3DReference):
    """CPU form of CylinderChannel3DSolver.time_step with spanwise_bc="periodic"."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.z = cfg.z_min + np.arange(cfg.nz) * cfg.dz
        perturb_start(self, self.z)
        self.iters_done = []

    def solve_pressure(self, div):
        c = self.cfg
        phi, n = rbgs3d_zper_numpy(div, None, dx=c.dx, dy=c.dy, dz=c.dz, dt=c.dt, iters=c.pressure_iterations,
                                   tol=c.pressure_tolerance, mask2d=self.cyl2d)
        self.iters_done.append(n)
        return phi

    def bc_ibm(self, u, v, w):
        c = self.cfg
        return channel_bc_ibm3d_zper_numpy(u, v, w, self.y, self.ibm, c.y_max, c.V_inf, self.step,
                                           min(1.0, self.step / c.initial_steps))

    def time_step(self):
        c = self.cfg
        sp = dict(dx=c.dx, dy=c.dy, dz=c.dz)
        dt = self.adaptive_time_step()
        if c.use_les:
            pr = predictor3d_les_zper_numpy(self.u, self.v, self.w, c.nu, c.artificial_viscosity,
                                            c.smagorinsky_constant, dt=dt, use_supg=c.use_supg, **sp)
            self.nu_t = pr["nu_t"]
        else:
            nu_eff = F(F(c.nu) + F(0.0)) + F(c.artificial_viscosity)
            pr = predictor3d_zper_numpy(self.u, self.v, self.w, nu_eff, dt=dt, use_supg=c.use_supg, **sp)
        self.u_star, self.v_star, self.w_star = pr["u_star"], pr["v_star"], pr["w_star"]
        self.bc_ibm(self.u_star, self.v_star, self.w_star)
        self.div_u_star = divergence3d_zper_numpy(self.u_star, self.v_star, self.w_star, **sp)
        diag = {"pre_div_max": np.max(np.abs(self.div_u_star))}
        self.phi = self.solve_pressure(self.div_u_star)
        self.u, self.v, self.w, diag["grad_max"] = project3d_zper_numpy(self.phi, self.u_star, self.v_star,
                                                                        self.w_star, dt=dt, **sp)
        stats = self.bc_ibm(self.u, self.v, self.w)
        self.force_history.append((self.step, *(float(x) for x in stats["force"])))
        self.force_stats.append(stats)
        self.dts.append(float(dt))
        diag["vorticity_max"] = np.nanmax(vorticity3d_zper_numpy(self.u, self.v, self.w, c.dx, c.dy, c.dz,
                                                                 self.mask)[3])
        self.diagnostics = diag
        e = F(0.5) * ((self.u * self.u + self.v * self.v) + self.w * self.w)
        self.energy_history.append((self.step, float(np.mean(e, dtype=np.float64))))
        for f in (self.u, self.v, self.w):
            np.clip(f, -c.max_velocity, c.max_velocity, out=f)
        self.step += 1
        return dt
