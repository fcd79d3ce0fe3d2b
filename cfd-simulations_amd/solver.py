"""GPU drop-in for the reference cylinder solver's time-stepping path.

``OptimizedTurbulentConfig`` and ``OptimizedTurbulentSolver`` keep the field
names, method names and return values of
``python/flow_over_cylinder (Fischer)/v5.py:41-441``.  The fields (``u``, ``v``,
``phi``, ``u_star``, ...) are torch tensors on the HIP device, float32
(``memory_efficient=True``, the reference default) or float64 (False,
v5.py:287).  Every
per-step array pass runs in libcfdsim's gfx950 kernels, and the step needs no
host synchronisation (except adaptive dt after step 1000, which, like the
reference, reads max|V|, and with LES the mean nu_t in the same read).

LES (``use_les=True``, v5.py:60,96-110,381-388): the Smagorinsky eddy
viscosity is formed inside the fused predictor (``K.predictor_fused_les``) and
kept in ``nu_t``.  The reference ships with LES switched off and has no LES
fixture, so this path is pinned to the project's own NumPy statement of the
arithmetic (tests/les_reference.py); parity with the reference is unpinned.

``LidDrivenCavity3DSolver`` is the same projection step in 3-D around the 3-D
pressure solves (the project's own generalisation: the reference is 2-D only).
With a ``LesCavity3DConfig`` it runs the 3-D LES predictor
(``K.predictor3d_fused_les``; pinned to tests/les3d_reference.py).
``CylinderChannel3DSolver`` is that step on the cylinder channel extruded along
z: channel boundary conditions with the immersed-boundary forcing in one
kernel, the masked 3-D pressure solves, drag / lift and vorticity (pinned to
tests/cyl3d_reference.py).

Out of scope: plotting and video (OptimizedVisualizer),
and HDF5 output (h5py is absent; ``save_snapshot`` writes the same layout to
``.npz``).
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import kernels as K
from ._lib import call, ptr, stream_handle, lib


@dataclass
class OptimizedTurbulentConfig:
    """v5.py:41-94; same fields, defaults and derived values (dx, dy, and the
    float32 casts of nu, dt and artificial_viscosity, v5.py:78-83)."""
    L: float = 1.0
    R_cylinder: float = 0.5
    V_inf: float = 1.0
    cylinder_center: tuple = (4.0, 2.0)
    x_min: float = 0.0
    x_max: float = 20.0
    y_min: float = 0.0
    y_max: float = 4.0
    nx: int = 600
    ny: int = 180
    T_total: float = 30.0
    dt_base: float = 0.00005
    cfl_target: float = 0.1
    adaptive_dt: bool = True
    dt_min: float = 1e-6
    dt_max: float = 0.0001
    Re: float = 600.0
    use_les: bool = False
    smagorinsky_constant: float = 0.0
    use_supg: bool = True
    artificial_viscosity: float = 0.001
    pressure_iterations: int = 1500
    pressure_tolerance: float = 1e-8
    max_velocity: float = 5.0
    initial_steps: int = 1000
    parallel_threads: int = 4
    use_fast_pressure: bool = True
    memory_efficient: bool = True
    vectorized_ops: bool = True
    save_interval: int = 200
    output_dir: str = "v5_re_600"
    hdf5_file: str = "v5_re_600.h5"
    dpi: int = 200
    # build-only knobs (not in the reference)
    log_diagnostics: bool = False   # compute the v5.py:410-435 log values on device
    # SUPG tau arithmetic: "exact" = the reference's NumPy scalar `**` (glibc
    # powf / pow; bit-exact time_step), "fast" = the compiled reference's
    # fastmath form (x*x, correctly rounded sqrt; within 1e-6 relative L-inf)
    supg_tau: str = "exact"
    device: str = "cuda"

    def __post_init__(self):
        self.dx = (self.x_max - self.x_min) / (self.nx - 1)
        self.dy = (self.y_max - self.y_min) / (self.ny - 1)
        self.nu = np.float32(1.0 / self.Re)
        self.dt = np.float32(self.dt_base)
        self.artificial_viscosity = np.float32(self.artificial_viscosity)
        self.parallel_threads = min(self.parallel_threads, os.cpu_count() or 1)
        if self.supg_tau not in ("exact", "fast"):
            raise ValueError(f"supg_tau must be 'exact' or 'fast', not {self.supg_tau!r}")


# ------------------------------------------------------- snapshot files
# The .npz snapshot files of the 2-D and 3-D solvers: groups step_%06d whose
# arrays are members "<group>/<name>.npy" of the zip archive.
def _npz_has_group(path, g):
    """Whether the snapshot file exists and already holds group ``g``."""
    import zipfile
    if not os.path.exists(path):
        return False
    with zipfile.ZipFile(path, "r") as z:
        return f"{g}/u.npy" in z.namelist()


def _npz_append(path, groups):
    """Append the arrays of ``groups`` (member name -> array) to the archive,
    creating it if need be: a save costs O(one group) however many it holds."""
    import zipfile
    with zipfile.ZipFile(path, "a" if os.path.exists(path) else "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, arr in groups.items():
            with z.open(f"{k}.npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arr), allow_pickle=False)


def _npz_pick_group(path, f, step):
    """The name of group ``step`` (None: the latest) of the open file ``f``."""
    steps = sorted({int(k.split("/")[0][5:]) for k in f.files if k.startswith("step_")})
    if not steps:
        raise ValueError(f"{path}: no step_%06d groups")
    g = f"step_{(steps[-1] if step is None else int(step)):06d}"
    if f"{g}/u" not in f.files:
        raise KeyError(f"{path}: no group {g} (have {steps})")
    return g


# ------------------------------------------------------------ host setup
# One-time host-side setup, kept as pure NumPy functions so the CPU tests can
# check them against the reference-generated fixtures without a GPU.
def host_grid(cfg):
    """setup_grid, v5.py:269-273."""
    x = np.linspace(cfg.x_min, cfg.x_max, cfg.nx)
    y = np.linspace(cfg.y_min, cfg.y_max, cfg.ny)
    X, Y = np.meshgrid(x, y, indexing="xy")
    return x, y, X, Y


def host_masks(cfg, X, Y):
    """setup_boundary_masks, v5.py:275-283: (dist, cylinder_mask, ibm_mask)."""
    x_c, y_c = cfg.cylinder_center
    dist = np.sqrt((X - x_c) ** 2 + (Y - y_c) ** 2)
    cyl = dist <= cfg.R_cylinder
    sigma = 2 * cfg.dx
    ibm = np.exp(-((dist - cfg.R_cylinder) / sigma) ** 2)
    ibm = np.where(dist < cfg.R_cylinder, 1.0,
                   np.where(dist < cfg.R_cylinder + 5 * cfg.dx, ibm, 0.0))
    return dist, cyl, ibm


def host_potential_flow(cfg, X, Y, dist, ibm_mask, dtype=np.float32):
    """initialize_potential_flow, v5.py:299-314, vectorised (same formulas,
    float64 then cast to the fields' dtype on assignment: float32, or float64
    when memory_efficient=False)."""
    x_c, y_c = cfg.cylinder_center
    r, m = dist, ibm_mask
    u = np.zeros((cfg.ny, cfg.nx), dtype)
    v = np.zeros((cfg.ny, cfg.nx), dtype)
    if dtype == np.float64:
        # float64 keeps every bit of the per-cell scalar arithmetic: NumPy
        # float64 scalar `**` is libm pow and scalar sin / cos take the scalar
        # loops, which the vectorised array forms below do not reproduce to
        # the last bit (float32 rounding hides that), so restate the loop
        for i in range(cfg.ny):
            for j in range(cfg.nx):
                rij, mv = r[i, j], m[i, j]
                if rij > cfg.R_cylinder + 4 * cfg.dx:
                    theta = np.arctan2(Y[i, j] - y_c, X[i, j] - x_c)
                    factor = (cfg.R_cylinder / rij) ** 2
                    u[i, j] = cfg.V_inf * (1 - factor * np.cos(2 * theta)) * (1 - mv)
                    v[i, j] = -cfg.V_inf * factor * np.sin(2 * theta) * (1 - mv)
                else:
                    blend = min(1.0, ((rij - cfg.R_cylinder) / (4 * cfg.dx)) ** 2)
                    u[i, j] = cfg.V_inf * blend * (1 - mv)
        return u, v
    far = r > cfg.R_cylinder + 4 * cfg.dx
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = np.arctan2(Y - y_c, X - x_c)
        factor = (cfg.R_cylinder / r) ** 2
        u_far = cfg.V_inf * (1 - factor * np.cos(2 * theta)) * (1 - m)
        v_far = -cfg.V_inf * factor * np.sin(2 * theta) * (1 - m)
    blend = np.minimum(1.0, ((r - cfg.R_cylinder) / (4 * cfg.dx)) ** 2)
    u_near = cfg.V_inf * blend * (1 - m)
    u[far] = u_far[far]
    v[far] = v_far[far]
    u[~far] = u_near[~far]
    return u, v


class OptimizedTurbulentSolver:
    """v5.py:259-441 on the GPU.  Array attributes are device tensors."""

    def __init__(self, config: OptimizedTurbulentConfig):
        self.config = config
        # v5.py:287: float32 fields when memory_efficient, else float64
        self.dtype = torch.float32 if config.memory_efficient else torch.float64
        self._sfx = "_f32" if config.memory_efficient else "_f64"
        self._np = np.float32 if config.memory_efficient else np.float64
        self.device = torch.device(config.device)
        if self.device.type != "cuda":
            raise TypeError("OptimizedTurbulentSolver runs on the HIP device only")
        self._has_ibm = True  # immersed-boundary forcing (the cylinder); the cavity has none
        self.setup_grid()
        self.setup_boundary_masks()
        self.initialize_fields()
        self.step = 0
        self._energy = torch.zeros(1024, dtype=torch.float64, device=self.device)
        self._energy_steps = []
        self.times = []

    # ------------------------------------------------------------- setup
    def setup_grid(self):  # v5.py:269-273 (host, one-time)
        self.x, self.y, self.X, self.Y = host_grid(self.config)
        self._y_dev = torch.from_numpy(self.y).to(self.device)

    def setup_boundary_masks(self):  # v5.py:275-283 (host, one-time)
        self.dist, cyl, ibm = host_masks(self.config, self.X, self.Y)
        self.cylinder_mask_host = cyl
        self.ibm_mask_host = ibm
        self.cylinder_mask = torch.from_numpy(cyl).to(self.device)
        self._mask_u8 = self.cylinder_mask.to(torch.uint8)
        self.ibm_mask = torch.from_numpy(ibm).to(self.device)

    def initialize_fields(self):  # v5.py:285-297
        cfg = self.config
        shape = (cfg.ny, cfg.nx)
        z = lambda: torch.zeros(shape, dtype=self.dtype, device=self.device)  # noqa: E731
        self.u, self.v, self.p, self.nu_t, self.tau_supg = z(), z(), z(), z(), z()
        self.u_star, self.v_star, self.div_u_star, self.phi = z(), z(), z(), z()
        self._phi_tmp = z()
        self._rhs_ws = z()
        # the GS workspace (small float32 grids: with the persistent solve's rings)
        self._gs_ws = torch.empty(int(lib().cfd_rbgs2d_workspace_bytes(cfg.ny, cfg.nx, cfg.pressure_iterations)),
                                  dtype=torch.uint8, device=self.device)
        self._gs_done = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._clean_ws = torch.empty(int(lib().cfd_clean_divergence_workspace_bytes(cfg.ny, cfg.nx)),
                                     dtype=torch.uint8, device=self.device)
        self._scal = torch.zeros(8, dtype=self.dtype, device=self.device)  # diagnostics
        # LES adaptive dt: [mean nu_t (float64), max|V| (the fields' dtype, first bytes)]: one host read
        self._dt_red = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.initialize_potential_flow()

    def initialize_potential_flow(self):  # v5.py:299-314 (host, one-time)
        u, v = host_potential_flow(self.config, self.X, self.Y, self.dist, self.ibm_mask_host, self._np)
        self.u.copy_(torch.from_numpy(u))
        self.v.copy_(torch.from_numpy(v))

    # --------------------------------------------------------- step parts
    def adaptive_time_step(self):  # v5.py:316-326
        cfg = self.config
        if not cfg.adaptive_dt:
            return cfg.dt_base
        if self.step < 1000:
            return np.float32(0.00002)
        if cfg.use_les:
            # np.mean(nu_t) of the previous step's nu_t (v5.py:323) as a float64 device mean
            # rounded to the fields' dtype, fetched with max|V| in the step's one host read
            self._dt_red.zero_()
            out = self._dt_red[1:2].view(self.dtype)[0:1]
            call("cfd_absmax2" + self._sfx, ptr(self.u), ptr(self.v), self.u.numel(), ptr(out), stream_handle())
            K.mean64(self.nu_t, out=self._dt_red[0:1])
            red = self._dt_red.cpu().numpy()
            vmax = red[1:2].view(self._np)[0]
            nu_t_mean = self._np(red[0])
        else:
            out = self._scal[0:1]
            out.zero_()
            call("cfd_absmax2" + self._sfx, ptr(self.u), ptr(self.v), self.u.numel(), ptr(out), stream_handle())
            vmax = self._np(out.item())  # the one host read of the step (as in the reference)
            nu_t_mean = self._np(0.0)  # np.mean(nu_t) == 0 in the fields' dtype
        vel_max = max(vmax, 1e-10)
        dt_cfl = cfg.cfl_target * min(cfg.dx, cfg.dy) / vel_max
        nu_total = cfg.nu + nu_t_mean + cfg.artificial_viscosity
        dt_visc = 0.4 * min(cfg.dx, cfg.dy) ** 2 / nu_total
        return np.float32(np.clip(min(dt_cfl, dt_visc), cfg.dt_min, cfg.dt_max))

    def solve_pressure_fast(self, div_u_star):  # v5.py:328-347
        cfg = self.config
        if cfg.use_fast_pressure:  # phi = zeros (v5.py:337) inside the solve
            K.solve_pressure_gauss_seidel_fast(self.phi, div_u_star, cfg.dx, cfg.dy, cfg.dt,
                                               self._mask_u8, cfg.pressure_iterations,
                                               cfg.pressure_tolerance, workspace=self._gs_ws,
                                               iters_done=self._gs_done, phi_tmp=self._phi_tmp,
                                               zero_start=True)
        else:  # phi = zeros (v5.py:337) inside the solve
            K.solve_pressure_jacobi(self.phi, div_u_star, cfg.dx, cfg.dt, self._mask_u8,
                                    cfg.pressure_iterations, phi_tmp=self._phi_tmp, rhs_ws=self._rhs_ws,
                                    zero_start=True)
        return self.phi

    def apply_boundary_conditions(self, u, v):  # v5.py:349-360
        cfg = self.config
        call("cfd_apply_bc2d" + self._sfx, ptr(u), ptr(v), ptr(self._y_dev), cfg.ny, cfg.nx, float(cfg.y_max),
             float(cfg.V_inf), int(self.step), stream_handle())

    def _bc_ibm(self, u, v, force_strength):
        """apply_boundary_conditions followed by apply_ibm_fast (when the
        cylinder mask exists) as one kernel, bit-identical to the two calls.
        A subclass with its own boundary conditions (the lid-driven cavity)
        gets its method, then the IBM call."""
        cfg = self.config
        if type(self).apply_boundary_conditions is not OptimizedTurbulentSolver.apply_boundary_conditions:
            self.apply_boundary_conditions(u, v)
            if self._has_ibm:
                K.apply_ibm_fast(u, v, self.ibm_mask, force_strength)
            return
        call("cfd_apply_bc_ibm2d" + self._sfx, ptr(u), ptr(v), ptr(self._y_dev), cfg.ny, cfg.nx, float(cfg.y_max),
             float(cfg.V_inf), int(self.step), ptr(self.ibm_mask) if self._has_ibm else None, float(force_strength),
             stream_handle())

    def compute_energy(self):  # v5.py:362-363
        return 0.5 * (self.u ** 2 + self.v ** 2)

    def compute_vorticity(self):  # v5.py:365-373
        cfg = self.config
        w = torch.empty_like(self.u)
        if self.dtype == torch.float64:
            call("cfd_vorticity2d_f64", ptr(self.u), ptr(self.v), ptr(self._mask_u8), ptr(w), None, cfg.ny,
                 cfg.nx, float(cfg.dx), float(cfg.dy), stream_handle())
        else:
            call("cfd_vorticity2d_f32", ptr(self.u), ptr(self.v), ptr(self._mask_u8), ptr(w), cfg.ny, cfg.nx,
                 float(cfg.dx), float(cfg.dy), stream_handle())
        return w

    @property
    def energy_history(self):
        """[(step, mean kinetic energy)] like v5.py:433; read lazily from the
        device so time_step() never synchronises for it."""
        n = len(self._energy_steps)
        vals = self._energy[:n].cpu().numpy() if n else np.zeros(0)
        return [(s, float(e)) for s, e in zip(self._energy_steps, vals)]

    @property
    def diagnostics(self):
        """The last step's log values (v5.py:410, 415, 422, 428-432), the same
        numbers the reference prints: max|div u*| before the pressure solve,
        max|grad phi|, max|div u| after the cleaning, nanmax|vorticity| (the
        first four need log_diagnostics=True) and the mean kinetic energy."""
        d = self._scal[1:5].cpu().numpy()
        n = len(self._energy_steps)
        e = float(self._energy[n - 1].item()) if n else float("nan")
        return {"pre_div_max": float(d[0]), "grad_max": float(d[1]), "post_div_max": float(d[2]),
                "vorticity_max": float(d[3]), "energy_mean": e}

    def log_lines(self):
        """The reference's five per-step INFO lines (v5.py:410-435) for the
        last step, formatted as it formats them (log_diagnostics=True)."""
        d, k = self.diagnostics, self.step - 1
        return [f"Step {k}: Pre-pressure divergence = {d['pre_div_max']:.3f}",
                f"Step {k}: Max pressure gradient = {d['grad_max']:.3f}",
                f"Step {k}: Post-pressure divergence = {d['post_div_max']:.3f}",
                f"Step {k}: Max vorticity = {d['vorticity_max']:.3f}",
                f"Step {k}: Mean kinetic energy = {d['energy_mean']:.3f}"]

    def _energy_slot(self):
        k = len(self._energy_steps)
        if k >= self._energy.numel():
            grown = torch.zeros(2 * self._energy.numel(), dtype=torch.float64, device=self.device)
            grown[:k] = self._energy[:k]
            self._energy = grown
        return self._energy[k:k + 1]

    def time_step(self):  # v5.py:375-441
        cfg = self.config
        s = stream_handle()
        diag = cfg.log_diagnostics
        dt = self.adaptive_time_step()
        if diag:
            self._scal[1:5].zero_()
        # predictor (v5.py:378-403): u_old/v_old are read-only here, so u/v are used directly
        if cfg.use_les:
            # nu_t of u_old, v_old (v5.py:381-384) formed inside the predictor, kept in self.nu_t;
            # nu_eff = (nu + nu_t) + art_visc per cell in the fields' dtype (v5.py:388)
            K.predictor_fused_les(self.u, self.v, cfg.dx, cfg.dy, dt, self._np(cfg.nu),
                                  self._np(cfg.artificial_viscosity), cfg.smagorinsky_constant, cfg.use_supg,
                                  u_star=self.u_star, v_star=self.v_star, tau=self.tau_supg, nu_t=self.nu_t,
                                  tau_mode=cfg.supg_tau)
        else:
            # nu_eff = nu + nu_t + art_visc with nu_t == 0 in the fields' dtype (v5.py:388)
            nu_eff = self._np(self._np(cfg.nu) + self._np(0.0)) + self._np(cfg.artificial_viscosity)
            K.predictor_fused(self.u, self.v, cfg.dx, cfg.dy, dt, nu_eff, cfg.use_supg,
                              u_star=self.u_star, v_star=self.v_star, tau=self.tau_supg, tau_mode=cfg.supg_tau)
        # (without SUPG the predictor writes tau_supg's zeros itself)
        force_strength = min(1.0, self.step / cfg.initial_steps)
        # apply_boundary_conditions then apply_ibm_fast (v5.py:405-407), one launch
        self._bc_ibm(self.u_star, self.v_star, force_strength)
        call("cfd_divergence2d" + self._sfx, ptr(self.u_star), ptr(self.v_star), ptr(self.div_u_star), cfg.ny,
             cfg.nx, float(cfg.dx), float(cfg.dy), ptr(self._scal[1:2]) if diag else None, s)
        self.solve_pressure_fast(self.div_u_star)
        K.project_velocity(self.phi, self.u_star, self.v_star, cfg.dx, cfg.dy, dt, u=self.u, v=self.v,
                           gradmax=self._scal[2:3] if diag else None)
        K.clean_divergence_fast(self.u, self.v, cfg.dx, cfg.dy, iterations=2, workspace=self._clean_ws)
        if diag:
            call("cfd_divergence2d" + self._sfx, ptr(self.u), ptr(self.v), ptr(self.div_u_star), cfg.ny, cfg.nx,
                 float(cfg.dx), float(cfg.dy), ptr(self._scal[3:4]), s)
            # the reference recomputes div for logging only; keep div_u_star as the pre-pressure one
            call("cfd_divergence2d" + self._sfx, ptr(self.u_star), ptr(self.v_star), ptr(self.div_u_star),
                 cfg.ny, cfg.nx, float(cfg.dx), float(cfg.dy), None, s)
        self._bc_ibm(self.u, self.v, force_strength)  # v5.py:424-425
        if diag and self.dtype == torch.float64:
            call("cfd_vorticity2d_f64", ptr(self.u), ptr(self.v), ptr(self._mask_u8), None, ptr(self._scal[4:5]),
                 cfg.ny, cfg.nx, float(cfg.dx), float(cfg.dy), s)
        elif diag:
            call("cfd_vorticity_absmax2d_f32", ptr(self.u), ptr(self.v), ptr(self._mask_u8), cfg.ny,
                 cfg.nx, float(cfg.dx), float(cfg.dy), ptr(self._scal[4:5]), s)
        # the energy of the unclipped fields (v5.py:431-435), then both clips (v5.py:437-438)
        call("cfd_energy_mean_clip2d" + self._sfx, ptr(self.u), ptr(self.v), self.u.numel(),
             ptr(self._energy_slot()), -float(cfg.max_velocity), float(cfg.max_velocity), s)
        self._energy_steps.append(self.step)
        self.times.append(self.step * dt)
        self.step += 1
        return dt

    # ------------------------------------------------------------ output
    def save_snapshot(self, path, step: int, current_time: float):
        """save_data_to_hdf5 layout (v5.py:454-470) as .npz (h5py is absent):
        group step_%06d with u, v, vorticity, X, Y and the time attribute.
        Like the reference's file (opened in append mode, a group written
        once, v5.py:457-458), an existing snapshot file keeps its groups and
        gains this one: the new group's arrays are appended as members of the
        .npz zip archive, so a save costs O(one group) however many the file
        holds, and a group already present is left alone without reading the
        device.  phi and the step counter are added (the reference stores
        neither) so that load_snapshot restarts the run exactly; with LES so
        is nu_t (the next adaptive dt reads the previous step's mean nu_t)."""
        g = f"step_{step:06d}"
        if _npz_has_group(path, g):  # `if group_name not in f` (v5.py:458)
            return
        groups = {f"{g}/u": self.u.cpu().numpy(), f"{g}/v": self.v.cpu().numpy(),
                  f"{g}/vorticity": self.compute_vorticity().cpu().numpy(),
                  f"{g}/X": self.X, f"{g}/Y": self.Y, f"{g}/phi": self.phi.cpu().numpy(),
                  f"{g}/time": np.float64(current_time), f"{g}/solver_step": np.int64(self.step)}
        if self.config.use_les:
            groups[f"{g}/nu_t"] = self.nu_t.cpu().numpy()
        _npz_append(path, groups)

    def load_snapshot(self, path, step=None):
        """Restart from a save_snapshot file: group step_%06d (the latest
        when ``step`` is None) gives u, v, phi and the step counter; returns
        the stored time.  The next time_step() then equals the uninterrupted
        run's bit for bit: a step reads only u, v and the counter (phi is
        zero-filled before each solve, v5.py:331/337)."""
        with np.load(path, allow_pickle=False) as f:
            g = _npz_pick_group(path, f, step)
            shape = (self.config.ny, self.config.nx)
            if f[f"{g}/u"].shape != shape:
                raise ValueError(f"{path}: {g} holds a {f[f'{g}/u'].shape} grid, the solver {shape}")
            self.u.copy_(torch.from_numpy(f[f"{g}/u"]))
            self.v.copy_(torch.from_numpy(f[f"{g}/v"]))
            self.phi.copy_(torch.from_numpy(f[f"{g}/phi"]))
            if self.config.use_les and f"{g}/nu_t" in f.files:
                self.nu_t.copy_(torch.from_numpy(f[f"{g}/nu_t"]))
            self.step = int(f[f"{g}/solver_step"]) if f"{g}/solver_step" in f.files else int(g[5:])
            return float(f[f"{g}/time"])


# ------------------------------------------------------ lid-driven cavity
@dataclass
class LidDrivenCavityConfig(OptimizedTurbulentConfig):
    """BASELINE.json config 1: the 2-D lid-driven cavity, 128 x 128, Re = 100,
    500 Jacobi iterations per pressure solve.  The reference has no
    incompressible cavity (its SWA cavity is compressible Euler,
    SWA/cavity_flow_v1.py:39-69), so this is the v5 projection step
    (v5.py:375-441, every kernel and quirk unchanged) on the unit square with
    cavity walls instead of the cylinder channel's inlet / outlet / IBM:
    nu = 1/Re = 0.01, artificial viscosity 1e-3, the
    NumPy Jacobi branch (use_fast_pressure=False), fluid at rest initially."""
    x_max: float = 1.0
    y_max: float = 1.0
    nx: int = 128
    ny: int = 128
    Re: float = 100.0
    artificial_viscosity: float = 0.001
    pressure_iterations: int = 500
    use_fast_pressure: bool = False
    lid_velocity: float = 1.0
    output_dir: str = "cavity_re_100"
    hdf5_file: str = "cavity_re_100.h5"


def host_lid_bc(u, v, u_lid):
    """The cavity walls on host arrays (what cfd_apply_lid_bc2d_f32 does):
    no-slip left / right / bottom, the lid u = u_lid on the top row, written
    last so it owns the top corners (the assignment pattern of v5.py:349-360)."""
    u[:, 0] = 0
    v[:, 0] = 0
    u[:, -1] = 0
    v[:, -1] = 0
    u[0, :] = 0
    v[0, :] = 0
    u[-1, :] = np.float32(u_lid)
    v[-1, :] = 0


class LidDrivenCavitySolver(OptimizedTurbulentSolver):
    """The v5 time step (OptimizedTurbulentSolver.time_step) on the lid-driven
    cavity: no solid cells (no mask, no IBM forcing), cavity walls as the
    boundary conditions, zero initial velocity."""

    def __init__(self, config: LidDrivenCavityConfig):
        super().__init__(config)
        self._has_ibm = False

    def setup_boundary_masks(self):
        cfg = self.config
        self.dist = None
        self.cylinder_mask_host = np.zeros((cfg.ny, cfg.nx), bool)
        self.ibm_mask_host = np.zeros((cfg.ny, cfg.nx), np.float64)
        self.cylinder_mask = torch.from_numpy(self.cylinder_mask_host).to(self.device)
        self._mask_u8 = None  # no solid cells: the sweeps skip the mask read
        self.ibm_mask = torch.from_numpy(self.ibm_mask_host).to(self.device)

    def initialize_potential_flow(self):
        self.u.zero_()
        self.v.zero_()

    def apply_boundary_conditions(self, u, v):
        call("cfd_apply_lid_bc2d" + self._sfx, ptr(u), ptr(v), self.config.ny, self.config.nx,
             float(self._np(self.config.lid_velocity)), stream_handle())


# --------------------------------------------------- 3-D lid-driven cavity
@dataclass
class LidDrivenCavity3DConfig(OptimizedTurbulentConfig):
    """The lid-driven cavity in 3-D: the v5 fields plus nz, z_min, z_max and
    the derived dz.  128^3 on the unit cube, Re = 100, artificial viscosity
    1e-3, 200 Jacobi iterations per pressure solve (use_fast_pressure=False;
    True selects the 3-D red-black GS), the lid y = y_max moving at
    lid_velocity in x."""
    x_max: float = 1.0
    y_max: float = 1.0
    z_min: float = 0.0
    z_max: float = 1.0
    nx: int = 128
    ny: int = 128
    nz: int = 128
    Re: float = 100.0
    artificial_viscosity: float = 0.001
    pressure_iterations: int = 200
    use_fast_pressure: bool = False
    lid_velocity: float = 1.0
    output_dir: str = "cavity3d_re_100"
    hdf5_file: str = "cavity3d_re_100.h5"
    _accepts_les = False  # LesCavity3DConfig: True

    def __post_init__(self):
        super().__post_init__()
        self.dz = (self.z_max - self.z_min) / (self.nz - 1)
        if self.use_les and not self._accepts_les:
            raise ValueError("LidDrivenCavity3DConfig: LES is 2-D only (3-D LES: LesCavity3DConfig)")
        if not self.memory_efficient:
            raise ValueError("LidDrivenCavity3DConfig: the 3-D step is float32 only (memory_efficient=True)")


@dataclass
class LesCavity3DConfig(LidDrivenCavity3DConfig):
    """LidDrivenCavity3DConfig with LES: the Smagorinsky eddy viscosity in its
    3-D form (K.compute_smagorinsky_viscosity3d; the project's own statement,
    tests/les3d_reference.py -- the reference is 2-D and ships with LES off)
    formed inside the predictor, nu_eff = (nu + nu_t) + artificial_viscosity
    per cell.  use_les=False behaves exactly like the base config."""
    use_les: bool = True
    smagorinsky_constant: float = 0.17
    _accepts_les = True


STATS_MOMENTS = ("u", "v", "w", "uu", "vv", "ww", "uv", "uw", "vw", "nu_t")
STATS_SCALAR_MOMENTS = ("T", "TT", "uT", "vT", "wT")  # behind the 9 or 10 above with scalar_moments


def derive_statistics(sums, weight, nz, span_average, scalar=False):
    """The averages of the float64 moment sums (STATS_MOMENTS' order; 9 or 10
    planes): every sum over weight * nz (span_average) or weight, the Reynolds
    stresses <ab> - <a><b>, tke = ((uu + vv) + ww) / 2.  ``scalar``: the sums
    end with STATS_SCALAR_MOMENTS' five planes (14 or 15 in all) and the
    result gains mean_T, the variance TT = <TT> - <T>^2 and the turbulent heat
    fluxes uT, vT, wT = <aT> - <a><T>."""
    sums = np.asarray(sums, np.float64)
    if sums.shape[0] not in ((14, 15) if scalar else (9, 10)):
        raise ValueError(f"derive_statistics: {sums.shape[0]} moment planes with scalar={bool(scalar)}")
    if scalar:
        out = derive_statistics(sums[:-5], weight, nz, span_average)
        norm = np.float64(weight) * np.float64(nz) if span_average else np.float64(weight)
        t = sums[-5:] / norm
        out["mean_T"] = t[0]
        out["TT"] = t[1] - t[0] * t[0]
        for q, name in enumerate(("uT", "vT", "wT")):
            out[name] = t[2 + q] - out["mean_" + name[0]] * t[0]
        return out
    norm = np.float64(weight) * np.float64(nz) if span_average else np.float64(weight)
    m = np.asarray(sums, np.float64) / norm
    out = {"weight": float(weight), "mean_u": m[0], "mean_v": m[1], "mean_w": m[2]}
    for q, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[STATS_MOMENTS[3 + q]] = m[3 + q] - m[a] * m[b]
    out["tke"] = 0.5 * ((out["uu"] + out["vv"]) + out["ww"])
    if m.shape[0] == 10:
        out["mean_nu_t"] = m[9]
    return out


class LidDrivenCavity3DSolver:
    """The projection step around the 3-D pressure solves on one GPU: the
    project's own 3-D generalisation of the v5 time step (every 2-D
    coefficient kept, a z term appended; tests/ref3d.py states the arithmetic)
    on the lid-driven cavity, fields (nz, ny, nx) float32 device tensors.

    time_step: dt, fused predictor (K.predictor3d_fused, tau not stored), lid
    walls, divergence, pressure solve (phi from zeros: cfd_jacobi3d_zero_f32,
    or cfd_rbgs3d_f32 with use_fast_pressure), projection, lid walls, mean
    kinetic energy and the three clips.  No host synchronisation, except the
    adaptive dt's one read of max|V| from step 1000 on.

    LES (a LesCavity3DConfig with use_les=True): the predictor is
    K.predictor3d_fused_les, which forms the Smagorinsky nu_t of the step's
    u, v, w per cell and keeps it in ``nu_t``; from step 1000 on the adaptive
    dt reads the float64 mean of the previous step's nu_t together with
    max|V| in the same single host read.

    Statistics (``enable_statistics``): float64 running sums of u, v, w, uu,
    vv, ww, uv, uw, vw (and nu_t with LES) of the step's final, clipped
    fields, one K.accumulate_flow_stats3d launch per sampled step, per cell or
    summed over z; ``statistics()`` derives the means, the Reynolds stresses
    and the turbulent kinetic energy.  A solver that carries the passive
    scalar can add T, TT, uT, vT, wT (``scalar_moments=True``).  With
    statistics off time_step launches what it launched without them.

    Snapshots: ``save_snapshot`` / ``load_snapshot`` keep the 2-D solver's
    .npz layout (groups step_%06d, appended) with u, v, w, phi, |omega|, the
    axes, nu_t with LES and the statistics' sums and settings; after a load
    every later step, field and statistics sum equals the uninterrupted run's
    bit for bit.

    Out of scope: immersed boundaries or masks (those:
    CylinderChannel3DSolver), float64, a
    slab-decomposed (multi-GPU) step, and the 2-D step's clean_divergence
    stage (a v5 quirk with serial semantics that does not generalise)."""

    _periodic_z = False  # CylinderChannel3DSolver with spanwise_bc="periodic": the *_zper stages
    _stats_span_default = False  # enable_statistics(span_average=None); the cylinder channel: True
    _stats = None  # (start_step, interval, span_average, weight) once statistics are enabled
    _stats_scalar = False  # enable_statistics(scalar_moments=True): T, TT, uT, vT, wT behind the flow moments

    def __init__(self, config: LidDrivenCavity3DConfig):
        self.config = cfg = config
        self.dtype = torch.float32
        self.device = torch.device(cfg.device)
        if self.device.type != "cuda":
            raise TypeError("LidDrivenCavity3DSolver runs on the HIP device only")
        shape = (cfg.nz, cfg.ny, cfg.nx)
        z = lambda: torch.zeros(shape, dtype=self.dtype, device=self.device)  # noqa: E731
        self.u, self.v, self.w = z(), z(), z()  # fluid at rest
        self.u_star, self.v_star, self.w_star = z(), z(), z()
        self.div_u_star, self.phi = z(), z()
        self._phi_tmp, self._rhs_ws = z(), z()
        self._gs_ws = torch.empty(int(lib().cfd_rbgs_workspace_bytes(cfg.pressure_iterations)), dtype=torch.uint8,
                                  device=self.device)
        self._gs_done = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._scal = torch.zeros(4, dtype=self.dtype, device=self.device)  # [max|V|, pre_div_max, grad_max]
        self._energy = torch.zeros(1024, dtype=torch.float64, device=self.device)
        self._energy_steps = []
        self.times = []
        self.step = 0
        self.use_les = bool(cfg.use_les)
        if self.use_les:
            self.nu_t = z()
            # LES adaptive dt: [mean nu_t (float64), max|V| (float32, first bytes)]: one host read
            self._dt_red = torch.zeros(2, dtype=torch.float64, device=self.device)

    def adaptive_time_step(self):
        """The v5 rule (v5.py:316-326) with max(|u|, |v|, |w|) and min(dx, dy, dz);
        with LES, np.mean(nu_t) of the previous step's nu_t as a float64 device
        mean rounded to float32, fetched with max|V| in the one host read."""
        cfg = self.config
        if not cfg.adaptive_dt:
            return cfg.dt_base
        if self.step < 1000:
            return np.float32(0.00002)
        s = stream_handle()
        n = self.u.numel()
        if self.use_les:
            self._dt_red.zero_()
            out = self._dt_red[1:2].view(self.dtype)[0:1]
        else:
            out = self._scal[0:1]
            out.zero_()
        call("cfd_absmax2_f32", ptr(self.u), ptr(self.v), n, ptr(out), s)
        call("cfd_absmax_f32", ptr(self.w), n, ptr(out), s)  # the max accumulates
        if self.use_les:
            K.mean64(self.nu_t, out=self._dt_red[0:1])
            red = self._dt_red.cpu().numpy()  # the one host read of the step
            vmax = red[1:2].view(np.float32)[0]
            nu_t_mean = np.float32(red[0])
        else:
            vmax = np.float32(out.item())  # the one host read of the step
            nu_t_mean = np.float32(0.0)
        vel_max = max(vmax, 1e-10)
        h = min(cfg.dx, cfg.dy, cfg.dz)
        dt_cfl = cfg.cfl_target * h / vel_max
        nu_total = cfg.nu + nu_t_mean + cfg.artificial_viscosity
        dt_visc = 0.4 * h ** 2 / nu_total
        return np.float32(np.clip(min(dt_cfl, dt_visc), cfg.dt_min, cfg.dt_max))

    def solve_pressure_fast(self, div_u_star):
        """phi = zeros, then the solve (with cfg.dt, like v5.py:328-347):
        red-black GS on any spacing (use_fast_pressure), else the 7-point
        Jacobi, which needs dx == dy == dz exactly."""
        cfg = self.config
        if cfg.use_fast_pressure:
            self.phi.zero_()
            K.solve_pressure_gauss_seidel3d(self.phi, div_u_star, cfg.dx, cfg.dy, cfg.dz, cfg.dt, None,
                                            cfg.pressure_iterations, cfg.pressure_tolerance, workspace=self._gs_ws,
                                            iters_done=self._gs_done, phi_tmp=self._phi_tmp)
        else:
            if not (cfg.dx == cfg.dy == cfg.dz):
                raise ValueError(f"the 3-D Jacobi solve needs dx == dy == dz (got {cfg.dx}, {cfg.dy}, {cfg.dz}); "
                                 "use_fast_pressure=True takes any spacing")
            K.solve_pressure_jacobi3d_zero(self.phi, div_u_star, cfg.dx, cfg.dt, cfg.pressure_iterations,
                                           phi_tmp=self._phi_tmp, rhs_ws=self._rhs_ws)
        return self.phi

    def apply_boundary_conditions(self, u, v, w):
        K.apply_lid_bc3d(u, v, w, self.config.lid_velocity)

    def _after_predictor(self, dt):
        """Stages that read the step's incoming u, v, w (and nu_t) before the
        projection overwrites them: none here (the cylinder channel's scalar)."""

    def _predictor_buoyancy(self):
        """Further keyword arguments of the step's predictor call: none here
        (the cylinder channel's buoyancy: T, buoyancy, t_ref)."""
        return {}

    @property
    def energy_history(self):
        """[(step, mean kinetic energy)], read lazily from the device."""
        n = len(self._energy_steps)
        vals = self._energy[:n].cpu().numpy() if n else np.zeros(0)
        return [(s, float(e)) for s, e in zip(self._energy_steps, vals)]

    @property
    def diagnostics(self):
        """The last step's max|div u*| before the pressure solve and
        max|grad phi| (both need log_diagnostics=True) and the mean kinetic
        energy."""
        d = self._scal[1:3].cpu().numpy()
        n = len(self._energy_steps)
        e = float(self._energy[n - 1].item()) if n else float("nan")
        return {"pre_div_max": float(d[0]), "grad_max": float(d[1]), "energy_mean": e}

    def _energy_slot(self):
        k = len(self._energy_steps)
        if k >= self._energy.numel():
            grown = torch.zeros(2 * self._energy.numel(), dtype=torch.float64, device=self.device)
            grown[:k] = self._energy[:k]
            self._energy = grown
        return self._energy[k:k + 1]

    def time_step(self):
        cfg = self.config
        sp = (cfg.dx, cfg.dy, cfg.dz)
        diag = cfg.log_diagnostics
        dt = self.adaptive_time_step()
        if diag:
            self._scal[1:3].zero_()
        if self.use_les:
            # nu_t of u, v, w formed inside the predictor and kept in self.nu_t;
            # nu_eff = (nu + nu_t) + art_visc per cell in float32
            K.predictor3d_fused_les(self.u, self.v, self.w, *sp, dt, cfg.nu, cfg.artificial_viscosity,
                                    cfg.smagorinsky_constant, cfg.use_supg, u_star=self.u_star,
                                    v_star=self.v_star, w_star=self.w_star, nu_t=self.nu_t, store_tau=False,
                                    periodic_z=self._periodic_z, **self._predictor_buoyancy())
        else:
            # nu_eff = (nu + 0) + art_visc in float32, a scalar
            nu_eff = np.float32(np.float32(cfg.nu) + np.float32(0.0)) + np.float32(cfg.artificial_viscosity)
            K.predictor3d_fused(self.u, self.v, self.w, *sp, dt, nu_eff, cfg.use_supg, u_star=self.u_star,
                                v_star=self.v_star, w_star=self.w_star, store_tau=False,
                                periodic_z=self._periodic_z, **self._predictor_buoyancy())
        self._after_predictor(dt)
        self.apply_boundary_conditions(self.u_star, self.v_star, self.w_star)
        K.compute_divergence3d(self.u_star, self.v_star, self.w_star, *sp, out=self.div_u_star,
                               absmax=self._scal[1:2] if diag else None, periodic_z=self._periodic_z)
        self.solve_pressure_fast(self.div_u_star)
        K.project_velocity3d(self.phi, self.u_star, self.v_star, self.w_star, *sp, dt, u=self.u, v=self.v, w=self.w,
                             gradmax=self._scal[2:3] if diag else None, periodic_z=self._periodic_z)
        self.apply_boundary_conditions(self.u, self.v, self.w)
        # the energy of the unclipped fields, then the three clips, one launch
        call("cfd_energy_mean_clip3d_f32", ptr(self.u), ptr(self.v), ptr(self.w), self.u.numel(),
             ptr(self._energy_slot()), -float(cfg.max_velocity), float(cfg.max_velocity), stream_handle())
        self._energy_steps.append(self.step)
        self.times.append(self.step * dt)
        if self._stats is not None:
            self._sample_statistics(dt)
        self.step += 1
        return dt

    # -------------------------------------------------------- statistics
    def enable_statistics(self, start_step=0, interval=1, span_average=None, weight="dt", scalar_moments=False):
        """Accumulate the flow moments of the clipped u, v, w (with LES also
        nu_t) at the end of every step k >= start_step with (k - start_step) %
        interval == 0, into zeroed float64 sums on the device.
        ``span_average`` (None: True for the cylinder channel, False for the
        cavity): sum over z into (ny, nx) planes instead of keeping
        (nz, ny, nx).  ``weight``: "dt" weights a sample by its step's dt
        (the dt is adaptive from step 1000 on, so equal weights would bias a
        time average), "sample" by 1.0.  ``scalar_moments`` (a solver that
        carries the passive scalar T, else ValueError): the sums gain T, TT,
        uT, vT, wT of the step's final T as five further planes, in the same
        single launch (K.accumulate_flow_scalar_stats3d).  Calling it again
        with the same settings does nothing; other settings raise ValueError
        unless reset_statistics() came first."""
        if span_average is None:
            span_average = self._stats_span_default
        if weight not in ("dt", "sample"):
            raise ValueError(f"enable_statistics: weight must be 'dt' or 'sample', not {weight!r}")
        if int(start_step) < 0 or int(interval) < 1:
            raise ValueError(f"enable_statistics: start_step >= 0 and interval >= 1 (got {start_step}, {interval})")
        scalar_moments = bool(scalar_moments)
        if scalar_moments and not getattr(self, "scalar", False):
            raise ValueError("enable_statistics: scalar_moments needs a solver that carries the passive scalar "
                             "(CylinderChannel3DConfig(scalar=True))")
        settings = (int(start_step), int(interval), bool(span_average), weight)
        if self._stats is not None:
            if settings == self._stats and scalar_moments == self._stats_scalar:
                return
            if not self._stats_reset:
                raise ValueError(f"enable_statistics: statistics are on with {self._stats}, scalar_moments="
                                 f"{self._stats_scalar}, asked for {settings}, scalar_moments={scalar_moments}; "
                                 "call reset_statistics() first")
        cfg = self.config
        nm = (10 if self.use_les else 9) + (5 if scalar_moments else 0)
        shape = (nm, cfg.ny, cfg.nx) if settings[2] else (nm, cfg.nz, cfg.ny, cfg.nx)
        self._stats = settings
        self._stats_scalar = scalar_moments
        self._stats_sums = torch.zeros(shape, dtype=torch.float64, device=self.device)
        self._stats_weight = np.float64(0.0)
        self._stats_samples = 0
        self._stats_reset = False

    def reset_statistics(self):
        """Zero the sums, the total weight and the sample count; the settings
        stay."""
        if self._stats is None:
            raise RuntimeError("reset_statistics: statistics are not enabled")
        self._stats_sums.zero_()
        self._stats_weight = np.float64(0.0)
        self._stats_samples = 0
        self._stats_reset = True

    def _sample_statistics(self, dt):
        start, interval, span, mode = self._stats
        k = self.step
        if k < start or (k - start) % interval:
            return
        wgt = float(dt) if mode == "dt" else 1.0
        nu_t = self.nu_t if self.use_les else None
        if self._stats_scalar:  # the step's final T: after the advance, the heating and the faces
            K.accumulate_flow_scalar_stats3d(self.u, self.v, self.w, self.T, self._stats_sums, wgt, span, nu_t=nu_t)
        else:
            K.accumulate_flow_stats3d(self.u, self.v, self.w, self._stats_sums, wgt, span, nu_t=nu_t)
        self._stats_weight = self._stats_weight + np.float64(wgt)
        self._stats_samples += 1
        self._stats_reset = False

    def statistics(self):
        """The averages so far, float64 NumPy arrays from one device read:
        ``samples``, ``weight`` (the total), ``mean_u``, ``mean_v``,
        ``mean_w``, the Reynolds stresses ``uu``, ``vv``, ``ww``, ``uv``,
        ``uw``, ``vw`` as <ab> - <a><b>, ``tke`` = (uu + vv + ww) / 2 and,
        with LES, ``mean_nu_t``; with scalar_moments also ``mean_T``, the
        variance ``TT`` and the turbulent heat fluxes ``uT``, ``vT``, ``wT``.
        Shapes: (ny, nx) with span_average (the sums over weight * nz), else
        (nz, ny, nx) (over weight).  RuntimeError before the first sample."""
        if self._stats is None or self._stats_samples == 0:
            raise RuntimeError("statistics(): no sample yet (enable_statistics, then time_step)")
        sums = self._stats_sums.cpu().numpy()  # the one device read
        out = derive_statistics(sums, self._stats_weight, self.config.nz, self._stats[2], scalar=self._stats_scalar)
        out["samples"] = self._stats_samples
        return out

    # ----------------------------------------------------------- output
    def compute_vorticity(self):
        """|omega| of the current fields, 0 on the six faces."""
        cfg = self.config
        return K.compute_vorticity3d(self.u, self.v, self.w, cfg.dx, cfg.dy, cfg.dz)

    def save_snapshot(self, path, step: int, current_time: float):
        """The 2-D solver's snapshot file in 3-D: group step_%06d of the .npz
        archive with u, v, w, phi, vorticity (|omega| from compute_vorticity),
        the axes x, y, z, time, solver_step, nu_t with LES and, when
        statistics are enabled, stats_sums, stats_weight, stats_samples and
        the four settings (stats_start_step, stats_interval,
        stats_span_average, stats_weight_mode), and with scalar_moments
        stats_scalar_moments (stats_sums then has 14 or 15 planes; a group
        without that member was written without them).  An existing file
        keeps its groups and gains this one as appended zip members; a group
        already present is left alone without reading the device."""
        g = f"step_{step:06d}"
        if _npz_has_group(path, g):
            return
        cfg = self.config
        z = getattr(self, "z", None)
        host = lambda t: t.cpu().numpy()  # noqa: E731
        groups = {f"{g}/u": host(self.u), f"{g}/v": host(self.v), f"{g}/w": host(self.w),
                  f"{g}/phi": host(self.phi), f"{g}/vorticity": host(self.compute_vorticity()),
                  f"{g}/x": np.linspace(cfg.x_min, cfg.x_max, cfg.nx),
                  f"{g}/y": np.linspace(cfg.y_min, cfg.y_max, cfg.ny),
                  f"{g}/z": np.linspace(cfg.z_min, cfg.z_max, cfg.nz) if z is None else z,
                  f"{g}/time": np.float64(current_time), f"{g}/solver_step": np.int64(self.step)}
        if self.use_les:
            groups[f"{g}/nu_t"] = host(self.nu_t)
        if self._stats is not None:
            start, interval, span, mode = self._stats
            groups.update({f"{g}/stats_sums": host(self._stats_sums),
                           f"{g}/stats_weight": np.float64(self._stats_weight),
                           f"{g}/stats_samples": np.int64(self._stats_samples),
                           f"{g}/stats_start_step": np.int64(start), f"{g}/stats_interval": np.int64(interval),
                           f"{g}/stats_span_average": np.bool_(span), f"{g}/stats_weight_mode": np.array(mode)})
            if self._stats_scalar:
                groups[f"{g}/stats_scalar_moments"] = np.bool_(True)
        groups.update({f"{g}/{name}": host(t) for name, t in self._snapshot_fields().items()})
        _npz_append(path, groups)

    def _snapshot_fields(self):
        """Further device fields of a snapshot group, {name: tensor}, restored
        by load_snapshot when the group holds them (the cylinder channel: T)."""
        return {}

    def load_snapshot(self, path, step=None):
        """Restart from a save_snapshot file: group step_%06d (the latest
        when ``step`` is None) gives u, v, w, phi, nu_t (LES), the step counter
        and, if the group holds them, the statistics: they are enabled with
        the stored settings (scalar_moments among them) if they are off, and a
        solver whose statistics are on with other settings raises ValueError,
        as does a file of another grid shape or moment count.  Returns the
        stored time.  The histories (energy, forces) start empty, on a solver
        that has already stepped too.  Two cases are accepted and fall outside the guarantee below: a group without nu_t
        (written with LES off) leaves an LES solver's nu_t as it is, which
        the adaptive dt reads from step 1000 on; a group without statistics
        (written with them off) leaves the solver's running sums, weight and
        count as they are, so averaging can start from a spin-up file.
        Otherwise every later time_step(), field and statistics sum then
        equals the uninterrupted run's bit for bit: a step reads only u, v, w,
        the counter and, with LES from step 1000 on, the mean of nu_t, and the
        statistics kernel's sums have a fixed order."""
        cfg = self.config
        with np.load(path, allow_pickle=False) as f:
            g = _npz_pick_group(path, f, step)
            shape = (cfg.nz, cfg.ny, cfg.nx)
            if f[f"{g}/u"].shape != shape:
                raise ValueError(f"{path}: {g} holds a {f[f'{g}/u'].shape} grid, the solver {shape}")
            has_stats = f"{g}/stats_sums" in f.files
            if has_stats:
                settings = (int(f[f"{g}/stats_start_step"]), int(f[f"{g}/stats_interval"]),
                            bool(f[f"{g}/stats_span_average"]), str(f[f"{g}/stats_weight_mode"]))
                key = f"{g}/stats_scalar_moments"
                scalar_moments = bool(f[key]) if key in f.files else False
                if self._stats is not None and (self._stats != settings or self._stats_scalar != scalar_moments):
                    raise ValueError(f"{path}: {g} holds statistics with {settings}, scalar_moments="
                                     f"{scalar_moments}, the solver's are on with {self._stats}, scalar_moments="
                                     f"{self._stats_scalar}")
                if scalar_moments and not getattr(self, "scalar", False):
                    raise ValueError(f"{path}: {g} holds statistics with scalar moments, the solver carries no "
                                     "scalar")
                sums = f[f"{g}/stats_sums"]
                nm = (10 if self.use_les else 9) + (5 if scalar_moments else 0)
                want = (nm, cfg.ny, cfg.nx) if settings[2] else (nm, *shape)
                if sums.shape != want:
                    raise ValueError(f"{path}: {g} holds {sums.shape} statistics sums, the solver {want}")
            for name in ("u", "v", "w", "phi"):  # phi may be a view of the padded array: copy into it
                getattr(self, name).copy_(torch.from_numpy(f[f"{g}/{name}"]))
            if self.use_les and f"{g}/nu_t" in f.files:
                self.nu_t.copy_(torch.from_numpy(f[f"{g}/nu_t"]))
            for name, t in self._snapshot_fields().items():
                if f"{g}/{name}" in f.files:
                    t.copy_(torch.from_numpy(f[f"{g}/{name}"]))
            if has_stats:
                if self._stats is None:
                    self.enable_statistics(*settings, scalar_moments=scalar_moments)
                self._stats_sums.copy_(torch.from_numpy(sums))
                self._stats_weight = np.float64(f[f"{g}/stats_weight"])
                self._stats_samples = int(f[f"{g}/stats_samples"])
                self._stats_reset = False
            self.step = int(f[f"{g}/solver_step"])
            self._restart_histories()
            return float(f[f"{g}/time"])

    def _restart_histories(self):
        self._energy_steps = []
        self.times = []


# ------------------------------------------------- 3-D cylinder channel
@dataclass
class CylinderChannel3DConfig(OptimizedTurbulentConfig):
    """The v5 cylinder channel extruded along z: every v5 default kept (the
    20 x 4 domain, the cylinder R = 0.5 at (4, 2), Re = 600, 600 x 180 cells,
    red-black GS) plus nz, z_min, z_max and the derived dz; the cylinder's
    axis is along z.  200 iterations per pressure solve, as in the 3-D cavity.
    use_les=True forms the 3-D Smagorinsky eddy viscosity (constant 0.17)
    inside the predictor; False (the default) ignores the constant.  float32
    only.

    spanwise_bc: "free_slip" (the default: planes 0 and nz-1 are free-slip
    walls, dz = (z_max - z_min) / (nz - 1)) or "periodic" (all nz planes are
    interior in z and plane nz-1's neighbour is plane 0; dz = (z_max - z_min)
    / nz, nz even and >= 4, red-black GS only).  spanwise_perturbation = a:
    the initial u of plane k is scaled by 1 + a cos(2 pi (z_k - z_min) / (z_max
    - z_min)), the one thing that makes the flow depend on z; 0.0 (the
    default) is the z-invariant start."""
    z_min: float = 0.0
    z_max: float = 4.0
    nz: int = 120
    pressure_iterations: int = 200
    smagorinsky_constant: float = 0.17
    output_dir: str = "cylinder3d_re_600"
    hdf5_file: str = "cylinder3d_re_600.h5"
    spanwise_bc: str = "free_slip"
    spanwise_perturbation: float = 0.0
    # passive scalar (temperature): off by default.  Diffusivity nu / prandtl
    # (artificial_viscosity is not added), with LES plus nu_t /
    # turbulent_prandtl per cell; T = scalar_inlet at the inlet and at the
    # start, the cylinder's forcing zone relaxes T towards scalar_cylinder
    scalar: bool = False
    prandtl: float = 0.71
    turbulent_prandtl: float = 0.85
    scalar_inlet: float = 0.0
    scalar_cylinder: float = 1.0
    # Boussinesq buoyancy (needs the scalar): off at richardson = 0.  Ri =
    # g beta dT D / V_inf^2 with dT = scalar_cylinder - scalar_inlet and D =
    # 2 R_cylinder; gravity_direction is g's direction in (x, y, z), any
    # non-zero length; T - scalar_reference (None: scalar_inlet) drives the
    # term, and hot fluid is pushed against g
    richardson: float = 0.0
    gravity_direction: tuple = (0.0, -1.0, 0.0)
    scalar_reference: float | None = None

    def __post_init__(self):
        super().__post_init__()
        if self.richardson != 0:
            if not self.scalar:
                raise ValueError("CylinderChannel3DConfig: richardson != 0 needs the scalar (scalar=True)")
            if self.scalar_cylinder == self.scalar_inlet:
                raise ValueError("CylinderChannel3DConfig: richardson != 0 needs scalar_cylinder != scalar_inlet "
                                 "(the temperature scale of the Richardson number)")
            try:
                g = [float(x) for x in self.gravity_direction]
            except (TypeError, ValueError):
                g = []
            if len(g) != 3 or not all(np.isfinite(g)) or not any(x != 0.0 for x in g):
                raise ValueError(f"CylinderChannel3DConfig: gravity_direction must be three finite numbers of "
                                 f"non-zero norm (got {self.gravity_direction!r})")
        if not (self.prandtl > 0.0 and self.turbulent_prandtl > 0.0):
            raise ValueError(f"CylinderChannel3DConfig: prandtl and turbulent_prandtl must be positive "
                             f"(got {self.prandtl}, {self.turbulent_prandtl})")
        if self.spanwise_bc not in ("free_slip", "periodic"):
            raise ValueError(f"CylinderChannel3DConfig: spanwise_bc must be 'free_slip' or 'periodic', "
                             f"not {self.spanwise_bc!r}")
        if self.spanwise_bc == "periodic":
            if self.nz < 4 or self.nz % 2:
                raise ValueError(f"CylinderChannel3DConfig: periodic spanwise boundaries need an even nz >= 4 "
                                 f"(got {self.nz}): the two planes of a wrap must have opposite red-black parity")
            if not self.use_fast_pressure:
                raise ValueError("CylinderChannel3DConfig: periodic spanwise boundaries need the red-black GS "
                                 "(use_fast_pressure=True): the blocked and masked Jacobi has no periodic form")
            self.dz = (self.z_max - self.z_min) / self.nz
        else:
            self.dz = (self.z_max - self.z_min) / (self.nz - 1)
        if not self.memory_efficient:
            raise ValueError("CylinderChannel3DConfig: the 3-D step is float32 only (memory_efficient=True)")


def host_ibm_bbox(ibm):
    """(i0, i1, j0, j1): the tight half-open box of rows and columns of the
    2-D mask ``ibm`` that holds every ibm > 0; the whole grid if there is none."""
    pos = np.asarray(ibm) > 0
    ny, nx = pos.shape
    rows, cols = np.flatnonzero(pos.any(axis=1)), np.flatnonzero(pos.any(axis=0))
    if rows.size == 0:
        return 0, ny, 0, nx
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


class CylinderChannel3DSolver(LidDrivenCavity3DSolver):
    """LidDrivenCavity3DSolver's projection step on the cylinder channel: the
    v5 geometry extruded along z (host_grid / host_masks / host_potential_flow
    on every plane, w = 0), fields (nz, ny, nx) float32 device tensors.

    time_step is the cavity's with two stages exchanged.  The lid walls
    become K.apply_channel_bc_ibm3d (inlet, outlet copy, free-slip spanwise
    faces, channel walls and the immersed-boundary forcing with
    force_strength = min(1, step / initial_steps), one launch, after the
    predictor and after the projection; ``ibm_mask`` stays the 2-D float64
    array and only its bounding box is visited).  The pressure solve takes the
    solid mask: phi = zeros, then cfd_rbgs3d_mask2d_f32 (use_fast_pressure,
    any spacing) with ``cylinder_mask2d``, the (ny, nx) uint8 mask that every
    plane shares -- fused passes whose waves hold its bits in registers -- or
    cfd_jacobi3d_f32 (dx == dy == dz) with ``cylinder_mask``, the same mask
    expanded once to (nz, ny, nx), which the vorticity kernel reads too.  LES as in the cavity
    solver.  No host synchronisation per step, except the adaptive dt's one
    read from step 1000 on.

    Forces: the second (post-projection) forcing call of each step adds the
    momentum it removes, sum(before - after) of u, v, w over the forced cells
    in float64, into that step's row of a device buffer; ``force_history`` and
    ``force_coefficients()`` read it lazily.  ``compute_vorticity()`` returns
    |omega| (NaN in the cylinder); with log_diagnostics ``diagnostics`` gains
    ``vorticity_max`` of the step's final unclipped fields.

    spanwise_bc="periodic": every stage is its *_zper form (the pad rule:
    the operator on the field with plane nz-1 put in front and plane 0 behind,
    cropped; tests/zper_reference.py), the boundary stage loses its face
    step, ``z`` = z_min + k dz with dz = Lz / nz, and the pressure solve is
    cfd_rbgs3d_zper_f32 on arrays padded by its ghost planes -- ``phi`` and
    ``div_u_star`` are the (nz, ny, nx) views of the owned planes.
    spanwise_perturbation (either spanwise_bc) scales the initial u per plane,
    which is what makes a run three-dimensional.

    Statistics and snapshots are the cavity solver's (enable_statistics,
    statistics, save_snapshot, load_snapshot); here the statistics default to
    the span average, the mean flow and Reynolds stresses over time and z on
    the (ny, nx) plane, and a snapshot's vorticity is NaN in the cylinder.
    With the scalar on, ``enable_statistics(scalar_moments=True)`` adds T, TT,
    uT, vT, wT of the step's final T to the sums in the same single launch
    (K.accumulate_flow_scalar_stats3d) and ``statistics()`` gains mean_T, the
    temperature variance TT and the turbulent heat fluxes uT, vT, wT; off by
    default, and then the sums, snapshots and launches are what they were.

    Passive scalar (config.scalar=True; off by default, and then nothing is
    allocated or launched): ``T`` starts at scalar_inlet.  Each step, directly
    after the predictor, K.scalar_advance3d advances it with the step's
    incoming u, v, w (diffusivity f32(nu / prandtl), with LES plus nu_t /
    turbulent_prandtl per cell from the nu_t the predictor has just stored;
    the artificial viscosity is not added) into a second buffer, the two swap,
    and K.apply_scalar_bc_heat3d relaxes T towards scalar_cylinder in the
    forcing zone with the step's force_strength and sets the faces (inlet
    scalar_inlet; outlet, adiabatic walls and spanwise faces copy).  Without
    buoyancy the scalar never acts back on the flow.  ``heat_history`` and
    ``nusselt_numbers()`` read the per-step heat sums lazily; snapshots gain
    T; tests/scalar3d_reference.py states the arithmetic.

    Buoyancy (config.richardson != 0, with the scalar; off by default, and
    then every launch is what it was): the predictor adds dt * (b_f * (T -
    t_ref)) in float32 to the interior cells' u*, v*, w*, inside its own
    kernel, with the step's incoming T, ``buoyancy_vector`` b = f32(-Ri
    V_inf^2 / (2 R_cylinder (scalar_cylinder - scalar_inlet)) g / |g|) and
    t_ref = f32(scalar_reference, else scalar_inlet): hot fluid is pushed
    against gravity_direction.  Snapshots need nothing new (T is stored), and
    the adaptive dt does not look at the buoyant acceleration;
    tests/buoyancy3d_reference.py states the arithmetic.

    Not yet: temporal blocking of the masked 3-D Jacobi (with a mask it runs
    single sweeps: DESIGN.md 4.4), a periodic form of that Jacobi, masks that
    vary along z in the fused GS, pressure statistics (the step keeps no p), a
    Strouhal estimate from the lift history, the scalar's advance fused into
    the predictor's march, float64 and the slab path."""

    _stats_span_default = True

    def __init__(self, config: CylinderChannel3DConfig):
        super().__init__(config)
        cfg = config
        self.x, self.y, self.X, self.Y = host_grid(cfg)
        self._periodic_z = cfg.spanwise_bc == "periodic"
        if self._periodic_z:
            self.z = cfg.z_min + np.arange(cfg.nz) * cfg.dz
            # the solve's arrays with its ghost planes; phi and div_u_star are the owned planes
            G = int(lib().cfd_rbgs3d_zper_ghost())
            pad = lambda: torch.zeros((cfg.nz + 2 * G, cfg.ny, cfg.nx), dtype=self.dtype,  # noqa: E731
                                      device=self.device)
            self._phi_pad, self._div_pad, self._phi_tmp = pad(), pad(), pad()
            self.phi, self.div_u_star = self._phi_pad[G:G + cfg.nz], self._div_pad[G:G + cfg.nz]
            self._rhs_ws = None  # the Jacobi's workspace: no periodic form
        else:
            self.z = np.linspace(cfg.z_min, cfg.z_max, cfg.nz)
        self._y_dev = torch.from_numpy(self.y).to(self.device)
        self.dist, cyl, ibm = host_masks(cfg, self.X, self.Y)
        self.cylinder_mask_host, self.ibm_mask_host = cyl, ibm
        self.ibm_mask = torch.from_numpy(ibm).to(self.device)
        self.ibm_bbox = host_ibm_bbox(ibm)
        self.cylinder_mask2d = torch.from_numpy(cyl).to(self.device).to(torch.uint8).contiguous()
        self.cylinder_mask = self.cylinder_mask2d.expand(cfg.nz, cfg.ny, cfg.nx).contiguous()
        u, v = host_potential_flow(cfg, self.X, self.Y, self.dist, ibm, np.float32)
        if cfg.spanwise_perturbation != 0.0:
            # u[k] = f32(f64(u2d) (1 + a cos(2 pi (z_k - z_min) / Lz))), host side, one time
            ph = 2.0 * np.pi * (self.z - cfg.z_min) / (cfg.z_max - cfg.z_min)
            u3 = (u.astype(np.float64)[None] * (1.0 + cfg.spanwise_perturbation * np.cos(ph))[:, None, None])
            self.u.copy_(torch.from_numpy(u3.astype(np.float32)).to(self.device))
        else:
            self.u.copy_(torch.from_numpy(u).to(self.device).expand_as(self.u))
        self.v.copy_(torch.from_numpy(v).to(self.device).expand_as(self.v))
        self._force = torch.zeros((1024, 3), dtype=torch.float64, device=self.device)
        self._dts = []
        self.scalar = bool(cfg.scalar)
        if self.scalar:
            self.T = torch.full_like(self.u, float(np.float32(cfg.scalar_inlet)))
            self._T_next = torch.empty_like(self.T)
            self._heat = torch.zeros(1024, dtype=torch.float64, device=self.device)
            # alpha = f32(nu / Pr), 1 / Pr_t = f32(1 / Pr_t): formed in double, rounded once
            self._alpha = np.float32(float(cfg.nu) / cfg.prandtl)
            self._inv_prt = np.float32(1.0 / cfg.turbulent_prandtl)
        if cfg.richardson != 0:
            # b_i = f32(-Ri V_inf^2 / (D dT) g_i / |g|): formed in double, rounded once per component
            dT = cfg.scalar_cylinder - cfg.scalar_inlet
            k = -cfg.richardson * cfg.V_inf ** 2 / (2.0 * cfg.R_cylinder * dT)
            gx, gy, gz = (float(x) for x in cfg.gravity_direction)
            n = np.sqrt(gx * gx + gy * gy + gz * gz)
            self.buoyancy_vector = tuple(np.float32(k * (g / n)) for g in (gx, gy, gz))
            self._t_ref = np.float32(cfg.scalar_inlet if cfg.scalar_reference is None else cfg.scalar_reference)

    def _predictor_buoyancy(self):
        """With richardson != 0 the predictor adds dt * (b_f * (T - t_ref)) to
        the interior cells' u*, v*, w* with the step's incoming T (the
        predictor runs before _after_predictor swaps T)."""
        if self.config.richardson == 0:
            return {}
        return {"T": self.T, "buoyancy": self.buoyancy_vector, "t_ref": self._t_ref}

    def _heat_slot(self):
        k = len(self._energy_steps)
        if k >= self._heat.numel():
            grown = torch.zeros(2 * self._heat.numel(), dtype=torch.float64, device=self.device)
            grown[:k] = self._heat[:k]
            self._heat = grown
        return self._heat[k:k + 1]

    def _after_predictor(self, dt):
        """The scalar's step: the advance with the step's incoming u, v, w
        (and the nu_t the predictor has just stored), then the heating with the
        step's force_strength and the faces; T and its second buffer swap."""
        if not self.scalar:
            return
        cfg = self.config
        K.scalar_advance3d(self.T, self.u, self.v, self.w, self._alpha, dt, cfg.dx, cfg.dy, cfg.dz, cfg.use_supg,
                           nu_t=self.nu_t if self.use_les else None, inv_prt=self._inv_prt, out=self._T_next,
                           periodic_z=self._periodic_z)
        self.T, self._T_next = self._T_next, self.T
        K.apply_scalar_bc_heat3d(self.T, self.ibm_mask, cfg.scalar_inlet, cfg.scalar_cylinder,
                                 min(1.0, self.step / cfg.initial_steps), bbox=self.ibm_bbox,
                                 heat_out=self._heat_slot(), periodic_z=self._periodic_z)

    def _snapshot_fields(self):
        return {"T": self.T} if self.scalar else {}

    @property
    def heat_history(self):
        """[(step, Q)]: per step, the float64 sum of after - before of T over
        the cells the heating changed, read lazily from the device (scalar=True)."""
        if not self.scalar:
            raise RuntimeError("heat_history: the scalar is off (CylinderChannel3DConfig(scalar=True))")
        n = len(self._energy_steps)
        vals = self._heat[:n].cpu().numpy() if n else np.zeros(0)
        return [(s, float(q)) for s, q in zip(self._energy_steps, vals)]

    def nusselt_numbers(self):
        """[(step, Nu)] from heat_history: Nu = Q dx dy dz / (dt (nu / Pr)
        (T_cyl - T_in) pi (z_max - z_min)) with the step's own dt -- the heat
        the forcing adds per unit time over the conductive scale k dT (pi D
        Lz) / D.  A volume-forcing estimate (the forcing zone is wider than
        the cylinder and relaxes T rather than fixing a wall flux): the heat
        counterpart of force_coefficients()."""
        cfg = self.config
        vol = cfg.dx * cfg.dy * cfg.dz
        alpha = float(cfg.nu) / cfg.prandtl  # cfg.nu is a float32: the division in double
        scale = alpha * (cfg.scalar_cylinder - cfg.scalar_inlet) * np.pi * (cfg.z_max - cfg.z_min)
        return [(s, q * vol / (dt * scale)) for (s, q), dt in zip(self.heat_history, self._dts)]

    def solve_pressure_fast(self, div_u_star):
        """phi = zeros, then the masked solve (with cfg.dt, like v5.py:328-347):
        red-black GS on any spacing (use_fast_pressure), else the 7-point
        Jacobi, which needs dx == dy == dz exactly.  Solid cells keep phi = 0."""
        cfg = self.config
        if not cfg.use_fast_pressure and not (cfg.dx == cfg.dy == cfg.dz):
            raise ValueError(f"the 3-D Jacobi solve needs dx == dy == dz (got {cfg.dx}, {cfg.dy}, {cfg.dz}); "
                             "use_fast_pressure=True takes any spacing")
        if self._periodic_z:  # div_u_star is the owned planes of _div_pad
            self._phi_pad.zero_()
            K.solve_pressure_gauss_seidel3d_zper(self._phi_pad, self._div_pad, cfg.dx, cfg.dy, cfg.dz, cfg.dt,
                                                 self.cylinder_mask2d, cfg.pressure_iterations,
                                                 cfg.pressure_tolerance, workspace=self._gs_ws,
                                                 iters_done=self._gs_done, phi_tmp=self._phi_tmp, nz=cfg.nz)
            return self.phi
        self.phi.zero_()
        if cfg.use_fast_pressure:
            K.solve_pressure_gauss_seidel3d(self.phi, div_u_star, cfg.dx, cfg.dy, cfg.dz, cfg.dt,
                                            self.cylinder_mask2d, cfg.pressure_iterations, cfg.pressure_tolerance, workspace=self._gs_ws,
                                            iters_done=self._gs_done, phi_tmp=self._phi_tmp)
        else:
            K.solve_pressure_jacobi3d(self.phi, div_u_star, cfg.dx, cfg.dt, self.cylinder_mask,
                                      cfg.pressure_iterations, phi_tmp=self._phi_tmp, rhs_ws=self._rhs_ws)
        return self.phi

    def _force_slot(self):
        k = len(self._energy_steps)
        if k >= self._force.shape[0]:
            grown = torch.zeros((2 * self._force.shape[0], 3), dtype=torch.float64, device=self.device)
            grown[:k] = self._force[:k]
            self._force = grown
        return self._force[k]

    def apply_boundary_conditions(self, u, v, w):
        """Channel BC + IBM forcing, one launch.  On the step's final fields
        (the post-projection call) it also accumulates the step's force row
        and, with log_diagnostics, takes max|omega| before the clips."""
        cfg = self.config
        final = u is self.u
        K.apply_channel_bc_ibm3d(u, v, w, self._y_dev, self.ibm_mask, cfg.y_max, cfg.V_inf, self.step,
                                 min(1.0, self.step / cfg.initial_steps), bbox=self.ibm_bbox,
                                 force_out=self._force_slot() if final else None, periodic_z=self._periodic_z)
        if final and cfg.log_diagnostics:
            self._scal[3:4].zero_()
            call("cfd_vorticity3d_zper_f32" if self._periodic_z else "cfd_vorticity3d_f32", ptr(u), ptr(v), ptr(w),
                 ptr(self.cylinder_mask), None, None, None, None, ptr(self._scal[3:4]), cfg.nz, cfg.ny, cfg.nx, float(cfg.dx), float(cfg.dy), float(cfg.dz),
                 stream_handle())

    def time_step(self):
        dt = super().time_step()
        self._dts.append(float(dt))
        return dt

    def _restart_histories(self):
        super()._restart_histories()
        self._dts = []
        self._force.zero_()  # the forcing kernel adds into its step's row, and the rows are handed out from 0 again
        if self.scalar:
            self._heat.zero_()

    def compute_vorticity(self):
        """|omega| of the current fields: 0 on the six faces (periodic: the
        four x / y faces), NaN in the cylinder."""
        cfg = self.config
        return K.compute_vorticity3d(self.u, self.v, self.w, cfg.dx, cfg.dy, cfg.dz, mask=self.cylinder_mask,
                                     periodic_z=self._periodic_z)

    @property
    def diagnostics(self):
        """The cavity solver's values plus ``vorticity_max``, nanmax|omega| of
        the last step's fields before the clips (log_diagnostics=True)."""
        d = LidDrivenCavity3DSolver.diagnostics.fget(self)
        d["vorticity_max"] = float(self._scal[3].item())
        return d

    @property
    def force_history(self):
        """[(step, Fx, Fy, Fz)]: per step, the sums of before - after of u, v,
        w over the cells the post-projection forcing changed (float64), read
        lazily from the device."""
        n = len(self._energy_steps)
        vals = self._force[:n].cpu().numpy() if n else np.zeros((0, 3))
        return [(s, float(f[0]), float(f[1]), float(f[2])) for s, f in zip(self._energy_steps, vals)]

    def force_coefficients(self):
        """[(step, Cd, Cl)] from force_history: C = 2 F dx dy dz / (dt V_inf^2
        2R (z_max - z_min)) with F = Fx (drag) or Fy (lift) and the step's own
        dt -- the momentum the forcing removed per unit time over the dynamic
        pressure times the cylinder's frontal area."""
        cfg = self.config
        vol = cfg.dx * cfg.dy * cfg.dz
        area = 2.0 * cfg.R_cylinder * (cfg.z_max - cfg.z_min)
        out = []
        for (s, fx, fy, _), dt in zip(self.force_history, self._dts):
            k = 2.0 * vol / (dt * cfg.V_inf ** 2 * area)
            out.append((s, k * fx, k * fy))
        return out


def monitor_simulation_health3d(solver: LidDrivenCavity3DSolver, step: int) -> bool:
    """monitor_simulation_health's thresholds (v5.py:599-613) on u, v, w
    (LidDrivenCavity3DSolver or CylinderChannel3DSolver):
    non-finite values, max|V| > max_velocity, max|div| above 20 (step <= 1000)
    or 2 (after); device reductions with one host read.  A spanwise-periodic
    solver's divergence is the periodic one; a solver that carries the passive
    scalar (scalar=True) also needs T finite."""
    cfg = solver.config
    s = stream_handle()
    n = solver.u.numel()
    cnt = torch.zeros(2, dtype=torch.int32, device=solver.device)
    red = torch.zeros(2, dtype=torch.float32, device=solver.device)
    call("cfd_nonfinite_count_f32", ptr(solver.u), ptr(solver.v), n, ptr(cnt[0:1]), s)
    # w, and the scalar T when the solver carries one
    call("cfd_nonfinite_count_f32", ptr(solver.w), ptr(solver.T) if getattr(solver, "scalar", False) else None, n,
         ptr(cnt[1:2]), s)
    for f in (solver.u, solver.v, solver.w):
        call("cfd_absmax_f32", ptr(f), n, ptr(red[0:1]), s)  # the max accumulates
    div = torch.empty_like(solver.u)
    call("cfd_divergence3d_zper_f32" if solver._periodic_z else "cfd_divergence3d_f32", ptr(solver.u),
         ptr(solver.v), ptr(solver.w), ptr(div), cfg.nz, cfg.ny, cfg.nx,
         float(cfg.dx), float(cfg.dy), float(cfg.dz), ptr(red[1:2]), s)
    n_bad = int(cnt.sum().item())
    vel_max, div_max = (float(x) for x in red.cpu().numpy())
    if n_bad:
        return False
    if vel_max > cfg.max_velocity:
        return False
    div_threshold = 20.0 if step <= 1000 else 2.0
    return not (div_max > div_threshold)


def monitor_simulation_health(solver: OptimizedTurbulentSolver, step: int) -> bool:
    """v5.py:599-613 as device reductions with one host read."""
    cfg = solver.config
    s = stream_handle()
    sfx = "_f32" if solver.u.dtype == torch.float32 else "_f64"
    cnt = torch.zeros(1, dtype=torch.int32, device=solver.device)
    red = torch.zeros(2, dtype=solver.u.dtype, device=solver.device)
    call("cfd_nonfinite_count" + sfx, ptr(solver.u), ptr(solver.v), solver.u.numel(), ptr(cnt), s)
    call("cfd_absmax2" + sfx, ptr(solver.u), ptr(solver.v), solver.u.numel(), ptr(red[0:1]), s)
    div = torch.empty_like(solver.u)
    call("cfd_divergence2d" + sfx, ptr(solver.u), ptr(solver.v), ptr(div), cfg.ny, cfg.nx, float(cfg.dx),
         float(cfg.dy), ptr(red[1:2]), s)
    n_bad = int(cnt.item())
    vel_max, div_max = (float(x) for x in red.cpu().numpy())
    # a persistent pressure solve whose tiles could not all run (a wait for a
    # neighbour tile expired) left phi all NaN: a failed step, reported here
    if K.persistent_failures():
        logging.getLogger(__name__).error("Step %d: a persistent pressure solve failed (a tile wait expired)",
                                          step)
        return False
    if n_bad:
        return False
    if vel_max > cfg.max_velocity:
        return False
    div_threshold = 20.0 if step <= 1000 else 2.0
    return not (div_max > div_threshold)
