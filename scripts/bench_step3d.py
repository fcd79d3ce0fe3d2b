#!/usr/bin/env python3
"""Times the 3-D projection step: the fused predictor alone at 512^3 and 1024^3
(the one-thread-per-cell kernel and the plane march, alternating in the same
run on the same inputs) and the full LidDrivenCavity3DSolver.time_step at 512^3
with 200 Jacobi iterations.  HIP events around windows of several launches,
every timed shape warmed up first.  One JSON line per measurement: ms per
launch (median and min over the rounds), Gcell/s and the fraction of the 8 TB/s
HBM peak at the algorithmic 24 B per cell (tau not stored).

--check: u*, v*, w* of the 1024^3 march on a sample of planes -- the first and
last two and the two on either side of every z-chunk boundary -- against
tests/ref3d.py's predictor3d_numpy, bit for bit (the one place offsets past
2^31 bytes are exercised); reports the count of mismatching cells.
--pmc-run KERNEL: only launches the 512^3 predictor (march / percell) a few
times, for a counter-only profiler pass of its own.

--les: the LES leg instead.  N(0, 1) inputs, tau not stored,
nu_t stored; per size, alternating window by window in one run: (a) the fused
LES predictor (cfd_predictor3d_les_f32) at every march shape and on the
per-cell kernel, (b) the array-nu march (cfd_predictor3d_nu_f32), (c) the
stand-alone cfd_smagorinsky3d_f32, and the scalar-nu march for context; SUPG at
every size, upwind at the first.  The fraction of the HBM peak is at the
algorithmic 28 B per cell for (a) and (b) (12 read + 16 written; 16 + 12 for
the array mode), 16 B for (c), 24 B for the scalar march.  Then the LES
time_step, always at 512^3 whatever --sizes says (--no-step skips it).  With
--check: the fused LES march at the largest size on the same sample of planes
against tests/les3d_reference.py, bit for bit.

--cylinder: the 3-D cylinder channel leg instead, at the
default 600 x 180 x 120 grid: cfd_apply_channel_bc_ibm3d_f32 with the mask's
tight box and with the whole-grid box and cfd_vorticity3d_f32 (ms, algorithmic
bytes and the fraction of the HBM peak), then the pressure solve alone -- 200
red-black GS iterations at tolerance 0, alternating window by window: (a)
cfd_rbgs3d_mask2d_f32 with the 2-D mask at 4 (auto) and at 2 half-sweeps per
pass, (b) cfd_rbgs3d_f32 with the mask expanded to 3-D (in-place colour
passes), (c) cfd_rbgs3d_f32 without a mask (the fused kernel's ceiling on this
grid), (p) cfd_rbgs3d_zper_f32, the spanwise-periodic solve with the 2-D mask
on its ghost-padded arrays -- then CylinderChannel3DSolver.time_step with the
red-black GS, LES off and on, with the pressure solve's share of it; then the
periodic leg: the fused predictor with and without periodic_z on the same
fields (scalar and LES) and time_step with spanwise_bc "free_slip" and
"periodic", each pair alternating window by window (medians of the rounds).

--stats: the flow statistics leg instead, at the same grid:
cfd_flow_stats3d_f32 in span mode without and with nu_t and in full mode (one
moment plane per column, or per cell), and cfd_vorticity3d_f32 writing |omega|
only as the yardstick of the same session, alternating window by window, each
with its algorithmic bytes (the fields read once, 16 B per accumulator
element), the time those bytes take at the HBM peak and the fraction of the
peak reached; the same with the scalar's moments (cfd_flow_scalar_stats3d_f32:
span with T, span with nu_t and T, full with T) and the fused launch's time
over the nm = 9 span launch's, against the two launches a separate T pass would
need; then CylinderChannel3DSolver.time_step with statistics off, in span mode
and in full mode, and on a scalar=True solver with statistics off and with
scalar_moments in span mode, the five solvers alternating window by window.

--scalar: the passive scalar leg instead, at the same grid:
cfd_scalar_advance3d_f32 as plane march (auto, and every rows x cells-per-lane
shape) and as per-cell kernel, with scalar alpha and with the nu_t array, SUPG
and upwind, the fused predictor (SUPG, scalar nu, 24 B per cell) as the
yardstick of the same session, cfd_scalar_bc_heat3d_f32 beside the BC + IBM
stage, all alternating window by window (the advance at its algorithmic 20 B
per cell, 24 B with nu_t); then CylinderChannel3DSolver.time_step with the
scalar off and on, the two solvers alternating.

--buoyancy: the Boussinesq buoyancy leg instead, at the same
grid: the buoyant predictor (cfd_predictor3d_buoy_f32 and its LES / periodic
forms, 28 B per cell against the plain predictor's 24; 32 against 28 with LES)
beside the plain one on the same fields, SUPG and upwind, scalar nu and LES,
flat and periodic, and the two-launch alternative (the plain predictor, then
torch passes that add the term to v*), all alternating window by window, with
each pair's ratio next to the byte model's; then
CylinderChannel3DSolver.time_step with scalar=True at richardson 0 and 1, the
two solvers alternating.

The script sets no time limits itself.  To give every GPU stage a limit of its
own, run one invocation per stage, each under `timeout` and chained with &&:
`--les --sizes 512 --no-step`, `--les --sizes 1024 --no-step --check`, then
`--les --step-only` (the two time_step timings and nothing else).
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import _pkgpath  # noqa: E402
_pkgpath.load()
from cfd_simulations_amd import _lib  # noqa: E402
from cfd_simulations_amd import kernels as K  # noqa: E402
from cfd_simulations_amd._lib import call  # noqa: E402

HBM_PEAK = 8.0e12   # B/s
BYTES_PER_CELL = 24
NU, DT = np.float32(0.011), np.float32(2e-5)


def march_zchunk(nz, ny, nx, cpl, rows):
    """Planes per z-chunk of the plane march (pred_planes_launch's rule)."""
    per = -(-nx // (64 * cpl)) * -(-ny // (4 * rows))
    return min(max(nz * per // 2048, 8), 32)


def make_fields(n, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn((n, n, n), device="cuda", generator=g) for _ in range(3)]


class Predictor:
    def __init__(self, n, supg=True):
        self.n, self.supg = n, supg
        self.h = 1.0 / (n - 1)
        self.ins = make_fields(n)
        self.outs = [torch.empty_like(self.ins[0]) for _ in range(3)]

    def launch(self):
        K.predictor3d_fused(*self.ins, self.h, self.h, self.h, DT, NU, self.supg, u_star=self.outs[0],
                            v_star=self.outs[1], w_star=self.outs[2], store_tau=False)

    def window(self, launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            self.launch()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / launches


def last_path():
    cpl = ctypes.c_int(0)
    return int(_lib.lib().cfd_get_last_predictor3d_path(ctypes.byref(cpl))), int(cpl.value)


def time_predictor(p, configs, rounds, launches):
    """configs: {label: (variant, rows, cells_per_lane)}; alternates them round by round."""
    ms = {k: [] for k in configs}
    paths = {}
    for k, cfg in configs.items():   # warm up every shape
        call("cfd_set_predictor3d_config", *cfg)
        for _ in range(3):
            p.launch()
        paths[k] = last_path()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, cfg in configs.items():
            call("cfd_set_predictor3d_config", *cfg)
            ms[k].append(p.window(launches))
    call("cfd_reset_tuning")
    cells = p.n ** 3
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = med
        print(json.dumps({"bench": "predictor3d", "n": p.n, "supg": p.supg, "kernel": k,
                          "path": "march" if paths[k][0] == 1 else "per_cell", "cells_per_lane": paths[k][1],
                          "config": list(configs[k]), "ms": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "rounds": rounds, "launches_per_round": launches,
                          "gcell_per_s": round(cells / med / 1e6, 1),
                          "hbm_fraction_24B": round(cells * BYTES_PER_CELL / (med * 1e-3) / HBM_PEAK, 3)}), flush=True)
    return out


def check_planes(p):
    sys.path.insert(0, str(ROOT / "tests"))
    from ref3d import predictor3d_numpy
    n = p.n
    call("cfd_reset_tuning")
    p.launch()
    path, cpl = last_path()
    zc = march_zchunk(n, n, n, cpl, 2)
    slabs = [(0, 3), (n - 3, n)] + [(b - 2, b + 2) for b in range(zc, n - 1, zc)]  # [lo, hi): interior planes checked
    bad = cells = planes = 0
    for lo, hi in slabs:
        u, v, w = (f[lo:hi].cpu().numpy() for f in p.ins)
        ref = predictor3d_numpy(u, v, w, NU, dx=p.h, dy=p.h, dz=p.h, dt=DT, use_supg=p.supg)
        first = lo == 0           # the grid's own first / last plane is a face of the slab too
        last = hi == n
        sel = slice(0 if first else 1, (hi - lo) if last else (hi - lo - 1))
        for name, t in zip(("u_star", "v_star", "w_star"), p.outs):
            got = t[lo:hi].cpu().numpy()[sel]
            bad += int((got.view(np.uint32) != ref[name][sel].view(np.uint32)).sum())
            cells += got.size
        planes += sel.stop - sel.start
    print(json.dumps({"bench": "predictor3d_check", "n": n, "path": "march" if path == 1 else "per_cell",
                      "cells_per_lane": cpl, "zchunk": zc, "planes": planes, "values_compared": cells,
                      "mismatching": bad, "last_plane_byte_offset": (n - 1) * n * n * 4}), flush=True)
    return bad


ART, CS = np.float32(0.001), 0.17
MARCH_SHAPES = [(r, c) for c in (4, 2, 1) for r in (2, 1)]   # (rows per wave, cells per lane)


class LesPredictor(Predictor):
    """The three LES-leg launches on one set of arrays (nu_eff: a positive field)."""

    def __init__(self, n, supg=True):
        super().__init__(n, supg)
        self.nu_t = torch.empty_like(self.ins[0])
        self.nu_eff = torch.rand((n, n, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        self.nu_eff.mul_(0.02).add_(0.002)
        self.sp = (self.h, self.h, self.h)
        self.o = dict(u_star=self.outs[0], v_star=self.outs[1], w_star=self.outs[2], store_tau=False)

    def les(self):
        K.predictor3d_fused_les(*self.ins, *self.sp, DT, NU, ART, CS, self.supg, nu_t=self.nu_t, **self.o)

    def array(self):
        K.predictor3d_fused(*self.ins, *self.sp, DT, self.nu_eff, self.supg, **self.o)

    def smag(self):
        K.compute_smagorinsky_viscosity3d(*self.ins, *self.sp, CS, out=self.nu_t)


def les_cases(p):
    """{label: (launch, predictor config, algorithmic bytes per cell)}"""
    cases = {f"les_march_r{r}_c{c}": (p.les, (2, r, c), 28) for r, c in MARCH_SHAPES}
    cases["les_auto"] = (p.les, (0, 0, 0), 28)
    cases["les_per_cell"] = (p.les, (1, 0, 0), 28)
    cases["array_march"] = (p.array, (0, 0, 0), 28)
    cases["smagorinsky3d"] = (p.smag, (0, 0, 0), 16)
    cases["scalar_march"] = (p.launch, (0, 0, 0), 24)
    return cases


def time_les(p, rounds, launches):
    cases = les_cases(p)
    ms = {k: [] for k in cases}
    paths = {}

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / launches

    for k, (fn, cfg, _) in cases.items():   # warm up every shape
        call("cfd_set_predictor3d_config", *cfg)
        for _ in range(3):
            fn()
        paths[k] = last_path() if k != "smagorinsky3d" else (0, 1)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, (fn, cfg, _) in cases.items():
            call("cfd_set_predictor3d_config", *cfg)
            ms[k].append(window(fn))
    call("cfd_reset_tuning")
    cells = p.n ** 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        nbytes = cases[k][2]
        print(json.dumps({"bench": "les3d_predictor", "n": p.n, "supg": p.supg, "kernel": k,
                          "path": "march" if paths[k][0] == 1 else "per_cell", "cells_per_lane": paths[k][1],
                          "config": list(cases[k][1]), "ms": round(med[k], 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "rounds": rounds, "launches_per_round": launches,
                          "gcell_per_s": round(cells / med[k] / 1e6, 1), "bytes_per_cell": nbytes,
                          "hbm_fraction": round(cells * nbytes / (med[k] * 1e-3) / HBM_PEAK, 3)}), flush=True)
    fused = {k: med[k] for k in med if k.startswith("les_march_")}
    best = min(fused, key=fused.get)
    comp = med["array_march"] + med["smagorinsky3d"]
    print(json.dumps({"bench": "les3d_decision", "n": p.n, "supg": p.supg, "fastest_fused": best,
                      "a_ms": round(fused[best], 4), "b_ms": round(med["array_march"], 4),
                      "c_ms": round(med["smagorinsky3d"], 4), "b_plus_c_ms": round(comp, 4),
                      "a_over_b_plus_c": round(fused[best] / comp, 3), "bar": 0.97,
                      "fused_wins": bool(fused[best] <= 0.97 * comp),
                      "les_auto_over_scalar_march": round(med["les_auto"] / med["scalar_march"], 3)}), flush=True)


def check_planes_les(p):
    """check_planes for the fused LES march: u*, v*, w* and nu_t."""
    sys.path.insert(0, str(ROOT / "tests"))
    from les3d_reference import predictor3d_les_numpy
    n = p.n
    call("cfd_reset_tuning")
    p.les()
    path, cpl = last_path()
    zc = march_zchunk(n, n, n, cpl, 2)
    slabs = [(0, 3), (n - 3, n)] + [(b - 2, b + 2) for b in range(zc, n - 1, zc)]
    bad = cells = planes = 0
    for lo, hi in slabs:
        u, v, w = (f[lo:hi].cpu().numpy() for f in p.ins)
        ref = predictor3d_les_numpy(u, v, w, NU, ART, CS, dx=p.h, dy=p.h, dz=p.h, dt=DT, use_supg=p.supg)
        first, last = lo == 0, hi == n
        sel = slice(0 if first else 1, (hi - lo) if last else (hi - lo - 1))
        for name, t in zip(("u_star", "v_star", "w_star", "nu_t"), p.outs + [p.nu_t]):
            got = t[lo:hi].cpu().numpy()[sel]
            bad += int((got.view(np.uint32) != ref[name][sel].view(np.uint32)).sum())
            cells += got.size
        planes += sel.stop - sel.start
    print(json.dumps({"bench": "les3d_predictor_check", "n": n, "path": "march" if path == 1 else "per_cell",
                      "cells_per_lane": cpl, "zchunk": zc, "planes": planes, "values_compared": cells,
                      "mismatching": bad, "last_plane_byte_offset": (n - 1) * n * n * 4}), flush=True)
    return bad


def time_step(n, iters, steps, les=False):
    from cfd_simulations_amd.solver import LesCavity3DConfig, LidDrivenCavity3DConfig, LidDrivenCavity3DSolver
    if les:
        return time_step_cfg(LidDrivenCavity3DSolver(LesCavity3DConfig(nz=n, ny=n, nx=n, pressure_iterations=iters)),
                             n, iters, steps, "les_cavity3d_time_step")
    c = LidDrivenCavity3DConfig(nz=n, ny=n, nx=n, pressure_iterations=iters)
    s = LidDrivenCavity3DSolver(c)
    return time_step_cfg(s, n, iters, steps, "cavity3d_time_step")


def time_step_cfg(s, n, iters, steps, label):
    for _ in range(2):
        s.time_step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        s.time_step()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / steps
    print(json.dumps({"bench": label, "n": n, "jacobi_iterations": iters, "steps": steps,
                      "ms_per_step": round(ms, 3), "gcell_per_s": round(n ** 3 / ms / 1e6, 2),
                      "jacobi_gcell_sweeps_per_s": round(n ** 3 * iters / ms / 1e6, 1),
                      "energy_last": s.energy_history[-1][1]}), flush=True)


def window_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def bc_ibm_bytes(nz, ny, nx, ibm, bbox):
    """Algorithmic bytes of one cfd_apply_channel_bc_ibm3d_f32 call: 12 B (u, v,
    w) per cell read or written once, the mask's box read once (8 B per cell)."""
    i0, i1, j0, j1 = bbox
    inner = (ny - 2) * (nx - 2)                      # a plane without walls, inlet and outlet columns
    rd = 2 * inner + (nz - 4) * (ny - 2)             # planes 1 and nz-2; the outlet's source column between them
    wr = 2 * ny * nx                                 # planes 0 and nz-1
    wr += (nz - 2) * (2 * nx + 2 * (ny - 2))         # wall rows, inlet and outlet columns of the other planes
    forced = int((ibm[1:-1, 1:-2] > 0).sum())        # forced cells not counted above: read and written
    rd += (nz - 4) * forced
    wr += (nz - 2) * forced
    return 12 * (rd + wr) + 8 * (i1 - i0) * (j1 - j0)


def last_tbr_shape():
    v = [ctypes.c_int() for _ in range(4)]
    call("cfd_get_last_tbr_shape", *[ctypes.byref(x) for x in v])
    return [x.value for x in v]


def cylinder_solves(s, rounds, iters=200):
    """The cylinder channel's pressure solve alone, `iters` iterations at
    tolerance 0 on the solver's grid and mask: {leg: (mask, blocking levels)}."""
    c = s.config
    cells = c.nz * c.ny * c.nx
    g = torch.Generator(device="cuda").manual_seed(11)
    div = torch.randn((c.nz, c.ny, c.nx), device="cuda", generator=g) * 1e-3
    phi, tmp = torch.zeros_like(div), torch.empty_like(div)
    legs = {"a_mask2d": (s.cylinder_mask2d, 0), "a_mask2d_2_levels": (s.cylinder_mask2d, 2),
            "b_mask3d": (s.cylinder_mask, 0), "c_unmasked": (None, 0), "p_mask2d_zper": (s.cylinder_mask2d, 0)}
    # the periodic solve's arrays: the same div on the owned planes of the ghost-padded layout
    G = int(_lib.lib().cfd_rbgs3d_zper_ghost())
    div_p = torch.zeros((c.nz + 2 * G, c.ny, c.nx), device="cuda")
    div_p[G:G + c.nz].copy_(div)
    phi_p, tmp_p = torch.zeros_like(div_p), torch.empty_like(div_p)

    def run(k):
        mask, levels = legs[k]
        call("cfd_set_jacobi3d_blocking", levels, 0, 0)
        if k == "p_mask2d_zper":
            K.solve_pressure_gauss_seidel3d_zper(phi_p, div_p, c.dx, c.dy, c.dz, c.dt, mask, iters, 0.0,
                                                 workspace=s._gs_ws, iters_done=s._gs_done, phi_tmp=tmp_p, nz=c.nz)
            return
        K.solve_pressure_gauss_seidel3d(phi, div, c.dx, c.dy, c.dz, c.dt, mask, iters, 0.0, workspace=s._gs_ws,
                                        iters_done=s._gs_done, phi_tmp=tmp)

    ms, shapes = {k: [] for k in legs}, {}
    for k in legs:   # warm up every leg
        run(k)
        shapes[k] = last_tbr_shape() if k != "b_mask3d" else None
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k in legs:
            ms[k].append(window_ms(lambda: run(k), 1))
    call("cfd_set_jacobi3d_blocking", 0, 0, 0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(json.dumps({"bench": "cylinder3d_solve", "grid": [c.nz, c.ny, c.nx], "leg": k, "iterations": iters,
                          "tolerance": 0.0, "last_tbr_shape": shapes[k], "ms": round(med[k], 3),
                          "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "rounds": rounds,
                          "ms_per_iteration": round(med[k] / iters, 4),
                          "gcell_updates_per_s": round(cells * iters / med[k] / 1e6, 1)}), flush=True)
    best = min(("a_mask2d", "a_mask2d_2_levels"), key=med.get)
    print(json.dumps({"bench": "cylinder3d_solve_decision", "fastest_masked": best,
                      "a_over_b": round(med["a_mask2d"] / med["b_mask3d"], 3),
                      "a2_over_b": round(med["a_mask2d_2_levels"] / med["b_mask3d"], 3),
                      "a_over_c": round(med["a_mask2d"] / med["c_unmasked"], 3), "bar": 0.97,
                      "fused_wins": bool(med[best] < 0.97 * med["b_mask3d"])}), flush=True)
    print(json.dumps({"bench": "cylinder3d_solve_zper", "periodic_over_free_slip":
                      round(med["p_mask2d_zper"] / med["a_mask2d"], 3),
                      "expected_plane_work": round((c.nz + 2 * G) / c.nz, 3), "ghost": G, "bar": 1.15}), flush=True)


def cylinder_zper_leg(rounds, launches, steps):
    """The spanwise-periodic legs next to their free-slip counterparts, each
    pair alternating window by window: the fused predictor with and without
    periodic_z on the solver's fields (scalar and LES), then time_step."""
    from cfd_simulations_amd.solver import CylinderChannel3DConfig, CylinderChannel3DSolver
    for les in (False, True):
        pair = {bc: CylinderChannel3DSolver(CylinderChannel3DConfig(use_les=les, spanwise_bc=bc,
                                                                    spanwise_perturbation=0.05))
                for bc in ("free_slip", "periodic")}
        c = pair["periodic"].config
        grid, cells = [c.nz, c.ny, c.nx], c.nz * c.ny * c.nx
        for s in pair.values():
            for _ in range(2):
                s.time_step()
        s = pair["periodic"]
        o = dict(u_star=s.u_star, v_star=s.v_star, w_star=s.w_star, store_tau=False)

        def pred(per):
            if les:
                K.predictor3d_fused_les(s.u, s.v, s.w, c.dx, c.dy, c.dz, DT, c.nu, c.artificial_viscosity,
                                        c.smagorinsky_constant, c.use_supg, nu_t=s.nu_t, periodic_z=per, **o)
            else:
                K.predictor3d_fused(s.u, s.v, s.w, c.dx, c.dy, c.dz, DT, NU, c.use_supg, periodic_z=per, **o)

        ms = {False: [], True: []}
        for per in ms:
            for _ in range(3):
                pred(per)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for per in ms:
                ms[per].append(window_ms(lambda: pred(per), launches))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"bench": "cylinder3d_predictor_zper", "grid": grid, "les": les, "path": last_path(),
                          "ms_free_slip": round(med[False], 4), "ms_periodic": round(med[True], 4),
                          "ms_min": [round(min(ms[False]), 4), round(min(ms[True]), 4)],
                          "ms_max": [round(max(ms[False]), 4), round(max(ms[True]), 4)],
                          "periodic_over_free_slip": round(med[True] / med[False], 3), "rounds": rounds,
                          "launches_per_round": launches}), flush=True)
        st = {k: [] for k in pair}
        for _ in range(rounds):
            for k, sv in pair.items():
                st[k].append(window_ms(sv.time_step, steps))
        med = {k: statistics.median(v) for k, v in st.items()}
        shape = last_tbr_shape()
        for k, sv in pair.items():
            f = sv.force_coefficients()[-1]
            print(json.dumps({"bench": "cylinder3d_time_step_zper", "grid": grid, "les": les, "spanwise_bc": k,
                              "pressure": "rbgs", "iterations": c.pressure_iterations, "steps_per_window": steps,
                              "rounds": rounds, "ms_per_step": round(med[k], 3), "ms_min": round(min(st[k]), 3),
                              "ms_max": round(max(st[k]), 3), "gcell_per_s": round(cells / med[k] / 1e6, 3),
                              "w_absmax": float(sv.w.abs().max().item()), "energy_last": sv.energy_history[-1][1],
                              "cd_last": f[1], "cl_last": f[2]}), flush=True)
        print(json.dumps({"bench": "cylinder3d_time_step_zper_ratio", "les": les, "last_tbr_shape": shape,
                          "periodic_over_free_slip": round(med["periodic"] / med["free_slip"], 3)}), flush=True)
        del pair, s
        torch.cuda.empty_cache()


def cylinder_leg(rounds, launches, steps):
    """The 3-D cylinder channel at its default 600 x 180 x 120 grid (DESIGN.md
    4.4): the BC + IBM stage with the mask's tight box and with the whole-grid
    box, the vorticity kernel, and time_step with RB-GS, LES off and on, with
    the pressure solve's share of the step (the library's solve timing)."""
    from cfd_simulations_amd.solver import CylinderChannel3DConfig, CylinderChannel3DSolver
    c = CylinderChannel3DConfig()
    s = CylinderChannel3DSolver(c)
    nz, ny, nx = c.nz, c.ny, c.nx
    cells = nz * ny * nx
    whole = (0, ny, 0, nx)
    force = torch.zeros(3, dtype=torch.float64, device="cuda")
    mag = torch.empty_like(s.u)

    def bc(bbox):
        K.apply_channel_bc_ibm3d(s.u, s.v, s.w, s._y_dev, s.ibm_mask, c.y_max, c.V_inf, 1500, 1e-3, bbox=bbox,
                                 force_out=force)

    def vort():
        call("cfd_vorticity3d_f32", _lib.ptr(s.u), _lib.ptr(s.v), _lib.ptr(s.w), _lib.ptr(s.cylinder_mask), None,
             None, None, _lib.ptr(mag), None, nz, ny, nx, c.dx, c.dy, c.dz, _lib.stream_handle())

    cases = {"bc_ibm_tight_box": (lambda: bc(s.ibm_bbox), bc_ibm_bytes(nz, ny, nx, s.ibm_mask_host, s.ibm_bbox)),
             "bc_ibm_whole_box": (lambda: bc(whole), bc_ibm_bytes(nz, ny, nx, s.ibm_mask_host, whole)),
             "vorticity3d": (vort, 17 * cells)}      # u, v, w and the mask read, |omega| written
    ms = {k: [] for k in cases}
    for fn, _ in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, (fn, _) in cases.items():
            ms[k].append(window_ms(fn, launches))
    i0, i1, j0, j1 = s.ibm_bbox
    for k, v in ms.items():
        med, nbytes = statistics.median(v), cases[k][1]
        print(json.dumps({"bench": "cylinder3d_kernel", "grid": [nz, ny, nx], "kernel": k, "ms": round(med, 4),
                          "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "rounds": rounds,
                          "launches_per_round": launches, "ibm_box": [i0, i1, j0, j1],
                          "box_fraction_of_plane": round((i1 - i0) * (j1 - j0) / (ny * nx), 4),
                          "algorithmic_bytes": nbytes, "full_pass_bytes": 24 * cells + 8 * ny * nx,
                          "hbm_fraction": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}), flush=True)
    cylinder_solves(s, rounds)
    del s, mag
    torch.cuda.empty_cache()
    ms_solve, n_sweeps = ctypes.c_double(0), ctypes.c_longlong(0)
    for les in (False, True):
        s = CylinderChannel3DSolver(CylinderChannel3DConfig(use_les=les))
        for _ in range(2):
            s.time_step()
        torch.cuda.synchronize()
        ms_step = window_ms(s.time_step, steps)
        # the solve's share: the same steps again with the library's event pairs around every solve
        call("cfd_timing_enable", 1)
        call("cfd_timing_read", ctypes.byref(ms_solve), ctypes.byref(n_sweeps), 1)
        for _ in range(steps):
            s.time_step()
        call("cfd_timing_read", ctypes.byref(ms_solve), ctypes.byref(n_sweeps), 1)
        call("cfd_timing_enable", 0)
        f = s.force_coefficients()[-1]
        print(json.dumps({"bench": "cylinder3d_time_step", "grid": [nz, ny, nx], "les": les, "pressure": "rbgs",
                          "iterations": c.pressure_iterations, "steps": steps, "ms_per_step": round(ms_step, 3),
                          "solve_ms_per_step": round(ms_solve.value / steps, 3),
                          "solve_share": round(ms_solve.value / steps / ms_step, 3),
                          "gcell_per_s": round(cells / ms_step / 1e6, 3), "energy_last": s.energy_history[-1][1],
                          "cd_last": f[1], "cl_last": f[2]}), flush=True)
        del s
        torch.cuda.empty_cache()


def stats_leg(rounds, launches, steps, step_only=False, no_step=False):
    """The flow statistics at the default 600 x 180 x 120 grid:
    cfd_flow_stats3d_f32 in span mode without and with nu_t and in full mode,
    with cfd_vorticity3d_f32 (|omega| only, masked) as the yardstick, the legs
    alternating window by window, cfd_flow_scalar_stats3d_f32 (T's moments
    in the same launch: nm = 14, 15) among them; then
    CylinderChannel3DSolver.time_step with statistics off, in span mode and in
    full mode, and with the scalar on without statistics and with
    scalar_moments in span mode, the solvers alternating."""
    from cfd_simulations_amd.solver import CylinderChannel3DConfig, CylinderChannel3DSolver
    c = CylinderChannel3DConfig()
    nz, ny, nx = c.nz, c.ny, c.nx
    cells, cols = nz * ny * nx, ny * nx
    grid = [nz, ny, nx]
    if not step_only:
        s = CylinderChannel3DSolver(CylinderChannel3DConfig(use_les=True, spanwise_perturbation=0.05, scalar=True))
        for _ in range(2):
            s.time_step()   # fields that depend on z, a nu_t and a heated T (the scalar is passive: u, v, w as without)
        mag = torch.empty_like(s.u)
        span9, span10, span14, span15 = (torch.zeros((nm, ny, nx), dtype=torch.float64, device="cuda")
                                         for nm in (9, 10, 14, 15))
        full9, full14 = (torch.zeros((nm, nz, ny, nx), dtype=torch.float64, device="cuda") for nm in (9, 14))

        def vort():
            call("cfd_vorticity3d_f32", _lib.ptr(s.u), _lib.ptr(s.v), _lib.ptr(s.w), _lib.ptr(s.cylinder_mask), None,
                 None, None, _lib.ptr(mag), None, nz, ny, nx, c.dx, c.dy, c.dz, _lib.stream_handle())

        # algorithmic bytes: the fields read once; an accumulator element read and written once
        cases = {"stats_span": (lambda: K.accumulate_flow_stats3d(s.u, s.v, s.w, span9, 2e-5, True),
                                12 * cells + 16 * 9 * cols),
                 "stats_span_nu_t": (lambda: K.accumulate_flow_stats3d(s.u, s.v, s.w, span10, 2e-5, True,
                                                                       nu_t=s.nu_t), 16 * cells + 16 * 10 * cols),
                 "stats_full": (lambda: K.accumulate_flow_stats3d(s.u, s.v, s.w, full9, 2e-5, False),
                                (12 + 16 * 9) * cells),
                 "scalar_stats_span": (lambda: K.accumulate_flow_scalar_stats3d(s.u, s.v, s.w, s.T, span14, 2e-5,
                                                                                True), 16 * cells + 16 * 14 * cols),
                 "scalar_stats_span_nu_t": (lambda: K.accumulate_flow_scalar_stats3d(
                     s.u, s.v, s.w, s.T, span15, 2e-5, True, nu_t=s.nu_t), 20 * cells + 16 * 15 * cols),
                 "scalar_stats_full": (lambda: K.accumulate_flow_scalar_stats3d(s.u, s.v, s.w, s.T, full14, 2e-5,
                                                                                False), (16 + 16 * 14) * cells),
                 "vorticity3d": (vort, 17 * cells)}      # u, v, w and the mask read, |omega| written
        ms = {k: [] for k in cases}
        for fn, _ in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, (fn, _) in cases.items():
                ms[k].append(window_ms(fn, launches))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            nbytes = cases[k][1]
            print(json.dumps({"bench": "stats3d_kernel", "grid": grid, "kernel": k, "ms": round(med[k], 4),
                              "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                              "windows_ms": [round(x, 4) for x in v], "rounds": rounds,
                              "launches_per_round": launches, "algorithmic_bytes": nbytes,
                              "ms_at_hbm_peak": round(nbytes / HBM_PEAK * 1e3, 4),
                              "hbm_fraction": round(nbytes / (med[k] * 1e-3) / HBM_PEAK, 4)}), flush=True)
        spread = max(max(v) - min(v) for v in (ms["stats_span"], ms["vorticity3d"]))
        print(json.dumps({"bench": "stats3d_span_vs_vorticity", "span_over_vorticity":
                          round(med["stats_span"] / med["vorticity3d"], 3), "window_spread_ms": round(spread, 4),
                          "span_not_slower": bool(med["stats_span"] <= med["vorticity3d"] + spread)}), flush=True)
        # the fused nm = 14 launch against two launches: a separate pass for T's five moments would read
        # u, v, w and T again, more bytes than the nm = 9 pass itself, so two launches cost at least 2x it
        a, b = ms["scalar_stats_span"], ms["stats_span"]
        spread = max(max(a) - min(a), max(b) - min(b))
        print(json.dumps({"bench": "stats3d_scalar_span_vs_span", "fused_over_span9":
                          round(med["scalar_stats_span"] / med["stats_span"], 3),
                          "byte_model_ratio": round(cases["scalar_stats_span"][1] / cases["stats_span"][1], 3),
                          "margin_ms_under_twice_span9": round(2 * med["stats_span"] - med["scalar_stats_span"], 4),
                          "window_spread_ms": round(spread, 4),
                          "fused_ships_by_rule": bool(2 * med["stats_span"] - med["scalar_stats_span"] > spread)}),
              flush=True)
        del s, mag, span9, span10, span14, span15, full9, full14, cases
        torch.cuda.empty_cache()
    if no_step:   # --no-step: the kernels only
        return
    # statistics: (span_average or None for off, scalar on, scalar_moments)
    modes = {"off": (None, False, False), "span": (True, False, False), "full": (False, False, False),
             "scalar_off": (None, True, False), "scalar_span_moments": (True, True, True)}
    solvers = {}
    for k, (span, scalar, moments) in modes.items():
        sv = solvers[k] = CylinderChannel3DSolver(CylinderChannel3DConfig(spanwise_perturbation=0.05, scalar=scalar))
        if span is not None:
            sv.enable_statistics(span_average=span, scalar_moments=moments)
        for _ in range(2):
            sv.time_step()
    torch.cuda.synchronize()
    st = {k: [] for k in solvers}
    for _ in range(rounds):
        for k, sv in solvers.items():
            st[k].append(window_ms(sv.time_step, steps))
    med = {k: statistics.median(v) for k, v in st.items()}
    for k, sv in solvers.items():
        print(json.dumps({"bench": "stats3d_time_step", "grid": grid, "statistics": k, "les": False,
                          "pressure": "rbgs", "iterations": c.pressure_iterations, "steps_per_window": steps,
                          "rounds": rounds, "ms_per_step": round(med[k], 3), "ms_min": round(min(st[k]), 3),
                          "ms_max": round(max(st[k]), 3), "windows_ms": [round(x, 3) for x in st[k]],
                          "scalar": modes[k][1], "scalar_moments": modes[k][2],
                          "delta_ms_over_off": round(med[k] - med["scalar_off" if modes[k][1] else "off"], 3),
                          "samples": 0 if modes[k][0] is None else sv.statistics()["samples"],
                          "energy_last": sv.energy_history[-1][1]}), flush=True)


def scalar_leg(rounds, launches, steps, step_only=False):
    """The passive scalar at the default 600 x 180 x 120 grid:
    cfd_scalar_advance3d_f32 as plane march (auto and every (rows, cells per
    lane)) and as per-cell kernel, scalar alpha and nu_t array, SUPG and
    upwind, with the fused predictor (SUPG, scalar nu) as the yardstick of the
    same session, then cfd_scalar_bc_heat3d_f32 beside the BC + IBM stage, the
    legs alternating window by window; then CylinderChannel3DSolver.time_step
    with the scalar off and on, the two solvers alternating."""
    from cfd_simulations_amd.solver import CylinderChannel3DConfig, CylinderChannel3DSolver
    c = CylinderChannel3DConfig()
    nz, ny, nx = c.nz, c.ny, c.nx
    cells = nz * ny * nx
    grid = [nz, ny, nx]
    if not step_only:
        s = CylinderChannel3DSolver(CylinderChannel3DConfig(use_les=True, spanwise_perturbation=0.05, scalar=True))
        for _ in range(2):
            s.time_step()   # fields that depend on z, a nu_t and a heated T
        out = torch.empty_like(s.T)
        stars = [torch.empty_like(s.u) for _ in range(3)]
        heat = torch.zeros(1, dtype=torch.float64, device="cuda")
        paths = {}

        def adv(label, cfg4, supg, nut):
            def fn():
                call("cfd_set_scalar3d_config", *cfg4)
                K.scalar_advance3d(s.T, s.u, s.v, s.w, s._alpha, DT, c.dx, c.dy, c.dz, supg,
                                   nu_t=s.nu_t if nut else None, inv_prt=s._inv_prt, out=out)
                cpl = ctypes.c_int(0)
                paths[label] = (int(_lib.lib().cfd_get_last_scalar3d_path(ctypes.byref(cpl))), int(cpl.value))
            return fn

        def pred():
            K.predictor3d_fused(s.u, s.v, s.w, c.dx, c.dy, c.dz, DT, NU, True, u_star=stars[0], v_star=stars[1],
                                w_star=stars[2], store_tau=False)

        def bc_heat():
            K.apply_scalar_bc_heat3d(out, s.ibm_mask, c.scalar_inlet, c.scalar_cylinder, 1.0, bbox=s.ibm_bbox,
                                     heat_out=heat)

        def bc_ibm():
            K.apply_channel_bc_ibm3d(*stars, s._y_dev, s.ibm_mask, c.y_max, c.V_inf, 2000, 1.0, bbox=s.ibm_bbox)

        cases = {}
        for supg in (True, False):
            for nut in (False, True):
                tag = ("supg" if supg else "upwind") + ("_nu_t" if nut else "")
                nb = (24 if nut else 20) * cells
                cases[f"advance_march_{tag}"] = (adv(f"advance_march_{tag}", (0, 0, 0, 0), supg, nut), nb)
                cases[f"advance_per_cell_{tag}"] = (adv(f"advance_per_cell_{tag}", (1, 0, 0, 0), supg, nut), nb)
        for supg, nut, tag in ((True, False, "supg"), (True, True, "supg_nu_t"), (False, False, "upwind"),
                               (False, True, "upwind_nu_t")):
            for r in (2, 1):
                for cpl in (4, 2, 1):
                    k = f"advance_march_{tag}_r{r}_c{cpl}"
                    cases[k] = (adv(k, (2, r, cpl, 0), supg, nut), (24 if nut else 20) * cells)
        cases["predictor3d_supg"] = (pred, BYTES_PER_CELL * cells)
        cases["scalar_bc_heat"] = (bc_heat, 0)
        cases["channel_bc_ibm"] = (bc_ibm, 0)
        ms = {k: [] for k in cases}
        try:
            for fn, _ in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, (fn, _) in cases.items():
                    ms[k].append(window_ms(fn, launches))
        finally:
            call("cfd_reset_tuning")
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            nbytes = cases[k][1]
            rec = {"bench": "scalar3d_kernel", "grid": grid, "kernel": k, "ms": round(med[k], 4),
                   "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows_ms": [round(x, 4) for x in v],
                   "rounds": rounds, "launches_per_round": launches}
            if k in paths:
                rec["path"], rec["cells_per_lane"] = paths[k]
            if nbytes:
                rec.update({"algorithmic_bytes": nbytes, "ms_at_hbm_peak": round(nbytes / HBM_PEAK * 1e3, 4),
                            "hbm_fraction": round(nbytes / (med[k] * 1e-3) / HBM_PEAK, 4)})
            print(json.dumps(rec), flush=True)
        for tag in ("supg", "supg_nu_t", "upwind", "upwind_nu_t"):
            m, p = ms[f"advance_march_{tag}"], ms[f"advance_per_cell_{tag}"]
            spread = max(max(m) - min(m), max(p) - min(p))
            gain = statistics.median(p) - statistics.median(m)
            print(json.dumps({"bench": "scalar3d_march_vs_per_cell", "mode": tag,
                              "per_cell_over_march": round(statistics.median(p) / statistics.median(m), 3),
                              "gain_ms": round(gain, 4), "window_spread_ms": round(spread, 4),
                              "march_is_default_by_rule": bool(gain > spread),
                              "march_over_predictor": round(statistics.median(m) / med["predictor3d_supg"], 3)}),
                  flush=True)
        del s, out, stars, cases
        torch.cuda.empty_cache()
    solvers = {}
    for k, on in (("off", False), ("on", True)):
        sv = solvers[k] = CylinderChannel3DSolver(CylinderChannel3DConfig(spanwise_perturbation=0.05, scalar=on))
        for _ in range(2):
            sv.time_step()
    torch.cuda.synchronize()
    st = {k: [] for k in solvers}
    for _ in range(rounds):
        for k, sv in solvers.items():
            st[k].append(window_ms(sv.time_step, steps))
    med = {k: statistics.median(v) for k, v in st.items()}
    for k, sv in solvers.items():
        print(json.dumps({"bench": "scalar3d_time_step", "grid": grid, "scalar": k, "les": False, "pressure": "rbgs",
                          "iterations": c.pressure_iterations, "steps_per_window": steps, "rounds": rounds,
                          "ms_per_step": round(med[k], 3), "ms_min": round(min(st[k]), 3),
                          "ms_max": round(max(st[k]), 3), "windows_ms": [round(x, 3) for x in st[k]],
                          "delta_ms_over_off": round(med[k] - med["off"], 3),
                          "heat_last": sv.heat_history[-1][1] if k == "on" else None,
                          "energy_last": sv.energy_history[-1][1]}), flush=True)


def buoyancy_leg(rounds, launches, steps, step_only=False):
    """Boussinesq buoyancy at the default 600 x 180 x 120 grid:
    the buoyant predictor beside the plain one on the same fields -- SUPG and
    upwind, scalar nu and LES, flat and periodic -- and the two-launch
    alternative (the plain predictor, then a torch add_ of the term on v*),
    all alternating window by window; then CylinderChannel3DSolver.time_step
    with scalar=True at richardson 0 and 1, the two solvers alternating."""
    from cfd_simulations_amd.solver import CylinderChannel3DConfig, CylinderChannel3DSolver
    c = CylinderChannel3DConfig()
    nz, ny, nx = c.nz, c.ny, c.nx
    cells = nz * ny * nx
    grid = [nz, ny, nx]
    if not step_only:
        s = CylinderChannel3DSolver(CylinderChannel3DConfig(use_les=True, spanwise_perturbation=0.05, scalar=True,
                                                            richardson=1.0))
        for _ in range(2):
            s.time_step()   # fields that depend on z and a heated T
        stars = [torch.empty_like(s.u) for _ in range(3)]
        nu_t = torch.empty_like(s.u)
        theta = torch.empty_like(s.u)
        b, t_ref = s.buoyancy_vector, s._t_ref
        o = dict(u_star=stars[0], v_star=stars[1], w_star=stars[2], store_tau=False)
        paths = {}

        def pred(label, supg, les, per, buoy, config=(0, 0, 0)):
            kw = dict(T=s.T, buoyancy=b, t_ref=t_ref) if buoy else {}

            def fn():
                call("cfd_set_predictor3d_config", *config)
                if les:
                    K.predictor3d_fused_les(s.u, s.v, s.w, c.dx, c.dy, c.dz, DT, c.nu, c.artificial_viscosity,
                                            c.smagorinsky_constant, supg, nu_t=nu_t, periodic_z=per, **o, **kw)
                else:
                    K.predictor3d_fused(s.u, s.v, s.w, c.dx, c.dy, c.dz, DT, NU, supg, periodic_z=per, **o, **kw)
                paths[label] = last_path()
            return fn

        def two_launch(plain):
            def fn():   # the term on v* as a second pass: theta = T - t_ref, v* += (dt by) theta
                plain()
                torch.sub(s.T, float(t_ref), out=theta)
                stars[1].add_(theta, alpha=float(DT) * float(b[1]))
            return fn

        def two_launch_one_pass(plain):
            def fn():   # the cheapest second pass torch offers: v* += (dt by) T (the constant left out)
                plain()
                stars[1].add_(s.T, alpha=float(DT) * float(b[1]))
            return fn

        cases = {}
        for supg in (True, False):
            for les in (False, True):
                for per in (False, True):
                    tag = ("supg" if supg else "upwind") + ("_les" if les else "") + ("_zper" if per else "")
                    nb = 28 if les else 24   # nu_t stored with LES
                    cases[f"plain_{tag}"] = (pred(f"plain_{tag}", supg, les, per, False), nb * cells)
                    cases[f"buoyant_{tag}"] = (pred(f"buoyant_{tag}", supg, les, per, True), (nb + 4) * cells)
        cases["two_launch_supg"] = (two_launch(cases["plain_supg"][0]), (24 + 8 + 12) * cells)
        cases["two_launch_one_pass_supg"] = (two_launch_one_pass(cases["plain_supg"][0]), (24 + 12) * cells)
        # every march shape of the buoyant LES kernels (where the registers of T show: DESIGN.md 4.7)
        for supg in (True, False):
            for r, cpl in MARCH_SHAPES:
                k = f"buoyant_{'supg' if supg else 'upwind'}_les_r{r}_c{cpl}"
                cases[k] = (pred(k, supg, True, False, True, (2, r, cpl)), 32 * cells)
        ms = {k: [] for k in cases}
        try:
            for fn, _ in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, (fn, _) in cases.items():
                    ms[k].append(window_ms(fn, launches))
        finally:
            call("cfd_reset_tuning")
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            nbytes = cases[k][1]
            rec = {"bench": "buoyancy3d_kernel", "grid": grid, "kernel": k, "ms": round(med[k], 4),
                   "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows_ms": [round(x, 4) for x in v],
                   "rounds": rounds, "launches_per_round": launches, "algorithmic_bytes": nbytes,
                   "ms_at_hbm_peak": round(nbytes / HBM_PEAK * 1e3, 4),
                   "hbm_fraction": round(nbytes / (med[k] * 1e-3) / HBM_PEAK, 4)}
            if k in paths:
                rec["path"], rec["cells_per_lane"] = paths[k]
            print(json.dumps(rec), flush=True)
        for mode in ("supg_les", "upwind_les"):
            sweep = {k: med[k] for k in cases if k.startswith(f"buoyant_{mode}_r")}
            best = min(sweep, key=sweep.get)
            print(json.dumps({"bench": "buoyancy3d_les_shapes", "mode": mode, "fastest": best,
                              "fastest_ms": round(sweep[best], 4), "auto_ms": round(med[f"buoyant_{mode}"], 4),
                              "auto_path": paths[f"buoyant_{mode}"], "plain_auto_ms": round(med[f"plain_{mode}"], 4),
                              "fastest_over_plain_auto": round(sweep[best] / med[f"plain_{mode}"], 3),
                              "over_plain_auto": {k[len(f"buoyant_{mode}_"):]: round(v / med[f"plain_{mode}"], 3)
                                                  for k, v in sweep.items()}}), flush=True)
        for k in [k for k in cases if k.startswith("buoyant_") and f"plain_{k[len('buoyant_'):]}" in cases]:
            tag = k[len("buoyant_"):]
            p, q = ms[f"plain_{tag}"], ms[k]
            rec = {"bench": "buoyancy3d_ratio", "mode": tag, "buoyant_over_plain": round(med[k] / med[f"plain_{tag}"], 3),
                   "byte_model_ratio": round(cases[k][1] / cases[f"plain_{tag}"][1], 3),
                   "delta_ms": round(med[k] - med[f"plain_{tag}"], 4),
                   "window_spread_ms": round(max(max(p) - min(p), max(q) - min(q)), 4)}
            if tag == "supg":
                rec["two_launch_over_plain"] = round(med["two_launch_supg"] / med["plain_supg"], 3)
                rec["two_launch_one_pass_over_plain"] = round(med["two_launch_one_pass_supg"] / med["plain_supg"], 3)
                rec["buoyant_over_two_launch_one_pass"] = round(med[k] / med["two_launch_one_pass_supg"], 3)
            print(json.dumps(rec), flush=True)
        del s, stars, nu_t, theta, cases
        torch.cuda.empty_cache()
    solvers = {}
    for k, ri in (("ri0", 0.0), ("ri1", 1.0)):
        sv = solvers[k] = CylinderChannel3DSolver(CylinderChannel3DConfig(spanwise_perturbation=0.05, scalar=True,
                                                                          richardson=ri))
        for _ in range(2):
            sv.time_step()
    torch.cuda.synchronize()
    st = {k: [] for k in solvers}
    for _ in range(rounds):
        for k, sv in solvers.items():
            st[k].append(window_ms(sv.time_step, steps))
    med = {k: statistics.median(v) for k, v in st.items()}
    for k, sv in solvers.items():
        print(json.dumps({"bench": "buoyancy3d_time_step", "grid": grid, "richardson": sv.config.richardson,
                          "scalar": True, "les": False, "pressure": "rbgs", "iterations": c.pressure_iterations,
                          "steps_per_window": steps, "rounds": rounds, "ms_per_step": round(med[k], 3),
                          "ms_min": round(min(st[k]), 3), "ms_max": round(max(st[k]), 3),
                          "windows_ms": [round(x, 3) for x in st[k]],
                          "delta_ms_over_ri0": round(med[k] - med["ri0"], 3),
                          "energy_last": sv.energy_history[-1][1]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="every (rows, cells per lane) of the march at the first size")
    ap.add_argument("--pmc-run", choices=["march", "percell"])
    ap.add_argument("--les", action="store_true", help="the LES leg (see above) instead of the scalar-nu one")
    ap.add_argument("--step-only", action="store_true", help="with --les: only the two 512^3 time_step timings")
    ap.add_argument("--cylinder", action="store_true", help="the 3-D cylinder channel leg (see above) and nothing else")
    ap.add_argument("--zper-only", action="store_true",
                    help="with --cylinder: only the predictor and time_step pairs of the periodic leg")
    ap.add_argument("--stats", action="store_true", help="the flow statistics leg (see above) and nothing else")
    ap.add_argument("--stats-step-only", action="store_true", help="with --stats: only the five time_step timings")
    ap.add_argument("--scalar", action="store_true", help="the passive scalar leg (see above) and nothing else")
    ap.add_argument("--scalar-step-only", action="store_true", help="with --scalar: only the two time_step timings")
    ap.add_argument("--buoyancy", action="store_true", help="the buoyancy leg (see above) and nothing else")
    ap.add_argument("--buoyancy-step-only", action="store_true",
                    help="with --buoyancy: only the two time_step timings")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_step3d.py needs the GPU")
    if a.buoyancy:
        buoyancy_leg(a.rounds, a.launches, 3, a.buoyancy_step_only)
        return
    if a.scalar:
        scalar_leg(a.rounds, a.launches, 3, a.scalar_step_only)
        return
    if a.stats:
        stats_leg(a.rounds, a.launches, 3, a.stats_step_only, a.no_step)
        return
    if a.cylinder:
        if not a.zper_only:
            cylinder_leg(a.rounds, a.launches, 3)
        cylinder_zper_leg(a.rounds, a.launches, 3)
        return
    if a.les:
        sizes = [] if a.step_only else [int(s) for s in a.sizes.split(",")]
        bad = 0
        for i, n in enumerate(sizes):
            p = LesPredictor(n)
            time_les(p, a.rounds, a.launches)
            if a.check and n == max(sizes):
                bad = check_planes_les(p)
            del p
            torch.cuda.empty_cache()
            if i == 0:
                p = LesPredictor(n, supg=False)
                time_les(p, a.rounds, a.launches)
                del p
                torch.cuda.empty_cache()
        if not a.no_step:
            time_step(512, 200, 5, les=True)
            time_step(512, 200, 5)
        sys.exit(1 if bad else 0)
    if a.pmc_run:
        p = Predictor(512)
        call("cfd_set_predictor3d_config", 2 if a.pmc_run == "march" else 1, 0, 0)
        for _ in range(5):
            p.launch()
        torch.cuda.synchronize()
        print("pmc run done", a.pmc_run, last_path())
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    bad = 0
    for i, n in enumerate(sizes):
        p = Predictor(n)
        configs = {"per_cell": (1, 0, 0), "march": (0, 0, 0)}
        if a.sweep and i == 0:
            configs.update({f"march_r{r}_c{c}": (2, r, c) for c in (4, 2, 1) for r in (2, 1)})
        ms = time_predictor(p, configs, a.rounds, a.launches)
        print(json.dumps({"bench": "predictor3d_gain", "n": n, "march_over_per_cell":
                          round(ms["per_cell"] / ms["march"], 3)}), flush=True)
        if i == 0:
            time_predictor(Predictor(n, supg=False), {"per_cell": (1, 0, 0), "march": (0, 0, 0)}, a.rounds,
                           a.launches)
        if a.check and n == max(sizes):
            bad = check_planes(p)
        del p
        torch.cuda.empty_cache()
    if not a.no_step:
        time_step(512, 200, 5)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
