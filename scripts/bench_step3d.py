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


def time_step(n, iters, steps):
    from cfd_simulations_amd.solver import LidDrivenCavity3DConfig, LidDrivenCavity3DSolver
    c = LidDrivenCavity3DConfig(nz=n, ny=n, nx=n, pressure_iterations=iters)
    s = LidDrivenCavity3DSolver(c)
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
    print(json.dumps({"bench": "cavity3d_time_step", "n": n, "jacobi_iterations": iters, "steps": steps,
                      "ms_per_step": round(ms, 3), "gcell_per_s": round(n ** 3 / ms / 1e6, 2),
                      "jacobi_gcell_sweeps_per_s": round(n ** 3 * iters / ms / 1e6, 1),
                      "energy_last": s.energy_history[-1][1]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="every (rows, cells per lane) of the march at the first size")
    ap.add_argument("--pmc-run", choices=["march", "percell"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_step3d.py needs the GPU")
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
