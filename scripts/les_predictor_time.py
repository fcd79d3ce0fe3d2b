#!/usr/bin/env python3
"""Is forming nu_t inside the predictor's row march worth it?  Times, on an
n x n grid (default 8192), float32 and float64, exact and fast tau:

  (a) the fused LES predictor (cfd_predictor2d_les_*: nu_t formed in the
      march's registers, u*, v*, tau and nu_t stored);
  (b) cfd_predictor2d_* with a nu_eff array -- the predictor of the unfused
      composition (nu_t pass, then this);
  (c) cfd_divergence2d_* -- reads u, v and writes one field, the traffic of a
      separate nu_t pass.

(b) and (c) run on the library given with --baseline-lib (a build of the
commit before the LES change, same ABI) when there is one, else on the
current library.  The condition for shipping the fused kernel is
(a) < (b) + (c).

Each launch is timed on its own by HIP events -- (a) and (b) through the
library's timing channel 1 (the event pair cfd_predictor2d_* records around
its launch), (c) by an event pair on the stream -- after warm-up launches of
every case; the three cases alternate within a round and the median over
the rounds is reported, so a drifting clock or a neighbour on the machine
hits all three alike.

    python scripts/les_predictor_time.py [--n 8192] [--rounds 30] [--baseline-lib PATH] [--out FILE.json]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import _pkgpath  # noqa: E402

_pkgpath.load()
import torch  # noqa: E402

from cfd_simulations_amd import _lib  # noqa: E402
from cfd_simulations_amd import kernels as K  # noqa: E402
from cfd_simulations_amd._lib import ptr, stream_handle  # noqa: E402
from cfd_simulations_amd.solver import OptimizedTurbulentConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

cur = _lib.lib()
if args.baseline_lib:
    base = ctypes.CDLL(str(Path(args.baseline_lib).resolve()))
    for name, (res, argtypes) in _lib.PROTOTYPES.items():
        if hasattr(base, name):
            getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
    assert base.cfd_abi_version() == cur.cfd_abi_version()
else:
    base = cur


def check(L, rc):
    if rc:
        raise RuntimeError(L.cfd_last_error().decode(errors="replace"))


def channel1_ms(L, launch):
    """One launch timed by the library's own event pair (timing channel 1)."""
    launch()
    ms, cnt = ctypes.c_double(), ctypes.c_longlong()
    check(L, L.cfd_timing_read_channel(1, ctypes.byref(ms), ctypes.byref(cnt), 1))
    assert cnt.value == 1
    return ms.value


def events_ms(launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


n = args.n
CS = 0.17
results = []
for dtype, sfx in ((torch.float32, "_f32"), (torch.float64, "_f64")):
    c = OptimizedTurbulentConfig(nx=n, ny=n, memory_efficient=(dtype == torch.float32))
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.rand((n, n), generator=g, device="cuda", dtype=dtype) * 2 - 1
    v = torch.rand((n, n), generator=g, device="cuda", dtype=dtype) * 2 - 1
    us, vs, tau, nut, div = (torch.empty_like(u) for _ in range(5))
    nu, art, dt = float(c.nu), float(c.artificial_viscosity), 2e-5
    # the unfused composition's nu_eff array
    nu_eff = (K.compute_smagorinsky_viscosity_fast(u, v, c.dx, c.dy, CS) + nu) + art
    s = stream_handle()

    def fused():
        check(cur, getattr(cur, "cfd_predictor2d_les" + sfx)(ptr(u), ptr(v), nu, art, CS, ptr(us), ptr(vs), ptr(tau),
                                                             ptr(nut), n, n, c.dx, c.dy, dt, 1, s))

    def array_nu():
        check(base, getattr(base, "cfd_predictor2d" + sfx)(ptr(u), ptr(v), ptr(nu_eff), 0.0, ptr(us), ptr(vs),
                                                           ptr(tau), n, n, c.dx, c.dy, dt, 1, s))

    def divergence():
        check(base, getattr(base, "cfd_divergence2d" + sfx)(ptr(u), ptr(v), ptr(div), n, n, c.dx, c.dy, None, s))

    for tau_name, tau_mode in (("exact", 0), ("fast", 1)):
        for L in {id(cur): cur, id(base): base}.values():
            check(L, L.cfd_reset_tuning())
            check(L, L.cfd_set_predictor2d_tau_mode(tau_mode))
        for _ in range(args.warmup):
            fused()
            array_nu()
            divergence()
        torch.cuda.synchronize()
        for L in {id(cur): cur, id(base): base}.values():
            check(L, L.cfd_timing_enable(1))
        ta, tb, tc = [], [], []
        for _ in range(args.rounds):
            ta.append(channel1_ms(cur, fused))
            tb.append(channel1_ms(base, array_nu))
            tc.append(events_ms(divergence))
        for L in {id(cur): cur, id(base): base}.values():
            check(L, L.cfd_timing_enable(0))
            check(L, L.cfd_reset_tuning())
        a, b, cc = (statistics.median(t) for t in (ta, tb, tc))
        cell = u.element_size()
        r = {"grid": [n, n], "dtype": sfx[1:], "tau": tau_name, "rounds": args.rounds,
             "a_fused_les_ms": round(a, 4), "b_predictor_array_nu_ms": round(b, 4), "c_divergence_ms": round(cc, 4),
             "a_min_ms": round(min(ta), 4), "b_min_ms": round(min(tb), 4), "c_min_ms": round(min(tc), 4),
             "a_over_b": round(a / b, 4), "b_plus_c_ms": round(b + cc, 4), "fused_beats_composition": a < b + cc,
             "a_GBps": round(6 * cell * n * n / a / 1e6, 1), "b_GBps": round(6 * cell * n * n / b / 1e6, 1),
             "c_GBps": round(3 * cell * n * n / cc / 1e6, 1),
             "baseline_lib": "given (--baseline-lib)" if args.baseline_lib else "the current library"}
        results.append(r)
        print(json.dumps(r), flush=True)
    del u, v, us, vs, tau, nut, div, nu_eff
    torch.cuda.empty_cache()

if args.out:
    doc = {"what": "fused LES predictor (a) against the unfused composition's predictor with a nu_eff array (b) "
                   "plus a u, v -> one field pass (c, cfd_divergence2d); medians of single launches, HIP events",
           "device": torch.cuda.get_device_name(0), "smagorinsky_constant": CS, "results": results}
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
