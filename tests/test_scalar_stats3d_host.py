"""The scalar statistics' host side (no GPU): the NumPy statement
(tests/scalar_stats3d_reference.py) against a plain triple loop, against
tests/stats3d_reference.py on the planes they share and against its own
identities, the solver's derive_statistics, the new entry point in the
bindings and the library, and its argument validation, which runs before any
device work."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import stats3d_reference as base
from cfd_simulations_amd import _lib
from cfd_simulations_amd.solver import derive_statistics
from scalar_stats3d_reference import SCALAR_MOMENTS, abs_terms, accumulate_numpy, derive, stats_bound

F = np.float32
ROOT = Path(__file__).resolve().parents[1]
SHAPE = (3, 2, 5)


def fields(seed, shape=SHAPE, n=5):
    """u, v, w, T, nu_t: 5 N(0, 1) as float32."""
    rng = np.random.default_rng(seed)
    return [(5 * rng.standard_normal(shape)).astype(F) for _ in range(n)]


def loop_terms(u, v, w, T, nt, k, i, j):
    a, b, c, s = float(u[k, i, j]), float(v[k, i, j]), float(w[k, i, j]), float(T[k, i, j])
    t = [a, b, c, a * a, b * b, c * c, a * b, a * c, b * c]
    t = t if nt is None else t + [float(nt[k, i, j])]
    return t + [s, s * s, a * s, b * s, c * s]


def test_reference_equals_a_triple_loop_and_the_flow_reference():
    nz, ny, nx = SHAPE
    for with_nut in (False, True):
        nm = 15 if with_nut else 14
        span, full = np.zeros((nm, ny, nx)), np.zeros((nm, nz, ny, nx))
        span_abs, want_span, want_full, want_abs = (np.zeros_like(a) for a in (span, span, full, span))
        flow_span, flow_full = np.zeros((nm - 5, ny, nx)), np.zeros((nm - 5, nz, ny, nx))
        for seed, wgt in ((1, 2e-5), (2, 7.3e-5)):
            u, v, w, T, nt = fields(seed)
            nt = nt if with_nut else None
            accumulate_numpy(span, u, v, w, T, wgt, True, nt)
            accumulate_numpy(full, u, v, w, T, wgt, False, nt)
            abs_terms(span_abs, u, v, w, T, wgt, True, nt)
            base.accumulate_numpy(flow_span, u, v, w, wgt, True, nt)
            base.accumulate_numpy(flow_full, u, v, w, wgt, False, nt)
            for i in range(ny):
                for j in range(nx):
                    col, col_abs = [0.0] * nm, [0.0] * nm
                    for k in range(nz):
                        t = loop_terms(u, v, w, T, nt, k, i, j)
                        for m in range(nm):
                            col[m] = col[m] + t[m]
                            col_abs[m] = col_abs[m] + abs(t[m])
                            want_full[m, k, i, j] += wgt * t[m]
                    for m in range(nm):
                        want_span[m, i, j] += wgt * col[m]
                        want_abs[m, i, j] += wgt * col_abs[m]
        assert np.array_equal(span, want_span) and np.array_equal(full, want_full)
        assert np.array_equal(span_abs, want_abs) and (span_abs >= np.abs(span)).all()
        # the planes shared with the flow statistics: the flow reference's, bit for bit
        assert np.array_equal(span[:nm - 5], flow_span) and np.array_equal(full[:nm - 5], flow_full)
        assert span[nm - 5:].all() and full[nm - 5:].all()
    assert SCALAR_MOMENTS == ("T", "TT", "uT", "vT", "wT") and len(base.MOMENTS) == 10
    assert stats_bound is base.stats_bound


def test_derived_statistics_identities():
    nz, ny, nx = SHAPE
    for span in (True, False):
        for nm in (14, 15):
            sums = np.zeros((nm, ny, nx) if span else (nm, nz, ny, nx))
            total = 0.0
            for seed, wgt in ((3, 0.5), (4, 0.25), (5, 1.0)):
                f = fields(seed)
                accumulate_numpy(sums, *f[:4], wgt, span, f[4] if nm == 15 else None)
                total += wgt
            d = derive(sums, total, nz, span)
            flow = base.derive(sums[:nm - 5], total, nz, span)
            assert set(d) == set(flow) | {"mean_T", "TT", "uT", "vT", "wT"}
            assert all(np.array_equal(d[k], flow[k]) for k in flow)
            assert ("mean_nu_t" in d) == (nm == 15)
            norm = total * nz if span else total
            assert np.array_equal(d["mean_T"], sums[nm - 5] / norm) and d["mean_T"].shape == sums.shape[1:]
            # a variance of O(25) against roundings of O(1e-15): never negative here
            assert (d["TT"] >= 0).all()
            for a in "uvw":   # Cauchy-Schwarz
                assert (d[a + "T"] ** 2 <= d[a + a] * d["TT"] * (1 + 1e-12)).all(), a
            # the solver's formulas are the reference's: same keys, same bits
            s = derive_statistics(sums, total, nz, span, scalar=True)
            assert s.keys() == d.keys() and all(np.array_equal(s[k], d[k]) for k in d)
            # the layout is stated, never guessed from the plane count
            with pytest.raises(ValueError):
                derive_statistics(sums, total, nz, span)
            with pytest.raises(ValueError):
                derive_statistics(sums[:nm - 5], total, nz, span, scalar=True)
            s = derive_statistics(sums[:nm - 5], total, nz, span)
            assert s.keys() == flow.keys() and all(np.array_equal(s[k], flow[k]) for k in flow)
        # a constant T: its mean exactly and no fluctuation at all.  T = -1/2, a power of two, so
        # that scaling by it commutes with every rounding: sum(wgt u T) is T sum(wgt u) exactly
        c = np.zeros_like(sums[:14])
        u, v, w = fields(6)[:3]
        for wgt in (0.5, 0.25, 1.0):
            accumulate_numpy(c, u, v, w, np.full(SHAPE, -0.5, F), wgt, span)
        k = derive(c, 1.75, nz, span)
        assert (k["mean_T"] == -0.5).all() and k["mean_u"].all()
        assert not k["TT"].any() and not k["uT"].any() and not k["vT"].any() and not k["wT"].any()
        # T = u: the scalar's moments are u's, bit for bit
        e = np.zeros_like(sums[:14])
        for seed, wgt in ((7, 2e-5), (8, 7.3e-5)):
            u, v, w = fields(seed)[:3]
            accumulate_numpy(e, u, v, w, u, wgt, span)
        k = derive(e, 9.3e-5, nz, span)
        for new, old in (("mean_T", "mean_u"), ("TT", "uu"), ("uT", "uu"), ("vT", "uv"), ("wT", "uw")):
            assert k[old].any() and np.array_equal(k[new], k[old]), (new, old)


def test_entry_point_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cfdsim.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+cfd_flow_scalar_stats3d_f32\s*\(", text, flags=re.M)
    assert len(_lib.PROTOTYPES["cfd_flow_scalar_stats3d_f32"][1]) == 12
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "cfd_flow_scalar_stats3d_f32")
    assert _lib.ABI_VERSION == 1 and re.search(r"CFD_ABI_VERSION\s+1\b", text)
    assert len(_lib.PROTOTYPES["cfd_flow_stats3d_f32"][1]) == 11


def test_host_refusals_need_no_gpu():
    L = _lib.lib()
    p = [ctypes.c_void_p(4096 * (q + 1)) for q in range(6)]  # never dereferenced
    u, v, w, nt, T, acc = p

    def refused(word, *a):
        assert L.cfd_flow_scalar_stats3d_f32(*a, None) == -1, a
        msg = L.cfd_last_error()
        assert msg.startswith(b"flow_scalar_stats3d_f32:") and word in msg, msg

    for q in (0, 1, 2, 4, 5):  # null u, v, w, T or acc (nu_t may be null)
        a = [u, v, w, nt, T, acc]
        a[q] = None
        refused(b"null", *a, 4, 5, 6, 1.0, 1)
    for a in ((u, u, w), (u, v, u), (u, v, v)):
        refused(b"three", *a, None, T, acc, 4, 5, 6, 1.0, 0)
    for shape in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (-1, 5, 6)):
        refused(b"shape", u, v, w, nt, T, acc, *shape, 1.0, 1)
    for wgt in (float("nan"), float("inf"), -float("inf")):
        refused(b"finite", u, v, w, nt, T, acc, 4, 5, 6, wgt, 0)
    for span in (2, -1):
        refused(b"span_average", u, v, w, nt, T, acc, 4, 5, 6, 1.0, span)
    # T may be one of u, v, w.  A call that passes validation would launch on these made-up
    # pointers, so the aliasing calls carry one bad argument that is checked after the arrays
    # (the checks run in the order above): they are refused for that argument and not for T.
    for alias in (u, v, w):
        refused(b"span_average", u, v, w, nt, alias, acc, 4, 5, 6, 1.0, 2)
        refused(b"finite", u, v, w, None, alias, acc, 4, 5, 6, float("nan"), 1)
