"""NumPy statement of the flow statistics with the passive scalar
(cfd_flow_scalar_stats3d_f32 and statistics() with scalar_moments).

tests/stats3d_reference.py's moments come first (u, v, w, uu, vv, ww, uv, uw,
vw and, when nu_t is given, nu_t), then T, TT, uT, vT, wT: 14 planes, or 15
with nu_t, each formed in float64 from the float32 values (the products are
exact).  The accumulation is that module's: per cell, or the sum over z with
the planes added in order, multiplied by the weight once and added once.
derive adds mean_T, the variance TT and the turbulent heat fluxes uT, vT, wT
to its derive.  stats_bound is reused as it is.
"""
import numpy as np

import stats3d_reference as base
from stats3d_reference import stats_bound  # noqa: F401  (re-exported)

F = np.float32
SCALAR_MOMENTS = ("T", "TT", "uT", "vT", "wT")


def terms(u, v, w, T, nu_t=None):
    """(nm, nz, ny, nx) float64: the moments of every cell, nm = 14 or 15."""
    assert T.dtype == F and T.shape == u.shape
    t = base.terms(u, v, w, nu_t)
    s = T.astype(np.float64)
    return np.concatenate([t, np.stack([s, s * s, t[0] * s, t[1] * s, t[2] * s])])


def accumulate_numpy(sums, u, v, w, T, weight, span_average, nu_t=None):
    """sums += weight * moments (span_average: * their sum over z), in place."""
    return base._accumulate(sums, terms(u, v, w, T, nu_t), weight, span_average)


def abs_terms(sums, u, v, w, T, weight, span_average, nu_t=None):
    """accumulate_numpy with |t| and |weight|: sum of weight |t| per element."""
    return base._accumulate(sums, np.abs(terms(u, v, w, T, nu_t)), abs(weight), span_average)


def derive(sums, weight, nz, span_average):
    """stats3d_reference.derive of the first 9 or 10 planes, then the last
    five over the same norm: mean_T, TT = <TT> - <T><T>, aT = <aT> - <a><T>."""
    sums = np.asarray(sums, np.float64)
    assert sums.shape[0] in (14, 15)
    out = base.derive(sums[:-5], weight, nz, span_average)
    norm = np.float64(weight) * np.float64(nz) if span_average else np.float64(weight)
    m = sums / norm
    k = sums.shape[0] - 5
    out["mean_T"] = m[k]
    out["TT"] = m[k + 1] - m[k] * m[k]
    for q, name in enumerate(("uT", "vT", "wT")):
        out[name] = m[k + 2 + q] - m[q] * m[k]
    return out
