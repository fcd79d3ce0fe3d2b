"""NumPy statement of the flow statistics (cfd_flow_stats3d_f32 and the
solvers' statistics()).

The moments of a cell are u, v, w, uu, vv, ww, uv, uw, vw and, when nu_t is
given, nu_t, each formed in float64 from the float32 values (a product of two
float32 values is exact in float64).  accumulate_numpy adds one weighted sample
into the running sums: per cell, or as the sum over z with the planes added in
order k = 0 .. nz-1, multiplied by the weight once and added once.  derive
turns the sums into the means, the Reynolds stresses and the turbulent kinetic
energy.  stats_bound is the allowed distance between two evaluations that add
the same exact float64 terms in different orders.
"""
import numpy as np

F = np.float32
MOMENTS = ("u", "v", "w", "uu", "vv", "ww", "uv", "uw", "vw", "nu_t")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def terms(u, v, w, nu_t=None):
    """(nm, nz, ny, nx) float64: the moments of every cell."""
    for a in (u, v, w) + (() if nu_t is None else (nu_t,)):
        assert a.dtype == F and a.ndim == 3
    f = [a.astype(np.float64) for a in (u, v, w)]
    t = f + [f[a] * f[b] for a, b in PAIRS]
    if nu_t is not None:
        t.append(nu_t.astype(np.float64))
    return np.stack(t)


def _accumulate(sums, t, weight, span_average):
    assert sums.dtype == np.float64
    w = np.float64(weight)
    if span_average:
        col = np.zeros(t.shape[:1] + t.shape[2:], np.float64)
        for k in range(t.shape[1]):  # the planes in order
            col = col + t[:, k]
        assert sums.shape == col.shape
        sums += w * col
    else:
        assert sums.shape == t.shape
        sums += w * t
    return sums


def accumulate_numpy(sums, u, v, w, weight, span_average, nu_t=None):
    """sums += weight * moments (span_average: * their sum over z), in place."""
    return _accumulate(sums, terms(u, v, w, nu_t), weight, span_average)


def abs_terms(sums, u, v, w, weight, span_average, nu_t=None):
    """accumulate_numpy with |t| and |weight|: sum of weight |t| per element."""
    return _accumulate(sums, np.abs(terms(u, v, w, nu_t)), abs(weight), span_average)


def derive(sums, weight, nz, span_average):
    """The formulas of statistics(): sums over weight * nz (span_average) or
    weight, stresses <ab> - <a><b>, tke = ((uu + vv) + ww) / 2."""
    norm = np.float64(weight) * np.float64(nz) if span_average else np.float64(weight)
    m = np.asarray(sums, np.float64) / norm
    out = {"weight": float(weight), "mean_u": m[0], "mean_v": m[1], "mean_w": m[2]}
    for q, (a, b) in enumerate(PAIRS):
        out[MOMENTS[3 + q]] = m[3 + q] - m[a] * m[b]
    out["tke"] = 0.5 * ((out["uu"] + out["vv"]) + out["ww"])
    if m.shape[0] == 10:
        out["mean_nu_t"] = m[9]
    return out


def stats_bound(n_terms, samples, abs_sum):
    """|a - b| allowed per element for two evaluations of the same running
    sum: each adds the same exact float64 terms (n_terms - 1 adds, in its own
    order) and rounds one weight product and one accumulation add per sample
    (force_bound's rule in tests/cyl3d_reference.py).  abs_sum: sum of
    weight |t| of the element."""
    return 2.0 * (n_terms + 2 * samples) * 2.0 ** -53 * abs_sum
