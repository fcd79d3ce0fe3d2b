"""Plain NumPy statements of the health / diagnostic reductions and of the
per-cell 2-D operators that feed them (host only, no device code).

These are the references of tests/test_gpu_reductions.py and
tests/test_gpu_fields2d_shapes.py; tests/test_diag_host.py checks them on the
CPU against the C oracle, a literal Python loop and ``OracleSolver`` before any
kernel is involved.

* ``fold_absmax``: the kernels' stated maximum (common.hpp: "NaN never wins:
  callers fold with `if (c > m) m = c`", v5.py:220-222).
* ``nonfinite_count``: v5.py:601.
* ``mean64_exact`` / ``energy_mean_exact``: correctly rounded sums
  (``math.fsum``) of the float64 values; the energy of a cell is formed in the
  fields' dtype as NumPy forms it (v5.py:431-432).
* ``vorticity2d``: ``OracleSolver.compute_vorticity`` (v5.py:365-373) for any
  dtype and mask.
* ``divergence2d`` / ``gradient2d`` / ``project2d``: v5.py:178-200, :413-417
  with the constants of oracle/stencil_oracle.c (``cx = dtype(0.5 / dx)``) in
  float32 and float64.

The sizes, shapes and seeded inputs the host and GPU tests share are drawn
here once and handed out read-only.
"""
import functools
import math

import numpy as np

# ------------------------------------------------------------ shared inputs
# Flat sizes: single lanes and waves and their neighbours, one workgroup and
# its neighbours, a ragged size, the last size k_absmax / k_nonfinite cover
# without a grid stride (2048 workgroups of 256), one past it, and two strides
# plus a ragged tail.
GRID1D = 2048 * 256
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, GRID1D, GRID1D + 1, 2 * GRID1D + 77]
# the sums also at the last many-block size of the energy and one past it
# (the atomic path)
ENERGY_ONE_PASS = 1 << 20
SUM_SIZES = SIZES + [ENERGY_ONE_PASS, ENERGY_ONE_PASS + 1]
# 2-D shapes: without an interior, one interior cell, nx around the 64-lane
# wave and the 256-column workgroup, two and five workgroups per row.
SHAPES_2D = [(3, 3), (1, 5), (5, 1), (2, 7), (7, 2), (4, 63), (4, 64), (5, 65), (3, 255), (3, 256), (6, 257),
             (5, 513), (37, 260), (9, 1030)]
DX, DY = 0.013, 0.0171  # dx != dy throughout


def has_interior(shape):
    return shape[0] > 2 and shape[1] > 2


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=16)  # the largest are 8 MB each
def noise(n, dtype, seed=0, lo=-1.0, hi=1.0):
    """Read-only uniform (lo, hi) noise of n values, drawn once per key."""
    rng = np.random.default_rng([n, seed, np.dtype(dtype).itemsize])
    return _frozen(rng.uniform(lo, hi, n).astype(dtype))


@functools.lru_cache(maxsize=None)
def fields2d(shape, dtype, quiescent=False):
    """u, v (read-only) drawn as test_predictor_shapes_bitexact draws them;
    quiescent: u = v = 0 over a patch (the SUPG tau's |V| <= eps branch)."""
    ny, nx = shape
    rng = np.random.default_rng(ny * 1000 + nx)
    u = rng.uniform(-1.5, 1.5, shape).astype(dtype)
    v = rng.uniform(-1.5, 1.5, shape).astype(dtype)
    if quiescent:
        u[ny // 4:ny // 4 + 3, nx // 3:nx // 3 + 70] = 0
        v[ny // 4:ny // 4 + 3, nx // 3:nx // 3 + 70] = 0
    return _frozen(u, v)


def _dtype(*arrays):
    dt = np.asarray(arrays[0]).dtype
    assert dt in (np.float32, np.float64), dt
    for a in arrays[1:]:
        assert np.asarray(a).dtype == dt, (dt, np.asarray(a).dtype)
    return dt.type


def fold_absmax(*arrays, start=0.0):
    """``m = start; for x in |a|: if x > m: m = x`` over every array in turn,
    in the arrays' dtype: NaN never wins, +/-Inf does, -0.0 gives +0.0 (it is
    not > 0), and ``start`` stands when nothing exceeds it."""
    T = _dtype(*arrays)
    m = T(start)
    for a in arrays:
        x = np.abs(np.asarray(a)).ravel()
        x = x[~np.isnan(x)]
        if x.size:
            c = x.max()
            if c > m:
                m = c
    return T(m)


def nonfinite_count(a, b=None):
    """Number of NaN / +Inf / -Inf entries of a, plus those of b."""
    n = int(np.count_nonzero(~np.isfinite(a)))
    if b is not None:
        n += int(np.count_nonzero(~np.isfinite(b)))
    return n


def mean64_exact(a):
    """The correctly rounded float64 sum of a's values, divided by n."""
    x = np.asarray(a, np.float64).ravel()
    return math.fsum(x.tolist()) / x.size


def energy_mean_exact(u, v):
    """Mean of 0.5 (u^2 + v^2): each cell in the fields' dtype as NumPy forms
    it, then the correctly rounded float64 sum, divided by n."""
    T = _dtype(u, v)
    with np.errstate(all="ignore"):
        e = T(0.5) * (u * u + v * v)
    x = e.astype(np.float64).ravel()
    return math.fsum(x.tolist()) / x.size


def vorticity2d(u, v, mask, dx, dy):
    """OracleSolver.compute_vorticity for any dtype: interior central
    differences divided by dtype(2 dx) / dtype(2 dy), ring 0, masked cells NaN
    (ring cells included)."""
    T = _dtype(u, v)
    w = np.zeros_like(u)
    with np.errstate(all="ignore"):
        w[1:-1, 1:-1] = ((v[1:-1, 2:] - v[1:-1, :-2]) / T(2 * dx)
                         - (u[2:, 1:-1] - u[:-2, 1:-1]) / T(2 * dy))
    if mask is not None:
        w[np.asarray(mask, bool)] = np.nan
    return w


def divergence2d(u, v, dx, dy):
    """oracle_divergence2d_f32's statement in u's dtype."""
    T = _dtype(u, v)
    cx, cy = T(0.5 / dx), T(0.5 / dy)
    d = np.zeros_like(u)
    with np.errstate(all="ignore"):
        d[1:-1, 1:-1] = (u[1:-1, 2:] - u[1:-1, :-2]) * cx + (v[2:, 1:-1] - v[:-2, 1:-1]) * cy
    return d


def gradient2d(phi, dx, dy):
    """oracle_gradient2d_f32's statement in phi's dtype: (gx, gy)."""
    T = _dtype(phi)
    cx, cy = T(0.5 / dx), T(0.5 / dy)
    gx, gy = np.zeros_like(phi), np.zeros_like(phi)
    with np.errstate(all="ignore"):
        gx[1:-1, 1:-1] = (phi[1:-1, 2:] - phi[1:-1, :-2]) * cx
        gy[1:-1, 1:-1] = (phi[2:, 1:-1] - phi[:-2, 1:-1]) * cy
    return gx, gy


def project2d(phi, u_star, v_star, dx, dy, dt):
    """k_project's statement (v5.py:413-417): u = u* - dt gx, v = v* - dt gy
    with dt in the fields' dtype, and max sqrt(gx^2 + gy^2) by the fold rule.
    Returns (u, v, gradmax)."""
    T = _dtype(phi, u_star, v_star)
    gx, gy = gradient2d(phi, dx, dy)
    with np.errstate(all="ignore"):
        u = u_star - T(dt) * gx
        v = v_star - T(dt) * gy
        g = np.sqrt(gx * gx + gy * gy)
    return u, v, fold_absmax(g)
