"""Edge-value inputs for the flow-statistics kernels of stats3d.hip and what
tests/test_gpu_stats3d_edges.py compares them with (TEST INFRASTRUCTURE ONLY).

Plain NumPy, no GPU.  The statement is accumulate_numpy of
tests/stats3d_reference.py (9 and 10 moments) and of
tests/scalar_stats3d_reference.py (14 and 15), called under
np.errstate(all="ignore"); tests/test_stats3d_edge_host.py pins it to literal
loops on these classes.

Shapes (nz, ny, nx).  The span kernel gives each of its eight waves a chunk of
ceil(nz / 8) planes, marched two at a time, and a workgroup 64 columns of the
flat (ny, nx) plane: (1, 3, 7) only wave 0 has a plane; (9, 5, 13) n is odd
(the one-cell full kernel), chunks of 2 and a last wave with 1; (12, 5, 13) n
even (the two-cell kernel); (67, 3, 70) chunks of 9 (the unroll tail runs in
every wave), 210 columns in three full tiles and one of 18.

A run is (samples, weights, the accumulator's start); a sample is (u, v, w,
nu_t, T).  Classes (``runs``):

* ``nonfinite``: unit fields with NaN, +Inf or -Inf at one cell of one of the
  five fields per run; the cells go round ``cells_of``: planes 0 and nz-1, the
  first and last plane of a middle wave's chunk and a chunk's tail plane,
  columns 0, 63, 64 and the last one.  One more run has +Inf and -Inf in one
  column of u at two planes.
* ``subnormal``, ``huge``, ``unit``: integers in [-4, 4] times 2^-149, 2^120
  and 1, three samples, weights 1, 1/2, 1/4: every product, z-sum and
  weighted add is an exact float64.  ``huge`` also has +-FLT_MAX cells, one
  per column (FLT_MAX^2 is exact in float64).
* ``signed_zero``: every field -0.0; the accumulator starts at +0.0 and at
  -0.0.
* ``weights``: a unit sample at weight 1, then one at 0, -1, 5e-324 or 1e300,
  on unit fields, on unit fields with an infinite column (0 * Inf = NaN) and,
  for 1e300, on the huge fields (the product overflows).
* ``accumulator``: starts with +Inf, NaN, -0.0 and 1e300 in single elements.
* ``mixed``: 5 N(0, 1) with columns of +-2^100 beside +-2^-100: the result
  depends on the order, the bar is stats_bound.

Bar for every class but ``mixed``: ``same_bits``.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import scalar_stats3d_reference as scalar_ref
import stats3d_reference as base_ref
from poisson_edge_reference import describe_difference, same_bits  # noqa: F401  (re-exported)
from stats3d_reference import stats_bound  # noqa: F401  (re-exported)

F = np.float32
FLT_MAX = np.finfo(F).max
SHAPES = ((1, 3, 7), (9, 5, 13), (12, 5, 13), (67, 3, 70))
COUNTS = (9, 10, 14, 15)
EXACT = ("nonfinite", "subnormal", "huge", "unit", "signed_zero", "weights", "accumulator")
CLASSES = EXACT + ("mixed",)
FIELD_NAMES = ("u", "v", "w", "nu_t", "T")
SCALES = {"subnormal": 2.0 ** -149, "huge": 2.0 ** 120, "unit": 1.0}
WEIGHTS3 = (1.0, 0.5, 0.25)
ODD_WEIGHTS = (0.0, -1.0, 5e-324, 1e300)
REFUSED_WEIGHTS = (np.nan, np.inf, -np.inf)
# the moments that contain each field, by name
MOMENTS = {9: base_ref.MOMENTS[:9], 10: base_ref.MOMENTS,
           14: base_ref.MOMENTS[:9] + scalar_ref.SCALAR_MOMENTS, 15: base_ref.MOMENTS + scalar_ref.SCALAR_MOMENTS}
CONTAINS = {"u": ("u", "uu", "uv", "uw", "uT"), "v": ("v", "vv", "uv", "vw", "vT"),
            "w": ("w", "ww", "uw", "vw", "wT"), "nu_t": ("nu_t",), "T": ("T", "TT", "uT", "vT", "wT")}


class Run(NamedTuple):
    name: str
    samples: tuple       # of (u, v, w, nu_t, T)
    weights: tuple
    start: tuple         # ((flat index or None for every element, value), ...): the accumulator before the run
    planted: tuple       # ((field name, cell), ...)


def acc_shape(shape, nm, span):
    return (nm,) + (tuple(shape[1:]) if span else tuple(shape))


def chunk_of(nz):
    return (nz + 7) // 8


def cells_of(shape):
    """The cells the planted values go round: five planes x four columns."""
    nz, ny, nx = shape
    ch = chunk_of(nz)
    mid = min(3, (nz - 1) // ch)                      # a middle wave that has planes
    planes = [0, nz - 1, mid * ch, min(mid * ch + ch, nz) - 1, min(ch, nz) - 1]
    plane = ny * nx
    cols = [0, min(63, plane - 1), min(64, plane - 1), plane - 1]
    return [(k,) + tuple(int(x) for x in np.unravel_index(p, (ny, nx))) for k in planes for p in cols]


def _ints(rng, shape, scale):
    return tuple((rng.integers(-4, 5, shape).astype(np.float64) * scale).astype(F) for _ in range(5))


def _freeze(run):
    for s in run.samples:
        for a in s:
            a.setflags(write=False)
    return run


@functools.lru_cache(maxsize=None)
def runs(cls, shape):
    """The runs of class ``cls`` on ``shape`` (a tuple of ``Run``, read-only)."""
    assert cls in CLASSES, cls
    rng = np.random.default_rng([8200 + CLASSES.index(cls), *shape])
    nz, ny, nx = shape
    out = []

    def add(name, samples, weights, start=(), planted=()):
        out.append(_freeze(Run(name, tuple(tuple(a.copy() for a in s) for s in samples), tuple(weights), tuple(start),
                               tuple(planted))))

    def exact_samples(scale, n=3):
        return [_ints(rng, shape, scale) for _ in range(n)]

    if cls == "nonfinite":
        base = exact_samples(1.0, 1)[0]
        cells = cells_of(shape)
        add("clean", [base], (0.5,))
        n = 0
        for q, name in enumerate(FIELD_NAMES):
            for val in (np.nan, np.inf, -np.inf):
                s = [a.copy() for a in base]
                cell = cells[(7 * n) % len(cells)]      # 7 and 20 are coprime: the runs spread over planes and columns
                s[q][cell] = val
                add(f"{name} {val!r} at {cell}", [s], (0.5,), planted=[(name, cell)])
                n += 1
        s = [a.copy() for a in base]
        col = cells_of(shape)[-1][1:]
        s[0][(0,) + col] = np.inf
        if nz > 1:
            s[0][(nz - 1,) + col] = -np.inf
        add("u +inf and -inf in one column", [s], (0.5,), planted=[("u", (0,) + col), ("u", (nz - 1,) + col)])
    elif cls in SCALES:
        samples = exact_samples(SCALES[cls])
        if cls == "huge":
            plane = ny * nx
            for n, p in enumerate(range(0, plane, max(1, plane // 10))):
                k, (i, j) = (5 * n) % nz, np.unravel_index(p, (ny, nx))
                samples[n % 3][n % 5][k, i, j] = FLT_MAX if n % 2 else -FLT_MAX
        add(cls, samples, WEIGHTS3)
    elif cls == "signed_zero":
        samples = [tuple(np.full(shape, -0.0, F) for _ in range(5)) for _ in range(2)]
        add("from +0.0", samples, (1.0, 0.5))
        add("from -0.0", samples, (1.0, 0.5), start=[(None, -0.0)])
        add("from -0.0, weight -1", samples, (1.0, -1.0), start=[(None, -0.0)])
    elif cls == "weights":
        unit = exact_samples(1.0, 2)
        infc = [unit[0], [a.copy() for a in unit[1]]]
        cell = cells_of(shape)[-1]
        infc[1][0][cell] = np.inf
        infc[1][4][cell] = -np.inf
        huge = exact_samples(2.0 ** 120, 2)
        for wgt in ODD_WEIGHTS:
            add(f"unit, weight {wgt!r}", unit, (1.0, wgt))
            add(f"infinite column, weight {wgt!r}", infc, (1.0, wgt), planted=[("u", cell), ("T", cell)])
        add("huge, weight 1e300", huge, (1.0, 1e300))
        add("huge, weight 5e-324", huge, (1.0, 5e-324))
    elif cls == "accumulator":
        samples = exact_samples(1.0, 2)
        size = 9 * ny * nx            # within the first nine moments of either mode
        spots = [int(x) for x in rng.choice(size, 4, replace=False)]
        add("odd elements", samples, (1.0, 0.5), start=list(zip(spots, (np.inf, np.nan, -0.0, 1e300))))
        add("clean", samples, (1.0, 0.5))
    else:   # mixed
        samples = []
        for _ in range(2):
            s = [(5 * rng.standard_normal(shape)).astype(F) for _ in range(5)]
            cols = rng.uniform(size=(ny, nx)) < 0.3
            for a in s:
                pick = rng.choice(np.array([2.0 ** 100, -2.0 ** 100, 2.0 ** -100, -2.0 ** -100]), shape).astype(F)
                a[:, cols] = pick[:, cols]
            samples.append(s)
        add("mixed", samples, (2e-5, 7.3e-5))
    return tuple(out)


# ------------------------------------------------------------ the reference
def start_array(run, shape, nm, span):
    acc = np.zeros(acc_shape(shape, nm, span))
    flat = acc.reshape(-1)
    for where, val in run.start:
        if where is None:
            flat[:] = val
        else:
            flat[where] = val
    return acc


def accumulate(acc, sample, weight, nm, span, absolute=False):
    """One sample into ``acc`` through the statement of the moment count."""
    u, v, w, nu_t, T = sample
    nt = nu_t if nm in (10, 15) else None
    with np.errstate(all="ignore"):
        if nm <= 10:
            fn = base_ref.abs_terms if absolute else base_ref.accumulate_numpy
            return fn(acc, u, v, w, weight, span, nt)
        fn = scalar_ref.abs_terms if absolute else scalar_ref.accumulate_numpy
        return fn(acc, u, v, w, T, weight, span, nt)


@functools.lru_cache(maxsize=None)
def reference(cls, shape, index, nm, span):
    """The accumulator after run ``index`` (read-only)."""
    run = runs(cls, shape)[index]
    acc = start_array(run, shape, nm, span)
    for s, wgt in zip(run.samples, run.weights):
        accumulate(acc, s, wgt, nm, span)
    acc.setflags(write=False)
    return acc


@functools.lru_cache(maxsize=None)
def abs_reference(cls, shape, index, nm, span):
    """Sum of |weight| |t| per element of run ``index`` (zero start)."""
    run = runs(cls, shape)[index]
    acc = np.zeros(acc_shape(shape, nm, span))
    for s, wgt in zip(run.samples, run.weights):
        accumulate(acc, s, wgt, nm, span, absolute=True)
    acc.setflags(write=False)
    return acc


def census(a) -> dict:
    x = np.asarray(a, np.float64)
    bits = np.ascontiguousarray(x).view(np.uint64)
    with np.errstate(all="ignore"):
        small = (x != 0) & (np.abs(x) < 2.0 ** -126)
    return {"n": x.size, "finite": int(np.isfinite(x).sum()), "nan": int(np.isnan(x).sum()),
            "inf": int(np.isinf(x).sum()), "neg_zero": int((bits == 1 << 63).sum()),
            "below_flt_min": int(small.sum())}
