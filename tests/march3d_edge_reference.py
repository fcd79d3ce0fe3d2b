"""Edge-value inputs for the 3-D predictor, LES and scalar marches and the
table of what tests/test_gpu_march3d_edges.py runs (TEST INFRASTRUCTURE ONLY).

Plain NumPy, no GPU.  No arithmetic is stated here: every reference is one of
the NumPy statements the suite already pins (tests/ref3d.py,
tests/les3d_reference.py, tests/zper_reference.py,
tests/buoyancy3d_reference.py, tests/scalar3d_reference.py).
tests/test_march3d_edge_host.py checks those statements against literal
per-cell loops on every input class below and asserts that each row of
``CASES`` holds what its class promises; the GPU file then compares every
kernel variant with the statement under ``same_bits``.

Shapes (nz, ny, nx).  ``MARCH`` = (10, 11, 132): the predictor's auto chunk is
8 planes (seams 8 + 2), 11 rows leave a partial tile at 4 and at 8 rows per
tile, 132 columns are three segments at 1 cell per lane (64 + 64 + 4), two at
2 (128 + 4) and one at 4; nz is even, as the periodic entries want.  ``CELL``
= (4, 5, 7): nx odd, so auto takes the per-cell kernels.  ``TINY`` = (3, 3, 3)
has one interior cell (non-periodic entries only: nz is odd).

Input classes (``build``), u, v, w, T, a viscosity array nu and an eddy
viscosity array nu_t each:

* ``nonfinite``: N(0, 1) fields with 48 seeds of NaN, +Inf, -Inf round-robin
  over u, v, w and 16 each in T and nu_t.  On ``MARCH`` the seeds sit on
  ``SEAM_CELLS`` (12 of the 48 on faces), so they are halo cells, cells of a
  row another wave owns, cells of a chunk's D plane and face cells.
* ``signed_zero``: fields drawn from {+0.0, -0.0} with 60 isolated N(0, 1)
  cells per field.
* ``neg_zero``: u, v, w, T, nu_t all -0.0.  The statements give +0.0 on every
  interior cell and copy -0.0 through on the faces.
* ``subnormal``: N(0, 1) * 1e-39 in u, v, w, T, nu_t.
* ``huge``: N(0, 1) fields with a patch of +1e38 in u overlapping one of -1e38
  in v, a block where u = v = w ~ 1.1e19 (each square and the sum of two are
  finite, the sum of three overflows: 1e19 itself would not, 3 * 1e38 <
  FLT_MAX), a block near 3e19 where one square overflows, and T's own +-1e38
  patches.  The patches straddle column 64 and plane 8.
* ``viscosity``: ordinary fields; nu carries bands of 0, -0.01, 3e38, 1e-42,
  +Inf and NaN that cross columns 64 and 128 and plane 8, the velocities are
  scaled by 1e-3 under the 3e38 band (pe is a subnormal quotient there).
  nu_t carries the same bands with 2.5e38 in place of 3e38: alpha + nu_t *
  inv_prt must stay finite for the band not to repeat the +Inf one.  For the
  entries that take a scalar viscosity the class is the list
  ``VISCOSITY_SCALARS`` with ordinary fields.

The ordinary viscosity array nu is positive in every class: a -0.0 viscosity
would keep the Laplacian at -0.0 and with it the interior of ``neg_zero``.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

import buoyancy3d_reference
import les3d_reference
import ref3d
import scalar3d_reference
import zper_reference
from poisson_edge_reference import describe_difference, same_bits  # noqa: F401  (re-exported)
from test_buoyancy3d_host import B, T_REF

F = np.float32
MARCH, CELL, TINY = (10, 11, 132), (4, 5, 7), (3, 3, 3)
SEAM_CELLS = tuple(itertools.product((0, 1, 7, 8, 9), (0, 1, 3, 4, 7, 8, 9, 10),
                                     (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 130, 131)))
CLASSES = ("nonfinite", "signed_zero", "neg_zero", "subnormal", "huge", "viscosity")
VISCOSITY_SCALARS = (F(0.0), F(-0.01), F(3e38), F(1e-42))
VISCOSITY_BANDS = (F(0.0), F(-0.01), F(3e38), F(1e-42), F(np.inf), F(np.nan))

SP = dict(dx=0.013, dy=0.011, dz=0.017)
DT = F(2e-3)
NU, ART, CS = F(0.011), F(0.001), 0.17
ALPHA, INV_PRT = F(0.004), F(1 / 0.85)
B_ONLY_V = (F(0.0), B[1], F(0.0))   # 0 * Inf = NaN in u_star and w_star: there is no shortcut for a zero component
T_ZERO = F(0.0)                     # T - 0 keeps a subnormal or zero T what it is (T - T_REF is -0.25 there)


# ---------------------------------------------------------------- the inputs
@dataclass(frozen=True)
class Inputs:
    u: np.ndarray
    v: np.ndarray
    w: np.ndarray
    T: np.ndarray
    nu: np.ndarray
    nu_t: np.ndarray
    dx: float
    dy: float
    dz: float
    dt: np.float32

    @property
    def shape(self):
        return self.u.shape

    @property
    def sp(self):
        return dict(dx=self.dx, dy=self.dy, dz=self.dz)


def face_cells(shape):
    f = np.ones(shape, bool)
    f[1:-1, 1:-1, 1:-1] = False
    return f


def _seed_positions(rng, shape, n_face, n_inner):
    """Cells for planted values: on MARCH from SEAM_CELLS (faces first), else
    any cells of the shape; no cell twice."""
    if shape == MARCH:
        face = face_cells(shape)
        on = [c for c in SEAM_CELLS if face[c]]
        off = [c for c in SEAM_CELLS if not face[c]]
        pick = [on[i] for i in rng.permutation(len(on))[:n_face]]
        pick += [off[i] for i in rng.permutation(len(off))[:n_inner]]
        return pick
    n = n_face + n_inner
    flat = rng.permutation(int(np.prod(shape)))[:n]
    return [tuple(int(i) for i in np.unravel_index(k, shape)) for k in flat]


def _bands(shape):
    """[(slices, index into VISCOSITY_BANDS)] of MARCH; None elsewhere."""
    if shape != MARCH:
        return None
    return [((slice(1, 3), slice(0, 11), slice(60, 70)), 0),       # 0: 180 interior cells across column 64
            ((slice(3, 5), slice(0, 11), slice(60, 70)), 1),       # -0.01: 180
            ((slice(7, 10), slice(0, 11), slice(58, 72)), 2),      # 3e38: 252, across plane 8 and column 64
            ((slice(1, 5), slice(0, 11), slice(124, 132)), 3),     # 1e-42, across column 128
            ((slice(5, 9), slice(1, 6), slice(124, 131)), 4),      # +Inf: 140, across column 128 and plane 8
            ((slice(5, 9), slice(6, 10), slice(126, 130)), 5)]     # NaN: 64


@functools.lru_cache(maxsize=None)
def build(cls, shape, seed=0) -> Inputs:
    """One deterministic set of inputs of class ``cls``; the arrays are
    read-only."""
    assert cls in CLASSES, cls
    rng = np.random.default_rng(7000 + 100 * CLASSES.index(cls) + 13 * seed + sum(shape))
    size = int(np.prod(shape))
    normal = lambda s=1.0: (rng.standard_normal(shape) * s).astype(F)   # noqa: E731
    nu = (F(0.002) + F(0.02) * rng.random(shape)).astype(F)
    nan, inf = F(np.nan), F(np.inf)
    if cls == "nonfinite":
        u, v, w, T = normal(), normal(), normal(), normal()
        nu_t = (F(1e-2) * rng.random(shape)).astype(F)
        per = 16 if shape == MARCH else max(1, min(16, size // 40))   # seeds per field
        nf = 4 if shape == MARCH else 0                               # of them on faces
        cells = _seed_positions(rng, shape, 5 * nf, 5 * (per - nf))
        on, off = cells[:5 * nf], cells[5 * nf:]
        take = lambda k, n: on[k * nf:(k + n) * nf] + off[k * (per - nf):(k + n) * (per - nf)]   # noqa: E731
        kinds = (nan, inf, -inf)
        for k, c in enumerate(take(0, 3)):          # 12 of the 48 velocity seeds on faces
            (u, v, w)[k % 3][c] = kinds[(k // 3) % 3]
        for k, c in enumerate(take(3, 1)):
            T[c] = kinds[k % 3]
        for k, c in enumerate(take(4, 1)):
            nu_t[c] = kinds[k % 3]
    elif cls in ("signed_zero", "neg_zero"):
        if cls == "neg_zero":
            u, v, w, T, nu_t = (np.full(shape, -0.0, F) for _ in range(5))
        else:
            u, v, w, T, nu_t = (np.where(rng.random(shape) < 0.5, F(-0.0), F(0.0)).astype(F) for _ in range(5))
            n = 60 if shape == MARCH else max(2, size // 30)
            for f in (u, v, w, T, nu_t):
                for c in _seed_positions(rng, shape, n // 6, n - n // 6):
                    f[c] = F(rng.standard_normal())
            nu_t *= F(1e-2)      # a zero keeps its sign
    elif cls == "subnormal":
        u, v, w, T, nu_t = (normal(1e-39) for _ in range(5))
    elif cls == "huge":
        u, v, w, T = normal(), normal(), normal(), normal()
        nu_t = (F(1e-2) * rng.random(shape)).astype(F)
        big = lambda n, base, spread: (base * (1.0 + spread * rng.random(n))).astype(F)   # noqa: E731
        if shape == MARCH:
            pu = (slice(6, 9), slice(2, 6), slice(60, 68))        # +1e38 in u
            pv = (slice(7, 10), slice(4, 8), slice(62, 70))       # -1e38 in v, overlapping it
            b19 = (slice(2, 5), slice(2, 7), slice(122, 130))     # u = v = w ~ 1.1e19
            b3 = (slice(1, 3), slice(7, 10), slice(62, 67))       # ~ 3e19
            tp, tm = (slice(7, 10), slice(1, 4), slice(20, 26)), (slice(7, 10), slice(3, 6), slice(24, 30))
        else:   # every mechanism on a few cells of a tiny shape
            pu, pv, b19, b3, tp, tm = (np.unravel_index(np.arange(k, size, 9), shape) for k in range(6))
        u[pu] = big(u[pu].shape, 1e38, 0.6)
        v[pv] = big(v[pv].shape, -1e38, 0.6)
        for f in (u, v, w):
            f[b19] = big(f[b19].shape, 1.1e19, 0.05)
            f[b3] = big(f[b3].shape, 3e19, 0.05)
        T[tp] = big(T[tp].shape, 1e38, 0.6)
        T[tm] = big(T[tm].shape, -1e38, 0.6)
    else:   # viscosity
        u, v, w, T = normal(), normal(), normal(), normal()
        nu_t = (F(1e-2) * rng.random(shape)).astype(F)
        bands = _bands(shape)
        if bands is None:
            bands = [(np.unravel_index(np.arange(k, size, 7), shape), k) for k in range(6)]
        for where, k in bands:
            nu[where] = VISCOSITY_BANDS[k]
            nu_t[where] = F(2.5e38) if k == 2 else VISCOSITY_BANDS[k]
            if k == 2:
                for f in (u, v, w):
                    f[where] *= F(1e-3)
    for a in (u, v, w, T, nu, nu_t):
        assert a.dtype == F
        a.setflags(write=False)
    return Inputs(u, v, w, T, nu, nu_t, SP["dx"], SP["dy"], SP["dz"], DT)


# ------------------------------------------------------- the table of cases
class Row(NamedTuple):
    entry: str          # a key of ENTRIES
    periodic: bool
    supg: bool
    cls: str
    nu: np.float32      # the scalar viscosity (predictor3d, LES, buoyant) or alpha (scalar advance); unused otherwise
    b: tuple | None     # the buoyancy vector (buoyant entries)
    t_ref: np.float32 | None


class Entry(NamedTuple):
    c_entry: str            # the library's entry point (the periodic form appends _zper before _f32)
    statement: str          # module.function of the NumPy statement that is the reference
    zper_statement: str | None
    outputs: tuple
    array_visc: bool        # takes a viscosity array: the banded class applies


ENTRIES = {
    "predictor3d": Entry("cfd_predictor3d_f32", "ref3d.predictor3d_numpy", "zper_reference.predictor3d_zper_numpy",
                         ("u_star", "v_star", "w_star", "tau"), False),
    "predictor3d_nu": Entry("cfd_predictor3d_nu_f32", "les3d_reference.predictor3d_nu_numpy", None,
                            ("u_star", "v_star", "w_star", "tau"), True),
    "predictor3d_les": Entry("cfd_predictor3d_les_f32", "les3d_reference.predictor3d_les_numpy",
                             "zper_reference.predictor3d_les_zper_numpy",
                             ("u_star", "v_star", "w_star", "tau", "nu_t"), False),
    "smagorinsky3d": Entry("cfd_smagorinsky3d_f32", "les3d_reference.smagorinsky3d_numpy", None, ("nu_t",), False),
    "predictor3d_buoy": Entry("cfd_predictor3d_buoy_f32", "buoyancy3d_reference.predictor3d_buoyant_numpy",
                              "buoyancy3d_reference.predictor3d_buoyant_numpy",
                              ("u_star", "v_star", "w_star", "tau"), False),
    "predictor3d_les_buoy": Entry("cfd_predictor3d_les_buoy_f32", "buoyancy3d_reference.predictor3d_les_buoyant_numpy",
                                  "buoyancy3d_reference.predictor3d_les_buoyant_numpy",
                                  ("u_star", "v_star", "w_star", "tau", "nu_t"), False),
    "scalar_advance3d": Entry("cfd_scalar_advance3d_f32", "scalar3d_reference.scalar_advance3d_numpy",
                              "scalar3d_reference.scalar_advance3d_numpy", ("T_new",), False),
    "scalar_advance3d_nut": Entry("cfd_scalar_advance3d_f32", "scalar3d_reference.scalar_advance3d_numpy",
                                  "scalar3d_reference.scalar_advance3d_numpy", ("T_new",), True),
}
_MODULES = {"ref3d": ref3d, "les3d_reference": les3d_reference, "zper_reference": zper_reference,
            "buoyancy3d_reference": buoyancy3d_reference, "scalar3d_reference": scalar3d_reference}


def statement(row):
    """The NumPy statement (a function of one of the reference modules) that
    is the reference of ``row``."""
    e = ENTRIES[row.entry]
    mod, fn = (e.zper_statement if row.periodic else e.statement).split(".")
    return getattr(_MODULES[mod], fn)


def c_entry(row):
    name = ENTRIES[row.entry].c_entry
    return name.replace("_f32", "_zper_f32") if row.periodic else name


def _rows():
    rows = []
    for name, e in ENTRIES.items():
        buoyant = "buoy" in name
        advance = name.startswith("scalar_advance3d")
        default = ALPHA if advance else NU
        for periodic in ((False, True) if e.zper_statement else (False,)):
            for supg in ((True,) if name == "smagorinsky3d" else (True, False)):
                for cls in CLASSES:
                    if cls == "viscosity" and name == "smagorinsky3d":
                        continue   # it takes no viscosity
                    nus = VISCOSITY_SCALARS if cls == "viscosity" and not e.array_visc else (default,)
                    terms = [(None, None)]
                    if buoyant:
                        terms = [(B, T_REF)]
                        if cls in ("nonfinite", "huge"):
                            terms.append((B_ONLY_V, T_REF))
                        if cls in ("subnormal", "signed_zero", "neg_zero"):
                            terms.append((B, T_ZERO))
                    for nu in nus:
                        for b, t_ref in terms:
                            rows.append(Row(name, periodic, supg, cls, nu, b, t_ref))
    return tuple(rows)


CASES = _rows()


def rows_of(entry, cls):
    return [r for r in CASES if r.entry == entry and r.cls == cls]


def inputs(row, shape) -> Inputs:
    return build(row.cls, shape)


@functools.lru_cache(maxsize=None)
def reference(row, shape):
    """{output name: array} of ``row`` on ``shape``: the row's statement on
    ``build(row.cls, shape)``.  Computed once; the arrays are read-only."""
    c = inputs(row, shape)
    fn = statement(row)
    kw = dict(dt=c.dt, use_supg=row.supg, **c.sp)
    with np.errstate(all="ignore"):
        if row.entry == "predictor3d":
            out = fn(c.u, c.v, c.w, row.nu, **kw)
        elif row.entry == "predictor3d_nu":
            out = fn(c.u, c.v, c.w, c.nu, **kw)
        elif row.entry == "predictor3d_les":
            out = fn(c.u, c.v, c.w, row.nu, ART, CS, **kw)
        elif row.entry == "smagorinsky3d":
            out = {"nu_t": fn(c.u, c.v, c.w, cs=CS, **c.sp)}
        elif row.entry == "predictor3d_buoy":
            out = fn(c.u, c.v, c.w, c.T, row.nu, row.b, row.t_ref, periodic_z=row.periodic, **kw)
        elif row.entry == "predictor3d_les_buoy":
            out = fn(c.u, c.v, c.w, c.T, row.nu, ART, CS, row.b, row.t_ref, periodic_z=row.periodic, **kw)
        else:
            nu_t = c.nu_t if row.entry == "scalar_advance3d_nut" else None
            out = {"T_new": fn(c.T, c.u, c.v, c.w, row.nu, nu_t, INV_PRT, periodic_z=row.periodic, **kw)}
    out = {k: out[k] for k in ENTRIES[row.entry].outputs}
    for a in out.values():
        assert a.dtype == F and a.shape == tuple(shape)
        a.setflags(write=False)
    return out


def source_of(row, name, c):
    """The input an output copies through on the faces (None: tau and nu_t,
    whose faces are 0)."""
    return {"u_star": c.u, "v_star": c.v, "w_star": c.w, "T_new": c.T}.get(name)


# --------------------------------------------------- what a result contains
def interior(a, periodic=False):
    """The cells the operator updates: with periodic z every plane."""
    return a[:, 1:-1, 1:-1] if periodic else a[1:-1, 1:-1, 1:-1]


def census(a, periodic=False) -> dict:
    """Counts and shares over the interior of ``a``: the units the class
    conditions are stated in."""
    x = np.ascontiguousarray(interior(np.asarray(a, F), periodic))
    bits = x.view(np.uint32)
    with np.errstate(all="ignore"):
        sub = (x != 0) & (np.abs(x) < np.finfo(F).tiny)
    n = x.size
    c = {"n": n, "nan": int(np.isnan(x).sum()), "inf": int(np.isinf(x).sum()), "subnormal": int(sub.sum()),
         "neg_zero": int((bits == 0x80000000).sum()), "pos_zero": int((bits == 0).sum()),
         "finite": int(np.isfinite(x).sum())}
    c.update({k + "_share": c[k] / n for k in ("nan", "inf", "subnormal", "neg_zero", "finite")})
    return c
