"""Edge-value inputs for the 3-D boundary stages and what
tests/test_gpu_bc3d_edges.py compares them with (TEST INFRASTRUCTURE ONLY).

Plain NumPy, no GPU.  No arithmetic is stated here: the references are
channel_bc_ibm3d_numpy (tests/cyl3d_reference.py), channel_bc_ibm3d_zper_numpy
(tests/zper_reference.py) and scalar_bc_heat3d_numpy
(tests/scalar3d_reference.py), called under np.errstate(all="ignore").
tests/test_bc3d_edge_host.py pins them to literal per-cell loops on every case
below and asserts that each class holds what it promises.

Shapes (nz, ny, nx), the smallest that reach every code path of
k_channel_bc_ibm3d: (3, 4, 5) planes 1 and nz-2 are one plane, (4, 5, 6) no
plane between them, (6, 6, 9) all four owner ranges and the clipped box are
non-empty, (8, 12, 40) more than 256 owners (several workgroups add into the
sum).  The periodic forms take the three with an even nz.

Classes (``cases`` for the channel stage, ``heat_cases`` for the scalar's);
each poisons as little as it can:

* ``field_nonfinite``: NaN, +Inf, -Inf in one field per case, at an owner cell
  (1, 1, nx-2) outside the mask (NaN: it must show in column nx-1 and, not
  periodic, in plane 0), at a forced cell of plane nz-2 (+Inf), at a forced
  cell of a middle plane (-Inf), and NaN at cells the stage overwrites (inlet
  column, wall row, column nx-1, planes 0 and nz-1); one more case per field
  has the unforced NaN alone, and every sum stays finite.  Heat: NaN at the
  interior corner (1, 1, nx-2) and at a face cell with a finite sum, then NaN,
  +Inf, -Inf at a heated cell.
* ``signed_zero``: fields of -0.0 and +0.0 in bands, every positive mask cell
  in [0.7, 1] with force_strength 1.5 (m * fs > 1: a negative factor), 0.5 and
  -1.0.
* ``subnormal``: fields k * 2^-149 with some cells just above FLT_MIN, V_inf =
  1e-40 (a subnormal inlet); heat: t_cyl = 1e-40.
* ``huge``: +-FLT_MAX and 3e38 cells under mask cells of 2.0 with
  force_strength 1.5 (factor -2) and -1.0 (factor 3): ``after`` overflows.
  Per case the positive cells are in u, the negative ones in v and both in w:
  the force components are -+Inf of a known sign and NaN (one more case has
  an ordinary w: a finite component beside the two infinite ones).
* ``mask_values``: finite fields; NaN, -0.0, -0.5, 5e-324, 1.0,
  nextafter(1, 0) and 2.0 rotate over ``MASK_SPOTS``: box cells, wall-row
  cells, cells of columns 0, nx-2 and nx-1 and the four plane corners; one more
  case has force_strength +Inf on a mask of +-0.0 with one positive cell (a
  forced zero mask cell would turn NaN).
* ``mask_inf``: one +Inf mask cell in the box and one on a wall row, with
  force_strength 0 (factor NaN) and 0.5 (factor -Inf, 0 * -Inf = NaN).
* ``ramp``: finite fields (bands scaled by 2^-25 .. 2^-40, so that the float64
  sums of the terms round), force_strength from ``RAMP``.
* ``inlet``: steps 1, 999, 1000, 1001, 2^31 - 1 with NaN and +Inf rows of y;
  heat: t_in = 1e40 (+Inf as float32), 1e-45, -0.0, NaN.
* ``preset``: the sum output starts at 1.0, -0.0, +Inf, NaN; finite terms, a
  NaN term with start 1.0, and force_strength 0 (the sum keeps its bits).

The sums.  ``reference`` returns the float64 terms themselves (force: before -
after per component, heat: after - before); ``sum_rule`` turns them into what
any summation order must give: NaN when a term is NaN or both infinities
occur, the infinity when only one sign occurs, else the statement's sum
within force_bound / heat_bound (a finite preset counts as one more term).
Finite partial sums cannot overflow: |t| < 2^129 and n is a few thousand.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from cyl3d_reference import channel_bc_ibm3d_numpy, force_bound
from poisson_edge_reference import describe_difference, same_bits  # noqa: F401  (re-exported)
from scalar3d_reference import face_mask, heat_bound, scalar_bc_heat3d_numpy
from zper_reference import channel_bc_ibm3d_zper_numpy

F = np.float32
FLT_MAX, FLT_MIN = np.finfo(F).max, np.finfo(F).tiny
NONPERIODIC = ((3, 4, 5), (4, 5, 6), (6, 6, 9), (8, 12, 40))
PERIODIC = ((4, 5, 6), (6, 6, 9), (8, 12, 40))
SHAPES = tuple((s, False) for s in NONPERIODIC) + tuple((s, True) for s in PERIODIC)
CLASSES = ("field_nonfinite", "signed_zero", "subnormal", "huge", "mask_values", "mask_inf", "ramp", "inlet",
           "preset")
Y_MAX, V_INF, STEP = 3.0, 1.25, 7
T_IN, T_CYL = 0.25, 1.5
RAMP = (1 / 7, 3 / 7, 7 / 200, 199 / 200, 1 / 3, float(np.nextafter(1.0, 0.0)), 5e-324, 1.5, -1.0)
INLET_STEPS = (1, 999, 1000, 1001, 2 ** 31 - 1)
MASK_VALUES = (np.nan, -0.0, -0.5, 5e-324, 1.0, float(np.nextafter(1.0, 0.0)), 2.0)
HEAT_T_IN = (1e40, 1e-45, -0.0, np.nan)
PRESETS = (1.0, -0.0, np.inf, np.nan)


class Case(NamedTuple):
    name: str
    u: np.ndarray
    v: np.ndarray
    w: np.ndarray
    y: np.ndarray
    mask: np.ndarray
    v_inf: float
    step: int
    fs: float
    preset: float       # every element of force_out before the call
    planted: tuple      # ((field index, cell, "survives" | "vanishes" | "vanishes if not periodic"), ...)


class HeatCase(NamedTuple):
    name: str
    T: np.ndarray
    mask: np.ndarray
    t_in: float
    t_cyl: float
    fs: float
    preset: float
    planted: tuple      # ((cell, "survives" | "vanishes" | "corner"), ...)


# ---------------------------------------------------------------- the inputs
def _rng(cls, shape, salt=0):
    return np.random.default_rng([9100 + 10 * CLASSES.index(cls) + salt, *shape])


def corner_mask(rng, ny, nx):
    """bc_case's mask of tests/test_gpu_fields3d_shapes.py: positive on about
    a third of the plane, with cells of rows 0 and ny-1, of columns 0, nx-2
    and nx-1 and the four plane corners among them."""
    m = np.where(rng.uniform(size=(ny, nx)) < 0.33, rng.uniform(0.05, 1, (ny, nx)), 0.0)
    m[0, 0], m[0, nx // 2], m[ny - 1, nx - 1], m[ny - 1, 1] = 0.5, 0.25, 0.75, 1.0
    m[1, 0], m[1, nx - 2], m[1, nx - 1], m[ny - 2, nx - 2] = 0.125, 0.3, 0.6, 0.9
    m[0, nx - 1], m[ny - 1, 0] = 0.4, 0.35
    return m


def inner_mask(rng, ny, nx):
    """Positive only on rows 1 .. ny-2 and columns 1 .. nx-3 (the tight box
    lies inside the plane), always at (1, 1) and (ny-2, 2)."""
    m = np.zeros((ny, nx))
    inner = np.where(rng.uniform(size=(ny - 2, nx - 3)) < 0.4, rng.uniform(0.05, 1, (ny - 2, nx - 3)), 0.0)
    m[1:-1, 1:-2] = inner
    m[1, 1], m[ny - 2, 2] = 0.75, 0.5
    return m


def mask_spots(ny, nx):
    """Where ``mask_values`` puts its values: the four plane corners, two
    wall-row cells, cells of columns 0, nx-2 and nx-1, three box cells."""
    return ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (0, nx // 2), (ny - 1, 1), (1, 0), (ny - 2, 0),
            (1, nx - 2), (ny - 2, nx - 2), (1, nx - 1), (ny - 2, nx - 1), (1, 1), (ny - 2, 2), (1, 2))


def _fields(rng, shape, n=3):
    return [rng.uniform(-3, 3, shape).astype(F) for _ in range(n)]


def _zero_bands(shape, phase):
    k, i, j = np.indices(shape)
    return np.where((k + i // 2 + j // 3 + phase) % 2 == 0, F(-0.0), F(0.0)).astype(F)


def _subnormal_field(rng, shape):
    f = (rng.integers(-4000, 4001, shape).astype(np.float64) * 2.0 ** -149).astype(F)
    near = rng.uniform(size=shape) < 0.2
    f[near] = (np.sign(rng.uniform(-1, 1, shape)) * FLT_MIN * (1 + rng.uniform(0, 0.5, shape))).astype(F)[near]
    return f


def _zero_mask(ny, nx):
    """+0.0 and -0.0 in a checkerboard, 1.0 at (1, 1) alone."""
    i, j = np.indices((ny, nx))
    m = np.where((i + j) % 2 == 0, -0.0, 0.0)
    m[1, 1] = 1.0
    return m


def _mid_plane(nz):
    return nz // 2 if nz > 4 else 1


def _freeze(c):
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def cases(cls, shape, periodic=False):
    """The channel stage's cases of class ``cls`` (a tuple of ``Case``, the
    arrays read-only).  The inputs do not depend on ``periodic``."""
    assert cls in CLASSES, cls
    nz, ny, nx = shape
    rng = _rng(cls, shape)
    y = np.linspace(-1.0, Y_MAX, ny)
    out = []

    def add(name, f, m, fs, *, yy=y, v_inf=V_INF, step=STEP, preset=0.0, planted=()):
        out.append(_freeze(Case(name, f[0].copy(), f[1].copy(), f[2].copy(), yy.copy(), np.array(m, np.float64),
                                float(v_inf), int(step), float(fs), float(preset), tuple(planted))))

    if cls == "field_nonfinite":
        m = inner_mask(rng, ny, nx)
        m[1, nx - 2] = m[1, nx - 1] = 0.0
        base = _fields(rng, shape)
        for q, name in enumerate("uvw"):
            for fs in (0.5, 1.5):
                f = [a.copy() for a in base]
                planted = [(q, (1, 1, nx - 2), "survives"), (q, (nz - 2, ny - 2, 2), "survives"),
                           (q, (_mid_plane(nz), 1, 1), "survives"), (q, (1, 1, 0), "vanishes"),
                           (q, (1, 0, 2), "vanishes"), (q, (nz - 2, ny - 2, nx - 1), "vanishes"),
                           (q, (0, ny - 2, 1), "vanishes if not periodic"),
                           (q, (nz - 1, 1, 2), "vanishes if not periodic")]
                for (_, cell, _), val in zip(planted, (np.nan, np.inf, -np.inf) + (np.nan,) * 5):
                    f[q][cell] = val
                add(f"{name} fs={fs}", f, m, fs, planted=planted)
            # the NaN outside the mask alone: it is copied and no term of any sum
            f = [a.copy() for a in base]
            planted = [p for p in planted if p[1][2] in (nx - 2, 0, nx - 1) or p[1][1] == 0][:4]
            for _, cell, _ in planted:
                f[q][cell] = np.nan
            add(f"{name} survivor only", f, m, 0.5, planted=planted)
    elif cls == "signed_zero":
        m = corner_mask(rng, ny, nx)
        m[m > 0] = rng.uniform(0.7, 1.0, int((m > 0).sum()))
        f = [_zero_bands(shape, p) for p in range(3)]
        for fs in (1.5, 0.5, -1.0):
            add(f"fs={fs}", f, m, fs)
    elif cls == "subnormal":
        m = corner_mask(rng, ny, nx)
        f = [_subnormal_field(rng, shape) for _ in range(3)]
        for fs in (1 / 3, 0.5, 1.5):
            add(f"fs={fs}", f, m, fs, v_inf=1e-40)
    elif cls == "huge":
        m = inner_mask(rng, ny, nx)
        spots = [(1, 1), (ny - 2, 2), (1, nx - 2)]
        for s in spots:
            m[s] = 2.0
        f = _fields(rng, shape)
        vals = (FLT_MAX, F(3e38), FLT_MAX)
        for k in range(nz):
            for s, val in zip(spots, vals):
                if (k + s[1]) % 2 == 0:
                    f[0][(k, *s)] = val
                    f[1][(k, *s)] = -val
                    f[2][(k, *s)] = val if k % 4 < 2 else -val
        f[2][(1, *spots[0])], f[2][(nz - 2, *spots[1])] = FLT_MAX, -FLT_MAX   # both signs, whatever nz
        f[0][(1, *spots[0])], f[1][(1, *spots[0])] = FLT_MAX, -FLT_MAX
        for fs in (1.5, -1.0):
            add(f"fs={fs}", f, m, fs)
        add("fs=1.5, w ordinary", f[:2] + _fields(rng, shape, 1), m, 1.5)      # a finite component
    elif cls == "mask_values":
        f = _fields(rng, shape)
        base = corner_mask(rng, ny, nx)
        spots = mask_spots(ny, nx)
        for r in range(len(MASK_VALUES)):
            m = base.copy()
            for n, s in enumerate(spots):
                m[s] = MASK_VALUES[(n + r) % len(MASK_VALUES)]
            add(f"rotation {r}", f, m, 0.75)
        add("zeros, fs=inf", f, _zero_mask(ny, nx), np.inf)   # 1 - 0 * Inf is NaN: no zero mask cell may be forced
    elif cls == "mask_inf":
        f = _fields(rng, shape)
        m = corner_mask(rng, ny, nx)
        m[1, 1] = m[0, nx // 2] = np.inf
        for fs in (0.0, 0.5):
            add(f"fs={fs}", f, m, fs)
    elif cls == "ramp":
        f = _fields(rng, shape)
        f[1][:, :, ::2] *= F(2.0 ** -25)     # exponents far apart: the float64 sums of the terms round
        f[2][::2] *= F(2.0 ** -40)
        m = corner_mask(rng, ny, nx)
        for fs in RAMP:
            add(f"fs={fs!r}", f, m, fs)
    elif cls == "inlet":
        f = _fields(rng, shape)
        m = corner_mask(rng, ny, nx)
        yy = y.copy()
        yy[0], yy[ny - 1], yy[ny - 2] = np.nan, np.inf, np.inf     # wall rows stay 0 whatever their y
        if ny >= 5:
            yy[1] = np.nan
        for step in INLET_STEPS:
            add(f"step={step}", f, m, 0.5, yy=yy, step=step)
    else:   # preset
        f = _fields(rng, shape)
        m = inner_mask(rng, ny, nx)
        for p in PRESETS:
            add(f"start {p!r}", f, m, 3 / 7, preset=p)
        g = [a.copy() for a in f]
        g[0][_mid_plane(nz), 1, 1] = np.nan     # a forced cell: a NaN term of u alone
        add("start 1.0, NaN term", g, m, 3 / 7, preset=1.0, planted=[(0, (_mid_plane(nz), 1, 1), "survives")])
        for p in (1.0, -0.0):
            add(f"start {p!r}, fs=0", f, m, 0.0, preset=p)
        add("start 1.0, fs=0, corner mask", f, corner_mask(rng, ny, nx), 0.0, preset=1.0)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def heat_cases(cls, shape, periodic=False):
    """The scalar stage's cases of class ``cls`` (a tuple of ``HeatCase``)."""
    assert cls in CLASSES, cls
    nz, ny, nx = shape
    rng = _rng(cls, shape, salt=5)
    out = []

    def add(name, T, m, fs, *, t_in=T_IN, t_cyl=T_CYL, preset=0.0, planted=()):
        out.append(_freeze(HeatCase(name, T.copy(), np.array(m, np.float64), float(t_in), float(t_cyl), float(fs),
                                    float(preset), tuple(planted))))

    def heat_mask():
        m = corner_mask(rng, ny, nx)
        m[1, 1], m[ny - 2, 2] = 0.75, 0.5       # heated whatever the draw
        return m

    T0 = rng.uniform(0, 1, shape).astype(F)
    hot = (nz - 2, ny - 2, 2)
    if cls == "field_nonfinite":
        m = heat_mask()
        m[1, nx - 2] = 0.0
        T = T0.copy()
        T[1, 1, nx - 2] = T[1, 0, 2] = np.nan
        add("corner and face", T, m, 0.5, planted=[((1, 1, nx - 2), "corner"), ((1, 0, 2), "vanishes")])
        for val in (np.nan, np.inf, -np.inf):
            T = T0.copy()
            T[hot] = val
            add(f"heated cell {val!r}", T, m, 0.5, planted=[(hot, "survives")])
    elif cls == "signed_zero":
        m = heat_mask()
        T = _zero_bands(shape, 1)
        for t_cyl in (0.0, -0.0):
            for fs in (0.5, -1.0):
                add(f"t_cyl={t_cyl!r} fs={fs}", T, m, fs, t_in=-0.0, t_cyl=t_cyl)
    elif cls == "subnormal":
        m = heat_mask()
        T = _subnormal_field(rng, shape)
        for fs in (1 / 3, 0.5):
            add(f"fs={fs}", T, m, fs, t_in=1e-45, t_cyl=1e-40)
    elif cls == "huge":
        m = heat_mask()
        spots = [(1, 1), (ny - 2, 2)]
        for sign, name in ((1.0, "positive"), (-1.0, "negative"), (0.0, "both")):
            T = T0.copy()
            mm = m.copy()
            for n, s in enumerate(spots):
                mm[s] = 2.0
                for k in range(0 if periodic else 1, nz if periodic else nz - 1):
                    sg = sign if sign else (1.0 if (k + n) % 2 == 0 else -1.0)
                    T[(k, *s)] = sg * (FLT_MAX if (k + n) % 3 else F(3e38))
            for fs in (1.5, -1.0):
                add(f"{name} fs={fs}", T, mm, fs, t_cyl=-3e38 * (sign if sign else 1.0))
        m = m.copy()
        m[1, nx - 2] = 0.0
        T = T0.copy()
        T[1, 1, nx - 2] = FLT_MAX       # not heated: the faces copy it, the sum is finite
        add("corner fs=1.5", T, m, 1.5)
    elif cls == "mask_values":
        base = heat_mask()
        spots = mask_spots(ny, nx)
        for r in range(len(MASK_VALUES)):
            m = base.copy()
            for n, s in enumerate(spots):
                m[s] = MASK_VALUES[(n + r) % len(MASK_VALUES)]
            add(f"rotation {r}", T0, m, 0.75)
        add("zeros, fs=inf", T0, _zero_mask(ny, nx), np.inf)
    elif cls == "mask_inf":
        m = heat_mask()
        m[1, 1] = m[0, nx // 2] = np.inf
        for fs in (0.0, 0.5):
            add(f"fs={fs}", T0, m, fs)
    elif cls == "ramp":
        m = heat_mask()
        T = T0.copy()
        T[:, :, ::2] *= F(2.0 ** -30)        # exponents far apart: the float64 sum of the terms rounds
        for fs in RAMP:
            add(f"fs={fs!r}", T, m, fs)
    elif cls == "inlet":
        m = heat_mask()
        for t_in in HEAT_T_IN:
            add(f"t_in={t_in!r}", T0, m, 0.5, t_in=t_in)
    else:   # preset
        m = heat_mask()
        for p in PRESETS:
            add(f"start {p!r}", T0, m, 3 / 7, preset=p)
        T = T0.copy()
        T[hot] = np.nan
        add("start 1.0, NaN term", T, m, 3 / 7, preset=1.0, planted=[(hot, "survives")])
        for p in (1.0, -0.0):
            add(f"start {p!r}, fs=0", T0, m, 0.0, preset=p)
    return tuple(out)


# ------------------------------------------------------------ the references
def statement(periodic):
    return channel_bc_ibm3d_zper_numpy if periodic else channel_bc_ibm3d_numpy


def _run(c, periodic, mask):
    f = [c.u.copy(), c.v.copy(), c.w.copy()]
    with np.errstate(all="ignore"):
        stats = statement(periodic)(*f, c.y, mask, Y_MAX, c.v_inf, c.step, c.fs)
    return f, stats


@functools.lru_cache(maxsize=None)
def reference(cls, shape, periodic, index):
    """Case ``index`` of the class through the statement: {"fields": [u, v,
    w], "stats": its return value, "terms": [before - after of u, v, w] as
    float64 (nz, cells with mask > 0), "unforced": the fields of the same call
    without a mask}.  Read-only."""
    c = cases(cls, shape, periodic)[index]
    fields, stats = _run(c, periodic, c.mask)
    unforced, _ = _run(c, periodic, None)
    sel = c.mask > 0
    with np.errstate(all="ignore"):
        terms = [b[:, sel].astype(np.float64) - a[:, sel].astype(np.float64) for b, a in zip(unforced, fields)]
    for a in fields + unforced + terms:
        a.setflags(write=False)
    return {"fields": fields, "stats": stats, "terms": terms, "unforced": unforced}


@functools.lru_cache(maxsize=None)
def heat_reference(cls, shape, periodic, index):
    """{"T", "stats", "terms": after - before of the heated cells as float64,
    "unheated": T of the same call without a mask}."""
    c = heat_cases(cls, shape, periodic)[index]
    T, bare = c.T.copy(), c.T.copy()
    with np.errstate(all="ignore"):
        stats = scalar_bc_heat3d_numpy(T, c.mask, c.t_in, c.t_cyl, c.fs, periodic)
        scalar_bc_heat3d_numpy(bare, None, c.t_in, c.t_cyl, c.fs, periodic)
        sel = np.broadcast_to(c.mask > 0, shape) & ~face_mask(shape, periodic)
        terms = T[sel].astype(np.float64) - c.T[sel].astype(np.float64)
    for a in (T, bare, terms):
        a.setflags(write=False)
    return {"T": T, "stats": stats, "terms": terms, "unheated": bare}


# ------------------------------------------------------------- the sum rule
def sum_rule(terms, preset, stats, bound_of, reference_sum):
    """What ``preset`` plus the terms must give in any order: ("nan",),
    ("inf", +-inf) or ("finite", the statement's sum plus the preset, the
    allowed distance).  A finite preset is one more term: n + 1 terms of
    magnitude abs + |preset|."""
    t = np.append(np.asarray(terms, np.float64).ravel(), np.float64(preset))
    pos, neg = bool(np.any(t == np.inf)), bool(np.any(t == -np.inf))
    if np.isnan(t).any() or (pos and neg):
        return ("nan",)
    if pos or neg:
        return ("inf", np.inf if pos else -np.inf)
    s = {"n": int(stats["n"]) + 1, "abs": float(np.sum(np.abs(t)))}
    return ("finite", float(reference_sum) + float(preset), bound_of(s))


def force_rule(ref, preset, q):
    """sum_rule of component ``q`` of a channel reference."""
    st = ref["stats"]
    return sum_rule(ref["terms"][q], preset, {"n": ref["terms"][q].size}, force_bound, st["force"][q])


def heat_rule(ref, preset):
    return sum_rule(ref["terms"], preset, {"n": ref["terms"].size}, heat_bound, ref["stats"]["heat"])


def obeys(value, rule):
    """(ok, err / bound or None) of a computed sum under a rule."""
    value = float(value)
    if rule[0] == "nan":
        return bool(np.isnan(value)), None
    if rule[0] == "inf":
        return value == rule[1], None
    err = abs(value - rule[1])
    if rule[2] == 0.0:
        return err == 0.0, 0.0
    return err <= rule[2], err / rule[2]


# --------------------------------------------------- what a result contains
def census(a) -> dict:
    """Counts over every cell of the float32 array ``a``."""
    x = np.ascontiguousarray(np.asarray(a, F))
    bits = x.view(np.uint32)
    with np.errstate(all="ignore"):
        sub = (x != 0) & (np.abs(x) < FLT_MIN)
    return {"n": x.size, "finite": int(np.isfinite(x).sum()), "nan": int(np.isnan(x).sum()),
            "inf": int(np.isinf(x).sum()), "neg_zero": int((bits == 0x80000000).sum()),
            "subnormal": int(sub.sum())}
