"""Edge-value inputs and independent references for the Poisson solves.

Plain NumPy, no GPU.  tests/test_poisson_edge_host.py checks the C oracle
against the statements below on every input class and asserts that each case
of tests/test_gpu_poisson_edges.py exercises what it claims to; the GPU file
then compares every dispatch route with the oracle under ``same_bits``.

Input classes (``build``):

* ``nonfinite``: ordinary fields with a few NaN, +Inf and -Inf cells in div
  and phi0: in the interior, on phi0's boundary ring, next to a solid cell and
  in solid cells.  ``nan_only`` keeps the NaN seeds alone (an infinite change
  counts in the stop rule, a NaN one does not).
* ``signed_zero``: phi0 and div drawn from {+0.0, -0.0}, a band of -0.0 that
  the operator keeps at -0.0, and a few isolated non-zero cells.
* ``neg_zero``: phi0 all -0.0, div all +0.0.
* ``subnormal``: |phi0| ~ 1e-39, |div| ~ 1e-41 (1e-310 / 1e-320 in float64)
  with dx = dt = 1, so every value stays subnormal.
* ``huge``: ordinary fields with patches of +-1e38 (1e308): the neighbour sum
  overflows inside a patch and not on its rim, and the +Inf and -Inf fronts of
  adjacent patches meet as NaN.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

CLASSES = ("nonfinite", "signed_zero", "neg_zero", "subnormal", "huge")


# ---------------------------------------------------------------- comparison
def same_bits(got, want) -> bool:
    """dtype and shape equal, NaNs at the same positions (payload and sign not
    compared: x86 produces the negative default NaN, the GPU the positive
    one), every other value bit for bit: -0.0 != +0.0."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    g = np.ascontiguousarray(got).view(u)
    w = np.ascontiguousarray(want).view(u)
    return bool(np.all((g == w) | gn))


def describe_difference(got, want) -> str:
    """A short account of where two arrays differ under ``same_bits``."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype}{got.shape} against {want.dtype}{want.shape}"
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(want).view(u)))
    idx = np.argwhere(bad)
    head = ", ".join(f"{tuple(int(i) for i in k)}: {got[tuple(k)]!r} != {want[tuple(k)]!r}" for k in idx[:4])
    return f"{len(idx)} of {want.size} cells differ ({int((gn != wn).sum())} by NaN position); {head}"


def fold_max(old, new):
    """The library's max-change fold over two successive states: start at 0,
    ``if (c > m) m = c`` with c = |new - old|: a NaN change never raises it,
    an infinite one does, an all-NaN step gives 0.  (np.abs(a - b).max()
    would propagate the NaN.)"""
    with np.errstate(all="ignore"):
        ch = np.abs(np.asarray(new) - np.asarray(old)).ravel()
    m = old.dtype.type(0)
    if ch.size:
        m = np.fmax.reduce(ch, initial=m)   # fmax drops a NaN operand
    return old.dtype.type(m)


# ---------------------------------------------------------------- the inputs
@dataclass(frozen=True)
class Case:
    div: np.ndarray
    phi0: np.ndarray
    mask: np.ndarray | None      # bool, the fields' shape
    dx: float
    dy: float
    dz: float
    dt: np.float32

    @property
    def shape(self):
        return self.div.shape


def _at(shape, frac, off=None):
    """The interior cell at the fractional position ``frac`` (plus ``off``)."""
    idx = [min(max(1, int(round(f * (n - 1)))), n - 2) for f, n in zip(frac, shape)]
    if off is not None:
        idx = [min(max(0, i + o), n - 1) for i, o, n in zip(idx, off, shape)]
    return tuple(idx)


def _frac(nd, fy, fx, fz=0.5):
    return (fz, fy, fx)[3 - nd:]


def _east(nd, k=1):
    return (0,) * (nd - 1) + (k,)


def _base_mask(rng, shape):
    """Scattered solid cells (3 %), among them boundary-ring cells, as the
    existing persistent-solve tests place them."""
    m = rng.random(shape) < 0.03
    nd = len(shape)
    ny, nx = shape[-2], shape[-1]
    lead = (shape[0] // 2,) if nd == 3 else ()
    m[lead + (0, min(5, nx - 1))] = True
    m[lead + (ny - 1, min(7, nx - 1))] = True
    m[lead + (ny // 2, 0)] = True
    return m


def build(cls, shape, dtype=np.float32, seed=0, masked=True, op="jacobi", nan_only=False, sparse=False,
          mask2d=False) -> Case:
    """One deterministic case of class ``cls``.  ``op`` ("jacobi" or "gs")
    only matters to ``signed_zero``: the sign of div that keeps a -0.0 cell at
    -0.0 differs between the two operators (the GS right side is -div / dt).
    ``sparse`` leaves out the interior infinite seeds of ``nonfinite`` and the
    second pair of patches of ``huge`` (for solves of many iterations: a
    non-finite value spreads one cell per Jacobi sweep, two per GS iteration).
    ``mask2d`` (3-D): the same solid cells in every plane."""
    assert cls in CLASSES, cls
    dtype = np.dtype(dtype)
    T = dtype.type
    f32 = dtype == np.float32
    nd = len(shape)
    rng = np.random.default_rng(1000 * CLASSES.index(cls) + 17 * seed + nd)
    mask = _base_mask(rng, shape) if masked else None
    dx, dy, dz, dt = 0.05, 0.04, 0.06, np.float32(1e-2)
    nan, inf = T(np.nan), T(np.inf)

    if cls == "nonfinite":
        div = (rng.standard_normal(shape) * 1e-3).astype(dtype)
        phi0 = (rng.standard_normal(shape) * 1e-4).astype(dtype)
        a = _at(shape, _frac(nd, 0.3, 0.2))
        phi0[a] = nan                                           # interior NaN in phi0
        b = _at(shape, _frac(nd, 0.65, 0.12, 0.3))
        div[b] = nan                                            # interior NaN in div, in a free cell
        if masked:
            mask[b] = False
        if not nan_only and not sparse:
            div[_at(shape, _frac(nd, 0.7, 0.5, 0.7))] = -inf
            phi0[_at(shape, _frac(nd, 0.35, 0.8, 0.3))] = -inf
            phi0[_at(shape, _frac(nd, 0.8, 0.85, 0.7))] = inf
        # the boundary ring of phi0 (held by every solve)
        ring = list(_at(shape, _frac(nd, 0.0, 0.6)))
        ring[-2] = 0
        phi0[tuple(ring)] = nan if nan_only else inf
        ring = list(_at(shape, _frac(nd, 0.5, 0.0)))
        ring[-1] = shape[-1] - 1
        phi0[tuple(ring)] = nan if nan_only else -inf
        if masked:
            mask[a] = False
            mask[_at(shape, _frac(nd, 0.3, 0.2), _east(nd))] = True      # a solid cell beside a NaN
            own = _at(shape, _frac(nd, 0.5, 0.35))
            mask[own] = True                                             # a solid cell that is non-finite itself
            phi0[own] = nan
            div[own] = nan if nan_only else inf
            for k in (-1, 1):
                mask[_at(shape, _frac(nd, 0.5, 0.35), _east(nd, k))] = False
    elif cls in ("signed_zero", "neg_zero"):
        band = int(0.6 * shape[-1])
        if masked:
            # a solid cell becomes +0.0 under Jacobi and eats into the -0.0 cells
            # around it, one cell per sweep: keep the band's interior free of them
            mask[(slice(1, -1),) * (nd - 1) + (slice(1, band),)] = False
        if cls == "neg_zero":
            phi0 = np.full(shape, -0.0, dtype)
            div = np.zeros(shape, dtype)
        else:
            phi0 = np.where(rng.random(shape) < 0.5, T(-0.0), T(0.0)).astype(dtype)
            div = np.where(rng.random(shape) < 0.5, T(-0.0), T(0.0)).astype(dtype)
            phi0[..., :band] = T(-0.0)
            div[..., :band] = T(0.0) if op == "jacobi" else T(-0.0)
            phi0[_at(shape, _frac(nd, 0.3, 0.85))] = T(1.5)
            div[_at(shape, _frac(nd, 0.7, 0.8, 0.3))] = T(-2e-3)
            phi0[_at(shape, _frac(nd, 0.5, 0.05, 0.7))] = T(-0.75)
    elif cls == "subnormal":
        ps, ds = (1e-39, 1e-41) if f32 else (1e-310, 1e-320)
        sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        phi0 = (sign * ps * (0.5 + rng.random(shape))).astype(dtype)
        div = (ds * (rng.random(shape) - 0.5) * 2).astype(dtype)
        dx = dy = dz = 1.0
        dt = np.float32(1.0)
    elif cls == "huge":
        big = 1e38 if f32 else 1e308
        div = (rng.standard_normal(shape) * 1e-3).astype(dtype)
        phi0 = rng.standard_normal(shape).astype(dtype)
        # two adjacent 5 x 5 patches (3 planes in 3-D) of opposite sign, twice
        for fy, fx, fz in ((0.3, 0.3, 0.4), (0.7, 0.75, 0.6))[:1 if sparse else 2]:
            c = _at(shape, _frac(nd, fy, fx, fz))
            for sgn, x0 in ((1.0, c[-1] - 5), (-1.0, c[-1])):
                sl = [slice(max(0, i - 2), i + 3) for i in c[:-1]] + [slice(max(0, x0), max(0, x0) + 5)]
                if nd == 3:
                    sl[0] = slice(max(0, c[0] - 1), c[0] + 2)
                n = phi0[tuple(sl)].shape
                phi0[tuple(sl)] = (sgn * big * (1.0 + 0.6 * rng.random(n))).astype(dtype)
                if masked:
                    mask[tuple(sl)] = False
    for a in (div, phi0):
        a.setflags(write=False)
    if mask is not None and mask2d and nd == 3:
        mask = np.broadcast_to(mask[_at(shape, _frac(nd, 0.5, 0.5))[0]], shape).copy()
    if mask is not None:
        mask.setflags(write=False)
    return Case(div, phi0, mask, dx, dy, dz, dt)


# ------------------------------------------- independent statements: Jacobi
def jacobi2d_statement(div, phi0=None, *, dx, dt, iters, mask=None):
    """v5.py:336-346 in the reference's own array form, from an initial guess,
    in div's dtype: phi_new = phi.copy(); the interior assignment;
    phi_new[mask] = 0.  (oracle.jacobi2d_numpy's idea, with phi0.)"""
    f32 = div.dtype == np.float32
    with np.errstate(all="ignore"):
        dx2 = np.float32(dx * dx) if f32 else dx * dx          # NEP 50: the Python float meets a float32 array
        dtv = np.float32(dt) if f32 else np.float64(np.float32(dt))
        rhs = (dx2 * div) / dtv
        phi = np.zeros_like(div) if phi0 is None else np.array(phi0, dtype=div.dtype)
        for _ in range(iters):
            phi_new = phi.copy()
            phi_new[1:-1, 1:-1] = 0.25 * (phi[1:-1, 2:] + phi[1:-1, :-2] + phi[2:, 1:-1] + phi[:-2, 1:-1]
                                          - rhs[1:-1, 1:-1])
            if mask is not None:
                phi_new[mask] = 0
            phi = phi_new
    return phi


def jacobi3d_statement(div, phi0=None, *, h, dt, iters, mask=None):
    """The 7-point form of the same template (float32):
    f32(1/6) * (((((E+W)+N)+S)+U)+D - f32(h*h)*div/dt), six faces held."""
    with np.errstate(all="ignore"):
        sixth = np.float32(1.0) / np.float32(6.0)
        rhs = (np.float32(h * h) * div) / np.float32(dt)
        phi = np.zeros_like(div) if phi0 is None else np.array(phi0, dtype=np.float32)
        c = (slice(1, -1),) * 3
        for _ in range(iters):
            phi_new = phi.copy()
            s = phi[1:-1, 1:-1, 2:] + phi[1:-1, 1:-1, :-2]
            s = s + phi[1:-1, 2:, 1:-1]
            s = s + phi[1:-1, :-2, 1:-1]
            s = s + phi[2:, 1:-1, 1:-1]
            s = s + phi[:-2, 1:-1, 1:-1]
            phi_new[c] = sixth * (s - rhs[c])
            if mask is not None:
                phi_new[mask] = 0
            phi = phi_new
    return phi


# ------------------------------------- independent statements: red-black GS
def _gs_constants(dtype, spacings, dt):
    """v5.py:205-210: the inverse squares and their denominator are Python
    floats, rounded to float32 where they meet float32 values (NEP 50) and
    kept in float64 against float64 fields; dt is np.float32, so
    dt_inv = 1.0 / dt is a float32 quotient in both."""
    T = np.dtype(dtype).type
    inv = [1.0 / (d * d) for d in spacings]
    denom_inv = 1.0 / (2.0 * sum(inv))
    dt_inv = np.float32(1.0) / np.float32(dt)
    return [T(c) for c in inv], T(denom_inv), T(dt_inv)


def rbgs2d_statement(div, phi0=None, *, dx, dy, dt, iters, tol, mask=None):
    """v5.py:202-226 as scalar loops on NumPy scalars of div's dtype (float32
    or float64).  Returns (phi, iterations done, max-change history).  Tiny
    grids only."""
    T = div.dtype.type
    ny, nx = div.shape
    phi = np.zeros_like(div) if phi0 is None else np.array(phi0, dtype=div.dtype)
    hist = []
    with np.errstate(all="ignore"):
        (cx, cy), cd, dt_inv = _gs_constants(div.dtype, (dx, dy), dt)
        ftol = T(tol)
        done = 0
        for _ in range(iters):
            max_change = T(0)
            for color in range(2):
                for i in range(1, ny - 1):
                    for j in range(1 + (i + color) % 2, nx - 1, 2):
                        if mask is not None and mask[i, j]:
                            continue
                        rhs = -div[i, j] * dt_inv
                        pn = (cx * (phi[i, j + 1] + phi[i, j - 1]) + cy * (phi[i + 1, j] + phi[i - 1, j]) - rhs) * cd
                        change = abs(pn - phi[i, j])
                        if change > max_change:
                            max_change = change
                        phi[i, j] = pn
            hist.append(max_change)
            done += 1
            if max_change < ftol:
                break
    return phi, done, np.array(hist, div.dtype)


def rbgs3d_statement(div, phi0=None, *, dx, dy, dz, dt, iters, tol, mask=None):
    """The 3-D red-black form: colour c updates (z + i + j) parity (1 + c) % 2;
    (((a + b) + e) - rhs) * cd.  Same returns as rbgs2d_statement."""
    T = div.dtype.type
    nz, ny, nx = div.shape
    phi = np.zeros_like(div) if phi0 is None else np.array(phi0, dtype=div.dtype)
    hist = []
    with np.errstate(all="ignore"):
        (cx, cy, cz), cd, dt_inv = _gs_constants(div.dtype, (dx, dy, dz), dt)
        ftol = T(tol)
        done = 0
        for _ in range(iters):
            max_change = T(0)
            for color in range(2):
                for z in range(1, nz - 1):
                    for i in range(1, ny - 1):
                        for j in range(1 + (z + i + color) % 2, nx - 1, 2):
                            if mask is not None and mask[z, i, j]:
                                continue
                            rhs = -div[z, i, j] * dt_inv
                            a = cx * (phi[z, i, j + 1] + phi[z, i, j - 1])
                            b = cy * (phi[z, i + 1, j] + phi[z, i - 1, j])
                            e = cz * (phi[z + 1, i, j] + phi[z - 1, i, j])
                            pn = (((a + b) + e) - rhs) * cd
                            change = abs(pn - phi[z, i, j])
                            if change > max_change:
                                max_change = change
                            phi[z, i, j] = pn
            hist.append(max_change)
            done += 1
            if max_change < ftol:
                break
    return phi, done, np.array(hist, div.dtype)


def rbgs3d_maxc(oracle_rbgs3d, div, phi0, n, **kw):
    """The oracle's per-iteration max|change| in 3-D (it has no history
    entry): every free cell is updated once per iteration, so it is the fold
    of |phi_(i+1) - phi_i|.  ``oracle_rbgs3d`` is oracle.rbgs3d."""
    phi = np.zeros_like(div) if phi0 is None else np.array(phi0, np.float32)
    out = []
    for _ in range(n):
        nxt, _ = oracle_rbgs3d(div, phi, iters=1, tol=0.0, **kw)
        out.append(fold_max(phi[1:-1, 1:-1, 1:-1], nxt[1:-1, 1:-1, 1:-1]))
        phi = nxt
    return np.array(out, np.float32)


# --------------------------------------------------- what a result contains
def census(a) -> dict:
    """Shares and counts the builder conditions are stated in."""
    a = np.asarray(a)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    bits = np.ascontiguousarray(a).view(u)
    sign = u(1) << u(8 * a.dtype.itemsize - 1)
    tiny = np.finfo(a.dtype).tiny
    inner = a[(slice(1, -1),) * a.ndim]
    with np.errstate(all="ignore"):
        sub = (inner != 0) & (np.abs(inner) < tiny)
    return {"finite": float(np.isfinite(a).mean()), "nan": int(np.isnan(a).sum()), "inf": int(np.isinf(a).sum()),
            "neg_zero": float((bits == sign).mean()), "pos_zero": float((bits == 0).mean()),
            "subnormal_interior": float(sub.mean()) if inner.size else 0.0}


# ------------------------------------------- the cases of the GPU test file
# name -> (operator, shape, dtype, iterations, options of build()).  Every
# fields-against-oracle comparison of tests/test_gpu_poisson_edges.py takes its
# inputs from here (gpu_case), and tests/test_poisson_edge_host.py asserts the
# builder conditions for each entry and class, so no GPU comparison is vacuous.
F32, F64 = np.float32, np.float64
GPU_CASES = {
    # 2-D Jacobi
    "j2_single": ("jacobi2d", (37, 53), F32, 5, {}),
    "j2_single_f64": ("jacobi2d", (37, 53), F64, 5, {}),
    "j2_blocked": ("jacobi2d", (48, 136), F32, 9, {"sparse": True}),
    "j2_blocked_f64": ("jacobi2d", (48, 136), F64, 9, {"sparse": True}),
    "j2_persist_53_7": ("jacobi2d", (53, 131), F32, 7, {"sparse": True}),
    "j2_persist_53_13": ("jacobi2d", (53, 131), F32, 13, {"sparse": True}),
    "j2_persist_36_7": ("jacobi2d", (36, 120), F32, 7, {"sparse": True}),
    "j2_persist_36_13": ("jacobi2d", (36, 120), F32, 13, {"sparse": True}),
    # 2-D red-black GS
    "gs2_color": ("gs2d", (37, 53), F32, 5, {}),
    "gs2_color_vec": ("gs2d", (40, 72), F32, 5, {}),
    "gs2_tile_5": ("gs2d", (48, 136), F32, 5, {"sparse": True}),
    "gs2_tile_7": ("gs2d", (48, 136), F32, 7, {"sparse": True}),
    "gs2_march": ("gs2d", (16387, 24), F32, 4, {}),
    "gs2_f64": ("gs2d", (31, 57), F64, 3, {"sparse": True}),
    # 3-D Jacobi
    "j3_single": ("jacobi3d", (10, 12, 36), F32, 4, {"sparse": True}),
    "j3_blocked": ("jacobi3d", (12, 21, 72), F32, 5, {"sparse": True}),
    "j3_k4_small": ("jacobi3d", (11, 40, 16), F32, 4, {"sparse": True}),
    "j3_k4_deep": ("jacobi3d", (52, 20, 264), F32, 4, {"sparse": True}),
    # 3-D red-black GS
    "gs3_color": ("gs3d", (10, 12, 36), F32, 3, {"sparse": True}),
    "gs3_fused": ("gs3d", (12, 21, 72), F32, 3, {"sparse": True, "mask2d": True}),
    "gs3_slab": ("gs3d", (30, 26, 40), F32, 3, {"sparse": True}),
    "gs3_zper": ("gs3zper", (12, 21, 72), F32, 3, {"sparse": True, "mask2d": True}),
}


# The cases the GPU file also solves from zeros (zero_start, cfd_*_zero_*).
# Those solves never read phi0, so only the div-borne part of a class is left:
# nonfinite keeps its NaN (and, where not sparse, -Inf) seeds in div, subnormal
# its subnormal div; signed_zero and neg_zero start from +0.0 and hold no -0.0
# any more, huge is ordinary data.  tests/test_poisson_edge_host.py asserts
# exactly that; the zero-start comparisons add the "phi is not read" property.
ZERO_START_CASES = ("j2_single", "j2_single_f64", "j2_blocked", "j2_blocked_f64", "j2_persist_53_7",
                    "j2_persist_53_13", "j2_persist_36_7", "j2_persist_36_13", "gs2_tile_5", "gs2_f64", "j3_blocked",
                    "j3_k4_small", "j3_k4_deep")


def reference(op, case, iters, tol=0.0, zero=False):
    """The reference result of one case: (phi, iterations done).  The C
    oracle, which tests/test_poisson_edge_host.py shows equal to the
    statements above on every class; the float64 GS, which has no C oracle,
    is the float64 statement (pinned to the reference's fixture there)."""
    import oracle
    c = case
    phi0 = None if zero else c.phi0
    if op == "jacobi2d":
        return oracle.jacobi2d(c.div, phi0, dx=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters
    if op == "jacobi3d":
        return oracle.jacobi3d(c.div, phi0, h=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters
    if op == "gs2d" and c.div.dtype == np.float64:
        phi, n, _ = rbgs2d_statement(c.div, phi0, dx=c.dx, dy=c.dy, dt=c.dt, iters=iters, tol=tol, mask=c.mask)
        return phi, n
    if op == "gs2d":
        return oracle.rbgs2d(c.div, phi0, dx=c.dx, dy=c.dy, dt=c.dt, iters=iters, tol=tol, mask=c.mask)
    if op == "gs3zper":     # periodic z: the NumPy statement of tests/zper_reference.py (no C oracle)
        from zper_reference import rbgs3d_zper_numpy
        with np.errstate(all="ignore"):
            return rbgs3d_zper_numpy(c.div, phi0, dx=c.dx, dy=c.dy, dz=c.dz, dt=c.dt, iters=iters, tol=tol,
                                     mask2d=None if c.mask is None else c.mask[0])
    assert op == "gs3d", op
    return oracle.rbgs3d(c.div, phi0, dx=c.dx, dy=c.dy, dz=c.dz, dt=c.dt, iters=iters, tol=tol, mask=c.mask)


def gpu_case(name, cls, masked=True, nan_only=False):
    """(operator, Case, iterations) of one GPU case."""
    op, shape, dtype, iters, opts = GPU_CASES[name]
    return op, build(cls, shape, dtype, masked=masked, op="gs" if op.startswith("gs") else "jacobi",
                     nan_only=nan_only, **opts), iters
