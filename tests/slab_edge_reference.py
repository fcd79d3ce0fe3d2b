"""The slab Poisson drivers at their edges: cases and a plain CPU statement.

``CASES`` names every (ranks, grid, ghost depth, mask, start, sweeps) the host
file tests/test_slab_edge_host.py and the GPU file tests/test_gpu_slab_edges.py
share.  ``make_case`` builds the seeded inputs of one of them.

``emulate_jacobi`` and ``emulate_rbgs`` run the slab schedule with R ranks in
one process: ``SlabPlan.scatter`` and ``SlabPlan.exchanges()`` move the planes,
``oracle.jacobi3d(..., iters=1)`` on a sub-block is one sweep of a plane range
(what the workers of tests/test_slab_gloo.py do), a NumPy colour pass with
global parity is one red-black half-sweep.  They are a second statement of
what the drivers must do -- the single-domain oracle stays the reference the
GPU is compared with, and the host file shows the two equal.

What a mask adds to the decomposed Jacobi solve: the single-domain reference
sets ``phi_new[mask] = 0`` over the whole array after every sweep: rows y = 0
and ny-1, columns x = 0 and nx-1 and the global Dirichlet planes included,
cells no sweep of a plane range writes.  The first sweep still reads the
guess there.  So every rank zeroes the masked cells of the planes it owns
after each pass and before the exchange; its neighbours see those zeros in
their ghosts after the first pass, not before it.  ``emulate_jacobi(...,
zeroing=False)`` leaves that step out: the host file's negative control.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace

import numpy as np

import oracle
from cfd_simulations_amd.slab import SlabPlan

F = np.float32
H, JDT = 0.05, F(1e-3)                       # Jacobi: grid step and dt
GDX, GDY, GDZ, GDT = 0.05, 0.06, 0.07, F(1e-2)   # GS
GS_ITERS = 7


@dataclass(frozen=True)
class Case:
    name: str
    op: str          # "jacobi" | "gs"
    R: int
    nz: int
    ny: int
    nx: int
    ghost: int
    masked: bool
    start: str       # "zero" | "guess"
    iters: int
    dx: float = GDX  # (GS only, as are dy, dz, tols, steps)
    dy: float = GDY
    dz: float = GDZ
    tols: tuple = ()  # (tolerance, the reference's iteration count) pairs
    steps: int = 0   # blocking depth the GPU file sets for the case (0: auto)

    @property
    def shape(self):
        return (self.nz, self.ny, self.nx)

    def plans(self):
        return [SlabPlan(self.nz, self.R, r, self.ghost) for r in range(self.R)]


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(key):
    name, op, R, nz, ny, nx, ghost, masked, start = key
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    div = rng.standard_normal((nz, ny, nx)).astype(F)
    phi0 = rng.standard_normal((nz, ny, nx)).astype(F)
    if op == "gs":
        div *= F(1e-3)
        phi0 *= F(1e-4)      # the size of the solution, so that max|change| falls from the first iteration
    if start == "zero":
        phi0 = np.zeros_like(div)
    mask = None
    if masked:
        assert ny >= 7 and nx >= 5, "the forced cells below need distinct places"
        mask = rng.random((nz, ny, nx)) < 0.15
        zm = nz // 2
        plans = [SlabPlan(nz, R, r, ghost) for r in range(R)]
        forced = [(0, 2, 3), (nz - 1, 2, 3), (zm, 0, 3), (zm, 2, nx - 1)]
        forced += [(p.z_lo, 3, 2) for p in plans] + [(p.z_hi - 1, 4, 1) for p in plans]
        if nz >= 3:
            forced.append((min(max(zm, 1), nz - 2), 5, 2))
        for c in forced:
            mask[c] = True
        # a case cannot lose the cells that matter:
        assert mask[0].any() and mask[nz - 1].any()              # the global Dirichlet planes
        assert mask[:, 0, :].any() and mask[:, :, nx - 1].any()  # a row and a column no sweep writes
        for p in plans:                                         # the planes the neighbours take as ghosts
            assert mask[p.z_lo].any() and mask[p.z_hi - 1].any()
        if nz >= 3:                                             # (two planes have no interior)
            inner = mask[1:-1, 1:-1, 1:-1]
            assert inner.any() and not inner.all()
        if start == "guess":    # the guess is non-zero where the mask zeroes it
            assert all(phi0[c] != 0 for c in forced)
        mask.setflags(write=False)
    div.setflags(write=False)
    phi0.setflags(write=False)
    return div, phi0, mask


def make_case(case):
    """(div, phi0, mask): float32, float32 and bool or None, seeded by the
    case's name, read-only and shared by every caller."""
    return _inputs((case.name, case.op, case.R, case.nz, case.ny, case.nx, case.ghost, case.masked, case.start))


def reference(case, tol=0.0):
    """The single-domain oracle's result: phi for Jacobi, (phi, count) for GS."""
    div, phi0, mask = make_case(case)
    if case.op == "jacobi":
        return oracle.jacobi3d(div, phi0, h=H, dt=JDT, iters=case.iters, mask=mask)
    return oracle.rbgs3d(div, phi0, dx=case.dx, dy=case.dy, dz=case.dz, dt=GDT, iters=case.iters, tol=tol,
                         mask=mask)


def history(case, n):
    """The oracle's max|change| of iterations 1 .. n of a GS case (it has no
    history entry in 3-D): every free cell is updated once per iteration and
    the others keep their value, so it is max|phi_(i+1) - phi_i|."""
    div, phi0, mask = make_case(case)
    phi, out = np.array(phi0), []
    for _ in range(n):
        nxt, _ = oracle.rbgs3d(div, phi, dx=case.dx, dy=case.dy, dz=case.dz, dt=GDT, iters=1, tol=0.0, mask=mask)
        out.append(np.abs(nxt - phi).max() if phi.size else F(0))
        phi = nxt
    return np.array(out, F)


def stop_tolerances(case, counts=(3, 4)):
    """((tol, n), ...): for each n of ``counts`` (an odd and an even one, so
    that a stop falls inside and at the end of a two-iteration pass) the
    float just above the oracle's max|change| of iteration n.  The oracle
    stops on max|change| < f32(tol): iteration n is below it and, asserted
    here, no earlier one is."""
    mc = history(case, max(counts))
    out = []
    for n in counts:
        tol = float(np.nextafter(mc[n - 1], F(np.inf)))
        assert mc[n - 1] > 0 and (mc[:n - 1] >= F(tol)).all() and 1 < n < case.iters, (case.name, n, mc)
        out.append((tol, n))
    return tuple(out)


# ------------------------------------------------------------------- cases
def _table():
    cases = []

    def j(group, R, nz, nx, G, masked, start, iters, ny=9):
        name = f"{group}-R{R}-nz{nz}-nx{nx}-g{G}-{'mask' if masked else 'free'}-{start}-it{iters}"
        cases.append(Case(name, "jacobi", R, nz, ny, nx, G, masked, start, iters))

    def g(group, R, nz, nx, G, masked, start, steps=0, ny=9, tols=True):
        name = f"{group}-R{R}-nz{nz}-ny{ny}-nx{nx}-g{G}-{'mask' if masked else 'free'}-{start}-s{steps}"
        c = Case(name, "gs", R, nz, ny, nx, G, masked, start, GS_ITERS, steps=steps)
        if tols:
            c = replace(c, tols=stop_tolerances(c))
        cases.append(c)

    starts, widths = ("zero", "guess"), (12, 10)
    # masked Jacobi: one sweep, and an odd and an even count (where the last pass lands)
    for R, nz in ((2, 13), (3, 13)):
        for G in (1, 2, 4):
            for nx in widths:
                for start in starts:
                    for iters in (1, 5, 6):
                        j("jmask", R, nz, nx, G, True, start, iters)
    # only the zeroing of masked Dirichlet-plane cells happens: (3, 3) has one updated plane, (2, 2) none
    for R, nz in ((3, 3), (2, 2)):
        for start, iters, nx in (("guess", 1, 12), ("guess", 2, 10), ("zero", 2, 12)):
            j("jmask-planes", R, nz, nx, 1, True, start, iters)
    # rows no float4 covers, deep ghosts, no mask: the unblocked solve
    for nx in (5, 10, 13):
        for G in (2, 3, 4):
            for start, iters in zip(starts, (5, 6)):
                j("jragged", 3, 14, nx, G, False, start, iters)
    # thinnest slabs; sweeps below K, and every sweeps mod K
    for R, nz, G in ((2, 8, 4), (3, 12, 4), (3, 13, 4), (3, 6, 2), (4, 8, 2), (2, 4, 2), (3, 3, 1)):
        for iters in (1, 2, 5, 7, 8):
            for start in starts:
                j("jthin", R, nz, 12, G, False, start, iters)
    # the middle rank's update range: 2G planes (overlap declined), then 2G + 1 (taken)
    for nz, G in ((12, 2), (15, 2), (24, 4), (27, 4)):
        for start in starts:
            j("jthreshold", 3, nz, 12, G, False, start, 5)
    # ghost 4 with fewer sweeps per pass (the GPU file sets the depth), thick and thin
    for nz in (20, 8):
        for iters in (5, 8):
            j("jdepth", 2, nz, 12, 4, False, starts[iters % 2], iters)
    # zero sweeps
    j("jnone", 2, 9, 12, 2, False, "guess", 0)

    # masked GS, in place.  (3 ranks with 4-deep ghosts need 12 planes.)
    n = 0
    for G in (1, 2, 4):
        for R in (2, 3):
            for nx in widths:
                g("gmask", R, 12 if R * G > 9 else 9, nx, G, True, "guess" if n % 3 == 2 else "zero")
                n += 1
    for G, nx in ((2, 10), (4, 13), (2, 5)):
        g("gragged", 2, 9, nx, G, False, "zero")
    for R, nz, G, steps in ((2, 4, 2, 2), (3, 6, 2, 0), (2, 8, 4, 4), (3, 12, 4, 4), (3, 13, 4, 0)):
        g("gthin", R, nz, 12, G, False, "zero", steps)
    for R, nz, G, masked in ((2, 9, 1, False), (3, 9, 2, False), (2, 9, 4, False), (3, 13, 4, False),
                             (2, 9, 2, True)):
        g("gguess", R, nz, 12, G, masked, "guess")
    for G in (1, 2):
        g("gflat", 2, 9, 12, G, False, "guess", ny=2, tols=False)
    return {c.name: c for c in cases}


CASES = _table()


def group(prefix):
    """The cases of one group, by name."""
    return [n for n in CASES if n.split("-R")[0] == prefix]


# --------------------------------------------------------------- emulation
def _scatter_owned(plan, glob):
    """The local array with the owned planes filled and NaN in the ghosts."""
    loc = np.full((plan.nz_total,) + glob.shape[1:], np.nan, F)
    loc[plan.owned()] = glob[plan.z_lo:plan.z_hi]
    return loc


def _exchange(plans, arrays):
    for p, a in zip(plans, arrays):
        for first, count, peer, recv in p.exchanges():
            arrays[peer][recv:recv + count] = a[first:first + count]


def _gather(plans, arrays):
    return np.concatenate([a[p.owned()] for p, a in zip(plans, arrays)])


def emulate_jacobi(case, K, zeroing=True):
    """The slab Jacobi schedule: passes of k = min(K, remaining) levels, level
    j on the update range widened by k - j planes (never past a Dirichlet
    plane), one exchange of ``ghost`` planes per pass.  A mask needs K = 1."""
    assert case.op == "jacobi" and 1 <= K <= case.ghost and not (case.masked and K != 1)
    div, phi0, mask = make_case(case)
    plans = case.plans()
    dloc = [p.scatter(div) for p in plans]
    mloc = [p.scatter(mask) for p in plans] if case.masked else [None] * case.R

    def sweep(r, a, lo, hi):
        """Planes [lo, hi) of one sweep: the oracle on the sub-block with
        planes lo-1 and hi held.  A sweep writes the cells inside the faces."""
        out = a.copy()
        if hi > lo:
            sub = oracle.jacobi3d(dloc[r][lo - 1:hi + 1], a[lo - 1:hi + 1], h=H, dt=JDT, iters=1,
                                  mask=None if mloc[r] is None else mloc[r][lo - 1:hi + 1])
            out[lo:hi, 1:-1, 1:-1] = sub[1:-1, 1:-1, 1:-1]
        return out

    phi = [_scatter_owned(p, phi0) for p in plans]
    _exchange(plans, phi)                       # the ghosts of the guess
    done = 0
    while done < case.iters:
        k = min(K, case.iters - done)
        new = []
        for r, p in enumerate(plans):
            zb, ze = p.z_update_begin, p.z_update_end
            fixed_lo, fixed_hi = p.z_lo == 0, p.z_hi == case.nz
            lev = phi[r]
            for lv in range(1, k + 1):
                w = k - lv
                lev = sweep(r, lev, zb if fixed_lo else zb - w, ze if fixed_hi else ze + w)
            out = phi[r].copy()
            out[zb:ze] = lev[zb:ze]
            if case.masked and zeroing:
                own = p.owned()
                out[own][mloc[r][own]] = 0      # (a view: writes out)
            new.append(out)
        _exchange(plans, new)
        phi, done = new, done + k
    return _gather(plans, phi)


def _colour_pass(phi, div, mask, colour, lo, hi, zoff, k):
    """Colour ``colour`` of local planes [lo, hi), global parity (zoff: the
    global index of local plane 0), masked cells skipped.  Cells of one
    colour read only the other, so the array form equals the serial one.
    Returns max|change|."""
    cx, cy, cz, cd, dt_inv = k
    if hi <= lo or phi.shape[1] < 3 or phi.shape[2] < 3:
        return F(0)
    z = np.arange(lo, hi)[:, None, None] + zoff
    y = np.arange(1, phi.shape[1] - 1)[None, :, None]
    x = np.arange(1, phi.shape[2] - 1)[None, None, :]
    sel = ((z + y + x + 1 + colour) % 2) == 0
    if mask is not None:
        sel = sel & ~mask[lo:hi, 1:-1, 1:-1].astype(bool)
    C = phi[lo:hi, 1:-1, 1:-1]
    rhs = -div[lo:hi, 1:-1, 1:-1] * dt_inv
    a = cx * (phi[lo:hi, 1:-1, 2:] + phi[lo:hi, 1:-1, :-2])
    b = cy * (phi[lo:hi, 2:, 1:-1] + phi[lo:hi, :-2, 1:-1])
    e = cz * (phi[lo + 1:hi + 1, 1:-1, 1:-1] + phi[lo - 1:hi - 1, 1:-1, 1:-1])
    new = (((a + b) + e) - rhs) * cd
    ch = np.abs(new - C)[sel]
    phi[lo:hi, 1:-1, 1:-1] = np.where(sel, new, C)
    return ch.max() if ch.size else F(0)


def emulate_rbgs(case, tol):
    """The slab red-black GS, in place: a colour on every rank's update range,
    an exchange, the other colour, an exchange; the iteration's max|change|
    is the largest over all ranks and the solve stops when it is below
    f32(tol).  Masked cells are held, not zeroed.  Returns (phi, count)."""
    assert case.op == "gs"
    div, phi0, mask = make_case(case)
    plans = case.plans()
    dloc = [p.scatter(div) for p in plans]
    mloc = [p.scatter(mask) for p in plans] if case.masked else [None] * case.R
    i2 = (1.0 / case.dx ** 2, 1.0 / case.dy ** 2, 1.0 / case.dz ** 2)
    k = tuple(F(v) for v in i2) + (F(1.0 / (2.0 * sum(i2))), F(1.0) / GDT)
    phi = [_scatter_owned(p, phi0) for p in plans]
    _exchange(plans, phi)
    for it in range(case.iters):
        m = F(0)
        for colour in (0, 1):
            for r, p in enumerate(plans):
                m = max(m, _colour_pass(phi[r], dloc[r], mloc[r], colour, p.z_update_begin, p.z_update_end,
                                        p.z_lo - case.ghost, k))
            _exchange(plans, phi)
        if m < F(tol):
            return _gather(plans, phi), it + 1
    return _gather(plans, phi), case.iters
