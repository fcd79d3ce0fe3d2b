"""CPU side of the Poisson edge-value tests (no GPU).

* ``same_bits`` and ``fold_max`` do what tests/test_gpu_poisson_edges.py
  relies on.
* The C oracle equals the independent NumPy statements of
  tests/poisson_edge_reference.py on every input class, operator and mask
  setting, iteration counts included -- so the oracle may serve as the
  reference of the GPU file on these classes.
* The float64 red-black GS statement (the reference of cfd_rbgs2d_f64, which
  has no C oracle) reproduces the reference's own float64 fixture.
* Every (shape, iterations, class) of the GPU file holds what its class
  promises in the reference result: conditions, not measurements, that keep a
  GPU comparison from passing vacuously.
* The stop rule's boundary on the oracle: tol equal to an iteration's
  max|change| does not stop at it, the next float up does.
"""
import functools

import numpy as np
import pytest

import oracle
import poisson_edge_reference as R
from poisson_edge_reference import CLASSES, GPU_CASES, census, fold_max, same_bits

F = np.float32


# ------------------------------------------------------------------ same_bits
def test_same_bits_separates_signed_zeros_and_equates_nans():
    pz, nz = np.array([0.0, 1.0], F), np.array([-0.0, 1.0], F)
    assert np.array_equal(pz, nz) and not same_bits(pz, nz)
    assert same_bits(nz, nz.copy()) and same_bits(pz, pz.copy())
    pos_nan = np.array([0x7FC00000, 0x3F800000], np.uint32).view(F)
    neg_nan = np.array([0xFFC00001, 0x3F800000], np.uint32).view(F)
    assert same_bits(pos_nan, neg_nan)
    assert not same_bits(pos_nan, np.array([1.0, 1.0], F))          # NaN against a number
    assert not same_bits(np.array([1.0, 1.0], F), pos_nan)
    assert not same_bits(np.array([np.inf], F), np.array([-np.inf], F))
    assert not same_bits(np.zeros(2, F), np.zeros(2, np.float64))   # dtype
    assert not same_bits(np.zeros(2, F), np.zeros((2, 1), F))       # shape
    d = np.array([-0.0, np.nan, 5e-324])
    assert same_bits(d, d.copy()) and not same_bits(d, np.array([0.0, np.nan, 5e-324]))
    assert not same_bits(d, np.array([-0.0, np.nan, 1e-323]))
    assert "1 of 3" in R.describe_difference(d, np.array([0.0, np.nan, 5e-324]))


def test_fold_max_is_the_conditional_fold():
    a = np.array([1.0, np.nan, 3.0, np.inf, -0.0], F)
    assert fold_max(a, np.array([1.5, 2.0, np.nan, np.inf, 0.0], F)) == F(0.5)      # NaN changes never count
    assert fold_max(a, np.array([1.0, 2.0, 3.0, 1.0, 0.0], F)) == F(np.inf)         # an infinite one does
    r = fold_max(a[1:2], np.array([7.0], F))
    assert r == 0 and not np.signbit(r) and r.dtype == F                           # all NaN: 0
    assert fold_max(np.zeros(0, F), np.zeros(0, F)) == 0


# ------------------------------------------- the oracle against the statements
def _both(op, case, iters, tol):
    c = case
    if op == "jacobi2d":
        return ((oracle.jacobi2d(c.div, c.phi0, dx=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters),
                (R.jacobi2d_statement(c.div, c.phi0, dx=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters))
    if op == "jacobi3d":
        return ((oracle.jacobi3d(c.div, c.phi0, h=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters),
                (R.jacobi3d_statement(c.div, c.phi0, h=c.dx, dt=c.dt, iters=iters, mask=c.mask), iters))
    if op == "gs2d":
        kw = dict(dx=c.dx, dy=c.dy, dt=c.dt, iters=iters, tol=tol, mask=c.mask)
        p, n, h = R.rbgs2d_statement(c.div, c.phi0, **kw)
        po, no, ho = oracle.rbgs2d_maxc(c.div, c.phi0, **kw)
        assert same_bits(ho, h), (ho, h)
        return (po, no), (p, n)
    kw = dict(dx=c.dx, dy=c.dy, dz=c.dz, dt=c.dt, iters=iters, tol=tol, mask=c.mask)
    p, n, h = R.rbgs3d_statement(c.div, c.phi0, **kw)
    ho = R.rbgs3d_maxc(oracle.rbgs3d, c.div, c.phi0, n, **{k: v for k, v in kw.items() if k not in ("iters", "tol")})
    assert same_bits(ho, h), (ho, h)
    return oracle.rbgs3d(c.div, c.phi0, **kw), (p, n)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("op,shape,dtype", [("jacobi2d", (12, 20), F), ("jacobi2d", (12, 20), np.float64),
                                            ("gs2d", (12, 20), F), ("jacobi3d", (6, 7, 12), F),
                                            ("gs3d", (6, 7, 12), F)])
@pytest.mark.parametrize("cls", CLASSES)
def test_oracle_equals_the_independent_statement(cls, op, shape, dtype, masked):
    for nan_only in ((False, True) if cls == "nonfinite" else (False,)):
        case = R.build(cls, shape, dtype, masked=masked, op="gs" if op.startswith("gs") else "jacobi",
                       nan_only=nan_only)
        (po, no), (ps, ns) = _both(op, case, 4, 0.0)
        assert no == ns == 4
        assert same_bits(po, ps), R.describe_difference(po, ps)
        if op.startswith("gs"):
            # an early stop taken from the history: same count, same bits
            kw = dict(dx=case.dx, dy=case.dy, dt=case.dt, mask=case.mask)
            hist = R.rbgs2d_statement(case.div, case.phi0, iters=4, tol=0.0, **kw)[2] if op == "gs2d" else \
                R.rbgs3d_statement(case.div, case.phi0, iters=4, tol=0.0, dz=case.dz, **kw)[2]
            for tol in (float(hist[1]), float(np.nextafter(hist[1], F(np.inf))), np.nan, np.inf, -1.0, 1e-50):
                (po, no), (ps, ns) = _both(op, case, 4, tol)
                assert no == ns, (tol, no, ns)
                assert same_bits(po, ps), (tol, R.describe_difference(po, ps))


def test_float64_gs_statement_reproduces_the_reference_fixture(golden):
    """cfd_rbgs2d_f64 has no C oracle: its reference is rbgs2d_statement in
    float64, whose constants' rounding (float64 inverse squares, a float32
    1 / dt) is pinned here to the reference's own float64 step: div_u_star ->
    phi of step 1 (solve_pressure_fast from zeros, v5.py:337-342)."""
    d = golden("step_v5_120x36_n3_f64_gs.npz")
    div, want, mask = d["div1"], d["phi1"], d["cylinder_mask"]
    assert div.dtype == want.dtype == np.float64 and div.shape == (36, 120) and mask.any()
    phi, n, hist = R.rbgs2d_statement(div, None, dx=20 / 119, dy=4 / 35, dt=F(0.00005), iters=200, tol=1e-8,
                                      mask=mask)
    assert same_bits(phi, want), R.describe_difference(phi, want)
    assert n == len(hist) <= 200 and want.any()
    # the float32 statement from the same inputs is not these bits: the pin is about float64
    p32 = R.rbgs2d_statement(div.astype(F), None, dx=20 / 119, dy=4 / 35, dt=F(0.00005), iters=3, tol=0.0,
                             mask=mask)[0]
    p64 = R.rbgs2d_statement(div, None, dx=20 / 119, dy=4 / 35, dt=F(0.00005), iters=3, tol=0.0, mask=mask)[0]
    assert not np.array_equal(p32.astype(np.float64), p64)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("cls", CLASSES)
def test_zper_statement_equals_the_oracle_without_the_wrap(cls, masked):
    """The z-periodic solve's reference is tests/zper_reference.py's NumPy
    statement; with periodic=False it is the oracle's solve, on these classes
    too (NaN changes dropped from the fold, signed zeros kept)."""
    from zper_reference import rbgs3d_zper_numpy
    case = R.build(cls, (6, 7, 12), masked=masked, op="gs", mask2d=True)
    kw = dict(dx=case.dx, dy=case.dy, dz=case.dz, dt=case.dt, iters=4, tol=0.0)
    with np.errstate(all="ignore"):
        got, n = rbgs3d_zper_numpy(case.div, case.phi0, mask2d=case.mask[0] if masked else None, periodic=False, **kw)
    want, n_ref = oracle.rbgs3d(case.div, case.phi0, mask=case.mask, **kw)
    assert n == n_ref == 4
    assert same_bits(got, want), R.describe_difference(got, want)


# ----------------------------------------------------- the builder conditions
@functools.lru_cache(maxsize=None)
def _result(name, cls, masked):
    op, case, iters = R.gpu_case(name, cls, masked)
    return op, case, R.reference(op, case, iters)[0]


def _neighbours(idx, shape):
    for ax in range(len(shape)):
        for s in (-1, 1):
            k = list(idx)
            k[ax] += s
            if 0 <= k[ax] < shape[ax]:
                yield tuple(k)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_builder_conditions_hold_for_every_gpu_case(name, cls, masked):
    op, case, ref = _result(name, cls, masked)
    n = census(ref)
    print(name, cls, masked, n)
    assert ref.dtype == case.div.dtype == GPU_CASES[name][2]
    if cls == "nonfinite":
        assert n["finite"] >= 0.5 and n["nan"] >= 20 and n["inf"] >= 5, n
        p = case.phi0
        ring = np.ones(p.shape, bool)
        ring[(slice(1, -1),) * p.ndim] = False
        assert (~np.isfinite(p[ring])).any()
        assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any() and (~np.isfinite(case.div)).any()
        if masked:
            bad = ~np.isfinite(p) | ~np.isfinite(case.div)
            solid = np.argwhere(case.mask)
            assert any(bad[tuple(k)] for k in solid)                                     # non-finite itself
            assert any(bad[q] and not case.mask[q] for k in solid for q in _neighbours(k, p.shape))
    elif cls == "signed_zero":
        assert n["neg_zero"] >= 0.1 and n["pos_zero"] >= 0.1, n
        assert (ref != 0).any()
    elif cls == "neg_zero":
        if op.startswith("jacobi"):     # (-0 ... -0) - (+0) = -0: kept; solid cells become +0
            assert n["neg_zero"] >= (0.1 if masked else 0.9) and (n["pos_zero"] > 0) == masked, n
        else:                           # the GS right side is -(+0) / dt = -0, and (-0) - (-0) = +0
            assert n["pos_zero"] >= 0.5 and n["neg_zero"] > 0, n
    elif cls == "subnormal":
        assert n["subnormal_interior"] >= 0.9, n
    elif cls == "huge":
        assert n["inf"] >= 5 and n["nan"] >= 5 and n["finite"] >= 0.5, n


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", R.ZERO_START_CASES)
def test_zero_start_cases_hold_the_div_borne_part(name, cls, masked):
    """The GPU file's zero-start solves never read phi0.  What their
    references still contain: the NaN (and -Inf, where the case is not sparse)
    seeds of div and their spread, the subnormal div; the zero classes start
    from +0.0 and hold no -0.0, ``huge`` is ordinary data."""
    op, case, iters = R.gpu_case(name, cls, masked)
    ref = R.reference(op, case, iters, zero=True)[0]
    n = census(ref)
    print(name, cls, masked, n)
    if cls == "nonfinite":
        assert n["finite"] >= 0.5 and n["nan"] >= 20, n
        assert (n["inf"] >= 5) == (not GPU_CASES[name][4].get("sparse", False)), n
    elif cls == "signed_zero":
        assert n["neg_zero"] == 0 and n["pos_zero"] >= 0.1 and (ref != 0).any(), n
    elif cls == "neg_zero":
        assert n["pos_zero"] == 1.0, n
    elif cls == "subnormal":
        assert n["subnormal_interior"] >= 0.9, n
    elif cls == "huge":
        assert n["finite"] == 1.0 and (ref != 0).mean() >= 0.5, n


def test_nan_only_inputs_hold_no_infinity():
    for name in ("gs2_color", "gs2_tile_7", "gs3_color"):
        op, case, iters = R.gpu_case(name, "nonfinite", True, nan_only=True)
        assert not np.isinf(case.phi0).any() and not np.isinf(case.div).any()
        assert np.isnan(case.phi0).any() and np.isnan(case.div).any()


# ------------------------------------ the cases tell a wrong operator apart
def _jacobi2d_variant(case, iters, solid="assign", order="reference", flush=False):
    """jacobi2d_statement with one deliberate deviation, each a way a kernel
    could be subtly wrong: solid cells multiplied by 0 instead of set to 0,
    the neighbour sum reassociated as (E + W) + (N + S), subnormal results
    flushed to zero."""
    d, m = case.div, case.mask
    with np.errstate(all="ignore"):
        rhs = (F(case.dx * case.dx) * d) / F(case.dt)
        phi = np.array(case.phi0)
        for _ in range(iters):
            new = phi.copy()
            e, w, n, s = phi[1:-1, 2:], phi[1:-1, :-2], phi[2:, 1:-1], phi[:-2, 1:-1]
            total = (e + w) + (n + s) if order == "pairs" else e + w + n + s
            new[1:-1, 1:-1] = 0.25 * (total - rhs[1:-1, 1:-1])
            if flush:
                new[np.abs(new) < np.finfo(F).tiny] = 0
            if m is not None:
                new[m] = new[m] * 0 if solid == "multiply" else 0
            phi = new
    return phi


def test_the_cases_tell_a_subtly_wrong_operator_apart():
    """What the edge classes add to the ordinary-data sweeps: each deviation
    below leaves N(0, 1) data bit-identical or np.array_equal, and is caught
    by same_bits on the class meant for it."""
    ref = {}
    for cls in CLASSES:
        op, case, iters = R.gpu_case("j2_single", cls, True)
        ref[cls] = (case, iters, R.reference(op, case, iters)[0])
        assert same_bits(_jacobi2d_variant(case, iters), ref[cls][2])          # the undeviated form: the oracle
    rng = np.random.default_rng(0)
    plain = R.Case(rng.standard_normal((37, 53)).astype(F), rng.standard_normal((37, 53)).astype(F),
                   ref["nonfinite"][0].mask, 0.05, 0.04, 0.06, F(1e-2))
    want = oracle.jacobi2d(plain.div, plain.phi0, dx=plain.dx, dt=plain.dt, iters=5, mask=plain.mask)
    # solid cells multiplied by 0: ordinary data cannot tell (-0.0 == +0.0), the classes can
    got = _jacobi2d_variant(plain, 5, solid="multiply")
    assert np.array_equal(got, want)
    for cls in ("nonfinite", "signed_zero", "huge"):
        case, iters, r = ref[cls]
        assert not same_bits(_jacobi2d_variant(case, iters, solid="multiply"), r), cls
    # flush to zero: invisible on ordinary data
    assert same_bits(_jacobi2d_variant(plain, 5, flush=True), want)
    case, iters, r = ref["subnormal"]
    assert not same_bits(_jacobi2d_variant(case, iters, flush=True), r)
    # a reassociated sum overflows in other cells
    case, iters, r = ref["huge"]
    assert not same_bits(_jacobi2d_variant(case, iters, order="pairs"), r)
    # the fold: a maximum that lets NaN win never stops where the oracle does
    op, case, _ = R.gpu_case("gs2_color", "nonfinite", True, nan_only=True)
    kw = dict(dx=case.dx, dy=case.dy, dt=case.dt, mask=case.mask)
    _, _, mc = oracle.rbgs2d_maxc(case.div, case.phi0, iters=8, tol=0.0, **kw)
    states, phi = [np.array(case.phi0)], case.phi0
    for _ in range(8):
        phi = oracle.rbgs2d(case.div, phi, iters=1, tol=0.0, **kw)[0]
        states.append(phi)
    with np.errstate(all="ignore"):
        nan_wins = [np.abs(b - a)[1:-1, 1:-1].max() for a, b in zip(states, states[1:])]
    assert np.isnan(nan_wins).all() and np.isfinite(mc).all()
    assert [fold_max(a[1:-1, 1:-1], b[1:-1, 1:-1]) for a, b in zip(states, states[1:])] == list(mc)


# -------------------------------------------------------------- the stop rule
def stop_problem(shape=(24, 36), seed=3):
    rng = np.random.default_rng(seed)
    div = rng.standard_normal(shape).astype(F) * F(1e-2)
    return div, dict(dx=0.1, dy=0.1, dt=F(1.0))


@pytest.mark.parametrize("c", [3, 5])
def test_stop_rule_boundary_on_the_oracle(c):
    """max_change < f32(tol) stops: tol equal to iteration c's max|change|
    runs on to iteration c + 1 (c + 2 done), the next float up stops at c."""
    div, kw = stop_problem()
    _, _, mc = oracle.rbgs2d_maxc(div, iters=12, tol=0.0, **kw)
    assert (np.diff(mc) < 0).all(), mc
    assert oracle.rbgs2d(div, iters=12, tol=float(mc[c]), **kw)[1] == c + 2
    assert oracle.rbgs2d(div, iters=12, tol=float(np.nextafter(mc[c], F(np.inf))), **kw)[1] == c + 1
    for tol in (np.nan, -1.0, 1e-50, 0.0):
        assert oracle.rbgs2d(div, iters=12, tol=tol, **kw)[1] == 12
    assert oracle.rbgs2d(div, iters=12, tol=np.inf, **kw)[1] == 1
    # 3-D, through the history helper
    div3 = np.random.default_rng(4).standard_normal((8, 10, 12)).astype(F) * F(1e-2)
    kw3 = dict(dx=0.1, dy=0.1, dz=0.1, dt=F(1.0))
    mc3 = R.rbgs3d_maxc(oracle.rbgs3d, div3, None, 10, **kw3)
    assert (np.diff(mc3) < 0).all(), mc3
    assert oracle.rbgs3d(div3, iters=10, tol=float(mc3[c]), **kw3)[1] == c + 2
    assert oracle.rbgs3d(div3, iters=10, tol=float(np.nextafter(mc3[c], F(np.inf))), **kw3)[1] == c + 1


def test_a_nan_change_never_counts_and_an_infinite_one_does():
    """With NaN seeds alone the NaN front moves every iteration and the solve
    still stops on the finite cells' changes; one infinite seed keeps
    max|change| at Inf (a cell turning infinite changes by Inf) and the solve
    never stops."""
    op, case, _ = R.gpu_case("gs2_color", "nonfinite", True, nan_only=True)
    kw = dict(dx=case.dx, dy=case.dy, dt=case.dt, mask=case.mask)
    phi, n, mc = oracle.rbgs2d_maxc(case.div, case.phi0, iters=8, tol=0.0, **kw)
    assert np.isfinite(mc).all() and (mc > 0).all()
    assert (np.diff(mc) < 0).all(), mc
    p3, n3 = oracle.rbgs2d(case.div, case.phi0, iters=8, tol=float(np.nextafter(mc[2], F(np.inf))), **kw)
    assert n3 == 3 and 20 <= np.isnan(p3).sum() < np.isnan(phi).sum()
    assert oracle.rbgs2d(case.div, case.phi0, iters=8, tol=float(mc[2]), **kw)[1] == 4
    op, case, _ = R.gpu_case("gs2_color", "nonfinite", True)
    _, n, mc = oracle.rbgs2d_maxc(case.div, case.phi0, iters=6, tol=1e30, dx=case.dx, dy=case.dy, dt=case.dt,
                                  mask=case.mask)
    assert n == 6 and np.isinf(mc).all()
