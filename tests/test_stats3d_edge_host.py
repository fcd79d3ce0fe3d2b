"""The edge-value runs of the flow statistics on the CPU
(tests/stats3d_edge_reference.py): the statements equal literal per-cell
loops of Python floats, every class holds what it promises (printed as a
census of finite, NaN, infinite, -0.0 and sub-FLT_MIN sums), and the exact
classes do not depend on the order of the planes."""
import numpy as np
import pytest

import stats3d_edge_reference as S
from stats3d_edge_reference import CLASSES, CONTAINS, COUNTS, EXACT, MOMENTS, SHAPES, census, same_bits

LOOP_SHAPES = SHAPES[:3]      # the literal loop is Python per cell: the three small shapes


def loop_terms(nm, u, v, w, e, s):
    t = [u, v, w, u * u, v * v, w * w, u * v, u * w, v * w]
    if nm in (10, 15):
        t.append(e)
    if nm > 10:
        t += [s, s * s, u * s, v * s, w * s]
    return t


def loop_run(run, shape, nm, span):
    nz, ny, nx = shape
    acc = S.start_array(run, shape, nm, span)
    for sample, wgt in zip(run.samples, run.weights):
        wgt = float(wgt)
        for i in range(ny):
            for j in range(nx):
                col = [0.0] * nm
                for k in range(nz):
                    t = loop_terms(nm, *(float(a[k, i, j]) for a in sample))
                    assert len(t) == nm
                    for m in range(nm):
                        if span:
                            col[m] = col[m] + t[m]
                        else:
                            acc[m, k, i, j] = float(acc[m, k, i, j]) + wgt * t[m]
                if span:
                    for m in range(nm):
                        acc[m, i, j] = float(acc[m, i, j]) + wgt * col[m]
    return acc


@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=str)
@pytest.mark.parametrize("cls", CLASSES)
def test_statement_equals_the_literal_loop(cls, shape):
    for n, run in enumerate(S.runs(cls, shape)):
        if cls == "nonfinite" and n % 4 not in (0, 1):
            continue      # every field and every kind still occurs
        for nm in COUNTS:
            for span in (True, False):
                want = S.reference(cls, shape, n, nm, span)
                got = loop_run(run, shape, nm, span)
                assert same_bits(got, want), (run.name, nm, span, S.describe_difference(got, want))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("cls", EXACT)
def test_exact_classes_do_not_depend_on_the_plane_order(cls, shape):
    for n, run in enumerate(S.runs(cls, shape)):
        flipped = run._replace(samples=tuple(tuple(a[::-1] for a in s) for s in run.samples))
        for nm in (10, 15):
            acc = S.start_array(run, shape, nm, True)
            for s, wgt in zip(flipped.samples, flipped.weights):
                S.accumulate(acc, tuple(np.ascontiguousarray(a) for a in s), wgt, nm, True)
            assert same_bits(acc, S.reference(cls, shape, n, nm, True)), (run.name, nm)


def moment_index(nm, names):
    return [MOMENTS[nm].index(x) for x in names if x in MOMENTS[nm]]


@pytest.mark.parametrize("cls", CLASSES)
def test_classes_hold_what_they_promise(cls):
    for shape in SHAPES:
        nz, ny, nx = shape
        total = {}
        for n, run in enumerate(S.runs(cls, shape)):
            for nm in COUNTS:
                for span in (True, False):
                    ref = S.reference(cls, shape, n, nm, span)
                    cen = census(ref)
                    for k, v in cen.items():
                        total[k] = total.get(k, 0) + v
                    # not NaN against NaN throughout (1e300 on the huge fields: infinities, compared by sign)
                    assert cen["nan"] < cen["n"] / 4, (cls, shape, run.name)
                    assert cen["finite"] > cen["n"] / 2 or run.name == "huge, weight 1e300", (cls, shape, run.name)
                    # the first 9 (10) planes are the smaller count's
                    if nm > 10:
                        assert same_bits(ref[:nm - 5], S.reference(cls, shape, n, nm - 5, span))
                    if cls == "nonfinite" and len(run.planted) == 1:
                        (name, cell), = run.planted
                        clean = S.reference(cls, shape, 0, nm, span)
                        where = (slice(None),) + (cell[1:] if span else cell)
                        hit = np.zeros(ref.shape, bool)
                        hit[where][moment_index(nm, CONTAINS[name])] = True
                        assert not np.isfinite(ref[hit]).any() and np.isfinite(ref[~hit]).all()
                        assert same_bits(ref[~hit], clean[~hit])
                    if cls == "nonfinite" and len(run.planted) == 2 and nz > 1:
                        col = (slice(None),) + run.planted[0][1][1:]
                        if span:      # +Inf and -Inf meet in the column: u = NaN, uu = +Inf
                            assert np.isnan(ref[col][0]) and ref[col][3] == np.inf
                    if cls == "accumulator" and run.start:
                        clean = S.reference(cls, shape, 1, nm, span).reshape(-1)
                        flat = ref.reshape(-1)
                        spots = [w for w, _ in run.start]
                        rest = np.ones(flat.size, bool)
                        rest[spots] = False
                        assert same_bits(flat[rest], clean[rest])
                        assert flat[spots[0]] == np.inf and np.isnan(flat[spots[1]])
                        assert flat[spots[2]] == clean[spots[2]] and flat[spots[3]] == 1e300 + clean[spots[3]]
                    if cls == "mixed":
                        ab = S.abs_reference(cls, shape, n, nm, span)
                        assert np.isfinite(ab).all() and (ab[:3] > 0).all()
        print("stats", cls, shape, total)
        if cls == "subnormal":
            assert total["below_flt_min"] > total["n"] / 2 and total["nan"] == total["inf"] == 0
        if cls == "huge":
            assert total["finite"] == total["n"]
            ref = S.reference(cls, shape, 0, 9, True)
            assert np.abs(ref[3:6]).max() >= float(S.FLT_MAX) ** 2 / 4      # a FLT_MAX^2 survived the weights
        if cls == "unit":
            assert total["finite"] == total["n"] and total["below_flt_min"] == 0
        if cls == "signed_zero":
            assert total["neg_zero"] > 0 and total["finite"] == total["n"]
            assert total["neg_zero"] < total["n"]      # the column sums start from +0.0
        if cls == "weights":
            assert total["nan"] > 0 and total["inf"] > 0 and total["below_flt_min"] > 0
        if cls in ("nonfinite", "accumulator"):
            assert total["nan"] > 0 and total["inf"] > 0


def test_the_planted_cells_reach_the_seams():
    nz, ny, nx = shape = (67, 3, 70)
    cells = S.cells_of(shape)
    assert S.chunk_of(nz) == 9 and {c[0] for c in cells} == {0, 66, 27, 35, 8}
    assert {c[1] * nx + c[2] for c in cells} == {0, 63, 64, 209}
    used = {r.planted[0][1] for r in S.runs("nonfinite", shape) if len(r.planted) == 1}
    assert len(used) == 15 and {c[0] for c in used} == {0, 66, 27, 35, 8}
    assert {c[1] * nx + c[2] for c in used} == {0, 63, 64, 209}
    assert S.chunk_of(9) == 2 and S.chunk_of(12) == 2 and S.chunk_of(1) == 1
    assert (9 * 5 * 13) % 2 == 1 and (12 * 5 * 13) % 2 == 0
