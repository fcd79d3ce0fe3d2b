"""The flow-statistics kernels of stats3d.hip on the GPU at edge values
(tests/stats3d_edge_reference.py): all four moment counts through
K.accumulate_flow_stats3d and K.accumulate_flow_scalar_stats3d, in span and in
full mode, on shapes that reach the chunk seams of the eight z-waves, the
unroll tail, a partial 64-column tile, the two-halves combine of the 14 and
15 moment kernels and both full-mode kernels.

Bar: ``same_bits`` with the NumPy statement for every class whose sums are
exact (non-finite cells, subnormal, huge and unit fields, signed zeros, odd
weights, odd accumulators); ``mixed`` depends on the order of the sums and is
held to the project's stats_bound, and to the same bits run to run.
tests/test_stats3d_edge_host.py pins the statement to literal loops on the
same runs.
"""
import functools

import numpy as np
import pytest
import torch

import stats3d_edge_reference as S
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import CfdError
from stats3d_edge_reference import COUNTS, EXACT, SHAPES, describe_difference, same_bits, stats_bound

pytestmark = pytest.mark.gpu


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=8)
def dev_samples(cls, shape, index):
    run = S.runs(cls, shape)[index]
    return [[torch.from_numpy(np.array(a, order="C")).to("cuda") for a in s] for s in run.samples]


def accumulate(acc, sample, weight, nm, span):
    u, v, w, nu_t, T = sample
    nt = nu_t if nm in (10, 15) else None
    if nm <= 10:
        return K.accumulate_flow_stats3d(u, v, w, acc, weight, span, nu_t=nt)
    return K.accumulate_flow_scalar_stats3d(u, v, w, T, acc, weight, span, nu_t=nt)


def run_gpu(cls, shape, index, nm, span):
    run = S.runs(cls, shape)[index]
    acc = torch.from_numpy(S.start_array(run, shape, nm, span)).to("cuda")
    for s, wgt in zip(dev_samples(cls, shape, index), run.weights):
        accumulate(acc, s, wgt, nm, span)
    return host(acc)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("cls", EXACT)
def test_exact_runs_same_bits(cls, shape):
    bad, compared = [], 0
    for n, run in enumerate(S.runs(cls, shape)):
        for nm in COUNTS:
            for span in (True, False):
                want = S.reference(cls, shape, n, nm, span)
                got = run_gpu(cls, shape, n, nm, span)
                compared += 1
                if not same_bits(got, want):
                    bad.append((run.name, nm, "span" if span else "full", describe_difference(got, want)))
    print("stats", cls, shape, compared, "arrays compared")
    assert compared
    assert not bad, f"{len(bad)} differ; the first: " + "; ".join(str(b) for b in bad[:6])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mixed_magnitudes_within_the_bound_and_deterministic(shape):
    worst, compared = 0.0, 0
    for n, run in enumerate(S.runs("mixed", shape)):
        for nm in COUNTS:
            for span in (True, False):
                ref = S.reference("mixed", shape, n, nm, span)
                ab = S.abs_reference("mixed", shape, n, nm, span)
                got = run_gpu("mixed", shape, n, nm, span)
                samples = len(run.samples)
                bound = stats_bound(samples * shape[0] if span else samples, samples, ab)
                err = np.abs(got - ref)
                assert np.isfinite(got).all() and (err <= bound).all(), (nm, span, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                compared += 1
                assert np.array_equal(run_gpu("mixed", shape, n, nm, span), got), (nm, span)
    print("stats mixed", shape, compared, "arrays compared, worst err / bound", worst)


@pytest.mark.parametrize("weight", S.REFUSED_WEIGHTS, ids=repr)
def test_a_non_finite_weight_is_refused_before_any_launch(weight):
    shape = (9, 5, 13)
    sample = dev_samples("unit", shape, 0)[0]
    for nm in COUNTS:
        for span in (True, False):
            acc = torch.full(S.acc_shape(shape, nm, span), 3.0, dtype=torch.float64, device="cuda")
            with pytest.raises(CfdError, match="weight"):
                accumulate(acc, sample, weight, nm, span)
            assert (host(acc) == 3.0).all()
