"""CPU side of the slab edge tests (no GPU).

* For every case of tests/slab_edge_reference.py the emulated slab schedule
  -- R ranks, ``SlabPlan`` scatter and exchanges, one oracle sweep per level
  on the plane range -- equals the single-domain oracle bit for bit, for
  every depth of pass the ghosts allow; the red-black emulation also in its
  iteration count, at zero and at both positive tolerances.  So the cases of
  tests/test_gpu_slab_edges.py are decomposable as the drivers decompose them,
  and the single-domain oracle may serve as their reference.
* A negative control pins what a mask demands of a decomposed Jacobi solve:
  without zeroing the masked cells of the owned planes after each pass, every
  masked case that starts from a guess differs from the oracle.  (From zeros
  the step changes nothing: those cells are zero already.)
* ``SlabPlan`` at its limits: every level range of a pass stays inside the
  local array and off the global Dirichlet planes, down to slabs of ``ghost``
  planes; one plane fewer is refused; a rank that updates nothing still
  exchanges.
"""
import numpy as np
import pytest

import slab_edge_reference as E
from cfd_simulations_amd.slab import SlabPlan
from slab_edge_reference import CASES

JACOBI = [n for n, c in CASES.items() if c.op == "jacobi"]
GS = [n for n, c in CASES.items() if c.op == "gs"]
MASKED_FROM_A_GUESS = [n for n in JACOBI if CASES[n].masked and CASES[n].start == "guess"]


def depths(case):
    return [1] if case.masked else sorted({1, min(2, case.ghost), case.ghost})


@pytest.mark.parametrize("name", JACOBI)
def test_emulated_jacobi_equals_the_oracle(name):
    case = CASES[name]
    ref = E.reference(case)
    for K in depths(case):
        assert np.array_equal(E.emulate_jacobi(case, K), ref), K


@pytest.mark.parametrize("name", GS)
def test_emulated_rbgs_equals_the_oracle(name):
    case = CASES[name]
    for tol, want in ((0.0, case.iters),) + case.tols:
        ref, n_ref = E.reference(case, tol)
        assert n_ref == want, (tol, n_ref, want)
        got, n = E.emulate_rbgs(case, tol)
        assert n == n_ref, (tol, n, n_ref)
        assert np.array_equal(got, ref), tol


def test_cases_cover_what_they_name():
    """Conditions the GPU file relies on, not measurements."""
    assert MASKED_FROM_A_GUESS and len(MASKED_FROM_A_GUESS) >= 12
    for name in GS:
        case = CASES[name]
        if case.ny >= 3:    # an odd and an even stop strictly inside the iterations
            assert sorted(n % 2 for _, n in case.tols) == [0, 1], name
            assert all(1 < n < case.iters and tol > 0 for tol, n in case.tols), name
    # the thinnest slabs, a rank that updates nothing, a rank whose only work is its Dirichlet plane
    thin = [CASES[n] for n in E.group("jthin")]
    assert any(c.nz == c.R * c.ghost for c in thin)
    empty = [[p.z_update_end <= p.z_update_begin for p in CASES[n].plans()] for n in E.group("jmask-planes")]
    assert [True, False, True] in empty and [True, True] in empty
    # the overlap threshold: the middle rank's range is 2G planes, then 2G + 1
    spans = {(c.nz, c.ghost): c.plans()[1].z_update_end - c.plans()[1].z_update_begin
             for c in (CASES[n] for n in E.group("jthreshold"))}
    assert spans == {(12, 2): 4, (15, 2): 5, (24, 4): 8, (27, 4): 9}


@pytest.mark.parametrize("name", MASKED_FROM_A_GUESS)
def test_masked_jacobi_needs_the_owned_planes_zeroed(name):
    case = CASES[name]
    assert not np.array_equal(E.emulate_jacobi(case, 1, zeroing=False), E.reference(case))


def limit_plans():
    for R in range(1, 5):
        for G in range(1, 5):
            for nz in range(max(R * G, 2), R * G + 3 * R + 2):
                yield [SlabPlan(nz, R, r, G) for r in range(R)]


def test_slab_plan_level_ranges_at_the_limits():
    """Level j of a k-level pass runs on [zb - w, ze + w), w = k - j <= G - 1,
    not widened on a Dirichlet side.  It reads one plane beyond each end."""
    ranks = empty = 0
    for plans in limit_plans():
        for p in plans:
            ranks += 1
            zb, ze = p.z_update_begin, p.z_update_end
            fixed_lo, fixed_hi = p.z_lo == 0, p.z_hi == p.nz
            assert p.ghost <= zb <= ze <= p.nz_local + p.ghost
            empty += ze <= zb
            for w in range(p.ghost):
                lo, hi = (zb if fixed_lo else zb - w), (ze if fixed_hi else ze + w)
                if hi <= lo:
                    continue
                assert 0 <= lo - 1 and hi + 1 <= p.nz_total, (p, w)       # the planes it reads
                glob = range(p.z_lo - p.ghost + lo, p.z_lo - p.ghost + hi)   # the planes it writes
                assert 0 not in glob and p.nz - 1 not in glob, (p, w)
                assert glob.start >= 1 and glob.stop <= p.nz - 1, (p, w)
            # a rank with nothing to update still lists its exchanges
            assert len(p.exchanges()) == (p.lo_peer >= 0) + (p.hi_peer >= 0)
            for first, count, peer, recv in p.exchanges():
                q = plans[peer]
                assert count == p.ghost and p.owned().start <= first and first + count <= p.owned().stop
                assert (recv, count, p.rank) in q.receives()
    assert ranks == 439 and empty == 14, (ranks, empty)


def test_slab_plan_refuses_slabs_thinner_than_the_ghosts():
    for R in range(1, 5):
        for G in range(1, 5):
            SlabPlan(R * G, R, R - 1, G)
            if R * G - 1 >= 1:
                with pytest.raises(ValueError):
                    SlabPlan(R * G - 1, R, 0, G)
