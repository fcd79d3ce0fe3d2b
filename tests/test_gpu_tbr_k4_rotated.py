"""The K = 4 Jacobi pass with rotated level queues (jacobi3d_tbr<4, 11, 2>,
march unrolled by 3): bit-identical to K single sweeps (oracle.jacobi3d).

The rotated march runs whole groups of 3 z-steps (the extra ones store
nothing), level 1 reads planes z and z + 1 from the LDS slot ring, and short
z-chunks keep the shifting-queue instantiation.  Shapes: step counts
(planes + 6) congruent to 0, 1, 2 mod 3; one, two and three x-segments with a
partial last one; a partial last y-tile; a degenerate grid.  z-chunks of 1, 5,
7 planes run the shifting instantiation and the march's start / end clipping;
the long chunks of `DEEP` run the rotated one with 0, 1 and 2 extra steps.
All three first-pass forms are covered: the solve from zeros with a workspace
(zero start + rhs forming), the solve from a guess with a workspace (rhs
forming) and the plain passes without one.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import call

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, DT = 0.06, np.float32(3e-3)

SHAPES = [(11, 40, 16), (12, 47, 264), (13, 30, 520), (5, 4, 8), (40, 31, 520)]
ZCHUNKS = [0, 1, 5, 7]
# (shape, z-chunk): chunks long enough for the rotated march (the launcher
# keeps shifting queues below 48 steps per step of round-up): 97, 98, 99, 50
# and 68 steps per chunk -- two, one, no, one and one extra steps -- each with
# a shorter, clipped last chunk
DEEP = [((100, 12, 264), 91), ((100, 12, 264), 92), ((100, 12, 264), 93), ((52, 20, 264), 44),
        ((72, 31, 520), 62)]


def dev(a):
    return torch.tensor(a, device=DEV)  # (a copy: the shared inputs stay read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def last_shape():
    v = [ctypes.c_int() for _ in range(4)]
    call("cfd_get_last_tbr_shape", *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


@pytest.fixture(autouse=True)
def _reset_tuning():
    call("cfd_reset_tuning")
    yield
    call("cfd_reset_tuning")


@functools.lru_cache(maxsize=None)
def fields(shape):
    rng = np.random.default_rng(31)
    div = rng.standard_normal(shape).astype(np.float32)
    phi0 = rng.standard_normal(shape).astype(np.float32)
    div.setflags(write=False)
    phi0.setflags(write=False)
    return div, phi0


@functools.lru_cache(maxsize=None)
def reference(shape, iters, zero):
    div, phi0 = fields(shape)
    ref = oracle.jacobi3d(div, h=H, dt=DT, iters=iters) if zero else oracle.jacobi3d(div, phi0, h=H, dt=DT, iters=iters)
    ref.setflags(write=False)
    return ref


def check_guess(shape, zchunk, iters):
    call("cfd_set_jacobi3d_blocking", 4, 16, zchunk)
    call("cfd_set_jacobi3d_prefetch", 1)
    div, phi0 = fields(shape)
    ref = reference(shape, iters, False)
    phi = dev(phi0)
    for rhs in (None, torch.empty_like(phi)):
        phi.copy_(dev(phi0))
        K.solve_pressure_jacobi3d(phi, dev(div), H, DT, None, iters, rhs_ws=rhs)
        assert np.array_equal(host(phi), ref)
        # the last tall-tile launch is a 4-level pass unless the solve ends
        # with a 2- or 3-level remainder (the workspace solve's iters % 4 = 1
        # splits as 3 + 4 + ... + 2; a 1-level remainder is a single sweep)
        if rhs is None or iters % 4 == 0:
            assert last_shape()[:3] == (4, 11, 2)


def check_zero(shape, zchunk, iters):
    call("cfd_set_jacobi3d_blocking", 4, 16, zchunk)
    call("cfd_set_jacobi3d_prefetch", 1)
    div, _ = fields(shape)
    ref = reference(shape, iters, True)
    for ws in (False, True):
        phi = torch.full(shape, 7.0, dtype=torch.float32, device=DEV)  # (the solve starts from zeros itself)
        rhs = torch.empty_like(phi) if ws else None
        K.solve_pressure_jacobi3d_zero(phi, dev(div), H, DT, iters, rhs_ws=rhs)
        assert np.array_equal(host(phi), ref)
        if not ws or iters % 4 == 0:
            assert last_shape()[:3] == (4, 11, 2)


@pytest.mark.parametrize("iters", [4, 8, 9, 12])
@pytest.mark.parametrize("zchunk", ZCHUNKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_k4_rotated_bitexact(shape, zchunk, iters):
    """Solve from a guess, with and without the rhs workspace: the PRE passes,
    the general-start first pass (rhs forming) and the raw-div passes."""
    check_guess(shape, zchunk, iters)


@pytest.mark.parametrize("iters", [4, 9])
@pytest.mark.parametrize("zchunk", ZCHUNKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_k4_rotated_zero_start_bitexact(shape, zchunk, iters):
    """Solve from zeros: with the workspace the first pass is the zero-start,
    rhs-forming form."""
    check_zero(shape, zchunk, iters)


@pytest.mark.parametrize("iters", [4, 9])
@pytest.mark.parametrize("shape,zchunk", DEEP)
def test_k4_rotated_long_chunks_bitexact(shape, zchunk, iters):
    """z-chunks long enough for the rotated march, with 0, 1 and 2 steps of
    round-up and a shorter last chunk, all first-pass forms."""
    check_guess(shape, zchunk, iters)
    check_zero(shape, zchunk, iters)
