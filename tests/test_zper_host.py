"""The spanwise-periodic statements of tests/zper_reference.py on the CPU, and
the config of the periodic cylinder channel (no GPU).

rbgs3d_zper_numpy is tied to the pinned C oracle in its non-periodic mode, to
a per-cell loop with the plane index modulo nz on a small grid, and to the
colour rule by shift equivariance; the pad rule is tied to an explicit np.roll
statement of the divergence."""
import functools

import numpy as np
import pytest

import oracle
from cfd_simulations_amd.solver import CylinderChannel3DConfig
from ref3d import divergence3d_numpy
from zper_reference import (crop_z, divergence3d_zper_numpy, pad_z, perturbed_u, rbgs3d_zper_numpy)

F = np.float32
SP = dict(dx=0.05, dy=0.04, dz=0.06)
DT = F(1e-2)


@functools.lru_cache(maxsize=None)
def problem(shape, seed):
    rng = np.random.default_rng(seed)
    div = rng.standard_normal(shape).astype(F) * F(1e-3)
    m2 = rng.uniform(size=shape[1:]) < 0.15
    m2[1, 1] = m2[0, 2] = m2[shape[1] - 2, shape[2] - 2] = True
    phi0 = rng.standard_normal(shape).astype(F) * F(1e-4)
    for a in (div, m2, phi0):
        a.setflags(write=False)
    return div, m2, phi0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("start", [False, True], ids=["zeros", "phi0"])
def test_nonperiodic_mode_is_the_oracle(masked, start):
    shape = (7, 9, 14)
    div, m2, phi0 = problem(shape, 3)
    m3 = np.broadcast_to(m2, shape) if masked else None
    p0 = phi0 if start else None
    mc = []
    rbgs3d_zper_numpy(div, p0, dt=DT, iters=12, tol=0.0, mask2d=m2 if masked else None, periodic=False, maxc=mc,
                      **SP)
    assert len(mc) == 12 and mc[5] < min(mc[:5])
    tol_stop = float((np.float64(mc[5]) + np.float64(min(mc[:5]))) / 2)   # stops after iteration 6
    for tol, iters in ((0.0, 5), (0.0, 12), (tol_stop, 12)):
        ref, n_ref = oracle.rbgs3d(div, p0, dt=DT, iters=iters, tol=tol, mask=m3, **SP)
        got, n = rbgs3d_zper_numpy(div, p0, dt=DT, iters=iters, tol=tol, mask2d=m2 if masked else None,
                                   periodic=False, **SP)
        assert n == n_ref == (6 if tol else iters)
        assert got.dtype == F and np.array_equal(got, ref)
    if masked and start:
        assert np.array_equal(got[m3], phi0[m3])


def _loop_zper(div, phi0, m2, iters, tol):
    """oracle_rbgs3d_f32 cell by cell with z over all planes and the plane
    neighbours modulo nz."""
    nz, ny, nx = div.shape
    phi = phi0.copy()
    cx, cy, cz = (F(1.0 / (d * d)) for d in (SP["dx"], SP["dy"], SP["dz"]))
    cd = F(1.0 / (2.0 * (1.0 / SP["dx"] ** 2 + 1.0 / SP["dy"] ** 2 + 1.0 / SP["dz"] ** 2)))
    dt_inv = F(1.0) / DT
    for it in range(iters):
        mx = F(0)
        for colour in (0, 1):
            for z in range(nz):
                for i in range(1, ny - 1):
                    for j in range(1 + (z + i + colour) % 2, nx - 1, 2):
                        if m2 is not None and m2[i, j]:
                            continue
                        rhs = -div[z, i, j] * dt_inv
                        a = cx * (phi[z, i, j + 1] + phi[z, i, j - 1])
                        b = cy * (phi[z, i + 1, j] + phi[z, i - 1, j])
                        e = cz * (phi[(z + 1) % nz, i, j] + phi[(z - 1) % nz, i, j])
                        pn = (((a + b) + e) - rhs) * cd
                        mx = max(mx, abs(pn - phi[z, i, j]))
                        phi[z, i, j] = pn
        if mx < F(tol):
            return phi, it + 1
    return phi, iters


@pytest.mark.parametrize("masked", [False, True])
def test_periodic_mode_is_the_modulo_loop(masked):
    shape = (4, 6, 9)
    div, m2, phi0 = problem(shape, 8)
    m = m2 if masked else None
    mc = []
    rbgs3d_zper_numpy(div, phi0, dt=DT, iters=8, tol=0.0, mask2d=m, maxc=mc, **SP)
    tol_stop = float((np.float64(mc[3]) + np.float64(min(mc[:3]))) / 2)
    assert mc[3] < min(mc[:3])
    for tol, iters in ((0.0, 3), (tol_stop, 8)):
        ref, n_ref = _loop_zper(div, phi0, m, iters, tol)
        got, n = rbgs3d_zper_numpy(div, phi0, dt=DT, iters=iters, tol=tol, mask2d=m, **SP)
        assert n == n_ref == (4 if tol else iters)
        assert np.array_equal(got, ref)
    # every plane was updated, the x / y faces kept their values
    assert all((got[k, 1:-1, 1:-1] != phi0[k, 1:-1, 1:-1]).any() for k in range(4))
    for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)):
        assert np.array_equal(got[sl], phi0[sl])


def test_periodic_solve_is_shift_equivariant_by_two_planes_only():
    """Rolling div and phi0 by 2 planes rolls the result by 2 planes bit for
    bit (the colour of a cell depends on z's parity); rolling by 1 does not."""
    shape = (6, 7, 10)
    div, m2, phi0 = problem(shape, 21)
    kw = dict(dt=DT, iters=5, tol=0.0, mask2d=m2, **SP)
    base, n = rbgs3d_zper_numpy(div, phi0, **kw)
    two, n2 = rbgs3d_zper_numpy(np.roll(div, 2, axis=0), np.roll(phi0, 2, axis=0), **kw)
    assert n == n2 == 5 and np.array_equal(two, np.roll(base, 2, axis=0))
    one, _ = rbgs3d_zper_numpy(np.roll(div, 1, axis=0), np.roll(phi0, 1, axis=0), **kw)
    assert not np.array_equal(one, np.roll(base, 1, axis=0))
    # the non-periodic solve is not equivariant at all
    flat, _ = rbgs3d_zper_numpy(div, phi0, periodic=False, **kw)
    assert not np.array_equal(flat, base)


def test_pad_rule_divergence_is_the_roll_statement():
    shape = (5, 6, 8)
    rng = np.random.default_rng(5)
    u, v, w = (rng.standard_normal(shape).astype(F) for _ in range(3))
    assert pad_z(u).shape == (7, 6, 8) and np.array_equal(pad_z(u)[0], u[-1]) and np.array_equal(pad_z(u)[-1], u[0])
    assert np.array_equal(crop_z(pad_z(u)), u)
    cx, cy, cz = F(0.5 / SP["dx"]), F(0.5 / SP["dy"]), F(0.5 / SP["dz"])
    want = np.zeros(shape, F)
    want[:, 1:-1, 1:-1] = (((u[:, 1:-1, 2:] - u[:, 1:-1, :-2]) * cx + (v[:, 2:, 1:-1] - v[:, :-2, 1:-1]) * cy)
                           + (np.roll(w, -1, axis=0) - np.roll(w, 1, axis=0))[:, 1:-1, 1:-1] * cz)
    got = divergence3d_zper_numpy(u, v, w, **SP)
    assert got.dtype == F and np.array_equal(got, want)
    # the interior planes are the non-periodic divergence's; planes 0 and nz-1 are not zero any more
    flat = divergence3d_numpy(u, v, w, **SP)
    assert np.array_equal(got[1:-1], flat[1:-1]) and got[0].any() and got[-1].any() and not flat[0].any()


def test_config_defaults_and_periodic_dz():
    c = CylinderChannel3DConfig()
    assert c.spanwise_bc == "free_slip" and c.spanwise_perturbation == 0.0
    assert c.dz == (c.z_max - c.z_min) / (c.nz - 1)
    p = CylinderChannel3DConfig(spanwise_bc="periodic")
    assert p.dz == (p.z_max - p.z_min) / p.nz and p.nz * p.dz == p.z_max - p.z_min
    q = CylinderChannel3DConfig(nz=10, z_min=0.5, z_max=1.75, spanwise_bc="periodic", spanwise_perturbation=0.05)
    assert q.dz == 1.25 / 10 and q.spanwise_perturbation == 0.05
    assert CylinderChannel3DConfig(nz=4, spanwise_bc="periodic").dz == 1.0


def test_config_refusals():
    with pytest.raises(ValueError, match="spanwise_bc"):
        CylinderChannel3DConfig(spanwise_bc="slip")
    for nz in (9, 3, 2, 121):
        with pytest.raises(ValueError, match="even nz"):
            CylinderChannel3DConfig(nz=nz, spanwise_bc="periodic")
    with pytest.raises(ValueError, match="red-black GS"):
        CylinderChannel3DConfig(spanwise_bc="periodic", use_fast_pressure=False)
    # the free-slip channel takes any nz and the Jacobi as before
    assert CylinderChannel3DConfig(nz=9, use_fast_pressure=False).dz == 4.0 / 8


def test_perturbed_start():
    rng = np.random.default_rng(2)
    u2 = rng.standard_normal((5, 7)).astype(F)
    z = 0.5 + np.arange(8) * 0.25
    assert np.array_equal(perturbed_u(u2, z, 0.5, 2.5, 0.0), np.broadcast_to(u2, (8, 5, 7)))
    p = perturbed_u(u2, z, 0.5, 2.5, 0.05)
    assert p.dtype == F and np.array_equal(p[0], (u2.astype(np.float64) * 1.05).astype(F))
    assert np.array_equal(p[4], (u2.astype(np.float64) * (1.0 + 0.05 * np.cos(np.pi))).astype(F))
    assert not np.array_equal(p[1], p[2])
