"""The NumPy statement of the 3-D LES arithmetic (tests/les3d_reference.py) on
the CPU: its array code against a per-cell scalar float32 loop, its reduction
to the 2-D statement's q on z-invariant fields, cs = 0 against the scalar-nu
predictor, and the LES config."""
import math

import numpy as np
import pytest

from cfd_simulations_amd.solver import LesCavity3DConfig, LidDrivenCavity3DConfig
from les3d_reference import (nu_eff3d_numpy, predictor3d_les_numpy, predictor3d_nu_numpy, smag3d_constant,
                             smagorinsky3d_numpy)
from les_reference import smagorinsky_numpy
from ref3d import pred_constants, predictor3d_numpy

F = np.float32
SP = dict(dx=0.013, dy=0.011, dz=0.017)
CS = 0.17


def fields(shape, seed):
    rng = np.random.default_rng(seed)
    u, v, w = (rng.standard_normal(shape).astype(F) for _ in range(3))
    u[1:3, 1:3, 1:4], v[1:3, 1:3, 1:4], w[1:3, 1:3, 1:4] = 0, 0, 0
    return u, v, w


def scalar_smagorinsky(u, v, w, dx, dy, dz, cs):
    """smagorinsky3d_numpy's arithmetic, one float32 scalar operation at a time."""
    kx, ky, kz = F(1.0 / dx), F(1.0 / dy), F(1.0 / dz)
    c2 = F((cs * (dx * dy * dz) ** (1.0 / 3.0)) ** 2)
    out = np.zeros_like(u)
    nz, ny, nx = u.shape
    for z in range(1, nz - 1):
        for j in range(1, ny - 1):
            for i in range(1, nx - 1):
                ux, uy, uz = ((u[z, j, i + 1] - u[z, j, i]) * kx, (u[z, j + 1, i] - u[z, j, i]) * ky,
                              (u[z + 1, j, i] - u[z, j, i]) * kz)
                vx, vy, vz = ((v[z, j, i + 1] - v[z, j, i]) * kx, (v[z, j + 1, i] - v[z, j, i]) * ky,
                              (v[z + 1, j, i] - v[z, j, i]) * kz)
                wx, wy, wz = ((w[z, j, i + 1] - w[z, j, i]) * kx, (w[z, j + 1, i] - w[z, j, i]) * ky,
                              (w[z + 1, j, i] - w[z, j, i]) * kz)
                d = (ux * ux + vy * vy) + wz * wz
                sxy, sxz, syz = uy + vx, uz + wx, vz + wy
                o = (sxy * sxy + sxz * sxz) + syz * syz
                q = F(2) * d + o
                r = c2 * np.sqrt(q)
                assert type(r) is F
                out[z, j, i] = r
    return out


def test_array_code_equals_scalar_loop():
    u, v, w = fields((5, 6, 7), 21)
    got = smagorinsky3d_numpy(u, v, w, cs=CS, **SP)
    assert got.dtype == F
    assert np.array_equal(got, scalar_smagorinsky(u, v, w, SP["dx"], SP["dy"], SP["dz"], CS))
    face = np.ones(u.shape, bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert not got[face].any() and (got[~face] > 0).sum() > 40 and (got[1, 1, 1:3] == 0).all()
    c2 = smag3d_constant(cs=CS, **SP)
    assert type(c2) is F and c2 == pytest.approx((CS * np.cbrt(SP["dx"] * SP["dy"] * SP["dz"])) ** 2, rel=1e-6)


def test_z_invariant_reduces_to_the_2d_q():
    """On z-invariant u, v and w = 0 every z term is an exact zero: nu_t is
    c2 sqrt(q) of the 2-D statement's q bit for bit."""
    dx, dy, dz = 0.013, 0.011, 0.02
    rng = np.random.default_rng(5)
    u2, v2 = (rng.standard_normal((9, 12)).astype(F) for _ in range(2))
    u2[3:5, 2:6], v2[3:5, 2:6] = 0, 0
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (5,) + a.shape))  # noqa: E731
    got = smagorinsky3d_numpy(rep(u2), rep(v2), np.zeros((5, 9, 12), F), dx, dy, dz, CS)
    # the 2-D statement's q (tests/les_reference.py), restated so that q itself is at hand ...
    c, d = u2[1:-1, 1:-1], v2[1:-1, 1:-1]
    dudx, dudy = (u2[1:-1, 2:] - c) * F(1.0 / dx), (u2[2:, 1:-1] - c) * F(1.0 / dy)
    dvdx, dvdy = (v2[1:-1, 2:] - d) * F(1.0 / dx), (v2[2:, 1:-1] - d) * F(1.0 / dy)
    q2 = 2 * (dudx * dudx + dvdy * dvdy) + (dudy + dvdx) * (dudy + dvdx)
    assert q2.dtype == F
    # ... and checked against that statement
    want2 = np.zeros_like(u2)
    want2[1:-1, 1:-1] = F((CS * math.sqrt(dx * dy)) ** 2) * np.sqrt(q2)
    assert np.array_equal(smagorinsky_numpy(u2, v2, dx, dy, CS), want2)
    want = smag3d_constant(dx, dy, dz, CS) * np.sqrt(q2)
    for z in range(1, 4):
        assert np.array_equal(got[z, 1:-1, 1:-1], want)
    assert (want > 0).any() and not got[0].any() and not got[-1].any()


@pytest.mark.parametrize("use_supg", [True, False])
def test_cs_zero_gives_the_scalar_nu_bits(use_supg):
    u, v, w = fields((5, 6, 7), 22)
    nu, art, dt = F(0.01), F(0.001), F(2e-3)
    les = predictor3d_les_numpy(u, v, w, nu, art, 0.0, dt=dt, use_supg=use_supg, **SP)
    assert not les["nu_t"].any()
    ref = predictor3d_numpy(u, v, w, F(nu + F(0.0)) + art, dt=dt, use_supg=use_supg, **SP)
    for name in ("u_star", "v_star", "w_star", "tau"):
        assert np.array_equal(les[name], ref[name]), name


def test_array_nu_cell_against_a_scalar_evaluation():
    """A cell of the array-nu predictor is the scalar predictor's with that
    cell's nu_eff (tau and the Laplacian factor both take it)."""
    u, v, w = fields((5, 6, 7), 23)
    nu_t = smagorinsky3d_numpy(u, v, w, cs=CS, **SP)
    ne = nu_eff3d_numpy(nu_t, 0.01, 0.001)
    got = predictor3d_nu_numpy(u, v, w, ne, dt=F(2e-3), **SP)
    for cell in ((2, 3, 4), (3, 4, 5), (1, 1, 1)):
        one = predictor3d_numpy(u, v, w, ne[cell], dt=F(2e-3), **SP)
        for name in ("u_star", "v_star", "w_star", "tau"):
            assert got[name][cell] == one[name][cell]
    assert pred_constants(**SP)["ux"] == F(1.0 / SP["dx"])


def test_les_config_3d():
    c = LesCavity3DConfig()
    assert c.use_les is True and c.smagorinsky_constant == 0.17
    assert (c.nz, c.ny, c.nx) == (128, 128, 128) and c.dz == 1.0 / 127 and c.artificial_viscosity == 0.001
    assert isinstance(c, LidDrivenCavity3DConfig)
    off = LesCavity3DConfig(use_les=False, nz=17)
    assert off.use_les is False and off.dz == 1.0 / 16
    with pytest.raises(ValueError):
        LidDrivenCavity3DConfig(use_les=True)
    with pytest.raises(ValueError):
        LesCavity3DConfig(memory_efficient=False)
