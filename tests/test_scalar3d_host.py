"""The passive scalar's NumPy statement (tests/scalar3d_reference.py) against
the statements the project already trusts (CPU only): the advance is the
predictor's per-field arithmetic with f = T, its LES form the LES predictor's,
its periodic form the pad rule; the ordered face assignments are the gather
the kernel uses."""
import numpy as np
import pytest

from les3d_reference import predictor3d_les_numpy, smagorinsky3d_numpy
from ref3d import predictor3d_numpy
from scalar3d_reference import (face_mask, scalar_advance3d_numpy, scalar_bc_heat3d_numpy,
                                scalar_faces3d_gather_numpy, scalar_faces3d_numpy, scalar_heat3d_numpy)
from zper_reference import crop_z, pad_z

F = np.float32
SP = dict(dx=0.013, dy=0.011, dz=0.017)
DT = F(1e-3)
NU = F(0.004)
BC_SHAPES = [(3, 3, 3), (5, 6, 7), (9, 20, 37)]


def fields(shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    u, v, w = (rng.uniform(-3, 3, shape).astype(F) for _ in range(3))
    u.flat[::7] = 0      # the upwind `> 0` branch at exactly 0
    v.flat[3::11] = 0
    for a in (u, v, w):  # tau's dt / 2 branch
        a.flat[5::13] = 0
    return u, v, w


def heat_mask(shape):
    """Positive on cells of row 1, row ny-2, column 1, column nx-2 (every plane
    has them: the mask is 2-D, so planes 1 / nz-2 feed the face planes) and on
    some face cells, where it must have no effect."""
    nz, ny, nx = shape
    rng = np.random.default_rng(7 + sum(shape))
    m = np.where(rng.uniform(size=(ny, nx)) < 0.33, rng.uniform(0.05, 1, (ny, nx)), 0.0)
    m[1, 1], m[1, nx - 2], m[ny - 2, 1], m[ny - 2, nx - 2] = 0.5, 0.25, 0.75, 1.0
    m[1, nx // 2] = m[ny - 2, nx // 2] = m[ny // 2, 1] = m[ny // 2, nx - 2] = 0.6
    m[0, 0], m[0, nx // 2], m[ny - 1, nx - 1], m[ny // 2, 0], m[ny // 2, nx - 1] = 0.5, 0.25, 0.75, 1.0, 0.3
    return m


@pytest.mark.parametrize("supg", [True, False])
@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 20, 37)])
def test_advance_is_the_predictor_with_f_equal_T(shape, supg):
    u, v, w = fields(shape)
    pr = predictor3d_numpy(u, v, w, NU, dt=DT, use_supg=supg, **SP)
    for T, name in ((u, "u_star"), (v, "v_star")):
        got = scalar_advance3d_numpy(T, u, v, w, NU, dt=DT, use_supg=supg, **SP)
        assert got.dtype == F and np.array_equal(got, pr[name]), name
    assert not np.array_equal(pr["u_star"], u)


@pytest.mark.parametrize("supg", [True, False])
@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 20, 37)])
def test_advance_with_nu_t_is_the_les_predictor(shape, supg):
    u, v, w = fields(shape, 1)
    cs = 0.17
    pr = predictor3d_les_numpy(u, v, w, NU, 0.0, cs, dt=DT, use_supg=supg, **SP)
    nu_t = smagorinsky3d_numpy(u, v, w, SP["dx"], SP["dy"], SP["dz"], cs)
    assert np.array_equal(nu_t, pr["nu_t"]) and nu_t.any()
    got = scalar_advance3d_numpy(u, u, v, w, NU, nu_t, 1.0, dt=DT, use_supg=supg, **SP)
    assert np.array_equal(got, pr["u_star"])
    # a Prandtl number changes the result
    other = scalar_advance3d_numpy(u, u, v, w, NU, nu_t, F(1 / 0.85), dt=DT, use_supg=supg, **SP)
    assert not np.array_equal(other, got)


@pytest.mark.parametrize("with_nut", [False, True])
@pytest.mark.parametrize("supg", [True, False])
def test_advance_periodic_is_the_pad_rule(supg, with_nut):
    shape = (6, 7, 9)
    u, v, w = fields(shape, 2)
    rng = np.random.default_rng(5)
    T = rng.uniform(0, 1, shape).astype(F)
    nu_t = rng.uniform(0, 1e-2, shape).astype(F) if with_nut else None
    ip = F(1 / 0.85)
    got = scalar_advance3d_numpy(T, u, v, w, NU, nu_t, ip, dt=DT, use_supg=supg, periodic_z=True, **SP)
    want = crop_z(scalar_advance3d_numpy(pad_z(T), pad_z(u), pad_z(v), pad_z(w), NU,
                                         None if nu_t is None else pad_z(nu_t), ip, dt=DT, use_supg=supg, **SP))
    assert np.array_equal(got, want)
    # every plane is interior in z; the four x / y faces copy through
    plain = scalar_advance3d_numpy(T, u, v, w, NU, nu_t, ip, dt=DT, use_supg=supg, **SP)
    assert np.array_equal(got[1:-1], plain[1:-1])
    assert not np.array_equal(got[0, 1:-1, 1:-1], T[0, 1:-1, 1:-1])
    assert not np.array_equal(got[-1, 1:-1, 1:-1], T[-1, 1:-1, 1:-1])
    f = face_mask(shape, True)
    assert np.array_equal(got[f], T[f])


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", BC_SHAPES)
def test_ordered_face_assignments_are_the_clamp_gather(shape, periodic):
    rng = np.random.default_rng(sum(shape))
    T0 = rng.uniform(0, 1, shape).astype(F)
    m = heat_mask(shape)
    for fs in (0.5, 1.0):
        heated = T0.copy()
        stats = scalar_heat3d_numpy(heated, m, 1.0, fs, periodic)
        faces = face_mask(shape, periodic)
        assert np.array_equal(heated[faces], T0[faces])       # the mask has no effect on face cells
        assert stats["n"] == int((np.broadcast_to(m > 0, shape) & ~faces).sum()) > 0
        assert not np.array_equal(heated, T0)
        ordered = heated.copy()
        scalar_faces3d_numpy(ordered, 0.25, periodic)
        gathered = scalar_faces3d_gather_numpy(heated, 0.25, periodic)
        assert np.array_equal(ordered, gathered)
        assert np.array_equal(ordered[~faces], heated[~faces])
        # face cells copy heated values: e.g. the outlet of row 1 is the heated (k, 1, nx-2)
        nz, ny, nx = shape
        assert ordered[1, 1, nx - 1] == heated[1, 1, nx - 2] != T0[1, 1, nx - 2]
        assert (ordered[:, :, 0] == F(0.25)).all()
        # the whole stage is the two in order
        both = T0.copy()
        s2 = scalar_bc_heat3d_numpy(both, m, 0.25, 1.0, fs, periodic)
        assert np.array_equal(both, ordered) and s2 == stats


@pytest.mark.parametrize("shape", BC_SHAPES)
def test_heating_limits(shape):
    rng = np.random.default_rng(sum(shape))
    T0 = rng.uniform(0, 1, shape).astype(F)
    m = heat_mask(shape)
    faces = face_mask(shape)
    T = T0.copy()
    s = scalar_bc_heat3d_numpy(T, m, 0.0, 1.0, 0.0)           # force_strength 0
    assert np.array_equal(T[~faces], T0[~faces]) and s["heat"] == 0.0 and s["abs"] == 0.0
    T = T0.copy()
    scalar_heat3d_numpy(T, np.where(m > 0, 1.0, 0.0), 0.7, 1.0)  # m = 1, s = 1
    sel = np.broadcast_to(m > 0, shape) & ~faces
    assert (T[sel] == F(0.7)).all() and np.array_equal(T[~sel], T0[~sel])
    T = T0.copy()
    assert scalar_bc_heat3d_numpy(T, None, 0.0, 1.0, 1.0)["n"] == 0   # no mask: faces only
    assert np.array_equal(T[~faces], T0[~faces])
