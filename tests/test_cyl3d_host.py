"""The 3-D cylinder channel's host side (no GPU): the NumPy statement of the
boundary conditions and the vorticity (tests/cyl3d_reference.py) against its
own ordered-assignment properties and the 2-D oracle, host_ibm_bbox, the config's
validation, and the two new entry points in the header and the library."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from cfd_simulations_amd import _lib
from cfd_simulations_amd.solver import CylinderChannel3DConfig, OptimizedTurbulentConfig, host_ibm_bbox
from cyl3d_reference import channel_bc_ibm3d_numpy, inlet_numpy, vorticity3d_numpy

F = np.float32
ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("cfd_apply_channel_bc_ibm3d_f32", "cfd_vorticity3d_f32")


def random_case(shape, seed=0):
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    u, v, w = (rng.uniform(-3, 3, shape).astype(F) for _ in range(3))
    m = np.where(rng.uniform(size=(ny, nx)) < 0.33, rng.uniform(0.05, 1, (ny, nx)), 0.0)
    return u, v, w, np.linspace(-1.0, 3.0, ny), m


@pytest.mark.parametrize("shape", [(3, 3, 3), (5, 6, 7), (9, 20, 37)])
@pytest.mark.parametrize("fs", [0.0, 0.5, 1.0])
def test_reference_bc_ordered_assignments(shape, fs):
    u, v, w, y, m = random_case(shape)
    m[0, :], m[-1, 1], m[1, 0], m[1, -1], m[1, -2] = 0.5, 0.25, 0.75, 0.5, 0.3
    u0 = u.copy()
    stats = channel_bc_ibm3d_numpy(u, v, w, y, m, 3.0, 1.5, 1500, fs)
    for f in (u, v, w):  # the walls own their edges
        assert not f[:, 0, :].any() and not f[:, -1, :].any()
    # free slip: the spanwise faces repeat their neighbour planes, after the IBM factor too
    assert np.array_equal(u[0], u[1]) and np.array_equal(v[0], v[1])
    assert np.array_equal(u[-1], u[-2]) and np.array_equal(v[-1], v[-2])
    assert not w[0].any() and not w[-1].any()
    # inlet and outlet, forced where the mask is set
    fac = np.where(m > 0, 1.0 - m * fs, 1.0)
    inlet = inlet_numpy(y, 3.0, 1.5, 1500)
    want = (inlet.astype(np.float64) * fac[:, 0]).astype(F)
    assert np.array_equal(u[1, 1:-1, 0], want[1:-1]) and not v[:, :, 0].any() and not w[:, :, 0].any()
    src = u0[1, 1:-1, -2].astype(np.float64)
    assert np.array_equal(u[1, 1:-1, -2], (src * fac[1:-1, -2]).astype(F))
    assert np.array_equal(u[1, 1:-1, -1], (src * fac[1:-1, -1]).astype(F))
    assert stats["n"] == shape[0] * int((m > 0).sum())
    if fs == 0.0:
        assert not stats["force"].any() and not stats["abs"].any()
    else:
        assert (stats["abs"] > 0).all() and (np.abs(stats["force"]) <= stats["abs"]).all()
    # without a mask: the same faces, no forcing
    a, b, c, _, _ = random_case(shape)
    none = channel_bc_ibm3d_numpy(a, b, c, y, None, 3.0, 1.5, 1500, fs)
    assert none["n"] == 0 and np.array_equal(a[1, 1:-1, 0], inlet[1:-1])
    assert np.array_equal(a[:, 1:-1, -1], a[:, 1:-1, -2])


def test_reference_inlet_is_the_2d_oracle_column():
    c = OptimizedTurbulentConfig(nx=12, ny=9)
    y = np.linspace(c.y_min, c.y_max, c.ny)
    z = np.zeros((c.ny, c.nx), F)
    for step in (0, 7, 1500):
        o = oracle.OracleSolver(c, z, z, np.zeros((c.ny, c.nx), bool), np.zeros((c.ny, c.nx)), y)
        o.step = step
        u2, v2 = np.ones((c.ny, c.nx), F), np.ones((c.ny, c.nx), F)
        o.apply_boundary_conditions(u2, v2)
        u, v, w = (np.ones((4, c.ny, c.nx), F) for _ in range(3))
        channel_bc_ibm3d_numpy(u, v, w, y, None, c.y_max, c.V_inf, step, 0.0)
        for k in range(4):  # every plane is the 2-D channel's
            assert np.array_equal(u[k], u2) and np.array_equal(v[k], v2)


def test_host_ibm_bbox():
    m = np.zeros((9, 14))
    assert host_ibm_bbox(m) == (0, 9, 0, 14)
    m[2, 5], m[6, 3], m[4, 11] = 0.5, 1.0, 1e-300
    m[7, 12] = -1.0  # not > 0
    assert host_ibm_bbox(m) == (2, 7, 3, 12)
    m[0, 0], m[8, 13] = 0.1, 0.1
    assert host_ibm_bbox(m) == (0, 9, 0, 14)
    one = np.zeros((5, 5))
    one[3, 1] = 2.0
    assert host_ibm_bbox(one) == (3, 4, 1, 2)


def test_vorticity_z_component_is_the_2d_vorticity():
    """z-invariant u, v and w = 0: oz of every interior plane is the oracle's
    2-D vorticity, ox = oy = 0 and mag = |oz|."""
    c = OptimizedTurbulentConfig(nx=23, ny=17)
    rng = np.random.default_rng(5)
    u2, v2 = (rng.standard_normal((c.ny, c.nx)).astype(F) for _ in range(2))
    cyl = np.zeros((c.ny, c.nx), bool)
    cyl[5:9, 6:11] = True
    o = oracle.OracleSolver(c, u2, v2, cyl, np.zeros((c.ny, c.nx)), np.zeros(c.ny))
    w2 = o.compute_vorticity()  # float32 arrays over the Python float 2 dx: divisions by f32(2 dx)
    assert w2.dtype == F and np.isnan(w2[cyl]).all() and np.isfinite(w2[~cyl]).all()
    nz = 5
    u, v = (np.ascontiguousarray(np.broadcast_to(a, (nz, c.ny, c.nx))) for a in (u2, v2))
    mask = np.broadcast_to(cyl, u.shape)
    ox, oy, oz, mag = vorticity3d_numpy(u, v, np.zeros_like(u), c.dx, c.dy, 0.3, mask)
    for k in range(1, nz - 1):
        assert np.array_equal(oz[k], w2, equal_nan=True)
        assert np.array_equal(mag[k], np.abs(w2), equal_nan=True)
    fluid = ~mask
    assert not ox[fluid].any() and not oy[fluid].any()
    assert np.isnan(oz[0][cyl]).all() and not oz[0][~cyl].any() and not oz[-1][~cyl].any()


def test_config_defaults_and_validation():
    c = CylinderChannel3DConfig()
    assert (c.nx, c.ny, c.nz) == (600, 180, 120) and (c.x_max, c.y_max, c.z_max) == (20.0, 4.0, 4.0)
    assert c.R_cylinder == 0.5 and c.cylinder_center == (4.0, 2.0) and c.Re == 600.0
    assert c.use_fast_pressure and c.pressure_iterations == 200 and c.smagorinsky_constant == 0.17
    assert c.dz == 4.0 / 119 and not c.use_les
    assert CylinderChannel3DConfig(use_les=True).use_les
    with pytest.raises(ValueError, match="float32"):
        CylinderChannel3DConfig(memory_efficient=False)
    with pytest.raises(ValueError, match="supg_tau"):
        CylinderChannel3DConfig(supg_tau="sloppy")


def test_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cfdsim.h").read_text(), flags=re.S)
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(L, name), name
    assert len(_lib.PROTOTYPES["cfd_apply_channel_bc_ibm3d_f32"][1]) == 18
    assert len(_lib.PROTOTYPES["cfd_vorticity3d_f32"][1]) == 16


def test_host_refusals_need_no_gpu():
    """Argument validation runs before any device work."""
    L = _lib.lib()
    p = [ctypes.c_void_p(4096 * (q + 1)) for q in range(8)]  # never dereferenced
    bc = lambda *a: L.cfd_apply_channel_bc_ibm3d_f32(*a, None, None)  # noqa: E731
    geo = (1.0, 1.0, 0, 0.5)
    assert bc(p[0], p[1], None, p[3], p[4], 4, 5, 6, *geo, 0, 5, 0, 6) == -1 and b"null" in L.cfd_last_error()
    assert bc(p[0], p[1], p[0], p[3], p[4], 4, 5, 6, *geo, 0, 5, 0, 6) == -1 and b"three" in L.cfd_last_error()
    assert bc(p[0], p[1], p[2], p[3], p[4], 2, 5, 6, *geo, 0, 5, 0, 6) == -1
    for box in ((0, 6, 0, 6), (0, 5, 0, 7), (-1, 5, 0, 6), (3, 2, 0, 6), (2, 2, 0, 6), (0, 5, 4, 4)):
        assert bc(p[0], p[1], p[2], p[3], p[4], 4, 5, 6, *geo, *box) == -1 and b"box" in L.cfd_last_error(), box
    vort = lambda *a: L.cfd_vorticity3d_f32(*a, 4, 5, 6, 0.1, 0.1, 0.1, None)  # noqa: E731
    assert vort(p[0], p[1], p[2], None, None, None, None, None, None) == -1 and b"output" in L.cfd_last_error()
    assert vort(p[0], p[1], p[2], None, p[3], p[1], None, None, None) == -1 and b"alias" in L.cfd_last_error()
    assert vort(p[0], None, p[2], None, p[3], None, None, None, None) == -1
