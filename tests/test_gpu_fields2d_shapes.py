"""The per-cell 2-D operators on their own (the fields2d_cells.hpp templates
k_supg_tau, k_conv_supg, k_conv_upwind, k_laplacian, k_divergence, k_gradient,
k_project and k_vorticity, in float and in double), each with its own
`j < nx` tail, swept over the shapes the fused predictor is swept over
elsewhere: without an interior, one interior cell, nx on both sides of a wave
and of a 256-column workgroup, several workgroups per row; float32 and
float64; nu_eff as a scalar and as an array; dx != dy.

Every comparison is BIT FOR BIT: tau, the two convections and the Laplacian
against oracle.predictor2d (the C statement pinned to the reference's
fixtures), divergence / gradient / projection / vorticity against the NumPy
statements of tests/diag_reference.py and, in float32, against the C oracle
too.  The C oracle is defined at shapes without an interior as well (its
loops run over nothing and leave the zero fill); it has no float64
divergence or gradient and no projection or vorticity, so there the NumPy
statement is the reference.

The tails of the float64 step -- the plain lexicographic sweep with
k_sub_gradient (clean_divergence_fast), the inlet / outlet and the cavity
walls, the IBM factor and the clip -- follow, each against plain NumPy float64
loops or assignments, bit for bit.
"""
import numpy as np
import pytest
import torch

import oracle
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import call, ptr, stream_handle
from diag_reference import (DX, DY, SHAPES_2D, divergence2d, fields2d, fold_absmax, gradient2d, noise, project2d,
                            vorticity2d)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [np.float32, np.float64]
DT = 2e-5
NU = 1.0 / 600.0 + 5e-4


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared inputs are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(autouse=True)
def _reset_tuning():
    call("cfd_reset_tuning")
    yield
    call("cfd_reset_tuning")


def same(got, want, equal_nan=False):
    got = host(got)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=equal_nan)


def nu_of(shape, dtype, nu_array):
    """(what the wrappers take, what the oracle takes): a scalar in the
    fields' precision, or an array that varies from cell to cell."""
    if not nu_array:
        nu = dtype(NU)
        return float(nu), nu
    ny, nx = shape
    nu = (dtype(NU) * (1 + noise(ny * nx, dtype, seed=6, lo=0.0, hi=1.0))).reshape(shape).astype(dtype)
    return dev(nu), nu


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nu_array", [False, True])
@pytest.mark.parametrize("quiescent", [False, True])
@pytest.mark.parametrize("shape", SHAPES_2D)
def test_predictor_components_bitexact(shape, quiescent, nu_array, dtype):
    """tau, SUPG convection of u and of v given the oracle's tau, upwind
    convection and the Laplacian through the kernels.py wrappers."""
    u, v = fields2d(shape, dtype, quiescent)
    dt = np.float32(DT) if dtype == np.float32 else DT
    nu_in, nu = nu_of(shape, dtype, nu_array)
    ref = oracle.predictor2d(u, v, nu, dx=DX, dy=DY, dt=dt, use_supg=True, dtype=dtype)
    up = oracle.predictor2d(u, v, nu, dx=DX, dy=DY, dt=dt, use_supg=False, dtype=dtype)
    if quiescent and shape[0] > 4 and shape[1] > 4:
        ny, nx = shape
        assert ref["tau"][ny // 4 + 1, nx // 3 + 1] == dtype(dt) / 2  # the |V| <= eps branch is taken
    ud, vd = dev(u), dev(v)
    assert same(K.compute_supg_stabilization_fast(ud, vd, DX, DY, dt, nu_in), ref["tau"])
    tau = dev(ref["tau"])
    assert same(K.compute_convection_supg_fast(ud, vd, ud, DX, DY, tau), ref["conv_u"])
    assert same(K.compute_convection_supg_fast(ud, vd, vd, DX, DY, tau), ref["conv_v"])
    assert same(K.compute_convection_fast(ud, vd, ud, DX, DY), up["conv_u"])
    assert same(K.compute_convection_fast(ud, vd, vd, DX, DY), up["conv_v"])
    assert same(K.compute_laplacian_fast(ud, DX, DY, nu_in), ref["lap_u"])
    assert same(K.compute_laplacian_fast(vd, DX, DY, nu_in), ref["lap_v"])
    assert np.array_equal(up["lap_u"], ref["lap_u"]) and not up["tau"].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quiescent", [False, True])
@pytest.mark.parametrize("shape", SHAPES_2D)
def test_divergence_gradient_project_bitexact(shape, quiescent, dtype):
    u, v = fields2d(shape, dtype, quiescent)
    phi = noise(shape[0] * shape[1], dtype, seed=5).reshape(shape)
    ud, vd, pd = dev(u), dev(v), dev(phi)
    div = divergence2d(u, v, DX, DY)
    gx, gy = gradient2d(phi, DX, DY)
    pu, pv, gmax = project2d(phi, u, v, DX, DY, DT)
    if dtype == np.float32:  # the C statement gives the same bits
        assert np.array_equal(div, oracle.divergence2d(u, v, dx=DX, dy=DY))
        ox, oy = oracle.gradient2d(phi, dx=DX, dy=DY)
        assert np.array_equal(gx, ox) and np.array_equal(gy, oy)
        assert np.array_equal(pu, u - np.float32(DT) * ox) and np.array_equal(pv, v - np.float32(DT) * oy)
    out = torch.zeros(1, dtype=ud.dtype, device=DEV)
    assert same(K.compute_divergence_fast(ud, vd, DX, DY, absmax=out), div)
    assert host(out)[0].tobytes() == fold_absmax(div).tobytes()
    assert same(K.compute_divergence_fast(ud, vd, DX, DY), div)  # absmax = NULL
    dgx, dgy = K.compute_gradient_fast(pd, DX, DY)
    assert same(dgx, gx) and same(dgy, gy)
    out = torch.zeros(1, dtype=ud.dtype, device=DEV)
    du, dv = K.project_velocity(pd, ud, vd, DX, DY, DT, gradmax=out)
    assert same(du, pu) and same(dv, pv) and host(out)[0].tobytes() == gmax.tobytes()
    du, dv = K.project_velocity(pd, ud, vd, DX, DY, DT)  # gradmax = NULL
    assert same(du, pu) and same(dv, pv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES_2D)
def test_vorticity_field_bitexact(shape, dtype):
    """The field with and without a mask: the ring is 0, masked cells are
    NaN, masked ring cells included."""
    ny, nx = shape
    u, v = fields2d(shape, dtype)
    mask = np.random.default_rng(ny * nx + 1).random(shape) < 0.3
    mask[0, 0] = mask[ny - 1, nx - 1] = True  # ring cells
    ud, vd = dev(u), dev(v)
    for mk in (None, mask):
        ref = vorticity2d(u, v, mk, DX, DY)
        md = None if mk is None else dev(mk.astype(np.uint8))
        w = torch.full_like(ud, 7.0)
        if dtype == np.float32:
            call("cfd_vorticity2d_f32", ptr(ud), ptr(vd), ptr(md), ptr(w), ny, nx, DX, DY, stream_handle())
        else:
            call("cfd_vorticity2d_f64", ptr(ud), ptr(vd), ptr(md), ptr(w), None, ny, nx, DX, DY, stream_handle())
        assert same(w, ref, equal_nan=True)
        got = host(w)
        ring = np.ones(shape, bool)
        ring[1:-1, 1:-1] = False
        if mk is None:
            assert not got[ring].any() and not np.isnan(got).any()
        else:
            assert np.isnan(got[mk]).all() and not np.isnan(got[~mk]).any() and not got[ring & ~mk].any()


# ------------------------------------------------- the float64 step's tails
def clean_divergence_f64(u, v, dx, dy, iterations):
    """oracle_clean_divergence2d_f32's loop in float64 with the Python-float
    constants unrounded (v5.py:239-257): div, the phi sweep in serial row-major
    order from phi = 0 (phi carries over between iterations), then u -= gx,
    v -= gy on the interior."""
    u, v = u.copy(), v.copy()
    ny, nx = u.shape
    cx, cy = 1.0 / (dx * dx), 1.0 / (dy * dy)
    cd = 1.0 / (2.0 * (cx + cy))
    phi = np.zeros((ny, nx), np.float64)
    for _ in range(iterations):
        div = divergence2d(u, v, dx, dy)
        for i in range(1, ny - 1):
            for j in range(1, nx - 1):
                a = cx * (phi[i, j + 1] + phi[i, j - 1])
                b = cy * (phi[i + 1, j] + phi[i - 1, j])
                phi[i, j] = ((a + b) - div[i, j]) * cd
        gx, gy = gradient2d(phi, dx, dy)
        u[1:-1, 1:-1] -= gx[1:-1, 1:-1]
        v[1:-1, 1:-1] -= gy[1:-1, 1:-1]
    return u, v


# one interior cell; a few rows and columns; 65 interior rows (the second wave
# holds one row); two full waves; 1028 interior rows (a second band of four
# rows after the 1024-row band); no interior
CLEAN_SHAPES = [(3, 3), (4, 7), (5, 4), (67, 30), (130, 17), (1030, 5), (2, 5), (5, 2)]


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("shape", CLEAN_SHAPES)
def test_clean_divergence_f64_bitexact(shape, iterations):
    u, v = fields2d(shape, np.float64)
    ru, rv = clean_divergence_f64(u, v, DX, DY, iterations)
    if not (shape[0] > 2 and shape[1] > 2):
        assert np.array_equal(ru, u) and np.array_equal(rv, v)
    ud, vd = dev(u), dev(v)
    K.clean_divergence_fast(ud, vd, DX, DY, iterations=iterations)
    assert same(ud, ru) and same(vd, rv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 2), (2, 5), (5, 2), (7, 300)])
def test_lid_bc_exact(shape, dtype):
    """No-slip left, right and bottom walls, then the lid, which owns the top
    corners."""
    ny, nx = shape
    u_lid = 1.1
    u = noise(ny * nx, dtype, seed=11).reshape(shape)
    v = noise(ny * nx, dtype, seed=12).reshape(shape)
    ru, rv = u.copy(), v.copy()
    ru[:, 0] = rv[:, 0] = 0
    ru[:, -1] = rv[:, -1] = 0
    ru[0, :] = rv[0, :] = 0
    ru[-1, :], rv[-1, :] = dtype(u_lid), 0
    ud, vd = dev(u), dev(v)
    call("cfd_apply_lid_bc2d" + ("_f32" if dtype == np.float32 else "_f64"), ptr(ud), ptr(vd), ny, nx, u_lid,
         stream_handle())
    assert same(ud, ru) and same(vd, rv)


@pytest.mark.parametrize("step", [0, 7, 1500])
@pytest.mark.parametrize("shape", [(7, 2), (5, 3), (36, 120)])
def test_bc_f64_exact(shape, step):
    """apply_boundary_conditions (v5.py:349-360) on float64 fields.  Given the
    inlet values, every other cell follows from the assignments exactly; the
    inlet values themselves, rounded to float32, are cfd_apply_bc2d_f32's (both
    kernels form the same double expression on the device)."""
    ny, nx = shape
    y_max, v_inf = 2.0, 1.3
    y = np.linspace(0.0, y_max, ny)
    u = noise(ny * nx, np.float64, seed=13).reshape(shape)
    v = noise(ny * nx, np.float64, seed=14).reshape(shape)
    yd = dev(y)
    ud, vd = dev(u), dev(v)
    call("cfd_apply_bc2d_f64", ptr(ud), ptr(vd), ptr(yd), ny, nx, y_max, v_inf, step, stream_handle())
    got_u = host(ud)
    ru, rv = u.copy(), v.copy()
    ru[:, 0], rv[:, 0] = got_u[:, 0], 0
    ru[:, -1], rv[:, -1] = ru[:, -2], rv[:, -2]
    ru[0, :] = ru[-1, :] = 0
    rv[0, :] = rv[-1, :] = 0
    assert same(ud, ru) and same(vd, rv)
    u32, v32 = dev(u.astype(np.float32)), dev(v.astype(np.float32))
    call("cfd_apply_bc2d_f32", ptr(u32), ptr(v32), ptr(yd), ny, nx, y_max, v_inf, step, stream_handle())
    inlet32 = host(u32)[1:-1, 0]
    assert inlet32.dtype == np.float32 and inlet32.size == ny - 2
    assert got_u[1:-1, 0].astype(np.float32).tobytes() == inlet32.tobytes()
    # |pert| <= the perturbation scale; 1 + pert and the product each round once
    assert np.all(np.abs(got_u[1:-1, 0] - v_inf) <= 0.01 * v_inf * min(1.0, step / 1000.0) + 4 * np.spacing(v_inf))


# one cell, either side of a workgroup, and past the 2048 x 256 threads of the
# grid, so the grid-stride loop wraps
TAIL_SIZES = [1, 255, 257, 2048 * 256 + 3]


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_ibm_f64_exact(n):
    """apply_ibm_fast (v5.py:228-237): cells with a positive mask value are
    scaled by 1 - m fs; zero and negative entries are left alone."""
    fs = 0.37
    u, v = noise(n, np.float64, seed=15), noise(n, np.float64, seed=16)
    m = noise(n, np.float64, seed=17, lo=-0.5, hi=1.0).copy()
    m[(m < -0.2) | (m > 0.6)] = 0.0  # about 40 % positive, 13 % negative, the rest 0
    sel = m > 0.0
    if n > 200:
        assert 0.3 < sel.mean() < 0.5 and (m == 0.0).any() and (m < 0.0).any()
    ru, rv = u.copy(), v.copy()
    ru[sel] = u[sel] * (1.0 - m[sel] * fs)
    rv[sel] = v[sel] * (1.0 - m[sel] * fs)
    ud, vd = dev(u), dev(v)
    K.apply_ibm_fast(ud, vd, dev(m), fs)
    assert same(ud, ru) and same(vd, rv)


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_clip_f64_exact(n):
    lo, hi = -0.5, 0.25
    a = noise(n, np.float64, seed=18).copy()
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, lo, hi, np.nextafter(lo, -1), np.nextafter(hi, 1)]
    if n >= len(special):
        a[:len(special) - 1] = special[:-1]
        a[-1] = special[-1]
        arrays = [a]
    else:  # one cell: each special value in its own call
        arrays = [np.array([x]) for x in special]
    for a in arrays:
        ref = np.clip(a, lo, hi)
        t = dev(a)
        call("cfd_clip_f64", ptr(t), n, lo, hi, stream_handle())
        assert same(t, ref, equal_nan=True)
        assert np.array_equal(np.signbit(host(t)), np.signbit(ref))
