"""The passive scalar of the 3-D cylinder channel on the GPU against its NumPy
statement (tests/scalar3d_reference.py): the advance as plane march and as
per-cell kernel, the heating / face stage, whole steps of
CylinderChannel3DSolver(scalar=True) and the snapshot restart.

Bars.  Fields and dt: BIT-EXACT.  The heat sum: both sides add the same
float64 terms and only the order differs, so |device - NumPy| <= 2 (n - 1)
2^-53 sum|t| (force_bound's bar, heat_bound here).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cfd_simulations_amd import _lib
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import call, ptr, stream_handle
from cfd_simulations_amd.solver import (CylinderChannel3DConfig, CylinderChannel3DSolver, host_ibm_bbox,
                                        monitor_simulation_health3d)
from cyl3d_reference import force_bound
from ref3d import monitor_health3d_numpy
from scalar3d_reference import (ScalarCylinder3DReference, ScalarPeriodicCylinder3DReference, face_mask, heat_bound,
                                nusselt_numpy, scalar_advance3d_numpy, scalar_bc_heat3d_numpy)
from test_gpu_cyl3d import CUBE
from test_scalar3d_host import BC_SHAPES, heat_mask

pytestmark = pytest.mark.gpu

F = np.float32
H = 1 / 8
DT = F(1e-3)
ALPHA = F(0.004)
INV_PRT = F(1 / 0.85)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")  # a writable copy


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def last_path():
    n = ctypes.c_int(-9)
    return _lib.lib().cfd_get_last_scalar3d_path(ctypes.byref(n)), n.value


# ------------------------------------------------------------------ advance
@functools.lru_cache(maxsize=None)
def adv_case(shape):
    """u, v, w uniform in [-3, 3] with a few cells exactly 0 in one component
    (the upwind `> 0` branch) and a few with u = v = w = 0 (tau's dt / 2
    branch); T uniform in [0, 1]; nu_t uniform in [0, 1e-2]."""
    rng = np.random.default_rng(101 + sum(shape))
    u, v, w = (rng.uniform(-3, 3, shape).astype(F) for _ in range(3))
    T = rng.uniform(0, 1, shape).astype(F)
    nu_t = rng.uniform(0, 1e-2, shape).astype(F)
    u.flat[1::7] = 0
    v.flat[2::11] = 0
    w.flat[3::5] = 0
    for a in (u, v, w):
        a.flat[4::13] = 0
    nz, ny, nx = shape
    u[nz // 2, ny // 2, nx // 2] = v[nz // 2, ny // 2, nx // 2] = w[nz // 2, ny // 2, nx // 2] = 0  # an interior cell
    for a in (T, u, v, w, nu_t):
        a.setflags(write=False)
    return T, u, v, w, nu_t


@functools.lru_cache(maxsize=None)
def adv_ref(shape, nut, supg, periodic):
    T, u, v, w, nu_t = adv_case(shape)
    r = scalar_advance3d_numpy(T, u, v, w, ALPHA, nu_t if nut else None, INV_PRT, dx=H, dy=H, dz=H, dt=DT,
                               use_supg=supg, periodic_z=periodic)
    assert not np.array_equal(r, T)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def adv_dev(shape):
    return tuple(dev(a) for a in adv_case(shape))


def run_advance(shape, nut, supg, periodic, config):
    """(T_new, path, cells per lane) under cfd_set_scalar3d_config(*config)."""
    T, u, v, w, nu_t = adv_dev(shape)
    out = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    call("cfd_set_scalar3d_config", *config)
    try:
        K.scalar_advance3d(T, u, v, w, ALPHA, DT, H, H, H, supg, nu_t=nu_t if nut else None, inv_prt=INV_PRT,
                           out=out, periodic_z=periodic)
        path = last_path()
    finally:
        call("cfd_reset_tuning")
    return host(out), *path


MODES = [(nut, supg) for nut in (False, True) for supg in (True, False)]


@pytest.mark.parametrize("nut,supg", MODES)
def test_advance_per_cell_bitexact(nut, supg):
    for shape, periodic in (((3, 3, 3), False), ((5, 6, 7), False), ((4, 6, 7), True)):
        got, path, vec = run_advance(shape, nut, supg, periodic, (0, 0, 0, 0))
        assert (path, vec) == (0, 1), shape   # nx odd: one thread per cell
        assert np.array_equal(got, adv_ref(shape, nut, supg, periodic)), shape
    # the per-cell kernel forced on a shape the march would take
    got, path, _ = run_advance((6, 11, 260), nut, supg, False, (1, 0, 0, 0))
    assert path == 0 and np.array_equal(got, adv_ref((6, 11, 260), nut, supg, False))


@pytest.mark.parametrize("nut,supg", MODES)
def test_advance_march_chunk_seams_partial_tiles_bitexact(nut, supg):
    """(7, 11, 8) with 3 planes per chunk: seams 3 + 3 + 1, a partial row
    tile (11 rows in tiles of 4 or 8) and a segment narrower than a wave."""
    shape = (7, 11, 8)
    ref = adv_ref(shape, nut, supg, False)
    for rows in (1, 2):
        for vec in (1, 2, 4):
            got, path, v = run_advance(shape, nut, supg, False, (2, rows, vec, 3))
            assert (path, v) == (1, vec), (rows, vec)
            assert np.array_equal(got, ref), (rows, vec)


@pytest.mark.parametrize("nut,supg", MODES)
def test_advance_march_segment_boundaries_bitexact(nut, supg):
    """(6, 11, 260): two (4 cells per lane) and five (1) segments, the x-halo
    load crosses a segment boundary, the last segment has 4 columns."""
    shape = (6, 11, 260)
    for periodic in (False, True):
        ref = adv_ref(shape, nut, supg, periodic)
        for vec in (4, 1):
            got, path, v = run_advance(shape, nut, supg, periodic, (2, 0, vec, 0))
            assert (path, v) == (1, vec), (periodic, vec)
            assert np.array_equal(got, ref), (periodic, vec)
        got, path, v = run_advance(shape, nut, supg, periodic, (0, 0, 0, 0))   # auto: the march at 2
        assert (path, v) == (1, 2) and np.array_equal(got, ref), periodic


@pytest.mark.parametrize("nut,supg", MODES)
def test_advance_march_periodic_wrap_at_chunk_ends_bitexact(nut, supg):
    """(8, 9, 64) periodic with 3 planes per chunk: D of plane 0 is plane 7, U
    of plane 7 is plane 0, both at chunk ends."""
    shape = (8, 9, 64)
    ref = adv_ref(shape, nut, supg, True)
    assert not np.array_equal(ref[0, 1:-1, 1:-1], adv_case(shape)[0][0, 1:-1, 1:-1])
    for rows, vec in ((0, 0), (1, 1), (2, 4), (1, 2)):
        got, path, _ = run_advance(shape, nut, supg, True, (2, rows, vec, 3))
        assert path == 1 and np.array_equal(got, ref), (rows, vec)


def test_advance_refusals():
    L = _lib.lib()
    s = stream_handle()
    t = [torch.ones((4, 5, 6), dtype=torch.float32, device="cuda") for _ in range(6)]
    p = [ptr(x) for x in t]

    def adv(T=p[0], u=p[1], v=p[2], w=p[3], nut=p[4], out=p[5], dims=(4, 5, 6), zper=False):
        f = L.cfd_scalar_advance3d_zper_f32 if zper else L.cfd_scalar_advance3d_f32
        return f(T, u, v, w, 0.01, nut, 1.0, out, *dims, H, H, H, 1e-3, 1, s)

    for name, kw in (("T", dict(out=p[0])), ("u", dict(out=p[1])), ("v", dict(out=p[2])), ("w", dict(out=p[3])),
                     ("nu_t", dict(out=p[4]))):
        assert adv(**kw) == -1 and b"alias " + name.encode() in L.cfd_last_error(), name
    for name in ("T", "u", "v", "w"):
        assert adv(**{name: None}) == -1 and b"null pointer: " + name.encode() in L.cfd_last_error(), name
    assert adv(out=None) == -1 and b"null pointer: T_new" in L.cfd_last_error()
    assert adv(dims=(4, 5, 2)) == -1 and b"nx" in L.cfd_last_error()
    assert adv(dims=(2, 5, 6)) == -1 and adv(dims=(4, 2, 6)) == -1
    assert adv(dims=(3, 5, 6), zper=True) == -1 and b"nz" in L.cfd_last_error()   # odd
    assert adv(dims=(2, 5, 6), zper=True) == -1                                     # too small
    torch.cuda.synchronize()
    assert (host(t[5]) == 1).all()   # nothing was launched
    assert adv(nut=None) == 0 and adv(zper=True) == 0
    # the checked wrapper
    with pytest.raises(ValueError):
        K.scalar_advance3d(t[0], t[1], t[2], t[3][:, :, :5], 0.01, 1e-3, H, H, H, True, out=t[5])
    with pytest.raises(TypeError):
        K.scalar_advance3d(t[0].double(), t[1], t[2], t[3], 0.01, 1e-3, H, H, H, True, out=t[5])
    with pytest.raises(ValueError):
        K.scalar_advance3d(t[0], t[1], t[2], t[3], 0.01, 1e-3, H, H, H, True, nu_t=t[4][:3], out=t[5])
    torch.cuda.synchronize()


# ------------------------------------------------------------- heating / faces
T_IN, T_CYL = 0.25, 1.0


@functools.lru_cache(maxsize=None)
def bc_case(shape):
    rng = np.random.default_rng(sum(shape))
    T = rng.uniform(0, 1, shape).astype(F)
    m = heat_mask(shape)
    T.setflags(write=False)
    m.setflags(write=False)
    return T, m


@functools.lru_cache(maxsize=None)
def bc_ref(shape, fs, periodic=False, masked=True):
    T, m = bc_case(shape)
    out = T.copy()
    stats = scalar_bc_heat3d_numpy(out, m if masked else None, T_IN, T_CYL, fs, periodic)
    out.setflags(write=False)
    return out, stats


def run_bc(shape, fs, mask, periodic=False, bbox=None, heat=None, T=None):
    t = dev(bc_case(shape)[0] if T is None else T)
    K.apply_scalar_bc_heat3d(t, None if mask is None else dev(mask), T_IN, T_CYL, fs, bbox=bbox, heat_out=heat,
                             periodic_z=periodic)
    return host(t)


@pytest.mark.parametrize("shape,periodic", [(s, False) for s in BC_SHAPES] + [((4, 6, 7), True)])
def test_bc_heat_bitexact_and_heat_sum(shape, periodic):
    T, m = bc_case(shape)
    for fs in (0.0, 0.5, 1.0):
        ref, stats = bc_ref(shape, fs, periodic)
        heat = torch.full((1,), 3.0, dtype=torch.float64, device="cuda")   # a non-zero start value
        got = run_bc(shape, fs, m, periodic, heat=heat)
        assert np.array_equal(got, ref), fs
        q = host(heat)[0] - 3.0
        print(shape, periodic, fs, "heat", q, "ref", stats["heat"], "bound", heat_bound(stats))
        # the start value 3.0 is one more term of the device's sum (n + 1 terms of magnitude
        # abs + 3, each order within (terms - 1) 2^-53 of that), and taking it off again rounds once
        bound = 2.0 * (stats["n"] + 1) * 2.0 ** -53 * (stats["abs"] + 3.0)
        assert abs(q - stats["heat"]) <= bound
        if fs == 0.0:
            assert host(heat)[0] == 3.0   # exact zeros: the atomic is skipped
        else:
            assert stats["heat"] != 0.0
            zero = torch.zeros(1, dtype=torch.float64, device="cuda")
            run_bc(shape, fs, m, periodic, heat=zero)
            assert abs(host(zero)[0] - stats["heat"]) <= heat_bound(stats)
    # no mask: only the faces change
    ref, _ = bc_ref(shape, 1.0, periodic, False)
    got = run_bc(shape, 1.0, None, periodic)
    faces = face_mask(shape, periodic)
    assert np.array_equal(got, ref) and np.array_equal(got[~faces], T[~faces])


@pytest.mark.parametrize("shape", BC_SHAPES[1:])
def test_bc_heat_any_covering_box_gives_the_same_bits(shape):
    T, m = bc_case(shape)
    nz, ny, nx = shape
    inner = np.zeros_like(m)
    inner[2:ny - 2, 2:nx - 3] = m[2:ny - 2, 2:nx - 3]
    inner[2, 2] = inner[ny - 3, nx - 4] = 0.5
    tight = host_ibm_bbox(inner)
    assert tight == (2, ny - 2, 2, nx - 3)
    want = T.copy()
    stats = scalar_bc_heat3d_numpy(want, inner, T_IN, T_CYL, 0.5)
    for bbox in (tight, None, (0, ny, 0, nx), (1, ny - 1, 2, nx)):
        heat = torch.zeros(1, dtype=torch.float64, device="cuda")
        got = run_bc(shape, 0.5, inner, bbox=bbox, heat=heat)
        assert np.array_equal(got, want), bbox
        assert abs(host(heat)[0] - stats["heat"]) <= heat_bound(stats), bbox
    # the border mask: the tight box is the whole plane
    assert host_ibm_bbox(m) == (0, ny, 0, nx)
    assert np.array_equal(run_bc(shape, 0.5, m, bbox=host_ibm_bbox(m)), bc_ref(shape, 0.5)[0])


def test_bc_heat_refusals():
    L = _lib.lib()
    s = stream_handle()
    t = torch.ones((4, 5, 6), dtype=torch.float32, device="cuda")
    m = torch.ones((5, 6), dtype=torch.float64, device="cuda")

    def bc(T=ptr(t), mm=ptr(m), dims=(4, 5, 6), box=(0, 5, 0, 6), zper=False):
        f = L.cfd_scalar_bc_heat3d_zper_f32 if zper else L.cfd_scalar_bc_heat3d_f32
        return f(T, mm, *dims, 0.0, 1.0, 0.5, *box, None, s)

    assert bc(T=None) == -1 and b"null pointer: T" in L.cfd_last_error()
    for box in ((0, 6, 0, 6), (0, 5, 0, 7), (-1, 5, 0, 6), (3, 2, 0, 6), (2, 2, 0, 6)):
        assert bc(box=box) == -1 and b"box" in L.cfd_last_error(), box
    assert bc(dims=(4, 5, 2), box=(0, 5, 0, 2)) == -1 and b"nx" in L.cfd_last_error()
    assert bc(dims=(3, 5, 6), zper=True) == -1 and b"nz" in L.cfd_last_error()
    torch.cuda.synchronize()
    assert (host(t) == 1).all()   # nothing was launched
    with pytest.raises(ValueError):
        K.apply_scalar_bc_heat3d(t, m.float(), 0.0, 1.0, 0.5)
    with pytest.raises(ValueError):
        K.apply_scalar_bc_heat3d(t, m[:, :5], 0.0, 1.0, 0.5)
    with pytest.raises(ValueError):
        K.apply_scalar_bc_heat3d(t, m, 0.0, 1.0, 0.5, heat_out=torch.zeros(2, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ whole steps
SCALAR = dict(scalar=True, scalar_inlet=0.25, scalar_cylinder=1.5)
STEP_CASES = {
    "rbgs-unequal": dict(CUBE, y_max=3.0, z_max=1.0, cylinder_center=(1.5, 1.5), **SCALAR),
    "rbgs-upwind": dict(CUBE, y_max=3.0, use_supg=False, cylinder_center=(1.5, 1.5), **SCALAR),
    "rbgs-les": dict(CUBE, z_max=1.0, use_les=True, **SCALAR),
    "rbgs-from-1000": dict(CUBE, z_max=1.0, **SCALAR),
    "periodic": dict(CUBE, z_max=1.0, spanwise_bc="periodic", spanwise_perturbation=0.05, **SCALAR),
    # initial_steps = 7, started at step 3: the forcing and the heating run at 3/7, 4/7, 5/7
    "rbgs-ramp-from-3": dict(CUBE, y_max=3.0, z_max=1.0, cylinder_center=(1.5, 1.5), initial_steps=7, **SCALAR),
}


def reference(c):
    return (ScalarPeriodicCylinder3DReference if c.spanwise_bc == "periodic" else ScalarCylinder3DReference)(c)


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_cylinder3d_scalar_steps(case):
    c = CylinderChannel3DConfig(**STEP_CASES[case])
    g, o = CylinderChannel3DSolver(c), reference(c)
    plain = CylinderChannel3DSolver(CylinderChannel3DConfig(**dict(STEP_CASES[case], scalar=False)))
    assert not hasattr(plain, "T") and not hasattr(plain, "_heat")   # nothing is allocated
    assert np.array_equal(host(g.T), o.T) and (o.T == F(0.25)).all()
    if case.endswith("1000"):
        g.step = o.step = plain.step = 1000   # full forcing strength, adaptive dt
    if case.endswith("from-3"):
        g.step = o.step = plain.step = 3      # the ramp min(1, step / 7) at 3/7, 4/7, 5/7
        assert c.initial_steps == 7
    first = g.step
    for k in range(first, first + 3):
        assert g.time_step() == o.time_step() == plain.time_step(), k
        assert np.array_equal(host(g.T), o.T), k
        for f in ("u", "v", "w", "phi"):
            assert np.array_equal(host(getattr(g, f)), getattr(o, f)), (f, k)
            # passive: the scalar-off solver has the same bits
            assert np.array_equal(host(getattr(g, f)), host(getattr(plain, f))), (f, k)
    assert o.T.max() > F(0.25)   # the cylinder heats the flow
    hh = g.heat_history
    assert [r[0] for r in hh] == [r[0] for r in o.heat_history] == list(range(first, first + 3))
    for (s, q), (_, qr), stats in zip(hh, o.heat_history, o.heat_stats):
        print(case, "heat", s, q, "ref", qr, "bound", heat_bound(stats))
        assert abs(q - qr) <= heat_bound(stats), s
    if first == 0:
        assert hh[0][1] == 0.0 and hh[2][1] != 0.0   # force_strength 0, then the ramp
    else:
        assert all(q != 0.0 for _, q in hh)
    for (s, nu), (_, q), dt in zip(g.nusselt_numbers(), hh, o.dts):
        assert nu == pytest.approx(nusselt_numpy(c, q, dt), rel=1e-12), s
    # passive: energy (a fixed summation order) and forces (atomics: within bound)
    assert g.energy_history == plain.energy_history
    for row, prow, stats in zip(g.force_history, plain.force_history, o.force_stats):
        assert (np.abs(np.array(row[1:]) - np.array(prow[1:])) <= force_bound(stats)).all(), row[0]
    # the health monitor: the reference's verdict on u, v, w, and T has to be finite too
    healthy = monitor_health3d_numpy(o.u, o.v, o.w, c, 1)
    assert monitor_simulation_health3d(g, 1) is monitor_simulation_health3d(plain, 1) is healthy
    assert healthy or first == 1000   # the cases from step 0 are healthy: the NaN below is what fails them
    g.T[3, 4, 5] = float("nan")
    assert monitor_simulation_health3d(g, 1) is False
    assert monitor_simulation_health3d(plain, 1) is healthy


def test_scalar_config_rejects_bad_prandtl_numbers():
    for kw in (dict(prandtl=0.0), dict(prandtl=-1.0), dict(turbulent_prandtl=0.0)):
        with pytest.raises(ValueError, match="prandtl"):
            CylinderChannel3DConfig(**dict(CUBE, **kw))
    c = CylinderChannel3DConfig(**CUBE)
    assert (c.scalar, c.prandtl, c.turbulent_prandtl, c.scalar_inlet, c.scalar_cylinder) == (False, 0.71, 0.85, 0.0,
                                                                                             1.0)


@pytest.mark.parametrize("case", ["rbgs-les", "periodic"])
def test_cylinder3d_scalar_restart(case, tmp_path):
    c = CylinderChannel3DConfig(**STEP_CASES[case])
    whole, o = CylinderChannel3DSolver(c), reference(c)
    path = tmp_path / "snap.npz"
    for k in range(4):
        whole.time_step()
        o.time_step()
        if k == 1:
            whole.save_snapshot(path, 2, 0.0)
    fresh = CylinderChannel3DSolver(c)
    fresh.load_snapshot(path)
    assert fresh.step == 2 and fresh.heat_history == []
    fresh.time_step()
    fresh.time_step()
    for f in ("T", "u", "v", "w"):
        assert np.array_equal(host(getattr(fresh, f)), host(getattr(whole, f))), f
    assert np.array_equal(host(fresh.T), o.T)
    hh = fresh.heat_history
    assert [s for s, _ in hh] == [2, 3]
    for (s, q), (_, qr), stats in zip(hh, o.heat_history[2:], o.heat_stats[2:]):
        assert abs(q - qr) <= heat_bound(stats) and q != 0.0, s
    # a group written with the scalar off leaves T alone
    off = CylinderChannel3DSolver(CylinderChannel3DConfig(**dict(STEP_CASES[case], scalar=False)))
    off.time_step()
    off_path = tmp_path / "off.npz"
    off.save_snapshot(off_path, 1, 0.0)
    with np.load(off_path) as f:
        assert "step_000001/T" not in f.files
    with np.load(path) as f:
        assert "step_000002/T" in f.files
    before = host(fresh.T).copy()
    fresh.load_snapshot(off_path)
    assert fresh.step == 1 and np.array_equal(host(fresh.T), before)
    assert np.array_equal(host(fresh.u), host(off.u))
