"""The one-thread-per-cell 3-D field kernels of csrc/fields3d.hip on their own
(k_divergence3d, k_project3d, k_smagorinsky3d, k_vorticity3d, k_lid_bc3d,
k_channel_bc_ibm3d and their spanwise-periodic forms), swept over
SHAPES_3D of tests/fields3d_reference.py: one interior cell, nx on both sides
of a wave and of a 256-column workgroup, shapes whose largest face is nz*nx or
nz*ny, ny and nz at the launch grid's limit 65535; dx != dy != dz.

Every field comparison is BIT FOR BIT against the existing NumPy statements
(tests/ref3d.py, cyl3d_reference.py, zper_reference.py, les3d_reference.py,
pinned on the CPU by tests/test_fields3d_host.py), the fused maxima against
the fold over the reference's field; the IBM force sums within force_bound.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from cfd_simulations_amd import _lib
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import call, ptr, stream_handle
from cyl3d_reference import channel_bc_ibm3d_numpy, force_bound, vorticity3d_numpy
from diag_reference import fold_absmax
from fields3d_reference import CS, DT, DX, DY, DZ, LID_EXTRA, SHAPES_3D, SP, fields3d, grad_mag3d, ref_field
from les3d_reference import smagorinsky3d_numpy
from ref3d import lid_bc3d_numpy, project3d_numpy
from zper_reference import channel_bc_ibm3d_zper_numpy, project3d_zper_numpy, vorticity3d_zper_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
D3 = (DX, DY, DZ)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the shared inputs are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(x):
    return np.asarray(x).tobytes()


def same(got, want):
    """Bit for bit (NaNs too: a kernel's and NumPy's default NaN are one pattern
    only by convention, so NaNs are compared as a mask and the rest as bytes)."""
    got = host(got) if isinstance(got, torch.Tensor) else got
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and bits(np.where(gn, 0, got)) == bits(np.where(wn, 0, want))


def scalar(value=0.0):
    return torch.full((1,), value, dtype=torch.float32, device=DEV)


def vorticity_ref(u, v, w, periodic, mask=None):
    return (vorticity3d_zper_numpy if periodic else vorticity3d_numpy)(u, v, w, DX, DY, DZ, mask)


# ------------------------------------------- the four field kernels, all shapes
@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", SHAPES_3D)
def test_divergence_projection_vorticity_at_every_shape(shape, periodic):
    u, v, w, phi = fields3d(shape)
    ud, vd, wd, pd = dev(u), dev(v), dev(w), dev(phi)
    # divergence
    ref = ref_field("div", (u, v, w), periodic)
    out = scalar()
    d = K.compute_divergence3d(ud, vd, wd, *D3, out=torch.full_like(ud, 7.0), absmax=out, periodic_z=periodic)
    assert same(d, ref)
    assert bits(host(out)[0]) == bits(fold_absmax(ref)) and (host(out)[0] > 0) == bool(ref.any())
    assert same(K.compute_divergence3d(ud, vd, wd, *D3, periodic_z=periodic), ref)  # absmax = NULL
    # projection
    ru, rv, rw, gmax = (project3d_zper_numpy if periodic else project3d_numpy)(phi, u, v, w, dt=DT, **SP)
    assert bits(gmax) == bits(fold_absmax(grad_mag3d(phi, periodic))) and gmax > 0
    out = scalar()
    got = K.project_velocity3d(pd, ud, vd, wd, *D3, DT, gradmax=out, periodic_z=periodic)
    assert all(same(g, r) for g, r in zip(got, (ru, rv, rw))) and bits(host(out)[0]) == bits(gmax)
    got = K.project_velocity3d(pd, ud, vd, wd, *D3, DT, periodic_z=periodic)  # gradmax = NULL
    assert all(same(g, r) for g, r in zip(got, (ru, rv, rw)))
    # vorticity, with and without the components
    ref = vorticity_ref(u, v, w, periodic)
    out = scalar()
    got = K.compute_vorticity3d(ud, vd, wd, *D3, components=True, absmax=out, periodic_z=periodic)
    assert all(same(g, r) for g, r in zip(got, ref)) and bits(host(out)[0]) == bits(fold_absmax(ref[3]))
    out = scalar()
    assert same(K.compute_vorticity3d(ud, vd, wd, *D3, absmax=out, periodic_z=periodic), ref[3])
    assert bits(host(out)[0]) == bits(fold_absmax(ref[3])) and host(out)[0] > 0
    # the inputs were read only
    assert same(ud, u) and same(vd, v) and same(wd, w) and same(pd, phi)


@pytest.mark.parametrize("shape", SHAPES_3D)
def test_smagorinsky_at_every_shape(shape):
    u, v, w, _ = fields3d(shape)
    ref = smagorinsky3d_numpy(u, v, w, DX, DY, DZ, CS)
    got = K.compute_smagorinsky_viscosity3d(dev(u), dev(v), dev(w), *D3, CS, out=torch.full(shape, 7.0, device=DEV))
    # (3, 3, 3): the zero block holds the one interior cell and its E, N, U neighbours, so nu_t = 0 there
    assert same(got, ref) and (ref[1:-1, 1:-1, 1:-1].any() or shape == (3, 3, 3))


# ------------------------------------------------------------------ refusals
def test_bad_shapes_are_refused_before_any_launch():
    """A dimension of 2, ny = 65536 and nz = 65536 (one past the launch grid's
    limit): -1 from the C ABI, nothing launched, every output as it was.  The
    check precedes the launch, so small buffers do."""
    L = _lib.lib()
    s = stream_handle()
    t = [torch.full((3, 3, 3), 1.0 + q, dtype=torch.float32, device=DEV) for q in range(8)]
    red = scalar(0.25)
    mask = torch.zeros((3, 3, 3), dtype=torch.uint8, device=DEV)
    p = [ptr(x) for x in t]
    r = ptr(red)
    bad = [(2, 3, 3), (3, 2, 3), (3, 3, 2), (3, 65536, 3), (65536, 3, 3), (65536, 65536, 3)]
    for dims in bad:
        for sfx in ("", "_zper"):
            assert getattr(L, "cfd_divergence3d" + sfx + "_f32")(p[0], p[1], p[2], p[3], *dims, *D3, r, s) == -1, dims
            assert b"shape" in L.cfd_last_error()
            assert getattr(L, "cfd_project3d" + sfx + "_f32")(p[0], p[1], p[2], p[3], p[4], p[5], p[6], *dims, *D3,
                                                              DT, r, s) == -1, dims
            assert getattr(L, "cfd_vorticity3d" + sfx + "_f32")(p[0], p[1], p[2], ptr(mask), p[3], p[4], p[5], p[6],
                                                                r, *dims, *D3, s) == -1, dims
        assert L.cfd_smagorinsky3d_f32(p[0], p[1], p[2], p[3], *dims, *D3, CS, s) == -1, dims
        assert L.cfd_apply_lid_bc3d_f32(p[0], p[1], p[2], *dims, 1.0, s) == -1, dims
        assert b"shape" in L.cfd_last_error()
    torch.cuda.synchronize()
    for q, x in enumerate(t):
        assert (host(x) == 1.0 + q).all()
    assert host(red)[0] == 0.25
    # the limit itself and nx past it are admitted (launched at SHAPES_3D's 65535 shapes; here: nx)
    wide = [torch.zeros((3, 3, 65537), dtype=torch.float32, device=DEV) for _ in range(4)]
    assert L.cfd_divergence3d_f32(*(ptr(x) for x in wide), 3, 3, 65537, *D3, None, s) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------- lid walls
def pattern(shape):
    """Three fields whose every cell is distinct and nonzero."""
    n = shape[0] * shape[1] * shape[2]
    assert 3 * n + 1 < 2 ** 24  # exact in float32
    return [(np.arange(n, dtype=F) + F(1 + q * n)).reshape(shape) for q in range(3)]


@pytest.mark.parametrize("shape", SHAPES_3D + LID_EXTRA)
def test_lid_bc_faces_and_interior_at_every_shape(shape):
    f = pattern(shape)
    inner = (slice(1, -1),) * 3
    for u_lid in (1.25, -0.75, 0.0):
        want = [a.copy() for a in f]
        lid_bc3d_numpy(*want, u_lid)
        got = [host(t) for t in K.apply_lid_bc3d(*(dev(a) for a in f), u_lid)]
        for name, g, r, a in zip("uvw", got, want, f):
            assert same(g, r), (name, u_lid)
            assert bits(g[inner]) == bits(a[inner]) and g[inner].all(), (name, u_lid)  # the interior's bits survive
        assert (got[0][:, -1, :] == F(u_lid)).all() and not got[0][:, :-1, 0].any() and not got[0][0, :-1].any()
        assert not np.signbit(got[0][:, :-1, -1]).any()


# ----------------------------------------------- vorticity: outputs and masks
VORT_SHAPES = [(3, 3, 3), (4, 5, 257), (7, 37, 260)]


def vort_call(ins, mask, want, periodic, preset=0.0):
    """cfd_vorticity3d_f32 with the outputs named in ``want`` (of ox, oy, oz,
    mag, absmax) and the others NULL: {name: host array}."""
    nz, ny, nx = ins[0].shape
    outs = {n: (scalar(preset) if n == "absmax" else torch.full_like(ins[0], 7.0)) if n in want else None
            for n in ("ox", "oy", "oz", "mag", "absmax")}
    call("cfd_vorticity3d_zper_f32" if periodic else "cfd_vorticity3d_f32", *(ptr(x) for x in ins), ptr(mask),
         *(ptr(outs[n]) for n in ("ox", "oy", "oz", "mag", "absmax")), nz, ny, nx, *D3, stream_handle())
    return {n: host(t) for n, t in outs.items() if t is not None}


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", VORT_SHAPES)
def test_vorticity_null_output_combinations(shape, periodic):
    """Every combination of outputs the entry point accepts: each single one,
    absmax alone, all, and every other subset; none at all is refused."""
    u, v, w, _ = fields3d(shape)
    ins = [dev(u), dev(v), dev(w)]
    rng = np.random.default_rng(sum(shape))
    mask = rng.uniform(size=shape) < 0.25
    mask[0, 0, 0] = mask[-1, -1, -1] = True
    names = ("ox", "oy", "oz", "mag", "absmax")
    for mk in (None, mask):
        ref = dict(zip(names, vorticity_ref(u, v, w, periodic, mk)))
        top = fold_absmax(ref["mag"])
        md = None if mk is None else dev(mk.astype(np.uint8))
        for r in range(1, 6):
            for want in itertools.combinations(names, r):
                got = vort_call(ins, md, want, periodic)
                assert set(got) == set(want)
                for n, g in got.items():
                    if n == "absmax":
                        assert bits(g[0]) == bits(top), (want, mk is None)
                    else:
                        assert same(g, ref[n]), (n, want, mk is None)
    L = _lib.lib()
    none = L.cfd_vorticity3d_f32(*(ptr(x) for x in ins), None, None, None, None, None, None, *shape, *D3,
                                 stream_handle())
    assert none == -1 and b"no output" in L.cfd_last_error()


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", VORT_SHAPES[1:])
def test_vorticity_masks(shape, periodic):
    nz, ny, nx = shape
    u, v, w, _ = fields3d(shape)
    ins = [dev(u), dev(v), dev(w)]
    names = ("ox", "oy", "oz", "mag", "absmax")
    free = vorticity_ref(u, v, w, periodic)[3]
    top = fold_absmax(free)

    def check(mask, preset=0.0):
        ref = vorticity_ref(u, v, w, periodic, mask)
        got = vort_call(ins, dev(mask.astype(np.uint8)), names, periodic, preset)
        for n, r in zip(names, ref):
            assert same(got[n], r), n
            assert np.isnan(got[n][mask]).all() and not np.isnan(got[n][~mask]).any(), n
        want = fold_absmax(ref[3], start=preset)
        assert bits(got["absmax"][0]) == bits(want)
        return want

    # the six faces masked, the interior free: the maximum is unchanged (free-slip: the faces are 0 anyway)
    faces = np.ones(shape, bool)
    faces[1:-1, 1:-1, 1:-1] = False
    m = check(faces)
    assert (m == top) if not periodic else (0 < m <= top)
    # the mask covers the cell that holds the maximum: the runner-up is returned
    at = np.unravel_index(np.argmax(free), shape)
    mask = np.zeros(shape, bool)
    mask[at] = True
    second = np.sort(free.ravel())[-2]
    assert 0 < second < top and check(mask) == second
    # everything masked: a zeroed absmax stays +0.0 and every output is NaN; a preset stands
    full = np.ones(shape, bool)
    assert bits(check(full)) == bits(F(0.0))
    assert check(full, preset=0.25) == F(0.25)
    # a NaN input: the cells it enters are NaN and never win
    u2 = np.array(u)
    u2[1, 0, nx // 2] = np.nan       # enters oz(1, 1, nx // 2)
    u2[nz - 2, ny - 2, 0] = np.nan   # a wall column cell: enters oz(nz - 2, ny - 3 | ny - 1, 0): faces, so nothing
    ref = vorticity_ref(u2, v, w, periodic)
    assert np.isnan(ref[3][1, 1, nx // 2]) and np.isnan(ref[2][1, 1, nx // 2]) and not np.isnan(ref[0]).any()
    got = vort_call([dev(u2), ins[1], ins[2]], None, names, periodic)
    assert all(same(got[n], r) for n, r in zip(names, ref))
    assert bits(got["absmax"][0]) == bits(fold_absmax(ref[3])) and got["absmax"][0] == np.nanmax(ref[3]) > 0


# --------------------------------------------------------- channel BC + IBM
Y_MAX, V_INF = 3.0, 1.5
BC_SHAPES = [((4, 3, 3), False), ((4, 5, 6), False), ((5, 3, 300), False), ((6, 4, 258), False), ((3, 6, 5), False),
             ((3, 5, 6), True), ((4, 5, 6), True), ((6, 4, 258), True)]  # cfd_apply_channel_bc_ibm3d_zper_f32 admits nz = 3


@functools.lru_cache(maxsize=None)
def bc_case(shape):
    """tests/test_gpu_cyl3d.py's case: random fields, row coordinates and a
    float64 mask positive on about a third of the plane, with cells of rows 0
    and ny-1 and of columns 0, nx-2 and nx-1 among them."""
    rng = np.random.default_rng([7, *shape])
    nz, ny, nx = shape
    u, v, w = (rng.uniform(-3, 3, shape).astype(F) for _ in range(3))
    m = np.where(rng.uniform(size=(ny, nx)) < 0.33, rng.uniform(0.05, 1, (ny, nx)), 0.0)
    m[0, 0], m[0, nx // 2], m[ny - 1, nx - 1], m[ny - 1, 1] = 0.5, 0.25, 0.75, 1.0
    m[1, 0], m[1, nx - 2], m[1, nx - 1], m[ny - 2, nx - 2] = 0.125, 0.3, 0.6, 0.9
    m[0, nx - 1], m[ny - 1, 0] = 0.4, 0.35  # the other two plane corners
    y = np.linspace(-1.0, Y_MAX, ny)
    for a in (u, v, w, m, y):
        a.setflags(write=False)
    return u, v, w, y, m


def boxes(ny, nx):
    """name -> (i0, i1, j0, j1): the whole plane, one cell at each plane
    corner, column nx-1 alone, column nx-2 alone, rows 0 and ny-1 alone."""
    return {"plane": (0, ny, 0, nx), "corner00": (0, 1, 0, 1), "corner0E": (0, 1, nx - 1, nx),
            "cornerN0": (ny - 1, ny, 0, 1), "cornerNE": (ny - 1, ny, nx - 1, nx), "last column": (0, ny, nx - 1, nx),
            "column nx-2": (0, ny, nx - 2, nx - 1), "row 0": (0, 1, 0, nx), "row ny-1": (ny - 1, ny, 0, nx)}


def boxed(m, box):
    """The mask as the kernel reads it: 0 outside the box."""
    i0, i1, j0, j1 = box
    out = np.zeros_like(m)
    out[i0:i1, j0:j1] = m[i0:i1, j0:j1]
    return out


@pytest.mark.parametrize("shape,periodic", BC_SHAPES)
def test_channel_bc_ibm_planes_columns_and_boxes(shape, periodic):
    """nz = 3 and 4 (no planes between 1 and nz-2), nx = 3 (columns 0 and nx-2
    adjacent, the clipped box empty), boxes that touch single corners, column
    nx-1 alone (which only the owner in column nx-2 writes), column nx-2, the
    wall rows; the full mask is handed over and the box decides what is read."""
    u, v, w, y, m = bc_case(shape)
    nz, ny, nx = shape
    numpy_bc = channel_bc_ibm3d_zper_numpy if periodic else channel_bc_ibm3d_numpy
    yd, md = dev(y), dev(m)

    def run(step, fs, mask, box):
        t = [dev(a) for a in (u, v, w)]
        force = torch.zeros(3, dtype=torch.float64, device=DEV)
        K.apply_channel_bc_ibm3d(*t, yd, mask, Y_MAX, V_INF, step, fs, bbox=box, force_out=force, periodic_z=periodic)
        return [host(a) for a in t], host(force)

    for step in (0, 7, 1500):
        for fs in (0.0, 0.5, 1.0):
            for name, box in boxes(ny, nx).items():
                seen = boxed(m, box)
                assert (seen > 0).any(), name
                want = [a.copy() for a in (u, v, w)]
                stats = numpy_bc(*want, y, seen, Y_MAX, V_INF, step, fs)
                got, force = run(step, fs, md, box)
                for q, g, r in zip("uvw", got, want):
                    assert same(g, r), (q, step, fs, name)
                assert stats["n"] == nz * int((seen > 0).sum())
                assert (np.abs(force - stats["force"]) <= force_bound(stats)).all(), (step, fs, name, force, stats)
                if fs == 0.0:
                    assert not force.any()
        want = [a.copy() for a in (u, v, w)]
        numpy_bc(*want, y, None, Y_MAX, V_INF, step, 1.0)
        got, force = run(step, 1.0, None, None)  # no IBM
        assert all(same(g, r) for g, r in zip(got, want)) and not force.any()
        # the forced cells are there: the IBM changes the fields
        assert not same(run(step, 0.5, md, None)[0][0], want[0])
