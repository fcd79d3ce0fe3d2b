"""tests/fields3d_reference.py on the CPU (no GPU needed): the NumPy statements
the 3-D field kernels are compared with are pinned to literal triple loops and,
in their periodic forms, to np.roll along z; the exact energy mean to a
fractions.Fraction sum; and the condition the GPU position tests rest on -- the
planted cell is the reference field's only, clear, finite maximum -- is shown
for every (kind, shape, cell) those tests use, so that a helper that planted
nothing could not make them vacuous."""
import fractions

import numpy as np
import pytest

from cyl3d_reference import vorticity3d_numpy
from diag_reference import fold_absmax
from fields3d_reference import (AT_GRID_LIMIT, DT, DX, DY, DZ, ENERGY3_BLOCK_CELLS, ENERGY3_CLIP, ENERGY3_FULL,
                                ENERGY3_MAX_BLOCKS, ENERGY3_ROUND, ENERGY3_SIZES, FACE_DOMINANT, FACTOR, GRID_LIMIT,
                                KINDS, LID_EXTRA, PLANT, POSITION_SHAPES, SHAPES_3D, SP, base_inputs, energy3_case,
                                energy_mean3_exact, fields3d, grad_mag3d, only_argmax, plant_argmax, plant_site,
                                positions3d, ref_field)
from ref3d import divergence3d_numpy, gradient3d_numpy, lid_bc3d_numpy, project3d_numpy
from zper_reference import divergence3d_zper_numpy, project3d_zper_numpy, vorticity3d_zper_numpy

F = np.float32
LOOP_SHAPES = [(3, 3, 3), (4, 5, 6), (5, 3, 7)]


def test_shapes_and_sizes_cover_the_kernel_paths():
    assert all(min(s) >= 3 for s in SHAPES_3D) and len(set(SHAPES_3D)) == len(SHAPES_3D) == 15
    assert {s[2] for s in SHAPES_3D} >= {3, 64, 65, 255, 256, 257, 513, 1030, 260}
    # each of k_lid_bc3d's three faces is somewhere the strictly largest but for (3, 300, 3)'s tie
    faces = {s: (s[1] * s[2], s[0] * s[2], s[0] * s[1]) for s in FACE_DOMINANT}
    assert faces[(40, 3, 5)] == (15, 200, 120) and faces[(40, 5, 3)] == (15, 120, 200)
    assert faces[(300, 3, 4)] == (12, 1200, 900) and faces[(3, 300, 3)] == (900, 9, 900)
    # each face alone exceeds the other two rounded up to 256-thread workgroups at some lid shape
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    lid = [(s[1] * s[2], s[0] * s[2], s[0] * s[1]) for s in SHAPES_3D + LID_EXTRA]
    for q in range(3):
        assert any(f[q] > up(max(f[p] for p in range(3) if p != q)) for f in lid), q
    assert AT_GRID_LIMIT == [(3, 65535, 3), (65535, 3, 3)] and GRID_LIMIT == 65535
    assert set(POSITION_SHAPES) <= set(SHAPES_3D)
    # the launcher's constants: ceil(n / 4096) blocks, at most 512; rounds of 4 x 256 cells
    assert (ENERGY3_BLOCK_CELLS, ENERGY3_MAX_BLOCKS, ENERGY3_ROUND, ENERGY3_FULL) == (4096, 512, 1024, 512 * 4096)
    assert ENERGY3_SIZES == [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 8193, 512 * 4096,
                             512 * 4096 + 1, 2 * 512 * 4096 + 77]
    for shape in SHAPES_3D:
        u, v, w, phi = fields3d(shape)
        assert all(a.dtype == F and a.shape == shape and not a.flags.writeable for a in (u, v, w, phi))
        assert np.abs(np.stack([u, v, w, phi])).max() < 1.5
        zero = (u == 0) & (v == 0) & (w == 0)
        assert zero.any() and (min(shape) == 3 or not zero.all())
    assert DX != DY != DZ != DX


def loops(u, v, w, phi, periodic):
    """Every operator as a literal loop over the cells, float32 scalars."""
    nz, ny, nx = u.shape
    cx, cy, cz = F(0.5 / DX), F(0.5 / DY), F(0.5 / DZ)
    dx2, dy2, dz2 = F(2.0 * DX), F(2.0 * DY), F(2.0 * DZ)
    dt = F(DT)
    o = {n: np.zeros(u.shape, F) for n in ("div", "gx", "gy", "gz", "ox", "oy", "oz", "mag", "g")}
    o["pu"], o["pv"], o["pw"] = u.copy(), v.copy(), w.copy()
    for k in range(nz):
        if not periodic and k in (0, nz - 1):
            continue
        ku, kd = (k + 1) % nz, (k - 1) % nz
        for j in range(1, ny - 1):
            for i in range(1, nx - 1):
                c = (k, j, i)
                o["div"][c] = (((u[k, j, i + 1] - u[k, j, i - 1]) * cx + (v[k, j + 1, i] - v[k, j - 1, i]) * cy)
                               + (w[ku, j, i] - w[kd, j, i]) * cz)
                gx = (phi[k, j, i + 1] - phi[k, j, i - 1]) * cx
                gy = (phi[k, j + 1, i] - phi[k, j - 1, i]) * cy
                gz = (phi[ku, j, i] - phi[kd, j, i]) * cz
                o["gx"][c], o["gy"][c], o["gz"][c] = gx, gy, gz
                o["g"][c] = np.sqrt((gx * gx + gy * gy) + gz * gz)
                o["pu"][c] = u[c] - dt * gx
                o["pv"][c] = v[c] - dt * gy
                o["pw"][c] = w[c] - dt * gz
                x = (w[k, j + 1, i] - w[k, j - 1, i]) / dy2 - (v[ku, j, i] - v[kd, j, i]) / dz2
                y = (u[ku, j, i] - u[kd, j, i]) / dz2 - (w[k, j, i + 1] - w[k, j, i - 1]) / dx2
                z = (v[k, j, i + 1] - v[k, j, i - 1]) / dx2 - (u[k, j + 1, i] - u[k, j - 1, i]) / dy2
                o["ox"][c], o["oy"][c], o["oz"][c] = x, y, z
                o["mag"][c] = np.sqrt((x * x + y * y) + z * z)
    assert all(a.dtype == F for a in o.values())
    return o


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_numpy_statements_equal_triple_loops(shape, periodic):
    rng = np.random.default_rng(sum(shape))
    u, v, w, phi = (rng.uniform(-1.5, 1.5, shape).astype(F) for _ in range(4))
    o = loops(u, v, w, phi, periodic)
    div = (divergence3d_zper_numpy if periodic else divergence3d_numpy)(u, v, w, **SP)
    assert np.array_equal(div, o["div"]) and np.array_equal(ref_field("div", (u, v, w), periodic), div)
    pu, pv, pw, gmax = (project3d_zper_numpy if periodic else project3d_numpy)(phi, u, v, w, dt=DT, **SP)
    for got, want in ((pu, "pu"), (pv, "pv"), (pw, "pw")):
        assert np.array_equal(got, o[want]), want
    g = grad_mag3d(phi, periodic)
    assert np.array_equal(g, o["g"]) and np.array_equal(ref_field("grad", (phi,), periodic), g)
    assert gmax.dtype == F and gmax == fold_absmax(g) == o["g"].max() > 0
    vort = (vorticity3d_zper_numpy if periodic else vorticity3d_numpy)(u, v, w, DX, DY, DZ)
    for got, want in zip(vort, ("ox", "oy", "oz", "mag")):
        assert got.dtype == F and np.array_equal(got, o[want]), want
    assert np.array_equal(ref_field("vort", (u, v, w), periodic), o["mag"])
    if not periodic:
        gx, gy, gz = gradient3d_numpy(phi, **SP)
        assert np.array_equal(gx, o["gx"]) and np.array_equal(gy, o["gy"]) and np.array_equal(gz, o["gz"])
    # a mask: NaN exactly there, face cells included
    mask = rng.uniform(size=shape) < 0.3
    mask[0, 0, 0] = mask[1, 1, 1] = True
    masked = (vorticity3d_zper_numpy if periodic else vorticity3d_numpy)(u, v, w, DX, DY, DZ, mask)
    for got, want in zip(masked, ("ox", "oy", "oz", "mag")):
        assert np.isnan(got[mask]).all() and np.array_equal(got[~mask], o[want][~mask]), want


@pytest.mark.parametrize("shape", LOOP_SHAPES)
def test_periodic_statements_equal_roll(shape):
    """The pad rule against np.roll along z: the U neighbour of plane nz - 1
    is plane 0, the D neighbour of plane 0 is plane nz - 1."""
    rng = np.random.default_rng(7 + sum(shape))
    u, v, w, phi = (rng.uniform(-1.5, 1.5, shape).astype(F) for _ in range(4))
    cx, cy, cz = F(0.5 / DX), F(0.5 / DY), F(0.5 / DZ)
    dx2, dy2, dz2 = F(2.0 * DX), F(2.0 * DY), F(2.0 * DZ)
    I = (slice(None), slice(1, -1), slice(1, -1))
    E, W = (slice(None), slice(1, -1), slice(2, None)), (slice(None), slice(1, -1), slice(None, -2))
    N, S = (slice(None), slice(2, None), slice(1, -1)), (slice(None), slice(None, -2), slice(1, -1))

    def ud(f):  # f(U) - f(D) on the x / y interior of every plane
        return (np.roll(f, -1, axis=0) - np.roll(f, 1, axis=0))[I]

    div = np.zeros(shape, F)
    div[I] = ((u[E] - u[W]) * cx + (v[N] - v[S]) * cy) + ud(w) * cz
    assert np.array_equal(divergence3d_zper_numpy(u, v, w, **SP), div)
    gx, gy, gz = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, F)
    gx[I], gy[I], gz[I] = (phi[E] - phi[W]) * cx, (phi[N] - phi[S]) * cy, ud(phi) * cz
    pu, pv, pw, gmax = project3d_zper_numpy(phi, u, v, w, dt=DT, **SP)
    for got, s, g in ((pu, u, gx), (pv, v, gy), (pw, w, gz)):
        want = s.copy()
        want[I] = s[I] - F(DT) * g[I]
        assert np.array_equal(got, want)
    assert gmax == np.sqrt((gx * gx + gy * gy) + gz * gz).max()
    ox, oy, oz = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, F)
    ox[I] = (w[N] - w[S]) / dy2 - ud(v) / dz2
    oy[I] = ud(u) / dz2 - (w[E] - w[W]) / dx2
    oz[I] = (v[E] - v[W]) / dx2 - (u[N] - u[S]) / dy2
    got = vorticity3d_zper_numpy(u, v, w, DX, DY, DZ)
    assert all(np.array_equal(a, b) for a, b in zip(got, (ox, oy, oz, np.sqrt((ox * ox + oy * oy) + oz * oz))))
    # the wrap matters: planes 0 and nz - 1 are not the free-slip statement's zeros
    assert div[0, 1:-1, 1:-1].all() and div[-1, 1:-1, 1:-1].all()
    assert not divergence3d_numpy(u, v, w, **SP)[0].any()


@pytest.mark.parametrize("shape", LOOP_SHAPES + [(40, 3, 5)])
def test_lid_bc_equals_a_triple_loop(shape):
    nz, ny, nx = shape
    n = nz * ny * nx
    for u_lid in (1.25, -0.75, 0.0):
        f = [(np.arange(n, dtype=F) + F(1 + q * n)).reshape(shape) for q in range(3)]
        want = [a.copy() for a in f]
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    if j == ny - 1:
                        want[0][k, j, i], want[1][k, j, i], want[2][k, j, i] = F(u_lid), 0, 0
                    elif k in (0, nz - 1) or j == 0 or i in (0, nx - 1):
                        want[0][k, j, i] = want[1][k, j, i] = want[2][k, j, i] = 0
        lid_bc3d_numpy(*f, u_lid)
        for a, b in zip(f, want):
            assert a.dtype == F and np.array_equal(a, b)
        assert np.array_equal(f[0][1:-1, 1:-1, 1:-1], want[0][1:-1, 1:-1, 1:-1]) and f[0][1:-1, 1:-1, 1:-1].all()


def test_energy_mean3_exact_equals_a_fraction_sum():
    for n in (1, 2, 7, 65, 257):
        u, v, w, exact = energy3_case(n)
        s = fractions.Fraction(0)
        for a, b, c in zip(u, v, w):
            e = F(0.5) * ((a * a + b * b) + c * c)
            assert type(e) is F
            s += fractions.Fraction(float(e))
        assert exact == energy_mean3_exact(u, v, w) == float(s) / n > 0
    # the cell energy is rounded in float32, in the stated order, before it is widened
    x = np.array([1.0 + 2.0 ** -12], F)
    y = np.array([2.0 ** -13], F)
    e32 = F(0.5) * ((x * x + y * y) + x * x)
    assert energy_mean3_exact(x, y, x) == float(e32[0]) != 0.5 * (2 * float(x[0]) ** 2 + float(y[0]) ** 2)
    # cases a float64 running sum loses
    big = np.array([2.0 ** 40, 2.0 ** -40, 2.0 ** 40], F)
    z = np.zeros(3, F)
    assert energy_mean3_exact(big, z, z) == (2.0 ** 80 + 2.0 ** -81) / 3
    assert np.isnan(energy_mean3_exact(np.array([np.nan], F), z[:1], z[:1]))
    assert energy_mean3_exact(np.array([np.inf], F), z[:1], z[:1]) == np.inf


@pytest.mark.parametrize("n", [s for s in ENERGY3_SIZES if s <= ENERGY3_FULL + 1])
def test_summation_bound_holds_for_numpy(n):
    """NumPy's pairwise float64 sum of the GPU test's own inputs is within the
    (n + 2) 2^-53 bound the kernel is held to; the clips are active."""
    u, v, w, want = energy3_case(n)
    e = F(0.5) * ((u * u + v * v) + w * w)
    assert want > 0 and abs(np.sum(e, dtype=np.float64) / n - want) <= (n + 2) * 2.0 ** -53 * want
    lo, hi = ENERGY3_CLIP
    if n >= 63:
        assert all((a < lo).any() and (a > hi).any() and ((a > lo) & (a < hi)).any() for a in (u, v, w))


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", POSITION_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_planted_cell_is_the_only_clear_maximum(kind, shape, periodic):
    """For every cell the GPU position tests use: np.argmax of the reference
    field is the cell and unique, the runner-up is below it by FACTOR, the
    maximum is finite and nonzero -- and it is the planting that does it."""
    nz, ny, nx = shape
    cells = positions3d(shape, periodic)
    corners = {(k, j, i) for k in (1, nz - 2) for j in (1, ny - 2) for i in (1, nx - 2)}
    assert corners <= set(cells) and len(set(cells)) == len(cells)
    for i in (63, 64, 255, 256, nx - 2):
        if 1 <= i <= nx - 2:
            assert {(k, j, i) for k in (1, nz - 2) for j in (1, ny - 2)} <= set(cells)
            if periodic:
                assert {(k, j, i) for k in (0, nz - 1) for j in (1, ny - 2)} <= set(cells)
    assert periodic or all(1 <= k <= nz - 2 for k, _, _ in cells)
    base = ref_field(kind, base_inputs(kind, shape), periodic)
    top = fold_absmax(base)
    assert np.isfinite(top) and top > 0
    for cell in cells:
        ins = plant_argmax(kind, shape, cell, periodic)
        which, site = plant_site(kind, shape, cell)
        assert ins[which][site] == PLANT and base_inputs(kind, shape)[which][site] != PLANT
        ref = ref_field(kind, ins, periodic)
        m = only_argmax(ref, cell)
        assert m == np.abs(ref[cell]) >= FACTOR * top
        changed = np.flatnonzero(ref.view(np.uint32) != base.view(np.uint32))
        assert changed.tolist() == [int(np.ravel_multi_index(cell, shape))], cell  # no other cell reads it
