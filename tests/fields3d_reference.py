"""Shapes, seeded inputs and plain references of the one-thread-per-cell 3-D
field kernels and their fused maxima (host only, no device code): what
tests/test_gpu_fields3d_shapes.py and tests/test_gpu_reductions3d.py compare
csrc/fields3d.hip with.  tests/test_fields3d_host.py pins everything here on
the CPU before any kernel is involved.

The arithmetic is not restated: the fields are the existing NumPy statements
(tests/ref3d.py, tests/cyl3d_reference.py, tests/zper_reference.py,
tests/les3d_reference.py) and the maximum is ``fold_absmax`` of
tests/diag_reference.py.  New here:

* ``SHAPES_3D``: one interior cell; nx around the 64-lane wave and the
  256-column workgroup with few rows and planes; a general shape; shapes
  whose largest face is nz*nx or nz*ny (k_lid_bc3d is launched over the
  largest of the three); ny and nz at 65535, the launch grid's limit.
* ``ref_field(kind, inputs, periodic)``: the field whose maximum a kernel
  fuses -- the divergence, |grad phi|, |omega|.
* ``plant_argmax`` / ``positions3d``: inputs whose reference field has its
  strict maximum at a chosen cell, and the cells it is steered to.
* ``energy_mean3_exact`` and ``ENERGY3_SIZES`` for cfd_energy_mean_clip3d_f32.
"""
import functools
import math

import numpy as np

from cyl3d_reference import vorticity3d_numpy
from diag_reference import fold_absmax
from ref3d import divergence3d_numpy, gradient3d_numpy, monitor_health3d_numpy
from zper_reference import crop_z, divergence3d_zper_numpy, pad_z, vorticity3d_zper_numpy

F = np.float32
DX, DY, DZ = 0.013, 0.0171, 0.0093  # dx != dy != dz throughout
SP = dict(dx=DX, dy=DY, dz=DZ)
DT = 2e-5
CS = 0.17

ONE_CELL = [(3, 3, 3)]
NX_EDGES = [(3, 3, 64), (3, 4, 65), (4, 3, 255), (3, 3, 256), (4, 5, 257), (3, 5, 513), (5, 3, 1030)]
GENERAL = [(7, 37, 260)]
# k_lid_bc3d's three faces: ny*nx, nz*nx and nz*ny cells.  (40, 3, 5): nz*nx = 200 is the largest,
# (40, 5, 3): nz*ny = 200, (3, 300, 3): ny*nx = nz*ny = 900, (300, 3, 4): nz*nx = 1200
FACE_DOMINANT = [(40, 3, 5), (40, 5, 3), (3, 300, 3), (300, 3, 4)]
# The launch is rounded up to workgroups of 256 threads, so a face shows only where it exceeds the
# other two rounded up: nz*nx does at (300, 3, 4) (1200 > 1024); for nz*ny the lid test adds
# (300, 4, 3) (1200 > 1024), which none of the shapes above provides
LID_EXTRA = [(300, 4, 3)]
GRID_LIMIT = 65535  # blockIdx.y / blockIdx.z of the per-cell launches
AT_GRID_LIMIT = [(3, GRID_LIMIT, 3), (GRID_LIMIT, 3, 3)]
SHAPES_3D = ONE_CELL + NX_EDGES + GENERAL + FACE_DOMINANT + AT_GRID_LIMIT
# where the fused maxima's argmax is steered around
POSITION_SHAPES = [(4, 5, 257), (5, 3, 1030), (7, 37, 260)]

# cfd_energy_mean_clip3d_f32's launcher: ceil(n / 4096) blocks of 256 threads, at most 512; a
# block's range is folded in rounds of 4 x 256 cells with a tail
ENERGY3_BLOCK_CELLS, ENERGY3_MAX_BLOCKS, ENERGY3_ROUND = 4096, 512, 1024
ENERGY3_FULL = ENERGY3_MAX_BLOCKS * ENERGY3_BLOCK_CELLS
ENERGY3_SIZES = [1, 63, 64, 65, 255, 256, 257, ENERGY3_ROUND - 1, ENERGY3_ROUND, ENERGY3_ROUND + 1,
                 ENERGY3_BLOCK_CELLS, ENERGY3_BLOCK_CELLS + 1, 2 * ENERGY3_BLOCK_CELLS + 1, ENERGY3_FULL,
                 ENERGY3_FULL + 1, 2 * ENERGY3_FULL + 77]
ENERGY3_CLIP = (F(-0.5), F(0.75))  # inside the inputs' range: both clips are active


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)  # the largest are the 2.4 MB fields of the 65535 shapes
def fields3d(shape):
    """u, v, w, phi (read-only): uniform (-1.5, 1.5), with u = v = w = 0
    exactly over a block (up to 2 planes x 3 rows x 70 columns)."""
    nz, ny, nx = shape
    assert min(shape) >= 3
    rng = np.random.default_rng([nz, ny, nx])
    u, v, w, phi = (rng.uniform(-1.5, 1.5, shape).astype(F) for _ in range(4))
    for f in (u, v, w):
        f[nz // 3:nz // 3 + 2, ny // 3:ny // 3 + 3, nx // 3:nx // 3 + 70] = 0
    return _frozen(u, v, w, phi)


@functools.lru_cache(maxsize=None)
def energy3_case(n):
    """(u, v, w, exact mean) of n cells: uniform (-1.5, 1.5), read-only."""
    rng = np.random.default_rng([n, 3])
    u, v, w = _frozen(*(rng.uniform(-1.5, 1.5, n).astype(F) for _ in range(3)))
    return u, v, w, energy_mean3_exact(u, v, w)


def energy_mean3_exact(u, v, w):
    """Mean of 0.5 ((u*u + v*v) + w*w): each cell in float32 in that order
    (k_energy_mean_clip3d, Cavity3DReference.time_step), then the correctly
    rounded sum of the float64 values, divided by n."""
    u, v, w = (np.asarray(a) for a in (u, v, w))
    assert u.dtype == v.dtype == w.dtype == F
    with np.errstate(all="ignore"):
        e = F(0.5) * ((u * u + v * v) + w * w)
    assert e.dtype == F
    x = e.astype(np.float64).ravel()
    return math.fsum(x.tolist()) / x.size


# ------------------------------------------------------- reference fields
KINDS = ("div", "grad", "vort")


def grad_mag3d(phi, periodic=False):
    """sqrt((gx gx + gy gy) + gz gz) of gradient3d_numpy (the pad rule when periodic)."""
    with np.errstate(all="ignore"):
        gx, gy, gz = gradient3d_numpy(pad_z(phi) if periodic else phi, **SP)
        g = np.sqrt((gx * gx + gy * gy) + gz * gz)
    assert g.dtype == F
    return crop_z(g) if periodic else g


def base_inputs(kind, shape):
    """The unplanted inputs of ``kind``: (u, v, w), or (phi,) for the gradient."""
    u, v, w, phi = fields3d(shape)
    return (phi,) if kind == "grad" else (u, v, w)


def ref_field(kind, inputs, periodic=False):
    """The field whose maximum the kernel of ``kind`` fuses: the divergence
    (its maximum is of |div|), |grad phi| or |omega|."""
    with np.errstate(all="ignore"):
        if kind == "div":
            return (divergence3d_zper_numpy if periodic else divergence3d_numpy)(*inputs, **SP)
        if kind == "grad":
            return grad_mag3d(*inputs, periodic)
        if kind == "vort":
            return (vorticity3d_zper_numpy if periodic else vorticity3d_numpy)(*inputs, DX, DY, DZ)[3]
    raise ValueError(kind)


# ------------------------------------------------------ steering the argmax
PLANT = F(-112.0)  # against inputs within (-1.5, 1.5)
FACTOR = 2.0       # the planted maximum exceeds every other cell at least this many times


def plant_site(kind, shape, cell):
    """(index of the input, the cell of it) to raise so that ``cell`` alone
    changes: the neighbour of ``cell`` on the wall row next to it, in the
    input whose y-difference enters the field (v for the divergence, phi for
    the gradient, u for the vorticity's z component).  A wall row's own field
    is 0 with and without a periodic z, and its other differences run along
    the wall, so no other cell reads the raised value."""
    nz, ny, nx = shape
    k, j, i = cell
    assert j in (1, ny - 2) and 1 <= i <= nx - 2 and 0 <= k < nz, (shape, cell)
    return {"div": 1, "grad": 0, "vort": 0}[kind], (k, 0 if j == 1 else ny - 1, i)


def plant_argmax(kind, shape, cell, periodic, value=PLANT):
    """The inputs of ``kind`` (base_inputs with one neighbour of ``cell``
    set to ``value``) for which ref_field has its strict maximum at ``cell``,
    at least FACTOR times every other cell's magnitude."""
    assert periodic or 1 <= cell[0] <= shape[0] - 2, (shape, cell)
    which, site = plant_site(kind, shape, cell)
    ins = list(base_inputs(kind, shape))
    ins[which] = np.array(ins[which])
    ins[which][site] = value
    return tuple(ins)


def positions3d(shape, periodic):
    """The eight corners of the interior, and the columns 63, 64, 255, 256 and
    nx - 2 (where interior) in the first and last interior row and plane;
    periodic: the same on the wrap planes 0 and nz - 1 too."""
    nz, ny, nx = shape
    ks = [1, nz - 2] + ([0, nz - 1] if periodic else [])
    cols = [1, nx - 2] + [i for i in (63, 64, 255, 256) if 1 <= i <= nx - 2]
    return list(dict.fromkeys((k, j, i) for k in ks for j in (1, ny - 2) for i in cols))


def only_argmax(ref, cell):
    """The fold over ``ref``; asserts that it is finite, nonzero, attained at
    ``cell`` alone and at least FACTOR times the runner-up."""
    a = np.abs(ref)
    m = fold_absmax(ref)
    flat = int(np.ravel_multi_index(cell, ref.shape))
    assert np.isfinite(m) and m > 0 and not np.isnan(a).any()
    assert np.flatnonzero(a == m).tolist() == [flat] and int(np.argmax(a)) == flat, (ref.shape, cell)
    rest = np.delete(a.ravel(), flat)
    assert rest.size == 0 or m >= FACTOR * rest.max(), (ref.shape, cell, m, rest.max())
    return m


def health3d_reference(u, v, w, cfg, step, periodic=False):
    """monitor_health3d_numpy; with a periodic z on the padded fields (the pad
    rule: the same values, and the padded planes' divergence is 0)."""
    if periodic:
        u, v, w = pad_z(u), pad_z(v), pad_z(w)
    with np.errstate(all="ignore"):
        return bool(monitor_health3d_numpy(u, v, w, cfg, step))
