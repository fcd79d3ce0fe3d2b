"""The Poisson solves at edge values, route by route, against the oracle.

Every dispatch route of the 2-D / 3-D Jacobi and red-black GS solves runs the
input classes of tests/poisson_edge_reference.py -- non-finite seeds, signed
zeros, subnormals, values that overflow -- and must give the C oracle's result
under ``same_bits`` (NaNs in the same cells, every other cell bit for bit, so
-0.0 != +0.0) and, where there is one, the oracle's iteration count.
tests/test_poisson_edge_host.py shows the oracle equal to an independent NumPy
statement on these classes and asserts, for every case used here, that the
reference result holds what the class promises.  The zero-start solves never
read phi0, so they carry only the div-borne part of a class (the NaN and -Inf
seeds of div, the subnormal div; no -0.0, no overflow): what they add is that
a garbage phi is not read.

Routes are selected with the library's own knobs, as the cited existing tests
select them; where the library reports the route (cfd_get_last_jacobi2d_path,
cfd_get_last_tbr_shape, cfd_get_jacobi3d_levels, cfd_get_rbgs3d_levels) the
test asserts that it ran.

The stop rule: the oracle stops on max|change| < f32(tol).  Per GS route:
tol equal to an iteration's max|change| does not stop at it and the next
float up does; a NaN, negative or float-zero tol runs every iteration and an
infinite one stops after the first; NaN changes never count (a solve with a
moving NaN front still stops), infinite ones do.

The residual outputs follow the same fold (fold_max): from 0, a NaN change
never raises it, an infinite one does.
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import oracle
import poisson_edge_reference as R
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd import slab as S
from cfd_simulations_amd._lib import call, lib, ptr
from poisson_edge_reference import CLASSES, describe_difference, fold_max, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
NAN = float("nan")
classes = pytest.mark.parametrize("cls", CLASSES)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # (a copy: the shared inputs are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def last_shape():
    v = [ctypes.c_int() for _ in range(4)]
    call("cfd_get_last_tbr_shape", *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def j2_path():
    spl = ctypes.c_int(-1)
    return lib().cfd_get_last_jacobi2d_path(ctypes.byref(spl)), spl.value


@pytest.fixture(autouse=True)
def cfd_reset_tuning():
    call("cfd_reset_tuning")
    yield
    call("cfd_reset_tuning")
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device error ends the run: nothing more is started on that device
        pytest.exit(f"device error after a Poisson edge test: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def case_ref(name, cls, masked=True, zero=False, nan_only=False, tol=0.0):
    """(operator, case, iterations, reference phi, reference count), computed once."""
    op, case, iters = R.gpu_case(name, cls, masked, nan_only)
    assert not zero or name in R.ZERO_START_CASES      # (the host file asserts what a zero start leaves of a class)
    ref, n = R.reference(op, case, iters, tol=tol, zero=zero)
    ref.setflags(write=False)
    return op, case, iters, ref, n


def agree(got, ref, *what):
    assert same_bits(got, ref), (what, describe_difference(got, ref))


def garbage(case):
    """A start the zero-start solves must not read: NaN inside, 7 on the ring."""
    g = np.full(case.shape, np.nan, case.div.dtype)
    g[0], g[-1], g[:, 0], g[:, -1] = 7.0, 7.0, 7.0, 7.0
    return g


# ================================================================ 2-D Jacobi
def run_j2(case, iters, masked, rhs, zero):
    phi = dev(garbage(case) if zero else case.phi0)
    K.solve_pressure_jacobi(phi, dev(case.div), case.dx, case.dt, dev(case.mask) if masked else None, iters,
                            rhs_ws=torch.full_like(phi, NAN) if rhs else None, zero_start=zero)
    return host(phi)


def sweep_j2(name, cls, path=None, combos=None):
    """One route over mask / workspace / zero-start settings."""
    for masked, rhs, zero in combos or [(m, r, z) for m in (True, False) for r in (False, True) for z in (False, True)]:
        op, case, iters, ref, _ = case_ref(name, cls, masked, zero)
        agree(run_j2(case, iters, masked, rhs, zero), ref, name, cls, masked, rhs, zero)
        if path is not None:
            assert j2_path() == path(iters), (j2_path(), masked, rhs, zero)


@classes
@pytest.mark.parametrize("name", ["j2_single", "j2_single_f64"])
def test_jacobi2d_single_sweeps(name, cls):
    """(37, 53): unaligned rows, one cell per lane, blocking off."""
    call("cfd_set_jacobi2d_blocking", 1)
    sweep_j2(name, cls, lambda it: (0, 1))


@classes
@pytest.mark.parametrize("depth", [2, 4, 8])
@pytest.mark.parametrize("name", ["j2_blocked", "j2_blocked_f64"])
def test_jacobi2d_blocked_passes(name, depth, cls):
    """jacobi2d_tbk at 2, 4 and 8 sweeps per pass (9 sweeps: passes and a last
    single sweep), with and without a mask; staged rows (4 ahead) without."""
    call("cfd_set_jacobi2d_blocking", depth)
    assert lib().cfd_get_jacobi2d_levels() == depth
    sweep_j2(name, cls, lambda it: (0, depth))
    if depth >= 4:
        call("cfd_set_jacobi2d_staging", 4)
        sweep_j2(name, cls, lambda it: (0, depth), [(False, False, False), (False, True, False)])


@classes
@pytest.mark.parametrize("shape", [None, (5, 1, 4)], ids=["default", "k5-rw1-vec4"])
@pytest.mark.parametrize("name", ["j2_blocked", "j2_blocked_f64"])
def test_jacobi2d_small_grid_launch_per_pass(name, shape, cls):
    """The preloaded small-grid kernel (the persistent solve off), as
    test_jacobi2d_small_shapes_bitexact selects it."""
    if shape:
        call("cfd_set_small2d_shape", *shape, 0, 0, 0)
    call("cfd_set_small2d_jacobi_persistent", 1, 0)
    sweep_j2(name, cls)
    flag, spl = j2_path()
    assert flag == 0 and (spl == 5 if shape else 1 <= spl <= 8), (flag, spl)


@classes
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("name,ni", [("j2_persist_53_7", 4), ("j2_persist_53_13", 10), ("j2_persist_36_7", 4),
                                     ("j2_persist_36_13", 10)])
def test_jacobi2d_persistent(name, ni, mode, cls):
    """jacobi2d_persist, one and two sweeps per LDS exchange, 4 and 10 sweeps
    per block, two blocks each (7 and 13 sweeps: an odd remainder), solid
    cells on the ring as in test_jacobi2d_persistent_bitexact."""
    call("cfd_set_small2d_jacobi_persistent", mode, ni)
    sweep_j2(name, cls, lambda it: (1, it))
    assert K.persistent_failures() == 0


# ================================================================ 2-D GS
def run_gs2(case, iters, tol, masked, zero=False):
    phi = dev(garbage(case) if zero else case.phi0)
    done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    K.solve_pressure_gauss_seidel_fast(phi, dev(case.div), case.dx, case.dy, case.dt,
                                       dev(case.mask) if masked else None, iters, tol, iters_done=done,
                                       zero_start=zero)
    return host(phi), int(host(done)[0])


def sweep_gs2(name, cls, zeros=(False,)):
    for masked in (True, False):
        for zero in zeros:
            op, case, iters, ref, n_ref = case_ref(name, cls, masked, zero)
            got, n = run_gs2(case, iters, 0.0, masked, zero)
            assert n == n_ref == iters, (n, n_ref)
            agree(got, ref, name, cls, masked, zero)


def gs2_colour_passes():
    call("cfd_set_jacobi2d_blocking", 1)


def gs2_per_wave(shape):
    def select():
        vec, rw, wpb = shape
        call("cfd_set_small2d_shape", 0, 0, 0, rw, vec, wpb)
        call("cfd_set_small2d_gs_iters", 2, 1)
    return select


def gs2_tile(ni, persistent):
    """The persistent GS has no path reporter; its diagnostic trace (block
    timestamps per tile, cfd_set_small2d_gs_trace) is written by the only
    kernel a GS solve launches that writes it (the persistent Jacobi writes
    the same buffer; no Jacobi solve runs between select() and ran()), so
    ``select.ran()`` tells whether the persistent solve ran."""
    def select():
        call("cfd_set_small2d_gs_iters", ni, 2)
        call("cfd_set_small2d_gs_persistent", persistent)
        select.trace = torch.zeros(1 << 19, dtype=torch.int64, device=DEV)
        call("cfd_set_small2d_gs_trace", ptr(select.trace), select.trace.numel() * 8)

    def ran():
        wrote = bool(host(select.trace).any())
        call("cfd_set_small2d_gs_trace", None, 0)
        select.trace = None
        return wrote
    select.ran = ran
    select.persistent = persistent != 1
    return select


def assert_gs2_route(select):
    if hasattr(select, "ran"):
        assert select.ran() == select.persistent


# (id, knobs, case name, iterations per launch / block)
GS2_ROUTES = [("colour", gs2_colour_passes, "gs2_color", 1), ("colour-vec4", gs2_colour_passes, "gs2_color_vec", 1),
              ("wave-1-1-4", gs2_per_wave((1, 1, 4)), "gs2_color_vec", 2),
              ("wave-4-2-16", gs2_per_wave((4, 2, 16)), "gs2_color_vec", 2)] + \
             [(f"tile-ni{ni}-p{p}", gs2_tile(ni, p), "gs2_tile_5" if ni == 2 else "gs2_tile_7", ni)
              for ni in (2, 5) for p in (1, 2, 3)] + \
             [("march", lambda: None, "gs2_march", 1)]
gs2_routes = pytest.mark.parametrize("select,name,block", [r[1:] for r in GS2_ROUTES], ids=[r[0] for r in GS2_ROUTES])


@classes
@gs2_routes
def test_rbgs2d_routes(select, name, block, cls):
    """In-place colour passes (one and four cells per lane), the fused
    per-wave kernel, the shared-row tile per launch (1) and as the persistent
    solve (2, 3) at 2 and 5 iterations per block, and the row march rbgs2d_tb,
    whose smallest grid is 16387 rows (poisson2d.hip: more than 16384 chunks
    of one row and segment)."""
    select()
    sweep_gs2(name, cls)
    assert K.persistent_failures() == 0
    assert_gs2_route(select)


@classes
@pytest.mark.parametrize("persistent", [1, 2])
def test_rbgs2d_zero_start(persistent, cls):
    """cfd_rbgs2d_zero_f32_ws on the launch-per-block path (1: zero fill
    first) and as the persistent solve (2: nothing of phi read), two
    iterations per block.  phi0 is never read, so what is left of a
    class is its div-borne part (test_poisson_edge_host.py asserts what)."""
    select = gs2_tile(2, persistent)
    select()
    sweep_gs2("gs2_tile_5", cls, zeros=(True,))
    assert K.persistent_failures() == 0
    assert_gs2_route(select)


@classes
def test_rbgs2d_float64_colour_passes(cls):
    """cfd_rbgs2d_f64 against the float64 statement (pinned to the reference's
    float64 fixture on the host)."""
    sweep_gs2("gs2_f64", cls, zeros=(False, True))


# ================================================================ 3-D Jacobi
def run_j3(case, iters, masked, rhs):
    phi = dev(case.phi0)
    K.solve_pressure_jacobi3d(phi, dev(case.div), case.dx, case.dt, dev(case.mask) if masked else None, iters,
                              phi_tmp=torch.full_like(phi, NAN), rhs_ws=torch.full_like(phi, NAN) if rhs else None)
    return host(phi)


def run_j3_zero(case, iters, rhs):
    phi = dev(garbage(case))
    K.solve_pressure_jacobi3d_zero(phi, dev(case.div), case.dx, case.dt, iters, phi_tmp=torch.full_like(phi, NAN),
                                   rhs_ws=torch.full_like(phi, NAN) if rhs else None)
    return host(phi)


@classes
@pytest.mark.parametrize("variant", [1, 2])
def test_jacobi3d_single_sweeps(variant, cls):
    """The LDS plane tile (1) and the cache kernel (2), with and without a
    3-D mask, with and without the RHS workspace."""
    call("cfd_set_jacobi3d_blocking", 1, 0, 0)
    call("cfd_set_jacobi3d_config", variant, 0, 0)
    before = last_shape()
    for masked in (True, False):
        for rhs in (False, True):
            op, case, iters, ref, _ = case_ref("j3_single", cls, masked)
            agree(run_j3(case, iters, masked, rhs), ref, cls, variant, masked, rhs)
    assert last_shape() == before        # no tall-tile launch


# Levels of the last tall-tile launch of the 5-sweep solve, by (levels per
# pass, workspace given).  Without the workspace: passes of K, then the
# remainder (2+2+1, 3+2, 4+1; a remainder of 1 is a single sweep, no tall
# tile).  With it the short pass comes first: 2+2+1, 2+3, 3+2.
LAST_TBR_LEVELS_OF_5 = {(2, False): 2, (3, False): 2, (4, False): 4,
                        (2, True): 2, (3, True): 3, (4, True): 2}


@classes
@pytest.mark.parametrize("levels", [2, 3, 4])
def test_jacobi3d_tall_tile_passes(levels, cls):
    """jacobi3d_tbr at 2, 3 and 4 levels: a general start without the
    workspace and with it (the RHS-forming first pass), and from zeros."""
    call("cfd_set_jacobi3d_blocking", levels, 0, 0)
    assert lib().cfd_get_jacobi3d_levels() == levels
    op, case, iters, ref, _ = case_ref("j3_blocked", cls, False)
    assert iters == 5
    for rhs in (False, True):
        agree(run_j3(case, iters, False, rhs), ref, cls, levels, rhs)
        assert last_shape()[0] == LAST_TBR_LEVELS_OF_5[levels, rhs], (last_shape(), rhs)
    zref = case_ref("j3_blocked", cls, False, True)[3]
    for rhs in (False, True):
        agree(run_j3_zero(case, iters, rhs), zref, cls, levels, rhs, "zero")
        assert last_shape()[0] == LAST_TBR_LEVELS_OF_5[levels, rhs], (last_shape(), rhs)


@classes
@pytest.mark.parametrize("name,zchunk", [("j3_k4_small", 0), ("j3_k4_small", 5), ("j3_k4_deep", 44)])
def test_jacobi3d_k4_routes(name, zchunk, cls):
    """The (4, 11, 2) tile as tests/test_gpu_tbr_k4_t1d.py and
    test_gpu_tbr_k4_rotated.py select it: short chunks (shifting queues) on
    their smallest grid, and the rotated march on a 44-plane chunk."""
    call("cfd_set_jacobi3d_blocking", 4, 16, zchunk)
    call("cfd_set_jacobi3d_prefetch", 1)
    op, case, iters, ref, _ = case_ref(name, cls, False)
    zref = case_ref(name, cls, False, True)[3]
    assert iters == 4
    for rhs in (False, True):
        agree(run_j3(case, iters, False, rhs), ref, cls, name, zchunk, rhs)
        assert last_shape()[:3] == (4, 11, 2), last_shape()
        agree(run_j3_zero(case, iters, rhs), zref, cls, name, zchunk, rhs, "zero")
        assert last_shape()[:3] == (4, 11, 2), last_shape()


@classes
def test_jacobi3d_sweep_range(cls):
    """slab.sweep_range, the slab driver's building block: planes 1 .. nz-2 of
    one sweep (rows 0 and ny-1 and the end planes are the caller's)."""
    for masked in (True, False):
        op, case, _, _, _ = case_ref("j3_single", cls, masked)
        ref = oracle.jacobi3d(case.div, case.phi0, h=case.dx, dt=case.dt, iters=1, mask=case.mask)
        out = torch.full(case.shape, NAN, dtype=torch.float32, device=DEV)
        m = dev(case.mask.astype(np.uint8)) if masked else None
        S.sweep_range(dev(case.phi0), out, dev(case.div), m, 1, case.shape[0] - 1, case.dx, case.dt)
        agree(host(out)[1:-1, 1:-1], ref[1:-1, 1:-1], cls, masked)


# ================================================================ 3-D GS
def run_gs3(case, iters, tol, mask):
    phi = dev(case.phi0)
    done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    K.solve_pressure_gauss_seidel3d(phi, dev(case.div), case.dx, case.dy, case.dz, case.dt,
                                    None if mask is None else dev(mask), iters, tol, iters_done=done,
                                    phi_tmp=torch.full_like(phi, NAN))
    return host(phi), int(host(done)[0])


def run_zper(case, iters, tol, masked, tmp=True):
    """tests/test_gpu_zper.py's call: ghost planes and phi_tmp handed over as NaN."""
    G = int(lib().cfd_rbgs3d_zper_ghost())
    nz = case.shape[0]

    def padded(a):
        p = np.full((nz + 2 * G,) + a.shape[1:], np.nan, F)
        p[G:G + nz] = a
        return dev(p)
    phi, d = padded(case.phi0), padded(case.div)
    done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    K.solve_pressure_gauss_seidel3d_zper(phi, d, case.dx, case.dy, case.dz, case.dt,
                                         dev(case.mask[0].astype(np.uint8)) if masked else None, iters, tol,
                                         iters_done=done, phi_tmp=torch.full_like(phi, NAN) if tmp else None, nz=nz)
    return host(phi)[G:G + nz], int(host(done)[0])


@classes
def test_rbgs3d_colour_passes_with_a_3d_mask(cls):
    op, case, iters, ref, n_ref = case_ref("gs3_color", cls, True)
    before = last_shape()
    got, n = run_gs3(case, iters, 0.0, case.mask)
    assert n == n_ref == iters
    agree(got, ref, cls)
    assert last_shape() == before


@classes
@pytest.mark.parametrize("levels", [2, 3, 4])
def test_rbgs3d_fused_passes(levels, cls):
    """Fused passes of 2, 3 and 4 half-sweeps without a mask; 3 iterations
    are 2+2+2, 3+3 and 4+2 half-sweeps."""
    call("cfd_set_jacobi3d_blocking", levels, 0, 0)
    assert lib().cfd_get_rbgs3d_levels() == levels
    op, case, iters, ref, n_ref = case_ref("gs3_fused", cls, False)
    got, n = run_gs3(case, iters, 0.0, None)
    assert n == n_ref == iters
    agree(got, ref, cls, levels)
    assert last_shape()[0] == {2: 2, 3: 3, 4: 2}[levels], last_shape()


@classes
@pytest.mark.parametrize("levels,rows,last", [(4, 16, (2, 9, 2)), (2, 16, (2, 9, 2)), (1, 0, None)],
                         ids=["fused4", "fused2", "in-place"])
def test_rbgs3d_mask2d(levels, rows, last, cls):
    """cfd_rbgs3d_mask2d_f32 on the tall tiles of tests/test_gpu_rbgs3d_mask2d.py
    and, with blocking off, as in-place colour passes."""
    op, case, iters, ref, n_ref = case_ref("gs3_fused", cls, True)
    before = last_shape()
    call("cfd_set_jacobi3d_blocking", levels, rows, 0)
    got, n = run_gs3(case, iters, 0.0, case.mask[0])
    assert n == n_ref == iters
    agree(got, ref, cls, levels)
    assert last_shape()[:3] == (last if last else before[:3]), last_shape()
    if last is None:
        assert last_shape() == before


@classes
@pytest.mark.parametrize("route", ["fused", "in-place"])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_rbgs3d_zper(masked, route, cls):
    """The z-periodic solve, fused (wrap after every pass) and in place (no
    phi_tmp), against tests/zper_reference.py's statement."""
    op, case, iters, ref, n_ref = case_ref("gs3_zper", cls, masked)
    before = last_shape()
    got, n = run_zper(case, iters, 0.0, masked, tmp=route == "fused")
    assert n == n_ref == iters
    agree(got, ref, cls, masked, route)
    if route == "fused":
        assert last_shape()[0] == 2, last_shape()       # 6 half-sweeps: 4 + 2
    else:
        assert last_shape() == before


def run_slab(case, iters, tol, R_=2, ghost=2, steps=2):
    """test_slab_rbgs_local_group_multirank's set-up: R ranks as host threads
    on one GPU, each with its stream and its own tuning."""
    nz, ny, nx = case.shape
    comms = S.LocalComm.group(R_)
    sols = []
    for r in range(R_):
        plan = S.SlabPlan(nz, R_, r, ghost=ghost)
        sg = S.SlabRBGS3D(plan, ny, nx, case.dx, case.dy, case.dz, case.dt, comms[r])
        sg.div.copy_(dev(plan.scatter(case.div)))
        sg.phi.copy_(dev(plan.scatter(case.phi0)))
        sols.append(sg)
    streams = [torch.cuda.Stream() for _ in range(R_)]
    torch.cuda.synchronize()
    errs = [None] * R_

    def work(r):
        try:
            call("cfd_set_jacobi3d_blocking", steps, 0, 0)
            with torch.cuda.stream(streams[r]):
                sols[r].solve(iters, tolerance=tol, overlap=False, zero_phi=False)
            streams[r].synchronize()
        except Exception as e:  # noqa: BLE001 -- reported below
            errs[r] = e

    th = [threading.Thread(target=work, args=(r,)) for r in range(R_)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    alive = any(t.is_alive() for t in th)
    if not alive:
        torch.cuda.synchronize()
        for c in comms:
            c.close()
    assert not alive, "a rank did not return"
    assert errs == [None] * R_, errs
    counts = [int(host(sg.iters_done)[0]) for sg in sols]
    return np.concatenate([host(sg.owned()) for sg in sols]), counts


@classes
def test_rbgs3d_two_rank_slab(cls):
    """One 2-rank local-group solve (fused passes, ghost 2): the cross-rank
    max fold and the ghost exchange carry the edge values."""
    op, case, iters, ref, n_ref = case_ref("gs3_slab", cls, False)
    got, counts = run_slab(case, iters, 0.0)
    assert counts == [n_ref, n_ref]
    agree(got, ref, cls)


# ================================================================ the stop rule
def history(op, case, n):
    """The reference's max|change| of iterations 1 .. n (tol = 0)."""
    kw = dict(dx=case.dx, dy=case.dy, dt=case.dt)
    if op == "gs2d" and case.div.dtype == np.float64:
        return R.rbgs2d_statement(case.div, case.phi0, iters=n, tol=0.0, mask=case.mask, **kw)[2]
    if op == "gs2d":
        return oracle.rbgs2d_maxc(case.div, case.phi0, iters=n, tol=0.0, mask=case.mask, **kw)[2]
    if op == "gs3d":
        return R.rbgs3d_maxc(oracle.rbgs3d, case.div, case.phi0, n, dz=case.dz, mask=case.mask, **kw)
    assert op == "gs3zper", op
    from zper_reference import rbgs3d_zper_numpy
    mc = []
    with np.errstate(all="ignore"):
        rbgs3d_zper_numpy(case.div, case.phi0, iters=n, tol=0.0, dz=case.dz, maxc=mc,
                          mask2d=None if case.mask is None else case.mask[0], **kw)
    return np.array(mc, F)


@functools.lru_cache(maxsize=None)
def stop_problem(op, shape, dtype=F):
    """Ordinary data with a strictly decreasing max|change| history."""
    rng = np.random.default_rng(3)
    div = (rng.standard_normal(shape).astype(F) * F(1e-2)).astype(dtype)
    div.setflags(write=False)
    case = R.Case(div, np.zeros_like(div), None, 0.1, 0.1, 0.1, F(1.0))
    mc = history(op, case, 10)
    assert mc.dtype == dtype and (np.diff(mc) < 0).all() and (mc > 0).all(), mc
    return case, mc


def check_stop_rule(run, name, N=8, cs=(2, 3, 4)):
    """``run(case, iters, tol) -> (phi, count)`` on one route, against the
    reference of GPU case ``name``'s operator, shape and type."""
    op, shape, dtype = R.GPU_CASES[name][:3]
    up = lambda x: float(np.nextafter(x, dtype(np.inf)))  # noqa: E731

    def both(case, iters, tol, want, *what):
        ref, n_ref = R.reference(op, case, iters, tol=tol)
        assert n_ref == want, (what, n_ref, want)
        got, n = run(case, iters, tol)
        assert n == n_ref, (what, tol, n, n_ref)
        agree(got, ref, *what)
        return ref

    case, mc = stop_problem(op, shape, dtype)
    for c in cs:
        both(case, N, float(mc[c]), c + 2, "tol == max|change|", c)
        both(case, N, up(mc[c]), c + 1, "the next float up", c)
    # (float64: the solve compares with the double itself; 1e-50 is then a positive tolerance no change is below)
    for tol, want in ((np.nan, N), (-1.0, N), (1e-50, N), (np.inf, 1)):
        both(case, N, tol, want, "tol", tol)
    # NaN seeds alone: the NaN front moves every iteration, the solve stops all the same
    _, ncase, _ = R.gpu_case(name, "nonfinite", False, nan_only=True)
    hist = history(op, ncase, N)
    assert np.isfinite(hist).all() and (np.diff(hist[:5]) < 0).all(), hist
    full = R.reference(op, ncase, N)[0]
    ref = both(ncase, N, up(hist[3]), 4, "NaN front")
    assert 20 <= np.isnan(ref).sum() < np.isnan(full).sum()
    # with an infinite seed every iteration's max|change| is Inf: no stop below Inf
    _, icase, _ = R.gpu_case(name, "nonfinite", False)
    assert np.isinf(history(op, icase, 4)).all()
    both(icase, 4, 1e30, 4, "infinite change")


@gs2_routes
def test_rbgs2d_stop_rule(select, name, block):
    """Stops at iterations 3 .. 6 of 8: inside and on the edge of blocks of 2
    and of 5 iterations."""
    select()
    check_stop_rule(lambda case, iters, tol: run_gs2(case, iters, tol, False), name)
    assert K.persistent_failures() == 0
    assert_gs2_route(select)


def test_rbgs2d_float64_stop_rule():
    """cfd_rbgs2d_f64 (colour passes, its own double max fold) against the
    float64 statement's history."""
    check_stop_rule(lambda case, iters, tol: run_gs2(case, iters, tol, False), "gs2_f64")


def prime_last_shape(levels):
    """Leave cfd_get_last_tbr_shape at ``levels``, which the route under test
    never launches, so that its own launches show: an unmasked fused solve
    whose half-sweeps are a whole number of passes."""
    call("cfd_set_jacobi3d_blocking", levels, 0, 0)
    case, _ = stop_problem("gs3d", R.GPU_CASES["gs3_fused"][1])
    run_gs3(case, {3: 3, 4: 2}[levels], 0.0, None)
    assert last_shape()[0] == levels, last_shape()
    call("cfd_reset_tuning")


# route -> (blocking, levels its launches may have: the pass, and the shorter
# remainder and rollback launches; empty: no tall-tile launch at all)
GS3_STOP_ROUTES = {"colour-mask3d": ((0, 0, 0), ()), "fused2": ((2, 0, 0), (2,)), "fused3": ((3, 0, 0), (3, 2, 1)),
                   "fused4": ((4, 0, 0), (4, 2)), "mask2d-fused": ((0, 0, 0), (4, 2)),
                   "mask2d-in-place": ((1, 0, 0), ())}


@pytest.mark.parametrize("route", sorted(GS3_STOP_ROUTES))
def test_rbgs3d_stop_rule(route):
    blocking, may = GS3_STOP_ROUTES[route]
    shape = R.GPU_CASES["gs3_fused"][1]
    primed = 3 if 4 in may else 4
    prime_last_shape(primed)
    before = last_shape()
    call("cfd_set_jacobi3d_blocking", *blocking)
    nothing3 = np.zeros(shape, bool)        # an empty mask selects the masked routes and changes no value
    mask = {"colour-mask3d": nothing3, "mask2d-fused": nothing3[0], "mask2d-in-place": nothing3[0]}.get(route)
    seen = set()

    def run(case, iters, tol):
        out = run_gs3(case, iters, tol, mask)
        seen.add(last_shape())
        return out
    check_stop_rule(run, "gs3_fused")
    if may:     # (the primed level is none of them: every solve launched tall tiles of this route;
        #          a solve that may stop ends with its rollback launches, so the pass itself need not show)
        assert lib().cfd_get_rbgs3d_levels() == may[0]
        assert seen and all(s[0] in may for s in seen), (seen, may)
    else:
        assert seen == {before}, (seen, before)


@pytest.mark.parametrize("route", ["fused", "in-place"])
def test_rbgs3d_zper_stop_rule(route):
    """The periodic solve (its own ghost wrap and count) against its
    statement's history; fused: passes of 4 half-sweeps, remainders and
    rollbacks of 2."""
    prime_last_shape(3)
    before = last_shape()
    seen = set()

    def run(case, iters, tol):
        out = run_zper(case, iters, tol, False, tmp=route == "fused")
        seen.add(last_shape())
        return out
    check_stop_rule(run, "gs3_zper", cs=(2, 3))
    if route == "fused":
        assert lib().cfd_get_rbgs3d_levels() == 4
        assert seen and all(s[0] in (4, 2) for s in seen), seen
    else:
        assert seen == {before}, (seen, before)


def test_rbgs3d_two_rank_slab_stop_rule():
    """Every rank stops at the same iteration: the cross-rank max fold."""
    def run(case, iters, tol):
        got, counts = run_slab(case, iters, tol)
        assert counts[0] == counts[1], counts
        return got, counts[0]
    check_stop_rule(run, "gs3_slab", cs=(2, 3))


# ================================================================ the residual
def resid_reference(step, case, iters, every):
    """fold_max over two successive oracle states, rows 1 .. ny-2 (and planes
    1 .. nz-2) of every column: the cells a sweep writes."""
    phi, out = np.array(case.phi0), []
    for it in range(1, iters + 1):
        nxt = step(phi)
        if it % every == 0:
            out.append(fold_max(phi[(slice(1, -1),) * (phi.ndim - 1)], nxt[(slice(1, -1),) * (phi.ndim - 1)]))
        phi = nxt
    return np.array(out, case.div.dtype), phi


@pytest.mark.parametrize("cls", ["nonfinite", "signed_zero"])
@pytest.mark.parametrize("name", ["j2_single", "j2_single_f64", "j3_single"])
def test_jacobi_residual_fold(name, cls):
    every = 2
    for masked in (True, False):
        op, case, iters, ref, _ = case_ref(name, cls, masked)
        if op == "jacobi2d":
            step = lambda p: oracle.jacobi2d(case.div, p, dx=case.dx, dt=case.dt, iters=1, mask=case.mask)  # noqa: E731
        else:
            step = lambda p: oracle.jacobi3d(case.div, p, h=case.dx, dt=case.dt, iters=1, mask=case.mask)  # noqa: E731
        want, end = resid_reference(step, case, iters, every)
        assert same_bits(end, ref) and len(want) == iters // every
        if cls == "nonfinite":
            assert np.isinf(want).all()      # a cell turning infinite: an infinite change counts
        else:
            assert np.isfinite(want).all() and (want > 0).all()
        phi = dev(case.phi0)
        out = torch.full((len(want),), NAN, dtype=phi.dtype, device=DEV)
        solve = K.solve_pressure_jacobi if op == "jacobi2d" else K.solve_pressure_jacobi3d
        solve(phi, dev(case.div), case.dx, case.dt, dev(case.mask) if masked else None, iters, resid_every=every,
              resid_out=out)
        agree(host(phi), ref, name, cls, masked)
        agree(host(out), want, name, cls, masked, "residual")


@pytest.mark.parametrize("name", ["j2_single", "j2_single_f64", "j3_single"])
def test_jacobi_residual_nan_changes_never_count(name):
    """NaN seeds alone: the residual is the finite cells' largest change,
    whatever the NaN front does; and a start of NaN everywhere gives 0."""
    op, case, iters, _, _ = case_ref(name, "nonfinite", False, False, True)
    two_d = op == "jacobi2d"
    solve = K.solve_pressure_jacobi if two_d else K.solve_pressure_jacobi3d
    if two_d:
        step = lambda p: oracle.jacobi2d(case.div, p, dx=case.dx, dt=case.dt, iters=1)  # noqa: E731
    else:
        step = lambda p: oracle.jacobi3d(case.div, p, h=case.dx, dt=case.dt, iters=1)  # noqa: E731
    want, end = resid_reference(step, case, iters, 1)
    assert np.isfinite(want).all() and (want > 0).all() and np.isnan(end).sum() >= 20
    phi = dev(case.phi0)
    out = torch.full((iters,), NAN, dtype=phi.dtype, device=DEV)
    solve(phi, dev(case.div), case.dx, case.dt, None, iters, resid_every=1, resid_out=out)
    agree(host(phi), end, name)
    agree(host(out), want, name, "residual")
    allnan = np.full(case.shape, np.nan, case.div.dtype)
    out = torch.full((2,), NAN, dtype=phi.dtype, device=DEV)
    solve(dev(allnan), dev(case.div), case.dx, case.dt, None, 2, resid_every=1, resid_out=out)
    agree(host(out), np.zeros(2, case.div.dtype), name, "all NaN")


@pytest.mark.parametrize("cls", ["nonfinite", "signed_zero"])
def test_sweep_range_residual_fold(cls):
    op, case, _, _, _ = case_ref("j3_single", cls, True)
    nxt = oracle.jacobi3d(case.div, case.phi0, h=case.dx, dt=case.dt, iters=1, mask=case.mask)
    want = fold_max(case.phi0[1:-1, 1:-1], nxt[1:-1, 1:-1])
    out = torch.full(case.shape, NAN, dtype=torch.float32, device=DEV)
    resid = torch.zeros(1, dtype=torch.float32, device=DEV)
    S.sweep_range(dev(case.phi0), out, dev(case.div), dev(case.mask.astype(np.uint8)), 1, case.shape[0] - 1, case.dx,
                  case.dt, resid=resid)
    agree(host(resid), np.array([want], F), cls)
