"""The multi-rank slab drivers off their usual road, against the oracle.

cfd_slab_jacobi3d_f32, cfd_slab_jacobi3d_zero_f32 and cfd_slab_rbgs3d_f32 run
through SlabJacobi3D / SlabRBGS3D on an in-process group (LocalComm.group(R):
one host thread and one stream per rank, device copies for the send/recv
pairs) on the cases of tests/slab_edge_reference.py: with a solid mask, with
rows no float4 covers, with fewer sweeps per pass than ghost planes, on the
thinnest slabs a plan allows, at the overlap threshold, from a guess whose
ghosts the driver must fetch, and with arguments it must refuse.  Every solve
is compared with the single-domain oracle under ``np.array_equal``, GS solves
also in the iteration count of every rank; tests/test_slab_edge_host.py shows
the same cases decomposable on the CPU.

phi_tmp, the RHS workspace and the ghost planes of phi are handed over as NaN
wherever the drivers' contract says they are not read (a zero start reads
nothing of phi; a start from a guess fetches its ghosts; ghost planes beyond
the domain are never read), so a stale read shows.

The tuning knobs and cfd_get_last_tbr_shape are per host thread: each rank's
thread sets its own knobs and reports the levels of its last tall-tile launch
(0: none), which the tests compare with the drivers' dispatch rules restated
here (``jacobi_levels``, ``gs_levels``).
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import slab_edge_reference as E
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd import slab as S
from cfd_simulations_amd._lib import CfdError, call, lib, ptr, stream_handle
from slab_edge_reference import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
NAN = float("nan")
overlaps = pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # (a copy: the shared inputs are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def last_shape():
    v = [ctypes.c_int() for _ in range(4)]
    call("cfd_get_last_tbr_shape", *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


@pytest.fixture(autouse=True)
def cfd_reset_tuning():
    call("cfd_reset_tuning")
    yield
    call("cfd_reset_tuning")
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device error ends the run: nothing more is started on that device
        pytest.exit(f"device error after a slab edge test: {e}", returncode=3)


def run_group(R, make, run, tune=None):
    """tests/test_gpu_parity.py's _run_local_group: R ranks of an in-process
    slab group, one host thread and one stream per rank, running the real
    drivers.  ``tune`` sets the (per-thread) knobs inside every rank's thread.
    Returns the solvers and each rank's cfd_get_last_tbr_shape levels."""
    comms = S.LocalComm.group(R)
    solvers = [make(r, comms[r]) for r in range(R)]
    streams = [torch.cuda.Stream() for _ in range(R)]
    torch.cuda.synchronize()
    errs, levels = [None] * R, [None] * R

    def work(r):
        try:
            call("cfd_reset_tuning")
            if tune is not None:
                tune()
            with torch.cuda.stream(streams[r]):
                run(solvers[r])
            streams[r].synchronize()
            levels[r] = last_shape()[0]
            call("cfd_reset_tuning")
        except Exception as e:  # noqa: BLE001 -- reported below
            errs[r] = e

    threads = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)     # (a rank that waits for a failed one gives up after 120 s: slab.hip, LocalGroup)
    if any(t.is_alive() for t in threads):
        pytest.exit("a rank hung: nothing more is launched", returncode=3)
    torch.cuda.synchronize()
    for c in comms:
        c.close()
    assert errs == [None] * R, errs
    return solvers, levels


def describe(got, ref):
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    if not len(bad):
        return "equal"
    z, y, x = bad[0]
    return (f"{len(bad)} of {ref.size} cells differ, planes {sorted(set(bad[:, 0].tolist()))}; "
            f"first (z, y, x) = {(z, y, x)}: got {got[z, y, x]!r}, reference {ref[z, y, x]!r}")


@functools.lru_cache(maxsize=None)
def reference(name, tol=0.0):
    ref = E.reference(CASES[name], tol)
    (ref if CASES[name].op == "jacobi" else ref[0]).setflags(write=False)
    return ref


def nonempty(case):
    return [p.z_update_end > p.z_update_begin for p in case.plans()]


# ================================================================ Jacobi
def jacobi_levels(case, rhs, steps=0, prefetch=1):
    """Levels of the solve's last tall-tile launch (0: none), by the rules of
    slab_jacobi3d and jacobi3d_schedule: blocked passes need ghost >= 2,
    blocking on, no mask and rows of float4; K = min(depth, ghost); with the
    workspace (and one plane of prefetch, two sweeps or more) the first pass
    is the fused one and takes the remainder, else the remainder comes last."""
    G, it = case.ghost, case.iters
    tb = G >= 2 and steps != 1 and not case.masked and case.nx % 4 == 0 and case.ny >= 3
    Kp = min(steps if steps >= 2 else 4, G) if tb else 1
    first = rhs and Kp >= 2 and prefetch == 1 and it >= 2
    r = it % Kp
    k1 = min(it, Kp if not first else r if r in (2, 3) else Kp if r == 0 else min(Kp, 3))
    depths, done = [], 0
    while done < it:
        k = k1 if done == 0 else min(Kp, it - done)
        depths.append(k)
        done += k
    tall = [k for k in depths if k >= 2]
    return tall[-1] if tall else 0


def solve_jacobi(name, overlap, rhs=True, steps=0, prefetch=1):
    """One group solve of a Jacobi case against the oracle; every rank's last
    tall-tile levels against ``jacobi_levels`` (a rank with an empty update
    range launches nothing)."""
    case = CASES[name]
    div, phi0, mask = E.make_case(case)
    zero = case.start == "zero"

    def make(r, comm):
        plan = S.SlabPlan(case.nz, case.R, r, ghost=case.ghost)
        m = dev(plan.scatter(mask.astype(np.uint8))) if case.masked else None
        sj = S.SlabJacobi3D(plan, case.ny, case.nx, E.H, E.JDT, comm, mask=m, rhs_workspace=rhs)
        sj.div.copy_(dev(plan.scatter(div)))
        for t in (sj.phi, sj.tmp) + ((sj.rhs,) if rhs else ()):
            t.fill_(NAN)
        if not zero:
            sj.phi[plan.owned()].copy_(dev(phi0[plan.z_lo:plan.z_hi]))   # ghosts left NaN: the driver fetches them
        return sj

    def tune():
        call("cfd_set_jacobi3d_blocking", steps, 0, 0)
        call("cfd_set_jacobi3d_prefetch", prefetch)

    sols, levels = run_group(case.R, make, lambda sj: sj.solve(case.iters, overlap=overlap, zero_phi=zero), tune)
    got = np.concatenate([host(sj.owned()) for sj in sols])
    what = (name, overlap, rhs, steps, prefetch)
    assert np.array_equal(got, reference(name)), (what, describe(got, reference(name)))
    want = jacobi_levels(case, rhs, steps, prefetch)
    assert levels == [want if some else 0 for some in nonempty(case)], (what, levels, want)
    return levels


@overlaps
@pytest.mark.parametrize("name", E.group("jmask") + E.group("jmask-planes"))
def test_jacobi_masked(name, overlap):
    """A mask turns blocking off at every ghost depth (nx = 12: the mask alone
    does): single sweeps with G-deep ghosts, the masked cells of the owned
    faces and Dirichlet planes zeroed by the driver in both buffers.  With and
    without the RHS workspace.  The (3, 3) and (2, 2) grids have ranks that
    update nothing: only that zeroing, and the exchange, happen there."""
    for rhs in (True, False):
        assert set(solve_jacobi(name, overlap, rhs)) == {0}


@overlaps
@pytest.mark.parametrize("name", E.group("jragged"))
def test_jacobi_ragged_rows(name, overlap):
    """nx = 5, 10, 13 with ghost 2..4 and no mask: the unblocked solve with
    deep ghosts.  From zeros with the workspace this is also the zero entry
    without a fused first pass (a zero fill, then the general solve)."""
    assert set(solve_jacobi(name, overlap)) == {0}


@overlaps
@pytest.mark.parametrize("name", E.group("jthin"))
def test_jacobi_thin_slabs(name, overlap):
    """Slabs of ``ghost`` planes (every owned plane a neighbour's ghost) and
    one more; sweeps below the pass depth and every remainder.  No slab here
    has the 2 G + 1 updated planes an overlap needs: a request is declined."""
    case = CASES[name]
    assert all(p.z_update_end - p.z_update_begin < 2 * case.ghost + 1 for p in case.plans())
    solve_jacobi(name, overlap)


@overlaps
@pytest.mark.parametrize("name", E.group("jthreshold"))
def test_jacobi_overlap_threshold(name, overlap):
    """Three ranks; the middle one, with two neighbours, updates 2 G planes
    (nz = 12, 24: overlap declined, slab_can_overlap) or 2 G + 1 (15, 27: taken,
    an interior of one plane), its neighbours one plane fewer."""
    solve_jacobi(name, overlap)


@overlaps
@pytest.mark.parametrize("steps,prefetch", [(1, 1), (2, 1), (3, 1), (0, 2)], ids=["off", "k2", "k3", "prefetch2"])
@pytest.mark.parametrize("name", E.group("jdepth"))
def test_jacobi_depth_below_ghost(name, steps, prefetch, overlap):
    """Ghost 4 with blocking off or 2 or 3 sweeps per pass (K < G), and two
    planes of prefetch: the workspace is given but no pass is the fused
    first one."""
    levels = solve_jacobi(name, overlap, True, steps, prefetch)
    assert max(levels) in {1: (0,), 2: (2,), 3: (2, 3), 0: (4,)}[steps]


def pick(group, **fields):
    """The first zero-start case of a group with these fields."""
    return next(n for n in E.group(group) if CASES[n].start == "zero" and
                all(getattr(CASES[n], k) == v for k, v in fields.items()))


# blocked (thin, thick, at the overlap threshold) and unblocked
ZERO_NO_WORKSPACE = [pick("jthin", nz=8, iters=5), pick("jthin", nz=6, iters=5), pick("jthreshold", nz=15),
                     pick("jthreshold", nz=27), pick("jragged", ghost=2), pick("jragged", ghost=4),
                     pick("jdepth", nz=20)]


@overlaps
@pytest.mark.parametrize("name", ZERO_NO_WORKSPACE)
def test_jacobi_zero_start_without_workspace(name, overlap):
    """cfd_slab_jacobi3d_zero_f32 with no RHS workspace: phi (NaN here) is
    zero-filled, then the general solve runs."""
    solve_jacobi(name, overlap, rhs=False)


@pytest.mark.parametrize("zero", [True, False], ids=["zero", "guess"])
def test_jacobi_no_sweeps(zero):
    """iters = 0: the zero entry leaves all of phi zero, ghosts included; the
    general entry leaves phi untouched."""
    case = CASES[E.group("jnone")[0]]
    _, phi0, _ = E.make_case(case)
    before = {}

    def make(r, comm):
        plan = S.SlabPlan(case.nz, case.R, r, ghost=case.ghost)
        sj = S.SlabJacobi3D(plan, case.ny, case.nx, E.H, E.JDT, comm)
        for t in (sj.phi, sj.tmp, sj.rhs):
            t.fill_(NAN)
        sj.phi[plan.owned()].copy_(dev(phi0[plan.z_lo:plan.z_hi]))
        before[r] = host(sj.phi).view(np.uint32).copy()
        return sj

    sols, _ = run_group(case.R, make, lambda sj: sj.solve(0, overlap=True, zero_phi=zero))
    for r, sj in enumerate(sols):
        got = host(sj.phi).view(np.uint32)
        assert np.array_equal(got, np.zeros_like(got) if zero else before[r]), r


# ================================================================ red-black GS
def gs_levels(case):
    """Levels a fused slab GS solve's tall-tile launches may have (empty: in
    place, none): fused needs ghost >= 2, blocking on, no mask and rows of
    float4; passes of 4 half-sweeps with ghost 4 and depth 4 or auto, else of
    2; remainders and the rollback of a stop inside a pair pass take 2."""
    fused = case.ghost >= 2 and case.steps != 1 and not case.masked and case.nx % 4 == 0 and case.ny >= 3
    if not fused:
        return ()
    return (4, 2) if case.ghost >= 4 and case.steps in (0, 4) else (2,)


def solve_rbgs(name, overlap, tol, want):
    case = CASES[name]
    div, phi0, mask = E.make_case(case)
    zero = case.start == "zero"
    ref, n_ref = reference(name, tol)
    assert n_ref == want, (name, tol, n_ref, want)

    def make(r, comm):
        plan = S.SlabPlan(case.nz, case.R, r, ghost=case.ghost)
        m = dev(plan.scatter(mask.astype(np.uint8))) if case.masked else None
        sg = S.SlabRBGS3D(plan, case.ny, case.nx, case.dx, case.dy, case.dz, E.GDT, comm, mask=m)
        sg.div.copy_(dev(plan.scatter(div)))
        sg.phi.fill_(NAN)
        sg.tmp.fill_(NAN)
        sg.iters_done.fill_(-7)
        if not zero:
            sg.phi[plan.owned()].copy_(dev(phi0[plan.z_lo:plan.z_hi]))   # ghosts left NaN: the driver fetches them
        return sg

    sols, levels = run_group(case.R, make,
                             lambda sg: sg.solve(case.iters, tolerance=tol, overlap=overlap, zero_phi=zero),
                             lambda: call("cfd_set_jacobi3d_blocking", case.steps, 0, 0))
    what = (name, overlap, tol)
    assert [int(host(sg.iters_done)[0]) for sg in sols] == [n_ref] * case.R, what
    got = np.concatenate([host(sg.owned()) for sg in sols])
    assert np.array_equal(got, ref), (what, describe(got, ref))
    may = gs_levels(case)
    assert all((lv in may) if some and may else lv == 0 for lv, some in zip(levels, nonempty(case))), \
        (what, levels, may)
    return sols


def sweep_rbgs(name, overlap):
    """tol = 0 (every iteration), then a stop at an odd and at an even count."""
    case = CASES[name]
    assert sorted(n % 2 for _, n in case.tols) == [0, 1]
    for tol, want in ((0.0, case.iters),) + case.tols:
        assert tol == 0.0 or 1 < want < case.iters
        solve_rbgs(name, overlap, tol, want)


@overlaps
@pytest.mark.parametrize("name", E.group("gmask"))
def test_rbgs_masked(name, overlap):
    """A mask selects the in-place colour passes at every ghost depth, with a
    G-plane exchange after each colour and the global maximum per iteration."""
    assert gs_levels(CASES[name]) == ()
    sweep_rbgs(name, overlap)


@overlaps
@pytest.mark.parametrize("name", E.group("gragged"))
def test_rbgs_ragged_rows(name, overlap):
    """No mask, deep ghosts, nx % 4 != 0: in place as well."""
    assert gs_levels(CASES[name]) == ()
    sweep_rbgs(name, overlap)


@overlaps
@pytest.mark.parametrize("name", E.group("gthin"))
def test_rbgs_thin_fused(name, overlap):
    """Fused passes on slabs of ``ghost`` planes, one and two iterations per
    pass; a stop at an odd count falls inside a pair pass and is rolled back."""
    assert gs_levels(CASES[name])
    sweep_rbgs(name, overlap)


@overlaps
@pytest.mark.parametrize("name", E.group("gguess"))
def test_rbgs_from_a_guess(name, overlap):
    """Owned planes from the guess, ghosts NaN: the driver fetches the ghosts
    of the guess before the first pass (in place, fused, pair passes, masked)."""
    sweep_rbgs(name, overlap)


@pytest.mark.parametrize("tol", [0.0, 1e-6])
@pytest.mark.parametrize("name", E.group("gflat"))
def test_rbgs_two_rows(name, tol):
    """ny = 2: no cell to update.  phi is unchanged on every rank and the
    count is the single-GPU solve's for the same grid."""
    case = CASES[name]
    div, phi0, _ = E.make_case(case)
    single = dev(phi0)
    done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    K.solve_pressure_gauss_seidel3d(single, dev(div), case.dx, case.dy, case.dz, E.GDT, None, case.iters, tol,
                                    iters_done=done)
    n_single = int(host(done)[0])
    # (the library counts every iteration of a grid without interior; the oracle, whose max|change| is then
    #  0, stops a positive tolerance after one.  No cell changes either way.)
    assert n_single == case.iters and np.array_equal(host(single), phi0)
    assert np.array_equal(reference(name, tol)[0], phi0)
    before = {}

    def make(r, comm):
        plan = S.SlabPlan(case.nz, case.R, r, ghost=case.ghost)
        sg = S.SlabRBGS3D(plan, case.ny, case.nx, case.dx, case.dy, case.dz, E.GDT, comm)
        sg.div.copy_(dev(plan.scatter(div)))
        sg.phi.fill_(NAN)
        sg.tmp.fill_(NAN)
        sg.iters_done.fill_(-7)
        sg.phi[plan.owned()].copy_(dev(phi0[plan.z_lo:plan.z_hi]))
        before[r] = host(sg.phi).view(np.uint32).copy()
        return sg

    sols, _ = run_group(case.R, make, lambda sg: sg.solve(case.iters, tolerance=tol, overlap=True, zero_phi=False))
    assert [int(host(sg.iters_done)[0]) for sg in sols] == [n_single] * case.R
    for r, sg in enumerate(sols):
        assert np.array_equal(host(sg.phi).view(np.uint32), before[r]), r


# ================================================================ argument checks
GOOD = dict(nz_local=9, ghost=2, ny=9, nx=12, lo=-1, hi=-1, zb=3, ze=10)
BAD = {"ghost-0": (dict(ghost=0), "ghost depth"), "ghost-5": (dict(ghost=5), "ghost depth"),
       "slab-thinner-than-ghost": (dict(nz_local=1, zb=2, ze=3), "bad shape"),
       "begin-in-the-ghosts": (dict(zb=1), "outside owned planes"),
       "end-in-the-ghosts": (dict(ze=12), "outside owned planes"),
       "begin-past-end": (dict(zb=6, ze=5), "outside owned planes"),
       "lo-peer": (dict(lo=1), "bad peer"), "hi-peer": (dict(hi=1), "bad peer")}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_slab_entries_refuse_bad_arguments(bad):
    """slab_check_args, on a one-rank group (no barrier): each entry raises
    the library's error and leaves a NaN-filled phi and phi_tmp untouched."""
    a = dict(GOOD, **BAD[bad][0])
    comm = S.LocalComm.group(1)[0]
    shape = (GOOD["nz_local"] + 2 * GOOD["ghost"], GOOD["ny"], GOOD["nx"])
    div = torch.zeros(shape, dtype=torch.float32, device=DEV)
    phi, tmp, rhs = (torch.full(shape, NAN, dtype=torch.float32, device=DEV) for _ in range(3))
    ws = torch.empty(int(lib().cfd_rbgs_workspace_bytes(3)), dtype=torch.uint8, device=DEV)
    done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    before = host(phi).view(np.uint32).copy()
    layout = (a["nz_local"], a["ghost"], a["ny"], a["nx"], a["lo"], a["hi"], a["zb"], a["ze"])
    entries = {
        "cfd_slab_jacobi3d_f32": (comm.handle, ptr(div), ptr(phi), ptr(tmp), ptr(rhs), None) + layout +
                                 (E.H, float(E.JDT), 3, 0, stream_handle(), None),
        "cfd_slab_jacobi3d_zero_f32": (comm.handle, ptr(div), ptr(phi), ptr(tmp), ptr(rhs)) + layout +
                                      (E.H, float(E.JDT), 3, 0, stream_handle(), None),
        "cfd_slab_rbgs3d_f32": (comm.handle, ptr(div), ptr(phi), ptr(tmp), None) + layout +
                               (0, E.GDX, E.GDY, E.GDZ, float(E.GDT), 3, 0.0, ptr(ws), ptr(done), 0,
                                stream_handle(), None),
    }
    try:
        for name, args in entries.items():
            with pytest.raises(CfdError, match=BAD[bad][1]):
                call(name, *args)
            for t in (phi, tmp):
                assert np.array_equal(host(t).view(np.uint32), before), name
            assert int(host(done)[0]) == -7
    finally:
        comm.close()
