"""The flow statistics and the 3-D snapshots on the GPU: cfd_flow_stats3d_f32
against tests/stats3d_reference.py (bit for bit where every operation is
exact, within stats_bound where only the order of the sums differs), its
determinism and its footprint, the solvers' statistics beside their NumPy
references, and restarts that continue the uninterrupted run bit for bit."""
import functools
import zipfile

import numpy as np
import pytest
import torch

from cfd_simulations_amd import kernels as K
from cfd_simulations_amd.solver import (CylinderChannel3DConfig, CylinderChannel3DSolver, LesCavity3DConfig,
                                        LidDrivenCavity3DSolver)
from cyl3d_reference import Cylinder3DReference, force_bound
from les3d_reference import Cavity3DLesReference
from zper_reference import PeriodicCylinder3DReference
from stats3d_reference import abs_terms, accumulate_numpy, derive, stats_bound

pytestmark = pytest.mark.gpu

F = np.float32
# the z-sum is split over 8 waves in chunks of ceil(nz / 8) planes, marched two
# planes at a time: (9, 5, 65) gives chunks of 2 with a last one of 1 (the odd
# tail) and three empty waves (and an odd cell count: one cell per thread in
# full mode), (45, 3, 70) chunks of 6 with 3 planes for the last wave
SHAPES = [(1, 3, 7), (5, 4, 65), (12, 53, 264), (67, 5, 130), (130, 3, 257), (9, 5, 65), (45, 3, 70)]
ORDERED = [(12, 53, 264), (67, 5, 130)]
FIELDS = ("u", "v", "w", "phi")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")  # a writable copy


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def acc_shape(shape, nm, span):
    return (nm,) + (shape[1:] if span else shape)


@functools.lru_cache(maxsize=None)
def int_samples(shape):
    """Three samples of u, v, w, nu_t: integers in [-4, 4] as float32 (read-only)."""
    rng = np.random.default_rng(sum(shape))
    out = [tuple(rng.integers(-4, 5, shape).astype(F) for _ in range(4)) for _ in range(3)]
    for s in out:
        for a in s:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normal_samples(shape):
    """Two samples of u, v, w, nu_t: 5 N(0, 1), the max_velocity scale (read-only)."""
    rng = np.random.default_rng(7 + sum(shape))
    out = [tuple((5 * rng.standard_normal(shape)).astype(F) for _ in range(4)) for _ in range(2)]
    for s in out:
        for a in s:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ordered_reference(shape, span, with_nut):
    """(sums, abs sums) of the two-sample sequence in NumPy (read-only)."""
    nm = 10 if with_nut else 9
    ref, ab = np.zeros(acc_shape(shape, nm, span)), np.zeros(acc_shape(shape, nm, span))
    for (u, v, w, nt), wgt in zip(normal_samples(shape), (2e-5, 7.3e-5)):
        accumulate_numpy(ref, u, v, w, wgt, span, nt if with_nut else None)
        abs_terms(ab, u, v, w, wgt, span, nt if with_nut else None)
    ref.setflags(write=False)
    ab.setflags(write=False)
    return ref, ab


def run_gpu(samples, weights, shape, span, with_nut):
    nm = 10 if with_nut else 9
    acc = torch.zeros(acc_shape(shape, nm, span), dtype=torch.float64, device="cuda")
    for (u, v, w, nt), wgt in zip(samples, weights):
        K.accumulate_flow_stats3d(dev(u), dev(v), dev(w), acc, wgt, span, nu_t=dev(nt) if with_nut else None)
    return host(acc)


@pytest.mark.parametrize("with_nut", [False, True], ids=["9", "10"])
@pytest.mark.parametrize("span", [True, False], ids=["span", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_sums_equal_the_reference(shape, span, with_nut):
    """Small integers and weights 1, 1/2, 1/4: every term, z-sum and weighted
    add is an exact float64 (magnitudes <= 16 * 130 * 3), so any order of the
    sums gives the reference's bits."""
    weights = (1.0, 0.5, 0.25)
    nm = 10 if with_nut else 9
    ref = np.zeros(acc_shape(shape, nm, span))
    for (u, v, w, nt), wgt in zip(int_samples(shape), weights):
        accumulate_numpy(ref, u, v, w, wgt, span, nt if with_nut else None)
    got = run_gpu(int_samples(shape), weights, shape, span, with_nut)
    assert ref.any() and np.array_equal(got, ref)


@pytest.mark.parametrize("with_nut", [False, True], ids=["9", "10"])
@pytest.mark.parametrize("span", [True, False], ids=["span", "full"])
@pytest.mark.parametrize("shape", ORDERED, ids=str)
def test_ordered_sums_within_the_bound_and_deterministic(shape, span, with_nut):
    ref, ab = ordered_reference(shape, span, with_nut)
    weights = (2e-5, 7.3e-5)
    got = run_gpu(normal_samples(shape), weights, shape, span, with_nut)
    bound = stats_bound(2 * shape[0] if span else 2, 2, ab)
    err = np.abs(got - ref)
    print(shape, "span" if span else "full", "max err / bound", (err / bound).max(), "max err", err.max())
    assert (err <= bound).all()
    # the same sequence again into a zeroed accumulator: the same bits
    assert np.array_equal(run_gpu(normal_samples(shape), weights, shape, span, with_nut), got)


@pytest.mark.parametrize("span", [True, False], ids=["span", "full"])
@pytest.mark.parametrize("shape", [(5, 4, 65), (9, 5, 65), (12, 53, 264)], ids=str)
def test_accumulator_untouched_elsewhere(shape, span):
    """One NaN-filled moment plane in front of acc and one behind it stay NaN."""
    for with_nut in (False, True):
        nm = 10 if with_nut else 9
        buf = torch.full(acc_shape(shape, nm + 2, span), float("nan"), dtype=torch.float64, device="cuda")
        acc = buf[1:nm + 1]
        acc.zero_()
        u, v, w, nt = int_samples(shape)[0]
        K.accumulate_flow_stats3d(dev(u), dev(v), dev(w), acc, 0.5, span, nu_t=dev(nt) if with_nut else None)
        out = host(buf)
        assert np.isnan(out[0]).all() and np.isnan(out[-1]).all()
        ref = accumulate_numpy(np.zeros(acc_shape(shape, nm, span)), u, v, w, 0.5, span, nt if with_nut else None)
        assert np.array_equal(out[1:-1], ref)


@pytest.mark.parametrize("odd", ["acc", "u", "w", "nu_t"])
def test_full_mode_with_an_even_cell_count_and_one_unaligned_array(odd):
    """Full mode takes two cells per thread only where n is even and the
    fields are 8-byte and acc 16-byte aligned.  Here n = 1300 is even and one
    array starts one element into a flat buffer (acc at 8 mod 16 bytes, a field
    at 4 mod 8): the one-cell kernel must be chosen by the alignment alone.
    The element in front of that array and the one behind it stay NaN."""
    shape = (5, 4, 65)
    n = shape[0] * shape[1] * shape[2]
    with_nut = odd == "nu_t"
    nm = 10 if with_nut else 9
    u, v, w, nt = int_samples(shape)[1]
    t = {"u": dev(u), "v": dev(v), "w": dev(w), "nu_t": dev(nt) if with_nut else None}
    flat = torch.full((nm * n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    if odd == "acc":
        acc = flat[1:-1].view((nm,) + shape)
        assert acc.data_ptr() % 16 == 8
    else:
        acc = flat[2:].view((nm,) + shape)
        assert acc.data_ptr() % 16 == 0
        pad = torch.full((n + 2,), float("nan"), device="cuda")
        pad[1:-1].copy_(t[odd].reshape(-1))
        t[odd] = pad[1:-1].view(shape)
        assert t[odd].data_ptr() % 8 == 4 and t[odd].is_contiguous()
    acc.zero_()
    for wgt in (1.0, 0.25):
        K.accumulate_flow_stats3d(t["u"], t["v"], t["w"], acc, wgt, False, nu_t=t["nu_t"])
    ref = np.zeros((nm,) + shape)
    for wgt in (1.0, 0.25):
        accumulate_numpy(ref, u, v, w, wgt, False, nt if with_nut else None)
    assert np.array_equal(host(acc), ref)
    out = host(flat)
    assert np.isnan(out[0]) and (np.isnan(out[-1]) if odd == "acc" else np.isnan(out[1]))


def test_wrapper_refusals_and_nan():
    shape = (4, 5, 6)
    t = [torch.zeros(shape, device="cuda") for _ in range(4)]
    acc = torch.zeros((9, 5, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="acc"):
        K.accumulate_flow_stats3d(*t[:3], acc, 1.0, False)
    with pytest.raises(ValueError, match="acc"):
        K.accumulate_flow_stats3d(*t[:3], acc, 1.0, True, nu_t=t[3])
    with pytest.raises(ValueError, match="acc"):
        K.accumulate_flow_stats3d(*t[:3], acc.float(), 1.0, True)
    with pytest.raises(TypeError):
        K.accumulate_flow_stats3d(t[0].double(), *t[1:3], acc, 1.0, True)
    with pytest.raises(ValueError):
        K.accumulate_flow_stats3d(t[0], t[1], t[2][:, :, :5], acc, 1.0, True)
    # every cell counts and a NaN propagates into its column, and only there
    t[0][2, 3, 4] = float("nan")
    out = host(K.accumulate_flow_stats3d(*t[:3], acc, 1.0, True))
    bad = np.isnan(out)
    assert bad[[0, 3, 6, 7], 3, 4].all() and bad.sum() == 4


# ------------------------------------------------------------------ solvers
# CylinderChannel3DConfig(**STEP_CASES["rbgs-les"]) of tests/test_gpu_cyl3d.py
CYL_LES = dict(nz=10, ny=24, nx=40, z_max=1.0, y_max=23 / 8, x_max=39 / 8, cylinder_center=(1.5, 23 / 16),
               initial_steps=2, pressure_iterations=30, log_diagnostics=True, use_les=True)
# the whole-step case of tests/test_gpu_zper.py
CYL_PER = dict(nz=10, ny=24, nx=40, z_max=1.0, y_max=3.0, x_max=39 / 8, cylinder_center=(1.5, 1.5), initial_steps=2,
               pressure_iterations=30, pressure_tolerance=0.0, log_diagnostics=True, spanwise_bc="periodic",
               spanwise_perturbation=0.05)
CAVITY = dict(nz=12, ny=12, nx=12, pressure_iterations=40)


def step_both(g, o, k, names):
    dg, do = g.time_step(), o.time_step()
    assert dg == do, k
    for f in names:
        assert np.array_equal(host(getattr(g, f)), getattr(o, f)), (f, k)
    return dg


def check_solver_statistics(g, o, span, mode, names):
    """Five steps with statistics from step 1 on every second step, beside
    the reference ``o`` with accumulate_numpy on its fields."""
    c = g.config
    nm = 10
    shape = (c.nz, c.ny, c.nx)
    ref, ab = np.zeros(acc_shape(shape, nm, span)), np.zeros(acc_shape(shape, nm, span))
    with pytest.raises(RuntimeError):
        g.statistics()
    total, before = np.float64(0.0), host(g._stats_sums).copy()
    assert not before.any()
    for k in range(5):
        dt = step_both(g, o, k, names)
        now = host(g._stats_sums).copy()
        if k in (1, 3):   # the sample steps, exactly
            wgt = float(dt) if mode == "dt" else 1.0
            accumulate_numpy(ref, o.u, o.v, o.w, wgt, span, o.nu_t)
            abs_terms(ab, o.u, o.v, o.w, wgt, span, o.nu_t)
            total = total + np.float64(wgt)
            assert not np.array_equal(now, before), k
        else:
            assert np.array_equal(now, before), k
            if k == 0:
                with pytest.raises(RuntimeError):
                    g.statistics()
        before = now
    bound = stats_bound(2 * c.nz if span else 2, 2, ab)
    err = np.abs(before - ref)
    print("solver sums: max err", err.max(), "max err / bound", np.nanmax(err / np.where(bound > 0, bound, np.nan)))
    assert ref[:3].any() and ref[9].any() and (err <= bound).all()
    s = g.statistics()
    assert s["samples"] == 2 and s["weight"] == total and type(s["weight"]) is float
    want = derive(before, total, c.nz, span)
    assert set(s) == set(want) | {"samples"} and "mean_nu_t" in s
    for key, val in want.items():
        assert np.array_equal(s[key], val, equal_nan=True), key
        if key != "weight":
            assert s[key].dtype == np.float64 and s[key].shape == (shape[1:] if span else shape), key


def test_cylinder_statistics_beside_the_reference():
    c = CylinderChannel3DConfig(**CYL_LES)
    g, o = CylinderChannel3DSolver(c), Cylinder3DReference(c)
    g.enable_statistics(start_step=1, interval=2)   # the cylinder's default: the span average, dt weights
    assert g._stats == (1, 2, True, "dt") and g._stats_sums.shape == (10, c.ny, c.nx)
    check_solver_statistics(g, o, True, "dt", FIELDS + ("nu_t",))


def test_cavity_statistics_beside_the_reference():
    c = LesCavity3DConfig(**CAVITY)
    g, o = LidDrivenCavity3DSolver(c), Cavity3DLesReference(c)
    g.enable_statistics(start_step=1, interval=2, weight="sample")   # the cavity's default: per cell
    assert g._stats == (1, 2, False, "sample") and g._stats_sums.shape == (10, c.nz, c.ny, c.nx)
    check_solver_statistics(g, o, False, "sample", FIELDS + ("nu_t",))


def test_statistics_off_changes_nothing():
    c = CylinderChannel3DConfig(**CYL_LES)
    g, o = CylinderChannel3DSolver(c), Cylinder3DReference(c)
    for k in range(5):
        step_both(g, o, k, FIELDS + ("nu_t", "u_star", "v_star", "w_star", "div_u_star"))
    assert g._stats is None and not hasattr(g, "_stats_sums")
    with pytest.raises(RuntimeError):
        g.statistics()
    with pytest.raises(RuntimeError):
        g.reset_statistics()


def test_enable_and_reset_statistics():
    g = LidDrivenCavity3DSolver(LesCavity3DConfig(**CAVITY))
    g.enable_statistics()
    assert g._stats == (0, 1, False, "dt")
    sums = g._stats_sums
    g.enable_statistics(0, 1, False, "dt")   # the same settings: nothing happens
    assert g._stats_sums is sums
    with pytest.raises(ValueError, match="reset_statistics"):
        g.enable_statistics(interval=2)
    with pytest.raises(ValueError):
        g.enable_statistics(weight="volume")
    dts = [g.time_step() for _ in range(2)]
    s = g.statistics()
    assert s["samples"] == 2 and s["weight"] == float(np.float64(float(dts[0])) + np.float64(float(dts[1])))
    assert s["mean_u"].shape == (12, 12, 12) and s["mean_u"].any()
    with pytest.raises(ValueError, match="reset_statistics"):
        g.enable_statistics(span_average=True)
    g.reset_statistics()
    assert g._stats == (0, 1, False, "dt") and not host(g._stats_sums).any()
    with pytest.raises(RuntimeError):
        g.statistics()
    g.enable_statistics(span_average=True, weight="sample")   # allowed after the reset
    assert g._stats_sums.shape == (10, 12, 12)
    g.time_step()
    s = g.statistics()
    assert s["samples"] == 1 and s["weight"] == 1.0 and s["tke"].shape == (12, 12)


# ------------------------------------------------------------------ restart
def make_restart_case(case):
    if case == "cylinder-les-1000":
        return (lambda **kw: CylinderChannel3DSolver(CylinderChannel3DConfig(**dict(CYL_LES, **kw))), 1000,
                dict(start_step=1001, interval=2), dict(nz=12), Cylinder3DReference)
    if case == "cylinder-periodic":
        return (lambda **kw: CylinderChannel3DSolver(CylinderChannel3DConfig(**dict(CYL_PER, **kw))), 0,
                dict(), dict(nz=12), PeriodicCylinder3DReference)
    return (lambda **kw: LidDrivenCavity3DSolver(LesCavity3DConfig(**dict(CAVITY, **kw))), 0,
            dict(interval=2, span_average=True, weight="sample"), dict(nx=13), None)


@pytest.mark.parametrize("case", ["cylinder-les-1000", "cylinder-periodic", "cavity"])
def test_restart_continues_bit_for_bit(case, tmp_path):
    make, first, stats, other, ref_cls = make_restart_case(case)
    path = str(tmp_path / "run.npz")
    a = make()
    a.enable_statistics(**stats)
    if first:
        a.time_step()          # a nu_t for the adaptive dt's mean
        a.step = first
    for _ in range(3):
        a.time_step()
    a.save_snapshot(path, a.step, 0.125)
    with zipfile.ZipFile(path) as z:
        members = z.namelist()
    g = f"step_{a.step:06d}"
    names = {"u", "v", "w", "phi", "vorticity", "x", "y", "z", "time", "solver_step", "stats_sums", "stats_weight",
             "stats_samples", "stats_start_step", "stats_interval", "stats_span_average", "stats_weight_mode"}
    names |= {"nu_t"} if a.use_les else set()
    assert sorted(members) == sorted(f"{g}/{n}.npy" for n in names)
    with np.load(path) as f:
        assert np.array_equal(f[f"{g}/vorticity"], host(a.compute_vorticity()), equal_nan=True)
        assert f[f"{g}/z"].shape == (a.config.nz,) and int(f[f"{g}/solver_step"]) == a.step
        assert np.array_equal(f[f"{g}/stats_sums"], host(a._stats_sums)) and f[f"{g}/stats_sums"].any()
    saved_step = a.step
    saved = {n: host(getattr(a, n)).copy() for n in ("u", "v", "w") + (("nu_t",) if a.use_les else ())}
    dts_a = [a.time_step() for _ in range(2)]

    b = make()
    if case == "cylinder-periodic":
        b.enable_statistics(**stats)   # already on with the file's settings; the others: enabled by the load
    assert b.load_snapshot(path) == 0.125
    assert b.step == saved_step and b._stats == a._stats and b.energy_history == []
    dts_b = [b.time_step() for _ in range(2)]
    assert dts_a == dts_b and all(type(x) is type(y) for x, y in zip(dts_a, dts_b))
    if first:
        assert dts_a[0] != np.float32(0.00002)   # the adaptive branch ran
    for name in FIELDS + (("nu_t",) if a.use_les else ()):
        fa, fb = host(getattr(a, name)), host(getattr(b, name))
        assert fa.any() and np.array_equal(fa, fb), name
    assert np.array_equal(host(a._stats_sums), host(b._stats_sums))
    assert a._stats_weight == b._stats_weight and a._stats_samples == b._stats_samples > 0
    sa, sb = a.statistics(), b.statistics()
    assert all(np.array_equal(sa[k], sb[k], equal_nan=True) for k in sa)
    assert b.step == a.step == saved_step + 2 and [s for s, _ in b.energy_history] == [saved_step, saved_step + 1]

    # the same step again: the file keeps its member list; a later step is appended
    a.save_snapshot(path, saved_step, 9.0)
    with zipfile.ZipFile(path) as z:
        assert z.namelist() == members
    a.save_snapshot(path, a.step, 0.25)
    with zipfile.ZipFile(path) as z:
        assert z.namelist()[:len(members)] == members and len(z.namelist()) == 2 * len(members)
    # a load into a solver that has stepped: its histories start empty again, the force rows at zero
    assert b.load_snapshot(path, step=saved_step) == 0.125 and b.step == saved_step
    assert b.energy_history == [] and b.times == []
    if ref_cls is not None:
        assert b.force_history == [] and b._dts == [] and not host(b._force).any()
    assert [b.time_step() for _ in range(2)] == dts_a
    for name in FIELDS + (("nu_t",) if a.use_les else ()):
        assert np.array_equal(host(getattr(a, name)), host(getattr(b, name))), name
    assert np.array_equal(host(a._stats_sums), host(b._stats_sums)) and a._stats_weight == b._stats_weight
    assert [s for s, _ in b.energy_history] == [saved_step, saved_step + 1]
    assert [e for _, e in b.energy_history] == [e for _, e in a.energy_history[-2:]]
    if ref_cls is not None:
        # The forces of those two steps.  A row is a float64 sum by atomics whose order is not
        # fixed (include/cfdsim.h), so runs A and B need not agree in the last bits: each is held
        # to force_bound of the NumPy reference continued from the saved fields, as in
        # tests/test_gpu_cyl3d.py, and so they differ by at most twice that.  A row added onto an
        # earlier run's row would be off by that row, a whole force.
        o = ref_cls(a.config)
        o.u, o.v, o.w = (saved[n].copy() for n in ("u", "v", "w"))
        if a.use_les:
            o.nu_t = saved["nu_t"].copy()
        o.step = saved_step
        assert [o.time_step() for _ in range(2)] == dts_a
        assert np.array_equal(o.u, host(b.u)) and np.array_equal(o.w, host(b.w))
        rows_a, rows_b = a.force_history[-2:], b.force_history
        assert [r[0] for r in rows_a] == [r[0] for r in rows_b] == [r[0] for r in o.force_history]
        for ra, rb, ro, stats in zip(rows_a, rows_b, o.force_history, o.force_stats):
            bound = force_bound(stats)
            fa, fb, fo = (np.array(r[1:]) for r in (ra, rb, ro))
            print(case, "force rows", ra, rb, "ref", ro, "bound", bound)
            assert fo[0] != 0 and (bound < 1e-9 * np.abs(fo[0])).all()   # a doubled row is far outside
            assert (np.abs(fa - fo) <= bound).all() and (np.abs(fb - fo) <= bound).all()
            assert (np.abs(fa - fb) <= 2 * bound).all()
        assert [c[0] for c in b.force_coefficients()] == [saved_step, saved_step + 1]
    assert b.load_snapshot(path) == 0.25 and b.step == saved_step + 2
    with pytest.raises(KeyError):
        b.load_snapshot(path, step=7)
    # statistics on with other settings, and a solver of another grid shape
    d = make()
    d.enable_statistics(start_step=5)
    with pytest.raises(ValueError, match="statistics"):
        d.load_snapshot(path)
    with pytest.raises(ValueError, match="grid"):
        make(**other).load_snapshot(path)
