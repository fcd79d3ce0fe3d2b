"""The edge-value cases of the 3-D predictor, LES and scalar marches on the
CPU (tests/march3d_edge_reference.py): on every input class the NumPy
statements equal literal per-cell loops written with Python ``if`` on
np.float32 scalars (so np.where against a branch is what is checked under
NaN), every row of ``CASES`` holds what its class promises on the shape the
GPU file runs (no GPU comparison there is NaN against NaN everywhere), and the
facts about ``SEAM_CELLS`` that file relies on."""
import pathlib

import numpy as np
import pytest

import march3d_edge_reference as M
from march3d_edge_reference import (ART, CASES, CELL, CLASSES, CS, ENTRIES, INV_PRT, MARCH, SEAM_CELLS, TINY, T_ZERO,
                                    census, describe_difference, face_cells, interior, same_bits)
from ref3d import pred_constants
from test_les3d_host import scalar_smagorinsky
from test_ref3d_host import scalar_predictor
from zper_reference import crop_z, pad_z

F = np.float32
COPIES = ("u_star", "v_star", "w_star", "T_new")   # outputs whose faces copy an input through
NEG0 = np.uint32(0x80000000)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------ literal loops
def loop_predictor(u, v, w, nu, sp, dt, supg):
    """scalar_predictor of tests/test_ref3d_host.py; with ``nu`` an array,
    cell by cell on the cell's 3 x 3 x 3 neighbourhood with the cell's nu."""
    if np.ndim(nu) == 0:
        return scalar_predictor(u, v, w, nu, sp["dx"], sp["dy"], sp["dz"], dt, supg)
    out = {n: f.copy() for n, f in (("u_star", u), ("v_star", v), ("w_star", w))}
    out["tau"] = np.zeros_like(u)
    nz, ny, nx = u.shape
    for z in range(1, nz - 1):
        for j in range(1, ny - 1):
            for i in range(1, nx - 1):
                box = (slice(z - 1, z + 2), slice(j - 1, j + 2), slice(i - 1, i + 2))
                one = scalar_predictor(u[box].copy(), v[box].copy(), w[box].copy(), nu[z, j, i], sp["dx"], sp["dy"],
                                       sp["dz"], dt, supg)
                for n in out:
                    out[n][z, j, i] = one[n][1, 1, 1]
    return out


def loop_les(u, v, w, nu, art, cs, sp, dt, supg):
    """scalar_smagorinsky of tests/test_les3d_host.py, (F(nu) + nu_t) + F(art)
    per cell, then the loop above with that array."""
    nu_t = scalar_smagorinsky(u, v, w, sp["dx"], sp["dy"], sp["dz"], cs)
    ne = np.zeros_like(u)
    for k in np.ndindex(u.shape):
        r = (F(nu) + nu_t[k]) + F(art)
        assert type(r) is F
        ne[k] = r
    out = loop_predictor(u, v, w, ne, sp, dt, supg)
    out["nu_t"] = nu_t
    return out


def loop_add_buoyancy(pr, T, b, t_ref, dt):
    """The literal loop of tests/test_buoyancy3d_host.py."""
    nz, ny, nx = T.shape
    for name, bf in zip(("u_star", "v_star", "w_star"), b):
        p = pr[name].copy()
        for k in range(1, nz - 1):
            for j in range(1, ny - 1):
                for i in range(1, nx - 1):
                    theta = F(T[k, j, i] - F(t_ref))
                    pr[name][k, j, i] = F(p[k, j, i] + F(F(dt) * F(F(bf) * theta)))
    return pr


def loop_scalar_advance(T, u, v, w, alpha, nu_t, inv_prt, sp, dt, supg, periodic):
    """scalar_advance3d_numpy one float32 scalar operation at a time, every
    np.where a Python branch, periodic z by indices modulo nz (not the pad
    rule)."""
    k = pred_constants(**sp)
    dt, two, one, zero = F(dt), F(2), F(1), F(0)
    out = T.copy()
    nz, ny, nx = T.shape
    for z in (range(nz) if periodic else range(1, nz - 1)):
        zu, zd = (z + 1) % nz, (z - 1) % nz
        for j in range(1, ny - 1):
            for i in range(1, nx - 1):
                ae = F(alpha)
                if nu_t is not None:
                    ae = F(alpha) + nu_t[z, j, i] * F(inv_prt)
                uc, vc, wc = u[z, j, i], v[z, j, i], w[z, j, i]
                c, e, ws, n, s, up, dn = (T[z, j, i], T[z, j, i + 1], T[z, j, i - 1], T[z, j + 1, i], T[z, j - 1, i],
                                          T[zu, j, i], T[zd, j, i])
                x2, y2, z2 = (e - two * c) + ws, (n - two * c) + s, (up - two * c) + dn
                if supg:
                    vm = np.sqrt((uc * uc + vc * vc) + wc * wc)
                    if vm > k["eps"]:
                        pe = (vm * k["h"]) / (ae + k["eps"])
                        half = pe / two
                        lim = half if half < one else one
                        t = (k["h"] / (two * vm)) * lim
                    else:
                        t = dt / two
                    ddx, ddy, ddz = (e - ws) * k["c1x"], (n - s) * k["c1y"], (up - dn) * k["c1z"]
                    conv = (uc * ddx + vc * ddy) + wc * ddz
                    if t > zero:
                        conv = conv - t * ((uc * (x2 * k["c2x"]) + vc * (y2 * k["c2y"])) + wc * (z2 * k["c2z"]))
                else:
                    ddx = (c - ws) * k["ux"] if uc > zero else (e - c) * k["ux"]
                    ddy = (c - s) * k["uy"] if vc > zero else (n - c) * k["uy"]
                    ddz = (c - dn) * k["uz"] if wc > zero else (up - c) * k["uz"]
                    conv = (uc * ddx + vc * ddy) + wc * ddz
                lap = ae * ((x2 * k["lx"] + y2 * k["ly"]) + z2 * k["lz"])
                r = c + dt * (-conv + lap)
                assert type(r) is F
                out[z, j, i] = r
    return out


def literal(row, shape):
    """The row's outputs from the loops alone."""
    c = M.inputs(row, shape)
    e = row.entry
    with np.errstate(all="ignore"):
        if e.startswith("scalar_advance3d"):
            nu_t = c.nu_t if e == "scalar_advance3d_nut" else None
            return {"T_new": loop_scalar_advance(c.T, c.u, c.v, c.w, row.nu, nu_t, INV_PRT, c.sp, c.dt, row.supg,
                                                 row.periodic)}
        u, v, w, T = ((pad_z(f) for f in (c.u, c.v, c.w, c.T)) if row.periodic else (c.u, c.v, c.w, c.T))
        if e == "smagorinsky3d":
            out = {"nu_t": scalar_smagorinsky(u, v, w, c.dx, c.dy, c.dz, CS)}
        elif e == "predictor3d_nu":
            out = loop_predictor(u, v, w, c.nu, c.sp, c.dt, row.supg)
        elif "les" in e:
            out = loop_les(u, v, w, row.nu, ART, CS, c.sp, c.dt, row.supg)
        else:
            out = loop_predictor(u, v, w, row.nu, c.sp, c.dt, row.supg)
        if "buoy" in e:
            loop_add_buoyancy(out, T, row.b, row.t_ref, c.dt)
    return {k: crop_z(a) for k, a in out.items()} if row.periodic else out


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_statements_equal_literal_loops(entry, cls):
    rows = M.rows_of(entry, cls)
    assert rows or (entry, cls) == ("smagorinsky3d", "viscosity")
    n = 0
    for row in rows:
        for shape in (CELL, TINY):
            if shape == TINY and row.periodic:
                continue   # a periodic nz is even
            ref, want = M.reference(row, shape), literal(row, shape)
            assert set(ref) == set(ENTRIES[entry].outputs)
            for name in ref:
                assert same_bits(ref[name], want[name]), (row, shape, name, describe_difference(ref[name], want[name]))
                n += 1
    assert n >= len(rows) * len(ENTRIES[entry].outputs)


# ------------------------------------------------- what each class promises
def shares_like_nonfinite(row, ref, finite=0.90, nan=0.001, inf=0.001):
    for name, a in ref.items():
        if name == "tau":
            assert np.isfinite(a).all(), row
            continue
        c = census(a, row.periodic)
        assert c["finite_share"] >= finite and c["nan_share"] >= nan and c["inf_share"] >= inf, (row, name, c)


def faces_of(shape, periodic):
    f = face_cells(shape)
    if periodic:
        f[0, 1:-1, 1:-1] = f[-1, 1:-1, 1:-1] = False
    return f


def check_class(row, ref, c):
    per, cls = row.periodic, row.cls
    face = faces_of(c.shape, per)
    copies = {n: (a, M.source_of(row, n, c)) for n, a in ref.items() if n in COPIES}
    assert copies or row.entry == "smagorinsky3d"
    # every case: the faces are the input's bits, and the operator did something on the interior
    for name, (a, src) in copies.items():
        assert np.array_equal(bits(a)[face], bits(src)[face]), (row, name)
        ai, si = interior(a, per), interior(src, per)
        if cls in ("neg_zero", "signed_zero"):   # mostly zeros: the signs are what changes
            assert (bits(ai) != bits(si)).sum() >= 0.25 * ai.size, (row, name)
        else:
            assert not same_bits(ai, si) and (ai != si).sum() >= 0.5 * ai.size, (row, name)
    plain_term = row.b is None or row.t_ref == T_ZERO    # else T - T_REF is -0.25 wherever T is tiny or zero
    if cls == "nonfinite":
        shares_like_nonfinite(row, ref)
        for name, (a, src) in copies.items():
            bad = face & ~np.isfinite(src)
            assert bad.sum() >= (1 if per else 4), (row, name)   # a seed on plane 0 or nz-1 is interior in periodic z
            assert same_bits(a[bad], src[bad]), (row, name)
    elif cls == "huge":
        shares_like_nonfinite(row, ref, inf=0.01, nan=0.0005)
    elif cls == "subnormal":
        tiny = np.finfo(F).tiny
        for name, (a, src) in copies.items():
            ai, si = interior(a, per), interior(src, per)
            assert (ai != 0).all() and (ai != si).all(), (row, name)
            if plain_term:
                assert (np.abs(ai) < tiny).all(), (row, name)
            else:
                assert (np.abs(ai) >= tiny).all(), (row, name)   # the term, dt * b * (-0.25), swamps the field
        if "nu_t" in ref:    # squares of subnormal gradients are 0
            assert not ref["nu_t"].any() and not np.signbit(ref["nu_t"]).any()
    elif cls == "neg_zero":
        for name, (a, src) in copies.items():
            assert (bits(a)[face] == NEG0).all(), (row, name)
            if plain_term:
                assert (bits(interior(a, per)) == 0).all(), (row, name)
            else:
                assert (interior(a, per) != 0).all(), (row, name)
        if "tau" in ref and row.supg:
            assert (interior(ref["tau"], per) == c.dt / F(2)).all(), row
    elif cls == "signed_zero":
        for name, (a, src) in copies.items():
            b = bits(a)
            assert (b == 0).any() and (b == NEG0).any() and np.count_nonzero(a) >= 100, (row, name)
    else:
        assert cls == "viscosity"
        if ENTRIES[row.entry].array_visc:
            shares_like_nonfinite(row, ref)
            if "tau" in ref and row.supg:
                t = interior(ref["tau"], per)
                sub = (t > 0) & (t < np.finfo(F).tiny)
                assert sub.sum() >= 100 and (t < 0).sum() >= 100 and (t == 0).sum() >= 100, (row, sub.sum())
        elif "tau" in ref and row.supg:
            t = interior(ref["tau"], per)
            assert np.isfinite(t).all()
            if row.nu == F(3e38):
                assert ((t > 0) & (t < np.finfo(F).tiny)).mean() >= 0.9, row
            elif row.nu < 0:
                assert (t < 0).mean() >= 0.9, row
            else:
                assert (t > 0).all(), row


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_case_holds_what_its_class_promises(entry, cls):
    for row in M.rows_of(entry, cls):
        ref = M.reference(row, MARCH)
        check_class(row, ref, M.inputs(row, MARCH))
        for a in ref.values():      # the GPU file's outputs start at 7.0: an unwritten cell shows
            assert not (a == 7.0).any()


def test_smagorinsky_cases_are_discriminating():
    """nu_t has no input to differ from: what its classes leave in it."""
    for cls in CLASSES[:-1]:
        (row,) = M.rows_of("smagorinsky3d", cls)
        ref = M.reference(row, MARCH)["nu_t"]
        c = census(ref)
        assert not ref[face_cells(MARCH)].any()
        if cls in ("nonfinite", "huge"):
            assert c["nan"] >= 10 and c["inf"] >= 10 and c["finite_share"] >= 0.9
        elif cls == "signed_zero":
            assert np.count_nonzero(interior(ref)) >= 100 and c["pos_zero"] >= 100
        else:
            assert c["pos_zero"] == c["n"]


# ------------------------------------------------------------- the builders
@pytest.mark.parametrize("shape", [MARCH, CELL, TINY])
def test_builders(shape):
    face = face_cells(shape)
    for cls in CLASSES:
        c = M.build(cls, shape)
        assert M.build(cls, shape) is c
        for a in (c.u, c.v, c.w, c.T, c.nu, c.nu_t):
            assert a.dtype == F and a.shape == shape and not a.flags.writeable
    c = M.build("nonfinite", shape)
    if shape == MARCH:
        vel = [tuple(k) for f in (c.u, c.v, c.w) for k in np.argwhere(~np.isfinite(f))]
        assert len(vel) == 48 and set(vel) <= set(SEAM_CELLS) and sum(face[k] for k in vel) >= 8
        for f in (c.T, c.nu_t):
            bad = [tuple(k) for k in np.argwhere(~np.isfinite(f))]
            assert len(bad) == 16 and set(bad) <= set(SEAM_CELLS) and sum(face[k] for k in bad) >= 4
        for f in (c.u, c.v, c.w, c.T, c.nu_t):
            assert np.isnan(f).any() and (f == np.inf).any() and (f == -np.inf).any()
    c = M.build("neg_zero", shape)
    for f in (c.u, c.v, c.w, c.T, c.nu_t):
        assert (bits(f) == NEG0).all()
    assert (c.nu > 0).all()
    c = M.build("signed_zero", shape)
    for f in (c.u, c.v, c.w, c.T, c.nu_t):
        b = bits(f)
        assert (b[face] == 0).any() and (b[face] == NEG0).any() and np.count_nonzero(f) >= (60 if shape == MARCH else 1)
    c = M.build("subnormal", shape)
    for f in (c.u, c.v, c.w, c.T, c.nu_t):
        assert (f != 0).all() and (np.abs(f) < np.finfo(F).tiny).all() and (f < 0).any() and (f > 0).any()
    c = M.build("huge", shape)
    with np.errstate(over="ignore"):
        sq = [f * f for f in (c.u, c.v, c.w)]
        two, three = sq[0] + sq[1], (sq[0] + sq[1]) + sq[2]
    assert (np.isfinite(two) & np.isinf(three) & np.isfinite(sq[2])).any()      # only the sum of three overflows
    assert (np.isinf(sq[0]) & (np.abs(c.u) < 1e20)).any()                        # one square overflows
    assert (c.u > 9e37).any() and (c.v < -9e37).any()
    assert (c.T > 9e37).any() and (c.T < -9e37).any()
    if shape == MARCH:
        assert ((c.u > 9e37) & (c.v < -9e37)).any()     # the two patches overlap
        for f, lim in ((c.u, 9e37), (-c.v, 9e37), (c.T, 9e37), (-c.T, 9e37)):
            z, _, x = np.nonzero(f > lim)
            assert z.min() < 8 <= z.max()
        _, _, x = np.nonzero(c.u > 9e37)
        assert x.min() < 64 <= x.max()
    c = M.build("viscosity", shape)
    for f in (c.nu, c.nu_t):
        assert (f == 0).any() and (f == F(-0.01)).any() and (f == F(1e-42)).any() and (f == np.inf).any()
        assert np.isnan(f).any() and (f > 2e38).any() and np.isfinite(f[f > 2e38]).any()
    with np.errstate(over="ignore"):
        assert (c.nu == F(3e38)).any() and np.isfinite(F(2.5e38) * INV_PRT) and not np.isfinite(F(3e38) * INV_PRT)
    if shape == MARCH:
        for val in M.VISCOSITY_BANDS:
            _, _, x = np.nonzero(np.isnan(c.nu) if np.isnan(val) else c.nu == val)
            assert (x.min() < 64 <= x.max()) or (x.min() < 128 <= x.max()), val
        xs = np.nonzero((c.nu == 0) | np.isnan(c.nu) | (c.nu == np.inf))[2]
        assert (xs < 64).any() and ((xs >= 64) & (xs < 128)).any() and (xs >= 128).any()


# --------------------------------------------- facts the GPU file relies on
def test_seam_cells():
    cells = np.array(SEAM_CELLS)
    assert len(SEAM_CELLS) == len(set(SEAM_CELLS)) == 480
    assert (cells >= 0).all() and (cells < np.array(MARCH)).all()
    z, y, x = cells.T
    for seam in (64, 128):      # cells in both segments on each side of the seam, the seam's own two columns among them
        assert {seam - 2, seam - 1, seam, seam + 1} <= set(x.tolist())
    assert {7, 8} <= set(z.tolist()) and (z > 8).any()          # both sides of the chunk seam at plane 8
    for row in (4, 8):                                           # both sides of the tile edges
        assert {row - 1, row} <= set(y.tolist())
    face = face_cells(MARCH)
    assert sum(face[c] for c in SEAM_CELLS) >= 100 and sum(not face[c] for c in SEAM_CELLS) >= 100


def test_cases_cover_the_family():
    names = {M.c_entry(r) for r in CASES}
    assert names == {"cfd_predictor3d_f32", "cfd_predictor3d_zper_f32", "cfd_predictor3d_nu_f32",
                     "cfd_predictor3d_les_f32", "cfd_predictor3d_les_zper_f32", "cfd_smagorinsky3d_f32",
                     "cfd_predictor3d_buoy_f32", "cfd_predictor3d_buoy_zper_f32", "cfd_predictor3d_les_buoy_f32",
                     "cfd_predictor3d_les_buoy_zper_f32", "cfd_scalar_advance3d_f32", "cfd_scalar_advance3d_zper_f32"}
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "cfdsim.h").read_text()
    for n in names:
        assert n + "(" in text, n
    for name, e in ENTRIES.items():
        for cls in CLASSES:
            rows = M.rows_of(name, cls)
            if (name, cls) == ("smagorinsky3d", "viscosity"):
                assert not rows
                continue
            assert {r.periodic for r in rows} == ({False, True} if e.zper_statement else {False}), (name, cls)
            assert {r.supg for r in rows} == ({True} if name == "smagorinsky3d" else {True, False}), (name, cls)
            if cls == "viscosity" and not e.array_visc:
                assert {r.nu for r in rows} == set(M.VISCOSITY_SCALARS)
            if "buoy" in name:
                assert all(r.b is not None and r.t_ref is not None for r in rows)
                if cls in ("nonfinite", "huge"):
                    assert any(r.b[0] == 0 and r.b[2] == 0 for r in rows)
    for r in CASES:
        assert callable(M.statement(r))
    assert len(CASES) == len(set(CASES))
