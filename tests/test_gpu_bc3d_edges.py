"""The 3-D boundary stages on the GPU at edge values
(tests/bc3d_edge_reference.py): k_channel_bc_ibm3d<ZP> through
K.apply_channel_bc_ibm3d and k_scalar_heat3d + k_scalar_faces3d<ZP> through
K.apply_scalar_bc_heat3d, every class on every shape, periodic and not, with
the tight box of the mask and with the whole plane, with and without the sum
output.

Bars.  Fields: ``same_bits`` on every cell (the stage works in place) -- NaNs
at the same cells, every other value bit for bit, -0.0 apart from +0.0.  Sums:
``sum_rule`` of the reference's float64 terms -- NaN, the one infinity, or the
statement's sum within the project's 2 (n - 1) 2^-53 sum|t| with a finite
preset as one more term.  force_strength 0 with a finite mask: the unforced
fields and the preset's own bits.  tests/test_bc3d_edge_host.py pins the
statements to literal loops on the same cases.
"""
import numpy as np
import pytest
import torch

import bc3d_edge_reference as B
from bc3d_edge_reference import CLASSES, SHAPES, Y_MAX, describe_difference, same_bits
from cfd_simulations_amd import kernels as K
from cfd_simulations_amd.solver import host_ibm_bbox

pytestmark = pytest.mark.gpu

IDS = [f"{s}{'-periodic' if p else ''}" for s, p in SHAPES]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")   # a writable copy


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def boxes_of(mask):
    return (("tight", host_ibm_bbox(mask)), ("plane", None))


def run_channel(c, periodic, box, preset):
    t = [dev(a) for a in (c.u, c.v, c.w)]
    force = None if preset is None else torch.full((3,), preset, dtype=torch.float64, device="cuda")
    K.apply_channel_bc_ibm3d(*t, dev(c.y), dev(c.mask), Y_MAX, c.v_inf, c.step, c.fs, bbox=box, force_out=force,
                             periodic_z=periodic)
    return [host(a) for a in t], None if force is None else host(force)


def run_heat(c, periodic, box, preset):
    t = dev(c.T)
    heat = None if preset is None else torch.full((1,), preset, dtype=torch.float64, device="cuda")
    K.apply_scalar_bc_heat3d(t, dev(c.mask), c.t_in, c.t_cyl, c.fs, bbox=box, heat_out=heat, periodic_z=periodic)
    return host(t), None if heat is None else host(heat)


def check_sum(value, rule, c, where, bad, worst):
    ok, ratio = B.obeys(value, rule)
    if ratio is not None:
        worst[0] = max(worst[0], ratio)
    if not ok:
        bad.append((c.name, *where, "sum", float(value), rule))
    if c.fs == 0 and np.isfinite(c.mask).all() and bits64(value) != bits64(c.preset):
        bad.append((c.name, *where, "fs = 0 changed the preset", float(value), c.preset))


@pytest.mark.parametrize("shape,periodic", SHAPES, ids=IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_channel_bc_ibm3d_edges(cls, shape, periodic):
    bad, worst, arrays, sums = [], [0.0], 0, 0
    for n, c in enumerate(B.cases(cls, shape, periodic)):
        ref = B.reference(cls, shape, periodic, n)
        rules = [B.force_rule(ref, c.preset, q) for q in range(3)]
        for label, box in boxes_of(c.mask):
            for preset in (c.preset, None):
                got, force = run_channel(c, periodic, box, preset)
                for name, g, r in zip("uvw", got, ref["fields"]):
                    arrays += 1
                    if not same_bits(g, r):
                        bad.append((c.name, label, preset, name, describe_difference(g, r)))
                if force is not None:
                    for q in range(3):
                        sums += 1
                        check_sum(force[q], rules[q], c, (label, "uvw"[q]), bad, worst)
        if c.fs == 0 and np.isfinite(c.mask).all():
            assert all(same_bits(a, b) for a, b in zip(ref["fields"], ref["unforced"]))
    print("channel", cls, shape, "periodic" if periodic else "", arrays, "arrays compared,", sums,
          "sums, worst err / bound", worst[0])
    assert arrays and sums
    assert not bad, f"{len(bad)} differ; the first: " + "; ".join(str(b) for b in bad[:6])


@pytest.mark.parametrize("shape,periodic", SHAPES, ids=IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_scalar_bc_heat3d_edges(cls, shape, periodic):
    bad, worst, arrays, sums = [], [0.0], 0, 0
    for n, c in enumerate(B.heat_cases(cls, shape, periodic)):
        ref = B.heat_reference(cls, shape, periodic, n)
        rule = B.heat_rule(ref, c.preset)
        for label, box in boxes_of(c.mask):
            for preset in (c.preset, None):
                got, heat = run_heat(c, periodic, box, preset)
                arrays += 1
                if not same_bits(got, ref["T"]):
                    bad.append((c.name, label, preset, describe_difference(got, ref["T"])))
                if heat is not None:
                    sums += 1
                    check_sum(heat[0], rule, c, (label,), bad, worst)
    print("heat", cls, shape, "periodic" if periodic else "", arrays, "arrays compared,", sums,
          "sums, worst err / bound", worst[0])
    assert arrays and sums
    assert not bad, f"{len(bad)} differ; the first: " + "; ".join(str(b) for b in bad[:6])
