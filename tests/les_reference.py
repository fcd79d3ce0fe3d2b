"""The project's NumPy statement of the LES arithmetic (use_les=True): the
Smagorinsky eddy viscosity of compute_smagorinsky_viscosity_fast
(v5.py:96-110) and the step's nu_eff (v5.py:388), as array code.

The reference ships with LES switched off and tests/golden/make_golden.py
generates no LES fixture, so the GPU path is pinned to these functions and
parity with the reference itself is unpinned until such a fixture exists.
tests/test_les_host.py checks them against a per-cell scalar loop.
"""
import math

import numpy as np


def smagorinsky_numpy(u, v, dx, dy, cs):
    """nu_t = (cs sqrt(dx dy))**2 |S| on the interior, forward differences to
    the east (j + 1) and north (i + 1) neighbours, 0 on the boundary ring.
    Python-float constants round to the arrays' dtype where they meet them
    (NEP 50); u, v float32 or float64."""
    nu_t = np.zeros_like(u)
    c = u[1:-1, 1:-1]
    d = v[1:-1, 1:-1]
    dudx = (u[1:-1, 2:] - c) * (1.0 / dx)
    dudy = (u[2:, 1:-1] - c) * (1.0 / dy)
    dvdx = (v[1:-1, 2:] - d) * (1.0 / dx)
    dvdy = (v[2:, 1:-1] - d) * (1.0 / dy)
    q = 2 * (dudx * dudx + dvdy * dvdy) + (dudy + dvdx) * (dudy + dvdx)
    nu_t[1:-1, 1:-1] = ((cs * math.sqrt(dx * dy)) ** 2) * np.sqrt(q)
    return nu_t


def nu_eff_numpy(nu_t, nu, art_visc):
    """(T(nu) + nu_t) + T(art_visc) in nu_t's dtype T (v5.py:388)."""
    T = nu_t.dtype.type
    return (T(nu) + nu_t) + T(art_visc)
