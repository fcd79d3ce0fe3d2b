"""cfd_rbgs3d_mask2d_f32's host side (no GPU): the entry point in the header,
the bindings and the library, its argument checks, and the wrapper's handling
of the mask shapes."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from cfd_simulations_amd import _lib
from cfd_simulations_amd import kernels as K

ROOT = Path(__file__).resolve().parents[1]
NAME = "cfd_rbgs3d_mask2d_f32"


def test_entry_point_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cfdsim.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+" + NAME + r"\s*\(", text, flags=re.M)
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), NAME)
    # the same argument list as cfd_rbgs3d_f32: only the mask's shape differs
    assert _lib.PROTOTYPES[NAME] == _lib.PROTOTYPES["cfd_rbgs3d_f32"] and len(_lib.PROTOTYPES[NAME][1]) == 16


def test_host_refusals_need_no_gpu():
    """cfd_rbgs3d_f32's argument checks, before any device work."""
    L = _lib.lib()
    p = [ctypes.c_void_p(4096 * (q + 1)) for q in range(5)]  # never dereferenced
    f = getattr(L, NAME)
    tail = (0.1, 0.1, 0.1, 0.01, 3, 0.0)
    assert f(None, p[1], p[2], 4, 5, 8, *tail, p[3], p[4], None, None) == -1 and b"null" in L.cfd_last_error()
    assert f(p[0], None, p[2], 4, 5, 8, *tail, p[3], p[4], None, None) == -1
    assert f(p[0], p[1], p[2], 4, 5, 8, *tail, p[3], None, None, None) == -1   # no workspace
    assert f(p[0], p[1], p[2], 0, 5, 8, *tail, p[3], p[4], None, None) == -1 and b"bad" in L.cfd_last_error()
    assert f(p[0], p[1], p[2], 4, 5, 8, 0.1, 0.1, 0.1, 0.01, -1, 0.0, p[3], p[4], None, None) == -1


@pytest.fixture
def calls(monkeypatch):
    """The wrapper with its library call recorded instead of made."""
    seen = []
    monkeypatch.setattr(K, "call", lambda name, *a: seen.append((name, a)))
    monkeypatch.setattr(K, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(K, "stream_handle", lambda: 0)
    return seen


def test_wrapper_picks_the_entry_by_mask_shape(calls):
    nz, ny, nx = 4, 5, 8
    phi, div = torch.zeros((nz, ny, nx)), torch.zeros((nz, ny, nx))
    args = (phi, div, 0.1, 0.1, 0.1, np.float32(0.01))
    m2 = torch.zeros((ny, nx), dtype=torch.bool)
    m2[2, 3] = True
    K.solve_pressure_gauss_seidel3d(*args, m2, 3, 0.0)
    K.solve_pressure_gauss_seidel3d(*args, m2.expand(nz, ny, nx), 3, 0.0)
    K.solve_pressure_gauss_seidel3d(*args, None, 3, 0.0)
    assert [c[0] for c in calls] == [NAME, "cfd_rbgs3d_f32", "cfd_rbgs3d_f32"]
    assert calls[0][1][2] is not None and calls[1][1][2] is not None and calls[2][1][2] is None
    assert [c[1][3:6] for c in calls] == [(nz, ny, nx)] * 3
    for bad in ((nx, ny), (ny, nx + 1), (1, ny, nx), (nz, ny, nx, 1), (ny * nx,)):
        with pytest.raises(ValueError, match="mask shape"):
            K.solve_pressure_gauss_seidel3d(*args, torch.zeros(bad, dtype=torch.uint8), 3, 0.0)
    assert len(calls) == 3


def test_wrapper_refuses_cpu_tensors():
    phi, div = torch.zeros((4, 5, 8)), torch.zeros((4, 5, 8))
    for mask in (torch.zeros((5, 8), dtype=torch.uint8), torch.zeros((4, 5, 8), dtype=torch.uint8)):
        with pytest.raises(TypeError, match="device tensors"):
            K.solve_pressure_gauss_seidel3d(phi, div, 0.1, 0.1, 0.1, np.float32(0.01), mask, 3, 0.0)
