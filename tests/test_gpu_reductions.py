"""The health and diagnostic reductions on the GPU against the plain NumPy
statements of tests/diag_reference.py (pinned on the host by
tests/test_diag_host.py):

* cfd_absmax_f32, cfd_absmax2_f32/_f64, cfd_nonfinite_count_f32/_f64 at sizes
  around a lane, a wave, a workgroup, the last size without a grid stride and
  past it: BIT FOR BIT / exact counts, with the spike or the non-finite value
  planted at the first and last element and on both sides of a wave boundary;
  NaN never wins, Inf does, -0.0 and denormals, `out` accumulates for the
  maxima and is reset for the count.
* cfd_mean_*, cfd_energy_mean2d_*, cfd_energy_mean_clip2d_*: against the
  correctly rounded sum within (n + 2) 2^-53 relative -- any order of n
  non-negative float64 additions is within (n - 1) 2^-53 of the exact sum to
  first order, the scaling adds a rounding -- through the many-block path, its
  last size 2^20 and the atomic path past it; run-to-run bits up to 2^20.
* the scratch (ticket word and partials) the many-block sums share, across
  back-to-back calls of different kernels and across two streams.
* the maxima fused into the 2-D field kernels (cfd_vorticity_absmax2d_f32,
  cfd_vorticity2d_f64, cfd_divergence2d_*, cfd_project2d_*): BIT FOR BIT
  against the fold over the reference's field, with the reference's argmax
  placed on every interior corner and on both sides of the wave and workgroup
  boundaries in x.
"""
import contextlib

import numpy as np
import pytest
import torch

from cfd_simulations_amd import kernels as K
from cfd_simulations_amd._lib import call, ptr, stream_handle
from diag_reference import (DX, DY, ENERGY_ONE_PASS, GRID1D, SHAPES_2D, SIZES, SUM_SIZES, divergence2d,
                            energy_mean_exact, fields2d, fold_absmax, gradient2d, has_interior, mean64_exact, noise,
                            nonfinite_count, project2d, vorticity2d)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [np.float32, np.float64]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
SFX = {torch.float32: "_f32", torch.float64: "_f64"}
EPS = 2.0 ** -53
INTERIOR = [s for s in SHAPES_2D if has_interior(s)]
NO_INTERIOR = [s for s in SHAPES_2D if not has_interior(s)]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared inputs are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(autouse=True)
def _reset_tuning():
    call("cfd_reset_tuning")
    yield
    call("cfd_reset_tuning")


def bits(x):
    return np.asarray(x).tobytes()


def scalar(dtype, value=0.0):
    return torch.full((1,), value, dtype=TORCH.get(dtype, dtype), device=DEV)


def positions(n):
    """First and last element, both sides of the first wave boundary, the middle."""
    return sorted({p for p in (0, 63, 64, n // 2, n - 1) if 0 <= p < n})


class Both:
    """An array on the host (a writable copy) and on the device."""

    def __init__(self, a):
        self.h = np.array(a)
        self.d = dev(self.h)

    @contextlib.contextmanager
    def planted(self, p, value):
        keep = self.h[p]
        self.h[p] = value
        self.d[p] = float(value)
        try:
            yield self
        finally:
            self.h[p] = keep
            self.d[p] = float(keep)


# ------------------------------------------------------------------ absmax
def absmax(a, b=None, out=None):
    """cfd_absmax_f32 / cfd_absmax2_f32 / cfd_absmax2_f64 (b may be NULL there)."""
    out = torch.zeros(1, dtype=a.dtype, device=DEV) if out is None else out
    if a.dtype == torch.float64:
        call("cfd_absmax2_f64", ptr(a), ptr(b), a.numel(), ptr(out), stream_handle())
    elif b is None:
        call("cfd_absmax_f32", ptr(a), a.numel(), ptr(out), stream_handle())
    else:
        call("cfd_absmax2_f32", ptr(a), ptr(b), a.numel(), ptr(out), stream_handle())
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_absmax_spike_positions(n, dtype):
    a, b = Both(noise(n, dtype, seed=1)), Both(noise(n, dtype, seed=2))
    assert bits(host(absmax(a.d))[0]) == bits(fold_absmax(a.h))
    assert bits(host(absmax(a.d, b.d))[0]) == bits(fold_absmax(a.h, b.h))
    for k, p in enumerate(positions(n)):
        spike = dtype(-(1.5 + 0.125 * k))  # larger than the noise, negative
        for x in (a, b):
            with x.planted(p, spike):
                want = fold_absmax(a.h, b.h)
                assert want == -spike == fold_absmax(x.h)
                assert bits(host(absmax(a.d, b.d))[0]) == bits(want), (p, x is a)
                assert bits(host(absmax(x.d))[0]) == bits(want), (p, x is a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_absmax_special_values(n, dtype):
    T = dtype
    a = Both(noise(n, dtype, seed=1))
    for p in positions(n):
        for s in (np.inf, -np.inf):
            with a.planted(p, T(s)):
                got = host(absmax(a.d))[0]
                assert got == np.inf and bits(got) == bits(fold_absmax(a.h)), (p, s)
    # NaNs scattered, the last element among them, are ignored
    x = np.array(a.h)
    idx = np.random.default_rng(n).choice(n, size=max(1, n // 7), replace=False)
    x[idx] = np.nan
    x[n - 1] = np.nan
    want = fold_absmax(x)
    assert (want > 0) == (n > 1) and not np.isnan(want)
    assert bits(host(absmax(dev(x)))[0]) == bits(want)
    assert bits(host(absmax(dev(x), dev(x)))[0]) == bits(want)
    # all NaN: a zeroed out stays 0; all -0.0: +0.0
    for fill in (np.nan, -0.0):
        x = dev(np.full(n, fill, dtype))
        for got in (host(absmax(x))[0], host(absmax(x, x))[0]):
            assert bits(got) == bits(T(0.0)) == bits(fold_absmax(np.full(n, fill, dtype)))
    # denormals: the maximum comes back exactly, not flushed
    tiny = np.finfo(dtype).tiny
    x = (a.h.astype(np.float64) * (float(tiny) / 128)).astype(dtype)
    want = fold_absmax(x)
    assert 0 < want < tiny
    assert bits(host(absmax(dev(x)))[0]) == bits(want)
    assert bits(host(absmax(dev(-x), dev(x)))[0]) == bits(want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1000, GRID1D + 1])
def test_absmax_accumulates_into_out(n, dtype):
    """`out` is not reset: a larger preset stands, a smaller one is raised,
    and three calls into one `out` give the maximum over the three fields
    (monitor_simulation_health3d, the 3-D adaptive dt)."""
    u, v, w = (noise(n, dtype, seed=s) for s in (1, 2, 3))
    m = fold_absmax(u)
    for preset in (7.5, float(np.nextafter(m, dtype(2)))):
        out = scalar(dtype, preset)
        assert bits(host(absmax(dev(u), out=out))[0]) == bits(dtype(preset)) == bits(fold_absmax(u, start=preset))
    for preset in (0.25, float(np.nextafter(m, dtype(0)))):
        out = scalar(dtype, preset)
        assert bits(host(absmax(dev(u), out=out))[0]) == bits(m) == bits(fold_absmax(u, start=preset))
    scale = {0: (3, 1, 2), 1: (1, 3, 2), 2: (1, 2, 3)}  # the largest field first, second, last
    for order in scale.values():
        fs = [(f * dtype(s)).astype(dtype) for f, s in zip((u, v, w), order)]
        out = scalar(dtype)
        for f in fs:
            absmax(dev(f), out=out)
        want = fold_absmax(*fs)
        assert want == fold_absmax(fs[order.index(3)]) > max(fold_absmax(fs[order.index(k)]) for k in (1, 2))
        assert bits(host(out)[0]) == bits(want)


def test_absmax_f64_orders_all_64_bits():
    """The float64 maximum goes through a 64-bit integer atomicMax of the bit
    pattern: magnitudes that differ only in the low word, a smaller high word
    under a larger low word, and values above 2^32."""
    n = 70001  # 274 workgroups: the waves' maxima meet in the atomic
    rng = np.random.default_rng(64)
    sign = rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)
    hi = np.uint64(0x3FF80000) << np.uint64(32)  # 1.5
    cases = []
    low = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    cases.append((hi | low | sign).view(np.float64))
    # half the values just below 1.5 with a large low word, half at 1.5 with a small one
    below = ((np.uint64(0x3FF7FFFF) << np.uint64(32)) | rng.integers(0xF0000000, 1 << 32, n, dtype=np.uint64))
    above = hi | rng.integers(0, 0x10000000, n, dtype=np.uint64)
    cases.append((np.where(rng.random(n) < 0.5, below, above) | sign).view(np.float64))
    big = rng.uniform(1.0, 1000.0, n) * 2.0 ** 32
    cases.append(np.where(sign > 0, -big, big))
    cases.append(np.where(rng.random(n) < 0.5, big, rng.uniform(0, 1, n) * 2.0 ** -40))
    for x in cases:
        assert not np.isnan(x).any()
        want = fold_absmax(x)
        assert want == np.abs(x).max()
        assert bits(host(absmax(dev(x)))[0]) == bits(want)
        assert bits(host(absmax(dev(x[::-1]), dev(-x)))[0]) == bits(want)
        # a preset one ulp below is raised, one ulp above stands
        lo, up = np.nextafter(want, 0.0), np.nextafter(want, np.inf)
        assert bits(host(absmax(dev(x), out=scalar(np.float64, float(lo))))[0]) == bits(want)
        assert bits(host(absmax(dev(x), out=scalar(np.float64, float(up))))[0]) == bits(up)


# --------------------------------------------------------- nonfinite_count
def nonfinite(a, b=None):
    out = torch.full((1,), 12345, dtype=torch.int32, device=DEV)  # reset by the call
    call("cfd_nonfinite_count" + SFX[a.dtype], ptr(a), ptr(b), a.numel(), ptr(out), stream_handle())
    return int(host(out)[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_count_planted(n, dtype):
    a, b = Both(noise(n, dtype, seed=1)), Both(noise(n, dtype, seed=2))
    assert nonfinite(a.d, b.d) == 0 == nonfinite_count(a.h, b.h) and nonfinite(a.d) == 0
    for p in positions(n):
        for s in (np.nan, np.inf, -np.inf):
            with a.planted(p, dtype(s)):
                assert nonfinite(a.d, b.d) == 1 == nonfinite_count(a.h, b.h), (p, s)
                assert nonfinite(a.d) == 1 == nonfinite_count(a.h), (p, s)
                with b.planted(p, dtype(s)):  # the same cell of both counts twice
                    assert nonfinite(a.d, b.d) == 2 == nonfinite_count(a.h, b.h), (p, s)
            with b.planted(p, dtype(s)):
                assert nonfinite(a.d, b.d) == 1 == nonfinite_count(a.h, b.h), (p, s)
                assert nonfinite(a.d) == 0 == nonfinite_count(a.h), (p, s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_count_scattered(n, dtype):
    rng = np.random.default_rng(n + 7)
    a, b = np.array(noise(n, dtype, seed=1)), np.array(noise(n, dtype, seed=2))
    for x in (a, b):
        idx = rng.choice(n, size=max(1, n // 9), replace=False)
        x[idx] = rng.choice([np.nan, np.inf, -np.inf], size=idx.size)
    a[0] = b[n - 1] = np.nan
    want = nonfinite_count(a, b)
    assert want >= 2
    assert nonfinite(dev(a), dev(b)) == want
    assert nonfinite(dev(b)) == nonfinite_count(b) and nonfinite(dev(a)) == nonfinite_count(a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_count_all_nan_counts_every_cell(dtype):
    n = SIZES[-1]
    x = dev(np.full(n, np.nan, dtype))
    assert nonfinite(x, x) == 2 * n == nonfinite_count(np.full(n, np.nan, dtype), np.full(n, np.nan, dtype))
    assert nonfinite(x) == n


# ------------------------------------------------------------------- means
def mean(a, out=None, stream=None):
    out = scalar(torch.float64, float("nan")) if out is None else out  # overwritten
    call("cfd_mean" + SFX[a.dtype], ptr(a), a.numel(), ptr(out), stream_handle(stream))
    return out


def energy(u, v, out=None, clip=None, stream=None):
    """cfd_energy_mean2d_* or, with clip = (lo, hi), cfd_energy_mean_clip2d_*."""
    out = scalar(torch.float64, float("nan")) if out is None else out  # overwritten
    if clip is None:
        call("cfd_energy_mean2d" + SFX[u.dtype], ptr(u), ptr(v), u.numel(), ptr(out), stream_handle(stream))
    else:
        call("cfd_energy_mean_clip2d" + SFX[u.dtype], ptr(u), ptr(v), u.numel(), ptr(out), float(clip[0]),
             float(clip[1]), stream_handle(stream))
    return out


def mean_inputs(n, dtype):
    return noise(n, dtype, seed=1, lo=0.0, hi=1.0), noise(n, dtype, seed=2)


def energy_inputs(n, dtype):
    return noise(n, dtype, seed=3, lo=-3.0, hi=3.0), noise(n, dtype, seed=4, lo=-3.0, hi=3.0)


def check_mean(got, a, scale_of=None):
    want = mean64_exact(a)
    scale = want if scale_of is None else mean64_exact(scale_of)
    print(f"mean n={a.size} {a.dtype}: got {got!r} want {want!r} |diff| {abs(got - want):.3e} "
          f"bound {(a.size + 2) * EPS * scale:.3e}")
    assert scale > 0 and abs(got - want) <= (a.size + 2) * EPS * scale, (got, want)


def check_energy(got, u, v):
    want = energy_mean_exact(u, v)
    print(f"energy n={u.size} {u.dtype}: got {got!r} want {want!r} |diff| {abs(got - want):.3e} "
          f"bound {(u.size + 2) * EPS * want:.3e}")
    assert want > 0 and abs(got - want) <= (u.size + 2) * EPS * want, (got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_mean(n, dtype):
    pos, signed = mean_inputs(n, dtype)
    for a, scale_of in ((pos, None), (signed, np.abs(signed))):
        d = dev(a)
        first = mean(d)
        check_mean(float(host(first)[0]), a, scale_of)
        assert bits(host(mean(d, out=scalar(torch.float64, 3.0)))) == bits(host(first))  # the same bits again


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_energy_mean(n, dtype):
    u, v = energy_inputs(n, dtype)
    ud, vd = dev(u), dev(v)
    first = host(energy(ud, vd))
    check_energy(float(first[0]), u, v)
    again = host(energy(ud, vd, out=scalar(torch.float64, 3.0)))
    check_energy(float(again[0]), u, v)
    if n <= ENERGY_ONE_PASS:  # past it the partial sums meet in atomics: no order promised
        assert bits(again) == bits(first)
    assert np.array_equal(host(ud), u) and np.array_equal(host(vd), v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_energy_mean_clip(n, dtype):
    """The energy is of the unclipped fields; the stored fields are np.clip's,
    a NaN passing through; a NaN cell makes the energy NaN.  Past 2^20 cells
    the call is three launches."""
    T = dtype
    lo, hi = T(-1.5), T(1.5)
    u, v = energy_inputs(n, dtype)
    assert n < 8 or ((np.abs(u) > 1.5).any() and (np.abs(u) < 1.5).any())
    ud, vd = dev(u), dev(v)
    first = host(energy(ud, vd, clip=(lo, hi)))
    check_energy(float(first[0]), u, v)
    assert bits(host(ud)) == bits(np.clip(u, lo, hi)) and bits(host(vd)) == bits(np.clip(v, lo, hi))
    if n <= ENERGY_ONE_PASS:
        assert bits(host(energy(dev(u), dev(v), clip=(lo, hi)))) == bits(first)
    u2, v2 = np.array(u), np.array(v)
    u2[n // 2] = np.nan
    v2[n - 1] = np.nan
    ud, vd = dev(u2), dev(v2)
    assert np.isnan(host(energy(ud, vd, clip=(lo, hi)))[0]) and np.isnan(energy_mean_exact(u2, v2))
    gu, gv = host(ud), host(vd)
    assert np.isnan(gu[n // 2]) and np.isnan(gv[n - 1])
    assert np.array_equal(gu, np.clip(u2, lo, hi), equal_nan=True)
    assert np.array_equal(gv, np.clip(v2, lo, hi), equal_nan=True)


# ---------------------------------------------------------- shared scratch
def test_scratch_back_to_back_kernels():
    """cfd_mean_* and cfd_energy_mean*2d_* of both types share one ticket word
    and one set of partials per stream: run in sequence with different n, each
    is right, and right again on a second round (the word is back at zero)."""
    n1, n2, n3, n4 = 65, 77001, 1000, 300007
    a32, _ = mean_inputs(n1, np.float32)
    u32, v32 = energy_inputs(n2, np.float32)
    u64, v64 = energy_inputs(n3, np.float64)
    a64, _ = mean_inputs(n4, np.float64)
    rounds = []
    for _ in range(2):
        ins = [dev(x) for x in (a32, u32, v32, u64, v64, a64)]
        outs = [mean(ins[0]), energy(ins[1], ins[2]), energy(ins[3], ins[4], clip=(-1.5, 1.5)), mean(ins[5])]
        got = [float(host(o)[0]) for o in outs]
        check_mean(got[0], a32)
        check_energy(got[1], u32, v32)
        check_energy(got[2], u64, v64)
        check_mean(got[3], a64)
        assert bits(host(ins[3])) == bits(np.clip(u64, -1.5, 1.5))
        rounds.append(got)
    assert rounds[0] == rounds[1]


def test_scratch_two_streams():
    """Each stream has its own scratch: eight calls per stream, interleaved on
    two non-default streams, give the bits of the same calls run alone."""
    kinds = ["mean32", "energy32", "mean64", "energy64"] * 2
    sizes = [[65, 77001, 1000, 300007, ENERGY_ONE_PASS, 257, 70000, 5000],
             [300001, 64, ENERGY_ONE_PASS, 999, 12345, 77003, 256, 1 << 19]]

    def inputs(kind, n):
        dtype = np.float32 if kind.endswith("32") else np.float64
        return mean_inputs(n, dtype)[1:] if kind.startswith("mean") else energy_inputs(n, dtype)

    def run(kind, ins, out, stream=None):
        return mean(ins[0], out, stream) if kind.startswith("mean") else energy(ins[0], ins[1], out, None, stream)

    hins = [[inputs(k, n) for k, n in zip(kinds, ns)] for ns in sizes]
    ins = [[[dev(x) for x in xs] for xs in row] for row in hins]
    alone = [[host(run(k, x, None)) for k, x in zip(kinds, xs)] for xs in ins]
    for s in (0, 1):  # the single-stream results are right to begin with
        for kind, xs, got in zip(kinds, hins[s], alone[s]):
            if kind.startswith("mean"):
                check_mean(float(got[0]), xs[0], np.abs(xs[0]))
            else:
                check_energy(float(got[0]), *xs)
    outs = [[scalar(torch.float64, float("nan")) for _ in kinds] for _ in sizes]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream and all(s.cuda_stream != 0 for s in streams)
    torch.cuda.synchronize()  # the inputs and the presets are in place
    for k, kind in enumerate(kinds):
        for s in (0, 1):
            run(kind, ins[s][k], outs[s][k], streams[s])
    torch.cuda.synchronize()  # ins and outs stay referenced up to here
    for s in (0, 1):
        for k in range(len(kinds)):
            assert bits(host(outs[s][k])) == bits(alone[s][k]), (s, k, kinds[k], sizes[s][k])


# ---------------------------------------------------------- 2-D reductions
def targets(shape):
    """Where the reference's maximum is put in turn: the interior corners,
    and in the last interior row the columns on both sides of the first wave
    boundary and of the first workgroup boundary."""
    ny, nx = shape
    t = [(1, 1), (1, nx - 2), (ny - 2, 1), (ny - 2, nx - 2)]
    t += [(ny - 2, c) for c in (63, 64, 255, 256) if 1 <= c <= nx - 2]
    return list(dict.fromkeys(t))


def spiked(f, k, i, j):
    """f with a spike on the boundary row next to row i, in column j: the
    one cell of a central y-difference it enters is (i, j)."""
    ny = f.shape[0]
    assert i in (1, ny - 2)
    g = np.array(f)
    g[0 if i == 1 else ny - 1, j] += f.dtype.type((40 + k) * (-1) ** k)
    return g


def only_argmax(ref, i, j):
    """The reference's maximum and that it is attained at (i, j) alone."""
    m = fold_absmax(ref)
    assert np.flatnonzero(np.abs(ref) == m).tolist() == [i * ref.shape[1] + j], (i, j)
    return m


def vort_absmax32(u, v, mask, out=None):
    out = scalar(np.float32) if out is None else out
    ny, nx = u.shape
    call("cfd_vorticity_absmax2d_f32", ptr(u), ptr(v), ptr(mask), ny, nx, DX, DY, ptr(out), stream_handle())
    return out


def vort32(u, v, mask):
    w = torch.empty_like(u)
    ny, nx = u.shape
    call("cfd_vorticity2d_f32", ptr(u), ptr(v), ptr(mask), ptr(w), ny, nx, DX, DY, stream_handle())
    return w


def vort64(u, v, mask, want_w=True, out=None):
    w = torch.full_like(u, 7.0) if want_w else None
    ny, nx = u.shape
    call("cfd_vorticity2d_f64", ptr(u), ptr(v), ptr(mask), ptr(w), ptr(out), ny, nx, DX, DY, stream_handle())
    return w


def check_vorticity(u, v, mask, ref):
    """Every vorticity entry point of u's dtype against the reference field
    `ref` and the fold over it."""
    m = fold_absmax(ref)
    ud, vd = dev(u), dev(v)
    md = None if mask is None else dev(np.asarray(mask, np.uint8))
    if u.dtype == np.float32:
        w = host(vort32(ud, vd, md))
        assert np.array_equal(w, ref, equal_nan=True)
        got = host(vort_absmax32(ud, vd, md))[0]
        assert bits(got) == bits(m) == bits(fold_absmax(w))
    else:
        out = scalar(np.float64)
        w = vort64(ud, vd, md, True, out)  # w and absmax together
        assert np.array_equal(host(w), ref, equal_nan=True) and bits(host(out)[0]) == bits(m)
        out = scalar(np.float64)
        assert vort64(ud, vd, md, False, out) is None and bits(host(out)[0]) == bits(m)  # w = NULL
        assert np.array_equal(host(vort64(ud, vd, md, True, None)), ref, equal_nan=True)  # absmax = NULL
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", INTERIOR)
def test_divergence_absmax_positions(shape, dtype):
    u, v = fields2d(shape, dtype)
    cases = [(v, None)] + [(spiked(v, k, i, j), (i, j)) for k, (i, j) in enumerate(targets(shape))]
    for v2, at in cases:
        ref = divergence2d(u, v2, DX, DY)
        m = fold_absmax(ref) if at is None else only_argmax(ref, *at)
        assert m > 0
        out = scalar(dtype)
        d = K.compute_divergence_fast(dev(u), dev(v2), DX, DY, absmax=out)
        assert bits(host(out)[0]) == bits(m), at
        assert np.array_equal(host(d), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", INTERIOR)
def test_project_gradmax_positions(shape, dtype):
    us, vs = fields2d(shape, dtype)
    phi = noise(shape[0] * shape[1], dtype, seed=5).reshape(shape)
    cases = [(phi, None)] + [(spiked(phi, k, i, j), (i, j)) for k, (i, j) in enumerate(targets(shape))]
    for phi2, at in cases:
        ru, rv, m = project2d(phi2, us, vs, DX, DY, 2e-5)
        gx, gy = gradient2d(phi2, DX, DY)
        g = np.sqrt(gx * gx + gy * gy)
        assert m > 0 and bits(m) == bits(fold_absmax(g) if at is None else only_argmax(g, *at))
        out = scalar(dtype)
        gu, gv = K.project_velocity(dev(phi2), dev(us), dev(vs), DX, DY, 2e-5, gradmax=out)
        assert bits(host(out)[0]) == bits(m), at
        assert np.array_equal(host(gu), ru) and np.array_equal(host(gv), rv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", INTERIOR)
def test_vorticity_absmax_positions(shape, dtype):
    u, v = fields2d(shape, dtype)
    cases = [(u, None)] + [(spiked(u, k, i, j), (i, j)) for k, (i, j) in enumerate(targets(shape))]
    for u2, at in cases:
        ref = vorticity2d(u2, v, None, DX, DY)
        m = fold_absmax(ref) if at is None else only_argmax(ref, *at)
        assert m > 0 and check_vorticity(u2, v, None, ref) == m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", NO_INTERIOR)
def test_2d_reductions_without_interior(shape, dtype):
    """No interior cell: every maximum is 0 and a preset `out` is left alone
    (the fields are the references': zero divergence and vorticity, u = u*)."""
    u, v = fields2d(shape, dtype)
    phi = noise(shape[0] * shape[1], dtype, seed=5).reshape(shape)
    mask = np.random.default_rng(3).random(shape) < 0.4
    for preset in (0.0, 0.25):
        out = scalar(dtype, preset)
        d = K.compute_divergence_fast(dev(u), dev(v), DX, DY, absmax=out)
        assert bits(host(out)[0]) == bits(dtype(preset)) and np.array_equal(host(d), divergence2d(u, v, DX, DY))
        assert not host(d).any()
        out = scalar(dtype, preset)
        gu, gv = K.project_velocity(dev(phi), dev(u), dev(v), DX, DY, 2e-5, gradmax=out)
        ru, rv, m = project2d(phi, u, v, DX, DY, 2e-5)
        assert m == 0 and bits(host(out)[0]) == bits(dtype(preset))
        assert bits(host(gu)) == bits(ru) == bits(u) and bits(host(gv)) == bits(rv)
        for mk in (None, mask):
            ref = vorticity2d(u, v, mk, DX, DY)
            assert fold_absmax(ref) == 0
            md = None if mk is None else dev(mk.astype(np.uint8))
            out = scalar(dtype, preset)
            if dtype == np.float32:
                vort_absmax32(dev(u), dev(v), md, out)
                w = host(vort32(dev(u), dev(v), md))
            else:
                w = host(vort64(dev(u), dev(v), md, True, out))
            assert bits(host(out)[0]) == bits(dtype(preset))
            assert np.array_equal(w, ref, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", INTERIOR)
def test_vorticity_absmax_masks(shape, dtype):
    ny, nx = shape
    u, v = fields2d(shape, dtype)
    free = vorticity2d(u, v, None, DX, DY)
    top = fold_absmax(free)
    # a random mask (ring cells included)
    mask = np.random.default_rng(ny * nx).random(shape) < 0.3
    check_vorticity(u, v, mask, vorticity2d(u, v, mask, DX, DY))
    # the mask covers the maximum: the next-largest cell wins
    at = np.unravel_index(np.argmax(np.abs(free)), shape)
    mask = np.zeros(shape, bool)
    mask[at] = True
    ref = vorticity2d(u, v, mask, DX, DY)
    second = np.sort(np.abs(free).ravel())[-2]
    assert fold_absmax(ref) == second < top
    assert check_vorticity(u, v, mask, ref) == second
    # every interior cell masked: 0, and a preset stands
    mask = np.zeros(shape, bool)
    mask[1:-1, 1:-1] = True
    ref = vorticity2d(u, v, mask, DX, DY)
    assert check_vorticity(u, v, mask, ref) == 0 and np.isnan(ref[1:-1, 1:-1]).all()
    # a NaN input: the cells it enters have |w| = NaN and never win
    u2, v2 = np.array(u), np.array(v)
    u2[0, nx // 2] = np.nan  # enters w(1, nx // 2)
    v2[ny - 2, 0] = np.nan   # enters w(ny - 2, 1)
    ref = vorticity2d(u2, v2, None, DX, DY)
    assert np.isnan(ref[1, nx // 2]) and np.isnan(ref[ny - 2, 1])
    m = check_vorticity(u2, v2, None, ref)
    assert m == np.nanmax(np.abs(ref)) and (m > 0) == (np.isfinite(ref[1:-1, 1:-1]).any())
    # an Inf input does win
    u2 = np.array(u)
    u2[ny - 1, nx - 2] = -np.inf  # enters w(ny - 2, nx - 2) alone
    ref = vorticity2d(u2, v, None, DX, DY)
    assert np.isinf(ref[ny - 2, nx - 2]) and not np.isnan(ref).any()
    assert check_vorticity(u2, v, None, ref) == np.inf
