"""Histograms without a GPU (pc_hip_hist_*, POLYCAP_HIST): the per-entry value and bin of polycap_amd/csrc/hip/pc_hist.h, compiled
for the host, against a numpy restatement of the contract in include/polycap-hip.h bit for bit; the identity sum(bins) + outside ==
sum W in Python integers; pc_hip_hist_validate field by field; the quantile and FWHM helpers against pure-Python restatements; and
the public call's variable."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import EXAMPLE, ROOT
from tests.test_spot_cpu import np_exit_dz, np_q

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "hist")
QUANTITIES = ("x", "y", "r", "slope_x", "slope_y", "tan_theta", "nrefl", "dtravel", "r_start", "z")
USES_DZ = (0, 1, 2, 3, 4, 5)
EXIT_ONLY = (7, 8)
# columns of a synthetic entry
X, Y, Z, DX, DY, DZ, N, DT, SX, SY = range(10)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------
def np_value(q, E, leak, zp=0., cx=0., cy=0.):
    """(v, ok): the value of quantity q for entries E [n, 10], and False where the entry is outside whatever v is"""
    with np.errstate(all="ignore"):
        ok = np.ones(len(E), dtype=bool)
        if q in USES_DZ:
            ok = E[:, DZ] > 0.
        if q in EXIT_ONLY and leak:
            ok = np.zeros(len(E), dtype=bool)
        if q in (0, 1, 2):
            t = (zp - E[:, Z]) / E[:, DZ]
            if q == 0:
                v = E[:, X] + E[:, DX] * t
            elif q == 1:
                v = E[:, Y] + E[:, DY] * t
            else:
                a, b = (E[:, X] + E[:, DX] * t) - cx, (E[:, Y] + E[:, DY] * t) - cy
                v = np.sqrt(a * a + b * b)
        elif q == 3:
            v = E[:, DX] / E[:, DZ]
        elif q == 4:
            v = E[:, DY] / E[:, DZ]
        elif q == 5:
            v = np.sqrt(E[:, DX] * E[:, DX] + E[:, DY] * E[:, DY]) / E[:, DZ]
        elif q == 6:
            v = E[:, N].copy()
        elif q == 7:
            v = E[:, DT].copy()
        elif q == 8:
            v = np.sqrt(E[:, SX] * E[:, SX] + E[:, SY] * E[:, SY])
        else:
            v = E[:, Z].copy()
    return v, ok


def np_bins(v, ok, lo, hi, n_bins):
    """bin in [0, n_bins) or -1"""
    with np.errstate(all="ignore"):
        f = ((v - lo) / (hi - lo)) * float(n_bins)
        inside = ok & (f >= 0.) & (f < float(n_bins))
    b = np.full(len(v), -1, dtype=np.int64)
    b[inside] = np.floor(f[inside]).astype(np.int64)
    return b


def np_hist(bins, W, n_bins):
    """(uint64 [S, n_bins], uint64 [S]) from bins [n] and quantised weights W uint64 [n, S]; limbs of 16 bits keep float64 sums exact"""
    S = W.shape[1]
    H, out = np.zeros((S, n_bins), dtype=np.uint64), np.zeros(S, dtype=np.uint64)
    inside = bins >= 0
    for s in range(S):
        for limb in range(4):
            part = ((W[:, s] >> np.uint64(16 * limb)) & np.uint64(0xffff)).astype(np.float64)
            h = np.bincount(bins[inside], weights=part[inside], minlength=n_bins)          # < 2^16 * n <= 2^53: exact
            H[s] += h.astype(np.uint64) << np.uint64(16 * limb)
            out[s] += np.uint64(int(part[~inside].sum())) << np.uint64(16 * limb)
    return H, out


# ---- the host compile of pc_hist.h ----------------------------------------------------------------------------------------------
def build_hist_host(directory):
    so = os.path.join(str(directory), "hist_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "hist_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, u64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.hist_bins_n.restype = None
    L.hist_bins_n.argtypes = [C.c_int64, dp, C.c_int, C.c_int, dp, C.c_int, dp, i32p, i32p]
    L.hist_q_n.restype = None
    L.hist_q_n.argtypes = [C.c_int64, dp, u64p]
    L.hist_quantile.restype = C.c_double
    L.hist_quantile.argtypes = [C.c_int32, C.c_double, C.c_double, u64p, C.c_double]
    L.hist_fwhm.restype = C.c_double
    L.hist_fwhm.argtypes = [C.c_int32, C.c_double, C.c_double, u64p, dp, dp]
    return L


@pytest.fixture(scope="module")
def hist_host(tmp_path_factory):
    return build_hist_host(tmp_path_factory.mktemp("hist_host"))


def host_bins(L, E, leak, q, zp, cx, cy, lo, hi, n_bins):
    E = np.ascontiguousarray(E, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    axis = np.array([zp, cx, cy, lo, hi], dtype=np.float64)
    v, ok, b = np.zeros(len(E)), np.zeros(len(E), dtype=np.int32), np.zeros(len(E), dtype=np.int32)
    L.hist_bins_n(len(E), E.ctypes.data_as(dp), int(leak), q, axis.ctypes.data_as(dp), n_bins, v.ctypes.data_as(dp),
                  ok.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_int32)))
    return v, ok.astype(bool), b.astype(np.int64)


def synthetic(q, lo, hi, n_bins, n=100000, seed=7):
    """entries whose value of quantity q spreads over and beyond [lo, hi), then rows with v exactly on lo, on hi and on every
    interior edge (dz = 1 and no transverse direction: every formula then returns the planted number itself), NaN in every field,
    dz <= 0, and both zeros"""
    rng = np.random.default_rng(seed + q)
    E = np.zeros((n, 10))
    span = hi - lo
    E[:, X:Z] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (n, 2))
    E[:, Z] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, n)
    E[:, DX:DZ] = rng.normal(0., 0.3 * span, (n, 2)) * rng.choice([1e-3, 1.], (n, 1))
    E[:, DZ] = np.where(rng.random(n) < 0.5, np_exit_dz(np.clip(E[:, DX], -0.7, 0.7), np.clip(E[:, DY], -0.7, 0.7)), rng.uniform(-0.2, 1., n))
    E[:, N] = np.floor(rng.uniform(lo - 0.2 * span, hi + 0.2 * span, n))
    E[:, DT] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, n)
    E[:, SX:] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (n, 2)) * 0.7
    edges = [lo + span * k / n_bins for k in range(n_bins + 1)] + [0.0, -0.0, np.nextafter(lo, -np.inf), np.nextafter(hi, -np.inf)]
    field = {0: X, 1: X, 2: X, 3: DX, 4: DX, 5: DX, 6: N, 7: DT, 8: SX, 9: Z}[q]
    S = np.zeros((len(edges), 10))
    S[:, DZ] = 1.
    for k, v in enumerate(edges):
        S[k, field] = v
        if q == 1:
            S[k, Y] = v
        if q == 4:
            S[k, DY] = v
    nan_rows = np.tile(E[:10], (1, 1))
    for k in range(10):
        nan_rows[k, k] = np.nan
    bad_dz = E[10:16].copy()
    bad_dz[:, DZ] = [0., -0., -0.5, -1., np.inf, -np.inf]
    return np.concatenate([E, S, nan_rows, bad_dz])


AXES = [(-0.5, 1.5, 64), (0., 2., 1), (0., 256., 256), (-0.0123, 0.0457, 37)]


@pytest.mark.parametrize("q", range(10))
def test_value_and_bin_equal_the_contract(hist_host, q):
    for lo, hi, n_bins in AXES:
        E = synthetic(q, lo, hi, n_bins)
        zp, cx, cy = (0.7, 0.0, 0.0) if q != 2 else (0.7, 0.03, -0.02)
        for leak in (0, 1):
            v, ok, b = host_bins(hist_host, E, leak, q, zp, cx, cy, lo, hi, n_bins)
            v2, ok2 = np_value(q, E, leak, zp, cx, cy)
            b2 = np_bins(v2, ok2, lo, hi, n_bins)
            assert same_bits(v, v2), (QUANTITIES[q], lo, hi)
            assert np.array_equal(ok, ok2) and np.array_equal(b, b2), (QUANTITIES[q], lo, hi, leak)
            if q in EXIT_ONLY and leak:
                assert (b == -1).all()
            else:
                assert (b >= 0).sum() > 1000 or n_bins == 1
                assert (b == -1).sum() > 1000
    # the planted rows of the first axis: v exactly on lo, on every interior edge, on hi; then +0, -0
    lo, hi, n_bins = AXES[0]
    E = synthetic(q, lo, hi, n_bins)[100000:100000 + n_bins + 3]
    zp = 0.7 if q != 9 else 0.
    v, ok, b = host_bins(hist_host, E, 0, q, zp, 0., 0., lo, hi, n_bins)
    if q in (2, 5, 8):          # radii: |v|
        want = [k if k >= 16 else None for k in range(n_bins)] + [-1]
    else:
        want = list(range(n_bins)) + [-1]
    for k, w in enumerate(want):
        if w is not None:
            assert b[k] == w, (QUANTITIES[q], k)
    # negative zero on an axis that starts at 0 lands in bin 0
    lo, hi, n_bins = AXES[1]
    E = synthetic(q, lo, hi, n_bins)[100000 + n_bins + 1:100000 + n_bins + 3]
    v, ok, b = host_bins(hist_host, E, 0, q, 0., 0., 0., lo, hi, n_bins)
    # (x + dx*t with dx*t = +0 and the radii's square roots give +0; the other quantities keep the sign)
    assert b.tolist() == [0, 0] and (q in (0, 1, 2, 5, 8) or np.signbit(v[1]))


def test_weights_equal_the_spot_maps(hist_host):
    rng = np.random.default_rng(3)
    w = np.concatenate([rng.random(5000), [0., -0., -1., np.nan, 1., 0.5 * 2.0 ** -32, 1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, np.inf * 0]])
    q = np.zeros(len(w), dtype=np.uint64)
    hist_host.hist_q_n(len(w), w.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert np.array_equal(q, np_q(w))
    assert q[-4:-1].tolist() == [0, 2, 2]


def test_identity_in_python_integers(hist_host):
    """sum(bins) + outside == sum W for every axis and energy, on the host compile's bins, in Python integers"""
    rng = np.random.default_rng(11)
    for q in range(10):
        lo, hi, n_bins = AXES[q % len(AXES)]
        E = synthetic(q, lo, hi, n_bins, n=20000)
        Wf = rng.random((len(E), 3)) * rng.choice([0., 1e-6, 1.], (len(E), 1))
        Wf[::97, 1] = np.nan
        W = np_q(Wf)
        for leak in (0, 1):
            _, _, b = host_bins(hist_host, E, leak, q, 0.7, 0., 0., lo, hi, n_bins)
            H, out = np_hist(b, W, n_bins)
            for s in range(3):
                bins = [0] * n_bins
                outside = 0
                for i in range(len(E)):
                    if b[i] >= 0:
                        bins[b[i]] += int(W[i, s])
                    else:
                        outside += int(W[i, s])
                assert sum(bins) + outside == sum(int(x) for x in W[:, s])
                assert [int(x) for x in H[s]] == bins and int(out[s]) == outside       # the numpy sums the GPU tests use
            if q in EXIT_ONLY and leak:
                assert not H.any()


# ---- pc_hip_hist_validate -------------------------------------------------------------------------------------------------------
def _validate(axes, energies=None, regime=0, ne=16, n_axes=None):
    from polycap_amd import _cabi
    from polycap_amd.hip import hist_axes
    L = _cabi.lib()
    arr = hist_axes(axes)
    e = None if energies is None else np.ascontiguousarray(energies, dtype=np.int32)
    spec = _cabi.HistSpecS(len(axes) if n_axes is None else n_axes, arr, 0 if e is None else len(e),
                           None if e is None else e.ctypes.data_as(C.POINTER(C.c_int32)), regime)
    st = L.pc_hip_hist_validate(C.byref(spec), ne)
    return st, (L.pc_hip_last_error() or b"").decode()


GOOD = dict(axis="x", d=0.5, range=(-0.01, 0.01), bins=2048)


def test_validate_accepts():
    assert _validate([GOOD])[0] == 0
    assert _validate([GOOD, dict(axis="r", d=0.5, centre=(0.001, -0.002), range=(0, 0.02), bins=1024),
                      dict(axis="nrefl", range=(0, 256), bins=256)], energies=[5, 0, 15])[0] == 0
    assert _validate([dict(axis=QUANTITIES[k % 10], range=(0, 1), bins=1) for k in range(16)], regime=2)[0] == 0
    # the limit: (sum n_bins) * n_selected == 2^24 exactly
    assert _validate([dict(axis="x", range=(0, 1), bins=1 << 19), dict(axis="z", range=(0, 1), bins=1 << 19)], ne=16)[0] == 0
    assert _validate([dict(axis="x", range=(0, 1), bins=1 << 24)], energies=[3], ne=16)[0] == 0


@pytest.mark.parametrize("axes,kw,field", [
    ([], {}, "n_axes"),
    ([dict(axis="z", range=(0, 1), bins=1)] * 17, {}, "n_axes"),
    ([dict(GOOD, axis=10)], {}, "quantity"),
    ([dict(GOOD, axis=-1)], {}, "quantity"),
    ([dict(GOOD, range=(0.01, 0.01))], {}, "lo"),
    ([dict(GOOD, range=(0.02, 0.01))], {}, "lo"),
    ([dict(GOOD, range=(float("nan"), 0.01))], {}, "lo"),
    ([dict(GOOD, range=(0., float("inf")))], {}, "hi"),
    ([dict(GOOD, bins=0)], {}, "n_bins"),
    ([dict(GOOD, bins=-3)], {}, "n_bins"),
    ([dict(GOOD, d=-0.1)], {}, " d "),
    ([dict(GOOD, d=float("nan"))], {}, " d "),
    ([dict(GOOD, d=float("inf"))], {}, " d "),
    ([dict(axis="slope_x", d=0.5, range=(0, 1), bins=4)], {}, " d "),
    ([dict(axis="nrefl", d=1e-9, range=(0, 1), bins=4)], {}, " d "),
    ([dict(GOOD, centre=(0.001, 0.))], {}, "cx"),
    ([dict(axis="y", d=0.5, centre=(0., 0.001), range=(0, 1), bins=4)], {}, "cy"),
    ([dict(axis="r", centre=(float("nan"), 0.), range=(0, 1), bins=4)], {}, "cx"),
    ([dict(axis="r", centre=(0., float("inf")), range=(0, 1), bins=4)], {}, "cy"),
    ([GOOD], dict(energies=[16]), "energies"),
    ([GOOD], dict(energies=[-1]), "energies"),
    ([GOOD], dict(energies=[3, 3]), "energies"),
    ([GOOD], dict(energies=list(range(16)) + [0]), "n_energies"),
    ([GOOD], dict(regime=3), "regime"),
    ([GOOD], dict(regime=-1), "regime"),
    ([dict(axis="x", range=(0, 1), bins=(1 << 20) + 1)], {}, "n_bins"),
    ([dict(axis="x", range=(0, 1), bins=1 << 19), dict(axis="z", range=(0, 1), bins=(1 << 19) + 1)], {}, "n_bins"),
])
def test_validate_refuses_and_names_the_field(axes, kw, field):
    st, msg = _validate(axes, **kw)
    assert st == -2, (axes, kw)
    assert msg.startswith("pc_hip_hist_validate") and field in msg, msg


def test_validate_refuses_null():
    from polycap_amd import _cabi
    L = _cabi.lib()
    assert L.pc_hip_hist_validate(None, 4) == -2
    spec = _cabi.HistSpecS(1, None, 0, None, 0)
    assert L.pc_hip_hist_validate(C.byref(spec), 4) == -2 and b"n_axes" in L.pc_hip_last_error()


# ---- quantile and FWHM ----------------------------------------------------------------------------------------------------------
def py_quantile(bins, lo, hi, q):
    n = len(bins)
    total = sum(bins)
    if total == 0 or not (0. <= q <= 1.):
        return math.nan
    target = q * float(total)
    before = 0
    for b in range(n):
        upto = before + bins[b]
        if bins[b] != 0 and float(upto) >= target:
            frac = (target - float(before)) / float(bins[b])
            return lo + ((float(b) + frac) / float(n)) * (hi - lo)
        before = upto
    return hi


def py_fwhm(bins, lo, hi):
    n = len(bins)
    nan3 = (math.nan, math.nan, math.nan)
    peak = bins.index(max(bins))            # the first bin of maximal count
    if bins[peak] == 0:
        return nan3
    half = float(bins[peak]) / 2.0
    i, j = peak - 1, peak + 1
    while i >= 0 and not float(bins[i]) < half:
        i -= 1
    while j < n and not float(bins[j]) < half:
        j += 1
    if i < 0 or j >= n:
        return nan3
    c = lambda b: lo + ((float(b) + 0.5) / float(n)) * (hi - lo)
    left = c(i) + (c(i + 1) - c(i)) * ((half - float(bins[i])) / (float(bins[i + 1]) - float(bins[i])))
    right = c(j) + (c(j - 1) - c(j)) * ((half - float(bins[j])) / (float(bins[j - 1]) - float(bins[j])))
    return right - left, left, right


def _helpers():
    from polycap_amd.hip import hist_fwhm, hist_quantile
    return hist_fwhm, hist_quantile


def _cases():
    rng = np.random.default_rng(5)
    cases = []
    for n in (2, 3, 7, 64, 2048):
        x = (np.arange(n) + 0.5) / n
        for width in (0.02, 0.1, 0.4):
            for centre in (0.5, 0.31, 0.02, 0.99):
                shape = np.exp(-0.5 * ((x - centre) / width) ** 2) + 0.02 * rng.random(n)
                cases.append([int(v) for v in (shape * rng.choice([50., 2.0 ** 40, 2.0 ** 61 / n])).astype(np.uint64)])
    cases += [[0] * 5, [7], [0], [9, 1, 0], [0, 1, 9], [1, 9, 9, 1], [3, 9, 2, 9, 3], [0, 4, 8, 4, 0], [5, 5, 5, 5], [1, 2, 4, 2, 1],
              [0, 0, 1 << 63, 0], [(1 << 63) - 1, 1 << 63, 1], [2, 4, 4, 4, 1]]
    return cases


def test_fwhm_equals_the_formula(hist_host):
    hist_fwhm, _ = _helpers()
    dp = C.POINTER(C.c_double)
    for bins in _cases():
        for lo, hi in ((-0.01, 0.01), (0., 256.), (3.5, 3.75)):
            want = py_fwhm(bins, lo, hi)
            got = hist_fwhm(np.array(bins, dtype=np.uint64), lo, hi)
            assert same_bits(got, want), (bins[:8], lo, hi, got, want)
            b = np.array(bins, dtype=np.uint64)
            l, r = C.c_double(0.), C.c_double(0.)
            w = hist_host.hist_fwhm(len(bins), lo, hi, b.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(l), C.byref(r))
            assert same_bits([w, l.value, r.value], want)
    nan = lambda b: all(math.isnan(v) for v in hist_fwhm(np.array(b, dtype=np.uint64), 0., 1.))
    assert nan([0] * 5) and nan([7]) and nan([9, 1, 0]) and nan([0, 1, 9]) and nan([5, 5, 5, 5])      # empty, one bin, peaks at an edge
    # two equal maxima: the first one is the peak, and the walk to the right passes the second
    w, l, r = hist_fwhm(np.array([3, 9, 2, 9, 3], dtype=np.uint64), 0., 5.)
    assert same_bits([w, l, r], py_fwhm([3, 9, 2, 9, 3], 0., 5.)) and 0.5 < l < 1.5 and 1.5 < r < 2.5
    w, l, r = hist_fwhm(np.array([0, 4, 8, 4, 0], dtype=np.uint64), 0., 5.)
    assert (w, l, r) == (3.0, 1.0, 4.0) or same_bits([w, l, r], py_fwhm([0, 4, 8, 4, 0], 0., 5.))


def test_quantile_equals_the_formula(hist_host):
    _, hist_quantile = _helpers()
    for bins in _cases():
        if sum(bins) >= 1 << 64:
            continue
        b = np.array(bins, dtype=np.uint64)
        for lo, hi in ((-0.01, 0.01), (0., 0.02)):
            for q in (0., 1e-9, 0.1, 0.5, 0.8, 0.9, 1. - 2.0 ** -53, 1., -0.1, 1.1, math.nan):
                want = py_quantile(bins, lo, hi, q)
                assert same_bits(hist_quantile(b, lo, hi, q, outside=12345), want), (bins[:8], lo, hi, q)
                assert same_bits(hist_host.hist_quantile(len(bins), lo, hi, b.ctypes.data_as(C.POINTER(C.c_uint64)), q), want)
    assert math.isnan(hist_quantile(np.zeros(5, dtype=np.uint64), 0., 1., 0.5))
    assert math.isnan(hist_quantile(np.zeros(5, dtype=np.uint64), 0., 1., 0.5, outside=100))        # the inside weight only
    assert hist_quantile(np.array([7], dtype=np.uint64), 0., 2., 0.5) == 1.0
    assert hist_quantile(np.array([1, 1, 1, 1], dtype=np.uint64), 0., 4., 0.5) == 2.0
    assert hist_quantile(np.array([0, 0, 4, 0], dtype=np.uint64), 0., 4., 0.) == 2.0
    assert hist_quantile(np.array([0, 0, 4, 0], dtype=np.uint64), 0., 4., 1.) == 3.0


# ---- the Python axes ------------------------------------------------------------------------------------------------------------
def test_axes_from_dicts_and_tuples():
    from polycap_amd.hip import hist_axes
    a = hist_axes([dict(axis="r", d=0.5, centre=(0.1, 0.2), range=(0, 0.02), bins=1024), ("nrefl", (0, 256), 256), ("x", (-1, 1), 8, 0.25), (9, (0, 5), 3)])
    got = [(x.quantity, x.d, x.cx, x.cy, x.lo, x.hi, x.n_bins) for x in a]
    assert got == [(2, 0.5, 0.1, 0.2, 0., 0.02, 1024), (6, 0., 0., 0., 0., 256., 256), (0, 0.25, 0., 0., -1., 1., 8), (9, 0., 0., 0., 0., 5., 3)]
    with pytest.raises(ValueError):
        hist_axes([dict(axis="x", range=(0, 1), bins=4, window=3)])
    with pytest.raises(ValueError):
        hist_axes([dict(axis="radius", range=(0, 1), bins=4)])


# ---- the public call's variable -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,what", [
    ("", "axis"),
    ("energies=all", "axis"),
    ("axis=q,range=0:1,bins=4", "axis must be one of"),
    ("axis=x,range=0:1", "range and bins"),
    ("axis=x,bins=4", "range and bins"),
    ("axis=x,range=0,1,bins=4", "range"),
    ("axis=x,range=0:1:2,bins=4", "range"),
    ("axis=x,range=1:0,bins=4", "lo"),
    ("axis=x,range=0:1,bins=0", "n_bins"),
    ("axis=x,range=0:1,bins=four", "bins"),
    ("axis=x,d=-1,range=0:1,bins=4", " d "),
    ("axis=nrefl,d=0.5,range=0:256,bins=256", " d "),
    ("axis=x,centre=0.1:0,range=0:1,bins=4", "cx"),
    ("axis=r,centre=0.1,range=0:1,bins=4", "centre"),
    ("axis=x,range=0:1,bins=4,width=3", "unknown key"),
    ("axis=x,range=0:1,bins=4;window=1", "every item"),
    ("axis=x,range=0:1,bins=4;energies=", "energies"),
    ("axis=x,range=0:1,bins=4;energies=0,x", "energies"),
    ("axis=x,range=0:1,bins=4;energies=291", "energies"),
    ("axis=x,range=0:1,bins=4;energies=1,1", "energies"),
    ("axis=x,range=0:1,bins=65536", "n_bins"),
    (";".join(["axis=z,range=0:1,bins=2"] * 17), "16 axes"),
])
def test_public_call_rejects_bad_hist_variable(value, what, monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_HIST", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_HIST") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert what in str(e.value), str(e.value)


def test_public_call_rejects_bad_share_with_hist(monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_HIST", "axis=x,d=0.5,range=-0.01:0.01,bins=2048")
    monkeypatch.setenv("POLYCAP_SPOT_SHARE", "1.5")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SPOT_SHARE"):
        src.get_transmission_efficiencies(1, 1000)


def test_public_call_with_hist_needs_a_device(monkeypatch):
    import polycap_amd
    from polycap_amd import capi
    if polycap_amd.device_count() > 0:
        return
    monkeypatch.setenv("POLYCAP_HIST", "axis=x,d=0.5,range=-0.01:0.01,bins=2048;axis=r,d=0.5,centre=0:0,range=0:0.02,bins=1024;"
                                       "axis=nrefl,range=0:256,bins=256;energies=all")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(RuntimeError, match="HIP"):
        src.get_transmission_efficiencies(1, 1000)


def test_hist_getter_fails_without_the_variable():
    """a result made elsewhere (from totals) carries no histograms: the getter says which variable was missing"""
    from polycap_amd import capi
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.full(291, 0.5), [10, 5, 3, 40, 0, 0])
    with pytest.raises(ValueError, match="POLYCAP_HIST"):
        eff.hist("exit")
