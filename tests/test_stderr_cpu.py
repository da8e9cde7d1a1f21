"""Standard errors without a GPU: pc_hip_efficiency_stderr against exact rational arithmetic on constructed moments, the
quantisation of the squared weights (pc_moments.h compiled for the host) against numpy, and the validation of POLYCAP_STDERR by
the public call before any device is used."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.conftest import EXAMPLE, ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
S = 2 ** 62


def split(v):
    """128-bit integer -> (lo, hi)"""
    assert 0 <= v < 2 ** 128
    return v & (2 ** 64 - 1), v >> 64


def stderr_c(A, B, counters):
    """pc_hip_efficiency_stderr on integer sums A, B (lists, one per energy)"""
    import polycap_amd
    a = np.array([x for v in A for x in split(v)], dtype=np.uint64)
    b = np.array([x for v in B for x in split(v)], dtype=np.uint64)
    return polycap_amd.efficiency_stderr(a, b, counters)


def stderr_exact(A, B, N):
    """the contract in exact arithmetic: variance max(0, q - m^2) / (N - 1) as a Fraction, or None for N < 2"""
    if N < 2:
        return None
    m = Fraction(A, N * S)
    q = Fraction(B, N * S)
    v = q - m * m
    return max(v, Fraction(0)) / (N - 1), q


def quantise(ws):
    """the sums the kernels make of a list of exit weights, with Python ints: A = sum int(w 2^62), B = sum int((w*w) 2^62)"""
    A = sum(int(w * 2.0 ** 62) for w in ws)
    B = sum(int((w * w) * 2.0 ** 62) for w in ws)
    return A, B


def check(A, B, counters):
    N = int(counters[0] + counters[1] + counters[2])
    got = stderr_c(A, B, counters)
    for e in range(len(A)):
        ex = stderr_exact(A[e], B[e], N)
        if ex is None:
            assert math.isnan(got[e])
            continue
        var, q = ex
        assert got[e] >= 0.0 and not math.isnan(got[e])
        # long double carries 64 bits: q - m^2 is good to a few units of 2^-64 of q, then one division and a square root
        tol = Fraction(8, 2 ** 64) * q / (N - 1)
        assert abs(Fraction(got[e]) ** 2 - var) <= tol + Fraction(got[e]) ** 2 * Fraction(1, 2 ** 50), (e, got[e], float(var))
    return got


def test_n_below_two_is_nan():
    A, B = quantise([0.5])
    got = check([A], [B], [1, 0, 0, 0, 0, 1])
    assert math.isnan(got[0])
    got = check([0], [0], [0, 0, 0, 0, 0, 0])
    assert math.isnan(got[0])
    # one started photon that was not transmitted: still N = 1
    assert math.isnan(stderr_c([0], [0], [0, 0, 1, 0, 0, 1])[0])


def test_all_weights_zero():
    got = check([0, 0], [0, 0], [0, 700, 300, 0, 0, 1000])
    assert np.array_equal(got, [0.0, 0.0])
    got = check([0], [0], [2, 0, 0, 0, 0, 2])          # two exit photons of weight 0
    assert got[0] == 0.0


@pytest.mark.parametrize("w", [1.0, 0.5, 0.75, 2.0 ** -20, 0.3, 0.123456789, 1.0 - 2.0 ** -53])
def test_all_weights_equal(w):
    """every started photon exits with the same weight: no spread.  Exactly 0 whenever w and w*w quantise without remainder; for the
    others the rounding of w*w (half an ulp, up to w^2 2^-53) and the truncations (2^-62 each) leave a residue in q - m^2 that is
    clamped at 0 or passed on: never negative and never NaN"""
    n = 1000
    A, B = quantise([w] * n)
    got = check([A], [B], [n, 0, 0, 0, 0, n])
    assert got[0] >= 0.0 and not math.isnan(got[0])
    if w in (1.0, 0.5, 0.75, 2.0 ** -20):
        assert got[0] == 0.0
    else:
        assert got[0] <= math.sqrt((2.0 ** -61 + w * w * 2.0 ** -53) / (n - 1))


def test_bernoulli_matches_textbook():
    """weights 1 for k of N photons: stderr = sqrt(p (1 - p) / (N - 1)) with p = k / N"""
    for N, k in ((10, 3), (1000, 1), (10 ** 6, 123456), (2, 1)):
        got = check([k * S], [k * S], [k, N - k, 0, 0, 0, N])
        p = k / N
        assert got[0] == pytest.approx(math.sqrt(p * (1 - p) / (N - 1)), rel=1e-15)


def test_random_weights_against_fractions():
    rng = np.random.default_rng(11)
    ws = list(rng.random(3000) ** 3)
    A, B = quantise(ws)
    n_ne, n_nt = 4000, 2000
    N = len(ws) + n_ne + n_nt
    got = check([A], [B], [len(ws), n_ne, n_nt, 0, 0, N])
    # and the textbook estimator on the doubles themselves (the quantisation moves it by ~2^-62)
    x = np.concatenate([np.array(ws), np.zeros(n_ne + n_nt)])
    assert got[0] == pytest.approx(math.sqrt(x.var(ddof=0) / (N - 1)), rel=1e-9)


def test_sums_near_two_to_the_hundred():
    """N ~ 2^32 photons with weights near 1: A and B near 2^94 .. 2^100, where the hi words carry most of the value"""
    N = 2 ** 32 + 12345
    k = 2 ** 32 - 999                                     # exit photons
    for wa, wb in ((1.0, 1.0), (0.9375, 0.87890625), (0.7, 0.49)):
        A = k * int(wa * 2.0 ** 62)
        B = k * int(wb * 2.0 ** 62)
        assert A >= 2 ** 93
        check([A], [B], [k, N - k, 0, 0, 0, N])
    # the largest sums the 128-bit counters can hold at N = 2^36 photons of weight 1
    N = 2 ** 36
    check([N * S - 1], [N * S - 1], [N, 0, 0, 0, 0, N])
    A = 2 ** 100 + 2 ** 70 + 12345
    B = 2 ** 99 + 987654321
    check([A, B], [B, B], [2 ** 38, 2 ** 38, 0, 0, 0, 2 ** 39])


def test_python_wrapper_shapes():
    import polycap_amd
    A, B = quantise([0.25, 0.5])
    a = np.array(split(A), dtype=np.uint64).reshape(1, 2)
    b = np.array(split(B), dtype=np.uint64).reshape(1, 2)
    r1 = polycap_amd.efficiency_stderr(a, b, [2, 2, 0, 0, 0, 4])
    r2 = polycap_amd.efficiency_stderr(a.reshape(-1), b.reshape(-1), np.array([2, 2, 0], dtype=np.int64))
    assert r1.shape == (1,) and np.array_equal(r1, r2)
    with pytest.raises(ValueError):
        polycap_amd.efficiency_stderr(a, np.zeros(4, dtype=np.uint64), [2, 2, 0, 0, 0, 4])


@pytest.fixture(scope="module")
def moments_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments_host")
    src = d / "moments_host.cpp"
    src.write_text('#include "pc_moments.h"\n'
                   'extern "C" unsigned long long fix_sq(double w) { return pc_fix_sq(w); }\n')
    so = d / "moments_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.fix_sq.restype = C.c_ulonglong
    L.fix_sq.argtypes = [C.c_double]
    return L


def np_fix_sq(w):
    w = np.asarray(w, dtype=np.float64)
    return ((w * w) * np.float64(2.0 ** 62)).astype(np.uint64)


def test_squared_weight_quantisation(moments_host):
    t = 2.0 ** -31
    sub = np.nextafter(0.0, 1.0)
    ws = [0.0, 1.0, t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), sub, 2.0 ** -1030, 2.0 ** -1022, 1e-20,
          0.5, 0.1, 1.0 / 3.0, np.nextafter(1.0, 0.0), 0.7071067811865476, 0.999999999]
    # values where w*w rounds: the product of the doubles is not representable
    rng = np.random.default_rng(5)
    ws += list(rng.random(200))
    ws = np.array(ws)
    got = np.array([moments_host.fix_sq(float(w)) for w in ws], dtype=np.uint64)
    want = np_fix_sq(ws)
    assert np.array_equal(got, want)
    # Python's own arithmetic agrees (what the GPU tests sum with)
    assert all(int(g) == int((float(w) * float(w)) * 2.0 ** 62) for g, w in zip(got, ws))
    assert got[1] == 2 ** 62 and got[2] == 1 and got[3] == 0 and got[4] == 1 and got[5] == 0 and got[0] == 0
    rounds = [w for w in ws if Fraction(float(w)) ** 2 != Fraction(float(w) * float(w))]
    assert len(rounds) > 100


BAD = ["2", "yes", "", "01", " 1", "1.0", "-1", "on"]


@pytest.mark.parametrize("value", BAD)
def test_public_call_rejects_bad_stderr_value(value, monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_STDERR", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_STDERR"):
        src.get_transmission_efficiencies(1, 1000)


def test_public_call_with_valid_stderr_needs_a_device(monkeypatch):
    import polycap_amd
    from polycap_amd import capi
    if polycap_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    for v in ("0", "1"):
        monkeypatch.setenv("POLYCAP_STDERR", v)
        src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
        with pytest.raises(RuntimeError, match="HIP"):
            src.get_transmission_efficiencies(1, 1000)


def test_getters_fail_on_a_result_without_stderr():
    """a result made without POLYCAP_STDERR (here: from totals, no device needed) has neither standard errors nor moments"""
    from polycap_amd import capi
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.array([0.5]), np.array([1, 1, 0, 0, 0, 2], dtype=np.int64))
    with pytest.raises(ValueError, match="POLYCAP_STDERR"):
        eff.efficiency_stderr()
    with pytest.raises(ValueError, match="POLYCAP_STDERR"):
        eff.moments()
