"""Relays without a GPU: the per-photon arithmetic of pc_relay.h, compiled for the host (tests/relay/relay_host.cpp), against a numpy
restatement of the contract in include/polycap-hip.h, bit for bit; the placement check; the efficiency and standard-error host
functions against exact Python arithmetic; and the exported symbols."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.conftest import ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "relay")
NEW_SYMBOLS = ("pc_hip_relay_efficiencies", "pc_hip_relay_run", "pc_hip_relay_totals", "pc_hip_relay_validate")


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def np_fly(x, y, dx, dy, ex, ey, gap, off_x, off_y):
    """[n, 10] = start (3), direction (3), electric vector (3), flight t: every operation one IEEE fp64 numpy operation"""
    f = np.float64
    with np.errstate(all="ignore"):
        dz = np.sqrt((f(1.) - dx * dx) - dy * dy)
        ez = -(ex * dx + ey * dy) / dz
        t = f(gap) / dz
        sx = (x + dx * t) - f(off_x)
        sy = (y + dy * t) - f(off_y)
    return np.stack([sx, sy, np.zeros_like(sx), dx, dy, dz, ex, ey, ez, t], axis=1)


def np_valid(exit_z, w0):
    return (exit_z > 0.) & (w0 > 0.)


def py_fix(w):
    return int(np.float64(w) * np.float64(2.0 ** 62))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))


# ---- the host compile of pc_relay.h ---------------------------------------------------------------------------------------------
def build_relay_host(directory):
    so = os.path.join(str(directory), "relay_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "relay_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, i64, u64p = C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_uint64)
    L.relay_fly_n.restype = None
    L.relay_fly_n.argtypes = [i64, dp, C.c_double, C.c_double, C.c_double, dp]
    L.relay_valid_n.restype = None
    L.relay_valid_n.argtypes = [i64, dp, dp, C.POINTER(C.c_int32)]
    L.relay_finish_n.restype = None
    L.relay_finish_n.argtypes = [i64, dp, dp, dp, u64p, u64p]
    L.relay_dtravel_n.restype = None
    L.relay_dtravel_n.argtypes = [i64, dp, dp, dp, dp]
    L.relay_placement_ok.restype = C.c_int
    L.relay_placement_ok.argtypes = [C.c_double] * 3
    L.relay_efficiency.restype = C.c_double
    L.relay_efficiency.argtypes = [C.c_uint64, C.c_uint64, C.c_int64]
    return L


def host_fly(L, six, gap, off_x, off_y):
    """six [n, 6] = x, y, dx, dy, ex, ey -> [n, 10]"""
    a = np.ascontiguousarray(six, dtype=np.float64)
    out = np.zeros((a.shape[0], 10))
    L.relay_fly_n(a.shape[0], a.ctypes.data_as(C.POINTER(C.c_double)), gap, off_x, off_y, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


@pytest.fixture(scope="module")
def relay_host(tmp_path_factory):
    return build_relay_host(tmp_path_factory.mktemp("relay_host"))


def _records(n, rng):
    """x, y, dx, dy, ex, ey of exit-like records, with the edge cases the contract has to survive"""
    a = np.zeros((n, 6))
    a[:, 0:2] = rng.normal(0., 0.05, (n, 2))
    a[:, 2:4] = rng.normal(0., 0.02, (n, 2))
    a[:, 4:6] = rng.integers(-1, 2, (n, 2)).astype(np.float64)          # the records hold rounded components
    k = n // 10
    ang = rng.uniform(0., 2. * np.pi, k)                                    # dz near 0, on both sides of it (NaN beyond)
    r = 1. + rng.choice([-1., 1.], k) * 10. ** rng.uniform(-17., -3., k)
    a[:k, 2], a[:k, 3] = r * np.cos(ang), r * np.sin(ang)
    a[k:2 * k] = 0.                                                         # zeroed records (failed slots)
    a[2 * k:3 * k, 4:6] = rng.normal(0., 1., (k, 2))                        # any electric vector
    return a


def test_fly_is_the_contract_bit_for_bit(relay_host):
    rng = np.random.default_rng(20240)
    a = _records(120000, rng)
    for gap, ox, oy in ((1.0, 0., 0.), (0., 0., 0.), (1.0, 0.002, -0.01), (0.8, 0.01, 0.), (123.456, -3.25, 1e-9)):
        got = host_fly(relay_host, a, gap, ox, oy)
        want = np_fly(*(a[:, k] for k in range(6)), gap, ox, oy)
        assert same_bits(got, want), (gap, ox, oy)
    # gap 0 leaves the position where it is (apart from the offset), whatever the direction
    got = host_fly(relay_host, a[30000:], 0., 0., 0.)
    assert same_bits(got[:, 0:2], a[30000:, 0:2] + 0.)
    # a zeroed record flies along the axis
    z = host_fly(relay_host, np.zeros((1, 6)), 1.0, 0.002, 0.)[0]
    assert z[5] == 1.0 and z[9] == 1.0 and z[0] == -0.002 and z[8] == 0.


def test_valid_entries(relay_host):
    rng = np.random.default_rng(3)
    n = 100000
    z = np.where(rng.random(n) < 0.3, 0., rng.uniform(-1., 9., n))
    w = np.where(rng.random(n) < 0.3, 0., rng.uniform(-0.1, 1., n))
    z[:4], w[:4] = [np.nan, 9., 0., -0.], [0.5, np.nan, 0.5, 0.5]
    got = np.zeros(n, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    relay_host.relay_valid_n(n, z.ctypes.data_as(dp), w.ctypes.data_as(dp), got.ctypes.data_as(C.POINTER(C.c_int32)))
    assert np.array_equal(got != 0, np_valid(z, w))
    assert not got[:4].any()


def test_finish_arithmetic(relay_host):
    rng = np.random.default_rng(11)
    n = 100000
    wa, wb = rng.random(n), rng.random(n)
    wa[:5], wb[:5] = [1., 0., 1e-300, 2.0 ** -62, 1.], [1., 1., 1e-300, 0.5, 2.0 ** -31]
    w = np.zeros(n)
    a, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    relay_host.relay_finish_n(n, wa.ctypes.data_as(dp), wb.ctypes.data_as(dp), w.ctypes.data_as(dp), a.ctypes.data_as(up), b.ctypes.data_as(up))
    assert same_bits(w, wa * wb)
    for k in list(range(8)) + list(rng.integers(0, n, 2000)):
        p = np.float64(wa[k]) * np.float64(wb[k])
        assert int(a[k]) == py_fix(p) and int(b[k]) == py_fix(p * p), k
    assert int(a[0]) == 1 << 62 and int(b[0]) == 1 << 62 and int(a[1]) == 0
    da, t, db = rng.uniform(0., 20., n), rng.uniform(0., 3., n), rng.uniform(0., 20., n)
    out = np.zeros(n)
    relay_host.relay_dtravel_n(n, da.ctypes.data_as(dp), t.ctypes.data_as(dp), db.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert same_bits(out, (da + t) + db)


BAD_PLACEMENTS = [(-1e-300, 0., 0.), (-1., 0., 0.), (math.nan, 0., 0.), (math.inf, 0., 0.), (1., math.nan, 0.), (1., 0., math.nan),
                  (1., math.inf, 0.), (1., 0., -math.inf)]
GOOD_PLACEMENTS = [(0., 0., 0.), (1., 0.002, -0.01), (1e6, -5., 5.), (5e-324, 0., 0.)]


def test_validate_refuses_bad_placements(relay_host):
    import polycap_amd
    L = polycap_amd.lib()
    assert L.pc_hip_relay_validate(None) == -2 and b"placement" in L.pc_hip_last_error()
    for pl in BAD_PLACEMENTS:
        assert not polycap_amd.relay_placement_valid(pl[0], pl[1:]), pl
        assert b"gap" in L.pc_hip_last_error()
        assert relay_host.relay_placement_ok(*pl) == 0
    for pl in GOOD_PLACEMENTS:
        assert polycap_amd.relay_placement_valid(pl[0], pl[1:]), pl
        assert relay_host.relay_placement_ok(*pl) == 1


def _ulps(a, b):
    if a == b:
        return 0
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_efficiencies_and_stderr_against_exact_arithmetic():
    import polycap_amd
    rng = np.random.default_rng(5)
    ne = 7
    for n_started, n_exit in ((33333, 4885), (10 ** 9 + 7, 10 ** 8), (2, 2), (1, 1), (0, 0)):
        # made-up exact totals: n_exit weights in [0, 1] -> sums below n_exit 2^62, squares below the sums
        A = [int(rng.integers(0, 1 << 62)) * max(n_exit, 0) // 3 + int(rng.integers(0, 1 << 40)) for _ in range(ne)]
        B = [a // int(rng.integers(2, 50)) for a in A]
        lohi = lambda v: [(x & ((1 << 64) - 1), x >> 64) for x in v]
        a = np.array(lohi(A), dtype=np.uint64)
        b = np.array(lohi(B), dtype=np.uint64)
        cnt = np.array([n_exit * 2, n_exit, 5, 6, 7, 8, 9, n_started], dtype=np.int64)
        eff, err = polycap_amd.relay_efficiencies(a, b, cnt)
        eff_only, none = polycap_amd.relay_efficiencies(a, None, cnt)
        assert none is None and same_bits(eff, eff_only)
        for e in range(ne):
            if n_started == 0:
                assert eff[e] == 0. and math.isnan(err[e])
                continue
            want = float(Fraction(A[e], n_started << 62))       # CPython rounds Fraction -> float correctly
            assert _ulps(eff[e], want) <= 1, (n_started, e, eff[e], want)
            if n_started < 2:
                assert math.isnan(err[e])
                continue
            m, q = Fraction(A[e], n_started << 62), Fraction(B[e], n_started << 62)
            v = max(Fraction(0), q - m * m) / (n_started - 1)
            want = math.sqrt(v) if v > 0 else 0.          # float(v) is correctly rounded; sqrt adds half an ulp
            assert abs(err[e] - want) <= 4e-16 * want + 1e-300, (n_started, e, err[e], want)
        # the same numbers as the source-run formula gives for N started photons
        ref = polycap_amd.efficiency_stderr(a, b, np.array([n_started, 0, 0, 0, 0, 0], dtype=np.int64))
        assert same_bits(err, ref)


def test_host_efficiency_equals_the_library(relay_host):
    import polycap_amd
    a = np.array([[123456789012345678, 77]], dtype=np.uint64)
    cnt = np.array([0, 0, 0, 0, 0, 0, 0, 20000], dtype=np.int64)
    eff, _ = polycap_amd.relay_efficiencies(a, None, cnt)
    assert eff[0] == relay_host.relay_efficiency(int(a[0, 0]), int(a[0, 1]), 20000)


def test_oracle_floors_are_the_ones_the_gpu_test_uses(oracle):
    """scripts/relay_floors.py on the oracle (no GPU): the flip caps and weight floors of tests/test_gpu_relay.py are its maxima,
    to the digits written there.  The oracle is plain C and deterministic; a tenth of a floor is left for another compiler's libm."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("relay_floors", os.path.join(ROOT, "scripts", "relay_floors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from tests.test_gpu_relay import CONFIGS
    for name, (_, _, flip_cap, c_floor) in CONFIGS.items():
        flips, cs, n1 = mod.floors(oracle, name)
        print(name, n1, flips, cs)
        assert abs(max(flips) - flip_cap) <= 0.1 * flip_cap, (name, flips)
        assert abs(max(cs) - c_floor) <= 0.1 * c_floor, (name, cs)


def test_new_symbols_are_exported_and_nothing_else_is():
    import polycap_amd
    polycap_amd.lib()
    so = os.path.join(ROOT, "polycap_amd", "lib", "libpolycap.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    relay = [n for n in names if "relay" in n]
    assert relay == sorted(NEW_SYMBOLS), relay
    text = open(os.path.join(ROOT, "include", "polycap-hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"POLYCAP_EXTERN\s+[^;(]*?\b(\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    # everything exported besides the declared C ABI was there before: no kernel stub, no C++ instantiation came with the relay
    assert not [n for n in names if n.startswith("_Z") or "pc_relay" in n]
    assert [n for n in names if n.startswith("pc_hip_") and n not in declared] == []
