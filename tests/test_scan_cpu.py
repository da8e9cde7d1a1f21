"""Scans without a device (include/polycap-hip.h, pc_hip_scan_*): argument checks, the order of scan_points, the per-row
efficiencies and standard errors, and a host compile of the scan's mapping and per-point sampler (pc_device.h) against the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.common import make_pair
from tests.conftest import ROOT

INVALID = -2


@pytest.fixture(scope="module")
def L():
    import polycap_amd
    return polycap_amd.lib()


def _validate(L, pts, n_points=None, n_per_point=1):
    a = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = a.shape[0] if n_points is None else n_points
    st = L.pc_hip_scan_validate(a.ctypes.data_as(C.POINTER(C.c_double)), n, n_per_point)
    return st, (L.pc_hip_last_error() or b"").decode()


def test_validate_messages(L):
    good = [[10., 0., 0.], [5., -0.1, 0.2]]
    assert _validate(L, good, n_per_point=1000)[0] == 0
    cases = [
        ([[0., 0., 0.]], None, 1, "pc_hip_scan_validate: point 0: d_source must be greater than 0"),
        ([[10., 0., 0.], [-1., 0., 0.]], None, 1, "pc_hip_scan_validate: point 1: d_source must be greater than 0"),
        ([[np.nan, 0., 0.]], None, 1, "pc_hip_scan_validate: point 0: d_source must be greater than 0"),
        ([[np.inf, 0., 0.]], None, 1, "pc_hip_scan_validate: point 0: d_source must be finite"),
        ([[1., np.inf, 0.]], None, 1, "pc_hip_scan_validate: point 0: src_shiftx must be finite"),
        ([[1., 0., np.nan]], None, 1, "pc_hip_scan_validate: point 0: src_shifty must be finite"),
        ([[1., 0., 0.]], 0, 1, "pc_hip_scan_validate: n_points must be >= 1"),
        ([[1., 0., 0.]], 1, 0, "pc_hip_scan_validate: n_per_point must be >= 1"),
        ([[1., 0., 0.]], 1, -5, "pc_hip_scan_validate: n_per_point must be >= 1"),
        ([[1., 0., 0.]] * 4, 4, 2 ** 62, "pc_hip_scan_validate: n_points * n_per_point overflows int64"),
    ]
    for pts, n, npp, msg in cases:
        st, text = _validate(L, pts, n, npp)
        assert st == INVALID and text == msg, (pts, n, npp, text)


def test_scan_points_order_and_shape():
    import polycap_amd
    x, y, d = [-0.1, 0.0, 0.1, 0.2], [0.5, -0.5], [3.0, 7.0, 9.0]
    p = polycap_amd.scan_points(x, y, d)
    assert p.shape == (len(x) * len(y) * len(d), 3) and p.dtype == np.float64
    for i_d in range(len(d)):
        for i_y in range(len(y)):
            for i_x in range(len(x)):
                row = (i_d * len(y) + i_y) * len(x) + i_x          # x fastest, then y, then d_source
                assert tuple(p[row]) == (d[i_d], x[i_x], y[i_y])
    q = polycap_amd.scan_points(x=[0.25])
    assert q.shape == (1, 3) and np.isnan(q[0, 0]) and tuple(q[0, 1:]) == (0.25, 0.0)
    assert polycap_amd.scan_points(y=np.linspace(-1, 1, 5), d_source=2.0).shape == (5, 3)


def _pairs(vals):
    return np.array([[v & (2 ** 64 - 1), v >> 64] for v in vals], dtype=np.uint64)


def test_row_efficiencies_and_stderr():
    """pc_hip_scan_efficiencies row by row equals pc_hip_efficiencies / pc_hip_efficiency_stderr of each row; a row where
    nothing entered a capillary gives 0, not NaN"""
    import polycap_amd
    ne = 3
    rng = np.random.default_rng(5)
    counters = np.array([[5000, 12000, 3000, 20000, 7, 20007],
                         [0, 2000, 0, 0, 2000, 2000],           # nothing entered: 0
                         [1, 0, 0, 4, 0, 1],
                         [123456, 1, 654321, 999, 0, 777778]], dtype=np.int64)
    a_int, b_int = [], []
    for c in counters:
        w = rng.random((int(c[0]), ne)) * 0.9
        a_int.append([int(v) for v in (w * 2.0 ** 62).astype(np.uint64).astype(object).sum(axis=0)] if c[0] else [0] * ne)
        b_int.append([int(v) for v in ((w * w) * 2.0 ** 62).astype(np.uint64).astype(object).sum(axis=0)] if c[0] else [0] * ne)
    A = np.stack([_pairs(r) for r in a_int])
    B = np.stack([_pairs(r) for r in b_int])
    eff, err = polycap_amd.scan_efficiencies(counters, A, B)
    assert eff.shape == (4, ne) and err.shape == (4, ne)
    assert np.all(eff[1] == 0.0) and np.all(np.isfinite(eff))
    for k in (0, 2, 3):
        sw = np.array([polycap_amd.fixed_to_double(lo, hi) for lo, hi in A[k]])
        assert np.array_equal(eff[k], polycap_amd.efficiencies(sw, counters[k]))
        assert np.array_equal(err[k], polycap_amd.efficiency_stderr(A[k], B[k], counters[k]), equal_nan=True)
    assert np.all(np.isnan(err[2]))          # one started photon: no standard error
    assert np.all(err[1] == 0.0)
    eff2, err2 = polycap_amd.scan_efficiencies(counters, A)
    assert err2 is None and np.array_equal(eff2, eff)


@pytest.fixture(scope="module")
def host_sampler(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "scan", "scan_sample_host.cpp")
    so = str(tmp_path_factory.mktemp("scan_host") / "libscan_sample_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-mfma",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "polycap_amd", "csrc", "hip"),
                           "-o", so, src])
    return C.CDLL(so)


def test_host_compile_of_scan_sampler_matches_oracle(host_sampler, oracle):
    """Flat index i of a scan -> point k = i // n_per_point, slot slot0 + i % n_per_point, sampled at point k's position: the same
    photons as the oracle's sampler with a source that sits at point k (circular, elliptical, uniform illumination)."""
    from polycap_amd._cabi import ProblemS
    seed, slot0, npp = 424242, 17, 50
    for which, source in (("xos1", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0)),
                          ("ellip", (0.05, 0.1, 0.1, 0.2, 0.2, 0., 0., 0.5)),
                          ("ellip", (2000., 0.2065, 0.1, 0., 0., 0.01, -0.02, 0.9)),
                          ("ellip", (5., 0.01, 0.01, -1., 0., 0., 0., 0.0))):
        optic, _, prob, _ = make_pair(oracle, which, source=source)
        pts = np.array([[source[0], source[5], source[6]], [source[0], 0.03, 0.0], [source[0], -0.05, 0.02],
                        [source[0] * 1.7, 0.01, -0.04], [source[0] * 0.5, 0.0, 0.0]])
        flat = np.arange(pts.shape[0] * npp, dtype=np.int64)
        att = (flat % 4).astype(np.uint32)
        out = np.zeros((flat.shape[0], 12))
        kj = np.zeros((flat.shape[0], 2), dtype=np.int64)
        f = host_sampler.scan_sample_host
        f.argtypes = [C.POINTER(ProblemS), C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p]
        assert f(C.byref(prob.s), pts.ctypes.data, npp, slot0, seed, flat.shape[0], flat.ctypes.data, att.ctypes.data,
                 out.ctypes.data, kj.ctypes.data) == 0
        assert np.array_equal(kj[:, 0], flat // npp) and np.array_equal(kj[:, 1], flat % npp)
        for k in range(pts.shape[0]):
            s = list(source)
            s[0], s[5], s[6] = pts[k]
            src_k = oracle.make_source(*s)
            rows = slice(k * npp, (k + 1) * npp)
            for a in range(4):
                sel = np.arange(npp)[(att[rows] == a)]
                ref = oracle.sample_photons(optic, src_k, seed, slot0 + sel, attempt=a)
                got = out[rows][sel]
                assert np.abs(got - ref).max() <= 1e-13, (which, source, k, a)
