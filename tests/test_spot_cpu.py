"""Spot maps without a GPU: the per-entry arithmetic of pc_spot.h compiled for the host against a numpy restatement of the contract
in include/polycap-hip.h, and the validation of POLYCAP_SPOT by the public call before any device is used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import EXAMPLE, ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")


def np_spot_bin(x, y, z, dx, dy, dz, zp, window, nx, ny):
    """the contract, operation by operation: bin iy*nx + ix, or -1 outside"""
    x0, x1, y0, y1 = window
    with np.errstate(all="ignore"):
        t = (zp - z) / dz
        xd = x + dx * t
        yd = y + dy * t
        fx = ((xd - x0) / (x1 - x0)) * float(nx)
        fy = ((yd - y0) / (y1 - y0)) * float(ny)
        inside = (dz > 0.) & (fx >= 0.) & (fx < nx) & (fy >= 0.) & (fy < ny)
        b = np.full(np.shape(fx), -1, dtype=np.int64)
        b[inside] = np.floor(fy[inside]).astype(np.int64) * nx + np.floor(fx[inside]).astype(np.int64)
    return b


def np_exit_dz(dx, dy):
    with np.errstate(all="ignore"):
        return np.sqrt((1. - dx * dx) - dy * dy)


def np_q(w):
    v = np.asarray(w, dtype=np.float64) * 4294967296.0
    q = np.zeros(v.shape, dtype=np.uint64)
    pos = v > 0.
    q[pos] = np.rint(v[pos]).astype(np.uint64)
    return q


@pytest.fixture(scope="module")
def spot_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("spot_host")
    src = d / "spot_host.cpp"
    src.write_text('#define PC_SPOT_HOST_ONLY\n#include "pc_spot.h"\n'
                   'extern "C" long long spot_bin(double x, double y, double z, double dx, double dy, double dz, double zp,\n'
                   '    double x0, double x1, double y0, double y1, int nx, int ny)\n'
                   '{ return pc_spot_bin(x, y, z, dx, dy, dz, zp, x0, x1, y0, y1, nx, ny); }\n'
                   'extern "C" double spot_exit_dz(double dx, double dy) { return pc_spot_exit_dz(dx, dy); }\n'
                   'extern "C" unsigned long long spot_q(double w) { return pc_spot_q(w); }\n')
    so = d / "spot_host.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.spot_bin.restype = C.c_longlong
    L.spot_bin.argtypes = [C.c_double] * 11 + [C.c_int, C.c_int]
    L.spot_exit_dz.restype = C.c_double
    L.spot_exit_dz.argtypes = [C.c_double, C.c_double]
    L.spot_q.restype = C.c_ulonglong
    L.spot_q.argtypes = [C.c_double]
    return L


def _adversarial():
    """entries whose lines cross bin edges, x1 and y1 exactly, or carry 0 / negative / NaN dz and signed zeros"""
    rng = np.random.default_rng(7)
    window = (-0.02, 0.02, -0.01, 0.03)
    nx, ny = 8, 5
    zp = 10.0
    rows = []
    # straight down the axis (dx = dy = 0): xd == x, so the positions can sit exactly on edges
    edges_x = np.linspace(window[0], window[1], nx + 1)
    edges_y = np.linspace(window[2], window[3], ny + 1)
    for ex in list(edges_x) + [np.nextafter(window[1], -1.), np.nextafter(window[0], -1.), 0.0, -0.0]:
        for ey in list(edges_y) + [np.nextafter(window[3], 1.), -0.0]:
            rows.append((ex, ey, 9.0, 0.0, 0.0, 1.0))
            rows.append((ex, ey, 9.0, -0.0, 0.0, 1.0))
    for dz in (0.0, -0.0, -1e-3, -0.5, np.nan, np.inf, 1e-300):
        rows.append((0.001, 0.002, 9.0, 1e-4, -1e-4, dz))
    for _ in range(400):
        rows.append((rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.04), rng.uniform(8.0, 10.5),
                     rng.normal(0, 2e-3), rng.normal(0, 2e-3), 1.0))
    rows.append((np.nan, 0.0, 9.0, 0.0, 0.0, 1.0))
    rows.append((0.0, 0.0, np.nan, 0.0, 0.0, 1.0))
    a = np.array(rows, dtype=np.float64)
    return a, window, nx, ny, zp


def test_host_bin_function_matches_numpy_contract(spot_host):
    a, window, nx, ny, zp = _adversarial()
    want = np_spot_bin(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], zp, window, nx, ny)
    got = np.array([spot_host.spot_bin(*r, zp, *window, nx, ny) for r in a], dtype=np.int64)
    assert np.array_equal(got, want)
    # every class is present: inside, on the last edge (outside), dz <= 0 / NaN (outside)
    assert (want >= 0).sum() > 50 and (want < 0).sum() > 20
    on_x1 = (a[:, 0] == window[1]) & (a[:, 3] == 0.)
    assert on_x1.any() and (want[on_x1] == -1).all()
    bad_dz = ~(a[:, 5] > 0.)
    assert bad_dz.sum() >= 5 and (want[bad_dz] == -1).all()
    on_x0 = (a[:, 0] == window[0]) & (a[:, 1] == window[2]) & (a[:, 3] == 0.)
    assert (want[on_x0] == 0).all()


def test_host_exit_dz_and_quantisation(spot_host):
    rng = np.random.default_rng(3)
    dx = np.concatenate([rng.normal(0, 0.01, 200), [0.0, -0.0, 0.6, 0.8, 1.0, 0.9, np.nan]])
    dy = np.concatenate([rng.normal(0, 0.01, 200), [0.0, 0.0, 0.8, 0.6, 0.0, 0.9, 0.0]])
    want = np_exit_dz(dx, dy)
    got = np.array([spot_host.spot_exit_dz(a, b) for a, b in zip(dx, dy)])
    assert np.array_equal(got, want, equal_nan=True)
    w = np.array([0.0, -0.0, 2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** -32, 1.0, 0.5 + 2.0 ** -33, np.nan, -1.0, 0.123456789])
    got = np.array([spot_host.spot_q(v) for v in w], dtype=np.uint64)
    want = np_q(w)
    assert np.array_equal(got, want)
    assert got[2] == 0 and got[3] == 2 and got[5] == 1 << 32          # halves go to the even neighbour


BAD_SPECS = [
    ("dist=1;window=0.02,-0.02,-0.02,0.02;bins=16x16;energies=all", "x0 < x1"),
    ("dist=1;window=-0.02,0.02,-0.02,0.02;bins=0x5;energies=all", "nx and ny"),
    ("dist=1;window=-0.02,0.02,-0.02,0.02;bins=16x16;energies=0,1000", "out of range"),
    ("dist=" + ",".join(["1"] * 65) + ";window=-0.02,0.02,-0.02,0.02;bins=16x16", "64"),
    ("dist=1,2;window=-0.02,0.02,-0.02,0.02;bins=16384x8192", "2\\^27"),
    ("dist=1;window=-0.02,0.02,-0.02,0.02", "required"),
    ("dist=1;window=-0.02,0.02,-0.02,0.02;bins=4x4;energies=0,0", "twice"),
]


@pytest.mark.parametrize("spec,match", BAD_SPECS)
def test_public_call_rejects_bad_spot_spec(spec, match, monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SPOT", spec)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SPOT") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert __import__("re").search(match, str(e.value)), str(e.value)


def test_public_call_with_valid_spot_spec_needs_a_device(monkeypatch):
    import polycap_amd
    from polycap_amd import capi
    if polycap_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    monkeypatch.setenv("POLYCAP_SPOT", "dist=0.5,1,2;window=-0.02,0.02,-0.02,0.02;bins=64x32;energies=all")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(RuntimeError, match="HIP"):
        src.get_transmission_efficiencies(1, 1000)
