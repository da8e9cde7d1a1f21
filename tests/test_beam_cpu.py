"""Exit-beam moments without a GPU: the per-entry arithmetic and the derived-parameter formulas of pc_beam.h, compiled for the host,
against a restatement of the contract in include/polycap-hip.h with exact Python integers; a synthetic beam and an oracle run for
signs and units; and the validation of POLYCAP_BEAM by the public call before any device is used."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import EXAMPLE, ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
Q24 = 16777216.0
PAIRS = [(a, b) for a in range(4) for b in range(a, 4)]        # XX, XY, XU, XV, YY, YU, YV, UU, UV, VV


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def py_q(w):
    """W = round_half_even(w * 2^32), 0 for w <= 0 and NaN"""
    v = float(np.float64(w) * np.float64(4294967296.0))
    return int(np.rint(v)) if v > 0. else 0


def py_entry(x, y, z, dx, dy, dz, ze):
    """(X, Y, U, V) as Python ints, or None when the entry is out of range"""
    f = np.float64
    with np.errstate(all="ignore"):
        t = (f(ze) - f(z)) / f(dz)
        xe, ye = f(x) + f(dx) * t, f(y) + f(dy) * t
        sx, sy = f(dx) / f(dz), f(dy) / f(dz)
        r = [np.rint(v * f(Q24)) for v in (xe, ye, sx, sy)]
    if not (f(dz) > 0.) or not all(abs(v) < 2.0 ** 31 for v in r):
        return None
    return tuple(int(v) for v in r)


def py_sums(q, W):
    """the 15 sums as Python ints from quantised entries q [n, 4] (in range) and weights W [n]"""
    S = [0] * 15
    for (X, Y, U, V), w in zip(q, W):
        P = (X, Y, U, V)
        S[0] += w
        for a in range(4):
            S[1 + a] += w * P[a]
        for k, (a, b) in enumerate(PAIRS):
            S[5 + k] += w * P[a] * P[b]
    return S


def to_lohi(S):
    """signed ints -> uint64 [len(S), 2] of 128-bit two's-complement (lo, hi) pairs"""
    out = np.zeros((len(S), 2), dtype=np.uint64)
    for k, v in enumerate(S):
        assert -(1 << 127) <= v < (1 << 127)
        u = v & ((1 << 128) - 1)
        out[k] = (u & ((1 << 64) - 1), u >> 64)
    return out


def _sqrt(v):
    """C's sqrt: NaN below zero (only sums that no set of entries can make have negative variances)"""
    return math.sqrt(v) if v >= 0. else float("nan")


def py_params(S):
    """the 26 columns, formula by formula, in the written order (Python floats are IEEE fp64; float(int) rounds to nearest even)"""
    nan = float("nan")
    s = float(S[0])
    row = [s * 2.0 ** -32] + [nan] * 25
    if not s > 0.:
        return row
    for a in range(4):
        row[1 + a] = (float(S[1 + a]) / s) * 2.0 ** -24
    ss = s * s
    for k, (a, b) in enumerate(PAIRS):
        n = S[0] * S[5 + k] - S[1 + a] * S[1 + b]
        row[5 + k] = (float(n) / ss) * 2.0 ** -48
    cxx, cxu, cyy, cyv, cuu, cvv = row[5], row[7], row[9], row[11], row[12], row[14]
    br, dr = cxu + cyv, cuu + cvv
    row[15] = -cxu / cuu if cuu != 0. else nan
    row[16] = -cyv / cvv if cvv != 0. else nan
    row[17] = -br / dr if dr != 0. else nan
    row[18] = math.sqrt(max(cxx - (cxu * cxu) / cuu, 0.)) if cuu != 0. else nan
    row[19] = math.sqrt(max(cyy - (cyv * cyv) / cvv, 0.)) if cvv != 0. else nan
    row[20] = math.sqrt(max((cxx + cyy) - (br * br) / dr, 0.)) if dr != 0. else nan
    row[21], row[22], row[23] = _sqrt(cxx), _sqrt(cyy), _sqrt(cxx + cyy)
    row[24], row[25] = _sqrt(cuu), _sqrt(cvv)
    return row


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (a.view(np.uint64) == b.view(np.uint64))))


# ---- the host compile of pc_beam.h ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beam_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("beam_host")
    src = d / "beam_host.cpp"
    src.write_text('#define PC_BEAM_HOST_ONLY\n#include "pc_beam.h"\n'
                   'extern "C" int beam_entry(double x, double y, double z, double dx, double dy, double dz, double ze, long long *q)\n'
                   '{ return pc_beam_entry(x, y, z, dx, dy, dz, ze, q); }\n'
                   'extern "C" void beam_params_row(const uint64_t *s, double *row) { pc_beam_params_row(s, row); }\n'
                   'extern "C" void beam_at_row(const double *row, double d, double *out) { pc_beam_at_row(row, d, out); }\n')
    so = d / "beam_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.beam_entry.restype = C.c_int
    L.beam_entry.argtypes = [C.c_double] * 7 + [C.POINTER(C.c_longlong)]
    L.beam_params_row.restype = None
    L.beam_params_row.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.beam_at_row.restype = None
    L.beam_at_row.argtypes = [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
    return L


def host_entry(L, x, y, z, dx, dy, dz, ze):
    q = (C.c_longlong * 4)()
    return tuple(int(v) for v in q) if L.beam_entry(x, y, z, dx, dy, dz, ze, q) else None


def host_row(L, lohi):
    s = np.ascontiguousarray(lohi, dtype=np.uint64)
    row = np.zeros(26)
    L.beam_params_row(s.ctypes.data_as(C.POINTER(C.c_uint64)), row.ctypes.data_as(C.POINTER(C.c_double)))
    return row


def host_entries(L, pos, dirs, ze):
    """quantised entries of arrays pos [n, 3], dirs [n, 3] through the host compile; None where out of range"""
    return [host_entry(L, *pos[i], *dirs[i], ze) for i in range(len(pos))]


# ---- per-entry arithmetic -------------------------------------------------------------------------------------------------------
def _edge_entries():
    ze = 10.0
    h24 = 2.0 ** -25                 # half a position quantum: ties of the rounding
    rows = []
    for k in range(-3, 4):
        for v in (k * h24, (2 * k + 1) * h24, np.nextafter((2 * k + 1) * h24, 1.), np.nextafter((2 * k + 1) * h24, -1.)):
            rows.append((v, -v, ze, 0.0, 0.0, 1.0))
            rows.append((0.0, 0.0, ze, v, -v, 1.0))        # slopes on the ties
    lim = 2.0 ** 31 / Q24                                   # 128 cm / slope 128 exactly: out of range
    for v in (lim, np.nextafter(lim, 0.), lim - 2.0 ** -24, lim - 2.0 ** -25, lim - 2.0 ** -26, -lim, -(lim - 2.0 ** -24),
              np.nextafter(-lim, 0.), -lim + 2.0 ** -25):
        rows.append((v, 0.0, ze, 0.0, 0.0, 1.0))
        rows.append((0.0, v, ze, 0.0, 0.0, 1.0))
        rows.append((0.0, 0.0, ze, v, 0.0, 1.0))            # slope dx / dz with dz = 1
        rows.append((0.0, 0.0, ze, 0.0, v * 0.5, 0.5))
    for dz in (0.0, -0.0, -1e-3, -1.0, np.nan, np.inf, 1e-300, 1e-9):
        rows.append((0.001, 0.002, 9.0, 1e-4, -1e-4, dz))
    for bad in (np.nan, np.inf, -np.inf):
        rows.append((bad, 0.0, ze, 0.0, 0.0, 1.0))
        rows.append((0.0, 0.0, bad, 1e-3, 0.0, 1.0))
        rows.append((0.0, 0.0, ze, bad, 0.0, 1.0))
    rows.append((-0.0, -0.0, ze, -0.0, -0.0, 1.0))
    return rows, ze


def test_host_entry_matches_exact_restatement(beam_host):
    rows, ze = _edge_entries()
    rng = np.random.default_rng(11)
    for _ in range(3000):
        z = ze - abs(rng.normal(0, 0.05))
        dz = rng.uniform(0.5, 1.0)
        rows.append((rng.normal(0, 0.03), rng.normal(0, 0.03), z, rng.normal(0, 0.01), rng.normal(0, 0.01), dz))
    n_out = 0
    for r in rows:
        want = py_entry(*r, ze)
        got = host_entry(beam_host, *r, ze)
        assert got == want, (r, got, want)
        n_out += want is None
    assert 40 < n_out < len(rows) - 3000          # both outcomes are exercised by the edges


def test_host_entry_rounds_ties_to_even(beam_host):
    h = 2.0 ** -25
    for k, want in ((1, 0), (3, 2), (5, 2), (-1, 0), (-3, -2), (7, 4)):
        assert host_entry(beam_host, k * h, 0.0, 10.0, 0.0, 0.0, 1.0, 10.0)[0] == want
    lim = 2.0 ** 31 / Q24
    assert host_entry(beam_host, lim - 2.0 ** -24, 0.0, 10.0, 0.0, 0.0, 1.0, 10.0)[0] == 2 ** 31 - 1
    assert host_entry(beam_host, lim - 2.0 ** -26, 0.0, 10.0, 0.0, 0.0, 1.0, 10.0) is None    # rounds up to 2^31
    assert host_entry(beam_host, -(lim - 2.0 ** -24), 0.0, 10.0, 0.0, 0.0, 1.0, 10.0)[0] == -(2 ** 31 - 1)


def test_weight_quantisation_is_the_spot_maps():
    from tests.test_spot_cpu import np_q
    w = np.array([1.0, 0.5, 0.0, -0.0, -1e-300, np.nan, 2.0 ** -33, 3 * 2.0 ** -33, 5 * 2.0 ** -33, 2.0 ** -32, 0.123456789])
    assert [py_q(v) for v in w] == [int(v) for v in np_q(w)]
    assert py_q(1.0) == 2 ** 32 and py_q(2.0 ** -33) == 0 and py_q(3 * 2.0 ** -33) == 2 and py_q(5 * 2.0 ** -33) == 2


# ---- derived parameters ---------------------------------------------------------------------------------------------------------
def _check_params(beam_host, S):
    lohi = to_lohi(S)
    want = py_params(S)
    got = host_row(beam_host, lohi)
    assert same_bits(got, want), (S, got, want)
    import polycap_amd
    lib = polycap_amd.beam_params(lohi.reshape(1, 15, 2))
    assert same_bits([lib[c][0] for c in polycap_amd.hip.beam_columns()], want)
    return got


def test_params_bit_for_bit_with_big_numerators(beam_host):
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(1, 1 << 31))
        big = trial % 3 == 0
        W = int(rng.integers(1, 1 << 32)) * n if big else int(rng.integers(1, 1 << 40))
        S = [W]
        for _ in range(4):
            S.append(int(rng.integers(-(1 << 62), 1 << 62)) * (int(rng.integers(1, 1 << 32)) if big else 1))
        for a, b in PAIRS:
            v = int(rng.integers(-(1 << 62), 1 << 62)) * int(rng.integers(1, 1 << 32)) * (int(rng.integers(1, 1 << 31)) if big else 1)
            S.append(abs(v) if a == b else v)
        S = [max(min(v, (1 << 126) - 1), -(1 << 126)) for v in S]
        _check_params(beam_host, S)
    # numerators far beyond 128 bits
    S = [(1 << 64) - 1] + [(1 << 94) + 12345] * 4 + [(1 << 125) + 7] * 10
    assert (S[0] * S[5]).bit_length() > 180
    _check_params(beam_host, S)


def test_params_edges(beam_host):
    nan_row = _check_params(beam_host, [0] * 15)
    assert nan_row[0] == 0. and np.isnan(nan_row[1:]).all()
    # a single entry: every covariance 0, waists NaN (denominator 0), sizes 0
    q, w = (1000, -2000, 30, 40), 1 << 32
    row = _check_params(beam_host, py_sums([q], [w]))
    assert row[0] == 1.0 and row[1] == 1000 * 2.0 ** -24 and (row[5:15] == 0).all() and np.isnan(row[15:21]).all()
    assert (row[21:] == 0).all()
    # slopes without spread in x only
    rng = np.random.default_rng(3)
    qs = [(int(rng.integers(-999, 999)), int(rng.integers(-999, 999)), 7, int(rng.integers(-99, 99))) for _ in range(50)]
    row = _check_params(beam_host, py_sums(qs, [int(rng.integers(1, 1 << 32)) for _ in qs]))
    assert np.isnan(row[15]) and np.isnan(row[18]) and np.isfinite(row[16]) and np.isfinite(row[17])


def test_params_keep_a_small_spread_around_a_far_centroid(beam_host):
    """centroid 10^4 times the RMS size: the exact numerators lose nothing to cancellation"""
    rng = np.random.default_rng(9)
    n = 4000
    X = (10 ** 6 + np.rint(rng.normal(0, 100, n))).astype(np.int64)
    Y = (-(10 ** 6) + np.rint(rng.normal(0, 100, n))).astype(np.int64)
    U = np.rint(rng.normal(0, 50, n)).astype(np.int64)
    V = np.rint(rng.normal(0, 50, n)).astype(np.int64)
    W = rng.integers(1, 1 << 32, n)
    qs = list(zip(*(map(int, a) for a in (X, Y, U, V))))
    row = _check_params(beam_host, py_sums(qs, [int(w) for w in W]))
    wf = W.astype(np.float64)
    Xd = X.astype(np.float64) - 10 ** 6            # shifted before the float sums: no cancellation here either
    var = np.sum(wf * Xd * Xd) / wf.sum() - (np.sum(wf * Xd) / wf.sum()) ** 2
    assert row[1] / row[21] > 9e3
    assert abs(row[1] / ((10 ** 6 + np.average(Xd, weights=wf)) * 2.0 ** -24) - 1) < 1e-12
    assert abs(row[5] / (var * 2.0 ** -48) - 1) < 1e-9


def test_at_distance_companion(beam_host):
    rng = np.random.default_rng(21)
    qs = [tuple(int(v) for v in rng.integers(-10 ** 6, 10 ** 6, 4)) for _ in range(300)]
    S = py_sums(qs, [int(w) for w in rng.integers(1, 1 << 32, len(qs))])
    row = py_params(S)
    import polycap_amd
    d = np.array([0.0, 0.5, 1.0, row[17], 3.25])
    lib = polycap_amd.beam_params(to_lohi(S).reshape(1, 15, 2), d)
    for k, dist in enumerate(d):
        vx = (row[5] + (2. * dist) * row[7]) + (dist * dist) * row[12]
        vy = (row[9] + (2. * dist) * row[11]) + (dist * dist) * row[14]
        want = [row[1] + dist * row[3], row[2] + dist * row[4], math.sqrt(max(vx, 0.)), math.sqrt(max(vy, 0.)),
                math.sqrt(max(vx, 0.) + max(vy, 0.))]
        got = [lib["at_" + c][0, k] for c in ("x", "y", "size_x", "size_y", "size_r")]
        assert same_bits(got, want)
        out = np.zeros(5)
        beam_host.beam_at_row(np.asarray(row).ctypes.data_as(C.POINTER(C.c_double)), dist, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert same_bits(out, want)
    # the round waist is where size_r is smallest
    assert lib["at_size_r"][0, 3] <= lib["at_size_r"][0].min()


# ---- a synthetic beam with a known waist ----------------------------------------------------------------------------------------
def test_synthetic_gaussian_waist_is_recovered(beam_host):
    rng = np.random.default_rng(2024)
    n, d0, s0, div = 20000, 3.0, 0.002, 0.001      # waist 3 cm behind the exit face, RMS size 20 um, divergence 1 mrad
    ze = 10.0
    sx, sy = rng.normal(0, div, n), rng.normal(0, div, n)
    xw, yw = rng.normal(0, s0, n), rng.normal(0, s0, n)
    dz = 1.0 / np.sqrt(1.0 + sx * sx + sy * sy)
    pos = np.stack([xw - d0 * sx, yw - d0 * sy, np.full(n, ze)], axis=1)
    dirs = np.stack([sx * dz, sy * dz, dz], axis=1)
    q = host_entries(beam_host, pos, dirs, ze)
    assert all(v is not None for v in q)
    W = [py_q(w) for w in rng.uniform(0.2, 1.0, n)]
    row = _check_params(beam_host, py_sums(q, W))
    tol_d = 5 * s0 / (div * math.sqrt(n))
    for col in (15, 16, 17):
        assert abs(row[col] - d0) < tol_d, (col, row[col])
    for col in (18, 19):
        assert abs(row[col] / s0 - 1) < 0.05, (col, row[col])
    assert abs(row[20] / (math.sqrt(2) * s0) - 1) < 0.05
    for col in (24, 25):
        assert abs(row[col] / div - 1) < 0.05


# ---- signs and units on the oracle's own photons ----------------------------------------------------------------------------------
def test_oracle_run_round_waist_matches_plane_ladder(beam_host, oracle):
    from tests.common import make_pair
    optic, src, prob, (E, A, S) = make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))
    o = oracle.transmission(optic, src, E, A, S, 777, 0, 3000, images=True)
    im, w = o["images"], o["exit_weights"][:, 0]
    ze = float(prob.z[-1])
    dx, dy = im[:, 11], im[:, 12]
    dz = np.sqrt((1. - dx * dx) - dy * dy)
    pos, dirs = im[:, 8:11], np.stack([dx, dy, dz], axis=1)
    q = host_entries(beam_host, pos, dirs, ze)
    keep = [i for i in range(len(q)) if q[i] is not None and py_q(w[i]) > 0]
    assert len(keep) > 2000
    row = _check_params(beam_host, py_sums([q[i] for i in keep], [py_q(w[i]) for i in keep]))
    d_star = row[17]
    assert 0.0 < d_star < 20.0, d_star
    # numpy: weighted RMS radius on a ladder of planes, photons propagated in floating point
    step = 0.002
    ladder = np.arange(0.0, 2 * d_star + 1.0, step)
    k = np.array(keep)
    t0 = (ze - pos[k, 2]) / dz[k]
    x0, y0 = pos[k, 0] + dx[k] * t0, pos[k, 1] + dy[k] * t0
    ux, uy, ww = dx[k] / dz[k], dy[k] / dz[k], w[k]
    r = []
    for d in ladder:
        x, y = x0 + d * ux, y0 + d * uy
        mx, my = np.average(x, weights=ww), np.average(y, weights=ww)
        r.append(np.sqrt(np.average((x - mx) ** 2 + (y - my) ** 2, weights=ww)))
    r = np.array(r)
    assert abs(ladder[np.argmin(r)] - d_star) <= step, (ladder[np.argmin(r)], d_star)
    assert abs(r.min() / row[20] - 1) < 1e-3 and abs(r[0] / row[23] - 1) < 1e-3


# ---- the public call's variable -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", ["2", "yes", "true", " 1", ""])
def test_public_call_rejects_bad_beam_variable(value, monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_BEAM", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_BEAM") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert "must be 0 or 1" in str(e.value)


def test_public_call_rejects_bad_share_with_beam(monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_BEAM", "1")
    monkeypatch.setenv("POLYCAP_SPOT_SHARE", "1.5")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SPOT_SHARE"):
        src.get_transmission_efficiencies(1, 1000)


def test_public_call_with_beam_needs_a_device(monkeypatch):
    import polycap_amd
    from polycap_amd import capi
    if polycap_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    monkeypatch.setenv("POLYCAP_BEAM", "1")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(RuntimeError, match="HIP"):
        src.get_transmission_efficiencies(1, 1000)


def test_beam_getters_fail_without_the_variable():
    """a result made elsewhere (from totals) carries no beam sums: the getters say which variable was missing"""
    from polycap_amd import capi
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.full(291, 0.5), [10, 5, 3, 40, 0, 0])
    with pytest.raises(ValueError, match="POLYCAP_BEAM"):
        eff.beam("exit")
