"""The squared-weight sums of the tallies without a GPU: the per-entry square W*W and the carry add of polycap_amd/csrc/hip/pc_tally.h,
compiled for the host (tests/squares/squares_host.cpp), against Python integers; the split of the cells into LDS tiles at its seams;
pc_hip_tally_stderr and pc_hip_select_transmission against mpmath; and the host part once under the address and undefined-behaviour
sanitizers, as a program of its own."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "squares")
M64 = (1 << 64) - 1
ULPS = 2          # long double carries 64 bits: its result rounded to double is the correctly rounded double or a neighbour


def build_squares_host(directory):
    so = os.path.join(str(directory), "squares_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "squares_host.cpp"), "-o", so])
    L = C.CDLL(so)
    u64p, i64p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.squares_entry.restype = C.c_uint64
    L.squares_entry.argtypes = [C.c_double, u64p]
    L.squares_accumulate.restype = None
    L.squares_accumulate.argtypes = [u64p, C.c_int64, u64p]
    L.squares_tile_split.restype = None
    L.squares_tile_split.argtypes = [C.c_int64, C.c_int64, C.c_int, i64p]
    L.squares_stderr.restype = None
    L.squares_stderr.argtypes = [C.c_int64, u64p, u64p, C.c_int64, dp]
    L.squares_transmission.restype = None
    L.squares_transmission.argtypes = [C.c_int64, u64p, u64p, u64p, u64p, dp, dp]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_squares_host(tmp_path_factory.mktemp("squares_host"))


def tile_split(L, total, tile, squares):
    out = (C.c_int64 * 2)()
    L.squares_tile_split(total, tile, 1 if squares else 0, out)
    return int(out[0]), int(out[1])


def to_pairs(ints):
    """Python integers (any nesting numpy can flatten) as uint64 (lo, hi) pairs [..., 2]"""
    a = np.asarray(ints, dtype=object)
    flat = [int(v) for v in a.ravel()]
    return np.array([[v & M64, v >> 64] for v in flat], dtype=np.uint64).reshape(a.shape + (2,))


def to_ints(pairs):
    p = np.asarray(pairs, dtype=np.uint64)
    return p[..., 0].astype(object) + p[..., 1].astype(object) * (1 << 64)


# ---- the per-entry square and the carry add --------------------------------------------------------------------------------------
def py_q(w):
    """round_half_even(w * 2^32), 0 for anything not above zero: exact in Python (w * 2^32 is a power-of-two scaling)"""
    if not w > 0.:
        return 0
    return round(w * 4294967296.0)          # Python rounds halves to even


WEIGHTS = [0., -1., float("nan"), 2.0 ** -33, 1e-6, 0.5, 1. - 2.0 ** -53, 1.]


@pytest.mark.parametrize("w", WEIGHTS)
def test_entry_square_equals_python_integers(host, w):
    out = (C.c_uint64 * 2)()
    W = int(host.squares_entry(w, out))
    assert W == py_q(w)
    assert (int(out[0]), int(out[1])) == ((W * W) & M64, (W * W) >> 64)


def test_the_largest_weight_needs_the_65th_bit(host):
    out = (C.c_uint64 * 2)()
    assert int(host.squares_entry(1., out)) == 1 << 32 and (int(out[0]), int(out[1])) == (0, 1)
    assert int(host.squares_entry(1. - 2.0 ** -53, out)) == 1 << 32                       # rounds up to 2^32
    assert int(host.squares_entry(2.0 ** -33, out)) == 0 and (int(out[0]), int(out[1])) == (0, 0)   # half a quantum: to even
    W = int(host.squares_entry(1e-6, out))
    assert W == 4295 and int(out[0]) == 4295 * 4295 > 0                                  # w*w = 1e-12 is far below 2^-32: a quantised w*w would be 0


def test_carry_add_equals_python_integers(host):
    rng = np.random.default_rng(64)
    cases = [np.full(9, 1 << 32, dtype=np.uint64),                                       # nine times 2^64: lo stays 0, hi counts
             np.full(7, (1 << 32) - 1, dtype=np.uint64),                                   # just below: lo wraps on the second add
             rng.integers(0, (1 << 32) + 1, 5000, dtype=np.uint64),
             np.array([], dtype=np.uint64)]
    for W in cases:
        for start in (0, M64, (5 << 64) | (M64 - 3)):
            v = (C.c_uint64 * 2)(start & M64, start >> 64)
            host.squares_accumulate(v, len(W), W.ctypes.data_as(C.POINTER(C.c_uint64)))
            want = start + sum(int(x) * int(x) for x in W)
            assert (int(v[0]), int(v[1])) == (want & M64, want >> 64)
    v = (C.c_uint64 * 2)(0, 0)
    W = np.full(3, (1 << 32) - 1, dtype=np.uint64)
    host.squares_accumulate(v, 3, W.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert int(v[1]) == 2                                                                  # three squares of about 2^64: two wraps of lo


# ---- the tiles -------------------------------------------------------------------------------------------------------------------
def test_tile_split_at_its_seams(host):
    for header, name in (("pc_spot.h", "PC_SPOT_TILE"), ("pc_cells.h", "PC_CELLS_TILE")):      # the histograms and the joint histograms share one
        tile = int(re.search(r"#define %s (\d+)" % name, open(os.path.join(HIPD, header)).read()).group(1))
        assert tile * 8 == 65536                                                           # all of the 64 KiB a workgroup's tile has
        cells, _ = tile_split(host, 1, tile, True)
        assert cells == tile // 3 and 3 * cells <= tile                                    # a weight sum and a (lo, hi) pair per cell
        assert tile_split(host, 1, tile, False)[0] == tile
        for squares, c in ((True, cells), (False, tile)):
            assert tile_split(host, 1, tile, squares) == (c, 1)
            assert tile_split(host, c - 1, tile, squares) == (c, 1)
            assert tile_split(host, c, tile, squares) == (c, 1)                             # exactly filling a tile
            assert tile_split(host, c + 1, tile, squares) == (c, 2)                         # and one more
            assert tile_split(host, 2 * c, tile, squares) == (c, 2)
            assert tile_split(host, 2 * c + 1, tile, squares) == (c, 3)
            assert tile_split(host, 1 << 27, tile, squares) == (c, -(-(1 << 27) // c))
        # cells that fit one tile of weights need up to three with their squares
        assert tile_split(host, tile, tile, True)[1] == 4 and tile_split(host, 3 * cells, tile, True)[1] == 3


# ---- the estimators against mpmath -----------------------------------------------------------------------------------------------
def ulps(got, want):
    if want == 0. or got == want:
        return 0. if got == want else float("inf")
    return abs(got - want) / math.ulp(want)


def mp_stderr(S, S2, N):
    import mpmath as mp
    mp.mp.prec = 400
    if N < 2:
        return float("nan")
    m = mp.mpf(S) / (mp.mpf(2) ** 32 * N)
    q = mp.mpf(S2) / (mp.mpf(2) ** 64 * N)
    v = q - m * m
    return float(mp.sqrt(max(v, mp.mpf(0)) / (N - 1)))


def host_stderr(L, S, S2, N):
    a = np.array(S, dtype=np.uint64)
    b = to_pairs(S2)
    out = np.zeros(len(S))
    L.squares_stderr(len(S), a.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_uint64)), N, out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def cells_of_entries(rng, n_cells, n_max):
    """S and S2 of cells that each hold up to n_max entries of random quantised weights, some tiny, some 2^32"""
    S, S2 = [], []
    for k in range(n_cells):
        n = int(rng.integers(0, n_max + 1))
        W = [int(v) for v in rng.integers(0, (1 << 32) + 1, n)]
        if k % 3 == 0:
            W = [w >> 20 for w in W]                                                       # weights around 1e-6
        if k % 5 == 0 and W:
            W[0] = 1 << 32
        S.append(sum(W))
        S2.append(sum(w * w for w in W))
    return S, S2


def test_stderr_equals_mpmath(host):
    """Cells of at most N / 2 entries: S*S <= n*S2 (Cauchy-Schwarz) gives m*m <= q / 2, so q - m*m cancels one bit at the most and the
    long double result, rounded to double, is within ULPS of the exact one"""
    rng = np.random.default_rng(97)
    for N in (2, 3, 1600, 10 ** 7, (1 << 32) - 1):
        S, S2 = cells_of_entries(rng, 200, min(400, N // 2))
        got = host_stderr(host, S, S2, N)
        for k in range(len(S)):
            want = mp_stderr(S[k], S2[k], N)
            assert ulps(got[k], want) <= ULPS, (N, k, got[k], want)
        assert (got > 0.).sum() > 50
    S, S2 = cells_of_entries(rng, 200, 400)
    # the public symbol is the same function
    from polycap_amd import tally_stderr
    assert np.array_equal(tally_stderr(np.array(S, dtype=np.uint64), to_pairs(S2), 1600), host_stderr(host, S, S2, 1600))
    assert tally_stderr(np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 3, 2), dtype=np.uint64), 10).shape == (2, 3)
    with pytest.raises(ValueError):
        tally_stderr(np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), 10)


def test_stderr_edges(host):
    S, S2 = [0, 1 << 31, 1 << 32], [0, 1 << 62, 1 << 64]
    for N in (-5, 0, 1):
        assert np.isnan(host_stderr(host, S, S2, N)).all()                                  # N < 2
    got = host_stderr(host, S, S2, 2)
    assert not np.isnan(got).any() and got[0] == 0.                                        # S == 0: an empty cell has no error
    assert got[1] == mp_stderr(S[1], S2[1], 2) == 0.25                                     # one entry of 0.5 among two photons
    # q - m*m negative (sums that no set of entries gives): clipped to 0, not NaN
    got = host_stderr(host, [3 << 30, 1 << 32, M64], [0, 1, 5], 4)
    assert got.tolist() == [0., 0., 0.]
    assert mp_stderr(3 << 30, 0, 4) == 0.
    # every started photon in one cell with the same weight: the variance cancels to nothing or nearly so
    n, w = 1000, 123456789
    got = host_stderr(host, [n * w], [n * w * w], n)
    assert 0. <= got[0] <= 1e-9


def mp_transmission(P, R, P2, R2):
    import mpmath as mp
    mp.mp.prec = 400
    p, r = mp.mpf(P) / mp.mpf(2) ** 32, mp.mpf(R) / mp.mpf(2) ** 32
    p2, r2 = mp.mpf(P2) / mp.mpf(2) ** 64, mp.mpf(R2) / mp.mpf(2) ** 64
    if p + r == 0:
        return float("nan"), float("nan")
    return float(p / (p + r)), float(mp.sqrt(r * r * p2 + p * p * r2) / ((p + r) * (p + r)))


def host_transmission(L, P, R, P2, R2):
    u64p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    a, b, c, d = np.array(P, dtype=np.uint64), np.array(R, dtype=np.uint64), to_pairs(P2), to_pairs(R2)
    T, E = np.zeros(len(P)), np.zeros(len(P))
    L.squares_transmission(len(P), a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), c.ctypes.data_as(u64p), d.ctypes.data_as(u64p),
                           T.ctypes.data_as(dp), E.ctypes.data_as(dp))
    return T, E


def test_transmission_equals_mpmath(host):
    rng = np.random.default_rng(11)
    P, P2 = cells_of_entries(rng, 120, 3000)
    R, R2 = cells_of_entries(rng, 120, 3000)
    P += [0, 0, 7, M64, 1 << 32]
    P2 += [0, 0, 49, (1 << 97) - 1, 1 << 64]
    R += [0, 5, 0, M64, 0]
    R2 += [0, 25, 0, (1 << 97) - 1, 0]
    T, E = host_transmission(host, P, R, P2, R2)
    for k in range(len(P)):
        t, e = mp_transmission(P[k], R[k], P2[k], R2[k])
        if P[k] + R[k] == 0:
            assert np.isnan(T[k]) and np.isnan(E[k]) and np.isnan(t)                        # P + R == 0
        else:
            assert ulps(T[k], t) <= ULPS and ulps(E[k], e) <= ULPS, (k, T[k], t, E[k], e)
    assert (T[-4], E[-4]) == (0., 0.) and (T[-3], E[-3]) == (1., 0.)                        # nothing passes; everything passes
    from polycap_amd import select_transmission
    t2, e2 = select_transmission(P, R, to_pairs(P2), to_pairs(R2))
    assert np.array_equal(t2, T, equal_nan=True) and np.array_equal(e2, E, equal_nan=True)


def test_pairs_sum_is_exact():
    from polycap_amd import pairs_sum
    rng = np.random.default_rng(5)
    v = [[int.from_bytes(rng.bytes(12), "little") for _ in range(7)] for _ in range(5)]   # below 2^96: sums stay below 2^128
    p = to_pairs(v)
    assert p.shape == (5, 7, 2)
    assert to_ints(pairs_sum(p, 0)).tolist() == [sum(v[i][j] for i in range(5)) for j in range(7)]
    assert to_ints(pairs_sum(p, 1)).tolist() == [sum(row) for row in v]
    assert to_ints(pairs_sum(to_pairs([M64, 1]), 0)) == 1 << 64                             # the carry


# ---- the python layer without a device ---------------------------------------------------------------------------------------------
def test_symbols_are_bound():
    from polycap_amd import _cabi
    L = _cabi.lib()
    for stem in ("spot", "hist", "joint", "select"):
        assert getattr(L, "pc_hip_%s_track_squares" % stem)(None) == -2                     # PC_HIP_ERR_INVALID: NULL object
        assert getattr(L, "pc_hip_%s_read_squares" % stem)(None, None, None) == -2
        assert b"must not be NULL" in L.pc_hip_last_error()


# ---- the host part under the sanitizers --------------------------------------------------------------------------------------------
def test_host_part_is_clean_under_the_sanitizers(tmp_path):
    """tests/squares/squares_host.cpp with its own main, built with -fsanitize=address,undefined, run once: nothing is loaded into python"""
    exe = str(tmp_path / "squares_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSQUARES_HOST_MAIN", "-I", HIPD, os.path.join(HERE, "squares_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "squares_host: 0 failures" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
