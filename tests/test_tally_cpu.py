"""What spot maps, beam moments and histograms share, without a GPU: the first part of polycap_amd/csrc/hip/pc_tally.h, compiled for
the host (tests/tally/tally_host.cpp).  The energy selection's one rule, case by case; the two grid formulas against the arithmetic
the three launch functions carried before they were shared, written out here; the 128-bit add against Python integers."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "tally")
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


@pytest.fixture(scope="module")
def tally(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("tally_host")), "tally_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "tally_host.cpp"), "-o", so])
    L = C.CDLL(so)
    ip, u64p = C.POINTER(C.c_int), C.POINTER(C.c_uint64)
    L.tally_sel_check.restype = C.c_int
    L.tally_sel_check.argtypes = [C.c_int, ip, C.c_int64, C.c_char_p, C.c_int]
    L.tally_sel_fill.restype = C.c_int
    L.tally_sel_fill.argtypes = [C.c_int, ip, C.c_int64, ip]
    L.tally_grid_tiles.restype = C.c_int64
    L.tally_grid_tiles.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    L.tally_grid_wide.restype = C.c_int64
    L.tally_grid_wide.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, ip]
    L.tally_add128.restype = None
    L.tally_add128.argtypes = [u64p, C.c_uint64, C.c_uint64]
    return L


# ---- the energy selection -------------------------------------------------------------------------------------------------------
def sel_check(L, sel, ne, n_sel=None):
    arr = None if sel is None else (C.c_int * max(len(sel), 1))(*sel)
    why = C.create_string_buffer(256)
    ok = L.tally_sel_check(len(sel) if n_sel is None else n_sel, arr, ne, why, 256)
    return bool(ok), why.value.decode()


def sel_fill(L, sel, ne):
    arr = None if not sel else (C.c_int * len(sel))(*sel)
    out = (C.c_int * ne)()
    n = L.tally_sel_fill(len(sel), arr, ne, out)
    return list(out[:n])


@pytest.mark.parametrize("sel,ne,expect", [
    ([], 5, [0, 1, 2, 3, 4]),               # 0 = all
    ([3, 0, 4, 1, 2], 5, [3, 0, 4, 1, 2]),   # a permutation, kept in its order
    ([2], 5, [2]),                           # a single index
    ([4], 5, [4]),
    ([0], 1, [0]),
])
def test_selection_accepted(tally, sel, ne, expect):
    ok, why = sel_check(tally, sel, ne)
    assert ok and why == ""
    assert sel_fill(tally, sel, ne) == expect


def test_selection_all_needs_no_pointer(tally):
    assert sel_check(tally, None, 5, n_sel=0) == (True, "")


@pytest.mark.parametrize("sel,ne,n_sel,words", [
    ([-1], 5, None, ("energies", "-1", "out of range")),
    ([5], 5, None, ("energies", "index 5", "out of range", "5 energies")),
    ([1, 3, 1], 5, None, ("energies", "index 1", "twice")),
    ([0, 1, 2, 3, 4, 0], 5, None, ("n_energies",)),          # more indices than energies
    (None, 5, 2, ("n_energies",)),                            # a NULL pointer with n_sel > 0
    ([0], 5, -1, ("n_energies",)),
])
def test_selection_refused_with_a_reason(tally, sel, ne, n_sel, words):
    ok, why = sel_check(tally, sel, ne, n_sel)
    assert not ok
    for w in words:
        assert w in why, why


# ---- the grids ------------------------------------------------------------------------------------------------------------------
CUS = (1, 256)
GROUPS = (1, 2, 129, 600)
N_SEL = (1, 2, 3, 63, 64, 65, 291)
ENTRIES = (1, 63, 64, 65, 511, 512, 513, 10 ** 7)
BLOCKS = (256, 512)


def old_tiles(cus, tiles, n, block):
    """pc_spot_launch and pc_hist_launch, LDS tiles, before the grids were shared"""
    bx = (2 * cus + tiles - 1) // tiles
    need = (n + block - 1) // block
    if bx > need:
        bx = need
    if bx < 1:
        bx = 1
    return bx


def old_wide(cus, groups, n_sel, n, block):
    """pc_spot_launch, pc_hist_launch (energies across lanes) and pc_beam_launch before the grids were shared: (bx, gw)"""
    bx = (8 * cus + groups - 1) // groups
    gw = 1
    while gw < n_sel and gw < 64:
        gw <<= 1
    need = (n * gw + block - 1) // block
    if bx > need:
        bx = need
    if bx < 1:
        bx = 1
    return bx, gw


def test_grid_tiles_is_the_old_arithmetic(tally):
    for cus, tiles, n, block in itertools.product(CUS, GROUPS, ENTRIES, BLOCKS):
        bx = tally.tally_grid_tiles(cus, tiles, n, block)
        assert bx == old_tiles(cus, tiles, n, block), (cus, tiles, n, block)
        assert 1 <= bx <= max(1, (n + block - 1) // block)


def test_grid_wide_is_the_old_arithmetic(tally):
    for cus, groups, n_sel, n, block in itertools.product(CUS, GROUPS, N_SEL, ENTRIES, BLOCKS):
        gw = C.c_int(0)
        bx = tally.tally_grid_wide(cus, groups, n_sel, n, block, C.byref(gw))
        assert (bx, gw.value) == old_wide(cus, groups, n_sel, n, block), (cus, groups, n_sel, n, block)
        assert 1 <= bx <= max(1, (n * gw.value + block - 1) // block)
        assert gw.value in (1, 2, 4, 8, 16, 32, 64) and (gw.value >= n_sel or gw.value == 64)


# ---- the 128-bit add ------------------------------------------------------------------------------------------------------------
def add128(L, a, b):
    v = (C.c_uint64 * 2)(a & M64, a >> 64)
    L.tally_add128(v, b & M64, b >> 64)
    return int(v[0]) | (int(v[1]) << 64)


def signed(v):
    return v - (1 << 128) if v >> 127 else v


SEAMS = (0, 1, M64, M64 + 1, M64 << 64, (M64 << 64) | 1, M128, M128 - 1, 1 << 127, (1 << 127) - 1, (1 << 127) | M64,
         (M64 - 1) << 64 | M64, 0x0123456789abcdef_fedcba9876543210)


def test_add128_at_the_carry_seams(tally):
    assert add128(tally, M64, 1) == 1 << 64                           # lo = 2^64 - 1 plus 1: the carry
    assert add128(tally, (M64 << 64) | M64, 1) == 0                   # the carry into a hi that wraps
    assert add128(tally, (5 << 64) | M64, (M64 << 64) | 1) == 5 << 64   # carry-in with hi + add_hi wrapping
    assert add128(tally, 0, 0) == 0
    assert add128(tally, M128, M128) == M128 - 1                      # all ones: -1 + -1 = -2
    for a, b in itertools.product(SEAMS, SEAMS):
        got = add128(tally, a, b)
        assert got == (a + b) & M128, (hex(a), hex(b))
        # the same bits are the two's complement sum of the signed values
        assert signed(got) == signed((signed(a) + signed(b)) & M128), (hex(a), hex(b))


def test_add128_random(tally):
    rng = np.random.default_rng(128)
    for _ in range(2000):
        a, b = (int.from_bytes(rng.bytes(16), "little") for _ in range(2))
        assert add128(tally, a, b) == (a + b) & M128
