"""Gathers without a GPU (pc_hip_select_gather, Selection.gather, POLYCAP_SELECT_RECORDS): the plain part of
polycap_amd/csrc/hip/pc_gather.h compiled for the host -- the tile planner of the compaction, the chunk split of a window, the
argument check -- against numpy; the refusals of the built library that need no device; the host part once under the address and
undefined-behaviour sanitizers, as a program of its own; and the public call's variable, refused before any device is used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_hist_cpu import HIPD
from tests.test_select_cpu import EXAMPLE_SELECT

HERE = os.path.join(ROOT, "tests", "gather")
INCLUDE = os.path.join(ROOT, "include")
FN = "pc_hip_select_gather"


@pytest.fixture(scope="module")
def gather_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("gather_host")), "gather_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", INCLUDE, "-I", HIPD, os.path.join(HERE, "gather_host.cpp"), "-o", so])
    L = C.CDLL(so)
    i64, i64p = C.c_int64, C.POINTER(C.c_int64)
    L.gather_plan.restype = i64
    L.gather_plan.argtypes = [i64, i64, i64, i64p, i64p]
    L.gather_tile_ok.restype = C.c_int
    L.gather_tile_ok.argtypes = [i64]
    L.gather_chunk_rows.restype = i64
    L.gather_chunk_rows.argtypes = [i64, i64]
    L.gather_chunks.restype = i64
    L.gather_chunks.argtypes = [i64, i64, i64, i64, i64p]
    L.gather_check.restype = C.c_int
    L.gather_check.argtypes = [C.c_int, C.c_int, i64, i64, C.c_int, i64, C.c_char_p, C.c_size_t]
    return L


# ---- the tile planner -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 128, 4096])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 1000001])
def test_tiles_cover_the_entries_once_in_order(gather_host, n, tile):
    want = -(-n // tile)
    spans = np.full((want + 1, 2), -1, dtype=np.int64)
    used = C.c_int64(0)
    tiles = gather_host.gather_plan(n, tile, want + 1, spans.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(used))
    assert tiles == want and used.value == tile
    assert (spans[want:] == -1).all()                                          # nothing behind the last tile
    lo, hi = spans[:want, 0], spans[:want, 1]
    assert np.array_equal(lo, np.arange(want, dtype=np.int64) * tile)          # in order, each begins where the one before ends
    assert np.array_equal(hi[:-1], lo[1:]) and (want == 0 or hi[-1] == n)      # exactly once, up to n
    assert np.all(hi[:-1] - lo[:-1] == tile)                                   # whole tiles but the last
    if want:
        assert 1 <= hi[-1] - lo[-1] <= tile


def test_tile_option(gather_host):
    used = C.c_int64(0)
    spans = np.zeros((300, 2), dtype=np.int64)
    tiles = gather_host.gather_plan(1000001, 0, 300, spans.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(used))
    assert used.value >= 64 and used.value % 64 == 0 and used.value <= 65536 and tiles == -(-1000001 // used.value)      # the automatic tile
    assert all(gather_host.gather_tile_ok(v) for v in (0, 64, 128, 4096, 65536))
    assert not any(gather_host.gather_tile_ok(v) for v in (-64, 1, 32, 63, 65, 96, 65536 + 64, 1 << 20))


# ---- the chunk split ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 1000])
def test_chunks_cover_the_window_once_in_order(gather_host, rows):
    n_pass = 5003
    for first, count in [(0, 1), (0, 7), (0, 1000), (0, 1001), (0, n_pass), (n_pass - 1, 1), (n_pass - 1001, 1001), (n_pass, 0), (0, 0),
                         (2500, 1), (2500, 999), (2500, 1000), (2499, 2003)]:
        want = -(-count // rows)
        chunks = np.full((want + 1, 2), -1, dtype=np.int64)
        nc = gather_host.gather_chunks(first, count, rows, want + 1, chunks.ctypes.data_as(C.POINTER(C.c_int64)))
        assert nc == want and (chunks[want:] == -1).all(), (first, count)
        lo, n = chunks[:want, 0], chunks[:want, 1]
        assert np.all(n >= 1) and np.all(n <= rows), (first, count)           # no chunk over the limit, none empty
        covered = np.concatenate([np.arange(a, a + b) for a, b in zip(lo, n)]) if want else np.zeros(0, dtype=np.int64)
        assert np.array_equal(covered, np.arange(first, first + count)), (first, count)


def test_automatic_chunk_is_128_mib(gather_host):
    for row in (13, 18, 19, 87, 308):
        rows = gather_host.gather_chunk_rows(0, row)
        assert rows * row * 8 <= 128 << 20 < (rows + 1) * row * 8
    assert gather_host.gather_chunk_rows(0, 1 << 40) == 1                      # a row that does not fit: one row at a time
    assert gather_host.gather_chunk_rows(1000, 18) == 1000


# ---- the argument check ---------------------------------------------------------------------------------------------------------
def _check(L, select=1, kind=0, first=0, count=1, records=1, n_pass=-1):
    why = C.create_string_buffer(512)
    st = L.gather_check(select, kind, first, count, records, n_pass, why, len(why))
    return st, why.value.decode()


def test_argument_check_accepts(gather_host):
    for kw in (dict(), dict(kind=2, first=5, count=0, records=0), dict(first=3, count=4, n_pass=7), dict(first=7, count=0, records=0, n_pass=7),
               dict(first=0, count=0, records=0, n_pass=0)):
        assert _check(gather_host, **kw) == (0, ""), kw


@pytest.mark.parametrize("kw,field", [
    (dict(select=0), "select"),
    (dict(kind=-1), "kind"),
    (dict(kind=3), "kind"),
    (dict(records=0), "records"),
    (dict(first=-1), "first"),
    (dict(count=-1), "count"),
    (dict(first=3, count=5, n_pass=7), "n_pass"),
    (dict(first=8, count=0, n_pass=7), "n_pass"),
    (dict(first=0, count=1, n_pass=0), "n_pass"),
    (dict(first=2 ** 63 - 1, count=2 ** 63 - 1, n_pass=7), "n_pass"),
])
def test_argument_check_refuses_and_names_the_function_and_the_field(gather_host, kw, field):
    st, why = _check(gather_host, **kw)
    assert st == -2 and why.startswith(FN + ":") and field in why, why


# ---- through the built library ---------------------------------------------------------------------------------------------------
def test_library_refuses_a_null_selection():
    from polycap_amd import _cabi
    L = _cabi.lib()
    rec = np.zeros(18)
    st = L.pc_hip_select_gather(None, 0, 0, 1, rec.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert st == _cabi.PC_HIP_ERR_INVALID
    msg = (L.pc_hip_last_error() or b"").decode()
    assert msg.startswith(FN) and "select" in msg, msg
    assert L.pc_hip_select_gather(None, 0, 0, 0, None, None) == _cabi.PC_HIP_ERR_INVALID


# ---- the host part under the sanitizers -----------------------------------------------------------------------------------------
def test_host_part_is_clean_under_the_sanitizers(tmp_path):
    """tests/gather/gather_host.cpp with its own main, built with -fsanitize=address,undefined, run once: nothing is loaded into python"""
    exe = str(tmp_path / "gather_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DGATHER_HOST_MAIN", "-I", INCLUDE, "-I", HIPD, os.path.join(HERE, "gather_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gather_host: 0 failures" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


# ---- the public call's variable: refused before any device is used --------------------------------------------------------------
@pytest.mark.parametrize("value", ["0", "-1", "abc", "2147483648"])
def test_public_call_rejects_bad_select_records_variable(value, monkeypatch):
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.setenv("POLYCAP_SELECT", EXAMPLE_SELECT)
    monkeypatch.setenv("POLYCAP_SELECT_RECORDS", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SELECT_RECORDS") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert value in str(e.value), str(e.value)


def test_public_call_rejects_select_records_without_select(monkeypatch):
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.delenv("POLYCAP_SELECT", raising=False)
    monkeypatch.setenv("POLYCAP_SELECT_RECORDS", "500")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SELECT_RECORDS") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert "POLYCAP_SELECT" in str(e.value).replace("POLYCAP_SELECT_RECORDS", ""), str(e.value)


def test_select_records_getter_fails_without_the_variable():
    """a result made elsewhere (from totals) carries no rows: the getter says which variable was missing"""
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.full(291, 0.5), [10, 5, 3, 40, 0, 0])
    with pytest.raises(ValueError, match="POLYCAP_SELECT_RECORDS"):
        eff.select_records()
