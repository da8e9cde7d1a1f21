"""Draws without a GPU (pc_hip_select_draw, Selection.draw, POLYCAP_DRAW): the shared first part of polycap_amd/csrc/hip/pc_draw.h
compiled for the host -- the thresholds t_k on 32/64-bit limbs and their inverse K(c), the very arithmetic the device runs -- equal,
not close, to Python integers; the model of tests/draw/model.py, the yardstick of the GPU tests, against the contract's properties;
the argument and window checks; the refusals of the built library that need no device; the host part once under the address and
undefined-behaviour sanitizers, as a program of its own; and the public call's variable, refused before any device is used."""
import ctypes as C
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.draw import model
from tests.test_hist_cpu import HIPD

HERE = os.path.join(ROOT, "tests", "draw")
INCLUDE = os.path.join(ROOT, "include")
FN = "pc_hip_select_draw"

TS = [1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, (2 ** 32 - 1) * 2 ** 32]
NS = [1, 2, 3, 2 ** 16 + 1, 2 ** 31 - 1]
PHASES = [0, 1, 2 ** 31, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def draw_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("draw_host")), "draw_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", INCLUDE, "-I", HIPD, os.path.join(HERE, "draw_host.cpp"), "-o", so])
    L = C.CDLL(so)
    i64, u64, u32, u64p = C.c_int64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)
    L.draw_thresholds.restype = None
    L.draw_thresholds.argtypes = [i64, u64p, u32, u64, u64, u64p]
    L.draw_belows.restype = None
    L.draw_belows.argtypes = [i64, u64p, u32, u64, u64, u64p]
    L.draw_mul64.restype = None
    L.draw_mul64.argtypes = [u64, u64, u64p, u64p]
    L.draw_range.restype = None
    L.draw_range.argtypes = [u64, u64, u32, u64, u64, u64, u64, u64p, u64p]
    L.draw_check.restype = C.c_int
    L.draw_check.argtypes = [C.c_int, C.c_int, i64, i64, i64, i64, i64, C.c_int, C.c_int, u64, C.c_char_p, C.c_size_t]
    return L


def _vec(fn, xs, phase, T, N):
    a = np.array(xs, dtype=np.uint64)
    out = np.zeros(len(xs), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    fn(len(xs), a.ctypes.data_as(u64p), phase, T, N, out.ctypes.data_as(u64p))
    return [int(v) for v in out]


def thresholds(L, ks, phase, T, N):
    return _vec(L.draw_thresholds, ks, phase, T, N)


def belows(L, cs, phase, T, N):
    return _vec(L.draw_belows, cs, phase, T, N)


# ---- the arithmetic against Python integers ---------------------------------------------------------------------------------------
def test_product_of_two_words(draw_host):
    rng = random.Random(5)
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    edge = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    pairs = [(a, b) for a in edge for b in edge] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(2000)]
    for a, b in pairs:
        draw_host.draw_mul64(a, b, C.byref(lo), C.byref(hi))
        assert (hi.value << 64) | lo.value == a * b, (a, b)


@pytest.mark.parametrize("T", TS)
def test_thresholds_equal_python_integers_on_the_grid(draw_host, T):
    for N in NS:
        for r in PHASES:
            ks = sorted({0, min(1, N - 1), N // 2, N - 1})
            got = thresholds(draw_host, ks, r, T, N)
            want = [model.threshold(k, r, T, N) for k in ks]
            assert got == want, (T, N, r)
            assert all(t < T for t in got) and got == sorted(got), (T, N, r)
            # K is the exact inverse: at 0, 1 and T, and around every threshold
            cs = sorted({0, 1, T} | {c for t in got for c in (t - 1, t, t + 1) if 0 <= c <= T})
            gotK = belows(draw_host, cs, r, T, N)
            assert gotK == [model.below(c, r, T, N) for c in cs], (T, N, r)
            assert gotK[0] == 0 and gotK[-1] == N
            for k, t in zip(ks, got):                    # K(t_k) <= k < K(t_k + 1)
                a, b = belows(draw_host, [t, t + 1], r, T, N)
                assert a <= k < b, (T, N, r, k)


def test_small_cases_by_enumeration(draw_host):
    """every k and every c of small T and N: K(c) counts the thresholds below c, as a count and not through model.below"""
    for T in (1, 2, 3, 7, 10, 64):
        for N in (1, 2, 3, 5, 17, 100):
            for r in (0, 1, 2 ** 31, 2 ** 32 - 1, 123456789):
                ts = thresholds(draw_host, list(range(N)), r, T, N)
                assert ts == [model.threshold(k, r, T, N) for k in range(N)]
                assert ts == sorted(ts) and ts[-1] < T
                cs = list(range(T + 1))
                want = [sum(1 for t in ts if t < c) for c in cs]
                assert belows(draw_host, cs, r, T, N) == want, (T, N, r)
                assert [model.below(c, r, T, N) for c in cs] == want, (T, N, r)


def test_random_thresholds_and_inverses(draw_host):
    rng = random.Random(20)
    for _ in range(4000):
        T = rng.choice([rng.randrange(1, 2 ** 64 - 2 ** 32 + 1), rng.randrange(1, 2 ** 40), rng.randrange(1, 2 ** 20)])
        N = rng.choice([rng.randrange(1, 2 ** 31), rng.randrange(1, 2 ** 12)])
        r = rng.getrandbits(32)
        k = rng.randrange(N)
        (t,) = thresholds(draw_host, [k], r, T, N)
        assert t == model.threshold(k, r, T, N) and t < T, (T, N, r, k)
        if k + 1 < N:
            assert thresholds(draw_host, [k + 1], r, T, N)[0] >= t
        c = rng.randrange(T + 1)
        cs = [c, t, t + 1]
        assert belows(draw_host, cs, r, T, N) == [model.below(x, r, T, N) for x in cs], (T, N, r, c)


def test_ranges_of_consecutive_bounds_tile_the_window(draw_host):
    """the draws of the cumulative ranges [c_j, c_j+1) cut to a window are the window, each draw once: what members and tiles rely on"""
    rng = random.Random(7)
    a, b = C.c_uint64(0), C.c_uint64(0)
    for _ in range(200):
        T = rng.randrange(1, 2 ** 50)
        N = rng.randrange(1, 5000)
        r = rng.getrandbits(32)
        first = rng.randrange(N + 1)
        count = rng.randrange(N - first + 1)
        bounds = sorted({0, T} | {rng.randrange(T + 1) for _ in range(6)})
        at = first
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            draw_host.draw_range(lo, hi, r, T, N, first, count, C.byref(a), C.byref(b))
            assert a.value <= b.value
            if b.value > a.value:
                assert a.value == at
                at = b.value
            for k in range(a.value, b.value):
                assert lo <= model.threshold(k, r, T, N) < hi
        assert at == first + count


# ---- the model, the yardstick of the GPU tests ---------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(11)
    n = 300
    q = lambda w: [int(v) for v in model.quantise(w)]
    zeros = rng.random(n)
    zeros[rng.random(n) < 0.6] = 0.
    dominant = rng.random(n) * 1e-6
    dominant[137] = 1.0
    single = np.zeros(n)
    single[211] = 0.37
    return dict(random=q(rng.random(n)), zeros=q(zeros), dominant=q(dominant), equal=q(np.full(n, 0.25)), single=q(single),
                tiny=[1, 0, 0, 2, 0, 1], full=[2 ** 32] * 40)


@pytest.mark.parametrize("name", list(_cases()))
def test_model_has_the_contracts_properties(name):
    V = _cases()[name]
    T = sum(V)
    rng = random.Random(3)
    for N in (1, 2, 7, len(V), 5 * len(V) + 3):
        for r in (0, 2 ** 32 - 1, rng.getrandbits(32)):
            pairs = model.positions(V, N, r)
            assert [k for k, _ in pairs] == list(range(N))                      # every draw lands, once
            pos = [p for _, p in pairs]
            assert pos == sorted(pos)
            vec, T2 = model.draw(np.array(V, dtype=np.uint64), N, r)
            assert T2 == T and [int(p) for p in vec] == pos                     # the vectorised form the GPU tests use
            mult = np.bincount(pos, minlength=len(V))
            assert mult.sum() == N
            for i, v in enumerate(V):
                assert N * v // T <= mult[i] <= -((-N * v) // T), (name, N, r, i)      # floor and ceil of N V_i / T, in integers
                assert v > 0 or mult[i] == 0
            # any split of the window
            cuts = sorted({0, N} | {rng.randrange(N + 1) for _ in range(3)})
            parts = [model.positions(V, N, r, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
            assert [x for p in parts for x in p] == pairs
            # any split of the entries into members with bases
            seams = sorted({0, len(V)} | {rng.randrange(len(V) + 1) for _ in range(3)})
            merged = []
            for a, b in zip(seams[:-1], seams[1:]):
                merged += [(k, a + p) for k, p in model.positions(V[a:b], N, r, base=sum(V[:a]), total=T)]
            assert merged == pairs


def test_quantise_is_round_half_even_of_w_times_two_to_32():
    w = np.array([0., 1., 0.5, 2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** -34, -1., np.nan, 0.1])
    want = [0, 2 ** 32, 2 ** 31, 0, 2, 0, 0, 0, round(Fraction(0.1) * 2 ** 32)]
    assert [int(v) for v in model.quantise(w)] == want


# ---- the argument and window checks ------------------------------------------------------------------------------------------------
def _check(L, select=1, kind=0, energy=0, ne=3, n=100, first=0, count=1, records=1, total=None):
    why = C.create_string_buffer(512)
    st = L.draw_check(select, kind, energy, ne, n, first, count, records, total is not None, total or 0, why, len(why))
    return st, why.value.decode()


def test_argument_check_accepts(draw_host):
    for kw in (dict(), dict(kind=2, energy=2, first=5, count=0, records=0), dict(n=1, count=1, total=1), dict(n=2 ** 31 - 1, first=2 ** 31 - 101, count=100, total=7),
               dict(first=100, count=0, records=0, total=9), dict(first=0, count=100, total=2 ** 64 - 1)):
        assert _check(draw_host, **kw) == (0, ""), kw


@pytest.mark.parametrize("kw,field", [
    (dict(select=0), "select"),
    (dict(kind=-1), "kind"),
    (dict(kind=3), "kind"),
    (dict(energy=-1), "energy"),
    (dict(energy=3), "energy"),
    (dict(n=0), "n_draw"),
    (dict(n=-5), "n_draw"),
    (dict(n=2 ** 31), "n_draw"),
    (dict(records=0), "records"),
    (dict(first=-1), "first"),
    (dict(count=-1), "count"),
    (dict(first=98, count=3, total=5), "n_draw"),
    (dict(first=101, count=0, total=5), "n_draw"),
    (dict(first=2 ** 63 - 1, count=2 ** 63 - 1, total=5), "n_draw"),
    (dict(total=0), "no weight to draw from"),
])
def test_argument_check_refuses_and_names_the_function_and_the_field(draw_host, kw, field):
    st, why = _check(draw_host, **kw)
    assert st == -2 and why.startswith(FN + ":") and field in why, why


# ---- through the built library ---------------------------------------------------------------------------------------------------
def test_library_refuses_a_null_selection():
    from polycap_amd import _cabi
    L = _cabi.lib()
    rec = np.zeros(18)
    total = C.c_uint64(77)
    st = L.pc_hip_select_draw(None, 0, 0, 10, 0, 0, 1, rec.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(total))
    assert st == _cabi.PC_HIP_ERR_INVALID and total.value == 77
    msg = (L.pc_hip_last_error() or b"").decode()
    assert msg.startswith(FN) and "select" in msg, msg
    assert L.pc_hip_select_draw(None, 0, 0, 10, 0, 0, 0, None, None, None) == _cabi.PC_HIP_ERR_INVALID


def test_select_all_is_one_cut_that_parses_and_validates():
    import polycap_amd
    from polycap_amd import _cabi, hip
    cuts = polycap_amd.select_all()
    assert len(cuts) == 1 and cuts[0]["axis"] == "nrefl" and tuple(cuts[0]["range"]) == (0., 2.0 ** 62)
    arr = hip.select_cuts(cuts)
    assert _cabi.lib().pc_hip_select_validate(C.byref(_cabi.SelectSpecS(1, arr))) == _cabi.PC_HIP_OK


# ---- the public call's variable: refused before any device is used --------------------------------------------------------------
@pytest.mark.parametrize("value,what", [
    ("", "empty"),
    ("n=100,colour=3", "colour: unknown key"),
    ("n=100,phase", "phase: unknown key"),
    ("100", "100: unknown key"),
    ("energy=0,phase=5", "n is missing"),
    ("n=0", "n=0: must be an integer in 1 .. 2^31 - 1"),
    ("n=-3", "n=-3"),
    ("n=2147483648", "n=2147483648"),
    ("n=abc", "n=abc"),
    ("n=1e5", "n=1e5"),
    ("n=100,energy=-1", "energy=-1: must be an index into the source's 291 energies"),
    ("n=100,energy=291", "energy=291"),
    ("n=100,energy=x", "energy=x"),
    ("n=100,phase=-1", "phase=-1: must be a uint32"),
    ("n=100,phase=4294967296", "phase=4294967296"),
    ("n=100,phase=1.5", "phase=1.5"),
    ("n=100,,phase=1", "unknown key"),
])
def test_public_call_rejects_bad_draw_variable(value, what, monkeypatch):
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.delenv("POLYCAP_SELECT", raising=False)
    monkeypatch.setenv("POLYCAP_DRAW", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_DRAW") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert what in str(e.value) and "polycap_source_get_transmission_efficiencies" in str(e.value), str(e.value)


def test_public_call_refuses_the_draw_variable_behind_the_others(monkeypatch):
    """a bad POLYCAP_DRAW beside another bad variable: the other one's recorded message stays the call's answer"""
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.setenv("POLYCAP_DRAW", "n=0")
    monkeypatch.setenv("POLYCAP_IMAGES", "0")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_IMAGES=0 cannot be combined with leak_calc"):
        src.get_transmission_efficiencies(1, 1000, leak_calc=True)
    monkeypatch.delenv("POLYCAP_IMAGES")
    monkeypatch.setenv("POLYCAP_SELECT", "axis=colour,range=0:1")
    with pytest.raises(ValueError, match="POLYCAP_SELECT=") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert "POLYCAP_DRAW" not in str(e.value)


def test_draw_getter_fails_without_the_variable():
    """a result made elsewhere (from totals) carries no sample: the getter says which variable was missing"""
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.full(291, 0.5), [10, 5, 3, 40, 0, 0])
    with pytest.raises(ValueError, match="POLYCAP_DRAW"):
        eff.draw()


# ---- the host part under the sanitizers -----------------------------------------------------------------------------------------
def test_host_part_is_clean_under_the_sanitizers(tmp_path):
    """tests/draw/draw_host.cpp with its own main, built with -fsanitize=address,undefined, run once: nothing is loaded into python"""
    exe = str(tmp_path / "draw_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DDRAW_HOST_MAIN", "-I", INCLUDE, "-I", HIPD, os.path.join(HERE, "draw_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "draw_host: 0 failures" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
