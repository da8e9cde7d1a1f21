"""Selections without a GPU (pc_hip_select_*, Selection): pc_select_pass of polycap_amd/csrc/hip/pc_select.h, compiled for the host,
against a numpy restatement of the contract in include/polycap-hip.h on synthetic entries of both kinds; pc_hip_select_validate
field by field; the parser of the cut grammar; and the host part once under the address and undefined-behaviour sanitizers, as a
program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_hist_cpu import DX, DY, DZ, DT, HIPD, N, SX, SY, X, Y, Z, np_bins
from tests.test_joint_cpu import EXIT_ONLY, FIELD, QUANTITIES, np_value2
from tests.test_spot_cpu import np_exit_dz

HERE = os.path.join(ROOT, "tests", "select")
INCLUDE = os.path.join(ROOT, "include")
USES_DZ = (0, 1, 2, 3, 4, 5)


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------
def cut(name, lo, hi, d=0., centre=(0., 0.), negate=False):
    c = dict(axis=name, d=d, centre=centre, range=(lo, hi))
    c["not"] = negate
    return c


def np_inside(c, E, leak, ze=0.):
    """inside = bin 0 of the one-bin axis over the cut's range"""
    v, ok = np_value2(QUANTITIES.index(c["axis"]), E, leak, ze + c["d"], *c["centre"])
    return np_bins(v, ok, c["range"][0], c["range"][1], 1) == 0


def np_pass(cuts, E, leak, ze=0.):
    """every cut: inside XOR not"""
    p = np.ones(len(E), dtype=bool)
    for c in cuts:
        p &= np_inside(c, E, leak, ze) ^ bool(c["not"])
    return p


# ---- the host compile of pc_select.h --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("select_host")), "select_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", INCLUDE, "-I", HIPD,
                           os.path.join(HERE, "select_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.select_pass_n.restype = C.c_int
    L.select_pass_n.argtypes = [C.c_int64, dp, C.c_int, C.c_int, dp, C.c_double, C.POINTER(C.c_uint8)]
    L.select_parse.restype = C.c_int
    L.select_parse.argtypes = [C.c_char_p, dp, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    return L


def host_pass(L, cuts, E, leak, ze=0.):
    E = np.ascontiguousarray(E, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    rows = np.array([[QUANTITIES.index(c["axis"]), c["d"], c["centre"][0], c["centre"][1], c["range"][0], c["range"][1], 1. if c["not"] else 0.]
                     for c in cuts], dtype=np.float64)
    out = np.zeros(len(E), dtype=np.uint8)
    st = L.select_pass_n(len(E), E.ctypes.data_as(dp), int(leak), len(cuts), rows.ctypes.data_as(dp), ze, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert st == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool)


def synthetic(c, n=20000, seed=5):
    """(E, n): n entries whose value of the cut's quantity spreads over and beyond its range; then rows with the value exactly on lo,
    one ulp below lo, one ulp below hi and on hi (dz = 1, z = zp, nothing else set: every formula returns the planted number itself);
    then NaN in every field; then dz = 0, -0, negative, infinite"""
    q = QUANTITIES.index(c["axis"])
    f = FIELD[q]
    lo, hi = c["range"]
    span = hi - lo
    rng = np.random.default_rng(seed + q)
    E = rng.normal(0., 0.05, (n, 10))
    E[:, DZ] = np.where(rng.random(n) < 0.7, np_exit_dz(np.clip(E[:, DX], -0.7, 0.7), np.clip(E[:, DY], -0.7, 0.7)), rng.uniform(-0.2, 1., n))
    E[:, f] = rng.uniform(lo - 0.3 * span, hi + 0.3 * span, n)
    if f == N:
        E[:, f] = np.floor(E[:, f])
    if c["axis"] == "r":
        E[:, Y] = c["centre"][1] + rng.normal(0., 0.1 * span, n)
    if c["axis"] == "tan_theta":
        E[:, DY] = rng.normal(0., 0.1 * span, n)
    if f != Z:
        E[:, Z] = c["d"] + rng.normal(0., 1e-3, n)
    edges = [lo, np.nextafter(lo, -np.inf), np.nextafter(hi, -np.inf), hi]
    S = np.zeros((4, 10))
    S[:, DZ] = 1.
    S[:, Z] = c["d"] if f != Z else 0.
    S[:, f] = edges
    nan_rows = E[:10].copy()
    for k in range(10):
        nan_rows[k, k] = np.nan
    bad_dz = E[10:16].copy()
    bad_dz[:, DZ] = [0., -0., -0.5, -1., np.inf, -np.inf]
    return np.concatenate([E, S, nan_rows, bad_dz]), n


# exact binary edges, so that the rows planted on lo and hi are on them after the formula
CUTS = [cut("x", -0.5, 1.5, d=0.5), cut("y", -0.25, 0.75, d=0.125), cut("r", 0.25, 1.25, d=0.25), cut("slope_x", -0.5, 0.25),
        cut("slope_y", -0.125, 0.5), cut("tan_theta", 0.125, 0.625), cut("nrefl", 3., 40.), cut("dtravel", 3., 7.), cut("r_start", 0.25, 0.5),
        cut("z", 0.5, 9.5), cut("start_x", -0.25, 0.5), cut("start_y", -1., 0.125)]


@pytest.mark.parametrize("k", range(len(CUTS)))
def test_one_cut_equals_the_contract(select_host, k):
    c = CUTS[k]
    q = QUANTITIES.index(c["axis"])
    E, n = synthetic(c)
    for leak in (0, 1):
        for negate in (False, True):
            cc = dict(c)
            cc["not"] = negate
            got = host_pass(select_host, [cc], E, leak)
            assert np.array_equal(got, np_pass([cc], E, leak)), (c["axis"], leak, negate)
            if leak and q in EXIT_ONLY:
                assert got.all() == negate and got.any() == negate          # a quantity the kind does not have: never inside
            else:
                assert 1000 < got[:n].sum() < n - 1000                       # a real cut: some pass, some do not
    got = host_pass(select_host, [c], E, 0)
    # on lo: inside; one ulp below lo: not; on hi: not; one ulp below hi: inside where v - lo is still below hi - lo after rounding
    lo, hi = c["range"]
    assert got[n:n + 4].tolist() == [True, False, bool(np.nextafter(hi, -np.inf) - lo < hi - lo), False], c["axis"]
    tail = got[n + 4:]
    assert not tail[FIELD[q]]                                                   # NaN in the field the quantity reads
    if q in USES_DZ:
        assert not tail[DZ] and not tail[10:14].any() and not tail[15]           # NaN, 0, -0, negative, -inf
    # negated, every one of those passes: not inside XOR negate
    cn = dict(c)
    cn["not"] = True
    assert np.array_equal(host_pass(select_host, [cn], E, 0), ~got)


def test_cuts_are_anded(select_host):
    rng = np.random.default_rng(17)
    cuts = [cut("r", 0., 0.06, d=0.25, centre=(0.01, -0.01)), cut("nrefl", 0., 1., negate=True), cut("tan_theta", 0., 0.05),
            cut("r_start", 0.02, 1.), cut("slope_x", -0.03, 0.04), cut("z", -0.05, 0.06), cut("start_x", -0.04, 0.2), cut("dtravel", -0.1, 0.02)]
    E = rng.normal(0., 0.05, (30000, 10))
    E[:, DZ] = np.where(rng.random(len(E)) < 0.8, np_exit_dz(E[:, DX], E[:, DY]), rng.uniform(-0.2, 1., len(E)))
    E[:, N] = np.floor(rng.uniform(0., 5., len(E)))
    E[::101, rng.integers(0, 10, len(E[::101]))] = np.nan
    for m in range(1, 9):
        for leak in (0, 1):
            got = host_pass(select_host, cuts[:m], E, leak)
            want = np_pass(cuts[:m], E, leak)
            assert np.array_equal(got, want), (m, leak)
            if not leak:
                assert 0 < got.sum() < len(E)
            elif m >= 4:
                assert not got.any()                                           # r_start on a leak kind, not negated: nothing passes
    # the complement of one cut: S and S with that cut negated split what the other cuts pass
    for leak in (0, 1):
        a = host_pass(select_host, cuts[:3], E, leak)
        neg = [cuts[0], cuts[1], dict(cuts[2], **{"not": True})]
        b = host_pass(select_host, neg, E, leak)
        assert not (a & b).any() and np.array_equal(a | b, host_pass(select_host, cuts[:2], E, leak))


# ---- pc_hip_select_validate -----------------------------------------------------------------------------------------------------
def _spec(cuts, n_cuts=None, patch=None):
    from polycap_amd import _cabi
    from polycap_amd.hip import select_cuts
    arr = select_cuts(cuts)
    if patch:
        patch(arr)
    return _cabi.SelectSpecS(len(cuts) if n_cuts is None else n_cuts, arr), arr


def _validate(cuts, n_cuts=None, patch=None):
    from polycap_amd import _cabi
    L = _cabi.lib()
    spec, keep = _spec(cuts, n_cuts, patch)
    st = L.pc_hip_select_validate(C.byref(spec))
    return st, (L.pc_hip_last_error() or b"").decode()


GOOD = dict(axis="r", d=0.5, centre=(0.001, -0.002), range=(0., 0.005))


def test_validate_accepts():
    assert _validate([GOOD])[0] == 0
    assert _validate([dict(axis=q, range=(0, 1)) for q in QUANTITIES[:8]])[0] == 0
    assert _validate([dict(axis=q, range=(-1e300, 1e300), **{"not": True}) for q in QUANTITIES[8:]])[0] == 0
    assert _validate([("nrefl", (0, 40)), ("x", (-1, 1), 0.5), ("r", (0, 1), 0.5, (0.1, 0.2), True)])[0] == 0


def _set(k, field, value):
    def patch(arr):
        if field == "negate":
            arr[k].negate = value
        else:
            setattr(arr[k].axis, field, value)
    return patch


@pytest.mark.parametrize("cuts,kw,fields", [
    ([], {}, ["n_cuts"]),
    ([GOOD] * 9, {}, ["n_cuts"]),
    ([GOOD], dict(patch=_set(0, "quantity", -1)), ["cut 0", "quantity"]),
    ([GOOD, GOOD], dict(patch=_set(1, "quantity", 12)), ["cut 1", "quantity"]),
    ([GOOD, dict(axis="nrefl", d=0.5, range=(0, 40))], {}, ["cut 1", " d "]),
    ([dict(GOOD, d=-1.)], {}, ["cut 0", " d "]),
    ([dict(GOOD, d=float("inf"))], {}, ["cut 0", " d "]),
    ([dict(axis="x", centre=(0.1, 0.), range=(0, 1))], {}, ["cut 0", "cx"]),
    ([GOOD, GOOD, dict(GOOD, centre=(0., float("nan")))], {}, ["cut 2", "cy"]),
    ([dict(GOOD, range=(0.01, 0.01))], {}, ["cut 0", "lo"]),
    ([GOOD, dict(GOOD, range=(0.02, 0.01))], {}, ["cut 1", "lo"]),
    ([dict(GOOD, range=(0., float("inf")))], {}, ["cut 0", "hi"]),
    ([GOOD] * 8, dict(patch=_set(7, "n_bins", 2)), ["cut 7", "n_bins"]),
    ([GOOD], dict(patch=_set(0, "n_bins", 0)), ["cut 0", "n_bins"]),
    ([GOOD, GOOD], dict(patch=_set(1, "negate", 2)), ["cut 1", "negate"]),
    ([GOOD], dict(patch=_set(0, "negate", -1)), ["cut 0", "negate"]),
])
def test_validate_refuses_and_names_the_cut_and_the_field(cuts, kw, fields):
    st, msg = _validate(cuts, **kw)
    assert st == -2, (cuts, kw)
    assert msg.startswith("pc_hip_select_validate") and all(f in msg for f in fields), msg


def test_validate_refuses_null():
    from polycap_amd import _cabi
    L = _cabi.lib()
    assert L.pc_hip_select_validate(None) == -2
    spec = _cabi.SelectSpecS(1, None)
    assert L.pc_hip_select_validate(C.byref(spec)) == -2 and b"n_cuts" in L.pc_hip_last_error()


def test_cuts_from_dicts_and_tuples():
    from polycap_amd.hip import select_cuts
    arr = select_cuts([dict(axis="r", d=0.5, centre=(0.1, 0.2), range=(0, 0.005)), ("nrefl", (0, 40), 0., (0., 0.), True),
                       {"axis": 10, "range": (-1, 1), "not": True}])
    got = [(c.axis.quantity, c.axis.d, c.axis.cx, c.axis.cy, c.axis.lo, c.axis.hi, c.axis.n_bins, c.negate) for c in arr]
    assert got == [(2, 0.5, 0.1, 0.2, 0., 0.005, 1, 0), (6, 0., 0., 0., 0., 40., 1, 1), (10, 0., 0., 0., -1., 1., 1, 1)]
    with pytest.raises(ValueError):
        select_cuts([dict(axis="r", range=(0, 1), bins=4)])
    with pytest.raises(ValueError):
        select_cuts([dict(axis="start_z", range=(0, 1))])
    with pytest.raises(ValueError):
        select_cuts([dict(axis="r", range=(0, 1), window=1)])


# ---- the parser -----------------------------------------------------------------------------------------------------------------
EXAMPLE_SELECT = "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not"


def _host_parse(L, value):
    rows = np.zeros((8, 7))
    n = C.c_int(0)
    why = C.create_string_buffer(512)
    st = L.select_parse(value.encode(), rows.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), why, len(why))
    return st, rows[:n.value], why.value.decode()


def test_the_example_parses_to_its_cuts(select_host):
    from polycap_amd.hip import select_parse
    want = [dict(axis="r", d=0.5, centre=(0., 0.), range=(0., 0.005)), dict(axis="nrefl", d=0., centre=(0., 0.), range=(0., 40.))]
    want[0]["not"], want[1]["not"] = False, True
    assert select_parse(EXAMPLE_SELECT) == want
    st, rows, why = _host_parse(select_host, EXAMPLE_SELECT)
    assert st == 0 and why == "" and rows.tolist() == [[2, 0.5, 0, 0, 0, 0.005, 0], [6, 0, 0, 0, 0, 40, 1]]
    got = select_parse("axis=start_y,not,range=-0.25:1e-3;;axis=x,range=-1:1,d=0.125;")
    assert [(c["axis"], c["range"], c["d"], c["not"]) for c in got] == [("start_y", (-0.25, 1e-3), 0., True), ("x", (-1., 1.), 0.125, False)]
    assert len(select_parse(";".join(["axis=z,range=0:1"] * 8))) == 8


BAD = [
    ("", "at least one cut"),
    (";;", "at least one cut"),
    ("energies=all", "item 0: every item must be a cut"),
    ("axis=r,range=0:1;window=1", "item 1: every item must be a cut"),
    (EXAMPLE_SELECT.replace("nrefl", "n_refl"), "item 1: axis must be one of"),
    ("axis=x", "item 0: a cut needs axis and range"),
    ("axis=x,range=0:1,bins=4", "item 0: unknown key"),
    ("axis=x,range=0:1,never", "item 0: every part of a cut"),
    ("axis=x,range=0", "item 0: range must be LO:HI"),
    ("axis=x,range=0:1x", "item 0: range must be LO:HI"),
    ("axis=x,range=0:1,d=far", "item 0: d must be"),
    ("axis=r,range=0:1,centre=0", "item 0: centre must be"),
    ("axis=x,range=0:1;axis=nrefl,d=0.5,range=0:40", "cut 1: d "),
    ("axis=x,range=1:0", "cut 0: lo"),
    ("axis=x,centre=0.1:0,range=0:1", "cut 0: cx"),
    (";".join(["axis=z,range=0:1"] * 9), "item 8: at most 8 cuts"),
]


@pytest.mark.parametrize("value,what", BAD)
def test_parser_refuses_with_the_reason(select_host, value, what):
    from polycap_amd.hip import select_parse
    with pytest.raises(ValueError, match="POLYCAP_SELECT") as e:
        select_parse(value)
    assert what in str(e.value), str(e.value)
    st, rows, why = _host_parse(select_host, value)
    assert st == -1 and what in why, why


# ---- the host part under the sanitizers -----------------------------------------------------------------------------------------
def test_host_part_is_clean_under_the_sanitizers(tmp_path):
    """tests/select/select_host.cpp with its own main, built with -fsanitize=address,undefined, run once: nothing is loaded into python"""
    exe = str(tmp_path / "select_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSELECT_HOST_MAIN", "-I", INCLUDE, "-I", HIPD, os.path.join(HERE, "select_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "select_host: 0 failures" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


# ---- the public call's variable -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,what", BAD)
def test_public_call_rejects_bad_select_variable(value, what, monkeypatch):
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.setenv("POLYCAP_SELECT", value)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(ValueError, match="POLYCAP_SELECT") as e:
        src.get_transmission_efficiencies(1, 1000)
    assert what in str(e.value), str(e.value)


def test_public_call_with_select_needs_a_device(monkeypatch):
    import polycap_amd
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    if polycap_amd.device_count() > 0:
        return
    monkeypatch.setenv("POLYCAP_SELECT", EXAMPLE_SELECT)
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    with pytest.raises(RuntimeError, match="HIP"):
        src.get_transmission_efficiencies(1, 1000)


def test_select_getter_fails_without_the_variable():
    """a result made elsewhere (from totals) carries no selection: the getter says which variable was missing"""
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))
    eff = capi.TransmissionEfficiencies.from_totals(src, np.full(291, 0.5), [10, 5, 3, 40, 0, 0])
    with pytest.raises(ValueError, match="POLYCAP_SELECT"):
        eff.select()
