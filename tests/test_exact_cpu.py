"""The arithmetic of exact sums without a GPU.  polycap_amd/csrc/hip/pc_exact.h alone, compiled for the host (tests/exact/exact_host.cpp),
against Python integers and Fractions; and the library's public host functions that are made of it against tests/golden/exact_functions.json,
recorded from a build of the commit before the header existed (scripts/record_exact_functions.py): every output bit for bit."""
import json
import math
import os
import random
from fractions import Fraction

import pytest

from tests.conftest import GOLDEN
from tests.exact.pyexact import ExactHost, call

with open(os.path.join(GOLDEN, "exact_functions.json")) as f:
    TABLE = json.load(f)

FUNCTIONS = ["pc_hip_fixed_to_double", "pc_hip_efficiencies", "pc_hip_efficiency_stderr", "pc_hip_relay_efficiencies",
             "pc_hip_scan_efficiencies", "pc_hip_tally_stderr", "pc_hip_select_transmission"]
T64, T128 = 2 ** 64, 2 ** 128


def test_the_table_covers_what_it_is_meant_to():
    assert sorted(TABLE) == sorted(FUNCTIONS)
    per = {fn: [inputs for inputs, _ in TABLE[fn]] for fn in FUNCTIONS}
    assert all(len(v) >= 200 for v in per.values())
    f2d = per["pc_hip_fixed_to_double"]
    assert any(i["lo"] == 0 and i["hi"] == 0 for i in f2d) and any(i["hi"] for i in f2d) and any(i["lo"] == T64 - 1 for i in f2d)
    for fn in ("pc_hip_efficiencies", "pc_hip_efficiency_stderr"):
        assert {0, 1, 2} <= {sum(i["counters"][:3]) for i in per[fn]}
    se = per["pc_hip_efficiency_stderr"]
    assert any(0 in i["A"] and 0 in i["B"] for i in se) and any(a >= T64 for i in se for a in i["A"]) and any(a % T64 == T64 - 1 for i in se for a in i["A"])
    # squares below the mean squared: B N < A^2 (both in units of 2^-62), where the variance is clamped to 0
    assert sum(1 for i in se for a, b in zip(i["A"], i["B"]) if sum(i["counters"][:3]) >= 2 and b * sum(i["counters"][:3]) < a * a // 2 ** 62) >= 20
    assert {0, 1, 2} <= {i["counters"][7] for i in per["pc_hip_relay_efficiencies"]} and any(i["B"] is None for i in per["pc_hip_relay_efficiencies"])
    scan = per["pc_hip_scan_efficiencies"]
    assert any(sum(c[:3]) == 0 for i in scan for c in i["counters"]) and any(c[0] + c[2] == 0 < c[1] for i in scan for c in i["counters"])
    assert {0, 1, 2} <= {i["n_started"] for i in per["pc_hip_tally_stderr"]}
    assert any(p + r == 0 for i in per["pc_hip_select_transmission"] for p, r in zip(i["pw"], i["rw"]))


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_public_functions_reproduce_the_recorded_bits(fn):
    for inputs, outputs in TABLE[fn]:
        assert [x.hex() for x in call(fn, inputs)] == outputs, inputs


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ExactHost(tmp_path_factory.mktemp("exact"))


def some_sums(n, seed):
    r = random.Random(seed)
    edge = [0, 1, T64 - 1, T64, T64 + 1, 2 ** 126, T128 - 1, T128 - T64, 2 ** 127]
    return edge + [r.getrandbits(r.randrange(1, 129)) for _ in range(n)]


def test_value_of_a_pair(host):
    assert host.scales() == [2 ** 32, 2 ** 62, 2 ** 64]
    for v in (0, T64 - 1, T64, 2 ** 126):
        assert host.value(v) == v                     # exact: at most 64 significant bits
    for v in some_sums(300, 1):
        hi, lo = divmod(v, T64)
        # hi 2^64 is exact, the one add rounds to 64 bits: to nearest, ties to even
        assert host.value(v) == round_to_bits(v, 64), v
        assert host.value(hi * T64) == hi * T64 and host.value(lo) == lo


def round_to_bits(v, bits):
    n = v.bit_length()
    if n <= bits:
        return v
    q, rem = divmod(v, 1 << (n - bits))
    half = 1 << (n - bits - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return q << (n - bits)


def test_add_carries_and_wraps(host):
    assert host.add(T64 - 1, 1) == T64 and host.add(T128 - 1, 1) == 0 and host.add(T128 - 1, T128 - 1) == T128 - 2
    s = some_sums(200, 2)
    for a, b in zip(s, reversed(s)):
        assert host.add(a, b) == (a + b) % T128
    assert host.add_pairs(s, list(reversed(s))) == [(a + b) % T128 for a, b in zip(s, reversed(s))]


def test_limbs_round_trip(host):
    for v in some_sums(300, 3):
        limbs = host.split(v)
        assert all(0 <= x < 2 ** 32 for x in limbs) and sum(x << (32 * k) for k, x in enumerate(limbs)) == v
        assert host.join(limbs) == v


def test_limb_sums_of_64_members_join_to_the_integer_sum(host):
    r = random.Random(4)
    for worst in (False, True):
        for _ in range(50):
            members = [T128 - 1 if worst else r.getrandbits(r.randrange(1, 129)) for _ in range(64)]
            total = [sum(col) for col in zip(*(host.split(v) for v in members))]
            assert all(0 <= x < 2 ** 38 for x in total)      # 64 limbs below 2^32 each: an int64 all-reduce cannot overflow
            assert host.join(total) == sum(members) % T128


def test_stderr_tail_against_the_exact_rational(host):
    """pc_exact_stderr on m = A / (N 2^62), q = B / (N 2^62), within the bound of tests/test_stderr_cpu.py"""
    r = random.Random(5)
    S = 2 ** 62
    cases = [(4 * S // 2, 4 * S // 4, 4), (S, 0, 2), (0, 0, 2), (2 ** 100, 2 ** 99, 2 ** 40)]
    for _ in range(300):
        N = r.randrange(2, 2 ** r.randrange(2, 50))
        A = r.randrange(0, N * S + 1)
        cases.append((A, r.choice([r.randrange(0, A + 1), A * A // (N * S) // 2]), N))
    for A, B, N in cases:
        got = host.stderr(A, B, N)
        m, q = Fraction(A, N * S), Fraction(B, N * S)
        var = max(q - m * m, Fraction(0)) / (N - 1)
        assert got >= 0.0 and not math.isnan(got)
        tol = Fraction(8, 2 ** 64) * q / (N - 1)
        assert abs(Fraction(got) ** 2 - var) <= tol + Fraction(got) ** 2 * Fraction(1, 2 ** 50), (A, B, N, got, float(var))
    assert host.stderr(S, 0, 2) == 0.0                    # q < m^2: clamped, not NaN
