"""The leak path's skip certificates on the MI355X (tests/devmath/probe.hip, ops WALL, OUTER and HEX: pc_wall_begin, pc_wall_step,
pc_wall_probe, pc_outer_intersect and pc_hex_index called as pc_leak_launch calls them, on the tables pc_build_tables makes): every
output, the trail included, equals the host compile's bit for bit in both modes, and the checks of tests/test_devmath_leak_cpu.py --
soundness against rational arithmetic, agreement with the literal search, the exact first node of the outer scan, the exact hexagon
cell -- hold on the device's own outputs.  Probe launches only, a few thousand rows, no trace kernel.  The device has no unit
counters: the kind of every unit is the host compile's, which the bit-for-bit test ties to the device's trail.  A literal row that
needs more than 200 000 units (the device's cap per lane) is compared with the host compile run to the same cap."""
import functools

import numpy as np
import pytest

from tests.devmath import grid, pyprobe
from tests.test_devmath_leak_cpu import (H, PROFILES, check_hex, check_outer, check_wall_literal, check_wall_outcomes,
                                         check_wall_soundness, hex_case, host_hex, host_outer, host_wall, outer_case, outer_rows,
                                         report, same_bits, wall_case, wall_rows)

pytestmark = pytest.mark.gpu
CAP = pyprobe.WALL_UNITS_DEVICE


@functools.lru_cache(maxsize=None)
def device_wall(name, literal=False):
    return pyprobe.run_wall(wall_case(name)["p"], wall_rows(name, literal, CAP), device=True)


@functools.lru_cache(maxsize=None)
def device_outer(name, literal=False):
    return pyprobe.run_outer(outer_case(name)["p"], outer_rows(name, literal), device=True)


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("name", PROFILES)
def test_wall_device_equals_host_compile_bit_for_bit(name, literal):
    dev, host = device_wall(name, literal), host_wall(name, literal, CAP)
    assert np.array_equal(dev[1], host[1]), (name, np.flatnonzero(dev[1] != host[1])[:8])
    same = same_bits(pyprobe.wall_shared(dev[0]), pyprobe.wall_shared(host[0]))
    assert same.all(), (name, np.argwhere(~same)[:8].tolist())


@pytest.mark.parametrize("name", PROFILES)
def test_certified_stretches_and_skipped_blocks_are_sound_device(name):
    out, code = device_wall(name)
    report(name, "device", check_wall_soundness(name, out, "device"))
    check_wall_outcomes(name, out, "device")


@pytest.mark.parametrize("name", PROFILES)
def test_literal_wall_search_agrees_device(name):
    out, lit = device_wall(name)[0], device_wall(name, True)[0]
    capped = check_wall_literal(name, out, lit, "device")
    # rows cut off at the device's cap: the host compile's full literal run is the one compared with the certified search
    full = host_wall(name, True)[0]
    assert capped == int((full[wall_case(name)["rows"][:, 5] > 0, H["units"]] > CAP).sum()), (name, capped)


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("name", grid.OUTER_PROFILES)
def test_outer_device_equals_host_compile_bit_for_bit(name, literal):
    dev, host = device_outer(name, literal), host_outer(name, literal)
    assert np.array_equal(dev[1], host[1]) and same_bits(dev[0], host[0]).all(), (name, np.argwhere(~same_bits(dev[0], host[0]))[:8].tolist())


@pytest.mark.parametrize("name", grid.OUTER_PROFILES)
def test_outer_scan_finds_the_exact_first_node_device(name):
    check_outer(name, device_outer(name)[0], device_outer(name, True)[0], "device")


def test_hex_index_device():
    dev = pyprobe.run_hex(hex_case()["p"], hex_case()["rows"], device=True)
    assert same_bits(dev[0], host_hex()[0]).all()
    check_hex(dev[0], "device")


def test_refused_rows_device():
    """dz == 0 (2^28 units by design), a non-finite value or more than 200 000 units never reach a kernel"""
    S = wall_case("cylinder")
    x = S["rows"][:1].copy()
    for col, v in ((5, 0.0), (0, np.nan), (8, float(CAP + 1))):
        y = x.copy()
        y[0, col] = v
        with pytest.raises(RuntimeError):
            pyprobe.run_wall(S["p"], y, device=True)
