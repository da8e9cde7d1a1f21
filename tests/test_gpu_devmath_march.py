"""The march certificates on the MI355X (tests/devmath/probe.hip, op MARCH: pc_launch_init, pc_march_step and pc_event_pre called as
the kernels call them, on the tables pc_build_tables makes): every output, the trail included, equals the host compile's bit for
bit, and the checks of tests/test_devmath_march_cpu.py -- soundness against rational arithmetic, agreement with the literal march,
the boundary classification, and that the grids are not vacuous -- hold on the device's own outputs.  Probe launches only, no trace
kernel; the exact maxima are computed once per process and shared (they depend on the rows and on the direction the probe reports,
which the bit-for-bit test pins)."""
import functools

import numpy as np
import pytest

from tests.devmath import pyprobe
from tests.test_devmath_march_cpu import (PROFILES, check_built, check_classification, check_crossings_visited,
                                          check_literal_agreement, check_soundness, check_widest, host_run, march_case, report,
                                          run_rows)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_run(name, literal=False):
    return run_rows(name, device=True, literal=literal)


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("name", PROFILES)
def test_device_equals_host_compile_bit_for_bit(name, literal):
    dev, host = device_run(name, literal), host_run(name, literal)
    assert np.array_equal(dev[1], host[1]), (name, np.flatnonzero(dev[1] != host[1])[:8])
    d, h = dev[0].view(np.uint64), host[0].view(np.uint64)
    same = (d == h) | (np.isnan(dev[0]) & np.isnan(host[0]))
    assert same.all(), (name, np.argwhere(~same)[:8].tolist())


@pytest.mark.parametrize("name", PROFILES)
def test_certified_steps_skip_only_segments_strictly_inside_device(name):
    out, code = device_run(name)
    report(name, "device", check_soundness(name, out, "device"))


@pytest.mark.parametrize("name", PROFILES)
def test_literal_march_agrees_at_the_adversarial_points_device(name):
    out, code = device_run(name)
    lit, code_lit = device_run(name, literal=True)
    check_literal_agreement(name, out, code, lit, code_lit, "device")


@pytest.mark.parametrize("name", PROFILES)
def test_grids_are_not_vacuous_on_the_device(name):
    out, code = device_run(name)
    assert check_classification(name, out, "device") == (0 if march_case(name)["t"]["mono"] else 3)
    check_built(name, out)
    check_crossings_visited(name, out, "device")
    if name in ("cylinder", "bulge"):
        check_widest(name, out, "device")


def test_grids_hold_enough_crossing_and_near_miss_rows_device():
    cross = near = 0
    for name in PROFILES:
        c, n = check_built(name, device_run(name)[0])
        cross, near = cross + c, near + n
    assert cross >= 200 and near >= 200
