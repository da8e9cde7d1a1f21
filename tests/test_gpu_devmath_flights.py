"""The march certificates on flights after a reflection, on the MI355X (tests/devmath/probe.hip, op FLIGHTS: pc_launch_init,
pc_march_step, pc_event_pre and pc_event_post called as the kernels call them, flight after flight, on the tables pc_build_tables
makes): every output, the trail included, equals the host compile's bit for bit, and the checks of
tests/test_devmath_flights_cpu.py -- soundness of every flight against rational arithmetic, the literal chain being the same chain,
the state pc_event_post and pc_trace_begin leave at a flight's start, the first-segment certificate passing where it must, the
reflection limit, and that the grids are not vacuous -- hold
on the device's own outputs.  Probe launches only, no trace kernel; the exact maxima are computed once per process and shared (they
depend on the P and d the probe reports per flight, which the bit-for-bit test pins)."""
import functools

import numpy as np
import pytest

from tests.test_devmath_flights_cpu import (FLOORS, PROFILES, check_endings, check_first_passes_where_it_must, check_limit,
                                            check_literal_agreement, check_soundness, check_state, host_run, report, run_rows,
                                            total_counts)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_run(name, literal=False):
    return run_rows(name, device=True, literal=literal)


@functools.lru_cache(maxsize=None)
def device_measure(name):
    return check_soundness(name, device_run(name)[0], "device")


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("name", PROFILES)
def test_device_equals_host_compile_bit_for_bit(name, literal):
    dev, host = device_run(name, literal), host_run(name, literal)
    assert np.array_equal(dev[1], host[1]), (name, np.flatnonzero(dev[1] != host[1])[:8])
    d, h = dev[0].view(np.uint64), host[0].view(np.uint64)
    same = (d == h) | (np.isnan(dev[0]) & np.isnan(host[0]))
    assert same.all(), (name, np.argwhere(~same)[:8].tolist())


@pytest.mark.parametrize("name", PROFILES)
def test_certified_steps_of_every_flight_skip_only_segments_strictly_inside_device(name):
    report(name, "device", device_measure(name))


@pytest.mark.parametrize("name", PROFILES)
def test_literal_chain_is_the_same_chain_bit_for_bit_device(name):
    out, code = device_run(name)
    lit, code_lit = device_run(name, literal=True)
    check_literal_agreement(name, out, code, lit, code_lit, "device")
    check_endings(name, lit, "device literal")


@pytest.mark.parametrize("name", PROFILES)
def test_state_limit_and_endings_on_the_device(name):
    out, code = device_run(name)
    check_state(name, out, "device")
    check_state(name, device_run(name, literal=True)[0], "device literal")
    n = check_limit(name, out, code, "device")
    check_endings(name, out, "device")
    check_first_passes_where_it_must(name, out, "device")
    if name in ("nmax1", "nmax4"):
        assert n >= 16


def test_grids_hold_what_the_exact_side_must_count_device():
    tot = total_counts(device_measure)
    assert all(tot[k] >= FLOORS[k] for k in FLOORS), tot
