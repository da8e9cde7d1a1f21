"""The geometric half of a reflection on the MI355X (tests/devmath/probe.hip: pc_segment, pc_reflect_geom, pc_refl_geom3, the
update of pc_reflect and pc_event_post, each called the way the kernels call it), element by element against the reference's
definitions in exact arithmetic and against the oracle's own error -- the checks of tests/test_devmath_geom_cpu.py on the device's
results -- and bit for bit against the host compile: every operation involved is an IEEE one on both sides (no fast-math branch:
pc_sqrt_fast, pc_div_fast and pc_exp_neg_fast belong to the Fresnel half).  One probe launch per test, no trace kernel.  Every
measured maximum is printed (run with -s)."""
import numpy as np
import pytest

from tests.devmath import pyprobe
from tests.test_devmath_geom_cpu import (check_bounce, check_bounce_chain, check_geom, check_segment_accuracy,
                                         check_segment_status, geom_case, segment_case)

pytestmark = pytest.mark.gpu


def _both(case, op):
    dev = pyprobe.run_geom(case["p"], op, case["rows"], device=True)
    host = pyprobe.run_geom(case["p"], op, case["rows"], device=False)
    return dev, host


def _same_bits(dev, host, what):
    assert np.array_equal(dev[1], host[1]), (what, np.flatnonzero(dev[1] != host[1])[:8])
    d, h = dev[0].view(np.uint64), host[0].view(np.uint64)
    # a NaN is a NaN whatever its payload
    same = (d == h) | (np.isnan(dev[0]) & np.isnan(host[0]))
    assert same.all(), (what, np.argwhere(~same)[:8].tolist())


def test_segment_status_device():
    S = segment_case()
    out, code = pyprobe.run_geom(S["p"], "segment", S["rows"], device=True)
    check_segment_status(out, code, "device")


def test_segment_hit_and_normal_device():
    """pc_segment on the device: hit and normal within M_ORACLE of the oracle's own error against the exact values per conditioning
    bucket (the device is held against the reference's arithmetic, not against itself); | |n| - 1 | <= NORMAL_LEN on both sides of
    the series switch."""
    S = segment_case()
    out, code = pyprobe.run_geom(S["p"], "segment", S["rows"], device=True)
    check_segment_accuracy(out, code, "device")


def test_reflection_geometry_device():
    G = geom_case()
    out, code = pyprobe.run_geom(G["p"], "geom", G["rows"], device=True)
    check_geom(out, code, "device")


def test_bounce_device():
    G = geom_case()
    out, code = pyprobe.run_geom(G["p"], "bounce", G["rows"], device=True)
    check_bounce(out, code, "device")


def test_bounce_chain_device():
    """64 bounces, each a probe launch on the previous launch's output: the length of the direction as measured"""
    check_bounce_chain(True, "device")


@pytest.mark.parametrize("op", ["segment", "geom", "bounce"])
def test_device_equals_host_compile_bit_for_bit(op):
    case = segment_case() if op == "segment" else geom_case()
    dev, host = _both(case, op)
    _same_bits(dev, host, op)
