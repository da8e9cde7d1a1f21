"""The two ends of a photon's life on the MI355X: probe ops SINCOS, UNIFORM, ENTER and EXIT (tests/devmath/probe.hip) and the
sampler kernel (ctx.sample_photons) equal the host compile bit for bit (the three elliptical sources, which call libm, excepted),
and the checks of tests/test_devmath_ends_cpu.py -- the integer Philox stream, 2 ulp for the quadrant sine and cosine, the sampler
against the exact restatement with the oracle as yardstick, the entrance decisions and state, the exit window -- hold on the
device's own outputs.  Probe launches and sampler calls only, except the last test.

Zero-reflection records: SEVEN_CASE and MONO_CASE, 3000 slots with images kept, through the default kernel, the pool and the
producer kernel and (SEVEN_CASE) one leak run.  A photon that left without a reflection flew straight: with dz = sqrt(1 - dx^2 -
dy^2) and t = z_end / dz from the record's own start fields its exit point is start + d t, its path t.  The record's exit x, y, z
and d_travel agree with that within 4 x the oracle's own worst error on its zero-reflection records of the same run (measured the
same way, in units of 2^-52 x scale: max(|start|, |d t|) per coordinate, z_end, t); the exit direction equals the start direction bit
for bit and the rounded electric vector is that of the start.  At least 1000 such records on SEVEN_CASE, 10 on MONO_CASE.
"""
import functools

import mpmath as mp
import numpy as np
import pytest

from tests.common import MONO_CASE, SEVEN_CASE, make_custom
from tests.devmath import exact, grid
from tests.test_devmath_ends_cpu import (bits_equal, check_axis_factors, check_enter, check_exit, check_sampler, check_sincos,
                                         check_uniforms, host_enter, run_enter, run_exit, run_sampler, run_sincos, run_uniform)

pytestmark = pytest.mark.gpu
U52 = 2.0 ** -52
RECORD_SEED, RECORD_SLOTS = 20260, 3000


@functools.lru_cache(maxsize=None)
def device_enter(name):
    return run_enter(name, device=True)


@functools.lru_cache(maxsize=None)
def device_sampler(name):
    return run_sampler(name, device=True)


def test_sincos_and_uniform_equal_the_host_compile_bit_for_bit_and_the_exact_side():
    sc = run_sincos(device=True)
    assert bits_equal(sc, run_sincos()).all()
    check_sincos(sc, "device")
    u = run_uniform(device=True)
    assert bits_equal(u, run_uniform()).all()
    check_uniforms(u, "device")


@pytest.mark.parametrize("name", tuple(grid.SAMPLER_CASES))
def test_sampler_on_the_device(name, oracle):
    got = device_sampler(name)
    if name not in grid.SAMPLER_GENERIC:
        same = bits_equal(got, run_sampler(name))
        assert same.all(), (name, np.argwhere(~same)[:8].tolist())
    check_sampler(name, got, "device")


@pytest.mark.parametrize("name", grid.ENTER_PROFILES)
def test_entrance_on_the_device(name):
    out, code = device_enter(name)
    host, host_code = host_enter(name)
    same = bits_equal(out, host)
    assert same.all() and np.array_equal(code, host_code), (name, np.argwhere(~same)[:8].tolist())
    check_enter(name, out, code, "device")


@pytest.mark.parametrize("name", grid.ENTER_PROFILES)
def test_entrance_axis_factors_within_one_ulp_on_the_device(name):
    out, code = device_enter(name)
    check_axis_factors(name, out, code, "device")


@pytest.mark.parametrize("name", grid.ENTER_PROFILES)
def test_exit_window_on_the_device(name):
    got = run_exit(name, device=True)
    assert bits_equal(got, run_exit(name)).all(), name
    check_exit(name, got, "device")


# --------------------------------------------------------------------------------------------------------------------------- records

def straight_flight_errors(img, z_end):
    """per zero-reflection record [n, 17]: |exit - exact| of x, y, z and of d_travel in units of 2^-52 x scale, against the exact
    extrapolation of the record's own start fields; a coordinate whose scale is 0 must be exact"""
    worst = dict(coord=0.0, travel=0.0)
    with mp.workdps(exact.EDPS):
        ze = mp.mpf(float(z_end))
        for r in img:
            sx, sy, dx, dy = (mp.mpf(float(v)) for v in r[2:6])
            dz = mp.sqrt(1 - dx * dx - dy * dy)
            t = ze / dz
            for got, start, step in ((r[8], sx, dx * t), (r[9], sy, dy * t), (r[10], mp.mpf(0), ze)):
                scale = max(abs(start), abs(step))
                err = abs(mp.mpf(float(got)) - (start + step))
                if scale == 0:
                    assert err == 0, r
                else:
                    worst["coord"] = max(worst["coord"], float(err / scale) / U52)
            worst["travel"] = max(worst["travel"], float(abs(mp.mpf(float(r[16])) - t) / t) / U52)
    return worst


@functools.lru_cache(maxsize=None)
def record_case(which):
    from oracle import pyoracle
    pyoracle.build()
    optic, src, prob, (E, amu, scatf) = make_custom(pyoracle, **(SEVEN_CASE if which == "seven" else MONO_CASE))
    ref = pyoracle.transmission(optic, src, E, amu, scatf, RECORD_SEED, 0, RECORD_SLOTS, images=True)
    img = ref["images"]
    zero = (ref["exit_weights"][:, 0] > 0) & (img[:, 15] == 0)
    return dict(problem=prob, z_end=float(prob.z[-1]), oracle=straight_flight_errors(img[zero], float(prob.z[-1])), n_oracle=int(zero.sum()))


RECORD_RUNS = [("seven", "default"), ("seven", "pool"), ("seven", "producer"), ("seven", "leak"),
               ("mono", "default"), ("mono", "pool"), ("mono", "producer")]


@pytest.mark.parametrize("which,kernel", RECORD_RUNS)
def test_zero_reflection_records_are_the_straight_flight(which, kernel, oracle):
    import polycap_amd as pa
    S = record_case(which)
    with pa.TraceContext(S["problem"]) as ctx:
        if kernel == "pool":
            ctx.set_option("pool", 1)
        elif kernel == "producer":
            ctx.set_option("pool", 0)
            ctx.set_option("producer", 1)
        r = ctx.transmission(RECORD_SEED, 0, RECORD_SLOTS, keep_images=True, leak_calc=(kernel == "leak"))
        name = ctx.last_kernel()
    want = dict(pool="pc_trace_pool_kernel", producer="pc_trace_producer_kernel", leak="pc_leak_kernel").get(kernel)
    assert want is None or name == want, (which, kernel, name)
    img = r["images"]
    zero = (r["exit_weights"][:, 0] > 0) & (r["nrefl"] == 0)
    n = int(zero.sum())
    got = straight_flight_errors(img[zero], S["z_end"])
    print("records %-5s %-8s (%s) %d zero-reflection records (oracle %d): worst coordinate %.2f (oracle %.2f), d_travel %.2f (oracle %.2f), units of 2^-52 x scale"
          % (which, kernel, name, n, S["n_oracle"], got["coord"], S["oracle"]["coord"], got["travel"], S["oracle"]["travel"]))
    assert n >= (1000 if which == "seven" else 10) and S["n_oracle"] >= (1000 if which == "seven" else 10), (which, kernel, n, S["n_oracle"])
    assert got["coord"] <= 4 * S["oracle"]["coord"] and got["travel"] <= 4 * S["oracle"]["travel"], (which, kernel, got, S["oracle"])
    z = img[zero]
    assert bits_equal(z[:, 11:13], z[:, 4:6]).all(), (which, kernel, "exit direction differs from the start direction")
    assert np.array_equal(z[:, 13:15], z[:, 6:8]), (which, kernel, "exit electric vector differs from the start's")
