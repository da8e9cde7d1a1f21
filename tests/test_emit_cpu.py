"""Emit relays without a GPU (a thin sample between two optics; include/polycap-hip.h, pc_hip_emit_*): the per-entry arithmetic of
pc_emit.h compiled for the host (tests/emit/emit_host.cpp) against a numpy restatement of the contract bit for bit, with Philox taken
from the oracle; its geometry against mpmath; the solid-angle weight against the exact solid angle of a square; the three `missed`
conditions at their edges; the frame; the spec check; and the exported symbols."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_relay_pose_cpu import ULP1, _edge, _walk

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "emit")
NEW_SYMBOLS = ("pc_hip_emit_counts", "pc_hip_emit_frame", "pc_hip_emit_run", "pc_hip_emit_validate")
FIELDS = ("focus", "sample_angle", "depth", "det_angle", "wd", "off_u", "off_v", "target_half")
PI = float.fromhex("0x1.921fb54442d18p+1")
INJECT, MISS_SAMPLE, MISS_DETECTOR = 1, 3, 4


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def np_frame(focus, beta, depth, alpha, wd, off_u, off_v):
    """the sixteen numbers of the frame: every operation one IEEE fp64 operation, in the contract's order"""
    f = np.float64
    focus, depth, wd, off_u, off_v = f(focus), f(depth), f(wd), f(off_u), f(off_v)
    sb, cb, sa, ca = f(math.sin(beta)), f(math.cos(beta)), f(math.sin(alpha)), f(math.cos(alpha))
    ns = [sb, f(0.), cb]
    hs = (ns[0] * (depth * ns[0]) + ns[1] * (depth * ns[1])) + ns[2] * (focus + depth * ns[2])
    u, v, n = [ca, f(0.), f(0.) - sa], [f(0.), f(1.), f(0.)], [sa, f(0.), ca]
    c0 = [f(0.), f(0.), focus]
    cb_ = [((c0[k] + wd * n[k]) + off_u * u[k]) + off_v * v[k] for k in range(3)]
    return np.array(ns + [hs] + u + v + n + cb_, dtype=np.float64)


def np_emit(x, y, dx, dy, slots, u1, u2, fr, R):
    """(out [n, 12] = start (3), direction (3), electric vector (3), t, r, g; what [n]): every operation one IEEE fp64 numpy
    operation, in the contract's order; the rows of photons that are not injected are zero"""
    f = np.float64
    ns, hs, u, v, n, c = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16]
    R = f(R)
    with np.errstate(all="ignore"):
        dz = np.sqrt((f(1.) - dx * dx) - dy * dy)
        sd = (ns[0] * dx + ns[1] * dy) + ns[2] * dz
        sp = hs - (ns[0] * x + ns[1] * y)
        on_sample = (sd > 0.) & (sp >= 0.)
        t = sp / sd
        p0, p1, p2 = x + dx * t, y + dy * t, dz * t
        a, b = (f(2.) * u1 - f(1.)) * R, (f(2.) * u2 - f(1.)) * R
        q0, q1, q2 = c[0] - p0, c[1] - p1, c[2] - p2
        f0 = a + ((u[0] * q0 + u[1] * q1) + u[2] * q2)
        f1 = b + ((v[0] * q0 + v[1] * q1) + v[2] * q2)
        f2 = (n[0] * q0 + n[1] * q1) + n[2] * q2
        seen = f2 > 0.
        r2 = (f0 * f0 + f1 * f1) + f2 * f2
        r = np.sqrt(r2)
        d0, d1, d2 = f0 / r, f1 / r, f2 / r
        g = ((R * R) * d2) / (f(PI) * r2)
        h = np.sqrt(d2 * d2 + d0 * d0)
        zero = np.zeros_like(h)
        e1 = [d2 / h, zero, f(0.) - d0 / h]
        e2 = [f(0.) - (d0 * d1) / h, h, f(0.) - (d1 * d2) / h]
        even = (slots & np.uint64(1)) == 0
        e = [np.where(even, e1[k], e2[k]) for k in range(3)]
        out = np.stack([a, b, zero, d0, d1, d2, e[0], e[1], e[2], t, r, g], axis=1)
    what = np.where(~on_sample, MISS_SAMPLE, np.where(~seen, MISS_DETECTOR, INJECT)).astype(np.int32)
    out[what != INJECT] = 0.
    return out, what


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))


# ---- the host compile ---------------------------------------------------------------------------------------------------------
def build_emit_host(directory):
    so = os.path.join(str(directory), "emit_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "emit_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    L.emit_state_n.restype = None
    L.emit_state_n.argtypes = [C.c_int64, dp, u64p, dp, C.c_double, C.c_uint64, dp, C.POINTER(C.c_int32)]
    L.emit_frame.restype = None
    L.emit_frame.argtypes = [dp, dp]
    L.emit_spec_bad.restype = C.c_int
    L.emit_spec_bad.argtypes = [dp]
    L.emit_field_name.restype = C.c_char_p
    L.emit_field_name.argtypes = [C.c_int]
    L.emit_finish_n.restype = None
    L.emit_finish_n.argtypes = [C.c_int64, dp, dp, dp, dp]
    L.emit_dtravel_n.restype = None
    L.emit_dtravel_n.argtypes = [C.c_int64, dp, dp, dp, dp, dp]
    return L


def host_emit(L, four, slots, frame, R, seed):
    """four [n, 4] = x, y, dx, dy; slots [n] -> (out [n, 12], zero rows where nothing is injected; what [n])"""
    a = np.ascontiguousarray(four, dtype=np.float64)
    s = np.ascontiguousarray(slots, dtype=np.uint64)
    fr = np.ascontiguousarray(frame, dtype=np.float64)
    out = np.zeros((a.shape[0], 12))
    what = np.zeros(a.shape[0], dtype=np.int32)
    dp = C.POINTER(C.c_double)
    L.emit_state_n(a.shape[0], a.ctypes.data_as(dp), s.ctypes.data_as(C.POINTER(C.c_uint64)), fr.ctypes.data_as(dp), R, seed,
                   out.ctypes.data_as(dp), what.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, what


def host_frame(L, spec8):
    s = np.array(spec8, dtype=np.float64)
    fr = np.zeros(16)
    L.emit_frame(s.ctypes.data_as(C.POINTER(C.c_double)), fr.ctypes.data_as(C.POINTER(C.c_double)))
    return fr


@pytest.fixture(scope="module")
def emit_host(tmp_path_factory):
    return build_emit_host(tmp_path_factory.mktemp("emit_host"))


SEED = 20000
ALPHAS = (0., math.pi / 4., math.pi / 2., 3. * math.pi / 4., math.pi)
BETAS = (0., math.pi / 4., -math.pi / 4.)


def _entries(n, rng):
    """x, y, dx, dy of an exit beam at its focus, with the cases the contract has to survive: photons that run along the sheet or
    away from it, photons that start behind it, directions off the unit sphere; and slots on both sides of 2^32"""
    a = np.zeros((n, 4))
    a[:, 0:2] = rng.normal(0., 0.01, (n, 2))
    a[:, 2:4] = rng.normal(0., 0.03, (n, 2))
    k = n // 10
    a[:k, 2] = rng.uniform(-1., -0.6, k)                    # away from a sheet tilted towards +x
    a[k:2 * k, 0] = rng.uniform(-3., 3., k)                 # behind a tilted sheet
    a[2 * k:3 * k, 2:4] = rng.uniform(0.6, 0.9, (k, 2))      # dx^2 + dy^2 around 1 and beyond: dz = NaN
    slots = rng.integers(0, 40000, n).astype(np.uint64)
    slots[1::4] = (np.uint64(1) << np.uint64(32)) - np.uint64(8) + rng.integers(0, 16, len(slots[1::4])).astype(np.uint64)
    slots[2::4] = rng.integers(1 << 33, 1 << 62, len(slots[2::4])).astype(np.uint64)
    return a, slots


def _uniforms(oracle, seed, slots):
    u1 = np.array([oracle.uniform(seed, int(s), 0, 0) for s in slots])
    u2 = np.array([oracle.uniform(seed, int(s), 0, 1) for s in slots])
    return u1, u2


# ---- 1. the contract, bit for bit -----------------------------------------------------------------------------------------------
def test_state_is_the_contract_bit_for_bit(emit_host, oracle):
    rng = np.random.default_rng(20250)
    a, slots = _entries(4000, rng)
    assert ((slots & np.uint64(1)) == 0).sum() > 1000 and ((slots & np.uint64(1)) == 1).sum() > 1000
    assert (slots < 1 << 32).sum() > 1000 and (slots >= 1 << 32).sum() > 1000
    u1, u2 = _uniforms(oracle, SEED, slots)
    assert 0. <= u1.min() and u1.max() < 1. and not np.array_equal(u1, u2)
    seen = np.zeros(5, dtype=np.int64)
    #          focus, depth, wd,     off_u, off_v,  R
    places = [(0.5, 0., 0.5, 0., 0., 0.0585), (0.5, 0.001, 0.5, 0.002, -0.001, 0.0585), (0.5, 0.02, 0.005, 0., 0., 0.01),
              (0., -0.003, 1.25, 0., 0.3, 0.2065)]
    for alpha in ALPHAS:
        for beta in BETAS:
            for focus, depth, wd, ou, ov, R in places:
                fr = host_frame(emit_host, (focus, beta, depth, alpha, wd, ou, ov, R))
                assert same_bits(fr, np_frame(focus, beta, depth, alpha, wd, ou, ov)), (alpha, beta)
                got, what = host_emit(emit_host, a, slots, fr, R, SEED)
                want, what_w = np_emit(a[:, 0], a[:, 1], a[:, 2], a[:, 3], slots, u1, u2, fr, R)
                assert np.array_equal(what, what_w), (alpha, beta, focus, depth)
                assert same_bits(got, want), (alpha, beta, focus, depth)
                ok = what == INJECT
                assert not got[:, 2].any() and np.all(got[ok, 5] > 0.) and np.all(got[ok, 11] > 0.) and np.all(np.abs(got[ok, 0:2]) <= R)
                seen += np.bincount(what, minlength=5)
    print("injected, missed the sample, missed the detector:", seen[INJECT], seen[MISS_SAMPLE], seen[MISS_DETECTOR])
    assert seen[INJECT] > 10000 and seen[MISS_SAMPLE] > 10000 and seen[MISS_DETECTOR] > 1000
    # another seed draws other points
    other, _ = host_emit(emit_host, a, slots, fr, R, SEED + 1)
    assert not same_bits(other, got)
    # the products of the finish
    n = 50000
    wa, g, wb, w = rng.random(n), rng.random(n) * 0.01, rng.random(n), np.zeros(n)
    dp = C.POINTER(C.c_double)
    emit_host.emit_finish_n(n, wa.ctypes.data_as(dp), g.ctypes.data_as(dp), wb.ctypes.data_as(dp), w.ctypes.data_as(dp))
    assert same_bits(w, (wa * g) * wb)
    da, t, r, db = rng.uniform(0., 20., n), rng.uniform(0., 3., n), rng.uniform(0., 3., n), rng.uniform(0., 20., n)
    emit_host.emit_dtravel_n(n, da.ctypes.data_as(dp), t.ctypes.data_as(dp), r.ctypes.data_as(dp), db.ctypes.data_as(dp), w.ctypes.data_as(dp))
    assert same_bits(w, ((da + t) + r) + db)


# ---- 2. geometry ----------------------------------------------------------------------------------------------------------------
def test_geometry_against_mpmath(emit_host):
    """The injected direction and electric vector as stored, evaluated by mpmath at 50 digits: |d| = 1, e . d = 0, |e| = 1, each
    within the 64 ulp of 1 that tests/test_relay_pose_cpu.py::test_fly_posed_geometry_against_mpmath allows its unit vectors.  With
    a target of half-side 1e-300 the drawn point vanishes beside B's centre, so that slots 2k and 2k + 1 get the same direction and
    one of e1, e2 each: e1 . e2 = 0 to the same accuracy."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(8)
    n = 300
    a = np.zeros((2 * n, 4))
    a[0::2, 0:2] = rng.normal(0., 0.01, (n, 2))
    a[0::2, 2:4] = rng.normal(0., 0.03, (n, 2))
    a[1::2] = a[0::2]
    slots = np.repeat(2 * rng.integers(0, 1 << 40, n).astype(np.uint64), 2)
    slots[1::2] += np.uint64(1)
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
    worst = [0., 0., 0., 0.]
    for alpha in ALPHAS:
        for beta in BETAS:
            for R in (0.0585, 1e-300):
                fr = host_frame(emit_host, (0.5, beta, 0.001, alpha, 0.5, 0.002, -0.001, R))
                got, what = host_emit(emit_host, a, slots, fr, R, SEED)
                assert np.all(what == INJECT)
                for i in range(2 * n):
                    d = [mp.mpf(float(v)) for v in got[i, 3:6]]
                    e = [mp.mpf(float(v)) for v in got[i, 6:9]]
                    worst[0] = max(worst[0], float(abs(mp.sqrt(dot(d, d)) - 1)))
                    worst[1] = max(worst[1], float(abs(dot(d, e))))
                    worst[2] = max(worst[2], float(abs(mp.sqrt(dot(e, e)) - 1)))
                if R == 1e-300:
                    assert same_bits(got[0::2, 3:6], got[1::2, 3:6])
                    assert np.all(got[0::2, 7] == 0.) and np.all(got[1::2, 7] > 0.)         # e1 on the even slots, e2 on the odd ones
                    for i in range(n):
                        e1 = [mp.mpf(float(v)) for v in got[2 * i, 6:9]]
                        e2 = [mp.mpf(float(v)) for v in got[2 * i + 1, 6:9]]
                        worst[3] = max(worst[3], float(abs(dot(e1, e2))))
    print("|d| - 1, e.d, |e| - 1, e1.e2: %s ulp of 1" % ", ".join("%.3g" % (w / ULP1) for w in worst))
    assert max(worst) <= 64. * ULP1, worst


# ---- 3. the solid angle ---------------------------------------------------------------------------------------------------------
def test_mean_weight_is_the_solid_angle_of_the_square(emit_host):
    """A point emitter on B's axis at distance wd (a photon along A's axis, an untilted sheet through the focus, B in line): the mean
    of g over 2e5 slots against Omega / 4 pi, Omega = 4 atan(R^2 / (wd sqrt(wd^2 + 2 R^2))), the solid angle of a square of
    half-side R seen from a point on its axis.  Bound: 4 standard errors of the mean, from the sample itself."""
    n = 200000
    slots = np.arange(n, dtype=np.uint64)
    a = np.zeros((n, 4))
    for wd, R in ((0.5, 0.0585), (0.5, 0.3), (0.1, 0.3)):
        fr = host_frame(emit_host, (0.5, 0., 0., 0., wd, 0., 0., R))
        got, what = host_emit(emit_host, a, slots, fr, R, SEED)
        assert np.all(what == INJECT) and np.all(got[:, 9] == 0.5)
        g = got[:, 11]
        want = 4. * math.atan(R * R / (wd * math.sqrt(wd * wd + 2. * R * R))) / (4. * math.pi)
        err = g.std(ddof=1) / math.sqrt(n)
        print("wd %g R %g: mean g %.8g, Omega/4pi %.8g, difference %.2f standard errors; R^2/(pi wd^2) = %.8g"
              % (wd, R, g.mean(), want, (g.mean() - want) / err, R * R / (math.pi * wd * wd)))
        assert abs(g.mean() - want) <= 4. * err, (wd, R, g.mean(), want, err)
        # the drawn points fill the square evenly
        assert abs(got[:, 0].mean()) <= 4. * R / math.sqrt(3. * n) and abs(got[:, 1].mean()) <= 4. * R / math.sqrt(3. * n)


# ---- 4. the edges ---------------------------------------------------------------------------------------------------------------
def test_missed_on_each_side_of_its_edges(emit_host):
    one = lambda four, fr, R=0.0585, slot=6: tuple(v[0] for v in host_emit(emit_host, [four], [slot], fr, R, SEED))
    # sd = 0 exactly: a photon along x onto an untilted sheet (dz = 0); one ulp inside the unit circle it hits
    fr = host_frame(emit_host, (0.5, 0., 0., 0., 0.5, 0., 0., 0.0585))
    assert one([0., 0., 1., 0.], fr)[1] == MISS_SAMPLE
    assert one([0., 0., np.nextafter(1., 0.), 0.], fr)[1] != MISS_SAMPLE
    # sd through 0 on a sheet tilted by pi/4: dx walked through the direction that lies in the sheet
    fr = host_frame(emit_host, (0.5, math.pi / 4., 0., math.pi / 2., 0.5, 0., 0., 0.0585))

    def sd(dx):
        dx = np.float64(dx)
        return (fr[0] * dx + fr[1] * np.float64(0.)) + fr[2] * np.sqrt((np.float64(1.) - dx * dx) - np.float64(0.))

    last = _edge(lambda v: sd(v) <= 0., -0.9, 0.)
    dxs = np.array([_walk(last, k) for k in range(-40, 41)])
    four = np.zeros((len(dxs), 4))
    four[:, 2] = dxs
    _, what = host_emit(emit_host, four, np.full(len(dxs), 6, dtype=np.uint64), fr, 0.0585, SEED)
    want = np.array([sd(v) > 0. for v in dxs])
    assert np.array_equal(what != MISS_SAMPLE, want) and what[40] == MISS_SAMPLE and what[41] != MISS_SAMPLE and sd(dxs[40]) <= 0. < sd(dxs[41])

    # sp = 0 exactly: the sheet passes through the photon's start (depth = -focus); it is emitted where it is, t = 0
    fr = host_frame(emit_host, (0.5, 0., -0.5, 0., 0.5, 0., 0., 0.0585))
    assert fr[3] == 0.
    o, w = one([0.001, 0., 0.01, 0.], fr)
    assert w == INJECT and o[9] == 0.
    fr = host_frame(emit_host, (0.5, 0., np.nextafter(-0.5, -1.), 0., 0.5, 0., 0., 0.0585))
    assert fr[3] < 0. and one([0.001, 0., 0.01, 0.], fr)[1] == MISS_SAMPLE
    # sp through 0 on the tilted sheet: x walked through the sheet
    fr = host_frame(emit_host, (0.01, math.pi / 4., 0., math.pi / 2., 0.5, 0., 0., 0.0585))

    def sp(x):
        return fr[3] - (fr[0] * np.float64(x) + fr[1] * np.float64(0.))

    last = _edge(lambda v: sp(v) >= 0., 0., 0.5)
    xs = np.array([_walk(last, k) for k in range(-40, 41)])
    four = np.zeros((len(xs), 4))
    four[:, 0] = xs
    got, what = host_emit(emit_host, four, np.full(len(xs), 6, dtype=np.uint64), fr, 0.0585, SEED)
    want = np.array([sp(v) >= 0. for v in xs])
    assert np.array_equal(what != MISS_SAMPLE, want) and what[40] != MISS_SAMPLE and what[41] == MISS_SAMPLE and sp(xs[41]) < 0. <= sp(xs[40])
    assert np.all(got[what == INJECT, 9] >= 0.)

    # f2 = 0 exactly: B in line, the sheet in B's entrance plane (depth = wd); one ulp of focus + depth in front of it the photon is
    # emitted
    fr = host_frame(emit_host, (0.5, 0., 0.25, 0., 0.25, 0., 0., 0.0585))
    assert one([0., 0., 0., 0.], fr)[1] == MISS_DETECTOR
    fr = host_frame(emit_host, (0.5, 0., 0.25 - 2. ** -53, 0., 0.25, 0., 0., 0.0585))
    o, w = one([0., 0., 0., 0.], fr)
    assert fr[3] == np.nextafter(0.75, 0.) and w == INJECT and o[5] > 0. and o[10] > 0.
    fr = host_frame(emit_host, (0.5, 0., 0.25 + 2. ** -53, 0., 0.25, 0., 0., 0.0585))
    assert fr[3] == np.nextafter(0.75, 1.) and one([0., 0., 0., 0.], fr)[1] == MISS_DETECTOR


# ---- 5. the frame ---------------------------------------------------------------------------------------------------------------
def test_frame_identity_and_library(emit_host):
    import polycap_amd
    f = polycap_amd.emit_frame(0.5, 0., 0.001, 0., 0.25, (0.002, 0.003))
    want = np.array([0., 0., 1., 0.5 + 0.001, 1., 0., 0., 0., 1., 0., 0., 0., 1., 0.002, 0.003, 0.5 + 0.25])
    assert same_bits(f["frame"], want), f["frame"]                 # the identity bit for bit: no minus sign on a zero
    assert not np.signbit(polycap_amd.emit_frame(0.5, 0., 0., 0., 0.25)["frame"]).any()
    assert same_bits(np.concatenate([f["n_s"], [f["h_s"]], f["u"], f["v"], f["n"], f["c_b"]]), f["frame"])
    # det_angle pi/2: B looks along -x ... its axis n points along +x, its x axis along -z
    g = polycap_amd.emit_frame(0.5, math.pi / 4., 0., math.pi / 2., 0.5)
    assert g["n"][0] == 1. and abs(g["n"][2]) < 1e-16 and g["u"][2] == -1. and abs(g["c_b"][0] - 0.5) < 1e-16 and abs(g["c_b"][2] - 0.5) < 1e-16
    assert g["n_s"][0] > 0. and polycap_amd.emit_frame(0.5, -math.pi / 4., 0., math.pi / 2., 0.5)["n_s"][0] < 0.
    # the library returns what the header computes and what the contract says
    for alpha in ALPHAS + (-math.pi / 2., -math.pi):
        for beta in BETAS + (1.5, -1e-9):
            spec = (0.5, beta, -0.002, alpha, 0.4, 0.01, -0.02, 0.0585)
            lib = polycap_amd.emit_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7])["frame"]
            assert same_bits(lib, host_frame(emit_host, spec)) and same_bits(lib, np_frame(*spec[:7])), (alpha, beta)


# ---- 6. the spec check ----------------------------------------------------------------------------------------------------------
HALF_PI = 1.5707963267948966
GOOD = (0.5, math.pi / 4., 0.001, math.pi / 2., 0.5, 0.002, 0., 0.0585)
BAD_VALUES = {"focus": (-1e-300, -1., math.nan, math.inf), "sample_angle": (HALF_PI, -HALF_PI, 2., math.nan, -math.inf),
              "depth": (math.nan, math.inf, -math.inf), "det_angle": (np.nextafter(PI, 4.), -np.nextafter(PI, 4.), 4., math.nan, math.inf),
              "wd": (0., -0., -0.5, math.nan, math.inf), "off_u": (math.nan, math.inf), "off_v": (math.nan, -math.inf),
              "target_half": (0., -0.0585, math.nan, math.inf)}
GOOD_SPECS = [GOOD, (0., 0., 0., 0., 5e-324, 0., 0., 5e-324), (0.5, np.nextafter(HALF_PI, 0.), -3., PI, 1e6, -5., 5., 10.),
              (0.5, -np.nextafter(HALF_PI, 0.), 3., -PI, 0.5, 0., 0., 0.0585)]


def test_validate_names_the_field(emit_host):
    import polycap_amd
    L = polycap_amd.lib()
    dp = C.POINTER(C.c_double)
    assert L.pc_hip_emit_validate(None) == -2 and b"spec" in L.pc_hip_last_error()
    assert [emit_host.emit_field_name(k).decode() for k in range(8)] == list(FIELDS)
    for k, name in enumerate(FIELDS):
        for bad in BAD_VALUES[name]:
            spec = list(GOOD)
            spec[k] = bad
            assert not polycap_amd.emit_valid(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7]), (name, bad)
            msg = L.pc_hip_last_error().decode()
            assert msg.startswith("pc_hip_emit_validate: " + name + " "), (name, bad, msg)
            assert emit_host.emit_spec_bad(np.array(spec).ctypes.data_as(dp)) == 1 + k
            with pytest.raises(polycap_amd.HipError) as e:
                polycap_amd.emit_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7])
            assert e.value.status == -2 and name in str(e.value)
    for spec in GOOD_SPECS:
        assert polycap_amd.emit_valid(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7]), spec
        assert emit_host.emit_spec_bad(np.array(spec, dtype=np.float64).ctypes.data_as(dp)) == 0
    # the map: absent, or a list of indices
    assert polycap_amd.emit_valid(*GOOD[:5], GOOD[5:7], GOOD[7], energy_map=[0, 0, 2])
    assert not polycap_amd.emit_valid(*GOOD[:5], GOOD[5:7], GOOD[7], energy_map=[0, -1]) and b"map[1]" in L.pc_hip_last_error()
    assert not polycap_amd.emit_valid(*GOOD[:5], GOOD[5:7], GOOD[7], energy_map=[]) and b"n_map" in L.pc_hip_last_error()
    from polycap_amd import _cabi
    s = _cabi.EmitS(*GOOD, 0, 3, None)
    assert L.pc_hip_emit_validate(C.byref(s)) == -2 and b"n_map" in L.pc_hip_last_error()
    assert C.sizeof(_cabi.EmitS) == 88


# ---- 7. symbols -----------------------------------------------------------------------------------------------------------------
def test_emit_symbols_are_exported_and_declared():
    import polycap_amd
    polycap_amd.lib()
    so = os.path.join(ROOT, "polycap_amd", "lib", "libpolycap.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert [n for n in names if "emit" in n] == sorted(NEW_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "polycap-hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"POLYCAP_EXTERN\s+[^;(]*?\b(\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    # nothing else came with them: no kernel stub, no C++ instantiation, no undeclared pc_hip_ name
    assert not [n for n in names if n.startswith("_Z") or "pc_emit" in n]
    assert [n for n in names if n.startswith("pc_hip_") and n not in declared] == []
