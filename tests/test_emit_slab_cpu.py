"""Slab emits without a GPU (an emit relay through a thick sample; include/polycap-hip.h, pc_hip_slab_*): the slab part of pc_emit.h
compiled for the host (tests/emit_slab/emit_slab_host.cpp) against a numpy restatement of the contract bit for bit, with Philox taken
from the oracle; its exponential against mpmath; zero attenuation; the closed form of the attenuated depth integral in the in-line and
in the reflection geometry; the edges; the spec check; and the exported symbols."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_emit_cpu import (BETAS, FIELDS, GOOD, INJECT, MISS_DETECTOR, MISS_SAMPLE, PI, SEED, _entries, build_emit_host,
                                 host_emit, np_frame, same_bits)

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "emit_slab")
NEW_SYMBOLS = ("pc_hip_slab_frame", "pc_hip_slab_run", "pc_hip_slab_validate")
N_STATE = 14
T_, R_, GL, S, SOUT = 9, 10, 11, 12, 13            # the state behind the emit's nine numbers

LOG2E, LN2_HI, LN2_LO = 1.4426950408889634074, 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_C = (2.50521083854417187751e-08, 2.75573192239858906526e-07, 2.75573192239858906526e-06, 2.48015873015873015873e-05,
         1.98412698412698412698e-04, 1.38888888888888888889e-03, 8.33333333333333333333e-03, 4.16666666666666666667e-02,
         1.66666666666666666667e-01, 0.5, 1.0, 1.0)


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def np_exp_neg(x):
    """E(x) of the contract: every operation one IEEE fp64 numpy operation"""
    f = np.float64
    x = np.asarray(x, dtype=np.float64)
    low, nan = x < -700., np.isnan(x)
    xs = np.where(low | nan, f(0.), x)
    k = np.rint(xs * f(LOG2E))
    r = xs - k * f(LN2_HI)
    r = r - k * f(LN2_LO)
    p = np.full_like(xs, EXP_C[0])
    for c in EXP_C[1:]:
        p = p * r + f(c)
    y = np.ldexp(p, k.astype(np.int32))
    return np.where(nan, x, np.where(low, f(0.), y))


def np_slab_frame(focus, beta, depth, alpha, wd, off_u, off_v, T):
    fr = np_frame(focus, beta, depth, alpha, wd, off_u, off_v)
    ns, u, v, n = fr[0:3], fr[4:7], fr[7:10], fr[10:13]
    k = [(ns[0] * a[0] + ns[1] * a[1]) + ns[2] * a[2] for a in (u, v, n)]
    return np.concatenate([fr, np.array(k + [np.float64(T)])])


def np_slab(x, y, dx, dy, odd, u1, u2, u3, fr, R):
    """(out [n, 14] = the emit's nine, t, r, gl, s, s_out; what [n]; the intermediate values by name): every operation one IEEE fp64
    numpy operation, in the contract's order; the rows of photons that are not injected are zero"""
    f = np.float64
    ns, hs, u, v, n, c, k, T = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16], fr[16:19], fr[19]
    R = f(R)
    with np.errstate(all="ignore"):
        dz = np.sqrt((f(1.) - dx * dx) - dy * dy)
        sd = (ns[0] * dx + ns[1] * dy) + ns[2] * dz
        sp = hs - (ns[0] * x + ns[1] * y)
        on_sample = (sd > 0.) & (sp >= 0.)
        t = sp / sd
        p0, p1, p2 = x + dx * t, y + dy * t, dz * t
        L = T / sd
        s = u3 * L
        zn = s * sd
        pp0, pp1, pp2 = p0 + dx * s, p1 + dy * s, p2 + dz * s
        a, b = (f(2.) * u1 - f(1.)) * R, (f(2.) * u2 - f(1.)) * R
        q0, q1, q2 = c[0] - pp0, c[1] - pp1, c[2] - pp2
        f0 = a + ((u[0] * q0 + u[1] * q1) + u[2] * q2)
        f1 = b + ((v[0] * q0 + v[1] * q1) + v[2] * q2)
        f2 = (n[0] * q0 + n[1] * q1) + n[2] * q2
        seen = f2 > 0.
        r2 = (f0 * f0 + f1 * f1) + f2 * f2
        r = np.sqrt(r2)
        d0, d1, d2 = f0 / r, f1 / r, f2 / r
        g = ((R * R) * d2) / (f(PI) * r2)
        h = np.sqrt(d2 * d2 + d0 * d0)
        cn = ((k[0] * f0 + k[1] * f1) + k[2] * f2) / r
        tz_raw = T - zn
        tz = np.where(tz_raw < 0., f(0.), tz_raw)
        s_out = np.where(cn > 0., tz / cn, zn / (f(0.) - cn))
        leaves = (cn > 0.) | (cn < 0.)
        gl = g * L
        fits = gl < 1.
        zero = np.zeros_like(h)
        e1 = [d2 / h, zero, f(0.) - d0 / h]
        e2 = [f(0.) - (d0 * d1) / h, h, f(0.) - (d1 * d2) / h]
        even = np.asarray(odd) == 0
        e = [np.where(even, e1[j], e2[j]) for j in range(3)]
        out = np.stack([a, b, zero, d0, d1, d2, e[0], e[1], e[2], t, r, gl, s, s_out], axis=1)
    what = np.where(~on_sample, MISS_SAMPLE, np.where(~seen | ~leaves, MISS_DETECTOR, np.where(~fits, MISS_SAMPLE, INJECT))).astype(np.int32)
    out[what != INJECT] = 0.
    return out, what, dict(cn=cn, L=L, g=g, gl=gl, tz_raw=tz_raw, sd=sd, zn=zn, f2=f2)


# ---- the host compile ---------------------------------------------------------------------------------------------------------
def build_slab_host(directory):
    so = os.path.join(str(directory), "emit_slab_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "emit_slab_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, u64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.slab_state_n.restype = None
    L.slab_state_n.argtypes = [C.c_int64, dp, u64p, dp, C.c_double, C.c_uint64, dp, i32p]
    L.slab_at_n.restype = None
    L.slab_at_n.argtypes = [C.c_int64, dp, i32p, dp, dp, C.c_double, dp, i32p]
    L.slab_frame.restype = None
    L.slab_frame.argtypes = [dp, C.c_double, dp]
    L.slab_bad.restype = C.c_int
    L.slab_bad.argtypes = [C.c_double, C.c_int, dp, C.c_int, dp, i32p]
    L.slab_exp_neg_n.restype = None
    L.slab_exp_neg_n.argtypes = [C.c_int64, dp, dp]
    L.slab_weight_n.restype = None
    L.slab_weight_n.argtypes = [C.c_int64] + [dp] * 8
    L.slab_dtravel_n.restype = None
    L.slab_dtravel_n.argtypes = [C.c_int64] + [dp] * 6
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_slab(L, four, slots, frame, R, seed):
    """four [n, 4] = x, y, dx, dy; slots [n] -> (out [n, 14], zero rows where nothing is injected; what [n])"""
    a = np.ascontiguousarray(four, dtype=np.float64)
    s = np.ascontiguousarray(slots, dtype=np.uint64)
    fr = np.ascontiguousarray(frame, dtype=np.float64)
    out = np.zeros((a.shape[0], N_STATE))
    what = np.zeros(a.shape[0], dtype=np.int32)
    L.slab_state_n(a.shape[0], _dp(a), s.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(fr), R, seed, _dp(out), what.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, what


def host_slab_at(L, four, odd, u, frame, R):
    """the same with the three uniforms given: u [n, 3]"""
    a = np.ascontiguousarray(four, dtype=np.float64)
    o = np.ascontiguousarray(odd, dtype=np.int32)
    uu = np.ascontiguousarray(u, dtype=np.float64)
    fr = np.ascontiguousarray(frame, dtype=np.float64)
    assert uu.shape == (a.shape[0], 3) and o.shape == (a.shape[0],)
    out = np.zeros((a.shape[0], N_STATE))
    what = np.zeros(a.shape[0], dtype=np.int32)
    L.slab_at_n(a.shape[0], _dp(a), o.ctypes.data_as(C.POINTER(C.c_int32)), _dp(uu), _dp(fr), R, _dp(out), what.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, what


def host_slab_frame(L, spec8, T):
    s = np.array(spec8, dtype=np.float64)
    fr = np.zeros(20)
    L.slab_frame(_dp(s), T, _dp(fr))
    return fr


def host_exp_neg(L, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    L.slab_exp_neg_n(x.shape[0], _dp(x), _dp(y))
    return y


def host_weight(L, wa, gl, mu_in, s, mu_out, s_out, wb):
    """pc_emit_slab_weight, elementwise over arrays broadcast to one shape"""
    arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in np.broadcast_arrays(wa, gl, mu_in, s, mu_out, s_out, wb)]
    w = np.zeros(arrs[0].shape)
    L.slab_weight_n(w.size, *[_dp(v) for v in arrs], _dp(w))
    return w


def np_weight(wa, gl, mu_in, s, mu_out, s_out, wb):
    f = np.float64
    with np.errstate(all="ignore"):
        a = mu_in * s + mu_out * s_out
        att = np_exp_neg(f(0.) - a)
        return ((wa * gl) * att) * wb


@pytest.fixture(scope="module")
def slab_host(tmp_path_factory):
    return build_slab_host(tmp_path_factory.mktemp("emit_slab_host"))


@pytest.fixture(scope="module")
def emit_host(tmp_path_factory):
    return build_emit_host(tmp_path_factory.mktemp("emit_host_for_slab"))


def _uniforms3(oracle, seed, slots):
    return np.array([[oracle.uniform(seed, int(s), 0, d) for d in range(3)] for s in slots])


# ---- 1. the contract, bit for bit -----------------------------------------------------------------------------------------------
def test_state_weight_path_and_frame_are_the_contract_bit_for_bit(slab_host, oracle):
    rng = np.random.default_rng(20251)
    a, slots = _entries(2000, rng)
    u = _uniforms3(oracle, SEED, slots)
    assert 0. <= u.min() and u.max() < 1. and not np.array_equal(u[:, 1], u[:, 2])
    odd = (slots & np.uint64(1)).astype(np.int32)
    seen = np.zeros(5, dtype=np.int64)
    signs = [0, 0]
    #          focus, depth, wd,  off_u, off_v,  R,      T
    places = [(0.5, 0., 0.5, 0., 0., 0.0585, 0.01), (0.5, -0.002, 0.5, 0.002, -0.001, 0.0585, 0.0037), (0.5, 0.02, 0.005, 0., 0., 0.01, 1.)]
    n_total = 0
    for alpha in (0., math.pi / 2., math.pi, 3. * math.pi / 4.):
        for beta in BETAS:
            for focus, depth, wd, ou, ov, R, T in places:
                fr = host_slab_frame(slab_host, (focus, beta, depth, alpha, wd, ou, ov, R), T)
                assert same_bits(fr, np_slab_frame(focus, beta, depth, alpha, wd, ou, ov, T)), (alpha, beta)
                got, what = host_slab(slab_host, a, slots, fr, R, SEED)
                want, what_w, mid = np_slab(a[:, 0], a[:, 1], a[:, 2], a[:, 3], odd, u[:, 0], u[:, 1], u[:, 2], fr, R)
                assert np.array_equal(what, what_w), (alpha, beta, focus, depth)
                assert same_bits(got, want), (alpha, beta, focus, depth)
                # the same through the entry point that takes the uniforms
                got_at, what_at = host_slab_at(slab_host, a, odd, u, fr, R)
                assert np.array_equal(what_at, what) and same_bits(got_at, got)
                ok = what == INJECT
                L = mid["L"][ok]
                assert not got[:, 2].any() and np.all(got[ok, 5] > 0.) and np.all(got[ok, GL] > 0.) and np.all(got[ok, GL] < 1.)
                assert np.all(got[ok, SOUT] >= 0.) and np.all(got[ok, S] >= 0.) and np.all(got[ok, S] < L)
                signs[0] += int((mid["cn"][ok] > 0.).sum())
                signs[1] += int((mid["cn"][ok] < 0.).sum())
                seen += np.bincount(what, minlength=5)
                n_total += len(what)
    print("entries", n_total, "injected, missed the sample, missed the detector:", seen[INJECT], seen[MISS_SAMPLE], seen[MISS_DETECTOR],
          "out through the back / the front:", signs)
    assert n_total >= 20000 and seen[INJECT] > 5000 and seen[MISS_SAMPLE] > 5000 and seen[MISS_DETECTOR] > 500 and min(signs) > 1000
    other, _ = host_slab(slab_host, a, slots, fr, R, SEED + 1)
    assert not same_bits(other, got)
    # the weight (with the exponential) and the path
    n = 50000
    wa, gl, wb = rng.random(n), rng.random(n), rng.random(n)
    mu_in, mu_out = rng.uniform(0., 3000., n), rng.uniform(0., 3000., n)
    s, s_out = rng.uniform(0., 0.02, n), rng.uniform(0., 0.02, n)
    mu_in[:100], mu_out[:100] = 0., 0.
    s_out[100:200] = 1e300                                   # an emitted ray along the slab: nothing comes out
    w = host_weight(slab_host, wa, gl, mu_in, s, mu_out, s_out, wb)
    assert same_bits(w, np_weight(wa, gl, mu_in, s, mu_out, s_out, wb))
    assert same_bits(w[:100], (wa[:100] * gl[:100]) * wb[:100]) and not w[100:200].any() and not np.signbit(w[100:200]).any()
    da, t, r, db, out = rng.uniform(0., 20., n), rng.uniform(0., 3., n), rng.uniform(0., 3., n), rng.uniform(0., 20., n), np.zeros(n)
    slab_host.slab_dtravel_n(n, _dp(da), _dp(t), _dp(s), _dp(r), _dp(db), _dp(out))
    assert same_bits(out, (((da + t) + s) + r) + db)
    # the exponential alone, special values included
    x = np.concatenate([-rng.uniform(0., 700., 20000), -np.exp(rng.uniform(-40., 7., 5000)), [0., -0., -700., np.nextafter(-700., -1e3), -701.,
                        -745., -1e10, -np.inf, np.nan, -5e-324, -1e-300, -0.5 * math.log(2.), np.nextafter(-0.5 * math.log(2.), -1.)]])
    assert same_bits(host_exp_neg(slab_host, x), np_exp_neg(x))


# ---- 2. the exponential ---------------------------------------------------------------------------------------------------------
def test_exponential_against_mpmath(slab_host):
    """pc_emit_exp_neg against mpmath at 40 digits on a grid over [-700, 0] (and points crowded towards 0 and around the reduction's
    half-way points): 1e-14 relative, the bound pc_device.h states for this polynomial's shape."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(3)
    half = (np.arange(0, 1010) + 0.5) * math.log(2.)
    x = np.concatenate([np.linspace(-700., 0., 14001), -np.exp(rng.uniform(-40., 6.55, 3000)), -half[half <= 700.],
                        -np.nextafter(half[half <= 700.], 0.), -rng.uniform(0., 700., 3000)])
    assert x.min() >= -700. and x.max() <= 0.
    y = host_exp_neg(slab_host, x)
    worst, at = 0., 0.
    for xi, yi in zip(x, y):
        e = mp.exp(mp.mpf(float(xi)))
        err = float(abs(mp.mpf(float(yi)) - e) / e)
        if err > worst:
            worst, at = err, xi
    print("pc_emit_exp_neg: worst relative error %.3g at x = %r over %d points" % (worst, at, len(x)))
    assert worst <= 1e-14
    assert np.all(y > 2.2250738585072014e-308)                        # normal everywhere on [-700, 0]
    z = host_exp_neg(slab_host, np.array([np.nextafter(-700., -1e3), -700.5, -746., -1e300, -np.inf]))
    assert not z.any() and not np.signbit(z).any()                    # +0 exactly below -700
    one = host_exp_neg(slab_host, np.array([0., -0.]))
    assert one[0] == 1. and one[1] == 1.
    assert np.isnan(host_exp_neg(slab_host, np.array([np.nan]))[0])


# ---- 3. zero attenuation --------------------------------------------------------------------------------------------------------
def test_zero_attenuation_and_the_thin_emit(slab_host, emit_host, oracle):
    """With both coefficients zero att is exactly 1.  With the interaction in the front face (u3 = 0, which pc_emit_slab_at takes as
    an argument) the slab's state is the thin emit's with gl = g * L bit for bit, and its outcome is the thin emit's: the two `missed`
    conditions are unchanged.  The first sixteen numbers of the frame are emit_frame's."""
    import polycap_amd
    rng = np.random.default_rng(77)
    a, slots = _entries(1500, rng)
    u = _uniforms3(oracle, SEED, slots)
    odd = (slots & np.uint64(1)).astype(np.int32)
    u0 = u.copy()
    u0[:, 2] = 0.
    n_inj = 0
    for alpha, beta, T in ((0., 0., 0.01), (math.pi / 2., math.pi / 4., 0.002), (math.pi / 2., -math.pi / 4., 0.3), (math.pi, 0., 1.)):
        spec = (0.5, beta, 0.001, alpha, 0.5, 0.002, -0.001, 0.0585)
        fr = host_slab_frame(slab_host, spec, T)
        lib = polycap_amd.emit_slab_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7], thickness=T)
        thin = polycap_amd.emit_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7])["frame"]
        assert same_bits(lib["frame"], fr) and same_bits(fr[:16], thin) and fr[19] == T and lib["thickness"] == T and same_bits(lib["k"], fr[16:19])
        got, what = host_slab_at(slab_host, a, odd, u0, fr, spec[7])
        t_out, t_what = host_emit(emit_host, a, slots, thin, spec[7], SEED)
        _, _, mid = np_slab(a[:, 0], a[:, 1], a[:, 2], a[:, 3], odd, u0[:, 0], u0[:, 1], u0[:, 2], fr, spec[7])
        with np.errstate(all="ignore"):
            guarded = (t_what == INJECT) & ~(mid["gl"] < 1.)
            flat = (t_what == INJECT) & (mid["cn"] == 0.)
        assert np.array_equal(what[~guarded & ~flat], t_what[~guarded & ~flat])
        assert np.all(what[guarded & ~flat] == MISS_SAMPLE) and np.all(what[flat] == MISS_DETECTOR)
        ok = what == INJECT
        n_inj += int(ok.sum())
        assert same_bits(got[ok, :11], t_out[ok, :11]) and not got[ok, S].any()
        sd = mid["sd"][ok]
        assert same_bits(got[ok, GL], t_out[ok, 11] * (np.float64(T) / sd))
        # mu = 0: att = 1 exactly, whatever the paths are
        full, what_f = host_slab(slab_host, a, slots, fr, spec[7], SEED)
        okf = what_f == INJECT
        wa, wb = rng.random(int(okf.sum())), rng.random(int(okf.sum()))
        w = host_weight(slab_host, wa, full[okf, GL], 0., full[okf, S], 0., full[okf, SOUT], wb)
        assert same_bits(w, (wa * full[okf, GL]) * wb)
        assert same_bits(host_weight(slab_host, 1., 1., 0., full[okf, S], 0., full[okf, SOUT], 1.), np.ones(int(okf.sum())))
    assert n_inj > 1500


# ---- 4. the closed form ---------------------------------------------------------------------------------------------------------
def test_mean_attenuation_is_the_closed_form(slab_host):
    """Photons on A's axis, a far detector (wd = 100) and a small target: every emitted ray has the cosine cn = k2 of the frame to the
    slab's normal but for what is derived below, and the mean of L * att over 2e5 streams is the depth integral over the path s,
    uniform on [0, L), L = T / sd:

      out through the front (cn < 0, case B: sample_angle -pi/4, det_angle pi/2), s_out = s sd / |cn|:
          integral_0^L exp(-(mu_in + mu_out sd/|cn|) s) ds = (1 - exp(-K T)) / (K sd),   K = mu_in/sd + mu_out/|cn|
      out through the back (cn > 0, case A: angles (0, 0)), s_out = (T - s sd) / cn:
          integral_0^L exp(-mu_in s - mu_out (T - s sd)/cn) ds = exp(-mu_out T/cn) (1 - exp(-K' T)) / (K' sd),   K' = mu_in/sd - mu_out/cn
      which is the first form, with K = mu_in/sd + mu_out/|cn|, exactly when mu_out = 0.

    Case A is therefore checked against the first form at mu_out = 0, where it holds for a ray through the back, and, beyond that,
    at mu_out > 0 against the second form, so that the path out through the back is checked too.  Case B is checked against the first
    form with both coefficients above zero.

    Margin: 4 standard errors of the mean, from the sample itself, plus 1e-6 relative for the variation of cn.  Its derived size: the
    point of emission lies within L of the axis point and the target point within R sqrt(2) of B's centre, so the ray deviates from
    the nominal one by delta <= (L + R sqrt(2)) / (wd - L), and |cn - k2| <= delta.  With T = 2^-15 cm, R = 1e-6 cm, sd >= cos(pi/4):
    L <= 4.4e-5, delta <= 4.5e-7, relative to |cn| >= 0.707: 6.4e-7.  The exponent mu_out s_out = x changes by x * 6.4e-7 and att by
    att * x * 6.4e-7 <= 0.37 * 6.4e-7 = 2.4e-7 (x exp(-x) <= 1/e) in absolute terms; the coefficients below keep the mean of att above
    0.4, so the mean moves by less than 6e-7 relative < 1e-6."""
    n = 200000
    T, R, wd = 2. ** -15, 1e-6, 100.
    slots = np.arange(n, dtype=np.uint64)
    four = np.zeros((n, 4))
    cases = (("A, mu_out = 0", 0., 0., 30000., 0.), ("A", 0., 0., 30000., 20000.), ("A, mu_in = 0", 0., 0., 0., 25000.),
             ("B", -math.pi / 4., math.pi / 2., 16000., 23000.), ("B, mu_in = 0", -math.pi / 4., math.pi / 2., 0., 23000.))
    for name, beta, alpha, mu_in, mu_out in cases:
        fr = host_slab_frame(slab_host, (0.5, beta, 0., alpha, wd, 0., 0., R), T)
        got, what = host_slab(slab_host, four, slots, fr, R, SEED)
        assert np.all(what == INJECT)
        sd, cn = float(fr[2]), float(fr[18])                   # n_s . (0, 0, 1) and n_s . n
        L = T / sd
        assert abs(sd - math.cos(beta)) < 1e-15 and abs(cn - math.cos(alpha - beta)) < 1e-15 and (L + R * math.sqrt(2.)) / (wd - L) <= 4.5e-7
        att = host_weight(slab_host, 1., 1., mu_in, got[:, S], mu_out, got[:, SOUT], 1.)
        v = L * att
        if cn < 0.:
            assert name.startswith("B")
            K = mu_in / sd + mu_out / abs(cn)
            want = (1. - math.exp(-K * T)) / (K * sd)
        else:
            assert name.startswith("A")
            K = mu_in / sd - mu_out / cn
            want = math.exp(-mu_out * T / cn) * (1. - math.exp(-K * T)) / (K * sd)
            if mu_out == 0.:
                Ki = mu_in / sd + mu_out / abs(cn)              # the first form, as it stands
                assert want == (1. - math.exp(-Ki * T)) / (Ki * sd)
        err = v.std(ddof=1) / math.sqrt(n)
        print("%s: mean L att %.9g, closed form %.9g, difference %.2f standard errors (%.3g relative); mean att %.4f"
              % (name, v.mean(), want, (v.mean() - want) / err, (v.mean() - want) / want, att.mean()))
        assert att.mean() > 0.4 and att.min() < 0.6
        assert abs(v.mean() - want) <= 4. * err + 1e-6 * want, (name, v.mean(), want, err)
        assert abs(got[:, S].mean() - 0.5 * L) <= 4. * L / math.sqrt(12. * n)          # the depth is drawn evenly


# ---- 5. the edges ---------------------------------------------------------------------------------------------------------------
def test_edges(slab_host):
    R = 0.0585
    one = lambda four, odd, u, fr, R=R: tuple(v[0] for v in host_slab_at(slab_host, [four], [odd], [u], fr, R))
    # cn of each sign: in line the ray leaves through the back, in the reflection geometry through the front
    fr = host_slab_frame(slab_host, (0.5, 0., 0., 0., 0.5, 0., 0., R), 0.01)
    o, w = one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.25], fr)
    assert w == INJECT and o[S] == 0.0025 and abs(o[SOUT] - 0.0075) < 1e-17 and o[T_] == 0.5
    fr = host_slab_frame(slab_host, (0.5, -math.pi / 4., 0., math.pi / 2., 0.5, 0., 0., R), 0.01)
    o, w = one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.25], fr)
    assert fr[18] < 0. and w == INJECT and abs(o[SOUT] - o[S]) < 0.02 * o[S] and o[S] > 0.      # sd = |cn| but for B's finite distance (s / wd = 0.007): out as far as in
    # cn = 0 exactly: an untilted slab, B at 90 degrees (k = (-1, 0, ca) with ca = cos of the double nearest pi/2), the interaction at
    # the height of B's centre and the target point in the centre: f0 = ca*q0, f2 = q0, so that k.f = -(ca*q0) + ca*q0 cancels
    T = 2. ** -6
    fr = host_slab_frame(slab_host, (0.5, 0., -2. ** -7, math.pi / 2., 0.5, 0., 0., R), T)
    assert fr[16] == -1. and fr[17] == 0. and 0. < fr[18] < 1e-16 and fr[15] == 0.5 and fr[3] == 0.5 - 2. ** -7
    o, w = one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.5], fr)
    _, w_np, mid = np_slab(*[np.array([0.])] * 4, [0], np.array([0.5]), np.array([0.5]), np.array([0.5]), fr, R)
    assert mid["cn"][0] == 0. and mid["f2"][0] > 0. and w == MISS_DETECTOR and w_np[0] == MISS_DETECTOR
    for u3 in (0.25, 0.75):                                          # above or below that height the ray leaves the slab
        o, w = one([0., 0., 0., 0.], 0, [0.5, 0.5, u3], fr)
        assert w == INJECT and 0. < o[SOUT] < 1e300
    # tz clamped at 0.  The stream's u3 < 1 gives s <= L - ulp(L), and zn = s*sd <= T follows (L <= (T/sd)(1 + 2^-53),
    # s <= L(1 - 2^-53), so s*sd < T before it is rounded); the clamp stands guard, and u3 = 1, which only pc_emit_slab_at can be
    # given, reaches it where L*sd rounds above T (T just below a power of two and L just above it: there L's rounding weighs most)
    fr = host_slab_frame(slab_host, (0.5, 0., 0., 0., 3., 0., 0., R), 0.97)
    rng = np.random.default_rng(5)
    four = np.zeros((4000, 4))
    four[:, 2] = rng.uniform(-0.3, 0.3, 4000)
    ones = np.tile([0.5, 0.5, 1.], (4000, 1))
    got, what = host_slab_at(slab_host, four, np.zeros(4000, dtype=np.int32), ones, fr, R)
    want, what_w, mid = np_slab(four[:, 0], four[:, 1], four[:, 2], four[:, 3], np.zeros(4000), ones[:, 0], ones[:, 1], ones[:, 2], fr, R)
    neg = mid["tz_raw"] < 0.
    print("u3 = 1: T - zn negative in", int(neg.sum()), "of 4000, zero in", int((mid["tz_raw"] == 0.).sum()))
    assert neg.sum() > 10 and np.all(what == INJECT) and same_bits(got, want)
    assert not got[neg, SOUT].any() and not np.signbit(got[neg, SOUT]).any()
    below = np.tile([0.5, 0.5, np.nextafter(1., 0.)], (4000, 1))
    _, _, mid = np_slab(four[:, 0], four[:, 1], four[:, 2], four[:, 3], np.zeros(4000), below[:, 0], below[:, 1], below[:, 2], fr, R)
    assert np.all(mid["tz_raw"] >= 0.) and np.all(mid["zn"] <= 0.97)
    # !(gl < 1): grazing incidence on a thick slab, the interaction in the front face (u3 = 0), the sheet through the photon's start
    # (t = 0) so that B stays near.  dx walks from normal to grazing incidence; each side of the edge gets its outcome
    fr = host_slab_frame(slab_host, (0.5, 0., -0.5, 0., 0.5, 0., 0., 0.3), 1.)
    dxs = np.concatenate([np.linspace(0., 0.9999, 300), 1. - np.logspace(-5, -15, 60)])
    four = np.zeros((len(dxs), 4))
    four[:, 2] = dxs
    zeros = np.tile([0.5, 0.5, 0.], (len(dxs), 1))
    got, what = host_slab_at(slab_host, four, np.zeros(len(dxs), dtype=np.int32), zeros, fr, 0.3)
    want, what_w, mid = np_slab(four[:, 0], four[:, 1], four[:, 2], four[:, 3], np.zeros(len(dxs)), zeros[:, 0], zeros[:, 1], zeros[:, 2], fr, 0.3)
    assert np.array_equal(what, what_w) and same_bits(got, want)
    assert np.array_equal(what == INJECT, mid["gl"] < 1.) and np.all(what[~(mid["gl"] < 1.)] == MISS_SAMPLE)
    assert (what == INJECT).sum() > 50 and (what == MISS_SAMPLE).sum() > 50 and mid["gl"].max() > 1e4
    dx_last = _edge_gl(fr, 0.3, 0., 0.9999)
    for dx, outcome in ((dx_last, INJECT), (np.nextafter(dx_last, 1.), MISS_SAMPLE)):
        assert one([0., 0., dx, 0.], 0, [0.5, 0.5, 0.], fr, 0.3)[1] == outcome
    # the emit's two conditions, at their edges: sd = 0 and one ulp inside; sp = 0 and one ulp behind; f2 = 0 and one ulp in front
    fr = host_slab_frame(slab_host, (0.5, 0., 0., 0., 0.5, 0., 0., R), 0.01)
    assert one([0., 0., 1., 0.], 0, [0.5, 0.5, 0.5], fr)[1] == MISS_SAMPLE
    fr = host_slab_frame(slab_host, (0.5, 0., -0.5, 0., 0.5, 0., 0., R), 0.01)
    o, w = one([0.001, 0., 0.01, 0.], 0, [0.5, 0.5, 0.5], fr)
    assert fr[3] == 0. and w == INJECT and o[T_] == 0.
    fr = host_slab_frame(slab_host, (0.5, 0., np.nextafter(-0.5, -1.), 0., 0.5, 0., 0., R), 0.01)
    assert fr[3] < 0. and one([0.001, 0., 0.01, 0.], 0, [0.5, 0.5, 0.5], fr)[1] == MISS_SAMPLE
    fr = host_slab_frame(slab_host, (0.5, 0., 0.25, 0., 0.25, 0., 0., R), 0.01)      # the front face in B's entrance plane
    assert one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.], fr)[1] == MISS_DETECTOR
    assert one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.5], fr)[1] == MISS_DETECTOR          # ... and the interaction behind it
    # one ulp in front of B's entrance plane g = R^2 / (pi r^2) is 9e28: a slab of 0.01 cm falls to the guard, one of 1e-40 cm emits
    fr = host_slab_frame(slab_host, (0.5, 0., 0.25 - 2. ** -53, 0., 0.25, 0., 0., R), 0.01)
    assert one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.], fr)[1] == MISS_SAMPLE
    fr = host_slab_frame(slab_host, (0.5, 0., 0.25 - 2. ** -53, 0., 0.25, 0., 0., R), 1e-40)
    o, w = one([0., 0., 0., 0.], 0, [0.5, 0.5, 0.], fr)
    assert w == INJECT and o[5] > 0. and o[R_] > 0. and 0. < o[GL] < 1e-10


def _edge_gl(fr, R, lo, hi):
    """the largest dx in [lo, hi) of a photon (0, 0, dx, 0) with u = (0.5, 0.5, 0) whose gl is below 1"""
    from tests.test_relay_pose_cpu import _edge

    def fits(dx):
        z = np.array([0.])
        with np.errstate(all="ignore"):
            return bool(np_slab(z, z, np.array([dx]), z, [0], np.array([0.5]), np.array([0.5]), z, fr, R)[2]["gl"][0] < 1.)

    return _edge(fits, lo, hi)


# ---- 6. the spec check and the symbols ------------------------------------------------------------------------------------------
def test_validate_names_the_field(slab_host):
    import polycap_amd
    from polycap_amd import _cabi
    L = polycap_amd.lib()
    valid = lambda spec=GOOD, **kw: polycap_amd.emit_slab_valid(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7],
                                                                 **dict(dict(thickness=0.01, mu_in=[100., 0.], mu_out=[50.]), **kw))
    assert valid() and valid(thickness=1.) and valid(thickness=5e-324) and valid(mu_in=[0.], mu_out=[1.7976931348623157e308])
    assert valid(energy_map=[0, 1, 1])
    at = C.c_int32(0)
    dp = C.POINTER(C.c_double)

    def header_says(T, mi, mo):
        mi, mo = np.array(mi, dtype=np.float64), np.array(mo, dtype=np.float64)
        return slab_host.slab_bad(T, len(mi), mi.ctypes.data_as(dp), len(mo), mo.ctypes.data_as(dp), C.byref(at)), at.value

    assert header_says(0.01, [100., 0.], [50.]) == (0, -1)
    for bad in (0., -0., -0.01, np.nextafter(1., 2.), 2., math.nan, math.inf, -math.inf):
        assert not valid(thickness=bad), bad
        msg = L.pc_hip_last_error().decode()
        assert msg.startswith("pc_hip_slab_validate: thickness "), (bad, msg)
        assert header_says(bad, [1.], [1.]) == (1, -1)
    for bad in (-1e-300, -1., math.nan, math.inf, -math.inf):
        assert not valid(mu_in=[3., bad]) and L.pc_hip_last_error().decode().startswith("pc_hip_slab_validate: mu_in[1] "), bad
        assert not valid(mu_out=[bad]) and L.pc_hip_last_error().decode().startswith("pc_hip_slab_validate: mu_out[0] "), bad
        assert header_says(0.5, [3., bad], [1.]) == (2, 1) and header_says(0.5, [3., 1.], [1., 2., bad]) == (3, 2)
    assert not valid(mu_in=[]) and b"n_mu_in" in L.pc_hip_last_error()
    assert not valid(mu_out=[]) and b"n_mu_out" in L.pc_hip_last_error()
    # the emit's fields are checked as the emit checks them, and first
    for k, name in enumerate(FIELDS):
        spec = list(GOOD)
        spec[k] = math.nan
        assert not valid(spec, thickness=0.) and L.pc_hip_last_error().decode().startswith("pc_hip_slab_validate: " + name + " "), name
        with pytest.raises(polycap_amd.HipError) as e:
            polycap_amd.emit_slab_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7], thickness=0.01)
        assert e.value.status == -2 and name in str(e.value)
    assert not valid(energy_map=[0, -1]) and b"map[1]" in L.pc_hip_last_error()
    with pytest.raises(polycap_amd.HipError) as e:
        polycap_amd.emit_slab_frame(*GOOD[:5], GOOD[5:7], GOOD[7], thickness=0.)
    assert e.value.status == -2 and "thickness" in str(e.value)
    assert L.pc_hip_slab_validate(None) == -2 and b"spec" in L.pc_hip_last_error()
    s = _cabi.SlabS(_cabi.EmitS(*GOOD, 0, 0, None), 0.01, 2, None, 1, None)
    assert L.pc_hip_slab_validate(C.byref(s)) == -2 and b"n_mu_in" in L.pc_hip_last_error()
    assert C.sizeof(_cabi.SlabS) == 128
    # the three arguments of a slab come together
    for kw in (dict(thickness=0.01), dict(mu_in=[1.]), dict(mu_out=[1.]), dict(thickness=0.01, mu_in=[1.]), dict(mu_in=[1.], mu_out=[1.])):
        with pytest.raises(ValueError):
            polycap_amd.emit_slab_valid(*GOOD[:5], GOOD[5:7], GOOD[7], **kw)
        with pytest.raises(ValueError):
            polycap_amd.hip._slab_given("emit", kw.get("thickness"), kw.get("mu_in"), kw.get("mu_out"))
    assert polycap_amd.hip._slab_given("emit", None, None, None) is False


def test_slab_symbols_are_exported_and_declared():
    import polycap_amd
    polycap_amd.lib()
    so = os.path.join(ROOT, "polycap_amd", "lib", "libpolycap.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert [n for n in names if n.startswith("pc_hip_") and "slab" in n] == sorted(NEW_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "polycap-hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"POLYCAP_EXTERN\s+[^;(]*?\b(\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    # nothing else came with them: no kernel stub, no C++ instantiation, no undeclared pc_hip_ name
    assert not [n for n in names if n.startswith("_Z") or "pc_emit" in n or "pc_rule" in n]
    assert [n for n in names if n.startswith("pc_hip_") and n not in declared] == []
