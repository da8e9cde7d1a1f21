"""Layered emits without a GPU (an emit relay through a stack of sample layers; include/polycap-hip.h, pc_hip_layers_*): the host part
of pc_emit_layers.h compiled for the host (tests/emit_layers/emit_layers_host.cpp) against a numpy restatement of the contract bit for
bit; the optical depths against exact fractions; the edges; the identities with the slab; the spec check; and the exported symbols."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_emit_cpu import BETAS, FIELDS, GOOD, INJECT, MISS_DETECTOR, MISS_SAMPLE, PI, SEED, _entries, same_bits
from tests.test_emit_slab_cpu import (GL, S, _uniforms3, build_slab_host, host_slab_at, host_slab_frame, host_weight, np_exp_neg,
                                      np_slab_frame)

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "emit_layers")
NEW_SYMBOLS = ("pc_hip_layers_frame", "pc_hip_layers_run", "pc_hip_layers_validate")
N_STATE = 18
L_T, L_R, L_GL, L_S, L_SD, L_CN, L_A, L_B, L_J = range(9, 18)          # the state behind the emit's nine numbers
BAD_N, BAD_THICKNESS, BAD_TOTAL, BAD_MU_IN, BAD_MU_OUT, BAD_PRODUCTION = range(1, 7)
U = 2. ** -53


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def np_bounds(thickness):
    Z = np.zeros(len(thickness) + 1)
    for j, t in enumerate(thickness):
        Z[j + 1] = Z[j] + np.float64(t)
    return Z


def np_tables(thickness, mu_in, mu_out):
    """(pin, pout, sout): the prefix sums left to right, the suffix sum right to left, each product formed before its add"""
    th = np.asarray(thickness, dtype=np.float64)
    mu_in, mu_out = np.asarray(mu_in, dtype=np.float64), np.asarray(mu_out, dtype=np.float64)
    n = len(th)
    pin, pout, sout = np.zeros_like(mu_in), np.zeros_like(mu_out), np.zeros_like(mu_out)
    for j in range(1, n):
        pin[j] = pin[j - 1] + mu_in[j - 1] * th[j - 1]
        pout[j] = pout[j - 1] + mu_out[j - 1] * th[j - 1]
    for j in range(n - 2, -1, -1):
        sout[j] = sout[j + 1] + mu_out[j + 1] * th[j + 1]
    return pin, pout, sout


def np_layers_frame(focus, beta, depth, alpha, wd, off_u, off_v, T, qmax):
    return np.concatenate([np_slab_frame(focus, beta, depth, alpha, wd, off_u, off_v, T), [np.float64(qmax)]])


def np_layers(x, y, dx, dy, odd, u1, u2, u3, fr, R, Z):
    """(out [n, 18] = the emit's nine, t, r, gl, s, sd, cn, za, zb, j; what [n]; the intermediate values by name): every operation one
    IEEE fp64 numpy operation, in the contract's order; the rows of photons that are not injected are zero"""
    f = np.float64
    ns, hs, u, v, n, c, k, T, qmax = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16], fr[16:19], fr[19], fr[20]
    R = f(R)
    Z = np.asarray(Z, dtype=np.float64)
    nl = len(Z) - 1
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
        leaves = (cn > 0.) | (cn < 0.)
        gl = g * L
        fits = gl * qmax < 1.
        j = np.zeros(len(zn), dtype=np.int64)
        for i in range(1, nl):
            j += zn >= Z[i]
        za = zn - Z[j]
        zb_raw = Z[j + 1] - zn
        zb = np.where(zb_raw < 0., f(0.), zb_raw)
        zero = np.zeros_like(h)
        e1 = [d2 / h, zero, f(0.) - d0 / h]
        e2 = [f(0.) - (d0 * d1) / h, h, f(0.) - (d1 * d2) / h]
        even = np.asarray(odd) == 0
        e = [np.where(even, e1[i], e2[i]) for i in range(3)]
        out = np.stack([a, b, zero, d0, d1, d2, e[0], e[1], e[2], t, r, gl, s, sd, cn, za, zb, j.astype(np.float64)], axis=1)
    what = np.where(~on_sample, MISS_SAMPLE, np.where(~seen | ~leaves, MISS_DETECTOR, np.where(~fits, MISS_SAMPLE, INJECT))).astype(np.int32)
    out[what != INJECT] = 0.
    return out, what, dict(cn=cn, L=L, g=g, gl=gl, zb_raw=zb_raw, sd=sd, zn=zn, f2=f2, j=j)


def np_weight(state, wa, wb, ea, e, pin, mu_in, sout, pout, mu_out, prod):
    """the contract's weight of every row of state at the energies (ea, e); tables [n_layers, energies].  Returns (w, tau_in, tau_out)"""
    f = np.float64
    j = state[:, L_J].astype(np.int64)
    sd, cn, za, zb, gl = state[:, L_SD], state[:, L_CN], state[:, L_A], state[:, L_B], state[:, L_GL]
    with np.errstate(all="ignore"):
        tau_in = (pin[j, ea] + mu_in[j, ea] * za) / sd
        back = (sout[j, e] + mu_out[j, e] * zb) / cn
        front = (pout[j, e] + mu_out[j, e] * za) / (f(0.) - cn)
        tau_out = np.where(cn > 0., back, front)
        w = ((wa * gl) * (prod[j, e] * np_exp_neg(f(0.) - (tau_in + tau_out)))) * wb
    return w, tau_in, tau_out


# ---- the host compile ---------------------------------------------------------------------------------------------------------
def build_layers_host(directory):
    so = os.path.join(str(directory), "emit_layers_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "emit_layers_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp, u64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.layers_state_n.restype = None
    L.layers_state_n.argtypes = [C.c_int64, dp, u64p, dp, C.c_double, C.c_int, dp, C.c_uint64, dp, i32p]
    L.layers_at_n.restype = None
    L.layers_at_n.argtypes = [C.c_int64, dp, i32p, dp, dp, C.c_double, C.c_int, dp, dp, i32p]
    L.layers_bounds.restype = None
    L.layers_bounds.argtypes = [C.c_int, dp, dp]
    L.layers_frame.restype = None
    L.layers_frame.argtypes = [dp, C.c_double, C.c_double, dp]
    L.layers_qmax.restype = C.c_double
    L.layers_qmax.argtypes = [C.c_int, C.c_int, dp]
    L.layers_tables.restype = None
    L.layers_tables.argtypes = [C.c_int, dp, C.c_int, dp, C.c_int, dp, dp, dp, dp]
    L.layers_bad.restype = C.c_int
    L.layers_bad.argtypes = [C.c_int, dp, C.c_int, dp, C.c_int, dp, dp, i32p, i32p]
    L.layers_weight_n.restype = None
    L.layers_weight_n.argtypes = [C.c_int64, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int] + [dp] * 7
    L.layers_tau_n.restype = None
    L.layers_tau_n.argtypes = [C.c_int64] + [dp] * 5
    L.layers_w_n.restype = None
    L.layers_w_n.argtypes = [C.c_int64] + [dp] * 7
    L.layers_dtravel_n.restype = None
    L.layers_dtravel_n.argtypes = [C.c_int64] + [dp] * 6
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Stack:
    """a stack of layers as the library lays it out: thickness [n], mu_in [n, n_in], mu_out and production [n, n_out], and, from the host
    compile, the boundaries, qmax and the prefix tables"""

    def __init__(self, L, thickness, mu_in, mu_out, production=None):
        self.th = _d(thickness).reshape(-1)
        self.n = len(self.th)
        self.mu_in, self.mu_out = _d(mu_in).reshape(self.n, -1), _d(mu_out).reshape(self.n, -1)
        self.prod = np.ones_like(self.mu_out) if production is None else _d(production).reshape(self.n, -1)
        self.n_in, self.n_out = self.mu_in.shape[1], self.mu_out.shape[1]
        self.Z = np.zeros(self.n + 1)
        L.layers_bounds(self.n, _dp(self.th), _dp(self.Z))
        self.T = float(self.Z[-1])
        self.qmax = L.layers_qmax(self.n, self.n_out, _dp(self.prod))
        self.pin, self.pout, self.sout = np.zeros_like(self.mu_in), np.zeros_like(self.mu_out), np.zeros_like(self.mu_out)
        L.layers_tables(self.n, _dp(self.th), self.n_in, _dp(self.mu_in), self.n_out, _dp(self.mu_out), _dp(self.pin), _dp(self.pout), _dp(self.sout))

    def as_layers(self):
        """the `layers=` argument of the Python layer"""
        return [dict(thickness=self.th[j], mu_in=self.mu_in[j], mu_out=self.mu_out[j], production=self.prod[j]) for j in range(self.n)]


def host_layers_frame(L, spec8, T, qmax):
    s = np.array(spec8, dtype=np.float64)
    fr = np.zeros(21)
    L.layers_frame(_dp(s), T, qmax, _dp(fr))
    return fr


def host_layers(L, four, slots, frame, R, Z, seed):
    """four [n, 4] = x, y, dx, dy; slots [n] -> (out [n, 18], zero rows where nothing is injected; what [n])"""
    a, s, fr, Z = _d(four), np.ascontiguousarray(slots, dtype=np.uint64), _d(frame), _d(Z)
    out = np.zeros((a.shape[0], N_STATE))
    what = np.zeros(a.shape[0], dtype=np.int32)
    L.layers_state_n(a.shape[0], _dp(a), s.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(fr), R, len(Z) - 1, _dp(Z), seed, _dp(out),
                     what.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, what


def host_layers_at(L, four, odd, u, frame, R, Z):
    """the same with the three uniforms given: u [n, 3]"""
    a, o, uu, fr, Z = _d(four), np.ascontiguousarray(odd, dtype=np.int32), _d(u), _d(frame), _d(Z)
    assert uu.shape == (a.shape[0], 3) and o.shape == (a.shape[0],)
    out = np.zeros((a.shape[0], N_STATE))
    what = np.zeros(a.shape[0], dtype=np.int32)
    L.layers_at_n(a.shape[0], _dp(a), o.ctypes.data_as(C.POINTER(C.c_int32)), _dp(uu), _dp(fr), R, len(Z) - 1, _dp(Z), _dp(out),
                  what.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, what


def host_layers_weight(L, state, wa, wb, ea, e, st):
    """pc_emit_layers_weight_at of every row of state at the energies (ea, e) of the stack st"""
    state = _d(state).reshape(-1, N_STATE)
    n = state.shape[0]
    wa, wb = _d(np.broadcast_to(wa, (n,))), _d(np.broadcast_to(wb, (n,)))
    w = np.zeros(n)
    L.layers_weight_n(n, _dp(state), _dp(wa), _dp(wb), st.n_in, int(ea), st.n_out, int(e), _dp(st.pin), _dp(st.mu_in), _dp(st.sout), _dp(st.pout),
                      _dp(st.mu_out), _dp(st.prod), _dp(w))
    return w


def host_tau(L, acc, mu, x, c):
    arrs = [_d(v) for v in np.broadcast_arrays(acc, mu, x, c)]
    tau = np.zeros(arrs[0].shape)
    L.layers_tau_n(tau.size, *[_dp(v) for v in arrs], _dp(tau))
    return tau


@pytest.fixture(scope="module")
def layers_host(tmp_path_factory):
    return build_layers_host(tmp_path_factory.mktemp("emit_layers_host"))


@pytest.fixture(scope="module")
def slab_host(tmp_path_factory):
    return build_slab_host(tmp_path_factory.mktemp("emit_slab_host_for_layers"))


def random_stack(L, rng, n, n_in, n_out, total, zero_some=False):
    th = rng.uniform(0.2, 1., n)
    th *= total / th.sum()
    mu_in, mu_out = rng.uniform(0., 3000., (n, n_in)), rng.uniform(0., 3000., (n, n_out))
    prod = rng.uniform(0., 5., (n, n_out))
    if zero_some:
        mu_in[0], mu_out[n - 1], prod[n // 2] = 0., 0., 0.
    return Stack(L, th, mu_in, mu_out, prod)


# ---- 1. the contract, bit for bit -----------------------------------------------------------------------------------------------
def test_state_and_weight_are_the_contract_bit_for_bit(layers_host, oracle):
    rng = np.random.default_rng(20261)
    a, slots = _entries(1500, rng)
    u = _uniforms3(oracle, SEED, slots)
    odd = (slots & np.uint64(1)).astype(np.int32)
    seen = np.zeros(5, dtype=np.int64)
    signs, per_layer = [0, 0], {}
    #          focus, depth, wd,  off_u, off_v,  R,      T
    places = [(0.5, 0., 0.5, 0., 0., 0.0585, 0.01), (0.5, -0.002, 0.5, 0.002, -0.001, 0.0585, 0.0037), (0.5, 0.02, 0.005, 0., 0., 0.01, 1.)]
    for n in (1, 3, 16):
        hit = np.zeros(n, dtype=np.int64)
        for alpha in (0., math.pi / 2., math.pi):
            for beta in BETAS:
                for focus, depth, wd, ou, ov, R, T in places:
                    st = random_stack(layers_host, rng, n, 2, 3, T, zero_some=n > 1)
                    assert same_bits(st.Z, np_bounds(st.th)) and st.qmax == st.prod.max()
                    for got_t, want_t in zip((st.pin, st.pout, st.sout), np_tables(st.th, st.mu_in, st.mu_out)):
                        assert same_bits(got_t, want_t)
                    assert not st.pin[0].any() and not st.pout[0].any() and not st.sout[n - 1].any()
                    fr = host_layers_frame(layers_host, (focus, beta, depth, alpha, wd, ou, ov, R), st.T, st.qmax)
                    assert same_bits(fr, np_layers_frame(focus, beta, depth, alpha, wd, ou, ov, st.T, st.qmax)), (alpha, beta)
                    got, what = host_layers(layers_host, a, slots, fr, R, st.Z, SEED)
                    want, what_w, mid = np_layers(a[:, 0], a[:, 1], a[:, 2], a[:, 3], odd, u[:, 0], u[:, 1], u[:, 2], fr, R, st.Z)
                    assert np.array_equal(what, what_w), (n, alpha, beta, focus, depth)
                    assert same_bits(got, want), (n, alpha, beta, focus, depth)
                    got_at, what_at = host_layers_at(layers_host, a, odd, u, fr, R, st.Z)
                    assert np.array_equal(what_at, what) and same_bits(got_at, got)
                    ok = what == INJECT
                    j = got[ok, L_J].astype(np.int64)
                    assert np.all((0 <= j) & (j < n)) and np.all(got[ok, L_A] >= 0.) and np.all(got[ok, L_B] >= 0.)
                    assert np.all(got[ok, L_A] <= st.th[j] * (1. + 1e-12)) and np.all(got[ok, L_B] <= st.th[j] * (1. + 1e-12))
                    hit += np.bincount(j, minlength=n)
                    signs[0] += int((got[ok, L_CN] > 0.).sum())
                    signs[1] += int((got[ok, L_CN] < 0.).sum())
                    seen += np.bincount(what, minlength=5)
                    # the weight at every pair of energies, through the function the kernel's rule calls
                    wa, wb = rng.random(int(ok.sum())), rng.random(int(ok.sum()))
                    for ea in range(st.n_in):
                        for e in range(st.n_out):
                            w = host_layers_weight(layers_host, got[ok], wa, wb, ea, e, st)
                            w_np, tau_in, tau_out = np_weight(got[ok], wa, wb, ea, e, st.pin, st.mu_in, st.sout, st.pout, st.mu_out, st.prod)
                            assert same_bits(w, w_np), (n, ea, e)
                            assert np.all(tau_in >= 0.) and np.all(tau_out >= 0.)
        per_layer[n] = hit
        assert hit.min() > 0, (n, hit)
    print("injected, missed the sample, missed the detector:", seen[INJECT], seen[MISS_SAMPLE], seen[MISS_DETECTOR],
          "out through the back / the front:", signs, "interactions per layer:", {k: v.tolist() for k, v in per_layer.items()})
    assert seen[INJECT] > 5000 and seen[MISS_SAMPLE] > 5000 and seen[MISS_DETECTOR] > 500 and min(signs) > 1000
    # the path is the slab's
    n = 1000
    da, t, s, r, db, out = rng.uniform(0., 20., n), rng.uniform(0., 3., n), rng.uniform(0., .02, n), rng.uniform(0., 3., n), rng.uniform(0., 20., n), np.zeros(n)
    layers_host.layers_dtravel_n(n, _dp(da), _dp(t), _dp(s), _dp(r), _dp(db), _dp(out))
    assert same_bits(out, (((da + t) + s) + r) + db)


# ---- 2. the optical depths against exact arithmetic -------------------------------------------------------------------------------
def exact_depth_integral(Zx, mu, z0, z1):
    """integral of the piecewise-constant mu (mu[k] on [Zx[k], Zx[k + 1]), 0 outside the stack) over [z0, z1], in fractions"""
    tot = Fraction(0)
    for k in range(len(mu)):
        lo, hi = max(Zx[k], z0), min(Zx[k + 1], z1)
        if hi > lo:
            tot += Fraction(float(mu[k])) * (hi - lo)
    return tot


def test_optical_depths_against_exact_arithmetic(layers_host, oracle):
    """tau_in and tau_out of the host compile against the exact integral of mu(z) along the two rays, in fractions.Fraction.

    What is exact: the inputs are the doubles the code gets (thicknesses, coefficients, the ray's s, sd and cn), and the true point of
    interaction lies at the depth z* = s*sd, the exact product.  The thicknesses are multiples of 2^-30 cm below 1 cm, so that every
    boundary Z_k is exact.  With n layers, c the ray's cosine and u = 2^-53:

      tau* = (P* + mu_j x*) / c,   P* the exact sum of at most n - 1 products mu_k T_k,   x* the exact offset in layer j.

    Every term is >= 0, so relative errors of the terms carry over to the sum.  The code rounds: each product mu_k T_k once and the
    prefix's adds at most n - 2 times (the first add, to 0, is exact): at most n - 1 roundings on P; the offset's subtraction, the
    product mu_j x, the add and the quotient: 4 more.  That is at most n + 3 factors (1 + d), |d| <= u, on tau: (n + 3) u tau* to first
    order, and (n + 4) u tau* covers the higher orders for n <= 16.

    The error of zn is absolute, not relative to tau: zn = z* (1 + d), so the offset is wrong by at most u z*, whatever its size, and tau
    by u mu z* / c, where mu is the coefficient of layer j -- or, when the rounding carried zn across a boundary, so that the code's layer
    and the exact one are neighbours, the larger of the two coefficients (the stretch between z* and zn, at most u z* long, is then
    counted with one coefficient in the place of the other).  The same term covers the clamp of b at the back face.  So

      |tau - tau*| <= (n + 4) u tau* + 1.01 u mu z* / c

    with mu = the largest coefficient of the code's and the exact layer.  A wrong layer, a wrong face or a prefix that is off by one
    layer moves tau by percents."""
    rng = np.random.default_rng(77)
    worst = [0., 0.]
    n_checked, n_cross = 0, 0
    for n in (1, 3, 16):
        for beta, alpha in ((math.pi / 4., math.pi / 2.), (-math.pi / 4., math.pi / 2.), (0., 0.)):
            th = rng.integers(1, 2 ** 15, n).astype(np.float64) * 2. ** -30
            st = Stack(layers_host, th, rng.uniform(0., 3000., (n, 1)) * rng.choice([1., 1e-3, 0.], (n, 1)), rng.uniform(1., 3000., (n, 1)))
            Zx = [Fraction(0)]
            for t in th:
                Zx.append(Zx[-1] + Fraction(float(t)))
            assert [float(z) for z in Zx] == list(st.Z) and all(Fraction(float(z)) == zx for z, zx in zip(st.Z, Zx))
            a, slots = _entries(500, rng)
            u = _uniforms3(oracle, SEED, slots)
            # a few interactions on and next to the boundaries
            u[:40, 2] = rng.choice(st.Z[:-1], 40) / st.T
            R = 0.0585
            fr = host_layers_frame(layers_host, (0.5, beta, -0.0005, alpha, 0.5, 0., 0., R), st.T, st.qmax)
            got, what = host_layers_at(layers_host, a, (slots & np.uint64(1)).astype(np.int32), u, fr, R, st.Z)
            ok = np.flatnonzero(what == INJECT)
            o = got[ok]
            j = o[:, L_J].astype(np.int64)
            tau_in = host_tau(layers_host, st.pin[j, 0], st.mu_in[j, 0], o[:, L_A], o[:, L_SD])
            back = o[:, L_CN] > 0.
            tau_out = np.where(back, host_tau(layers_host, st.sout[j, 0], st.mu_out[j, 0], o[:, L_B], o[:, L_CN]),
                               host_tau(layers_host, st.pout[j, 0], st.mu_out[j, 0], o[:, L_A], 0. - o[:, L_CN]))
            for i in range(len(ok)):
                zs = Fraction(float(o[i, L_S])) * Fraction(float(o[i, L_SD]))
                jx = max(k for k in range(n) if Zx[k] <= zs) if zs < Zx[n] else n - 1
                assert abs(jx - j[i]) <= 1
                n_cross += jx != j[i]
                sd, cn = Fraction(float(o[i, L_SD])), Fraction(float(o[i, L_CN]))
                want_in = exact_depth_integral(Zx, st.mu_in[:, 0], Fraction(0), zs) / sd
                want_out = exact_depth_integral(Zx, st.mu_out[:, 0], zs, Zx[n]) / cn if cn > 0 else exact_depth_integral(Zx, st.mu_out[:, 0], Fraction(0), zs) / -cn
                for which, (have, want, mu, c) in enumerate(((tau_in[i], want_in, st.mu_in[:, 0], sd), (tau_out[i], want_out, st.mu_out[:, 0], abs(cn)))):
                    bound = (n + 4) * Fraction(U) * want + Fraction(1.01) * Fraction(U) * Fraction(float(max(mu[j[i]], mu[jx]))) * zs / c
                    err = abs(Fraction(float(have)) - want)
                    assert err <= bound, (n, which, i, have, float(want), float(err), float(bound))
                    if bound > 0:
                        worst[which] = max(worst[which], float(err / bound))
                n_checked += 1
    print("optical depths: %d rays, %d with the layer moved by zn's rounding; worst error %.3f (in) %.3f (out) of the bound"
          % (n_checked, n_cross, worst[0], worst[1]))
    assert n_checked > 1500


# ---- 3. the edges ---------------------------------------------------------------------------------------------------------------
def test_edges(layers_host):
    R = 0.0585
    axis = [0., 0., 0., 0.]
    one = lambda four, odd, u, fr, Z, R=R: tuple(v[0] for v in host_layers_at(layers_host, [four], [odd], [u], fr, R, Z))
    # an untilted stack in line, a photon on the axis: sd = 1, L = T, zn = s = u3*T, all exact with T = 2^-6
    st = Stack(layers_host, np.array([0.25, 0.25, 0.5]) * 2. ** -6, [[100.], [200.], [300.]], [[10.], [20.], [30.]])
    assert st.T == 2. ** -6 and list(st.Z) == [0., 2. ** -8, 2. ** -7, 2. ** -6]
    fr = host_layers_frame(layers_host, (0.5, 0., 0., 0., 0.5, 0., 0., R), st.T, st.qmax)
    below = np.nextafter(1., 0.)
    #           u3            layer  za                         zb
    for u3, j, za, zb in ((0., 0, 0., 2. ** -8), (0.25 * below, 0, 2. ** -8 * below, 2. ** -8 - 2. ** -8 * below), (0.25, 1, 0., 2. ** -8),
                          (0.5 * below, 1, 2. ** -7 * below - 2. ** -8, 2. ** -7 - 2. ** -7 * below), (0.5, 2, 0., 2. ** -7),
                          (below, 2, 2. ** -6 * below - 2. ** -7, 2. ** -6 - 2. ** -6 * below), (1., 2, 2. ** -7, 0.)):
        o, w = one(axis, 0, [0.5, 0.5, u3], fr, st.Z)
        assert w == INJECT and (o[L_J], o[L_A], o[L_B]) == (j, za, zb) and o[L_SD] == 1. and o[L_S] == u3 * st.T, (u3, o[L_J], o[L_A], o[L_B])
        assert not np.signbit(o[L_A]) and not np.signbit(o[L_B])
    # the clamp of b: u3 = 1, which only pc_emit_layers_at can be given, carries zn past T where L*sd rounds above T; the interaction
    # stays in the last layer with b = +0 (the slab's case: T just below a power of two)
    st97 = Stack(layers_host, [0.5, 0.25, 0.22], np.zeros((3, 1)), np.zeros((3, 1)))
    assert st97.T == 0.97
    fr97 = host_layers_frame(layers_host, (0.5, 0., 0., 0., 3., 0., 0., R), st97.T, 1.)
    rng = np.random.default_rng(5)
    four = np.zeros((4000, 4))
    four[:, 2] = rng.uniform(-0.3, 0.3, 4000)
    ones = np.tile([0.5, 0.5, 1.], (4000, 1))
    got, what = host_layers_at(layers_host, four, np.zeros(4000, dtype=np.int32), ones, fr97, R, st97.Z)
    want, what_w, mid = np_layers(four[:, 0], four[:, 1], four[:, 2], four[:, 3], np.zeros(4000), ones[:, 0], ones[:, 1], ones[:, 2], fr97, R, st97.Z)
    neg = mid["zb_raw"] < 0.
    print("u3 = 1: Z_n - zn negative in", int(neg.sum()), "of 4000")
    assert neg.sum() > 10 and np.all(what == INJECT) and same_bits(got, want)
    assert np.all(got[:, L_J] == 2.) and not got[neg, L_B].any() and not np.signbit(got[neg, L_B]).any() and np.all(mid["zn"][neg] > 0.97)
    # cn = 0 exactly: the slab's case (an untilted stack, B at 90 degrees, the interaction at the height of B's centre, which is also
    # the boundary of the two layers)
    st2 = Stack(layers_host, [2. ** -7, 2. ** -7], np.zeros((2, 1)), np.zeros((2, 1)))
    fr0 = host_layers_frame(layers_host, (0.5, 0., -2. ** -7, math.pi / 2., 0.5, 0., 0., R), st2.T, 1.)
    o, w = one(axis, 0, [0.5, 0.5, 0.5], fr0, st2.Z)
    _, w_np, mid = np_layers(*[np.array([0.])] * 4, [0], np.array([0.5]), np.array([0.5]), np.array([0.5]), fr0, R, st2.Z)
    assert mid["cn"][0] == 0. and mid["f2"][0] > 0. and w == MISS_DETECTOR and w_np[0] == MISS_DETECTOR
    for u3, j in ((0.25, 0), (0.75, 1)):
        o, w = one(axis, 0, [0.5, 0.5, u3], fr0, st2.Z)
        assert w == INJECT and o[L_J] == j and o[L_CN] != 0.
    # the guard: gl*qmax >= 1 is missed the sample while gl < 1.  dx walks from normal to grazing incidence on a thick stack; every
    # qmax gets its own edge, and qmax = 0 lets everything through
    thick = Stack(layers_host, [0.5, 0.5], np.zeros((2, 1)), np.zeros((2, 1)))
    dxs = np.concatenate([np.linspace(0., 0.9999, 300), 1. - np.logspace(-5, -15, 60)])
    four = np.zeros((len(dxs), 4))
    four[:, 2] = dxs
    zeros = np.tile([0.5, 0.5, 0.], (len(dxs), 1))
    odd0 = np.zeros(len(dxs), dtype=np.int32)
    n_between = 0
    for qmax in (1., 1e6, 3.7, 0.):
        frq = host_layers_frame(layers_host, (0.5, 0., -0.5, 0., 0.5, 0., 0., 0.3), thick.T, qmax)
        got, what = host_layers_at(layers_host, four, odd0, zeros, frq, 0.3, thick.Z)
        want, what_w, mid = np_layers(four[:, 0], four[:, 1], four[:, 2], four[:, 3], odd0, zeros[:, 0], zeros[:, 1], zeros[:, 2], frq, 0.3, thick.Z)
        assert np.array_equal(what, what_w) and same_bits(got, want)
        with np.errstate(all="ignore"):
            fits = mid["gl"] * qmax < 1.
        assert np.array_equal(what == INJECT, fits) and np.all(what[~fits] == MISS_SAMPLE)
        if qmax == 0.:
            assert np.all(what == INJECT) and mid["gl"].max() > 1e4
        elif qmax == 1e6:                                        # nothing fits, the photons with gl < 1 included
            between = ~fits & (mid["gl"] < 1.)
            n_between = int(between.sum())
            assert n_between > 50 and np.all(what[between] == MISS_SAMPLE)
        else:
            assert fits.sum() > 20 and (~fits).sum() > 50
    # qmax = 0: production is zero everywhere and every weight is +0, whatever the attenuation
    dark = Stack(layers_host, [0.5, 0.5], [[10.], [0.]], [[0.], [20.]], np.zeros((2, 1)))
    assert dark.qmax == 0.
    frq = host_layers_frame(layers_host, (0.5, 0., -0.5, 0., 0.5, 0., 0., 0.3), dark.T, dark.qmax)
    got, what = host_layers_at(layers_host, four[:200], odd0[:200], np.tile([0.5, 0.5, 0.7], (200, 1)), frq, 0.3, dark.Z)
    w = host_layers_weight(layers_host, got, 0.9, 0.8, 0, 0, dark)
    assert np.all(what == INJECT) and not w.any() and not np.signbit(w).any()
    # the emit's two conditions, at their edges, as the slab has them
    st1 = Stack(layers_host, [0.005, 0.005], np.zeros((2, 1)), np.zeros((2, 1)))
    fr = host_layers_frame(layers_host, (0.5, 0., 0., 0., 0.5, 0., 0., R), st1.T, 1.)
    assert one([0., 0., 1., 0.], 0, [0.5, 0.5, 0.5], fr, st1.Z)[1] == MISS_SAMPLE
    fr = host_layers_frame(layers_host, (0.5, 0., np.nextafter(-0.5, -1.), 0., 0.5, 0., 0., R), st1.T, 1.)
    assert fr[3] < 0. and one([0.001, 0., 0.01, 0.], 0, [0.5, 0.5, 0.5], fr, st1.Z)[1] == MISS_SAMPLE
    fr = host_layers_frame(layers_host, (0.5, 0., 0.25, 0., 0.25, 0., 0., R), st1.T, 1.)
    assert one(axis, 0, [0.5, 0.5, 0.], fr, st1.Z)[1] == MISS_DETECTOR


# ---- 4. identities with the slab ------------------------------------------------------------------------------------------------
def test_identities_with_the_slab(layers_host, slab_host, oracle):
    """Whatever the split of T, the geometric part of the state (the injected photon, t, r, gl, s) and the outcome are
    pc_emit_slab_at's for the thickness T bit for bit (production 1, so that the guard is the slab's); and with every mu zero and
    production 1 the weight is the slab's at mu = 0, bit for bit.  The splits are dyadic, so that their left-to-right sum is T exactly."""
    rng = np.random.default_rng(99)
    a, slots = _entries(1500, rng)
    u = _uniforms3(oracle, SEED, slots)
    odd = (slots & np.uint64(1)).astype(np.int32)
    n_inj = 0
    for alpha, beta, T in ((0., 0., 0.0078125), (math.pi / 2., math.pi / 4., 0.001953125), (math.pi / 2., -math.pi / 4., 0.25), (math.pi, 0., 1.)):
        spec = (0.5, beta, 0.001, alpha, 0.5, 0.002, -0.001, 0.0585)
        fr_slab = host_slab_frame(slab_host, spec, T)
        want, what_w = host_slab_at(slab_host, a, odd, u, fr_slab, spec[7])
        ok = what_w == INJECT
        n_inj += int(ok.sum())
        wa, wb = rng.random(int(ok.sum())), rng.random(int(ok.sum()))
        w_slab = host_weight(slab_host, wa, want[ok, GL], 0., want[ok, S], 0., want[ok, 13], wb)
        for parts in ([1.], [0.5, 0.5], [0.25] * 4, [0.125, 0.5, 0.25, 0.0625, 0.0625], [1. / 16.] * 16):
            st = Stack(layers_host, np.array(parts) * T, np.zeros((len(parts), 1)), np.zeros((len(parts), 1)))
            assert st.T == T and st.qmax == 1.
            fr = host_layers_frame(layers_host, spec, st.T, st.qmax)
            assert same_bits(fr[:20], fr_slab) and fr[20] == 1.
            got, what = host_layers_at(layers_host, a, odd, u, fr, spec[7], st.Z)
            assert np.array_equal(what, what_w), parts
            assert same_bits(got[:, :13], want[:, :13]), parts
            assert same_bits(host_layers_weight(layers_host, got[ok], wa, wb, 0, 0, st), w_slab), parts
            j = got[ok, L_J].astype(np.int64)
            assert j.min() >= 0 and j.max() < len(parts)
        # the library's frame is the host compile's
        import polycap_amd
        lib = polycap_amd.emit_layers_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7], layers=st.as_layers())
        assert same_bits(lib["frame"], fr) and lib["thickness"] == T and lib["qmax"] == 1. and same_bits(lib["bounds"], st.Z)
    assert n_inj > 1500


# ---- 5. the spec check and the symbols ------------------------------------------------------------------------------------------
def _layers(n=3, n_in=2, n_out=1, **kw):
    lay = [dict(thickness=0.001 * (j + 1), mu_in=[100. + j] * n_in, mu_out=[50. + j] * n_out, production=[1. + j] * n_out) for j in range(n)]
    for k, (j, v) in kw.items():
        lay[j][k] = v
    return lay


def test_validate_names_the_table_the_layer_and_the_index(layers_host):
    import polycap_amd
    from polycap_amd import _cabi
    L = polycap_amd.lib()
    valid = lambda layers, spec=GOOD, **kw: polycap_amd.emit_layers_valid(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7], layers=layers, **kw)
    said = lambda: L.pc_hip_last_error().decode()
    assert valid(_layers()) and valid(_layers(1)) and valid(_layers(16, thickness=(0, 5e-324))) and valid(_layers(), energy_map=[0, 1, 1])
    assert valid([dict(thickness=1., mu_in=[0.], mu_out=[1.7976931348623157e308])])                     # production defaults to ones
    assert valid([dict(thickness=0.5, mu_in=[0.], mu_out=[0.], production=[0.]), dict(thickness=0.5, mu_in=[0.], mu_out=[0.])])
    i32 = C.POINTER(C.c_int32)

    def header_says(layers):
        st, keep = polycap_amd.hip._layers_spec(*GOOD[:5], GOOD[5:7], GOOD[7], 0, None, layers)
        layer, at = C.c_int32(0), C.c_int32(0)
        bad = layers_host.layers_bad(st.n_layers, st.thickness, st.n_mu_in, st.mu_in, st.n_mu_out, st.mu_out, st.production, C.byref(layer), C.byref(at))
        return bad, layer.value, at.value

    assert header_says(_layers()) == (0, -1, -1)
    # n_layers outside 1 .. 16
    for n in (0, 17, 40):
        assert not valid(_layers(n)) and said().startswith("pc_hip_layers_validate: n_layers is %d" % n), said()
        assert header_says(_layers(n)) == (BAD_N, -1, -1)
    # a thickness not finite or not in (0, 1]
    for bad in (0., -0., -0.01, np.nextafter(1., 2.), 2., math.nan, math.inf, -math.inf):
        assert not valid(_layers(thickness=(1, bad))) and said().startswith("pc_hip_layers_validate: thickness[1] "), (bad, said())
        assert header_says(_layers(thickness=(1, bad))) == (BAD_THICKNESS, 1, -1)
    # a total above 1 cm
    over = [dict(thickness=t, mu_in=[1.], mu_out=[1.]) for t in (0.5, 0.5, 2. ** -52)]
    assert not valid(over) and "total thickness" in said() and header_says(over) == (BAD_TOTAL, -1, -1)
    assert valid(over[:2]) and valid([dict(thickness=t, mu_in=[1.], mu_out=[1.]) for t in (0.5, 0.5, 2. ** -60)])      # the sum rounds to 1
    # an entry of a table not finite or negative: the table, the layer, the index
    for bad in (-1e-300, -1., math.nan, math.inf, -math.inf):
        assert not valid(_layers(mu_in=(2, [3., bad]))) and said().startswith("pc_hip_layers_validate: mu_in[2][1] "), (bad, said())
        assert not valid(_layers(mu_out=(0, [bad]))) and said().startswith("pc_hip_layers_validate: mu_out[0][0] "), (bad, said())
        assert not valid(_layers(n_out=3, production=(1, [1., 2., bad]))) and said().startswith("pc_hip_layers_validate: production[1][2] "), (bad, said())
        assert header_says(_layers(mu_in=(2, [3., bad]))) == (BAD_MU_IN, 2, 1) and header_says(_layers(mu_out=(0, [bad]))) == (BAD_MU_OUT, 0, 0)
        assert header_says(_layers(n_out=3, production=(1, [1., 2., bad]))) == (BAD_PRODUCTION, 1, 2)
    # mu_in is checked before mu_out, mu_out before production, a thickness before any of them
    lay = _layers(mu_in=(2, [3., -1.]), mu_out=(0, [-1.]), production=(0, [-1.]))
    assert not valid(lay) and "mu_in[2][1]" in said()
    lay[2]["mu_in"] = [3., 1.]
    assert not valid(lay) and "mu_out[0][0]" in said()
    lay[0]["mu_out"] = [1.]
    assert not valid(lay) and "production[0][0]" in said()
    lay[1]["thickness"] = 0.
    assert not valid(lay) and "thickness[1]" in said()
    # empty rows
    assert not valid([dict(thickness=0.1, mu_in=[], mu_out=[1.])]) and "n_mu_in" in said()
    assert not valid([dict(thickness=0.1, mu_in=[1.], mu_out=[])]) and "n_mu_out" in said()
    # the emit's fields are checked as the emit checks them, and first
    for k, name in enumerate(FIELDS):
        spec = list(GOOD)
        spec[k] = math.nan
        assert not valid(_layers(thickness=(0, 0.)), spec) and said().startswith("pc_hip_layers_validate: " + name + " "), name
        with pytest.raises(polycap_amd.HipError) as e:
            polycap_amd.emit_layers_frame(spec[0], spec[1], spec[2], spec[3], spec[4], spec[5:7], spec[7], layers=_layers())
        assert e.value.status == -2 and name in str(e.value)
    assert not valid(_layers(), energy_map=[0, -1]) and "map[1]" in said()
    with pytest.raises(polycap_amd.HipError) as e:
        polycap_amd.emit_layers_frame(*GOOD[:5], GOOD[5:7], GOOD[7], layers=_layers(thickness=(2, 1.5)))
    assert e.value.status == -2 and "thickness[2]" in str(e.value)
    # NULL pointers
    assert L.pc_hip_layers_validate(None) == -2 and "spec" in said()
    th = np.array([0.1])
    for fields, name in (((1, None, 1, None, 1, None, None), "thickness"), ((1, _dp(th), 1, None, 1, None, None), "n_mu_in"),
                         ((1, _dp(th), 1, _dp(th), 1, None, None), "n_mu_out"), ((1, _dp(th), 1, _dp(th), 1, _dp(th), None), "production")):
        s = _cabi.LayersS(_cabi.EmitS(*GOOD, 0, 0, None), *fields)
        assert L.pc_hip_layers_validate(C.byref(s)) == -2 and name in said(), (name, said())
    assert C.sizeof(_cabi.LayersS) == 144
    # the Python layer's own refusals
    for kw in (dict(thickness=0.01), dict(mu_in=[1.]), dict(mu_out=[1.]), dict(thickness=0.01, mu_in=[1.], mu_out=[1.])):
        with pytest.raises(ValueError):
            polycap_amd.hip._layers_given("emit", _layers(), kw.get("thickness"), kw.get("mu_in"), kw.get("mu_out"))
    assert polycap_amd.hip._layers_given("emit", None, 0.01, [1.], [1.]) is False and polycap_amd.hip._layers_given("emit", _layers(), None, None, None) is True
    for lay in ([dict(thickness=0.1, mu_in=[1.])], [dict(thickness=0.1, mu_in=[1.], mu_out=[1.], mu=[1.])], _layers(mu_in=(1, [1.])),
                _layers(mu_out=(2, [1., 2.])), _layers(production=(0, [1., 2.]))):
        with pytest.raises(ValueError):
            valid(lay)
    with pytest.raises(ValueError):
        polycap_amd.emit_layers_valid(*GOOD[:5], GOOD[5:7], GOOD[7])
    with pytest.raises(ValueError):
        polycap_amd.emit_layers_frame(*GOOD[:5], GOOD[5:7], GOOD[7])
    # emit() and emit_depth_scan() take layers=
    import inspect
    assert "layers" in inspect.signature(polycap_amd.TraceContext.emit).parameters
    assert "layers" in inspect.signature(polycap_amd.emit_depth_scan).parameters


def test_layers_symbols_are_exported_and_declared():
    import polycap_amd
    polycap_amd.lib()
    so = os.path.join(ROOT, "polycap_amd", "lib", "libpolycap.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert [n for n in names if n.startswith("pc_hip_") and "layers" in n] == sorted(NEW_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "polycap-hip.h")).read()
    assert re.search(r"#define\s+PC_HIP_MAX_LAYERS\s+16\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"POLYCAP_EXTERN\s+[^;(]*?\b(\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    assert not [n for n in names if n.startswith("_Z") or "pc_emit" in n or "pc_rule" in n]
    assert [n for n in names if n.startswith("pc_hip_") and n not in declared] == []
